// lincov.hip -- linear covariance analysis of the tracking law u = U_k - K_k (x(t_k) - X_k) + b + w_k around every trajectory of a
// batch: the joint covariance S_k of the state deviation and the constant control offset is carried through the closed loop of
// the discrete Jacobians [Ad_k | Bd_k] of the handle's last gusto_tvlqr, and turned into margins -- the signed distance of every
// (robot component, keep-out component) pair and the room of every control entry under its bounds, each divided by its standard
// deviation.  No counterpart in the reference; include/gusto_hip.h states the definitions (recursion, margins, summaries,
// status).  The analytic counterpart of simulate.hip: one pass per problem instead of S roll-outs.
// One launch, one wave per problem, the knots in sequence (as tvlqr_riccati).  S_k, G_k = [Ad - Bd K | Bd], T = G_k S_k, K_k
// and V = [-K I] S_k live in LDS (8.4 KB for n = 13); the 64 lanes split the entries of every product (entry e = lane + 64 r),
// each entry one dot product in a fixed order.  [Ad | Bd] arrives in the buffer of G: the product Bd K reads its Bd columns
// and K, and overwrites the Ad columns only.  Sxx of the next knot is computed on the upper triangle and mirrored, so it is
// symmetric to the bit.  [Ad | Bd] and K of the next knot are loaded into registers while the current knot computes.
// Margins: lanes take the (component, obstacle) pairs, pair p = lane + 64 r (ordinal component n_obs + obstacle, as
// verify.hip); the obstacle tables go through problem_env, shared or per problem.  The minimum of a knot is a wave_reduce of
// the lanes' minima, its ordinal a second one over the lanes that hold that minimum: the lowest ordinal of equal minima.
// Over the knots a strict < keeps the lowest knot.  The control margins (m <= 6) are walked by every lane on the same LDS values.
// No atomics, nothing crosses a problem: a problem's outputs are the same bit for bit whatever batch it sits in.
// gusto_lincov_disturbed is the PLANT = true instantiation of the same kernel (as DIST is in simulate.hip): the deviation is
// augmented by the constant plant deviation, z = [dx; b; theta~], so S, G = [Ad - Bd K | Bd | Cd] and T gain GUSTO_NPLANT columns
// (11.8 KB of LDS for n = 13) and every dot product the theta terms BEHIND the terms it has; PLANT = false is what it was.  Cd
// comes from a launch ahead of it on the same stream:
//   lincov_plant_sens  grid (problem, tile of IPB intervals), 256 lanes.  Work item (k, c) = lane: interval k and the c-th plant
//     scalar the model reads (2 or 4 of them: IPB = 128 or 64).  A lane carries the nominal state and ONE tangent column
//     d = dx/dtheta_j through every substep: tvlqr_linearise's step (rk4_tangent.inc) with the source dfdth_j(stage point, u).  The
//     tile is staged in LDS ([interval][row][6], the layout of Cd, zeros in the columns the model does not read) and copied out
//     by the whole workgroup, consecutive lanes to consecutive addresses.
// gusto_lincov_dense is gusto_lincov_disturbed with DENSE = true -- the knot pass also writes the x-rows of S_k of every knot and
// the [b theta] block, which stays -- and two launches behind it on the same stream:
//   lincov_dense         grid (problem, tile of 4 intervals), one wave per interval: the margins at the dense samples inside it
//     (the comment at the kernel has the mapping)
//   lincov_dense_reduce  one wave per problem: the minimum over the intervals in their order, zeros behind nfull_b
#include <hip/hip_runtime.h>

#include "post.hpp"
#include "rollout.hpp"

using namespace gusto;

namespace {

constexpr int NO_ORD = 1 << 30;    // (ordinals stay below 2 * 64)

struct LcArgs {
    const double *X, *U, *K, *AB;  // [B][N][n], [B][N][m], [B][N-1][m][n], [B][N-1][n][n+m]
    const double* S0;              // [B][n+m][n+m], or null: diag(dx0^2 / 3, du0^2 / 3)
    const int* active;             // gusto_set_active: null = every problem, else the mask [B]
    const int *tv_status, *tv_fail;   // K = NULL: status and fail_knot of the gains' gusto_tvlqr; a caller's K: null
    double dx0[GUSTO_MAXN], du0[GUSTO_MAXM], du_white[GUSTO_MAXM], u_lo[GUSTO_MAXM], u_hi[GUSTO_MAXM];
    int store_S;
    int *status, *fail_knot, *obs_knot, *obs_pair, *ctl_knot, *ctl_entry;   // [B]
    double *min_z_obs, *p_bound, *min_z_ctl;                                // [B]
    double *sigma_x, *sigma_u, *z_obs, *Sxx;   // [B][N][n], [B][N-1][m], [B][N], [B][N][n][n] (store_S)
};

// gusto_lincov_disturbed: LcArgs and the plant dispersion
struct LcArgsP : LcArgs {
    const double* Cd;              // [B][N-1][n][GUSTO_NPLANT]: lincov_plant_sens
    const double* Sth;             // [B][GUSTO_NPLANT][GUSTO_NPLANT], or null: diag((nominal plant_rel)^2 / 3)
    double plant_rel[GUSTO_NPLANT], dw[GUSTO_MAXM];
    double* Sxt;                   // [B][N][n][GUSTO_NPLANT] (store_S)
};

// gusto_lincov_dense: what its knot pass leaves for the dense pass
struct LcArgsD : LcArgsP {
    double* Srow;                  // [B][N][n][NZ]: the x-rows of S_k, NZ = n + m + GUSTO_NPLANT
    double* Sbt;                   // [B][m + GUSTO_NPLANT][m + GUSTO_NPLANT]: the [b theta] block, which stays
};

struct SensArgs {
    const double *X, *U;           // [B][N][n], [B][N][m]
    const int* active;
    double dt_min;                 // the roll-out options of the handle's last gusto_tvlqr
    int nstep;
    double* Cd;
};

// the plant scalars a model reads: their number and the GUSTO_NPLANT entry of the c-th of them
template <int MODEL> struct PlantCols {
    static constexpr int count() { int c = 0; for (int j = 0; j < GUSTO_NPLANT; j++) c += plant_entry_read(MODEL, j) ? 1 : 0; return c; }
    static constexpr int NR = count();
    static constexpr int IPB = 256 / NR;   // whole intervals per workgroup: its slice of Cd is one contiguous range
    static constexpr int entry(int c) {
        for (int j = 0; j < GUSTO_NPLANT; j++)
            if (plant_entry_read(MODEL, j) && c-- == 0) return j;
        return 0;
    }
};

// the standard deviation of a variance: what rounding leaves below zero counts as zero (a NaN stays one)
GD double sigma_of(double var) { return sqrt(var < 0.0 ? 0.0 : var); }

// a margin in standard deviations; without any deviation the sign of the margin decides
GD double margin_z(double d, double sigma) {
    if (sigma == 0.0) return d >= 0.0 ? INFINITY : -INFINITY;
    return d / sigma;
}

// z_obs of one knot and the ordinal of the pair it occurs at (NO_ORD: +inf), the same in every lane.  xk: the knot's state;
// sS: S_k in rows of nz doubles, whose leading WS x WS block is the covariance of the workspace location (the component offsets are translations)
template <int MODEL, int nz> GD void obstacle_margin(const KParams& P, const Env& E, const double* xk, const double* sS, int lane, double* zk, int* pk) {
    using T = MT<MODEL>;
    constexpr int WS = T::WS;   // (nz: the row length of sS)
    double zb = INFINITY;
    int ob = NO_ORD;
    if constexpr (T::HAS_OBS) {
        const int npair = P.mp.n_robot_comp * E.n_obs;
        double x[WS];
#pragma unroll
        for (int j = 0; j < WS; j++) x[j] = xk[j];
        for (int p0 = 0; p0 < npair; p0 += 64) {   // (uniform bound)
            const int p = p0 + lane;
            if (p < npair) {
                const int c = p / E.n_obs, i = p % E.n_obs;
                double nh[WS];
                const double d = signed_distance<WS>(P, E, c, x, i, nh);
                double q = 0.0;
#pragma unroll
                for (int a = 0; a < WS; a++) {
                    double s = 0.0;
#pragma unroll
                    for (int j = 0; j < WS; j++) s += sS[a * nz + j] * nh[j];
                    q += nh[a] * s;
                }
                const double z = margin_z(d, sigma_of(q));
                if (z < zb) { zb = z; ob = p; }   // (ascending ordinals: the first of equal minima stays; a NaN never wins)
            }
        }
    }
    const double zmin = wave_reduce(zb, OpMin());
    *pk = (int)wave_reduce((ob != NO_ORD && zb == zmin) ? (double)ob : (double)NO_ORD, OpMin());
    *zk = zmin;
}

template <int MODEL> __global__ void __launch_bounds__(256) lincov_plant_sens(const KParams P, const SensArgs V) {
    using D = Dyn<MODEL>;
    using PC = PlantCols<MODEL>;
    constexpr int n = MT<MODEL>::n, m = MT<MODEL>::m, NT = GUSTO_NPLANT, NR = PC::NR, IPB = PC::IPB;
    static_assert(IPB * NR == 256, "every lane has a work item");
    __shared__ double stage[IPB * n * NT];
    const int b = blockIdx.x, k0 = blockIdx.y * IPB, t = threadIdx.x, N = P.N;
    if (V.active && !V.active[b]) return;   // (the whole workgroup)
    const double dt = P.tf[b] / (N - 1);
    const int nstep = rollout_nstep(dt, V.nstep, V.dt_min);
    const double h = dt / nstep;
    const int kl = t / NR, c = t % NR;
    const bool valid = k0 + kl < N - 1;
    const int k = valid ? k0 + kl : 0;   // (idle lanes roll interval 0 out and store nothing)
    int j = 0;
#pragma unroll
    for (int q = 0; q < NR; q++)
        if (c == q) j = PC::entry(q);
    const double* Xk = V.X + ((size_t)b * N + k) * n;
    const double* Uk = V.U + ((size_t)b * N + k) * m;
    double x[n], u[m], d[n];
#pragma unroll
    for (int i = 0; i < n; i++) { x[i] = Xk[i]; d[i] = 0.0; }
#pragma unroll
    for (int i = 0; i < m; i++) u[i] = Uk[i];
    for (int s = 0; s < nstep; s++) {
#define RK4_TANGENT_SOURCE(xp, g) (D::dfdth(P.mp, xp, u, j, g), g)
#include "rk4_tangent.inc"
    }
    // the columns the model does not read are zeros; a lane writes column j of its interval (disjoint addresses)
    for (int e = t; e < IPB * n * NT; e += 256)
        if (!plant_entry_read(MODEL, e % NT)) stage[e] = 0.0;
    if (valid)
#pragma unroll
        for (int i = 0; i < n; i++) stage[(kl * n + i) * NT + j] = d[i];
    __syncthreads();
    const int cnt = min(IPB, N - 1 - k0) * n * NT;   // (the lanes past it hold nothing: never read)
    double* out = V.Cd + ((size_t)b * (N - 1) + k0) * n * NT;
    for (int e = t; e < cnt; e += 256) out[e] = stage[e];
}

// NZ: the size of the augmented deviation, the row length of S, G and T.  PLANT = false: NZ = nz, NGZ = NG, NT = 0 -- the loops
// over the theta entries are empty.  DENSE (gusto_lincov_dense, with PLANT): the x-rows of S_k of every knot and the [b theta]
// block go out for lincov_dense; DENSE = false is what it was
template <int MODEL, bool PLANT, bool DENSE = false>
__global__ void __launch_bounds__(64) lincov_kernel(const KParams P, const std::conditional_t<DENSE, LcArgsD, std::conditional_t<PLANT, LcArgsP, LcArgs>> V) {
    static_assert(PLANT || !DENSE, "the dense pass reads the augmented S");
    using T = MT<MODEL>;
    constexpr int n = T::n, m = T::m, nz = n + m, NT = PLANT ? GUSTO_NPLANT : 0, NZ = nz + NT;
    constexpr int NG = n * nz, RG = (NG + 63) / 64;                 // entries of [Ad | Bd], per lane
    constexpr int NGZ = n * NZ, RGZ = (NGZ + 63) / 64;              // entries of G and of T
    constexpr int NC = n * NT, RC = (NC + 63) / 64;                 // entries of Cd
    constexpr int NK = m * n, RK = (NK + 63) / 64;
    constexpr int NV = m * nz, RV = (NV + 63) / 64;                 // V = [-K I] S
    constexpr int NP = n * (n + 1) / 2, RP = (NP + 63) / 64;        // upper triangle of Sxx
    constexpr int NS = NZ * NZ, RS = (NS + 63) / 64, NPF = n * n, RPF = (NPF + 63) / 64;
    __shared__ double sS[NS], sG[NGZ], sT[NGZ], sK[NK], sV[NV], sSu[m];
    const int b = blockIdx.x, lane = threadIdx.x, N = P.N;
    if (V.active && !V.active[b]) return;   // (an inactive problem's outputs are left as they are)
    const double* X = V.X + (size_t)b * N * n;
    const double* U = V.U + (size_t)b * N * m;
    const double* AB = V.AB + (size_t)b * (N - 1) * NG;
    const double* K = V.K + (size_t)b * (N - 1) * NK;
    double* sx = V.sigma_x + (size_t)b * N * n;
    double* su = V.sigma_u + (size_t)b * (N - 1) * m;
    double* zo = V.z_obs + (size_t)b * N;
    double* Sall = V.store_S ? V.Sxx + (size_t)b * N * NPF : nullptr;
    [[maybe_unused]] const double* Cd = nullptr;
    [[maybe_unused]] double* Tall = nullptr;   // Sxt of every knot
    if constexpr (PLANT) {
        Cd = V.Cd + (size_t)b * (N - 1) * NC;
        if (V.store_S) Tall = V.Sxt + (size_t)b * N * NC;
    }
    [[maybe_unused]] double* Rall = nullptr;   // the x-rows of S of every knot
    if constexpr (DENSE) Rall = V.Srow + (size_t)b * N * NGZ;
    const Env E = problem_env(P, b);

    // gains of a failed gusto_tvlqr: its fail_knot, every output zero
    const bool dead = V.tv_status && !V.tv_status[b];   // (wave-uniform)
    int fail = dead ? V.tv_fail[b] : 0;
    int zero_from = dead ? 1 : N + 1;                   // the per-knot rows from this knot on are zeros

    // the upper-triangle entries this lane owns, found once
    int pa[RP], pb[RP];
#pragma unroll
    for (int r = 0; r < RP; r++) {
        int rem = lane + 64 * r, a = 0;
        if (rem >= NP) rem = 0;
        while (rem >= n - a) { rem -= n - a; a++; }
        pa[r] = a; pb[r] = a + rem;
    }
    double w2[m];
#pragma unroll
    for (int q = 0; q < m; q++) {
        w2[q] = V.du_white[q] * V.du_white[q];
        if constexpr (PLANT) w2[q] += V.dw[q] * V.dw[q] / 3.0;   // the variance of the uniform draw with the half-width dw
    }

    // S_1 = S0; PLANT: blockdiag(S0, Stheta), Stheta on the entries the model reads
#pragma unroll
    for (int r = 0; r < RS; r++) {
        const int e = lane + 64 * r;
        if (e < NS) {
            const int i = e / NZ, c = e % NZ;
            double v = 0.0;
            if constexpr (!PLANT) {
                if (V.S0) v = V.S0[(size_t)b * NS + e];
                else if (i == c) { const double w = i < n ? V.dx0[i] : V.du0[i - n]; v = w * w / 3.0; }
            } else {
                if (i < nz && c < nz) {
                    if (V.S0) v = V.S0[(size_t)b * nz * nz + i * nz + c];
                    else if (i == c) { const double w = i < n ? V.dx0[i] : V.du0[i - n]; v = w * w / 3.0; }
                }
                const PlantNominal nominal(P.mp);
#pragma unroll
                for (int ji = 0; ji < NT; ji++)
#pragma unroll
                    for (int jc = 0; jc < NT; jc++)
                        if (plant_entry_read(MODEL, ji) && plant_entry_read(MODEL, jc) && i == nz + ji && c == nz + jc) {
                            if (V.Sth) v = V.Sth[(size_t)b * NT * NT + ji * NT + jc];
                            else if (ji == jc) { const double t = nominal.v[ji] * V.plant_rel[ji]; v = (t * t) / 3.0; }
                        }
            }
            sS[e] = v;
            if constexpr (DENSE)
                if (i >= n && c >= n) V.Sbt[((size_t)b * (NZ - n) + (i - n)) * (NZ - n) + (c - n)] = v;
        }
    }
    double g[RG], kr[RK];
    [[maybe_unused]] double cd[RC > 0 ? RC : 1];
#pragma unroll
    for (int r = 0; r < RG; r++) { const int e = lane + 64 * r; g[r] = (!dead && e < NG) ? AB[e] : 0.0; }
    if constexpr (PLANT)
#pragma unroll
        for (int r = 0; r < RC; r++) { const int e = lane + 64 * r; cd[r] = (!dead && e < NC) ? Cd[e] : 0.0; }
#pragma unroll
    for (int r = 0; r < RK; r++) { const int e = lane + 64 * r; kr[r] = (!dead && e < NK) ? K[e] : 0.0; }
    __syncthreads();

    double zo_min = INFINITY, zc_min = INFINITY, psum = 0.0;
    int zo_knot = 0, zo_pair = -1, zc_knot = 0, zc_entry = -1;

    // the rows of knot k (lincov_knot_rows.inc has the list) from S_k
    auto emit = [&](int k, double zk, bool with_u) {
#define KNOT_ROWS_LIVE true
#include "lincov_knot_rows.inc"
    };
    auto note_obstacles = [&](int k, double zk, int pk) {
        if (zk < zo_min) { zo_min = zk; zo_knot = k; zo_pair = pk; }   // (strict: the lowest knot of equal minima)
        psum += 0.5 * erfc(zk / sqrt(2.0));
    };

    for (int k = 1; k <= N - 1 && !dead; k++) {   // knot k (1-based): interval k - 1 of the arrays
#pragma unroll
        for (int r = 0; r < RG; r++) { const int e = lane + 64 * r; if (e < NG) sG[PLANT ? (e / nz) * NZ + e % nz : e] = g[r]; }
        if constexpr (PLANT)
#pragma unroll
            for (int r = 0; r < RC; r++) { const int e = lane + 64 * r; if (e < NC) sG[(e / NT) * NZ + nz + e % NT] = cd[r]; }
#pragma unroll
        for (int r = 0; r < RK; r++) { const int e = lane + 64 * r; if (e < NK) sK[e] = kr[r]; }
        __syncthreads();
        // [Ad | Bd] and K of the next knot, in flight while this one computes
        double gp[RG], kp[RK];
        [[maybe_unused]] double cdp[RC > 0 ? RC : 1];
        if constexpr (PLANT)
#pragma unroll
            for (int r = 0; r < RC; r++) { const int e = lane + 64 * r; cdp[r] = (k < N - 1 && e < NC) ? Cd[(size_t)k * NC + e] : 0.0; }
#pragma unroll
        for (int r = 0; r < RG; r++) { const int e = lane + 64 * r; gp[r] = (k < N - 1 && e < NG) ? AB[(size_t)k * NG + e] : 0.0; }
#pragma unroll
        for (int r = 0; r < RK; r++) { const int e = lane + 64 * r; kp[r] = (k < N - 1 && e < NK) ? K[(size_t)k * NK + e] : 0.0; }
        // G = [Ad - Bd K | Bd]: reads the Bd columns and K, writes the Ad columns
#pragma unroll
        for (int r = 0; r < RG; r++) {
            const int e = lane + 64 * r;
            if (e < NG && e % nz < n) {
                const int i = e / nz, c = e % nz;
                double s = g[r];
#pragma unroll
                for (int q = 0; q < m; q++) s -= sG[i * NZ + n + q] * sK[q * n + c];
                sG[PLANT ? i * NZ + c : e] = s;
            }
        }
        // V = [-K I] S
#pragma unroll
        for (int r = 0; r < RV; r++) {
            const int e = lane + 64 * r;
            if (e < NV) {
                const int i = e / nz, c = e % nz;
                double s = sS[(n + i) * NZ + c];
#pragma unroll
                for (int j = 0; j < n; j++) s -= sK[i * n + j] * sS[j * NZ + c];
                sV[e] = s;
            }
        }
        __syncthreads();
        bool bad = false;
        // T = G S; its columns from n on are Sxb (PLANT: and Sx-theta) of the next knot
#pragma unroll
        for (int r = 0; r < RGZ; r++) {
            const int e = lane + 64 * r;
            if (e < NGZ) {
                const int i = e / NZ, c = e % NZ;
                double s = 0.0;
#pragma unroll
                for (int p = 0; p < NZ; p++) s += sG[i * NZ + p] * sS[p * NZ + c];
                sT[e] = s;
                if (c >= n && !(fabs(s) < INFINITY)) bad = true;
            }
        }
        // sigma_u = sqrt(diag(V [-K I]') + du_white^2)
        if (lane < m) {
            double s = sV[lane * nz + n + lane];
#pragma unroll
            for (int j = 0; j < n; j++) s -= sV[lane * nz + j] * sK[lane * n + j];
            const double w = V.du_white[lane];
            s += w * w;
            if constexpr (PLANT) { const double hw = V.dw[lane]; s += hw * hw / 3.0; }   // (after gusto_lincov's terms: a zero dw changes nothing)
            const double sd = sigma_of(s);
            sSu[lane] = sd;
            if (!(fabs(sd) < INFINITY)) bad = true;
        }
        __syncthreads();
        // Sxx of the next knot = T G' + Bd diag(du_white^2) Bd', upper triangle
        double pn[RP];
#pragma unroll
        for (int r = 0; r < RP; r++) {
            pn[r] = 0.0;
            if (lane + 64 * r < NP) {
                const int a = pa[r], c = pb[r];
                double s = 0.0;
#pragma unroll
                for (int p = 0; p < nz; p++) s += sT[a * NZ + p] * sG[c * NZ + p];
#pragma unroll
                for (int q = 0; q < m; q++) s += sG[a * NZ + n + q] * w2[q] * sG[c * NZ + n + q];
#pragma unroll
                for (int p = nz; p < NZ; p++) s += sT[a * NZ + p] * sG[c * NZ + p];   // (PLANT: the theta terms, last)
                pn[r] = s;
                if (!(fabs(s) < INFINITY)) bad = true;
            }
        }
        if (wave_reduce(bad ? 1.0 : 0.0, OpMax()) != 0.0) { fail = k; zero_from = k; break; }   // (wave-uniform)
        // the margins of knot k on S_k
        double zk;
        int pk;
        obstacle_margin<MODEL, NZ>(P, E, X + (size_t)(k - 1) * n, sS, lane, &zk, &pk);
        note_obstacles(k, zk, pk);
        {
            double zc = INFINITY;
            int ec = -1;
#pragma unroll
            for (int i = 0; i < m; i++) {
                const double u = U[(size_t)(k - 1) * m + i];
                const double z = margin_z(fmin(V.u_hi[i] - u, u - V.u_lo[i]), sSu[i]);
                if (z < zc) { zc = z; ec = i; }
            }
            if (zc < zc_min) { zc_min = zc; zc_knot = k; zc_entry = ec; }
        }
        emit(k, zk, true);
        __syncthreads();   // (the readers of S_k are done)
        // S_{k+1}: Sxx mirrored, Sxb and its transpose; Sbb stays
#pragma unroll
        for (int r = 0; r < RP; r++) {
            if (lane + 64 * r < NP) { sS[pa[r] * NZ + pb[r]] = pn[r]; sS[pb[r] * NZ + pa[r]] = pn[r]; }
        }
#pragma unroll
        for (int r = 0; r < RGZ; r++) {
            const int e = lane + 64 * r;
            if (e < NGZ && e % NZ >= n) { const int i = e / NZ, c = e % NZ; const double v = sT[e]; sS[i * NZ + c] = v; sS[c * NZ + i] = v; }
        }
        if constexpr (PLANT)
#pragma unroll
            for (int r = 0; r < RC; r++) cd[r] = cdp[r];
#pragma unroll
        for (int r = 0; r < RG; r++) g[r] = gp[r];
#pragma unroll
        for (int r = 0; r < RK; r++) kr[r] = kp[r];
        __syncthreads();
    }
    if (!dead && !fail) {   // knot N: no control
        double zk;
        int pk;
        obstacle_margin<MODEL, NZ>(P, E, X + (size_t)(N - 1) * n, sS, lane, &zk, &pk);
        note_obstacles(N, zk, pk);
        emit(N, zk, false);
    }
    for (int k = zero_from; k <= N; k++) {   // zeros from a failed knot on
        const bool with_u = k <= N - 1;
        const double zk = 0.0;
#define KNOT_ROWS_LIVE false
#include "lincov_knot_rows.inc"
    }
    if (lane == 0) {
        V.status[b] = (dead || fail) ? 0 : 1;
        V.fail_knot[b] = fail;
        V.obs_knot[b] = dead ? 0 : zo_knot;
        V.obs_pair[b] = dead ? 0 : (zo_knot ? zo_pair : -1);
        V.ctl_knot[b] = dead ? 0 : zc_knot;
        V.ctl_entry[b] = dead ? 0 : (zc_knot ? zc_entry : -1);
        V.min_z_obs[b] = dead ? 0.0 : zo_min;
        V.p_bound[b] = dead ? 0.0 : fmin(1.0, psum);
        V.min_z_ctl[b] = dead ? 0.0 : zc_min;
    }
}

// gusto_lincov_dense: the margins at the dense samples between the knots, from what the DENSE knot pass left
struct DnArgs {
    const double *X, *U, *K;       // K: the gains the knot pass used
    const double *Srow, *Sbt;      // LcArgsD
    const int* active;
    const int* tv_status;          // as LcArgs: null with a caller's K
    const int* fail_knot;          // of the knot pass
    double dt_min;                 // the roll-out options of the handle's last gusto_tvlqr
    int nstep;
    double du_white[GUSTO_MAXM], dw[GUSTO_MAXM];
    int store_dense, rows;         // rows = nfull_max: the row count of the per-sample arrays
    double* zint;                  // [B][N-1]: the smallest z of every interval (knot N belongs to the last one),
    int *jint, *pint;              // its dense sample and pair ordinal (-1: +inf)
    double* z_dense;               // [B][rows]
    int* pair_dense;               // [B][rows]
    double* Spos;                  // [B][rows][WS][WS]
    int *nfull, *dense_sample, *dense_pair;   // [B]
    double* min_z_dense;                      // [B]
};

// grid (problem, tile of 4 intervals), 256 lanes: one wave per interval.  Lane j < NZ carries the nominal state and column j of
// G_{k,i} = [Phi - Gamma K | Gamma | C] through the RK4 stages (rk4_tangent.inc, as tvlqr_linearise; the theta columns take dfdth as
// their source, as lincov_plant_sens): the closed loop sits in the seed -- x-columns start at e_j with the control direction -K e_j, b-
// columns at 0 with e_c, theta-columns at 0 -- and B du is formed once.  After every substep the first WS entries of the columns
// go to LDS, the wave forms T = Gp S_k and the upper triangle of Spos = T Gp' + Gammap diag(sw2) Gammap' in a fixed order (S_k:
// the interval's x-rows of the knot pass, completed by symmetry and the constant block, in LDS throughout), and all 64 lanes
// take the pairs through obstacle_margin.  At i = 0 and at knot N Spos is the knot pass's Sxx block, by definition.  Every wave
// of a workgroup walks the same number of substeps (Nstep is the problem's), so the barriers are the workgroup's; a wave past
// the last interval rolls interval 0 out and stores nothing.  z and the pair of sample i wait in lane i mod 64 and go out 64
// at a time, consecutive lanes to consecutive addresses.
template <int MODEL> __global__ void __launch_bounds__(256) lincov_dense(const KParams P, const DnArgs V) {
    using T = MT<MODEL>;
    using D = Dyn<MODEL>;
    constexpr int n = T::n, m = T::m, nz = n + m, NT = GUSTO_NPLANT, NZ = nz + NT, NB = m + NT, WS = T::WS, IPB = 4;
    constexpr int NS = NZ * NZ, RS = (NS + 63) / 64, NGP = WS * NZ, RGP = (NGP + 63) / 64, NSP = WS * WS, NGZ = n * NZ;
    static_assert(NZ <= 64 && NSP <= 64, "a lane per column and per entry of Spos");
    __shared__ double sS[IPB][NS], sGp[IPB][NGP], sT[IPB][NGP], sSp[IPB][NSP], sX[IPB][WS];
    const int b = blockIdx.x, wv = threadIdx.x >> 6, lane = threadIdx.x & 63, N = P.N;
    if (V.active && !V.active[b]) return;   // (the whole workgroup)
    const double dt = P.tf[b] / (N - 1);
    const int nstep = rollout_nstep(dt, V.nstep, V.dt_min);
    const double h = dt / nstep;
    const bool valid = (int)blockIdx.y * IPB + wv < N - 1;
    const int k = valid ? blockIdx.y * IPB + wv : 0;          // interval k (0-based): knot k + 1
    const bool has_last = blockIdx.y == gridDim.y - 1, last = valid && k == N - 2;
    const bool dead = V.tv_status && !V.tv_status[b];
    const int fail = V.fail_knot[b];
    const bool live = valid && !dead && (fail == 0 || k + 1 < fail);   // (wave-uniform) else: zeros
    const Env E = problem_env(P, b);
    const double* Xk = V.X + ((size_t)b * N + k) * n;
    const double* Uk = V.U + ((size_t)b * N + k) * m;
    const double* Kk = V.K + ((size_t)b * (N - 1) + k) * m * n;
    const double* Sr = V.Srow + ((size_t)b * N + k) * NGZ;
    const double* Sb = V.Sbt + (size_t)b * NB * NB;
#pragma unroll
    for (int r = 0; r < RS; r++) {
        const int e = lane + 64 * r;
        if (e < NS) {
            const int i = e / NZ, c = e % NZ;
            sS[wv][e] = i < n ? Sr[e] : (c < n ? Sr[c * NZ + i] : Sb[(i - n) * NB + (c - n)]);
        }
    }
    double w2[m];
#pragma unroll
    for (int q = 0; q < m; q++) w2[q] = V.du_white[q] * V.du_white[q] + V.dw[q] * V.dw[q] / 3.0;
    const bool col = lane < NZ;
    const int j = col ? lane : 0;             // (idle lanes carry column 0 and store nothing)
    const int jx = j < n ? j : 0, jt = j >= nz ? j - nz : 0;
    double x[n], u[m], d[n], bu[n];
#pragma unroll
    for (int i = 0; i < n; i++) { x[i] = Xk[i]; d[i] = i == j ? 1.0 : 0.0; }
#pragma unroll
    for (int i = 0; i < m; i++) u[i] = Uk[i];
    {   // B du: B does not depend on the state in any model
        double Bm[n * m], du[m];
        D::B(P.mp, Bm);
#pragma unroll
        for (int c = 0; c < m; c++) du[c] = j < n ? -Kk[c * n + jx] : (n + c == j ? 1.0 : 0.0);
#pragma unroll
        for (int i = 0; i < n; i++) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < m; c++)
                if (T::Bnz(i, c)) s += Bm[i * m + c] * du[c];
            bu[i] = s;
        }
    }
    // the source of a stage: B du, and behind the controls df/dtheta_jt at the stage point
    auto source = [&](const double* xp, double* g) {
        D::dfdth(P.mp, xp, u, jt, g);
#pragma unroll
        for (int i = 0; i < n; i++) g[i] = j >= nz ? g[i] : bu[i];
    };
    __syncthreads();

    double zi = INFINITY, zreg = 0.0;
    int ji = -1, pi = -1, preg = 0;
    const int iend = nstep - 1 + (has_last ? 1 : 0);   // (uniform in the workgroup) the sample at i = nstep is knot N
    for (int i = 0; i <= iend; i++) {
        const bool end = i == nstep;
        if (end) {   // knot N, kept by the last interval's wave: X[:,N] and the knot pass's Sxx
            if (lane < WS) sX[wv][lane] = Xk[n + lane];
            if (lane < NSP) sSp[wv][lane] = Sr[NGZ + (lane / WS) * NZ + lane % WS];
        } else if (i == 0) {
            if (lane < WS) sX[wv][lane] = Xk[lane];
            if (lane < NSP) sSp[wv][lane] = sS[wv][(lane / WS) * NZ + lane % WS];
        } else {
            if (lane == 0)
#pragma unroll
                for (int a = 0; a < WS; a++) sX[wv][a] = x[a];
            if (col)
#pragma unroll
                for (int a = 0; a < WS; a++) sGp[wv][a * NZ + j] = d[a];
            __syncthreads();
#pragma unroll
            for (int r = 0; r < RGP; r++) {
                const int e = lane + 64 * r;
                if (e < NGP) {
                    const int a = e / NZ, c = e % NZ;
                    double s = 0.0;
#pragma unroll
                    for (int p = 0; p < NZ; p++) s += sGp[wv][a * NZ + p] * sS[wv][p * NZ + c];
                    sT[wv][e] = s;
                }
            }
            __syncthreads();
            if (lane < NSP && lane / WS <= lane % WS) {
                const int a = lane / WS, c = lane % WS;
                double s = 0.0;
#pragma unroll
                for (int p = 0; p < NZ; p++) s += sT[wv][a * NZ + p] * sGp[wv][c * NZ + p];
#pragma unroll
                for (int q = 0; q < m; q++) s += sGp[wv][a * NZ + n + q] * w2[q] * sGp[wv][c * NZ + n + q];
                sSp[wv][a * WS + c] = s;
                sSp[wv][c * WS + a] = s;
            }
        }
        __syncthreads();
        double zk;
        int pk;
        obstacle_margin<MODEL, WS>(P, E, sX[wv], sSp[wv], lane, &zk, &pk);
        const bool mine = valid && (!end || last);   // the sample is a row of this wave
        if (mine && live && zk < zi) { zi = zk; ji = k * nstep + i; pi = pk; }   // (strict: the first sample of equal minima)
        if (V.store_dense) {
            const size_t row = (size_t)b * V.rows + (size_t)k * nstep;
            if (mine && lane < NSP) V.Spos[(row + i) * NSP + lane] = live ? sSp[wv][lane] : 0.0;
            if (lane == (i & 63)) { zreg = live ? zk : 0.0; preg = live ? (pk == NO_ORD ? -1 : pk) : 0; }
            if ((i & 63) == 63 || i == iend) {
                const int i0 = i & ~63, il = i0 + lane;
                if (valid && il <= i && (il != nstep || last)) { V.z_dense[row + il] = zreg; V.pair_dense[row + il] = preg; }
            }
        }
        __syncthreads();   // (the readers of sX, sGp and sSp are done)
        if (i >= nstep - 1) continue;   // no substep behind the interval's last sample: the next interval restarts at its knot
#define RK4_TANGENT_SOURCE(xp, g) (source(xp, g), g)
#include "rk4_tangent.inc"
    }
    if (valid && lane == 0) {
        V.zint[(size_t)b * (N - 1) + k] = zi;
        V.jint[(size_t)b * (N - 1) + k] = ji;
        V.pint[(size_t)b * (N - 1) + k] = ji < 0 || pi == NO_ORD ? -1 : pi;
    }
}

// one wave per problem: the minimum over the intervals in their order (lane 0; a strict <, so the first sample of equal minima
// stays), and zeros in the rows behind nfull_b
template <int MODEL> __global__ void __launch_bounds__(64) lincov_dense_reduce(const KParams P, const DnArgs V) {
    constexpr int NSP = MT<MODEL>::WS * MT<MODEL>::WS;
    const int b = blockIdx.x, lane = threadIdx.x, N = P.N;
    if (V.active && !V.active[b]) return;
    const double dt = P.tf[b] / (N - 1);
    const int nstep = rollout_nstep(dt, V.nstep, V.dt_min);
    const int nfull = nstep * (N - 1) + 1;
    const bool dead = V.tv_status && !V.tv_status[b];
    if (lane == 0) {
        double zb = INFINITY;
        int jb = -1, pb = -1;
        for (int k = 0; k < N - 1; k++) {
            const double z = V.zint[(size_t)b * (N - 1) + k];
            if (z < zb) { zb = z; jb = V.jint[(size_t)b * (N - 1) + k]; pb = V.pint[(size_t)b * (N - 1) + k]; }
        }
        V.nfull[b] = nfull;
        V.min_z_dense[b] = dead ? 0.0 : zb;
        V.dense_sample[b] = dead ? 0 : jb;
        V.dense_pair[b] = dead ? 0 : pb;
    }
    if (V.store_dense) {
        for (int r = nfull + lane; r < V.rows; r += 64) { V.z_dense[(size_t)b * V.rows + r] = 0.0; V.pair_dense[(size_t)b * V.rows + r] = 0; }
        for (size_t e = (size_t)nfull * NSP + lane; e < (size_t)V.rows * NSP; e += 64) V.Spos[(size_t)b * V.rows * NSP + e] = 0.0;
    }
}

// The launches of one call, in their order on the handle's stream.  W: null for gusto_lincov, else V with the dispersion (V is
// its base) and A for the sensitivity launch; Dn: null, or (gusto_lincov_dense: W is set and V is an LcArgsD) the dense pass
template <int MODEL> int launch_lincov(gusto_handle h, const KParams& P, const LcArgs& V, const LcArgsP* W, const SensArgs& A,
                                       const DnArgs* Dn = nullptr) {
    if (W) {   // the sensitivities Cd of the dispersion
        const int tiles = (h->N - 1 + PlantCols<MODEL>::IPB - 1) / PlantCols<MODEL>::IPB;
        hipLaunchKernelGGL((lincov_plant_sens<MODEL>), dim3(h->B, tiles), dim3(256), 0, h->stream, P, A);
        HIPCHK(h, hipGetLastError());
    }
    // the knot pass
    if (Dn) hipLaunchKernelGGL((lincov_kernel<MODEL, true, true>), dim3(h->B), dim3(64), 0, h->stream, P, static_cast<const LcArgsD&>(V));
    else if (W) hipLaunchKernelGGL((lincov_kernel<MODEL, true>), dim3(h->B), dim3(64), 0, h->stream, P, *W);
    else hipLaunchKernelGGL((lincov_kernel<MODEL, false>), dim3(h->B), dim3(64), 0, h->stream, P, V);
    HIPCHK(h, hipGetLastError());
    if (Dn) {   // the dense pass and its reduction
        hipLaunchKernelGGL((lincov_dense<MODEL>), dim3(h->B, (h->N - 1 + 3) / 4), dim3(256), 0, h->stream, P, *Dn);
        HIPCHK(h, hipGetLastError());
        hipLaunchKernelGGL((lincov_dense_reduce<MODEL>), dim3(h->B), dim3(64), 0, h->stream, P, *Dn);
        HIPCHK(h, hipGetLastError());
    }
    return GUSTO_OK;
}

// gusto_lincov (dist = null) and gusto_lincov_disturbed (dist: the options, never null; Sth: the caller's or null);
// gusto_lincov_dense: store_dense = the caller's, not yet checked; else null
int lincov_host(gusto_handle h, const char* who_c, const double* X, const double* U, const double* K, const double* S0,
                const gusto_lincov_opts* opts, const gusto_disturb_opts* dist, const double* Sth, const int* store_dense = nullptr);

}  // namespace

extern "C" {

int gusto_default_lincov_opts(int model_id, gusto_lincov_opts* o) {
    const ModelInfo* mi = model_info(model_id);
    if (!o || !mi) return GUSTO_ERR_ARG;
    memset(o, 0, sizeof(*o));
    for (int i = 0; i < mi->n; i++) o->dx0[i] = 0.01;   // (a placeholder: the caller knows the units of its states)
    for (int i = 0; i < GUSTO_MAXM; i++) { o->u_lo[i] = -INFINITY; o->u_hi[i] = INFINITY; }
    return GUSTO_OK;
}

int gusto_lincov(gusto_handle h, const double* X, const double* U, const double* K, const double* S0, const gusto_lincov_opts* opts) {
    return lincov_host(h, "gusto_lincov", X, U, K, S0, opts, nullptr, nullptr);
}

int gusto_lincov_disturbed(gusto_handle h, const double* X, const double* U, const double* K, const double* S0, const double* Sth,
                           const gusto_lincov_opts* opts, const gusto_disturb_opts* d) {
    gusto_disturb_opts zero;
    gusto_default_disturb_opts(&zero);
    return lincov_host(h, "gusto_lincov_disturbed", X, U, K, S0, opts, d ? d : &zero, Sth);
}

int gusto_lincov_dense(gusto_handle h, const double* X, const double* U, const double* K, const double* S0, const double* Sth,
                       const gusto_lincov_opts* opts, const gusto_disturb_opts* d, int store_dense) {
    gusto_disturb_opts zero;
    gusto_default_disturb_opts(&zero);
    return lincov_host(h, "gusto_lincov_dense", X, U, K, S0, opts, d ? d : &zero, Sth, &store_dense);
}

}  // extern "C"

namespace {

int lincov_host(gusto_handle h, const char* who_c, const double* X, const double* U, const double* K, const double* S0,
                const gusto_lincov_opts* opts, const gusto_disturb_opts* dist, const double* Sth, const int* store_dense) {
    if (int rc = post_enter(h, who_c, X, U)) return rc;   // (the handle first: the refusals of every stage)
    if (store_dense)
        if (int rc = lincov_dense_args_host(*store_dense, &h->err)) return rc;
    const int dense = store_dense ? *store_dense : -1;    // 0 / 1: gusto_lincov_dense; -1: the knot pass alone
    const std::string who(who_c);
    gusto_lincov_opts o;
    gusto_default_lincov_opts(h->model, &o);
    if (opts) o = *opts;
    if (int rc = lincov_args_host(h->n, h->m, h->B, &o, S0, &h->err, who_c)) return rc;
    if (dist)
        if (int rc = lincov_plant_args_host(h->model, h->m, h->B, dist, Sth, &h->err, who_c)) return rc;
    if (!h->tvlqr.have) {
        h->err = who + ": no discrete Jacobians: call gusto_tvlqr first";
        return GUSTO_ERR_STATE;
    }
    LincovState& S = h->lincov;
    const size_t Bc = h->batch_cap, B = h->B, N = h->N, n = h->n, m = h->m, nz = n + m, NT = GUSTO_NPLANT;
    KParams P = post_params(h);
    if (!fill_env(h, P, model_info(h->model)->has_obs, true)) {
        h->err = who + ": gusto_set_env_batch was called with a different number of problems than gusto_set_problems";
        return GUSTO_ERR_STATE;
    }
    // grow-only, zeroed when (re)allocated
    HIPCHK(h, S.I.ensure_zeroed(6 * Bc, h->stream)); HIPCHK(h, S.D.ensure_zeroed(3 * Bc, h->stream));
    HIPCHK(h, S.Sx.ensure_zeroed(Bc * N * n, h->stream)); HIPCHK(h, S.Su.ensure_zeroed(Bc * (N - 1) * m, h->stream));
    HIPCHK(h, S.Z.ensure_zeroed(Bc * N, h->stream));
    if (o.store_S) HIPCHK(h, S.Sxx.ensure_zeroed(Bc * N * n * n, h->stream));
    if (!S.have) S.have_Sxx = false;   // (new problems: whatever Sxx the buffer holds belongs to the old ones)
    // a masked first call since gusto_set_problems: the inactive problems read as zeros (an unmasked call writes every problem)
    if (h->n_active >= 0) {
        if (!S.have) {
            HIPCHK(h, hipMemsetAsync(S.I, 0, sizeof(int) * S.I.count(), h->stream));
            HIPCHK(h, hipMemsetAsync(S.D, 0, sizeof(double) * S.D.count(), h->stream));
            HIPCHK(h, hipMemsetAsync(S.Sx, 0, sizeof(double) * S.Sx.count(), h->stream));
            HIPCHK(h, hipMemsetAsync(S.Su, 0, sizeof(double) * S.Su.count(), h->stream));
            HIPCHK(h, hipMemsetAsync(S.Z, 0, sizeof(double) * S.Z.count(), h->stream));
        }
        if (o.store_S && !S.have_Sxx) HIPCHK(h, hipMemsetAsync(S.Sxx, 0, sizeof(double) * S.Sxx.count(), h->stream));
    }
    if (dist) {   // (Cd and Sxt of a problem this call leaves out are those of the last disturbed call, or zeros)
        HIPCHK(h, S.Cd.ensure_zeroed(Bc * (N - 1) * n * NT, h->stream));
        if (o.store_S) HIPCHK(h, S.Sxt.ensure_zeroed(Bc * N * n * NT, h->stream));
        if (h->n_active >= 0 && !(S.have && S.plant)) {
            HIPCHK(h, hipMemsetAsync(S.Cd, 0, sizeof(double) * S.Cd.count(), h->stream));
            if (S.Sxt.count()) HIPCHK(h, hipMemsetAsync(S.Sxt, 0, sizeof(double) * S.Sxt.count(), h->stream));
        }
    }
    // gusto_lincov_dense: the x-rows of S and the per-interval minima; the per-sample arrays with store_dense.  A first call since
    // gusto_set_problems, or another row count: zeros everywhere (what an inactive problem then reads)
    const size_t NZ = nz + NT, NB = m + NT;
    size_t rows = 0, nsp = 0;
    if (dense >= 0) {
        int ws = 0;
        for_model(h->model, [&](auto M) { ws = MT<M()>::WS; return GUSTO_OK; });
        nsp = (size_t)ws * ws;
        rows = (size_t)h->tvlqr.nstep_max * (N - 1) + 1;
        const bool fresh = !S.have_dense || S.dense_rows != rows;
        HIPCHK(h, S.Srow.ensure_zeroed(Bc * N * n * NZ, h->stream)); HIPCHK(h, S.Sbt.ensure_zeroed(Bc * NB * NB, h->stream));
        HIPCHK(h, S.Zint.ensure_zeroed(Bc * (N - 1), h->stream)); HIPCHK(h, S.Jint.ensure_zeroed(2 * Bc * (N - 1), h->stream));
        HIPCHK(h, S.DI.ensure_zeroed(3 * Bc, h->stream)); HIPCHK(h, S.DD.ensure_zeroed(Bc, h->stream));
        if (fresh) {
            HIPCHK(h, hipMemsetAsync(S.DI, 0, sizeof(int) * S.DI.count(), h->stream));
            HIPCHK(h, hipMemsetAsync(S.DD, 0, sizeof(double) * S.DD.count(), h->stream));
            S.have_dense_rows = false;
        }
        if (dense) {
            HIPCHK(h, S.Zd.ensure_zeroed(Bc * rows, h->stream)); HIPCHK(h, S.Pd.ensure_zeroed(Bc * rows, h->stream));
            HIPCHK(h, S.Spos.ensure_zeroed(Bc * rows * nsp, h->stream));
            if (!S.have_dense_rows) {
                HIPCHK(h, hipMemsetAsync(S.Zd, 0, sizeof(double) * S.Zd.count(), h->stream));
                HIPCHK(h, hipMemsetAsync(S.Pd, 0, sizeof(int) * S.Pd.count(), h->stream));
                HIPCHK(h, hipMemsetAsync(S.Spos, 0, sizeof(double) * S.Spos.count(), h->stream));
            }
        }
    }
    LcArgsD V{};
    SensArgs A{};
    DnArgs Dn{};
    if (int rc = stage_traj(h, X, U, Bc, S.X, S.U, &V.X, &V.U)) return rc;
    V.AB = h->tvlqr.AB;
    V.K = h->tvlqr.K;
    V.tv_status = h->tvlqr.St; V.tv_fail = h->tvlqr.St + h->tvlqr.St.count() / 2;
    if (K) {
        HIPCHK(h, S.K.ensure(Bc * (N - 1) * m * n));
        HIPCHK(h, hipMemcpyAsync(S.K, K, sizeof(double) * B * (N - 1) * m * n, hipMemcpyHostToDevice, h->stream));
        V.K = S.K; V.tv_status = nullptr; V.tv_fail = nullptr;
    }
    if (S0) {
        HIPCHK(h, S.S0.ensure(Bc * nz * nz));
        HIPCHK(h, hipMemcpyAsync(S.S0, S0, sizeof(double) * B * nz * nz, hipMemcpyHostToDevice, h->stream));
        V.S0 = S.S0;
    }
    V.active = active_mask(h);
    memcpy(V.dx0, o.dx0, sizeof(V.dx0)); memcpy(V.du0, o.du0, sizeof(V.du0)); memcpy(V.du_white, o.du_white, sizeof(V.du_white));
    memcpy(V.u_lo, o.u_lo, sizeof(V.u_lo)); memcpy(V.u_hi, o.u_hi, sizeof(V.u_hi));
    V.store_S = o.store_S;
    V.status = S.I; V.fail_knot = S.I + Bc; V.obs_knot = S.I + 2 * Bc; V.obs_pair = S.I + 3 * Bc; V.ctl_knot = S.I + 4 * Bc;
    V.ctl_entry = S.I + 5 * Bc;
    V.min_z_obs = S.D; V.p_bound = S.D + Bc; V.min_z_ctl = S.D + 2 * Bc;
    V.sigma_x = S.Sx; V.sigma_u = S.Su; V.z_obs = S.Z; V.Sxx = S.Sxx;
    if (dist) {
        if (Sth) {
            HIPCHK(h, S.Sth.ensure(Bc * NT * NT));
            HIPCHK(h, hipMemcpyAsync(S.Sth, Sth, sizeof(double) * B * NT * NT, hipMemcpyHostToDevice, h->stream));
            V.Sth = S.Sth;
        }
        memcpy(V.plant_rel, dist->plant_rel, sizeof(V.plant_rel)); memcpy(V.dw, dist->dw, sizeof(V.dw));
        V.Cd = S.Cd; V.Sxt = S.Sxt;
        A.X = V.X; A.U = V.U; A.active = V.active; A.Cd = S.Cd;
        A.dt_min = h->tvlqr.dt_min; A.nstep = h->tvlqr.nstep;
    }
    if (dense >= 0) {
        V.Srow = S.Srow; V.Sbt = S.Sbt;
        Dn.X = V.X; Dn.U = V.U; Dn.K = V.K; Dn.Srow = S.Srow; Dn.Sbt = S.Sbt; Dn.active = V.active; Dn.tv_status = V.tv_status;
        Dn.fail_knot = V.fail_knot; Dn.dt_min = A.dt_min; Dn.nstep = A.nstep;
        memcpy(Dn.du_white, V.du_white, sizeof(Dn.du_white)); memcpy(Dn.dw, V.dw, sizeof(Dn.dw));
        Dn.store_dense = dense; Dn.rows = (int)rows;
        Dn.zint = S.Zint; Dn.jint = S.Jint; Dn.pint = S.Jint + Bc * (N - 1);
        Dn.z_dense = S.Zd; Dn.pair_dense = S.Pd; Dn.Spos = S.Spos;
        Dn.nfull = S.DI; Dn.dense_sample = S.DI + Bc; Dn.dense_pair = S.DI + 2 * Bc; Dn.min_z_dense = S.DD;
    }
    HIPCHK(h, S.t0.record(h->stream));
    if (int rc = for_model(h->model, [&](auto M) { return launch_lincov<M()>(h, P, V, dist ? &V : nullptr, A, dense >= 0 ? &Dn : nullptr); })) return rc;
    HIPCHK(h, S.t1.record(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, event_ms(S.t0, S.t1, &S.last_ms));
    if (o.store_S) S.have_Sxx = true;
    S.have = true;
    S.store_S = o.store_S != 0;
    S.plant = dist != nullptr;
    S.staged = X != nullptr;
    S.dense = dense >= 0;
    if (dense >= 0) {
        S.have_dense = true; S.dense_rows = rows; S.dense_nsp = nsp; S.store_dense = dense != 0;
        if (dense) S.have_dense_rows = true;
    }
    return GUSTO_OK;
}

}  // namespace

extern "C" {

int gusto_get_lincov_plant(gusto_handle h, double* Cd, double* Sxt) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    const LincovState& S = h->lincov;
    if (!S.have || !S.plant) { h->err = "gusto_get_lincov_plant: the last covariance analysis was not a gusto_lincov_disturbed"; return GUSTO_ERR_STATE; }
    if (Sxt && !S.store_S) { h->err = "gusto_get_lincov_plant: the last gusto_lincov_disturbed did not run with store_S = 1"; return GUSTO_ERR_STATE; }
    const size_t B = h->B, N = h->N, n = h->n;
    if (int rc = copy_out(h, Cd, S.Cd, B * (N - 1) * n * GUSTO_NPLANT)) return rc;
    return copy_out(h, Sxt, S.Sxt, B * N * n * GUSTO_NPLANT);
}

int gusto_get_lincov(gusto_handle h, gusto_lincov_report* out) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    if (!out) return GUSTO_ERR_ARG;
    const LincovState& S = h->lincov;
    if (!S.have) { h->err = "gusto_get_lincov: call gusto_lincov first"; return GUSTO_ERR_STATE; }
    if (out->Sxx && !S.store_S) { h->err = "gusto_get_lincov: the last gusto_lincov did not run with store_S = 1"; return GUSTO_ERR_STATE; }
    const size_t B = h->B, Bc = h->batch_cap, N = h->N, n = h->n, m = h->m;
    if (int rc = copy_out(h, out->status, S.I, B)) return rc;
    if (int rc = copy_out(h, out->fail_knot, S.I + Bc, B)) return rc;
    if (int rc = copy_out(h, out->obs_knot, S.I + 2 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->obs_pair, S.I + 3 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->ctl_knot, S.I + 4 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->ctl_entry, S.I + 5 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->min_z_obs, S.D, B)) return rc;
    if (int rc = copy_out(h, out->p_collision_bound, S.D + Bc, B)) return rc;
    if (int rc = copy_out(h, out->min_z_ctl, S.D + 2 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->sigma_x, S.Sx, B * N * n)) return rc;
    if (int rc = copy_out(h, out->sigma_u, S.Su, B * (N - 1) * m)) return rc;
    if (int rc = copy_out(h, out->z_obs, S.Z, B * N)) return rc;
    return copy_out(h, out->Sxx, S.Sxx, B * N * n * n);
}

int gusto_get_lincov_dense(gusto_handle h, gusto_lincov_dense_report* out, int* nfull_max) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    const LincovState& S = h->lincov;
    if (!S.have || !S.dense) { h->err = "gusto_get_lincov_dense: the last covariance analysis was not a gusto_lincov_dense"; return GUSTO_ERR_STATE; }
    if (nfull_max) *nfull_max = (int)S.dense_rows;
    if (!out) return GUSTO_OK;
    if ((out->z_dense || out->pair_dense || out->Spos) && !S.store_dense) {
        h->err = "gusto_get_lincov_dense: the last gusto_lincov_dense did not run with store_dense = 1";
        return GUSTO_ERR_STATE;
    }
    const size_t B = h->B, Bc = h->batch_cap, rows = S.dense_rows;
    if (int rc = copy_out(h, out->nfull, S.DI, B)) return rc;
    if (int rc = copy_out(h, out->dense_sample, S.DI + Bc, B)) return rc;
    if (int rc = copy_out(h, out->dense_pair, S.DI + 2 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->min_z_dense, S.DD, B)) return rc;
    if (int rc = copy_out(h, out->z_dense, S.Zd, B * rows)) return rc;
    if (int rc = copy_out(h, out->pair_dense, S.Pd, B * rows)) return rc;
    return copy_out(h, out->Spos, S.Spos, B * rows * S.dense_nsp);
}

int gusto_last_lincov_ms(gusto_handle h, double* ms) {
    if (!h || !ms) return GUSTO_ERR_ARG;
    if (!h->lincov.have) { h->err = "gusto_last_lincov_ms: call gusto_lincov first"; return GUSTO_ERR_STATE; }
    *ms = h->lincov.last_ms;
    return GUSTO_OK;
}

}  // extern "C"
