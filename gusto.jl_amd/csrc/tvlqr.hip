// tvlqr.hip -- batched time-varying LQR tracking gains around the trajectories of a batch: u = U_k - K_k (x(t_k) - X_k).
// No counterpart in the reference; include/gusto_hip.h states the definitions (roll-out map, discrete Jacobians, recursion).
// Two launches on the handle's stream:
//   tvlqr_linearise  grid (problem, tile of IPB intervals), 256 lanes.  Work item (k, j) = lane: interval k, column j of
//     [dF_k/dx | dF_k/du].  A lane carries the nominal state (every lane of an interval recomputes the cheap nominal roll-out)
//     and ONE tangent column, 2 n doubles, through the four RK4 stages of every substep (rk4_tangent.inc, the text lincov.hip's
//     linearising kernels include too): kd = A(stage point) d + B e_j, with
//     Dyn<MODEL>::A written into a local array that full unrolling dissolves -- only its structural nonzeros (MT<MODEL>::Anz) are
//     multiplied, nothing indexes it at run time.  A lane owns column j of the n rows of its interval, n + m doubles apart: the tile is staged in LDS
//     ([interval][row][column], the layout of AB) and copied out by the whole workgroup, consecutive lanes to consecutive
//     addresses (as verify.hip stages its dense samples).
//   tvlqr_riccati    one wave per problem, for every N.  P, [Ad | Bd], T = P [Ad Bd], H and W live in LDS (9.4 KB for n = 13); the
//     64 lanes split the entries of every product (entry e = lane + 64 r), each entry one dot product in a fixed order.  H and
//     P' are computed on the upper triangle and mirrored, so P is symmetric to the bit.  The m x m Cholesky (m <= 6) is done by
//     every lane on the same LDS values -- the pivot test is wave-uniform without a broadcast -- and lane j < n then solves
//     column j of W = L^-1 H_ux and K = L^-T W.  [Ad | Bd] of the next stage is loaded into registers before the current stage
//     computes.  K (and P with store_P) go out from LDS, lane e to double e.
//     (The same stage with every product on v_mfma_f64_16x16x4_f64 and P resident in accumulators, modelled on
//     factor_sweep_mfma, was built and measured for the 12/13-state models: 0.856 ms against 0.803 ms for this one at 8192
//     astrobeeSE3 problems, N = 50 -- profiles/tvlqr.txt.  It lost and is not in the library.)
// No atomics, nothing crosses a problem: a problem's output is the same bit for bit whatever batch it sits in.
#include <hip/hip_runtime.h>

#include "post.hpp"
#include "rollout.hpp"

using namespace gusto;

namespace {

struct TvArgs {
    const double *X, *U;     // [B][N][n], [B][N][m]: the handle's trajectories or the caller's copies
    const int* active;       // gusto_set_active: null = every problem, else the mask [B]
    double dt_min;
    int nstep, store_P;
    double Q[GUSTO_MAXN], R[GUSTO_MAXM], Qf[GUSTO_MAXN];
    double *AB, *K, *P1, *Pall;
    int *status, *fail_knot;
};

template <int MODEL> struct LinTile {
    static constexpr int n = MT<MODEL>::n, m = MT<MODEL>::m, nz = n + m;
    static constexpr int IPB = 256 / nz;   // whole intervals per workgroup: its slice of AB is one contiguous range
};

template <int MODEL> __global__ void __launch_bounds__(256) tvlqr_linearise(const KParams P, const TvArgs V) {
    using D = Dyn<MODEL>;
    using LT = LinTile<MODEL>;
    constexpr int n = LT::n, m = LT::m, nz = LT::nz, IPB = LT::IPB;
    __shared__ double stage[IPB * n * nz];
    const int b = blockIdx.x, k0 = blockIdx.y * IPB, t = threadIdx.x, N = P.N;
    if (V.active && !V.active[b]) return;   // (the whole workgroup)
    const double dt = P.tf[b] / (N - 1);
    const int nstep = rollout_nstep(dt, V.nstep, V.dt_min);
    const double h = dt / nstep;
    const int kl = t / nz, j = t % nz;
    const bool valid = kl < IPB && k0 + kl < N - 1;
    const int k = valid ? k0 + kl : 0;   // (idle lanes roll interval 0 out and store nothing)
    const double* Xk = V.X + ((size_t)b * N + k) * n;
    const double* Uk = V.U + ((size_t)b * N + k) * m;
    double x[n], u[m], d[n], bu[n];
#pragma unroll
    for (int i = 0; i < n; i++) { x[i] = Xk[i]; d[i] = i == j ? 1.0 : 0.0; }
#pragma unroll
    for (int i = 0; i < m; i++) u[i] = Uk[i];
    {   // B e_j: B does not depend on the state in any model
        double Bm[n * m];
        D::B(P.mp, Bm);
#pragma unroll
        for (int i = 0; i < n; i++) {
            double s = 0.0;
#pragma unroll
            for (int c = 0; c < m; c++)
                if (MT<MODEL>::Bnz(i, c)) s += n + c == j ? Bm[i * m + c] : 0.0;
            bu[i] = s;
        }
    }
    for (int s = 0; s < nstep; s++) {
#define RK4_TANGENT_SOURCE(xp, g) bu   // B e_j, the same at every stage point
#include "rk4_tangent.inc"
    }
    if (valid)
#pragma unroll
        for (int i = 0; i < n; i++) stage[(kl * n + i) * nz + j] = d[i];
    __syncthreads();
    const int cnt = min(IPB, N - 1 - k0) * n * nz;
    double* out = V.AB + ((size_t)b * (N - 1) + k0) * n * nz;
    for (int e = t; e < cnt; e += 256) out[e] = stage[e];
}

template <int MODEL> __global__ void __launch_bounds__(64) tvlqr_riccati(const KParams P, const TvArgs V) {
    constexpr int n = MT<MODEL>::n, m = MT<MODEL>::m, nz = n + m;
    constexpr int NG = n * nz, RG = (NG + 63) / 64;                 // entries of [Ad | Bd] and of T, per lane
    constexpr int NH = nz * (nz + 1) / 2, RH = (NH + 63) / 64;      // upper triangle of H
    constexpr int NP = n * (n + 1) / 2, RP = (NP + 63) / 64;        // upper triangle of P
    constexpr int NK = m * n, RK = (NK + 63) / 64, NPF = n * n, RPF = (NPF + 63) / 64;
    __shared__ double sP[n * n], sG[NG], sT[NG], sH[nz * nz], sW[NK], sK[NK];
    const int b = blockIdx.x, lane = threadIdx.x, N = P.N;
    if (V.active && !V.active[b]) return;
    const double* AB = V.AB + (size_t)b * (N - 1) * NG;
    double* Kout = V.K + (size_t)b * (N - 1) * NK;
    double* Pall = V.store_P ? V.Pall + (size_t)b * N * NPF : nullptr;

    // the entries this lane owns: (row, column) of the upper triangles, found once
    int ha[RH], hb[RH], pa[RP], pb[RP];
#pragma unroll
    for (int r = 0; r < RH; r++) {
        int rem = lane + 64 * r, a = 0;
        if (rem >= NH) rem = 0;
        while (rem >= nz - a) { rem -= nz - a; a++; }
        ha[r] = a; hb[r] = a + rem;
    }
#pragma unroll
    for (int r = 0; r < RP; r++) {
        int rem = lane + 64 * r, a = 0;
        if (rem >= NP) rem = 0;
        while (rem >= n - a) { rem -= n - a; a++; }
        pa[r] = a; pb[r] = a + rem;
    }
    // P_N = diag(Qf)
#pragma unroll
    for (int r = 0; r < RPF; r++) {
        const int e = lane + 64 * r;
        if (e < NPF) {
            const double v = e / n == e % n ? V.Qf[e / n] : 0.0;
            sP[e] = v;
            if (Pall) Pall[(size_t)(N - 1) * NPF + e] = v;
        }
    }
    double g[RG];
#pragma unroll
    for (int r = 0; r < RG; r++) { const int e = lane + 64 * r; g[r] = e < NG ? AB[(size_t)(N - 2) * NG + e] : 0.0; }
#pragma unroll
    for (int r = 0; r < RG; r++) { const int e = lane + 64 * r; if (e < NG) sG[e] = g[r]; }
    __syncthreads();

    int fail = 0;
    for (int k = N - 1; k >= 1; k--) {   // knot k (1-based): interval k - 1 of the arrays
        if (k > 1)                       // [Ad | Bd] of the next stage, in flight while this one computes
#pragma unroll
            for (int r = 0; r < RG; r++) { const int e = lane + 64 * r; g[r] = e < NG ? AB[(size_t)(k - 2) * NG + e] : 0.0; }
        // T = P [Ad Bd]
#pragma unroll
        for (int r = 0; r < RG; r++) {
            const int e = lane + 64 * r;
            if (e < NG) {
                const int i = e / nz, c = e % nz;
                double s = 0.0;
#pragma unroll
                for (int p = 0; p < n; p++) s += sP[i * n + p] * sG[p * nz + c];
                sT[e] = s;
            }
        }
        __syncthreads();
        // H = diag(Q, R) + [Ad Bd]' T, upper triangle, mirrored
#pragma unroll
        for (int r = 0; r < RH; r++) {
            if (lane + 64 * r < NH) {
                const int a = ha[r], c = hb[r];
                double s = a == c ? (a < n ? V.Q[a] : V.R[a - n]) : 0.0;
#pragma unroll
                for (int p = 0; p < n; p++) s += sG[p * nz + a] * sT[p * nz + c];
                sH[a * nz + c] = s;
                sH[c * nz + a] = s;
            }
        }
        __syncthreads();
        if (k > 1)
#pragma unroll
            for (int r = 0; r < RG; r++) { const int e = lane + 64 * r; if (e < NG) sG[e] = g[r]; }
        // L = chol(H_uu): every lane, the same values
        double L[m][m];
        bool bad = false;
#pragma unroll
        for (int c = 0; c < m; c++) {
            double dg = sH[(n + c) * nz + n + c];
#pragma unroll
            for (int p = 0; p < c; p++) dg -= L[c][p] * L[c][p];
            if (!(dg > 0.0) || !(dg < INFINITY)) bad = true;
            const double l = sqrt(dg);
            L[c][c] = l;
#pragma unroll
            for (int q = c + 1; q < m; q++) {
                double s = sH[(n + q) * nz + n + c];
#pragma unroll
                for (int p = 0; p < c; p++) s -= L[q][p] * L[c][p];
                L[q][c] = s / l;
            }
        }
        if (bad) { fail = k; break; }   // (wave-uniform)
        // W = L^-1 H_ux, K = L^-T W: lane j solves column j
        if (lane < n) {
            double w[m];
#pragma unroll
            for (int c = 0; c < m; c++) {
                double s = sH[(n + c) * nz + lane];
#pragma unroll
                for (int p = 0; p < c; p++) s -= L[c][p] * w[p];
                w[c] = s / L[c][c];
                sW[c * n + lane] = w[c];
            }
#pragma unroll
            for (int c = m - 1; c >= 0; c--) {
                double s = w[c];
#pragma unroll
                for (int p = c + 1; p < m; p++) s -= L[p][c] * w[p];
                w[c] = s / L[c][c];
                sK[c * n + lane] = w[c];
            }
        }
        __syncthreads();
        // P_k = H_xx - W' W, upper triangle, mirrored
#pragma unroll
        for (int r = 0; r < RP; r++) {
            if (lane + 64 * r < NP) {
                const int a = pa[r], c = pb[r];
                double s = sH[a * nz + c];
#pragma unroll
                for (int p = 0; p < m; p++) s -= sW[p * n + a] * sW[p * n + c];
                sP[a * n + c] = s;
                sP[c * n + a] = s;
            }
        }
#pragma unroll
        for (int r = 0; r < RK; r++) { const int e = lane + 64 * r; if (e < NK) Kout[(size_t)(k - 1) * NK + e] = sK[e]; }
        __syncthreads();
        if (Pall)
#pragma unroll
            for (int r = 0; r < RPF; r++) { const int e = lane + 64 * r; if (e < NPF) Pall[(size_t)(k - 1) * NPF + e] = sP[e]; }
    }
    // a failed pivot at knot `fail`: zeros from there down to knot 1
    for (int k = fail; k >= 1; k--) {
#pragma unroll
        for (int r = 0; r < RK; r++) { const int e = lane + 64 * r; if (e < NK) Kout[(size_t)(k - 1) * NK + e] = 0.0; }
        if (Pall)
#pragma unroll
            for (int r = 0; r < RPF; r++) { const int e = lane + 64 * r; if (e < NPF) Pall[(size_t)(k - 1) * NPF + e] = 0.0; }
    }
#pragma unroll
    for (int r = 0; r < RPF; r++) { const int e = lane + 64 * r; if (e < NPF) V.P1[(size_t)b * NPF + e] = fail ? 0.0 : sP[e]; }
    if (lane == 0) { V.status[b] = fail ? 0 : 1; V.fail_knot[b] = fail; }
}

template <int MODEL> int launch_tvlqr(gusto_handle h, const KParams& P, const TvArgs& V) {
    const int tiles = (h->N - 1 + LinTile<MODEL>::IPB - 1) / LinTile<MODEL>::IPB;
    hipLaunchKernelGGL((tvlqr_linearise<MODEL>), dim3(h->B, tiles), dim3(256), 0, h->stream, P, V);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, h->tvlqr.mid.record(h->stream));
    hipLaunchKernelGGL((tvlqr_riccati<MODEL>), dim3(h->B), dim3(64), 0, h->stream, P, V);
    HIPCHK(h, hipGetLastError());
    return GUSTO_OK;
}

}  // namespace

extern "C" {

int gusto_default_tvlqr_opts(int model_id, gusto_tvlqr_opts* o) {
    const ModelInfo* mi = model_info(model_id);
    if (!o || !mi) return GUSTO_ERR_ARG;
    memset(o, 0, sizeof(*o));
    for (int i = 0; i < mi->n; i++) o->Q[i] = o->Qf[i] = 1.0;
    for (int i = 0; i < mi->m; i++) o->R[i] = 1.0;
    o->dt_min = 0.1; o->nstep = 0; o->nstep_cap = 64; o->store_P = 0;
    return GUSTO_OK;
}

int gusto_tvlqr(gusto_handle h, const double* X, const double* U, const gusto_tvlqr_opts* opts) {
    if (int rc = post_enter(h, "gusto_tvlqr", X, U)) return rc;
    gusto_tvlqr_opts o;
    gusto_default_tvlqr_opts(h->model, &o);
    if (opts) o = *opts;
    if (!nstep_opts_ok(o.dt_min, o.nstep, o.nstep_cap) || (o.store_P != 0 && o.store_P != 1)) {
        h->err = "gusto_tvlqr: bad options";
        return GUSTO_ERR_ARG;
    }
    for (int i = 0; i < h->n; i++)
        if (!(o.Q[i] >= 0 && o.Q[i] < INFINITY && o.Qf[i] >= 0 && o.Qf[i] < INFINITY)) {
            h->err = "gusto_tvlqr: Q and Qf must be finite and >= 0 (entry " + std::to_string(i) + ")";
            return GUSTO_ERR_ARG;
        }
    for (int i = 0; i < h->m; i++)
        if (!(o.R[i] > 0 && o.R[i] < INFINITY)) {
            h->err = "gusto_tvlqr: R must be finite and > 0 (entry " + std::to_string(i) + ")";
            return GUSTO_ERR_ARG;
        }
    TvlqrState& S = h->tvlqr;
    const size_t B = h->B, N = h->N, n = h->n, m = h->m;
    int nstep_max = 0;   // (as gusto_verify; gusto_lincov_dense sizes its per-sample arrays by the largest count)
    if (int rc = resolve_nstep(h, "gusto_tvlqr", o.dt_min, o.nstep, o.nstep_cap, &nstep_max)) return rc;
    const KParams P = post_params(h);
    // grow-only, zeroed when (re)allocated.  Growing discards the contents: it happens only after a gusto_set_problems with a
    // larger batch, which has invalidated them (S.have) anyway
    HIPCHK(h, S.AB.ensure_zeroed(B * (N - 1) * n * (n + m), h->stream));
    HIPCHK(h, S.K.ensure_zeroed(B * (N - 1) * m * n, h->stream));
    HIPCHK(h, S.P1.ensure_zeroed(B * n * n, h->stream));
    HIPCHK(h, S.St.ensure_zeroed(2 * B, h->stream));
    if (o.store_P) HIPCHK(h, S.Pall.ensure_zeroed(B * N * n * n, h->stream));
    if (!S.have) S.have_Pall = false;   // (new problems: whatever P the buffer holds belongs to the old ones)
    // a masked first call since gusto_set_problems: the inactive problems read as zeros, not as the last problem set's gains
    // (an unmasked call writes every problem)
    if (h->n_active >= 0) {
        if (!S.have) {
            HIPCHK(h, hipMemsetAsync(S.AB, 0, sizeof(double) * S.AB.count(), h->stream));
            HIPCHK(h, hipMemsetAsync(S.K, 0, sizeof(double) * S.K.count(), h->stream));
            HIPCHK(h, hipMemsetAsync(S.P1, 0, sizeof(double) * S.P1.count(), h->stream));
            HIPCHK(h, hipMemsetAsync(S.St, 0, sizeof(int) * S.St.count(), h->stream));
        }
        if (o.store_P && !S.have_Pall) HIPCHK(h, hipMemsetAsync(S.Pall, 0, sizeof(double) * S.Pall.count(), h->stream));
    }
    TvArgs V{};
    if (int rc = stage_traj(h, X, U, B, S.X, S.U, &V.X, &V.U)) return rc;
    V.active = active_mask(h);
    V.dt_min = o.dt_min; V.nstep = o.nstep; V.store_P = o.store_P;
    memcpy(V.Q, o.Q, sizeof(V.Q)); memcpy(V.R, o.R, sizeof(V.R)); memcpy(V.Qf, o.Qf, sizeof(V.Qf));
    V.AB = S.AB; V.K = S.K; V.P1 = S.P1; V.Pall = S.Pall;
    V.status = S.St; V.fail_knot = S.St + S.St.count() / 2;
    HIPCHK(h, S.t0.record(h->stream));
    if (int rc = for_model(h->model, [&](auto M) { return launch_tvlqr<M()>(h, P, V); })) return rc;
    HIPCHK(h, S.t1.record(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, event_ms(S.t0, S.t1, &S.last_ms));
    HIPCHK(h, event_ms(S.t0, S.mid, &S.lin_ms));
    HIPCHK(h, event_ms(S.mid, S.t1, &S.ric_ms));
    if (o.store_P) S.have_Pall = true;
    S.have = true;
    S.store_P = o.store_P != 0;
    S.dt_min = o.dt_min; S.nstep = o.nstep; S.nstep_max = nstep_max;
    return GUSTO_OK;
}

int gusto_get_tvlqr(gusto_handle h, int* status, int* fail_knot, double* K, double* Pm, double* AB) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    const TvlqrState& S = h->tvlqr;
    if (!S.have) { h->err = "gusto_get_tvlqr: call gusto_tvlqr first"; return GUSTO_ERR_STATE; }
    const size_t B = h->B, N = h->N, n = h->n, m = h->m;
    if (int rc = copy_out(h, status, S.St, B)) return rc;
    if (int rc = copy_out(h, fail_knot, S.St + S.St.count() / 2, B)) return rc;
    if (int rc = copy_out(h, K, S.K, B * (N - 1) * m * n)) return rc;
    if (int rc = copy_out(h, AB, S.AB, B * (N - 1) * n * (n + m))) return rc;
    return S.store_P ? copy_out(h, Pm, S.Pall, B * N * n * n) : copy_out(h, Pm, S.P1, B * n * n);
}

int gusto_dev_tvlqr(gusto_handle h, double* linearise_ms, double* riccati_ms) {
    if (!h) return GUSTO_ERR_ARG;
    if (!h->tvlqr.have) { h->err = "gusto_dev_tvlqr: call gusto_tvlqr first"; return GUSTO_ERR_STATE; }
    if (linearise_ms) *linearise_ms = h->tvlqr.lin_ms;
    if (riccati_ms) *riccati_ms = h->tvlqr.ric_ms;
    return GUSTO_OK;
}

int gusto_last_tvlqr_ms(gusto_handle h, double* ms) {
    if (!h || !ms) return GUSTO_ERR_ARG;
    if (!h->tvlqr.have) { h->err = "gusto_last_tvlqr_ms: call gusto_tvlqr first"; return GUSTO_ERR_STATE; }
    *ms = h->tvlqr.last_ms;
    return GUSTO_OK;
}

}  // extern "C"
