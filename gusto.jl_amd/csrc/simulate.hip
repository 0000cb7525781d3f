// simulate.hip -- closed-loop Monte Carlo roll-outs of the tracking law u = U_k - K_k (x(t_k) - X_k) around every trajectory of
// a batch, from perturbed starts and with clipped controls.  No counterpart in the reference; include/gusto_hip.h states the
// definitions (roll-out, dense samples, distance, non-finite samples, the generated perturbations).
// LANE = SAMPLE, a wave is 64 samples of ONE problem.  Grid (problem, tile of up to 256 samples), 64 ceil(samples / 64) lanes.
// X_k, U_k, K_k, tf, the substep count and every obstacle index are wave-uniform: the nominal data, the gains of a knot and the
// control bounds are copied to LDS once per knot by the whole workgroup and read by every lane at the same address (a
// broadcast; as scalar loads they cost the 12/13-state kernels ~200 spilled SGPRs and a private segment), the obstacle tables
// go through the constant address space as in verify.hip; only the state, the held control, the perturbation of the control
// and the RK4 stages are per lane.
// Loop bounds are wave-uniform; a lane without a sample, or whose state went non-finite, is predicated off and keeps its state.
// Per-sample results go out lane s to element s.  The per-problem report is reduce_problem(), a reduction over the per-sample
// arrays in a fixed order and without atomics: at the end of the roll-out kernel when one tile holds all samples (the
// workgroup reads back what it wrote), otherwise in a second small launch -- the same code, the same bits.  Nothing crosses a
// problem: its report and per-sample arrays do not depend on the batch it sits in.
// store_knots: the tile's states of a knot are staged in LDS ([lane][i], the layout of Xcl) and copied out by the whole
// workgroup, consecutive lanes to consecutive addresses (as verify.hip stages its dense samples).
// gusto_simulate_disturbed is the DIST = true instantiation of the same kernel: a lane carries the plant scalars its model
// reads (at most 4 doubles, for the whole roll-out) in a copy of the model parameters that f is evaluated with, and adds the
// noise of the interval to the commanded control -- u_dim integer hashes, or one load from the caller's [B][N-1][S][u_dim]
// array (a wave's samples of one interval are contiguous), formed ahead of the gain products: inside them the hash chains
// cost the 12/13-state kernels a resident workgroup (profiles/simulate_disturbed.txt).  DIST = false compiles to what it was:
// the same gfx950 instructions; what it needs extra is ONE unused local (a second one already moves its schedule).
#include <hip/hip_runtime.h>

#include "post.hpp"
#include "rollout.hpp"
#include "simrng.hpp"

using namespace gusto;

namespace {

constexpr int TILE = 256;          // samples per workgroup
constexpr int NO_SAMPLE = 1 << 30;

struct SimArgs {
    const double *X, *U, *K;       // [B][N][n], [B][N][m], [B][N-1][m][n]
    const double* pert;            // [B][S][n + m], or null: generated
    const int* active;             // gusto_set_active: null = every problem, else the mask [B]
    int S, tiles;
    unsigned long long seed, first_problem;
    double dx0[GUSTO_MAXN], du0[GUSTO_MAXM], u_lo[GUSTO_MAXM], u_hi[GUSTO_MAXM];
    double dt_min;
    int nstep, dense_collision;
    double *smin, *xfin, *dev;     // [B][S], [B][S][n], [B][S][n]
    int *sidx, *sflags;            // [B][S]
    double* knots;                 // [B][N][S][n] (store_knots)
    int *n_free, *n_finite, *n_clipped, *worst_sample, *worst_dense;   // [B]
    double *min_dist, *max_dev, *max_final_dev;                        // [B], [B][n], [B][n]
};

// gusto_simulate_disturbed: SimArgs and the two disturbances
struct SimArgsD : SimArgs {
    const double* plant_in;        // [B][S][GUSTO_NPLANT], or null: generated
    const double* white;           // [B][N-1][S][m], or null: generated
    double* plant;                 // [B][S][GUSTO_NPLANT]: the plant scalars used
    unsigned long long seed_plant, seed_white;   // (hashed on the host: simrng_plant_seed, simrng_white_seed)
    double plant_rel[GUSTO_NPLANT], dw[GUSTO_MAXM];
};

// what a lane of the DIST kernel carries besides the state: the model parameters with its own plant scalars (f reads at most
// four of them) and the noise of the current interval
template <int M> struct DistLane {
    gusto_model_params plant;
    double wk[M];
};

// The report of problem b from its per-sample arrays; every thread of the workgroup calls.  Thread t walks the samples
// t, t + blockDim, ... in ascending order, the partial results meet in block_reduce: minima, maxima and exact counts, so the
// split over the threads does not show in the result.  Non-finite samples enter the counts only.
template <int MODEL> GD void reduce_problem(const SimArgs& V, const double* Xend, int b, double* sred) {
    constexpr int n = MT<MODEL>::n;
    const int S = V.S, t = threadIdx.x, nt = blockDim.x;
    const size_t o = (size_t)b * S;
    double dmin = INFINITY, nfree = 0, nfin = 0, nclip = 0, dv[n], df[n];
    int smin = NO_SAMPLE;
#pragma unroll
    for (int i = 0; i < n; i++) { dv[i] = 0.0; df[i] = 0.0; }
    for (int s = t; s < S; s += nt) {
        const int fl = V.sflags[o + s];
        nclip += (fl >> 1) & 1;
        if (fl & 4) continue;
        nfin += 1;
        nfree += (fl & 1) ? 0 : 1;
        const double d = V.smin[o + s];
        if (d < dmin) { dmin = d; smin = s; }
#pragma unroll
        for (int i = 0; i < n; i++) {
            dv[i] = fmax(dv[i], V.dev[(o + s) * n + i]);
            df[i] = fmax(df[i], fabs(V.xfin[(o + s) * n + i] - Xend[i]));
        }
    }
    const double dall = block_reduce(dmin, OpMin(), sred);
    const int worst = (int)block_reduce((smin != NO_SAMPLE && dmin == dall) ? (double)smin : (double)NO_SAMPLE, OpMin(), sred);
    nfree = block_reduce(nfree, OpSum(), sred);
    nfin = block_reduce(nfin, OpSum(), sred);
    nclip = block_reduce(nclip, OpSum(), sred);
#pragma unroll
    for (int i = 0; i < n; i++) { dv[i] = block_reduce(dv[i], OpMax(), sred); df[i] = block_reduce(df[i], OpMax(), sred); }
    if (t == 0) {
        const bool none = worst == NO_SAMPLE;   // (no obstacles, or no finite sample: the distance is +inf)
        V.n_free[b] = (int)nfree; V.n_finite[b] = (int)nfin; V.n_clipped[b] = (int)nclip;
        V.min_dist[b] = dall;
        V.worst_sample[b] = none ? -1 : worst;
        V.worst_dense[b] = none ? -1 : V.sidx[o + worst];
#pragma unroll
        for (int i = 0; i < n; i++) { V.max_dev[(size_t)b * n + i] = dv[i]; V.max_final_dev[(size_t)b * n + i] = df[i]; }
    }
}

template <int MODEL, bool KNOTS, bool DIST>
__global__ void __launch_bounds__(TILE) simulate_kernel(const KParams P, const std::conditional_t<DIST, SimArgsD, SimArgs> V) {
    using T = MT<MODEL>;
    using D = Dyn<MODEL>;
    constexpr int n = T::n, m = T::m, nz = n + m;
    __shared__ double stage[KNOTS ? TILE * n : 1];   // KNOTS: [lane][i]
    __shared__ double sred[8];
    __shared__ double sK[m * n], sX[n], sU[m], sLo[m], sHi[m];   // knot k: K_k, X_k, U_k; the bounds
    const int b = blockIdx.x, s0 = blockIdx.y * TILE, t = threadIdx.x, N = P.N, S = V.S, nt = blockDim.x;
    if (V.active && !V.active[b]) return;   // (the whole workgroup: an inactive problem's results are left as they are)
    const int s = s0 + t;
    const bool valid = s < S;
    const double dt = P.tf[b] / (N - 1);
    const int nstep = rollout_nstep(dt, V.nstep, V.dt_min);
    const double h = dt / nstep;
    const double* X = V.X + (size_t)b * N * n;
    const double* U = V.U + (size_t)b * N * m;
    const double* K = V.K + (size_t)b * (N - 1) * m * n;
    const Env E = problem_env(P, b);
    const int cnt = min(TILE, S - s0) * n;   // doubles of one knot of this tile
    double* knots = KNOTS ? V.knots + ((size_t)b * N * S + s0) * n : nullptr;

    if (t < n) sX[t] = X[t];
    if (t < m) { sLo[t] = V.u_lo[t]; sHi[t] = V.u_hi[t]; }
    __syncthreads();
    // the perturbation: the start state and the offset of every control
    double x[n], pu[m], dev[n];
    {
        double p[nz];
#pragma unroll
        for (int i = 0; i < nz; i++) {
            if (V.pert) p[i] = valid ? V.pert[((size_t)b * S + s) * nz + i] : 0.0;
            else p[i] = simrng_pert(V.seed, V.first_problem + b, S, valid ? s : 0, nz, i, i < n ? V.dx0[i] : V.du0[i - n]);
        }
#pragma unroll
        for (int i = 0; i < n; i++) { x[i] = sX[i] + p[i]; dev[i] = 0.0; }
#pragma unroll
        for (int i = 0; i < m; i++) pu[i] = p[n + i];
    }
    // DIST: the plant of this lane.  All GUSTO_NPLANT scalars are formed and written out; those f reads stay in registers
    [[maybe_unused]] std::conditional_t<DIST, DistLane<m>, char> L;
    if constexpr (DIST) {
        const PlantNominal nominal(P.mp);
        double th[GUSTO_NPLANT];
#pragma unroll
        for (int j = 0; j < GUSTO_NPLANT; j++) {
            if (V.plant_in) th[j] = valid ? V.plant_in[((size_t)b * S + s) * GUSTO_NPLANT + j] : nominal.v[j];
            else th[j] = simrng_plant(V.seed_plant, V.first_problem + b, S, valid ? s : 0, GUSTO_NPLANT, j, nominal.v[j], V.plant_rel[j]);
            if (valid) V.plant[((size_t)b * S + s) * GUSTO_NPLANT + j] = th[j];
        }
        L.plant = P.mp;
        L.plant.mass = th[0]; L.plant.Jdiag[0] = th[1]; L.plant.Jdiag[1] = th[2]; L.plant.Jdiag[2] = th[3];
        L.plant.dubins_v = th[4]; L.plant.dubins_k = th[5];
    }
    bool alive = valid, fin = true, clipped = false;
#pragma unroll
    for (int i = 0; i < n; i++) fin = fin && fabs(x[i]) < INFINITY;
    alive = alive && fin;
    double dmin = INFINITY;
    int dj = -1;

    for (int k = 0; k < N - 1; k++) {   // knot k + 1 and the interval behind it
        double u[m];
        __syncthreads();   // (the readers of knot k are done)
        for (int e = t; e < m * n; e += nt) sK[e] = K[(size_t)k * m * n + e];
        if (t < n) sX[t] = X[k * n + t];
        if (t < m) sU[t] = U[k * m + t];
        __syncthreads();
        if constexpr (DIST) {   // the noise of this interval
#pragma unroll
            for (int c = 0; c < m; c++) {
                if (V.white) L.wk[c] = valid ? V.white[(((size_t)b * (N - 1) + k) * S + s) * m + c] : 0.0;
                else L.wk[c] = simrng_white(V.seed_white, V.first_problem + b, S, valid ? s : 0, N - 1, k, m, c, V.dw[c]);
            }
        }
        {
            double d[n];
#pragma unroll
            for (int i = 0; i < n; i++) {
                d[i] = x[i] - sX[i];
                if (alive) dev[i] = fmax(dev[i], fabs(d[i]));
            }
#pragma unroll
            for (int c = 0; c < m; c++) {
                double acc = 0.0;
#pragma unroll
                for (int j = 0; j < n; j++) acc += sK[c * n + j] * d[j];
                double v = (sU[c] - acc) + pu[c];
                if constexpr (DIST) v += L.wk[c];   // the noise of this interval, added last
                const double lo = sLo[c], hi = sHi[c];
                if (alive && (v < lo || v > hi)) clipped = true;
                u[c] = v < lo ? lo : (v > hi ? hi : v);
            }
        }
        if constexpr (KNOTS) {
#pragma unroll
            for (int i = 0; i < n; i++) stage[t * n + i] = x[i];
            __syncthreads();
            for (int e = t; e < cnt; e += nt) knots[(size_t)k * S * n + e] = stage[e];
            __syncthreads();
        }
        for (int q = 0; q < nstep; q++) {
            if (alive) {
                if constexpr (T::HAS_OBS) {
                    if (V.dense_collision || q == 0) {
                        const double dq = robot_min_distance<MODEL>(P, E, x);
                        if (dq < dmin) { dmin = dq; dj = k * nstep + q; }
                    }
                }
                fin = true;
                if constexpr (DIST) {
#define RK4_STEP_MP L.plant
#define RK4_STEP_NEW(i) fin = fin && fabs(x[i]) < INFINITY
#include "rk4_step.inc"
                } else {
#define RK4_STEP_MP P.mp
#define RK4_STEP_NEW(i) fin = fin && fabs(x[i]) < INFINITY
#include "rk4_step.inc"
                }
                alive = fin;
            }
        }
    }
    // knot N
    __syncthreads();
    if (t < n) sX[t] = X[(N - 1) * n + t];
    __syncthreads();
    if (alive) {
#pragma unroll
        for (int i = 0; i < n; i++) dev[i] = fmax(dev[i], fabs(x[i] - sX[i]));
        if constexpr (T::HAS_OBS) {
            const double dq = robot_min_distance<MODEL>(P, E, x);
            if (dq < dmin) { dmin = dq; dj = (N - 1) * nstep; }
        }
    }
    if constexpr (KNOTS) {
#pragma unroll
        for (int i = 0; i < n; i++) stage[t * n + i] = x[i];
        __syncthreads();
        for (int e = t; e < cnt; e += nt) knots[(size_t)(N - 1) * S * n + e] = stage[e];
    }
    if (valid) {
        const size_t o = (size_t)b * S + s;
        V.smin[o] = dmin;
        V.sidx[o] = dj;
        V.sflags[o] = (dmin < 0 ? 1 : 0) | (clipped ? 2 : 0) | (fin ? 0 : 4);
#pragma unroll
        for (int i = 0; i < n; i++) { V.xfin[o * n + i] = x[i]; V.dev[o * n + i] = dev[i]; }
    }
    if (V.tiles == 1) {   // (uniform) the workgroup holds every sample of the problem: it reads back what it has just written
        __syncthreads();
        reduce_problem<MODEL>(V, sX, b, sred);
    }
}

template <int MODEL> __global__ void __launch_bounds__(TILE) simulate_reduce(const KParams P, const SimArgs V) {
    constexpr int n = MT<MODEL>::n;
    __shared__ double sred[8];
    const int b = blockIdx.x;
    if (V.active && !V.active[b]) return;
    double xe[n];
#pragma unroll
    for (int i = 0; i < n; i++) xe[i] = V.X[((size_t)b * P.N + P.N - 1) * n + i];
    reduce_problem<MODEL>(V, xe, b, sred);
}

// W: null for gusto_simulate, else V with the disturbances (V is its base)
template <int MODEL> int launch_simulate(gusto_handle h, const KParams& P, const SimArgs& V, const SimArgsD* W, bool knots) {
    const int nt = 64 * ((std::min(V.S, TILE) + 63) / 64);
    const dim3 grid(h->B, V.tiles);
    if (W && knots) hipLaunchKernelGGL((simulate_kernel<MODEL, true, true>), grid, dim3(nt), 0, h->stream, P, *W);
    else if (W) hipLaunchKernelGGL((simulate_kernel<MODEL, false, true>), grid, dim3(nt), 0, h->stream, P, *W);
    else if (knots) hipLaunchKernelGGL((simulate_kernel<MODEL, true, false>), grid, dim3(nt), 0, h->stream, P, V);
    else hipLaunchKernelGGL((simulate_kernel<MODEL, false, false>), grid, dim3(nt), 0, h->stream, P, V);
    HIPCHK(h, hipGetLastError());
    if (V.tiles > 1) {
        hipLaunchKernelGGL((simulate_reduce<MODEL>), dim3(h->B), dim3(TILE), 0, h->stream, P, V);
        HIPCHK(h, hipGetLastError());
    }
    return GUSTO_OK;
}

// The arguments of gusto_simulate_disturbed that gusto_simulate does not have: GUSTO_ERR_ARG and the text, which names the
// offending problem, sample and entry (plant_entry_read: post.hpp).  No device
int disturb_args_host(gusto_handle h, const std::string& who, size_t B, size_t Ns, const gusto_disturb_opts& d, const double* plant,
                      const double* white) {
    const size_t N = h->N, m = h->m;
    for (int j = 0; j < GUSTO_NPLANT; j++)
        if (!(d.plant_rel[j] >= 0 && d.plant_rel[j] < 1)) return refuse(h, who, "plant_rel must lie in [0, 1) (entry " + std::to_string(j) + ")");
    for (size_t i = 0; i < m; i++)
        if (!(d.dw[i] >= 0 && d.dw[i] < INFINITY)) return refuse(h, who, "dw must be finite and >= 0 (entry " + std::to_string(i) + ")");
    for (size_t e = 0; plant && e < B * Ns * GUSTO_NPLANT; e++) {
        const int j = (int)(e % GUSTO_NPLANT);
        if (!plant_entry_read(h->model, j)) continue;
        const double v = plant[e];
        const bool ok = j < 4 ? (v > 0 && v < INFINITY) : fabs(v) < INFINITY;
        if (!ok)
            return refuse(h, who, std::string(j < 4 ? "plant: mass and Jdiag must be finite and > 0" : "plant: dubins_v and dubins_k must be finite") +
                                      " (problem " + std::to_string(e / GUSTO_NPLANT / Ns) + ", sample " + std::to_string(e / GUSTO_NPLANT % Ns) +
                                      ", entry " + std::to_string(j) + ")");
    }
    for (size_t e = 0; white && e < B * (N - 1) * Ns * m; e++)
        if (!(fabs(white[e]) < INFINITY))
            return refuse(h, who, "white must be finite (problem " + std::to_string(e / m / Ns / (N - 1)) + ", interval " +
                                      std::to_string(e / m / Ns % (N - 1) + 1) + ", sample " + std::to_string(e / m % Ns) + ", entry " +
                                      std::to_string(e % m) + ")");
    return GUSTO_OK;
}

// gusto_simulate (dist = null) and gusto_simulate_disturbed (dist: the options, never null; plant, white: the caller's or null)
int simulate_host(gusto_handle h, const char* who_c, const double* X, const double* U, const double* K, const double* pert,
                  const gusto_simulate_opts* opts, const gusto_disturb_opts* dist, const double* plant, const double* white);

}  // namespace

extern "C" {

int gusto_default_simulate_opts(int model_id, gusto_simulate_opts* o) {
    const ModelInfo* mi = model_info(model_id);
    if (!o || !mi) return GUSTO_ERR_ARG;
    memset(o, 0, sizeof(*o));
    o->n_samples = 64;
    for (int i = 0; i < mi->n; i++) o->dx0[i] = 0.01;   // (a placeholder: the caller knows the units of its states)
    for (int i = 0; i < GUSTO_MAXM; i++) { o->u_lo[i] = -INFINITY; o->u_hi[i] = INFINITY; }
    o->dt_min = 0.1; o->nstep = 0; o->nstep_cap = 64; o->dense_collision = 1; o->store_knots = 0;
    return GUSTO_OK;
}

int gusto_simulate(gusto_handle h, const double* X, const double* U, const double* K, const double* pert, const gusto_simulate_opts* opts) {
    return simulate_host(h, "gusto_simulate", X, U, K, pert, opts, nullptr, nullptr, nullptr);
}

int gusto_default_disturb_opts(gusto_disturb_opts* d) {
    if (!d) return GUSTO_ERR_ARG;
    memset(d, 0, sizeof(*d));
    return GUSTO_OK;
}

int gusto_simulate_disturbed(gusto_handle h, const double* X, const double* U, const double* K, const double* pert, const double* plant,
                             const double* white, const gusto_simulate_opts* opts, const gusto_disturb_opts* d) {
    gusto_disturb_opts zero;
    gusto_default_disturb_opts(&zero);
    return simulate_host(h, "gusto_simulate_disturbed", X, U, K, pert, opts, d ? d : &zero, plant, white);
}

}  // extern "C"

namespace {

int simulate_host(gusto_handle h, const char* who_c, const double* X, const double* U, const double* K, const double* pert,
                  const gusto_simulate_opts* opts, const gusto_disturb_opts* dist, const double* plant, const double* white) {
    if (int rc = post_enter(h, who_c, X, U)) return rc;
    const std::string who(who_c);
    gusto_simulate_opts o;
    gusto_default_simulate_opts(h->model, &o);
    if (opts) o = *opts;
    if (o.n_samples < 1 || o.n_samples > 4096) return refuse(h, who, "n_samples outside 1 .. 4096");
    if (!nstep_opts_ok(o.dt_min, o.nstep, o.nstep_cap) || (o.dense_collision != 0 && o.dense_collision != 1) ||
        (o.store_knots != 0 && o.store_knots != 1))
        return refuse(h, who, "bad options");
    for (int i = 0; i < h->n; i++)
        if (!(o.dx0[i] >= 0 && o.dx0[i] < INFINITY)) return refuse(h, who, "dx0 must be finite and >= 0 (entry " + std::to_string(i) + ")");
    for (int i = 0; i < h->m; i++) {
        if (!(o.du0[i] >= 0 && o.du0[i] < INFINITY)) return refuse(h, who, "du0 must be finite and >= 0 (entry " + std::to_string(i) + ")");
        if (!(o.u_lo[i] <= o.u_hi[i])) return refuse(h, who, "u_lo must not exceed u_hi (entry " + std::to_string(i) + ")");
    }
    if (dist)
        if (int rc = disturb_args_host(h, who, h->B, o.n_samples, *dist, plant, white)) return rc;
    SimulateState& S = h->simulate;
    if (!K && !h->tvlqr.have) {
        h->err = who + ": no gains: pass K or call gusto_tvlqr first";
        return GUSTO_ERR_STATE;
    }
    const size_t Bc = h->batch_cap, B = h->B, N = h->N, n = h->n, m = h->m, Ns = o.n_samples;
    KParams P = post_params(h);
    if (!fill_env(h, P, model_info(h->model)->has_obs, true)) {
        h->err = who + ": gusto_set_env_batch was called with a different number of problems than gusto_set_problems";
        return GUSTO_ERR_STATE;
    }
    int nstep_max = 0;   // (as gusto_verify; the largest count is of no use here)
    if (int rc = resolve_nstep(h, who_c, o.dt_min, o.nstep, o.nstep_cap, &nstep_max)) return rc;
    // grow-only; the layout depends on n_samples: results of another layout, or of other problems, are zeros before the launch
    HIPCHK(h, S.D.ensure(Bc * Ns)); HIPCHK(h, S.I.ensure(2 * Bc * Ns));
    HIPCHK(h, S.Xfin.ensure(Bc * Ns * n)); HIPCHK(h, S.Dev.ensure(Bc * Ns * n));
    HIPCHK(h, S.RI.ensure(5 * Bc)); HIPCHK(h, S.RD.ensure(Bc * (1 + 2 * n)));
    if (o.store_knots) HIPCHK(h, S.Knots.ensure(Bc * N * Ns * n));
    const bool fresh = !S.have || S.S != o.n_samples;
    if (fresh) {
        S.have = false; S.have_knots = false;
        HIPCHK(h, hipMemsetAsync(S.D, 0, sizeof(double) * Bc * Ns, h->stream));
        HIPCHK(h, hipMemsetAsync(S.I, 0, sizeof(int) * 2 * Bc * Ns, h->stream));
        HIPCHK(h, hipMemsetAsync(S.Xfin, 0, sizeof(double) * Bc * Ns * n, h->stream));
        HIPCHK(h, hipMemsetAsync(S.Dev, 0, sizeof(double) * Bc * Ns * n, h->stream));
        HIPCHK(h, hipMemsetAsync(S.RI, 0, sizeof(int) * 5 * Bc, h->stream));
        HIPCHK(h, hipMemsetAsync(S.RD, 0, sizeof(double) * Bc * (1 + 2 * n), h->stream));
    }
    if (o.store_knots && !S.have_knots) HIPCHK(h, hipMemsetAsync(S.Knots, 0, sizeof(double) * Bc * N * Ns * n, h->stream));
    if (dist) {   // (the plant scalars of a problem this call leaves out are those of the last disturbed call, or zeros)
        HIPCHK(h, S.Plant.ensure(Bc * Ns * GUSTO_NPLANT));
        if (fresh || !S.disturbed) HIPCHK(h, hipMemsetAsync(S.Plant, 0, sizeof(double) * Bc * Ns * GUSTO_NPLANT, h->stream));
    }
    SimArgsD V{};
    if (int rc = stage_traj(h, X, U, Bc, S.X, S.U, &V.X, &V.U)) return rc;
    V.K = h->tvlqr.K;
    if (K) {
        HIPCHK(h, S.K.ensure(Bc * (N - 1) * m * n));
        HIPCHK(h, hipMemcpyAsync(S.K, K, sizeof(double) * B * (N - 1) * m * n, hipMemcpyHostToDevice, h->stream));
        V.K = S.K;
    }
    if (pert) {
        HIPCHK(h, S.Pert.ensure(Bc * Ns * (n + m)));
        HIPCHK(h, hipMemcpyAsync(S.Pert, pert, sizeof(double) * B * Ns * (n + m), hipMemcpyHostToDevice, h->stream));
        V.pert = S.Pert;
    }
    V.active = active_mask(h);
    V.S = o.n_samples; V.tiles = (o.n_samples + TILE - 1) / TILE;
    V.seed = o.seed; V.first_problem = o.first_problem;
    memcpy(V.dx0, o.dx0, sizeof(V.dx0)); memcpy(V.du0, o.du0, sizeof(V.du0));
    memcpy(V.u_lo, o.u_lo, sizeof(V.u_lo)); memcpy(V.u_hi, o.u_hi, sizeof(V.u_hi));
    V.dt_min = o.dt_min; V.nstep = o.nstep; V.dense_collision = o.dense_collision;
    V.smin = S.D; V.xfin = S.Xfin; V.dev = S.Dev; V.sidx = S.I; V.sflags = S.I + Bc * Ns; V.knots = S.Knots;
    V.n_free = S.RI; V.n_finite = S.RI + Bc; V.n_clipped = S.RI + 2 * Bc; V.worst_sample = S.RI + 3 * Bc; V.worst_dense = S.RI + 4 * Bc;
    V.min_dist = S.RD; V.max_dev = S.RD + Bc; V.max_final_dev = S.RD + Bc + Bc * n;
    if (dist) {
        if (plant) {
            HIPCHK(h, S.PlantIn.ensure(Bc * Ns * GUSTO_NPLANT));
            HIPCHK(h, hipMemcpyAsync(S.PlantIn, plant, sizeof(double) * B * Ns * GUSTO_NPLANT, hipMemcpyHostToDevice, h->stream));
            V.plant_in = S.PlantIn;
        }
        if (white) {
            HIPCHK(h, S.White.ensure(Bc * (N - 1) * Ns * m));
            HIPCHK(h, hipMemcpyAsync(S.White, white, sizeof(double) * B * (N - 1) * Ns * m, hipMemcpyHostToDevice, h->stream));
            V.white = S.White;
        }
        V.plant = S.Plant;
        V.seed_plant = simrng_plant_seed(o.seed); V.seed_white = simrng_white_seed(o.seed);
        memcpy(V.plant_rel, dist->plant_rel, sizeof(V.plant_rel)); memcpy(V.dw, dist->dw, sizeof(V.dw));
    }
    HIPCHK(h, S.t0.record(h->stream));
    if (int rc = for_model(h->model, [&](auto M) { return launch_simulate<M()>(h, P, V, dist ? &V : nullptr, o.store_knots != 0); })) return rc;
    HIPCHK(h, S.t1.record(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, event_ms(S.t0, S.t1, &S.last_ms));
    S.have = true; S.S = o.n_samples;
    S.have_knots = o.store_knots != 0;
    S.disturbed = dist != nullptr;
    return GUSTO_OK;
}

}  // namespace

extern "C" {

int gusto_get_simulate(gusto_handle h, gusto_simulate_report* out) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    if (!out) return GUSTO_ERR_ARG;
    const SimulateState& S = h->simulate;
    if (!S.have) { h->err = "gusto_get_simulate: call gusto_simulate first"; return GUSTO_ERR_STATE; }
    const size_t B = h->B, Bc = h->batch_cap, n = h->n, Ns = S.S;
    if (int rc = copy_out(h, out->n_free, S.RI, B)) return rc;
    if (int rc = copy_out(h, out->n_finite, S.RI + Bc, B)) return rc;
    if (int rc = copy_out(h, out->n_clipped, S.RI + 2 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->worst_sample, S.RI + 3 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->worst_dense_sample, S.RI + 4 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->min_dist, S.RD, B)) return rc;
    if (int rc = copy_out(h, out->max_dev, S.RD + Bc, B * n)) return rc;
    if (int rc = copy_out(h, out->max_final_dev, S.RD + Bc + Bc * n, B * n)) return rc;
    if (int rc = copy_out(h, out->sample_min_dist, S.D, B * Ns)) return rc;
    if (int rc = copy_out(h, out->sample_dense_index, S.I, B * Ns)) return rc;
    if (int rc = copy_out(h, out->sample_flags, S.I + Bc * Ns, B * Ns)) return rc;
    return copy_out(h, out->x_final, S.Xfin, B * Ns * n);
}

int gusto_get_simulate_knots(gusto_handle h, double* Xcl) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    const SimulateState& S = h->simulate;
    if (!S.have_knots) { h->err = "gusto_get_simulate_knots: the last gusto_simulate did not run with store_knots = 1"; return GUSTO_ERR_STATE; }
    return copy_out(h, Xcl, S.Knots, (size_t)h->B * h->N * S.S * h->n);
}

int gusto_get_simulate_plant(gusto_handle h, double* plant) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    const SimulateState& S = h->simulate;
    if (!S.have || !S.disturbed) { h->err = "gusto_get_simulate_plant: the last roll-out was not a gusto_simulate_disturbed"; return GUSTO_ERR_STATE; }
    return copy_out(h, plant, S.Plant, (size_t)h->B * S.S * GUSTO_NPLANT);
}

int gusto_last_simulate_ms(gusto_handle h, double* ms) {
    if (!h || !ms) return GUSTO_ERR_ARG;
    if (!h->simulate.have) { h->err = "gusto_last_simulate_ms: call gusto_simulate first"; return GUSTO_ERR_STATE; }
    *ms = h->simulate.last_ms;
    return GUSTO_OK;
}

}  // extern "C"
