// verify.hip -- batched post-solve verification: interpolate_traj, dynamics_constraint_satisfaction and
// verify_collision_free of the two Astrobee model files, for every problem of a batch and every model of the library.
//   interpolate_traj                   src/dynamics/astrobee_se3_manifold.jl:1011-1042, astrobee_se3.jl:495-527
//   dynamics_constraint_satisfaction   astrobee_se3_manifold.jl:1044-1055, astrobee_se3.jl:529-540
//   verify_collision_free              astrobee_se3_manifold.jl:1057-1077, astrobee_se3.jl:542-560
// One WORKGROUP per problem, 64 ceil(N / 64) lanes, lane k = knot k and the interval k -> k + 1.  A lane evaluates the signed
// distances of its knot, the forward-Euler defect of its interval and rolls its interval out: Nstep = ceil(dt / dt_min)
// classical RK4 steps of dt / Nstep from X[:,k] under the held control U[:,k] (every interval restarts from its knot, as the
// reference does).  The per-problem numbers are reductions over the lanes -- DPP / v_readlane inside a wave, LDS across the
// waves (common.hpp: block_reduce) -- in a fixed order and without atomics: a problem's report is the same bit for bit
// whatever batch it sits in.  Dynamics: Dyn<MODEL>::f; distances: signed_distance<WS> at the workspace location the solver
// uses (the first WS states plus the component offset, every component of mp.n_robot_comp), obstacle tables read through
// the constant address space with a wave-uniform index (models.hpp), shared (gusto_set_env) or per problem
// (gusto_set_env_batch).
// verify_collision_free looks at the KNOTS only and returns the first hit of its loop nest, obstacle-major: a lane keeps the
// first (component, obstacle) pair that penetrates at its knot, the key (component n_obs + obstacle) N + knot orders the
// hits of all lanes as the reference's loops would meet them (components outermost, as in trust_region_ratio_gusto; the
// reference's function has rb_idx = 1 only).  What the reference lacks -- the smallest distance over ALL dense samples, the
// sample it occurs at and the gap between the end of a rolled-out interval and the next knot (the value its
// `Xfull[:,istart] = X[:,k]` overwrites) -- is reported next to it.
// Stores of the dense trajectory: lane k owns the Nstep n consecutive doubles of its interval, Nstep n doubles away from its
// neighbour's -- a cache line per lane per store if written directly.  The samples of DENSE_TILE substeps are staged in LDS
// ([lane][substep][i]) and copied out by the whole workgroup, consecutive threads to consecutive addresses inside each
// lane's DENSE_TILE n doubles; the held controls are copied straight from U (thread e writes double e of the problem).
#include <hip/hip_runtime.h>

#include "post.hpp"
#include "rollout.hpp"

using namespace gusto;

namespace {

constexpr int DENSE_TILE = 4;      // substeps staged in LDS per copy-out: 4 n doubles per lane (26.6 KB for N <= 64, n = 13)
// (NO_HIT, rollout.hpp: the keys below stay under 2 * 64 * 256)

struct VerifyArgs {
    const double *X, *U;           // [B][N][n], [B][N][m]: the handle's trajectories or the caller's copies
    const int* active;             // gusto_set_active: null = every problem, else the mask [B]
    double dt_min;
    int nstep, dense_collision;
    int nfull_max;                 // rows per problem of Xfull (dense output only)
    int *collision_free, *first_knot, *min_dense_sample, *nfull;
    double *first_dist, *min_dist_knots, *dyn_defect_l1, *min_dist_dense, *max_gap;
    double *Xfull, *Ufull;         // [B][nfull_max][n], [B][nfull_max - 1][m]
};

template <int MODEL, bool DENSE> __global__ void __launch_bounds__(256) verify_kernel(const KParams P, const VerifyArgs V) {
    using T = MT<MODEL>;
    constexpr int n = T::n, m = T::m;
    extern __shared__ double stage[];   // DENSE: [lanes][DENSE_TILE][n]
    __shared__ double sred[8];
    const int b = blockIdx.x, k = threadIdx.x, N = P.N, nt = blockDim.x;
    if (V.active && !V.active[b]) return;   // (the whole workgroup: an inactive problem's report is left as it is)
    const double dt = P.tf[b] / (N - 1);
    const int nstep = rollout_nstep(dt, V.nstep, V.dt_min);
    const int nfull = nstep * (N - 1) + 1;
    if (DENSE && nfull > V.nfull_max) return;
    const double h = dt / nstep;
    const double* X = V.X + (size_t)b * N * n;
    const double* U = V.U + (size_t)b * N * m;
    const bool knot = k < N, ival = k < N - 1;
    double x[n], xn[n], u[m];
#pragma unroll
    for (int i = 0; i < n; i++) { x[i] = knot ? X[k * n + i] : 0.0; xn[i] = ival ? X[(k + 1) * n + i] : 0.0; }
#pragma unroll
    for (int i = 0; i < m; i++) u[i] = knot ? U[k * m + i] : 0.0;
    const Env E = problem_env(P, b);

    // verify_collision_free: the knots
    double dk = INFINITY, hit_d = 0.0;
    int hit = NO_HIT;
    if constexpr (T::HAS_OBS) {
        if (knot) {
            dk = robot_min_distance<MODEL, true>(P, E, x, &hit, &hit_d);
            if (hit != NO_HIT) hit = hit * N + k;
        }
    }
    // dynamics_constraint_satisfaction: the forward-Euler defect of the interval
    double defect = 0.0;
    if (ival) {
        double f[n];
        Dyn<MODEL>::f(P.mp, x, u, f);
#pragma unroll
        for (int i = 0; i < n; i++) defect += fabs((xn[i] - x[i]) / dt - f[i]);
    }
    // interpolate_traj: the interval from its knot, zero-order hold of u
    double dd = INFINITY, gap = 0.0;
    int di = -1;
    double* Xf = DENSE ? V.Xfull + (size_t)b * V.nfull_max * n : nullptr;
    for (int s0 = 0; s0 < nstep; s0 += DENSE_TILE) {
        const int cnt = min(DENSE_TILE, nstep - s0);
        for (int s = s0; s < s0 + cnt; s++) {
            const bool samp = ival || (k == N - 1 && s == 0);   // (the last dense sample is the last knot)
            if constexpr (T::HAS_OBS) {
                if (samp && V.dense_collision) {
                    const double d = robot_min_distance<MODEL, true>(P, E, x, nullptr, nullptr);   // (rollout.hpp: why HIT)
                    if (d < dd) { dd = d; di = k * nstep + s; }
                }
            }
            if constexpr (DENSE) {
                if (samp)
#pragma unroll
                    for (int i = 0; i < n; i++) stage[(k * DENSE_TILE + (s - s0)) * n + i] = x[i];
            }
            if (ival) rk4_step<MODEL>(P.mp, x, u, h);
        }
        if constexpr (DENSE) {
            __syncthreads();
            for (int e = k; e < nt * DENSE_TILE * n; e += nt) {
                const int kk = e / (DENSE_TILE * n), r = e % (DENSE_TILE * n);
                const int rows = kk < N - 1 ? cnt : ((kk == N - 1 && s0 == 0) ? 1 : 0);
                if (r / n < rows) Xf[((size_t)kk * nstep + s0) * n + r] = stage[e];
            }
            __syncthreads();
        }
    }
    if (ival) {
#pragma unroll
        for (int i = 0; i < n; i++) gap = nanmax(gap, fabs(x[i] - xn[i]));
    }
    if constexpr (DENSE) {   // held controls, and zeros behind the problem's own samples
        double* Uf = V.Ufull + (size_t)b * (V.nfull_max - 1) * m;
        for (int e = k; e < (nfull - 1) * m; e += nt) Uf[e] = U[(e / m / nstep) * m + e % m];
        for (int e = (nfull - 1) * m + k; e < (V.nfull_max - 1) * m; e += nt) Uf[e] = 0.0;
        for (int e = nfull * n + k; e < V.nfull_max * n; e += nt) Xf[e] = 0.0;
    }

    const double dk_all = block_reduce(dk, OpMin(), sred);
    const int first = (int)block_reduce((double)hit, OpMin(), sred);
    const double def_all = block_reduce(defect, OpSum(), sred);
    const double dd_all = block_reduce(dd, OpMin(), sred);
    const int di_all = (int)block_reduce((di >= 0 && dd == dd_all) ? (double)di : (double)NO_HIT, OpMin(), sred);
    const double gap_all = block_reduce(gap, OpNanMax(), sred);
    if (first != NO_HIT && hit == first) V.first_dist[b] = hit_d;   // (one lane: keys are distinct)
    if (k == 0) {
        V.collision_free[b] = first == NO_HIT;
        V.first_knot[b] = first == NO_HIT ? 0 : first % N + 1;
        if (first == NO_HIT) V.first_dist[b] = 0.0;
        V.min_dist_knots[b] = dk_all;
        V.dyn_defect_l1[b] = def_all;
        V.min_dist_dense[b] = dd_all;
        V.min_dense_sample[b] = di_all == NO_HIT ? -1 : di_all;
        V.max_gap[b] = gap_all;
        if (DENSE) V.nfull[b] = nfull;
    }
}

template <int MODEL> int launch_verify(gusto_handle h, const KParams& P, const VerifyArgs& V, bool dense) {
    const int nt = 64 * ((h->N + 63) / 64);
    if (dense) {
        const size_t lds = sizeof(double) * nt * DENSE_TILE * MT<MODEL>::n;
        auto kern = &verify_kernel<MODEL, true>;
        HIPCHK(h, hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(h->B), dim3(nt), lds, h->stream, P, V);
    } else {
        hipLaunchKernelGGL((verify_kernel<MODEL, false>), dim3(h->B), dim3(nt), 0, h->stream, P, V);
    }
    HIPCHK(h, hipGetLastError());
    return GUSTO_OK;
}

int verify_impl(gusto_handle h, const double* X, const double* U, const gusto_verify_opts* opts, bool dense, int* nfull_max, const char* who) {
    if (int rc = post_enter(h, who, X, U)) return rc;
    gusto_verify_opts o;
    gusto_default_verify_opts(&o);
    if (opts) o = *opts;
    if (!nstep_opts_ok(o.dt_min, o.nstep, o.nstep_cap) || (o.dense_collision != 0 && o.dense_collision != 1)) {
        h->err = std::string(who) + ": bad options";
        return GUSTO_ERR_ARG;
    }
    VerifyState& S = h->verify;
    const size_t Bc = h->batch_cap, N = h->N, n = h->n, m = h->m;
    KParams P = post_params(h);
    if (!fill_env(h, P, model_info(h->model)->has_obs, true)) {
        h->err = std::string(who) + ": gusto_set_env_batch was called with a different number of problems than gusto_set_problems";
        return GUSTO_ERR_STATE;
    }
    int nstep_max = 0;
    if (int rc = resolve_nstep(h, who, o.dt_min, o.nstep, o.nstep_cap, &nstep_max)) return rc;
    // (the report is zeroed once)
    HIPCHK(h, S.I.ensure_zeroed(4 * Bc, h->stream)); HIPCHK(h, S.D.ensure_zeroed(5 * Bc, h->stream));
    VerifyArgs V{};
    if (int rc = stage_traj(h, X, U, Bc, S.X, S.U, &V.X, &V.U)) return rc;
    V.active = active_mask(h);
    V.dt_min = o.dt_min; V.nstep = o.nstep; V.dense_collision = o.dense_collision;
    V.collision_free = S.I; V.first_knot = S.I + Bc; V.min_dense_sample = S.I + 2 * Bc; V.nfull = S.I + 3 * Bc;
    V.first_dist = S.D; V.min_dist_knots = S.D + Bc; V.dyn_defect_l1 = S.D + 2 * Bc; V.min_dist_dense = S.D + 3 * Bc;
    V.max_gap = S.D + 4 * Bc;
    if (dense) {
        const int nf = nstep_max * (int)(N - 1) + 1;
        if (nf != S.dense_rows) {   // another layout: a new buffer, zeros everywhere
            S.Xf.reset(); S.Uf.reset();
            S.dense_rows = 0; S.have_dense = false;
            HIPCHK(h, S.Xf.ensure_zeroed(Bc * nf * n, h->stream)); HIPCHK(h, S.Uf.ensure_zeroed(Bc * (nf - 1) * m, h->stream));
            HIPCHK(h, hipMemsetAsync(V.nfull, 0, sizeof(int) * Bc, h->stream));
            S.dense_rows = nf;
        }
        V.nfull_max = nf; V.Xfull = S.Xf; V.Ufull = S.Uf;
    }
    HIPCHK(h, S.t0.record(h->stream));
    if (int rc = for_model(h->model, [&](auto M) { return launch_verify<M()>(h, P, V, dense); })) return rc;
    HIPCHK(h, S.t1.record(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, event_ms(S.t0, S.t1, &S.last_ms));
    S.have = true;
    if (dense) { S.have_dense = true; if (nfull_max) *nfull_max = V.nfull_max; }
    return GUSTO_OK;
}

}  // namespace

extern "C" {

int gusto_default_verify_opts(gusto_verify_opts* o) {
    if (!o) return GUSTO_ERR_ARG;
    o->dt_min = 0.1;           // interpolate_traj(traj, SCPP, dt_min=0.1)
    o->nstep = 0; o->nstep_cap = 64; o->dense_collision = 1;
    return GUSTO_OK;
}

int gusto_verify(gusto_handle h, const double* X, const double* U, const gusto_verify_opts* o) {
    return verify_impl(h, X, U, o, false, nullptr, "gusto_verify");
}

int gusto_interpolate(gusto_handle h, const double* X, const double* U, const gusto_verify_opts* o, int* nfull_max) {
    return verify_impl(h, X, U, o, true, nfull_max, "gusto_interpolate");
}

int gusto_get_verify(gusto_handle h, gusto_verify_report* out) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    if (!out) return GUSTO_ERR_ARG;
    const VerifyState& S = h->verify;
    if (!S.have) { h->err = "gusto_get_verify: call gusto_verify first"; return GUSTO_ERR_STATE; }
    const size_t B = h->B, Bc = h->batch_cap;
    if (int rc = copy_out(h, out->collision_free, S.I, B)) return rc;
    if (int rc = copy_out(h, out->first_knot, S.I + Bc, B)) return rc;
    if (int rc = copy_out(h, out->min_dense_sample, S.I + 2 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->first_dist, S.D, B)) return rc;
    if (int rc = copy_out(h, out->min_dist_knots, S.D + Bc, B)) return rc;
    if (int rc = copy_out(h, out->dyn_defect_l1, S.D + 2 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->min_dist_dense, S.D + 3 * Bc, B)) return rc;
    return copy_out(h, out->max_gap, S.D + 4 * Bc, B);
}

int gusto_get_dense(gusto_handle h, int* nfull, double* Xfull, double* Ufull) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    const VerifyState& S = h->verify;
    if (!S.have_dense) { h->err = "gusto_get_dense: call gusto_interpolate first"; return GUSTO_ERR_STATE; }
    const size_t B = h->B, nf = S.dense_rows;
    if (int rc = copy_out(h, nfull, S.I + 3 * h->batch_cap, B)) return rc;
    if (int rc = copy_out(h, Xfull, S.Xf, B * nf * h->n)) return rc;
    return copy_out(h, Ufull, S.Uf, B * (nf - 1) * h->m);
}

int gusto_last_verify_ms(gusto_handle h, double* ms) {
    if (!h || !ms) return GUSTO_ERR_ARG;
    if (!h->verify.have) { h->err = "gusto_last_verify_ms: call gusto_verify first"; return GUSTO_ERR_STATE; }
    *ms = h->verify.last_ms;
    return GUSTO_OK;
}

}  // extern "C"
