// fleet.hip -- fleet coordination: robot-to-robot separation and departure delays.  Every other stage treats a problem as if it
// were alone in the workspace; here R consecutive problems are the robots of one fleet (the multi-start layout with K = R) and are
// held against each other: prioritised planning on fixed paths.  The stage runs around gusto_solve and reads what
// gusto_interpolate left on the device; no solve kernel knows of it.  The definitions are stated in include/gusto_hip.h.
//   gusto_fleet_schedule     tracks, the departure delays, and the separation report of the shifts it chose
//   gusto_fleet_separation   tracks and the separation report of the last schedule's shifts or of a caller's
//   gusto_get_fleet / gusto_get_fleet_tracks / gusto_last_fleet_ms
// Track kernel: one workgroup per robot, thread t takes the clock samples t, t + 256, ...: consecutive threads write consecutive
// samples of Q [B][Jmax][WS].  A thread keeps the bounding box and the finiteness of its samples; WS + WS + 1 block reductions
// end the kernel.  Every operation of a sample is rounded on its own (contraction off), so numpy reproduces the track bit for bit.
// Schedule kernel: one workgroup of four waves per fleet, robots placed in sequence.  Lane = clock sample: both tracks are read
// with consecutive addresses, a shift is an integer offset, nothing is interpolated.  Candidates are tried in ascending order;
// the waves take the robots placed so far round-robin, each in placement order, a wave stops at the first step that refutes
// (one wave-uniform __ballot per 64 steps) and at the first robot that does; the waves meet through LDS, where the lowest
// refuting placement is the `blocker` of candidate 0.  Work stops at the first feasible candidate.  A placed robot whose track's
// bounding box lies further from the candidate's than thr plus the largest component offset cannot refute and is skipped
// (gusto_fleet_opts.prune; the bound is taken with a relative slack of 1e-9, far above the roundings of d2).
// Separation kernel: one workgroup per fleet, waves take the pairs a < b round-robin, lanes the clock samples; a lane keeps its
// smallest D2 and the first step it saw it at (strict <), then the two-reduction argmin of multistart.hip / tighten.hip:
// the minimum, then the lowest step among the ties.  The per-robot and per-fleet rows come from the pair table in index order.
// The other mapping (lane = candidate, tracks tiled through LDS) has not been built: profiles/fleet.txt says why this one ships.
// No atomics, nothing crosses a fleet: a fleet's outputs are the same bit for bit in any batch.
#include <hip/hip_runtime.h>

#include "fleet.hpp"
#include "seed.hpp"

using namespace gusto;

namespace {

constexpr int FI_STATUS = 0, FI_SIGMA = 1, FI_BLOCKER = 2, FI_PARTNER = 3, FI_STEP = 4, FI_NB = 5;   // rows [B] of FleetState::I
constexpr int FF_NSCHED = 0, FF_NBLOCKED = 1, FF_NCONF = 2, FF_MAKESPAN = 3, FF_NF = 4;              // rows [F] behind pair_step [B][R]
constexpr int FD_DELAY = 0, FD_MINSEP = 1, FD_NB = 2;                                                // rows [B] of FleetState::D
constexpr int SC_STATUS = 0, SC_SIGMA = 1, SC_BLOCKER = 2, SC_NB = 3;                                // rows [B] of FleetState::Sch
constexpr int FLEET_WAVES = 4, FLEET_THREADS = 64 * FLEET_WAVES, TRACK_THREADS = 256;
constexpr int NONE_PLACED = 0x7fffffff;

// what the kernels know of the robot and the options
struct FleetGeom {
    double h, thr2, two_r, far;     // clock step, (2 radius + margin)^2, 2 radius, the pruning distance (< 0: no pruning)
    double doff[4][3];              // comp_off[ca] - comp_off[cb] of the component pairs, ca outer and cb inner
    int npair, n_delays, stride;
};

struct TrackArgs {
    const double *Xf, *tf;          // the dense samples [batch_cap][nf_rows][n], tf [B]
    const int* nfull;               // [B]
    double *Q, *Box;
    int *J, *Fin;
    double h;
    int nf_rows, n, Jmax;
};

template <int WS> __global__ void __launch_bounds__(TRACK_THREADS) track_kernel(const TrackArgs A) {
    __shared__ double sred[TRACK_THREADS / 64];
    const int b = blockIdx.x, t = threadIdx.x;
    const int nf = min(A.nfull[b], A.nf_rows);
    const double tf = A.tf[b];
    const int J = (int)ceil(tf / A.h) + 1;   // (2 .. clock_cap: fleet_args_host)
    const double* P = A.Xf + (size_t)b * A.nf_rows * A.n;
    double lo[WS], hi[WS], fin = 1.0;
#pragma unroll
    for (int x = 0; x < WS; x++) { lo[x] = INFINITY; hi[x] = -INFINITY; }
    for (int j = t; j < A.Jmax; j += TRACK_THREADS) {
        double q[WS];
        if (j >= J) {
#pragma unroll
            for (int x = 0; x < WS; x++) q[x] = 0.0;
        } else if (nf < 2) {
#pragma unroll
            for (int x = 0; x < WS; x++) q[x] = NAN;
        } else if (j == J - 1) {
#pragma unroll
            for (int x = 0; x < WS; x++) q[x] = P[(size_t)(nf - 1) * A.n + x];
        } else {
#pragma clang fp contract(off)
            const double hb = tf / (double)(nf - 1);
            const double tau = (double)j * A.h;
            const double s = tau / hb;
            const int i = min((int)floor(s), nf - 2);
            const double w = s - (double)i;
            const double w1 = 1.0 - w;
#pragma unroll
            for (int x = 0; x < WS; x++) {
                const double a = w1 * P[(size_t)i * A.n + x];
                const double c = w * P[(size_t)(i + 1) * A.n + x];
                q[x] = a + c;
            }
        }
#pragma unroll
        for (int x = 0; x < WS; x++) {
            A.Q[((size_t)b * A.Jmax + j) * WS + x] = q[x];
            if (j < J) {
                lo[x] = fmin(lo[x], q[x]); hi[x] = fmax(hi[x], q[x]);
                if (!(fabs(q[x]) < INFINITY)) fin = 0.0;
            }
        }
    }
#pragma unroll
    for (int x = 0; x < WS; x++) {
        lo[x] = block_reduce(lo[x], OpMin(), sred);
        hi[x] = block_reduce(hi[x], OpMax(), sred);
    }
    fin = block_reduce(fin, OpMin(), sred);
    if (t == 0) {
#pragma unroll
        for (int x = 0; x < WS; x++) { A.Box[(size_t)b * 2 * WS + x] = lo[x]; A.Box[(size_t)b * 2 * WS + WS + x] = hi[x]; }
        A.J[b] = J;
        A.Fin[b] = fin != 0.0;
    }
}

// D2 of two positions: the smallest squared centre distance over the component pairs, fmin from +inf
template <int WS> GD double pair_d2(const double* pa, const double* pb, const FleetGeom& G) {
#pragma clang fp contract(off)
    double best = INFINITY;
    for (int c = 0; c < G.npair; c++) {
        double d2 = 0.0;
#pragma unroll
        for (int x = 0; x < WS; x++) {
            const double dp = pa[x] - pb[x];
            const double dx = dp + G.doff[c][x];
            const double sq = dx * dx;
            d2 = d2 + sq;
        }
        best = fmin(best, d2);
    }
    return best;
}
// p_b(j; sigma) of the track Q with J samples
template <int WS> GD const double* position(const double* Q, int J, int sigma, int j) {
    const int i = sigma < 0 ? 0 : min(max(j - sigma, 0), J - 1);
    return Q + (size_t)i * WS;
}
GD int end_step(int sigma, int J) { return sigma < 0 ? 0 : sigma + J - 1; }
// the boxes of two tracks lie further apart along some axis than `far`
template <int WS> GD bool boxes_apart(const double* Ba, const double* Bb, double far) {
    bool apart = false;
#pragma unroll
    for (int x = 0; x < WS; x++) apart = apart || Ba[x] - Bb[WS + x] > far || Bb[x] - Ba[WS + x] > far;
    return apart;
}

struct FleetArgs {
    FleetGeom G;
    const double *Q, *Box;
    const int *J, *Fin;
    const int *ord, *elig, *st_i;   // a caller's order and eligibility (null: index order, the status words)
    const int* sig;                 // a caller's shifts (null: the schedule's)
    int* Sch;                       // the schedule's rows [SC_NB][B]
    int* I;
    double* D;
    int B, R, Jmax;
};

template <int WS> __global__ void __launch_bounds__(FLEET_THREADS) schedule_kernel(const FleetArgs A) {
    __shared__ int s_sig[GUSTO_MAX_STARTS], s_rob[GUSTO_MAX_STARTS], s_first[FLEET_WAVES];
    const FleetGeom& G = A.G;
    const int f = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63, R = A.R, base = f * R;
    for (int p = 0; p < R; p++) {
        const int i = A.ord ? A.ord[base + p] : p, bi = base + i;
        const bool ok = (A.elig ? A.elig[bi] != 0 : (A.st_i[(size_t)bi * ST_NI + ST_CONV] != 0 && A.st_i[(size_t)bi * ST_NI + ST_SUCC] != 0)) &&
                        A.Fin[bi] != 0;
        const double* Qi = A.Q + (size_t)bi * A.Jmax * WS;
        const int Ji = A.J[bi];
        int chosen = -1, blocker = -1;
        for (int d = 0; ok && d < G.n_delays && chosen < 0; d++) {   // (ok, d, chosen: the same in every thread)
            const int sg = d * G.stride;
            int first = NONE_PLACED;
            for (int q = w; q < p && first == NONE_PLACED; q += FLEET_WAVES) {
                const int bk = base + s_rob[q], sk = s_sig[q], Jk = A.J[bk];
                if (G.far >= 0 && boxes_apart<WS>(A.Box + (size_t)bi * 2 * WS, A.Box + (size_t)bk * 2 * WS, G.far)) continue;
                const double* Qk = A.Q + (size_t)bk * A.Jmax * WS;
                const int jend = max(end_step(sg, Ji), end_step(sk, Jk));
                for (int j0 = 0; j0 <= jend; j0 += 64) {
                    const int j = j0 + lane;
                    const bool hit = j <= jend && pair_d2<WS>(position<WS>(Qi, Ji, sg, j), position<WS>(Qk, Jk, sk, j), G) < G.thr2;
                    if (__ballot(hit)) { first = q; break; }
                }
            }
            if (lane == 0) s_first[w] = first;
            __syncthreads();
            int m = s_first[0];
#pragma unroll
            for (int v = 1; v < FLEET_WAVES; v++) m = min(m, s_first[v]);
            __syncthreads();
            if (d == 0 && m != NONE_PLACED) blocker = s_rob[m];
            if (m == NONE_PLACED) chosen = d;
        }
        if (t == 0) {
            const int sigma = chosen < 0 ? -1 : chosen * G.stride;
            A.Sch[SC_STATUS * A.B + bi] = !ok ? GUSTO_FLEET_NO_PLAN : (chosen < 0 ? GUSTO_FLEET_BLOCKED : GUSTO_FLEET_SCHEDULED);
            A.Sch[SC_SIGMA * A.B + bi] = sigma;
            A.Sch[SC_BLOCKER * A.B + bi] = blocker;
            s_sig[p] = sigma; s_rob[p] = i;
        }
        __syncthreads();
    }
}

template <int WS> __global__ void __launch_bounds__(FLEET_THREADS) separation_kernel(const FleetArgs A) {
    __shared__ int s_sig[GUSTO_MAX_STARTS], s_st[GUSTO_MAX_STARTS], s_conf[FLEET_WAVES];
    const FleetGeom& G = A.G;
    const int f = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63, R = A.R, base = f * R, B = A.B;
    double* pair_sep = A.D + (size_t)FD_NB * B + (size_t)base * R;
    int* pair_step = A.I + (size_t)FI_NB * B + (size_t)base * R;
    // the shifts of the report: the schedule's rows, or a caller's
    if (t < R) {
        const int b = base + t;
        const int sigma = A.sig ? A.sig[b] : A.Sch[SC_SIGMA * B + b];
        const int st = A.sig ? (sigma >= 0 ? GUSTO_FLEET_SCHEDULED : GUSTO_FLEET_NO_PLAN) : A.Sch[SC_STATUS * B + b];
        s_sig[t] = sigma; s_st[t] = st;
        A.I[FI_STATUS * B + b] = st;
        A.I[FI_SIGMA * B + b] = sigma;
        A.I[FI_BLOCKER * B + b] = A.sig ? -1 : A.Sch[SC_BLOCKER * B + b];
        A.D[FD_DELAY * B + b] = sigma < 0 ? 0.0 : (double)sigma * G.h;
        pair_sep[t * R + t] = INFINITY; pair_step[t * R + t] = -1;
    }
    __syncthreads();
    int n_conf = 0, idx = 0;
    for (int a = 0; a < R; a++)
        for (int b = a + 1; b < R; b++, idx++) {
            if (idx % FLEET_WAVES != w) continue;
            const int ba = base + a, bb = base + b, Ja = A.J[ba], Jb = A.J[bb], sa = s_sig[a], sb = s_sig[b];
            const double *Qa = A.Q + (size_t)ba * A.Jmax * WS, *Qb = A.Q + (size_t)bb * A.Jmax * WS;
            const int jend = max(end_step(sa, Ja), end_step(sb, Jb));
            double best = INFINITY;
            int bj = -1;
            for (int j = lane; j <= jend; j += 64) {
                const double d2 = pair_d2<WS>(position<WS>(Qa, Ja, sa, j), position<WS>(Qb, Jb, sb, j), G);
                if (d2 < best) { best = d2; bj = j; }
            }
            const double dmin = wave_reduce(best, OpMin());
            const double jmin = wave_reduce((best == dmin && bj >= 0) ? (double)bj : INFINITY, OpMin());   // (steps: exact in a double)
            n_conf += dmin < G.thr2;
            if (lane == 0) {
                const double sep = sqrt(dmin) - G.two_r;
                const int step = jmin < INFINITY ? (int)jmin : -1;
                pair_sep[a * R + b] = sep; pair_sep[b * R + a] = sep;
                pair_step[a * R + b] = step; pair_step[b * R + a] = step;
            }
        }
    if (lane == 0) s_conf[w] = n_conf;
    __syncthreads();   // (the pair table: written and read by this workgroup only)
    if (t < R) {
        double best = INFINITY;
        int partner = -1;
        for (int b = 0; b < R; b++) {
            const double s = pair_sep[t * R + b];
            if (s < best) { best = s; partner = b; }
        }
        A.D[FD_MINSEP * B + base + t] = best;
        A.I[FI_PARTNER * B + base + t] = partner;
        A.I[FI_STEP * B + base + t] = partner < 0 ? -1 : pair_step[t * R + partner];
    }
    if (t == 0) {
        double best = INFINITY;
        int n_s = 0, n_b = 0, span = 0, conf = 0;
        for (int a = 0; a < R; a++) {
            for (int b = a + 1; b < R; b++) best = fmin(best, pair_sep[a * R + b]);
            n_s += s_st[a] == GUSTO_FLEET_SCHEDULED; n_b += s_st[a] == GUSTO_FLEET_BLOCKED;
            if (s_st[a] == GUSTO_FLEET_SCHEDULED) span = max(span, end_step(s_sig[a], A.J[base + a]));
        }
        for (int v = 0; v < FLEET_WAVES; v++) conf += s_conf[v];
        const int F = B / R;
        int* If = A.I + (size_t)FI_NB * B + (size_t)B * R;
        If[FF_NSCHED * F + f] = n_s; If[FF_NBLOCKED * F + f] = n_b; If[FF_NCONF * F + f] = conf; If[FF_MAKESPAN * F + f] = span;
        A.D[(size_t)FD_NB * B + (size_t)B * R + f] = best;
    }
}

// the robot and the options as the kernels read them
FleetGeom fleet_geom(const gusto_model_params& mp, const gusto_fleet_opts& o, int ws) {
    FleetGeom G;
    memset(&G, 0, sizeof(G));
    const double thr = 2 * mp.radius + o.margin;
    G.h = o.dt_clock; G.thr2 = thr * thr; G.two_r = 2 * mp.radius;
    G.n_delays = o.n_delays; G.stride = o.delay_stride;
    const int nc = o.components ? std::max(1, std::min(mp.n_robot_comp, 2)) : 1;
    double omax = 0.0;
    for (int ca = 0; ca < nc; ca++)
        for (int cb = 0; cb < nc; cb++, G.npair++)
            for (int x = 0; x < ws; x++) {
                G.doff[G.npair][x] = mp.comp_off[ca][x] - mp.comp_off[cb][x];
                omax = std::max(omax, fabs(G.doff[G.npair][x]));   // (an axis gap g leaves |delta_x| >= g - |doff_x|)
            }
    G.far = o.prune ? (thr + omax) * (1 + 1e-9) : -1.0;
    return G;
}

int fleet_opts(gusto_handle h, const gusto_fleet_opts* o, gusto_fleet_opts* out) {
    if (int rc = gusto_default_fleet_opts(h->model_pub, out)) return rc;
    out->margin = h->mp.clearance;   // (the handle's own, not the model's default)
    if (o) *out = *o;
    return GUSTO_OK;
}

// both entries: schedule (delay_steps unused) or separation of the last schedule's / a caller's shifts
int fleet_run(gusto_handle h, const char* who, bool schedule, int R, const int* order, const int* eligible, const int* delay_steps,
              const gusto_fleet_opts* opts) {
    if (int rc = post_enter(h, who, nullptr, nullptr)) return rc;
    gusto_fleet_opts o;
    if (int rc = fleet_opts(h, opts, &o)) return rc;
    if (int rc = fleet_args_host(h->model_pub, h->B, R, &o, order, delay_steps, nullptr, nullptr, who, &h->err)) return rc;
    FleetState& S = h->fleet;
    const VerifyState& V = h->verify;
    if (!V.have_dense) return refuse(h, who, "call gusto_interpolate first (the stage reads its dense trajectories)", GUSTO_ERR_STATE);
    if (!schedule && !delay_steps) {
        if (!S.have_sched) return refuse(h, who, "delay_steps = NULL before any gusto_fleet_schedule on these problems", GUSTO_ERR_STATE);
        if (R != S.R) return refuse(h, who, "delay_steps = NULL: R differs from the schedule's");
        if (o.dt_clock != S.sched_dt) return refuse(h, who, "delay_steps = NULL: dt_clock differs from the schedule's");
    }
    const size_t B = h->B, F = B / R, Bc = h->batch_cap;
    std::vector<double> tf(B);
    HIPCHK(h, hipMemcpyAsync(tf.data(), h->d_tf, sizeof(double) * B, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int Jmax = 0;
    if (int rc = fleet_args_host(h->model_pub, h->B, R, &o, nullptr, nullptr, tf.data(), &Jmax, who, &h->err)) return rc;
    const int ws = h->model_pub == GUSTO_FREEFLYER_SE2 ? 2 : 3;
    // (from here on the stage's state changes)
    S.have = false;
    if (schedule) S.have_sched = false;
    HIPCHK(h, S.Q.ensure(B * Jmax * ws)); HIPCHK(h, S.Box.ensure(B * 2 * ws)); HIPCHK(h, S.J.ensure(B)); HIPCHK(h, S.Fin.ensure(B));
    HIPCHK(h, S.I.ensure(FI_NB * B + B * R + FF_NF * F)); HIPCHK(h, S.D.ensure(FD_NB * B + B * R + F));
    HIPCHK(h, S.Sch.ensure_zeroed(SC_NB * Bc, h->stream));
    HIPCHK(h, S.t0.record(h->stream));
    FleetArgs A;
    memset(&A, 0, sizeof(A));
    const auto staged = [&](DevBuf<int>& buf, const int* src, const int** dst) -> int {
        *dst = nullptr;
        if (!src) return GUSTO_OK;
        HIPCHK(h, buf.ensure(B));
        HIPCHK(h, hipMemcpyAsync(buf, src, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
        *dst = buf;
        return GUSTO_OK;
    };
    if (int rc = staged(S.Ord, order, &A.ord)) return rc;
    if (int rc = staged(S.Elig, eligible, &A.elig)) return rc;
    if (int rc = staged(S.Sig, delay_steps, &A.sig)) return rc;
    A.G = fleet_geom(h->mp, o, ws);
    A.Q = S.Q; A.Box = S.Box; A.J = S.J; A.Fin = S.Fin; A.st_i = h->d_sti;
    A.Sch = S.Sch; A.I = S.I; A.D = S.D;
    A.B = h->B; A.R = R; A.Jmax = Jmax;
    TrackArgs T{V.Xf, h->d_tf, V.I.get() + 3 * Bc, S.Q, S.Box, S.J, S.Fin, o.dt_clock, V.dense_rows, h->n, Jmax};
    const dim3 fleets((unsigned)F), robots((unsigned)B);
    if (ws == 2) hipLaunchKernelGGL(track_kernel<2>, robots, dim3(TRACK_THREADS), 0, h->stream, T);
    else hipLaunchKernelGGL(track_kernel<3>, robots, dim3(TRACK_THREADS), 0, h->stream, T);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, S.t1.record(h->stream));
    if (schedule) {
        if (ws == 2) hipLaunchKernelGGL(schedule_kernel<2>, fleets, dim3(FLEET_THREADS), 0, h->stream, A);
        else hipLaunchKernelGGL(schedule_kernel<3>, fleets, dim3(FLEET_THREADS), 0, h->stream, A);
        HIPCHK(h, hipGetLastError());
    }
    HIPCHK(h, S.t2.record(h->stream));
    if (ws == 2) hipLaunchKernelGGL(separation_kernel<2>, fleets, dim3(FLEET_THREADS), 0, h->stream, A);
    else hipLaunchKernelGGL(separation_kernel<3>, fleets, dim3(FLEET_THREADS), 0, h->stream, A);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, S.t3.record(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (the staged host arrays are read by then)
    HIPCHK(h, event_ms(S.t0, S.t3, &S.last_ms));
    HIPCHK(h, event_ms(S.t0, S.t1, &S.stage_ms[0]));
    HIPCHK(h, event_ms(S.t1, S.t2, &S.stage_ms[1]));
    HIPCHK(h, event_ms(S.t2, S.t3, &S.stage_ms[2]));
    if (!schedule) S.stage_ms[1] = 0.0;
    S.F = (int)F; S.R = R; S.Jmax = Jmax; S.ws = ws;
    S.have = true;
    if (schedule) { S.have_sched = true; S.sched_dt = o.dt_clock; }
    return GUSTO_OK;
}

int fleet_getter(gusto_handle h, const char* who) {
    if (!h) return GUSTO_ERR_ARG;
    if (h->trajopt) return refuse(h, who, "TrajOpt handle (not supported)");
    if (!h->fleet.have) return refuse(h, who, "call gusto_fleet_schedule or gusto_fleet_separation first", GUSTO_ERR_STATE);
    return post_enter(h, who, nullptr, nullptr);
}

}  // namespace

extern "C" {

int gusto_default_fleet_opts(int model_id, gusto_fleet_opts* o) {
    if (!o || !model_info(model_id)) return GUSTO_ERR_ARG;
    gusto_scp_params sp;
    gusto_model_params mp;
    if (int rc = gusto_default_params(model_id, &sp, &mp)) return rc;
    o->dt_clock = 0.1;          // the default dt_min of gusto_verify_opts
    o->margin = mp.clearance;   // the distance the solver itself keeps from keep-out components
    o->n_delays = 64; o->delay_stride = 10; o->clock_cap = 8192; o->components = 1; o->prune = 1;
    return GUSTO_OK;
}

int gusto_fleet_schedule(gusto_handle h, int R, const int* order, const int* eligible, const gusto_fleet_opts* o) {
    return fleet_run(h, "gusto_fleet_schedule", true, R, order, eligible, nullptr, o);
}

int gusto_fleet_separation(gusto_handle h, int R, const int* delay_steps, const gusto_fleet_opts* o) {
    return fleet_run(h, "gusto_fleet_separation", false, R, nullptr, nullptr, delay_steps, o);
}

int gusto_get_fleet(gusto_handle h, gusto_fleet_report* out, int* F, int* R) {
    if (int rc = fleet_getter(h, "gusto_get_fleet")) return rc;
    const FleetState& S = h->fleet;
    if (F) *F = S.F;
    if (R) *R = S.R;
    if (!out) return GUSTO_OK;
    const size_t B = (size_t)S.F * S.R, nf = S.F, BR = B * S.R;
    const int* If = S.I.get() + FI_NB * B + BR;
    if (int rc = copy_out(h, out->status, S.I.get() + FI_STATUS * B, B)) return rc;
    if (int rc = copy_out(h, out->delay_steps, S.I.get() + FI_SIGMA * B, B)) return rc;
    if (int rc = copy_out(h, out->delay, S.D.get() + FD_DELAY * B, B)) return rc;
    if (int rc = copy_out(h, out->blocker, S.I.get() + FI_BLOCKER * B, B)) return rc;
    if (int rc = copy_out(h, out->min_sep, S.D.get() + FD_MINSEP * B, B)) return rc;
    if (int rc = copy_out(h, out->partner, S.I.get() + FI_PARTNER * B, B)) return rc;
    if (int rc = copy_out(h, out->step, S.I.get() + FI_STEP * B, B)) return rc;
    if (int rc = copy_out(h, out->pair_min_sep, S.D.get() + FD_NB * B, BR)) return rc;
    if (int rc = copy_out(h, out->pair_step, S.I.get() + FI_NB * B, BR)) return rc;
    if (int rc = copy_out(h, out->n_scheduled, If + FF_NSCHED * nf, nf)) return rc;
    if (int rc = copy_out(h, out->n_blocked, If + FF_NBLOCKED * nf, nf)) return rc;
    if (int rc = copy_out(h, out->n_conflicts, If + FF_NCONF * nf, nf)) return rc;
    if (int rc = copy_out(h, out->fleet_min_sep, S.D.get() + FD_NB * B + BR, nf)) return rc;
    if (int rc = copy_out(h, out->makespan_steps, If + FF_MAKESPAN * nf, nf)) return rc;
    if (out->stage_ms) memcpy(out->stage_ms, S.stage_ms, sizeof(S.stage_ms));
    return GUSTO_OK;
}

int gusto_get_fleet_tracks(gusto_handle h, int* J, double* Q, int* J_max) {
    if (int rc = fleet_getter(h, "gusto_get_fleet_tracks")) return rc;
    const FleetState& S = h->fleet;
    const size_t B = (size_t)S.F * S.R;
    if (J_max) *J_max = S.Jmax;
    if (int rc = copy_out(h, J, S.J.get(), B)) return rc;
    return copy_out(h, Q, S.Q.get(), B * S.Jmax * S.ws);
}

int gusto_last_fleet_ms(gusto_handle h, double* ms) {
    return stage_last_ms(h, &gusto_handle_s::fleet, ms, "gusto_last_fleet_ms", "call gusto_fleet_schedule or gusto_fleet_separation first");
}

}  // extern "C"
