// legs.hip -- goal timeline: the goals of a query before its final time, flown as legs and joined on the device.  A GoalSet of
// the reference is keyed by time (src/goals.jl:18-30), its goal row functions hard-code knot N: a goal before the final time is
// carried and ignored by the solve, there and in gusto_solve.  The timeline runs around gusto_solve, as the final-time search
// (tfsearch.hip) and replanning (replan.hip) do; no solve kernel knows of it.  The definitions are stated in include/gusto_hip.h.
//   gusto_legs_begin     SEQUENTIAL: the Bq queries' first legs are the B = Bq problems of the handle; PARALLEL: Bq queries x L
//                        legs are its B = Bq L problems, problem q L + l = leg l of query q
//   gusto_legs_advance   after a solve: the solved legs into the joined buffers and the report, the next legs' seeds
//   gusto_get_legs / gusto_get_legs_dev / gusto_last_legs_ms
// The timeline, the report and the joined trajectories stay on the device between the launches; an advance reads the Bq status
// words back (the finished queries go to gusto_set_active as inactive) and nothing else.
// Begin kernel: a thread per (problem, knot), the shape of fan_kernel (multistart.hip); consecutive threads write consecutive
// knots, the thread of knot 0 also writes the problem's x_init, goal_lo, goal_hi and tf, that of a query's first problem the
// query's report.  The straight line is straight_line() of seed.hpp, the one init_straightline_kernel (scp.hpp) evaluates: that
// kernel's output bit for bit.
// Residual kernel: one wavefront per leg in flight, lane i = state entry i (n <= 13 of 64 lanes), two wave_reduce maxima: gap and
// arrive.  It runs before the advance kernel, on the problems as the solve left them.
// Advance kernel: a thread per (leg in flight, knot): the knot's X and U rows into the joined buffers, its time, the next leg's
// seed knot; the thread of knot 0 also the leg's report row, the query's summary and the next problem's inputs.  A SEQUENTIAL
// advance writes the problem whose last knot every thread of it reads: the X rows are read from a staging copy made on the
// stream, device to device, as replan.hip does for a shared source; U is read and written by the same thread only.  The status
// words the kernels test are a copy as well: the thread of knot 0 writes the originals.
// The leg times and the time grid are one rounded operation each (contraction switched off where they are formed).  No atomics,
// nothing crosses a query: a query's report, joined buffers and seeds are the same bit for bit in any batch.
#include <hip/hip_runtime.h>

#include "seed.hpp"

using namespace gusto;

namespace {

constexpr int LI_STATUS = 0, LI_FAILED = 1, LI_NDONE = 2, LI_PREV = 3, LI_NQ = 4;   // rows [Bq] of LegsState::I, then the rows [Bq][L]:
constexpr int LL_ITER = 0, LL_CONV = 1, LL_SUCC = 2, LL_STOP = 3, LL_NI = 4;
constexpr int LD_J = 0, LD_GAP = 1, LD_ARRIVE = 2, LD_ND = 3;                        // rows [Bq][L] of LegsState::D behind J_total [Bq]

// tf of leg l of a timeline T: T_l - T_{l-1}, one rounded difference; T_0 itself
GD double leg_tf(const double* T, int l) { return l == 0 ? T[0] : T[l] - T[l - 1]; }
// the time of knot k of a leg that starts at T0 and lasts tf: T0 + k (tf / (N - 1)), every operation rounded on its own (the
// pragma keeps the product and the sum apart, as in tfsearch.hip)
GD double knot_time(double T0, double tf, int k, int N) {
#pragma clang fp contract(off)
    const double dt = tf / (double)(N - 1);
    const double up = (double)k * dt;
    return T0 + up;
}

// the stage's state as the kernels see it
struct LegsDev {
    const double *xi, *glo, *ghi, *T;   // [Bq][n], [Bq][L][n] twice, [Bq][L]
    const int* nl;                      // [Bq]
    int* I;
    double *D, *Xj, *Uj, *tj;
    int Bq, L, N, K;                    // K: problems per query, 1 (SEQUENTIAL) or L (PARALLEL)
    GD int* leg_i(int row) const { return I + (size_t)LI_NQ * Bq + (size_t)row * Bq * L; }
    GD double* leg_d(int row) const { return D + Bq + (size_t)row * Bq * L; }
};

struct BeginArgs {
    LegsDev S;
    SeedOut out;
    int B;
};

template <int MODEL> __global__ void begin_kernel(const BeginArgs A) {
    using T = MT<MODEL>;
    constexpr int n = T::n, m = T::m;
    const LegsDev& S = A.S;
    KnotId id;
    if (!knot_id(A.B, S.K, S.N, id)) return;
    const int b = id.b, k = id.k, q = id.q;
    const int l = min(id.j, S.nl[q] - 1);   // (the problems behind a ragged query's last leg: that leg)
    // PARALLEL: every interior goal is a full point, the junction; SEQUENTIAL has K = 1, l = 0
    const double* xi = l == 0 ? S.xi + (size_t)q * n : S.glo + ((size_t)q * S.L + l - 1) * n;
    const double* lo = S.glo + ((size_t)q * S.L + l) * n;
    const double* hi = S.ghi + ((size_t)q * S.L + l) * n;
    double* Xo = A.out.X + ((size_t)b * S.N + k) * n;
    double* Uo = A.out.U + ((size_t)b * S.N + k) * m;
#pragma unroll
    for (int i = 0; i < n; i++) Xo[i] = straight_line(id.t, xi[i], lo[i], hi[i]);
#pragma unroll
    for (int i = 0; i < m; i++) Uo[i] = 0.0;
    if (k == 0) {
        seed_problem_tail<MODEL>(A.out, b, xi, lo, hi, leg_tf(S.T + (size_t)q * S.L, l));
        if (id.j == 0) {
            S.I[LI_STATUS * S.Bq + q] = GUSTO_LEGS_FLYING; S.I[LI_FAILED * S.Bq + q] = -1; S.I[LI_NDONE * S.Bq + q] = 0;
            S.D[q] = 0.0;
        }
    }
}

struct AdvanceArgs {
    LegsDev S;
    const int* elig;                          // [B], null: converged && successful
    const int* st_i;                          // the handle's status words [B][ST_NI]
    const double* Jt;                         // its J_true history [B][hist_cap]
    const double *Xs, *U;                     // the solved rows: X (SEQUENTIAL: the staging copy) and the handle's U
    const double *xinit, *hlo, *hhi;          // the handle's problems [B][n]
    SeedOut out;
    int B, hist_cap, round;
};

// the leg that problem b of query q holds, -1: none in flight (the query is finished, or the problem lies behind its last leg)
GD int leg_in_flight(const AdvanceArgs& A, int q, int j) {
    if (A.S.I[LI_PREV * A.S.Bq + q] != GUSTO_LEGS_FLYING) return -1;
    const int l = A.S.K == 1 ? A.round : j;
    return l < A.S.nl[q] ? l : -1;
}
GD bool leg_ok(const AdvanceArgs& A, size_t b) {
    return A.elig ? A.elig[b] != 0 : (A.st_i[b * ST_NI + ST_CONV] != 0 && A.st_i[b * ST_NI + ST_SUCC] != 0);
}
GD double leg_J(const AdvanceArgs& A, size_t b) {
    const int nJ = A.st_i[b * ST_NI + ST_NJ];
    return nJ > 0 ? A.Jt[b * A.hist_cap + nJ - 1] : NAN;
}

// (64 lanes: every lane takes part in the reductions, the state entries are the lanes below n)
__global__ void __launch_bounds__(64) residual_kernel(const AdvanceArgs A, int n) {
    const LegsDev& S = A.S;
    const int b = blockIdx.x, lane = threadIdx.x, q = b / S.K;
    const int l = leg_in_flight(A, q, b % S.K);   // (the whole wave)
    if (l < 0) return;
    double g = 0.0, a = 0.0;
    if (lane < n) {
        const double* X = A.Xs + (size_t)b * S.N * n;
        const double x0 = X[lane], xe = X[(size_t)(S.N - 1) * n + lane];
        const double lo = A.hlo[(size_t)b * n + lane], hi = A.hhi[(size_t)b * n + lane];
        if (l > 0) g = fabs(x0 - A.xinit[(size_t)b * n + lane]);
        a = lo == hi ? fabs(xe - lo) : fmax(fmax(lo - xe, xe - hi), 0.0);
    }
    g = wave_reduce(g, OpMax());
    a = wave_reduce(a, OpMax());
    if (lane == 0) {
        S.leg_d(LD_GAP)[(size_t)q * S.L + l] = g;
        S.leg_d(LD_ARRIVE)[(size_t)q * S.L + l] = a;
    }
}

template <int MODEL> __global__ void advance_kernel(const AdvanceArgs A) {
    using T = MT<MODEL>;
    constexpr int n = T::n, m = T::m;
    const LegsDev& S = A.S;
    KnotId id;
    if (!knot_id(A.B, S.K, S.N, id)) return;
    const int b = id.b, k = id.k, q = id.q, N = S.N, L = S.L, Bq = S.Bq;
    const int l = leg_in_flight(A, q, id.j);
    if (l < 0) return;
    const bool parallel = S.K > 1;
    const int Lq = S.nl[q];
    const bool ok = leg_ok(A, b);
    const double* Tq = S.T + (size_t)q * L;
    // 1. the join: knot l (N - 1) + k of the query
    const size_t Nj = (size_t)L * (N - 1) + 1, row = (size_t)q * Nj + (size_t)l * (N - 1) + k;
    const double* Xr = A.Xs + ((size_t)b * N + k) * n;
    double* Uo = A.out.U + ((size_t)b * N + k) * m;
    if (k > 0 || l == 0) {   // (a junction's X and t: the last knot of the leg before)
#pragma unroll
        for (int i = 0; i < n; i++) S.Xj[row * n + i] = Xr[i];
        S.tj[row] = k == N - 1 ? Tq[l] : knot_time(l == 0 ? 0.0 : Tq[l - 1], leg_tf(Tq, l), k, N);
    }
    // (a junction's U: the first knot of the leg behind; SEQUENTIAL writes the last knot of every leg, the next advance over it)
    if (!parallel || k < N - 1 || l == Lq - 1) {
#pragma unroll
        for (int i = 0; i < m; i++) S.Uj[row * m + i] = Uo[i];
    }
    // 2. the problem's next start: the next leg from the junction, or the straight line of the leg it flew
    const bool next = !parallel && ok && l + 1 < Lq;
    const double* xi = next ? A.Xs + ((size_t)b * N + N - 1) * n : A.xinit + (size_t)b * n;
    const double* lo = next ? S.glo + ((size_t)q * L + l + 1) * n : A.hlo + (size_t)b * n;
    const double* hi = next ? S.ghi + ((size_t)q * L + l + 1) * n : A.hhi + (size_t)b * n;
    double* Xo = A.out.X + ((size_t)b * N + k) * n;
#pragma unroll
    for (int i = 0; i < n; i++) Xo[i] = straight_line(id.t, xi[i], lo[i], hi[i]);
#pragma unroll
    for (int i = 0; i < m; i++) Uo[i] = 0.0;
    if (k != 0) return;
    // (a finished problem keeps its inputs: nothing of them is written while the other threads read them)
    if (next) seed_problem_tail<MODEL>(A.out, b, xi, lo, hi, leg_tf(Tq, l + 1));
    // 3. the leg's report row
    const size_t ql = (size_t)q * L + l;
    const double J = leg_J(A, b);
    S.leg_i(LL_ITER)[ql] = A.st_i[(size_t)b * ST_NI + ST_ITER];
    S.leg_i(LL_CONV)[ql] = A.st_i[(size_t)b * ST_NI + ST_CONV];
    S.leg_i(LL_SUCC)[ql] = A.st_i[(size_t)b * ST_NI + ST_SUCC];
    S.leg_i(LL_STOP)[ql] = A.st_i[(size_t)b * ST_NI + ST_STOP];
    S.leg_d(LD_J)[ql] = J;
    // 4. the query's summary
    if (!parallel) {
        S.D[q] = S.D[q] + J;
        if (ok) {
            S.I[LI_NDONE * Bq + q] = l + 1;
            S.I[LI_STATUS * Bq + q] = l + 1 == Lq ? GUSTO_LEGS_DONE : GUSTO_LEGS_FLYING;
        } else {
            S.I[LI_STATUS * Bq + q] = GUSTO_LEGS_FAILED;
            S.I[LI_FAILED * Bq + q] = l;
        }
    } else if (l == 0) {   // every leg of the query, in leg order, from the handle's own words (not from the other threads' rows)
        double Jtot = 0.0;
        int failed = -1;
        for (int ll = 0; ll < Lq; ll++) {
            const size_t bb = (size_t)q * L + ll;
            Jtot = Jtot + leg_J(A, bb);
            if (failed < 0 && !leg_ok(A, bb)) failed = ll;
        }
        S.D[q] = Jtot;
        S.I[LI_NDONE * Bq + q] = failed < 0 ? Lq : failed;
        S.I[LI_FAILED * Bq + q] = failed;
        S.I[LI_STATUS * Bq + q] = failed < 0 ? GUSTO_LEGS_DONE : GUSTO_LEGS_FAILED;
    }
}

LegsDev legs_dev(gusto_handle h) {
    const LegsState& S = h->legs;
    const size_t q = S.Bq, L = S.L, n = h->n;
    const double* in = S.In;
    return {in, in + q * n, in + q * n * (1 + L), in + q * n * (1 + 2 * L), S.NL, S.I, S.D, S.X, S.U, S.T,
            S.Bq, S.L, h->N, S.mode == GUSTO_LEGS_PARALLEL ? S.L : 1};
}

// every interior goal of every query pins every entry
bool full_points(int Bq, int L, int n, const int* n_legs, const double* glo, const double* ghi) {
    for (size_t q = 0; q < (size_t)Bq; q++)
        for (size_t l = 0; l + 1 < (size_t)(n_legs ? n_legs[q] : L); l++)
            for (size_t i = 0; i < (size_t)n; i++) {
                const double lo = glo[(q * L + l) * n + i], hi = ghi[(q * L + l) * n + i];
                if (!(lo == hi && fabs(lo) < INFINITY)) return false;
            }
    return true;
}

// The arguments of gusto_legs_begin behind query_args_host; *mode comes back resolved (never AUTO).  GUSTO_ERR_ARG and the text,
// which names the first offending query, in *err.  No device, no handle.
int legs_args_host(int Bq, int L, int n, int batch_cap, const int* n_legs, const double* x_init, const double* glo, const double* ghi,
                   const double* t_goal, int* mode, const char* who, std::string* err) {
    const std::string w = std::string(who) + ": ";
    const auto at = [](size_t q) { return " (query " + std::to_string(q) + ")"; };
    if (*mode != GUSTO_LEGS_AUTO && *mode != GUSTO_LEGS_SEQUENTIAL && *mode != GUSTO_LEGS_PARALLEL) { *err = w + "unknown mode"; return GUSTO_ERR_ARG; }
    for (size_t q = 0; q < (size_t)Bq; q++) {
        const int Lq = n_legs ? n_legs[q] : L;
        if (Lq < 1 || Lq > L) { *err = w + "n_legs outside 1 .. L" + at(q); return GUSTO_ERR_ARG; }
        for (int l = 0; l < Lq; l++) {
            const double T = t_goal[q * L + l], before = l ? t_goal[q * L + l - 1] : 0.0;
            if (!(T > before && T < INFINITY)) { *err = w + "need 0 < T_0 < T_1 < ... < inf" + at(q); return GUSTO_ERR_ARG; }
        }
        for (int i = 0; i < n; i++)
            if (!(fabs(x_init[q * n + i]) < INFINITY)) { *err = w + "x_init must be finite" + at(q); return GUSTO_ERR_ARG; }
    }
    const bool points = full_points(Bq, L, n, n_legs, glo, ghi);
    if (*mode == GUSTO_LEGS_PARALLEL && !points) {
        *err = w + "GUSTO_LEGS_PARALLEL: an interior goal does not pin every entry (lo == hi, finite)";
        return GUSTO_ERR_ARG;
    }
    if (*mode == GUSTO_LEGS_AUTO) *mode = points ? GUSTO_LEGS_PARALLEL : GUSTO_LEGS_SEQUENTIAL;
    if ((long long)Bq * (*mode == GUSTO_LEGS_PARALLEL ? L : 1) > batch_cap) { *err = w + "B above batch_cap"; return GUSTO_ERR_ARG; }
    return GUSTO_OK;
}

// the refusals of advance and the getters, then the handle's device and its enqueued solve
int legs_enter(gusto_handle h, const char* who) {
    if (!h) return GUSTO_ERR_ARG;
    if (h->trajopt) return refuse(h, who, "TrajOpt handle (not supported)");
    if (!h->legs.have) return refuse(h, who, "the handle's problems were not set by gusto_legs_begin", GUSTO_ERR_STATE);
    return post_enter(h, who, nullptr, nullptr);
}

// what follows the kernels of begin and advance: everything gusto_set_problems does, and the stage's time
int legs_loaded(gusto_handle h) {
    LegsState& S = h->legs;
    if (int rc = gusto_problems_loaded(h, false)) return rc;   // (waits for the stream: the host arrays are read, written by then)
    HIPCHK(h, event_ms(S.t0, S.t1, &S.last_ms));
    S.solves_at = h->solves;
    S.have = true;
    return GUSTO_OK;
}

}  // namespace

extern "C" {

int gusto_default_legs_opts(int model_id, gusto_legs_opts* o) {
    if (!o || !model_info(model_id)) return GUSTO_ERR_ARG;
    o->mode = GUSTO_LEGS_AUTO;
    return GUSTO_OK;
}

int gusto_legs_begin(gusto_handle h, int Bq, int L, const int* n_legs, const double* x_init, const double* glo, const double* ghi,
                     const double* t_goal, const gusto_legs_opts* o) {
    const char* who = "gusto_legs_begin";
    int mode = o ? o->mode : GUSTO_LEGS_AUTO;
    // (B is Bq or Bq L, which the goals decide: the shared check asks for Bq problems, legs_args_host for those of the mode)
    if (int rc = seed_enter(h, who, Bq, L, GUSTO_MAX_STARTS, "GUSTO_MAX_STARTS", {x_init, glo, ghi, t_goal}, [&]() -> int {
            return legs_args_host(Bq, L, h->n, h->batch_cap, n_legs, x_init, glo, ghi, t_goal, &mode, who, &h->err);
        }, 1))
        return rc;
    const size_t n = h->n, m = h->m, N = h->N, q = Bq, nl = L, K = mode == GUSTO_LEGS_PARALLEL ? L : 1, Nj = nl * (N - 1) + 1;
    std::vector<double> in(q * n * (1 + 2 * nl) + q * nl);   // x_init | goal_lo | goal_hi | t_goal: one copy
    memcpy(in.data(), x_init, sizeof(double) * q * n);
    memcpy(in.data() + q * n, glo, sizeof(double) * q * nl * n);
    memcpy(in.data() + q * n * (1 + nl), ghi, sizeof(double) * q * nl * n);
    memcpy(in.data() + q * n * (1 + 2 * nl), t_goal, sizeof(double) * q * nl);
    std::vector<int> legs(q, L), active(q * K, 1);
    if (n_legs) legs.assign(n_legs, n_legs + q);
    for (size_t b = 0; b < q * K; b++) active[b] = (int)(b % K) < legs[b / K] || K == 1;
    LegsState& S = h->legs;
    S.have = false;
    HIPCHK(h, S.In.ensure(in.size())); HIPCHK(h, S.NL.ensure(q));
    HIPCHK(h, S.I.ensure((LI_NQ + LL_NI * nl) * q)); HIPCHK(h, S.D.ensure((1 + LD_ND * nl) * q));
    HIPCHK(h, S.X.ensure(q * Nj * n)); HIPCHK(h, S.U.ensure(q * Nj * m)); HIPCHK(h, S.T.ensure(q * Nj));
    seed_set_B(h, q * K);
    S.Bq = Bq; S.L = L; S.mode = mode; S.round = 0; S.n_flying = Bq;
    HIPCHK(h, S.t0.record(h->stream));
    HIPCHK(h, hipMemcpyAsync(S.In, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(S.NL, legs.data(), sizeof(int) * q, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(S.I, 0, sizeof(int) * (LI_NQ + LL_NI * nl) * q, h->stream));   // (the rows of the legs not stored yet)
    HIPCHK(h, hipMemsetAsync(S.D, 0, sizeof(double) * (1 + LD_ND * nl) * q, h->stream));
    HIPCHK(h, hipMemsetAsync(S.X, 0, sizeof(double) * q * Nj * n, h->stream));
    HIPCHK(h, hipMemsetAsync(S.U, 0, sizeof(double) * q * Nj * m, h->stream));
    HIPCHK(h, hipMemsetAsync(S.T, 0, sizeof(double) * q * Nj, h->stream));
    const BeginArgs A{legs_dev(h), seed_out(h), h->B};
    if (int rc = launch_per_knot(h, A, [](auto M) { return begin_kernel<decltype(M)::value>; })) return rc;
    HIPCHK(h, S.t1.record(h->stream));
    if (int rc = legs_loaded(h)) return rc;
    // the problems behind a ragged query's last leg: inactive
    return std::find(active.begin(), active.end(), 0) == active.end() ? GUSTO_OK : gusto_set_active(h, active.data());
}

int gusto_legs_advance(gusto_handle h, const int* eligible) {
    const char* who = "gusto_legs_advance";
    if (int rc = legs_enter(h, who)) return rc;
    LegsState& S = h->legs;
    if (S.n_flying == 0) return refuse(h, who, "no query is still flying", GUSTO_ERR_STATE);
    if (!eligible && h->solves == S.solves_at)
        return refuse(h, who, "no gusto_solve since the last begin or advance (the default eligibility reads its status)", GUSTO_ERR_STATE);
    const bool parallel = S.mode == GUSTO_LEGS_PARALLEL;
    const size_t B = h->B, q = S.Bq, n = h->n, N = h->N, K = parallel ? S.L : 1;
    HIPCHK(h, S.t0.record(h->stream));
    AdvanceArgs A;
    A.S = legs_dev(h);
    A.elig = nullptr;
    if (eligible) {
        HIPCHK(h, S.Elig.ensure(B));
        HIPCHK(h, hipMemcpyAsync(S.Elig, eligible, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
        A.elig = S.Elig;
    }
    HIPCHK(h, hipMemcpyAsync(S.I.get() + LI_PREV * q, S.I.get() + LI_STATUS * q, sizeof(int) * q, hipMemcpyDeviceToDevice, h->stream));
    A.Xs = h->d_X;
    if (!parallel) {   // (a PARALLEL thread reads the knot it writes and no other)
        HIPCHK(h, S.Xs.ensure(B * N * n));
        HIPCHK(h, hipMemcpyAsync(S.Xs, h->d_X, sizeof(double) * B * N * n, hipMemcpyDeviceToDevice, h->stream));
        A.Xs = S.Xs;
    }
    A.st_i = h->d_sti; A.Jt = h->d_Jt; A.U = h->d_U; A.xinit = h->d_xinit; A.hlo = h->d_glo; A.hhi = h->d_ghi;
    A.out = seed_out(h);
    A.B = h->B; A.hist_cap = h->hist_cap; A.round = S.round;
    hipLaunchKernelGGL(residual_kernel, dim3((unsigned)B), dim3(64), 0, h->stream, A, h->n);
    HIPCHK(h, hipGetLastError());
    if (int rc = launch_per_knot(h, A, [](auto M) { return advance_kernel<decltype(M)::value>; })) return rc;
    std::vector<int> st(q);
    HIPCHK(h, hipMemcpyAsync(st.data(), S.I.get() + LI_STATUS * q, sizeof(int) * q, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, S.t1.record(h->stream));
    if (int rc = legs_loaded(h)) return rc;   // (st is written by then)
    S.round++;
    std::vector<int> active(B);
    int flying = 0;
    for (size_t i = 0; i < q; i++) {
        const int on = st[i] == GUSTO_LEGS_FLYING;
        flying += on;
        for (size_t j = 0; j < K; j++) active[i * K + j] = on;
    }
    S.n_flying = flying;
    return flying == S.Bq ? GUSTO_OK : gusto_set_active(h, active.data());   // the finished queries' problems: inactive
}

int gusto_get_legs(gusto_handle h, gusto_legs_report* out, int* round, int* n_flying) {
    if (int rc = legs_enter(h, "gusto_get_legs")) return rc;
    const LegsState& S = h->legs;
    if (round) *round = S.round;
    if (n_flying) *n_flying = S.n_flying;
    if (!out) return GUSTO_OK;
    const size_t q = S.Bq, ql = q * S.L, Nj = (size_t)S.L * (h->N - 1) + 1;
    const int* Il = S.I.get() + LI_NQ * q;
    const double* Dl = S.D.get() + q;
    if (int rc = copy_out(h, out->status, S.I.get() + LI_STATUS * q, q)) return rc;
    if (int rc = copy_out(h, out->failed_leg, S.I.get() + LI_FAILED * q, q)) return rc;
    if (int rc = copy_out(h, out->n_done, S.I.get() + LI_NDONE * q, q)) return rc;
    if (int rc = copy_out(h, out->J_total, S.D.get(), q)) return rc;
    if (int rc = copy_out(h, out->iterations, Il + LL_ITER * ql, ql)) return rc;
    if (int rc = copy_out(h, out->converged, Il + LL_CONV * ql, ql)) return rc;
    if (int rc = copy_out(h, out->successful, Il + LL_SUCC * ql, ql)) return rc;
    if (int rc = copy_out(h, out->stop_reason, Il + LL_STOP * ql, ql)) return rc;
    if (int rc = copy_out(h, out->J, Dl + LD_J * ql, ql)) return rc;
    if (int rc = copy_out(h, out->gap, Dl + LD_GAP * ql, ql)) return rc;
    if (int rc = copy_out(h, out->arrive, Dl + LD_ARRIVE * ql, ql)) return rc;
    if (int rc = copy_out(h, out->X, S.X.get(), q * Nj * h->n)) return rc;
    if (int rc = copy_out(h, out->U, S.U.get(), q * Nj * h->m)) return rc;
    return copy_out(h, out->t, S.T.get(), q * Nj);
}

int gusto_get_legs_dev(gusto_handle h, const double** X_dev, const double** U_dev, const double** t_dev) {
    if (int rc = legs_enter(h, "gusto_get_legs_dev")) return rc;
    const LegsState& S = h->legs;
    if (X_dev) *X_dev = S.X;
    if (U_dev) *U_dev = S.U;
    if (t_dev) *t_dev = S.T;
    return GUSTO_OK;
}

int gusto_last_legs_ms(gusto_handle h, double* ms) {
    return stage_last_ms(h, &gusto_handle_s::legs, ms, "gusto_last_legs_ms", "the handle's problems were not set by gusto_legs_begin");
}

}  // extern "C"
