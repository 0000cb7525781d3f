// tfsearch.hip -- final-time search: per query the shortest final time whose solve is eligible, by K-section over solves.  The
// reference's free final time is a JuMP variable with the single row Tf >= 0.1 that nothing moves (fixed_final_time = false is
// inert there and in this library's host layer); the search is this library's own.  The definitions are stated in
// include/gusto_hip.h.
//   gusto_tfsearch_begin    Bq queries x K candidate final times become the B = Bq K problems of the handle, problem q K + j =
//                           candidate j of query q
//   gusto_tfsearch_update   after a solve: incumbent, bracket, status, the next round's candidates and their seeds
//   gusto_get_tfsearch / gusto_get_tfsearch_dev / gusto_last_tfsearch_ms
// The bracket, the incumbent plans, the candidates and their seeds stay on the device between the launches; an update reads the
// Bq status words back (the done queries go to gusto_set_active as inactive) and nothing else.
// Begin kernel: a thread per (query, candidate) writes the round-0 candidate, the thread of candidate 0 the query's state.
// Update kernel: one wavefront per query, lane j = candidate j (K <= 64), the shape of select_kernel (multistart.hip): a
// wave_reduce minimum over the eligible final times, a second one over the lanes that hold it picks the lowest lane; the whole
// wave gathers that problem's X and U, lane-consecutive, into the incumbent buffers.
// Seed kernel: a thread per (problem, knot), the shape of fan_kernel (multistart.hip); consecutive threads write consecutive
// knots, the thread of knot 0 also writes the problem's x_init, goal_lo, goal_hi and tf.  The straight line is straight_line()
// of seed.hpp, the one init_straightline_kernel (scp.hpp) evaluates: that kernel's output bit for bit.  The incumbent is read from
// the search's own buffers, never from the rows the kernel writes.
// The candidates are one rounded difference, division, product and sum each (contraction switched off where they are formed).  No atomics,
// nothing crosses a query: a query's report and seeds are the same bit for bit in any batch.
#include <hip/hip_runtime.h>

#include "seed.hpp"

using namespace gusto;

namespace {

constexpr int TF_LO = 0, TF_HI = 1, TF_LO0 = 2, TF_HI0 = 3, TF_BEST = 4, TF_J = 5, TF_ND = 6;   // rows of TfsearchState::D
constexpr int TI_STATUS = 0, TI_FOUND = 1, TI_NELIG = 2, TI_PARKED = 3, TI_NI = 4;              // rows of TfsearchState::I
constexpr int TF_FINISHED = GUSTO_TFSEARCH_NONE | GUSTO_TFSEARCH_DONE;

// candidate j of K in (lo, hi]: lo + (j + 1) (w / div), every operation rounded on its own (HIP's __dmul_rn / __dadd_rn are a
// plain product and sum, which hipcc contracts once they are inlined: the pragma is what keeps the product and the sum apart)
GD double candidate(double lo, double hi, int j, int div) {
#pragma clang fp contract(off)
    const double w = hi - lo;
    const double step = w / (double)div;
    const double up = (double)(j + 1) * step;
    return lo + up;
}
// hi - lo <= rtol hi, likewise
GD bool narrow(double lo, double hi, double rtol) {
#pragma clang fp contract(off)
    const double w = hi - lo, allowed = rtol * hi;
    return w <= allowed;
}

// the entries of a state that are rates: they scale with 1 / tf under a retiming
template <int MODEL> GD constexpr bool rate_entry(int i) {
    if (MODEL == GUSTO_FREEFLYER_SE2) return i >= 3 && i < 6;
    if (MODEL == GUSTO_ASTROBEE_SE3) return (i >= 3 && i < 6) || (i >= 9 && i < 12);
    if (MODEL == GUSTO_ASTROBEE_SE3_MANIFOLD) return (i >= 3 && i < 6) || (i >= 10 && i < 13);
    return false;
}

__global__ void begin_kernel(const double* lo0, const double* hi0, double* D, int* I, double* cand, int Bq, int K) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= Bq * K) return;
    const int q = gid / K, j = gid % K;
    const double lo = lo0[q], hi = hi0[q];
    cand[gid] = j == K - 1 ? hi : candidate(lo, hi, j, K);   // (the upper end is always tried)
    if (j == 0) {
        D[TF_LO * Bq + q] = lo; D[TF_HI * Bq + q] = hi; D[TF_LO0 * Bq + q] = lo; D[TF_HI0 * Bq + q] = hi;
        D[TF_BEST * Bq + q] = NAN; D[TF_J * Bq + q] = NAN;
        I[TI_STATUS * Bq + q] = 0; I[TI_FOUND * Bq + q] = -1; I[TI_NELIG * Bq + q] = 0; I[TI_PARKED * Bq + q] = 0;
    }
}

struct UpdateArgs {
    const int* elig;       // [B], null: converged && successful
    const int* st_i;       // the handle's status words [B][ST_NI]
    const double* Jt;      // its J_true history [B][hist_cap]
    const double* tf;      // its final times [B]: the candidates of the round
    const double *X, *U;   // its trajectories, rows of nx = N n and nu = N m doubles
    double *D, *cand, *Xb, *Ub;
    int* I;
    int Bq, K, hist_cap, nx, nu, round;
    double rtol;
};

// (64 lanes: every lane takes part in the reductions, the candidates are the lanes below K)
__global__ void __launch_bounds__(64) update_kernel(const UpdateArgs A) {
    const int q = blockIdx.x, lane = threadIdx.x, Bq = A.Bq;
    const int st_old = A.I[TI_STATUS * Bq + q];
    if (st_old & TF_FINISHED) {   // (the whole wave: a done query is not touched)
        if (lane == 0) A.I[TI_PARKED * Bq + q] = 1;
        return;
    }
    const size_t b = (size_t)q * A.K + lane;
    const bool in = lane < A.K;
    bool ok = false;
    double T = NAN;
    if (in) {
        const int* st = A.st_i + b * ST_NI;
        ok = A.elig ? A.elig[b] != 0 : (st[ST_CONV] != 0 && st[ST_SUCC] != 0);
        T = A.tf[b];
    }
    const double lo_old = A.D[TF_LO * Bq + q], lo0 = A.D[TF_LO0 * Bq + q], hi0 = A.D[TF_HI0 * Bq + q];
    double F = A.D[TF_BEST * Bq + q];
    bool have = A.I[TI_FOUND * Bq + q] >= 0;
    // 1. the incumbent: the smallest eligible final time, ties to the lowest candidate; it replaces on a strict < only
    const double Fn = wave_reduce(ok ? T : INFINITY, OpMin());
    const int w = (int)wave_reduce((ok && T == Fn) ? (double)lane : 64.0, OpMin());
    const int ne = (int)wave_reduce(ok ? 1.0 : 0.0, OpSum());
    const int first_ok = (int)wave_reduce(ok ? (double)lane : 64.0, OpMin());
    const int last_bad = (int)wave_reduce((in && !ok) ? (double)lane : -1.0, OpMax());
    const bool take = w < 64 && (!have || Fn < F);
    if (take) {
        const size_t bw = (size_t)q * A.K + w;
        const double* Xw = A.X + bw * A.nx;
        const double* Uw = A.U + bw * A.nu;
        for (int e = lane; e < A.nx; e += 64) A.Xb[(size_t)q * A.nx + e] = Xw[e];
        for (int e = lane; e < A.nu; e += 64) A.Ub[(size_t)q * A.nu + e] = Uw[e];
        if (lane == 0) {
            const int nJ = A.st_i[bw * ST_NI + ST_NJ];
            A.D[TF_BEST * Bq + q] = Fn;
            A.D[TF_J * Bq + q] = nJ > 0 ? A.Jt[bw * A.hist_cap + nJ - 1] : NAN;
            A.I[TI_FOUND * Bq + q] = A.round;
        }
        F = Fn; have = true;
    }
    // 2. the bracket
    double lo, hi;
    if (have) {
        const double refuted = wave_reduce((in && !ok && T < F) ? T : -INFINITY, OpMax());
        lo = fmax(lo0, refuted);
        if (lo_old < F) lo = fmax(lo, lo_old);
        hi = F;
    } else {
        lo = wave_reduce(in ? T : -INFINITY, OpMax());
        hi = hi0;
    }
    // 3. the status word
    int st = st_old & GUSTO_TFSEARCH_NONMONOTONE;
    if (!have) st |= GUSTO_TFSEARCH_NONE;
    if (narrow(lo, hi, A.rtol)) st |= GUSTO_TFSEARCH_DONE;
    if (lo == lo0) st |= GUSTO_TFSEARCH_FLOOR;
    if (first_ok < last_bad || (have && lo_old >= F)) st |= GUSTO_TFSEARCH_NONMONOTONE;
    // 4. the next round's candidates; those of a done query are its hi
    if (in) A.cand[b] = (st & TF_FINISHED) ? hi : candidate(lo, hi, lane, A.K + 1);
    if (lane == 0) {
        A.D[TF_LO * Bq + q] = lo; A.D[TF_HI * Bq + q] = hi;
        A.I[TI_STATUS * Bq + q] = st; A.I[TI_NELIG * Bq + q] = ne; A.I[TI_PARKED * Bq + q] = 0;
    }
}

struct SeedArgs {
    QueryDev Q;                         // the queries (extra: the bracket of gusto_tfsearch_begin, not read here)
    const double *D, *cand, *Xb, *Ub;   // the search's state
    const int* I;
    SeedOut out;
    int B, Bq, K, N, seed;
};

template <int MODEL> __global__ void seed_kernel(const SeedArgs A) {
    using T = MT<MODEL>;
    constexpr int n = T::n, m = T::m;
    KnotId id;
    if (!knot_id(A.B, A.K, A.N, id)) return;
    const int b = id.b, k = id.k, q = id.q;
    if (A.I[TI_PARKED * A.Bq + q]) return;   // done before the last update: its problems stay as they are
    const double t = id.t;
    const size_t qn = (size_t)q * n;   // the query's row of xi, glo, ghi
    const double Tj = A.cand[b];
    const bool retime = A.seed == GUSTO_TFSEARCH_SEED_INCUMBENT && A.I[TI_FOUND * A.Bq + q] >= 0 &&
                        !(A.I[TI_STATUS * A.Bq + q] & TF_FINISHED);
    double* Xo = A.out.X + ((size_t)b * A.N + k) * n;
    double* Uo = A.out.U + ((size_t)b * A.N + k) * m;
    double x[n];
#pragma unroll
    for (int i = 0; i < n; i++) x[i] = straight_line(t, A.Q.xi[qn + i], A.Q.glo[qn + i], A.Q.ghi[qn + i]);
    if (!retime) {
#pragma unroll
        for (int i = 0; i < n; i++) Xo[i] = x[i];
#pragma unroll
        for (int i = 0; i < m; i++) Uo[i] = 0.0;
    } else {
        const double s = A.D[TF_BEST * A.Bq + q] / Tj, s2 = s * s;
        const double* Xr = A.Xb + ((size_t)q * A.N + k) * n;
        const double* Ur = A.Ub + ((size_t)q * A.N + k) * m;
#pragma unroll
        for (int i = 0; i < n; i++) {
            // s Xr + (1 - s) x, the second product fused as it always was (straight_line in seed.hpp: why it is written out)
            const double v = rate_entry<MODEL>(i) ? fma(1 - s, x[i], s * Xr[i]) : Xr[i];
            Xo[i] = k == 0 ? A.Q.xi[qn + i] : v;
        }
#pragma unroll
        for (int i = 0; i < m; i++) Uo[i] = s2 * Ur[i];
    }
    if (k == 0) seed_problem_tail<MODEL>(A.out, b, A.Q.xi + qn, A.Q.glo + qn, A.Q.ghi + qn, Tj);
}

bool bracket_ok(double lo, double hi) { return lo > 0 && lo < hi && hi < INFINITY; }

int launch_seed(gusto_handle h) {
    const TfsearchState& S = h->tfsearch;
    const SeedArgs A{query_dev(S.In, S.Bq, h->n), S.D, S.Cand, S.X, S.U, S.I, seed_out(h), h->B, S.Bq, S.K, h->N, S.seed};
    return launch_per_knot(h, A, [](auto M) { return seed_kernel<decltype(M)::value>; });
}

// the refusals of update and the getters, then the handle's device and its enqueued solve
int search_enter(gusto_handle h, const char* who) {
    if (!h) return GUSTO_ERR_ARG;
    if (h->trajopt) return refuse(h, who, "TrajOpt handle (not supported)");
    if (!h->tfsearch.have) return refuse(h, who, "the handle's problems were not set by gusto_tfsearch_begin", GUSTO_ERR_STATE);
    return post_enter(h, who, nullptr, nullptr);
}

}  // namespace

extern "C" {

int gusto_default_tfsearch_opts(int model_id, gusto_tfsearch_opts* o) {
    if (!o || !model_info(model_id)) return GUSTO_ERR_ARG;
    o->tf_lo = 1.0; o->tf_hi = 100.0;   // (placeholders: a caller knows its own range)
    o->rtol = 0.01;
    o->seed = model_id == GUSTO_DUBINS_CAR ? GUSTO_TFSEARCH_SEED_LINE : GUSTO_TFSEARCH_SEED_INCUMBENT;
    return GUSTO_OK;
}

int gusto_tfsearch_begin(gusto_handle h, int Bq, int K, const double* x_init, const double* glo, const double* ghi,
                         const double* tf_lo, const double* tf_hi, const gusto_tfsearch_opts* o) {
    const char* who = "gusto_tfsearch_begin";
    gusto_tfsearch_opts opts;
    std::vector<double> br;   // lo0 | hi0
    if (int rc = seed_enter(h, who, Bq, K, GUSTO_MAX_STARTS, "GUSTO_MAX_STARTS", {x_init, glo, ghi}, [&]() -> int {
            if (o) opts = *o;
            else gusto_default_tfsearch_opts(h->model_pub, &opts);
            if (!(opts.rtol >= 1e-6 && opts.rtol < 1)) return refuse(h, who, "rtol must lie in [1e-6, 1)");
            if (opts.seed != GUSTO_TFSEARCH_SEED_LINE && opts.seed != GUSTO_TFSEARCH_SEED_INCUMBENT) return refuse(h, who, "unknown seed");
            if (opts.seed == GUSTO_TFSEARCH_SEED_INCUMBENT && h->model_pub == GUSTO_DUBINS_CAR)
                return refuse(h, who, "DubinsCar: the speed is a constant of the model, nothing retimes (GUSTO_TFSEARCH_SEED_LINE)");
            br.resize(2 * (size_t)Bq);
            for (size_t i = 0, q = Bq; i < q; i++) {
                br[i] = tf_lo ? tf_lo[i] : opts.tf_lo;
                br[q + i] = tf_hi ? tf_hi[i] : opts.tf_hi;
                if (!bracket_ok(br[i], br[q + i])) return refuse(h, who, "need 0 < tf_lo < tf_hi < inf (query " + std::to_string(i) + ")");
            }
            return GUSTO_OK;
        }))
        return rc;
    const size_t n = h->n, m = h->m, N = h->N, q = Bq;
    const std::vector<double> in = pack_queries(q, n, x_init, glo, ghi, {{br.data(), 2 * q}});
    TfsearchState& S = h->tfsearch;
    S.have = false;
    HIPCHK(h, S.In.ensure(in.size())); HIPCHK(h, S.D.ensure(TF_ND * q)); HIPCHK(h, S.I.ensure(TI_NI * q));
    HIPCHK(h, S.Cand.ensure(q * K)); HIPCHK(h, S.X.ensure(q * N * n)); HIPCHK(h, S.U.ensure(q * N * m));
    HIPCHK(h, hipMemsetAsync(S.X, 0, sizeof(double) * q * N * n, h->stream));   // (the report's X, U before the first incumbent)
    HIPCHK(h, hipMemsetAsync(S.U, 0, sizeof(double) * q * N * m, h->stream));
    seed_set_B(h, q * K);
    S.K = K; S.Bq = Bq; S.round = 0; S.n_searching = Bq; S.seed = opts.seed; S.rtol = opts.rtol;
    HIPCHK(h, S.t0.record(h->stream));
    HIPCHK(h, hipMemcpyAsync(S.In, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, h->stream));
    const double* lo0 = query_dev(S.In, q, n).extra;
    hipLaunchKernelGGL(begin_kernel, dim3((h->B + 255) / 256), dim3(256), 0, h->stream, lo0, lo0 + q, S.D.get(), S.I.get(), S.Cand.get(), Bq, K);
    HIPCHK(h, hipGetLastError());
    if (int rc = launch_seed(h)) return rc;
    HIPCHK(h, S.t1.record(h->stream));
    if (int rc = gusto_problems_loaded(h, false)) return rc;   // (waits for the stream: `in` is read by then)
    HIPCHK(h, event_ms(S.t0, S.t1, &S.last_ms));
    S.solves_at = h->solves;
    S.have = true;
    return GUSTO_OK;
}

int gusto_tfsearch_update(gusto_handle h, const int* eligible) {
    const char* who = "gusto_tfsearch_update";
    if (int rc = search_enter(h, who)) return rc;
    TfsearchState& S = h->tfsearch;
    if (S.n_searching == 0) return refuse(h, who, "no query is still searching", GUSTO_ERR_STATE);
    if (!eligible && h->solves == S.solves_at)
        return refuse(h, who, "no gusto_solve since the last begin or update (the default eligibility reads its status)", GUSTO_ERR_STATE);
    const size_t B = h->B, q = S.Bq, nx = (size_t)h->N * h->n, nu = (size_t)h->N * h->m;
    HIPCHK(h, S.t0.record(h->stream));
    UpdateArgs A;
    A.elig = nullptr;
    if (eligible) {
        HIPCHK(h, S.Elig.ensure(B));
        HIPCHK(h, hipMemcpyAsync(S.Elig, eligible, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
        A.elig = S.Elig;
    }
    A.st_i = h->d_sti; A.Jt = h->d_Jt; A.tf = h->d_tf; A.X = h->d_X; A.U = h->d_U;
    A.D = S.D; A.cand = S.Cand; A.Xb = S.X; A.Ub = S.U; A.I = S.I;
    A.Bq = S.Bq; A.K = S.K; A.hist_cap = h->hist_cap; A.nx = (int)nx; A.nu = (int)nu; A.round = S.round; A.rtol = S.rtol;
    hipLaunchKernelGGL(update_kernel, dim3((unsigned)q), dim3(64), 0, h->stream, A);
    HIPCHK(h, hipGetLastError());
    if (int rc = launch_seed(h)) return rc;
    std::vector<int> st(q);
    HIPCHK(h, hipMemcpyAsync(st.data(), S.I.get() + TI_STATUS * q, sizeof(int) * q, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, S.t1.record(h->stream));
    if (int rc = gusto_problems_loaded(h, false)) return rc;   // (waits for the stream: `eligible` is read, `st` written by then)
    HIPCHK(h, event_ms(S.t0, S.t1, &S.last_ms));
    S.round++;
    S.solves_at = h->solves;
    S.have = true;
    std::vector<int> active(B);
    int searching = 0;
    for (size_t i = 0; i < q; i++) {
        const int on = (st[i] & TF_FINISHED) == 0;
        searching += on;
        for (int j = 0; j < S.K; j++) active[i * S.K + j] = on;
    }
    S.n_searching = searching;
    return searching == S.Bq ? GUSTO_OK : gusto_set_active(h, active.data());   // the done queries' problems: inactive
}

int gusto_get_tfsearch(gusto_handle h, gusto_tfsearch_report* out, int* round, int* n_searching) {
    if (int rc = search_enter(h, "gusto_get_tfsearch")) return rc;
    const TfsearchState& S = h->tfsearch;
    if (round) *round = S.round;
    if (n_searching) *n_searching = S.n_searching;
    if (!out) return GUSTO_OK;
    const size_t q = S.Bq, nx = (size_t)h->N * h->n, nu = (size_t)h->N * h->m;
    if (int rc = copy_out(h, out->status, S.I.get() + TI_STATUS * q, q)) return rc;
    if (int rc = copy_out(h, out->round_found, S.I.get() + TI_FOUND * q, q)) return rc;
    if (int rc = copy_out(h, out->n_eligible, S.I.get() + TI_NELIG * q, q)) return rc;
    if (int rc = copy_out(h, out->lo, S.D.get() + TF_LO * q, q)) return rc;
    if (int rc = copy_out(h, out->hi, S.D.get() + TF_HI * q, q)) return rc;
    if (int rc = copy_out(h, out->tf_best, S.D.get() + TF_BEST * q, q)) return rc;
    if (int rc = copy_out(h, out->J_best, S.D.get() + TF_J * q, q)) return rc;
    if (int rc = copy_out(h, out->cand, S.Cand.get(), q * S.K)) return rc;
    if (int rc = copy_out(h, out->X, S.X.get(), q * nx)) return rc;
    return copy_out(h, out->U, S.U.get(), q * nu);
}

int gusto_get_tfsearch_dev(gusto_handle h, const double** X_dev, const double** U_dev, const double** tf_best_dev) {
    if (int rc = search_enter(h, "gusto_get_tfsearch_dev")) return rc;
    const TfsearchState& S = h->tfsearch;
    if (X_dev) *X_dev = S.X;
    if (U_dev) *U_dev = S.U;
    if (tf_best_dev) *tf_best_dev = S.D.get() + TF_BEST * (size_t)S.Bq;
    return GUSTO_OK;
}

int gusto_last_tfsearch_ms(gusto_handle h, double* ms) {
    return stage_last_ms(h, &gusto_handle_s::tfsearch, ms, "gusto_last_tfsearch_ms", "the handle's problems were not set by gusto_tfsearch_begin");
}

}  // extern "C"
