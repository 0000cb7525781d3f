// multistart.hip -- multi-start solves: a fan of detour starts per query, generated on the device, and the best start of every
// query, selected and gathered on the device.  No counterpart in the reference, whose init_traj_straightline
// (freeflyer_se2.jl:97-111) is the start with a zero offset; the definitions are stated in include/gusto_hip.h.
//   gusto_set_problems_multistart   Bq queries x K starts become the B = Bq K problems of the handle, problem q K + j = start j
//                                   of query q
//   gusto_select_best / gusto_get_best / gusto_get_best_dev   per query the eligible start with the smallest score
// Fan kernel: a thread per (problem, knot), the shape of init_straightline_kernel (scp.hpp).  A thread derives its query's
// frame from the [Bq] inputs -- a handful of flops, cheaper than a second launch and a frame buffer -- and writes its knot's n
// states and m controls; the thread of knot 1 also writes the problem's replicated x_init, goal_lo, goal_hi and tf.
// Consecutive threads write consecutive knots, so a wavefront covers one contiguous range of X and of U.  The straight line
// is straight_line() of seed.hpp, the one init_straightline_kernel evaluates: a start with a zero offset is that kernel's output
// bit for bit, and so are the entries behind the workspace of every start.
// Select kernel: one wavefront per query, lane j = start j (K <= 64).  A wave_reduce minimum over the eligible scores, a
// second one over the lanes that hold it picks the lowest lane (the idiom of obstacle_margin in lincov.hip), then the whole
// wave copies the winner's N n and N m doubles, lane-consecutive, into the compact buffers, or writes zeros.  No atomics,
// nothing crosses a query: a query's report is the same bit for bit in any batch.
#include <hip/hip_runtime.h>

#include "seed.hpp"

using namespace gusto;

namespace {

struct FanArgs {
    QueryDev Q;   // the queries; extra: tf [Bq], then the offsets [K][2]
    SeedOut out;
    int B, Bq, K, N;
};

template <int MODEL> __global__ void fan_kernel(const FanArgs A) {
    using T = MT<MODEL>;
    constexpr int n = T::n, m = T::m, WS = T::WS;
    KnotId id;
    if (!knot_id(A.B, A.K, A.N, id)) return;
    const int b = id.b, k = id.k, j = id.j;
    const double t = id.t;
    const size_t qn = (size_t)id.q * n;   // the query's row of xi, glo, ghi
    const double *tf = A.Q.extra, *fan = tf + A.Bq;
    double* Xo = A.out.X + ((size_t)b * A.N + k) * n;
    double x[WS], pi[WS], pg[WS];   // the workspace entries; the others are the line's and go out at once
#pragma unroll
    for (int i = 0; i < n; i++) {
        const double xl = straight_line(t, A.Q.xi[qn + i], A.Q.glo[qn + i], A.Q.ghi[qn + i]);
        if (i < WS) { x[i] = xl; pi[i] = A.Q.xi[qn + i]; pg[i] = goal_centre(A.Q.glo[qn + i], A.Q.ghi[qn + i]); }
        else Xo[i] = xl;
    }
    const double a2 = fan[2 * j], a3 = WS == 3 ? fan[2 * j + 1] : 0.0;   // (a3 is ignored in the plane)
    if (a2 != 0.0 || a3 != 0.0) {
        double d[WS], e1[WS], w[WS];
#pragma unroll
        for (int i = 0; i < WS; i++) d[i] = pg[i] - pi[i];
        double L;
        if constexpr (WS == 2) L = hypot(d[0], d[1]);
        else L = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
#pragma unroll
        for (int i = 0; i < WS; i++) e1[i] = L == 0.0 ? (i == 0 ? 1.0 : 0.0) : d[i] / L;
        if constexpr (WS == 2) {
            w[0] = a2 * -e1[1]; w[1] = a2 * e1[0];
        } else {
            const double hh = hypot(e1[0], e1[1]);
            double e2[3] = {1.0, 0.0, 0.0};
            if (hh > 1e-9) { e2[0] = -e1[1] / hh; e2[1] = e1[0] / hh; }
            const double e3[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
#pragma unroll
            for (int i = 0; i < 3; i++) w[i] = a2 * e2[i] + a3 * e3[i];
        }
        const double tent = 1.0 - fabs(2.0 * t - 1.0);
#pragma unroll
        for (int i = 0; i < WS; i++) x[i] += tent * w[i];
    }
#pragma unroll
    for (int i = 0; i < WS; i++) Xo[i] = x[i];
#pragma unroll
    for (int i = 0; i < m; i++) A.out.U[((size_t)b * A.N + k) * m + i] = 0.0;
    if (k == 0) seed_problem_tail<MODEL>(A.out, b, A.Q.xi + qn, A.Q.glo + qn, A.Q.ghi + qn, tf[id.q]);
}

struct SelectArgs {
    const double* score;   // [B], null: the last true cost
    const int* elig;       // [B], null: converged && successful
    const int* st_i;       // the handle's status words [B][ST_NI]
    const double* Jt;      // its J_true history [B][hist_cap]
    const double *X, *U;   // its trajectories, rows of nx = N n and nu = N m doubles
    int K, hist_cap, nx, nu;
    int *winner, *winner_problem, *n_eligible;
    double *best, *Xb, *Ub;
};

// (64 lanes: every lane takes part in the reductions, the starts are the lanes below K)
__global__ void __launch_bounds__(64) select_kernel(const SelectArgs A) {
    const int q = blockIdx.x, lane = threadIdx.x;
    const size_t b = (size_t)q * A.K + lane;
    bool el = false;
    double s = NAN;
    if (lane < A.K) {
        const int* st = A.st_i + b * ST_NI;
        el = A.elig ? A.elig[b] != 0 : (st[ST_CONV] != 0 && st[ST_SUCC] != 0);
        const int nJ = st[ST_NJ];
        s = A.score ? A.score[b] : (nJ > 0 ? A.Jt[b * A.hist_cap + nJ - 1] : NAN);
    }
    const bool cand = el && !isnan(s);   // a NaN never wins
    const double smin = wave_reduce(cand ? s : INFINITY, OpMin());
    const int w = (int)wave_reduce((cand && s == smin) ? (double)lane : 64.0, OpMin());   // ties: the lowest start
    const int ne = (int)wave_reduce(el ? 1.0 : 0.0, OpSum());
    const bool won = w < 64;
    if (lane == (won ? w : 0)) {
        A.winner[q] = won ? w : -1;
        A.winner_problem[q] = won ? q * A.K + w : -1;
        A.n_eligible[q] = ne;
        A.best[q] = won ? s : INFINITY;
    }
    const double* Xw = A.X + ((size_t)q * A.K + (won ? w : 0)) * A.nx;
    const double* Uw = A.U + ((size_t)q * A.K + (won ? w : 0)) * A.nu;
    for (int e = lane; e < A.nx; e += 64) A.Xb[(size_t)q * A.nx + e] = won ? Xw[e] : 0.0;
    for (int e = lane; e < A.nu; e += 64) A.Ub[(size_t)q * A.nu + e] = won ? Uw[e] : 0.0;
}

// the refusals of the two getters, then the handle's device and its enqueued solve
int best_enter(gusto_handle h, const char* who) {
    if (int rc = post_enter(h, who, nullptr, nullptr)) return rc;
    if (!h->select.have) { h->err = std::string(who) + ": call gusto_select_best first"; return GUSTO_ERR_STATE; }
    return GUSTO_OK;
}

}  // namespace

extern "C" {

int gusto_set_problems_multistart(gusto_handle h, int Bq, int K, const double* x_init, const double* glo, const double* ghi,
                                  const double* tf, const double* fan) {
    const char* who = "gusto_set_problems_multistart";
    if (int rc = seed_enter(h, who, Bq, K, GUSTO_MAX_STARTS, "GUSTO_MAX_STARTS", {x_init, glo, ghi, tf, fan}, [&]() -> int {
            for (int i = 0; i < 2 * K; i++)
                if (!(fabs(fan[i]) < INFINITY)) return refuse(h, who, "fan must be finite (start " + std::to_string(i / 2) + ")");
            return GUSTO_OK;
        }))
        return rc;
    const std::vector<double> in = pack_queries(Bq, h->n, x_init, glo, ghi, {{tf, (size_t)Bq}, {fan, 2 * (size_t)K}});
    SelectState& S = h->select;
    HIPCHK(h, S.In.ensure(in.size()));
    seed_set_B(h, (size_t)Bq * K);
    HIPCHK(h, hipMemcpyAsync(S.In, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, h->stream));
    const FanArgs A{query_dev(S.In, Bq, h->n), seed_out(h), h->B, Bq, K, h->N};
    if (int rc = launch_per_knot(h, A, [](auto M) { return fan_kernel<decltype(M)::value>; })) return rc;
    return gusto_problems_loaded(h, false);   // (waits for the stream: `in` is read by then)
}

int gusto_select_best(gusto_handle h, int K, const double* score, const int* eligible) {
    const char* who = "gusto_select_best";
    if (int rc = post_enter(h, who, nullptr, nullptr)) return rc;
    if (K < 1 || K > GUSTO_MAX_STARTS || h->B % K != 0) return refuse(h, who, "K must lie in 1 .. GUSTO_MAX_STARTS and divide the handle's B");
    SelectState& S = h->select;
    S.have = false;
    const size_t B = h->B, Bq = B / K, nx = (size_t)h->N * h->n, nu = (size_t)h->N * h->m;
    HIPCHK(h, S.Rep.ensure(3 * Bq)); HIPCHK(h, S.Best.ensure(Bq)); HIPCHK(h, S.X.ensure(Bq * nx)); HIPCHK(h, S.U.ensure(Bq * nu));
    SelectArgs A;
    A.score = nullptr; A.elig = nullptr;
    if (score) {
        HIPCHK(h, S.Score.ensure(B));
        HIPCHK(h, hipMemcpyAsync(S.Score, score, sizeof(double) * B, hipMemcpyHostToDevice, h->stream));
        A.score = S.Score;
    }
    if (eligible) {
        HIPCHK(h, S.Elig.ensure(B));
        HIPCHK(h, hipMemcpyAsync(S.Elig, eligible, sizeof(int) * B, hipMemcpyHostToDevice, h->stream));
        A.elig = S.Elig;
    }
    A.st_i = h->d_sti; A.Jt = h->d_Jt; A.X = h->d_X; A.U = h->d_U;
    A.K = K; A.hist_cap = h->hist_cap; A.nx = (int)nx; A.nu = (int)nu;
    A.winner = S.Rep; A.winner_problem = S.Rep + Bq; A.n_eligible = S.Rep + 2 * Bq;
    A.best = S.Best; A.Xb = S.X; A.Ub = S.U;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)Bq), dim3(64), 0, h->stream, A);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipStreamSynchronize(h->stream));
    S.K = K; S.Bq = (int)Bq; S.have = true;
    return GUSTO_OK;
}

int gusto_get_best(gusto_handle h, gusto_best_report* out) {
    if (int rc = best_enter(h, "gusto_get_best")) return rc;
    if (!out) return GUSTO_OK;
    const SelectState& S = h->select;
    const size_t Bq = S.Bq, nx = (size_t)h->N * h->n, nu = (size_t)h->N * h->m;
    if (int rc = copy_out(h, out->winner, S.Rep.get(), Bq)) return rc;
    if (int rc = copy_out(h, out->winner_problem, S.Rep.get() + Bq, Bq)) return rc;
    if (int rc = copy_out(h, out->n_eligible, S.Rep.get() + 2 * Bq, Bq)) return rc;
    if (int rc = copy_out(h, out->best_score, S.Best.get(), Bq)) return rc;
    if (int rc = copy_out(h, out->X, S.X.get(), Bq * nx)) return rc;
    return copy_out(h, out->U, S.U.get(), Bq * nu);
}

int gusto_get_best_dev(gusto_handle h, const double** X_dev, const double** U_dev, const int** winner_problem_dev) {
    if (int rc = best_enter(h, "gusto_get_best_dev")) return rc;
    if (X_dev) *X_dev = h->select.X;
    if (U_dev) *U_dev = h->select.U;
    if (winner_problem_dev) *winner_problem_dev = h->select.Rep + h->select.Bq;
    return GUSTO_OK;
}

}  // extern "C"
