// seed.hpp -- what a seeding stage starts from: the stages that turn Bq queries x K starts into the handle's B = Bq K problems
// (multistart.hip, trajlib.hip, replan.hip, roadmap.hip, tfsearch.hip, legs.hip).  On the device: the straight line of
// init_straightline_kernel (scp.hpp, which includes this header for it) as ONE expression, so that an unseeded start of every
// stage is that kernel's output bit for bit, the decode of a thread into (problem, knot, query, start), and the knot-0 tail
// that replicates a query into the handle's [B] arrays.  On the host, in the manner of post.hpp: the refusals every query entry
// begins with, the staging vector of the queries, the per-knot launch and the getter of a stage's GPU time.  A new seeding
// stage is a kernel body between knot_id() and seed_problem_tail(), a struct of its own in handle.hpp and a report.
#pragma once
#include <initializer_list>
#include <utility>

#include "post.hpp"

namespace gusto {

// center(goal), zeros elsewhere (freeflyer_se2.jl:97-111)
GD double goal_centre(double lo, double hi) { return (isfinite(lo) && isfinite(hi)) ? 0.5 * (lo + hi) : 0.0; }

// The straight line from a to the goal's centre at the LinRange parameter t = k / (N - 1): (1 - t) * a + t * xg, with the one
// fused multiply-add that the compiler made of it in every kernel that used to spell the sum out.  Which of the two products
// it fuses depends on the code around the sum, and the two choices round differently: written as a sum here, the seeds of
// every stage moved by an ulp.  The fma pins the rounding, whatever a kernel does around it.
GD double straight_line(double t, double a, double lo, double hi) {
    const double xg = goal_centre(lo, hi);
    return fma(t, xg, (1 - t) * a);
}

// a thread of a per-knot launch (launch_per_knot): knot k of problem b = q K + j, start j of query q; t of the knot
struct KnotId {
    int b, k, q, j;
    double t;
};
// false: the thread lies behind the last knot of the B problems
GD bool knot_id(int B, int K, int N, KnotId& id) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * N) return false;
    id.b = gid / N; id.k = gid % N; id.q = id.b / K; id.j = id.b % K;
    id.t = (double)id.k / (double)(N - 1);  // LinRange element: (1-t)*a + t*b
    return true;
}

// what every seed kernel writes: the handle's trajectories and its [B] arrays
struct SeedOut {
    double *X, *U, *x_init, *goal_lo, *goal_hi, *tf_b;
};
// the thread of knot 0 replicates its problem's inputs (rows of n doubles, and tf) into the handle's arrays
template <int MODEL> GD void seed_problem_tail(const SeedOut& O, int b, const double* xi, const double* lo, const double* hi, double tf) {
    constexpr int n = MT<MODEL>::n;
#pragma unroll
    for (int i = 0; i < n; i++) {
        O.x_init[(size_t)b * n + i] = xi[i];
        O.goal_lo[(size_t)b * n + i] = lo[i];
        O.goal_hi[(size_t)b * n + i] = hi[i];
    }
    O.tf_b[b] = tf;
}

// the queries as the kernels read them, carved out of one staged vector (pack_queries): [Bq][n] each, then the call's own
struct QueryDev {
    const double *xi, *glo, *ghi, *extra;
};

}  // namespace gusto

static inline gusto::SeedOut seed_out(gusto_handle h) { return {h->d_X, h->d_U, h->d_xinit, h->d_glo, h->d_ghi, h->d_tf}; }

// The arguments every query entry has: K in 1 .. k_max (k_name: the limit's name in the text), Bq >= 1 with Bq K problems that
// fit the handle, no null array.  GUSTO_ERR_ARG and the text in *err, the first of these that applies.  No device, no handle.
// cap_K > 0: an entry whose problems per query its own refusals decide (gusto_legs_begin: 1 or K) names the least count here,
// Bq cap_K problems must fit, and checks the count it takes itself.
static inline int query_args_host(int Bq, int K, int k_max, const char* k_name, int batch_cap, std::initializer_list<const void*> arrays,
                                  const char* who, std::string* err, int cap_K = 0) {
    const std::string w = std::string(who) + ": ";
    if (K < 1 || K > k_max) { *err = w + "K outside 1 .. " + k_name; return GUSTO_ERR_ARG; }
    if (cap_K > 0 && (Bq < 1 || (long long)Bq * cap_K > batch_cap)) {
        *err = w + "need Bq >= 1 and at least " + std::to_string(cap_K) + " problem(s) per query within batch_cap";
        return GUSTO_ERR_ARG;
    }
    if (cap_K <= 0 && (Bq < 1 || (long long)Bq * K > batch_cap)) { *err = w + "need Bq >= 1 and Bq K <= batch_cap"; return GUSTO_ERR_ARG; }
    for (const void* a : arrays)
        if (!a) { *err = w + "a null array"; return GUSTO_ERR_ARG; }
    return GUSTO_OK;
}
// ... behind the handle's own refusals; then `own()`, the refusals of the entry itself (it answers a GUSTO_* code), and only
// then the handle's device and its enqueued solve: nothing on the handle changes when a call is refused
template <class Own> static int seed_enter(gusto_handle h, const char* who, int Bq, int K, int k_max, const char* k_name,
                                           std::initializer_list<const void*> arrays, Own&& own, int cap_K = 0) {
    if (!h) return GUSTO_ERR_ARG;
    if (h->trajopt) return refuse(h, who, "TrajOpt handle (not supported)");
    if (int rc = query_args_host(Bq, K, k_max, k_name, h->batch_cap, arrays, who, &h->err, cap_K)) return rc;
    if (int rc = own()) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return gusto_complete(h);
}

// x_init | goal_lo | goal_hi | extra ...: the q queries of n states in one vector, one copy to the device
static inline std::vector<double> pack_queries(size_t q, size_t n, const double* x_init, const double* glo, const double* ghi,
                                               std::initializer_list<std::pair<const double*, size_t>> extra) {
    size_t total = 3 * q * n;
    for (const auto& e : extra) total += e.second;
    std::vector<double> in(total);
    double* at = in.data();
    for (const double* src : {x_init, glo, ghi}) { memcpy(at, src, sizeof(double) * q * n); at += q * n; }
    for (const auto& e : extra) { memcpy(at, e.first, sizeof(double) * e.second); at += e.second; }
    return in;
}
// ... where its parts lie once it is in `In`
static inline gusto::QueryDev query_dev(const double* In, size_t q, size_t n) { return {In, In + q * n, In + 2 * q * n, In + 3 * q * n}; }

// every problem of the handle is set again, B of them (a latched scheduler error ends here)
static inline void seed_set_B(gusto_handle h, size_t B) {
    h->sched_err = 0;
    h->B = (int)B;
}

// a thread per (problem, knot) of the handle's B problems; kernel_of(std::integral_constant<int, MODEL>{}) is the kernel
template <class Args, class Pick> static int launch_per_knot(gusto_handle h, const Args& A, Pick&& kernel_of) {
    const int tot = h->B * h->N;
    return for_model(h->model_pub, [&](auto M) -> int {
        hipLaunchKernelGGL(kernel_of(M), dim3((tot + 255) / 256), dim3(256), 0, h->stream, A);
        HIPCHK(h, hipGetLastError());
        return GUSTO_OK;
    });
}

// gusto_last_*_ms of a stage struct with `have` and `last_ms`; need: what to call first
template <class S> static int stage_last_ms(gusto_handle h, S gusto_handle_s::*stage, double* ms, const char* who, const char* need) {
    if (!h || !ms) return GUSTO_ERR_ARG;
    if (!(h->*stage).have) return refuse(h, who, need, GUSTO_ERR_STATE);
    *ms = (h->*stage).last_ms;
    return GUSTO_OK;
}
