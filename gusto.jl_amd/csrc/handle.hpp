// handle.hpp -- the opaque gusto_handle: its owned device memory, the model table and the per-model launch operations
// (one translation unit per model).
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "common.hpp"

// Device memory owned by the handle: freed when the handle goes, whatever entry point allocated it.  count() is the number
// of elements asked for (0 while empty); a count of 0 still allocates one element, so get() is never null after a success.
// A failed allocation hands the hipError_t back (HIPCHK) and leaves the buffer empty.
template <class T> class __attribute__((visibility("hidden"))) DevBuf {
    T* p_ = nullptr;
    size_t n_ = 0;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), n_(std::exchange(o.n_, 0)) {}   // (move-only: no copies)
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); n_ = std::exchange(o.n_, 0); }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    // allocates once: a buffer that holds memory already is left as it is
    hipError_t alloc(size_t count) {
        if (p_) return hipSuccess;
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, (count ? count : 1) * sizeof(T));
        if (e == hipSuccess) { p_ = static_cast<T*>(q); n_ = count; }
        return e;
    }
    // grow-only: a buffer too small is freed and allocated anew (its contents are not kept)
    hipError_t ensure(size_t count) {
        if (p_ && count <= n_) return hipSuccess;
        reset();
        return alloc(count);
    }
    // ensure(), and zeros (enqueued on `s`) whenever that (re)allocated: a buffer large enough keeps its contents
    hipError_t ensure_zeroed(size_t count, hipStream_t s) {
        if (p_ && count <= n_) return hipSuccess;
        const hipError_t e = ensure(count);
        return e != hipSuccess ? e : hipMemsetAsync(p_, 0, sizeof(T) * count, s);
    }
    T* get() const { return p_; }
    operator T*() const { return p_; }
    size_t count() const { return n_; }
};

// an event owned by the handle; create() is lazy and idempotent
struct __attribute__((visibility("hidden"))) DevEvent {
    hipEvent_t e = nullptr;
    DevEvent() = default;
    DevEvent(const DevEvent&) = delete;
    ~DevEvent() { if (e) (void)hipEventDestroy(e); }
    hipError_t create(unsigned flags = hipEventDefault) { return e ? hipSuccess : hipEventCreateWithFlags(&e, flags); }
    operator hipEvent_t() const { return e; }
    hipError_t record(hipStream_t s) { const hipError_t c = create(); return c != hipSuccess ? c : hipEventRecord(e, s); }
};
// a timer on a stream: from.record() (which creates it the first time), the launches, to.record(), hipStreamSynchronize, this
static inline hipError_t event_ms(const DevEvent& from, const DevEvent& to, double* ms) {
    float f = 0;
    const hipError_t e = hipEventElapsedTime(&f, from, to);
    if (e == hipSuccess) *ms = f;
    return e;
}

// What the host side knows about a model, indexed by the public gusto_model_id: state and control dimensions, the internal id
// of its TrajOpt variant (common.hpp: GUSTO_TO_*; -1 = none), whether it has keep-out sets and a shooting ODE.
struct ModelInfo { int n, m, trajopt_variant; bool has_obs, has_shoot; };
template <int MODEL> constexpr ModelInfo model_row(int trajopt_variant, bool has_shoot) {
    return {gusto::MT<MODEL>::n, gusto::MT<MODEL>::m, trajopt_variant, gusto::MT<MODEL>::HAS_OBS, has_shoot};
}
constexpr ModelInfo MODEL_TABLE[] = {
    model_row<GUSTO_FREEFLYER_SE2>(gusto::GUSTO_TO_FREEFLYER_SE2, false),
    model_row<GUSTO_DUBINS_CAR>(-1, true),
    model_row<GUSTO_ASTROBEE_SE3>(gusto::GUSTO_TO_ASTROBEE_SE3, false),
    model_row<GUSTO_ASTROBEE_SE3_MANIFOLD>(gusto::GUSTO_TO_ASTROBEE_SE3_MANIFOLD, true),
};
static_assert(GUSTO_FREEFLYER_SE2 == 0 && GUSTO_DUBINS_CAR == 1 && GUSTO_ASTROBEE_SE3 == 2 && GUSTO_ASTROBEE_SE3_MANIFOLD == 3,
              "MODEL_TABLE is indexed by gusto_model_id");
// null: no such model
static inline const ModelInfo* model_info(int model) {
    return model >= 0 && model < (int)(sizeof(MODEL_TABLE) / sizeof(MODEL_TABLE[0])) ? &MODEL_TABLE[model] : nullptr;
}

// What the post-solve stages (post.hpp) keep on the handle; invalidate() is gusto_set_problems: the buffers stay.
// Indirect shooting (shoot.hip): trajectories, converged costates, seeds, residuals, status, Newton iterations
struct __attribute__((visibility("hidden"))) ShootState {
    DevBuf<double> X, U, P, P0, Res;
    DevBuf<double> Xt, Ut;   // knot-major staging of the shooting trajectories ([N][n][B])
    DevBuf<int> St, It, List;
    bool have = false;
    void invalidate() { have = false; }
};
// Verification (verify.hip): the report ([4][batch_cap] ints: collision_free, first_knot, min_dense_sample, nfull; [5][batch_cap]
// doubles: first_dist, min_dist_knots, dyn_defect_l1, min_dist_dense, max_gap), copies of a caller's X / U, the dense
// trajectories of gusto_interpolate ([batch_cap][dense_rows][n], [batch_cap][dense_rows - 1][m])
struct __attribute__((visibility("hidden"))) VerifyState {
    DevBuf<int> I;
    DevBuf<double> D, X, U, Xf, Uf;
    int dense_rows = 0;
    bool have = false, have_dense = false;
    DevEvent t0, t1;
    double last_ms = 0.0;
    void invalidate() { have = false; have_dense = false; }
};
// Time-varying LQR gains (tvlqr.hip), B the batch of the call that allocated them: [B][N - 1][n][n + m] rows of [Ad | Bd],
// [B][N - 1][m][n] gains, [B][n][n] P of knot 1, [B][N][n][n] P of every knot (first call with store_P only), [2][B] status and
// fail_knot, copies of a caller's X / U.  A later call with a larger batch grows them, contents discarded.  `mid` is recorded
// between the two launches (gusto_dev_tvlqr).  have_Pall outlives invalidate(): the next gusto_tvlqr resets it.  dt_min, nstep:
// the roll-out options of the last call, which its [Ad | Bd] belong to (gusto_lincov_disturbed rolls out with the same)
struct __attribute__((visibility("hidden"))) TvlqrState {
    DevBuf<double> AB, K, P1, Pall, X, U;
    DevBuf<int> St;
    bool have = false, store_P = false, have_Pall = false;
    double dt_min = 0.0;
    int nstep = 0, nstep_max = 0;   // nstep_max: the largest Nstep_b of that call (the row count of gusto_lincov_dense)
    DevEvent t0, mid, t1;
    double last_ms = 0.0, lin_ms = 0.0, ric_ms = 0.0;
    void invalidate() { have = false; }
};

// Closed-loop roll-outs (simulate.hip), S the n_samples of the last call: per sample [batch_cap][S] the smallest distance (D),
// its dense index and the flags (I: [2][batch_cap][S]), [batch_cap][S][n] the final state and the largest deviation per state
// (Xfin, Dev); the per-problem report (RI: [5][batch_cap] n_free, n_finite, n_clipped, worst_sample, worst_dense_sample; RD:
// [batch_cap] min_dist, then [batch_cap][n] max_dev, [batch_cap][n] max_final_dev); the knots [batch_cap][N][S][n] (first call
// with store_knots only); copies of a caller's X / U / K / pert.  gusto_simulate_disturbed: Plant [batch_cap][S][GUSTO_NPLANT],
// the plant scalars the kernel used; PlantIn and White, the copies of a caller's plant and noise [batch_cap][N - 1][S][m] (they
// exist only once one was supplied); disturbed: the last call was a disturbed one
struct __attribute__((visibility("hidden"))) SimulateState {
    DevBuf<double> D, Xfin, Dev, RD, Knots, X, U, K, Pert, Plant, PlantIn, White;
    DevBuf<int> I, RI;
    int S = 0;
    bool have = false, have_knots = false, disturbed = false;
    DevEvent t0, t1;
    double last_ms = 0.0;
    void invalidate() { have = false; have_knots = false; disturbed = false; }
};

// Linear covariance analysis (lincov.hip): I [6][batch_cap] status, fail_knot, obs_knot, obs_pair, ctl_knot, ctl_entry; D
// [3][batch_cap] min_z_obs, p_collision_bound, min_z_ctl; Sx [batch_cap][N][n], Su [batch_cap][N - 1][m], Z [batch_cap][N] the
// per-knot rows; Sxx [batch_cap][N][n][n] (first call with store_S only); copies of a caller's X / U / K / S0.  have_Sxx
// outlives invalidate(): the next gusto_lincov resets it.  gusto_lincov_disturbed: Cd [batch_cap][N - 1][n][GUSTO_NPLANT], Sxt
// [batch_cap][N][n][GUSTO_NPLANT] (first call with store_S only), Sth the copy of a caller's [batch_cap][GUSTO_NPLANT]
// [GUSTO_NPLANT]; plant: the last call was a disturbed one.  gusto_lincov_dense: Srow [batch_cap][N][n][n + m + GUSTO_NPLANT] the
// x-rows of S_k and Sbt [batch_cap][m + GUSTO_NPLANT][m + GUSTO_NPLANT] its constant block, from the knot pass to the dense one;
// Zint [batch_cap][N - 1] and Jint [2][batch_cap][N - 1] the minimum, sample and pair of every interval; DI [3][batch_cap] nfull,
// dense_sample, dense_pair; DD [batch_cap] min_z_dense; with store_dense Zd, Pd [batch_cap][dense_rows] and Spos
// [batch_cap][dense_rows][dense_nsp = WS WS].  dense: the last call was a dense one; have_dense: DI, DD belong to these problems
// and to dense_rows; have_dense_rows: so do Zd, Pd, Spos
struct __attribute__((visibility("hidden"))) LincovState {
    DevBuf<double> D, Sx, Su, Z, Sxx, X, U, K, S0, Cd, Sxt, Sth, Srow, Sbt, Zint, DD, Zd, Spos;
    DevBuf<int> I, Jint, DI, Pd;
    bool have = false, store_S = false, have_Sxx = false, plant = false;
    bool dense = false, store_dense = false, have_dense = false, have_dense_rows = false;
    bool staged = false;   // the last call read a caller's X, U (the copies in X, U), not the handle's own (gusto_tighten_env)
    size_t dense_rows = 0, dense_nsp = 0;
    DevEvent t0, t1;
    double last_ms = 0.0;
    void invalidate() { have = false; plant = false; dense = false; have_dense = false; have_dense_rows = false; }
};

// Multi-start solves (multistart.hip).  In: the [Bq] inputs of gusto_set_problems_multistart as the fan kernel reads them
// (x_init, goal_lo, goal_hi [Bq][n] each, tf [Bq], fan [K][2]).  gusto_select_best with K starts per query, Bq = B / K: Score,
// Elig [B] the copies of a caller's arrays; Rep [3][Bq] winner, winner_problem, n_eligible; Best [Bq] the winners' scores; X
// [Bq][N][n], U [Bq][N][m] their trajectories
struct __attribute__((visibility("hidden"))) SelectState {
    DevBuf<double> In, Score, Best, X, U;
    DevBuf<int> Elig, Rep;
    int K = 0, Bq = 0;
    bool have = false;
    void invalidate() { have = false; }
};

// Trajectory library (trajlib.hip), on the handle: In the [Bq] inputs of gusto_set_problems_trajlib as its kernels read them
// (x_init, goal_lo, goal_hi [Bq][n] each, tf [Bq]) and Tag their tags [Bq]; Entry, Dist [B] the seeds, Found [Bq]; Mask [2][B]
// the copies of mask and tag of gusto_trajlib_add
struct __attribute__((visibility("hidden"))) TrajlibState {
    DevBuf<double> In, Dist;
    DevBuf<int> Tag, Entry, Found, Mask;
    int K = 0, Bq = 0;
    bool have = false;
    DevEvent t0, mid, t1;   // `mid` is recorded between the two launches (gusto_dev_trajlib)
    double last_ms = 0.0, search_ms = 0.0, retarget_ms = 0.0;
    void invalidate() { have = false; }
};

// Receding-horizon replanning (replan.hip): In the HOST inputs of the call as its kernel reads them (tau [B], x_now [B][n], then
// the caller's goal_lo, goal_hi [B][n] each when given) and Meta [2][B] seeded and source problem; G (tf [Bs], goal_lo, goal_hi
// [Bs][n]) and Xs, Us the staging copies of the source's rows when source and destination share memory; Xnow [B][n] the states
// gusto_set_problems_replan_knots gathers (Meta holds its knots meanwhile).  seeded, tau, x_now: what the last call used, on the
// host (gusto_get_replan)
struct __attribute__((visibility("hidden"))) ReplanState {
    DevBuf<double> In, G, Xs, Us, Xnow;
    DevBuf<int> Meta;
    std::vector<int> seeded;
    std::vector<double> tau, x_now;
    bool have = false;
    DevEvent t0, t1;
    double last_ms = 0.0;
    void invalidate() { have = false; }
};

// Risk-tightened keep-out sets (tighten.hip): Bbox, Bsph the caller's base tables of the last call and Rec [2][batch_cap][4] the
// (box offset, n_box, sphere offset, n_sph) records of every problem, in the base tables and in the tightened ones; M
// [batch_cap][64] the margins, which outlive gusto_set_problems* (mem: they belong to mem_B problems with the counts cnt
// [mem_B][2]; gusto_set_env / gusto_set_env_batch end that); the report I [5][batch_cap] status, knot, pair, n_grown, blocked and
// D [2][batch_cap] min_z_base, max_margin of the last call on these problems (have), n_obs_max its largest component count
struct __attribute__((visibility("hidden"))) TightenState {
    DevBuf<double> Bbox, Bsph, M, D;
    DevBuf<int> Rec, I;
    std::vector<int> cnt;
    int mem_B = 0, n_obs_max = 0;
    bool have = false, mem = false;
    DevEvent t0, t1;
    double last_ms = 0.0;
    void invalidate() { have = false; }
    void forget() { mem = false; mem_B = 0; cnt.clear(); }
};

// Roadmap seeds (roadmap.hip): In the [Bq] inputs of gusto_set_problems_roadmap as its kernels read them (x_init, goal_lo,
// goal_hi [Bq][n] each, tf [Bq]) and Rec [n_env][4] the (box offset, n_box, sphere offset, n_sph) record of every query's set in
// the handle's tables; the graph of every set, Ve rows sized from the call's largest component count: Nodes [n_env][Ve][WS], Dead
// [n_env][Ve], Vis [n_env][Ve][ceil(Ve / 64)]; the report I ([B] status, [B] n_via, [B][16] via, [B][8] banned), Len [B] and the
// polylines Pts [B][18][3] the seed kernel resamples.  stage_ms: graph (with the copies), search, seed
struct __attribute__((visibility("hidden"))) RoadmapState {
    DevBuf<double> In, Nodes, Len, Pts;
    DevBuf<int> Rec, Dead, I;
    DevBuf<unsigned long long> Vis;
    int K = 0, Bq = 0;
    bool have = false;
    DevEvent t0, t1, t2, t3;
    double last_ms = 0.0, stage_ms[3] = {0.0, 0.0, 0.0};
    void invalidate() { have = false; }
};

// Final-time search (tfsearch.hip), Bq queries x K candidates: In the queries as the seed kernel reads them (x_init, goal_lo,
// goal_hi [Bq][n] each); D [6][Bq] lo, hi, lo0, hi0, tf_best, J_best; I [4][Bq] status, round_found, n_eligible, parked (the
// query was done before the last update: its problems are left alone); Cand [Bq][K]; X [Bq][N][n], U [Bq][N][m] the incumbents;
// Elig [B] the copy of a caller's eligibility.  round: updates so far; n_searching: queries neither NONE nor DONE; solves_at: the
// handle's count of solve calls at the last begin or update.  have: gusto_problems_loaded ends it, tfsearch.hip sets it again
// behind its own call
struct __attribute__((visibility("hidden"))) TfsearchState {
    DevBuf<double> In, D, Cand, X, U;
    DevBuf<int> I, Elig;
    int K = 0, Bq = 0, round = 0, n_searching = 0, seed = 0;
    double rtol = 0.0;
    unsigned long long solves_at = 0;
    bool have = false;
    DevEvent t0, t1;
    double last_ms = 0.0;
    void invalidate() { have = false; }
};

// Goal timeline (legs.hip), Bq queries x L legs: In the timeline as the kernels read it (x_init [Bq][n], goal_lo, goal_hi
// [Bq][L][n], t_goal [Bq][L]) and NL the leg counts [Bq]; I: [4][Bq] status, failed_leg, n_done and the copy of the status words
// an advance reads (it writes the others), then [4][Bq][L] iterations, converged, successful, stop_reason; D: [Bq] J_total, then
// [3][Bq][L] J, gap, arrive; the joined X [Bq][Nj][n], U [Bq][Nj][m], T [Bq][Nj], Nj = L (N - 1) + 1; Xs the staging copy of the
// handle's X a SEQUENTIAL advance reads; Elig [B] the copy of a caller's eligibility.  mode: SEQUENTIAL or PARALLEL, never AUTO;
// round: advances so far; n_flying; solves_at: the handle's count of solve calls at the last begin or advance.  have:
// gusto_problems_loaded ends it, legs.hip sets it again behind its own call
struct __attribute__((visibility("hidden"))) LegsState {
    DevBuf<double> In, D, X, U, T, Xs;
    DevBuf<int> NL, I, Elig;
    int Bq = 0, L = 0, mode = 0, round = 0, n_flying = 0;
    unsigned long long solves_at = 0;
    bool have = false;
    DevEvent t0, t1;
    double last_ms = 0.0;
    void invalidate() { have = false; }
};

// Fleet coordination (fleet.hip), F fleets x R robots of the last call: Q [B][Jmax][WS] the tracks on the fleet clock, Box [B][2 WS]
// their bounding boxes (lo, hi), J [B] the sample counts and Fin [B] whether a track is finite; Ord, Elig, Sig [B] the copies of a
// caller's order, eligibility and shifts; Sch the last schedule's rows ([3][B] status, sigma, blocker); the report I ([5][B] status,
// delay_steps, blocker, partner, step; [F][R][R] pair_step; [4][F] n_scheduled, n_blocked, n_conflicts, makespan_steps) and D ([2][B]
// delay, min_sep; [F][R][R] pair_min_sep; [F] fleet_min_sep).  have: a report belongs to these problems; have_sched: so does Sch,
// made on the clock step sched_dt.  stage_ms: track, schedule, separation
struct __attribute__((visibility("hidden"))) FleetState {
    DevBuf<double> Q, Box, D;
    DevBuf<int> J, Fin, Ord, Elig, Sig, Sch, I;
    int F = 0, R = 0, Jmax = 0, ws = 0;
    double sched_dt = 0.0;
    bool have = false, have_sched = false;
    DevEvent t0, t1, t2, t3, t4;
    double last_ms = 0.0, stage_ms[3] = {0.0, 0.0, 0.0};
    void invalidate() { have = false; have_sched = false; }
};

// The library itself: `count` of `cap` entries on `device`, entry e at row e of xi, c [cap][n], tf, tag [cap], X [cap][N][n], U
// [cap][N][m].  The features are the F positive-weight terms of the distance, in its order of summation: term f has the weight
// w[f] and reads entry fmap[f] & 15 of x_init (fmap[f] >> 4 == 0), of the goal centre (1) or tf (2).  Feat is feature-major,
// [F][cap]: consecutive lanes read consecutive entries of one feature.
constexpr int TRAJLIB_MAX_F = 2 * GUSTO_MAXN + 1;
struct gusto_trajlib_s {
    int model = 0, n = 0, m = 0, N = 0, cap = 0, device = 0, count = 0, F = 0, lds_tile = 1;
    int fmap[TRAJLIB_MAX_F] = {0};
    double w[TRAJLIB_MAX_F] = {0};
    DevBuf<double> xi, c, tf, X, U, Feat;
    DevBuf<int> tag;
    std::string err;
    __attribute__((visibility("hidden"))) ~gusto_trajlib_s() = default;
};

struct gusto_handle_s {
    int model = 0, n = 0, m = 0, N = 0, batch_cap = 0, hist_cap = 0, device = 0, B = 0;
    // TrajOpt handles (gusto_create_trajopt): `model` is the internal variant (common.hpp: GUSTO_TO_*), `m` its control
    // dimension u_dim + x_dim (u | defect); the C ABI moves U with the model's u_dim columns, `m_pub`
    bool trajopt = false;
    int m_pub = 0, model_pub = 0;
    gusto_trajopt_params tp{};
    DevBuf<double> d_to_mu, d_to_xtol, d_to_ftol, d_to_ctol;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    gusto_scp_params sp{};
    gusto_model_params mp{};
    gusto_ipm_opts io{};
    int n_box = 0, n_sph = 0;
    DevBuf<double> d_box, d_sph;
    // gusto_set_env_batch: one keep-out set per problem -- d_box / d_sph hold the concatenated tables, d_env the
    // (box offset, n_box, sphere offset, n_sph) record of every problem, env_B their number, n_obs_max the largest count
    DevBuf<int> d_env;
    int env_B = 0, n_obs_max = 0;
    DevBuf<double> d_X, d_U, d_xinit, d_glo, d_ghi, d_tf;
    DevBuf<int> d_sti;
    DevBuf<double> d_std, d_Jt, d_Jf, d_conv, d_Delta, d_omega, d_rho;
    DevBuf<int> d_acc, d_scp, d_sol, d_tr, d_cvx, d_ipm;
    DevBuf<double> d_ws;       // interior point workspaces, one per resident workgroup (grown by the launches)
    DevBuf<long long> d_prof;
    DevBuf<double> d_subD, d_subW, d_subT, d_subX, d_subU, d_subObj;
    DevBuf<int> d_subSt, d_subIt;
    DevEvent ev0, ev1;
    DevEvent ev_gather;   // gusto_gather_peer: this shard's copy to the gathering GPU has been enqueued up to here
    double last_ms = 0.0;
    bool pending = false;  // a gusto_solve_async launch has not been waited for yet
    int probe_iters = 2, probe_min_batch = 2048;  // longest-first schedule (gusto_set_schedule)
    bool sched_forced = false;                    // gusto_set_schedule was called: the caller's choice overrides the model default
    DevBuf<int> d_order;      // waiting lists of the scheduler, [SCHED_LEVELS][probe_iters * batch_cap]
    DevBuf<int> d_queue;      // work-queue heads, one per launch of a gusto_solve call
    DevBuf<int> d_sched_ord;  // [2][batch_cap]: difficulty bucket and hand-out order of the fresh problems (hardest first)
    int slots = 0;            // resident workgroups the last launch used (persistent kernel)
    int lds_bytes = 0, per_cu = 0;   // ... its dynamic LDS per workgroup and workgroups per CU (gusto_dev_launch_info)
    int sched_init[gusto::SQ_WORDS] = {0};   // initial scheduler words of a launch (host side of an async copy)
    bool have_problems = false;
    int decomposition = 0;         // gusto_set_decomposition: 0 auto, 1 a wave per problem, 3 / 4 two / four waves per problem (2: reserved, refused)
    int waves = 0;                 // waves per problem of the GuSTO kernel (0 = one per 64 knots; development builds: GUSTO_DEV_WAVES)
    // gusto_set_active: the problems the next gusto_solve calls iterate (n_active < 0: all of them); d_active = the mask [B]
    // (gusto_shoot reads it), d_active + batch_cap = the list of active problems (the hand-out order of the launch)
    DevBuf<int> d_active;
    int n_active = -1;
    int sched_err = 0;             // latched scheduler error of the last solve (gusto_finish): getters and solves fail until the next set_problems
    int* h_sched_err = nullptr;    // pinned host word the error flag is copied to on the handle's stream, before the stream is waited for
    DevBuf<double> d_gX, d_gU;     // gusto_gather_peer: the shards of several handles, one after the other, on this handle's GPU
    DevBuf<double> d_Upub;         // TrajOpt handles: U compacted to the public [B][N][u_dim] layout for gusto_get_traj_dev
    ShootState shoot; VerifyState verify; TvlqrState tvlqr; SimulateState simulate; LincovState lincov;   // the post-solve stages
    SelectState select;
    TrajlibState trajlib;
    ReplanState replan;
    TightenState tighten;
    RoadmapState roadmap;
    TfsearchState tfsearch;
    LegsState legs;
    FleetState fleet;
    unsigned long long solves = 0;   // gusto_solve / gusto_solve_async calls that enqueued a launch (gusto_tfsearch_update, gusto_legs_advance ask for one)
    std::string err;

    // (the buffers and events free themselves; the caller has made `device` current: gusto_destroy)
    __attribute__((visibility("hidden"))) ~gusto_handle_s() {
        if (h_sched_err) (void)hipHostFree(h_sched_err);
        if (own_stream && stream) (void)hipStreamDestroy(stream);
    }
};

extern thread_local std::string g_err;

#define HIPCHK(h, call)                                                                        \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess) {                                                                \
            std::string msg_ = std::string(#call) + ": " + hipGetErrorString(e_);             \
            if (h) (h)->err = msg_;                                                            \
            g_err = msg_;                                                                      \
            return GUSTO_ERR_HIP;                                                              \
        }                                                                                      \
    } while (0)

// completes an enqueued solve: blocks on the handle's stream and takes the kernel time from its events
static inline int gusto_sched_err_rc(gusto_handle h) {
    if (!h->sched_err) return GUSTO_OK;
    h->err = h->sched_err == 1 ? "scheduler: a claimed waiting-list entry never arrived (problem lost); set the problems again"
                               : "scheduler: workgroups gave up waiting for problems still in their probing slices; set the problems again";
    return GUSTO_ERR_STATE;
}
// The device-side scheduler reports a problem it lost instead of leaving it half-solved (scp.hpp: sched_pop).  The flag is
// copied on the handle's OWN stream into pinned memory right behind the kernel (launch.hpp), so reading it here needs no
// blocking copy on the null stream (which would serialise with the other handle of an overlapped pair).  The error is
// LATCHED until gusto_set_problems: every getter and every further solve fails with it (a batch that lost a problem is
// not resumed), the setters (environment, parameters, stream, ...) do not -- they may come before or after the problems.
// gusto_complete: waits for an enqueued solve and latches its error; GUSTO_ERR_HIP only.
static inline int gusto_complete(gusto_handle h) {
    if (!h->pending) return GUSTO_OK;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, event_ms(h->ev0, h->ev1, &h->last_ms));
    h->pending = false;
    if (h->h_sched_err && *h->h_sched_err) h->sched_err = *h->h_sched_err;
    return GUSTO_OK;
}
// gusto_finish: gusto_complete, then the latched scheduler error (getters, gusto_wait, gusto_solve*)
static inline int gusto_finish(gusto_handle h) {
    const int rc = gusto_complete(h);
    return rc ? rc : gusto_sched_err_rc(h);
}
// enqueued behind a solve kernel on the handle's stream: the scheduler's error word -> pinned host memory
static inline hipError_t gusto_fetch_sched_err(gusto_handle h) {
    if (!h->h_sched_err) {
        hipError_t e = hipHostMalloc(reinterpret_cast<void**>(&h->h_sched_err), sizeof(int), hipHostMallocDefault);
        if (e != hipSuccess) return e;
    }
    *h->h_sched_err = 0;
    if (!h->d_queue) return hipSuccess;
    return hipMemcpyAsync(h->h_sched_err, h->d_queue + gusto::SQ_ERR, sizeof(int), hipMemcpyDeviceToHost, h->stream);
}

// every setter first completes an enqueued solve (gusto_solve_async) on the handle's own device; a latched scheduler error
// is not the setter's business (it is surfaced by the getters and the solves until gusto_set_problems)
static inline int setter_enter(gusto_handle h) {
    HIPCHK(h, hipSetDevice(h->device));
    return gusto_complete(h);
}
// every getter first completes an enqueued solve and fails with a latched scheduler error, then refuses a handle without
// problems (need_problems) and makes the handle's device current.  A null handle is GUSTO_ERR_STATE here: the entry points
// that answer GUSTO_ERR_ARG to one check it themselves.
static inline int getter_enter(gusto_handle h, bool need_problems) {
    if (!h) return GUSTO_ERR_STATE;
    { int rc = gusto_finish(h); if (rc) return rc; }
    if (need_problems && !h->have_problems) return GUSTO_ERR_STATE;
    HIPCHK(h, hipSetDevice(h->device));
    return GUSTO_OK;
}

// The keep-out part of KParams (P.B is set): one set for the whole batch (gusto_set_env), or one per problem
// (gusto_set_env_batch: n_obs sizes the slots, the records say the rest).  false: the records describe another number of
// problems than P.B (checked with check_B; the caller words the refusal).
static inline bool fill_env(gusto_handle h, gusto::KParams& P, bool has_obs, bool check_B) {
    P.n_box = h->n_box; P.n_sph = h->n_sph; P.box = h->d_box; P.sph = h->d_sph;
    P.n_obs = has_obs ? h->n_box + h->n_sph : 0;
    if (!has_obs || !h->d_env) return true;
    if (check_B && h->env_B != P.B) return false;
    P.n_obs = h->n_obs_max; P.n_box = 0; P.n_sph = 0; P.env = h->d_env;
    return true;
}

// The launches of one model (launch.hpp), defined once in model_<id>.hip for the internal ids 0 .. 6; a null member: the
// model has no such kernel.  (The solve launches only enqueue; gusto_finish completes them.)
struct ModelOps {
    int (*init)(gusto_handle, bool straight);
    int (*scp)(gusto_handle, int mode, int max_iter, int force);
    int (*trajopt)(gusto_handle, int mode, int max_iter);
};
template <int MODEL> __attribute__((visibility("hidden"))) const ModelOps& model_ops();

// What gusto_set_problems does once the inputs, X and U of h->B problems are on the device or enqueued on the handle's stream
// (gusto_hip.hip): the straight line when asked for, the history reset, the post-solve stages invalidated, every problem active
__attribute__((visibility("hidden"))) int gusto_problems_loaded(gusto_handle h, bool straight);
