/*
 * gusto_hip.h -- C ABI of libgusto_hip.so: batched GuSTO sequential convex programming on MI355X.
 *
 * One call solves a batch of independent SCP problems of one model type on one GPU.  The library
 * replaces the reference's `solve_method!` plug-in for the GuSTO path,
 *     solve_gusto_jump!(SCPS, SCPP, solver, max_iter, force; kw...)      src/scp/scp_gusto.jl:49
 * which is what `solve_SCP!` calls through its function argument           src/traj_opt.jl:47-72
 * Each entry point names the reference interface it stands in for.
 *
 * Conventions: every function returns 0 on success or a negative gusto_rc; per-problem failures are
 * data (status arrays), never a failing return code.  All pointers are HOST memory unless the name ends
 * in `_dev`.  Layouts are the reference's Julia column-major X[n,N], U[m,N] per problem, problem index
 * slowest: X[b][k][i].  A handle is not thread-safe; use one handle per host thread / GPU.
 */
#ifndef GUSTO_HIP_H
#define GUSTO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define GUSTO_MAXN 13
#define GUSTO_MAXM 6

/* typeof(SCPP.PD.model) -> id (src/dynamics/{freeflyer_se2,dubins_car,astrobee_se3,astrobee_se3_manifold}.jl) */
enum gusto_model_id {
    GUSTO_FREEFLYER_SE2 = 0,
    GUSTO_DUBINS_CAR = 1,
    GUSTO_ASTROBEE_SE3 = 2,
    GUSTO_ASTROBEE_SE3_MANIFOLD = 3
};

enum gusto_rc {
    GUSTO_OK = 0,
    GUSTO_ERR_ARG = -1,       /* bad argument / unsupported size            */
    GUSTO_ERR_HIP = -2,       /* HIP runtime error, see gusto_last_error()  */
    GUSTO_ERR_STATE = -3,     /* call order (e.g. solve before set_problems) */
    GUSTO_ERR_NO_DEVICE = -4  /* no usable GPU: there is no CPU fallback     */
};

/* SCPS.scp_status entries (Symbols in scp_gusto.jl:126-146) */
enum { GUSTO_SCP_NA = 0, GUSTO_SCP_OK = 1, GUSTO_SCP_INACCURATE_MODEL = 2, GUSTO_SCP_VIOLATES_CONSTRAINTS = 3,
       GUSTO_SCP_TRUST_REGION_VIOLATED = 4 };
/* SCPS.solver_status entries (MOI termination codes accepted/rejected at scp_gusto.jl:106-111) */
enum { GUSTO_SOLVER_NA = 0, GUSTO_SOLVER_OPTIMAL = 1, GUSTO_SOLVER_ALMOST = 2, GUSTO_SOLVER_FAILED = 3 };
/* why the outer loop of a problem stopped */
enum { GUSTO_STOP_MAXITER = 0, GUSTO_STOP_CONVERGED = 1, GUSTO_STOP_SUBPROBLEM_FAILED = 2, GUSTO_STOP_OMEGA_MAX = 3,
       GUSTO_STOP_HIST_FULL = 4 /* a history vector reached hist_cap before iter_cap: create the handle with more */ };

/* SCPParam + SCPParam_GuSTO (types.jl:65-73, scp_gusto.jl:4-24; per-model values e.g. freeflyer_se2.jl:22-39) */
typedef struct {
    double Delta0, omega0, omega_max, eps, rho0, rho1, beta_succ, beta_fail, gamma_fail;
    double convergence_threshold;
} gusto_scp_params;

/* robot + model scalars (robot/freeflyer.jl:28-62, robot/astrobee3D.jl:15-33, dubins_car.jl:22-33) */
typedef struct {
    double mass, Jdiag[3], radius, clearance;
    double hard_limit_vel, hard_limit_accel, hard_limit_omega, hard_limit_alpha;
    double dubins_v, dubins_k, u_max, u_min;
    double x_max[GUSTO_MAXN], x_min[GUSTO_MAXN];
    int n_robot_comp;      /* convex robot components looped by trust_region_ratio_gusto */
    double comp_off[2][3]; /* their offsets in the robot frame                            */
} gusto_model_params;

/* inner convex solver (stands in for the `kwarg...` forwarded to the optimizer, scp_gusto.jl:82-92) */
/* tr_tol: slack of trust_region_satisfied_gusto.  The reference tests `max_k ||x_k - xp_k||^2 - Delta <= 0` (scp_gusto.jl:34-44)
 * on the optimum its solver returns; whenever the trust region row is ACTIVE the left-hand side is zero up to the solver's
 * accuracy, so the literal test is decided by the last digits of Ipopt / Gurobi (or of the interior point method here).
 * This library evaluates `<= tr_tol * max(1, Delta)` with the DEFAULT tr_tol = 1e-6 (100 x the primal tolerance `tol`), which
 * makes the verdict independent of solver noise; tr_tol = 0 selects the literal test (1 of the 44 844 accept / reject decisions
 * of the 4096-problem freeflyerSE2 batch changes; tests/test_gpu_parity.py runs both settings against the oracle). */
typedef struct {
    double tol, tol_acc, mu_floor /* smallest complementarity target; < 0 (default): 1e-10 for astrobeeSE3manifold, 1e-11 otherwise */, tr_tol;
    double mu_warm; /* complementarity of the centred start used from the second subproblem of an SCP run on (the
                       iterate then starts at the previous optimum); 0 = always the cold start; < 0 (the default) = the model's
                       own triple (mu_warm, mu_warm_gain, mu_warm_max), see below */
    int max_iter;
    int acc_iter;   /* stop with ALMOST_LOCALLY_SOLVED once the acceptable level tol_acc has held for this many consecutive
                       iterations without reaching tol (Ipopt's acceptable_iter; the reference takes MOI.ALMOST_LOCALLY_SOLVED as
                       solved, scp_gusto.jl:107).  0 = only at the iteration cap.  An interior point solve that cycles at the 1e-6
                       level (seen on astrobeeSE3manifold: a period-4 cycle of mu between 3e-10 and 3e-9) then costs 10 extra
                       iterations instead of running to the cap of 60 */
    /* The start level follows the size of the last trajectory change: a subproblem whose linearisation point moved far from
     * the previous one is started further from the boundary,
     *     mu_start = min(max(mu_warm, mu_warm_max), max(mu_warm, mu_warm_gain * c^2)),   c = convergence_measure[end]
     * (traj_opt.jl:74-85, the relative change of the trajectory in the previous SCP iteration).  mu_warm_gain = 0: the fixed
     * level mu_warm.  Model defaults (measured, tools/ipm_opts_scan.py; an internal heuristic of the interior point method, the
     * optimum it converges to is the same): freeflyerSE2 (1e-4, 0.1, 1e-2), dubins_car (1e-9, 0, -), astrobeeSE3
     * (1e-6, 1, 1e-2), astrobeeSE3manifold (1e-4, 1, 1e-2). */
    double mu_warm_gain, mu_warm_max;
    /* Upper bound of Mehrotra's centring parameter sigma = (mu_aff / mu)^3: the corrector never aims at less than a
     * (1 - sigma_max) reduction of the complementarity.  Without the bound (sigma_max >= 1) a predictor that makes no progress
     * sets sigma ~ 1, and the method can then cycle near the solution (mu between 3e-10 and 3e-9 with period 4, traced on
     * astrobeeSE3manifold) until the iteration cap, or fail.  Default (< 0): 0.1 for gusto_solve, none for gusto_solve_trajopt
     * (whose subproblems were validated with the unbounded rule); measured on the BASELINE batches: SubproblemFailed
     * 23 -> 1 of 4096 (freeflyerSE2), 22 -> 0 of 8192 (astrobeeSE3), 10 -> 7 of 2048 (manifold), and 1-3 % fewer KKT solves. */
    double sigma_max;
} gusto_ipm_opts;

typedef struct gusto_handle_s* gusto_handle;

/* fills the per-model defaults: SCPParam(model, fft), SCPParam_GuSTO(model), robot constructors */
int gusto_default_params(int model_id, gusto_scp_params* sp, gusto_model_params* mp);
int gusto_default_ipm_opts(gusto_ipm_opts* o);
int gusto_model_dims(int model_id, int* x_dim, int* u_dim);

/* SCPProblem(TOP) for a batch (types.jl:256-259): allocates all device memory for up to batch_cap problems of
 * N knots and hist_cap SCP iterations of history.  device = HIP device ordinal.
 * Horizons: 3 <= N <= 256 is accepted here, but a problem's workgroup keeps its KKT blocks in the 160 KiB LDS of a CU, which
 * bounds N per model: FreeflyerSE2 256, DubinsCar 256, AstrobeeSE3 200, AstrobeeSE3Manifold 182.  A larger N is refused with
 * GUSTO_ERR_ARG ("does not fit the 160 KiB LDS") by the first gusto_solve / gusto_solve_async / gusto_subproblem, which
 * launches nothing (tests/horizons.py holds the table, tests/test_boundary.py checks it against the layout). */
int gusto_create(gusto_handle* h, int model_id, int N, int batch_cap, int hist_cap, int device);
int gusto_destroy(gusto_handle h);
const char* gusto_last_error(gusto_handle h);

int gusto_set_params(gusto_handle h, const gusto_scp_params* sp, const gusto_model_params* mp);
int gusto_set_ipm_opts(gusto_handle h, const gusto_ipm_opts* o);
/* Workspace(robot, env) (types.jl:12-24): keep-out set = keepout_zones then obstacle_set, as AABBs
 * (min xyz, max xyz) followed by spheres (centre xyz, radius) */
int gusto_set_env(gusto_handle h, int n_box, const double* box_min_max, int n_sph, const double* sph_c_r);
/* One Workspace PER PROBLEM -- in the reference every ProblemDefinition owns its env (types.jl:32-39) and its
 * Workspace(robot, env) (types.jl:12-24), so a batch may mix obstacle layouts.  Problem b has n_box[b] AABBs and n_sph[b]
 * spheres (at most 64 components together); box_min_max / sph_c_r hold the tables of all B problems one after the other
 * in problem order ([sum n_box][6], [sum n_sph][4]).  B must equal the B of gusto_set_problems by the time of the solve
 * (either call may come first).  gusto_set_env returns the handle to one shared keep-out set. */
int gusto_set_env_batch(gusto_handle h, int B, const int* n_box, const double* box_min_max, const int* n_sph,
                        const double* sph_c_r);
/* Longest-first schedule of a gusto_solve call (new; affects time only, results are bit-identical).  gusto_solve is ONE
 * launch of persistent workgroups that pull work from a device-side scheduler.  In batches of at least `min_batch`
 * problems the first `probe_iters` time slices of a problem are one SCP iteration each; between slices the problem
 * waits in the list of its penalty level (number of omega raises so far -- the problems whose omega was raised early are
 * the long ones); workgroups take the highest raised level waiting, then fresh problems (the ones that start deepest
 * inside an obstacle first), then level 0; from slice `probe_iters` on a problem runs to its end (freeflyerSE2 problems of
 * level 0: in slices of four iterations).  probe_iters = 0: first come, first served.  Without this call: every batch that
 * does not fit the GPU's resident workgroups at once (and any batch of >= 2048 problems), 2 probing slices for freeflyerSE2,
 * 1 for the other models.  Results do not depend on the schedule. */
int gusto_set_schedule(gusto_handle h, int probe_iters, int min_batch);
/* How a gusto_solve maps problems to the GPU (new; affects time only -- both kernels run scp_gusto.jl:49-176 on the same
 * subproblem, scp_gusto.jl:178-314, to the same tolerances).  WAVE: one wavefront per problem, lane k = knot k, the
 * Newton system staged in LDS (every model).  LANE (one lane per problem) is reserved and refused with GUSTO_ERR_ARG: that kernel
 * was measured slower at every batch size and is not in the library; the value keeps its number.
 * WAVE2 / WAVE4 (round 6; astrobeeSE3 and astrobeeSE3manifold, N <= 64): two or four wavefronts per problem -- the horizon split into
 * as many Riccati chains, a wave each, joined by coarse LQR stages, and each knot's obstacle rows shared between the waves
 * (csrc/segw.hpp).  For batches that leave SIMDs without a wave: AUTO takes WAVE4 up to six problems per CU, WAVE2 up to sixteen
 * (astrobeeSE3manifold: eight), one wave per problem beyond (measured on MI355X); WAVE forces one wave per problem.  Same subproblems to the same tolerances;
 * the iterates differ in rounding (the KKT solve is reassociated), the SCP iteration counts do not on the test batches.  A model
 * or horizon without these kernels answers GUSTO_ERR_ARG at gusto_solve. */
enum { GUSTO_DECOMP_AUTO = 0, GUSTO_DECOMP_WAVE = 1, GUSTO_DECOMP_LANE = 2, GUSTO_DECOMP_WAVE2 = 3, GUSTO_DECOMP_WAVE4 = 4 };
int gusto_set_decomposition(gusto_handle h, int decomposition);
/* run on a caller-owned hipStream_t (NULL = a new stream owned by the handle).  Like every setter it first completes
 * a pending gusto_solve_async on the stream that solve was enqueued on. */
int gusto_set_stream(gusto_handle h, void* hip_stream);

/* ProblemDefinition + init trajectory + SCPSolution(SCPP, traj_init) for B problems (types.jl:32-39,233):
 * goal_lo == goal_hi -> PointGoal row, finite lo < hi -> BoxGoal rows, +-Inf -> coordinate has no goal.
 * X0/U0 == NULL -> init_traj_straightline (freeflyer_se2.jl:97-111).  Resets every history. */
int gusto_set_problems(gusto_handle h, int B, const double* x_init, const double* goal_lo, const double* goal_hi,
                       const double* tf, const double* X0, const double* U0);
/* same, inputs already resident in HBM on the handle's device */
int gusto_set_problems_dev(gusto_handle h, int B, const double* x_init_dev, const double* goal_lo_dev,
                           const double* goal_hi_dev, const double* tf_dev, const double* X0_dev,
                           const double* U0_dev);

/* solve_gusto_jump!(SCPS, SCPP, solver, max_iter, force) for the whole batch (scp_gusto.jl:49-176).
 * Synchronous.  Re-entrant: a second call resumes every problem (iter_cap = iterations + max_iter, :67). */
int gusto_solve(gusto_handle h, int max_iter, int force);
/* The same solve, enqueued on the handle's stream without blocking the host; gusto_wait (or any getter, setter or
 * solve on the handle) completes it.  New: the reference is blocking.  Two handles used alternately keep the GPU
 * full across consecutive batches -- the tail of one batch (its slowest problems) overlaps the head of the next. */
int gusto_solve_async(gusto_handle h, int max_iter, int force);
/* Which problems of the batch the following gusto_solve / gusto_solve_async / gusto_shoot calls work on: active [B], nonzero =
 * iterate, NULL = all again (the state after gusto_set_problems).  The reference's drivers loop per problem --
 * solve_SCPshooting! takes another SCP iteration and another shooting attempt only `while !SCPS.converged &&
 * SCPS.iterations < max_iter` (src/traj_opt.jl:23) -- and a batch needs that condition per problem: an inactive problem
 * keeps its trajectory, histories and counters untouched.  Not for TrajOpt handles. */
int gusto_set_active(gusto_handle h, const int* active);
int gusto_wait(gusto_handle h);
/* GPU time of the last gusto_solve, measured with HIP events on the stream the kernel ran on */
int gusto_last_solve_ms(gusto_handle h, double* ms);

/* SCPS.traj (X,U) -- TOS.traj aliases it (traj_opt.jl:58) */
int gusto_get_traj(gusto_handle h, double* X, double* U);
/* The problems the handle holds, as gusto_set_problems* or a seeding stage left them: x_init, goal_lo, goal_hi [B][x_dim], tf [B]
 * (any pointer may be NULL) */
int gusto_get_problems(gusto_handle h, double* x_init, double* goal_lo, double* goal_hi, double* tf);
int gusto_get_traj_dev(gusto_handle h, const double** X_dev, const double** U_dev);
/* Final gather of a multi-GPU run from ONE host process (one handle per GPU, shards enqueued with gusto_solve_async): completes
 * every source's solve and copies the shards, in the order of `src`, into buffers on the GPU of `dst` -- one direct peer copy
 * per shard over xGMI (fan-in); `dst` may itself be one of the sources.  Outputs (any may be NULL): device
 * pointers to X [B_total][N][x_dim] and U [B_total][N][u_dim] on dst's GPU (valid until the next gather on dst), host copies
 * of the same, the number of problems.  New: the reference is one process, one problem.  (Between processes -- one rank per
 * GPU -- the same gather runs over RCCL from the views of gusto_get_traj_dev: gusto.jl_amd/host.py gather_batch_results.) */
int gusto_gather_peer(gusto_handle dst, int n_src, const gusto_handle* src, const double** X_dev, const double** U_dev,
                      double* X_host, double* U_host, int* B_total);
/* SCPS.iterations / converged / successful per problem, plus stop reason and inner iteration count */
int gusto_get_status(gusto_handle h, int* iterations, int* converged, int* successful, int* stop_reason,
                     int* ipm_iters);
/* SCPS.dual = -dual(init rows) (freeflyer_se2.jl:486-489): [B][n] */
int gusto_get_dual(gusto_handle h, double* dual);

/* SCPSolution / SCPParam_GuSTO history vectors (types.jl:150-173, scp_gusto.jl:15-19) as [B][hist_cap]
 * arrays; n_hist[b] entries are valid in the per-iteration vectors, nJ[b] in J_true/J_full and n_rho[b] in
 * rho (those get one extra leading entry per gusto_solve call, scp_gusto.jl:73-75).  Any pointer may be NULL. */
typedef struct {
    int hist_cap; /* IN: row capacity of the arrays below, >= the handle's (gusto_get_hist_cap); else GUSTO_ERR_ARG */
    int *n_hist, *nJ, *n_rho;
    double *J_true, *J_full, *convergence_measure, *Delta, *omega, *rho;
    int *accept_solution, *scp_status, *solver_status, *trust_region_satisfied, *convex_ineq_satisfied, *ipm_iters;
} gusto_history;
int gusto_get_history(gusto_handle h, gusto_history* out);
int gusto_get_hist_cap(gusto_handle h, int* hist_cap);
/* When a problem stops with GUSTO_STOP_SUBPROBLEM_FAILED the reference has pushed one more solver_status entry than
 * any other vector (scp_gusto.jl:106): it is solver_status[b][n_hist[b]]. */

/* SCPParam_GuSTO supplied by the caller -- scp_gusto.jl:60 keeps a `param.alg` that is already defined, so a user
 * can start from her own Delta_vec[end] / omega_vec[end].  Overwrites the last Delta / omega history entry of every
 * problem (after gusto_set_problems: the initial Delta0 / omega0).  Either pointer may be NULL.  [B] each. */
int gusto_set_trust_state(gusto_handle h, const double* Delta, const double* omega);

/* Indirect shooting seeded by the SCP dual: solve!(SS::ShootingSolution, SP::ShootingProblem) (src/shooting.jl:4-49)
 * for every problem of the batch, the refinement step of solve_SCPshooting! (src/traj_opt.jl:4-45).  The two models
 * that have a shooting ODE in the reference: DubinsCar (shooting_ode! / get_control, dubins_car.jl:259-280) and
 * AstrobeeSE3Manifold (dynamics_shooting! / shooting_ode! / get_control, astrobee_se3_manifold.jl:831-895, 26 states +
 * costates); other models return GUSTO_ERR_ARG.  The reference's ODE and
 * nonlinear solvers (DifferentialEquations, NLsolve) are external and absent: the scheme is RK4 with `substeps` steps
 * per knot interval and Newton with a forward-difference Jacobian on F(p0) = x_goal - x(tf; p0), |F|_inf <= ftol.
 * p0: [B][n] host seeds, or NULL = SCPS.dual of every problem (what ShootingProblem(TOP, SCPS) takes, types.jl:219-227). */
typedef struct {
    int substeps;    /* RK4 steps per knot interval (default 4)             */
    int max_newton;  /* nlsolve(..., iterations = 100, ...)  shooting.jl:14 */
    double ftol;     /* nlsolve(..., ftol = 1e-3)            shooting.jl:14 */
    int no_group_pass;  /* 0 (default, also what a zero- or brace-initialised struct gives): problems still iterating after 8
                         * Newton steps go on with 16 lanes each; 1: a lane per problem throughout -- the same results bit for
                         * bit, slower for the stragglers (tests compare the two).  Any other value: GUSTO_ERR_ARG */
} gusto_shoot_opts;
int gusto_default_shoot_opts(gusto_shoot_opts* o);
int gusto_shoot(gusto_handle h, const double* p0, const gusto_shoot_opts* opts);
/* status [B]: 1 = :Optimal (sol_newton.f_converged), 0 = :Diverged; p0 [B][n] the converged initial costate; X [B][N][n],
 * U [B][N][m] the recovered trajectory of the :Optimal problems (shooting.jl:26-36); the X and U of a problem that is not
 * :Optimal in the last gusto_shoot are zeros.  A problem that gusto_set_active left out of that call reports status 0, 0 Newton
 * iterations, a NaN residual and its seed as p0.  Any pointer may be NULL. */
int gusto_get_shoot(gusto_handle h, int* status, int* newton_iters, double* resid, double* p0, double* X, double* U);

/* Post-solve verification of every problem of the batch (csrc/verify.hip): interpolate_traj, dynamics_constraint_satisfaction
 * and verify_collision_free of the Astrobee model files (astrobee_se3_manifold.jl:1011-1077, astrobee_se3.jl:495-560), for all
 * four models.  X [B][N][x_dim], U [B][N][u_dim]: host trajectories to check, or NULL, NULL = the handle's current ones (SCPS.traj);
 * neither call changes the handle's trajectories, status or histories.  Honours the keep-out sets of gusto_set_env / _batch and
 * gusto_set_active (an inactive problem's report is left as the last call wrote it).  Runs on the handle's stream, after any
 * pending gusto_solve_async; timed with events of its own (gusto_last_solve_ms keeps its value).
 * Roll-out: every interval k -> k+1 restarts from X[:,k], holds U[:,k] and takes Nstep_b classical RK4 steps of dt_b / Nstep_b,
 * Nstep_b = nstep if nstep > 0, else ceil(dt_b / dt_min), dt_b = tf_b / (N - 1).  An Nstep_b above nstep_cap (or below 1) is
 * GUSTO_ERR_ARG for the whole call: the count is never clamped.  The dense trajectory has Nstep_b (N - 1) + 1 samples, the last
 * one X[:,N].  dense_collision = 0 skips the distances at the dense samples (min_dist_dense = +inf, min_dense_sample = -1).
 * TrajOpt handles answer GUSTO_ERR_ARG: their device-side controls carry the defect variables; not supported here. */
typedef struct {
    double dt_min;        /* interpolate_traj(traj, SCPP, dt_min=0.1) */
    int nstep;            /* > 0: this many substeps for every problem; 0 (default): ceil(dt / dt_min) */
    int nstep_cap;        /* default 64 */
    int dense_collision;  /* default 1 */
} gusto_verify_opts;
int gusto_default_verify_opts(gusto_verify_opts* o);
int gusto_verify(gusto_handle h, const double* X, const double* U, const gusto_verify_opts* o);
/* Caller-owned arrays [B]; any pointer may be NULL.
 * collision_free, first_knot, first_dist: verify_collision_free as written -- knots only, `dist < 0` on the raw signed distance
 *   (clearance is read there and unused), the first hit in the reference's obstacle-major loop order (obstacle, then knot; robot
 *   components outermost); first_knot is 1-based, and 0 with first_dist 0.0 when the trajectory is free.
 * min_dist_knots: smallest signed distance over knots, obstacles and robot components.
 * dyn_defect_l1: sum_k |(x_{k+1} - x_k) / dt - f(x_k, u_k)|_1, dynamics_constraint_satisfaction (forward Euler, as written).
 * min_dist_dense, min_dense_sample: smallest signed distance over all dense samples and the 0-based sample it occurs at (the
 *   first one on a tie); not in the reference.
 * max_gap: max_k |xhat_{k+1} - X[:,k+1]|_inf, xhat_{k+1} the end of the roll-out of interval k (the value interpolate_traj
 *   overwrites with the knot).
 * DubinsCar (no keep-out set), or an empty one: the distances are +inf, collision_free 1, min_dense_sample -1. */
typedef struct {
    int *collision_free, *first_knot;
    double *first_dist, *min_dist_knots, *dyn_defect_l1, *min_dist_dense;
    int *min_dense_sample;
    double *max_gap;
} gusto_verify_report;
int gusto_get_verify(gusto_handle h, gusto_verify_report* out);
/* gusto_verify that also keeps the dense trajectories on the device: nfull_max (may be NULL) receives the row count of the
 * buffers, the largest Nstep_b (N - 1) + 1 of the batch.  gusto_get_dense copies them out: nfull [B], Xfull [B][nfull_max][x_dim],
 * Ufull [B][nfull_max - 1][u_dim] (the held controls); the rows behind nfull[b] (Ufull: nfull[b] - 1) are zeros.  Only this call
 * allocates the dense buffers.  GPU time of the last gusto_verify / gusto_interpolate kernel: gusto_last_verify_ms. */
int gusto_interpolate(gusto_handle h, const double* X, const double* U, const gusto_verify_opts* o, int* nfull_max);
int gusto_get_dense(gusto_handle h, int* nfull, double* Xfull, double* Ufull);
int gusto_last_verify_ms(gusto_handle h, double* ms);

/* Time-varying LQR tracking gains around every trajectory of the batch (csrc/tvlqr.hip): the feedback law
 *     u = U[:,k] - K_k (x(t_k) - X[:,k])
 * that goes with the open-loop X, U, t.  No counterpart in the reference (it hands its trajectories over open loop); the
 * definitions are therefore stated here.
 * Roll-out map: F_k(x, u) is Nstep_b classical RK4 steps of dt_b / Nstep_b from x under the held control u, Nstep_b exactly as
 *   gusto_verify computes it (nstep, or ceil(dt_b / dt_min); outside 1 .. nstep_cap: GUSTO_ERR_ARG for the whole call, nothing
 *   is launched).  It is the map whose value at (X[:,k], U[:,k]) gusto_interpolate rolls out.  States are not renormalised: the
 *   quaternion of AstrobeeSE3Manifold is carried as 13 plain states.
 * Discrete Jacobians: Ad_k = dF_k/dx, Bd_k = dF_k/du at (X[:,k], U[:,k]), k = 1 .. N-1 -- the exact derivative of that discrete
 *   map, forward mode through the four RK4 stages of every substep with the models' own A = df/dx at each stage point and
 *   B = df/du (not a matrix exponential, not a finite difference).
 * Riccati recursion: P_N = diag(Qf); for k = N-1 .. 1
 *     H = diag(Q, R) + [Ad_k Bd_k]' P_{k+1} [Ad_k Bd_k],   L = chol(H_uu),   W = L^-1 H_ux,   K_k = L^-T W,
 *     P_k = H_xx - W' W   (stored symmetric; H_uu^-1 is never formed).
 * Status: a Cholesky pivot <= 0 or not finite at knot k gives the problem status 0 and fail_knot k (1-based); its gains, and
 *   its P, from that knot down to knot 1 are zeros.  Otherwise status 1, fail_knot 0.  Failures are data, not return codes.
 * X [B][N][x_dim], U [B][N][u_dim]: host trajectories, or NULL, NULL = the handle's current ones; exactly one NULL is
 *   GUSTO_ERR_ARG.  The call honours gusto_set_active (an inactive problem's outputs stay as the last call wrote them), runs on
 *   the handle's stream after any pending gusto_solve_async, is timed with events of its own (gusto_last_solve_ms and
 *   gusto_last_verify_ms keep their values) and never changes trajectories, status or histories.  TrajOpt handles answer
 *   GUSTO_ERR_ARG, a handle without problems GUSTO_ERR_STATE, a weight out of range (Q, Qf >= 0 and R > 0 on the model's
 *   x_dim / u_dim entries, all finite) GUSTO_ERR_ARG.  Every horizon gusto_create accepts, all four models.
 * The device buffers (AB, K, P; several hundred MB at 8192 problems of AstrobeeSE3) exist only after the first call and are
 *   sized by the batch of that call (a later call with a larger batch, after a new gusto_set_problems, grows them); the P of
 *   every knot only after the first call with store_P.  A masked first call after gusto_set_problems leaves zeros for the
 *   inactive problems.  "As the last call wrote them" holds per buffer: the P of every knot is written by calls with store_P
 *   only, so after calls that mix store_P an inactive problem's full P can be older than its K and its P of knot 1. */
typedef struct {
    double Q[GUSTO_MAXN], R[GUSTO_MAXM], Qf[GUSTO_MAXN]; /* diagonal weights */
    double dt_min; int nstep, nstep_cap;                 /* the roll-out of gusto_verify_opts, same meaning, same refusal */
    int store_P;                                         /* 1: keep P of every knot; 0 (default): only P of knot 1 */
} gusto_tvlqr_opts;
/* Q = Qf = R = 1 on the model's entries (0 behind them), dt_min 0.1, nstep 0, nstep_cap 64, store_P 0 */
int gusto_default_tvlqr_opts(int model_id, gusto_tvlqr_opts* o);
int gusto_tvlqr(gusto_handle h, const double* X, const double* U, const gusto_tvlqr_opts* o);
/* Caller-owned arrays; any pointer may be NULL.  status, fail_knot [B]; K [B][N-1][u_dim][x_dim]; AB [B][N-1][x_dim][x_dim + u_dim],
 * the rows of [Ad | Bd]; P [B][N][x_dim][x_dim] when the LAST call ran with store_P (P_N = diag(Qf) included), else
 * [B][x_dim][x_dim], the P of knot 1.  The signature carries no size: a caller that wants every knot's P passes store_P = 1
 * to the call before (gusto.jl_amd/_capi.py refuses the full P after a call without store_P with GUSTO_ERR_STATE's code).
 * Before the first gusto_tvlqr since gusto_set_problems: GUSTO_ERR_STATE. */
int gusto_get_tvlqr(gusto_handle h, int* status, int* fail_knot, double* K, double* P, double* AB);
/* GPU time of both phases of the last gusto_tvlqr (linearise + Riccati), from HIP events on the handle's stream */
int gusto_last_tvlqr_ms(gusto_handle h, double* ms);

/* Closed-loop Monte Carlo roll-outs of the tracking law (csrc/simulate.hip): every trajectory of the batch is flown S times
 * with its gains, from perturbed starts and with limited actuators.  No counterpart in the reference; the definitions:
 * Roll-out of sample s of problem b, p = pert[b][s] a vector of x_dim + u_dim numbers:
 *     x <- X[:,1] + p[0:x_dim];
 *     at every knot k = 1 .. N-1:  v = (U[:,k] - K_k (x - X[:,k])) + p[x_dim:],  u = clip(v, u_lo, u_hi) entry-wise
 *     (u_i = u_lo_i if v_i < u_lo_i, u_hi_i if v_i > u_hi_i, else v_i; +-infinity = no bound); u is held for Nstep_b classical
 *     RK4 steps of dt_b / Nstep_b -- the map gusto_interpolate rolls out and gusto_tvlqr linearised, Nstep_b by the same rule
 *     (nstep, or ceil(dt_b / dt_min); outside 1 .. nstep_cap: GUSTO_ERR_ARG for the whole call).  The state is NOT restarted at
 *     the knots and not renormalised: the quaternion of AstrobeeSE3Manifold is 13 plain states.
 * Dense samples: j = (k - 1) Nstep_b + i (0-based) is the state before substep i of interval k; j = (N - 1) Nstep_b is knot N.
 * Signed distance: the smallest over the robot's components and the keep-out components of gusto_set_env / _batch, at every
 *   dense sample (dense_collision = 1) or at the knots only (0; the index stays the dense one).  sample_min_dist is the
 *   smallest over the samples evaluated, sample_dense_index the first j it occurs at.  A sample COLLIDES when that distance
 *   is < 0, the raw test of verify_collision_free.  DubinsCar, or an empty keep-out set: +inf, index -1, never a collision.
 * Non-finite: a sample whose state has an entry that is not finite -- at the start or after any RK4 step -- is flagged and
 *   advanced no further: its state stays what it was then (x_final and the knots from there on hold it), its distance is
 *   the smallest up to there.  It counts as not free and is left out of every minimum and maximum of the per-problem report.
 * Perturbations: the caller's pert [B][S][x_dim + u_dim] as given, or (pert = NULL) generated on the device from integers only
 *   (csrc/simrng.hpp, which host and device code both compile): sample 0 is always the unperturbed one (zeros); for entry i
 *   of sample s >= 1 of problem b
 *     idx = ((first_problem + b) S + s) (x_dim + u_dim) + i,   z = seed + 0x9E3779B97F4A7C15 (idx + 1),
 *     z = (z ^ z >> 30) 0xBF58476D1CE4E5B9,   z = (z ^ z >> 27) 0x94D049BB133111EB,   z ^= z >> 31     (mod 2^64: splitmix64)
 *     r = (z >> 11) 2^-53,   p[i] = (2 r - 1) w[i],   w = (dx0, du0)
 *   so a shard created with first_problem = its offset draws what the whole batch would draw.
 * K [B][N-1][u_dim][x_dim]: host gains, or NULL = the gains of the handle's last gusto_tvlqr (before any: GUSTO_ERR_STATE).
 * X, U: host trajectories or NULL, NULL = the handle's current ones (exactly one NULL: GUSTO_ERR_ARG).  The call honours
 *   gusto_set_active: an inactive problem's report, per-sample arrays and knots stay as the last call with the same n_samples
 *   wrote them (zeros after new problems or another n_samples).  It runs on the handle's stream after any pending
 *   gusto_solve_async, is timed with events of its own and changes neither trajectories, status, histories nor gains.
 *   TrajOpt handles answer GUSTO_ERR_ARG, a handle without problems GUSTO_ERR_STATE; n_samples outside 1 .. 4096, a
 *   half-width that is negative or not finite, u_lo > u_hi (or a NaN bound), dense_collision / store_knots other than 0 / 1 and
 *   bad roll-out options answer GUSTO_ERR_ARG.  The device buffers exist only after the first call and only grow.
 * A problem's report and per-sample arrays are the same bit for bit whatever batch it sits in and whatever else is active. */
typedef struct {
    int n_samples;                            /* S, 1 .. 4096; default 64 */
    unsigned long long seed, first_problem;   /* generated perturbations only; default 0, 0 */
    double dx0[GUSTO_MAXN], du0[GUSTO_MAXM];  /* half-widths of the generated perturbations.  The default dx0 = 0.01 on every
                                               * state is a PLACEHOLDER: the states have different units, the caller sets it */
    double u_lo[GUSTO_MAXM], u_hi[GUSTO_MAXM];/* actuator limits; default -inf, +inf: no clipping */
    double dt_min; int nstep, nstep_cap;      /* the roll-out of gusto_verify_opts, same meaning, same refusal */
    int dense_collision;                      /* default 1 */
    int store_knots;                          /* 1: keep the closed-loop states at the knots; default 0 */
} gusto_simulate_opts;
/* 64 samples, seed 0, first_problem 0, dx0 = 0.01 on the model's x_dim entries (0 behind them), du0 = 0, no clipping,
 * dt_min 0.1, nstep 0, nstep_cap 64, dense_collision 1, store_knots 0 */
int gusto_default_simulate_opts(int model_id, gusto_simulate_opts* o);
int gusto_simulate(gusto_handle h, const double* X, const double* U, const double* K, const double* pert,
                   const gusto_simulate_opts* o);
/* Caller-owned arrays; any pointer may be NULL.  Per problem ([B] unless stated), reduced over the samples in a fixed order:
 * n_free: samples that stayed finite and did not collide; n_finite: samples that stayed finite; n_clipped: samples with a
 *   clipped control entry at some knot.
 * min_dist: the smallest sample_min_dist over the finite samples (+inf without obstacles or finite samples); worst_sample: the
 *   lowest sample it occurs at, worst_dense_sample: that sample's sample_dense_index (both -1 when min_dist is +inf).
 * max_dev [B][x_dim]: the largest |x_i(t_k) - X[i,k]| over the finite samples and the knots k = 1 .. N; max_final_dev
 *   [B][x_dim]: the same at knot N (zeros without finite samples).
 * Per sample: sample_min_dist, sample_dense_index, sample_flags [B][S] (bit 0 collided, bit 1 some control entry was clipped,
 *   bit 2 non-finite), x_final [B][S][x_dim]. */
typedef struct {
    int *n_free, *n_finite, *n_clipped, *worst_sample, *worst_dense_sample;
    double *min_dist, *max_dev, *max_final_dev;
    double *sample_min_dist;
    int *sample_dense_index, *sample_flags;
    double *x_final;
} gusto_simulate_report;
int gusto_get_simulate(gusto_handle h, gusto_simulate_report* out);
/* Xcl [B][N][S][x_dim], the closed-loop state of every sample at every knot: one knot of the 64 samples of a wavefront is one
 * contiguous range.  Only after a gusto_simulate with store_knots = 1, otherwise GUSTO_ERR_STATE. */
int gusto_get_simulate_knots(gusto_handle h, double* Xcl);
/* GPU time of the last gusto_simulate (roll-out and, for more than 256 samples, the reduction launch), from HIP events */
int gusto_last_simulate_ms(gusto_handle h, double* ms);

/* gusto_simulate with an uncertain plant and an actuator noise drawn anew in every hold interval (csrc/simulate.hip).  No
 * counterpart in the reference.  Everything gusto_simulate defines stays as it is -- the roll-out, the dense samples, the
 * distance, the non-finite rule, pert and its generator, K, X, U, gusto_set_active, stream and timing, the refusals (under this
 * call's name), the grow-only buffers, "the same bit for bit whatever batch it sits in" -- and the controller is the NOMINAL
 * one: K, X, U and the law are unchanged, only the plant that is integrated and the control it receives differ.
 * Plant of sample s of problem b: theta = plant[b][s][0 .. GUSTO_NPLANT-1] = (mass, Jdiag[0], Jdiag[1], Jdiag[2], dubins_v,
 *   dubins_k), ABSOLUTE values as given by the caller, or (plant = NULL) generated: theta_j = nominal_j (1 + e_j), nominal the
 *   handle's gusto_model_params, e_j uniform in [-plant_rel_j, plant_rel_j), one rounding for the sum and one for the product;
 *   sample 0 draws zeros: it is the nominal plant, exactly.  The RK4 stages evaluate f with theta in place of mass, Jdiag,
 *   dubins_v, dubins_k; nothing else of gusto_model_params changes: radius, clearance and the robot's components are the
 *   nominal ones.  freeflyerSE2 reads mass and Jdiag[2], DubinsCar dubins_v and dubins_k, both Astrobee models mass and
 *   Jdiag[0 .. 2]; entries a model does not read are ignored, whatever they hold.
 * Actuator noise: in interval k = 1 .. N-1
 *     v = ((U[:,k] - K_k (x - X[:,k])) + p[x_dim:]) + w_k,   u = clip(v, u_lo, u_hi) as in gusto_simulate
 *   with w_k = white[b][k-1][s][0 .. u_dim-1] as given by the caller -- [B][N-1][S][u_dim], knot-major like Xcl, so a
 *   wavefront's 64 samples of one interval are one contiguous range -- or (white = NULL) generated: entry i uniform in
 *   [-dw_i, dw_i), zeros for sample 0.  The clipped flag and n_clipped see v after the noise.  This is the sampled form of
 *   the du_white of gusto_lincov with du_white_i = dw_i / sqrt(3), the convention of that stage's default S0 (the variances of
 *   the uniform draws with the same half-widths); gusto_lincov covers dw in this way; gusto_lincov_disturbed also the plant dispersion,
 *   to first order.
 * Generator: splitmix64 and the r -> (2 r - 1) w step of gusto_simulate on two streams of their own.  Streams whose seeds
 *   differ by a multiple of 0x9E3779B97F4A7C15 would be shifted copies of the pert stream, so the stream seeds are hashed, with
 *   sm(seed, idx) output number idx of splitmix64 started at seed (the z of gusto_simulate's text):
 *     seed_plant = sm(seed ^ 0x504C414E54, 0),   idx_plant = ((first_problem + b) S + s) 6 + j
 *     seed_white = sm(seed ^ 0x5748495445, 0),   idx_white = (((first_problem + b) S + s) (N - 1) + (k - 1)) u_dim + i
 *   (seed, first_problem of gusto_simulate_opts): a shard with first_problem = its offset draws what the whole batch draws.
 * gusto_get_simulate, gusto_get_simulate_knots and gusto_last_simulate_ms report the last call of either kind;
 *   gusto_get_simulate_plant returns the theta the kernel used, generated or supplied (the kernel writes them out; an inactive
 *   problem's are those of the last disturbed call with the same n_samples, zeros if a plain gusto_simulate came between), and
 *   answers GUSTO_ERR_STATE when the last call was a plain gusto_simulate or there was none.
 * GUSTO_ERR_ARG, nothing launched, the offending problem, sample and entry in gusto_last_error: a plant_rel outside [0, 1) or
 *   not finite; a dw that is negative or not finite; a supplied plant whose mass or Jdiag entry, where the model reads it, is
 *   not finite or not > 0, or whose dubins_v or dubins_k, where read, is not finite; a supplied white with a non-finite entry.
 * With d NULL or all zeros and plant = white = NULL every output equals that of gusto_simulate with the same remaining
 *   arguments, as numbers (adding a zero noise can at most turn a -0.0 into +0.0); likewise when the caller supplies the
 *   nominal theta and zeros as white.
 * plant_rel[0] = 1.36 / 16.72 = 0.08134 spans the reference free-flyer's 15.36 .. 18.08 kg (robot/freeflyer.jl:32-34). */
#define GUSTO_NPLANT 6    /* mass, Jdiag[0], Jdiag[1], Jdiag[2], dubins_v, dubins_k */
typedef struct {
    double plant_rel[GUSTO_NPLANT]; /* half-widths of the relative dispersion of the plant's scalars; default 0 */
    double dw[GUSTO_MAXM];          /* half-widths of the actuator noise drawn anew in every hold interval; default 0 */
} gusto_disturb_opts;
int gusto_default_disturb_opts(gusto_disturb_opts* d);            /* all zeros */
int gusto_simulate_disturbed(gusto_handle h, const double* X, const double* U, const double* K, const double* pert,
                             const double* plant, const double* white,
                             const gusto_simulate_opts* o, const gusto_disturb_opts* d);
int gusto_get_simulate_plant(gusto_handle h, double* plant);     /* [B][S][GUSTO_NPLANT] of the last disturbed call */

/* Linear covariance analysis of the tracking law (csrc/lincov.hip): the analytic counterpart of gusto_simulate -- one forward
 * pass per problem carries a covariance through the closed loop and turns it into margins.  No counterpart in the reference;
 * the definitions, for one problem with n = x_dim, m = u_dim:
 * Augmented deviation z = [dx; b]: dx the deviation of the closed-loop state from X[:,k], b the constant control offset (the
 *   p[x_dim:] of gusto_simulate).  S_k = [[Sxx, Sxb], [Sbx, Sbb]], (n + m) x (n + m), is its covariance at knot k.
 * Start: S_1 = S0, the caller's [B][n + m][n + m] array, or (S0 = NULL) diag(dx0_i^2 / 3, du0_j^2 / 3): the variances of the
 *   uniform draws of gusto_simulate's generator with the same half-widths.
 * Recursion, k = 1 .. N-1, with [Ad_k | Bd_k] of the handle's LAST gusto_tvlqr and G_k = [Ad_k - Bd_k K_k | Bd_k] (n x (n + m)):
 *     Sxx_{k+1} = G_k S_k G_k' + Bd_k diag(du_white^2) Bd_k',   Sxb_{k+1} = G_k S_k[:, n:],   Sbb stays.
 *   Sxx is computed on the upper triangle and mirrored: symmetric to the bit.  du_white is the standard deviation of an
 *   independent actuator noise w_k per hold interval (gusto_simulate has no such term; gusto_simulate_disturbed samples it
 *   with the half-widths dw = sqrt(3) du_white).
 * Commanded control at knot k: its deviation is dv = [-K_k | I] z + w_k,
 *     sigma_u[k][i] = sqrt(([-K_k I] S_k [-K_k I]' + diag(du_white^2))_ii);   sigma_x[k][i] = sqrt(Sxx_k[i][i]).
 *   Under every square root here and below, a variance that rounding leaves below zero counts as zero: the feedback cancels a
 *   constant offset, so the variance of the commanded control decays to rounding noise along a long horizon.
 * Obstacle margin at knot k: for every robot component c and keep-out component i (gusto_set_env / gusto_set_env_batch) the
 *   signed distance d at X[:,k] and its outward normal nh -- the component offsets are translations, so nh is the exact
 *   gradient with respect to the first WS states (2 in the plane, 3 in space);
 *     sigma_d = sqrt(nh' Sxx[0:WS, 0:WS] nh),   z = d / sigma_d;   sigma_d == 0: z = +inf for d >= 0, -inf for d < 0.
 *   z_obs[k] is the smallest z over the pairs in loop order, components outermost: pair ordinal c n_obs + i.  DubinsCar, or an
 *   empty keep-out set: +inf.  (A z that is NaN never wins a minimum.)
 * Control margin at knot k <= N-1, entry i: min(u_hi_i - U[i,k], U[i,k] - u_lo_i) / sigma_u[k][i]; an infinite bound gives +inf,
 *   sigma_u == 0 is decided by the sign of the room as for sigma_d.
 * Per problem: min_z_obs, the smallest z_obs[k], with obs_knot (1-based; 0 when it is +inf) and obs_pair (the ordinal; -1 when
 *   it is +inf); min_z_ctl with ctl_knot and ctl_entry likewise; ties go to the lowest knot, then the lowest ordinal / entry;
 *     p_collision_bound = min(1, sum_k erfc(z_obs[k] / sqrt(2)) / 2)
 *   -- Boole's inequality over the knots if the deviations are read as Gaussian.  It is a BOUND UNDER THAT READING, not a
 *   probability: nothing here says the deviations are Gaussian, and between the knots nothing is looked at.
 * Status: 1 and fail_knot 0 normally.  K = NULL and a problem whose gusto_tvlqr status is 0: status 0, fail_knot that of
 *   gusto_tvlqr, every output zero.  A non-finite entry in Sxx_{k+1}, Sxb_{k+1} or sigma_u at knot k: status 0, fail_knot k, the
 *   per-knot rows from that knot on are zeros and the summaries cover the knots before it.  Failures are data, not return codes.
 * K [B][N-1][u_dim][x_dim]: host gains, or NULL = the gains of the handle's last gusto_tvlqr.  [Ad | Bd] ALWAYS come from the
 *   handle's last gusto_tvlqr (before any since gusto_set_problems: GUSTO_ERR_STATE): the caller passes the X, U that call saw,
 *   as for gusto_simulate.  X, U: host trajectories or NULL, NULL = the handle's current ones (exactly one NULL: GUSTO_ERR_ARG).
 * The call honours gusto_set_active (an inactive problem keeps what the last call wrote; zeros after a masked first call since
 *   gusto_set_problems), runs on the handle's stream after any pending gusto_solve_async, is timed with events of its own and
 *   changes neither trajectories, status, histories nor gains.  TrajOpt handles answer GUSTO_ERR_ARG, a handle without problems
 *   GUSTO_ERR_STATE.  GUSTO_ERR_ARG, with the offending problem and entry in gusto_last_error: a half-width or du_white that is
 *   negative or not finite, u_lo > u_hi or a NaN bound, store_S other than 0 / 1, an S0 that is not finite, has a negative
 *   diagonal entry or is not symmetric to the bit.  Whether S0 is positive semi-definite is the caller's business.
 * The device buffers exist only after the first call and only grow; Sxx of every knot only after a call with store_S.  All
 *   reductions run in a fixed order without atomics: a problem's outputs are the same bit for bit in any batch and under any
 *   gusto_set_active mask. */
typedef struct {
    double dx0[GUSTO_MAXN], du0[GUSTO_MAXM];   /* default S0: half-widths as in gusto_simulate_opts; the default dx0 = 0.01 is the
                                                * same PLACEHOLDER, du0 = 0 */
    double du_white[GUSTO_MAXM];               /* default 0 */
    double u_lo[GUSTO_MAXM], u_hi[GUSTO_MAXM]; /* default -inf, +inf */
    int store_S;                               /* 1: keep Sxx of every knot; default 0 */
} gusto_lincov_opts;
int gusto_default_lincov_opts(int model_id, gusto_lincov_opts* o);
int gusto_lincov(gusto_handle h, const double* X, const double* U, const double* K, const double* S0, const gusto_lincov_opts* o);
/* Caller-owned arrays; any pointer may be NULL.  Per problem [B]: status, fail_knot, obs_knot, obs_pair, ctl_knot, ctl_entry,
 * min_z_obs, p_collision_bound, min_z_ctl.  Per knot: sigma_x, sigma_u, z_obs, and Sxx after a call with store_S = 1 (asked for
 * after a call without: GUSTO_ERR_STATE). */
typedef struct {
    int *status, *fail_knot, *obs_knot, *obs_pair, *ctl_knot, *ctl_entry;
    double *min_z_obs, *p_collision_bound, *min_z_ctl;
    double *sigma_x;   /* [B][N][x_dim]   */
    double *sigma_u;   /* [B][N-1][u_dim] */
    double *z_obs;     /* [B][N]          */
    double *Sxx;       /* [B][N][x_dim][x_dim] */
} gusto_lincov_report;
int gusto_get_lincov(gusto_handle h, gusto_lincov_report* out);
/* GPU time of the last gusto_lincov (one launch), gusto_lincov_disturbed (both launches) or gusto_lincov_dense (all four), from
 * HIP events on the handle's stream */
int gusto_last_lincov_ms(gusto_handle h, double* ms);

/* gusto_lincov with an uncertain plant (csrc/lincov.hip): the analytic counterpart of gusto_simulate_disturbed.  No counterpart
 * in the reference.  Everything gusto_lincov defines stays as it is, word for word -- sigma_x, sigma_u and the variance-below-
 * zero rule, the obstacle and control margins and their tie rules, min_z_obs / min_z_ctl with their indices, p_collision_bound,
 * status and fail_knot (K = NULL with a failed gusto_tvlqr; a non-finite entry at knot k, where Sxb now reads S_{x,[b theta]}),
 * X, U, K, S0, gusto_set_active, stream and timing, the refusals (under this call's name), the grow-only buffers, "the same bit
 * for bit in any batch and under any mask" -- and the deviation carries the plant with it:
 * Plant deviation: theta = (mass, Jdiag[0], Jdiag[1], Jdiag[2], dubins_v, dubins_k), the GUSTO_NPLANT vector of
 *   gusto_simulate_disturbed; theta_nom comes from the handle's gusto_model_params, theta~ = theta - theta_nom is constant per
 *   flight.  freeflyerSE2 reads mass and Jdiag[2], DubinsCar dubins_v and dubins_k, both Astrobee models mass and Jdiag[0 .. 2].
 * Sensitivity of the roll-out map: Cd_k = dF_k/dtheta at (X[:,k], U[:,k], theta_nom), n x GUSTO_NPLANT, k = 1 .. N-1, F_k the map
 *   of gusto_tvlqr (Nstep_b classical RK4 steps under the held control).  It is the EXACT derivative of that discrete map,
 *   forward mode through the four stages of every substep, kd = A(stage point) d + df/dtheta_j(stage point, u) with the model's
 *   own A -- not a finite difference.  Columns of entries the model does not read are zeros.  Nstep_b, dt_min and nstep are
 *   those of the handle's last gusto_tvlqr, which the call remembers.
 * Augmented deviation z = [dx; b; theta~], of size n + m + GUSTO_NPLANT, with the covariance S_k.
 * Start: S_1 = blockdiag(S0, Stheta).  S0 exactly as in gusto_lincov, the caller's or the default diagonal.  Stheta is the
 *   caller's Sth [B][GUSTO_NPLANT][GUSTO_NPLANT], or (Sth = NULL) diag((theta_nom_j plant_rel_j)^2 / 3) on the entries the
 *   model reads -- the variance of the uniform draw of gusto_simulate_disturbed with the same half-width, computed as
 *   t = nominal * rel; (t * t) / 3.  Rows and columns of entries the model does not read are zero, whatever a supplied Sth
 *   holds there.
 * Recursion, k = 1 .. N-1, with G^_k = [Ad_k - Bd_k K_k | Bd_k | Cd_k] (n x (n + m + GUSTO_NPLANT)):
 *     Sxx_{k+1} = G^_k S_k G^_k' + Bd_k diag(sw2) Bd_k',   S_{x,[b theta]}_{k+1} = G^_k S_k[:, n:],   the [b theta] block stays,
 *   sw2_i = du_white_i^2 + dw_i^2 / 3: du_white of gusto_lincov_opts, dw of gusto_disturb_opts, the convention stated for
 *   gusto_simulate_disturbed.  Sxx is computed on the upper triangle and mirrored.  In every dot product the terms gusto_lincov
 *   adds come first, in its order, the theta terms after them.
 * Commanded control: dv = [-K_k | I | 0] z + w_k, sigma_u with sw2 in place of du_white^2.
 * What the stage is NOT: it is first order in theta~ around (X, U, theta_nom).  1 / mass and 1 / J are not linear in theta:
 *   at plant_rel = 0.08 the neglected term is of relative order plant_rel^2; gusto_simulate_disturbed samples the full plant.
 * gusto_get_lincov and gusto_last_lincov_ms report the last call of either kind (the time covers both launches);
 *   gusto_get_lincov_plant answers GUSTO_ERR_STATE when the last call was a plain gusto_lincov or there was none.  Cd and Sxt
 *   of a problem that gusto_set_active leaves out are those of the last disturbed call, zeros if there was none since
 *   gusto_set_problems or a plain gusto_lincov came between.
 * GUSTO_ERR_ARG, nothing launched, the offending problem and entry in gusto_last_error: everything gusto_lincov refuses; a
 *   plant_rel outside [0, 1) or not finite; a dw that is negative or not finite; an Sth that, on the entries the model reads,
 *   is not finite, has a negative diagonal entry or is not symmetric to the bit; TrajOpt handles.  GUSTO_ERR_STATE: no
 *   problems, or no gusto_tvlqr since gusto_set_problems.
 * With d NULL or all zeros and Sth = NULL every output of gusto_get_lincov equals that of gusto_lincov with the same remaining
 *   arguments, as numbers (adding exact zeros can at most turn a -0.0 into +0.0). */
int gusto_lincov_disturbed(gusto_handle h, const double* X, const double* U, const double* K, const double* S0,
                           const double* Sth, const gusto_lincov_opts* o, const gusto_disturb_opts* d);
/* Cd [B][N-1][n][GUSTO_NPLANT]; Sxt [B][N][n][GUSTO_NPLANT], the x-theta block of S_k, after a call with store_S = 1
 * (asked for after a call without: GUSTO_ERR_STATE).  Either may be NULL. */
int gusto_get_lincov_plant(gusto_handle h, double* Cd, double* Sxt);

/* gusto_lincov_disturbed with the obstacle margins at the dense samples between the knots (csrc/lincov.hip): what
 * min_dist_dense is to gusto_verify and worst_dense_sample to gusto_simulate.  No counterpart in the reference.  Everything
 * gusto_lincov_disturbed defines stays as it is, word for word; the call runs that knot pass and adds a dense pass:
 * Dense samples: the index of gusto_simulate and gusto_interpolate, j = (k - 1) Nstep_b + i (0-based), i = 0 .. Nstep_b - 1;
 *   j = (N - 1) Nstep_b is knot N, so nfull_b = Nstep_b (N - 1) + 1.  Nstep_b, dt_min and nstep are those of the handle's last
 *   gusto_tvlqr, as gusto_lincov_disturbed takes them.
 * Nominal point of sample (k, i): xbar_{k,i}, the state after i classical RK4 substeps from X[:,k] under the held U[:,k] and
 *   theta_nom.  Every interval is restarted at its knot; the arithmetic is that of gusto_tvlqr's nominal roll-out.
 * Sensitivities inside an interval: Phi_{k,i} = d xbar_{k,i} / d x_k, Gamma_{k,i} = d / d u_k, C_{k,i} = d / d theta: the EXACT
 *   derivative of the discrete map after i substeps, forward mode through the four stages with the models' own A, B and
 *   df/dtheta -- no finite differences.  At i = 0 they are I, 0, 0.
 * Deviation at the sample: the closed loop holds u = U_k - K_k dx_k + b + w_k for the whole interval.  With z_k = [dx_k; b; theta~]
 *     dx_{k,i} = G_{k,i} z_k + Gamma_{k,i} w_k,   G_{k,i} = [Phi - Gamma K_k | Gamma | C]   (n x (n + m + GUSTO_NPLANT)),
 *     Spos_{k,i} = Gp S_k Gp' + Gammap diag(sw2) Gammap'   (WS x WS; Gp, Gammap: the first WS rows of G_{k,i}, Gamma_{k,i}),
 *   computed on the upper triangle and mirrored; S_k and sw2 are those of the knot pass.  At i = 0, and at knot N, Spos is BY
 *   DEFINITION the leading WS x WS block of the knot pass's Sxx.
 * Margin: for every pair (robot component c, keep-out component o), in gusto_lincov's order, ordinal c n_obs + o: d and nh from
 *   the signed distance at xbar_{k,i}, sigma_d = sqrt(nh' Spos nh) under the variance-below-zero rule, z = d / sigma_d with the
 *   sigma_d == 0 rule.  z_dense[j] is the smallest over the pairs, pair_dense[j] its lowest ordinal; a NaN never wins.
 *   DubinsCar, or an empty keep-out set: +inf and -1.
 * Per problem: min_z_dense, the smallest z_dense[j]; dense_sample, the first j it occurs at (0-based; -1 when it is +inf);
 *   dense_pair, the pair there (-1 likewise); nfull.  z_dense at every i = 0 sample and at knot N is z_obs of that knot, to the
 *   bit, so min_z_dense <= min_z_obs, and dense_sample sets against gusto_simulate's worst_dense_sample.
 * NO Boole bound is formed over the dense samples: neighbouring samples are strongly correlated, the sum grows with Nstep
 *   without saying more, and it would look like a probability.  p_collision_bound stays the knots' (gusto_get_lincov).
 * Status: that of the knot pass (gusto_get_lincov).  A problem with status 0 and fail_knot f from the recursion: the per-sample
 *   rows from sample (f - 1) Nstep_b on are zeros, the summary covers the samples before (none: +inf, -1, -1).  A problem dead
 *   from gusto_tvlqr: every per-sample row and min_z_dense, dense_sample, dense_pair are zero; nfull is the layout's, as ever.
 * store_dense = 1 keeps z_dense, pair_dense [B][nfull_max] and Spos [B][nfull_max][WS][WS], nfull_max = the largest nfull_b of
 *   the handle's last gusto_tvlqr (gusto_get_lincov_dense returns it); rows behind nfull[b] are zeros.
 * d NULL or all zeros with Sth = NULL gives the dense form of plain gusto_lincov.  X, U, K, S0, Sth, o, d, gusto_set_active (an
 *   inactive problem keeps what the last call with the same nfull_max wrote; zeros after new problems), stream and events, the
 *   grow-only buffers and the refusals are gusto_lincov_disturbed's, under this call's name; store_dense other than 0 / 1:
 *   GUSTO_ERR_ARG; TrajOpt handles: GUSTO_ERR_ARG.  After the call gusto_get_lincov and gusto_get_lincov_plant report its knot
 *   pass, which equals gusto_lincov_disturbed's with the same arguments bit for bit, and gusto_last_lincov_ms covers all four
 *   launches (sensitivities, knot pass, dense pass, reduction).  gusto_get_lincov_dense answers GUSTO_ERR_STATE before the
 *   first gusto_lincov_dense, after a gusto_lincov or gusto_lincov_disturbed came between, and for a per-sample array after a
 *   call without store_dense.  All reductions run in a fixed order without atomics: every dense output of a problem is the
 *   same bit for bit whatever batch it sits in and under any mask. */
int gusto_lincov_dense(gusto_handle h, const double* X, const double* U, const double* K, const double* S0,
                       const double* Sth, const gusto_lincov_opts* o, const gusto_disturb_opts* d, int store_dense);
/* Caller-owned arrays; any pointer may be NULL */
typedef struct {
    int *nfull, *dense_sample, *dense_pair;   /* [B] */
    double *min_z_dense;                      /* [B] */
    double *z_dense; int *pair_dense;         /* [B][nfull_max], store_dense = 1 */
    double *Spos;                             /* [B][nfull_max][WS][WS], store_dense = 1 */
} gusto_lincov_dense_report;
/* out and nfull_max may each be NULL */
int gusto_get_lincov_dense(gusto_handle h, gusto_lincov_dense_report* out, int* nfull_max);

/* Multi-start solves (csrc/multistart.hip): GuSTO is a local method, so one planning query is started from a fan of K initial
 * trajectories in the same launch and the best result is handed back.  No counterpart in the reference; its
 * init_traj_straightline is the start with a zero offset.  The definitions:
 * Layout: Bq queries with K starts each become the B = Bq K problems of the handle; problem b = q K + j is start j of query q.
 *   x_init, goal_lo, goal_hi [Bq][x_dim] and tf [Bq] are HOST arrays with the meaning they have in gusto_set_problems; a kernel
 *   replicates them into the handle's [B] arrays and writes the K initial trajectories of every query.  Everything
 *   gusto_set_problems does afterwards happens unchanged: the history reset, the post-solve stages (and the selection below)
 *   invalidated, every problem active again, the end of a latched scheduler error.
 * Workspace dimension: WS = 2 for freeflyerSE2 and DubinsCar, 3 for the Astrobee models.
 * End points: p_i = x_init[0:WS]; p_g the goal centre on the same entries by the straight line's rule, (lo + hi) / 2 where
 *   both are finite, else 0.  Direction d = p_g - p_i, L = |d| (hypot in the plane, sqrt(dx dx + dy dy + dz dz) in space).
 * Frame: e1 = d / L, or the first axis when L == 0.  Plane: e2 = (-e1_y, e1_x).  Space: h = hypot(e1_x, e1_y);
 *   e2 = (-e1_y, e1_x, 0) / h if h > 1e-9, else (1, 0, 0); e3 = e1 x e2.  (For 0 < h <= 1e-9 the frame is orthogonal up to h.)
 * Detour of start j: (a2, a3) = fan[j], in metres; w = a2 e2 + a3 e3.  a3 is not read in the plane.
 * Trajectory: X0[k] is the straight line's knot, (1 - t_k) x_init + t_k centre with t_k = k / (N - 1), k = 0 .. N-1, the exact
 *   expression of init_traj_straightline here; on the entries i < WS only, tent(t_k) w_i is added, tent(t) = 1 - |2 t - 1|: zero
 *   at both ends, one in the middle.  Velocities, attitude and rates stay the straight line's.  U0 = 0.
 * Zero offset: a start with a2 == a3 == 0 (in the plane: a2 == 0) skips the addition: it is the straight line bit for bit.
 * GUSTO_ERR_ARG, nothing launched, the handle left as it was: K outside 1 .. GUSTO_MAX_STARTS, Bq < 1, Bq K > batch_cap, a null
 *   array, a fan entry that is not finite, a TrajOpt handle.  All four models.
 * Keep-out sets: gusto_set_env applies as ever; gusto_set_env_batch needs B = Bq K sets, each query's repeated K times. */
#define GUSTO_MAX_STARTS 64
int gusto_set_problems_multistart(gusto_handle h, int Bq, int K, const double* x_init, const double* goal_lo,
                                  const double* goal_hi, const double* tf, const double* fan /* [K][2] */);
/* The winner of every group of K consecutive problems, selected and gathered on the device (csrc/multistart.hip).  K must lie in
 * 1 .. GUSTO_MAX_STARTS and divide the handle's B (else GUSTO_ERR_ARG); Bq = B / K.  The problems need not come from
 * gusto_set_problems_multistart.  The call completes a pending gusto_solve_async, runs on the handle's stream and changes
 * nothing else on the handle.
 * eligible [B] (HOST; nonzero = may win), or NULL = converged && successful as gusto_get_status reports them.
 * score [B] (HOST), or NULL = the last true cost, J_true[b][nJ[b] - 1] of gusto_get_history (a problem with nJ[b] == 0: NaN).
 * Winner of a query: the eligible start with the smallest score under a strict `<` in ascending j -- ties go to the lowest
 *   start; a NaN score never wins.  A query without such a start reports winner = winner_problem = -1, best_score = +inf and
 *   zero rows, the convention of gusto_get_shoot for problems that are not :Optimal.  n_eligible counts the eligible starts,
 *   whatever their scores.
 * With a caller's score and eligible the call is a general best-of-group: the report of gusto_verify, a min_z_obs of
 *   gusto_lincov or anything else the caller has can decide.  To run the post-solve stages on the winners only, pass the mask
 *   built from winner_problem to gusto_set_active.
 * One wavefront per query, reductions in a fixed order, no atomics: a query's report is the same bit for bit in any batch.
 * Both getters: GUSTO_ERR_STATE before the first gusto_select_best since the problems were set and on a handle without
 *   problems, GUSTO_ERR_ARG on a TrajOpt handle. */
int gusto_select_best(gusto_handle h, int K, const double* score /* [B] or NULL */, const int* eligible /* [B] or NULL */);
typedef struct {
    int *winner;          /* [Bq] start index j, -1: no eligible start        */
    int *winner_problem;  /* [Bq] q K + j, -1 likewise                          */
    int *n_eligible;      /* [Bq]                                               */
    double *best_score;   /* [Bq] +inf when there is no winner                  */
    double *X, *U;        /* [Bq][N][x_dim], [Bq][N][u_dim]: the winners' trajectories, zeros without a winner */
} gusto_best_report;      /* caller-owned, any pointer may be NULL */
int gusto_get_best(gusto_handle h, gusto_best_report* out);
/* the same compact buffers on the device (valid until the next gusto_select_best on the handle); any pointer may be NULL */
int gusto_get_best_dev(gusto_handle h, const double** X_dev, const double** U_dev, const int** winner_problem_dev);

/* Trajectory library (csrc/trajlib.hip): GuSTO is warm-started at its previous iterate (scp_gusto.jl:100-102), so a query that
 * starts from the solved trajectory of a similar query needs fewer trips than one that starts from the straight line.  A
 * library keeps solved trajectories on the device; every query of a batch is seeded from its K nearest entries, retargeted to
 * its own end points.  No counterpart in the reference; the definitions:
 * Object: a gusto_trajlib is bound to a model, a horizon N, a capacity cap (1 .. GUSTO_TRAJLIB_MAX_CAP entries; the device
 *   memory for all of them is allocated at creation) and a device.  Entry e stores x_init [x_dim], the goal centre c [x_dim] by
 *   the straight line's rule ((lo + hi) / 2 where both are finite, else 0), tf, an integer tag, X [N][x_dim], U [N][u_dim] and a
 *   compact feature row (below).  Entries keep their insertion order; that index is their identity.  A library is not
 *   thread-safe.  Every call that touches one returns only after its device work is complete.
 * Distance between query q and entry e, xi = x_init:
 *     d2(q, e) = sum_i w_init[i] (xi_q[i] - xi_e[i])^2 + sum_i w_goal[i] (c_q[i] - c_e[i])^2 + w_tf (tf_q - tf_e)^2
 *   accumulated in that order from 0.  The weights are fixed at creation, non-negative and finite (else GUSTO_ERR_ARG); only
 *   the entries with a positive weight are read, and only they are stored in the feature row: a freeflyerSE2 search reads 96 B
 *   per entry with the defaults, 32 B with weights on the position alone, not the trajectory.  The default, 1 on the model's
 *   x_dim entries of both vectors and w_tf = 0, is a PLACEHOLDER: the states have different units, the caller sets it (as dx0
 *   of gusto_simulate_opts).  The heading is in by default because a DubinsCar seed with another heading is a poor one.
 * Neighbours: the eligible entries of query q are all entries, or, when the query tags are given, those with tag_e == tag_q.
 *   Neighbour j of q is the j-th smallest eligible entry in ascending (d2, e): ties go to the lowest entry; an entry whose d2
 *   is NaN is never a neighbour (+inf is a number).  n_found[q] = min(K, eligible entries whose d2 is a number).
 * Layout: Bq queries with K neighbours each become the B = Bq K problems of the handle, the layout of
 *   gusto_set_problems_multistart: problem b = q K + j is seeded from neighbour j of query q, so gusto_select_best with the same
 *   K and gusto_set_active work on them unchanged.
 * Retargeting, t_k = k / (N - 1), k = 0 .. N-1, on every state entry i (the quaternion entries of AstrobeeSE3Manifold
 *   included: the affine correction the straight line gives them):
 *     X0[k][i] = X_e[k][i] + ((1 - t_k) (xi_q[i] - xi_e[i]) + t_k (c_q[i] - c_e[i])),   U0 = U_e;
 *   knot 0 is written as xi_q itself.  A query whose x_init and centre equal an entry's gets that entry's X back as numbers:
 *   only exact zeros are added.  tf is NOT retargeted: an entry solved for another tf is copied as it is.
 * Starts j >= n_found[q] report entry = -1, dist2 = +inf and are the straight line, bit for bit what gusto_set_problems with
 *   X0 = NULL writes, U0 = 0: an empty library gives K straight lines.
 * Out of scope: a diversity rule among the K neighbours, resampling between horizons (gusto_set_problems_replan below does it
 *   for a source handle, Ns != N), eviction, TrajOpt handles, more than one device (a library travels by gusto_trajlib_get and
 *   gusto_trajlib_add_host).
 * Search kernel: one wavefront per query; the lanes stride over the feature rows, each keeps its K best in registers, then K
 *   rounds of two reductions (the smallest d2, then the lowest entry among the lanes that hold it).  Fixed order, no atomics,
 *   nothing crosses a query: a query's seeds are the same bit for bit in any batch. */
#define GUSTO_TRAJLIB_MAX_K 8
#define GUSTO_TRAJLIB_MAX_CAP (1 << 20)
typedef struct gusto_trajlib_s* gusto_trajlib;
typedef struct {
    double w_init[GUSTO_MAXN], w_goal[GUSTO_MAXN];   /* weights on x_init and on the goal centre; the entries behind x_dim are ignored */
    double w_tf;
    int lds_tile;   /* 1 (default): the wavefronts of a workgroup share each tile of feature rows through LDS; 0: every wavefront
                     * reads the rows from global memory.  The same seeds bit for bit; a measurement switch (profiles/trajlib.txt) */
} gusto_trajlib_opts;
/* 1 on the model's x_dim entries of w_init and w_goal (0 behind them), w_tf = 0, lds_tile = 1 */
int gusto_default_trajlib_opts(int model_id, gusto_trajlib_opts* o);
/* opts = NULL: the defaults.  GUSTO_ERR_ARG: an unknown model, N outside 3 .. 256, cap outside 1 .. GUSTO_TRAJLIB_MAX_CAP, a weight
 * that is negative or not finite, lds_tile other than 0 / 1; GUSTO_ERR_NO_DEVICE as gusto_create */
int gusto_trajlib_create(gusto_trajlib* lib, int model_id, int N, int cap, int device, const gusto_trajlib_opts* opts);
int gusto_trajlib_destroy(gusto_trajlib lib);
const char* gusto_trajlib_last_error(gusto_trajlib lib);   /* lib = NULL: the last error of a failed creation */
int gusto_trajlib_size(gusto_trajlib lib, int* count, int* cap);   /* either pointer may be NULL */
int gusto_trajlib_clear(gusto_trajlib lib);
/* Appends the problems of handle h whose mask[b] is nonzero, in ascending b, with their current trajectories: a device-to-device
 * compaction, one kernel, the destination of a problem being the count of the selected problems before it, summed in a fixed
 * order (no atomics).  mask [B] (HOST), or NULL = converged && successful as gusto_get_status reports them; tag [B] (HOST) the
 * tags of the problems, or NULL = 0; n_added may be NULL.  The call completes a pending gusto_solve_async on h.
 * GUSTO_ERR_ARG: a model, N or device that differ, a TrajOpt handle; and a selection that does not fit the remaining
 * capacity: nothing is appended then and n_added = 0.  GUSTO_ERR_STATE: a handle without problems. */
int gusto_trajlib_add(gusto_trajlib lib, gusto_handle h, const int* mask, const int* tag, int* n_added);
/* Appends n entries from HOST arrays: x_init, goal_lo, goal_hi [n][x_dim], tf [n], tag [n] or NULL = 0, X [n][N][x_dim],
 * U [n][N][u_dim].  A non-finite x_init, tf, X or U and n above the remaining capacity are refused (GUSTO_ERR_ARG, nothing
 * appended); n = 0 is allowed. */
int gusto_trajlib_add_host(gusto_trajlib lib, int n, const double* x_init, const double* goal_lo, const double* goal_hi,
                           const double* tf, const int* tag, const double* X, const double* U);
/* Copies every entry out, [count] rows each; any pointer may be NULL.  A library written by this call and reloaded by
 * gusto_trajlib_add_host with goal_lo = goal_hi = goal_c is the same library. */
int gusto_trajlib_get(gusto_trajlib lib, double* x_init, double* goal_c, double* tf, int* tag, double* X, double* U);
/* Bq queries seeded from their K nearest entries (definitions above).  x_init, goal_lo, goal_hi [Bq][x_dim], tf [Bq] are HOST
 * arrays as in gusto_set_problems_multistart; tag [Bq] (HOST), or NULL to ignore the tags.  Afterwards everything
 * gusto_set_problems does happens unchanged: the history reset, the post-solve stages and the selection invalidated, every
 * problem active again, the end of a latched scheduler error.
 * GUSTO_ERR_ARG, nothing launched, the handle left as it was: K outside 1 .. GUSTO_TRAJLIB_MAX_K, Bq < 1, Bq K > batch_cap, a
 *   null array (tag excepted), a null library, a TrajOpt handle, a library of another model, N or device. */
int gusto_set_problems_trajlib(gusto_handle h, gusto_trajlib lib, int Bq, int K, const double* x_init, const double* goal_lo,
                               const double* goal_hi, const double* tf, const int* tag);
/* The seeds of the last gusto_set_problems_trajlib: entry [B] (-1: the straight line), dist2 [B] (+inf likewise), n_found [Bq];
 * any pointer may be NULL.  GUSTO_ERR_STATE when the handle's problems were set by another call. */
int gusto_get_trajlib_seeds(gusto_handle h, int* entry, double* dist2, int* n_found);
/* GPU time of search plus retargeting of that call, from HIP events on the handle's stream */
int gusto_last_trajlib_ms(gusto_handle h, double* ms);

/* Receding-horizon replanning (csrc/replan.hip): after a few knots of flight the robot is not on its plan, and a new plan is
 * wanted from the measured state to the same goal in the time that is left.  GuSTO is warm-started at its previous iterate
 * (scp_gusto.jl:100-102), so the solved plan, shifted in time and bent to the new start, is the seed; the trajectory library is
 * the same idea across queries, this one along time.  No counterpart in the reference; the definitions:
 * Source handle: src = NULL means h itself; src has the model and the device of h, its horizon Ns may differ from the N of h.
 * Source rows: GUSTO_REPLAN_TRAJ: source problem b is problem b of src, with its current X [Ns][x_dim], U [Ns][u_dim], tf_s,
 *   goal_lo and goal_hi; B <= the B of src.  GUSTO_REPLAN_BEST: source b is query b of the last gusto_select_best on src: X and U
 *   are row b of the compact winner buffers, tf_s and the goals those of problem winner_problem[b]; B <= Bq; src may be h.
 * Inputs: tau [B] (HOST), the fraction of the source's time already flown, 0 <= tau < 1; x_now [B][x_dim] (HOST), the state to
 *   start from, finite.
 * New problem b: x_init = x_now, tf' = (1 - tau) tf_s, and the caller's goal_lo / goal_hi (HOST, [B][x_dim], both or neither);
 *   NULL: the source problem's goals, copied as they are.
 * Seeded: seeded[b] = mask[b] != 0 when mask [B] (HOST) is given; without it the source problem is converged && successful as
 *   gusto_get_status reports them (TRAJ), or the query has a winner (BEST).  A BEST query without a winner is never seeded,
 *   whatever the mask says; it takes tf_s and its goals from problem b K of src.
 * Seeded start: t_k = k / (N - 1), k = 0 .. N-1, evaluated in this order:
 *     sigma_k = (tau (N - 1 - k) + k) (Ns - 1) / (N - 1),   j = min(floor(sigma_k), Ns - 2),   a = sigma_k - j
 *     S_k = (1 - a) X_s[j] + a X_s[j + 1],   U0[k] = (1 - a) U_s[j] + a U_s[j + 1]
 *     X0[k][i] = S_k[i] + ((1 - t_k) (x_now[i] - S_0[i]) + t_k (c_new[i] - c_old[i]))
 *   with c the goal centre by the straight line's rule ((lo + hi) / 2 where both are finite, else 0); the t_k term is skipped
 *   entirely when no goals are passed.  Knot 0 is written as x_now itself; for knot N - 1, S and U0 are the source's last knot
 *   itself.  The quaternion entries of AstrobeeSE3Manifold get the same affine treatment as in gusto_set_problems_trajlib.
 * Identity: with tau = 0, Ns = N, x_now = X_s[0] and no goals the result is the source trajectory as numbers: only exact zeros
 *   are added.
 * Unseeded start: the straight line from x_now to the goal centre, U0 = 0: bit for bit what gusto_set_problems with X0 = NULL
 *   writes for that x_init, goal and tf'.
 * Afterwards everything gusto_set_problems does happens unchanged: the history reset, the post-solve stages and the selection
 *   invalidated, every problem active again, the end of a latched scheduler error.  The B of h becomes B.
 * GUSTO_ERR_ARG: a TrajOpt handle on either side, another model or device, B < 1, B > the batch_cap of h, B above the source's
 *   count, an unknown source, a null tau or x_now, exactly one goal array, a tau outside [0, 1) or NaN, an x_now that is not
 *   finite.  GUSTO_ERR_STATE: a source without problems, BEST before a gusto_select_best.  A refused call launches nothing that
 *   touches the problem arrays of h and leaves h as it was.
 * Kernel: a thread per (problem, knot), consecutive threads on consecutive knots; no atomics, nothing crosses a problem: a
 *   problem's start is the same bit for bit in any batch.  When source and destination share memory (src = h) the source rows are
 *   read from a staging copy made on the stream, device to device.
 * Out of scope: TrajOpt handles; carrying Delta / omega over (gusto_set_trust_state exists for that); a changed N of h itself;
 *   more than one device. */
enum { GUSTO_REPLAN_TRAJ = 0, GUSTO_REPLAN_BEST = 1 };
int gusto_set_problems_replan(gusto_handle h, gusto_handle src, int source, int B, const double* tau, const double* x_now,
                              const double* goal_lo, const double* goal_hi, const int* mask);
/* The same from the stored closed-loop knots of src, GUSTO_REPLAN_TRAJ only: tau_b = knot_b / (Ns - 1) with knot_b in
 * 0 .. Ns - 2, and x_now[b] = Xcl[b][knot_b][sample][:], read on the device from the knots the last gusto_simulate or
 * gusto_simulate_disturbed on src stored (store_knots = 1; sample < n_samples): a kernel gathers the B x_dim values into a
 * staging buffer, which comes to the host in one copy.  An integer knot only: a replan between knots goes through the general
 * call with any tau.  GUSTO_ERR_ARG also: a null knot, a knot or sample out of range, a stored state that is not finite (a
 * sample flagged non-finite).  GUSTO_ERR_STATE also: no stored knots on src. */
int gusto_set_problems_replan_knots(gusto_handle h, gusto_handle src, int B, const int* knot, int sample,
                                    const double* goal_lo, const double* goal_hi, const int* mask);
/* What the last of the two calls above used: seeded [B], tau [B], x_now [B][x_dim]; any pointer may be NULL.  GUSTO_ERR_STATE
 * when the handle's problems were set by another call. */
int gusto_get_replan(gusto_handle h, int* seeded, double* tau, double* x_now);
/* GPU time of that call (copies, staging and the kernel), from HIP events on the stream of h; GUSTO_ERR_STATE likewise */
int gusto_last_replan_ms(gusto_handle h, double* ms);

/* Risk-tightened keep-out sets (csrc/tighten.hip): gusto_lincov says how many standard deviations of closed-loop dispersion lie
 * between a plan and the nearest keep-out component; this call feeds that back into planning.  From a caller's BASE keep-out
 * tables and the covariances of the last gusto_lincov it writes per-problem tables into the handle, where gusto_set_env_batch
 * puts its own, so that the next gusto_solve plans around them.  The solver's obstacle rows look at robot component 0 only (the
 * reference does: freeflyer_se2.jl:251,273) while gusto_verify and gusto_lincov look at every component, so every keep-out
 * component is first extended over the component offsets, then grown.  No counterpart in the reference; the definitions, for one
 * problem, WS = 2 in the plane and 3 in space:
 * Base set: n_box / box_min_max / n_sph / sph_c_r in the form of gusto_set_env_batch.  n_env = 1: one set for all B problems;
 *   n_env = B: one per problem; at most 64 components per problem.  The handle's current tables are NOT read: a caller that
 *   passes the same base every time never compounds margins.
 * Inputs from the handle: the last gusto_lincov, gusto_lincov_disturbed or gusto_lincov_dense since gusto_set_problems*, which
 *   must have run with store_S = 1 (else GUSTO_ERR_STATE): its Sxx [N][x_dim][x_dim], its per-problem status, and the X that call
 *   saw (its copy of a caller's X, or the handle's own trajectories).
 * Per pair: for robot component c, base component i and knot k, the signed distance d at X[:,k] and its outward normal nh, and
 *     sigma_d = sqrt(max(0, nh' Sxx_k[0:WS, 0:WS] nh)),   z = d / sigma_d   (sigma_d == 0: the sign of d decides, +-inf)
 *   exactly as gusto_lincov defines them.
 * Margin of base component i:
 *     m_i = min(margin_cap, max over the (c, k) with d - kappa sigma_d <= reach of max(0, kappa sigma_d - slack))
 *   (0 when no pair counts).  With monotone = 1, m_i = max(m_i, previous m_i).  A NaN never wins a maximum.
 * Previous margins: those the last gusto_tighten_env on this handle wrote for this problem, if that call had the same B and the
 *   problem the same n_box and n_sph; zeros otherwise.  gusto_set_env and gusto_set_env_batch drop them; gusto_set_problems*
 *   does not (a driver sets problems again between two calls).
 * Cover (cover_components = 1): omax_j, omin_j = the largest and smallest of comp_off[c][j] - comp_off[0][j] over the robot's
 *   components, j < WS (component 0 contributes 0).  A box becomes [lo - omax, hi - omin]; a sphere gets the centre
 *   c - (omax + omin) / 2 and the radius R + |(omax - omin) / 2|.  cover_components = 0: omax = omin = 0.
 * Grow: a box becomes [(lo - omax) - m_i, (hi - omin) + m_i] in the first WS coordinates, the others are copied; a sphere's
 *   radius becomes (R + |(omax - omin) / 2|) + m_i.  With cover off and m_i = 0 the component is the base one bit for bit.
 * Guarantee (cover on): for every location q and component c, the signed distance of component 0 at q to the tightened component
 *   is at most the signed distance of component c at q to the base component, minus m_i (up to rounding).
 * Report, per problem [B]: min_z_base, knot, pair -- gusto_lincov's min_z_obs, obs_knot (1-based; 0: +inf) and obs_pair (ordinal
 *   c n_obs + i; -1: +inf) with its tie rules, but on the BASE set: independent of cover and margins.  max_margin the largest
 *   m_i, n_grown the number of components with m_i > 0, blocked = 1 when x_init, or the goal centre (goal_lo + goal_hi) / 2
 *   where its first WS entries are finite, has a negative component-0 signed distance to a component of the problem's own
 *   tightened set.  margin [B][n_obs_max], n_obs_max the largest component count of the call: zeros behind a problem's own count.
 * Skipped problems: inactive under gusto_set_active, or gusto_lincov status 0.  status = 0 (else 1), min_z_base, knot and pair
 *   zero; the margins are the previous ones, and the problem's tables are still written, as cover plus those margins, so the
 *   handle's set is whole; max_margin, n_grown and blocked describe those tables.
 * Afterwards the handle holds per-problem tables for B problems (as after gusto_set_env_batch) and the next gusto_solve reads
 *   them.  Trajectories, status, histories and the results of the post-solve stages are untouched.
 * GUSTO_ERR_ARG: a TrajOpt handle, DubinsCar, n_env neither 1 nor B, more than 64 components or a negative count, a null or
 *   non-finite table, kappa or slack negative or not finite, margin_cap negative or NaN, reach NaN, a flag other than 0 / 1.
 *   GUSTO_ERR_STATE: a handle without problems, no covariances.  A refused call leaves the handle as it was.
 * Kernel: one wave per problem, a lane per keep-out component, the knots in sequence; reductions in a fixed order, no atomics:
 *   a problem's outputs are the same bit for bit in any batch.  The call runs on the handle's stream after any pending
 *   gusto_solve_async and is timed with events of its own.
 * Out of scope: margins on the controls, per-knot margins, margins from the dense samples, TrajOpt handles. */
typedef struct {
    double kappa;          /* margin in standard deviations; finite, >= 0; default 3 */
    double slack;          /* m = max(0, kappa sigma_d - slack); finite, >= 0; default 0 */
    double margin_cap;     /* upper bound of a component's margin; >= 0, may be +inf; default +inf */
    double reach;          /* a (component, obstacle) pair counts at knot k only if d - kappa sigma_d <= reach; default +inf */
    int cover_components;  /* 1: extend every obstacle over the robot's component offsets first; default 1 */
    int monotone;          /* 1: a margin never falls below the one the previous call wrote for this problem; default 1 */
} gusto_tighten_opts;
int gusto_default_tighten_opts(int model_id, gusto_tighten_opts* o);
int gusto_tighten_env(gusto_handle h, int n_env, const int* n_box, const double* box_min_max, const int* n_sph,
                      const double* sph_c_r, const gusto_tighten_opts* o);
typedef struct {
    int *status, *knot, *pair, *n_grown, *blocked;   /* [B] */
    double *min_z_base, *max_margin;                 /* [B] */
    double *margin;                                  /* [B][n_obs_max] */
} gusto_tighten_report;                              /* caller-owned, any pointer may be NULL */
/* The report of the last gusto_tighten_env since gusto_set_problems* (none: GUSTO_ERR_STATE); out = NULL: n_obs_max alone */
int gusto_get_tighten(gusto_handle h, gusto_tighten_report* out, int* n_obs_max);
/* The handle's current keep-out tables in the form of gusto_set_env_batch: *n_env = 1 after gusto_set_env (or before any), else
 * the number of problems; n_box, n_sph [n_env]; the tables.  Any pointer may be NULL: a size query passes the arrays as NULL. */
int gusto_get_env(gusto_handle h, int* n_env, int* n_box, double* box_min_max, int* n_sph, double* sph_c_r);
/* GPU time of the last gusto_tighten_env (copies and the kernel), from HIP events on the handle's stream */
int gusto_last_tighten_ms(gusto_handle h, double* ms);

/* Roadmap seeds (csrc/roadmap.hip): GuSTO is a local method, and the fan, the library and replanning all start from the straight
 * line or from earlier plans; none looks at the keep-out set before the first solve.  This call does: every query starts from a
 * shortest collision-free polyline through the corners of its inflated keep-out set (a visibility graph), its alternates from
 * the shortest paths that avoid the corners of one more component each.  No counterpart in the reference, whose
 * init_traj_straightline is what a query with an unblocked line gets.  The definitions, WS = 2 in the plane and 3 in space:
 * Layout: that of gusto_set_problems_multistart.  Bq queries with K alternates each, 1 <= K <= GUSTO_ROADMAP_MAX_K, become the
 *   B = Bq K problems of the handle; problem b = q K + j is alternate j of query q.  x_init, goal_lo, goal_hi [Bq][x_dim] and tf
 *   [Bq] are HOST arrays; everything gusto_set_problems does afterwards happens unchanged.
 * Keep-out set: the handle's current tables.  After gusto_set_env the set is shared by the batch; after gusto_set_env_batch or
 *   gusto_tighten_env the handle must hold Bq K sets (else GUSTO_ERR_STATE) and query q uses the set of problem q K.  Components
 *   come in table order, boxes then spheres, C <= 64; without components every query is DIRECT.  Coordinates are the first WS of
 *   min, max and centre: the planar reading the solver has for WS = 2.
 * Blocking sets: box i blocks the open box (lo - inflate, hi + inflate), the L-infinity inflation, a superset of the disc's;
 *   sphere i blocks the open ball of radius R + inflate.
 * Nodes: node 0 is x_init[0:WS]; node 1 the goal centre on those entries by the straight line's rule; node 2 + 2^WS i + c is
 *   corner c of component i, bit j of c choosing the low or the high side: (lo_j - inflate) - pad or (hi_j + inflate) + pad for
 *   a box, c_j -+ ((R + inflate) + pad) for a sphere.  A node strictly inside any blocking set is dead; so are the nodes of a
 *   banned component (the component itself still blocks).
 * Edges: two live nodes see each other when the segment between them meets no blocking set; the length of an edge is
 *   sqrt(sum d_j^2) in coordinate order.
 * Status of a search: GUSTO_ROADMAP_END_BLOCKED node 0 or node 1 is dead, else GUSTO_ROADMAP_DIRECT 0 sees 1, else
 *   GUSTO_ROADMAP_PATH a path was found, GUSTO_ROADMAP_NO_PATH none exists, GUSTO_ROADMAP_TOO_LONG the shortest one has more than
 *   GUSTO_ROADMAP_MAX_VIA interior nodes.
 * Shortest path: Dijkstra from node 0 -- the unsettled node of smallest distance goes next, ties to the lowest index; a
 *   predecessor changes on a strict `<` only; the search stops when node 1 is settled.
 * Alternates: alternate 0 has no ban.  After alternate j - 1 the component that owns its first interior node joins the ban list;
 *   alternate j is the shortest path under that list.  Once an alternate is not PATH, it and all later ones are the straight
 *   line with the status, length and ban list of that alternate and n_via = 0.
 * straight_first = 1: problem q K is the straight line and the alternates follow, problem q K + 1 + j is alternate j; with K >= 2
 *   that is the pair a gusto_select_best decides.  The row of problem q K is that of alternate 0 when it is not PATH, else
 *   status GUSTO_ROADMAP_STRAIGHT, n_via = 0, length +inf and an empty ban list.
 * Seed of a PATH alternate: Lp the length of the polyline node 0, interior nodes, node 1, summed from node 0; t_k = k / (N - 1).
 *   The first WS entries of X0[k] are the point at arc length t_k Lp on the polyline: on the first segment i whose end lies beyond
 *   that length (the last one otherwise), P_i + ((t_k Lp - cum_i) / len_i) (P_{i+1} - P_i).  Knot 0 is written as x_init's own
 *   entries and knot N - 1 as the goal centre's.  Every other entry is the straight line's expression, as the fan writes it;
 *   U0 = 0.  Any other status is the straight line, bit for bit what gusto_set_problems with X0 = NULL writes.
 * Options: inflate and pad default to radius + 0.02 and 0.03 -- placeholders taken from the table study of profiles/roadmap.txt
 *   (the planar obstacle table, N = 50), not tuned for anything else.
 * Report: all arrays [Bq K], caller-owned, any pointer may be NULL.  via: node indices, -1 behind n_via; length: Lp for PATH, the
 *   distance from node 0 to node 1 for DIRECT, +inf otherwise; banned: the ban list the alternate was searched under, component
 *   indices, -1 behind the count; stage_ms [3]: GPU time of the graph kernel (with the copies), the search and the seed kernel.
 * GUSTO_ERR_ARG, nothing launched, the handle left as it was: K outside 1 .. GUSTO_ROADMAP_MAX_K, Bq < 1, Bq K > batch_cap, a
 *   null array, options that are not finite or out of range, a TrajOpt handle.  All four models, one device.
 * Kernels: the graph once per keep-out set (a wave per node and block of 64 nodes, the visibility matrix as a bit mask), the
 *   search with one wavefront per query, the seed with a thread per knot; they run on the handle's stream and are timed together
 *   with events.  No atomics, reductions in a fixed order: a query's outputs are the same bit for bit in any batch, and for a
 *   shared set or the same set passed per problem. */
#define GUSTO_ROADMAP_MAX_K 8
#define GUSTO_ROADMAP_MAX_VIA 16
#define GUSTO_ROADMAP_DIRECT 0
#define GUSTO_ROADMAP_PATH 1
#define GUSTO_ROADMAP_END_BLOCKED 2
#define GUSTO_ROADMAP_NO_PATH 3
#define GUSTO_ROADMAP_TOO_LONG 4
#define GUSTO_ROADMAP_STRAIGHT 5
typedef struct {
    double inflate;       /* growth of every component before it blocks; finite, >= 0; default radius + 0.02 (placeholder) */
    double pad;           /* distance of the corner nodes from the blocking sets; finite, > 0; default 0.03 (placeholder) */
    int straight_first;   /* 1: problem q K is the straight line, the alternates follow; default 0 */
} gusto_roadmap_opts;
int gusto_default_roadmap_opts(int model_id, gusto_roadmap_opts* o);
int gusto_set_problems_roadmap(gusto_handle h, int Bq, int K, const double* x_init, const double* goal_lo,
                               const double* goal_hi, const double* tf, const gusto_roadmap_opts* o /* NULL: the defaults */);
typedef struct {
    int *status, *n_via;   /* [Bq K] */
    int *via;              /* [Bq K][GUSTO_ROADMAP_MAX_VIA] */
    double *length;        /* [Bq K] */
    int *banned;           /* [Bq K][GUSTO_ROADMAP_MAX_K] */
    double *stage_ms;      /* [3] graph, search, seed */
} gusto_roadmap_report;    /* caller-owned, any pointer may be NULL */
/* The report of the last gusto_set_problems_roadmap since the problems were set (none: GUSTO_ERR_STATE) */
int gusto_get_roadmap(gusto_handle h, gusto_roadmap_report* out);
/* GPU time of the last gusto_set_problems_roadmap (copies and the three kernels), from HIP events on the handle's stream */
int gusto_last_roadmap_ms(gusto_handle h, double* ms);

/* Final-time search (csrc/tfsearch.hip): per query the shortest final time whose solve is eligible, found by K-section over
 * solves.  The reference's free final time is a variable with the single row Tf >= 0.1 that nothing moves, so every solve runs at
 * the caller's guess; Tf does not become a variable of the subproblem here either -- the search runs around gusto_solve:
 *     gusto_tfsearch_begin; repeat { gusto_solve; gusto_tfsearch_update; } while queries are searching; gusto_get_tfsearch.
 * Bracket, incumbent plans, candidates and seeds stay on the device between the launches.  The definitions:
 * Layout: that of gusto_set_problems_multistart.  Bq queries with K candidate final times each, 1 <= K <= GUSTO_MAX_STARTS, are
 *   the B = Bq K problems of the handle; problem b = q K + j is candidate j of query q and its tf is the candidate T_j.  x_init,
 *   goal_lo, goal_hi [Bq][x_dim] and the range tf_lo, tf_hi [Bq] (NULL: the options' value for every query) are HOST arrays;
 *   gusto_set_env_batch needs B sets, as for multi-start.  After begin, and after every update, everything gusto_set_problems
 *   does has happened: history reset, stages and selection invalidated, every problem active (but those of a done query, below).
 * Per query: the bracket lo, hi and the caller's lo0, hi0; the incumbent -- tf_best, its X [N][x_dim] and U [N][u_dim] as the
 *   solve left them, J_best its last J_true (NaN when it has none), round_found (-1: no incumbent, tf_best NaN) --; the status
 *   word; the current candidates.
 * Candidates: w = hi - lo.  Round 0 (no incumbent): T_j = lo + (j + 1) (w / K) for j < K - 1 and T_{K-1} = hi itself.  With an
 *   incumbent hi is known good: T_j = lo + (j + 1) (w / (K + 1)), j = 0 .. K - 1.  One rounded difference, division, product and
 *   sum in IEEE double, nothing fused.  K = 1 is bisection after the first round.
 * Seeds.  GUSTO_TFSEARCH_SEED_LINE, or a query without an incumbent: the straight line and U0 = 0, bit for bit what
 *   gusto_set_problems with X0 = NULL writes for that x_init, goal and tf.  GUSTO_TFSEARCH_SEED_INCUMBENT with an incumbent: the
 *   incumbent retimed, s = tf_best / T_j: X0[k][i] = X_inc[k][i] outside the rate entries R, s X_inc[k][i] + (1 - s) L_k[i] on
 *   them (L_k the straight line's knot), U0[k] = (s s) U_inc[k], knot 0 x_init itself.  R: FreeflyerSE2 {3, 4, 5}, AstrobeeSE3
 *   {3, 4, 5, 9, 10, 11}, AstrobeeSE3Manifold {3, 4, 5, 10, 11, 12}.  Time scaling is an exact symmetry of these models (double
 *   integrator, attitude kinematics, Euler's equations) and of their trapezoid rows: the position and attitude rows of the
 *   collocation defect are unchanged, the rate rows multiplied by s; the (1 - s) L term only restores non-zero end rates.  The
 *   speed of DubinsCar is a constant of the model, nothing retimes: GUSTO_TFSEARCH_SEED_INCUMBENT is GUSTO_ERR_ARG there.
 * Update, after a solve of the round's problems.  T_j is the problem's tf on the device; ok_j is eligible[q K + j] != 0 (a HOST
 *   array [B]) or, for NULL, converged && successful.
 *   1. F' = the smallest T_j with ok_j, ties to the lowest j.  If it exists and there is no incumbent or F' < tf_best (strict),
 *      that problem becomes the incumbent; round_found = the number of updates before this one.  n_eligible = |{j : ok_j}|.
 *   2. F = tf_best.  With an incumbent hi = F and lo = max({lo0}, {lo_old if lo_old < F}, {T_j : !ok_j, T_j < F}); without one
 *      lo = max_j T_j and hi = hi0.
 *   3. Status bits: GUSTO_TFSEARCH_NONE no incumbent after a round; GUSTO_TFSEARCH_DONE hi - lo <= rtol hi (a rounded difference
 *      and product); GUSTO_TFSEARCH_FLOOR lo == lo0, the lower end was never refuted and the answer may lie below the range;
 *      GUSTO_TFSEARCH_NONMONOTONE some i < j with ok_i && !ok_j, or lo_old >= F, in this or an earlier round.  NONE or DONE: the
 *      query is done.
 *   4. A searching query gets the next candidates and their seeds.  A done query is not touched by later updates; its K
 *      problems become the straight line at tf = hi (so do its candidates) and are inactive (gusto_set_active) in later solves.
 *   No rule assumes that the verdicts are monotone in tf.  After round 0 hi - lo <= w0 / K, and after every further round the
 *   width is at most the previous one divided by K + 1, up to the roundings of the candidates.
 * GUSTO_ERR_ARG, nothing launched, the handle left as it was: a TrajOpt handle, K outside 1 .. GUSTO_MAX_STARTS, Bq < 1,
 *   Bq K > batch_cap, a null x_init or goal array, a query whose range is not 0 < tf_lo < tf_hi < inf, rtol outside [1e-6, 1),
 *   an unknown seed, DubinsCar with GUSTO_TFSEARCH_SEED_INCUMBENT.  GUSTO_ERR_STATE: update or a getter before begin or after any
 *   other gusto_set_problems* call on the handle; update when no query is searching; update with eligible = NULL and no
 *   gusto_solve / gusto_solve_async since the last begin or update.
 * Kernels: begin with a thread per candidate, update with one wavefront per query (lane j = candidate j), seed with a thread
 *   per (problem, knot); on the handle's stream, timed with events.  An update reads the Bq status words back, nothing else.
 *   No atomics, nothing crosses a query: a query's report and seeds are the same bit for bit in any batch. */
enum { GUSTO_TFSEARCH_SEED_LINE = 0, GUSTO_TFSEARCH_SEED_INCUMBENT = 1 };
#define GUSTO_TFSEARCH_NONE 1
#define GUSTO_TFSEARCH_DONE 2
#define GUSTO_TFSEARCH_FLOOR 4
#define GUSTO_TFSEARCH_NONMONOTONE 8
typedef struct {
    double tf_lo, tf_hi;   /* used where the per-query arrays are NULL; 0 < tf_lo < tf_hi, finite; default 1, 100 (placeholders) */
    double rtol;           /* a query is done when hi - lo <= rtol * hi; in [1e-6, 1); default 0.01 */
    int seed;              /* GUSTO_TFSEARCH_SEED_*; default INCUMBENT (DubinsCar: LINE) */
} gusto_tfsearch_opts;
int gusto_default_tfsearch_opts(int model_id, gusto_tfsearch_opts* o);
int gusto_tfsearch_begin(gusto_handle h, int Bq, int K, const double* x_init, const double* goal_lo, const double* goal_hi,
                         const double* tf_lo /* [Bq] or NULL */, const double* tf_hi /* [Bq] or NULL */,
                         const gusto_tfsearch_opts* o /* NULL: the defaults */);
int gusto_tfsearch_update(gusto_handle h, const int* eligible /* [B] HOST, or NULL = converged && successful */);
typedef struct {
    int *status, *round_found, *n_eligible;   /* [Bq]; n_eligible: of the query's last round */
    double *lo, *hi, *tf_best, *J_best;       /* [Bq] */
    double *cand;                             /* [Bq][K] */
    double *X, *U;                            /* [Bq][N][x_dim], [Bq][N][u_dim]: the incumbents (zeros before the first) */
} gusto_tfsearch_report;                      /* caller-owned, any pointer may be NULL */
/* The search's report; *round the number of updates so far, *n_searching the queries neither NONE nor DONE (either may be NULL) */
int gusto_get_tfsearch(gusto_handle h, gusto_tfsearch_report* out, int* round, int* n_searching);
/* Device pointers to the incumbents [Bq][N][x_dim], [Bq][N][u_dim] and tf_best [Bq], valid until the next begin */
int gusto_get_tfsearch_dev(gusto_handle h, const double** X_dev, const double** U_dev, const double** tf_best_dev);
/* GPU time of the last begin or update (copies and kernels), from HIP events on the handle's stream */
int gusto_last_tfsearch_ms(gusto_handle h, double* ms);

/* Goal timeline (csrc/legs.hip): the goals of a query before its final time, flown as legs and joined on the device.  A GoalSet
 * of the reference is keyed by time and Goal(params, t_guess, ...) may sit at any t_guess (src/goals.jl:18-30), but every goal
 * row function hard-codes knot N, so a goal before the final time is carried and ignored by the solve -- there and in
 * gusto_solve.  No solve kernel changes here either: the timeline runs around gusto_solve,
 *     gusto_legs_begin; repeat { gusto_solve; gusto_legs_advance; } while n_flying > 0; gusto_get_legs.
 * Every goal interval is a LEG, an ordinary problem: start at the previous junction, goal rows of that goal, tf the interval.
 * The definitions:
 * Timeline.  Query q has L_q = n_legs[q] goals (NULL: L for every query), 1 <= L_q <= L <= GUSTO_MAX_STARTS, at the times
 *   T_0 < T_1 < ... < T_{L_q - 1}, finite, T_0 > 0 (t_goal [Bq][L]; entries behind L_q are not read).  Goal l is goal_lo/hi[q][l]
 *   ([Bq][L][x_dim]) under the rules of gusto_set_problems: lo == hi a point row, lo != hi a box row on every finite side, +-Inf
 *   no goal on that side.  Leg l has tf_l = T_l - T_{l-1}, one rounded difference, and tf_0 = T_0 itself.  All arrays are HOST.
 * Modes (gusto_legs_opts.mode).  GUSTO_LEGS_SEQUENTIAL: the handle holds B = Bq problems, problem q is the query's current leg;
 *   round r (the number of advances so far) solves leg r of every query that still flies.  The state a leg arrives in is the
 *   state the next leg starts from: the mode for junctions a goal leaves partly free (position-only waypoints).  It is greedy:
 *   leg l arrives as is cheapest for itself, the state at a partly free junction is not optimised across legs.
 *   GUSTO_LEGS_PARALLEL: the multi-start layout, B = Bq L, problem b = q L + l is leg l; one launch solves all legs and one
 *   advance joins them.  Refused (GUSTO_ERR_ARG) unless every interior goal (l < L_q - 1) of every query pins every entry, lo ==
 *   hi finite: leg l + 1 then starts from that point.  Problems l >= L_q of a ragged query are the straight line of the query's
 *   last leg, and inactive (gusto_set_active).  GUSTO_LEGS_AUTO (the default): PARALLEL where allowed, else SEQUENTIAL.
 *   gusto_set_env_batch needs B sets as laid out: Bq for SEQUENTIAL, Bq L for PARALLEL.
 * Leg problem: x_init the junction (x_init[q] for leg 0), the goal goal l, tf = tf_l.  Its seed is the straight line with U0 =
 *   0, bit for bit what gusto_set_problems with X0 = NULL writes for those inputs.  After begin, and after every advance,
 *   everything gusto_set_problems does has happened: history reset, stages and selection invalidated, every problem active but
 *   those named inactive here.
 * Advance, SEQUENTIAL, after a solve of round r.  ok_q is eligible[q] != 0 (a HOST array [B]) or, for NULL, converged &&
 *   successful as gusto_get_status reports them.  For every flying query: (1) leg r is STORED: its X, U go to the joined
 *   buffers, its iterations, converged, successful, stop reason and last J_true (NaN when it has none) to the report; (2) ok_q
 *   and r + 1 < L_q: the junction is X_r[N-1] as stored, copied not recomputed; it becomes x_init of leg r + 1, whose seed is
 *   written, and the query keeps flying; (3) ok_q and r + 1 == L_q: status DONE; (4) !ok_q: status FAILED, failed_leg = r, no
 *   later leg is run.  A finished query's problem becomes the straight line of the leg it flew last and is inactive in later
 *   solves; later advances do not touch its report.
 * Advance, PARALLEL: once, eligible [B] over the problems.  Every leg l < L_q is stored; failed_leg is the first leg that is
 *   not ok, else the status is DONE.  Every problem becomes the straight line of its own leg and is inactive afterwards.
 * Join.  Nj = L (N - 1) + 1 knots per query; rows behind the last stored leg are zeros.  Stored leg l fills the knots l (N - 1)
 *   ... (l + 1)(N - 1).  X at a junction knot is leg l's last knot; U there is leg l + 1's U[0] -- leg l's U[N-1] is the
 *   reference's free u_N and is dropped --, and the last knot of the last stored leg takes that leg's U[N-1].
 *   t[l (N - 1) + k] = T_{l-1} + k (tf_l / (N - 1)) with T_{-1} = 0: one division, product and sum in IEEE double, nothing fused,
 *   and T_l itself for k = N - 1.  Everything else is copies.
 * Report, per query: status (one of the bits GUSTO_LEGS_FLYING / DONE / FAILED), failed_leg (-1: none), n_done (the legs that
 *   arrived: stored and ok, before the first that is not), J_total (the sum of the stored legs' J, in leg order).  Per query and
 *   leg [Bq][L] (zeros where no leg is stored): iterations, converged, successful, stop_reason, J; gap = max_i |X_l[0][i] -
 *   junction[i]|, the residual of the hard init row as the solve left it, and 0 for leg 0; arrive = the largest violation of goal
 *   l's rows at the leg's last knot: |x - lo| on point entries, max(lo - x, x - hi, 0) on the others.  And the joined X, U, t.
 * GUSTO_ERR_ARG, nothing launched, the handle left as it was: a TrajOpt handle, L outside 1 .. GUSTO_MAX_STARTS, an n_legs[q]
 *   outside 1 .. L, Bq < 1, B > batch_cap, a null x_init, goal or t_goal, times not finite or not strictly increasing from > 0, a
 *   non-finite x_init, an unknown mode, PARALLEL with an interior goal that is not a full point.  GUSTO_ERR_STATE: advance or a
 *   getter before begin or after any other gusto_set_problems* call on the handle; advance with n_flying == 0; advance with
 *   eligible = NULL and no gusto_solve / gusto_solve_async since the last begin or advance.
 * Kernels: begin with a thread per (problem, knot); advance with a thread per (leg in flight, knot), which copies the knot into
 *   the joined buffers and writes the next leg's seed knot -- the thread of knot 0 also the leg's report row and the problem's
 *   inputs --, behind one wavefront per leg that forms gap and arrive; on the handle's stream, timed with events.  The rows a
 *   SEQUENTIAL advance reads are a staging copy: it writes the problem it reads.  An advance reads the Bq status words back,
 *   nothing else.  No atomics, nothing crosses a query: a query's report, joined buffers and seeds are the same bit for bit in
 *   any batch.  Out of scope: TrajOpt handles, a different N per leg, post-solve stages on the joined trajectory (they run per
 *   leg on the handle). */
enum { GUSTO_LEGS_AUTO = 0, GUSTO_LEGS_SEQUENTIAL = 1, GUSTO_LEGS_PARALLEL = 2 };
#define GUSTO_LEGS_FLYING 1
#define GUSTO_LEGS_DONE 2
#define GUSTO_LEGS_FAILED 4
typedef struct {
    int mode;              /* GUSTO_LEGS_*; default AUTO */
} gusto_legs_opts;
int gusto_default_legs_opts(int model_id, gusto_legs_opts* o);
int gusto_legs_begin(gusto_handle h, int Bq, int L, const int* n_legs /* [Bq] or NULL = L */, const double* x_init /* [Bq][x_dim] */,
                     const double* goal_lo, const double* goal_hi /* [Bq][L][x_dim] */, const double* t_goal /* [Bq][L] */,
                     const gusto_legs_opts* o /* NULL: the defaults */);
int gusto_legs_advance(gusto_handle h, const int* eligible /* [B] HOST, or NULL = converged && successful */);
typedef struct {
    int *status, *failed_leg, *n_done;                        /* [Bq] */
    double *J_total;                                          /* [Bq] */
    int *iterations, *converged, *successful, *stop_reason;   /* [Bq][L] */
    double *J, *gap, *arrive;                                 /* [Bq][L] */
    double *X, *U, *t;                                        /* [Bq][Nj][x_dim], [Bq][Nj][u_dim], [Bq][Nj], Nj = L (N - 1) + 1 */
} gusto_legs_report;                                          /* caller-owned, any pointer may be NULL */
/* The timeline's report; *round the number of advances so far, *n_flying the queries still flying (either may be NULL) */
int gusto_get_legs(gusto_handle h, gusto_legs_report* out, int* round, int* n_flying);
/* Device pointers to the joined X [Bq][Nj][x_dim], U [Bq][Nj][u_dim] and t [Bq][Nj], valid until the next begin */
int gusto_get_legs_dev(gusto_handle h, const double** X_dev, const double** U_dev, const double** t_dev);
/* GPU time of the last begin or advance (copies and kernels), from HIP events on the handle's stream */
int gusto_last_legs_ms(gusto_handle h, double* ms);

/* Fleet coordination (csrc/fleet.hip): robot-to-robot separation and departure delays.  Every other stage treats a problem as
 * if it were alone in the workspace; this one holds the robots of a fleet against each other.  It is prioritised planning on
 * fixed paths: every robot keeps its solved path, a robot of lower priority departs later, by the smallest delay out of a set
 * of candidates that keeps it `margin` away from every robot ranked above it, for all time.  Robots hold at their start before
 * they depart and stay parked at their goal after they arrive.  No counterpart in the reference (it plans one robot, once);
 * the definitions are therefore stated here.
 *     gusto_solve; gusto_interpolate; gusto_fleet_schedule; gusto_get_fleet.
 * WHETHER A ROBOT CAN HOLD AT ITS START OR PARK AT ITS GOAL IS THE CALLER'S BUSINESS: the stage does not look at velocities.  (The
 * table and ISS problem generators start and end at rest.)
 * Layout: that of gusto_set_problems_multistart with K = R.  A fleet is R consecutive problems of the handle, problem f R + i is
 *   robot i of fleet f; 1 <= R <= GUSTO_MAX_STARTS and R divides B, F = B / R.  GuSTO handles of FreeflyerSE2, AstrobeeSE3 and
 *   AstrobeeSE3Manifold; DubinsCar cannot hold at its start and has no robot geometry: GUSTO_ERR_ARG.
 * Inputs: the dense trajectories of the last gusto_interpolate since gusto_set_problems* (without them GUSTO_ERR_STATE): nfull[b],
 *   the first WS entries P_s of Xfull[b][s] (WS = 2 in the plane, 3 in space), and tf[b].  The stage writes none of the handle's
 *   trajectories, status, histories, keep-out tables or dense buffers.  gusto_set_active is not consulted: `eligible` says which
 *   robots have a plan.  A problem gusto_interpolate left out (nfull[b] < 2) has a track of NaN.
 * Track on the fleet clock: the clock step is h = dt_clock.  Robot b has J_b = (int)ceil(tf_b / h) + 1 clock samples; a J_b
 *   above clock_cap (or a tf_b that is not positive and finite) is GUSTO_ERR_ARG for the whole call, the text names the first
 *   such problem, nothing is clamped.  With h_b = tf_b / (double)(nfull_b - 1), for j < J_b - 1:
 *       tau = (double)j * h;  s = tau / h_b;  i = min((int)floor(s), nfull_b - 2);  w = s - (double)i;
 *       Q_b[j] = (1 - w) * P_i + w * P_{i+1}
 *   and Q_b[J_b - 1] = P_{nfull_b - 1} exactly.  Every operation is rounded on its own (no fused multiply-add).
 * Position: with a departure shift sigma >= 0 in clock steps, p_b(j; sigma) = Q_b[clamp(j - sigma, 0, J_b - 1)]; sigma = -1: the
 *   robot never departs, p_b = Q_b[0] for all j.  end_b = sigma + J_b - 1, and 0 for sigma = -1: nothing moves behind it.
 * Separation: the robot's components are spheres of `radius` at p + comp_off[c], as everywhere.  For robots a, b at step j and
 *   the component pair (ca, cb), ca outer and cb inner: delta_x = (pa_x - pb_x) + (comp_off[ca][x] - comp_off[cb][x]), x < WS;
 *   d2 = sum_x delta_x^2 in coordinate order, every operation rounded on its own.  D2(a, b, j): the smallest d2 over the component
 *   pairs, fmin from +inf (a NaN never wins); components = 0: pair (0, 0) only.  thr = 2 radius + margin, thr2 = thr * thr.  A
 *   conflict is D2 < thr2: no square root enters a decision.  The reported separation is sqrt(D2) - 2 radius.
 * Schedule: robots are placed in the order order[f][0 .. R - 1], a permutation of 0 .. R - 1 per fleet (NULL: index order).  A
 *   robot that is not eligible gets GUSTO_FLEET_NO_PLAN and is placed with sigma = -1: it still blocks a path through its
 *   start.  Eligible: eligible[b] != 0, or with NULL converged and successful from the status words; a robot whose track has a
 *   non-finite entry is never eligible.  An eligible robot i has the candidates sigma_d = d * delay_stride, d = 0 .. n_delays - 1.
 *   Candidate d is feasible when for every robot k placed before i and every j = 0 .. max(end_i, end_k): D2(i, k, j) >= thr2 at
 *   p_i(j; sigma_d), p_k(j; sigma_k).  The robot takes the smallest feasible candidate: GUSTO_FLEET_SCHEDULED; with none it is
 *   GUSTO_FLEET_BLOCKED and placed with sigma = -1.  blocker: the first robot in placement order that refutes candidate 0 (its
 *   index in the fleet), -1 when candidate 0 is feasible or the robot is NO_PLAN.  delay = (double)sigma * h, 0 for sigma = -1.
 * Separation report, for given shifts -- gusto_fleet_schedule reports it for the shifts it chose; gusto_fleet_separation for the
 *   last schedule's (delay_steps = NULL; dt_clock must be the schedule's) or for a caller's delay_steps [B], in which -1 is allowed:
 *   then status is SCHEDULED where delay_steps >= 0 and NO_PLAN elsewhere, blocker -1, and the last schedule's stay what NULL means.
 *   Per pair a != b: the smallest D2 over j = 0 .. max(end_a, end_b) as a separation, and the first step where it occurs;
 *   [F][R][R], symmetric, the diagonal (and a pair without a finite D2) +inf / -1.  Per robot: the smallest entry of its row of the
 *   pair table, the partner (the lowest index on a tie, -1: none below +inf) and that pair's step.  Per fleet: n_conflicts, the
 *   pairs a < b with min D2 < thr2; the smallest separation; makespan_steps, the largest end over SCHEDULED robots (0: none);
 *   n_scheduled and n_blocked.
 * Runs on the handle's stream, after any pending gusto_solve_async; timed with events of its own.  No atomics, nothing crosses a
 *   fleet: a fleet's outputs are the same bit for bit whatever else is in the batch and wherever the fleet sits in it.
 * GUSTO_ERR_ARG, nothing launched, the handle and the stage's state left as they were, in this order: a TrajOpt handle; DubinsCar;
 *   R outside 1 .. GUSTO_MAX_STARTS or not dividing B; bad options; `order` not a permutation (the text names the fleet); a
 *   delay_steps entry outside -1 .. GUSTO_FLEET_MAX_SHIFT (it names the problem); a J_b above clock_cap (likewise).
 * GUSTO_ERR_STATE: no problems; no dense trajectories; gusto_fleet_separation with delay_steps = NULL before any schedule; the
 *   getters before any call.  gusto_set_problems* ends the stage's state. */
#define GUSTO_FLEET_NO_PLAN 0
#define GUSTO_FLEET_SCHEDULED 1
#define GUSTO_FLEET_BLOCKED 2
#define GUSTO_FLEET_MAX_SHIFT (1 << 24)
typedef struct {
    double dt_clock;       /* clock step, > 0 and finite; default 0.1, the default dt_min of gusto_verify_opts */
    double margin;         /* finite, >= 0; default the model's clearance, the distance the solver keeps from keep-out components */
    int n_delays;          /* 1 .. 64; default 64 */
    int delay_stride;      /* clock steps between candidates, 1 .. GUSTO_FLEET_MAX_SHIFT / 64; default 10 */
    int clock_cap;         /* largest J_b allowed, 2 .. GUSTO_FLEET_MAX_SHIFT; default 8192 */
    int components;        /* 0: component pair (0, 0) only; 1 (default): every pair */
    int prune;             /* development: 1 (default) skips a placed robot whose track's bounding box lies further from the
                              candidate's than thr plus the component offsets; 0 tests it.  The results are the same bit for bit */
} gusto_fleet_opts;
int gusto_default_fleet_opts(int model_id, gusto_fleet_opts* o);
int gusto_fleet_schedule(gusto_handle h, int R, const int* order /* [B] HOST: order[f R + p] = the robot placed p-th, or NULL */,
                         const int* eligible /* [B] HOST, or NULL = converged && successful */, const gusto_fleet_opts* o /* NULL: defaults */);
int gusto_fleet_separation(gusto_handle h, int R, const int* delay_steps /* [B] HOST, or NULL = the last schedule's */,
                           const gusto_fleet_opts* o);
typedef struct {
    int *status, *delay_steps;                 /* [B]: GUSTO_FLEET_*, sigma */
    double *delay;                             /* [B] */
    int *blocker;                              /* [B] */
    double *min_sep;                           /* [B] */
    int *partner, *step;                       /* [B] */
    double *pair_min_sep;                      /* [F][R][R] */
    int *pair_step;                            /* [F][R][R] */
    int *n_scheduled, *n_blocked, *n_conflicts;   /* [F] */
    double *fleet_min_sep;                     /* [F] */
    int *makespan_steps;                       /* [F] */
    double *stage_ms;                          /* [3]: GPU time of the track, schedule and separation kernels of the last call (0: not run) */
} gusto_fleet_report;                          /* caller-owned, any pointer may be NULL */
/* The report of the last gusto_fleet_schedule / gusto_fleet_separation; *F and *R its shape (out, F, R may be NULL) */
int gusto_get_fleet(gusto_handle h, gusto_fleet_report* out, int* F, int* R);
/* The tracks of that call: J [B], Q [B][J_max][WS] (rows behind J[b] are zeros), *J_max the largest J_b.  A size query passes
 * the arrays as NULL. */
int gusto_get_fleet_tracks(gusto_handle h, int* J, double* Q, int* J_max);
/* GPU time of the last gusto_fleet_schedule / gusto_fleet_separation (copies and kernels), from HIP events on the handle's stream */
int gusto_last_fleet_ms(gusto_handle h, double* ms);

/* One convex subproblem per problem (what scp_gusto.jl:82-104 builds and solves in one trip), linearised at
 * (Xp,Up)[b] with the given Delta/omega/obstacle_toggle_distance[b].  Used by the parity tests.
 * Outputs: Xn,Un [B][N][.], obj [B] (JuMP.objective_value), status [B] (GUSTO_SOLVER_*), iters [B]. */
int gusto_subproblem(gusto_handle h, int B, const double* Xp, const double* Up, const double* Delta,
                     const double* omega, const double* toggle, double* Xn, double* Un, double* obj, int* status,
                     int* iters);

/* ---- TrajOpt: solve_trajopt_jump!(SCPS, SCPP, solver, max_iter, force) (src/scp/scp_trajopt.jl:33-157), the second SCP
 * algorithm the reference passes through the same `solve_method!` argument of solve_SCP! (src/traj_opt.jl:47-72) ----------
 * FreeflyerSE2, AstrobeeSE3 and AstrobeeSE3Manifold (the models of this library with a SCPParam_TrajOpt: freeflyer_se2.jl:49-64,
 * astrobee_se3.jl:50-65, astrobee_se3_manifold.jl:56-70; the manifold model has no trust region row, and its quaternion
 * norm row -- a convex_state_eq row, hard in TrajOpt, scp_trajopt.jl:200-208 -- is carried as the hard band |h| <= 1e-4).  A TrajOpt handle is a gusto_handle created by gusto_create_trajopt: gusto_set_env,
 * gusto_set_problems(_dev), gusto_get_traj, gusto_get_status, gusto_get_dual, gusto_last_solve_ms work on it unchanged
 * (U has the model's u_dim columns on the host side).  Where the file cannot run as written the math it states is built;
 * the list is in DESIGN.md section 4 (intended L1 dynamics penalty, hard x_1 = x_init, index typos of
 * trust_region_ratio_trajopt, the class evaluate_ctol drops, max_iter as a cap on the subproblem solves). */
/* SCPParam_TrajOpt (scp_trajopt.jl:3-30) */
typedef struct {
    double mu0, s0, c, tau_plus, tau_minus, k, ftol, xtol, ctol;
    int max_penalty_iteration, max_convex_iteration, max_trust_iteration;
} gusto_trajopt_params;
int gusto_default_trajopt_params(int model_id, gusto_trajopt_params* tp);
/* SCPProblem(TOP) + SCPParam_TrajOpt(model) for a batch; hist_cap >= 2 * max_penalty * max_convex * max_trust + 8 entries.
 * Horizons as for gusto_create, with the TrajOpt kernel's larger LDS layout (the defect variables): FreeflyerSE2 N <= 256,
 * AstrobeeSE3 N <= 157, AstrobeeSE3Manifold N <= 139.  A larger N is refused with GUSTO_ERR_ARG ("does not fit the 160 KiB
 * LDS") by the first gusto_solve_trajopt / gusto_solve_trajopt_async / gusto_subproblem_trajopt, which launches nothing. */
int gusto_create_trajopt(gusto_handle* h, int model_id, int N, int batch_cap, int hist_cap, int device);
int gusto_set_trajopt_params(gusto_handle h, const gusto_trajopt_params* tp);
/* the whole three-loop schedule (penalty mu x k, convex iterations, trust region s x tau+-) for every problem of the batch;
 * max_iter caps the number of convex subproblems per problem (the reference computes iter_cap and never reads it) */
int gusto_solve_trajopt(gusto_handle h, int max_iter);
/* ... enqueued on the handle's stream like gusto_solve_async: returns once the one launch of the batch is queued; gusto_wait
 * or any getter completes it.  One handle per GPU (SURVEY.md 8(b) threading row): the shards of a multi-GPU TrajOpt batch,
 * or two handles on one GPU, run side by side instead of one after the other. */
int gusto_solve_trajopt_async(gusto_handle h, int max_iter);
/* SCPParam_TrajOpt vectors as [B][hist_cap] arrays with their lengths [B]: rho_vec and s_vec have 1 + iterations entries,
 * J_true 1 + iterations, J_full / convergence_measure / solver_status iterations (solver_status, ipm_iters and
 * convergence_measure start at row 1 like the GuSTO histories).  Any pointer may be NULL. */
typedef struct {
    int hist_cap; /* IN: row capacity of the arrays below, >= the handle's */
    int *n_solves, *n_mu, *n_xtol, *n_ftol, *n_ctol;
    double *rho_vec, *s_vec, *mu_vec, *xtol_vec, *ftol_vec, *ctol_vec, *J_true, *J_full, *convergence_measure;
    int *solver_status, *ipm_iters;
} gusto_trajopt_history;
int gusto_get_trajopt_history(gusto_handle h, gusto_trajopt_history* out);
/* One TrajOpt subproblem (:159-279) per problem around (Xp, Up)[b] with penalty mu[b] and trust region s[b] (parity tests).
 * Up, Un: [B][N][u_dim]; Dn (may be NULL): the defect variables of the optimum, [B][N][x_dim]. */
int gusto_subproblem_trajopt(gusto_handle h, int B, const double* Xp, const double* Up, const double* mu, const double* s,
                             double* Xn, double* Un, double* Dn, double* obj, int* status, int* iters);

/* Development hook (libraries built with -DGUSTO_PROFILE only, otherwise GUSTO_ERR_STATE): per-problem cycle counters of
 * the kernel's phases, [B][48] (tools/gpu_prof.py).  Stands in for SCPS.iter_elapsed_times at a finer grain. */
int gusto_dev_get_prof(gusto_handle h, long long* out);
/* Development hook: the GPU time of the two launches of the last gusto_tvlqr -- linearise, Riccati -- split by a third event
 * between them (tools/tvlqr_time.py).  Either pointer may be NULL; GUSTO_ERR_STATE before the first gusto_tvlqr. */
int gusto_dev_tvlqr(gusto_handle h, double* linearise_ms, double* riccati_ms);
/* Development hook: the GPU time of the two launches of the last gusto_set_problems_trajlib -- search, retargeting -- split by a
 * third event between them (tools/trajlib_rate.py).  Either pointer may be NULL; GUSTO_ERR_STATE as gusto_last_trajlib_ms. */
int gusto_dev_trajlib(gusto_handle h, double* search_ms, double* retarget_ms);
/* Development hook: shape of the last gusto_solve / gusto_subproblem launch -- resident (persistent) workgroups, dynamic
 * LDS bytes per workgroup, workgroups per CU.  GUSTO_ERR_STATE before the first launch.  (The freeflyerSE2 N = 50 kernel
 * is tuned to 4 problems per CU: 40 664 B of the 160 KiB; tests/test_gpu_parity.py guards it.) */
int gusto_dev_launch_info(gusto_handle h, int* slots, int* lds_bytes, int* per_cu);
/* Development hook: bytes of the handle's interior point workspace in HBM (resident workgroups x per-slot workspace; what the
 * kernel re-reads between the phases of a KKT solve -- bench.py sets it against the 256 MiB Infinity Cache next to the
 * L2 <-> fabric traffic it reports).  No counterpart in the reference (JuMP's model memory). */
int gusto_dev_workspace_bytes(gusto_handle h, long long* bytes);

#ifdef __cplusplus
}
#endif
#endif
