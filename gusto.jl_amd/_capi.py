"""ctypes binding of libgusto_hip.so (include/gusto_hip.h).  No fallback: if the HIP library is missing or no
GPU is present the functions raise -- the product never routes through a CPU path."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
LIB_PATH = os.path.join(_HERE, "libgusto_hip.so")
MAXN, MAXM = 13, 6

FREEFLYER_SE2, DUBINS_CAR, ASTROBEE_SE3, ASTROBEE_SE3_MANIFOLD = 0, 1, 2, 3
MODEL_DIMS = {0: (6, 3), 1: (3, 1), 2: (12, 6), 3: (13, 6)}   # (x_dim, u_dim): lib() checks it against gusto_model_dims
SCP_STATUS = {0: "NA", 1: "OK", 2: "InaccurateModel", 3: "ViolatesConstraints", 4: "TrustRegionViolated"}
SOLVER_STATUS = {0: "NA", 1: "OPTIMAL", 2: "ALMOST_LOCALLY_SOLVED", 3: "FAILED"}
STOP_REASON = {0: "MaxIter", 1: "Converged", 2: "SubproblemFailed", 3: "OmegaMaxExceeded", 4: "HistoryFull"}

# every symbol include/gusto_hip.h declares
SYMBOLS = ["gusto_default_params", "gusto_default_ipm_opts", "gusto_model_dims", "gusto_create", "gusto_destroy",
           "gusto_last_error", "gusto_set_params", "gusto_set_ipm_opts", "gusto_set_env", "gusto_set_env_batch", "gusto_set_schedule", "gusto_set_decomposition", "gusto_dev_workspace_bytes",
           "gusto_set_stream",
           "gusto_set_problems", "gusto_set_problems_dev", "gusto_solve", "gusto_solve_async", "gusto_set_active", "gusto_wait",
           "gusto_last_solve_ms", "gusto_get_traj", "gusto_get_problems",
           "gusto_get_traj_dev", "gusto_gather_peer", "gusto_get_status", "gusto_get_dual", "gusto_get_history", "gusto_get_hist_cap",
           "gusto_set_trust_state", "gusto_subproblem", "gusto_default_shoot_opts", "gusto_shoot", "gusto_get_shoot",
           "gusto_default_trajopt_params", "gusto_create_trajopt", "gusto_set_trajopt_params", "gusto_solve_trajopt", "gusto_solve_trajopt_async",
           "gusto_get_trajopt_history", "gusto_subproblem_trajopt",
           "gusto_default_verify_opts", "gusto_verify", "gusto_get_verify", "gusto_interpolate", "gusto_get_dense",
           "gusto_last_verify_ms",
           "gusto_default_tvlqr_opts", "gusto_tvlqr", "gusto_get_tvlqr", "gusto_last_tvlqr_ms",
           "gusto_default_simulate_opts", "gusto_simulate", "gusto_get_simulate", "gusto_get_simulate_knots", "gusto_last_simulate_ms",
           "gusto_default_disturb_opts", "gusto_simulate_disturbed", "gusto_get_simulate_plant",
           "gusto_default_lincov_opts", "gusto_lincov", "gusto_get_lincov", "gusto_last_lincov_ms",
           "gusto_lincov_disturbed", "gusto_get_lincov_plant", "gusto_lincov_dense", "gusto_get_lincov_dense",
           "gusto_set_problems_multistart", "gusto_select_best", "gusto_get_best", "gusto_get_best_dev",
           "gusto_default_trajlib_opts", "gusto_trajlib_create", "gusto_trajlib_destroy", "gusto_trajlib_last_error", "gusto_trajlib_size",
           "gusto_trajlib_clear", "gusto_trajlib_add", "gusto_trajlib_add_host", "gusto_trajlib_get", "gusto_set_problems_trajlib",
           "gusto_get_trajlib_seeds", "gusto_last_trajlib_ms",
           "gusto_set_problems_replan", "gusto_set_problems_replan_knots", "gusto_get_replan", "gusto_last_replan_ms",
           "gusto_default_tighten_opts", "gusto_tighten_env", "gusto_get_tighten", "gusto_get_env", "gusto_last_tighten_ms",
           "gusto_default_roadmap_opts", "gusto_set_problems_roadmap", "gusto_get_roadmap", "gusto_last_roadmap_ms",
           "gusto_default_tfsearch_opts", "gusto_tfsearch_begin", "gusto_tfsearch_update", "gusto_get_tfsearch", "gusto_get_tfsearch_dev",
           "gusto_last_tfsearch_ms",
           "gusto_default_legs_opts", "gusto_legs_begin", "gusto_legs_advance", "gusto_get_legs", "gusto_get_legs_dev", "gusto_last_legs_ms",
           "gusto_default_fleet_opts", "gusto_fleet_schedule", "gusto_fleet_separation", "gusto_get_fleet", "gusto_get_fleet_tracks",
           "gusto_last_fleet_ms",
           "gusto_dev_get_prof", "gusto_dev_launch_info", "gusto_dev_tvlqr", "gusto_dev_trajlib"]


class ScpParams(C.Structure):
    _fields_ = [(k, C.c_double) for k in
                ("Delta0", "omega0", "omega_max", "eps", "rho0", "rho1", "beta_succ", "beta_fail", "gamma_fail",
                 "convergence_threshold")]


class ModelParams(C.Structure):
    _fields_ = [("mass", C.c_double), ("Jdiag", C.c_double * 3), ("radius", C.c_double), ("clearance", C.c_double),
                ("hard_limit_vel", C.c_double), ("hard_limit_accel", C.c_double), ("hard_limit_omega", C.c_double),
                ("hard_limit_alpha", C.c_double), ("dubins_v", C.c_double), ("dubins_k", C.c_double),
                ("u_max", C.c_double), ("u_min", C.c_double), ("x_max", C.c_double * MAXN),
                ("x_min", C.c_double * MAXN), ("n_robot_comp", C.c_int), ("comp_off", (C.c_double * 3) * 2)]


class IpmOpts(C.Structure):
    _fields_ = [("tol", C.c_double), ("tol_acc", C.c_double), ("mu_floor", C.c_double), ("tr_tol", C.c_double),
                ("mu_warm", C.c_double), ("max_iter", C.c_int), ("acc_iter", C.c_int), ("mu_warm_gain", C.c_double), ("mu_warm_max", C.c_double), ("sigma_max", C.c_double)]


class ShootOpts(C.Structure):
    _fields_ = [("substeps", C.c_int), ("max_newton", C.c_int), ("ftol", C.c_double), ("no_group_pass", C.c_int)]


class VerifyOpts(C.Structure):
    _fields_ = [("dt_min", C.c_double), ("nstep", C.c_int), ("nstep_cap", C.c_int), ("dense_collision", C.c_int)]


class TvlqrOpts(C.Structure):
    """gusto_tvlqr_opts: diagonal weights, the roll-out of gusto_verify_opts, store_P"""
    _fields_ = [("Q", C.c_double * MAXN), ("R", C.c_double * MAXM), ("Qf", C.c_double * MAXN), ("dt_min", C.c_double),
                ("nstep", C.c_int), ("nstep_cap", C.c_int), ("store_P", C.c_int)]


class TvlqrResult:
    """What gusto_get_tvlqr returns: K [B, N-1, m, n], AB [B, N-1, n, n+m] (rows of [Ad | Bd]), status / fail_knot [B], and P --
    [B, N, n, n] after a call with store_P, else [B, n, n], the P of knot 1."""

    def __init__(self, K, P, AB, status, fail_knot):
        self.K, self.P, self.AB, self.status, self.fail_knot = K, P, AB, status, fail_knot


class SimulateOpts(C.Structure):
    """gusto_simulate_opts: samples, the generated perturbations, actuator limits, the roll-out of gusto_verify_opts"""
    _fields_ = [("n_samples", C.c_int), ("seed", C.c_ulonglong), ("first_problem", C.c_ulonglong), ("dx0", C.c_double * MAXN),
                ("du0", C.c_double * MAXM), ("u_lo", C.c_double * MAXM), ("u_hi", C.c_double * MAXM), ("dt_min", C.c_double),
                ("nstep", C.c_int), ("nstep_cap", C.c_int), ("dense_collision", C.c_int), ("store_knots", C.c_int)]


NPLANT = 6   # GUSTO_NPLANT: mass, Jdiag[0], Jdiag[1], Jdiag[2], dubins_v, dubins_k


class DisturbOpts(C.Structure):
    """gusto_disturb_opts: half-widths of the relative plant dispersion and of the per-interval actuator noise"""
    _fields_ = [("plant_rel", C.c_double * NPLANT), ("dw", C.c_double * MAXM)]


# gusto_simulate_report in the header's order: (field, dtype, shape as a function of (B, S, n))
SIMULATE_FIELDS = (("n_free", np.int32, lambda B, S, n: (B,)), ("n_finite", np.int32, lambda B, S, n: (B,)),
                   ("n_clipped", np.int32, lambda B, S, n: (B,)), ("worst_sample", np.int32, lambda B, S, n: (B,)),
                   ("worst_dense_sample", np.int32, lambda B, S, n: (B,)), ("min_dist", np.float64, lambda B, S, n: (B,)),
                   ("max_dev", np.float64, lambda B, S, n: (B, n)), ("max_final_dev", np.float64, lambda B, S, n: (B, n)),
                   ("sample_min_dist", np.float64, lambda B, S, n: (B, S)), ("sample_dense_index", np.int32, lambda B, S, n: (B, S)),
                   ("sample_flags", np.int32, lambda B, S, n: (B, S)), ("x_final", np.float64, lambda B, S, n: (B, S, n)))


class SimulateReport(C.Structure):
    """gusto_simulate_report: caller-owned arrays"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in SIMULATE_FIELDS]


class LincovOpts(C.Structure):
    """gusto_lincov_opts: the half-widths of the default start covariance, the actuator noise and limits, store_S"""
    _fields_ = [("dx0", C.c_double * MAXN), ("du0", C.c_double * MAXM), ("du_white", C.c_double * MAXM), ("u_lo", C.c_double * MAXM),
                ("u_hi", C.c_double * MAXM), ("store_S", C.c_int)]


# gusto_lincov_report in the header's order: (field, dtype, shape as a function of (B, N, n, m))
LINCOV_FIELDS = tuple((k, np.int32, lambda B, N, n, m: (B,)) for k in ("status", "fail_knot", "obs_knot", "obs_pair", "ctl_knot", "ctl_entry")) + \
                tuple((k, np.float64, lambda B, N, n, m: (B,)) for k in ("min_z_obs", "p_collision_bound", "min_z_ctl")) + \
                (("sigma_x", np.float64, lambda B, N, n, m: (B, N, n)), ("sigma_u", np.float64, lambda B, N, n, m: (B, N - 1, m)),
                 ("z_obs", np.float64, lambda B, N, n, m: (B, N)), ("Sxx", np.float64, lambda B, N, n, m: (B, N, n, n)))


class LincovReport(C.Structure):
    """gusto_lincov_report: caller-owned arrays"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in LINCOV_FIELDS]


# gusto_lincov_dense_report in the header's order: (field, dtype, shape as a function of (B, nfull_max, WS)); the last three
# only after a call with store_dense = 1
LINCOV_DENSE_FIELDS = tuple((k, np.int32, lambda B, R, ws: (B,)) for k in ("nfull", "dense_sample", "dense_pair")) + \
                      (("min_z_dense", np.float64, lambda B, R, ws: (B,)), ("z_dense", np.float64, lambda B, R, ws: (B, R)),
                       ("pair_dense", np.int32, lambda B, R, ws: (B, R)), ("Spos", np.float64, lambda B, R, ws: (B, R, ws, ws)))
WS_DIM = {0: 2, 1: 2, 2: 3, 3: 3}   # workspace dimension of the public models (csrc/common.hpp: MT<MODEL>::WS)


class LincovDenseReport(C.Structure):
    """gusto_lincov_dense_report: caller-owned arrays"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in LINCOV_DENSE_FIELDS]


MAX_STARTS = 64   # GUSTO_MAX_STARTS
# gusto_best_report in the header's order: (field, dtype, shape as a function of (Bq, N, n, m))
BEST_FIELDS = (("winner", np.int32, lambda Q, N, n, m: (Q,)), ("winner_problem", np.int32, lambda Q, N, n, m: (Q,)),
               ("n_eligible", np.int32, lambda Q, N, n, m: (Q,)), ("best_score", np.float64, lambda Q, N, n, m: (Q,)),
               ("X", np.float64, lambda Q, N, n, m: (Q, N, n)), ("U", np.float64, lambda Q, N, n, m: (Q, N, m)))


class BestReport(C.Structure):
    """gusto_best_report: caller-owned arrays"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in BEST_FIELDS]


TRAJLIB_MAX_K, TRAJLIB_MAX_CAP = 8, 1 << 20   # GUSTO_TRAJLIB_MAX_K, GUSTO_TRAJLIB_MAX_CAP
REPLAN_SOURCE = {"traj": 0, "best": 1}        # GUSTO_REPLAN_TRAJ, GUSTO_REPLAN_BEST


class TightenOpts(C.Structure):
    """gusto_tighten_opts: the margin in standard deviations and the rules around it"""
    _fields_ = [("kappa", C.c_double), ("slack", C.c_double), ("margin_cap", C.c_double), ("reach", C.c_double),
                ("cover_components", C.c_int), ("monotone", C.c_int)]


MAX_OBS = 64   # keep-out components per problem
# gusto_tighten_report in the header's order: (field, dtype, shape as a function of (B, n_obs_max))
TIGHTEN_FIELDS = tuple((k, np.int32, lambda B, W: (B,)) for k in ("status", "knot", "pair", "n_grown", "blocked")) + \
                 tuple((k, np.float64, lambda B, W: (B,)) for k in ("min_z_base", "max_margin")) + \
                 (("margin", np.float64, lambda B, W: (B, W)),)


class TightenReport(C.Structure):
    """gusto_tighten_report: caller-owned arrays"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in TIGHTEN_FIELDS]


class RoadmapOpts(C.Structure):
    """gusto_roadmap_opts: the growth of the keep-out components, the stand-off of the corner nodes, the straight line first"""
    _fields_ = [("inflate", C.c_double), ("pad", C.c_double), ("straight_first", C.c_int)]


ROADMAP_MAX_K, ROADMAP_MAX_VIA = 8, 16   # GUSTO_ROADMAP_MAX_K, GUSTO_ROADMAP_MAX_VIA
ROADMAP_STATUS = {0: "DIRECT", 1: "PATH", 2: "END_BLOCKED", 3: "NO_PATH", 4: "TOO_LONG", 5: "STRAIGHT"}
# gusto_roadmap_report in the header's order: (field, dtype, shape as a function of B)
ROADMAP_FIELDS = (("status", np.int32, lambda B: (B,)), ("n_via", np.int32, lambda B: (B,)),
                  ("via", np.int32, lambda B: (B, ROADMAP_MAX_VIA)), ("length", np.float64, lambda B: (B,)),
                  ("banned", np.int32, lambda B: (B, ROADMAP_MAX_K)), ("stage_ms", np.float64, lambda B: (3,)))


class RoadmapReport(C.Structure):
    """gusto_roadmap_report: caller-owned arrays"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in ROADMAP_FIELDS]


class TfsearchOpts(C.Structure):
    """gusto_tfsearch_opts: the range used where the per-query arrays are None, the relative width that ends a query, the seed"""
    _fields_ = [("tf_lo", C.c_double), ("tf_hi", C.c_double), ("rtol", C.c_double), ("seed", C.c_int)]


TFSEARCH_SEED = {"line": 0, "incumbent": 1}   # GUSTO_TFSEARCH_SEED_LINE, GUSTO_TFSEARCH_SEED_INCUMBENT
TFSEARCH_NONE, TFSEARCH_DONE, TFSEARCH_FLOOR, TFSEARCH_NONMONOTONE = 1, 2, 4, 8   # bits of the status word
# gusto_tfsearch_report in the header's order: (field, dtype, shape as a function of (Bq, K, N, n, m))
TFSEARCH_FIELDS = tuple((k, np.int32, lambda Q, K, N, n, m: (Q,)) for k in ("status", "round_found", "n_eligible")) + \
                  tuple((k, np.float64, lambda Q, K, N, n, m: (Q,)) for k in ("lo", "hi", "tf_best", "J_best")) + \
                  (("cand", np.float64, lambda Q, K, N, n, m: (Q, K)), ("X", np.float64, lambda Q, K, N, n, m: (Q, N, n)),
                   ("U", np.float64, lambda Q, K, N, n, m: (Q, N, m)))


class TfsearchReport(C.Structure):
    """gusto_tfsearch_report: caller-owned arrays"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in TFSEARCH_FIELDS]


class LegsOpts(C.Structure):
    """gusto_legs_opts: the mode"""
    _fields_ = [("mode", C.c_int)]


LEGS_MODE = {"auto": 0, "sequential": 1, "parallel": 2}   # GUSTO_LEGS_AUTO, GUSTO_LEGS_SEQUENTIAL, GUSTO_LEGS_PARALLEL
LEGS_FLYING, LEGS_DONE, LEGS_FAILED = 1, 2, 4             # the status word
# gusto_legs_report in the header's order: (field, dtype, shape as a function of (Bq, L, Nj, n, m))
LEGS_FIELDS = tuple((k, np.int32, lambda Q, L, Nj, n, m: (Q,)) for k in ("status", "failed_leg", "n_done")) + \
              (("J_total", np.float64, lambda Q, L, Nj, n, m: (Q,)),) + \
              tuple((k, np.int32, lambda Q, L, Nj, n, m: (Q, L)) for k in ("iterations", "converged", "successful", "stop_reason")) + \
              tuple((k, np.float64, lambda Q, L, Nj, n, m: (Q, L)) for k in ("J", "gap", "arrive")) + \
              (("X", np.float64, lambda Q, L, Nj, n, m: (Q, Nj, n)), ("U", np.float64, lambda Q, L, Nj, n, m: (Q, Nj, m)),
               ("t", np.float64, lambda Q, L, Nj, n, m: (Q, Nj)))


class LegsReport(C.Structure):
    """gusto_legs_report: caller-owned arrays"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in LEGS_FIELDS]


class TrajLibOpts(C.Structure):
    """gusto_trajlib_opts"""
    _fields_ = [("w_init", C.c_double * MAXN), ("w_goal", C.c_double * MAXN), ("w_tf", C.c_double), ("lds_tile", C.c_int)]


VERIFY_FIELDS = (("collision_free", np.int32), ("first_knot", np.int32), ("first_dist", np.float64),
                 ("min_dist_knots", np.float64), ("dyn_defect_l1", np.float64), ("min_dist_dense", np.float64),
                 ("min_dense_sample", np.int32), ("max_gap", np.float64))


class VerifyReport(C.Structure):
    """gusto_verify_report: caller-owned arrays [B]"""
    _fields_ = [(k, C.c_void_p) for k, _ in VERIFY_FIELDS]


class FleetOpts(C.Structure):
    """gusto_fleet_opts: the fleet clock, the margin, the candidate delays, the clock cap, component pairs, pruning"""
    _fields_ = [("dt_clock", C.c_double), ("margin", C.c_double), ("n_delays", C.c_int), ("delay_stride", C.c_int),
                ("clock_cap", C.c_int), ("components", C.c_int), ("prune", C.c_int)]


FLEET_NO_PLAN, FLEET_SCHEDULED, FLEET_BLOCKED = 0, 1, 2   # GUSTO_FLEET_*
# gusto_fleet_report in the header's order: (field, dtype, shape as a function of (F, R))
FLEET_FIELDS = (("status", np.int32, lambda F, R: (F * R,)), ("delay_steps", np.int32, lambda F, R: (F * R,)),
                ("delay", np.float64, lambda F, R: (F * R,)), ("blocker", np.int32, lambda F, R: (F * R,)),
                ("min_sep", np.float64, lambda F, R: (F * R,)), ("partner", np.int32, lambda F, R: (F * R,)),
                ("step", np.int32, lambda F, R: (F * R,)), ("pair_min_sep", np.float64, lambda F, R: (F, R, R)),
                ("pair_step", np.int32, lambda F, R: (F, R, R)), ("n_scheduled", np.int32, lambda F, R: (F,)),
                ("n_blocked", np.int32, lambda F, R: (F,)), ("n_conflicts", np.int32, lambda F, R: (F,)),
                ("fleet_min_sep", np.float64, lambda F, R: (F,)), ("makespan_steps", np.int32, lambda F, R: (F,)),
                ("stage_ms", np.float64, lambda F, R: (3,)))


class FleetReport(C.Structure):
    """gusto_fleet_report: caller-owned arrays"""
    _fields_ = [(k, C.c_void_p) for k, _, _ in FLEET_FIELDS]


class TrajOptParams(C.Structure):
    """gusto_trajopt_params = SCPParam_TrajOpt (scp_trajopt.jl:3-30)"""
    _fields_ = [(k, C.c_double) for k in ("mu0", "s0", "c", "tau_plus", "tau_minus", "k", "ftol", "xtol", "ctol")] + \
               [(k, C.c_int) for k in ("max_penalty_iteration", "max_convex_iteration", "max_trust_iteration")]


class TrajOptHistory(C.Structure):
    _fields_ = [("hist_cap", C.c_int)] + [(k, C.c_void_p) for k in
                ("n_solves", "n_mu", "n_xtol", "n_ftol", "n_ctol", "rho_vec", "s_vec", "mu_vec", "xtol_vec", "ftol_vec",
                 "ctol_vec", "J_true", "J_full", "convergence_measure", "solver_status", "ipm_iters")]


class History(C.Structure):
    _fields_ = [("hist_cap", C.c_int), ("n_hist", C.c_void_p), ("nJ", C.c_void_p), ("n_rho", C.c_void_p),
                ("J_true", C.c_void_p), ("J_full", C.c_void_p), ("convergence_measure", C.c_void_p),
                ("Delta", C.c_void_p), ("omega", C.c_void_p), ("rho", C.c_void_p), ("accept_solution", C.c_void_p),
                ("scp_status", C.c_void_p), ("solver_status", C.c_void_p), ("trust_region_satisfied", C.c_void_p),
                ("convex_ineq_satisfied", C.c_void_p), ("ipm_iters", C.c_void_p)]


def build(force=False, verbose=False):
    """Compile libgusto_hip.so for gfx950 with hipcc (cross-compiles without a GPU): one translation unit per
    model plus the C ABI, compiled in parallel, then linked."""
    from concurrent.futures import ThreadPoolExecutor
    csrc = os.path.join(_HERE, "csrc")
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(_ROOT, "include", "gusto_hip.h")]
    if not force and os.path.exists(LIB_PATH) and all(os.path.getmtime(s) <= os.path.getmtime(LIB_PATH) for s in deps):
        return LIB_PATH
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(_ROOT, "include"), "-fPIC",
             "-Wno-unused-value", "-Wno-pass-failed"]
    units = ["gusto_hip", "shoot", "verify", "tvlqr", "simulate", "lincov", "multistart", "trajlib", "replan", "tighten", "roadmap", "tfsearch", "legs", "fleet", "model_0", "model_1", "model_2", "model_3", "model_4", "model_5", "model_6"]
    bdir = os.path.join(_HERE, "build")
    os.makedirs(bdir, exist_ok=True)

    def cc(u):
        cmd = [hipcc] + flags + ["-c", os.path.join(csrc, u + ".hip"), "-o", os.path.join(bdir, u + ".o")]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(cc, units))
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + [os.path.join(bdir, u + ".o") for u in units] + \
          ["-o", LIB_PATH]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return LIB_PATH


_lib = None
_dp = np.ctypeslib.ndpointer(dtype=np.float64, flags="C_CONTIGUOUS")


def lib():
    """Load the HIP library; raises if it has not been built (no CPU fallback exists)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                               "(hipcc --offload-arch=gfx950); gusto.jl_amd has no CPU fallback")
        L = C.CDLL(LIB_PATH)
        vp, ci = C.c_void_p, C.c_int
        L.gusto_last_error.restype = C.c_char_p
        L.gusto_last_error.argtypes = [vp]
        L.gusto_default_params.argtypes = [ci, C.POINTER(ScpParams), C.POINTER(ModelParams)]
        L.gusto_default_ipm_opts.argtypes = [C.POINTER(IpmOpts)]
        L.gusto_model_dims.argtypes = [ci, C.POINTER(ci), C.POINTER(ci)]
        L.gusto_create.argtypes = [C.POINTER(vp), ci, ci, ci, ci, ci]
        L.gusto_destroy.argtypes = [vp]
        L.gusto_dev_launch_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.gusto_dev_workspace_bytes.argtypes = [vp, C.POINTER(C.c_longlong)]
        L.gusto_set_params.argtypes = [vp, C.POINTER(ScpParams), C.POINTER(ModelParams)]
        L.gusto_set_ipm_opts.argtypes = [vp, C.POINTER(IpmOpts)]
        L.gusto_set_env.argtypes = [vp, ci, vp, ci, vp]
        L.gusto_set_env_batch.argtypes = [vp, ci, vp, vp, vp, vp]
        L.gusto_set_stream.argtypes = [vp, vp]
        L.gusto_set_problems.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
        L.gusto_set_problems_dev.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp]
        L.gusto_set_schedule.argtypes = [vp, ci, ci]
        L.gusto_set_decomposition.argtypes = [vp, ci]
        L.gusto_solve.argtypes = [vp, ci, ci]
        L.gusto_solve_async.argtypes = [vp, ci, ci]
        L.gusto_wait.argtypes = [vp]
        L.gusto_set_active.argtypes = [vp, vp]
        L.gusto_last_solve_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_get_traj.argtypes = [vp, vp, vp]
        L.gusto_get_problems.argtypes = [vp, vp, vp, vp, vp]
        L.gusto_get_traj_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
        L.gusto_get_status.argtypes = [vp, vp, vp, vp, vp, vp]
        L.gusto_gather_peer.argtypes = [vp, ci, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), vp, vp, C.POINTER(ci)]
        L.gusto_get_dual.argtypes = [vp, vp]
        L.gusto_get_history.argtypes = [vp, C.POINTER(History)]
        L.gusto_get_hist_cap.argtypes = [vp, C.POINTER(ci)]
        L.gusto_set_trust_state.argtypes = [vp, vp, vp]
        L.gusto_default_shoot_opts.argtypes = [C.POINTER(ShootOpts)]
        L.gusto_shoot.argtypes = [vp, vp, C.POINTER(ShootOpts)]
        L.gusto_get_shoot.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.gusto_subproblem.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        L.gusto_default_verify_opts.argtypes = [C.POINTER(VerifyOpts)]
        L.gusto_verify.argtypes = [vp, vp, vp, C.POINTER(VerifyOpts)]
        L.gusto_get_verify.argtypes = [vp, C.POINTER(VerifyReport)]
        L.gusto_interpolate.argtypes = [vp, vp, vp, C.POINTER(VerifyOpts), C.POINTER(ci)]
        L.gusto_get_dense.argtypes = [vp, vp, vp, vp]
        L.gusto_last_verify_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_default_tvlqr_opts.argtypes = [ci, C.POINTER(TvlqrOpts)]
        L.gusto_tvlqr.argtypes = [vp, vp, vp, C.POINTER(TvlqrOpts)]
        L.gusto_get_tvlqr.argtypes = [vp, vp, vp, vp, vp, vp]
        L.gusto_last_tvlqr_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_dev_tvlqr.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.gusto_default_simulate_opts.argtypes = [ci, C.POINTER(SimulateOpts)]
        L.gusto_simulate.argtypes = [vp, vp, vp, vp, vp, C.POINTER(SimulateOpts)]
        L.gusto_get_simulate.argtypes = [vp, C.POINTER(SimulateReport)]
        L.gusto_get_simulate_knots.argtypes = [vp, vp]
        L.gusto_last_simulate_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_default_disturb_opts.argtypes = [C.POINTER(DisturbOpts)]
        L.gusto_simulate_disturbed.argtypes = [vp, vp, vp, vp, vp, vp, vp, C.POINTER(SimulateOpts), C.POINTER(DisturbOpts)]
        L.gusto_get_simulate_plant.argtypes = [vp, vp]
        L.gusto_default_lincov_opts.argtypes = [ci, C.POINTER(LincovOpts)]
        L.gusto_lincov.argtypes = [vp, vp, vp, vp, vp, C.POINTER(LincovOpts)]
        L.gusto_get_lincov.argtypes = [vp, C.POINTER(LincovReport)]
        L.gusto_last_lincov_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_lincov_disturbed.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(LincovOpts), C.POINTER(DisturbOpts)]
        L.gusto_get_lincov_plant.argtypes = [vp, vp, vp]
        L.gusto_lincov_dense.argtypes = [vp, vp, vp, vp, vp, vp, C.POINTER(LincovOpts), C.POINTER(DisturbOpts), ci]
        L.gusto_get_lincov_dense.argtypes = [vp, C.POINTER(LincovDenseReport), C.POINTER(ci)]
        L.gusto_set_problems_multistart.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
        L.gusto_select_best.argtypes = [vp, ci, vp, vp]
        L.gusto_get_best.argtypes = [vp, C.POINTER(BestReport)]
        L.gusto_get_best_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.gusto_default_trajlib_opts.argtypes = [ci, C.POINTER(TrajLibOpts)]
        L.gusto_trajlib_create.argtypes = [C.POINTER(vp), ci, ci, ci, ci, C.POINTER(TrajLibOpts)]
        L.gusto_trajlib_destroy.argtypes = [vp]
        L.gusto_trajlib_last_error.restype = C.c_char_p
        L.gusto_trajlib_last_error.argtypes = [vp]
        L.gusto_trajlib_size.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
        L.gusto_trajlib_clear.argtypes = [vp]
        L.gusto_trajlib_add.argtypes = [vp, vp, vp, vp, C.POINTER(ci)]
        L.gusto_trajlib_add_host.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp]
        L.gusto_trajlib_get.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.gusto_set_problems_trajlib.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp]
        L.gusto_get_trajlib_seeds.argtypes = [vp, vp, vp, vp]
        L.gusto_last_trajlib_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_dev_trajlib.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.gusto_set_problems_replan.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, vp]
        L.gusto_set_problems_replan_knots.argtypes = [vp, vp, ci, vp, ci, vp, vp, vp]
        L.gusto_get_replan.argtypes = [vp, vp, vp, vp]
        L.gusto_last_replan_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_default_tighten_opts.argtypes = [ci, C.POINTER(TightenOpts)]
        L.gusto_tighten_env.argtypes = [vp, ci, vp, vp, vp, vp, C.POINTER(TightenOpts)]
        L.gusto_get_tighten.argtypes = [vp, C.POINTER(TightenReport), C.POINTER(ci)]
        L.gusto_get_env.argtypes = [vp, C.POINTER(ci), vp, vp, vp, vp]
        L.gusto_last_tighten_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_default_roadmap_opts.argtypes = [ci, C.POINTER(RoadmapOpts)]
        L.gusto_set_problems_roadmap.argtypes = [vp, ci, ci, vp, vp, vp, vp, C.POINTER(RoadmapOpts)]
        L.gusto_get_roadmap.argtypes = [vp, C.POINTER(RoadmapReport)]
        L.gusto_last_roadmap_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_default_tfsearch_opts.argtypes = [ci, C.POINTER(TfsearchOpts)]
        L.gusto_tfsearch_begin.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, C.POINTER(TfsearchOpts)]
        L.gusto_tfsearch_update.argtypes = [vp, vp]
        L.gusto_get_tfsearch.argtypes = [vp, C.POINTER(TfsearchReport), C.POINTER(ci), C.POINTER(ci)]
        L.gusto_get_tfsearch_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.gusto_last_tfsearch_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_default_legs_opts.argtypes = [ci, C.POINTER(LegsOpts)]
        L.gusto_legs_begin.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, C.POINTER(LegsOpts)]
        L.gusto_legs_advance.argtypes = [vp, vp]
        L.gusto_get_legs.argtypes = [vp, C.POINTER(LegsReport), C.POINTER(ci), C.POINTER(ci)]
        L.gusto_get_legs_dev.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
        L.gusto_last_legs_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_default_fleet_opts.argtypes = [ci, C.POINTER(FleetOpts)]
        L.gusto_fleet_schedule.argtypes = [vp, ci, vp, vp, C.POINTER(FleetOpts)]
        L.gusto_fleet_separation.argtypes = [vp, ci, vp, C.POINTER(FleetOpts)]
        L.gusto_get_fleet.argtypes = [vp, C.POINTER(FleetReport), C.POINTER(ci), C.POINTER(ci)]
        L.gusto_get_fleet_tracks.argtypes = [vp, vp, vp, C.POINTER(ci)]
        L.gusto_last_fleet_ms.argtypes = [vp, C.POINTER(C.c_double)]
        L.gusto_default_trajopt_params.argtypes = [ci, C.POINTER(TrajOptParams)]
        L.gusto_create_trajopt.argtypes = [C.POINTER(vp), ci, ci, ci, ci, ci]
        L.gusto_set_trajopt_params.argtypes = [vp, C.POINTER(TrajOptParams)]
        L.gusto_solve_trajopt.argtypes = [vp, ci]
        L.gusto_solve_trajopt_async.argtypes = [vp, ci]
        L.gusto_get_trajopt_history.argtypes = [vp, C.POINTER(TrajOptHistory)]
        L.gusto_subproblem_trajopt.argtypes = [vp, ci, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        n, m = ci(), ci()
        for model, dims in MODEL_DIMS.items():   # the library's model table (csrc/handle.hpp) is the source
            if L.gusto_model_dims(model, C.byref(n), C.byref(m)) or (n.value, m.value) != dims:
                raise RuntimeError(f"MODEL_DIMS[{model}] = {dims}, libgusto_hip.so says {(n.value, m.value)}")
        _lib = L
    return _lib


def default_params(model):
    sp, mp = ScpParams(), ModelParams()
    rc = lib().gusto_default_params(model, C.byref(sp), C.byref(mp))
    if rc:
        raise ValueError(f"gusto_default_params({model}) -> {rc}")
    return sp, mp


def default_trajopt_params(model):
    tp = TrajOptParams()
    rc = lib().gusto_default_trajopt_params(model, C.byref(tp))
    if rc:
        raise ValueError(f"gusto_default_trajopt_params({model}) -> {rc}: the model has no TrajOpt variant")
    return tp


def default_ipm_opts():
    o = IpmOpts()
    lib().gusto_default_ipm_opts(C.byref(o))
    return o


def default_verify_opts():
    o = VerifyOpts()
    lib().gusto_default_verify_opts(C.byref(o))
    return o


def default_tvlqr_opts(model):
    o = TvlqrOpts()
    rc = lib().gusto_default_tvlqr_opts(model, C.byref(o))
    if rc:
        raise ValueError(f"gusto_default_tvlqr_opts({model}) -> {rc}")
    return o


def default_simulate_opts(model):
    o = SimulateOpts()
    rc = lib().gusto_default_simulate_opts(model, C.byref(o))
    if rc:
        raise ValueError(f"gusto_default_simulate_opts({model}) -> {rc}")
    return o


def default_lincov_opts(model):
    o = LincovOpts()
    rc = lib().gusto_default_lincov_opts(model, C.byref(o))
    if rc:
        raise ValueError(f"gusto_default_lincov_opts({model}) -> {rc}")
    return o


def default_tighten_opts(model):
    o = TightenOpts()
    rc = lib().gusto_default_tighten_opts(model, C.byref(o))
    if rc:
        raise ValueError(f"gusto_default_tighten_opts({model}) -> {rc}")
    return o


def default_roadmap_opts(model):
    o = RoadmapOpts()
    rc = lib().gusto_default_roadmap_opts(model, C.byref(o))
    if rc:
        raise ValueError(f"gusto_default_roadmap_opts({model}) -> {rc}")
    return o


def default_tfsearch_opts(model):
    o = TfsearchOpts()
    rc = lib().gusto_default_tfsearch_opts(model, C.byref(o))
    if rc:
        raise ValueError(f"gusto_default_tfsearch_opts({model}) -> {rc}")
    return o


def default_legs_opts(model):
    o = LegsOpts()
    rc = lib().gusto_default_legs_opts(model, C.byref(o))
    if rc:
        raise ValueError(f"gusto_default_legs_opts({model}) -> {rc}")
    return o


def default_fleet_opts(model):
    o = FleetOpts()
    rc = lib().gusto_default_fleet_opts(model, C.byref(o))
    if rc:
        raise ValueError(f"gusto_default_fleet_opts({model}) -> {rc}")
    return o


def legs_mode(goal_lo, goal_hi, n_legs=None, mode="auto"):
    """The mode a timeline is flown in, as LEGS_MODE names it: `mode` itself unless "auto", then "parallel" where every goal
    before a query's last pins every entry (lo == hi, finite), else "sequential".  goal_lo, goal_hi [Bq, L, n]; n_legs [Bq]"""
    if mode not in LEGS_MODE:
        raise ValueError(f"legs: mode is 'auto', 'sequential' or 'parallel', not {mode!r}")
    if mode != "auto":
        return mode
    lo, hi = np.asarray(goal_lo, float), np.asarray(goal_hi, float)
    Bq, L = lo.shape[:2]
    inner = np.arange(L)[None, :] < (np.full(Bq, L) if n_legs is None else np.asarray(n_legs).reshape(Bq))[:, None] - 1
    return "parallel" if ((lo == hi) & np.isfinite(lo)).all(axis=2)[inner].all() else "sequential"


def default_trajlib_opts(model):
    o = TrajLibOpts()
    rc = lib().gusto_default_trajlib_opts(model, C.byref(o))
    if rc:
        raise ValueError(f"gusto_default_trajlib_opts({model}) -> {rc}")
    return o


def _arr(a, dtype=np.float64):
    return np.ascontiguousarray(np.asarray(a, dtype=dtype))


class _View:
    """__cuda_array_interface__ v2 of a device array (float64 unless typestr says otherwise): lets torch wrap a raw device
    pointer without a copy"""

    def __init__(self, ptr, shape, typestr="<f8"):
        self.__cuda_array_interface__ = dict(shape=shape, typestr=typestr, data=(int(ptr), False), version=2)


def _dev_view(ptr, shape, device, typestr="<f8"):
    import torch
    return torch.as_tensor(_View(ptr, shape, typestr), device=torch.device("cuda", device))


class GustoError(RuntimeError):
    pass


class BatchSolver:
    """Thin owner of one gusto_handle: a batch of SCP problems of one model on one GPU."""
    # gusto_set_decomposition applied to every new handle of the models it means something for (0 = the library's choice); tests set
    # it: 1 / 3 / 4 (one / two / four waves per problem) reaches the 12/13-state models
    default_decomposition = 0

    def __init__(self, model, N, batch_cap, hist_cap=64, device=0, boxes=None, spheres=None, scp_params=None,
                 model_params=None, ipm_opts=None):
        self.L = lib()
        self.model, self.N, self.batch_cap, self.hist_cap, self.device = model, N, batch_cap, hist_cap, device
        self.n, self.m = MODEL_DIMS[model]
        self.h = C.c_void_p()
        rc = self._create(model, N, batch_cap, hist_cap, device)
        if rc:
            msg = self.L.gusto_last_error(self.h if self.h else None)
            self.h = C.c_void_p()
            raise GustoError(f"gusto_create -> {rc}: {msg.decode() if msg else ''}")
        self.B = 0
        if scp_params is not None or model_params is not None:
            self.set_params(scp_params, model_params)
        if ipm_opts is not None:
            self._chk(self.L.gusto_set_ipm_opts(self.h, C.byref(ipm_opts)), "set_ipm_opts")
        if BatchSolver.default_decomposition and type(self) is BatchSolver and model in (ASTROBEE_SE3, ASTROBEE_SE3_MANIFOLD):
            self.set_decomposition(BatchSolver.default_decomposition)
        self.set_env(boxes, spheres)

    def _create(self, model, N, batch_cap, hist_cap, device):
        return self.L.gusto_create(C.byref(self.h), model, N, batch_cap, hist_cap, device)

    def _chk(self, rc, what):
        if rc:
            msg = self.L.gusto_last_error(self.h)
            raise GustoError(f"gusto_{what} -> {rc}: {msg.decode() if msg else ''}")

    def set_params(self, scp_params=None, model_params=None):
        """gusto_set_params: the SCP and / or the robot and model parameters of every later call on this handle (None: kept)"""
        self._chk(self.L.gusto_set_params(self.h, C.byref(scp_params) if scp_params is not None else None,
                                          C.byref(model_params) if model_params is not None else None), "set_params")
        if model_params is not None:
            self._model_params = model_params   # (fleet_opts: the default margin is the handle's clearance)

    def close(self):
        if getattr(self, "h", None) and self.h:
            self.L.gusto_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_env(self, boxes=None, spheres=None):
        self.boxes = _arr(boxes if boxes is not None else np.zeros((0, 6))).reshape(-1, 6)
        self.spheres = _arr(spheres if spheres is not None else np.zeros((0, 4))).reshape(-1, 4)
        self._chk(self.L.gusto_set_env(self.h, len(self.boxes), self.boxes.ctypes.data, len(self.spheres),
                                       self.spheres.ctypes.data), "set_env")

    def set_env_batch(self, boxes_list, spheres_list=None):
        """gusto_set_env_batch: one keep-out set per problem -- boxes_list[b] is [n_box_b, 6], spheres_list[b] [n_sph_b, 4]
        (None = no spheres anywhere).  In the reference every ProblemDefinition owns its env (types.jl:32-39)."""
        B = len(boxes_list)
        bl = [_arr(b if b is not None else np.zeros((0, 6))).reshape(-1, 6) for b in boxes_list]
        sl = [_arr(s if s is not None else np.zeros((0, 4))).reshape(-1, 4) for s in (spheres_list or [None] * B)]
        if len(sl) != B:
            raise ValueError("set_env_batch: as many sphere tables as box tables")
        nb, ns = _arr([len(b) for b in bl], np.int32), _arr([len(s) for s in sl], np.int32)
        box = _arr(np.concatenate(bl, axis=0)) if bl else np.zeros((0, 6))
        sph = _arr(np.concatenate(sl, axis=0)) if sl else np.zeros((0, 4))
        self.boxes, self.spheres = bl, sl
        self._chk(self.L.gusto_set_env_batch(self.h, B, nb.ctypes.data, box.ctypes.data, ns.ctypes.data, sph.ctypes.data),
                  "set_env_batch")

    def set_problems(self, x_init, goal_lo, goal_hi, tf, X0=None, U0=None):
        x_init, goal_lo, goal_hi = _arr(x_init).reshape(-1, self.n), _arr(goal_lo).reshape(-1, self.n), \
            _arr(goal_hi).reshape(-1, self.n)
        B = x_init.shape[0]
        tf = _arr(np.broadcast_to(np.asarray(tf, dtype=np.float64), (B,)))
        self._keep = (x_init, goal_lo, goal_hi, tf, None if X0 is None else _arr(X0), None if U0 is None else _arr(U0))
        self._chk(self.L.gusto_set_problems(self.h, B, x_init.ctypes.data, goal_lo.ctypes.data, goal_hi.ctypes.data,
                                            tf.ctypes.data, None if X0 is None else self._keep[4].ctypes.data,
                                            None if U0 is None else self._keep[5].ctypes.data), "set_problems")
        self.B, self._tf = B, tf.copy()

    def _query_arrays(self, x_init, goal_lo, goal_hi, tf=None):
        """the [Bq] inputs of a query entry as the C ABI reads them: x_init, goal_lo, goal_hi [Bq, n], tf [Bq] (a scalar is
        broadcast; None stays None), and Bq"""
        x_init, goal_lo, goal_hi = (_arr(a).reshape(-1, self.n) for a in (x_init, goal_lo, goal_hi))
        Bq = x_init.shape[0]
        return x_init, goal_lo, goal_hi, None if tf is None else _arr(np.broadcast_to(np.asarray(tf, dtype=np.float64), (Bq,))), Bq

    def _env_per_query(self, K, boxes, spheres):
        """one keep-out set per query, repeated K times into set_env_batch; None for both leaves the environment as it is"""
        if boxes is not None or spheres is not None:
            rep = lambda tables: None if tables is None else [t for t in tables for _ in range(K)]
            self.set_env_batch(rep(boxes) if boxes is not None else [None] * self.B, rep(spheres))

    def set_problems_multistart(self, x_init, goal_lo, goal_hi, tf, fan, boxes=None, spheres=None):
        """gusto_set_problems_multistart: Bq queries x K = len(fan) starts become the B = Bq K problems of the handle, problem
        q K + j = start j of query q; fan [K, 2] the lateral offsets (a2, a3) in metres, (0, 0) the straight line.  boxes / spheres:
        one keep-out set PER QUERY (lists of Bq tables), repeated K times into set_env_batch; None leaves the environment as it is."""
        x_init, goal_lo, goal_hi, tf, Bq = self._query_arrays(x_init, goal_lo, goal_hi, tf)
        fan = _arr(fan).reshape(-1, 2)
        K = fan.shape[0]
        self._chk(self.L.gusto_set_problems_multistart(self.h, Bq, K, x_init.ctypes.data, goal_lo.ctypes.data, goal_hi.ctypes.data,
                                                       tf.ctypes.data, fan.ctypes.data), "set_problems_multistart")
        self.B, self._tf = Bq * K, np.repeat(tf, K)
        self._env_per_query(K, boxes, spheres)

    def select_best(self, K, score=None, eligible=None):
        """gusto_select_best + gusto_get_best: per group of K consecutive problems the eligible one with the smallest score (ties:
        the lowest; NaN never wins).  score [B] (None: the last true cost), eligible [B] (None: converged and successful).  A dict of
        winner, winner_problem, n_eligible [Bq] (-1: no winner), best_score [Bq] (+inf likewise), X [Bq, N, n], U [Bq, N, m]."""
        sc = None if score is None else _arr(score).reshape(self.B)
        el = None if eligible is None else _arr(np.asarray(eligible).astype(bool), np.int32).reshape(self.B)
        self._chk(self.L.gusto_select_best(self.h, int(K), None if sc is None else sc.ctypes.data,
                                           None if el is None else el.ctypes.data), "select_best")
        self._select_K = int(K)
        return self.get_best(self.B // int(K))

    def get_best(self, Bq):
        """gusto_get_best: the report of the last select_best, which had Bq groups"""
        out = {k: np.zeros(shape(Bq, self.N, self.n, self.m), dtype=t) for k, t, shape in BEST_FIELDS}
        rep = BestReport(**{k: v.ctypes.data for k, v in out.items()})
        self._chk(self.L.gusto_get_best(self.h, C.byref(rep)), "get_best")
        return out

    def best_dev(self, Bq):
        """gusto_get_best_dev as zero-copy torch views of the compact buffers of the last select_best: X [Bq, N, n], U [Bq, N, m]
        and winner_problem [Bq] (int32); valid until the next select_best"""
        px, pu, pw = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.L.gusto_get_best_dev(self.h, C.byref(px), C.byref(pu), C.byref(pw)), "get_best_dev")
        return (_dev_view(px.value, (Bq, self.N, self.n), self.device), _dev_view(pu.value, (Bq, self.N, self.m), self.device),
                _dev_view(pw.value, (Bq,), self.device, "<i4"))

    def set_problems_roadmap(self, x_init, goal_lo, goal_hi, tf, K=1, opts=None, **kw):
        """gusto_set_problems_roadmap: Bq queries x K alternates become the B = Bq K problems of the handle, problem q K + j =
        alternate j of query q, each seeded from a shortest collision-free polyline through the corners of the handle's current
        keep-out set (set_env: shared; set_env_batch / tighten_env: Bq K sets, query q uses that of problem q K).  opts: None (the
        defaults on the handle's radius), a RoadmapOpts, or keywords of its fields (inflate, pad, straight_first) over the model's
        defaults.  The report: roadmap_info()."""
        x_init, goal_lo, goal_hi, tf, Bq = self._query_arrays(x_init, goal_lo, goal_hi, tf)
        K = int(K)
        if kw:   # (a caller's RoadmapOpts is not written to)
            opts = default_roadmap_opts(self.model) if opts is None else RoadmapOpts(opts.inflate, opts.pad, opts.straight_first)
        for k, v in kw.items():
            if k not in [f for f, _ in RoadmapOpts._fields_]:
                raise TypeError(f"unknown roadmap option {k!r}")
            setattr(opts, k, v)
        self._chk(self.L.gusto_set_problems_roadmap(self.h, Bq, K, x_init.ctypes.data, goal_lo.ctypes.data, goal_hi.ctypes.data,
                                                    tf.ctypes.data, None if opts is None else C.byref(opts)), "set_problems_roadmap")
        self.B, self._tf = Bq * K, np.repeat(tf, K)

    def roadmap_info(self):
        """gusto_get_roadmap: the report of the last set_problems_roadmap as a dict of arrays over the B problems -- status
        (ROADMAP_STATUS), n_via, via [B, 16] (node indices, -1 behind n_via), length, banned [B, 8] (component indices, -1 behind
        the count) -- and stage_ms [3], the GPU time of graph, search and seed"""
        out = {k: np.zeros(shape(self.B), dtype=t) for k, t, shape in ROADMAP_FIELDS}
        rep = RoadmapReport(**{k: v.ctypes.data for k, v in out.items()})
        self._chk(self.L.gusto_get_roadmap(self.h, C.byref(rep)), "get_roadmap")
        return out

    def last_roadmap_ms(self):
        """gusto_last_roadmap_ms: GPU time of the last set_problems_roadmap (copies, graph, search, seed)"""
        return self._last_ms("last_roadmap_ms")

    def tfsearch_begin(self, x_init, goal_lo, goal_hi, tf_lo=None, tf_hi=None, K=8, rtol=None, seed=None, boxes=None, spheres=None):
        """gusto_tfsearch_begin: Bq queries x K candidate final times become the B = Bq K problems of the handle, problem q K + j =
        candidate j of query q, each started from the straight line.  tf_lo, tf_hi: a scalar or [Bq], the range searched (None: the
        library's default); rtol: a query is done when hi - lo <= rtol hi; seed "incumbent" (later candidates start from the
        query's retimed incumbent) or "line".  boxes / spheres: one keep-out set PER QUERY, repeated K times into set_env_batch;
        None leaves the environment as it is.  Then: solve(); tfsearch_update(); ... while it returns queries still searching."""
        x_init, goal_lo, goal_hi, _, Bq = self._query_arrays(x_init, goal_lo, goal_hi)
        K = int(K)
        o = default_tfsearch_opts(self.model)
        if rtol is not None:
            o.rtol = float(rtol)
        if seed is not None:
            if seed not in TFSEARCH_SEED and seed not in TFSEARCH_SEED.values():
                raise ValueError(f"tfsearch_begin: seed is 'line' or 'incumbent', not {seed!r}")
            o.seed = TFSEARCH_SEED.get(seed, seed)
        lo, hi = (None if v is None else _arr(np.broadcast_to(np.asarray(v, dtype=np.float64), (Bq,))) for v in (tf_lo, tf_hi))
        self._chk(self.L.gusto_tfsearch_begin(self.h, Bq, K, x_init.ctypes.data, goal_lo.ctypes.data, goal_hi.ctypes.data,
                                              None if lo is None else lo.ctypes.data, None if hi is None else hi.ctypes.data,
                                              C.byref(o)), "tfsearch_begin")
        self.B, self._tf, self._tfsearch = Bq * K, None, (Bq, K)
        self._env_per_query(K, boxes, spheres)

    def tfsearch_update(self, eligible=None):
        """gusto_tfsearch_update, after a solve of the round's problems: incumbents, brackets and status words, the next round's
        candidates and seeds; the problems of the queries that are done become inactive.  eligible [B]: which problems count
        (None: the converged and successful ones).  Returns the number of queries still searching."""
        el = None if eligible is None else _arr(np.asarray(eligible).astype(bool), np.int32).reshape(self.B)
        self._chk(self.L.gusto_tfsearch_update(self.h, None if el is None else el.ctypes.data), "tfsearch_update")
        ns = C.c_int()
        self._chk(self.L.gusto_get_tfsearch(self.h, None, None, C.byref(ns)), "get_tfsearch")
        return ns.value

    def tfsearch_info(self):
        """gusto_get_tfsearch: a dict over the Bq queries of status (bits TFSEARCH_NONE / DONE / FLOOR / NONMONOTONE), round_found
        (-1: no incumbent), n_eligible, lo, hi, tf_best (NaN: no incumbent), J_best, cand [Bq, K], the incumbents X [Bq, N, n] and
        U [Bq, N, m], and the scalars round (updates so far) and n_searching"""
        Bq, K = self._tfsearch
        out = {k: np.zeros(shape(Bq, K, self.N, self.n, self.m), dtype=t) for k, t, shape in TFSEARCH_FIELDS}
        rep = TfsearchReport(**{k: v.ctypes.data for k, v in out.items()})
        rd, ns = C.c_int(), C.c_int()
        self._chk(self.L.gusto_get_tfsearch(self.h, C.byref(rep), C.byref(rd), C.byref(ns)), "get_tfsearch")
        out["round"], out["n_searching"] = rd.value, ns.value
        return out

    def tfsearch_dev(self):
        """gusto_get_tfsearch_dev as zero-copy torch views: the incumbents X [Bq, N, n], U [Bq, N, m] and tf_best [Bq]"""
        Bq, _ = self._tfsearch
        px, pu, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.L.gusto_get_tfsearch_dev(self.h, C.byref(px), C.byref(pu), C.byref(pt)), "get_tfsearch_dev")
        return (_dev_view(px.value, (Bq, self.N, self.n), self.device), _dev_view(pu.value, (Bq, self.N, self.m), self.device),
                _dev_view(pt.value, (Bq,), self.device))

    def last_tfsearch_ms(self):
        """gusto_last_tfsearch_ms: GPU time of the last tfsearch_begin / tfsearch_update (copies and kernels)"""
        return self._last_ms("last_tfsearch_ms")

    def legs_begin(self, x_init, goal_lo, goal_hi, t_goal, n_legs=None, mode="auto", boxes=None, spheres=None):
        """gusto_legs_begin: Bq queries with a timeline of L goals each, goal_lo / goal_hi [Bq, L, n] at the times t_goal [Bq, L]
        (n_legs [Bq]: the goals a query has, None = L), flown as legs.  mode "sequential": B = Bq, problem q is the query's current
        leg; "parallel" (every interior goal a full point): B = Bq L, problem q L + l = leg l; "auto": legs_mode() decides here.
        boxes / spheres: one keep-out set PER QUERY, repeated once per problem of the query into set_env_batch; None leaves the
        environment as it is.  Then: solve(); legs_advance(); ... while it returns queries still flying.  Returns the mode taken."""
        x_init, lo, hi, _, Bq = self._query_arrays(x_init, goal_lo, goal_hi)      # (the goals: [Bq L, n])
        L = lo.shape[0] // Bq
        t_goal = _arr(np.broadcast_to(np.asarray(t_goal, dtype=np.float64), (Bq, L)))
        nl = None if n_legs is None else _arr(n_legs, np.int32).reshape(Bq)
        mode = legs_mode(lo.reshape(Bq, L, self.n), hi.reshape(Bq, L, self.n), nl, mode)      # (never "auto": the library checks it)
        o = LegsOpts(LEGS_MODE[mode])
        self._chk(self.L.gusto_legs_begin(self.h, Bq, L, None if nl is None else nl.ctypes.data, x_init.ctypes.data, lo.ctypes.data,
                                          hi.ctypes.data, t_goal.ctypes.data, C.byref(o)), "legs_begin")
        K = L if mode == "parallel" else 1
        self.B, self._tf, self._legs = Bq * K, None, (Bq, L)
        self._env_per_query(K, boxes, spheres)
        return mode

    def legs_advance(self, eligible=None):
        """gusto_legs_advance, after a solve: the solved legs into the joined buffers and the report, the next legs' seeds; the
        problems of the finished queries become inactive.  eligible [B]: which problems count (None: the converged and successful
        ones).  Returns the number of queries still flying."""
        el = None if eligible is None else _arr(np.asarray(eligible).astype(bool), np.int32).reshape(self.B)
        self._chk(self.L.gusto_legs_advance(self.h, None if el is None else el.ctypes.data), "legs_advance")
        nf = C.c_int()
        self._chk(self.L.gusto_get_legs(self.h, None, None, C.byref(nf)), "get_legs")
        return nf.value

    def legs_info(self):
        """gusto_get_legs: a dict over the Bq queries of status (LEGS_FLYING / DONE / FAILED), failed_leg (-1: none), n_done,
        J_total; over queries and legs [Bq, L] of iterations, converged, successful, stop_reason, J, gap, arrive; the joined X
        [Bq, Nj, n], U [Bq, Nj, m], t [Bq, Nj] with Nj = L (N - 1) + 1; and the scalars round (advances so far) and n_flying"""
        Bq, L = self._legs
        out = {k: np.zeros(shape(Bq, L, L * (self.N - 1) + 1, self.n, self.m), dtype=t) for k, t, shape in LEGS_FIELDS}
        rep = LegsReport(**{k: v.ctypes.data for k, v in out.items()})
        rd, nf = C.c_int(), C.c_int()
        self._chk(self.L.gusto_get_legs(self.h, C.byref(rep), C.byref(rd), C.byref(nf)), "get_legs")
        out["round"], out["n_flying"] = rd.value, nf.value
        return out

    def legs_dev(self):
        """gusto_get_legs_dev as zero-copy torch views: the joined X [Bq, Nj, n], U [Bq, Nj, m] and t [Bq, Nj]"""
        Bq, L = self._legs
        Nj = L * (self.N - 1) + 1
        px, pu, pt = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._chk(self.L.gusto_get_legs_dev(self.h, C.byref(px), C.byref(pu), C.byref(pt)), "get_legs_dev")
        return (_dev_view(px.value, (Bq, Nj, self.n), self.device), _dev_view(pu.value, (Bq, Nj, self.m), self.device),
                _dev_view(pt.value, (Bq, Nj), self.device))

    def last_legs_ms(self):
        """gusto_last_legs_ms: GPU time of the last legs_begin / legs_advance (copies and kernels)"""
        return self._last_ms("last_legs_ms")

    def fleet_opts(self, opts=None, **kw):
        """a gusto_fleet_opts from None (the library's defaults on the handle's clearance: a null pointer unless keywords are
        given), a FleetOpts, or keywords of its fields (dt_clock, margin, n_delays, delay_stride, clock_cap, components, prune)"""
        if opts is None and not kw:
            return None
        if opts is None:
            o = default_fleet_opts(self.model)
            mp = getattr(self, "_model_params", None)
            if mp is not None:
                o.margin = mp.clearance
        else:   # (a caller's FleetOpts is not written to)
            o = FleetOpts(*(getattr(opts, f) for f, _ in FleetOpts._fields_))
        for k, v in kw.items():
            if k not in [f for f, _ in FleetOpts._fields_]:
                raise TypeError(f"unknown fleet option {k!r}")
            setattr(o, k, float(v) if k in ("dt_clock", "margin") else int(v))
        return o

    def fleet_schedule(self, R, order=None, eligible=None, opts=None, **kw):
        """gusto_fleet_schedule + gusto_get_fleet, after interpolate(): the B problems are F = B / R fleets of R robots, problem
        f R + i robot i of fleet f.  Robots are placed in the order order [F, R] (None: index order); a robot departs by the
        smallest candidate delay that keeps it `margin` away from every robot placed before it.  eligible [B]: which robots have
        a plan (None: converged and successful).  Returns fleet_info()."""
        o = self.fleet_opts(opts, **kw)
        od = None if order is None else _arr(order, np.int32).reshape(self.B)
        el = None if eligible is None else _arr(np.asarray(eligible).astype(bool), np.int32).reshape(self.B)
        self._chk(self.L.gusto_fleet_schedule(self.h, int(R), None if od is None else od.ctypes.data,
                                              None if el is None else el.ctypes.data, None if o is None else C.byref(o)), "fleet_schedule")
        return self.fleet_info()

    def fleet_separation(self, R, delay_steps=None, opts=None, **kw):
        """gusto_fleet_separation + gusto_get_fleet: the pairwise separation report for the last schedule's shifts (None) or for
        delay_steps [B] in clock steps, -1 = the robot never departs.  Returns fleet_info()."""
        o = self.fleet_opts(opts, **kw)
        ds = None if delay_steps is None else _arr(delay_steps, np.int32).reshape(self.B)
        self._chk(self.L.gusto_fleet_separation(self.h, int(R), None if ds is None else ds.ctypes.data,
                                                None if o is None else C.byref(o)), "fleet_separation")
        return self.fleet_info()

    def fleet_info(self):
        """gusto_get_fleet: a dict over the B robots of status (FLEET_NO_PLAN / SCHEDULED / BLOCKED), delay_steps, delay, blocker,
        min_sep, partner, step; over pairs [F, R, R] of pair_min_sep, pair_step; over the F fleets of n_scheduled, n_blocked,
        n_conflicts, fleet_min_sep, makespan_steps; stage_ms [3] (track, schedule, separation) and the scalars F, R"""
        F, R = C.c_int(), C.c_int()
        self._chk(self.L.gusto_get_fleet(self.h, None, C.byref(F), C.byref(R)), "get_fleet")
        out = {k: np.zeros(shape(F.value, R.value), dtype=t) for k, t, shape in FLEET_FIELDS}
        rep = FleetReport(**{k: v.ctypes.data for k, v in out.items()})
        self._chk(self.L.gusto_get_fleet(self.h, C.byref(rep), None, None), "get_fleet")
        out["F"], out["R"] = F.value, R.value
        return out

    def fleet_tracks(self):
        """gusto_get_fleet_tracks: (J [B], Q [B, J_max, WS]) of the last fleet call; rows behind J[b] are zeros"""
        jm = C.c_int()
        self._chk(self.L.gusto_get_fleet_tracks(self.h, None, None, C.byref(jm)), "get_fleet_tracks")
        J, Q = np.zeros(self.B, dtype=np.int32), np.zeros((self.B, jm.value, WS_DIM[self.model]))
        self._chk(self.L.gusto_get_fleet_tracks(self.h, J.ctypes.data, Q.ctypes.data, None), "get_fleet_tracks")
        return J, Q

    def last_fleet_ms(self):
        """gusto_last_fleet_ms: GPU time of the last fleet_schedule / fleet_separation (copies and kernels)"""
        return self._last_ms("last_fleet_ms")

    def set_problems_trajlib(self, lib, x_init, goal_lo, goal_hi, tf, K=1, tag=None, boxes=None, spheres=None):
        """gusto_set_problems_trajlib: Bq queries seeded from their K nearest entries of the TrajLib `lib` become the B = Bq K problems
        of the handle, problem q K + j = neighbour j of query q (a start without a neighbour is the straight line).  tag [Bq]: only
        the entries with the query's tag are eligible (None: all).  boxes / spheres: one keep-out set PER QUERY, repeated K times
        into set_env_batch; None leaves the environment as it is.  The seeds: trajlib_seeds()."""
        x_init, goal_lo, goal_hi, tf, Bq = self._query_arrays(x_init, goal_lo, goal_hi, tf)
        K = int(K)
        tg = None if tag is None else _arr(tag, np.int32).reshape(Bq)
        self._chk(self.L.gusto_set_problems_trajlib(self.h, lib.h, Bq, K, x_init.ctypes.data, goal_lo.ctypes.data, goal_hi.ctypes.data,
                                                    tf.ctypes.data, None if tg is None else tg.ctypes.data), "set_problems_trajlib")
        self.B, self._trajlib_K, self._tf = Bq * K, K, np.repeat(tf, K)
        self._env_per_query(K, boxes, spheres)

    def trajlib_seeds(self):
        """gusto_get_trajlib_seeds: a dict of entry [Bq, K] (-1: the straight line), dist2 [Bq, K] (+inf likewise), n_found [Bq]"""
        K = self._trajlib_K
        out = dict(entry=np.zeros((self.B // K, K), np.int32), dist2=np.zeros((self.B // K, K)), n_found=np.zeros(self.B // K, np.int32))
        self._chk(self.L.gusto_get_trajlib_seeds(self.h, out["entry"].ctypes.data, out["dist2"].ctypes.data, out["n_found"].ctypes.data),
                  "get_trajlib_seeds")
        return out

    def last_trajlib_ms(self):
        """gusto_last_trajlib_ms: GPU time of search plus retargeting of the last set_problems_trajlib"""
        return self._last_ms("last_trajlib_ms")

    def trajlib_phase_ms(self):
        """gusto_dev_trajlib: (search_ms, retarget_ms) of the last set_problems_trajlib"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.gusto_dev_trajlib(self.h, C.byref(a), C.byref(b)), "dev_trajlib")
        return a.value, b.value

    def _replan_args(self, B, goal_lo, goal_hi, mask):
        if (goal_lo is None) != (goal_hi is None):
            raise ValueError("replan: goal_lo and goal_hi are given together or not at all")
        lo = None if goal_lo is None else _arr(np.broadcast_to(np.asarray(goal_lo, dtype=np.float64), (B, self.n)))
        hi = None if goal_hi is None else _arr(np.broadcast_to(np.asarray(goal_hi, dtype=np.float64), (B, self.n)))
        mk = None if mask is None else _arr(np.asarray(mask).astype(bool), np.int32).reshape(B)
        return lo, hi, mk

    def replan_tf(self, tau, src=None, source="traj"):
        """tf' [B] = (1 - tau) tf_s of a set_problems_replan* call with these arguments, from the host's record of the source's tf
        (the arithmetic of the device); None when the source's problems were set from device pointers"""
        src = self if src is None else src
        tf_s = getattr(src, "_tf", None)
        if tf_s is None:
            return None
        tau = np.atleast_1d(np.asarray(tau, dtype=np.float64))
        if source == "best":
            K = getattr(src, "_select_K", None)
            if K is None:
                return None
            try:
                wp = src.get_best(src.B // K)["winner_problem"][:len(tau)]
            except GustoError:      # (no selection: the call itself says so)
                return None
            if len(wp) < len(tau):
                return None
            tf_s = tf_s[np.where(wp >= 0, wp, np.arange(len(tau)) * K)]
        return (1 - tau) * tf_s[:len(tau)] if len(tf_s) >= len(tau) else None

    def _replan_env(self, boxes, spheres):
        if boxes is not None or spheres is not None:
            self.set_env_batch(boxes if boxes is not None else [None] * self.B, spheres)

    def set_problems_replan(self, tau, x_now, src=None, source="traj", goal_lo=None, goal_hi=None, mask=None, boxes=None, spheres=None):
        """gusto_set_problems_replan: B = len(x_now) new problems from the states x_now [B, n] to the goals of the source problems
        (or goal_lo / goal_hi [B, n]) in the time that is left, tf' = (1 - tau) tf_s, every seeded one started from its source
        trajectory shifted by the fraction tau [B] already flown and bent to x_now (and to a moved goal), the others from the
        straight line.  src: the BatchSolver that holds the plans (None: this one; its N may differ); source "traj": problem b of
        src, "best": query b of its last select_best.  mask [B]: which problems are seeded (None: the converged and successful
        ones / the queries with a winner).  boxes / spheres: one keep-out set per problem into set_env_batch; None leaves the
        environment as it is.  What was used: replan_info()."""
        x_now = _arr(x_now).reshape(-1, self.n)
        B = x_now.shape[0]
        tau = _arr(np.broadcast_to(np.asarray(tau, dtype=np.float64), (B,)))
        lo, hi, mk = self._replan_args(B, goal_lo, goal_hi, mask)
        ptr = lambda a: None if a is None else a.ctypes.data
        tf_new = self.replan_tf(tau, src, source)
        self._chk(self.L.gusto_set_problems_replan(self.h, None if src is None else src.h, REPLAN_SOURCE[source], B, tau.ctypes.data,
                                                   x_now.ctypes.data, ptr(lo), ptr(hi), ptr(mk)), "set_problems_replan")
        self.B, self._tf = B, tf_new
        self._replan_env(boxes, spheres)

    def set_problems_replan_knots(self, knot, sample, src=None, B=None, goal_lo=None, goal_hi=None, mask=None, boxes=None, spheres=None):
        """gusto_set_problems_replan_knots: set_problems_replan with tau = knot / (Ns - 1) and x_now = Xcl[b, knot_b, sample], read on
        the device from the knots the last simulate() / simulate_disturbed() on src stored (store_knots = 1).  knot: a scalar or
        [B]; B: None = every problem of src."""
        B = int((self if src is None else src).B if B is None else B)
        kn = _arr(np.broadcast_to(np.asarray(knot), (B,)), np.int32)
        lo, hi, mk = self._replan_args(B, goal_lo, goal_hi, mask)
        ptr = lambda a: None if a is None else a.ctypes.data
        tf_new = self.replan_tf(kn / float((self if src is None else src).N - 1), src)
        self._chk(self.L.gusto_set_problems_replan_knots(self.h, None if src is None else src.h, B, kn.ctypes.data, int(sample), ptr(lo),
                                                         ptr(hi), ptr(mk)), "set_problems_replan_knots")
        self.B, self._tf = B, tf_new
        self._replan_env(boxes, spheres)

    def replan_info(self):
        """gusto_get_replan: a dict of seeded [B] (bool), tau [B], x_now [B, n] of the last set_problems_replan*"""
        sd, tau, x = np.zeros(self.B, np.int32), np.zeros(self.B), np.zeros((self.B, self.n))
        self._chk(self.L.gusto_get_replan(self.h, sd.ctypes.data, tau.ctypes.data, x.ctypes.data), "get_replan")
        return dict(seeded=sd.astype(bool), tau=tau, x_now=x)

    def last_replan_ms(self):
        """gusto_last_replan_ms: GPU time of the last set_problems_replan*"""
        return self._last_ms("last_replan_ms")

    def set_trust_state(self, Delta=None, omega=None):
        """gusto_set_trust_state: the caller's own Delta_vec[end] / omega_vec[end] for the next trip of every problem."""
        D = None if Delta is None else _arr(np.broadcast_to(np.asarray(Delta, dtype=np.float64), (self.B,)))
        W = None if omega is None else _arr(np.broadcast_to(np.asarray(omega, dtype=np.float64), (self.B,)))
        self._chk(self.L.gusto_set_trust_state(self.h, None if D is None else D.ctypes.data,
                                               None if W is None else W.ctypes.data), "set_trust_state")

    def set_decomposition(self, decomposition):
        """0 auto, 1 one wave per problem, 3 / 4 two / four waves per problem (astrobeeSE3, astrobeeSE3manifold: csrc/segw.hpp);
        2 is reserved and refused (GustoError); gusto_hip.h: gusto_set_decomposition."""
        self._chk(self.L.gusto_set_decomposition(self.h, int(decomposition)), "set_decomposition")

    def set_schedule(self, probe_iters=2, min_batch=2048):
        self._chk(self.L.gusto_set_schedule(self.h, int(probe_iters), int(min_batch)), "set_schedule")

    def solve(self, max_iter=30, force=False):
        self._chk(self.L.gusto_solve(self.h, int(max_iter), int(bool(force))), "solve")

    def set_active(self, active=None):
        """gusto_set_active: the problems the following solve / shoot calls work on (boolean mask [B]; None = all)."""
        if active is None:
            self._chk(self.L.gusto_set_active(self.h, None), "set_active")
            return
        a = _arr(np.asarray(active).astype(bool), np.int32).reshape(self.B)
        self._chk(self.L.gusto_set_active(self.h, a.ctypes.data), "set_active")

    def solve_async(self, max_iter=30, force=False):
        """Enqueue the solve on the handle's stream and return; wait() (or any getter) completes it."""
        self._chk(self.L.gusto_solve_async(self.h, int(max_iter), int(bool(force))), "solve_async")

    def wait(self):
        self._chk(self.L.gusto_wait(self.h), "wait")

    def set_problems_dev(self, B, x_init_ptr, goal_lo_ptr, goal_hi_ptr, tf_ptr, X0_ptr=None, U0_ptr=None):
        """gusto_set_problems_dev: inputs already resident in HBM (raw device pointers)."""
        self._chk(self.L.gusto_set_problems_dev(self.h, int(B), x_init_ptr, goal_lo_ptr, goal_hi_ptr, tf_ptr, X0_ptr,
                                                U0_ptr), "set_problems_dev")
        self.B, self._tf = int(B), None

    def last_solve_ms(self):
        return self._last_ms("last_solve_ms")

    def traj(self):
        X, U = np.zeros((self.B, self.N, self.n)), np.zeros((self.B, self.N, self.m))
        self._chk(self.L.gusto_get_traj(self.h, X.ctypes.data, U.ctypes.data), "get_traj")
        return X, U

    def problems(self):
        """gusto_get_problems: (x_init, goal_lo, goal_hi [B, n], tf [B]) as the handle holds them"""
        xi, lo, hi, tf = np.zeros((self.B, self.n)), np.zeros((self.B, self.n)), np.zeros((self.B, self.n)), np.zeros(self.B)
        self._chk(self.L.gusto_get_problems(self.h, xi.ctypes.data, lo.ctypes.data, hi.ctypes.data, tf.ctypes.data), "get_problems")
        return xi, lo, hi, tf

    def traj_dev(self):
        """gusto_get_traj_dev as zero-copy torch views of the handle's HBM buffers: X [B,N,n], U [B,N,m] (valid until
        the next set_problems / solve on this handle).  For device-side consumers, e.g. the RCCL gather."""
        px, pu = C.c_void_p(), C.c_void_p()
        self._chk(self.L.gusto_get_traj_dev(self.h, C.byref(px), C.byref(pu)), "get_traj_dev")
        return (_dev_view(px.value, (self.B, self.N, self.n), self.device),
                _dev_view(pu.value, (self.B, self.N, self.m), self.device))

    def gather_peer(self, sources, host=True):
        """gusto_gather_peer: the shards of `sources` (BatchSolvers, one per GPU, solves possibly still in flight) onto this
        handle's GPU by direct peer copies; returns (X, U) of all problems in the order of `sources` -- numpy arrays, or
        with host=False zero-copy torch views of the gathered device buffers."""
        hs = (C.c_void_p * len(sources))(*[q.h for q in sources])
        px, pu, bt = C.c_void_p(), C.c_void_p(), C.c_int()
        Bt = sum(q.B for q in sources)
        X = np.zeros((Bt, self.N, self.n)) if host else None
        U = np.zeros((Bt, self.N, self.m)) if host else None
        self._chk(self.L.gusto_gather_peer(self.h, len(sources), hs, C.byref(px), C.byref(pu),
                                           X.ctypes.data if host else None, U.ctypes.data if host else None, C.byref(bt)),
                  "gather_peer")
        assert bt.value == Bt
        if host:
            return X, U
        return (_dev_view(px.value, (Bt, self.N, self.n), self.device),
                _dev_view(pu.value, (Bt, self.N, self.m), self.device))

    def status(self):
        a = [np.zeros(self.B, dtype=np.int32) for _ in range(5)]
        self._chk(self.L.gusto_get_status(self.h, *[x.ctypes.data for x in a]), "get_status")
        return dict(iterations=a[0], converged=a[1].astype(bool), successful=a[2].astype(bool), stop_reason=a[3],
                    ipm_iters=a[4])

    def dual(self):
        d = np.zeros((self.B, self.n))
        self._chk(self.L.gusto_get_dual(self.h, d.ctypes.data), "get_dual")
        return d

    def history(self):
        B, H = self.B, self.hist_cap
        dk = ("J_true", "J_full", "convergence_measure", "Delta", "omega", "rho")
        ik = ("accept_solution", "scp_status", "solver_status", "trust_region_satisfied", "convex_ineq_satisfied",
              "ipm_iters")
        out = {k: np.zeros((B, H)) for k in dk}
        out.update({k: np.zeros((B, H), dtype=np.int32) for k in ik})
        cnt = {k: np.zeros(B, dtype=np.int32) for k in ("n_hist", "nJ", "n_rho")}
        hs = History()
        hs.hist_cap = H
        for k, v in list(out.items()) + list(cnt.items()):
            setattr(hs, k, v.ctypes.data)
        self._chk(self.L.gusto_get_history(self.h, C.byref(hs)), "get_history")
        out.update(cnt)
        return out

    def launch_info(self):
        """gusto_dev_launch_info: (persistent workgroups, LDS bytes per workgroup, workgroups per CU) of the last launch."""
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        self._chk(self.L.gusto_dev_launch_info(self.h, C.byref(a), C.byref(b), C.byref(c)), "dev_launch_info")
        return a.value, b.value, c.value

    def workspace_bytes(self):
        """gusto_dev_workspace_bytes: bytes of the handle's interior point workspace in HBM."""
        v = C.c_longlong()
        self._chk(self.L.gusto_dev_workspace_bytes(self.h, C.byref(v)), "dev_workspace_bytes")
        return int(v.value)

    def shoot(self, p0=None, substeps=4, max_newton=100, ftol=1e-3, group_pass=True):
        """gusto_shoot + gusto_get_shoot: indirect shooting of every problem from p0 (default: the SCP duals)."""
        o = ShootOpts(substeps=substeps, max_newton=max_newton, ftol=ftol, no_group_pass=int(not group_pass))
        pv = None if p0 is None else _arr(p0).reshape(self.B, self.n)
        self._chk(self.L.gusto_shoot(self.h, None if pv is None else pv.ctypes.data, C.byref(o)), "shoot")
        B = self.B
        st, it = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        res, pp = np.zeros(B), np.zeros((B, self.n))
        X, U = np.zeros((B, self.N, self.n)), np.zeros((B, self.N, self.m))
        self._chk(self.L.gusto_get_shoot(self.h, st.ctypes.data, it.ctypes.data, res.ctypes.data, pp.ctypes.data,
                                         X.ctypes.data, U.ctypes.data), "get_shoot")
        return dict(status=st, newton_iters=it, resid=res, p0=pp, X=X, U=U)

    def _traj_ptrs(self, X, U, who):
        """the optional X, U of verify / interpolate / tvlqr -- given together or not at all -- as [B, N, n] and [B, N, m] arrays:
        (their addresses or None, None; the arrays, for the caller to hold during the call)"""
        if (X is None) != (U is None):
            raise ValueError(f"{who}: X and U are given together or not at all")
        if X is None:
            return None, None, ()
        keep = _arr(X).reshape(self.B, self.N, self.n), _arr(U).reshape(self.B, self.N, self.m)
        return keep[0].ctypes.data, keep[1].ctypes.data, keep

    def _last_ms(self, what):
        ms = C.c_double()
        self._chk(getattr(self.L, "gusto_" + what)(self.h, C.byref(ms)), what)
        return ms.value

    def _verify_args(self, opts):
        o = default_verify_opts()
        for k, v in opts.items():
            if k not in ("dt_min", "nstep", "nstep_cap", "dense_collision"):
                raise TypeError(f"unknown verify option {k!r}")
            setattr(o, k, float(v) if k == "dt_min" else int(v))
        return o

    def get_verify(self):
        """gusto_get_verify: the report of the last verify() / interpolate() as a dict of [B] arrays."""
        out = {k: np.zeros(self.B, dtype=t) for k, t in VERIFY_FIELDS}
        rep = VerifyReport(**{k: v.ctypes.data for k, v in out.items()})
        self._chk(self.L.gusto_get_verify(self.h, C.byref(rep)), "get_verify")
        out["collision_free"] = out["collision_free"].astype(bool)
        return out

    def verify(self, X=None, U=None, **opts):
        """gusto_verify + gusto_get_verify: collision check at the knots, forward-Euler defect, RK4 roll-out between the knots
        (dense minimum distance, gap at the knots) of X, U (default: the handle's trajectories, left as they are).
        opts: dt_min, nstep, nstep_cap, dense_collision (gusto_verify_opts)."""
        px, pu, _keep = self._traj_ptrs(X, U, "verify")
        self._chk(self.L.gusto_verify(self.h, px, pu, C.byref(self._verify_args(opts))), "verify")
        return self.get_verify()

    def interpolate(self, X=None, U=None, **opts):
        """gusto_interpolate + gusto_get_dense: (nfull [B], Xfull [B, nfull_max, n], Ufull [B, nfull_max - 1, m]); rows behind
        nfull[b] are zeros.  get_verify() then holds the report of the same pass."""
        px, pu, _keep = self._traj_ptrs(X, U, "interpolate")
        nf = C.c_int()
        self._chk(self.L.gusto_interpolate(self.h, px, pu, C.byref(self._verify_args(opts)), C.byref(nf)), "interpolate")
        nfull = np.zeros(self.B, dtype=np.int32)
        Xf, Uf = np.zeros((self.B, nf.value, self.n)), np.zeros((self.B, nf.value - 1, self.m))
        self._chk(self.L.gusto_get_dense(self.h, nfull.ctypes.data, Xf.ctypes.data, Uf.ctypes.data), "get_dense")
        return nfull, Xf, Uf

    def last_verify_ms(self):
        return self._last_ms("last_verify_ms")

    def tvlqr_opts(self, opts=None):
        """a gusto_tvlqr_opts from None (the defaults), a TvlqrOpts, or a dict of its fields -- Q, R, Qf as scalars or vectors of
        the model's x_dim / u_dim entries"""
        if isinstance(opts, TvlqrOpts):
            return opts
        o = default_tvlqr_opts(self.model)
        for k, v in (opts or {}).items():
            if k in ("Q", "R", "Qf"):
                dim = self.m if k == "R" else self.n
                w = np.broadcast_to(np.asarray(v, dtype=np.float64), (dim,))
                for i in range(dim):
                    getattr(o, k)[i] = float(w[i])
            elif k in ("nstep", "nstep_cap", "store_P"):
                setattr(o, k, int(v))
            elif k == "dt_min":
                o.dt_min = float(v)
            else:
                raise TypeError(f"unknown tvlqr option {k!r}")
        return o

    def tvlqr(self, opts=None, X=None, U=None):
        """gusto_tvlqr + gusto_get_tvlqr: the time-varying LQR gains K_k of u = U_k - K_k (x - X_k) around X, U (default: the
        handle's trajectories, left as they are), on the exact derivative of the RK4 roll-out interpolate() performs."""
        px, pu, _keep = self._traj_ptrs(X, U, "tvlqr")
        o = self.tvlqr_opts(opts)
        self._chk(self.L.gusto_tvlqr(self.h, px, pu, C.byref(o)), "tvlqr")
        self._tvlqr_store_P = bool(o.store_P)
        return self.get_tvlqr()

    def get_tvlqr(self, full_P=None):
        """gusto_get_tvlqr as a TvlqrResult.  full_P: None = whatever the last call kept; True = the P of every knot, refused
        (-3, as the C ABI's state errors) after a call without store_P; False = the P of knot 1 only."""
        B, N, n, m = self.B, self.N, self.n, self.m
        kept = getattr(self, "_tvlqr_store_P", None)
        if full_P and kept is False:
            raise GustoError("gusto_get_tvlqr -> -3: the last gusto_tvlqr ran without store_P: only the P of knot 1 exists")
        st, fk = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        K, AB = np.zeros((B, N - 1, m, n)), np.zeros((B, N - 1, n, n + m))
        P = np.zeros((B, N, n, n) if kept else (B, n, n))
        self._chk(self.L.gusto_get_tvlqr(self.h, st.ctypes.data, fk.ctypes.data, K.ctypes.data, P.ctypes.data, AB.ctypes.data),
                  "get_tvlqr")
        if kept and full_P is False:
            P = P[:, 0].copy()
        return TvlqrResult(K, P, AB, st, fk)

    def tvlqr_phase_ms(self):
        """gusto_dev_tvlqr: (linearise ms, riccati ms) of the last tvlqr call"""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.gusto_dev_tvlqr(self.h, C.byref(a), C.byref(b)), "dev_tvlqr")
        return a.value, b.value

    def last_tvlqr_ms(self):
        return self._last_ms("last_tvlqr_ms")

    def simulate_opts(self, opts=None):
        """a gusto_simulate_opts from None (the defaults), a SimulateOpts, or a dict of its fields -- dx0, du0, u_lo, u_hi as
        scalars or vectors of the model's x_dim / u_dim entries"""
        if isinstance(opts, SimulateOpts):
            return opts
        o = default_simulate_opts(self.model)
        for k, v in (opts or {}).items():
            if k in ("dx0", "du0", "u_lo", "u_hi"):
                dim = self.n if k == "dx0" else self.m
                w = np.broadcast_to(np.asarray(v, dtype=np.float64), (dim,))
                for i in range(dim):
                    getattr(o, k)[i] = float(w[i])
            elif k in ("n_samples", "seed", "first_problem", "nstep", "nstep_cap", "dense_collision", "store_knots"):
                setattr(o, k, int(v))
            elif k == "dt_min":
                o.dt_min = float(v)
            else:
                raise TypeError(f"unknown simulate option {k!r}")
        return o

    def simulate(self, opts=None, X=None, U=None, K=None, pert=None):
        """gusto_simulate + gusto_get_simulate: closed-loop roll-outs of u = U_k - K_k (x - X_k), clipped to u_lo .. u_hi, from
        n_samples perturbed starts per problem, around X, U (default: the handle's trajectories) with the gains K [B, N-1, m, n]
        (default: those of the last tvlqr()) and the perturbations pert [B, S, n + m] (default: generated on the device).
        Returns the report as a dict (gusto_simulate_report's fields)."""
        px, pu, _keep = self._traj_ptrs(X, U, "simulate")
        o = self.simulate_opts(opts)
        Kk = None if K is None else _arr(K).reshape(self.B, self.N - 1, self.m, self.n)
        pp = None if pert is None else _arr(pert).reshape(self.B, o.n_samples, self.n + self.m)
        self._chk(self.L.gusto_simulate(self.h, px, pu, None if Kk is None else Kk.ctypes.data,
                                        None if pp is None else pp.ctypes.data, C.byref(o)), "simulate")
        self._simulate_S = int(o.n_samples)
        return self.get_simulate()

    def disturb_opts(self, disturb=None):
        """a gusto_disturb_opts from None (zeros), a DisturbOpts, or a dict: plant_rel as a scalar or NPLANT entries, dw as a
        scalar or the model's u_dim entries"""
        if isinstance(disturb, DisturbOpts):
            return disturb
        d = DisturbOpts()
        self.L.gusto_default_disturb_opts(C.byref(d))
        for k, v in (disturb or {}).items():
            if k not in ("plant_rel", "dw"):
                raise TypeError(f"unknown disturb option {k!r}")
            dim = NPLANT if k == "plant_rel" else self.m
            w = np.broadcast_to(np.asarray(v, dtype=np.float64), (dim,))
            for i in range(dim):
                getattr(d, k)[i] = float(w[i])
        return d

    def simulate_disturbed(self, opts=None, disturb=None, X=None, U=None, K=None, pert=None, plant=None, white=None):
        """gusto_simulate_disturbed + gusto_get_simulate: simulate() with the nominal law, on a plant whose scalars differ per
        sample -- plant [B, S, NPLANT] absolute values, default: generated with the relative half-widths disturb["plant_rel"] --
        and with an actuator noise per hold interval -- white [B, N-1, S, m], default: generated with the half-widths
        disturb["dw"].  Returns the report as a dict; get_simulate_plant() has the plant scalars that were used."""
        px, pu, _keep = self._traj_ptrs(X, U, "simulate_disturbed")
        o, d = self.simulate_opts(opts), self.disturb_opts(disturb)
        S = int(o.n_samples)
        Kk = None if K is None else _arr(K).reshape(self.B, self.N - 1, self.m, self.n)
        pp = None if pert is None else _arr(pert).reshape(self.B, S, self.n + self.m)
        pl = None if plant is None else _arr(plant).reshape(self.B, S, NPLANT)
        wh = None if white is None else _arr(white).reshape(self.B, self.N - 1, S, self.m)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._chk(self.L.gusto_simulate_disturbed(self.h, px, pu, ptr(Kk), ptr(pp), ptr(pl), ptr(wh), C.byref(o), C.byref(d)),
                  "simulate_disturbed")
        self._simulate_S = S
        return self.get_simulate()

    def get_simulate_plant(self):
        """gusto_get_simulate_plant: the plant scalars [B, S, NPLANT] of the last simulate_disturbed()"""
        plant = np.zeros((self.B, getattr(self, "_simulate_S", 1), NPLANT))
        self._chk(self.L.gusto_get_simulate_plant(self.h, plant.ctypes.data), "get_simulate_plant")
        return plant

    def get_simulate(self):
        """gusto_get_simulate: the report of the last simulate() as a dict of arrays"""
        S = getattr(self, "_simulate_S", 1)
        out = {k: np.zeros(shape(self.B, S, self.n), dtype=t) for k, t, shape in SIMULATE_FIELDS}
        rep = SimulateReport(**{k: v.ctypes.data for k, v in out.items()})
        self._chk(self.L.gusto_get_simulate(self.h, C.byref(rep)), "get_simulate")
        return out

    def get_simulate_knots(self):
        """gusto_get_simulate_knots: Xcl [B, N, S, n] of the last simulate() with store_knots = 1"""
        Xcl = np.zeros((self.B, self.N, getattr(self, "_simulate_S", 1), self.n))
        self._chk(self.L.gusto_get_simulate_knots(self.h, Xcl.ctypes.data), "get_simulate_knots")
        return Xcl

    def last_simulate_ms(self):
        return self._last_ms("last_simulate_ms")

    def lincov_opts(self, opts=None):
        """a gusto_lincov_opts from None (the defaults), a LincovOpts, or a dict of its fields -- dx0, du0, du_white, u_lo, u_hi as
        scalars or vectors of the model's x_dim / u_dim entries"""
        if isinstance(opts, LincovOpts):
            return opts
        o = default_lincov_opts(self.model)
        for k, v in (opts or {}).items():
            if k in ("dx0", "du0", "du_white", "u_lo", "u_hi"):
                dim = self.n if k == "dx0" else self.m
                w = np.broadcast_to(np.asarray(v, dtype=np.float64), (dim,))
                for i in range(dim):
                    getattr(o, k)[i] = float(w[i])
            elif k == "store_S":
                o.store_S = int(v)
            else:
                raise TypeError(f"unknown lincov option {k!r}")
        return o

    def lincov(self, opts=None, X=None, U=None, K=None, S0=None):
        """gusto_lincov + gusto_get_lincov: the covariance of (state deviation, control offset) carried through the closed loop of
        u = U_k - K_k (x - X_k) on the [Ad | Bd] of the last tvlqr(), from S0 [B, n + m, n + m] (default: the variances of
        simulate()'s generated perturbations with the same dx0, du0), around X, U (default: the handle's trajectories; pass what
        that tvlqr() saw) with the gains K [B, N-1, m, n] (default: those of the last tvlqr()).  Returns the report as a dict
        (gusto_lincov_report's fields; Sxx only with store_S = 1)."""
        px, pu, _keep = self._traj_ptrs(X, U, "lincov")
        o = self.lincov_opts(opts)
        Kk = None if K is None else _arr(K).reshape(self.B, self.N - 1, self.m, self.n)
        Ss = None if S0 is None else _arr(S0).reshape(self.B, self.n + self.m, self.n + self.m)
        self._chk(self.L.gusto_lincov(self.h, px, pu, None if Kk is None else Kk.ctypes.data,
                                      None if Ss is None else Ss.ctypes.data, C.byref(o)), "lincov")
        self._lincov_store_S = bool(o.store_S)
        return self.get_lincov()

    def lincov_disturbed(self, opts=None, disturb=None, X=None, U=None, K=None, S0=None, Sth=None):
        """gusto_lincov_disturbed + gusto_get_lincov: lincov() with the deviation augmented by the constant plant deviation
        theta - theta_nom, to first order -- Sth [B, NPLANT, NPLANT] its covariance, default: the variances of the uniform draws
        of simulate_disturbed() with the relative half-widths disturb["plant_rel"] -- and with disturb["dw"] added to du_white as
        dw^2 / 3.  Returns the report as a dict like lincov(); get_lincov_plant() has Cd and the x-theta block of S."""
        px, pu, _keep = self._traj_ptrs(X, U, "lincov_disturbed")
        o, d = self.lincov_opts(opts), self.disturb_opts(disturb)
        Kk = None if K is None else _arr(K).reshape(self.B, self.N - 1, self.m, self.n)
        Ss = None if S0 is None else _arr(S0).reshape(self.B, self.n + self.m, self.n + self.m)
        St = None if Sth is None else _arr(Sth).reshape(self.B, NPLANT, NPLANT)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._chk(self.L.gusto_lincov_disturbed(self.h, px, pu, ptr(Kk), ptr(Ss), ptr(St), C.byref(o), C.byref(d)), "lincov_disturbed")
        self._lincov_store_S = bool(o.store_S)
        return self.get_lincov()

    def lincov_dense(self, opts=None, disturb=None, X=None, U=None, K=None, S0=None, Sth=None, store_dense=1):
        """gusto_lincov_dense + gusto_get_lincov_dense: lincov_disturbed() (its knot pass is what get_lincov() and
        get_lincov_plant() then report) and the obstacle margins at the dense samples between the knots -- the samples of
        simulate() and interpolate(), with the roll-out options of the last tvlqr().  Returns the dense report as a dict: nfull,
        dense_sample, dense_pair, min_z_dense [B] and, with store_dense = 1, z_dense, pair_dense [B, nfull_max] and Spos
        [B, nfull_max, WS, WS]."""
        px, pu, _keep = self._traj_ptrs(X, U, "lincov_dense")
        o, d = self.lincov_opts(opts), self.disturb_opts(disturb)
        Kk = None if K is None else _arr(K).reshape(self.B, self.N - 1, self.m, self.n)
        Ss = None if S0 is None else _arr(S0).reshape(self.B, self.n + self.m, self.n + self.m)
        St = None if Sth is None else _arr(Sth).reshape(self.B, NPLANT, NPLANT)
        ptr = lambda a: None if a is None else a.ctypes.data
        self._chk(self.L.gusto_lincov_dense(self.h, px, pu, ptr(Kk), ptr(Ss), ptr(St), C.byref(o), C.byref(d), int(store_dense)),
                  "lincov_dense")
        self._lincov_store_S = bool(o.store_S)
        self._lincov_store_dense = bool(store_dense)
        return self.get_lincov_dense()

    def get_lincov_dense(self, rows=None):
        """gusto_get_lincov_dense: the dense report of the last lincov_dense() as a dict of arrays.  rows: None = with the
        per-sample arrays if the last call kept them; True = ask for them (refused with -3 after a call without store_dense);
        False = without."""
        want = getattr(self, "_lincov_store_dense", False) if rows is None else bool(rows)
        R = C.c_int(0)
        self._chk(self.L.gusto_get_lincov_dense(self.h, None, C.byref(R)), "get_lincov_dense")
        out = {k: np.zeros(shape(self.B, R.value, WS_DIM[self.model]), dtype=t) for k, t, shape in LINCOV_DENSE_FIELDS
               if want or k not in ("z_dense", "pair_dense", "Spos")}
        rep = LincovDenseReport(**{k: v.ctypes.data for k, v in out.items()})
        self._chk(self.L.gusto_get_lincov_dense(self.h, C.byref(rep), None), "get_lincov_dense")
        return out

    def get_lincov_plant(self, Sxt=None):
        """gusto_get_lincov_plant: (Cd [B, N-1, n, NPLANT], Sxt [B, N, n, NPLANT]) of the last lincov_disturbed().  Sxt: None = the
        array if the last call kept it, else None in its place; True = ask for it (refused with -3 after a call without
        store_S); False = without."""
        want = getattr(self, "_lincov_store_S", False) if Sxt is None else bool(Sxt)
        Cd = np.zeros((self.B, self.N - 1, self.n, NPLANT))
        St = np.zeros((self.B, self.N, self.n, NPLANT)) if want else None
        self._chk(self.L.gusto_get_lincov_plant(self.h, Cd.ctypes.data, None if St is None else St.ctypes.data), "get_lincov_plant")
        return Cd, St

    def get_lincov(self, Sxx=None):
        """gusto_get_lincov: the report of the last lincov() as a dict of arrays.  Sxx: None = with Sxx [B, N, n, n] if the last
        call kept it; True = ask for it (refused with -3 after a call without store_S); False = without."""
        want = getattr(self, "_lincov_store_S", False) if Sxx is None else bool(Sxx)
        out = {k: np.zeros(shape(self.B, self.N, self.n, self.m), dtype=t) for k, t, shape in LINCOV_FIELDS if k != "Sxx" or want}
        rep = LincovReport(**{k: v.ctypes.data for k, v in out.items()})
        self._chk(self.L.gusto_get_lincov(self.h, C.byref(rep)), "get_lincov")
        return out

    def last_lincov_ms(self):
        return self._last_ms("last_lincov_ms")

    def tighten_opts(self, opts=None, **kw):
        """a gusto_tighten_opts from None (the defaults), a TightenOpts, or a dict / keywords of its fields"""
        if isinstance(opts, TightenOpts) and not kw:
            return opts
        o = default_tighten_opts(self.model)
        names = [k for k, _ in TightenOpts._fields_]
        for k, v in {**(dict(opts) if opts else {}), **kw}.items():
            if k not in names:
                raise TypeError(f"unknown tighten option {k!r}")
            setattr(o, k, int(v) if k in ("cover_components", "monotone") else float(v))
        return o

    def tighten_env(self, boxes_list, spheres_list=None, **opts):
        """gusto_tighten_env + gusto_get_tighten: per-problem keep-out tables from the BASE set -- boxes_list / spheres_list as
        set_env_batch takes them, of length 1 (one set for the batch) or B -- extended over the robot's component offsets and grown
        by kappa standard deviations of the last lincov(store_S=1); the next solve reads them.  opts: the fields of
        gusto_tighten_opts (kappa, slack, margin_cap, reach, cover_components, monotone).  Returns get_tighten()."""
        E = len(boxes_list)
        bl = [_arr(b if b is not None else np.zeros((0, 6))).reshape(-1, 6) for b in boxes_list]
        sl = [_arr(s if s is not None else np.zeros((0, 4))).reshape(-1, 4) for s in (spheres_list or [None] * E)]
        if len(sl) != E:
            raise ValueError("tighten_env: as many sphere tables as box tables")
        nb, ns = _arr([len(b) for b in bl], np.int32), _arr([len(s) for s in sl], np.int32)
        box = _arr(np.concatenate(bl, axis=0)) if bl else np.zeros((0, 6))
        sph = _arr(np.concatenate(sl, axis=0)) if sl else np.zeros((0, 4))
        o = self.tighten_opts(opts.pop("opts", None), **opts)
        self._chk(self.L.gusto_tighten_env(self.h, E, nb.ctypes.data, box.ctypes.data, ns.ctypes.data, sph.ctypes.data, C.byref(o)),
                  "tighten_env")
        self.boxes, self.spheres = self.get_env()
        return self.get_tighten()

    def get_tighten(self):
        """gusto_get_tighten: the report of the last tighten_env() as a dict of arrays (gusto_tighten_report's fields; margin
        [B, n_obs_max])"""
        W = C.c_int()
        self._chk(self.L.gusto_get_tighten(self.h, None, C.byref(W)), "get_tighten")
        out = {k: np.zeros(shape(self.B, W.value), dtype=t) for k, t, shape in TIGHTEN_FIELDS}
        rep = TightenReport(**{k: v.ctypes.data for k, v in out.items()})
        self._chk(self.L.gusto_get_tighten(self.h, C.byref(rep), None), "get_tighten")
        return out

    def get_env(self):
        """gusto_get_env: the handle's current keep-out tables as (boxes_list, spheres_list), lists of [n_box_b, 6] and [n_sph_b, 4]
        arrays: of length 1 after set_env, else one entry per problem"""
        E = C.c_int()
        self._chk(self.L.gusto_get_env(self.h, C.byref(E), None, None, None, None), "get_env")
        nb, ns = np.zeros(E.value, dtype=np.int32), np.zeros(E.value, dtype=np.int32)
        self._chk(self.L.gusto_get_env(self.h, None, nb.ctypes.data, None, ns.ctypes.data, None), "get_env")
        box, sph = np.zeros((int(nb.sum()), 6)), np.zeros((int(ns.sum()), 4))
        self._chk(self.L.gusto_get_env(self.h, None, None, box.ctypes.data, None, sph.ctypes.data), "get_env")
        ob, os_ = np.concatenate([[0], np.cumsum(nb)]), np.concatenate([[0], np.cumsum(ns)])
        return ([box[ob[e]:ob[e + 1]].copy() for e in range(E.value)], [sph[os_[e]:os_[e + 1]].copy() for e in range(E.value)])

    def last_tighten_ms(self):
        """gusto_last_tighten_ms: GPU time of the last tighten_env()"""
        return self._last_ms("last_tighten_ms")

    def subproblem(self, Xp, Up, Delta, omega, toggle):
        B = self.B
        Xp, Up = _arr(Xp).reshape(B, self.N, self.n), _arr(Up).reshape(B, self.N, self.m)
        Delta, omega, toggle = (_arr(np.broadcast_to(np.asarray(v, dtype=np.float64), (B,))) for v in
                                (Delta, omega, toggle))
        Xn, Un, obj = np.zeros_like(Xp), np.zeros_like(Up), np.zeros(B)
        st, it = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        self._chk(self.L.gusto_subproblem(self.h, B, Xp.ctypes.data, Up.ctypes.data, Delta.ctypes.data,
                                          omega.ctypes.data, toggle.ctypes.data, Xn.ctypes.data, Un.ctypes.data,
                                          obj.ctypes.data, st.ctypes.data, it.ctypes.data), "subproblem")
        return dict(X=Xn, U=Un, obj=obj, status=st, iters=it, dual=self.dual())


class TrajOptSolver(BatchSolver):
    """A gusto_handle created by gusto_create_trajopt: the TrajOpt algorithm (src/scp/scp_trajopt.jl) for a batch of problems
    of FreeflyerSE2, AstrobeeSE3 or AstrobeeSE3Manifold.  set_env / set_problems / traj / status / dual / last_solve_ms as for BatchSolver."""

    def __init__(self, model, N, batch_cap, hist_cap=272, device=0, boxes=None, spheres=None, model_params=None,
                 trajopt_params=None, ipm_opts=None):
        super().__init__(model, N, batch_cap, hist_cap, device, boxes, spheres, None, model_params, ipm_opts)
        if trajopt_params is not None:
            self._chk(self.L.gusto_set_trajopt_params(self.h, C.byref(trajopt_params)), "set_trajopt_params")

    def _create(self, model, N, batch_cap, hist_cap, device):
        return self.L.gusto_create_trajopt(C.byref(self.h), model, N, batch_cap, hist_cap, device)

    def solve(self, max_iter=125, force=False):
        self._chk(self.L.gusto_solve_trajopt(self.h, int(max_iter)), "solve_trajopt")

    def solve_async(self, max_iter=125, force=False):
        """gusto_solve_trajopt_async: enqueue the launch of the batch and return; wait() or any getter completes it."""
        self._chk(self.L.gusto_solve_trajopt_async(self.h, int(max_iter)), "solve_trajopt_async")

    def history(self):
        B, H = self.B, self.hist_cap
        dk = ("rho_vec", "s_vec", "mu_vec", "xtol_vec", "ftol_vec", "ctol_vec", "J_true", "J_full", "convergence_measure")
        out = {k: np.zeros((B, H)) for k in dk}
        out.update({k: np.zeros((B, H), dtype=np.int32) for k in ("solver_status", "ipm_iters")})
        cnt = {k: np.zeros(B, dtype=np.int32) for k in ("n_solves", "n_mu", "n_xtol", "n_ftol", "n_ctol")}
        hs = TrajOptHistory()
        hs.hist_cap = H
        for k, v in list(out.items()) + list(cnt.items()):
            setattr(hs, k, v.ctypes.data)
        self._chk(self.L.gusto_get_trajopt_history(self.h, C.byref(hs)), "get_trajopt_history")
        out.update(cnt)
        return out

    def subproblem(self, Xp, Up, mu, s):
        """gusto_subproblem_trajopt: one convex subproblem per problem around (Xp, Up) with penalty mu and trust region s."""
        B = self.B
        Xp, Up = _arr(Xp).reshape(B, self.N, self.n), _arr(Up).reshape(B, self.N, self.m)
        mu, s = (_arr(np.broadcast_to(np.asarray(v, dtype=np.float64), (B,))) for v in (mu, s))
        Xn, Un, Dn, obj = np.zeros_like(Xp), np.zeros_like(Up), np.zeros_like(Xp), np.zeros(B)
        st, it = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
        self._chk(self.L.gusto_subproblem_trajopt(self.h, B, Xp.ctypes.data, Up.ctypes.data, mu.ctypes.data, s.ctypes.data,
                                                  Xn.ctypes.data, Un.ctypes.data, Dn.ctypes.data, obj.ctypes.data,
                                                  st.ctypes.data, it.ctypes.data), "subproblem_trajopt")
        return dict(X=Xn, U=Un, D=Dn, obj=obj, status=st, iters=it, dual=self.dual())

    def shoot(self, *a, **k):
        raise GustoError("TrajOptSolver: shooting belongs to the GuSTO path")

    def verify(self, *a, **k):
        raise GustoError("TrajOptSolver: verify / interpolate are not supported on TrajOpt handles (gusto_verify answers GUSTO_ERR_ARG)")

    interpolate = verify

    def tvlqr(self, *a, **k):
        raise GustoError("TrajOptSolver: tvlqr is not supported on TrajOpt handles (gusto_tvlqr answers GUSTO_ERR_ARG)")

    def simulate(self, *a, **k):
        raise GustoError("TrajOptSolver: simulate is not supported on TrajOpt handles (gusto_simulate answers GUSTO_ERR_ARG)")

    def simulate_disturbed(self, *a, **k):
        raise GustoError("TrajOptSolver: simulate_disturbed is not supported on TrajOpt handles (gusto_simulate_disturbed answers GUSTO_ERR_ARG)")

    def lincov(self, *a, **k):
        raise GustoError("TrajOptSolver: lincov is not supported on TrajOpt handles (gusto_lincov answers GUSTO_ERR_ARG)")

    def lincov_disturbed(self, *a, **k):
        raise GustoError("TrajOptSolver: lincov_disturbed is not supported on TrajOpt handles (gusto_lincov_disturbed answers GUSTO_ERR_ARG)")

    def lincov_dense(self, *a, **k):
        raise GustoError("TrajOptSolver: lincov_dense is not supported on TrajOpt handles (gusto_lincov_dense answers GUSTO_ERR_ARG)")

    def set_problems_multistart(self, *a, **k):
        raise GustoError("TrajOptSolver: multi-start problems are not supported on TrajOpt handles (gusto_set_problems_multistart answers GUSTO_ERR_ARG)")

    def select_best(self, *a, **k):
        raise GustoError("TrajOptSolver: select_best is not supported on TrajOpt handles (gusto_select_best answers GUSTO_ERR_ARG)")

    def set_problems_replan(self, *a, **k):
        raise GustoError("TrajOptSolver: replanning is not supported on TrajOpt handles (gusto_set_problems_replan answers GUSTO_ERR_ARG)")

    set_problems_replan_knots = set_problems_replan

    def tighten_env(self, *a, **k):
        raise GustoError("TrajOptSolver: tighten_env is not supported on TrajOpt handles (gusto_tighten_env answers GUSTO_ERR_ARG)")

    def set_problems_roadmap(self, *a, **k):
        raise GustoError("TrajOptSolver: roadmap seeds are not supported on TrajOpt handles (gusto_set_problems_roadmap answers GUSTO_ERR_ARG)")

    def set_problems_trajlib(self, *a, **k):
        raise GustoError("TrajOptSolver: library seeds are not supported on TrajOpt handles (gusto_set_problems_trajlib answers GUSTO_ERR_ARG)")


class TrajLib:
    """Thin owner of one gusto_trajlib: solved trajectories of one model and horizon on one GPU, the seeds of later queries
    (BatchSolver.set_problems_trajlib).  w_init / w_goal [x_dim], w_tf: the weights of the distance (None: the library's defaults,
    1 on every state of both vectors and 0 -- a placeholder, the states have different units)."""

    def __init__(self, model, N, cap, device=0, w_init=None, w_goal=None, w_tf=None, lds_tile=None):
        self.L = lib()
        self.model, self.N, self.cap, self.device = model, N, cap, device
        self.n, self.m = MODEL_DIMS[model]
        o = default_trajlib_opts(model)
        for name, w in (("w_init", w_init), ("w_goal", w_goal)):
            if w is not None:
                w = np.broadcast_to(np.asarray(w, dtype=np.float64), (self.n,))
                for i in range(self.n):
                    getattr(o, name)[i] = w[i]
        if w_tf is not None:
            o.w_tf = float(w_tf)
        if lds_tile is not None:
            o.lds_tile = int(lds_tile)
        self.opts = o
        self.h = C.c_void_p()
        rc = self.L.gusto_trajlib_create(C.byref(self.h), model, N, cap, device, C.byref(o))
        if rc:
            msg = self.L.gusto_trajlib_last_error(None)
            self.h = C.c_void_p()
            raise GustoError(f"gusto_trajlib_create -> {rc}: {msg.decode() if msg else ''}")

    def _chk(self, rc, what):
        if rc:
            msg = self.L.gusto_trajlib_last_error(self.h)
            raise GustoError(f"gusto_trajlib_{what} -> {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "h", None) and self.h:
            self.L.gusto_trajlib_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        c, cap = C.c_int(), C.c_int()
        self._chk(self.L.gusto_trajlib_size(self.h, C.byref(c), C.byref(cap)), "size")
        return c.value

    def clear(self):
        self._chk(self.L.gusto_trajlib_clear(self.h), "clear")

    def add_from(self, solver, mask=None, tag=None):
        """gusto_trajlib_add: appends the problems of the BatchSolver whose mask is nonzero (None: converged and successful), in
        ascending order, device to device; tag [B] or one integer for all (None: 0).  Returns the number appended."""
        mk = None if mask is None else _arr(np.asarray(mask).astype(bool), np.int32).reshape(solver.B)
        tg = None if tag is None else _arr(np.broadcast_to(np.asarray(tag, dtype=np.int32), (solver.B,)), np.int32)
        n = C.c_int()
        self._chk(self.L.gusto_trajlib_add(self.h, solver.h, None if mk is None else mk.ctypes.data, None if tg is None else tg.ctypes.data,
                                           C.byref(n)), "add")
        return n.value

    def add_host(self, x_init, goal_lo, goal_hi, tf, X, U, tag=None):
        """gusto_trajlib_add_host: appends entries from host arrays ([n, x_dim] each, tf [n], X [n, N, x_dim], U [n, N, u_dim])"""
        x_init, goal_lo, goal_hi = (_arr(a).reshape(-1, self.n) for a in (x_init, goal_lo, goal_hi))
        n = x_init.shape[0]
        tf = _arr(np.broadcast_to(np.asarray(tf, dtype=np.float64), (n,)))
        X, U = _arr(X).reshape(n, self.N, self.n), _arr(U).reshape(n, self.N, self.m)
        tg = None if tag is None else _arr(np.broadcast_to(np.asarray(tag, dtype=np.int32), (n,)), np.int32)
        self._chk(self.L.gusto_trajlib_add_host(self.h, n, x_init.ctypes.data, goal_lo.ctypes.data, goal_hi.ctypes.data, tf.ctypes.data,
                                                None if tg is None else tg.ctypes.data, X.ctypes.data, U.ctypes.data), "add_host")

    def get(self):
        """gusto_trajlib_get: a dict of x_init, goal_c [L, x_dim], tf [L], tag [L], X [L, N, x_dim], U [L, N, u_dim]"""
        c = len(self)
        out = dict(x_init=np.zeros((c, self.n)), goal_c=np.zeros((c, self.n)), tf=np.zeros(c), tag=np.zeros(c, np.int32),
                   X=np.zeros((c, self.N, self.n)), U=np.zeros((c, self.N, self.m)))
        self._chk(self.L.gusto_trajlib_get(self.h, *(out[k].ctypes.data for k in ("x_init", "goal_c", "tf", "tag", "X", "U"))), "get")
        return out

    def save(self, path):
        """the entries and the weights as an .npz (numpy appends the suffix when it is missing)"""
        o = self.opts
        np.savez(path, model=self.model, N=self.N, w_init=np.array(o.w_init[:self.n]), w_goal=np.array(o.w_goal[:self.n]), w_tf=o.w_tf,
                 **self.get())

    @classmethod
    def load(cls, path, cap=None, device=0):
        """a library from save(): the same entries in the same order, the same weights; cap: at least the entries (None: exactly)"""
        d = np.load(path)
        c = len(d["tf"])
        out = cls(int(d["model"]), int(d["N"]), max(c, 1) if cap is None else cap, device=device, w_init=d["w_init"], w_goal=d["w_goal"],
                  w_tf=float(d["w_tf"]))
        if c:
            out.add_host(d["x_init"], d["goal_c"], d["goal_c"], d["tf"], d["X"], d["U"], tag=d["tag"])
        return out
