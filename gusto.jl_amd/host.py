"""Host-side mirror of the reference's driver interface for the GuSTO path.

The reference is Julia (no Julia toolchain in this image), so the host layer above the C ABI is written in Python
with the reference's names and argument meaning; julia/GuSTOHIP.jl holds the same logic as `ccall`s for a Julia
host.  What is mirrored (reference file:line):

  Goal / PointGoal / BoxGoal / GoalSet / add_goal!        src/goals.jl:1-48, src/types.jl:26-30
  ProblemDefinition, Trajectory                           src/types.jl:32-46,235
  TrajectoryOptimizationProblem / ...Solution             src/types.jl:48-61,196-202,228
  SCPProblem, SCPSolution (+ SCPParam_GuSTO histories)    src/types.jl:78-86,150-173,233,256-259; scp_gusto.jl:4-24
  solve_SCP!(TOS, TOP, solve_method!, init, solver; ...)  src/traj_opt.jl:47-72
  solve_gusto_jump! -> solve_gusto_hip!                   src/scp/scp_gusto.jl:49   (the plug-in seam)

plus `solve_SCP_batch!`, which the reference does not have (it solves one problem at a time), and the rank
sharding used for multi-GPU runs (independent problems, no data-path collective).
"""
import numpy as np

from . import _capi
from ._capi import (ASTROBEE_SE3, ASTROBEE_SE3_MANIFOLD, DUBINS_CAR, FREEFLYER_SE2, MODEL_DIMS, SCP_STATUS,
                    SOLVER_STATUS, BatchSolver)


# ---- models / robots / environments: parameter holders (src/dynamics/*.jl, src/robot/*.jl, src/environment/*.jl) ----
class _Model:
    model_id = None

    def __init__(self):
        self.x_dim, self.u_dim = MODEL_DIMS[self.model_id]


class FreeflyerSE2(_Model):
    model_id = FREEFLYER_SE2


class DubinsCar(_Model):
    model_id = DUBINS_CAR


class AstrobeeSE3(_Model):
    model_id = ASTROBEE_SE3


class AstrobeeSE3Manifold(_Model):
    model_id = ASTROBEE_SE3_MANIFOLD


class Robot:
    """Freeflyer() / Astrobee3D() / Car(): the constants live in gusto_model_params (gusto_default_params)."""


class Environment:
    """keepout_zones + obstacle_set as AABBs [min xyz | max xyz] and spheres [c xyz | r]  (types.jl:12-24)."""

    def __init__(self, boxes=None, spheres=None):
        self.boxes = np.zeros((0, 6)) if boxes is None else np.asarray(boxes, float).reshape(-1, 6)
        self.spheres = np.zeros((0, 4)) if spheres is None else np.asarray(spheres, float).reshape(-1, 4)


def Table(room="stanford"):
    from . import problems
    if room != "stanford":
        raise NotImplementedError("only Table(:stanford) is tabulated")
    return Environment(problems.table_stanford_boxes())


def ISSCorner(with_obstacles=False):
    from . import problems
    b, s = problems.iss_corner_env(with_obstacles)
    return Environment(b, s)


def BlankEnv():
    return Environment()


# ---- goals (src/goals.jl) ---------------------------------------------------------------------------
class PointGoal:
    def __init__(self, point):
        self.point = np.asarray(point, float)


class BoxGoal:
    def __init__(self, lower_bound, upper_bound):
        self.lower_bound, self.upper_bound = np.asarray(lower_bound, float), np.asarray(upper_bound, float)


class Goal:
    def __init__(self, params, t_guess, ind_coordinates):
        """ind_coordinates: a model (all coordinates) or 0-based indices (the reference is 1-based)."""
        self.params, self.t_guess, self.k_timestep, self.t_final = params, float(t_guess), None, None
        if isinstance(ind_coordinates, _Model):
            ind_coordinates = range(ind_coordinates.x_dim)
        self.ind_coordinates = np.asarray(list(ind_coordinates), int)


class GoalSet:
    def __init__(self):
        self.goals = []


def add_goal(goal_set, goal):
    goal_set.goals.append(goal)
    goal_set.goals.sort(key=lambda g: g.t_guess)


def _goal_bounds(goal_set, x_dim, tf_guess):
    """Flatten the goals active at tf_guess into (lo, hi): lo == hi -> hard equality row (csbce_goal_constraints),
    lo < hi -> hard box rows (csbci_goal_constraints), +-inf -> no goal on that coordinate (dynamics.jl:30-42)."""
    lo, hi = np.full(x_dim, -np.inf), np.full(x_dim, np.inf)
    for g in goal_set.goals:
        if g.t_guess != tf_guess:
            continue   # every row function of the reference hard-codes knot N (dynamics.jl:33,40)
        if isinstance(g.params, PointGoal):
            lo[g.ind_coordinates] = hi[g.ind_coordinates] = g.params.point
        elif isinstance(g.params, BoxGoal):
            lo[g.ind_coordinates], hi[g.ind_coordinates] = g.params.lower_bound, g.params.upper_bound
        else:
            raise NotImplementedError("BallGoal has no row function in the reference either")
    return lo, hi


# ---- problem / solution containers (src/types.jl) ---------------------------------------------------
class ProblemDefinition:
    def __init__(self, robot, model, env, x_init, goal_set):
        self.robot, self.model, self.env = robot, model, env
        self.x_init, self.goal_set = np.asarray(x_init, float), goal_set


class Trajectory:
    def __init__(self, X, U, Tf):
        self.X, self.U, self.Tf = X, U, float(Tf)        # X is x_dim x N as in the reference
        self.dt = self.Tf / (self.X.shape[1] - 1)         # types.jl:235


class TrajectoryOptimizationProblem:
    """types.jl:48-61,228.  fixed_final_time=False mirrors what the reference actually does with it: `Tf` becomes a free
    JuMP variable with the single row `Tf >= 0.1` (scp_gusto.jl:185-187,248-250), but no dynamics row, cost term or
    trust region contains it -- the trapezoid rows use traj_prev.dt (freeflyer_se2.jl:170) -- so the subproblem leaves
    it at its start value tf_guess (scp_gusto.jl:102) and every trip runs with dt = tf_guess/(N-1).  The mirror keeps
    Tf = tf_guess and enforces the one row there is."""

    def __init__(self, PD, N, tf_guess, fixed_final_time=False):
        if not fixed_final_time and tf_guess < 0.1:
            raise ValueError("free final time: the only row on Tf is Tf >= 0.1 (scp_gusto.jl:248-250); tf_guess violates it")
        self.PD, self.N, self.tf_guess, self.fixed_final_time = PD, int(N), float(tf_guess), bool(fixed_final_time)
        assign_timesteps(PD.goal_set, self.N, self.tf_guess)       # types.jl:58 via the constructor at :228


def assign_timesteps(goal_set, N, tf_guess):
    """goals.jl:18-22, literally: k_timestep = fld(N*tf_guess, N*t_guess) = floor(tf_guess / t_guess) -- 1 for a goal at the
    final time, NOT its knot index.  Nothing reads it for placement: the goal row functions hard-code knot N
    (dynamics.jl:33,40) and SCPConstraints only registers the goals whose time equals tf_guess (freeflyer_se2.jl:352-358),
    so goals at intermediate times are carried in the GoalSet and ignored by the solve -- here exactly as there."""
    for g in goal_set.goals:
        g.k_timestep = int((N * tf_guess) // (N * g.t_guess)) if g.t_guess > 0 else None


class SCPProblem:
    def __init__(self, TOP):
        self.PD, self.N, self.tf_guess = TOP.PD, TOP.N, TOP.tf_guess
        self.scp_params, self.model_params = _capi.default_params(TOP.PD.model.model_id)   # SCPParam + SCPParam_GuSTO
        self.Delta_vec, self.omega_vec, self.rho_vec = [], [], []
        self.trust_region_satisfied_vec, self.convex_ineq_satisfied_vec = [], []


class SCPSolution:
    def __init__(self, SCPP, traj_init):
        self.traj, self.SCPP = traj_init, SCPP
        self.dual = np.zeros(SCPP.PD.model.x_dim)
        self.J_true, self.J_full = [], []
        self.solver_status, self.scp_status = ["NA"], ["NA"]
        self.accept_solution, self.convergence_measure = [True], [0.0]
        self.successful = self.converged = False
        self.stop_reason = "MaxIter"      # gusto_get_status stop reason of the last solve_method! call (_capi.STOP_REASON)
        self.iterations, self.iter_elapsed_times, self.total_time = 0, [0.0], 0.0
        self._solver = None     # the GuSTO gusto_handle that owns the device-side state of this solution (resume, shooting)
        self._solver_trajopt = None   # the TrajOpt handle of this solution (gusto_create_trajopt), kept apart: neither algorithm
                                      # ever finds the other's handle


class TrajectoryOptimizationSolution:
    def __init__(self, TOP):
        n, m = TOP.PD.model.x_dim, TOP.PD.model.u_dim
        self.traj = Trajectory(np.zeros((n, TOP.N)), np.zeros((m, TOP.N)), TOP.tf_guess)
        self.SCPS = None
        self.total_time = 0.0


def init_traj_straightline(TOP):
    """freeflyer_se2.jl:97-111: linear interpolation x_init -> centre of the goals at the final time, U = 0."""
    n, m, N = TOP.PD.model.x_dim, TOP.PD.model.u_dim, TOP.N
    lo, hi = _goal_bounds(TOP.PD.goal_set, n, TOP.tf_guess)
    fin = np.isfinite(lo) & np.isfinite(hi)
    xg = np.where(fin, 0.5 * (np.where(fin, lo, 0.0) + np.where(fin, hi, 0.0)), 0.0)
    t = np.arange(N) / (N - 1)
    X = (1 - t)[None, :] * TOP.PD.x_init[:, None] + t[None, :] * xg[:, None]
    return Trajectory(X, np.zeros((m, N)), TOP.tf_guess)


# ---- the plug-in: solve_method!(SCPS, SCPP, solver, max_iter, force; kw...) ---------------------------------------
def _fetch(bs, XU=None):
    """Everything a solution needs from one handle, copied device -> host ONCE per solve (not once per problem).
    `XU`: the shard's trajectories when a device-side gather (gusto_gather_peer) has already brought them over."""
    X, U = XU if XU is not None else bs.traj()
    return dict(X=X, U=U, st=bs.status(), h=bs.history(), dual=bs.dual())


def _fill_solution(SCPS, SCPP, snap, b, elapsed):
    st, h = snap["st"], snap["h"]
    stop = int(st["stop_reason"][b])
    if stop == 4:
        raise _capi.GustoError("history capacity of the handle reached before iter_cap (GUSTO_STOP_HIST_FULL): the "
                               "solver would silently stop iterating; create the solution with a larger hist_cap")
    SCPS.traj.X, SCPS.traj.U = snap["X"][b].T.copy(), snap["U"][b].T.copy()
    nh, nJ, nr = h["n_hist"][b], h["nJ"][b], h["n_rho"][b]
    SCPS.J_true, SCPS.J_full = list(h["J_true"][b, :nJ]), list(h["J_full"][b, :nJ])
    # a failed subproblem pushes its status and nothing else before the early return (scp_gusto.jl:106-111)
    ns = nh + 1 if stop == 2 else nh
    SCPS.solver_status = [SOLVER_STATUS[int(v)] for v in h["solver_status"][b, :ns]]
    SCPS.scp_status = [SCP_STATUS[int(v)] for v in h["scp_status"][b, :nh]]
    SCPS.accept_solution = [bool(v) for v in h["accept_solution"][b, :nh]]
    SCPS.convergence_measure = list(h["convergence_measure"][b, :nh])
    SCPS.iterations = int(st["iterations"][b])
    SCPS.converged, SCPS.successful = bool(st["converged"][b]), bool(st["successful"][b])
    SCPS.stop_reason = _capi.STOP_REASON[stop]
    SCPS.dual = snap["dual"][b].copy()
    SCPS.total_time += elapsed
    SCPS.iter_elapsed_times = [0.0] + [SCPS.total_time / max(1, SCPS.iterations)] * SCPS.iterations
    SCPP.Delta_vec, SCPP.omega_vec = list(h["Delta"][b, :nh]), list(h["omega"][b, :nh])
    SCPP.rho_vec = list(h["rho"][b, :nr])
    SCPP.trust_region_satisfied_vec = [bool(v) for v in h["trust_region_satisfied"][b, :nh]]
    SCPP.convex_ineq_satisfied_vec = [bool(v) for v in h["convex_ineq_satisfied"][b, :nh]]
    SCPP.obstacle_toggle_distance = SCPP.Delta_vec[-1] / 8 + SCPP.model_params.clearance


def _hist_cap(max_iter):
    """Every call adds its iterations plus one leading J_true/rho entry; room for a few resumed calls."""
    return max(64, 4 * max_iter + 16)


def solve_gusto_hip(SCPS, SCPP, solver="hip", max_iter=30, force=False, device=0, hist_cap=None, **kwarg):
    """Same positional signature as solve_gusto_jump! (scp_gusto.jl:49).  Mutates SCPS / SCPP in place; a second
    call resumes from SCPS (iter_cap = iterations + max_iter, scp_gusto.jl:67).

    `hist_cap` sizes the history vectors of the handle the FIRST call creates: every call consumes one leading
    J_true / rho entry plus one entry per trip, so a caller that resumes in short calls (solve_SCPshooting: one trip per
    call) passes the capacity of its whole iteration budget; the default covers a few resumed calls of `max_iter`."""
    model = SCPP.PD.model
    n, N = model.x_dim, SCPP.N
    bs = SCPS._solver
    if not (type(bs) is BatchSolver and bs.h and bs.model == model.model_id and bs.N == N and bs.device == device):
        if bs is not None:      # (a handle of another model / horizon / device cannot resume this solution)
            bs.close()
        env = SCPP.PD.env
        bs = BatchSolver(model.model_id, N, 1, hist_cap=hist_cap or _hist_cap(max_iter), device=device, boxes=env.boxes,
                         spheres=env.spheres, scp_params=SCPP.scp_params, model_params=SCPP.model_params)
        lo, hi = _goal_bounds(SCPP.PD.goal_set, n, SCPP.tf_guess)
        bs.set_problems(SCPP.PD.x_init[None], lo[None], hi[None], [SCPP.tf_guess],
                        SCPS.traj.X.T[None].copy(), SCPS.traj.U.T[None].copy())
        SCPS._solver = bs
    bs.solve(max_iter, force)
    _fill_solution(SCPS, SCPP, _fetch(bs), 0, bs.last_solve_ms() * 1e-3)


def solve_SCP(TOS, TOP, solve_method, init_method, solver="hip", max_iter=30, force=False, **kwarg):
    """traj_opt.jl:47-72 (both overloads: `init_method` may be a function of TOP or a Trajectory)."""
    SCPP = SCPProblem(TOP)
    traj_init = init_method(TOP) if callable(init_method) else init_method
    SCPS = SCPSolution(SCPP, traj_init)
    TOS.traj, TOS.SCPS = SCPS.traj, SCPS          # aliasing as in traj_opt.jl:58
    solve_method(SCPS, SCPP, solver, max_iter, force, **kwarg)
    return SCPS


# ---- TrajOpt behind the same seam: solve_trajopt_jump! -> solve_trajopt_hip! (src/scp/scp_trajopt.jl:33) ------------------
def solve_trajopt_hip(SCPS, SCPP, solver="hip", max_iter=125, force=False, device=0, trajopt_params=None, **kwarg):
    """Same positional signature as solve_trajopt_jump! (scp_trajopt.jl:33): solve_SCP!(TOS, TOP, solve_trajopt_hip!, init,
    "hip").  FreeflyerSE2 and AstrobeeSE3.  Fills the SCPSolution vectors the reference pushes (J_true, J_full,
    convergence_measure, solver_status, dual, iterations, converged) and SCPP.param.alg's rho_vec / mu_vec / s_vec /
    xtol_vec / ftol_vec / ctol_vec (here: attributes of SCPP).  `max_iter` caps the convex subproblems (the reference
    computes iter_cap and never reads it); `force` is unused there too."""
    model = SCPP.PD.model
    n, N = model.x_dim, SCPP.N
    env = SCPP.PD.env
    tp = trajopt_params or _capi.default_trajopt_params(model.model_id)
    total = tp.max_penalty_iteration * tp.max_convex_iteration * tp.max_trust_iteration
    # one handle per SCPSolution: a repeated call re-uses it (device allocations, kernel attributes) and only sets the problem
    # again -- solve_trajopt_jump! has no resume either, every call runs the whole three-loop schedule from SCPS.traj
    bs = SCPS._solver_trajopt
    if not (isinstance(bs, _capi.TrajOptSolver) and bs.h and bs.model == model.model_id and bs.N == N and bs.device == device
            and bs.hist_cap >= 2 * total + 16):
        if bs is not None:
            bs.close()
        bs = _capi.TrajOptSolver(model.model_id, N, 1, hist_cap=2 * total + 16, device=device, boxes=env.boxes,
                                 spheres=env.spheres, model_params=SCPP.model_params, trajopt_params=tp)
    else:
        bs.set_env(env.boxes, env.spheres)
        bs._chk(bs.L.gusto_set_params(bs.h, None, _capi.C.byref(SCPP.model_params)), "set_params")
        bs._chk(bs.L.gusto_set_trajopt_params(bs.h, _capi.C.byref(tp)), "set_trajopt_params")
    if kwarg.get("ipm_opts") is not None:       # (applied on every call, re-used handle or not)
        bs._chk(bs.L.gusto_set_ipm_opts(bs.h, _capi.C.byref(kwarg["ipm_opts"])), "set_ipm_opts")
    lo, hi = _goal_bounds(SCPP.PD.goal_set, n, SCPP.tf_guess)
    bs.set_problems(SCPP.PD.x_init[None], lo[None], hi[None], [SCPP.tf_guess], SCPS.traj.X.T[None].copy(), SCPS.traj.U.T[None].copy())
    bs.solve(max_iter)
    X, U = bs.traj()
    _fill_trajopt_solution(SCPS, SCPP, dict(X=X, U=U, st=bs.status(), h=bs.history(), dual=bs.dual()), 0,
                           bs.last_solve_ms() * 1e-3)
    SCPS._solver_trajopt = bs


def _fill_trajopt_solution(SCPS, SCPP, snap, b, elapsed):
    """The vectors solve_trajopt_jump! pushes (scp_trajopt.jl:60-157) for problem b of a TrajOpt handle's snapshot."""
    X, U, st, h = snap["X"], snap["U"], snap["st"], snap["h"]
    ns = int(st["iterations"][b])
    SCPS.traj.X, SCPS.traj.U = X[b].T.copy(), U[b].T.copy()
    SCPS.J_true = list(h["J_true"][b, :ns + 1])
    SCPS.J_full = list(h["J_full"][b, :ns])
    SCPS.convergence_measure = [0.0] + list(h["convergence_measure"][b, 1:ns + 1])
    stop = int(st["stop_reason"][b])
    SCPS.solver_status = [SOLVER_STATUS[int(v)] for v in h["solver_status"][b, :ns + 1 + (stop == 2)]]
    SCPS.iterations, SCPS.converged, SCPS.successful = ns, bool(st["converged"][b]), False
    SCPS.stop_reason = _capi.STOP_REASON[stop]
    SCPS.dual = snap["dual"][b].copy()
    SCPS.total_time += elapsed
    SCPS.iter_elapsed_times = [0.0] + [SCPS.total_time / max(1, ns)] * ns
    SCPP.rho_vec, SCPP.s_vec = list(h["rho_vec"][b, :ns + 1]), list(h["s_vec"][b, :ns + 1])
    SCPP.mu_vec = list(h["mu_vec"][b, :h["n_mu"][b]])
    SCPP.xtol_vec, SCPP.ftol_vec = list(h["xtol_vec"][b, :h["n_xtol"][b]]), list(h["ftol_vec"][b, :h["n_ftol"][b]])
    SCPP.ctol_vec = list(h["ctol_vec"][b, :h["n_ctol"][b]])
    SCPP.obstacle_toggle_distance = SCPP.model_params.clearance + 1.0      # scp_trajopt.jl:64


# ---- indirect shooting seeded by the SCP dual (src/shooting.jl, src/traj_opt.jl:4-45, src/types.jl:187-227) --------------
class ShootingProblem:
    """types.jl:219-227: p0 = SCPS.dual, tf = SCPS.traj.Tf, x_goal = centre of the goals at the final time (zeros
    elsewhere).  (At HEAD the constructor reads an undefined `N`; `TOP.N` is what it means.)"""

    def __init__(self, TOP, SCPS):
        n = TOP.PD.model.x_dim
        lo, hi = _goal_bounds(TOP.PD.goal_set, n, TOP.tf_guess)
        fin = np.isfinite(lo) & np.isfinite(hi)
        self.PD, self.N, self.tf = TOP.PD, TOP.N, SCPS.traj.Tf
        self.dt = self.tf / (self.N - 1)
        self.p0 = np.array(SCPS.dual, float)
        self.x_goal = np.where(fin, 0.5 * (np.where(fin, lo, 0.0) + np.where(fin, hi, 0.0)), 0.0)
        self._scps = SCPS


class ShootingSolution:
    """types.jl:198-209"""

    def __init__(self, SP, traj_init):
        self.traj, self.SP = traj_init, SP
        self.J_true, self.prob_status, self.convergence_measure = [], ["NA"], [float("nan")]
        self.converged, self.iter_elapsed_times = False, [0.0]


def cost_true(traj):
    """freeflyer_se2.jl:66-76 / dubins_car.jl:54-69: trapezoid control effort."""
    U = traj.U
    return float(np.sum(0.5 * traj.dt * (U[:, :-1] ** 2 + U[:, 1:] ** 2)))


def convergence_metric(traj, traj_prev):
    """traj_opt.jl:74-85"""
    return float(np.linalg.norm(traj.X - traj_prev.X, axis=0).max() / np.linalg.norm(traj.X, axis=0).max())


def solve_shooting(SS, SP, **opts):
    """solve!(SS, SP) (shooting.jl:4-49) on the GPU: gusto_shoot on the handle that holds the SCP state of this problem."""
    import time
    bs = SP._scps._solver
    if bs is None:
        raise _capi.GustoError("solve!(SS, SP): run solve_gusto_hip! on the SCPSolution first (it owns the device state)")
    t0 = time.perf_counter()
    r = bs.shoot(SP.p0[None], **opts)
    el = time.perf_counter() - t0
    if int(r["status"][0]) == 1:                                   # sol_newton.f_converged
        new_traj = Trajectory(r["X"][0].T.copy(), r["U"][0].T.copy(), SP.tf)
        SS.prob_status.append("Optimal")
        SS.J_true.append(cost_true(new_traj))
        SS.convergence_measure.append(convergence_metric(new_traj, SS.traj))
        SS.traj = new_traj
    else:
        SS.prob_status.append("Diverged")
        SS.J_true.append(float("nan"))
        SS.convergence_measure.append(float("nan"))
    SS.iter_elapsed_times.append(el)
    SS.p0 = r["p0"][0]
    return r


def solve_SCPshooting(TOS, TOP, solve_method, init_method, solver="hip", max_iter=30, **kwarg):
    """traj_opt.jl:4-45: one SCP iteration, then alternately a shooting attempt seeded by the SCP dual and another SCP
    iteration, until two consecutive successful shooting runs agree (sum of their convergence measures below the
    threshold) or the SCP itself converges / runs out of iterations."""
    SCPP = SCPProblem(TOP)
    traj_init = init_method(TOP) if callable(init_method) else init_method
    TOS.SCPS = SCPS = SCPSolution(SCPP, traj_init)
    SP = ShootingProblem(TOP, SCPS)
    TOS.SS = SS = ShootingSolution(SP, Trajectory(traj_init.X.copy(), traj_init.U.copy(), traj_init.Tf))
    # one-trip calls: each consumes two history entries (its leading J_true / rho entry and the trip), so the handle is
    # sized for the whole budget here -- the reference's vectors grow without bound (scp_gusto.jl:15-19)
    kwarg.setdefault("hist_cap", _hist_cap(max_iter))
    solve_method(SCPS, SCPP, solver, 1, **kwarg)
    SS.J_true.append(SCPS.J_true[0])
    # (a run that stopped for good -- failed subproblem, omega > omega_max -- leaves the loop: the reference's solve_method!
    # returns early there without counting an iteration, scp_gusto.jl:107-111,163-166, and its loop would spin for ever)
    while not SCPS.converged and SCPS.iterations < max_iter and SCPS.stop_reason not in _DEAD_STOPS:
        SP = ShootingProblem(TOP, SCPS)
        solve_shooting(SS, SP)
        spread = 2
        cm = SS.convergence_measure[-spread:]
        if SCPS.iterations > spread and not any(np.isnan(cm)) and sum(cm) <= SCPP.scp_params.convergence_threshold:
            SS.converged = True
            TOS.traj = Trajectory(SS.traj.X.copy(), SS.traj.U.copy(), SS.traj.Tf)
            TOS.total_time = SCPS.total_time + sum(SS.iter_elapsed_times)
            return TOS
        solve_method(SCPS, SCPP, solver, 1, **kwarg)
    TOS.traj = Trajectory(SCPS.traj.X.copy(), SCPS.traj.U.copy(), SCPS.traj.Tf)
    TOS.total_time = SCPS.total_time + sum(SS.iter_elapsed_times)
    return TOS


_DEAD_STOPS = ("SubproblemFailed", "OmegaMaxExceeded", "HistoryFull")


def solve_SCPshooting_batch(TOSs, TOPs, solve_method=None, init_method=init_traj_straightline, solver="hip", max_iter=30,
                            device=0, **kwarg):
    """solve_SCPshooting! (traj_opt.jl:4-45) for a list of problems of one model and horizon on ONE handle: per round one
    gusto_shoot and one gusto_solve(1) over the problems still in their loop (gusto_set_active carries the per-problem
    condition `!SCPS.converged && SCPS.iterations < max_iter` of traj_opt.jl:23), every problem leaving exactly where the
    single-problem driver above leaves -- its SCPSolution / ShootingSolution are those solve_SCPshooting fills, bit for bit."""
    import time
    if solve_method not in (None, solve_gusto_hip):
        raise NotImplementedError("solve_SCPshooting_batch!: the shooting refinement follows the GuSTO solve (solve_gusto_hip)")
    if len(TOSs) != len(TOPs) or not TOPs:
        raise ValueError("solve_SCPshooting_batch!: need as many solutions as problems, at least one")
    TOP0 = TOPs[0]
    model, N, B = TOP0.PD.model, TOP0.N, len(TOPs)
    n = model.x_dim
    for t in TOPs[1:]:
        if type(t.PD.model) is not type(model) or t.N != N:
            raise ValueError("solve_SCPshooting_batch!: all problems must share the model type and N")
    same_env = all(np.array_equal(t.PD.env.boxes, TOP0.PD.env.boxes) and np.array_equal(t.PD.env.spheres, TOP0.PD.env.spheres)
                   for t in TOPs[1:])
    SCPPs = [SCPProblem(t) for t in TOPs]
    inits = [init_method(t) if callable(init_method) else Trajectory(init_method.X.copy(), init_method.U.copy(), init_method.Tf)
             for t in TOPs]
    SCPSs = [SCPSolution(p, i) for p, i in zip(SCPPs, inits)]
    # ONE handle solves the batch with ONE set of SCP and model parameters (gusto_set_params): a problem with another robot's
    # mass or another trust-region schedule would silently be solved with problem 0's
    for p in SCPPs[1:]:
        if bytes(p.scp_params) != bytes(SCPPs[0].scp_params) or bytes(p.model_params) != bytes(SCPPs[0].model_params):
            raise ValueError("solve_SCPshooting_batch!: all problems must share the SCP parameters and the model / robot parameters")
    bs = BatchSolver(model.model_id, N, B, hist_cap=kwarg.get("hist_cap") or _hist_cap(max_iter), device=device,
                     boxes=TOP0.PD.env.boxes, spheres=TOP0.PD.env.spheres, scp_params=SCPPs[0].scp_params,
                     model_params=SCPPs[0].model_params)
    if not same_env:
        bs.set_env_batch([t.PD.env.boxes for t in TOPs], [t.PD.env.spheres for t in TOPs])
    bounds = [_goal_bounds(t.PD.goal_set, n, t.tf_guess) for t in TOPs]
    bs.set_problems(np.stack([t.PD.x_init for t in TOPs]), np.stack([b[0] for b in bounds]), np.stack([b[1] for b in bounds]),
                    np.array([t.tf_guess for t in TOPs]), np.stack([t.X.T for t in inits]), np.stack([t.U.T for t in inits]))
    SSs = []
    for b, (TOS, TOP) in enumerate(zip(TOSs, TOPs)):
        TOS.SCPS = SCPSs[b]
        SP = ShootingProblem(TOP, SCPSs[b])
        TOS.SS = ShootingSolution(SP, Trajectory(inits[b].X.copy(), inits[b].U.copy(), inits[b].Tf))
        SSs.append(TOS.SS)

    def scp_round(live):       # solve_method!(SCPS, SCPP, solver, 1) of every live problem: ONE launch
        bs.set_active(live)
        bs.solve(1)
        snap = _fetch(bs)
        per = bs.last_solve_ms() * 1e-3 / max(1, int(np.sum(live)))
        for b in np.flatnonzero(live):
            _fill_solution(SCPSs[b], SCPPs[b], snap, b, per)

    live = np.ones(B, bool)
    scp_round(live)
    for b in range(B):
        SSs[b].J_true.append(SCPSs[b].J_true[0])
    done_by_shooting = np.zeros(B, bool)
    while True:
        live = np.array([not S.converged and S.iterations < max_iter and S.stop_reason not in _DEAD_STOPS for S in SCPSs]) \
            & ~done_by_shooting
        if not live.any():
            break
        bs.set_active(live)
        t0 = time.perf_counter()
        r = bs.shoot()                                    # seeds = SCPS.dual of every problem, read on the device
        el = (time.perf_counter() - t0) / int(live.sum())
        for b in np.flatnonzero(live):
            SS, SCPS = SSs[b], SCPSs[b]
            SS.SP = ShootingProblem(TOPs[b], SCPS)
            if int(r["status"][b]) == 1:
                new_traj = Trajectory(r["X"][b].T.copy(), r["U"][b].T.copy(), SS.SP.tf)
                SS.prob_status.append("Optimal")
                SS.J_true.append(cost_true(new_traj))
                SS.convergence_measure.append(convergence_metric(new_traj, SS.traj))
                SS.traj = new_traj
            else:
                SS.prob_status.append("Diverged")
                SS.J_true.append(float("nan"))
                SS.convergence_measure.append(float("nan"))
            SS.iter_elapsed_times.append(el)
            SS.p0 = r["p0"][b]
            cm = SS.convergence_measure[-2:]
            if SCPS.iterations > 2 and not any(np.isnan(cm)) and sum(cm) <= SCPPs[b].scp_params.convergence_threshold:
                SS.converged = True
                done_by_shooting[b] = True
        live &= ~done_by_shooting
        if live.any():
            scp_round(live)
    bs.set_active(None)
    for b, TOS in enumerate(TOSs):
        src = SSs[b].traj if done_by_shooting[b] else SCPSs[b].traj
        TOS.traj = Trajectory(src.X.copy(), src.U.copy(), src.Tf)
        TOS.total_time = SCPSs[b].total_time + sum(SSs[b].iter_elapsed_times)
        SCPSs[b]._solver = None          # (the batch handle is not a per-problem resume handle)
    bs.close()
    return TOSs


# ---- batch API (new: the reference has no batch mode) --------------------------------------------------------------
# ---- post-solve checks of the Astrobee model files on the device (csrc/verify.hip) --------------------------------
def _verify_handle(traj, SCPP, device=0):
    """A one-problem handle that holds `traj` as its trajectory: the model, robot scalars and Workspace of SCPP."""
    model = SCPP.PD.model
    n, N = model.x_dim, SCPP.N
    if traj.X.shape != (n, N):
        raise ValueError("traj does not have the problem's x_dim x N")
    env = SCPP.PD.env
    bs = BatchSolver(model.model_id, N, 1, hist_cap=8, device=device, boxes=env.boxes, spheres=env.spheres,
                     scp_params=SCPP.scp_params, model_params=SCPP.model_params)
    lo, hi = _goal_bounds(SCPP.PD.goal_set, n, SCPP.tf_guess)
    bs.set_problems(SCPP.PD.x_init[None], lo[None], hi[None], [traj.Tf], traj.X.T[None].copy(), traj.U.T[None].copy())
    return bs


def interpolate_traj(traj, SCPP, dt_min=0.1):
    """astrobee_se3_manifold.jl:1011-1042: the trajectory at Nstep = ceil(dt / dt_min) RK4 samples per knot interval, every
    interval restarted from its knot under the held control; a Trajectory with X x_dim x Nfull, U u_dim x (Nfull - 1)."""
    bs = _verify_handle(traj, SCPP)
    try:
        nfull, Xf, Uf = bs.interpolate(dt_min=dt_min, nstep_cap=max(64, int(np.ceil(traj.dt / dt_min))))
    finally:
        bs.close()
    out = Trajectory(Xf[0, :nfull[0]].T.copy(), Uf[0, :nfull[0] - 1].T.copy(), traj.Tf)
    return out


def verify_collision_free(traj, SCPP):
    """astrobee_se3_manifold.jl:1057-1077: (free, k, dist) -- the first knot (1-based) whose signed distance is negative, in
    the reference's obstacle-major order; (True, 0, 0.0) for a free trajectory."""
    bs = _verify_handle(traj, SCPP)
    try:
        r = bs.verify(nstep=1, dense_collision=0)
    finally:
        bs.close()
    return bool(r["collision_free"][0]), int(r["first_knot"][0]), float(r["first_dist"][0])


def dynamics_constraint_satisfaction(traj, SCPP):
    """astrobee_se3_manifold.jl:1044-1055: sum_k |(x_{k+1} - x_k) / dt - f(x_k, u_k)|_1."""
    bs = _verify_handle(traj, SCPP)
    try:
        r = bs.verify(nstep=1, dense_collision=0)
    finally:
        bs.close()
    return float(r["dyn_defect_l1"][0])


def tvlqr(traj, SCPP, Q=1.0, R=1.0, Qf=1.0, dt_min=0.1, store_P=False):
    """Time-varying LQR gains around one trajectory (gusto_tvlqr; no counterpart in the reference): the feedback law
    u = U[:, k] - K[k] (x(t_k) - X[:, k]) on the exact derivative of the zero-order-hold RK4 roll-out interpolate_traj performs.
    Q, R, Qf: diagonal weights, scalars or vectors.  Returns the one-problem result: K [N-1, u_dim, x_dim], AB [N-1, x_dim,
    x_dim + u_dim], P [x_dim, x_dim] of knot 1 ([N, x_dim, x_dim] with store_P), status, fail_knot."""
    bs = _verify_handle(traj, SCPP)
    try:
        r = bs.tvlqr(dict(Q=Q, R=R, Qf=Qf, dt_min=dt_min, nstep_cap=max(64, int(np.ceil(traj.dt / dt_min))), store_P=int(store_P)))
    finally:
        bs.close()
    return _capi.TvlqrResult(r.K[0], r.P[0], r.AB[0], int(r.status[0]), int(r.fail_knot[0]))


def simulate(traj, SCPP, K=None, pert=None, Q=1.0, R=1.0, Qf=1.0, disturb=None, plant=None, white=None, **opts):
    """Closed-loop Monte Carlo roll-outs of the tracking law around one trajectory (gusto_simulate; no counterpart in the
    reference): u = clip(U[:, k] - K[k] (x(t_k) - X[:, k]), u_lo, u_hi) from n_samples perturbed starts.  K [N-1, u_dim, x_dim]:
    the gains, default those of tvlqr(traj, SCPP, Q, R, Qf); pert [S, x_dim + u_dim]: the perturbations, default generated on
    the device; opts: gusto_simulate_opts fields.  Returns the one-problem report as a dict.
    disturb (a dict: plant_rel, dw), plant [S, 6] or white [N-1, S, u_dim]: when any of them is given the roll-outs are those of
    gusto_simulate_disturbed -- the same law on a plant whose mass, inertia, dubins_v and dubins_k differ per sample, with an
    actuator noise drawn anew in every hold interval -- and the report carries `plant`, the [S, 6] scalars that were used."""
    bs = _verify_handle(traj, SCPP)
    try:
        cap = max(64, int(np.ceil(traj.dt / opts.get("dt_min", 0.1))))
        if K is None:
            bs.tvlqr(dict(Q=Q, R=R, Qf=Qf, dt_min=opts.get("dt_min", 0.1), nstep=opts.get("nstep", 0), nstep_cap=opts.get("nstep_cap", cap)))
        one = lambda a: None if a is None else np.asarray(a, float)[None]
        if disturb is None and plant is None and white is None:
            r = bs.simulate(dict(dict(nstep_cap=cap), **opts), K=one(K), pert=one(pert))
        else:
            r = bs.simulate_disturbed(dict(dict(nstep_cap=cap), **opts), disturb, K=one(K), pert=one(pert), plant=one(plant), white=one(white))
            r["plant"] = bs.get_simulate_plant()
    finally:
        bs.close()
    return {k: v[0] for k, v in r.items()}


def lincov(traj, SCPP, K=None, S0=None, Q=1.0, R=1.0, Qf=1.0, dt_min=0.1, **opts):
    """Linear covariance analysis of the tracking law around one trajectory (gusto_lincov; no counterpart in the reference): the
    covariance of the state deviation and of a constant control offset carried through the closed loop of
    u = U[:, k] - K[k] (x(t_k) - X[:, k]) on the discrete Jacobians of tvlqr(traj, SCPP, Q, R, Qf, dt_min), and the margins it leaves
    to the keep-out set and the control bounds.  K [N-1, u_dim, x_dim]: the gains, default those of that tvlqr; S0
    [x_dim + u_dim, x_dim + u_dim]: the start covariance, default diag(dx0^2 / 3, du0^2 / 3); opts: gusto_lincov_opts fields.
    Returns the one-problem report as a dict."""
    bs = _verify_handle(traj, SCPP)
    try:
        bs.tvlqr(dict(Q=Q, R=R, Qf=Qf, dt_min=dt_min, nstep_cap=max(64, int(np.ceil(traj.dt / dt_min)))))
        r = bs.lincov(opts, K=None if K is None else np.asarray(K, float)[None], S0=None if S0 is None else np.asarray(S0, float)[None])
    finally:
        bs.close()
    return {k: v[0] for k, v in r.items()}


def lincov_disturbed(traj, SCPP, K=None, S0=None, Sth=None, disturb=None, Q=1.0, R=1.0, Qf=1.0, dt_min=0.1, **opts):
    """lincov() with an uncertain plant (gusto_lincov_disturbed; no counterpart in the reference): the deviation is augmented by
    the constant deviation of the plant scalars (mass, Jdiag, dubins_v, dubins_k) from the model's, to first order, and the
    per-interval noise disturb["dw"] joins du_white.  Sth [6, 6]: the covariance of the plant deviation, default the variances of
    the uniform draws of simulate()'s disturb["plant_rel"].  Returns lincov()'s report with Cd [N-1, x_dim, 6], the sensitivity
    of the roll-out map, and -- with store_S = 1 -- Sxt [N, x_dim, 6], the state / plant block of the covariance."""
    bs = _verify_handle(traj, SCPP)
    try:
        bs.tvlqr(dict(Q=Q, R=R, Qf=Qf, dt_min=dt_min, nstep_cap=max(64, int(np.ceil(traj.dt / dt_min)))))
        one = lambda a: None if a is None else np.asarray(a, float)[None]
        r = bs.lincov_disturbed(opts, disturb, K=one(K), S0=one(S0), Sth=one(Sth))
        r["Cd"], Sxt = bs.get_lincov_plant()
        if Sxt is not None:
            r["Sxt"] = Sxt
    finally:
        bs.close()
    return {k: v[0] for k, v in r.items()}


def lincov_dense(traj, SCPP, K=None, S0=None, Sth=None, disturb=None, Q=1.0, R=1.0, Qf=1.0, dt_min=0.1, store_dense=True, **opts):
    """lincov_disturbed() with the obstacle margins at the dense samples between the knots (gusto_lincov_dense; no counterpart in
    the reference): the samples of interpolate_traj / simulate() with the roll-out of tvlqr(traj, SCPP, Q, R, Qf, dt_min), the
    position covariance carried inside every hold interval by the exact derivative of the RK4 substeps.  Returns
    lincov_disturbed()'s report of the knot pass with nfull, min_z_dense, dense_sample, dense_pair and -- with store_dense --
    z_dense, pair_dense [nfull] and Spos [nfull, WS, WS]."""
    bs = _verify_handle(traj, SCPP)
    try:
        bs.tvlqr(dict(Q=Q, R=R, Qf=Qf, dt_min=dt_min, nstep_cap=max(64, int(np.ceil(traj.dt / dt_min)))))
        one = lambda a: None if a is None else np.asarray(a, float)[None]
        dense = bs.lincov_dense(opts, disturb, K=one(K), S0=one(S0), Sth=one(Sth), store_dense=int(bool(store_dense)))
        r = bs.get_lincov()
        r["Cd"], Sxt = bs.get_lincov_plant()
        if Sxt is not None:
            r["Sxt"] = Sxt
        r.update(dense)
    finally:
        bs.close()
    return {k: v[0] for k, v in r.items()}


def shard_bounds(B, world_size, rank):
    """Contiguous block of ceil(B/G) problems per rank; the tail rank may get fewer."""
    per = -(-B // world_size)
    lo = min(B, rank * per)
    return lo, min(B, lo + per)


def solve_SCP_batch(TOSs, TOPs, solve_method=None, init_method=init_traj_straightline, solver="hip", max_iter=30,
                    force=False, device=0, devices=None, decomposition=0, verify=False, tvlqr=None, simulate=None, disturb=None):
    """All TOPs must share model and N (each may bring its own environment); one gusto_solve covers the whole list.

    `verify` (GuSTO handles only): one gusto_verify per shard after its solve; every SCPS then carries `verify`, the dict of its
    problem's report (collision_free, first_knot, first_dist, min_dist_knots, dyn_defect_l1, min_dist_dense, min_dense_sample,
    max_gap).  A dict of gusto_verify_opts fields instead of True sets them.  Without it the solutions are what they were.

    `tvlqr` (GuSTO handles only): a dict of gusto_tvlqr_opts fields (Q, R, Qf, dt_min, nstep, nstep_cap, store_P; {} = the
    defaults) -- one gusto_tvlqr per shard after its solve; every SCPS then carries `tvlqr`, its problem's K, P, AB, status and
    fail_knot.  Without it the solutions are what they were.

    `simulate` (requires `tvlqr`): a dict of gusto_simulate_opts fields ({} = the defaults) -- one gusto_simulate per shard after
    its gusto_tvlqr, with that shard's gains and first_problem = the shard's offset, so the generated perturbations are those of
    the unsharded batch; every SCPS then carries `simulate`, the dict of its problem's report.

    `disturb` (requires `simulate`): a dict of gusto_disturb_opts fields (plant_rel, dw; {} = zeros) -- the roll-outs of every
    shard are those of gusto_simulate_disturbed, and the report carries `plant`, the plant scalars of the problem's samples.

    `decomposition` (gusto_set_decomposition; GuSTO handles only): 0 = the library's choice by batch size -- for the 12/13-state
    models two or four wavefronts per problem while the batch leaves SIMDs idle --, 1 one wave per problem, 3 / 4 two / four.

    `devices` = list of GPU ordinals: the problems are sharded in contiguous blocks (shard_bounds) over
    one handle per entry, every shard is enqueued with gusto_solve_async and the shards run concurrently -- the
    single-process form of the multi-GPU path (an ordinal may repeat: two shards on one GPU overlap like two batches)."""
    if solve_method not in (None, solve_gusto_hip, solve_trajopt_hip):
        raise NotImplementedError("solve_SCP_batch! runs the batched kernels: solve_method must be solve_gusto_hip or solve_trajopt_hip")
    trajopt = solve_method is solve_trajopt_hip
    if verify and trajopt:
        raise NotImplementedError("solve_SCP_batch!: verify is not available for TrajOpt handles")
    if tvlqr is not None and trajopt:
        raise NotImplementedError("solve_SCP_batch!: tvlqr is not available for TrajOpt handles")
    if simulate is not None and tvlqr is None:
        raise ValueError("solve_SCP_batch!: simulate needs the gains: pass tvlqr= as well")
    if disturb is not None and simulate is None:
        raise ValueError("solve_SCP_batch!: disturb belongs to the roll-outs: pass simulate= as well")
    if len(TOSs) != len(TOPs) or not TOPs:
        raise ValueError("solve_SCP_batch!: need as many solutions as problems, at least one")
    TOP0 = TOPs[0]
    model, N = TOP0.PD.model, TOP0.N
    n = model.x_dim
    B = len(TOPs)
    for t in TOPs[1:]:      # one gusto_handle = one model, one horizon, one Workspace
        if type(t.PD.model) is not type(model) or t.N != N:
            raise ValueError("solve_SCP_batch!: all problems must share the model type and N")
    # every ProblemDefinition owns its env (types.jl:32-39): a batch whose environments differ goes through
    # gusto_set_env_batch (one Workspace per problem), a batch that shares one through gusto_set_env
    same_env = all(np.array_equal(t.PD.env.boxes, TOP0.PD.env.boxes) and np.array_equal(t.PD.env.spheres, TOP0.PD.env.spheres)
                   for t in TOPs[1:])
    devs = list(devices) if devices else [device]
    sp, mp = _capi.default_params(model.model_id)
    x0 = np.stack([t.PD.x_init for t in TOPs])
    bounds = [_goal_bounds(t.PD.goal_set, n, t.tf_guess) for t in TOPs]
    lo, hi = np.stack([b[0] for b in bounds]), np.stack([b[1] for b in bounds])
    tf = np.array([t.tf_guess for t in TOPs])
    # every problem owns its initial trajectory (a Trajectory passed for all of them is copied, never aliased)
    inits = [init_method(t) if callable(init_method) else Trajectory(init_method.X.copy(), init_method.U.copy(), init_method.Tf)
             for t in TOPs]
    X0 = np.stack([t.X.T for t in inits])
    U0 = np.stack([t.U.T for t in inits])
    shards = []
    for r, dv in enumerate(devs):
        b0, b1 = shard_bounds(B, len(devs), r)
        if b1 <= b0:
            continue
        if trajopt:     # the second algorithm behind the seam (scp_trajopt.jl:33): one gusto_solve_trajopt per shard
            tp = _capi.default_trajopt_params(model.model_id)
            total = tp.max_penalty_iteration * tp.max_convex_iteration * tp.max_trust_iteration
            bs = _capi.TrajOptSolver(model.model_id, N, b1 - b0, hist_cap=2 * total + 16, device=dv, boxes=TOP0.PD.env.boxes,
                                     spheres=TOP0.PD.env.spheres, model_params=mp, trajopt_params=tp)
        else:
            bs = BatchSolver(model.model_id, N, b1 - b0, hist_cap=_hist_cap(max_iter), device=dv,
                             boxes=TOP0.PD.env.boxes, spheres=TOP0.PD.env.spheres, scp_params=sp, model_params=mp)
            if decomposition:
                bs.set_decomposition(decomposition)
        if not same_env:
            bs.set_env_batch([t.PD.env.boxes for t in TOPs[b0:b1]], [t.PD.env.spheres for t in TOPs[b0:b1]])
        bs.set_problems(x0[b0:b1], lo[b0:b1], hi[b0:b1], tf[b0:b1], X0[b0:b1], U0[b0:b1])
        if trajopt:
            bs.solve_async(max_iter)    # gusto_solve_trajopt_async: the shards of a TrajOpt batch run side by side too
        else:
            bs.solve_async(max_iter, force)
        shards.append((b0, b1, bs))
    out = [None] * B
    gathered = None
    if len(shards) > 1:
        # the final gather of the multi-GPU path below the host language: every shard to the first handle's GPU by one
        # direct peer copy over xGMI (gusto_gather_peer; it completes each shard's solve first), then ONE copy to the host
        gathered = shards[0][2].gather_peer([bs for _, _, bs in shards])
    for b0, b1, bs in shards:
        bs.wait()
        snap = _fetch(bs, None if gathered is None else (gathered[0][b0:b1], gathered[1][b0:b1]))
        per = bs.last_solve_ms() * 1e-3 / (b1 - b0)
        rep = bs.verify(**(verify if isinstance(verify, dict) else {})) if verify else None
        lq = bs.tvlqr(tvlqr) if tvlqr is not None else None
        sim = None
        if simulate is not None:
            so = dict(simulate, first_problem=simulate.get("first_problem", 0) + b0)
            sim = bs.simulate(so) if disturb is None else dict(bs.simulate_disturbed(so, disturb), plant=bs.get_simulate_plant())
        for b in range(b0, b1):
            SCPP = SCPProblem(TOPs[b])
            SCPS = SCPSolution(SCPP, inits[b])
            (_fill_trajopt_solution if trajopt else _fill_solution)(SCPS, SCPP, snap, b - b0, per)
            if rep is not None:
                SCPS.verify = {k: v[b - b0].item() for k, v in rep.items()}
            if lq is not None:
                SCPS.tvlqr = _capi.TvlqrResult(lq.K[b - b0], lq.P[b - b0], lq.AB[b - b0], int(lq.status[b - b0]),
                                               int(lq.fail_knot[b - b0]))
            if sim is not None:
                SCPS.simulate = {k: v[b - b0] for k, v in sim.items()}
            TOSs[b].traj, TOSs[b].SCPS = SCPS.traj, SCPS
            out[b] = SCPS
    return out


def default_fan(model_id):
    """The lateral detours of a multi-start solve, in metres, start 0 the straight line: 0, +-0.5, +-1 across the direction of
    travel in the plane; +-0.5 along each of the two axes across it in space."""
    if _capi.WS_DIM[model_id] == 2:
        return np.array([(0.0, 0.0), (0.5, 0.0), (-0.5, 0.0), (1.0, 0.0), (-1.0, 0.0)])
    return np.array([(0.0, 0.0), (0.5, 0.0), (-0.5, 0.0), (0.0, 0.5), (0.0, -0.5)])


class _QueryBatch:
    """What the query drivers share (solve_SCP_multistart_batch, solve_SCP_min_time_batch, solve_SCP_trajlib_batch,
    solve_SCP_roadmap_batch): every TOP is one planning query, all of one model and N, each with its own environment or all with
    the same.  The checks (in the driver's name `who`), the stacked inputs x0, lo, hi [Q, n] and tf [Q], the BatchSolver, the
    environment of a subset of the queries, the filling of a query's solution and report, and the fanned launches of the queries
    that are left without a winner.  out[q] is the driver's report of query q."""

    def __init__(self, who, TOSs, TOPs, early=None):
        """early: the text of a refusal of the driver's own that comes before the model check (None: there is none)"""
        if len(TOSs) != len(TOPs) or not TOPs:
            raise ValueError(f"{who}!: need as many solutions as problems, at least one")
        if early is not None:
            raise ValueError(f"{who}!: {early}")
        TOP0 = TOPs[0]
        self.TOSs, self.TOPs, self.model, self.N, self.Q = TOSs, TOPs, TOP0.PD.model, TOP0.N, len(TOPs)
        for t in TOPs[1:]:
            if type(t.PD.model) is not type(self.model) or t.N != self.N:
                raise ValueError(f"{who}!: all problems must share the model type and N")
        self.same_env = all(np.array_equal(t.PD.env.boxes, TOP0.PD.env.boxes) and np.array_equal(t.PD.env.spheres, TOP0.PD.env.spheres)
                            for t in TOPs[1:])
        self.x0 = np.stack([t.PD.x_init for t in TOPs])
        bounds = [_goal_bounds(t.PD.goal_set, self.model.x_dim, t.tf_guess) for t in TOPs]
        self.lo, self.hi = np.stack([b[0] for b in bounds]), np.stack([b[1] for b in bounds])
        self.tf = np.array([t.tf_guess for t in TOPs])
        self.out = [None] * self.Q

    def solver(self, cap, max_iter, force, device):
        """the BatchSolver of the call, for cap problems, on the first query's environment"""
        sp, mp = _capi.default_params(self.model.model_id)
        env = self.TOPs[0].PD.env
        self.cap, self.max_iter, self.force = cap, max_iter, force
        self.bs = BatchSolver(self.model.model_id, self.N, cap, hist_cap=_hist_cap(max_iter), device=device, boxes=env.boxes,
                              spheres=env.spheres, scp_params=sp, model_params=mp)
        return self.bs

    def env(self, qs=None):
        """boxes / spheres of the queries qs (None: all), one set per query, for a set_problems_* call; {} when all share one"""
        if self.same_env:
            return {}
        tops = self.TOPs if qs is None else [self.TOPs[q] for q in qs]
        return dict(boxes=[t.PD.env.boxes for t in tops], spheres=[t.PD.env.spheres for t in tops])

    def take(self, q, snap, b, per, solved_tf=None, **report):
        """problem b of the snapshot is query q's answer: TOSs[q] and out[q] = report + SCPS.  tf: the final time it was solved
        with (solved_tf) when that is not the query's tf_guess"""
        TOP = self.TOPs[q]
        SCPP = SCPProblem(TOP)
        if solved_tf is None:
            init = init_traj_straightline(TOP)
        else:
            SCPP.tf_guess = float(solved_tf)
            init = Trajectory(np.zeros((self.model.x_dim, self.N)), np.zeros((self.model.u_dim, self.N)), solved_tf)
        SCPS = SCPSolution(SCPP, init)
        _fill_solution(SCPS, SCPP, snap, b, per)
        self.TOSs[q].traj, self.TOSs[q].SCPS = SCPS.traj, SCPS
        self.out[q] = dict(report, SCPS=SCPS)

    def solved(self, K, nq):
        """solve what is set, nq queries of K starts, and select: (best, snapshot, seconds per query)"""
        self.bs.solve(self.max_iter, self.force)
        best = self.bs.select_best(K)
        return best, _fetch(self.bs), self.bs.last_solve_ms() * 1e-3 / nq

    def fanned(self, qs, fan):
        """the queries qs through one launch of the multi-start fan"""
        qs = np.asarray(qs)
        self.bs.set_problems_multistart(self.x0[qs], self.lo[qs], self.hi[qs], self.tf[qs], fan, **self.env(qs))
        return self.solved(len(fan), len(qs))

    def chunks(self, again, K):
        """the queries `again` in as many pieces as K starts each need on this handle"""
        step = self.cap // K
        return [again[c:c + step] for c in range(0, len(again), step)]


def _fallback_fan(model_id, fallback_fan):
    """fallback_fan of a driver: None / False (none), True (default_fan) or the offsets [Kf, 2]"""
    if fallback_fan is None or fallback_fan is False:
        return None
    return default_fan(model_id) if fallback_fan is True else np.asarray(fallback_fan, float).reshape(-1, 2)


def solve_SCP_multistart_batch(TOSs, TOPs, fan=None, policy="all", solver="hip", max_iter=30, force=False, device=0):
    """Every TOP is one planning QUERY, started from a fan of K initial trajectories (gusto_set_problems_multistart: the straight
    line bent sideways by fan[j] = (a2, a3) metres; None = default_fan) and answered with the best start that is converged and
    successful (gusto_select_best on the last true cost).  All TOPs share model and N; each may bring its own environment.

    policy="all": one launch of len(TOPs) K problems.  policy="retry": a plain straight-line solve of the queries first, then
    the fan for the queries that are not successful only, on the same handle (sized for the larger batch; a retry that does not
    fit runs in several launches); a query solved in the first pass keeps that result untouched.

    Returns one dict per query: `winner` (the start's index in the fan, -1 when no start qualified), `cost` (its last J_true,
    +inf likewise) and `SCPS`, the filled SCPSolution of the winner -- without one, of the straight line's solve.  TOSs[q].traj
    and TOSs[q].SCPS are set as by solve_SCP_batch."""
    if policy not in ("all", "retry"):
        raise ValueError("solve_SCP_multistart_batch!: policy is 'all' or 'retry'")
    qb = _QueryBatch("solve_SCP_multistart_batch", TOSs, TOPs)
    Q, x0, lo, hi, tf = qb.Q, qb.x0, qb.lo, qb.hi, qb.tf
    fan = default_fan(qb.model.model_id) if fan is None else np.asarray(fan, float).reshape(-1, 2)
    K = len(fan)
    bs = qb.solver(Q * K if policy == "all" else max(Q, K), max_iter, force, device)

    def fanned(qs, keep_loser):
        """the queries qs through one fanned launch; a query without a winner is taken from start 0 when keep_loser"""
        best, snap, per = qb.fanned(qs, fan)
        for i, q in enumerate(qs):
            if best["winner"][i] >= 0:
                qb.take(q, snap, best["winner_problem"][i], per, winner=int(best["winner"][i]), cost=float(best["best_score"][i]))
            elif keep_loser:
                qb.take(q, snap, i * K, per, winner=-1, cost=float(np.inf))

    try:
        if policy == "all":
            fanned(np.arange(Q), True)
        else:
            if not qb.same_env:
                bs.set_env_batch([t.PD.env.boxes for t in TOPs], [t.PD.env.spheres for t in TOPs])
            bs.set_problems(x0, lo, hi, tf)
            bs.solve(max_iter, force)
            snap = _fetch(bs)
            per = bs.last_solve_ms() * 1e-3 / Q
            ok = snap["st"]["converged"] & snap["st"]["successful"]
            for q in range(Q):
                last = snap["h"]["J_true"][q, snap["h"]["nJ"][q] - 1]
                qb.take(q, snap, q, per, winner=0 if ok[q] else -1, cost=float(last if ok[q] else np.inf))
            for qs in qb.chunks(np.flatnonzero(~ok), K):
                fanned(qs, False)
    finally:
        bs.close()
    return qb.out


def solve_SCP_min_time_batch(TOSs, TOPs, tf_lo, tf_hi, K=8, rounds=3, rtol=0.01, seed="incumbent", eligible=None, solver="hip",
                             max_iter=30, force=False, device=0):
    """Every TOP is one planning QUERY, answered with the shortest final time in [tf_lo, tf_hi] (scalars or one per query) whose
    solve is eligible: a K-section search over solves (gusto_tfsearch_begin / gusto_tfsearch_update), K candidate final times per
    query and round, at most `rounds` rounds, a query done once hi - lo <= rtol hi.  TOP.tf_guess is not read but for the goals'
    times; TrajectoryOptimizationProblem(fixed_final_time=False) stays as inert as in the reference -- the search is this call.
    All TOPs share model and N; each may bring its own environment.

    seed: "incumbent" starts the later candidates from the query's retimed incumbent, "line" from the straight line.  eligible:
    None (converged and successful) or a callable bs -> boolean mask [B] over the BatchSolver's problems after a round's solve --
    "that also passes verify", "with min_z_obs >= kappa", "with J <= budget" are the same call.

    Returns one dict per query: `tf` (NaN without an incumbent), `lo`, `hi`, `status` (bits _capi.TFSEARCH_NONE / DONE / FLOOR /
    NONMONOTONE), `J` (the incumbent's last J_true) and `SCPS`, the filled SCPSolution of the solve that found the incumbent -- for
    a NONE query of the straight line's solve at tf_hi.  TOSs[q].traj is the incumbent with Tf = tf, TOSs[q].SCPS that SCPS."""
    qb = _QueryBatch("solve_SCP_min_time_batch", TOSs, TOPs, early="need at least one round" if rounds < 1 else None)
    Q, K = qb.Q, int(K)
    bs = qb.solver(Q * K, max_iter, force, device)
    out = qb.out

    def take(q, snap, b, per, tf, info):
        qb.take(q, snap, b, per, solved_tf=tf, tf=float(info["tf_best"][q]), lo=float(info["lo"][q]), hi=float(info["hi"][q]),
                status=int(info["status"][q]), J=float(info["J_best"][q]))

    try:
        bs.tfsearch_begin(qb.x0, qb.lo, qb.hi, tf_lo, tf_hi, K=K, rtol=rtol, seed=seed, **qb.env())
        cand = bs.tfsearch_info()["cand"]
        for r in range(rounds):
            bs.solve(max_iter, force)
            snap = _fetch(bs)
            per = bs.last_solve_ms() * 1e-3 / Q
            ok = np.asarray(eligible(bs)).astype(bool) if eligible is not None else snap["st"]["converged"] & snap["st"]["successful"]
            searching = bs.tfsearch_update(ok if eligible is not None else None)
            info = bs.tfsearch_info()
            for q in range(Q):
                if info["round_found"][q] == r:      # the incumbent of this round: the lowest candidate at tf_best that counts
                    j = int(np.flatnonzero(ok[q * K:(q + 1) * K] & (cand[q] == info["tf_best"][q]))[0])
                    take(q, snap, q * K + j, per, cand[q, j], info)
                elif out[q] is None and info["round_found"][q] < 0:
                    take(q, snap, q * K + K - 1, per, cand[q, K - 1], info)   # (round 0, no incumbent: the line at tf_hi)
                else:
                    out[q].update(lo=float(info["lo"][q]), hi=float(info["hi"][q]), status=int(info["status"][q]))
            cand = info["cand"]
            if searching == 0:
                break
    finally:
        bs.close()
    return out


def _timeline_of(TOP):
    """The goal timeline of a problem: every goal of its GoalSet with 0 < t_guess <= tf_guess, grouped by time into a list of
    (T, lo, hi) in the order of time, lo / hi by the rules of _goal_bounds at that time (two goals at one time are one entry; a
    coordinate no goal of that time names is +-inf).  Goals behind tf_guess are left out, as the plain solve leaves out all but
    those at tf_guess.  The last entry must be at tf_guess itself: a final time without a goal is an error."""
    gs, n, tf = TOP.PD.goal_set, TOP.PD.model.x_dim, TOP.tf_guess
    times = sorted({g.t_guess for g in gs.goals if 0 < g.t_guess <= tf})
    if not times or times[-1] != tf:
        raise ValueError("_timeline_of: no goal at the final time tf_guess")
    return [(T,) + _goal_bounds(gs, n, T) for T in times]


def solve_SCP_timeline_batch(TOSs, TOPs, mode="auto", verify=False, solver="hip", max_iter=30, force=False, device=0):
    """Every TOP is one planning QUERY whose GoalSet is flown as a timeline (gusto_legs_begin / gusto_legs_advance): every goal
    time in (0, tf_guess] ends a LEG, an ordinary GuSTO problem from the previous junction to that goal in the time between the
    two, and the solved legs are joined on the device.  solve_SCP and the other drivers ignore the goals before tf_guess, as the
    reference does; this call is the one that flies them.  All TOPs share model and N; each may bring its own environment and its
    own number of goals.

    mode "sequential": one leg per query and round, the state a leg arrives in is the next leg's start (goals that leave a
    junction partly free); "parallel": every leg of every query in one launch (every goal before the last must pin every
    coordinate); "auto": parallel where allowed.  verify=True: BatchSolver.verify runs per round and a leg counts only if it is
    also collision-free.

    Returns one dict per query, also TOSs[q].timeline: status (_capi.LEGS_DONE / LEGS_FAILED), failed_leg (-1: none), n_done,
    J_total, T [L_q] and per leg iterations, converged, successful, stop_reason, J, gap, arrive [L_q].  TOSs[q].traj is the joined
    trajectory, X [n, L_q (N - 1) + 1] and U with the knot times in traj.t and Tf the last goal's time (rows behind a failed leg
    are zeros); TOSs[q].SCPS the list of the filled SCPSolutions of the legs that were flown."""
    qb = _QueryBatch("solve_SCP_timeline_batch", TOSs, TOPs)
    Q, N, n = qb.Q, qb.N, qb.model.x_dim
    lines = [_timeline_of(t) for t in TOPs]
    nl = np.array([len(tl) for tl in lines], np.int32)
    L = int(nl.max())
    T, lo, hi = np.zeros((Q, L)), np.full((Q, L, n), -np.inf), np.full((Q, L, n), np.inf)
    for q, tl in enumerate(lines):
        for l, (t, a, b) in enumerate(tl):
            T[q, l], lo[q, l], hi[q, l] = t, a, b
    mode = _capi.legs_mode(lo, hi, nl, mode)
    K = L if mode == "parallel" else 1
    bs = qb.solver(Q * K, max_iter, force, device)
    scps = [[] for _ in range(Q)]
    try:
        bs.legs_begin(qb.x0, lo, hi, T, n_legs=nl, mode=mode, **qb.env())
        flying = np.ones(Q, bool)
        rnd = 0
        while flying.any():
            bs.solve(max_iter, force)
            snap = _fetch(bs)
            per = bs.last_solve_ms() * 1e-3 / (int(flying.sum()) if K == 1 else int(nl.sum()))   # (seconds per leg solved)
            ok = None
            if verify:
                ok = snap["st"]["converged"] & snap["st"]["successful"] & (bs.verify()["collision_free"] != 0)
            for q in np.flatnonzero(flying):
                for l in (range(nl[q]) if K > 1 else [rnd]):
                    SCPP = SCPProblem(TOPs[q])
                    SCPP.tf_guess = float(T[q, l] - (T[q, l - 1] if l else 0.0))
                    SCPS = SCPSolution(SCPP, Trajectory(np.zeros((n, N)), np.zeros((qb.model.u_dim, N)), SCPP.tf_guess))
                    _fill_solution(SCPS, SCPP, snap, q * K + (l if K > 1 else 0), per)
                    scps[q].append(SCPS)
            bs.legs_advance(ok)
            info = bs.legs_info()
            flying = info["status"] == _capi.LEGS_FLYING
            rnd += 1
        for q in range(Q):
            Lq, Nq = int(nl[q]), int(nl[q]) * (N - 1) + 1
            traj = Trajectory(info["X"][q, :Nq].T.copy(), info["U"][q, :Nq].T.copy(), T[q, Lq - 1])
            traj.t = info["t"][q, :Nq].copy()
            rep = {k: (int if k != "J_total" else float)(info[k][q]) for k in ("status", "failed_leg", "n_done", "J_total")}
            rep.update({k: info[k][q, :Lq].copy() for k in ("iterations", "converged", "successful", "stop_reason", "J", "gap", "arrive")})
            rep["T"] = T[q, :Lq].copy()
            TOSs[q].traj, TOSs[q].SCPS, TOSs[q].timeline = traj, scps[q], rep
            qb.out[q] = rep
    finally:
        bs.close()
    return qb.out


def fleet_park_spheres(start, goal, R, radius, margin, comp_off, n_base=None):
    """The parking keep-outs of fleets of R consecutive robots: robot b plans around one sphere at the start and one at the goal
    centre of every other robot of its fleet.  start, goal [B, WS]; comp_off [n_comp, >= WS] the robot's component offsets;
    n_base [B] the components robot b's base set has already (None: none).

    Sphere radius: radius + margin + 2 omax, omax = max_c |comp_off[c] - comp_off[0]| over the first WS entries: clearing the
    sphere with component 0 keeps every component pair `margin` apart from a robot parked there.  A sphere that would contain
    the robot's own start or goal is left out and listed.  More than 64 components for one robot: ValueError.

    Returns (spheres, skipped): spheres[b] is [k_b, 4] rows (x, y, z, r), skipped a list of (robot, other, "start" / "goal")."""
    start, goal = np.asarray(start, float), np.asarray(goal, float)
    B, ws = start.shape
    if R < 1 or B % R:
        raise ValueError("fleet_park_spheres!: R must divide the number of robots")
    off = np.asarray(comp_off, float)[:, :ws]
    omax = float(np.max(np.sqrt(np.sum((off - off[0]) ** 2, axis=1))))
    rad = radius + margin + 2 * omax
    spheres, skipped = [], []
    for b in range(B):
        rows = []
        for o in range(b - b % R, b - b % R + R):
            for what, c in (("start", start[o]), ("goal", goal[o])):
                if o == b:
                    continue
                if min(np.linalg.norm(start[b] - c), np.linalg.norm(goal[b] - c)) < rad:
                    skipped.append((b, o, what))
                    continue
                rows.append(list(c) + [0.0] * (3 - ws) + [rad])
        if (0 if n_base is None else int(n_base[b])) + len(rows) > 64:
            raise ValueError(f"fleet_park_spheres!: robot {b} would have more than 64 keep-out components")
        spheres.append(np.asarray(rows, float).reshape(-1, 4))
    return spheres, skipped


def solve_SCP_fleet_batch(TOSs, TOPs, R, margin=None, order=None, park_keepouts=True, fleet_opts=None, solver="hip", max_iter=30,
                          force=False, device=0):
    """Every TOP is one ROBOT, R consecutive TOPs one fleet that shares a workspace: solve, interpolate, gusto_fleet_schedule,
    gusto_fleet_separation.  Prioritised planning on fixed paths: every robot keeps its solved path, a robot of lower priority
    (order [F, R], None: index order) departs later, by the smallest candidate delay that keeps it `margin` (None: the model's
    clearance) away from every robot placed before it.  Robots hold at their start before they depart and stay parked at their
    goal: whether they can is the caller's business.  All TOPs share model and N; each may bring its own environment.

    park_keepouts: every robot plans around a sphere at the start and at the goal centre of every other robot of its fleet
    (fleet_park_spheres), on top of its own environment, so that a parked robot is never flown through.

    fleet_opts: a dict of gusto_fleet_opts fields (dt_clock, n_delays, delay_stride, clock_cap, components).

    Every TOS is filled as by solve_SCP_batch, plus TOS.fleet_status (_capi.FLEET_*), TOS.delay and the time grid TOS.traj.t =
    delay + k dt (export.write(..., t=) takes it).  Returns the fleet report of BatchSolver.fleet_info() as a dict, with
    `park_skipped` (fleet_park_spheres), `robots`, one dict per robot (status, delay, blocker, min_sep, SCPS), and `dense`, the
    (nfull [B], positions [B, nfull_max, WS]) of gusto_interpolate that the stage read."""
    who = "solve_SCP_fleet_batch"
    qb = _QueryBatch(who, TOSs, TOPs, early=None if R >= 1 and len(TOPs) % max(R, 1) == 0 else "R must divide the number of problems")
    Q, N, mid = qb.Q, qb.N, qb.model.model_id
    _, mp = _capi.default_params(mid)
    margin = float(mp.clearance if margin is None else margin)
    ws = _capi.WS_DIM[mid]
    skipped = []
    boxes = [t.PD.env.boxes for t in TOPs]
    spheres = [np.asarray(t.PD.env.spheres, float).reshape(-1, 4) for t in TOPs]
    if park_keepouts:
        centre = np.where(np.isfinite(qb.lo) & np.isfinite(qb.hi), 0.5 * (qb.lo + qb.hi), 0.0)
        off = np.array([list(mp.comp_off[c]) for c in range(max(1, mp.n_robot_comp))])
        park, skipped = fleet_park_spheres(qb.x0[:, :ws], centre[:, :ws], R, mp.radius, margin, off,
                                           [len(b) + len(s) for b, s in zip(boxes, spheres)])
        spheres = [np.concatenate([s, p], axis=0) for s, p in zip(spheres, park)]
    bs = qb.solver(Q, max_iter, force, device)
    try:
        if park_keepouts or not qb.same_env:
            bs.set_env_batch(boxes, spheres)
        bs.set_problems(qb.x0, qb.lo, qb.hi, qb.tf)
        bs.solve(max_iter, force)
        snap = _fetch(bs)
        per = bs.last_solve_ms() * 1e-3 / Q
        nfull, Xfull, _ = bs.interpolate()
        kw = dict(fleet_opts or {}, margin=margin)
        bs.fleet_schedule(R, order=order, **kw)
        rep = bs.fleet_separation(R, **kw)
        for q in range(Q):
            qb.take(q, snap, q, per, status=int(rep["status"][q]), delay=float(rep["delay"][q]), blocker=int(rep["blocker"][q]),
                    min_sep=float(rep["min_sep"][q]))
            TOS = TOSs[q]
            TOS.fleet_status, TOS.delay = int(rep["status"][q]), float(rep["delay"][q])
            TOS.traj.t = TOS.delay + np.arange(N) * (qb.tf[q] / (N - 1))
    finally:
        bs.close()
    rep["park_skipped"], rep["robots"] = skipped, qb.out
    rep["dense"] = (nfull, Xfull[:, :, :ws].copy())   # the dense positions the stage read
    return rep


class TrajLib(_capi.TrajLib):
    """A device-resident library of solved trajectories (gusto_trajlib): TrajLib(model_id, N, cap, device=0, w_init=None,
    w_goal=None, w_tf=None).  add_from(solver, mask=None, tag=None) appends the converged and successful (or the masked) problems
    of a BatchSolver device to device, save(path) / TrajLib.load(path, cap=None, device=0) move a library through an .npz with its
    weights, len() is its fill; solve_SCP_trajlib_batch seeds queries from it."""


def solve_SCP_trajlib_batch(TOSs, TOPs, lib, K=1, fallback_fan=None, learn=False, solver="hip", max_iter=30, force=False, device=0):
    """Every TOP is one planning QUERY, seeded from its K nearest entries of the TrajLib `lib` (gusto_set_problems_trajlib: the
    entry's trajectory retargeted to the query's end points; a start without a neighbour is the straight line), solved in one
    launch of len(TOPs) K problems and answered with the best start that is converged and successful (gusto_select_best on the
    last true cost).  All TOPs share the library's model and N; each may bring its own environment.

    fallback_fan: the queries without a winner go through the multi-start path afterwards (gusto_set_problems_multistart with this
    fan [Kf, 2]; True = default_fan), on the same handle.  learn: the winners are appended to the library, device to device, so a
    later batch is seeded from them too (a full library refuses: GustoError, the solutions of this batch are filled by then).

    Returns one dict per query: `winner` (the start's index, -1 when no start qualified), `cost` (its last J_true, +inf
    likewise), `source` ("library", "fan", or None without a winner), `entry` (the library entry the winning start was seeded
    from; -1 for a straight line or a fan start) and `SCPS`, the filled SCPSolution of the winner -- without one, of start 0.
    TOSs[q].traj and TOSs[q].SCPS are set as by solve_SCP_batch."""
    qb = _QueryBatch("solve_SCP_trajlib_batch", TOSs, TOPs)
    Q, K = qb.Q, int(K)
    if lib.model != qb.model.model_id or lib.N != qb.N:
        raise ValueError("solve_SCP_trajlib_batch!: the library belongs to another model or N")
    fan = _fallback_fan(qb.model.model_id, fallback_fan)
    bs = qb.solver(Q * K if fan is None else max(Q * K, len(fan)), max_iter, force, lib.device)

    def finish(qs, Ks, source, entries, keep_loser):
        """solve what is set, select, fill the queries qs; with learn the winners join the library.  Returns the losers"""
        best, snap, per = qb.solved(Ks, len(qs))
        lost = []
        for i, q in enumerate(qs):
            w = best["winner"][i]
            if w >= 0:
                qb.take(q, snap, best["winner_problem"][i], per, winner=int(w), cost=float(best["best_score"][i]), source=source,
                        entry=int(-1 if entries is None else entries[i, w]))
            else:
                lost.append(q)
                if keep_loser:
                    qb.take(q, snap, i * Ks, per, winner=-1, cost=float(np.inf), source=None, entry=-1)
        if learn and (best["winner"] >= 0).any():
            mask = np.zeros(bs.B, bool)
            mask[best["winner_problem"][best["winner"] >= 0]] = True
            lib.add_from(bs, mask)
        return np.array(lost, dtype=int)

    try:
        bs.set_problems_trajlib(lib, qb.x0, qb.lo, qb.hi, qb.tf, K, **qb.env())
        again = finish(np.arange(Q), K, "library", bs.trajlib_seeds()["entry"], True)
        if fan is not None:
            for qs in qb.chunks(again, len(fan)):
                bs.set_problems_multistart(qb.x0[qs], qb.lo[qs], qb.hi[qs], qb.tf[qs], fan, **qb.env(qs))
                finish(qs, len(fan), "fan", None, False)
    finally:
        bs.close()
    return qb.out


def solve_SCP_roadmap_batch(TOSs, TOPs, K=1, fallback_fan=None, straight_first=False, roadmap_opts=None, solver="hip", max_iter=30,
                            force=False, device=0):
    """Every TOP is one planning QUERY, seeded from a shortest collision-free polyline through the corners of its inflated
    keep-out set (gusto_set_problems_roadmap: K alternates of other homotopy classes; a query with an unblocked line, or without
    a path, is the straight line), solved in one launch of len(TOPs) K problems and answered with the best alternate that is
    converged and successful (gusto_select_best on the last true cost).  All TOPs share model and N; each may bring its own
    environment.  straight_first: alternate 0 is the straight line and the paths follow.  roadmap_opts: a dict of inflate / pad
    over the model's defaults.

    fallback_fan: the queries without a winner go through the multi-start path afterwards (gusto_set_problems_multistart with this
    fan [Kf, 2]; True = default_fan), on the same handle -- the retry of solve_SCP_multistart_batch(policy="retry").

    Returns one dict per query: `winner` (the alternate's index, -1 when none qualified), `cost` (its last J_true, +inf
    likewise), `source` ("roadmap", "fan", or None without a winner), `status` (the ROADMAP_STATUS code of the winning alternate's
    seed, of alternate 0 without a roadmap winner) and `SCPS`, the filled SCPSolution of the winner -- without one, of alternate 0.
    `roadmap_ms` is the GPU time of the seeding call.  TOSs[q].traj and TOSs[q].SCPS are set as by solve_SCP_batch."""
    qb = _QueryBatch("solve_SCP_roadmap_batch", TOSs, TOPs)
    Q, K, out = qb.Q, int(K), qb.out
    fan = _fallback_fan(qb.model.model_id, fallback_fan)
    bs = qb.solver(Q * K if fan is None else max(Q * K, len(fan)), max_iter, force, device)

    def take(q, snap, b, per, winner, cost, source, status, ms):
        qb.take(q, snap, b, per, winner=int(winner), cost=float(cost), source=source, status=int(status), roadmap_ms=float(ms))

    try:
        if not qb.same_env:   # one set per query, repeated K times: query q reads that of problem q K
            bs.set_env_batch([t.PD.env.boxes for t in TOPs for _ in range(K)], [t.PD.env.spheres for t in TOPs for _ in range(K)])
        opts = dict(roadmap_opts or {}, straight_first=int(bool(straight_first)))
        bs.set_problems_roadmap(qb.x0, qb.lo, qb.hi, qb.tf, K, **opts)
        info, ms = bs.roadmap_info(), bs.last_roadmap_ms()
        best, snap, per = qb.solved(K, Q)
        for q in range(Q):
            w = best["winner"][q]
            if w >= 0:
                take(q, snap, best["winner_problem"][q], per, w, best["best_score"][q], "roadmap", info["status"][q * K + w], ms)
            else:
                take(q, snap, q * K, per, -1, np.inf, None, info["status"][q * K], ms)
        if fan is not None:
            for qs in qb.chunks(np.flatnonzero(best["winner"] < 0), len(fan)):
                best, snap, per = qb.fanned(qs, fan)
                for i, q in enumerate(qs):
                    if best["winner"][i] >= 0:
                        take(q, snap, best["winner_problem"][i], per, best["winner"][i], best["best_score"][i], "fan", out[q]["status"], ms)
    finally:
        bs.close()
    return out


def _check_replan_tf(tf_new, who):
    """the reference's only row on the final time, Tf >= 0.1 (scp_gusto.jl:248-250), on tf' as TrajectoryOptimizationProblem
    checks it on tf_guess"""
    if tf_new is None:
        raise ValueError(who + ": the tf of the source problems is not known on the host (they were set from device pointers)")
    if (np.asarray(tf_new) < 0.1).any():
        bad = int(np.flatnonzero(np.asarray(tf_new) < 0.1)[0])
        raise ValueError(f"{who}: tf' = (1 - tau) tf of problem {bad} is {float(np.asarray(tf_new)[bad]):g}; the only row on Tf is Tf >= 0.1 "
                         "(scp_gusto.jl:248-250)")


def replan_batch(bs, tau, x_now, src=None, source="traj", goal_lo=None, goal_hi=None, mask=None, boxes=None, spheres=None):
    """Receding-horizon replanning on a BatchSolver (gusto_set_problems_replan): problem b restarts from the state x_now[b] with
    the time that is left, tf' = (1 - tau[b]) tf, seeded from its plan on `src` (None: bs itself) shifted by tau and bent to
    x_now; the arguments are those of BatchSolver.set_problems_replan.  tf' must respect the reference's Tf >= 0.1.  Returns
    replan_info()."""
    x_now = np.asarray(x_now, float).reshape(-1, bs.n)
    tau = np.broadcast_to(np.asarray(tau, float), (len(x_now),))
    _check_replan_tf(bs.replan_tf(tau, src, source), "replan_batch!")
    bs.set_problems_replan(tau, x_now, src=src, source=source, goal_lo=goal_lo, goal_hi=goal_hi, mask=mask, boxes=boxes, spheres=spheres)
    return bs.replan_info()


def solve_SCP_receding_batch(TOSs, TOPs, steps, knots_per_step, sim_opts=None, disturb=None, tvlqr_opts=None, max_iter=30, force=False,
                             device=0):
    """A receding-horizon loop on one handle.  Per step: gusto_solve, gusto_tvlqr, gusto_simulate_disturbed with store_knots = 1
    and two samples (sample 0 is the unperturbed one, so sample 1 is the flight), then gusto_set_problems_replan_knots with
    knot = knots_per_step and sample = 1: the next step plans from where the roll-out is after knots_per_step knots, to the same
    goals, in the time that is left.  All TOPs share model and N; each may bring its own environment.  sim_opts / disturb /
    tvlqr_opts: dicts of the fields of gusto_simulate_opts / gusto_disturb_opts / gusto_tvlqr_opts (n_samples and store_knots are
    set here).

    Returns one dict per step: iterations, converged, successful [B] and solve_ms of the step's solve; x_now [B, n], tau [B],
    seeded [B] and replan_ms of the replan that ends it (x_now is the x_init of the next step).  TOSs take the last plan."""
    who = "solve_SCP_receding_batch!"
    if len(TOSs) != len(TOPs) or not TOPs:
        raise ValueError(who + ": need as many solutions as problems, at least one")
    TOP0 = TOPs[0]
    model, N = TOP0.PD.model, TOP0.N
    n, B = model.x_dim, len(TOPs)
    for t in TOPs[1:]:
        if type(t.PD.model) is not type(model) or t.N != N:
            raise ValueError(who + ": all problems must share the model type and N")
    if steps < 1 or not 0 <= knots_per_step <= N - 2:
        raise ValueError(who + ": need steps >= 1 and 0 <= knots_per_step <= N - 2")
    same_env = all(np.array_equal(t.PD.env.boxes, TOP0.PD.env.boxes) and np.array_equal(t.PD.env.spheres, TOP0.PD.env.spheres)
                   for t in TOPs[1:])
    sp, mp = _capi.default_params(model.model_id)
    bounds = [_goal_bounds(t.PD.goal_set, n, t.tf_guess) for t in TOPs]
    sim = dict(sim_opts or {})
    sim.update(n_samples=2, store_knots=1)
    bs = BatchSolver(model.model_id, N, B, hist_cap=_hist_cap(max_iter), device=device, boxes=TOP0.PD.env.boxes,
                     spheres=TOP0.PD.env.spheres, scp_params=sp, model_params=mp)
    out = []
    try:
        if not same_env:
            bs.set_env_batch([t.PD.env.boxes for t in TOPs], [t.PD.env.spheres for t in TOPs])
        bs.set_problems(np.stack([t.PD.x_init for t in TOPs]), np.stack([b[0] for b in bounds]), np.stack([b[1] for b in bounds]),
                        np.array([t.tf_guess for t in TOPs]))
        for _ in range(steps):
            tf_now = bs._tf.copy()
            bs.solve(max_iter, force)
            snap = _fetch(bs)
            solve_ms = bs.last_solve_ms()
            bs.tvlqr(tvlqr_opts or {})
            bs.simulate_disturbed(sim, disturb)
            _check_replan_tf(bs.replan_tf(np.full(B, knots_per_step / (N - 1))), who)
            bs.set_problems_replan_knots(knots_per_step, 1)
            info = bs.replan_info()
            out.append(dict(iterations=snap["st"]["iterations"].copy(), converged=snap["st"]["converged"].copy(),
                            successful=snap["st"]["successful"].copy(), solve_ms=solve_ms, x_now=info["x_now"], tau=info["tau"],
                            seeded=info["seeded"], replan_ms=bs.last_replan_ms()))
        for q in range(B):
            SCPP = SCPProblem(TOPs[q])
            SCPS = SCPSolution(SCPP, init_traj_straightline(TOPs[q]))
            _fill_solution(SCPS, SCPP, snap, q, solve_ms * 1e-3 / B)
            SCPS.traj.Tf = float(tf_now[q])
            SCPS.traj.dt = SCPS.traj.Tf / (N - 1)
            TOSs[q].traj, TOSs[q].SCPS = SCPS.traj, SCPS
    finally:
        bs.close()
    return out


def solve_SCP_chance_batch(TOSs, TOPs, kappa=3.0, rounds=3, lincov_opts=None, tvlqr_opts=None, disturb=None, tighten_opts=None,
                           max_iter=30, force=False, device=0):
    """Plans that keep kappa standard deviations of closed-loop dispersion from every keep-out component, for every robot
    component, on one handle.  Solve; then per round: gusto_tvlqr and gusto_lincov (store_S = 1; gusto_lincov_disturbed with
    `disturb`) on the plans, gusto_tighten_env from the BASE keep-out sets for the answered problems still below kappa, and a
    re-solve of those from their own plan (gusto_set_problems_replan on the handle itself, tau = 0, x_now = x_init); the ones that
    pass loses go once more from the straight line.  A problem whose start or goal lies inside its own tightened set (blocked) is
    not re-solved, and one that loses both passes keeps its last answered plan and is left alone afterwards.  At the end the base
    set is restored and gusto_tvlqr, gusto_lincov and gusto_verify run on it.  All TOPs share model and N; each may bring its own
    environment.  lincov_opts / tvlqr_opts / disturb / tighten_opts: dicts of the fields of the C structs; kappa overrides
    tighten_opts' own.  Without actuator noise (du_white) or a plant dispersion the covariance decays to rounding noise along the
    horizon and a margin built on it means nothing: such options raise ValueError.

    Returns a dict: `answered` [B] (converged and successful, the problems that have a plan), `met_before` and `met` [B]
    (answered, min_z_obs >= kappa and collision-free on the base set, before the first round and at the end), `min_z_obs` and
    `collision_free` [B] of the final analysis, `env` (get_env() of the handle at the end: the base set), and `rounds`, one dict per round: `tried` [B] (re-solved), `min_z_base`,
    `max_margin`, `blocked` [B] of gusto_tighten_env (zeros for the problems it skipped), `lost` [B] (lost both passes),
    `second_pass` [B], `iterations` [B] of the re-solves, and tighten_ms / lincov_ms / solve_ms.  TOSs take the final plans."""
    who = "solve_SCP_chance_batch!"
    if len(TOSs) != len(TOPs) or not TOPs:
        raise ValueError(who + ": need as many solutions as problems, at least one")
    lo_ = dict(lincov_opts or {})
    white = np.asarray(lo_.get("du_white", 0.0), float)
    noisy = bool((white != 0).any())
    if disturb is not None:
        d = dict(disturb)
        noisy = noisy or bool((np.asarray(d.get("plant_rel", 0.0), float) != 0).any() or (np.asarray(d.get("dw", 0.0), float) != 0).any())
    if not noisy:
        raise ValueError(who + ": du_white is all zero and no plant dispersion is given: the covariance decays to rounding noise "
                         "along the horizon and a margin in its standard deviations means nothing")
    if not (kappa >= 0 and np.isfinite(kappa)) or rounds < 0:
        raise ValueError(who + ": need a finite kappa >= 0 and rounds >= 0")
    TOP0 = TOPs[0]
    model, N = TOP0.PD.model, TOP0.N
    n, B = model.x_dim, len(TOPs)
    for t in TOPs[1:]:
        if type(t.PD.model) is not type(model) or t.N != N:
            raise ValueError(who + ": all problems must share the model type and N")
    lo_["store_S"] = 1
    to_ = dict(tighten_opts or {})
    to_["kappa"] = float(kappa)
    same_env = all(np.array_equal(t.PD.env.boxes, TOP0.PD.env.boxes) and np.array_equal(t.PD.env.spheres, TOP0.PD.env.spheres)
                   for t in TOPs[1:])
    base = ([TOP0.PD.env.boxes], [TOP0.PD.env.spheres]) if same_env else ([t.PD.env.boxes for t in TOPs], [t.PD.env.spheres for t in TOPs])
    sp, mp = _capi.default_params(model.model_id)
    bounds = [_goal_bounds(t.PD.goal_set, n, t.tf_guess) for t in TOPs]
    x0 = np.stack([t.PD.x_init for t in TOPs])
    bs = BatchSolver(model.model_id, N, B, hist_cap=_hist_cap(max_iter), device=device, boxes=TOP0.PD.env.boxes,
                     spheres=TOP0.PD.env.spheres, scp_params=sp, model_params=mp)

    def restore_base():
        if same_env:
            bs.set_env(*[t[0] for t in base])
        else:
            bs.set_env_batch(*base)

    def analyse(X, U):
        bs.tvlqr(tvlqr_opts or {}, X, U)
        return bs.lincov(lo_, X=X, U=U) if disturb is None else bs.lincov_disturbed(lo_, disturb, X=X, U=U)

    out = dict(rounds=[])
    try:
        restore_base()
        bs.set_problems(x0, np.stack([b[0] for b in bounds]), np.stack([b[1] for b in bounds]), np.array([t.tf_guess for t in TOPs]))
        bs.solve(max_iter, force)
        snap = _fetch(bs)
        per = bs.last_solve_ms() * 1e-3 / B
        answered = snap["st"]["converged"] & snap["st"]["successful"]
        keepX, keepU = snap["X"].copy(), snap["U"].copy()
        src = [(snap, per)] * B                 # where the kept plan of every problem comes from
        onh = np.ones(B, bool)                  # the handle's trajectory of the problem IS its kept plan
        done, stuck = np.zeros(B, bool), np.zeros(B, bool)
        lc = analyse(keepX, keepU)
        vr = bs.verify(keepX, keepU)
        out["met_before"] = answered & (lc["min_z_obs"] >= kappa) & vr["collision_free"]
        done |= answered & (lc["min_z_obs"] >= kappa)
        tau0 = np.zeros(B)

        def resolve(mask_seed, active):
            """restart from the kept plans (mask_seed) or the straight line, solve the active ones, keep the winners' plans"""
            nonlocal keepX, keepU
            bs.set_problems_replan(tau0, x0, mask=mask_seed)
            bs.set_active(active)
            bs.solve(max_iter, force)
            bs.set_active(None)
            s = _fetch(bs)
            win = active & s["st"]["converged"] & s["st"]["successful"]
            keepX[win], keepU[win] = s["X"][win], s["U"][win]
            p = bs.last_solve_ms() * 1e-3 / max(1, int(active.sum()))
            for q in np.flatnonzero(win):
                src[q] = (s, p)
            onh[active & ~win] = False
            return win, s["st"]["iterations"], bs.last_solve_ms()

        for r in range(rounds):
            open_ = answered & ~done & ~stuck
            if not open_.any():
                break
            if r:
                lc = analyse(keepX, keepU)
            lincov_ms = bs.last_lincov_ms()
            bs.set_active(open_)
            rep = bs.tighten_env(*base, **to_)
            bs.set_active(None)
            done |= open_ & (rep["min_z_base"] >= kappa)
            blocked = rep["blocked"].astype(bool)
            todo = open_ & ~done & ~blocked
            stuck |= open_ & ~done & blocked
            rd = dict(tried=todo.copy(), min_z_base=rep["min_z_base"], max_margin=rep["max_margin"], blocked=blocked,
                      lost=np.zeros(B, bool), second_pass=np.zeros(B, bool), iterations=np.zeros(B, dtype=np.int32),
                      tighten_ms=bs.last_tighten_ms(), lincov_ms=lincov_ms, solve_ms=0.0)
            if todo.any():
                win, it, ms = resolve(onh, todo)
                rd["iterations"][todo] = it[todo]
                rd["solve_ms"] += ms
                again = todo & ~win
                if again.any():
                    win2, it2, ms2 = resolve(onh, again)
                    rd["second_pass"] = again
                    rd["iterations"][again] += it2[again]
                    rd["solve_ms"] += ms2
                    rd["lost"] = again & ~win2
                    stuck |= rd["lost"]
            out["rounds"].append(rd)
        restore_base()
        lc = analyse(keepX, keepU)
        vr = bs.verify(keepX, keepU)
        out.update(env=bs.get_env(), answered=answered, min_z_obs=lc["min_z_obs"], collision_free=vr["collision_free"],
                   met=answered & (lc["min_z_obs"] >= kappa) & vr["collision_free"])
        for q in range(B):
            SCPP = SCPProblem(TOPs[q])
            SCPS = SCPSolution(SCPP, init_traj_straightline(TOPs[q]))
            _fill_solution(SCPS, SCPP, src[q][0], q, src[q][1])
            SCPS.traj.X, SCPS.traj.U = keepX[q].T.copy(), keepU[q].T.copy()
            TOSs[q].traj, TOSs[q].SCPS = SCPS.traj, SCPS
    finally:
        bs.close()
    return out


def solve_batch_sharded(model_id, N, x_init, goal_lo, goal_hi, tf, world_size, rank, device=0, max_iter=30, boxes=None,
                        spheres=None, group=None, solver=None):
    """The multi-GPU path of SURVEY.md 8(e) in one call (one process per GPU, launched by torch.distributed.run):
    rank r solves the contiguous block shard_bounds(B, G, r) of the batch on its own GPU -- independent problems, no
    data-path collective -- and the trajectories are gathered to rank 0 STRAIGHT FROM HBM (BatchSolver.traj_dev views,
    RCCL under the nccl backend), together with the per-problem status vectors.  Returns on rank 0 a dict with X, U
    (torch tensors on the gather device), iterations, converged, successful, stop_reason (numpy); None elsewhere.
    `solver` lets a caller keep a BatchSolver (and its device buffers) across calls."""
    x_init, goal_lo, goal_hi = (np.asarray(a, float) for a in (x_init, goal_lo, goal_hi))
    B = x_init.shape[0]
    lo, hi = shard_bounds(B, world_size, rank)
    tf = np.broadcast_to(np.asarray(tf, float), (B,))
    bs = solver or BatchSolver(model_id, N, max(1, hi - lo), hist_cap=_hist_cap(max_iter), device=device, boxes=boxes,
                               spheres=spheres)
    bs.set_problems(x_init[lo:hi], goal_lo[lo:hi], goal_hi[lo:hi], tf[lo:hi])
    bs.solve(max_iter)
    Xd, Ud = bs.traj_dev()
    st = bs.status()
    local = dict(X=Xd, U=Ud, iterations=st["iterations"].astype(np.int64), converged=st["converged"].astype(np.int64),
                 successful=st["successful"].astype(np.int64), stop_reason=st["stop_reason"].astype(np.int64))
    return gather_batch_results(local, world_size, rank, group)


def gather_batch_results(local, world_size, rank, group=None):
    """Final gather of per-rank results to rank 0: the only communication of a multi-GPU run.
    `local` maps names to arrays with the problem index leading: torch tensors ALREADY ON THE GPU (the views
    BatchSolver.traj_dev() returns -- they go to RCCL as they are, no host staging) or numpy arrays (gloo on CPU, or
    small host-side vectors, moved once).  Ranks may hold different numbers of problems.  Rank 0 gets the concatenated
    dict in the type it passed in, the other ranks None."""
    import torch
    import torch.distributed as dist
    import os
    if world_size == 1 and not os.environ.get("GUSTO_FORCE_GATHER"):   # (the variable makes a 1-rank run exercise the collectives)
        return local
    out = {}
    backend = dist.get_backend(group)
    dev = torch.device("cuda", torch.cuda.current_device()) if backend == "nccl" else torch.device("cpu")
    count = torch.tensor([next(iter(local.values())).shape[0]], dtype=torch.int64, device=dev)
    sizes = [torch.zeros(1, dtype=torch.int64, device=dev) for _ in range(world_size)]
    dist.all_gather(sizes, count, group=group)
    sizes = [int(s.item()) for s in sizes]
    mx = max(sizes)
    for k, v in local.items():
        as_numpy = not torch.is_tensor(v)
        t = (torch.from_numpy(np.ascontiguousarray(v)) if as_numpy else v).to(dev)
        if t.shape[0] != mx:                   # ragged tail rank: pad to the common block size
            pad = torch.zeros((mx,) + tuple(t.shape[1:]), dtype=t.dtype, device=dev)
            pad[:t.shape[0]] = t
            t = pad
        bufs = [torch.empty_like(t) for _ in range(world_size)] if rank == 0 else None
        dist.gather(t.contiguous(), bufs, dst=0, group=group)
        if rank == 0:
            cat = torch.cat([b[:s] for b, s in zip(bufs, sizes)], dim=0)
            out[k] = cat.cpu().numpy() if as_numpy else cat
    return out if rank == 0 else None
