"""GPU parity of TrajOpt behind the seam (src/scp/scp_trajopt.jl -> gusto_solve_trajopt): the HIP path through the C ABI
against the CPU oracle on identical seeded problems -- subproblem by subproblem, trip by trip of whole runs (lock-step:
the oracle's own (traj, mu, s) of every trip goes to the device), whole runs, and properties at a larger batch.
Tolerances: both sides run the same interior point algorithm to a 1e-8 residual of the problem scaled by 1/max(1, mu).
The L1-penalised dynamics make the subproblem nearly a linear programme in the defect directions (their only curvature is
the 1e-4 regularisation), so its optimum is determined less sharply than GuSTO's: X, U, defects
within 5e-5 * max(1, mu) (measured: 1e-14 ... 1.5e-5), objective 1e-6 relative, rho and the tolerance measures 1e-4 relative (rho is a ratio of
differences), schedules (s_vec, mu_vec, counts, statuses) exact."""
import numpy as np
import pytest

import gusto_jl_amd as g
import gusto_oracle as go
import horizons as HZ
from test_kkt_certificate import as_params

pytestmark = pytest.mark.gpu
P = g.problems
H = g.host


def _setup(model, B):
    if model == g.FREEFLYER_SE2:
        return P.freeflyer_batch(B), P.freeflyer_env(), None
    bx, sp = P.iss_corner_env(True)
    if model == g.ASTROBEE_SE3_MANIFOLD:
        return P.astrobee_manifold_batch(B), bx, sp
    return P.astrobee_se3_batch(B), bx, sp


@pytest.mark.parametrize("model", [g.FREEFLYER_SE2, g.ASTROBEE_SE3, g.ASTROBEE_SE3_MANIFOLD])
@pytest.mark.parametrize("mu,s_tr", [(1.0, 1.0), (5.0, 0.25), (125.0, 0.03)])
def test_subproblem_parity(model, mu, s_tr):
    (x0, glo, ghi, tf), boxes, spheres = _setup(model, 24)
    _subproblem_parity(model, 50, boxes, spheres, (x0, glo, ghi, tf), mu, s_tr)


def _subproblem_parity(model, N, boxes, spheres, prob, mu, s_tr, Xp=None, Up=None, model_params=None):
    """one TrajOpt subproblem per problem of `prob` from (Xp, Up) (default: the straight line) against the oracle's; model_params
    (default: the model's own) goes to both sides"""
    x0, glo, ghi, tf = prob
    B = len(x0)
    s = g.TrajOptSolver(model, N, B, boxes=boxes, spheres=spheres, model_params=as_params(g.ModelParams, model_params))
    s.set_problems(x0, glo, ghi, tf)
    X0, U0 = s.traj() if Xp is None else (Xp, Up)
    r = s.subproblem(X0, U0, mu, s_tr)
    o = go.OracleTrajOpt(model, N, boxes=boxes, spheres=spheres, model_params=as_params(go.ModelParams, model_params))
    for b in range(B):
        o.set_problem(x0[b], glo[b], ghi[b], tf[b])
        ro = o.subproblem(X0[b], U0[b], mu, s_tr)
        assert r["status"][b] == ro["status"] and ro["status"] in (1, 2), (b, r["status"][b], ro["status"])
        tol = 5e-5 * max(1.0, mu)
        # (manifold model: the state is determined only up to the +-1e-4 BoxGoal on its goal quaternion -- as in the
        # GuSTO lock-step test of that model: X within 5e-4, the controls and defects at the common tolerance)
        xtol = 10 * tol if model == g.ASTROBEE_SE3_MANIFOLD else tol
        assert np.abs(r["X"][b] - ro["X"]).max() < xtol and np.abs(r["U"][b] - ro["U"]).max() < tol, b
        assert np.abs(r["D"][b] - ro["D"]).max() < tol
        assert abs(r["obj"][b] - ro["obj"]) <= 1e-6 * max(1.0, mu) * max(1.0, abs(ro["obj"]))
        # (manifold model: x_1 is pinned, so the quaternion-norm row of knot 1 is a constant and its multiplier free --
        # the quaternion components of the init dual are determined to the complementarity tolerance only)
        ed = np.abs(r["dual"][b] - ro["dual"])
        wd = 1e-5 * max(1.0, np.abs(ro["dual"]).max()) * max(1.0, mu)
        if model == g.ASTROBEE_SE3_MANIFOLD:
            assert ed[:6].max() < wd and ed[10:].max() < wd and ed[6:10].max() < 1e-2 * max(1.0, mu)
        else:
            assert ed.max() < wd
    return r


@pytest.mark.parametrize("model", [g.FREEFLYER_SE2, g.ASTROBEE_SE3, g.ASTROBEE_SE3_MANIFOLD])
def test_subproblem_parity_of_the_multi_wave_phases(model):
    """N > 64: the generic multi-wave phases (factor_sweep_mw; csrc/sweeps.hpp: backward_sweep_mw / forward_sweep_mw) -- a one-wave
    problem (every N = 50 case of this file) takes factor_sweep_w1 and backward_sweep_1w / forward_sweep_1w since round 5, so this is the test that keeps the
    generic TrajOpt path under parity.  Same tolerances as test_subproblem_parity."""
    _multi_wave_parity(model, 80)


# horizons of the TrajOpt kernel at its edges: 3, the last one-wave N, the first and last N of 2 and 3 waves (freeflyerSE2: 4 waves
# as well) and the largest N the model's LDS layout takes (tests/horizons.py).  The manifold model starts at N = 16: at N <= 8 the
# ORACLE itself ends 5 or 6 of these 6 straight-line subproblems at its 60-iteration cap (ALMOST_LOCALLY_SOLVED; N = 3, 4, 6, 8
# measured) -- its hard quaternion-norm row and the +-1e-4 BoxGoal leave a few knots no interior to converge in --, N = 16 is the
# first horizon where all six solve in 7-12 iterations.
EDGE_HORIZONS = {g.FREEFLYER_SE2: [3, 64, 65, 128, 129, 192, 193, HZ.TRAJOPT[g.FREEFLYER_SE2]],
                 g.ASTROBEE_SE3: [3, 64, 65, 128, 129, HZ.TRAJOPT[g.ASTROBEE_SE3]],
                 g.ASTROBEE_SE3_MANIFOLD: [16, 64, 65, 128, 129, HZ.TRAJOPT[g.ASTROBEE_SE3_MANIFOLD]]}


@pytest.mark.parametrize("model,N", [pytest.param(m, N, id=f"{m}-{N}") for m, Ns in EDGE_HORIZONS.items() for N in Ns])
def test_subproblem_parity_at_the_horizon_edges(model, N):
    """test_subproblem_parity_of_the_multi_wave_phases at every wave count of the TrajOpt kernel up to the model's largest N.
    astrobeeSE3 at (mu, s) = (1, 1), one of test_subproblem_parity's settings: at (5, 0.25) its problem 0 joins problem 5 at the
    edge of break-down around N = 64 (measured on the device against the oracle from the same point: 17 against 22 iterations at
    N = 64, problem 5 17 against 25 at N = 65, with X, U, D and the objective within the tolerances)"""
    _multi_wave_parity(model, N, *((1.0, 1.0) if model == g.ASTROBEE_SE3 else (5.0, 0.25)))


def _multi_wave_parity(model, N, mu=5.0, s_tr=0.25):
    B = 6
    (x0, glo, ghi, tf), boxes, spheres = _setup(model, B)
    s = g.TrajOptSolver(model, N, B, boxes=boxes, spheres=spheres)
    s.set_problems(x0, glo, ghi, tf)
    X0, U0 = s.traj()
    r = s.subproblem(X0, U0, mu, s_tr)
    o = go.OracleTrajOpt(model, N, boxes=boxes, spheres=spheres)
    marginal = 0
    for b in range(B):
        o.set_problem(x0[b], glo[b], ghi[b], tf[b])
        ro = o.subproblem(X0[b], U0[b], mu, s_tr)
        # A solve the ORACLE needs more than 30 iterations for (7-17 is what this set takes otherwise) is a marginal one: the
        # interior point iteration wanders at the edge of break-down and where it ends up -- 19, 37 or 58 iterations, or
        # SOLVER_FAILED -- moves with the summation order on both sides (astrobeeSE3 problem 5 at every N tried: 19 / 35 / 18
        # device iterations against 37 / 41 / 25 at N = 50 / 64 / 65; astrobeeSE3manifold problem 5 at N >= 65: the oracle
        # stops SOLVER_FAILED at its 60-iteration cap).  At most one such problem in this set; it is not compared.
        if ro["iters"] > 30:
            marginal += 1
            continue
        assert ro["status"] in (1, 2), (b, ro["status"])
        assert r["status"][b] in (1, 2), (b, r["status"][b], ro["status"])
        tol = 5e-5 * max(1.0, mu)
        # (manifold model: X within 10 x tol inside the +-1e-4 BoxGoal of its goal quaternion, as in test_subproblem_parity)
        xtol = 10 * tol if model == g.ASTROBEE_SE3_MANIFOLD else tol
        assert np.abs(r["X"][b] - ro["X"]).max() < xtol and np.abs(r["U"][b] - ro["U"]).max() < tol, b
        assert np.abs(r["D"][b] - ro["D"]).max() < tol
        assert abs(r["obj"][b] - ro["obj"]) <= 1e-6 * max(1.0, mu) * max(1.0, abs(ro["obj"]))
        assert abs(int(r["iters"][b]) - int(ro["iters"])) <= 3, (b, r["iters"][b], ro["iters"])
    assert marginal <= 1, marginal


@pytest.mark.parametrize("model,B", [(g.FREEFLYER_SE2, 48), (g.ASTROBEE_SE3, 24), (g.ASTROBEE_SE3_MANIFOLD, 128)])
def test_whole_runs_match_the_oracle(model, B):
    """solve_trajopt_jump! end to end: identical schedules (number of solves, s_vec, mu_vec, lengths of every vector,
    converged, stop reason) on EVERY problem -- no divergence is allowed --, rho / xtol / ftol / ctol / J histories and the final
    trajectory.

    Manifold model, round 6: its convex_state_eq row (the linearised quaternion norm) is the hard equality the reference states
    (scp_trajopt.jl:200-208; an equality row of the interior point method, common.hpp: TRAJOPT_EQ_DELTA) instead of the band
    |h| <= 1e-4 of rounds 3-5, whose barrier weights decided 4 of these 128 runs in the last digits (SubproblemFailed on one side
    only).  With the equality every one of the 128 schedules is identical.  What the equality does NOT give is a contracting SCP
    loop: this model has no trust-region row (astrobee_se3_manifold.jl:601), from the sixth solve on the trust-region ratio turns
    negative, steps are rejected, and the loop amplifies the last digits of every subproblem solution by ~10x per solve
    (tools/to_whole_diff.py, worst of 128 runs by solve index: convergence measure 9e-8, 3e-6, 3e-4, 1e-3, 6e-4, 6e-2, 0.2 ...;
    J_true 5e-8 ... 3e-4).  So the histories of this model are compared tightly over the first three solves, J over the whole run,
    and the per-trip agreement -- every trip of every problem from the oracle's own state -- is test_lockstep_every_trip."""
    (x0, glo, ghi, tf), boxes, spheres = _setup(model, B)
    man = model == g.ASTROBEE_SE3_MANIFOLD
    s = g.TrajOptSolver(model, 50, B, boxes=boxes, spheres=spheres)
    s.set_problems(x0, glo, ghi, tf)
    s.solve(125)
    X, U = s.traj()
    st, h = s.status(), s.history()
    o = go.OracleTrajOpt(model, 50, boxes=boxes, spheres=spheres)
    trips = n_soft = 0
    for b in range(B):
        o.set_problem(x0[b], glo[b], ghi[b], tf[b])
        R = o.solve_trajopt(125)
        S = R["solves"]
        trips += S
        assert st["iterations"][b] == S and bool(st["converged"][b]) == R["converged"] and st["stop_reason"][b] == R["stop_reason"], b
        assert h["n_mu"][b] == len(R["mu_vec"]) and h["n_xtol"][b] == len(R["xtol_vec"]) and h["n_ftol"][b] == len(R["ftol_vec"])
        assert h["n_ctol"][b] == len(R["ctol_vec"])
        assert np.array_equal(h["s_vec"][b, :S + 1], R["s_vec"]) and np.array_equal(h["mu_vec"][b, :h["n_mu"][b]], R["mu_vec"])
        # (OPTIMAL against ALMOST_LOCALLY_SOLVED -- the 60-iteration cap reached within the acceptable level on one side, the
        #  tolerance met just before it on the other -- is the same accepted solve; measured: one such entry in the astrobee run)
        sd, so = h["solver_status"][b, 1:S + 1], np.asarray(R["solver_status"][1:S + 1])
        soft = (sd != so) & np.isin(sd, (1, 2)) & np.isin(so, (1, 2))
        assert np.array_equal(sd[~soft], so[~soft]), b
        n_soft += int(soft.sum())
        if man:   # (see the docstring: the first three solves at 1e-3 / 1e-5, J over the whole run, the final state loosely)
            E = min(S, 3)
            assert np.allclose(h["rho_vec"][b, :E + 1], R["rho_vec"][:E + 1], rtol=1e-3, atol=1e-8), b
            assert np.allclose(h["xtol_vec"][b, :E + 1], R["xtol_vec"][:E + 1], rtol=1e-3, atol=1e-9), b
            assert np.allclose(h["convergence_measure"][b, 1:E + 1], R["conv"][1:E + 1], rtol=1e-3, atol=1e-9), b
            assert np.allclose(h["J_true"][b, :E + 1], R["J_true"][:E + 1], rtol=1e-5, atol=1e-12), b
            assert np.allclose(h["J_full"][b, :E], R["J_full"][:E], rtol=1e-4, atol=1e-9), b
            assert np.allclose(h["J_true"][b, :S + 1], R["J_true"], rtol=2e-3, atol=1e-12), b          # (measured 2.9e-4)
            assert np.abs(X[b] - R["X"]).max() < 0.1 * R["mu_vec"][-1], b                                # (measured 2.4e-2)
            continue
        rt = 1e-4
        assert np.allclose(h["rho_vec"][b, :S + 1], R["rho_vec"], rtol=rt, atol=1e-8)
        for k, ref in (("xtol_vec", R["xtol_vec"]), ("ftol_vec", R["ftol_vec"]), ("ctol_vec", R["ctol_vec"])):
            assert np.allclose(h[k][b, :len(ref)], ref, rtol=rt, atol=1e-9), (b, k)
        assert np.allclose(h["J_true"][b, :S + 1], R["J_true"], rtol=1e-7, atol=1e-12)   # (beyond this set: 11 of 1024 freeflyerSE2 runs up to 2.4e-5, tools/to_sweep.py)
        assert np.allclose(h["J_full"][b, :S], R["J_full"], rtol=1e-6, atol=1e-9)
        assert np.allclose(h["convergence_measure"][b, 1:S + 1], R["conv"][1:S + 1], rtol=1e-4, atol=1e-9)
        assert np.abs(X[b] - R["X"]).max() < 5e-5 * R["mu_vec"][-1] and np.abs(U[b] - R["U"]).max() < 5e-5 * R["mu_vec"][-1], b
    print(f"model {model}: {B} whole runs, {trips} solves, OPTIMAL-against-ALMOST entries {n_soft}")
    assert trips >= 5 * B and n_soft <= max(2, B // 8), (trips, n_soft)


@pytest.mark.parametrize("model,B", [(g.FREEFLYER_SE2, 32), (g.ASTROBEE_SE3, 16), (g.ASTROBEE_SE3_MANIFOLD, 12)])
def test_lockstep_every_trip(model, B):
    """Every trip of every problem from the ORACLE's own state: its (traj, defects, mu, s) before the trip goes through
    gusto_subproblem_trajopt and the optimum must be the oracle's optimum of that trip."""
    _lockstep(model, B, 50)


@pytest.mark.parametrize("model,B", [(g.FREEFLYER_SE2, 8), (g.ASTROBEE_SE3, 6), (g.ASTROBEE_SE3_MANIFOLD, 5)])
def test_lockstep_every_trip_at_the_largest_horizon(model, B):
    """test_lockstep_every_trip at the largest N of the model's TrajOpt kernel (tests/horizons.py: 4 / 3 / 3 waves).  The manifold
    set stops before its problem 5, the marginal one of test_subproblem_parity_at_the_horizon_edges (its first subproblem at N = 139:
    the oracle's run ALMOST_LOCALLY_SOLVED, the device SOLVER_FAILED; from the straight line the oracle alone fails it at N >= 65)."""
    _lockstep(model, B, HZ.TRAJOPT[model])


def _lockstep(model, B, N):
    (x0, glo, ghi, tf), boxes, spheres = _setup(model, B)
    o = go.OracleTrajOpt(model, N, boxes=boxes, spheres=spheres)
    m0 = o.m0
    s = g.TrajOptSolver(model, N, B, boxes=boxes, spheres=spheres)
    s.set_problems(x0, glo, ghi, tf)
    runs = []
    for b in range(B):
        o.set_trace(64)
        o.set_problem(x0[b], glo[b], ghi[b], tf[b])
        R = o.solve_trajopt(125)
        runs.append((R, o.trace()))
    T = max(R["solves"] for R, _ in runs)
    trips = 0
    for t in range(T):
        # problems that have no trip t repeat their last one (the batch call wants B problems)
        tt = [min(t, R["solves"] - 1) for R, _ in runs]
        Xp = np.stack([tr[i]["Xp"] for (R, tr), i in zip(runs, tt)])
        Up = np.stack([tr[i]["Up"][:, :m0] for (R, tr), i in zip(runs, tt)])
        mu = np.array([R["omega"][i + 1] for (R, _), i in zip(runs, tt)])
        s_tr = np.array([R["Delta"][i + 1] for (R, _), i in zip(runs, tt)])
        sub = s.subproblem(Xp, Up, mu, s_tr)
        for b, ((R, tr), i) in enumerate(zip(runs, tt)):
            if i != t:
                continue
            trips += 1
            assert sub["status"][b] == R["solver_status"][i + 1] or {int(sub["status"][b]), int(R["solver_status"][i + 1])} == {1, 2}, (b, t)
            tol = 5e-5 * max(1.0, mu[b])
            man = model == g.ASTROBEE_SE3_MANIFOLD       # (X inside the +-1e-4 BoxGoal of the goal quaternion, see test_subproblem_parity)
            assert np.abs(sub["X"][b] - tr[i]["Xn"]).max() < (10 if man else 1) * tol and np.abs(sub["U"][b] - tr[i]["Un"][:, :m0]).max() < tol, (b, t)
            assert np.abs(sub["D"][b] - tr[i]["Un"][:, m0:]).max() < tol
            # (the objective is a sum over the knots: its tolerance grows with N / 50 -- measured 1.9e-6 relative at freeflyerSE2 N = 256)
            assert abs(sub["obj"][b] - R["J_full"][i]) <= (1e-4 if man else 1e-6) * max(1.0, N / 50) * max(1.0, mu[b]) * max(1.0, abs(R["J_full"][i]))
    assert trips == sum(R["solves"] for R, _ in runs) >= 5 * B


def test_properties_at_batch_1024():
    """size-independent properties at a larger batch: bitwise determinism, hard boundary rows, the trust region of the last
    step, vanishing defects once the penalty has grown, the cost histories."""
    model, B = g.FREEFLYER_SE2, 1024
    (x0, glo, ghi, tf), boxes, spheres = _setup(model, B)
    s = g.TrajOptSolver(model, 50, B, boxes=boxes, spheres=spheres)
    out = []
    for _ in range(2):
        s.set_problems(x0, glo, ghi, tf)
        s.solve(125)
        out.append(s.traj() + (s.status(), s.history()))
    (X, U, st, h), (X2, U2, st2, h2) = out
    assert np.array_equal(X, X2) and np.array_equal(U, U2) and np.array_equal(st["iterations"], st2["iterations"])
    assert np.array_equal(h["rho_vec"], h2["rho_vec"])
    # (a failed subproblem is data: 3 of these 1024 problems stop with SubproblemFailed -- on the oracle too)
    ok = st["stop_reason"] <= 1
    assert (st["stop_reason"] <= 2).all() and ok.sum() >= B - 8 and (st["iterations"][ok] >= 4).all()
    assert np.abs(X[:, 0] - x0).max() < 1e-9 and np.abs(X[ok, -1] - glo[ok]).max() < 1e-7
    tp = g.default_trajopt_params(model)
    for b in range(0, B, 37):
        S = st["iterations"][b]
        sv, rv = h["s_vec"][b, :S + 1], h["rho_vec"][b, :S + 1]
        assert sv[0] == tp.s0 and all(sv[i + 1] == (tp.tau_plus if rv[i + 1] > tp.c else tp.tau_minus) * sv[i] for i in range(S))
        mv = h["mu_vec"][b, :h["n_mu"][b]]
        assert mv[0] == tp.mu0 and np.allclose(mv[1:] / mv[:-1], tp.k)
        assert np.isfinite(h["J_true"][b, :S + 1]).all() and (h["J_true"][b, 1:S + 1] > 0).all() or not ok[b]
    # trapezoid defects of the returned trajectories: below 1e-6 for most problems whose penalty reached 25 (two increases)
    mp = g.default_params(model)[1]
    dt = tf[0] / 49
    A = np.kron(np.array([[0.0, 1.0], [0.0, 0.0]]), np.eye(3))
    Bm = np.zeros((6, 3)); Bm[3, 0] = Bm[4, 1] = 1 / mp.mass; Bm[5, 2] = 1 / mp.Jdiag[2]
    a = X @ A.T + U @ Bm.T
    F = X[:, 1:] - X[:, :-1] - 0.5 * dt * (a[:, :-1] + a[:, 1:])
    grown = (h["n_mu"] >= 3) & ok
    small = np.abs(F[grown]).reshape(grown.sum(), -1).max(axis=1) < 1e-6
    assert grown.sum() > B // 2 and small.mean() > 0.9


def test_through_the_seam_and_error_paths():
    """solve_SCP!(TOS, TOP, solve_trajopt_hip!, init_traj_straightline, "hip") on the notebook problem; the models without
    a SCPParam_TrajOpt and the calls that belong to the other algorithm fail loudly."""
    model = H.FreeflyerSE2()
    gs = H.GoalSet()
    H.add_goal(gs, H.Goal(H.PointGoal(P.FREEFLYER_X_GOAL), P.FREEFLYER_TF, model))
    PD = H.ProblemDefinition(H.Robot(), model, H.Environment(P.freeflyer_env()), P.FREEFLYER_X_INIT, gs)
    TOP = H.TrajectoryOptimizationProblem(PD, 50, P.FREEFLYER_TF, fixed_final_time=True)
    TOS = H.TrajectoryOptimizationSolution(TOP)
    SCPS = H.solve_SCP(TOS, TOP, H.solve_trajopt_hip, H.init_traj_straightline, "hip", max_iter=125)
    o = go.OracleTrajOpt(go.FREEFLYER_SE2, 50, boxes=P.freeflyer_env())
    o.set_problem(P.FREEFLYER_X_INIT, P.FREEFLYER_X_GOAL, P.FREEFLYER_X_GOAL, P.FREEFLYER_TF)
    R = o.solve_trajopt(125)
    assert SCPS.iterations == R["solves"] and SCPS.converged == R["converged"] and TOS.traj is SCPS.traj
    assert np.abs(TOS.traj.X.T - R["X"]).max() < 1e-6 and TOS.traj.U.shape == (3, 50)
    assert len(SCPS.J_true) == R["solves"] + 1 and len(SCPS.J_full) == R["solves"] == len(SCPS.convergence_measure) - 1
    assert SCPS.SCPP.mu_vec == list(R["mu_vec"]) and SCPS.SCPP.s_vec == list(R["s_vec"])
    assert np.abs(SCPS.dual - R["dual"]).max() < 1e-5 * max(1.0, np.abs(R["dual"]).max()) * R["mu_vec"][-1]
    with pytest.raises(g.GustoError):
        g.TrajOptSolver(g.DUBINS_CAR, 30, 2)
    s = g.TrajOptSolver(g.FREEFLYER_SE2, 50, 2, boxes=P.freeflyer_env())
    x0, glo, ghi, tf = P.freeflyer_batch(2)
    s.set_problems(x0, glo, ghi, tf)
    with pytest.raises(g.GustoError):
        g.BatchSolver.solve(s, 30)                 # gusto_solve on a TrajOpt handle
    b = g.BatchSolver(g.FREEFLYER_SE2, 50, 2, boxes=P.freeflyer_env())
    b.set_problems(x0, glo, ghi, tf)
    assert b.L.gusto_solve_trajopt(b.h, 10) != 0   # and the other way round
    small = g.TrajOptSolver(g.FREEFLYER_SE2, 50, 2, hist_cap=16, boxes=P.freeflyer_env())
    small.set_problems(x0, glo, ghi, tf)
    with pytest.raises(g.GustoError):
        small.solve(125)                           # hist_cap below the schedule's needs: refused, not truncated


def test_batch_through_the_seam_and_handle_reuse():
    """solve_SCP_batch!(TOSs, TOPs, solve_trajopt_hip!, ...): one gusto_solve_trajopt for the list (also sharded over two
    handles) gives what solve_SCP! gives problem by problem; a second solve_trajopt_hip! on the same SCPSolution re-uses
    its handle (no new device allocation per call) and, like solve_trajopt_jump!, starts the schedule again from SCPS.traj."""
    x0, glo, ghi, tf = P.freeflyer_batch(5)
    TOPs = []
    for b in range(5):
        model = H.FreeflyerSE2()
        gs = H.GoalSet()
        H.add_goal(gs, H.Goal(H.PointGoal(glo[b]), tf[b], model))
        TOPs.append(H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.Environment(P.freeflyer_env()), x0[b], gs),
                                                    30, tf[b], fixed_final_time=True))
    ones = [H.solve_SCP(H.TrajectoryOptimizationSolution(t), t, H.solve_trajopt_hip, H.init_traj_straightline, "hip", max_iter=125)
            for t in TOPs]
    for devices in (None, [0, 0]):
        TOSs = [H.TrajectoryOptimizationSolution(t) for t in TOPs]
        out = H.solve_SCP_batch(TOSs, TOPs, H.solve_trajopt_hip, H.init_traj_straightline, "hip", max_iter=125, devices=devices)
        for b in range(5):
            assert out[b].iterations == ones[b].iterations and out[b].converged == ones[b].converged
            assert np.array_equal(out[b].traj.X, ones[b].traj.X) and np.array_equal(out[b].traj.U, ones[b].traj.U)
            assert out[b].SCPP.mu_vec == ones[b].SCPP.mu_vec and out[b].SCPP.s_vec == ones[b].SCPP.s_vec
            assert TOSs[b].traj is out[b].traj and out[b].traj.U.shape == (3, 30)
    S = ones[0]
    handle = S._solver_trajopt
    n1 = S.iterations
    H.solve_trajopt_hip(S, S.SCPP, "hip", 125)
    assert S._solver_trajopt is handle and S._solver is None and S.iterations > 0 and len(S.J_true) == S.iterations + 1
    assert n1 > 0
    # the two algorithms never find each other's handle: a GuSTO solve on the same SCPSolution creates its own and the
    # shooting refinement (which needs the GuSTO handle's device state) is not disturbed by a TrajOpt call in between
    H.solve_gusto_hip(S, S.SCPP, "hip", 2)
    gh = S._solver
    assert type(gh) is g.BatchSolver and S._solver_trajopt is handle
    H.solve_trajopt_hip(S, S.SCPP, "hip", 125)
    assert S._solver is gh and gh.h


def test_async_solves_of_two_handles_overlap_and_change_nothing():
    """gusto_solve_trajopt_async + gusto_wait: two TrajOpt handles on one GPU with their launches in flight together give,
    bit for bit, what gusto_solve_trajopt gives each of them alone, and the pair takes less wall time than the two
    synchronous solves one after the other (each batch is small enough to leave most of the GPU to the other)."""
    import time
    B = 96
    x0, glo, ghi, tf = P.freeflyer_batch(2 * B)
    hs = [g.TrajOptSolver(g.FREEFLYER_SE2, 50, B, boxes=P.freeflyer_env()) for _ in range(2)]
    ref, t_sync = [], 0.0
    for rep in range(2):                       # (first round warms both handles up)
        ref, t_sync = [], 0.0
        for j, s in enumerate(hs):
            s.set_problems(x0[j * B:(j + 1) * B], glo[j * B:(j + 1) * B], ghi[j * B:(j + 1) * B], tf[j * B:(j + 1) * B])
            t0 = time.perf_counter()
            s.solve(125)
            t_sync += time.perf_counter() - t0
            ref.append((s.traj(), s.status(), s.history()))
    for j, s in enumerate(hs):
        s.set_problems(x0[j * B:(j + 1) * B], glo[j * B:(j + 1) * B], ghi[j * B:(j + 1) * B], tf[j * B:(j + 1) * B])
    t0 = time.perf_counter()
    for s in hs:
        s.solve_async(125)                     # both launches queued before either is waited for
    for s in hs:
        s.wait()
    t_async = time.perf_counter() - t0
    for j, s in enumerate(hs):
        (X, U), st, h = ref[j]
        Xa, Ua = s.traj()
        assert np.array_equal(X, Xa) and np.array_equal(U, Ua)
        sa = s.status()
        assert all(np.array_equal(st[k], sa[k]) for k in st)
        ha = s.history()
        assert all(np.array_equal(h[k], ha[k], equal_nan=(h[k].dtype.kind == "f")) for k in h)
    # (a measurement, not a gate: single wall-clock samples of ~10 ms solves on a shared box say nothing reliable; what the test
    # holds is that the overlapped solves change no bit -- above)
    print(f"trajopt 2 x {B}: sync {1e3 * t_sync:.1f} ms, async pair {1e3 * t_async:.1f} ms")
    # the error paths of the new entry point are those of the synchronous one
    gs = g.BatchSolver(g.FREEFLYER_SE2, 50, 2, boxes=P.freeflyer_env())
    gs.set_problems(x0[:2], glo[:2], ghi[:2], tf[:2])
    assert gs.L.gusto_solve_trajopt_async(gs.h, 10) != 0
    fresh = g.TrajOptSolver(g.FREEFLYER_SE2, 50, 2, boxes=P.freeflyer_env())
    with pytest.raises(g.GustoError):
        fresh.solve_async(125)                 # no problems set
