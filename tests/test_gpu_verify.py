"""gusto_verify / gusto_interpolate on the device against tests/np_verify.py, the numpy restatement of the reference's
interpolate_traj, dynamics_constraint_satisfaction and verify_collision_free (plus the dense minimum distance and the gap).

Tolerances: the integer and flag fields are compared exactly; distances, defect and gap to 1e-9 max(1, |ref|); the dense
trajectory to 1e-10 relative.  Both are fp64 reassociation bounds of an RK4 step and a sum over at most 256 knots (the device
contracts a x + b into one rounding and sums the knots as a tree), not measurements.  tests/test_verify_cpu.py shows that the
distances of the straight-line inputs stay 1e-6 away from zero, so no flag can hinge on those last digits."""
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import np_verify as V
from test_verify_cpu import FIRST, batch, straight_line

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = g.problems
N = 50
INT_FIELDS = ("collision_free", "first_knot", "min_dense_sample")
DBL_FIELDS = ("first_dist", "min_dist_knots", "dyn_defect_l1", "min_dist_dense", "max_gap")


def _close(a, ref, tol=1e-9):
    if np.isinf(ref) or np.isnan(ref):
        return (np.isnan(a) and np.isnan(ref)) or a == ref
    return abs(a - ref) <= tol * max(1.0, abs(ref))


def _compare(model, rep, X, U, tf, env_of, idx=None, flags_if=None, dense=None, **opts):
    """every field of the device report `rep` against np_verify for the problems `idx`; returns the number of problems whose
    flag fields were left out by `flags_if` (a predicate on the reference report)"""
    left_out = 0
    worst = dict.fromkeys(DBL_FIELDS, 0.0)
    for b in (range(len(X)) if idx is None else idx):
        bx, sp = env_of(b)
        r = V.report(model, X[b], U[b], tf[b], bx, sp, **opts)
        if flags_if is None or flags_if(r):
            for k in INT_FIELDS:
                assert int(rep[k][b]) == int(r[k]), (b, k, rep[k][b], r[k], r["min_dist_knots"], r["min_dist_dense"])
        else:
            left_out += 1
        for k in DBL_FIELDS:
            if k == "first_dist" and flags_if is not None and not flags_if(r):
                continue
            if np.isfinite(r[k]):
                worst[k] = max(worst[k], abs(rep[k][b] - r[k]) / max(1.0, abs(r[k])))
            assert _close(rep[k][b], r[k]), (b, k, rep[k][b], r[k])
        if dense is not None:
            nfull, Xf, Uf = dense
            assert nfull[b] == r["nfull"], (b, nfull[b], r["nfull"])
            ref = r["Xfull"]
            err = np.abs(Xf[b, :nfull[b]] - ref).max() / max(1.0, np.abs(ref).max())
            assert err <= 1e-10, (b, err)
            assert np.array_equal(Uf[b, :nfull[b] - 1], r["Ufull"])
            assert not Xf[b, nfull[b]:].any() and not Uf[b, nfull[b] - 1:].any()
    print(f"model {model}: worst relative differences {worst}")
    return left_out


def _solver(model, B, boxes, spheres, n_knots=N, hist_cap=64):
    return g.BatchSolver(model, n_knots, B, hist_cap=hist_cap, boxes=boxes, spheres=spheres)


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_straight_line_inits_against_numpy(model):
    """(1) B = 256, N = 50, the straight-line inits passed as X, U: every field for every problem, and the dense trajectory."""
    B = 256
    x0, glo, ghi, tf, boxes, spheres = batch(model, B, FIRST.get(model, 0))
    Xs, Us = straight_line(model, x0, glo, ghi)
    s = _solver(model, B, boxes, spheres)
    s.set_problems(x0, glo, ghi, tf)
    rep = s.verify(Xs, Us)
    assert s.last_verify_ms() > 0
    dense = s.interpolate(Xs, Us)
    rep2 = s.get_verify()
    for k in INT_FIELDS + DBL_FIELDS:                      # interpolate is verify plus the dense stores
        assert np.array_equal(rep[k], rep2[k], equal_nan=True), k
    _compare(model, rep, Xs, Us, tf, lambda b: (boxes, spheres), dense=dense)
    if model == g.DUBINS_CAR:
        assert rep["collision_free"].all() and np.isinf(rep["min_dist_knots"]).all() and np.isinf(rep["min_dist_dense"]).all()
        assert (rep["min_dense_sample"] == -1).all() and not rep["first_knot"].any()
    else:
        assert not rep["collision_free"].all()             # (straight lines through the obstacle field: some of them collide)
    s.close()


@pytest.mark.parametrize("model", [0, 2, 3])
def test_solved_trajectories_on_the_handle(model):
    """(2) after a real solve(30), X = U = None: the handle's trajectories, status and histories are what they were, and the report
    is np_verify's of those trajectories.  Flag fields are compared wherever the reference |min distance| exceeds 1e-9; at most 1 %
    of the problems may fall below (asserted)."""
    B = 256
    x0, glo, ghi, tf, boxes, spheres = batch(model, B, FIRST[model])
    s = _solver(model, B, boxes, spheres)
    s.set_problems(x0, glo, ghi, tf)
    s.solve(30)
    ms = s.last_solve_ms()
    X, U = s.traj()
    st, h = s.status(), s.history()
    rep = s.verify()
    X1, U1 = s.traj()
    assert np.array_equal(X, X1) and np.array_equal(U, U1)
    st1, h1 = s.status(), s.history()
    assert all(np.array_equal(st[k], st1[k]) for k in st) and all(np.array_equal(h[k], h1[k], equal_nan=True) for k in h)
    assert s.last_solve_ms() == ms
    ok = lambda r: min(abs(r["min_dist_knots"]), abs(r["min_dist_dense"])) > 1e-9
    left_out = _compare(model, rep, X, U, tf, lambda b: (boxes, spheres), flags_if=ok)
    assert left_out <= 0.01 * B, left_out
    assert (rep["min_dist_dense"] <= rep["min_dist_knots"]).all()      # (every knot is a dense sample)
    s.close()


def test_per_problem_environments():
    """(3) gusto_set_env_batch: every problem against its own keep-out set (the layouts of freeflyer_random_layouts)."""
    B = 64
    x0, glo, ghi, tf = P.freeflyer_batch(B)
    bl, sl = P.freeflyer_random_layouts(B)
    Xs, Us = straight_line(0, x0, glo, ghi)
    s = g.BatchSolver(0, N, B, hist_cap=16)
    s.set_env_batch(bl, sl)
    s.set_problems(x0, glo, ghi, tf)
    rep = s.verify(Xs, Us, nstep=8)
    _compare(0, rep, Xs, Us, tf, lambda b: (bl[b], sl[b]), nstep=8)
    assert len({(len(b), len(q)) for b, q in zip(bl, sl)}) >= 4
    s.close()
    # the four fixed layouts of test_gpu_env_batch.py, the empty one among them
    full = P.freeflyer_env()
    layouts = [(full, None), (np.vstack([full[:4], full[[5, 8, 9, 12]]]), np.array([[1.7, 1.2, 0.0, 0.18]])), (full[:4].copy(), None),
               (None, None)]
    lay = [b % 4 for b in range(B)]
    s = g.BatchSolver(0, N, B, hist_cap=16)
    s.set_env_batch([layouts[l][0] for l in lay], [layouts[l][1] for l in lay])
    s.set_problems(x0, glo, ghi, tf)
    rep = s.verify(Xs, Us, nstep=8)
    _compare(0, rep, Xs, Us, tf, lambda b: layouts[lay[b]], nstep=8)
    assert np.isinf(rep["min_dist_dense"][3::4]).all() and (rep["min_dense_sample"][3::4] == -1).all()
    s.close()


def test_step_counts_per_problem_and_the_cap():
    """(4) nstep fixed against dt_min; per-problem tf giving different Nstep_b in one batch, zeros behind every problem's own
    samples; an Nstep_b above nstep_cap is an error, never clamped."""
    B = 16
    x0, glo, ghi, tf, boxes, spheres = batch(2, B)
    tf = np.linspace(20.0, 95.0, B)                        # dt = tf / 49: 5 .. 20 substeps of at most 0.1 s
    Xs, Us = straight_line(2, x0, glo, ghi)
    s = _solver(2, B, boxes, spheres)
    s.set_problems(x0, glo, ghi, tf)
    rep = s.verify(Xs, Us)
    dense = s.interpolate(Xs, Us)
    ns = np.array([V.n_substeps(t, N) for t in tf])
    assert len(set(ns)) > 4 and np.array_equal(dense[0], ns * (N - 1) + 1) and dense[1].shape[1] == ns.max() * (N - 1) + 1
    _compare(2, rep, Xs, Us, tf, lambda b: (boxes, spheres), dense=dense)
    rep = s.verify(Xs, Us, nstep=3, dt_min=1e-9)           # nstep > 0: dt_min is not looked at
    dense = s.interpolate(Xs, Us, nstep=3)
    assert (dense[0] == 3 * (N - 1) + 1).all()
    _compare(2, rep, Xs, Us, tf, lambda b: (boxes, spheres), dense=dense, nstep=3)
    rep = s.verify(Xs, Us, dense_collision=0)
    assert np.isinf(rep["min_dist_dense"]).all() and (rep["min_dense_sample"] == -1).all()
    for bad in (dict(nstep_cap=int(ns.max()) - 1), dict(dt_min=0.01), dict(nstep=65), dict(nstep=-1), dict(dt_min=0.0),
                dict(dense_collision=2)):
        with pytest.raises(g._capi.GustoError, match="-> -1"):
            s.verify(Xs, Us, **bad)
    assert s.verify(Xs, Us, nstep_cap=int(ns.max()))["collision_free"].shape == (B,)
    s.close()


@pytest.mark.parametrize("n_knots", [3, 64, 65, 128])
def test_horizons_and_the_multi_wave_reduction(n_knots):
    """(4) N = 3, 64, 65, 128 (tests/horizons.py: N_MIN, one wave full, the first two-wave horizon, two waves full)."""
    import horizons as HZ
    assert n_knots >= HZ.N_MIN and n_knots <= min(HZ.GUSTO.values()) and HZ.waves(65) == 2
    B = 24
    for model in (0, 3):
        x0, glo, ghi, tf, boxes, spheres = batch(model, B)
        tf = tf * (n_knots - 1) / 98.0                     # (keeps dt, and with it Nstep, at half the N = 50 batch's)
        Xs, Us = straight_line(model, x0, glo, ghi, n_knots)
        s = _solver(model, B, boxes, spheres, n_knots, hist_cap=16)
        s.set_problems(x0, glo, ghi, tf)
        dense = s.interpolate(Xs, Us)
        _compare(model, s.get_verify(), Xs, Us, tf, lambda b: (boxes, spheres), dense=dense)
        s.close()


def test_a_report_does_not_depend_on_the_batch():
    """(5) the same problem alone and inside B = 256: bitwise equal report and dense trajectory; set_active leaves the reports
    of the inactive problems as they were."""
    B = 256
    for model in (0, 2):
        x0, glo, ghi, tf, boxes, spheres = batch(model, B)
        Xs, Us = straight_line(model, x0, glo, ghi)
        s = _solver(model, B, boxes, spheres)
        s.set_problems(x0, glo, ghi, tf)
        nfull, Xf, Uf = s.interpolate(Xs, Us)
        rep = s.get_verify()
        for b in (0, 77, 255):
            s1 = _solver(model, 1, boxes, spheres)
            s1.set_problems(x0[b:b + 1], glo[b:b + 1], ghi[b:b + 1], tf[b:b + 1])
            n1, X1, U1 = s1.interpolate(Xs[b:b + 1], Us[b:b + 1])
            r1 = s1.get_verify()
            for k in INT_FIELDS + DBL_FIELDS:
                assert np.array_equal(rep[k][b:b + 1], r1[k], equal_nan=True), (model, b, k)
            assert n1[0] == nfull[b] and np.array_equal(X1[0], Xf[b]) and np.array_equal(U1[0], Uf[b])
            s1.close()
        # the second half only, on trajectories that differ: the first half keeps its report
        act = np.arange(B) >= B // 2
        s.set_active(act)
        rep2 = s.verify(Xs[::-1].copy(), Us[::-1].copy())
        for k in INT_FIELDS + DBL_FIELDS:
            assert np.array_equal(rep2[k][~act], rep[k][~act], equal_nan=True), k
        assert not np.array_equal(rep2["dyn_defect_l1"][act], rep["dyn_defect_l1"][act])
        _compare(model, rep2, Xs[::-1], Us[::-1], tf, lambda b: (boxes, spheres), idx=range(B // 2, B, 16))
        s.set_active(None)
        s.close()


def test_refusals():
    """(6) TrajOpt handles are refused with a message, verify before set_problems is a state error, X without U an argument error."""
    x0, glo, ghi, tf, boxes, spheres = batch(0, 4)
    t = g._capi.TrajOptSolver(0, N, 4, boxes=boxes)
    t.set_problems(x0, glo, ghi, tf)
    with pytest.raises(g._capi.GustoError):
        t.verify()
    with pytest.raises(g._capi.GustoError):
        t.interpolate()
    rc = t.L.gusto_verify(t.h, None, None, None)
    assert rc == -1 and b"TrajOpt" in t.L.gusto_last_error(t.h)
    t.close()
    s = _solver(0, 4, boxes, None)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.B = 4
        s.verify()
    s.set_problems(x0, glo, ghi, tf)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_verify()
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.last_verify_ms()
    Xs, Us = straight_line(0, x0, glo, ghi)
    assert s.L.gusto_verify(s.h, Xs.ctypes.data, None, None) == -1
    s.verify()
    s.set_problems(x0, glo, ghi, tf)                       # new problems: the old report is gone
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_verify()
    s.close()


def test_host_mirror_and_batch_option():
    """host.py: the three reference functions on one trajectory, and solve_SCP_batch(..., verify=True)."""
    H = g.host
    env = P.freeflyer_env()
    x0 = P.freeflyer_random_x_init(6)
    TOPs = []
    for b in range(6):
        model = H.FreeflyerSE2()
        gs = H.GoalSet()
        H.add_goal(gs, H.Goal(H.PointGoal(P.FREEFLYER_X_GOAL), 200.0, model))
        TOPs.append(H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.Environment(env), x0[b], gs), N, 200.0,
                                                    fixed_final_time=True))
    SCPP = H.SCPProblem(TOPs[1])
    traj = H.init_traj_straightline(TOPs[1])
    r = V.report(0, traj.X.T, traj.U.T, 200.0, env, None)
    free, k, d = H.verify_collision_free(traj, SCPP)
    assert (free, k) == (r["collision_free"], r["first_knot"]) and _close(d, r["first_dist"])
    assert _close(H.dynamics_constraint_satisfaction(traj, SCPP), r["dyn_defect_l1"])
    full = H.interpolate_traj(traj, SCPP)
    assert isinstance(full, H.Trajectory) and full.X.shape == (6, r["nfull"]) and full.U.shape == (3, r["nfull"] - 1)
    assert np.abs(full.X.T - r["Xfull"]).max() <= 1e-10 * max(1.0, np.abs(r["Xfull"]).max()) and full.Tf == 200.0
    TOSs = [H.TrajectoryOptimizationSolution(t) for t in TOPs]
    plain = H.solve_SCP_batch(TOSs, TOPs)
    assert not hasattr(plain[0], "verify")
    TOSs = [H.TrajectoryOptimizationSolution(t) for t in TOPs]
    out = H.solve_SCP_batch(TOSs, TOPs, verify=True)
    for b in range(6):
        assert np.array_equal(out[b].traj.X, plain[b].traj.X)
        r = V.report(0, out[b].traj.X.T, out[b].traj.U.T, 200.0, env, None)
        assert out[b].verify["collision_free"] == r["collision_free"] and _close(out[b].verify["min_dist_dense"], r["min_dist_dense"])


def test_c_program_through_the_verification_entry_points(tmp_path):
    """(6) tests/c/c_abi_verify.c, a plain C consumer with checks of its own; its report against np_verify."""
    exe = os.path.join(tmp_path, "c_abi_verify")
    lib = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_verify.c"), "-o", exe, "-L" + lib, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + lib])
    env = P.freeflyer_env()
    boxes = os.path.join(tmp_path, "boxes.txt")
    with open(boxes, "w") as f:
        f.write(f"{len(env)}\n" + "\n".join(" ".join(repr(float(v)) for v in row) for row in env) + "\n")
    out = subprocess.run([exe, boxes], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 3
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.6, 0.9, 0, 0, 0, 0]], float)
    goal = np.tile(P.FREEFLYER_X_GOAL, (2, 1))
    Xs, Us = straight_line(0, x0, goal, goal)
    for b, tf in enumerate((200.0, 100.0)):
        v = lines[1 + b].split()
        r = V.report(0, Xs[b], Us[b], tf, env, None)
        assert (int(v[0]), int(v[1]), int(v[6])) == (int(r["collision_free"]), r["first_knot"], r["min_dense_sample"])
        for got, k in zip((v[2], v[3], v[4], v[5], v[7]), DBL_FIELDS):
            assert _close(float(got), r[k]), (b, k, got, r[k])
