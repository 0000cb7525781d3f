"""gusto_simulate on the device against tests/np_simulate.py, the numpy restatement in float64; tests/test_simulate_cpu.py pins
that restatement and the conditioning of the inputs without a GPU.

Inputs: tests/sim_cases.py -- np_tvlqr.smooth_batch, B = 5 problems of different tf, two spheres and a box next to the paths for
models 0, 2, 3; gains from the device's own gusto_tvlqr (and passed back explicitly: the same bits); S = 1, 63, 64, 65, 256, 257
at N = 3 and S = 65 at N = 50 and 65, over nstep = 1, nstep = 5, nstep = 0 with dt_min = 0.2, dense_collision 0 / 1, clipping off /
on, generated and caller-supplied perturbations.

Exact: the generated perturbations (the knot-1 states of store_knots are X_1 + p to the bit), the integer fields and the flags
of every sample whose reference is not within 1e-9 of a decision (at most 1 % are), and the report as the stated reduction of
the device's own per-sample arrays.

Tolerance: TOL is not taken from the device.  tools/simulate_errors.py measures on the CPU, over exactly these cases, the
largest relative difference between the float64 and the np.longdouble run of the restatement -- one rounding per operation:
  sample_min_dist 3.6e-14, x_final 5.2e-15, max_dev 7.1e-15, max_final_dev 7.3e-15, min_dist 5.4e-15, Xcl 4.0e-14
TOL is 100 x the largest, rounded up to a power of ten: the device contracts a x + b and orders its sums differently; two
decimal orders over a one-rounding-per-operation perturbation is the margin.  profiles/simulate.txt holds these values; the
device's own errors against the float64 restatement (tools/simulate_errors.py --device) are still to be measured there."""
import functools
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import np_simulate as NS
import sim_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL = 1e-11         # 100 x 4.0e-14 (tools/simulate_errors.py, float64 against longdouble), rounded up to a power of ten
REPORT_INT = ("n_free", "n_finite", "n_clipped", "worst_sample", "worst_dense_sample")
PER_SAMPLE = ("sample_min_dist", "sample_dense_index", "sample_flags", "x_final")


def _rel(a, ref):
    a, ref = np.asarray(a, float), np.asarray(ref, float)
    fin = np.isfinite(ref)
    assert np.array_equal(a[~fin], ref[~fin], equal_nan=True)
    return float(np.abs(a[fin] - ref[fin]).max() / np.abs(ref[fin]).max()) if fin.any() else 0.0


def _solver(model, N, X, U, tf, cap=None):
    boxes, spheres = SC.env(model)
    s = g.BatchSolver(model, N, cap or len(X), hist_cap=16, boxes=boxes, spheres=spheres)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    return s


def _opts(case, **more):
    model, N, S, mode, dense, clip, gen = case
    lo, hi = SC.bounds(model, clip)
    return dict(dict(n_samples=S, seed=SC.SEED, dx0=SC.dx0(model), du0=SC.du0(model), u_lo=lo, u_hi=hi, dense_collision=dense,
                     **SC.MODES[mode]), **more)


@functools.lru_cache(maxsize=None)
def device_and_reference(case):
    """(the device's report with store_knots, its Xcl, the restatement's results with the DEVICE's gains), computed once per
    case and shared.  Along the way: the gains passed explicitly give the bits of the handle's own, store_knots changes no result,
    generated and caller-supplied perturbations agree."""
    model, N, S, mode, dense, clip, gen = case
    X, U, tf, (Q, R, Qf) = SC.inputs(model, N)
    s = _solver(model, N, X, U, tf)
    K = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]), X, U).K
    pert = None if gen else SC.perturbation(model, S)
    r0 = s.simulate(_opts(case), X, U, pert=pert)
    assert s.last_simulate_ms() > 0
    r = s.simulate(_opts(case, store_knots=1), X, U, K=K, pert=pert)
    Xcl = s.get_simulate_knots()
    for k in r:
        assert np.array_equal(r[k], r0[k], equal_nan=True), (case, k)
    other = s.simulate(_opts(case), X, U, pert=SC.perturbation(model, S) if gen else None)
    for k in r:
        assert np.array_equal(r[k], other[k], equal_nan=True), (case, k)
    s.close()
    ref = SC.reference(case, K=K)
    return r, Xcl, ref


@pytest.mark.parametrize("case", SC.CASES, ids=lambda c: "m%d-N%d-S%d-mode%d-dense%d-clip%d-gen%d" % c)
def test_against_the_restatement(case):
    model, N, S, mode, dense, clip, gen = case
    r, Xcl, ref = device_and_reference(case)
    X = SC.inputs(model, N)[0]
    n = X.shape[2]
    # the perturbations, exactly: knot 1 of every sample is X_1 + p
    P = SC.perturbation(model, S)
    assert np.array_equal(Xcl[:, 0], X[:, None, 0, :] + P[:, :, :n])
    assert np.array_equal(Xcl[:, N - 1], r["x_final"])
    left_out = 0
    for b in range(SC.B):
        q = ref[b]
        ok = ~SC.undecided(q)
        left_out += int((~ok).sum())
        assert np.array_equal(r["sample_flags"][b][ok], q["sample_flags"][ok]), (case, b)
        assert np.array_equal(r["sample_dense_index"][b][ok], q["sample_dense_index"][ok]), (case, b)
        if ok.all():
            for k in REPORT_INT:
                assert r[k][b] == q[k], (case, b, k, r[k][b], q[k])
        for k in ("sample_min_dist", "x_final", "max_dev", "max_final_dev", "min_dist"):
            e = _rel(r[k][b], q[k])
            assert e <= TOL, (case, b, k, e)
        e = _rel(Xcl[b], q["Xcl"])
        assert e <= TOL, (case, b, "Xcl", e)
        # the report is the stated reduction of the device's own per-sample arrays
        own = NS.report(r["sample_min_dist"][b], r["sample_dense_index"][b], r["sample_flags"][b], r["x_final"][b],
                        np.abs(Xcl[b] - X[b][:, None, :]).max(axis=0), X[b, N - 1])
        for k in REPORT_INT:
            assert r[k][b] == own[k], (case, b, k)
        assert r["min_dist"][b] == own["min_dist"]
        assert np.array_equal(r["max_dev"][b], own["max_dev"]) and np.array_equal(r["max_final_dev"][b], own["max_final_dev"])
        assert np.array_equal((r["sample_flags"][b] & 1) != 0, r["sample_min_dist"][b] < 0)
    assert left_out <= 0.01 * SC.B * S, (case, left_out)


BITS = [c for c in SC.CASES if (c[1], c[2]) in ((3, 257), (50, 65))]


@pytest.mark.parametrize("case", BITS, ids=lambda c: "m%d-N%d-S%d" % c[:3])
def test_a_result_does_not_depend_on_the_batch_or_the_call(case):
    """a problem alone against the same problem inside the batch; two calls; first_problem sharding (handles of 2 and 3 problems
    against one of 5); an active mask keeps the inactive problems' earlier results -- all bit for bit"""
    model, N, S, mode, dense, clip, gen = case
    X, U, tf, _ = SC.inputs(model, N)
    r, _, _ = device_and_reference(case)
    K = None
    parts = []
    for lo, hi in ((0, 2), (2, 5)):
        s = _solver(model, N, X[lo:hi], U[lo:hi], tf[lo:hi])
        Q, R, Qf = SC.WEIGHTS
        s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]))
        pert = None if gen else SC.perturbation(model, S)[lo:hi]
        parts.append(s.simulate(_opts(case, first_problem=lo), pert=pert))
        again = s.simulate(_opts(case, first_problem=lo), pert=pert)
        for k in again:
            assert np.array_equal(again[k], parts[-1][k], equal_nan=True), k
        if lo == 2:   # problems 2 and 4 only, with other bounds: problem 3 keeps what it had
            s.set_active(np.array([1, 0, 1], bool))
            m = s.simulate(_opts(case, first_problem=lo, u_lo=-1e-3, u_hi=1e-3), pert=pert)
            for k in m:
                assert np.array_equal(m[k][1], again[k][1], equal_nan=True), k
            assert (m["n_clipped"][[0, 2]] == S).all() and not np.array_equal(m["x_final"][0], again["x_final"][0])
            s.set_active(None)
        s.close()
    for k in r:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), r[k], equal_nan=True), k
    j = 3
    s = _solver(model, N, X[j:j + 1], U[j:j + 1], tf[j:j + 1])
    Q, R, Qf = SC.WEIGHTS
    s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]))
    one = s.simulate(_opts(case, first_problem=j), pert=None if gen else SC.perturbation(model, S)[j:j + 1])
    s.close()
    for k in r:
        assert np.array_equal(one[k][0], r[k][j], equal_nan=True), k


def test_nonfinite_samples_are_flagged_counted_and_kept_out():
    """problem 2 gets gains of 1e200 from the caller: its perturbed samples go non-finite (bit 2, as the restatement says), n_finite
    counts the rest, no NaN reaches a minimum or maximum, the other problems are what they are without it, bit for bit"""
    case = next(c for c in SC.CASES if c[:3] == (2, 50, 65))
    model, N, S, mode, dense, clip, gen = case
    X, U, tf, (Q, R, Qf) = SC.inputs(model, N)
    s = _solver(model, N, X, U, tf)
    K = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]), X, U).K
    P = SC.perturbation(model, S)
    clean = s.simulate(_opts(case), X, U, K=K, pert=P)
    Kb = K.copy()
    Kb[2] = 1e200
    r = s.simulate(_opts(case), X, U, K=Kb, pert=P)
    s.close()
    lo, hi = SC.bounds(model, clip)
    boxes, spheres = SC.env(model)
    q = NS.simulate(model, X[2], U[2], Kb[2], tf[2], P[2], lo, hi, boxes, spheres, dense_collision=bool(dense), **SC.MODES[mode])
    assert ((r["sample_flags"][2, 1:] & 4) != 0).all()
    assert np.array_equal(r["sample_flags"][2] & 4, q["sample_flags"] & 4)
    assert r["n_finite"][2] == q["n_finite"] == int(((r["sample_flags"][2] & 4) == 0).sum())
    assert r["n_free"][2] <= r["n_finite"][2]
    assert not np.isnan(r["min_dist"]).any() and np.isfinite(r["max_dev"]).all() and np.isfinite(r["max_final_dev"]).all()
    for j in (0, 1, 3, 4):
        for k in r:
            assert np.array_equal(r[k][j], clean[k][j], equal_nan=True), (k, j)


def test_after_a_real_solve():
    """freeflyerSE2, B = 64, N = 50: solve, tvlqr, simulate with X = U = K = None.  Trajectories, status, histories and the solve
    time are what they were; the results are those of the restatement fed with get_traj and get_tvlqr -- sample 0's deviation at
    the knots among them, which is the open-loop gap of gusto_verify carried through the closed loop"""
    from test_verify_cpu import batch
    model, Bs, N, S = 0, 64, 50, 64
    x0, glo, ghi, tf, boxes, spheres = batch(model, Bs)
    s = g.BatchSolver(model, N, Bs, hist_cap=64, boxes=boxes, spheres=spheres)
    s.set_problems(x0, glo, ghi, tf)
    s.solve(30)
    ms = s.last_solve_ms()
    X, U = s.traj()
    st, h = s.status(), s.history()
    gap = s.verify()["max_gap"]
    K = s.tvlqr().K
    o = dict(n_samples=S, seed=7, dx0=[0.02, 0.02, 0.05, 0.005, 0.005, 0.01], store_knots=1)
    r = s.simulate(o)
    Xcl = s.get_simulate_knots()
    X1, U1 = s.traj()
    st1, h1 = s.status(), s.history()
    assert np.array_equal(X, X1) and np.array_equal(U, U1) and s.last_solve_ms() == ms
    assert all(np.array_equal(st[k], st1[k]) for k in st) and all(np.array_equal(h[k], h1[k], equal_nan=True) for k in h)
    arr = s.simulate(o, X, U, K=K)
    s.close()
    for k in r:
        assert np.array_equal(r[k], arr[k], equal_nan=True), k
    P = NS.perturbations(model, Bs, S, o["dx0"], 0.0, 7)
    for b in range(0, Bs, 7):
        q = NS.simulate(model, X[b], U[b], K[b], tf[b], P[b], boxes=boxes, spheres=spheres)
        d0, want = np.abs(Xcl[b, :, 0] - X[b]).max(axis=1), np.abs(q["Xcl"][:, 0] - X[b]).max(axis=1)
        assert np.abs(d0 - want).max() <= TOL * max(1.0, np.abs(X[b]).max()), b
        assert d0[0] == 0.0 and (gap[b] == 0 or d0.max() > 0)
        for k in ("sample_min_dist", "x_final", "max_dev"):
            assert _rel(r[k][b], q[k]) <= TOL, (b, k)
        ok = ~((np.abs(q["sample_min_dist"]) < SC.BAND))
        assert np.array_equal(r["sample_flags"][b][ok], q["sample_flags"][ok])


def test_refusals():
    """each with its code and a text in gusto_last_error"""
    case = next(c for c in SC.CASES if c[:3] == (0, 50, 65))
    model, N, S = case[:3]
    X, U, tf, (Q, R, Qf) = SC.inputs(model, N)
    L = g.lib()
    t = g._capi.TrajOptSolver(0, N, SC.B)
    t.set_problems(X[:, 0], X[:, -1], X[:, -1], tf)
    with pytest.raises(g._capi.GustoError):
        t.simulate()
    assert L.gusto_simulate(t.h, None, None, None, None, None) == -1 and b"TrajOpt" in L.gusto_last_error(t.h)
    t.close()
    s = g.BatchSolver(model, N, SC.B, hist_cap=16)
    assert L.gusto_simulate(s.h, None, None, None, None, None) == -3 and b"gusto_set_problems" in L.gusto_last_error(s.h)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    assert L.gusto_simulate(s.h, None, None, None, None, None) == -3 and b"gusto_tvlqr" in L.gusto_last_error(s.h)   # no gains
    for call in (s.get_simulate, s.get_simulate_knots, s.last_simulate_ms):
        with pytest.raises(g._capi.GustoError, match="-> -3"):
            call()
    K = s.tvlqr(dict(Q=Q, R=R, Qf=Qf)).K
    lo, hi = np.full(3, -1.0), np.full(3, 1.0)
    hi[1] = -2.0
    neg = np.full(6, 0.01)
    neg[4] = -1e-3
    need = int(np.ceil(SC.DT.max() / 0.05))
    for bad, text in ((dict(n_samples=0), b"n_samples"), (dict(n_samples=4097), b"n_samples"), (dict(u_lo=lo, u_hi=hi), b"u_lo"),
                      (dict(u_lo=np.nan), b"u_lo"), (dict(dx0=neg), b"dx0"), (dict(du0=-1.0), b"du0"), (dict(dx0=np.inf), b"dx0"),
                      (dict(dt_min=0.05, nstep_cap=need - 1), b"substeps"), (dict(nstep=65), b"nstep_cap"), (dict(nstep=-1), b"bad options"),
                      (dict(dt_min=0.0), b"bad options"), (dict(dense_collision=2), b"bad options"), (dict(store_knots=-1), b"bad options")):
        with pytest.raises(g._capi.GustoError, match="-> -1"):
            s.simulate(bad)
        assert text in L.gusto_last_error(s.h), (bad, L.gusto_last_error(s.h))
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_simulate()                                       # (nothing was launched)
    assert L.gusto_simulate(s.h, X.ctypes.data, None, None, None, None) == -1 and b"together" in L.gusto_last_error(s.h)
    assert L.gusto_simulate(s.h, None, U.ctypes.data, None, None, None) == -1
    assert L.gusto_simulate(None, None, None, None, None, None) == -1 and L.gusto_get_simulate(None, None) == -1
    assert L.gusto_get_simulate_knots(None, None) == -1 and L.gusto_last_simulate_ms(s.h, None) == -1
    assert L.gusto_default_simulate_opts(0, None) == -1 and L.gusto_default_simulate_opts(9, g.SimulateOpts()) == -1
    r = s.simulate(dict(n_samples=3, dt_min=0.05, nstep_cap=need), K=K)
    assert r["n_finite"].tolist() == [3] * SC.B and L.gusto_get_simulate(s.h, None) == -1
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_simulate_knots()                                 # (the call ran without store_knots)
    assert b"store_knots" in L.gusto_last_error(s.h)
    s.simulate(dict(n_samples=3, store_knots=1))
    assert s.get_simulate_knots().shape == (SC.B, N, 3, 6)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)     # new problems: the old results and gains are gone
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_simulate()
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.simulate()
    s.close()


def test_host_mirror_and_batch_option():
    """host.simulate on one trajectory; solve_SCP_batch(..., tvlqr=, simulate=) over two shards draws what one shard draws"""
    H, P = g.host, g.problems
    env = P.freeflyer_env()
    x0 = P.freeflyer_random_x_init(4)
    TOPs = []
    for b in range(4):
        model = H.FreeflyerSE2()
        gs = H.GoalSet()
        H.add_goal(gs, H.Goal(H.PointGoal(P.FREEFLYER_X_GOAL), 200.0, model))
        TOPs.append(H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.Environment(env), x0[b], gs), 50, 200.0,
                                                    fixed_final_time=True))
    with pytest.raises(ValueError):
        H.solve_SCP_batch([H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs, max_iter=3, simulate={})
    lq, sim = dict(Q=10.0, R=1.0, Qf=10.0), dict(n_samples=5, seed=3)
    one = H.solve_SCP_batch([H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs, max_iter=3, tvlqr=lq, simulate=sim)
    two = H.solve_SCP_batch([H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs, max_iter=3, tvlqr=lq, simulate=sim, devices=[0, 0])
    for b in range(4):
        for k in one[b].simulate:
            assert np.array_equal(one[b].simulate[k], two[b].simulate[k], equal_nan=True), (b, k)
        assert one[b].simulate["n_finite"] == 5 and one[b].simulate["x_final"].shape == (5, 6)
    traj = H.init_traj_straightline(TOPs[1])
    r = H.simulate(traj, H.SCPProblem(TOPs[1]), Q=10.0, R=1.0, Qf=10.0, n_samples=5, seed=3)
    assert r["n_finite"] == 5 and r["sample_flags"].shape == (5,) and not r["x_final"][0].tolist() == r["x_final"][1].tolist()


def test_c_program_through_the_simulate_entry_points(tmp_path):
    """tests/c/c_abi_simulate.c, a plain C consumer with checks of its own; the numbers it prints against the restatement"""
    from test_verify_cpu import straight_line
    import np_tvlqr as T
    exe = os.path.join(tmp_path, "c_abi_simulate")
    lib = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_simulate.c"), "-o", exe, "-L" + lib, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 3
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.6, 0.9, 0, 0, 0, 0]], float)
    goal = np.tile(np.array([3.0, 0.5, 0, 0.05, -0.05, 0]), (2, 1))
    Xs, Us = straight_line(0, x0, goal, goal)
    P = NS.perturbations(0, 2, 8, 0.01, 0.0, 11)
    for b, tf in enumerate((200.0, 100.0)):
        v = np.array([float(x) for x in lines[1 + b].split()])
        _, K, _ = T.tvlqr(0, Xs[b], Us[b], tf, 1.0, 1.0, 1.0)
        q = NS.simulate(0, Xs[b], Us[b], K, tf, P[b], u_lo=-0.05, u_hi=0.05, boxes=[[1.0, 0.6, -1.0, 1.2, 0.8, 1.0]])
        assert np.abs(v[:6] - q["x_final"][7]).max() <= TOL * np.abs(q["x_final"]).max()
        assert abs(v[6] - q["min_dist"]) <= TOL * abs(q["min_dist"]) and int(v[7]) == q["n_free"] and int(v[8]) == q["n_clipped"]
