"""gusto_tvlqr on the device against tests/np_tvlqr.py, the numpy restatement (complex-step Jacobians of the RK4 roll-out, the
plain Riccati recursion); tests/test_tvlqr_cpu.py pins that restatement without a GPU.

Inputs: np_tvlqr.smooth_batch -- a straight line plus seeded sinusoids, controls of the size of the models' limits, the
manifold quaternion normalised at the knots -- and np_tvlqr.weights, diagonal Q, R, Qf spanning 1e-2 .. 1e2.  Shapes: every
model at N = 3, 50, 64, 65 with B = 5 problems of different tf, rolled out with nstep = 1, nstep = 5 and nstep = 0 (dt_min = 0.2:
three substeps for four of the problems, four for the other).

Tolerances: both sides are fp64 evaluations of the same finite formulas, so a difference is rounding times the conditioning of
the recursion.  Each constant below is ten times the largest relative error measured on an MI355X over all cases of its row,
rounded up to a power of ten; tools/tvlqr_errors.py measures them, profiles/tvlqr.txt holds the values.  Every error is taken against the numpy
restatement.  The bit-for-bit rows have no tolerance."""
import functools
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import np_tvlqr as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL_AB = 1e-14         # profiles/tvlqr.txt: AB against the complex step, worst 6.3e-16
TOL_RICCATI = 1e-13    # profiles/tvlqr.txt: K, P against the numpy recursion on the device's AB, worst 4.2e-15 (K), 5.1e-15 (P)
TOL_END = 1e-13        # profiles/tvlqr.txt: K, P_1 against the restatement's own AB and recursion, worst 4.2e-15 (K), 4.1e-15 (P_1)
TOL_IDENTITY = 1e-14   # profiles/tvlqr.txt: Riccati identity residual / |P_k|, worst 1.0e-15

MODELS = (0, 1, 2, 3)
HORIZONS = (3, 50, 64, 65)
B = 5
DT = np.array([0.5, 0.58, 0.45, 0.7, 0.55])       # dt of the five problems; dt_min = 0.2 gives 3, 3, 3, 4, 3 substeps
MODES = (dict(nstep=1), dict(nstep=5), dict(nstep=0, dt_min=0.2))


def _rel(a, ref):
    return np.abs(a - ref).max() / np.abs(ref).max()


def _solver(model, N, X, U, tf):
    s = g.BatchSolver(model, N, len(X), hist_cap=16)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    return s


@functools.lru_cache(maxsize=None)
def _inputs(model, N):
    X, U = T.smooth_batch(model, B, N)
    return X, U, DT * (N - 1), T.weights(model)


@functools.lru_cache(maxsize=None)
def _reference(model, N, mode):
    """the restatement's AB, K, P of the five problems (computed once, shared, never written to)"""
    X, U, tf, (Q, R, Qf) = _inputs(model, N)
    out = [T.tvlqr(model, X[b], U[b], tf[b], Q, R, Qf, **MODES[mode]) for b in range(B)]
    res = tuple(np.stack([o[i] for o in out]) for i in range(3))
    for a in res:
        a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def _device(model, N, mode):
    """(result without store_P, result with store_P) of one handle"""
    X, U, tf, (Q, R, Qf) = _inputs(model, N)
    s = _solver(model, N, X, U, tf)
    o = dict(Q=Q, R=R, Qf=Qf, **MODES[mode])
    r0 = s.tvlqr(o, X, U)
    assert s.last_tvlqr_ms() > 0
    r1 = s.tvlqr(dict(o, store_P=1), X, U)
    s.close()
    assert r0.P.shape == (B, s.n, s.n) and r1.P.shape == (B, N, s.n, s.n)
    assert r0.status.all() and r1.status.all() and not r0.fail_knot.any() and not r1.fail_knot.any()
    return r0, r1


CASES = [(m, N) for m in MODELS for N in HORIZONS]


@pytest.mark.parametrize("model,N", CASES)
def test_jacobians_against_the_complex_step(model, N):
    """AB = [Ad | Bd] of every interval against the complex step through the whole roll-out"""
    for mode in range(len(MODES)):
        AB = _reference(model, N, mode)[0]
        r0, r1 = _device(model, N, mode)
        assert np.array_equal(r0.AB, r1.AB)
        err = max(_rel(r0.AB[b, k], AB[b, k]) for b in range(B) for k in range(N - 1))
        assert err <= TOL_AB, (model, N, mode, err)


@pytest.mark.parametrize("model,N", CASES)
def test_riccati_stage_alone(model, N):
    """K and P against the numpy recursion fed with the DEVICE's AB, without and with store_P"""
    _, _, _, (Q, R, Qf) = _inputs(model, N)
    for mode in range(len(MODES)):
        r0, r1 = _device(model, N, mode)
        assert np.array_equal(r0.K, r1.K) and np.array_equal(r0.P, r1.P[:, 0])
        for b in range(B):
            K, P = T.riccati(r1.AB[b], Q, R, Qf)
            assert np.array_equal(r1.P[b, N - 1], np.diag(Qf))
            eK = _rel(r1.K[b], K)
            eP = max(_rel(r1.P[b, k], P[k]) for k in range(N))
            assert eK <= TOL_RICCATI and eP <= TOL_RICCATI, (model, N, mode, b, eK, eP)


@pytest.mark.parametrize("model,N", CASES)
def test_end_to_end(model, N):
    """K and P of knot 1 against the restatement's own AB and recursion"""
    for mode in range(len(MODES)):
        _, K, P = _reference(model, N, mode)
        r0, _ = _device(model, N, mode)
        for b in range(B):
            eK, eP = _rel(r0.K[b], K[b]), _rel(r0.P[b], P[b, 0])
            assert eK <= TOL_END and eP <= TOL_END, (model, N, mode, b, eK, eP)


@pytest.mark.parametrize("model,N", CASES)
def test_riccati_identity(model, N):
    """with store_P: P_k = Q + Ad' P_{k+1} (Ad - Bd K_k) relative to |P_k|; P_k symmetric to the bit; no eigenvalue below
    -TOL_IDENTITY |P_k|"""
    n, _ = g.MODEL_DIMS[model]
    _, _, _, (Q, R, Qf) = _inputs(model, N)
    for mode in range(len(MODES)):
        _, r1 = _device(model, N, mode)
        for b in range(B):
            for k in range(N - 1):
                A, Bd, Pk = r1.AB[b, k, :, :n], r1.AB[b, k, :, n:], r1.P[b, k]
                nrm = np.abs(Pk).max()
                res = np.abs(Pk - (np.diag(Q) + A.T @ r1.P[b, k + 1] @ (A - Bd @ r1.K[b, k]))).max() / nrm
                assert res <= TOL_IDENTITY, (model, N, mode, b, k, res)
                assert np.array_equal(Pk, Pk.T)
                assert np.linalg.eigvalsh(Pk).min() >= -TOL_IDENTITY * nrm


def test_phase_times_of_the_development_hook():
    """gusto_dev_tvlqr: the two launches' times add up to the call's"""
    X, U, tf, _ = _inputs(0, 50)
    s = _solver(0, 50, X, U, tf)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.tvlqr_phase_ms()
    assert s.tvlqr().status.all()
    lin, ric = s.tvlqr_phase_ms()
    assert lin > 0 and ric > 0 and lin + ric <= s.last_tvlqr_ms() * 1.001 + 1e-6
    assert s.L.gusto_dev_tvlqr(None, None, None) == -1
    s.close()


@pytest.mark.parametrize("model", MODELS)
def test_a_result_does_not_depend_on_the_batch(model):
    """problem j of the B = 5 batch equals, bit for bit, the same problem alone and at another index"""
    N, mode = 50, 2
    X, U, tf, (Q, R, Qf) = _inputs(model, N)
    o = dict(Q=Q, R=R, Qf=Qf, store_P=1, **MODES[mode])
    _, r = _device(model, N, mode)
    perm = np.array([3, 4, 0, 1, 2])
    s = _solver(model, N, X[perm], U[perm], tf[perm])
    rp = s.tvlqr(o, X[perm], U[perm])
    s.close()
    for name in ("K", "P", "AB", "status", "fail_knot"):
        assert np.array_equal(getattr(rp, name), getattr(r, name)[perm]), name
    for j in (1, 3):
        s = _solver(model, N, X[j:j + 1], U[j:j + 1], tf[j:j + 1])
        r1 = s.tvlqr(o, X[j:j + 1], U[j:j + 1])
        s.close()
        for name in ("K", "P", "AB", "status", "fail_knot"):
            assert np.array_equal(getattr(r1, name)[0], getattr(r, name)[j]), (name, j)


def test_mask_keeps_the_inactive_problem():
    """gusto_set_active: the inactive problem keeps the first call's outputs, its neighbours follow the changed weights; a masked
    FIRST call after new problems leaves zeros for the inactive problem"""
    model, N = 2, 50
    X, U, tf, (Q, R, Qf) = _inputs(model, N)
    s = _solver(model, N, X, U, tf)
    a = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, nstep=1, store_P=1), X, U)
    act = np.array([1, 1, 0, 1, 1], bool)
    s.set_active(act)
    b = s.tvlqr(dict(Q=Qf, R=2 * R, Qf=Q, nstep=1, store_P=1), X, U)
    for name in ("K", "P", "AB", "status", "fail_knot"):
        assert np.array_equal(getattr(b, name)[2], getattr(a, name)[2]), name
    assert np.array_equal(b.AB, a.AB)
    for j in (1, 3):
        assert not np.array_equal(b.K[j], a.K[j])
        K, P = T.riccati(b.AB[j], Qf, 2 * R, Q)
        assert _rel(b.K[j], K) <= TOL_RICCATI and _rel(b.P[j, 0], P[0]) <= TOL_RICCATI
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    s.set_active(act)
    c = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, nstep=1, store_P=1), X, U)
    assert not c.K[2].any() and not c.P[2].any() and not c.AB[2].any() and c.status[2] == 0
    assert np.array_equal(c.K[act], a.K[act]) and np.array_equal(c.P[act], a.P[act])
    s.set_active(None)
    s.close()


@pytest.mark.parametrize("model", [0, 2])
def test_the_handles_own_trajectories(model):
    """after solve(3): tvlqr(X = NULL) equals tvlqr of the arrays get_traj returns, bit for bit; trajectories, status, histories
    and the solve time are what they were"""
    from test_verify_cpu import batch
    Bs, N = 4, 50
    x0, glo, ghi, tf, boxes, spheres = batch(model, Bs)
    s = g.BatchSolver(model, N, Bs, hist_cap=16, boxes=boxes, spheres=spheres)
    s.set_problems(x0, glo, ghi, tf)
    s.solve(3)
    ms = s.last_solve_ms()
    X, U = s.traj()
    st, h = s.status(), s.history()
    Q, R, Qf = T.weights(model)
    o = dict(Q=Q, R=R, Qf=Qf, store_P=1, nstep=4)
    own = s.tvlqr(o)
    X1, U1 = s.traj()
    st1, h1 = s.status(), s.history()
    assert np.array_equal(X, X1) and np.array_equal(U, U1) and s.last_solve_ms() == ms
    assert all(np.array_equal(st[k], st1[k]) for k in st) and all(np.array_equal(h[k], h1[k], equal_nan=True) for k in h)
    arr = s.tvlqr(o, X, U)
    for name in ("K", "P", "AB", "status", "fail_knot"):
        assert np.array_equal(getattr(own, name), getattr(arr, name)), name
    assert own.status.all() and np.abs(own.K).max() > 0
    s.close()


def test_failure_is_data():
    """one NaN in problem 2's state at the start of the last interval: that problem has status 0, fail_knot N - 1 and zero
    gains; the other problems are what they are without it, bit for bit"""
    model, N = 2, 50
    X, U, tf, (Q, R, Qf) = _inputs(model, N)
    _, clean = _device(model, N, 0)
    Xn = X.copy()
    Xn[2, N - 2, 10] = np.nan
    s = _solver(model, N, X, U, tf)
    r = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, store_P=1, **MODES[0]), Xn, U)
    s.close()
    assert list(r.status) == [1, 1, 0, 1, 1] and list(r.fail_knot) == [0, 0, N - 1, 0, 0]
    assert not r.K[2].any() and not r.P[2, :N - 1].any() and np.array_equal(r.P[2, N - 1], np.diag(Qf))
    for j in (0, 1, 3, 4):
        for name in ("K", "P", "AB"):
            assert np.array_equal(getattr(r, name)[j], getattr(clean, name)[j]), (name, j)


def test_refusals():
    """TrajOpt handle; before set_problems; R with a zero; Q negative; nstep_cap one below the need; X without U; the full P
    after a call without store_P"""
    model, N = 0, 50
    X, U, tf, (Q, R, Qf) = _inputs(model, N)
    t = g._capi.TrajOptSolver(0, N, B)
    t.set_problems(X[:, 0], X[:, -1], X[:, -1], tf)
    with pytest.raises(g._capi.GustoError):
        t.tvlqr()
    assert t.L.gusto_tvlqr(t.h, None, None, None) == -1 and b"TrajOpt" in t.L.gusto_last_error(t.h)
    t.close()
    s = g.BatchSolver(model, N, B, hist_cap=16)
    assert s.L.gusto_tvlqr(s.h, None, None, None) == -3 and b"gusto_set_problems" in s.L.gusto_last_error(s.h)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_tvlqr()
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.last_tvlqr_ms()
    R0, Qn = R.copy(), Q.copy()
    R0[1], Qn[4] = 0.0, -1e-3
    need = int(np.ceil(DT.max() / 0.05))
    for bad in (dict(R=R0), dict(Q=Qn), dict(Qf=Qn), dict(Q=np.full(6, np.nan)), dict(dt_min=0.05, nstep_cap=need - 1), dict(nstep=65),
                dict(nstep=-1), dict(dt_min=0.0), dict(store_P=2)):
        with pytest.raises(g._capi.GustoError, match="-> -1"):
            s.tvlqr(bad)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_tvlqr()                                      # (nothing was launched)
    assert s.tvlqr(dict(dt_min=0.05, nstep_cap=need)).status.all()
    assert s.L.gusto_tvlqr(s.h, X.ctypes.data, None, None) == -1 and s.L.gusto_tvlqr(s.h, None, U.ctypes.data, None) == -1
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_tvlqr(full_P=True)
    assert s.tvlqr(dict(store_P=1)).P.shape == (B, N, 6, 6) and s.get_tvlqr(full_P=True).P.shape == (B, N, 6, 6)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)   # new problems: the old gains are gone
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_tvlqr()
    s.close()


def test_host_mirror_batch_option_and_export(tmp_path):
    """host.tvlqr on one trajectory, solve_SCP_batch(..., tvlqr=opts), export of the gains"""
    H, P = g.host, g.problems
    env = P.freeflyer_env()
    x0 = P.freeflyer_random_x_init(3)
    TOPs = []
    for b in range(3):
        model = H.FreeflyerSE2()
        gs = H.GoalSet()
        H.add_goal(gs, H.Goal(H.PointGoal(P.FREEFLYER_X_GOAL), 200.0, model))
        TOPs.append(H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.Environment(env), x0[b], gs), 50, 200.0,
                                                    fixed_final_time=True))
    traj = H.init_traj_straightline(TOPs[1])
    one = H.tvlqr(traj, H.SCPProblem(TOPs[1]), Q=2.0, R=0.5, Qf=3.0)
    AB, K, Pn = T.tvlqr(0, traj.X.T, traj.U.T, 200.0, 2.0, 0.5, 3.0)
    assert one.status == 1 and _rel(one.K, K) <= TOL_END and _rel(one.P, Pn[0]) <= TOL_END and _rel(one.AB, AB) <= TOL_AB
    plain = H.solve_SCP_batch([H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs, max_iter=3)
    assert not hasattr(plain[0], "tvlqr")
    out = H.solve_SCP_batch([H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs, max_iter=3, tvlqr=dict(Q=2.0, R=0.5, Qf=3.0))
    for b in range(3):
        assert np.array_equal(out[b].traj.X, plain[b].traj.X)
        _, K, Pn = T.tvlqr(0, out[b].traj.X.T, out[b].traj.U.T, 200.0, 2.0, 0.5, 3.0)
        assert out[b].tvlqr.status == 1 and _rel(out[b].tvlqr.K, K) <= TOL_END and _rel(out[b].tvlqr.P, Pn[0]) <= TOL_END
    p = str(tmp_path / "one.npz")
    g.export.write(p, 0, out[0].traj.X.T, out[0].traj.U.T, 200.0, K=out[0].tvlqr.K)
    assert np.array_equal(g.export.read(p)["traj"]["k_traj"], out[0].tvlqr.K)


def test_c_program_through_the_tvlqr_entry_points(tmp_path):
    """tests/c/c_abi_tvlqr.c, a plain C consumer with checks of its own; the gains it prints against the restatement"""
    from test_verify_cpu import straight_line
    exe = os.path.join(tmp_path, "c_abi_tvlqr")
    lib = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_tvlqr.c"), "-o", exe, "-L" + lib, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 3
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.6, 0.9, 0, 0, 0, 0]], float)
    goal = np.tile(g.problems.FREEFLYER_X_GOAL, (2, 1))
    Xs, Us = straight_line(0, x0, goal, goal)
    Q, R, Qf = np.ones(6), np.ones(3), np.ones(6)
    Q[0], R[2], Qf[5] = 4.0, 0.5, 9.0
    for b, tf in enumerate((200.0, 100.0)):
        v = np.array([float(x) for x in lines[1 + b].split()])
        _, K, Pn = T.tvlqr(0, Xs[b], Us[b], tf, Q, R, Qf)
        assert np.abs(v[:6] - K[0, 0]).max() <= TOL_END * np.abs(K[0]).max() and abs(v[6] - Pn[0, 0, 0]) <= TOL_END * np.abs(Pn[0]).max()
