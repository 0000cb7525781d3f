"""gusto_lincov on the device against tests/np_lincov.py, the numpy restatement, and against gusto_simulate;
tests/test_lincov_cpu.py pins the restatement and the conditioning of the inputs without a GPU.

Inputs: tests/lincov_cases.py -- all four models at N = 3, 4, 50 with B = 5 problems, the three roll-out modes, three
environments (shared, empty, per problem with 0 .. 64 components) and two start covariances (default, full).

Tolerances: both sides are fp64 evaluations of the same finite formulas.  Each constant below is ten times the largest relative
error of its row, rounded up to a power of ten, every error taken against the restatement in np.longdouble, never against the
device: profiles/lincov.txt holds the values and where each comes from (tools/lincov_errors.py measures the device's).  Relative =
|a - ref|_max / |ref|_max per array per problem; margins of +-inf are compared exactly and left out of the norm.  The bit-for-bit
rows have no tolerance."""
import functools
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import lincov_cases as LC
import np_lincov as NL
import sim_cases as SC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TOL_KNOT = 1e-13       # profiles/lincov.txt 1(a), 2: sigma_x, sigma_u, z_obs, Sxx on the device's AB, K; the formulas' own fp64 error 2.8e-15
TOL_SUMMARY = 1e-11    # profiles/lincov.txt 1(a), 2: min_z_obs, min_z_ctl, p_collision_bound likewise; own error 2.3e-13 (erfc's tails)
TOL_END = 1e-11        # profiles/lincov.txt 2: every array against the restatement's own AB, K: gusto_tvlqr's 6e-15 over 49 knots
TOL_SIMULATE = 1e-11   # profiles/lincov.txt 2: Sxx against the second moment of gusto_simulate's closed-loop deviations

B = LC.B
KNOT_FIELDS = ("sigma_x", "sigma_u", "z_obs", "Sxx")
INDEX_FIELDS = ("status", "fail_knot", "obs_knot", "obs_pair", "ctl_knot", "ctl_entry")
SUMMARY_FIELDS = ("min_z_obs", "min_z_ctl", "p_collision_bound")
ALL_FIELDS = INDEX_FIELDS + SUMMARY_FIELDS + KNOT_FIELDS


def rel(a, ref):
    """|a - ref|_max / |ref|_max over the finite entries of ref; where ref is +-inf (or NaN), a must equal it exactly"""
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    fin = np.isfinite(ref)
    if not np.array_equal(a[~fin], ref[~fin], equal_nan=True):
        return np.inf
    if not fin.any():
        return 0.0
    nrm = np.abs(ref[fin]).max()
    err = np.abs(a[fin] - ref[fin]).max()
    return float(err / nrm) if nrm > 0 else float(err)


def solver(model, N, X, U, tf, which_env="empty", nb=None):
    s = g.BatchSolver(model, N, len(X), hist_cap=16)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    set_env(s, model, which_env, nb)
    return s


def set_env(s, model, which_env, idx=None):
    """the environment of a case on the handle; idx: the problems of the batch the handle holds (default: all five)"""
    sets, shared = LC.env(model, which_env)
    idx = range(B) if idx is None else idx
    if shared:
        s.set_env(*sets[0])
    else:
        s.set_env_batch([sets[b][0] for b in idx], [sets[b][1] for b in idx])


def tvlqr_opts(mode):
    Q, R, Qf = LC.WEIGHTS
    return dict(Q=Q, R=R, Qf=Qf, **LC.MODES[mode])


@functools.lru_cache(maxsize=None)
def device(model, N, mode):
    """one handle: the gains of gusto_tvlqr, then gusto_lincov with store_S = 1 for every environment and start covariance
    (computed once, shared, never written to)"""
    X, U, tf, _ = LC.inputs(model, N)
    s = solver(model, N, X, U, tf)
    tv = s.tvlqr(tvlqr_opts(mode), X, U)
    assert tv.status.all()
    out = {}
    for e in LC.ENVS:
        set_env(s, model, e)
        for st in LC.STARTS:
            out[e, st] = s.lincov(LC.options(model, N, mode, store_S=1), X, U, S0=LC.start(model, st))
            assert s.last_lincov_ms() > 0
            for a in out[e, st].values():
                a.setflags(write=False)
    s.close()
    return tv, out


def compare(dev, ref, b, tol_knot, tol_summary, where):
    for f in INDEX_FIELDS:
        assert dev[f][b] == ref[f], (where, f, dev[f][b], ref[f])
    for f in KNOT_FIELDS:
        e = rel(dev[f][b], ref[f])
        assert e <= tol_knot, (where, f, e)
    for f in SUMMARY_FIELDS:
        e = rel(dev[f][b], ref[f])
        assert e <= tol_summary, (where, f, e)


@pytest.mark.parametrize("model,N", LC.CASES)
def test_every_output_against_the_restatement_on_the_devices_jacobians_and_gains(model, N):
    """every per-knot array, Sxx, the summaries and (exactly) the indices, np_lincov fed with the device's AB and K: all roll-out
    modes, environments and start covariances"""
    for mode in range(len(LC.MODES)):
        tv, out = device(model, N, mode)
        for e in LC.ENVS:
            for st in LC.STARTS:
                ref = LC.reference(model, N, mode, e, st, tv.AB, tv.K)
                for b in range(B):
                    compare(out[e, st], ref[b], b, TOL_KNOT, TOL_SUMMARY, (model, N, mode, e, st, b))


@pytest.mark.parametrize("model,N", LC.CASES)
def test_end_to_end(model, N):
    """... against the restatement's own AB and K (complex-step Jacobians, the plain Riccati recursion)"""
    for mode in range(len(LC.MODES)):
        _, out = device(model, N, mode)
        for e, st in (("sim", "default"), ("batch", "full")):
            ref = LC.reference(model, N, mode, e, st)
            for b in range(B):
                compare(out[e, st], ref[b], b, TOL_END, TOL_END, (model, N, mode, e, st, b))


def second_moment_start(P):
    """S0 = sym(P'P / S) of perturbations P [S, n + m], symmetrised as 0.5 (S + S')"""
    M = P.T @ P / len(P)
    return 0.5 * (M + M.T)


def test_second_moment_of_gusto_simulate():
    """freeflyerSE2 is linear: without clipping the second moment of the closed-loop deviations Xcl[:, :, s] - Xcl[:, :, 0] of
    gusto_simulate is the image of the second moment of its perturbations, which is what gusto_lincov carries -- no statistics"""
    model, N, mode, S = 0, 50, 2, 257
    X, U, tf, _ = LC.inputs(model, N)
    s = solver(model, N, X, U, tf)
    assert s.tvlqr(tvlqr_opts(mode), X, U).status.all()
    P = SC.perturbation(model, S)
    s.simulate(dict(n_samples=S, store_knots=1, dense_collision=0, **LC.MODES[mode]), X, U, pert=P)
    Xcl = s.get_simulate_knots()                                        # [B, N, S, n]
    D = Xcl - Xcl[:, :, :1]
    M = np.einsum("bksi,bksj->bkij", D, D) / S
    S0 = np.stack([second_moment_start(P[b]) for b in range(B)])
    r = s.lincov(dict(store_S=1), X, U, S0=S0)
    s.close()
    assert r["status"].all()
    for b in range(B):
        e = max(rel(r["Sxx"][b, k], M[b, k]) for k in range(N))
        assert e <= TOL_SIMULATE, (b, e)


@pytest.mark.parametrize("model", LC.MODELS)
def test_bit_for_bit_rows(model):
    """Sxx symmetric; S_1 = S0 on the state block; store_S 0 and 1 agree on every shared output; K = NULL is the device's K
    passed back; a problem alone (B = 1) and in the batch of five"""
    N, mode = 50, 1
    X, U, tf, _ = LC.inputs(model, N)
    n = g.MODEL_DIMS[model][0]
    tv, out = device(model, N, mode)
    for (e, st), r in out.items():
        assert np.array_equal(r["Sxx"], np.swapaxes(r["Sxx"], -1, -2))
        S0 = LC.start(model, st)
        S1 = np.stack([NL.default_S0(model, SC.dx0(model), SC.du0(model))] * B) if S0 is None else S0
        assert np.array_equal(r["Sxx"][:, 0], S1[:, :n, :n])
    e, st = "batch", "full"
    s = solver(model, N, X, U, tf, e)
    s.tvlqr(tvlqr_opts(mode), X, U)
    o = LC.options(model, N, mode)
    r0 = s.lincov(o, X, U, S0=LC.start(model, st))
    assert "Sxx" not in r0
    rk = s.lincov(dict(o, store_S=1), X, U, K=tv.K, S0=LC.start(model, st))
    s.close()
    for f in ALL_FIELDS:
        assert f == "Sxx" or np.array_equal(r0[f], out[e, st][f]), f
        assert np.array_equal(rk[f], out[e, st][f]), f
    for j in (1, 3, 4):
        s1 = solver(model, N, X[j:j + 1], U[j:j + 1], tf[j:j + 1], e, [j])
        s1.tvlqr(tvlqr_opts(mode), X[j:j + 1], U[j:j + 1])
        r1 = s1.lincov(dict(o, store_S=1), X[j:j + 1], U[j:j + 1], S0=LC.start(model, st)[j:j + 1])
        s1.close()
        for f in ALL_FIELDS:
            assert np.array_equal(r1[f][0], out[e, st][f][j]), (f, j)


def test_mask_keeps_the_inactive_problem():
    """gusto_set_active: the active problems are what they are in the full batch, bit for bit; the inactive one is untouched by
    a second call with other options; a masked FIRST call after new problems leaves zeros for it"""
    model, N, mode, e, st = 2, 50, 0, "sim", "default"
    X, U, tf, _ = LC.inputs(model, N)
    _, out = device(model, N, mode)
    full = out[e, st]
    s = solver(model, N, X, U, tf, e)
    s.tvlqr(tvlqr_opts(mode), X, U)
    o = LC.options(model, N, mode, store_S=1)
    a = s.lincov(o, X, U)
    act = np.array([1, 1, 0, 1, 1], bool)
    s.set_active(act)
    b = s.lincov(dict(o, dx0=2 * SC.dx0(model)), X, U)
    for f in ALL_FIELDS:
        assert np.array_equal(a[f], full[f]), f
        assert np.array_equal(b[f][2], a[f][2]), f
    assert not np.array_equal(b["sigma_x"][1], a["sigma_x"][1])
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    s.set_active(None)
    s.tvlqr(tvlqr_opts(mode), X, U)
    s.set_active(act)
    c = s.lincov(o, X, U)
    for f in ALL_FIELDS:
        assert not np.asarray(c[f][2]).any(), f
        assert np.array_equal(c[f][act], full[f][act]), f
    s.set_active(None)
    s.close()


def test_failures_are_data():
    """a caller's K with a NaN at knot 2 of problem 3: status 0, fail_knot 2, zeros from there on, the other four problems
    unchanged to the bit; weights that make gusto_tvlqr fail: its fail_knot and zeros everywhere"""
    model, N, mode, e, st = 2, 50, 0, "sim", "default"
    X, U, tf, _ = LC.inputs(model, N)
    tv, out = device(model, N, mode)
    clean = out[e, st]
    Kn = tv.K.copy()
    Kn[3, 1, 2, 5] = np.nan
    s = solver(model, N, X, U, tf, e)
    s.tvlqr(tvlqr_opts(mode), X, U)
    r = s.lincov(LC.options(model, N, mode, store_S=1), X, U, K=Kn)
    assert list(r["status"]) == [1, 1, 1, 0, 1] and list(r["fail_knot"]) == [0, 0, 0, 2, 0]
    for f in KNOT_FIELDS:
        assert np.array_equal(r[f][3, :1], clean[f][3, :1]) and not r[f][3, 1:].any(), f
    # the summaries cover knot 1 alone
    assert r["obs_knot"][3] == 1 and r["ctl_knot"][3] == 1 and r["min_z_obs"][3] == clean["z_obs"][3, 0]
    for j in (0, 1, 2, 4):
        for f in ALL_FIELDS:
            assert np.array_equal(r[f][j], clean[f][j]), (f, j)
    # gusto_tvlqr fails where a NaN state enters its backward recursion (tests/test_gpu_tvlqr.py: test_failure_is_data)
    Xn = X.copy()
    Xn[2, N - 2, 10] = np.nan
    t = s.tvlqr(tvlqr_opts(mode), Xn, U)
    assert list(t.status) == [1, 1, 0, 1, 1] and t.fail_knot[2] == N - 1
    d = s.lincov(LC.options(model, N, mode, store_S=1), X, U)
    assert list(d["status"]) == [1, 1, 0, 1, 1] and d["fail_knot"][2] == N - 1
    for f in ALL_FIELDS:
        assert f in ("status", "fail_knot") or not np.asarray(d[f][2]).any(), f
    for j in (0, 1, 3, 4):
        for f in ALL_FIELDS:
            assert np.array_equal(d[f][j], clean[f][j]), (f, j)
    s.close()


def test_refusals_and_state():
    """TrajOpt handle; before set_problems; before gusto_tvlqr; every refused option and S0; X without U; Sxx after a call
    without store_S; after a new gusto_set_problems"""
    model, N = 0, 50
    X, U, tf, _ = LC.inputs(model, N)
    n, m = g.MODEL_DIMS[model]
    t = g._capi.TrajOptSolver(0, N, B)
    t.set_problems(X[:, 0], X[:, -1], X[:, -1], tf)
    with pytest.raises(g._capi.GustoError):
        t.lincov()
    assert t.L.gusto_lincov(t.h, None, None, None, None, None) == -1 and b"TrajOpt" in t.L.gusto_last_error(t.h)
    t.close()
    s = g.BatchSolver(model, N, B, hist_cap=16)
    assert s.L.gusto_lincov(s.h, None, None, None, None, None) == -3 and b"gusto_set_problems" in s.L.gusto_last_error(s.h)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.lincov()                                         # no gusto_tvlqr yet
    assert b"gusto_tvlqr" in s.L.gusto_last_error(s.h)
    s.tvlqr(tvlqr_opts(0), X, U)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_lincov()
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.last_lincov_ms()
    inf, nan = np.inf, np.nan
    neg = np.full(n, 0.01); neg[4] = -1e-3
    for bad in (dict(dx0=neg), dict(dx0=inf), dict(dx0=nan), dict(du0=-1.0), dict(du0=inf), dict(du_white=-1e-9), dict(du_white=nan),
                dict(du_white=inf), dict(u_lo=1.0, u_hi=0.5), dict(u_lo=nan), dict(u_hi=nan), dict(store_S=2), dict(store_S=-1)):
        with pytest.raises(g._capi.GustoError, match="-> -1"):
            s.lincov(bad)
    good = np.array(LC.full_S0(model))
    for i, j, v, word in ((2, 2, -1e-12, "negative"), (1, 3, nan, "finite"), (0, 0, inf, "finite"), (4, 7, 1e-3, "symmetric")):
        S0 = good.copy()
        S0[3, i, j] = v
        with pytest.raises(g._capi.GustoError, match="-> -1") as err:
            s.lincov(None, S0=S0)
        assert word in str(err.value) and "problem 3" in str(err.value) and "%d, %d" % (i, j) in str(err.value)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_lincov()                                     # (nothing was launched)
    assert s.L.gusto_lincov(s.h, X.ctypes.data, None, None, None, None) == -1
    assert s.L.gusto_lincov(s.h, None, U.ctypes.data, None, None, None) == -1
    # accepted edges: zero widths, infinite bounds, a symmetric S0 with a zero diagonal
    r = s.lincov(dict(dx0=0.0, du0=0.0, u_lo=-inf, u_hi=inf))
    assert r["status"].all() and not r["sigma_x"].any() and np.all(r["min_z_ctl"] == inf) and np.all(r["ctl_entry"] == -1)
    assert s.lincov(None, S0=np.zeros((B, n + m, n + m)))["status"].all()
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_lincov(Sxx=True)
    assert s.lincov(dict(store_S=1))["Sxx"].shape == (B, N, n, n) and s.get_lincov(Sxx=True)["Sxx"].shape == (B, N, n, n)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)   # new problems: the old results and Jacobians are gone
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_lincov()
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.lincov()
    s.close()


def test_zero_position_variance_and_the_handles_own_trajectories():
    """dx0 = 0 on the positions: sigma_d = 0 at knot 1, z_obs[1] = +inf outside the keep-out set; X = NULL reads the handle's
    trajectories and leaves them, the gains and the other stages' times alone"""
    model, N, mode, e = 0, 4, 0, "sim"
    X, U, tf, _ = LC.inputs(model, N)
    s = solver(model, N, X, U, tf, e)
    tv = s.tvlqr(tvlqr_opts(mode))
    ms = s.last_tvlqr_ms()
    w = SC.dx0(model).copy()
    w[:2] = 0.0
    own = s.lincov(dict(LC.options(model, N, mode, store_S=1), dx0=w))
    arr = s.lincov(dict(LC.options(model, N, mode, store_S=1), dx0=w), X, U)
    for f in ALL_FIELDS:
        assert np.array_equal(own[f], arr[f]), f
    ref = LC.reference(model, N, mode, e, "default", tv.AB, tv.K)
    d1 = np.array([r["d_pairs"][0].min() for r in ref])
    assert np.array_equal(own["z_obs"][:, 0], np.where(d1 >= 0, np.inf, -np.inf))
    X1, U1 = s.traj()
    t2 = s.get_tvlqr()
    assert np.array_equal(X1, X) and np.array_equal(U1, U) and np.array_equal(t2.K, tv.K) and s.last_tvlqr_ms() == ms
    s.close()


def test_host_mirror_and_export(tmp_path):
    """host.lincov on one trajectory against the restatement; export of sigma_x next to the gains"""
    H, P = g.host, g.problems
    import np_tvlqr as T
    model = H.FreeflyerSE2()
    gs = H.GoalSet()
    H.add_goal(gs, H.Goal(H.PointGoal(P.FREEFLYER_X_GOAL), 200.0, model))
    env = P.freeflyer_env()
    TOP = H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.Environment(env), P.freeflyer_random_x_init(1)[0], gs),
                                          50, 200.0, fixed_final_time=True)
    traj = H.init_traj_straightline(TOP)
    one = H.lincov(traj, H.SCPProblem(TOP), Q=2.0, R=0.5, Qf=3.0, dx0=0.02, du0=0.01, du_white=0.005)
    AB, K, _ = T.tvlqr(0, traj.X.T, traj.U.T, 200.0, 2.0, 0.5, 3.0)
    ref = NL.lincov(0, traj.X.T, traj.U.T, AB, K, None, 0.02, 0.01, 0.005, boxes=env)
    assert one["status"] == 1 and one["obs_knot"] == ref["obs_knot"] and one["obs_pair"] == ref["obs_pair"]
    assert rel(one["sigma_x"], ref["sigma_x"]) <= TOL_END and rel(one["z_obs"], ref["z_obs"]) <= TOL_END
    p = str(tmp_path / "one.npz")
    g.export.write(p, 0, traj.X.T, traj.U.T, 200.0, K=K, sigma=one["sigma_x"])
    assert np.array_equal(g.export.read(p)["traj"]["sigma_traj"], one["sigma_x"])


def test_c_program_through_the_lincov_entry_points(tmp_path):
    """tests/c/c_abi_lincov.c, a plain C consumer with checks of its own; the numbers it prints against the restatement"""
    from test_verify_cpu import straight_line
    import np_tvlqr as T
    exe = os.path.join(tmp_path, "c_abi_lincov")
    lib = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_lincov.c"), "-o", exe, "-L" + lib, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 3
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.6, 0.9, 0, 0, 0, 0]], float)
    goal = np.tile(g.problems.FREEFLYER_X_GOAL, (2, 1))
    Xs, Us = straight_line(0, x0, goal, goal)
    box = np.array([[1.4, 0.2, -0.2, 1.8, 0.6, 0.2]])
    for b, tf in enumerate((200.0, 100.0)):
        v = [float(x) for x in lines[1 + b].split()]
        AB, K, _ = T.tvlqr(0, Xs[b], Us[b], tf, 1.0, 1.0, 1.0)
        ref = NL.lincov(0, Xs[b], Us[b], AB, K, None, 0.02, 0.01, 0.005, -0.3 + 0.05 * np.arange(3), 0.4, boxes=box)
        assert (int(v[0]), int(v[1]), int(v[2]), int(v[3])) == (ref["obs_knot"], ref["obs_pair"], ref["ctl_knot"], ref["ctl_entry"])
        got = np.array(v[4:])
        want = np.array([ref["min_z_obs"], ref["p_collision_bound"], ref["min_z_ctl"], ref["sigma_x"][-1, 0], ref["sigma_u"][-1, 2]])
        assert np.all(np.abs(got - want) <= TOL_END * np.abs(want)), (got, want)
