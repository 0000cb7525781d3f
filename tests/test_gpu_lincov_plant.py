"""gusto_lincov_disturbed on the device against tests/np_lincov_plant.py, the numpy restatement, against gusto_simulate_disturbed and
against gusto_lincov; tests/test_lincov_plant_cpu.py pins the restatement and the conditioning of the inputs without a GPU.

Inputs: tests/lincov_plant_cases.py -- lincov_cases (four models, N = 3, 4, 50, B = 5, three roll-out modes, three environments,
two start covariances) with plant_rel = 0.08134 on the mass and 0.05 on the other scalars, half-widths dw, and one full Sth per
problem with the "full" start.

Tolerances: the rule of tests/test_gpu_lincov.py.  Each constant is ten times the largest relative error of its row, rounded up
to a power of ten, every error that of the float64 restatement against the np.longdouble restatement, measured on the CPU by
tools/lincov_plant_errors.py and written with its source into profiles/lincov_plant.txt; never taken from the device.  Relative =
|a - ref|_max / |ref|_max per array per problem (Cd: per column).  The bit-for-bit rows have no tolerance."""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import lincov_cases as LC
import lincov_plant_cases as PC
import np_lincov_plant as NP
import np_simulate_disturbed as NSD
from test_gpu_lincov import rel, set_env, solver, tvlqr_opts
from test_lincov_plant_cpu import TOL_SENS

pytestmark = pytest.mark.gpu

TOL_CD = 1e-14         # profiles/lincov_plant.txt 1(a): Cd by complex step, float64 against long double 5.2e-16
TOL_KNOT = 1e-12       # 1(a): sigma_x, sigma_u, z_obs, Sxx, Sxt on the device's AB, K, Cd; the formulas' own fp64 error 6.8e-14 (sigma_u)
TOL_SUMMARY = 1e-11    # 1(a): min_z_obs, min_z_ctl, p_collision_bound likewise; own error 2.0e-13 (erfc's tails)
TOL_END = 1e-11        # 1(b): every array against the restatement's own AB, K, Cd: gusto_tvlqr's 6e-15 over 49 knots
TOL_SENS_DEVICE = TOL_SENS   # 1(c): ten times the disagreement of the two restatements

B = LC.B
KNOT_FIELDS = ("sigma_x", "sigma_u", "z_obs", "Sxx", "Sxt")
INDEX_FIELDS = ("status", "fail_knot", "obs_knot", "obs_pair", "ctl_knot", "ctl_entry")
SUMMARY_FIELDS = ("min_z_obs", "min_z_ctl", "p_collision_bound")
ALL_FIELDS = INDEX_FIELDS + SUMMARY_FIELDS + KNOT_FIELDS
PLAIN_FIELDS = tuple(f for f in ALL_FIELDS if f != "Sxt")


def run(s, model, N, mode, st, X, U, idx=None, store_S=1, K=None):
    """lincov_disturbed of a case on the handle s (idx: the problems it holds), with Sxt and Cd in the report"""
    idx = slice(None) if idx is None else idx
    S0, Sth = LC.start(model, st), PC.start_theta(model, st)
    r = s.lincov_disturbed(LC.options(model, N, mode, store_S=store_S), PC.disturb(model), X, U, K=K,
                           S0=None if S0 is None else S0[idx], Sth=None if Sth is None else Sth[idx])
    r["Cd"], Sxt = s.get_lincov_plant()
    if store_S:
        r["Sxt"] = Sxt
    return r


@functools.lru_cache(maxsize=None)
def device(model, N, mode):
    """one handle: the gains of gusto_tvlqr, then gusto_lincov_disturbed with store_S = 1 for every environment and start
    (computed once, shared, never written to).  Returns (tvlqr result, Cd, {(env, start): report with Sxt})"""
    X, U, tf, _ = LC.inputs(model, N)
    s = solver(model, N, X, U, tf)
    tv = s.tvlqr(tvlqr_opts(mode), X, U)
    assert tv.status.all()
    out = {}
    for e in LC.ENVS:
        set_env(s, model, e)
        for st in LC.STARTS:
            out[e, st] = run(s, model, N, mode, st, X, U)
            assert s.last_lincov_ms() > 0
            for a in out[e, st].values():
                a.setflags(write=False)
    s.close()
    Cd = out["sim", "default"]["Cd"]
    assert all(np.array_equal(r["Cd"], Cd) for r in out.values())
    return tv, Cd, out


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
def test_sensitivities_against_the_restatement(model, N):
    """Cd of every case and roll-out mode against the complex step; the columns of scalars the model does not read are zeros"""
    unread = ~NP.read_mask(model)
    for mode in range(len(LC.MODES)):
        _, Cd, _ = device(model, N, mode)
        ref = PC.sensitivities(model, N, mode)
        assert not Cd[:, :, :, unread].any()
        for b in range(B):
            for j in NSD.READS[model]:
                e = rel(Cd[b, :, :, j], ref[b, :, :, j])
                assert e <= TOL_CD, (model, N, mode, b, j, e)


@pytest.mark.parametrize("model,N", LC.CASES)
def test_every_output_against_the_restatement_on_the_devices_jacobians_gains_and_sensitivities(model, N):
    """every per-knot array, Sxx, Sxt, the summaries and (exactly) the indices, np_lincov_plant fed with the device's AB, K and Cd"""
    for mode in range(len(LC.MODES)):
        tv, Cd, out = device(model, N, mode)
        for e in LC.ENVS:
            for st in LC.STARTS:
                ref = PC.reference(model, N, mode, e, st, tv.AB, tv.K, Cd)
                for b in range(B):
                    compare(out[e, st], ref[b], b, TOL_KNOT, TOL_SUMMARY, (model, N, mode, e, st, b))


@pytest.mark.parametrize("model,N", LC.CASES)
def test_end_to_end(model, N):
    """... against the restatement's own AB, K (complex-step Jacobians, the plain Riccati recursion) and Cd (complex step)"""
    for mode in range(len(LC.MODES)):
        _, _, out = device(model, N, mode)
        for e, st in (("sim", "default"), ("batch", "full")):
            ref = PC.reference(model, N, mode, e, st)
            for b in range(B):
                compare(out[e, st], ref[b], b, TOL_END, TOL_END, (model, N, mode, e, st, b))


def closed_loop_on_the_device(model, N, mode):
    """the worst disagreement between the central differences of gusto_simulate_disturbed's Xcl over supplied plants
    theta_nom (1 +- eps e_j) and column j of gusto_lincov_disturbed's Sxt_k / Stheta_jj, on roll-out consistent trajectories with
    S0 = 0, no clipping, no noise"""
    X, U, tf = PC.consistent_inputs(model, N, mode)
    n, m = g.MODEL_DIMS[model]
    theta = PC.fd_plants(model)
    S = len(theta)
    s = solver(model, N, X, U, tf)
    assert s.tvlqr(tvlqr_opts(mode), X, U).status.all()
    s.simulate_disturbed(dict(n_samples=S, store_knots=1, dense_collision=0, **LC.MODES[mode]), None, X, U, pert=np.zeros((B, S, n + m)),
                         plant=np.tile(theta, (B, 1, 1)), white=np.zeros((B, N - 1, S, m)))
    Xcl, used = s.get_simulate_knots(), s.get_simulate_plant()
    r = s.lincov_disturbed(dict(dx0=0.0, du0=0.0, store_S=1), dict(plant_rel=PC.PLANT_REL), X, U)
    _, Sxt = s.get_lincov_plant()
    s.close()
    # the nominal sample tracks X: the device's roll-out fuses multiply-adds, a few ulp per interval that the feedback contracts
    assert r["status"].all() and np.abs(Xcl[:, :, 0] - X).max() <= 1e-12 * np.abs(X).max()
    Sth = NP.default_Sth(model, PC.PLANT_REL)
    return max(PC.sens_rel(PC.fd_sensitivity(model, Xcl[b], used[b]), NP.closed_loop_sensitivity(dict(Sxt=Sxt[b]), Sth), model) for b in range(B))


@pytest.mark.parametrize("model,N,mode", PC.CONSISTENT)
def test_closed_loop_sensitivity_against_gusto_simulate_disturbed(model, N, mode):
    """tests/test_lincov_plant_cpu.py's check of the two restatements, on the device: the two stages check each other, no statistics"""
    e = closed_loop_on_the_device(model, N, mode)
    print("closed-loop sensitivity on the device, model %d N %d mode %d: %.3e" % (model, N, mode, e))
    assert e <= TOL_SENS_DEVICE, e


@pytest.mark.parametrize("model", LC.MODELS)
def test_reduction_to_gusto_lincov(model):
    """zero dispersion (d all zeros, and d = NULL) and Sth = NULL: every output of gusto_get_lincov equals gusto_lincov's as
    numbers; Cd is what it is with a dispersion, Sxt is zero"""
    N, mode = 50, 1
    X, U, tf, _ = LC.inputs(model, N)
    _, Cd, _ = device(model, N, mode)
    s = solver(model, N, X, U, tf, "batch")
    s.tvlqr(tvlqr_opts(mode), X, U)
    for st in LC.STARTS:
        o = LC.options(model, N, mode, store_S=1)
        plain = s.lincov(o, X, U, S0=LC.start(model, st))
        with pytest.raises(g._capi.GustoError, match="-> -3"):
            s.get_lincov_plant()
        for d in (None, dict(plant_rel=0.0, dw=0.0)):
            z = s.lincov_disturbed(o, d, X, U, S0=LC.start(model, st))
            cd, Sxt = s.get_lincov_plant()
            for f in PLAIN_FIELDS:
                assert np.array_equal(z[f], plain[f]), (st, f)
            assert np.array_equal(cd, Cd) and not Sxt.any()
    s.close()


@pytest.mark.parametrize("model", LC.MODELS)
def test_bit_for_bit_rows(model):
    """Sxx symmetric; S_1 = blockdiag(S0, Stheta) on the blocks that come back; store_S 0 and 1 agree on every shared output;
    K = NULL is the device's K passed back; a problem alone (B = 1) and in the batch of five"""
    N, mode = 50, 1
    X, U, tf, _ = LC.inputs(model, N)
    tv, Cd, out = device(model, N, mode)
    for r in out.values():
        assert np.array_equal(r["Sxx"], np.swapaxes(r["Sxx"], -1, -2)) and not r["Sxt"][:, 0].any()
    e, st = "batch", "full"
    s = solver(model, N, X, U, tf, e)
    s.tvlqr(tvlqr_opts(mode), X, U)
    r0 = run(s, model, N, mode, st, X, U, store_S=0)
    assert "Sxx" not in r0 and "Sxt" not in r0
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_lincov_plant(Sxt=True)
    rk = run(s, model, N, mode, st, X, U, K=tv.K)
    s.close()
    for f in ALL_FIELDS + ("Cd",):
        assert f in ("Sxx", "Sxt") or np.array_equal(r0[f], out[e, st][f]), f
        assert np.array_equal(rk[f], out[e, st][f]), f
    for j in (1, 3, 4):
        s1 = solver(model, N, X[j:j + 1], U[j:j + 1], tf[j:j + 1], e, [j])
        s1.tvlqr(tvlqr_opts(mode), X[j:j + 1], U[j:j + 1])
        r1 = run(s1, model, N, mode, st, X[j:j + 1], U[j:j + 1], idx=slice(j, j + 1))
        s1.close()
        for f in ALL_FIELDS + ("Cd",):
            assert np.array_equal(r1[f][0], out[e, st][f][j]), (f, j)


def test_mask_keeps_the_inactive_problem():
    """gusto_set_active: the active problems are what they are in the full batch, bit for bit; the inactive one is untouched by
    a second call with another dispersion; a masked FIRST call after new problems leaves zeros for it, Cd and Sxt included"""
    model, N, mode, e, st = 3, 50, 0, "sim", "default"
    X, U, tf, _ = LC.inputs(model, N)
    _, _, out = device(model, N, mode)
    full = out[e, st]
    s = solver(model, N, X, U, tf, e)
    s.tvlqr(tvlqr_opts(mode), X, U)
    a = run(s, model, N, mode, st, X, U)
    act = np.array([1, 1, 0, 1, 1], bool)
    s.set_active(act)
    b = s.lincov_disturbed(LC.options(model, N, mode, store_S=1), dict(plant_rel=2 * PC.PLANT_REL), X, U)
    b["Cd"], b["Sxt"] = s.get_lincov_plant()
    for f in ALL_FIELDS + ("Cd",):
        assert np.array_equal(a[f], full[f]), f
        assert np.array_equal(b[f][2], a[f][2]), f
    assert not np.array_equal(b["sigma_x"][1], a["sigma_x"][1]) and not np.array_equal(b["Sxt"][1], a["Sxt"][1])
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    s.set_active(None)
    s.tvlqr(tvlqr_opts(mode), X, U)
    s.set_active(act)
    c = run(s, model, N, mode, st, X, U)
    for f in ALL_FIELDS + ("Cd",):
        assert not np.asarray(c[f][2]).any(), f
        assert np.array_equal(c[f][act], full[f][act]), f
    s.set_active(None)
    s.close()


@pytest.mark.parametrize("model", LC.MODELS)
def test_tile_seam_of_the_sensitivity_kernel(model):
    """N - 1 intervals over two workgroup tiles of lincov_plant_sens with one interval in the last: Cd of every interval against
    the restatement, then the recursion on the device's AB, K, Cd; a second handle with N - 1 = one full tile agrees on its
    intervals bit for bit"""
    N, mode = PC.SEAM_N[model], 1
    X, U, tf = PC.seam_inputs(model)
    nb = PC.SEAM_B
    s = solver(model, N, X, U, tf, "empty")
    tv = s.tvlqr(tvlqr_opts(mode), X, U)
    assert tv.status.all()
    o = dict(dx0=LC.SC.dx0(model), du0=LC.SC.du0(model), du_white=LC.du_white(model, N, mode), store_S=1)
    r = s.lincov_disturbed(o, PC.disturb(model), X, U)
    Cd, Sxt = s.get_lincov_plant()
    s.close()
    r["Sxt"] = Sxt
    assert r["status"].all()
    for b in range(nb):
        ref = NP.sensitivities(model, X[b], U[b], tf[b], **LC.MODES[mode])
        for j in NSD.READS[model]:
            e = rel(Cd[b, :, :, j], ref[:, :, j])
            assert e <= TOL_CD, (model, b, j, e)
            assert rel(Cd[b, -1:, :, j], ref[-1:, :, j]) <= TOL_CD and rel(Cd[b, -2:-1, :, j], ref[-2:-1, :, j]) <= TOL_CD
        want = NP.lincov_plant(model, X[b], U[b], tv.AB[b], tv.K[b], Cd[b], None, None, LC.SC.dx0(model), LC.SC.du0(model),
                               LC.du_white(model, N, mode), PC.dw(model), PC.PLANT_REL)
        compare(r, want, b, TOL_KNOT, TOL_SUMMARY, (model, N, b))
    # the same first N - 2 intervals on a handle whose horizon ends with the first tile
    s = solver(model, N - 1, X[:, :N - 1], U[:, :N - 1], tf * (N - 2) / (N - 1), "empty")
    s.tvlqr(tvlqr_opts(mode), X[:, :N - 1], U[:, :N - 1])
    s.lincov_disturbed(dict(o, store_S=0), PC.disturb(model), X[:, :N - 1], U[:, :N - 1])
    Cd1, _ = s.get_lincov_plant()
    s.close()
    assert np.array_equal(Cd1, Cd[:, :N - 2])


def test_failures_are_data_and_state_errors():
    """a problem whose gusto_tvlqr failed: its fail_knot, status 0 and zeros, Sxt included, the other four unchanged to the bit;
    gusto_get_lincov_plant after a plain gusto_lincov, before any call and after new problems: GUSTO_ERR_STATE; the refusals
    through the C ABI"""
    model, N, mode, e, st = 2, 50, 0, "sim", "default"
    X, U, tf, _ = LC.inputs(model, N)
    n, m = g.MODEL_DIMS[model]
    _, _, out = device(model, N, mode)
    clean = out[e, st]
    s = solver(model, N, X, U, tf, e)
    assert s.L.gusto_get_lincov_plant(s.h, None, None) == -3
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.lincov_disturbed()                               # no gusto_tvlqr yet
    assert b"gusto_tvlqr" in s.L.gusto_last_error(s.h) and b"gusto_lincov_disturbed" in s.L.gusto_last_error(s.h)
    # gusto_tvlqr fails where a NaN state enters its backward recursion (tests/test_gpu_lincov.py: test_failures_are_data)
    Xn = X.copy()
    Xn[2, N - 2, 10] = np.nan
    t = s.tvlqr(tvlqr_opts(mode), Xn, U)
    assert list(t.status) == [1, 1, 0, 1, 1] and t.fail_knot[2] == N - 1
    d = run(s, model, N, mode, st, X, U)
    assert list(d["status"]) == [1, 1, 0, 1, 1] and d["fail_knot"][2] == N - 1
    for f in ALL_FIELDS:
        assert f in ("status", "fail_knot") or not np.asarray(d[f][2]).any(), f
    for j in (0, 1, 3, 4):
        for f in ALL_FIELDS + ("Cd",):
            assert np.array_equal(d[f][j], clean[f][j]), (f, j)
    # a caller's K with a NaN at knot 2 of problem 3: fail_knot 2, the rows of knot 1 stay
    s.tvlqr(tvlqr_opts(mode), X, U)
    Kn = s.get_tvlqr().K.copy()
    Kn[3, 1, 2, 5] = np.nan
    r = run(s, model, N, mode, st, X, U, K=Kn)
    assert list(r["status"]) == [1, 1, 1, 0, 1] and list(r["fail_knot"]) == [0, 0, 0, 2, 0]
    for f in KNOT_FIELDS:
        assert np.array_equal(r[f][3, :1], clean[f][3, :1]) and not r[f][3, 1:].any(), f
    # state: a plain gusto_lincov in between
    s.lincov(LC.options(model, N, mode), X, U)
    assert s.L.gusto_get_lincov_plant(s.h, None, None) == -3 and b"gusto_lincov_disturbed" in s.L.gusto_last_error(s.h)
    # refusals: nothing launched, the report of the plain call stays
    inf, nan = np.inf, np.nan
    rel6 = np.zeros(6); rel6[3] = 1.0
    for bad in (dict(plant_rel=-1e-9), dict(plant_rel=rel6), dict(plant_rel=nan), dict(plant_rel=inf), dict(dw=-1.0), dict(dw=nan), dict(dw=inf)):
        with pytest.raises(g._capi.GustoError, match="-> -1"):
            s.lincov_disturbed(None, bad)
    for o in (dict(dx0=-1.0), dict(du_white=nan), dict(store_S=2), dict(u_lo=1.0, u_hi=0.5)):
        with pytest.raises(g._capi.GustoError, match="-> -1") as err:
            s.lincov_disturbed(o)
        assert "gusto_lincov_disturbed" in str(err.value)
    good = np.array(PC.full_Sth(model))
    for i, j, v, word in ((2, 2, -1e-12, "negative"), (1, 3, nan, "finite"), (0, 0, inf, "finite"), (0, 2, 1e-3, "symmetric")):
        Sth = good.copy()
        Sth[3, i, j] = v
        with pytest.raises(g._capi.GustoError, match="-> -1") as err:
            s.lincov_disturbed(None, None, Sth=Sth)
        assert word in str(err.value) and "problem 3" in str(err.value) and "%d, %d" % (i, j) in str(err.value)
    assert s.L.gusto_get_lincov_plant(s.h, None, None) == -3
    assert s.L.gusto_lincov_disturbed(s.h, X.ctypes.data, None, None, None, None, None, None) == -1
    # accepted: garbage on the scalars the model does not read (PC.full_Sth holds 1e3 and a NaN there)
    assert s.lincov_disturbed(None, None, Sth=good)["status"].all()
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)   # new problems: the old results and Jacobians are gone
    assert s.L.gusto_get_lincov_plant(s.h, None, None) == -3
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.lincov_disturbed()
    s.close()
    t = g._capi.TrajOptSolver(0, 50, B)
    X0, _, tf0, _ = LC.inputs(0, 50)
    t.set_problems(X0[:, 0], X0[:, -1], X0[:, -1], tf0)
    with pytest.raises(g._capi.GustoError):
        t.lincov_disturbed()
    assert t.L.gusto_lincov_disturbed(t.h, None, None, None, None, None, None, None) == -1 and b"TrajOpt" in t.L.gusto_last_error(t.h)
    t.close()


def test_host_mirror():
    """host.lincov_disturbed on one trajectory against the restatement: the report of host.lincov with Cd and Sxt"""
    import np_tvlqr as T
    H, P = g.host, g.problems
    model = H.FreeflyerSE2()
    gs = H.GoalSet()
    H.add_goal(gs, H.Goal(H.PointGoal(P.FREEFLYER_X_GOAL), 200.0, model))
    env = P.freeflyer_env()
    TOP = H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.Environment(env), P.freeflyer_random_x_init(1)[0], gs),
                                          50, 200.0, fixed_final_time=True)
    traj = H.init_traj_straightline(TOP)
    one = H.lincov_disturbed(traj, H.SCPProblem(TOP), disturb=dict(plant_rel=PC.PLANT_REL, dw=0.01), Q=2.0, R=0.5, Qf=3.0, dx0=0.02,
                             du0=0.01, du_white=0.005, store_S=1)
    AB, K, _ = T.tvlqr(0, traj.X.T, traj.U.T, 200.0, 2.0, 0.5, 3.0)
    Cd = NP.sensitivities(0, traj.X.T, traj.U.T, 200.0)
    ref = NP.lincov_plant(0, traj.X.T, traj.U.T, AB, K, Cd, None, None, 0.02, 0.01, 0.005, 0.01, PC.PLANT_REL, boxes=env)
    assert one["status"] == 1 and one["obs_knot"] == ref["obs_knot"] and one["obs_pair"] == ref["obs_pair"]
    assert one["Cd"].shape == Cd.shape and one["Sxt"].shape == ref["Sxt"].shape
    assert max(rel(one["Cd"][:, :, j], Cd[:, :, j]) for j in NSD.READS[0]) <= TOL_CD
    for f in ("sigma_x", "sigma_u", "z_obs", "Sxx", "Sxt"):
        assert rel(one[f], ref[f]) <= TOL_END, f
