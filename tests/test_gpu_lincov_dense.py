"""gusto_lincov_dense on the device against tests/np_lincov_dense.py, the numpy restatement, against gusto_lincov_disturbed (its own
knot pass, and as a second kernel path on the dense trajectory), and on the corner-cut case; tests/test_lincov_dense_cpu.py pins
the restatement and the conditioning of the inputs without a GPU.

Inputs: tests/lincov_dense_cases.py -- lincov_plant_cases (four models, N = 3, 4, 50, B = 5, three roll-out modes, the dispersion)
with the environment / start pairs ("sim", "default"), ("batch", "full"), ("empty", "default").

Tolerances: the rule of tests/test_gpu_lincov.py.  Each constant is ten times the largest relative error of its row, rounded up
to a power of ten, every error that of the float64 restatement against the np.longdouble restatement, measured on the CPU by
tools/lincov_dense_errors.py and written with its source into profiles/lincov_dense.txt; never taken from the device.  Relative =
|a - ref|_max / |ref|_max per array per problem.  The bit-for-bit rows have no tolerance."""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import lincov_cases as LC
import lincov_dense_cases as DC
import lincov_plant_cases as PC
import np_lincov_dense as ND
import np_lincov_plant as NP
import np_tvlqr as T
from test_gpu_lincov import rel, set_env, solver, tvlqr_opts

pytestmark = pytest.mark.gpu

TOL_Z = 1e-13          # profiles/lincov_dense.txt 1: z_dense on the device's AB, K, Cd; the formulas' own fp64 error 7.3e-15
TOL_SPOS = 1e-13       # 1: Spos likewise; own error 1.1e-15
TOL_MIN = 1e-12        # 1: min_z_dense likewise; own error 7.4e-14 (relative to itself: one number per problem)
TOL_END = 1e-11        # every array against the restatement's own AB, K, Cd: profiles/lincov_plant.txt 1(b), gusto_tvlqr's 6e-15 over
#                        49 knots; the dense pass adds the products of row 1 to it
TOL_TWO = 1e-13        # profiles/lincov_dense.txt 2: ten times the disagreement of the restatement's two routes, 2.4e-15

B = LC.B
COMBOS = (("sim", "default"), ("batch", "full"), ("empty", "default"))
SUMMARY = ("nfull", "dense_sample", "dense_pair", "min_z_dense")
ROWS = ("z_dense", "pair_dense", "Spos")
DENSE = SUMMARY + ROWS
KNOT = ("status", "fail_knot", "obs_knot", "obs_pair", "ctl_knot", "ctl_entry", "min_z_obs", "min_z_ctl", "p_collision_bound",
        "sigma_x", "sigma_u", "z_obs", "Sxx", "Sxt", "Cd")


def run(s, model, N, mode, st, X, U, idx=None, store_dense=1, K=None, disturb=True, opts=None):
    """lincov_dense of a case on the handle s (idx: the problems it holds): the dense report, and under "knot" what
    gusto_get_lincov and gusto_get_lincov_plant say after it"""
    idx = slice(None) if idx is None else idx
    S0, Sth = LC.start(model, st), PC.start_theta(model, st)
    d = s.lincov_dense(LC.options(model, N, mode, store_S=1) if opts is None else opts, PC.disturb(model) if disturb is True else disturb,
                       X, U, K=K, S0=None if S0 is None else S0[idx], Sth=None if Sth is None else Sth[idx], store_dense=store_dense)
    d["knot"] = knot_of(s)
    return d


def knot_of(s):
    k = s.get_lincov()
    k["Cd"], k["Sxt"] = s.get_lincov_plant()
    return k


@functools.lru_cache(maxsize=None)
def device(model, N, mode):
    """one handle: the gains of gusto_tvlqr, then gusto_lincov_dense with store_dense = 1 for COMBOS (computed once, shared, never
    written to).  Returns (tvlqr result, Cd, {(env, start): dense report with the knot pass under "knot"})"""
    X, U, tf, _ = LC.inputs(model, N)
    s = solver(model, N, X, U, tf)
    tv = s.tvlqr(tvlqr_opts(mode), X, U)
    assert tv.status.all()
    out = {}
    for e, st in COMBOS:
        set_env(s, model, e)
        out[e, st] = run(s, model, N, mode, st, X, U)
        assert s.last_lincov_ms() > 0
        for a in list(out[e, st].values()) + list(out[e, st]["knot"].values()):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    s.close()
    return tv, out["sim", "default"]["knot"]["Cd"], out


def compare(dev, ref, b, tol_z, tol_spos, tol_min, where):
    nf = ref["nfull"]
    assert dev["nfull"][b] == nf and dev["dense_sample"][b] == ref["dense_sample"] and dev["dense_pair"][b] == ref["dense_pair"], where
    assert np.array_equal(dev["pair_dense"][b][:nf], ref["pair_dense"]), where
    assert not dev["z_dense"][b][nf:].any() and not dev["pair_dense"][b][nf:].any() and not dev["Spos"][b][nf:].any(), where
    for f, tol in (("z_dense", tol_z), ("Spos", tol_spos)):
        e = rel(dev[f][b][:nf], ref[f])
        assert e <= tol, (where, f, e)
    e = rel(dev["min_z_dense"][b], ref["min_z_dense"])
    assert e <= tol_min, (where, "min_z_dense", e)


@pytest.mark.parametrize("model,N", LC.CASES)
def test_every_dense_output_against_the_restatement_on_the_devices_inputs(model, N):
    """z_dense, Spos, the summary and (exactly) pair_dense, dense_sample, dense_pair, nfull; the restatement fed with the device's AB,
    K and Cd (its S rows are np_lincov_plant's on them); rows behind nfull are zeros"""
    for mode in range(len(LC.MODES)):
        tv, Cd, out = device(model, N, mode)
        for e, st in COMBOS:
            ref = DC.dense_reference(model, N, mode, e, st, tv.AB, tv.K, Cd)
            for b in range(B):
                compare(out[e, st], ref[b], b, TOL_Z, TOL_SPOS, TOL_MIN, (model, N, mode, e, st, b))


@pytest.mark.parametrize("model,N", LC.CASES)
def test_end_to_end(model, N):
    """... against the restatement's own AB, K and Cd"""
    for mode in range(len(LC.MODES)):
        _, _, out = device(model, N, mode)
        for e, st in COMBOS[:2]:
            ref = DC.dense_reference(model, N, mode, e, st)
            for b in range(B):
                compare(out[e, st], ref[b], b, TOL_END, TOL_END, TOL_END, (model, N, mode, e, st, b))


@pytest.mark.parametrize("model", LC.MODELS)
def test_bit_for_bit_rows(model):
    """no tolerance: the i = 0 samples and knot N are the knot pass's z_obs, pair and Sxx block; nstep = 1 makes the dense summary
    the knot summary; gusto_get_lincov / gusto_get_lincov_plant after the dense call are those after gusto_lincov_disturbed;
    store_dense = 0 agrees on the summary; a problem alone, in the batch and on a handle larger than B"""
    N = 50
    ws = g._capi.WS_DIM[model]
    X, U, tf, _ = LC.inputs(model, N)
    for mode in range(len(LC.MODES)):
        tv, Cd, out = device(model, N, mode)
        for (e, st), d in out.items():
            k = d["knot"]
            for b in range(B):
                ns = (d["nfull"][b] - 1) // (N - 1)
                at = np.arange(N) * ns
                assert np.array_equal(d["z_dense"][b][at], k["z_obs"][b]) and np.array_equal(d["Spos"][b][at], k["Sxx"][b][:, :ws, :ws])
                assert np.array_equal(d["Spos"][b], np.swapaxes(d["Spos"][b], 1, 2))
                if k["obs_knot"][b]:
                    assert d["pair_dense"][b][at[k["obs_knot"][b] - 1]] == k["obs_pair"][b]
                assert d["min_z_dense"][b] <= k["min_z_obs"][b]
                if ns == 1:
                    assert d["min_z_dense"][b] == k["min_z_obs"][b] and d["dense_sample"][b] == k["obs_knot"][b] - 1
                    assert d["dense_pair"][b] == k["obs_pair"][b]
            # the pair at every knot: the restatement's, exactly (lincov_dense_cases keeps them conditioned)
            ref = PC.reference(model, N, mode, e, st, tv.AB, tv.K, Cd)
            for b in range(B):
                ns = (d["nfull"][b] - 1) // (N - 1)
                assert [d["pair_dense"][b][j * ns] for j in range(N)] == [NP.NL._first_min(zp)[1] for zp in ref[b]["z_pairs"]]
    mode, e, st = 1, "batch", "full"
    tv, Cd, out = device(model, N, mode)
    full = out[e, st]
    s = solver(model, N, X, U, tf, e)
    s.tvlqr(tvlqr_opts(mode), X, U)
    S0, Sth = LC.start(model, st), PC.start_theta(model, st)
    s.lincov_disturbed(LC.options(model, N, mode, store_S=1), PC.disturb(model), X, U, S0=S0, Sth=Sth)
    plain = knot_of(s)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_lincov_dense()
    for f in KNOT:
        assert np.array_equal(plain[f], full["knot"][f]), f
    d0 = run(s, model, N, mode, st, X, U, store_dense=0)
    assert all(f not in d0 for f in ROWS)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_lincov_dense(rows=True)
    for f in SUMMARY:
        assert np.array_equal(d0[f], full[f]), f
    for f in KNOT:
        assert np.array_equal(d0["knot"][f], full["knot"][f]), f
    # d = NULL (and all zeros) with Sth = NULL: the dense form of plain gusto_lincov -- its knot pass reports gusto_lincov's numbers
    o = LC.options(model, N, mode, store_S=1)
    lin = s.lincov(o, X, U, S0=S0)
    for dz in (None, dict(plant_rel=0.0, dw=0.0)):
        z = s.lincov_dense(o, dz, X, U, S0=S0)
        kz = knot_of(s)
        for f in KNOT[:-2]:
            assert np.array_equal(kz[f], lin[f]), f
        assert not kz["Sxt"].any() and np.array_equal(kz["Cd"], Cd)
        for b in range(B):
            at = np.arange(N) * ((z["nfull"][b] - 1) // (N - 1))
            assert np.array_equal(z["z_dense"][b][at], lin["z_obs"][b]) and np.array_equal(z["Spos"][b][at], lin["Sxx"][b][:, :ws, :ws])
    s.close()
    for j in (1, 4):
        s1 = solver(model, N, X[j:j + 1], U[j:j + 1], tf[j:j + 1], e, [j])
        s1.tvlqr(tvlqr_opts(mode), X[j:j + 1], U[j:j + 1])
        r1 = run(s1, model, N, mode, st, X[j:j + 1], U[j:j + 1], idx=slice(j, j + 1))
        s1.close()
        for f in DENSE:
            assert np.array_equal(r1[f][0], full[f][j]), (f, j)
    big = g.BatchSolver(model, N, B + 3, hist_cap=16)
    big.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    set_env(big, model, e)
    big.tvlqr(tvlqr_opts(mode), X, U)
    rb = run(big, model, N, mode, st, X, U)
    big.close()
    for f in DENSE:
        assert np.array_equal(rb[f], full[f]), f


def test_mask_keeps_the_inactive_problem():
    """gusto_set_active: the active problems are what they are in the full batch, bit for bit; the inactive one keeps its rows
    through a second call with another dispersion; a masked FIRST call after new problems leaves zeros for it"""
    model, N, mode, e, st = 3, 50, 2, "sim", "default"
    X, U, tf, _ = LC.inputs(model, N)
    _, _, out = device(model, N, mode)
    full = out[e, st]
    s = solver(model, N, X, U, tf, e)
    s.tvlqr(tvlqr_opts(mode), X, U)
    a = run(s, model, N, mode, st, X, U)
    act = np.array([1, 1, 0, 1, 1], bool)
    s.set_active(act)
    b = run(s, model, N, mode, st, X, U, disturb=dict(plant_rel=2 * PC.PLANT_REL))
    for f in DENSE:
        assert np.array_equal(a[f], full[f]), f
        assert np.array_equal(b[f][2], a[f][2]), f
    assert not np.array_equal(b["Spos"][1], a["Spos"][1])
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    s.set_active(None)
    s.tvlqr(tvlqr_opts(mode), X, U)
    s.set_active(act)
    c = run(s, model, N, mode, st, X, U)
    for f in DENSE:
        assert not np.asarray(c[f][2]).any(), f
        assert np.array_equal(c[f][act], full[f][act]), f
    s.set_active(None)
    s.close()


@pytest.mark.parametrize("model", LC.MODELS)
def test_two_kernel_paths_agree_sample_for_knot(model):
    """gains of zero, no noise, full S0 / Sth: sample j of the dense call on (N = 50, nstep = 5) against knot j + 1 of
    gusto_lincov_disturbed on a second handle of 246 knots and nstep = 1, whose X' is the device's own gusto_get_dense output of
    the first handle and whose U' are the held controls -- the one-step Jacobians of tvlqr_linearise chained by the recursion
    against the propagation inside the interval of lincov_dense"""
    N, mode, ns = DC.TWO_N, DC.TWO_MODE, DC.TWO_NS
    n, m = g.MODEL_DIMS[model]
    ws = g._capi.WS_DIM[model]
    X, U, tf, _ = LC.inputs(model, N)
    S0, Sth = LC.full_S0(model), PC.full_Sth(model)
    s = solver(model, N, X, U, tf, "sim")
    s.tvlqr(tvlqr_opts(mode), X, U)
    nfull, Xd, _ = s.interpolate(X, U, **LC.MODES[mode])
    d = s.lincov_dense(dict(dx0=0.0, du0=0.0), None, X, U, K=np.zeros((B, N - 1, m, n)), S0=S0, Sth=Sth)
    s.close()
    N2 = ns * (N - 1) + 1
    assert list(nfull) == [N2] * B and list(d["nfull"]) == [N2] * B and N2 == 246
    Ud = DC.held_controls(U)
    s2 = solver(model, N2, Xd, Ud, tf, "sim")
    s2.tvlqr(dict(tvlqr_opts(mode), nstep=1), Xd, Ud)
    k = s2.lincov_disturbed(dict(dx0=0.0, du0=0.0, store_S=1), None, Xd, Ud, K=np.zeros((B, N2 - 1, m, n)), S0=S0, Sth=Sth)
    s2.close()
    assert k["status"].all()
    for b in range(B):
        for name, a, ref in (("Spos", d["Spos"][b], k["Sxx"][b][:, :ws, :ws]), ("z_dense", d["z_dense"][b], k["z_obs"][b])):
            e = rel(a, ref)
            print("two kernel paths, model %d problem %d %s: %.3e" % (model, b, name, e))
            assert e <= TOL_TWO, (model, b, name, e)


def test_corner_cut_case():
    """the hand-built case of tests/lincov_dense_cases.py: the device finds the interior sample and the pair the restatement found,
    and the margin the knots do not show"""
    X, U, tf, spheres = DC.corner_inputs()
    model, N, mode = DC.CORNER["model"], DC.CORNER["N"], DC.CORNER["mode"]
    knot, ref = DC.corner_reference()
    s = g.BatchSolver(model, N, 1, hist_cap=16)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    s.set_env(None, spheres)
    s.tvlqr(tvlqr_opts(mode), X, U)
    d = s.lincov_dense(DC.corner_options(), PC.disturb(model), X, U)
    k = s.get_lincov()
    s.close()
    assert (d["nfull"][0], d["dense_sample"][0], d["dense_pair"][0]) == (16, ref["dense_sample"], ref["dense_pair"]) == (16, 7, 1)
    assert k["obs_knot"][0] == knot["obs_knot"] and d["min_z_dense"][0] < k["min_z_obs"][0] / 3
    compare(d, ref, 0, TOL_END, TOL_END, TOL_END, "corner")


@pytest.mark.parametrize("model", LC.MODELS)
def test_seams_of_the_dense_kernel(model):
    """N = 7: six intervals over two workgroups of four waves, the second half empty; nstep = 64, the cap, at N = 3 (z and pair go
    out 64 samples at a time, the 65th row is knot N's neighbour); the restatement fed with the device's AB, K, Cd"""
    for N, kw in ((DC.SEAM_N, dict(nstep=5)), (3, dict(nstep=DC.CAP_NSTEP))):
        X, U, tf = DC.seam_inputs(model, N)
        s = solver(model, N, X, U, tf, "empty")
        if model != 1:
            s.set_env(*LC.SC.env(model))
        Q, R, Qf = LC.WEIGHTS
        tv = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **kw), X, U)
        assert tv.status.all()
        o = dict(dx0=LC.SC.dx0(model), du0=LC.SC.du0(model), du_white=LC.du_white(model, N, 1))
        d = s.lincov_dense(o, PC.disturb(model), X, U)
        Cd, _ = s.get_lincov_plant()
        s.close()
        assert list(d["nfull"]) == [kw["nstep"] * (N - 1) + 1] * DC.SEAM_B
        for b, (_, ref) in enumerate(DC.seam_reference(model, X, U, tf, tv.AB, tv.K, Cd, kw)):
            compare(d, ref, b, TOL_Z, TOL_SPOS, TOL_MIN, (model, N, b))


def test_longest_horizon():
    """N = 256 with B = 2 (freeflyerSE2, nstep = 2): 255 intervals, 64 workgroups per problem with three waves in the last"""
    model, N, kw = 0, DC.LONG_N, dict(nstep=2)
    X, U, tf = DC.seam_inputs(model, N)
    s = solver(model, N, X, U, tf, "empty")
    s.set_env(*LC.SC.env(model))
    Q, R, Qf = LC.WEIGHTS
    tv = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **kw), X, U)
    d = s.lincov_dense(dict(dx0=LC.SC.dx0(model), du0=LC.SC.du0(model), du_white=LC.du_white(model, N, 1)), PC.disturb(model), X, U)
    Cd, _ = s.get_lincov_plant()
    s.close()
    assert tv.status.all() and list(d["nfull"]) == [2 * (N - 1) + 1] * DC.SEAM_B
    for b, (_, ref) in enumerate(DC.seam_reference(model, X, U, tf, tv.AB, tv.K, Cd, kw)):
        compare(d, ref, b, TOL_Z, TOL_SPOS, TOL_MIN, (model, N, b))


def test_failures_are_data_and_state_errors():
    """a problem dead from gusto_tvlqr: zeros, the other four unchanged to the bit; a non-finite S at knot 2: zeros from sample
    Nstep on, the summary over the samples before; the getters' state errors and the refusals, under the call's name"""
    model, N, mode, e, st = 2, 50, 1, "sim", "default"
    ns = 5
    X, U, tf, _ = LC.inputs(model, N)
    _, _, out = device(model, N, mode)
    clean = out[e, st]
    s = solver(model, N, X, U, tf, e)
    assert s.L.gusto_get_lincov_dense(s.h, None, None) == -3
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.lincov_dense()                               # no gusto_tvlqr yet
    assert b"gusto_tvlqr" in s.L.gusto_last_error(s.h) and b"gusto_lincov_dense" in s.L.gusto_last_error(s.h)
    Xn = X.copy()
    Xn[2, N - 2, 10] = np.nan
    t = s.tvlqr(tvlqr_opts(mode), Xn, U)
    assert list(t.status) == [1, 1, 0, 1, 1]
    d = run(s, model, N, mode, st, X, U)
    assert list(d["knot"]["status"]) == [1, 1, 0, 1, 1] and d["nfull"][2] == ns * (N - 1) + 1
    for f in DENSE:
        assert f == "nfull" or not np.asarray(d[f][2]).any(), f
    for j in (0, 1, 3, 4):
        for f in DENSE:
            assert np.array_equal(d[f][j], clean[f][j]), (f, j)
    # a caller's K with a NaN at knot 2 of problem 3: fail_knot 2, the samples of interval 1 stay, zeros from sample Nstep on
    s.tvlqr(tvlqr_opts(mode), X, U)
    Kn = s.get_tvlqr().K.copy()
    Kn[3, 1, 2, 5] = np.nan
    r = run(s, model, N, mode, st, X, U, K=Kn)
    assert list(r["knot"]["status"]) == [1, 1, 1, 0, 1] and list(r["knot"]["fail_knot"]) == [0, 0, 0, 2, 0]
    for f in ROWS:
        assert np.array_equal(r[f][3, :ns], clean[f][3, :ns]) and not r[f][3, ns:].any(), f
    j = int(np.argmin(clean["z_dense"][3, :ns]))
    assert r["min_z_dense"][3] == clean["z_dense"][3, j] and r["dense_sample"][3] == j and r["dense_pair"][3] == clean["pair_dense"][3, j]
    for f in DENSE:
        assert np.array_equal(r[f][:3], clean[f][:3]) and np.array_equal(r[f][4], clean[f][4]), f
    # state: a plain gusto_lincov or a gusto_lincov_disturbed in between
    s.lincov(LC.options(model, N, mode), X, U)
    assert s.L.gusto_get_lincov_dense(s.h, None, None) == -3 and b"gusto_lincov_dense" in s.L.gusto_last_error(s.h)
    # refusals: nothing launched
    nan = np.nan
    for sd in (2, -1, 7):
        with pytest.raises(g._capi.GustoError, match="-> -1") as err:
            s.lincov_dense(store_dense=sd)
        assert "store_dense" in str(err.value) and "gusto_lincov_dense" in str(err.value)
    for bad in (dict(plant_rel=-1e-9), dict(plant_rel=nan), dict(dw=-1.0), dict(dw=np.inf)):
        with pytest.raises(g._capi.GustoError, match="-> -1") as err:
            s.lincov_dense(None, bad)
        assert "gusto_lincov_dense" in str(err.value)
    for o in (dict(dx0=-1.0), dict(du_white=nan), dict(store_S=2), dict(u_lo=1.0, u_hi=0.5)):
        with pytest.raises(g._capi.GustoError, match="-> -1") as err:
            s.lincov_dense(o)
        assert "gusto_lincov_dense" in str(err.value)
    Sth = np.array(PC.full_Sth(model))
    Sth[3, 0, 2] = 1e-3
    with pytest.raises(g._capi.GustoError, match="-> -1") as err:
        s.lincov_dense(None, None, Sth=Sth)
    assert "symmetric" in str(err.value) and "problem 3" in str(err.value) and "gusto_lincov_dense" in str(err.value)
    assert s.L.gusto_get_lincov_dense(s.h, None, None) == -3
    assert s.L.gusto_lincov_dense(s.h, X.ctypes.data, None, None, None, None, None, None, 1) == -1
    s.lincov_dense(store_dense=0)
    assert s.L.gusto_get_lincov_dense(s.h, None, None) == 0
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)   # new problems: the old results and Jacobians are gone
    assert s.L.gusto_get_lincov_dense(s.h, None, None) == -3
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.lincov_dense()
    s.close()
    t = g._capi.TrajOptSolver(0, 50, B)
    X0, _, tf0, _ = LC.inputs(0, 50)
    t.set_problems(X0[:, 0], X0[:, -1], X0[:, -1], tf0)
    with pytest.raises(g._capi.GustoError):
        t.lincov_dense()
    assert t.L.gusto_lincov_dense(t.h, None, None, None, None, None, None, None, 1) == -1 and b"TrajOpt" in t.L.gusto_last_error(t.h)
    t.close()


def test_host_mirror():
    """host.lincov_dense on one trajectory against the restatement: the report of host.lincov_disturbed with the dense fields"""
    H, P = g.host, g.problems
    model = H.FreeflyerSE2()
    gs = H.GoalSet()
    H.add_goal(gs, H.Goal(H.PointGoal(P.FREEFLYER_X_GOAL), 200.0, model))
    env = P.freeflyer_env()
    TOP = H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.Environment(env), P.freeflyer_random_x_init(1)[0], gs),
                                          50, 200.0, fixed_final_time=True)
    traj = H.init_traj_straightline(TOP)
    one = H.lincov_dense(traj, H.SCPProblem(TOP), disturb=dict(plant_rel=PC.PLANT_REL, dw=0.01), Q=2.0, R=0.5, Qf=3.0, dx0=0.02,
                         du0=0.01, du_white=0.005, store_S=1)
    AB, K, _ = T.tvlqr(0, traj.X.T, traj.U.T, 200.0, 2.0, 0.5, 3.0)
    Cd = NP.sensitivities(0, traj.X.T, traj.U.T, 200.0)
    knot = NP.lincov_plant(0, traj.X.T, traj.U.T, AB, K, Cd, None, None, 0.02, 0.01, 0.005, 0.01, PC.PLANT_REL, boxes=env)
    ref = ND.lincov_dense(0, traj.X.T, traj.U.T, K, knot, 200.0, 0.005, 0.01, env, None)
    assert one["status"] == 1 and one["obs_knot"] == knot["obs_knot"] and one["nfull"] == ref["nfull"] == 41 * 49 + 1
    assert one["dense_sample"] == ref["dense_sample"] and one["dense_pair"] == ref["dense_pair"]
    assert one["Spos"].shape == ref["Spos"].shape and one["Cd"].shape == Cd.shape
    for f in ("z_dense", "Spos", "min_z_dense"):
        assert rel(one[f], ref[f]) <= TOL_END, f
