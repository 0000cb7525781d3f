"""gusto_tighten_env on the device against tests/np_tighten.py, the numpy restatement written from include/gusto_hip.h;
tests/test_tighten_cpu.py pins the restatement and the conditioning of the inputs without a GPU.

Inputs: tests/tighten_cases.py -- models 0, 2, 3 at N = 3, 4, 50 with B = 5 problems, three environments (shared, empty, per
problem with 0 .. 64 components), two start covariances and the option sets.  The restatement is fed with the DEVICE's own Sxx
(gusto_get_lincov), so what is compared is the tightening alone.

Tolerances: TOL_KNOT and TOL_SUMMARY of tests/test_gpu_lincov.py (profiles/lincov.txt): margins, tables and max_margin are sums and
products of a handful of fp64 terms of the same formulas as its per-knot rows, compared relative to the coordinate scale
(max(1, |X|_max) of the problem); min_z_base is gusto_lincov's min_z_obs.  The bit-for-bit rows have no tolerance."""
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import lincov_cases as LC
import np_verify as V
import tighten_cases as TC
from test_gpu_lincov import TOL_KNOT, TOL_SUMMARY, rel, set_env, solver, tvlqr_opts

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = TC.B
INT_FIELDS = ("status", "knot", "pair", "n_grown", "blocked")


def handle(model, N):
    """a handle with the case's trajectories and the gains of gusto_tvlqr"""
    X, U, tf, _ = LC.inputs(model, N)
    s = solver(model, N, X, U, tf)
    assert s.tvlqr(tvlqr_opts(TC.MODE), X, U).status.all()
    return s, X, U


def analyse(s, model, N, env, st, X, U, **kw):
    """the case's environment on the handle, then gusto_lincov with store_S = 1"""
    set_env(s, model, env)
    return s.lincov(LC.options(model, N, TC.MODE, store_S=1), X, U, S0=LC.start(model, st), **kw)


def check(dev, tabs, ref, X, model, where):
    """one call's report and tables (gusto_get_env) against the restatement's five results"""
    for b in range(B):
        r = ref[b]
        n_obs = len(r["margin"])
        for f in INT_FIELDS:
            assert dev[f][b] == r[f], (where, b, f, dev[f][b], r[f])
        scale = max(1.0, np.abs(X[b][:, :V.WS_DIM[model]]).max())
        err = np.abs(dev["margin"][b, :n_obs] - r["margin"]).max() if n_obs else 0.0
        assert err <= TOL_KNOT * scale, (where, b, "margin", err)
        assert not dev["margin"][b, n_obs:].any(), (where, b)                          # zeros behind the problem's own count
        assert abs(dev["max_margin"][b] - r["max_margin"]) <= TOL_KNOT * scale, (where, b)
        e = rel(dev["min_z_base"][b], r["min_z_base"])
        assert e <= TOL_SUMMARY, (where, b, "min_z_base", e)
        for got, want in ((tabs[0][b], r["boxes"]), (tabs[1][b], r["spheres"])):
            assert got.shape == want.shape, (where, b)
            assert (np.abs(got - want).max() if want.size else 0.0) <= TOL_KNOT * scale, (where, b, "tables")


@pytest.mark.parametrize("model,N", TC.CASES)
def test_margins_tables_and_report_against_the_restatement(model, N):
    """every environment, start covariance and option set; with the base being the handle's set, min_z_base, knot and pair are
    those of the same call's gusto_lincov"""
    s, X, U = handle(model, N)
    for env in TC.ENVS:
        base = TC.base(model, env)
        for st in TC.STARTS:
            for name, o in TC.OPTION_SETS.items():
                if env != "batch" and name not in ("default", "reach"):
                    continue
                lc = analyse(s, model, N, env, st, X, U)
                assert lc["status"].all()
                dev = s.tighten_env(*base, monotone=0, **o)
                assert s.last_tighten_ms() > 0
                tabs = s.get_env()
                assert len(tabs[0]) == B
                ref = TC.reference(model, N, env, st, Sxx=lc["Sxx"], monotone=0, **o)
                check(dev, tabs, ref, X, model, (model, N, env, st, name))
                assert np.array_equal(dev["knot"], lc["obs_knot"]) and np.array_equal(dev["pair"], lc["obs_pair"])
                assert rel(dev["min_z_base"], lc["min_z_obs"]) <= TOL_SUMMARY
    s.close()


@pytest.mark.parametrize("model", TC.MODELS)
def test_monotone_memory_and_skipped_problems(model):
    """two calls with different kappa: monotone keeps the first call's margins, monotone = 0 does not; a problem inactive under
    gusto_set_active or with gusto_lincov status 0 keeps its margins, gets status 0 and still gets its tables; the memory
    outlives gusto_set_problems_replan and ends at gusto_set_env"""
    N, env, st = 50, "batch", "full"
    s, X, U = handle(model, N)
    base = TC.base(model, env)
    lc = analyse(s, model, N, env, st, X, U)
    first = s.tighten_env(*base, **TC.OPTION_SETS["default"])
    prev = [first["margin"][b, :len(r["margin"])] for b, r in enumerate(TC.reference(model, N, env, st, Sxx=lc["Sxx"]))]
    # monotone = 1 with a smaller kappa: the first call's margins, bit for bit
    keep = s.tighten_env(*base, **TC.SECOND)
    assert np.array_equal(keep["margin"], first["margin"])
    check(keep, s.get_env(), TC.reference(model, N, env, st, Sxx=lc["Sxx"], prev=prev, **TC.SECOND), X, model, "keep")
    # inactive problems 1 and 4 under monotone = 0: they keep, the others drop
    act = np.array([1, 0, 1, 1, 0], bool)
    s.set_active(act)
    drop = s.tighten_env(*base, monotone=0, **TC.SECOND)
    s.set_active(None)
    check(drop, s.get_env(), TC.reference(model, N, env, st, Sxx=lc["Sxx"], prev=prev, skipped=~act, monotone=0, **TC.SECOND), X, model, "drop")
    assert np.array_equal(drop["status"], act.astype(np.int32))
    assert np.array_equal(drop["margin"][~act], first["margin"][~act]) and (drop["margin"][3] < first["margin"][3]).any()
    prev = [drop["margin"][b, :len(p)] for b, p in enumerate(prev)]
    # gusto_lincov status 0 for problem 2: gains that overflow the covariance
    K = s.get_tvlqr().K.copy()
    K[2] *= 1e200
    lc0 = s.lincov(LC.options(model, N, TC.MODE, store_S=1), X, U, K=K, S0=LC.start(model, st))   # (no gusto_set_env: that would end the memory)
    assert list(lc0["status"]) == [1, 1, 0, 1, 1]
    dead = s.tighten_env(*base, **TC.OPTION_SETS["default"])
    assert list(dead["status"]) == [1, 1, 0, 1, 1] and np.array_equal(dead["margin"][2], drop["margin"][2])
    Sx = lc0["Sxx"].copy()
    Sx[2] = lc["Sxx"][2]                                             # (never read for a skipped problem)
    check(dead, s.get_env(), TC.reference(model, N, env, st, Sxx=Sx, prev=prev, skipped=[0, 0, 1, 0, 0]), X, model, "dead")
    # the memory outlives new problems on the handle ...
    tau, x0 = np.zeros(B), X[:, 0]
    s.set_problems_replan(tau, x0, mask=np.ones(B, bool))
    with pytest.raises(g.GustoError, match="-3"):
        s.get_tighten()                                              # (the report does not)
    with pytest.raises(g.GustoError, match="-3"):
        s.tighten_env(*base)                                         # (nor the covariances)
    assert s.tvlqr(tvlqr_opts(TC.MODE), X, U).status.all()
    lc = s.lincov(LC.options(model, N, TC.MODE, store_S=1), X, U, S0=LC.start(model, st))
    again = s.tighten_env(*base, **TC.SECOND)
    assert np.array_equal(again["margin"], dead["margin"])
    # ... and ends at gusto_set_env / gusto_set_env_batch
    set_env(s, model, env)
    lc = s.lincov(LC.options(model, N, TC.MODE, store_S=1), X, U, S0=LC.start(model, st))
    fresh = s.tighten_env(*base, **TC.SECOND)
    check(fresh, s.get_env(), TC.reference(model, N, env, st, Sxx=lc["Sxx"], **TC.SECOND), X, model, "fresh")
    assert (fresh["margin"][4] < dead["margin"][4]).all()
    s.close()


@pytest.mark.parametrize("model", TC.MODELS)
def test_a_problem_alone_and_in_the_batch_bit_for_bit(model):
    """B = 1: every problem of the batch of five on a handle of its own gives the batch's row, to the bit"""
    N, env, st = 50, "batch", "full"
    s, X, U = handle(model, N)
    base = TC.base(model, env)
    analyse(s, model, N, env, st, X, U)
    dev = s.tighten_env(*base, **TC.OPTION_SETS["reach"])
    tabs = s.get_env()
    s.close()
    _, _, tf, _ = LC.inputs(model, N)
    for b in range(B):
        one = solver(model, N, X[b:b + 1], U[b:b + 1], tf[b:b + 1], env, [b])
        assert one.tvlqr(tvlqr_opts(TC.MODE), X[b:b + 1], U[b:b + 1]).status.all()
        S0 = LC.start(model, st)
        one.lincov(LC.options(model, N, TC.MODE, store_S=1), X[b:b + 1], U[b:b + 1], S0=S0[b:b + 1])
        r = one.tighten_env([base[0][b]], [base[1][b]], **TC.OPTION_SETS["reach"])
        t1 = one.get_env()
        one.close()
        w = r["margin"].shape[1]
        for f in INT_FIELDS + ("min_z_base", "max_margin"):
            assert r[f][0].tobytes() == dev[f][b].tobytes(), (b, f)
        assert r["margin"][0].tobytes() == dev["margin"][b, :w].tobytes() and not dev["margin"][b, w:].any()
        assert t1[0][0].tobytes() == tabs[0][b].tobytes() and t1[1][0].tobytes() == tabs[1][b].tobytes()


def test_refusals_leave_the_handles_tables_as_they_were():
    model, N = 0, 4
    s, X, U = handle(model, N)
    boxes, spheres = TC.base(model, "sim")

    bx, sp = V.obstacles(boxes[0], spheres[0])

    def same():
        t = s.get_env()
        return len(t[0]) == 1 and t[0][0].tobytes() == np.ascontiguousarray(bx).tobytes() and t[1][0].tobytes() == np.ascontiguousarray(sp).tobytes()

    def refused(code, *a, **k):
        with pytest.raises(g.GustoError, match=str(code)):
            s.tighten_env(*a, **k)
        assert same()

    set_env(s, model, "sim")
    assert same()
    refused(-3, boxes, spheres)                                                   # no covariances yet
    s.lincov(LC.options(model, N, TC.MODE), X, U)
    refused(-3, boxes, spheres)                                                   # ... and none stored
    s.lincov(LC.options(model, N, TC.MODE, store_S=1), X, U)
    refused(-1, boxes * 2, spheres * 2)                                           # n_env neither 1 nor B
    refused(-1, [np.zeros((65, 6))])                                              # more than 64 components
    bad = np.array(bx, float)
    bad[0, 4] = np.nan
    refused(-1, [bad], spheres)                                                   # a non-finite entry
    for o in (dict(kappa=-1.0), dict(kappa=np.inf), dict(slack=-0.1), dict(slack=np.nan), dict(margin_cap=-1.0), dict(margin_cap=np.nan),
              dict(reach=np.nan), dict(cover_components=2), dict(monotone=-1)):
        refused(-1, boxes, spheres, **o)
    assert s.tighten_env(boxes, spheres)["status"].all() and len(s.get_env()[0]) == B and not same()
    s.close()
    d = g.BatchSolver(1, N, B, hist_cap=16)                                       # DubinsCar: no keep-out sets
    Xd, Ud, tfd, _ = LC.inputs(1, N)
    d.set_problems(Xd[:, 0], Xd[:, -1], Xd[:, -1], tfd, Xd, Ud)
    with pytest.raises(g.GustoError, match="-1"):
        d.tighten_env([None])
    d.close()
    t = g.TrajOptSolver(0, N, B)
    with pytest.raises(g.GustoError, match="TrajOpt"):
        t.tighten_env([None])
    rc = t.L.gusto_tighten_env(t.h, 1, np.zeros(1, np.int32).ctypes.data, None, np.zeros(1, np.int32).ctypes.data, None, None)
    assert rc == -1
    t.close()


def test_c_consumer(tmp_path):
    """tests/c/c_abi_tighten.c, a plain C consumer with checks of its own; what it prints is the Python path's"""
    exe = os.path.join(tmp_path, "c_abi_tighten")
    libdir = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_tighten.c"), "-o", exe, "-L" + libdir, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 4
    goal = [3.0, 0.5, 0, 0.05, -0.05, 0]
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.4, 1.9, 0, 0, 0, 0], [0.3, 0.4, 0, 0, 0, 0]], float)
    box = np.array([[1.4, 0.9, -0.2, 1.8, 1.5, 0.2]])
    s = g.BatchSolver(0, 50, 3, hist_cap=64, boxes=box)
    s.set_problems(x0, np.tile(goal, (3, 1)), np.tile(goal, (3, 1)), [200.0, 150.0, 100.0])
    s.solve(30)
    s.tvlqr({})
    s.lincov(dict(du_white=0.0074, store_S=1))
    r = s.tighten_env([box])
    tb = s.get_env()[0]
    for b in range(3):
        v = lines[1 + b].split()
        assert [int(x) for x in v[:5]] == [r[f][b] for f in INT_FIELDS]
        assert [float(x) for x in v[5:]] == [r["min_z_base"][b], r["margin"][b, 0], tb[b][0, 0], tb[b][0, 1], tb[b][0, 3], tb[b][0, 4]]
    s.close()


def test_chance_driver_on_table_queries():
    """solve_SCP_chance_batch on 16 table queries at N = 50: every query reported `met` passes gusto_verify and gusto_lincov on the
    base set, recomputed here on a handle of its own, and the driver's handle holds the base set again at the end, to the bit"""
    from test_gpu_multistart import host_problems
    H, P = g.host, g.problems
    Q, kappa = 16, 3.0
    TOPs, TOSs = host_problems(Q)
    lco = dict(dx0=[.02, .02, .02, .002, .002, .002], du0=0.0, du_white=0.0074)
    tvo = dict(Q=1.0, R=1.0, Qf=1.0, dt_min=0.1)
    out = H.solve_SCP_chance_batch(TOSs, TOPs, kappa=kappa, rounds=2, lincov_opts=lco, tvlqr_opts=tvo)
    assert len(out["rounds"]) >= 1 and out["rounds"][0]["tighten_ms"] > 0
    print("answered %d, met before %d, met after %d; rounds: %s" % (
        out["answered"].sum(), out["met_before"].sum(), out["met"].sum(),
        [(int(r["tried"].sum()), int(r["blocked"].sum()), int(r["second_pass"].sum()), int(r["lost"].sum())) for r in out["rounds"]]))
    assert not (out["met"] & ~out["answered"]).any()
    base = np.ascontiguousarray(P.freeflyer_env(), float)
    assert len(out["env"][0]) == 1 and out["env"][0][0].tobytes() == base.tobytes() and out["env"][1][0].size == 0   # the base, to the bit
    x0, lo, hi, tf = P.freeflyer_batch(Q)
    sp, mp = g.default_params(0)
    s = g.BatchSolver(0, 50, Q, hist_cap=64, boxes=P.freeflyer_env(), scp_params=sp, model_params=mp)
    s.set_problems(x0, lo, hi, tf)
    X = np.stack([TOSs[q].traj.X.T for q in range(Q)])
    U = np.stack([TOSs[q].traj.U.T for q in range(Q)])
    s.tvlqr(tvo, X, U)
    lc = s.lincov(lco, X, U)
    vr = s.verify(X, U)
    met = out["met"]
    assert (lc["min_z_obs"][met] >= kappa).all() and vr["collision_free"][met].all()
    assert np.array_equal(lc["min_z_obs"], out["min_z_obs"]) and np.array_equal(vr["collision_free"], out["collision_free"])
    s.close()
