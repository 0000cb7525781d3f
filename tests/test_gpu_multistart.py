"""gusto_set_problems_multistart, gusto_select_best, gusto_get_best and gusto_get_best_dev on the device against tests/np_multistart.py,
the numpy restatement (tests/test_multistart_cpu.py proves it without a GPU), against gusto_set_problems on the same handle, against
plain solves, and on the study that motivates them: the 48 table problems, fanned, next to the CPU oracle.

Tolerances.  Everything is compared bit for bit except
  - the workspace entries of the starts with an offset: 16 ulp of (max(|x_init_i|, |centre_i|) + |a2| + |a3|) absolute per entry, from
    the roundings of the definition (two products and a sum for the straight line, the direction, its length, the division, the hypot
    and the division of e2, the cross product, two products and a sum for w, the tent and its product) with a margin of two; not
    measured on the device;
  - the comparison with the oracle: what tests/test_gpu_parity.py grants whole solves of freeflyerSE2 (test_scp_parity_freeflyer): one
    problem whose decisions differ, and J_true to 1e-4 relative, scaled by max(1, omega_max / 1e3)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import np_multistart as MS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52
PLANE_FAN = np.array([(0.0, 0.0), (0.5, 0.0), (-0.5, 0.0), (1.0, 0.0), (-1.0, 0.0)])
PARITY_MAX_DIVERGED, PARITY_RTOL = 1, 1e-4      # tests/test_gpu_parity.py: test_scp_parity_freeflyer, _scp_parity


# ---- 1. the fan -------------------------------------------------------------------------------------------------------------
def query(model, kind, rng):
    """(x_init, goal_lo, goal_hi) of one query: "point" goals, a "box" goal on the workspace, a coordinate with "inf" bounds (a
    workspace one: its centre is 0), "zero": d = 0, "vertical": d along z (in the plane: along y)"""
    n, ws = MS.X_DIM[model], MS.WS_DIM[model]
    x_init, c = rng.uniform(-2, 2, n), rng.uniform(-2, 2, n)
    lo, hi = c.copy(), c.copy()
    if kind == "box":
        lo[:ws] -= rng.uniform(0.05, 0.4, ws)
        hi[:ws] += rng.uniform(0.05, 0.4, ws)
    elif kind == "inf":
        lo[1], hi[ws - 1], hi[n - 1] = -np.inf, np.inf, np.inf
    elif kind == "zero":
        lo[:ws] = hi[:ws] = x_init[:ws]
    elif kind == "vertical":
        lo[:ws - 1] = hi[:ws - 1] = x_init[:ws - 1]
        lo[ws - 1] = hi[ws - 1] = x_init[ws - 1] - 1.75
    return x_init, lo, hi


def fan_of(K, rng):
    """start 0 the straight line (K = 1: one offset start), an e3-only start, a second zero offset, the rest anywhere in +-1 m"""
    if K == 1:
        return np.array([(0.4, -0.3)])
    fan = rng.uniform(-1, 1, (K, 2))
    fan[0] = 0.0
    if K >= 5:
        fan[2], fan[3], fan[4] = (0.0, 0.6), (-0.0, 0.0), (-0.75, 0.0)
    return fan


COMBOS = ((1, 1, ("point",)), (2, 3, ("box", "inf", "zero")), (5, 3, ("point", "vertical", "box")), (64, 1, ("vertical",)),
          (64, 3, ("zero", "point", "inf")))


@pytest.mark.parametrize("N", [3, 4, 50])
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_fan_against_the_restatement(model, N):
    """X, U of every start against the restatement and against gusto_set_problems with X0 = NULL on the same handle for the
    replicated inputs; the replicated x_init at knot 1, the goal centre at knot N, tf through the verify stage's nfull, and x_init,
    goal_lo, goal_hi, tf together through one convex subproblem, which reads all four: bit for bit what gusto_set_problems gives"""
    rng = np.random.default_rng(100 * model + N)
    n, ws = MS.X_DIM[model], MS.WS_DIM[model]
    sp, mp = g.default_params(model)
    s = g.BatchSolver(model, N, 192, hist_cap=8)
    for K, Bq, kinds in COMBOS:
        qs = [query(model, k, rng) for k in kinds]
        x_init, lo, hi = (np.stack([q[i] for q in qs]) for i in range(3))
        tf = np.array([21.0, 27.0, 34.0])[:Bq]
        dt_min = 2.5 / (N - 1)                             # 9, 11 and 14 substeps per interval: nfull tells the tf apart
        fan = fan_of(K, rng)
        s.set_problems_multistart(x_init, lo, hi, tf, fan)
        assert s.B == Bq * K
        X, U = s.traj()
        nfull, _, _ = s.interpolate(dt_min=dt_min)
        sub = s.subproblem(X, U, sp.Delta0, sp.omega0, sp.Delta0 / 8 + mp.clearance) if K == 2 else None
        xi, l, h, t, Xr, Ur = MS.fan_problems(model, x_init, lo, hi, tf, N, fan)
        assert list(nfull) == [{21.0: 9, 27.0: 11, 34.0: 14}[v] * (N - 1) + 1 for v in t]
        s.set_problems(xi, l, h, t)                        # the straight lines of the replicated inputs, same handle
        Xs, Us = s.traj()
        assert np.array_equal(U, Us) and not U.any()
        assert np.array_equal(X[:, :, ws:], Xs[:, :, ws:])
        assert np.array_equal(X[:, 0], xi) and np.array_equal(X[:, -1], MS.goal_centre(l, h))
        for b in range(Bq * K):
            a2, a3 = fan[b % K][0], fan[b % K][1] if ws == 3 else 0.0
            if a2 == 0 and a3 == 0:
                assert np.array_equal(X[b], Xs[b]), (K, b)
                continue
            bound = 16 * ULP * (np.maximum(np.abs(xi[b, :ws]), np.abs(MS.goal_centre(l[b], h[b])[:ws])) + abs(a2) + abs(a3))
            err = np.abs(X[b, :, :ws] - Xr[b, :, :ws])
            assert (err <= bound[None, :]).all(), (K, b, err.max(), bound)
            assert not np.array_equal(X[b, 1, :ws], Xs[b, 1, :ws])       # (the detour is there)
        if sub is not None:
            s.set_problems(xi, l, h, t, X, U)
            ref = s.subproblem(X, U, sp.Delta0, sp.omega0, sp.Delta0 / 8 + mp.clearance)
            for f in ("X", "U", "obj", "status", "iters", "dual"):
                assert np.array_equal(sub[f], ref[f], equal_nan=True), (f, K)
    s.close()


# ---- 2. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_and_state_errors():
    P = g.problems
    x0, glo, ghi, tf = P.freeflyer_batch(4)
    s = g.BatchSolver(0, 50, 12, hist_cap=8)
    L, h = s.L, s.h
    rep = g._capi.BestReport()
    ptr = lambda a: np.ascontiguousarray(a, float).ctypes.data
    fan3 = np.array([(0, 0), (0.5, 0), (-0.5, 0)], float)
    call = lambda Bq, K, fan, xi=x0: L.gusto_set_problems_multistart(h, Bq, K, None if xi is None else ptr(xi), ptr(glo), ptr(ghi), ptr(tf),
                                                                   None if fan is None else ptr(fan))
    assert L.gusto_get_best(h, C.byref(rep)) == -3 and L.gusto_select_best(h, 1, None, None) == -3      # no problems
    assert call(4, 0, fan3) == -1 and b"GUSTO_MAX_STARTS" in L.gusto_last_error(h)
    assert call(1, 65, np.zeros((65, 2))) == -1
    assert call(0, 3, fan3) == -1
    assert call(3, 5, np.zeros((5, 2))) == -1 and b"batch_cap" in L.gusto_last_error(h)            # 15 = batch_cap + 3
    assert L.gusto_set_problems_multistart(h, 13, 1, ptr(np.zeros((13, 6))), ptr(np.zeros((13, 6))), ptr(np.zeros((13, 6))),
                                           ptr(np.ones(13)), ptr(np.zeros((1, 2)))) == -1        # batch_cap + 1
    for bad in (np.nan, np.inf, -np.inf):
        f = fan3.copy()
        f[1, 1] = bad
        assert call(4, 3, f) == -1 and b"start 1" in L.gusto_last_error(h)
    assert call(4, 3, None) == -1 and call(4, 3, fan3, None) == -1
    assert L.gusto_set_problems_multistart(None, 4, 3, ptr(x0), ptr(glo), ptr(ghi), ptr(tf), ptr(fan3)) == -1
    assert L.gusto_get_traj(h, None, None) == -3            # every refusal left the handle as it was: without problems
    assert call(4, 3, fan3) == 0                              # batch_cap itself
    s.B = 12
    assert L.gusto_get_best(h, C.byref(rep)) == -3 and L.gusto_get_best_dev(h, None, None, None) == -3      # no select yet
    assert b"gusto_select_best" in L.gusto_last_error(h)
    for K in (5, 7, 0, -1, 65, 24):
        assert L.gusto_select_best(h, K, None, None) == -1, K
    before = s.traj()
    assert call(3, 5, np.zeros((5, 2))) == -1 and call(4, 3, None) == -1      # refused with problems set: they stay
    after = s.traj()
    assert s.B == 12 and np.array_equal(before[0], after[0])
    r = s.select_best(3, score=np.arange(12.0), eligible=np.ones(12))
    assert list(r["winner"]) == [0, 0, 0, 0] and L.gusto_get_best(h, None) == 0
    s.set_problems(x0, glo, ghi, tf)                          # new problems: the selection is gone
    assert L.gusto_get_best(h, C.byref(rep)) == -3 and L.gusto_get_best_dev(h, None, None, None) == -3
    s.select_best(2, score=np.arange(4.0), eligible=np.ones(4))
    s.set_problems_multistart(x0, glo, ghi, tf, fan3)         # ... and after the fanned form of it
    assert L.gusto_get_best(h, C.byref(rep)) == -3
    s.close()
    t = g._capi.TrajOptSolver(0, 50, 12)
    assert t.L.gusto_set_problems_multistart(t.h, 4, 3, ptr(x0), ptr(glo), ptr(ghi), ptr(tf), ptr(fan3)) == -1
    assert b"TrajOpt" in t.L.gusto_last_error(t.h)
    t.set_problems(x0, glo, ghi, tf)
    assert t.L.gusto_select_best(t.h, 2, None, None) == -1 and t.L.gusto_get_best(t.h, None) == -1
    assert t.L.gusto_get_best_dev(t.h, None, None, None) == -1
    for f in (t.set_problems_multistart, t.select_best):
        with pytest.raises(g._capi.GustoError):
            f()
    t.close()


# ---- 3. the selection -------------------------------------------------------------------------------------------------------
def check_select(s, K, score, elig, X, U, st=None, hist=None):
    """select_best on the handle against the restatement, exactly; the _dev views against the host report"""
    r = s.select_best(K, score=score, eligible=elig)
    if score is None or elig is None:
        dsc, del_ = MS.default_inputs(st if st is not None else s.status(), hist if hist is not None else s.history())
        score_r, elig_r = (dsc if score is None else score), (del_ if elig is None else elig)
    else:
        score_r, elig_r = score, elig
    ref = MS.select_best(K, score_r, elig_r, X=X, U=U)
    for f in ("winner", "winner_problem", "n_eligible", "best_score", "X", "U"):
        assert np.array_equal(r[f], ref[f]), (K, f, r[f], ref[f])
    Xd, Ud, wd = s.best_dev(s.B // K)
    assert np.array_equal(Xd.cpu().numpy(), r["X"]) and np.array_equal(Ud.cpu().numpy(), r["U"])
    assert np.array_equal(wd.cpu().numpy(), r["winner_problem"])
    return r


def test_select_against_the_restatement():
    rng = np.random.default_rng(3)
    nan = np.nan
    B, N = 12, 3
    x0, glo, ghi, tf = g.problems.freeflyer_batch(B)
    X0, U0 = rng.normal(size=(B, N, 6)), rng.normal(size=(B, N, 3))
    s = g.BatchSolver(0, N, B, hist_cap=8)
    s.set_problems(x0, glo, ghi, tf, X0, U0)
    #                 a tie of bit-equal scores          a NaN beside finite ones     nothing eligible
    score = np.array([3.0, 1.5, 1.5, 2.0, nan, 4.0, 0.5, 3.5, 1.0, 2.0, 3.0, 4.0])
    elig = np.array([1, 1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0])
    for K in (1, 3, 4, 12):
        check_select(s, K, score, elig, X0, U0)
    r = check_select(s, 4, score, elig, X0, U0)
    assert list(r["winner"]) == [1, 3, -1] and list(r["n_eligible"]) == [4, 3, 0] and not r["X"][2].any() and not r["U"][2].any()
    r = check_select(s, 3, np.array([nan, nan, nan, 1.0, -np.inf, np.inf, np.inf, np.inf, nan, -0.0, 0.0, 5.0]), np.ones(B), X0, U0)
    assert list(r["winner"]) == [-1, 1, 0, 0] and list(r["n_eligible"]) == [3, 3, 3, 3]
    # before any solve the default score is NaN (no cost entry) and nothing is converged: eligible given, and score given
    r = check_select(s, 4, None, elig, X0, U0)
    assert list(r["winner"]) == [-1, -1, -1] and list(r["n_eligible"]) == [4, 3, 0]
    r = check_select(s, 4, score, None, X0, U0)
    assert list(r["winner"]) == [-1, -1, -1] and not r["n_eligible"].any()
    before = s.traj()
    assert np.array_equal(before[0], X0) and np.array_equal(before[1], U0)      # the call changes nothing else
    s.close()
    # the widest row and a full wave of starts
    B, N, K = 128, 4, 64
    X0, U0 = rng.normal(size=(B, N, 13)), rng.normal(size=(B, N, 6))
    s = g.BatchSolver(3, N, B, hist_cap=8)
    s.set_problems(X0[:, 0], X0[:, -1], X0[:, -1], np.full(B, 40.0), X0, U0)
    score = rng.integers(0, 12, B).astype(float)         # many ties
    score[rng.integers(0, B, 10)] = nan
    elig = rng.integers(0, 4, B) > 0
    elig[63], score[63], score[:63] = True, -1.0, np.where(np.isnan(score[:63]), nan, score[:63] + 5)    # the last lane wins query 0
    r = check_select(s, K, score, elig, X0, U0)
    assert r["winner"][0] == 63 and r["winner"][1] >= 0
    check_select(s, K, score, np.zeros(B), X0, U0)
    check_select(s, 32, score, elig, X0, U0)
    s.close()


# ---- 4. - 6. fanned solves ----------------------------------------------------------------------------------------------------
def snapshot(s):
    X, U = s.traj()
    return dict(X=X, U=U, st=s.status(), h=s.history())


@functools.lru_cache(maxsize=None)
def fanned(Bq):
    """the first Bq table problems, freeflyerSE2, N = 50, K = 5, 30 iterations, with select_best on the defaults (shared, not written to)"""
    P = g.problems
    x0, glo, ghi, tf = P.freeflyer_batch(Bq)
    s = g.BatchSolver(0, 50, Bq * 5, hist_cap=40, boxes=P.freeflyer_env())
    s.set_problems_multistart(x0, glo, ghi, tf, PLANE_FAN)
    s.solve(30)
    out = snapshot(s)
    out["best"] = s.select_best(5)
    out["solver"] = s
    return out


@functools.lru_cache(maxsize=None)
def plain(Bq):
    P = g.problems
    x0, glo, ghi, tf = P.freeflyer_batch(Bq)
    s = g.BatchSolver(0, 50, Bq, hist_cap=40, boxes=P.freeflyer_env())
    s.set_problems(x0, glo, ghi, tf)
    s.solve(30)
    out = snapshot(s)
    s.close()
    return out


def test_default_score_and_eligibility():
    f = fanned(8)
    s = f["solver"]
    score, elig = MS.default_inputs(f["st"], f["h"])
    ref = MS.select_best(5, score, elig, X=f["X"], U=f["U"])
    for k in ("winner", "winner_problem", "n_eligible", "best_score", "X", "U"):
        assert np.array_equal(f["best"][k], ref[k]), k
    assert (f["best"]["winner"] >= 0).any() and np.isfinite(score).all()
    # eligible given with the default score, and the other way round
    el = np.ones(40)
    el[f["best"]["winner_problem"][f["best"]["winner"] >= 0]] = 0        # the winners of the default run may not win
    r = check_select(s, 5, None, el, f["X"], f["U"], f["st"], f["h"])
    assert all(a != b for a, b in zip(r["winner"], f["best"]["winner"]) if b >= 0)
    check_select(s, 5, -score, None, f["X"], f["U"], f["st"], f["h"])     # the most expensive successful start
    check_select(s, 5, None, None, f["X"], f["U"], f["st"], f["h"])


def test_a_fanned_batch_changes_no_problems_result():
    """start 0 of every query is the plain solve of that problem on a second handle, bit for bit; a query's report does not depend
    on the batch it sits in"""
    f, p = fanned(8), plain(8)
    z = np.arange(8) * 5
    for k in ("iterations", "converged", "successful", "stop_reason", "ipm_iters"):
        assert np.array_equal(f["st"][k][z], p["st"][k]), k
    assert np.array_equal(f["X"][z], p["X"]) and np.array_equal(f["U"][z], p["U"])
    for k in ("n_hist", "nJ", "n_rho"):
        assert np.array_equal(f["h"][k][z], p["h"][k]), k
    for q in range(8):
        for k, cnt in (("J_true", "nJ"), ("J_full", "nJ"), ("omega", "n_hist"), ("Delta", "n_hist"), ("scp_status", "n_hist")):
            c = p["h"][cnt][q]
            assert np.array_equal(f["h"][k][5 * q, :c], p["h"][k][q, :c]), (q, k)
    f3 = fanned(3)
    for k in ("winner", "n_eligible", "best_score", "X", "U"):
        assert np.array_equal(f3["best"][k], f["best"][k][:3]), k
    assert np.array_equal(f3["X"], f["X"][:15]) and np.array_equal(f3["st"]["iterations"], f["st"]["iterations"][:15])


def test_the_fan_rescues_what_the_straight_line_loses():
    """the 48 problems of the CPU study on the device, next to the oracle on the same 240 starts"""
    from test_multistart_cpu import STUDY_B, oracle_study
    res, obest = oracle_study()
    f = fanned(STUDY_B)
    best = f["best"]
    has, ohas = best["winner"] >= 0, obest["winner"] >= 0
    differ = np.flatnonzero(has != ohas)
    print("queries with a winner: device %d, oracle %d; differing %s" % (has.sum(), ohas.sum(), list(differ)))
    assert len(differ) <= PARITY_MAX_DIVERGED, differ
    _, elig = MS.default_inputs(f["st"], f["h"])
    straight = elig[0::5]
    print("device: straight line successful on %d of %d, with the fan %d" % (straight.sum(), STUDY_B, has.sum()))
    assert has.sum() > straight.sum() and (has | ~straight).all()
    same = np.flatnonzero(has & ohas & (best["winner"] == obest["winner"]))
    print("same winning start on %d queries" % len(same))
    # (a differing winner needs two starts of a query whose costs lie closer than the parity tolerance, or a diverged solve: the
    # exception, so the comparison below covers the majority)
    assert len(same) > STUDY_B // 2
    for q in same:
        r = res[obest["winner_problem"][q]]
        w = max(1.0, r["omega"].max() / 1e3)
        e = abs(best["best_score"][q] - obest["best_score"][q]) / abs(obest["best_score"][q])
        assert e <= PARITY_RTOL * w, (q, e)


# ---- 7. the drivers -----------------------------------------------------------------------------------------------------------
def host_problems(B):
    H, P = g.host, g.problems
    model = H.FreeflyerSE2()
    env = H.Environment(P.freeflyer_env())
    x0, glo, ghi, tf = P.freeflyer_batch(B)
    TOPs = []
    for b in range(B):
        gs = H.GoalSet()
        H.add_goal(gs, H.Goal(H.PointGoal(glo[b]), tf[b], model))
        TOPs.append(H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, env, x0[b], gs), 50, tf[b], fixed_final_time=True))
    return TOPs, [H.TrajectoryOptimizationSolution(t) for t in TOPs]


def test_host_drivers():
    """policy "all" and "retry" solve the same queries; "retry" leaves a first-pass success untouched; the winner's SCPSolution"""
    H = g.host
    B = 16
    TOPs, TOSa = host_problems(B)
    a = H.solve_SCP_multistart_batch(TOSa, TOPs, policy="all")
    _, TOSr = host_problems(B)
    r = H.solve_SCP_multistart_batch(TOSr, TOPs, policy="retry")
    p = plain(B)
    f = fanned(B)
    ok = p["st"]["converged"] & p["st"]["successful"]
    assert not ok.all() and ok.any()
    solved_a, solved_r = [x["winner"] >= 0 for x in a], [x["winner"] >= 0 for x in r]
    assert solved_a == solved_r == list(f["best"]["winner"] >= 0) and sum(solved_a) > ok.sum()
    for q in range(B):
        assert a[q]["winner"] == f["best"]["winner"][q] and a[q]["cost"] == f["best"]["best_score"][q]
        assert a[q]["SCPS"] is TOSa[q].SCPS and TOSa[q].traj is a[q]["SCPS"].traj
        if a[q]["winner"] >= 0:
            assert np.array_equal(a[q]["SCPS"].traj.X.T, f["best"]["X"][q]) and a[q]["SCPS"].successful and a[q]["SCPS"].J_true[-1] == a[q]["cost"]
        if ok[q]:      # untouched by the retry: the plain solve, bit for bit
            assert r[q]["winner"] == 0 and np.array_equal(r[q]["SCPS"].traj.X.T, p["X"][q]) and np.array_equal(r[q]["SCPS"].traj.U.T, p["U"][q])
            assert r[q]["cost"] == p["h"]["J_true"][q, p["h"]["nJ"][q] - 1]
        else:          # re-solved from the fan: what the fanned launch found for it
            assert r[q]["winner"] == a[q]["winner"] and r[q]["cost"] == a[q]["cost"]
            assert np.array_equal(r[q]["SCPS"].traj.X.T, a[q]["SCPS"].traj.X.T)
    with pytest.raises(ValueError):
        H.solve_SCP_multistart_batch(TOSa, TOPs, policy="some")


def test_per_query_environments_are_repeated():
    """boxes / spheres per query through set_problems_multistart: the same results as the shared environment"""
    P = g.problems
    f = fanned(3)
    x0, glo, ghi, tf = P.freeflyer_batch(3)
    s = g.BatchSolver(0, 50, 15, hist_cap=40)
    s.set_problems_multistart(x0, glo, ghi, tf, PLANE_FAN, boxes=[P.freeflyer_env()] * 3)
    s.solve(30)
    X, _ = s.traj()
    r = s.select_best(5)
    s.close()
    assert np.array_equal(X, f["X"]) and np.array_equal(r["winner"], f["best"]["winner"])


def test_c_consumer(tmp_path):
    """tests/c/c_abi_multistart.c, a plain C consumer with checks of its own; the winners it prints are the Python path's"""
    exe = os.path.join(tmp_path, "c_abi_multistart")
    lib = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_multistart.c"), "-o", exe, "-L" + lib, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 4
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.4, 1.9, 0, 0, 0, 0], [0.3, 0.4, 0, 0, 0, 0]], float)
    goal = np.tile([3.0, 0.5, 0, 0.05, -0.05, 0], (3, 1))
    s = g.BatchSolver(0, 50, 9, hist_cap=64, boxes=np.array([[1.4, 0.9, -0.2, 1.8, 1.5, 0.2]]))
    s.set_problems_multistart(x0, goal, goal, [200.0, 150.0, 100.0], PLANE_FAN[:3])
    s.solve(30)
    r = s.select_best(3)
    s.close()
    for q in range(3):
        v = lines[1 + q].split()
        assert (int(v[0]), int(v[1]), int(v[2])) == (r["winner"][q], r["winner_problem"][q], r["n_eligible"][q])
        assert float(v[3]) == r["best_score"][q]


def test_post_solve_stages_on_the_winners_only():
    """gusto_set_active built from winner_problem, then gusto_verify: the winners' reports are those of the unmasked call, the other
    problems' stay as the call before left them"""
    f = fanned(8)
    s = f["solver"]
    wp = f["best"]["winner_problem"]
    mask = np.zeros(40, bool)
    mask[wp[wp >= 0]] = True
    s.set_active(None)
    full = s.verify(nstep=2)
    s.verify(nstep=1)                   # another roll-out: max_gap and min_dist_dense change
    other = s.get_verify()
    assert not np.array_equal(other["max_gap"], full["max_gap"])
    s.set_active(mask)
    masked = s.verify(nstep=2)
    s.set_active(None)
    for k in full:
        assert np.array_equal(masked[k][mask], full[k][mask]), k
        assert np.array_equal(masked[k][~mask], other[k][~mask]), k
    assert 0 < mask.sum() < 40
