"""tests/np_multistart.py, the numpy restatement of the multi-start entry points, proven without a GPU: the geometry of the fan
against host.init_traj_straightline and against its own definitions, the selection rule on hand-made scores, and the study
that motivates the feature, pinned on the CPU oracle (tests/test_gpu_multistart.py repeats it on the device)."""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import np_multistart as MS

ULP = 2.0 ** -52
PLANE_FAN = np.array([(0.0, 0.0), (0.5, 0.0), (-0.5, 0.0), (1.0, 0.0), (-1.0, 0.0)])
STUDY_B, STUDY_N, STUDY_ITERS = 48, 50, 30
STUDY_STRAIGHT_FAILS = {1, 5, 7, 37, 40}


def host_top(model, x_init, x_goal, N, tf):
    H = g.host
    gs = H.GoalSet()
    H.add_goal(gs, H.Goal(H.PointGoal(x_goal), tf, model))
    return H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.BlankEnv(), x_init, gs), N, tf, fixed_final_time=True)


@pytest.mark.parametrize("model_id", [0, 1, 2, 3])
def test_zero_offset_is_the_hosts_straight_line(model_id):
    H = g.host
    model = (H.FreeflyerSE2, H.DubinsCar, H.AstrobeeSE3, H.AstrobeeSE3Manifold)[model_id]()
    rng = np.random.default_rng(model_id)
    n = MS.X_DIM[model_id]
    for N in (3, 4, 50):
        x_init, x_goal = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
        ref = H.init_traj_straightline(host_top(model, x_init, x_goal, N, 40.0))
        for off in ((0.0, 0.0), (-0.0, 0.0)):
            assert np.array_equal(MS.fan_start(model_id, x_init, x_goal, x_goal, N, off), ref.X.T)
        if MS.WS_DIM[model_id] == 2:      # a3 is not read in the plane
            assert np.array_equal(MS.fan_start(model_id, x_init, x_goal, x_goal, N, (0.0, 0.7)), ref.X.T)
        _, _, _, _, X0, U0 = MS.fan_problems(model_id, x_init, x_goal, x_goal, 40.0, N, [(0, 0), (0.3, -0.2)])
        assert np.array_equal(X0[0], ref.X.T) and not U0.any() and U0.shape == (2, N, MS.U_DIM[model_id])


@pytest.mark.parametrize("model_id", [0, 1, 2, 3])
def test_end_knots_and_the_entries_behind_the_workspace_are_the_straight_lines(model_id):
    rng = np.random.default_rng(10 + model_id)
    n, ws = MS.X_DIM[model_id], MS.WS_DIM[model_id]
    for N in (3, 4, 50):
        tt = MS.tent(N)
        assert tt[0] == 0.0 and tt[-1] == 0.0 and tt.max() <= 1.0 and (tt[1:-1] > 0).all()
        x_init, x_goal = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
        line = MS.straight_line(x_init, x_goal, x_goal, N)
        for off in ((0.5, 0.0), (-1.0, 0.25), (0.0, 0.5)):
            X = MS.fan_start(model_id, x_init, x_goal, x_goal, N, off)
            assert np.array_equal(X[0], line[0]) and np.array_equal(X[-1], line[-1])
            assert np.array_equal(X[:, ws:], line[:, ws:])
    assert MS.tent(3)[1] == 1.0


def test_planar_apex():
    """N = 3: the middle knot is the midpoint moved by a2 along e2, the left normal of the direction of travel"""
    x_init, x_goal = np.array([1.0, 2.0, 0.3, 0, 0, 0]), np.array([4.0, 6.0, -0.2, 0, 0, 0])
    X = MS.fan_start(0, x_init, x_goal, x_goal, 3, (0.5, 0.0))
    e1, e2 = MS.frame(2, x_init[:2], x_goal[:2])
    assert np.array_equal(e1, [0.6, 0.8]) and np.array_equal(e2, [-0.8, 0.6])
    mid = 0.5 * x_init + 0.5 * x_goal
    assert np.array_equal(X[1, :2], mid[:2] + 0.5 * e2) and np.array_equal(X[1, 2:], mid[2:])
    assert np.array_equal(MS.fan_start(0, x_init, x_goal, x_goal, 3, (-0.5, 0.0))[1, :2], mid[:2] - 0.5 * e2)


def orthonormal_error(f):
    E = np.stack(f)
    return np.abs(E @ E.T - np.eye(len(E))).max()


def test_frames_are_orthonormal():
    """to 4 ulp: random directions, the axes, d along z (both signs), L == 0, and both sides of the threshold on h.  With
    0 < h <= 1e-9 the definition's e2 = (1, 0, 0) is orthogonal to e1 only up to h, which is what the header says."""
    rng = np.random.default_rng(5)
    for ws in (2, 3):
        dirs = [rng.normal(size=ws) * 10.0 ** rng.integers(-3, 4) for _ in range(200)] + list(np.eye(ws)) + list(-np.eye(ws))
        for d in dirs:
            p = rng.uniform(-5, 5, ws)
            f = MS.frame(ws, p, p + d)
            assert orthonormal_error(f) <= 4 * ULP, (d, orthonormal_error(f))
        f = MS.frame(ws, np.ones(ws), np.ones(ws))                      # L == 0: the axes themselves
        assert np.array_equal(np.stack(f), np.eye(ws))
    for z in (2.5, -2.5):                                               # d along z: h == 0
        f = MS.frame(3, np.array([1.0, 2.0, 3.0]), np.array([1.0, 2.0, 3.0 + z]))
        assert np.array_equal(f[0], [0, 0, np.sign(z)]) and np.array_equal(f[1], [1, 0, 0]) and np.array_equal(f[2], [0, np.sign(z), 0])
        assert orthonormal_error(f) == 0.0
    above = MS.frame(3, np.zeros(3), np.array([1.2e-9, 1.6e-9, 1.0]))   # h = 2e-9 > 1e-9: the regular branch
    assert above[1][2] == 0.0 and abs(above[1][0] + 0.8) < 1e-15 and abs(above[1][1] - 0.6) < 1e-15 and orthonormal_error(above) <= 4 * ULP
    below = MS.frame(3, np.zeros(3), np.array([3e-10, 4e-10, 1.0]))     # h = 5e-10: the fallback
    assert np.array_equal(below[1], [1, 0, 0]) and orthonormal_error(below) <= 5e-10 * (1 + 4 * ULP)


def test_replication_and_layout():
    rng = np.random.default_rng(7)
    x_init, lo = rng.uniform(-1, 1, (3, 12)), rng.uniform(-1, 1, (3, 12))
    hi = lo + np.array([0.0, 0.2, 0.0])[:, None]
    hi[2, 1], lo[2, 4] = np.inf, -np.inf
    tf = np.array([10.0, 20.0, 30.0])
    fan = [(0, 0), (0.5, 0), (0, -0.5), (0.25, 0.25)]
    xi, l, h, t, X0, U0 = MS.fan_problems(2, x_init, lo, hi, tf, 4, fan)
    assert X0.shape == (12, 4, 12) and U0.shape == (12, 4, 6)
    for q in range(3):
        for j in range(4):
            b = q * 4 + j
            assert np.array_equal(xi[b], x_init[q]) and np.array_equal(l[b], lo[q]) and np.array_equal(h[b], hi[q]) and t[b] == tf[q]
            assert np.array_equal(X0[b], MS.fan_start(2, x_init[q], lo[q], hi[q], 4, fan[j]))
    c = MS.goal_centre(lo[2], hi[2])
    assert c[1] == 0.0 and c[4] == 0.0 and c[0] == 0.5 * (lo[2, 0] + hi[2, 0])


def test_selection_rule():
    nan, inf = np.nan, np.inf
    #            query 0: a tie of bit-equal scores   1: a NaN beside finite ones   2: nothing eligible   3: eligible NaNs only
    score = np.array([3.0, 1.5, 1.5, 2.0, nan, 4.0, 0.5, 3.5, 1.0, 2.0, 3.0, 4.0, nan, nan, 1.0, nan])
    elig = np.array([1, 1, 1, 1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 1, 0, 1])
    X = np.arange(16 * 6, dtype=float).reshape(16, 3, 2) + 1
    r = MS.select_best(4, score, elig, X=X)
    assert list(r["winner"]) == [1, 3, -1, -1] and list(r["winner_problem"]) == [1, 7, -1, -1]
    assert list(r["n_eligible"]) == [4, 3, 0, 3] and list(r["best_score"]) == [1.5, 3.5, inf, inf]
    assert np.array_equal(r["X"][0], X[1]) and np.array_equal(r["X"][1], X[7]) and not r["X"][2:].any()
    r1 = MS.select_best(1, score, elig)                                  # K = 1: every eligible problem with a number wins
    assert list(r1["winner"]) == [0 if e and s == s else -1 for s, e in zip(score, elig)]
    assert list(r1["winner_problem"]) == [b if w == 0 else -1 for b, w in enumerate(r1["winner"])]
    r16 = MS.select_best(16, score, elig)
    assert list(r16["winner"]) == [1] and r16["n_eligible"][0] == 10 and r16["best_score"][0] == 1.5
    assert list(MS.select_best(2, [inf, inf, -0.0, 0.0], [1, 1, 1, 1])["winner"]) == [0, 0]   # +inf can win; -0.0 == 0.0 is a tie
    assert list(MS.select_best(2, [inf, 1.0], [0, 0])["best_score"]) == [inf]


@functools.lru_cache(maxsize=None)
def oracle_study():
    """the 240 starts of the first 48 table problems on the oracle: (results [48][5], selection report)"""
    import gusto_oracle as go
    P = g.problems
    x0, glo, ghi, tf = P.freeflyer_batch(STUDY_B)
    o = go.Oracle(go.FREEFLYER_SE2, STUDY_N, boxes=P.freeflyer_env())
    xi, lo, hi, t, X0, U0 = MS.fan_problems(0, x0, glo, ghi, tf, STUDY_N, PLANE_FAN)
    res = []
    for b in range(len(xi)):
        o.set_problem(xi[b], lo[b], hi[b], t[b], X0[b], U0[b])
        res.append(o.solve(STUDY_ITERS))
    ok = np.array([r["converged"] and r["successful"] for r in res])
    cost = np.array([r["J_true"][-1] for r in res])
    return res, MS.select_best(len(PLANE_FAN), cost, ok)


def test_oracle_study_is_pinned():
    """the straight line is successful on 43 of the 48 problems, every failure converged; the fan of five yields a winner for all;
    start 0 of the fan IS the oracle's own straight-line solve"""
    import gusto_oracle as go
    P = g.problems
    res, best = oracle_study()
    K = len(PLANE_FAN)
    straight = res[0::K]
    fails = {q for q, r in enumerate(straight) if not (r["converged"] and r["successful"])}
    assert fails == STUDY_STRAIGHT_FAILS and all(straight[q]["converged"] for q in fails)
    assert (best["winner"] >= 0).all() and all(best["winner"][q] > 0 for q in fails)
    better = [q for q in range(STUDY_B) if q not in fails and best["best_score"][q] < 0.95 * straight[q]["J_true"][-1]]
    assert len(better) == 3, better
    x0, glo, ghi, tf = P.freeflyer_batch(STUDY_B)
    o = go.Oracle(go.FREEFLYER_SE2, STUDY_N, boxes=P.freeflyer_env())
    for q in (0, 1, 40):
        o.set_problem(x0[q], glo[q], ghi[q], tf[q])
        r = o.solve(STUDY_ITERS)
        assert np.array_equal(r["X"], straight[q]["X"]) and r["iterations"] == straight[q]["iterations"]
