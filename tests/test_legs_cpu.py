"""tests/np_legs.py, the numpy restatement of the goal timeline, proven without a GPU: the leg seeds against
host.init_traj_straightline, the advance rule on hand-made verdict tables, the join's indices, junction rule and time grid,
host._timeline_of on GoalSets, the refusals of the argument check, and the study that motivates the feature, pinned on the CPU
oracle (tests/test_gpu_legs.py repeats tables and join on the device)."""
import functools
import os
import re

import numpy as np
import pytest

import gusto_jl_amd as g
import np_legs as NL
import np_multistart as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUDY_Q, STUDY_N, STUDY_ITERS, STUDY_L = 48, 50, 30, 3
# the study on the oracle (profiles/legs.txt, section 1): the queries that fail and the leg they fail at, the trips per round
STUDY_FAILED = {5: 1, 6: 0, 19: 1, 20: 0, 37: 1, 38: 0}
STUDY_TRIPS = [274, 296, 313]


def host_model(model_id):
    H = g.host
    return (H.FreeflyerSE2, H.DubinsCar, H.AstrobeeSE3, H.AstrobeeSE3Manifold)[model_id]()


def host_top(model, x_init, lo, hi, N, tf):
    H = g.host
    gs = H.GoalSet()
    H.add_goal(gs, H.Goal(H.BoxGoal(lo, hi), tf, model))
    return H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.BlankEnv(), x_init, gs), N, tf, fixed_final_time=True)


def timeline(model_id, Bq, L, rng, points=False):
    """random timelines; unless `points`, the goals are a mix of point and box entries and one entry of goal 0 of query 0 is
    unbounded on either side (its centre is 0)"""
    n = MS.X_DIM[model_id]
    x_init, lo = rng.uniform(-2, 2, (Bq, n)), rng.uniform(-2, 2, (Bq, L, n))
    hi = lo.copy() if points else lo + rng.uniform(0, 0.3, (Bq, L, n)) * (rng.uniform(size=(Bq, L, n)) < 0.5)
    if not points:
        hi[0, 0, 1], lo[0, 0, n - 1] = np.inf, -np.inf
    T = np.cumsum(rng.uniform(3, 30, (Bq, L)), axis=1)
    return x_init, lo, hi, T


def fake_solve(rng, N, n, m, keep_start=True):
    """a stand-in for a solve: random trajectories of the active problems (knot 0 near, not at, x_init) and random status words"""
    def solve(xi, lo, hi, tf, X0, U0, active):
        B = len(tf)
        X, U = X0.copy(), U0.copy()
        for b in np.flatnonzero(active):
            X[b], U[b] = rng.uniform(-2, 2, (N, n)), rng.uniform(-1, 1, (N, m))
            X[b, 0] = xi[b] + (0 if keep_start else 1e-9 * rng.uniform(-1, 1, n))
        st = dict(iterations=rng.integers(1, 30, B), converged=rng.integers(0, 2, B), successful=rng.integers(0, 2, B),
                  stop_reason=rng.integers(0, 4, B), J=rng.uniform(0, 5, B))
        return X, U, st
    return solve


# ---- 1. leg seeds -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_id", [0, 1, 2, 3])
def test_leg_seeds_are_the_hosts_straight_line(model_id):
    """every leg's seed is host.init_traj_straightline at that x_init, goal and tf_l, bit for bit, in both layouts; tf_l is one
    rounded difference; the problems behind a ragged query's last leg are that leg, inactive"""
    H = g.host
    model = host_model(model_id)
    rng = np.random.default_rng(model_id)
    n, m = MS.X_DIM[model_id], MS.U_DIM[model_id]
    for N in (3, 4, 50):
        for L, Bq in ((1, 2), (3, 3), (5, 1)):
            x_init, lo, hi, T = timeline(model_id, Bq, L, rng)
            S = NL.Timeline(model_id, N, x_init, lo, hi, T)
            assert S.mode == (NL.PARALLEL if L == 1 else NL.SEQUENTIAL) and S.B == Bq
            xi, l, h, tf, X0, U0, act = S.problems()
            assert act.all() and not U0.any() and X0.shape == (Bq, N, n) and U0.shape == (Bq, N, m)
            for q in range(Bq):
                assert tf[q] == T[q, 0] and np.array_equal(xi[q], x_init[q])
                ref = H.init_traj_straightline(host_top(model, x_init[q], lo[q, 0], hi[q, 0], N, tf[q]))
                assert np.array_equal(X0[q], ref.X.T) and ref.Tf == tf[q]
            # the later legs: from the junction an advance hands over
            solve = fake_solve(rng, N, n, m)
            for r in range(L - 1):
                X, U, st = solve(*S.problems())
                S.advance(np.ones(Bq), X, U, st)
                xi, l, h, tf, X0, U0, act = S.problems()
                for q in range(Bq):
                    assert tf[q] == T[q, r + 1] - T[q, r] and np.array_equal(xi[q], X[q, N - 1])
                    assert np.array_equal(l[q], lo[q, r + 1]) and np.array_equal(h[q], hi[q, r + 1])
                    ref = H.init_traj_straightline(host_top(model, X[q, N - 1], lo[q, r + 1], hi[q, r + 1], N, tf[q]))
                    assert np.array_equal(X0[q], ref.X.T) and not U0[q].any()
            # PARALLEL: leg l starts at the point goal l - 1
            x_init, lo, hi, T = timeline(model_id, Bq, L, rng, points=True)
            nl = np.maximum(1, L - np.arange(Bq))
            S = NL.Timeline(model_id, N, x_init, lo, hi, T, n_legs=nl)
            assert S.mode == NL.PARALLEL and S.B == Bq * L
            xi, l, h, tf, X0, U0, act = S.problems()
            for q in range(Bq):
                for j in range(L):
                    b, le = q * L + j, min(j, nl[q] - 1)
                    assert act[b] == (j < nl[q])
                    start = x_init[q] if le == 0 else lo[q, le - 1]
                    assert np.array_equal(xi[b], start) and tf[b] == (T[q, 0] if le == 0 else T[q, le] - T[q, le - 1])
                    ref = H.init_traj_straightline(host_top(model, start, lo[q, le], hi[q, le], N, tf[b]))
                    assert np.array_equal(X0[b], ref.X.T) and np.array_equal(l[b], lo[q, le]) and np.array_equal(h[b], hi[q, le])


def test_device_line_is_the_straight_line_to_an_ulp():
    """device_line, the fused rounding csrc/seed.hpp pins, is within one ulp of the host's sum and equal at both ends"""
    rng = np.random.default_rng(5)
    for N in (3, 4, 50):
        x, lo = rng.uniform(-3, 3, 6), rng.uniform(-3, 3, 6)
        hi = lo + np.array([0, 0.1, 0, np.inf, 0, 0.2])
        a, b = NL.device_line(x, lo, hi, N), MS.straight_line(x, lo, hi, N)
        assert np.abs(a - b).max() <= 2.0 ** -52 * np.abs(b).max() and np.array_equal(a[0], x) and np.array_equal(a[-1], MS.goal_centre(lo, hi))


# ---- 2. the advance rule on hand-made verdict tables --------------------------------------------------------------------------
# name: (n_legs per query, L, the verdicts per round [Bq], expected status, failed_leg, n_done, n_flying after every round)
D, F = NL.DONE, NL.FAILED
SEQ_TABLES = {
    "all_ok": ([3, 3], 3, [[1, 1], [1, 1], [1, 1]], [D, D], [-1, -1], [3, 3], [2, 2, 0]),
    "fail_first": ([3, 3], 3, [[0, 1], [1, 1], [1, 1]], [F, D], [0, -1], [0, 3], [1, 1, 0]),
    "fail_middle": ([3, 3], 3, [[1, 1], [1, 0], [1, 1]], [D, F], [-1, 1], [3, 1], [2, 1, 0]),
    "fail_last": ([3, 3], 3, [[1, 1], [1, 1], [0, 1]], [F, D], [2, -1], [2, 3], [2, 2, 0]),
    "ragged": ([1, 3, 2], 3, [[1, 1, 1], [1, 1, 1], [1, 1, 1]], [D, D, D], [-1, -1, -1], [1, 3, 2], [2, 1, 0]),
    "ragged_fail": ([2, 3, 1], 3, [[1, 1, 0], [0, 1, 1], [1, 1, 1]], [F, D, F], [1, -1, 0], [1, 3, 0], [2, 1, 0]),
    "single": ([1, 1], 1, [[1, 0]], [D, F], [-1, 0], [1, 0], [0]),
}


@pytest.mark.parametrize("name", sorted(SEQ_TABLES))
def test_advance_rule_sequential(name):
    nl, L, verdicts, status, failed, n_done, flying = SEQ_TABLES[name]
    Bq, N, model_id = len(nl), 4, 0
    n, m = MS.X_DIM[model_id], MS.U_DIM[model_id]
    rng = np.random.default_rng(len(name))
    x_init, lo, hi, T = timeline(model_id, Bq, L, rng)
    S = NL.Timeline(model_id, N, x_init, lo, hi, T, n_legs=nl, mode=NL.SEQUENTIAL)
    solve = fake_solve(rng, N, n, m, keep_start=False)
    stored = [[] for _ in range(Bq)]          # per query the (X, U, st row, x_init, lo, hi) of its stored legs
    r = 0
    while S.n_flying():
        was = S.flying()
        prob = S.problems()
        assert np.array_equal(prob[6], was)                                  # the finished queries' problems: inactive
        X, U, st = solve(*prob)
        for q in np.flatnonzero(was):
            stored[q].append((X[q].copy(), U[q].copy(), {k: v[q] for k, v in st.items()}, prob[0][q], prob[1][q], prob[2][q]))
        assert S.advance(verdicts[r], X, U, st) == flying[r]
        after = S.problems()
        for q in np.flatnonzero(~S.flying() & was):                          # finished now: the line of the leg it flew
            assert np.array_equal(after[0][q], prob[0][q]) and after[3][q] == prob[3][q] and np.array_equal(after[4][q], prob[4][q])
        for q in np.flatnonzero(~was):                                       # finished before: untouched
            assert all(np.array_equal(after[i][q], prob[i][q]) for i in range(6))
        r += 1
    assert r == len(flying) and S.round == r
    assert list(S.status) == status and list(S.failed_leg) == failed and list(S.n_done) == n_done
    check_join(S, stored, T, nl)


def test_advance_rule_parallel_with_a_failed_middle_leg():
    Bq, L, N, model_id = 3, 3, 4, 0
    n, m = MS.X_DIM[model_id], MS.U_DIM[model_id]
    rng = np.random.default_rng(11)
    x_init, lo, hi, T = timeline(model_id, Bq, L, rng, points=True)
    nl = [3, 2, 3]
    S = NL.Timeline(model_id, N, x_init, lo, hi, T, n_legs=nl, mode=NL.PARALLEL)
    prob = S.problems()
    assert list(prob[6]) == [1, 1, 1, 1, 1, 0, 1, 1, 1]
    X, U, st = fake_solve(rng, N, n, m, keep_start=False)(*prob)
    ok = np.array([1, 0, 1, 1, 1, 0, 1, 1, 0])                               # (problem 5 lies behind query 1's last leg)
    assert S.advance(ok, X, U, st) == 0
    assert list(S.status) == [F, D, F] and list(S.failed_leg) == [1, -1, 2] and list(S.n_done) == [1, 2, 2]
    stored = [[(X[q * L + l], U[q * L + l], {k: v[q * L + l] for k, v in st.items()}, prob[0][q * L + l], prob[1][q * L + l],
                prob[2][q * L + l]) for l in range(nl[q])] for q in range(Bq)]     # every leg is stored, the failed ones too
    check_join(S, stored, T, nl)
    after = S.problems()
    assert not after[6].any() and np.array_equal(after[4], prob[4]) and not after[5].any()      # every problem: its own line, inactive
    with pytest.raises(AssertionError):
        S.advance(ok, X, U, st)                                              # it runs once


def check_join(S, stored, T, nl):
    """the joined buffers and the report against the stored legs, by the header's sentences"""
    N, L = S.N, S.L
    assert S.X.shape[1] == S.Nj == L * (N - 1) + 1
    for q, legs in enumerate(stored):
        Jt = np.float64(0.0)
        for l, (X, U, st, xi, lo, hi) in enumerate(legs):
            at = l * (N - 1)
            assert np.array_equal(S.X[q, at + 1:at + N], X[1:])                              # a junction's X: leg l's last knot
            assert np.array_equal(S.X[q, at], X[0] if l == 0 else legs[l - 1][0][N - 1])
            assert np.array_equal(S.U[q, at:at + N - 1], U[:N - 1])                          # a junction's U: leg l + 1's U[0]
            if l == len(legs) - 1:
                assert np.array_equal(S.U[q, at + N - 1], U[N - 1])                          # the last stored leg keeps its own
            T0 = 0.0 if l == 0 else T[q, l - 1]
            tf = T[q, 0] if l == 0 else T[q, l] - T[q, l - 1]
            for k in range(N - 1):
                assert S.t[q, at + k] == T0 + k * (tf / (N - 1))
            assert S.t[q, at + N - 1] == T[q, l]                                             # exactly
            for key in ("iterations", "converged", "successful", "stop_reason", "J"):
                assert getattr(S, key)[q, l] == st[key]
            assert S.gap[q, l] == (0.0 if l == 0 else np.abs(X[0] - xi).max())
            point = lo == hi
            viol = np.where(point, np.abs(X[N - 1] - lo), np.maximum(np.maximum(lo - X[N - 1], X[N - 1] - hi), 0.0))
            assert S.arrive[q, l] == viol.max()
            Jt = Jt + st["J"]
        assert S.J_total[q] == Jt
        done = len(legs) * (N - 1) + 1
        assert not S.X[q, done:].any() and not S.U[q, done:].any() and not S.t[q, done:].any()   # behind the stored legs: zeros
        for key in NL.PER_LEG:
            assert not getattr(S, key)[q, len(legs):].any()
        assert (np.diff(S.t[q, :done]) > 0).all()


# ---- 3. host._timeline_of -----------------------------------------------------------------------------------------------------
def test_timeline_of_a_goal_set():
    H = g.host
    model = H.FreeflyerSE2()
    x_init = np.zeros(6)

    def top(goals, tf=30.0):
        gs = H.GoalSet()
        for goal in goals:
            H.add_goal(gs, goal)
        return H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.BlankEnv(), x_init, gs), 10, tf, fixed_final_time=True)

    final = H.Goal(H.PointGoal(np.arange(6.0)), 30.0, model)
    # one goal at the final time: one leg, the plain problem
    tl = H._timeline_of(top([final]))
    assert len(tl) == 1 and tl[0][0] == 30.0 and np.array_equal(tl[0][1], np.arange(6.0)) and np.array_equal(tl[0][2], np.arange(6.0))
    lo, hi = H._goal_bounds(top([final]).PD.goal_set, 6, 30.0)
    assert np.array_equal(tl[0][1], lo) and np.array_equal(tl[0][2], hi)
    # an intermediate full point, a box on two coordinates, a partial point; two goals at one time are merged
    goals = [final, H.Goal(H.PointGoal(np.ones(6)), 10.0, model),
             H.Goal(H.BoxGoal([0.5, 0.6], [0.7, 0.8]), 20.0, [0, 1]), H.Goal(H.PointGoal([0.25]), 20.0, [2]),
             H.Goal(H.PointGoal(np.full(6, 9.0)), 45.0, model)]                       # (behind tf_guess: left out)
    tl = H._timeline_of(top(goals))
    assert [t for t, _, _ in tl] == [10.0, 20.0, 30.0]
    assert np.array_equal(tl[0][1], np.ones(6)) and np.array_equal(tl[0][2], np.ones(6))
    assert np.array_equal(tl[1][1], [0.5, 0.6, 0.25, -np.inf, -np.inf, -np.inf]) and np.array_equal(tl[1][2], [0.7, 0.8, 0.25, np.inf, np.inf, np.inf])
    assert np.array_equal(tl[2][1], np.arange(6.0))
    # the plain path is as it was: the goals before the final time do not reach _goal_bounds or the straight line
    lo, hi = H._goal_bounds(top(goals).PD.goal_set, 6, 30.0)
    assert np.array_equal(lo, np.arange(6.0)) and np.array_equal(H.init_traj_straightline(top(goals)).X[:, -1], np.arange(6.0))
    # a final time without a goal
    with pytest.raises(ValueError, match="final time"):
        H._timeline_of(top([H.Goal(H.PointGoal(np.ones(6)), 10.0, model)]))
    with pytest.raises(ValueError, match="final time"):
        H._timeline_of(top([H.Goal(H.PointGoal(np.ones(6)), 45.0, model)]))
    # the restatement takes what it yields: SEQUENTIAL by the partial goal at 20 s
    lo, hi, T = (np.stack([e[i] for e in tl])[None] for i in (1, 2, 0))
    assert NL.Timeline(0, 10, x_init[None], lo, hi, T).mode == NL.SEQUENTIAL
    assert NL.Timeline(0, 10, x_init[None], lo[:, [0, 2]], hi[:, [0, 2]], T[:, [0, 2]]).mode == NL.PARALLEL


# ---- 4. the refusals of the argument check ------------------------------------------------------------------------------------
def refusal_cases(n, Bq=2, L=3, seed=3):
    """(name, keyword overrides of check_args, a word of the cause) of every GUSTO_ERR_ARG the header lists"""
    rng = np.random.default_rng(seed)
    x_init, lo = rng.uniform(-1, 1, (Bq, n)), rng.uniform(-1, 1, (Bq, L, n))
    T = np.cumsum(rng.uniform(1, 5, (Bq, L)), axis=1)
    base = dict(n=n, batch_cap=Bq * L, Bq=Bq, L=L, n_legs=None, x_init=x_init, goal_lo=lo, goal_hi=lo.copy(), t_goal=T, mode=NL.AUTO)

    def bad(a, idx, v):
        c = a.copy()
        c[idx] = v
        return c

    part = lo.copy()
    part[1, 0, n - 1] = np.inf                                            # an interior goal that leaves one side free
    cases = [("trajopt", dict(trajopt=True), "TrajOpt"), ("L_low", dict(L=0), "L outside"), ("L_high", dict(L=65), "L outside"),
             ("Bq", dict(Bq=0), "Bq"), ("null_x", dict(x_init=None), "null"), ("null_lo", dict(goal_lo=None), "null"),
             ("null_hi", dict(goal_hi=None), "null"), ("null_T", dict(t_goal=None), "null"), ("mode", dict(mode=3), "mode"),
             ("legs_low", dict(n_legs=[1, 0]), "n_legs"), ("legs_high", dict(n_legs=[4, 1]), "n_legs"),
             ("T_zero", dict(t_goal=bad(T, (0, 0), 0.0)), "T_0"), ("T_equal", dict(t_goal=bad(T, (1, 2), T[1, 1])), "T_0"),
             ("T_nan", dict(t_goal=bad(T, (1, 1), np.nan)), "T_0"), ("T_inf", dict(t_goal=bad(T, (0, 2), np.inf)), "T_0"),
             ("x_nan", dict(x_init=bad(x_init, (1, 0), np.nan)), "x_init"), ("x_inf", dict(x_init=bad(x_init, (0, n - 1), -np.inf)), "x_init"),
             ("parallel_partial", dict(goal_hi=part, mode=NL.PARALLEL), "PARALLEL"),
             ("cap_parallel", dict(batch_cap=Bq * L - 1), "batch_cap"), ("cap_sequential", dict(batch_cap=Bq - 1, mode=NL.SEQUENTIAL), "batch_cap")]
    return base, cases


def test_refusals_of_the_argument_check():
    base, cases = refusal_cases(6)
    assert NL.check_args(**base) == NL.PARALLEL and NL.check_args(**dict(base, mode=NL.SEQUENTIAL)) == NL.SEQUENTIAL
    for name, over, word in cases:
        with pytest.raises(ValueError, match=re.escape(word)):
            NL.check_args(**dict(base, **over))
    # what is not refused: times behind a ragged query's last leg are not read, a partial LAST goal is a point timeline still,
    # a partial interior goal is SEQUENTIAL under AUTO, and SEQUENTIAL needs Bq problems only
    T = base["t_goal"].copy()
    T[1, 2] = -1.0
    assert NL.check_args(**dict(base, t_goal=T, n_legs=[3, 2])) == NL.PARALLEL
    last = base["goal_hi"].copy()
    last[:, 2, 0] = np.inf
    assert NL.check_args(**dict(base, goal_hi=last)) == NL.PARALLEL
    inner = base["goal_hi"].copy()
    inner[0, 1, 0] += 0.5
    assert NL.check_args(**dict(base, goal_hi=inner)) == NL.SEQUENTIAL
    assert NL.check_args(**dict(base, goal_hi=inner, batch_cap=2)) == NL.SEQUENTIAL


# ---- 5. the study, pinned on the oracle ---------------------------------------------------------------------------------------
def study_timeline(Q=STUDY_Q, L=STUDY_L, full_points=False):
    """The first Q table queries of config 2; waypoint l of query q is the position of the start of query (q + l + 1) mod Q --
    the position entries only, or with full_points the whole start state --, the last goal the config's own; times equally
    spaced to the config's tf.  (x_init [Q, n], lo, hi [Q, L, n], T [Q, L], the keep-out boxes)"""
    P = g.problems
    x0, glo, ghi, tf = P.freeflyer_batch(Q)
    lo, hi = np.full((Q, L, 6), -np.inf), np.full((Q, L, 6), np.inf)
    for l in range(L - 1):
        w = x0[(np.arange(Q) + l + 1) % Q]
        sel = slice(0, 6) if full_points else slice(0, 2)
        lo[:, l, sel] = hi[:, l, sel] = w[:, sel]
    lo[:, L - 1], hi[:, L - 1] = glo, ghi
    T = tf[:, None] * np.arange(1, L + 1)[None, :] / L
    return x0, lo, hi, T, P.freeflyer_env()


def oracle_solve_fn(o, iters):
    """a solve function for np_legs.fly on the CPU oracle: the active problems one after the other"""
    def solve(xi, lo, hi, tf, X0, U0, active):
        B = len(tf)
        X, U = X0.copy(), U0.copy()
        st = dict(iterations=np.zeros(B, int), converged=np.zeros(B, int), successful=np.zeros(B, int), stop_reason=np.zeros(B, int),
                  J=np.full(B, np.nan))
        for b in np.flatnonzero(active):
            o.set_problem(xi[b], lo[b], hi[b], tf[b], X0[b], U0[b])
            r = o.solve(iters)
            X[b], U[b] = r["X"], r["U"]
            for k in ("iterations", "converged", "successful", "stop_reason"):
                st[k][b] = r[k]
            st["J"][b] = r["J_true"][-1] if len(r["J_true"]) else np.nan
        ok = (st["converged"] != 0) & (st["successful"] != 0)
        return ok, X, U, st, st["iterations"].copy()
    return solve


@functools.lru_cache(maxsize=None)
def oracle_study():
    import gusto_oracle as go
    x0, lo, hi, T, env = study_timeline()
    o = go.Oracle(go.FREEFLYER_SE2, STUDY_N, boxes=env)
    return NL.fly(oracle_solve_fn(o, STUDY_ITERS), 0, STUDY_N, x0, lo, hi, T, mode=NL.SEQUENTIAL)


def test_oracle_study_is_pinned():
    """48 table queries through two position-only waypoints, SEQUENTIAL, on the oracle: status, failed_leg and the trips per
    round are pinned; the largest gap and arrive over the done queries are printed and recorded in profiles/legs.txt"""
    S, log = oracle_study()
    failed = {int(q): int(S.failed_leg[q]) for q in np.flatnonzero(S.status == NL.FAILED)}
    trips = [int(info[act].sum()) for act, _, info in log]
    done = S.status == NL.DONE
    print("failed {query: leg}", failed, "trips per round", trips, "flying per round", [int(a.sum()) for a, _, _ in log])
    print("done %d, largest gap %.3g, largest arrive %.3g, J_total of the done: mean %.6g" %
          (done.sum(), S.gap[done].max(), S.arrive[done].max(), S.J_total[done].mean()))
    assert (S.status[~done] == NL.FAILED).all() and S.n_flying() == 0
    assert failed == STUDY_FAILED and trips == STUDY_TRIPS
    assert (S.n_done[done] == STUDY_L).all() and all(S.n_done[q] == l for q, l in failed.items())
    T = study_timeline()[3]
    for q in np.flatnonzero(done):                                # the joined plan: its time grid passes through the goal times
        assert np.array_equal(S.t[q, ::STUDY_N - 1], np.concatenate([[0.0], T[q]])) and (np.diff(S.t[q]) > 0).all()


# ---- the Julia mirror and the ctypes mirror of the structs --------------------------------------------------------------------
def test_mirrors_of_the_structs():
    """GustoLegsOpts and GustoLegsReport of julia/GuSTOHIPBatch.jl have the header's fields in the header's order and types (what
    tests/test_boundary.py checks of the structs it lists), and so do the ctypes mirrors; the six entry points appear in both"""
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    jl = open(os.path.join(ROOT, "gusto.jl_amd", "julia", "GuSTOHIPBatch.jl")).read()

    def c_fields(name):
        end = hdr.index("} %s;" % name)
        body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end) + len("typedef struct {"):end], flags=re.S)
        out = []
        for decl in body.split(";"):
            if decl.strip():
                ctype, rest = decl.strip().split(None, 1)
                for v in rest.split(","):
                    v = v.strip()
                    out.append((v.lstrip("*"), {"double": "Cdouble", "int": "Cint"}[ctype] if not v.startswith("*") else
                                {"double": "Ptr{Cdouble}", "int": "Ptr{Cint}"}[ctype]))
        return out

    def jl_fields(name):
        body = re.search(r"struct %s\b[^\n]*\n(.*?)\nend" % name, jl, re.S).group(1)
        return [tuple(x.strip() for x in f.split("::")) for f in re.split(r"[;\n]", re.sub(r"#[^\n]*", "", body)) if f.strip()]

    assert c_fields("gusto_legs_opts") == jl_fields("GustoLegsOpts") == [("mode", "Cint")]
    assert c_fields("gusto_legs_report") == jl_fields("GustoLegsReport")
    import ctypes as C
    assert g._capi.LegsOpts._fields_ == [("mode", C.c_int)]
    assert [k for k, _ in c_fields("gusto_legs_report")] == [k for k, _, _ in g._capi.LEGS_FIELDS] == list(NL.REPORT)
    for (k, ty), (_, dt, _) in zip(c_fields("gusto_legs_report"), g._capi.LEGS_FIELDS):
        assert dt == (np.int32 if ty == "Ptr{Cint}" else np.float64), k
    assert (g._capi.LEGS_FLYING, g._capi.LEGS_DONE, g._capi.LEGS_FAILED) == (NL.FLYING, NL.DONE, NL.FAILED)
    for name, val in (("GUSTO_LEGS_FLYING", 1), ("GUSTO_LEGS_DONE", 2), ("GUSTO_LEGS_FAILED", 4)):
        assert re.search(r"#define %s %d\b" % (name, val), hdr)
    assert re.search(r"GUSTO_LEGS_AUTO = 0, GUSTO_LEGS_SEQUENTIAL = 1, GUSTO_LEGS_PARALLEL = 2", hdr)
    assert g._capi.LEGS_MODE == {"auto": NL.AUTO, "sequential": NL.SEQUENTIAL, "parallel": NL.PARALLEL}
    for s in ("gusto_default_legs_opts", "gusto_legs_begin", "gusto_legs_advance", "gusto_get_legs", "gusto_get_legs_dev", "gusto_last_legs_ms"):
        assert s in g._capi.SYMBOLS and re.search(r"ccall\(\(:%s, libgusto_hip\)" % s, jl), s


def test_export_writes_the_knot_times(tmp_path):
    """export.write(..., t=...) stores the joined time grid as traj/t_traj; without t the uniform grid, as before"""
    X, U = np.zeros((7, 6)), np.zeros((7, 3))
    t = np.array([0.0, 1.0, 2.0, 3.0, 5.0, 7.0, 9.0])
    tree = g.export.write(str(tmp_path / "a.npz"), 0, X, U, 9.0, t=t)
    assert np.array_equal(tree["traj"]["t_traj"], t) and np.array_equal(np.load(str(tmp_path / "a.npz"))["traj/t_traj"], t)
    assert np.array_equal(g.export.write(str(tmp_path / "b.npz"), 0, X, U, 9.0)["traj"]["t_traj"], np.linspace(0.0, 9.0, 7))
    with pytest.raises(ValueError):
        g.export.write(str(tmp_path / "c.npz"), 0, X, U, 9.0, t=t[:-1])
