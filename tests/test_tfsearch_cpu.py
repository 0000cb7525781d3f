"""tests/np_tfsearch.py, the numpy restatement of the final-time search, proven without a GPU: the line seeds against
host.init_traj_straightline, the retimed seeds against the time-scaling symmetry of the models (tests/np_models.py), the update
rule on hand-made tables, the width guarantee on random verdicts, and the study that motivates the feature, pinned on the CPU
oracle (tests/test_gpu_tfsearch.py repeats tables and study on the device)."""
import functools
import os
import re

import numpy as np
import pytest

import gusto_jl_amd as g
import np_models as NM
import np_multistart as MS
import np_tfsearch as TS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52
NP_MODEL = {0: NM.FreeflyerSE2, 2: NM.AstrobeeSE3, 3: NM.AstrobeeSE3Manifold}
STUDY_Q, STUDY_N, STUDY_ITERS, STUDY_K, STUDY_ROUNDS, STUDY_RANGE = 12, 50, 30, 8, 3, (4.0, 84.0)
# the study on the oracle, per seed mode: tf_best per query (NaN: none), the NONMONOTONE queries, the trips of each round's solves
STUDY_PINS = {
    TS.SEED_LINE: dict(tf=[5.481481481481481, 4.1234567901234565, 10.91358024691358, 20.049382716049383, 14.493827160493828,
                           15.604938271604938, 25.604938271604937, np.nan, 18.814814814814813, 6.71604938271605, 16.098765432098766,
                           5.9753086419753085],
                       nonmonotone={0, 2, 3, 9}, trips=[539, 444, 465]),
    TS.SEED_INCUMBENT: dict(tf=[5.481481481481481, 4.1234567901234565, 10.91358024691358, 20.049382716049383, 14.493827160493828,
                                15.604938271604938, 24.123456790123456, np.nan, 18.814814814814813, 6.345679012345679,
                                16.098765432098766, 6.345679012345679],
                            nonmonotone={0, 9}, trips=[539, 318, 411]),
}
STUDY_NONE, STUDY_FLOOR = {7}, {1}
# the issue's scratch run with line seeds, sorted (its restatement lacked the knot-0 rule, which the line seeds do not use)
ISSUE_TF_LINE = [4.12, 5.48, 5.98, 6.72, 10.91, 14.49, 15.61, 16.10, 18.82, 20.05, 25.61]


def host_top(model, x_init, lo, hi, N, tf):
    H = g.host
    gs = H.GoalSet()
    H.add_goal(gs, H.Goal(H.BoxGoal(lo, hi), tf, model))
    return H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.BlankEnv(), x_init, gs), N, tf, fixed_final_time=True)


# ---- 1. line seeds ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_id", [0, 1, 2, 3])
def test_line_seeds_are_the_hosts_straight_line(model_id):
    """every candidate's seed is host.init_traj_straightline at that tf, bit for bit; replication and layout of the B = Bq K problems"""
    H = g.host
    model = (H.FreeflyerSE2, H.DubinsCar, H.AstrobeeSE3, H.AstrobeeSE3Manifold)[model_id]()
    rng = np.random.default_rng(model_id)
    n, m = MS.X_DIM[model_id], MS.U_DIM[model_id]
    for N in (3, 4, 50):
        for K, Bq in ((1, 2), (3, 3), (64, 1)):
            x_init, lo = rng.uniform(-3, 3, (Bq, n)), rng.uniform(-3, 3, (Bq, n))
            hi = lo + rng.uniform(0, 0.2, (Bq, n)) * (rng.uniform(size=(Bq, n)) < 0.5)
            hi[0, 1], lo[0, n - 1] = np.inf, -np.inf                 # a centre of 0 by the straight line's rule
            tf_lo, tf_hi = rng.uniform(1, 5, Bq), rng.uniform(20, 90, Bq)
            for seed in (TS.SEED_LINE,) + ((TS.SEED_INCUMBENT,) if model_id != 1 else ()):
                S = TS.Search(model_id, N, K, x_init, lo, hi, tf_lo, tf_hi, seed=seed)
                xi, l, h, t, X0, U0 = S.problems()
                assert X0.shape == (Bq * K, N, n) and U0.shape == (Bq * K, N, m) and not U0.any()
                for q in range(Bq):
                    T = TS.candidates(tf_lo[q], tf_hi[q], K, False)
                    assert T[-1] == tf_hi[q] and (np.diff(T) > 0).all() and T[0] > tf_lo[q]
                    for j in range(K):
                        b = q * K + j
                        assert np.array_equal(xi[b], x_init[q]) and np.array_equal(l[b], lo[q]) and np.array_equal(h[b], hi[q])
                        assert t[b] == T[j] == S.cand[q, j]
                        ref = H.init_traj_straightline(host_top(model, x_init[q], lo[q], hi[q], N, t[b]))
                        assert np.array_equal(X0[b], ref.X.T) and ref.Tf == t[b]
    # the candidates as numbers: [4, 84] in eight cells, and in nine with an incumbent
    assert list(TS.candidates(4.0, 84.0, 8, False)) == [14.0, 24.0, 34.0, 44.0, 54.0, 64.0, 74.0, 84.0]
    assert list(TS.candidates(4.0, 94.0, 8, True)) == [14.0, 24.0, 34.0, 44.0, 54.0, 64.0, 74.0, 84.0]
    assert list(TS.candidates(1.0, 2.0, 1, False)) == [2.0] and list(TS.candidates(1.0, 2.0, 1, True)) == [1.5]     # K = 1: bisection


# ---- 2. retimed seeds ---------------------------------------------------------------------------------------------------------
def defect(model_id, X, U, tf):
    """the trapezoid collocation defect [N - 1, n] of (X, U) at the final time tf, with the dynamics of tests/np_models.py"""
    M = NP_MODEL[model_id]
    f = np.stack([M.f(x, u) for x, u in zip(X, U)])
    dt = tf / (len(X) - 1)
    return X[:-1] - X[1:] + 0.5 * dt * (f[:-1] + f[1:])


@pytest.mark.parametrize("model_id", [0, 2, 3])
def test_retimed_seeds(model_id):
    """Random X, U in [-1, 1], dt = 1, s in [0.5, 2].

    Tolerance of the defect comparison: 96 * 64 ulp, absolute.  Both sides are sums of at most 12 terms -- two states and the two
    f of the trapezoid, each f at most five products --; a term is at most 64 in magnitude (|x| <= 1; with dt' = dt / s <= 2,
    |F| / mass <= 4 / 7, |M| / J <= 4 / 0.1083 = 37, |w x J w| / J <= 2 |w|^2 <= 8, the attitude rates <= 1.5 |w| <= 3, and the
    factor dt' / 2 <= 1); and a term carries at most 8 roundings (s, s s, the two seed products, the products and sums of f, dt'
    and the trapezoid's product).  12 * 8 * 64 ulp = 1.4e-12.  Nothing here was measured on the code under test."""
    rng = np.random.default_rng(40 + model_id)
    n, m, N = MS.X_DIM[model_id], MS.U_DIM[model_id], 9
    rates = list(TS.RATES[model_id])
    others = [i for i in range(n) if i not in rates]
    tol = 96 * 64 * ULP
    for trial in range(20):
        X, U = rng.uniform(-1, 1, (N, n)), rng.uniform(-1, 1, (N, m))
        x_init, goal = X[0].copy(), rng.uniform(-1, 1, n)
        x_init[rates], goal[rates] = 0.0, 0.0                    # zero end rates: the line's rate entries vanish
        X[0] = x_init
        tf = float(N - 1)
        # s == 1: the source itself for k >= 1, knot 0 x_init
        X1, U1 = TS.retimed_seed(model_id, x_init, goal, goal, N, tf, X, U, tf)
        assert np.array_equal(X1[1:], X[1:]) and np.array_equal(U1, U) and np.array_equal(X1[0], x_init)
        other_init = rng.uniform(-1, 1, n)
        assert np.array_equal(TS.retimed_seed(model_id, other_init, goal, goal, N, tf, X, U, tf)[0][0], other_init)
        for s_want in (0.5, 0.8, 1.25, 2.0, rng.uniform(0.5, 2.0)):
            T = tf / s_want
            s = tf / T
            X0, U0 = TS.retimed_seed(model_id, x_init, goal, goal, N, tf, X, U, T)
            assert np.array_equal(X0[:, others], X[:, others]) and np.array_equal(U0, (s * s) * U)
            d_src, d_new = defect(model_id, X, U, tf), defect(model_id, X0, U0, T)
            assert np.abs(d_new[:, others] - d_src[:, others]).max() <= tol
            assert np.abs(d_new[:, rates] - s * d_src[:, rates]).max() <= tol
        # a goal with end rates (the table goal has v = (0.05, -0.05)): the last knot's rates are s X_inc + (1 - s) c, exactly
        goal2 = goal.copy()
        goal2[rates] = rng.uniform(-0.1, 0.1, len(rates))
        T = tf / 0.7
        s = tf / T
        X0, _ = TS.retimed_seed(model_id, x_init, goal2, goal2, N, tf, X, U, T)
        assert np.array_equal(X0[-1, rates], s * X[-1, rates] + (1 - s) * goal2[rates])
        assert np.array_equal(X0[-1, others], X[-1, others])


# ---- 3. the update rule -------------------------------------------------------------------------------------------------------
def table(K, lo0, hi0, verdicts, rtol=0.01):
    return dict(K=K, lo0=np.atleast_1d(np.asarray(lo0, float)), hi0=np.atleast_1d(np.asarray(hi0, float)), rtol=rtol,
                verdicts=[np.asarray(v).astype(bool).reshape(-1) for v in verdicts])


ONE = 1.0 + ULP
# tables whose candidates are the search's own: the GPU test runs them too.  verdicts[r] is [Bq K] of round r
TABLES = dict(
    # q0 all eligible, q1 none, q2 a non-monotone round 0, q3 monotone thresholds
    k4=table(4, [4, 4, 4, 4], [84, 84, 84, 84],
             [[1, 1, 1, 1, 0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 1, 1],
              [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1, 1],
              [1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]]),
    # bisection: K = 1; q1 is DONE exactly at hi - lo == rtol hi after round 0, q2 one ulp wider is not
    k1=table(1, [2.5, 3.0, np.nextafter(3.0, 0.0)], [4, 4, 4], [[1, 1, 1], [0, 0, 0], [1, 1, 1]], rtol=0.25),
    k64=table(64, [1.0, 2.0], [65.0, 130.0],
              [np.concatenate([np.arange(64) >= 9, (np.arange(64) % 7 == 3)]),
               np.concatenate([np.arange(64) >= 40, np.zeros(64)]),
               np.concatenate([np.zeros(64), np.arange(64) >= 63])]),
    # a range one ulp wide: candidates 0 and 1 round to lo0 itself, so F == lo_old in round 0
    ulp=table(4, [1.0], [ONE], [[1, 1, 1, 1]]),
)


def run_table(t, seed=TS.SEED_LINE):
    """the reports after every round of a table on the restatement (freeflyerSE2, N = 3, any queries)"""
    Bq = len(t["lo0"])
    rng = np.random.default_rng(Bq)
    S = TS.Search(0, 3, t["K"], rng.uniform(-1, 1, (Bq, 6)), np.zeros((Bq, 6)), np.zeros((Bq, 6)), t["lo0"], t["hi0"], t["rtol"], seed)
    reps = []
    for v in t["verdicts"]:
        if not S.searching().any():
            break
        S.update(v)
        reps.append(S.report())
    return S, reps


def test_update_rule_on_hand_made_tables():
    N_, D_, F_, M_ = TS.NONE, TS.DONE, TS.FLOOR, TS.NONMONOTONE
    S, r = run_table(TABLES["k4"])
    # round 0: candidates 24, 44, 64, 84
    assert list(r[0]["status"]) == [F_, N_ | D_, M_, 0] and list(r[0]["n_eligible"]) == [4, 0, 2, 3]
    assert list(r[0]["tf_best"][[0, 2, 3]]) == [24.0, 44.0, 44.0] and np.isnan(r[0]["tf_best"][1]) and np.isnan(r[0]["J_best"]).all()
    assert list(r[0]["lo"]) == [4.0, 84.0, 24.0, 24.0] and list(r[0]["hi"]) == [24.0, 84.0, 44.0, 44.0]
    assert list(r[0]["round_found"]) == [0, -1, 0, 0]
    assert list(r[0]["cand"][0]) == [8.0, 12.0, 16.0, 20.0] and list(r[0]["cand"][1]) == [84.0] * 4 and list(r[0]["cand"][3]) == [28.0, 32.0, 36.0, 40.0]
    # round 1: q0 all eligible again; q1 is done and not touched; q2 eligible at 36 but not at 40 (non-monotone, sticky); q3 36, 40
    assert list(r[1]["status"]) == [F_, N_ | D_, M_, 0] and list(r[1]["n_eligible"]) == [4, 0, 1, 2]
    assert list(r[1]["lo"]) == [4.0, 84.0, 32.0, 32.0] and list(r[1]["hi"]) == [8.0, 84.0, 36.0, 36.0]
    assert list(r[1]["round_found"]) == [1, -1, 1, 1]
    # round 2: q2 nothing eligible: the incumbent stays, lo moves to the last candidate; q3 all eligible: hi moves, lo stays
    assert list(r[2]["round_found"]) == [2, -1, 1, 2] and r[2]["tf_best"][2] == 36.0 and r[2]["lo"][2] == r[1]["cand"][2, 3]
    assert r[2]["lo"][3] == 32.0 and r[2]["hi"][3] == r[1]["cand"][3, 0] and r[2]["status"][3] == 0 and r[2]["status"][2] & M_
    assert r[2]["status"][0] & F_ and r[2]["hi"][0] == r[1]["cand"][0, 0] and r[2]["lo"][0] == 4.0
    for a, b in zip(r, r[1:]):      # a done query: the same report after every later update
        for k in a:
            assert np.array_equal(a[k][1], b[k][1], equal_nan=True), k
    # K = 1: round 0 tries hi itself
    S, r = run_table(TABLES["k1"])
    assert list(r[0]["tf_best"]) == [4.0, 4.0, 4.0] and list(r[0]["status"]) == [F_, F_ | D_, F_]       # 1 <= 0.25 * 4, exactly
    assert list(r[0]["cand"][:, 0]) == [3.25, 4.0, 0.5 * (np.nextafter(3.0, 0.0) + 4.0)]
    assert list(r[1]["lo"]) == [3.25, 3.0, r[0]["cand"][2, 0]] and list(r[1]["status"]) == [D_, F_ | D_, D_] and len(r) == 2
    # K = 64
    S, r = run_table(TABLES["k64"])
    assert list(r[0]["tf_best"]) == [11.0, 10.0] and list(r[0]["lo"]) == [10.0, 8.0] and list(r[0]["status"]) == [0, M_]
    assert list(r[0]["n_eligible"]) == [55, 9] and r[0]["cand"].shape == (2, 64)
    assert r[1]["round_found"][0] == 1 and r[1]["round_found"][1] == 0 and r[1]["lo"][1] == r[0]["cand"][1, 63] and r[1]["hi"][1] == 10.0
    assert r[1]["lo"][0] == r[0]["cand"][0, 39] and r[1]["hi"][0] == r[0]["cand"][0, 40]
    # lo_old >= F through the roundings of a range one ulp wide
    S, r = run_table(TABLES["ulp"])
    assert list(TS.candidates(1.0, ONE, 4, False)) == [1.0, 1.0, ONE, ONE]
    assert r[0]["tf_best"][0] == 1.0 and r[0]["lo"][0] == 1.0 and r[0]["hi"][0] == 1.0 and r[0]["status"][0] == D_ | F_ | M_


def test_update_rule_with_the_callers_final_times():
    """T is read from the problems, not from the candidates: lo_old >= F, and an equal tf that does not replace the incumbent"""
    S = TS.Search(0, 3, 2, np.zeros((1, 6)), np.zeros((1, 6)), np.zeros((1, 6)), 4.0, 84.0)
    X = np.arange(2 * 3 * 6, dtype=float).reshape(2, 3, 6) + 1
    U = -np.arange(2 * 3 * 3, dtype=float).reshape(2, 3, 3) - 1
    S.update([0, 1], X=X, U=U, J=[5.0, 7.0])                  # 44 refuted, 84 the incumbent
    assert S.tf_best[0] == 84.0 and S.lo[0] == 44.0 and S.J_best[0] == 7.0 and np.array_equal(S.X[0], X[1]) and S.status[0] == 0
    S.update([1, 1], T=[84.0, 84.0], X=X[::-1], U=U, J=[1.0, 2.0])   # equal: the incumbent of round 0 stays
    assert S.round_found[0] == 0 and S.J_best[0] == 7.0 and np.array_equal(S.X[0], X[1]) and S.lo[0] == 44.0 and S.hi[0] == 84.0
    S.update([1, 0], T=[40.0, 41.0], X=X, U=U, J=[1.0, 2.0])  # below lo_old = 44: taken, lo falls back to lo0, flagged
    assert S.round_found[0] == 2 and S.tf_best[0] == 40.0 and S.lo[0] == 4.0 and S.hi[0] == 40.0 and np.array_equal(S.U[0], U[0])
    assert S.status[0] == TS.NONMONOTONE | TS.FLOOR
    S.update([0, 0])                                          # the FLOOR bit goes once a candidate below F is refuted
    assert S.status[0] == TS.NONMONOTONE and S.lo[0] == 28.0


# ---- 4. the width guarantee ---------------------------------------------------------------------------------------------------
def test_width_guarantee():
    """3000 random (lo0, hi0, T*, K), three rounds.  Monotone verdicts ok = (T >= T*): lo < T* <= hi, or FLOOR when T* <= lo0, or
    NONE when T* > hi0.  The width is at most w0 / K after round 0 and the previous one over K + 1 after every further round; the
    allowance for the roundings of the candidate formula is 4 ulp of hi (a difference, a division, a product and a sum, each half
    an ulp of a number below hi, on both ends of the cell).  Random verdicts: the bound alone."""
    rng = np.random.default_rng(2024)
    for trial in range(3000):
        K = int(rng.choice([1, 2, 3, 4, 7, 8, 16, 63, 64]))
        lo0 = 10.0 ** rng.uniform(-2, 2)
        hi0 = lo0 * (1 + 10.0 ** rng.uniform(-3, 2))
        Tstar = rng.uniform(0.5 * lo0, 1.2 * hi0)
        for monotone in (True, False):
            S = TS.Search(0, 3, K, np.zeros((1, 6)), np.zeros((1, 6)), np.zeros((1, 6)), lo0, hi0, rtol=1e-6)
            width = hi0 - lo0
            for r in range(3):
                if not S.searching()[0]:
                    break
                T = S.cand[0]
                S.update(T >= Tstar if monotone else rng.uniform(size=K) < 0.4)
                if S.status[0] & TS.NONE:
                    assert S.lo[0] == S.hi[0] == hi0
                    break
                bound = width / (K if r == 0 else K + 1)
                assert S.hi[0] - S.lo[0] <= bound + 4 * ULP * S.hi[0], (trial, r, K, S.hi[0] - S.lo[0], bound)
                width = S.hi[0] - S.lo[0]
            if monotone:
                if Tstar > hi0:
                    assert S.status[0] & TS.NONE and np.isnan(S.tf_best[0])
                elif Tstar <= lo0:
                    assert S.status[0] & TS.FLOOR and S.lo[0] == lo0 and not S.status[0] & TS.NONE
                else:
                    assert S.lo[0] < Tstar <= S.hi[0] == S.tf_best[0], (trial, K, lo0, hi0, Tstar, S.lo[0], S.hi[0])
                    assert not S.status[0] & (TS.NONE | TS.NONMONOTONE)


# ---- 5. the study, pinned on the oracle ---------------------------------------------------------------------------------------
def oracle_solve_fn(o, iters):
    """a solve function for np_tfsearch.search on the CPU oracle: the active problems one after the other"""
    def solve(xi, lo, hi, tf, X0, U0, active):
        B = len(tf)
        ok, J, trips = np.zeros(B, bool), np.full(B, np.nan), np.zeros(B, int)
        X, U = X0.copy(), U0.copy()
        for b in np.flatnonzero(active):
            o.set_problem(xi[b], lo[b], hi[b], tf[b], X0[b], U0[b])
            r = o.solve(iters)
            ok[b], X[b], U[b], trips[b] = r["converged"] and r["successful"], r["X"], r["U"], r["iterations"]
            J[b] = r["J_true"][-1] if len(r["J_true"]) else np.nan
        return ok, X, U, J, trips
    return solve


@functools.lru_cache(maxsize=None)
def oracle_study(seed):
    """the first 12 table queries through three rounds of eight candidates in [4, 84] on the oracle: (Search, log)"""
    import gusto_oracle as go
    P = g.problems
    x0, glo, ghi, _ = P.freeflyer_batch(STUDY_Q)
    o = go.Oracle(go.FREEFLYER_SE2, STUDY_N, boxes=P.freeflyer_env())
    return TS.search(oracle_solve_fn(o, STUDY_ITERS), 0, STUDY_N, STUDY_K, x0, glo, ghi, *STUDY_RANGE, STUDY_ROUNDS, seed=seed)


def check_incumbents(tf_best, X, U, x0, glo, have):
    """what tests/test_gpu_parity.py::test_full_batch_properties_freeflyer asks of solved problems, with its tolerances, of the
    incumbents at their own final times"""
    mp = g.default_params(g.FREEFLYER_SE2)[1]
    X, U, tf, N = X[have], U[have], tf_best[have], X.shape[1]
    assert np.abs(X[:, 0, :] - x0[have]).max() < 1e-9
    assert np.abs(X[:, -1, :] - glo[have]).max() < 1e-7
    dt = tf[:, None, None] / (N - 1)
    f = np.concatenate([X[:, :, 3:6], U[:, :, 0:2] / mp.mass, U[:, :, 2:3] / mp.Jdiag[2]], axis=2)
    res = X[:, :-1, :] - X[:, 1:, :] + 0.5 * dt * (f[:, :-1, :] + f[:, 1:, :])
    assert np.abs(res).max() < 1e-6
    acc = np.sqrt(U[:, :-1, 0] ** 2 + U[:, :-1, 1] ** 2) / mp.mass
    assert acc.max() <= mp.hard_limit_accel * (1 + 1e-6)
    assert np.abs(U[:, :-1, 2] / mp.Jdiag[2]).max() <= mp.hard_limit_alpha * (1 + 1e-6)
    v2 = X[:, :, 3] ** 2 + X[:, :, 4] ** 2
    assert (v2 - mp.hard_limit_vel ** 2).max() < 1e-2
    return np.abs(res).max(), np.abs(X[:, -1, :] - glo[have]).max(), (v2 - mp.hard_limit_vel ** 2).max()


@pytest.mark.parametrize("seed", [TS.SEED_LINE, TS.SEED_INCUMBENT])
def test_oracle_study_is_pinned(seed):
    S, log = oracle_study(seed)
    pins = STUDY_PINS[seed]
    x0, glo, _, _ = g.problems.freeflyer_batch(STUDY_Q)
    trips = [int(info.sum()) for _, _, info in log]
    none = {q for q in range(STUDY_Q) if S.status[q] & TS.NONE}
    floor = {q for q in range(STUDY_Q) if S.status[q] & TS.FLOOR}
    nonmono = {q for q in range(STUDY_Q) if S.status[q] & TS.NONMONOTONE}
    print("tf_best", [float(v) for v in S.tf_best], "\nissue's line-seed run, sorted", ISSUE_TF_LINE, "\nNONE", none, "FLOOR", floor,
          "NONMONOTONE", nonmono, "trips", trips)
    have = S.round_found >= 0
    print("worst collocation residual, goal row, v2 excess:", check_incumbents(S.tf_best, S.X, S.U, x0, glo, have))
    assert np.array_equal(S.tf_best, pins["tf"], equal_nan=True)
    assert none == STUDY_NONE and floor == STUDY_FLOOR and nonmono == pins["nonmonotone"] and trips == pins["trips"]
    # round 0: the verdicts over 14, 24, ..., 84 s are monotone in tf for all 12 queries
    cand0, ok0, _ = log[0]
    assert np.array_equal(cand0[0], np.arange(14.0, 85.0, 10.0)) and (np.diff(ok0.astype(int), axis=1) >= 0).all()
    # every answer is bracketed to a ninth of a ninth of a cell
    w = (STUDY_RANGE[1] - STUDY_RANGE[0]) / STUDY_K / (STUDY_K + 1) ** 2
    assert ((S.hi - S.lo)[have] <= w + 4 * ULP * S.hi[have]).all() and (S.hi[have] == S.tf_best[have]).all()


# ---- the Julia mirror of gusto_tfsearch_opts ----------------------------------------------------------------------------------
def test_julia_mirror_of_the_options_struct():
    """GustoTfsearchOpts of julia/GuSTOHIPBatch.jl has the header's fields in the header's order and types (what
    tests/test_boundary.py checks of the structs it lists), and so does the ctypes mirror; the six entry points appear in both"""
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    jl = open(os.path.join(ROOT, "gusto.jl_amd", "julia", "GuSTOHIPBatch.jl")).read()
    end = hdr.index("} gusto_tfsearch_opts;")
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end) + len("typedef struct {"):end], flags=re.S)
    cf = []
    for decl in body.split(";"):
        if decl.strip():
            ctype, rest = decl.strip().split(None, 1)
            cf += [(v.strip(), {"double": "Cdouble", "int": "Cint"}[ctype]) for v in rest.split(",")]
    jbody = re.search(r"struct GustoTfsearchOpts\b[^\n]*\n(.*?)\nend", jl, re.S).group(1)
    jf = [tuple(x.strip() for x in f.split("::")) for f in re.split(r"[;\n]", re.sub(r"#[^\n]*", "", jbody)) if f.strip()]
    assert cf == jf == [("tf_lo", "Cdouble"), ("tf_hi", "Cdouble"), ("rtol", "Cdouble"), ("seed", "Cint")]
    import ctypes as C
    to_c = {"Cdouble": C.c_double, "Cint": C.c_int}
    assert [(k, t) for k, t in g._capi.TfsearchOpts._fields_] == [(k, to_c[t]) for k, t in cf]
    rep_end = hdr.index("} gusto_tfsearch_report;")
    rep = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, rep_end):rep_end], flags=re.S)
    assert re.findall(r"\*(\w+)", rep) == [k for k, _, _ in g._capi.TFSEARCH_FIELDS]
    for s in ("gusto_default_tfsearch_opts", "gusto_tfsearch_begin", "gusto_tfsearch_update", "gusto_get_tfsearch", "gusto_get_tfsearch_dev",
              "gusto_last_tfsearch_ms"):
        assert s in g._capi.SYMBOLS and re.search(r"ccall\(\(:%s, libgusto_hip\)" % s, jl), s
    o = g._capi.default_tfsearch_opts(g.FREEFLYER_SE2)
    assert (o.tf_lo, o.tf_hi, o.rtol, o.seed) == (1.0, 100.0, 0.01, 1) and g._capi.default_tfsearch_opts(g.DUBINS_CAR).seed == 0
