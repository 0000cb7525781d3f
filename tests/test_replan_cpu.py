"""tests/np_replan.py, the numpy restatement of receding-horizon replanning, proven without a GPU: the identity case, the end
knots, tf', a moved goal, resampling between horizons against np.interp, and the study that motivates the feature, pinned on the
CPU oracle (tests/test_gpu_replan.py repeats its knot-5 case on the device)."""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import np_replan as RP

STUDY_B, STUDY_N, STUDY_ITERS = 48, 50, 30
STUDY_STRAIGHT_FAILS = {1, 5, 7, 37, 40}
# replan knot -> (successful, SCP trips (sum), trips of the longest problem) over the 43 queries the first solve answered, and the
# queries that fail either way
STUDY_WARM = {5: (43, 148, 7), 25: (39, 137, 6)}
STUDY_COLD = {5: (43, 469, 15), 25: (39, 378, 14)}
STUDY_REPLAN_FAILS = {5: set(), 25: {3, 4, 34, 46}}


def random_source(model_id, Ns, rng, B=1):
    n, m = RP.X_DIM[model_id], RP.U_DIM[model_id]
    return rng.normal(size=(B, Ns, n)), rng.normal(size=(B, Ns, m))


@pytest.mark.parametrize("model_id", [0, 1, 2, 3])
def test_identity_returns_the_source_bits(model_id):
    """tau = 0, Ns = N, x_now = X_s[0], no goals: only exact zeros are added"""
    rng = np.random.default_rng(model_id)
    for N in (3, 5, 50, 65):
        Xs, Us = random_source(model_id, N, rng)
        X0, U0 = RP.seeded_start(Xs[0], Us[0], 0.0, Xs[0, 0], N)
        assert X0.tobytes() == Xs[0].tobytes() and U0.tobytes() == Us[0].tobytes()


@pytest.mark.parametrize("model_id", [0, 1, 2, 3])
def test_end_knots_and_tf(model_id):
    """knot 0 is x_now; without goals the last knot is the source's last knot (its U too); tf' = (1 - tau) tf_s; an unseeded
    problem is the straight line, U0 = 0"""
    rng = np.random.default_rng(10 + model_id)
    n = RP.X_DIM[model_id]
    for N, Ns in ((3, 3), (5, 9), (50, 50), (12, 7)):
        B = 4
        Xs, Us = random_source(model_id, Ns, rng, B)
        tau, x_now = np.array([0.0, 0.25, 10 / 49, 0.999]), rng.normal(size=(B, n))
        tf_s, lo = rng.uniform(20, 60, B), rng.normal(size=(B, n))
        hi = lo + rng.uniform(0, 0.3, (B, n))
        out = RP.replan(N, Xs, Us, tf_s, lo, hi, tau, x_now, [1, 1, 1, 0])
        assert np.array_equal(out["X0"][:, 0], x_now) and np.array_equal(out["x_init"], x_now)
        assert np.array_equal(out["X0"][:3, -1], Xs[:3, -1]) and np.array_equal(out["U0"][:3, -1], Us[:3, -1])
        assert np.array_equal(out["tf"], (1 - tau) * tf_s) and np.array_equal(out["goal_lo"], lo) and np.array_equal(out["goal_hi"], hi)
        assert np.array_equal(out["X0"][3], RP.straight_line(x_now[3], lo[3], hi[3], N)) and not out["U0"][3].any()


def test_a_moved_goal_shifts_the_last_knot_by_the_difference_of_the_centres():
    rng = np.random.default_rng(3)
    Xs, Us = random_source(0, 50, rng)
    lo = rng.normal(size=6)
    hi = lo + 0.2
    nlo, nhi = lo + 0.5, hi + 0.75
    nhi[5] = np.inf                                            # its centre is 0
    x_now = rng.normal(size=6)
    X0, _ = RP.seeded_start(Xs[0], Us[0], 0.1, x_now, 50, RP.goal_centre(lo, hi), RP.goal_centre(nlo, nhi))
    shift = RP.goal_centre(nlo, nhi) - RP.goal_centre(lo, hi)
    assert np.array_equal(X0[-1], Xs[0, -1] + (0.0 * (x_now - Xs[0, 0]) + 1.0 * shift)) and shift[5] == -RP.goal_centre(lo, hi)[5]
    same, _ = RP.seeded_start(Xs[0], Us[0], 0.1, x_now, 50, RP.goal_centre(lo, hi), RP.goal_centre(lo, hi))
    none, _ = RP.seeded_start(Xs[0], Us[0], 0.1, x_now, 50)
    assert np.array_equal(same, none)                          # an unmoved goal adds exact zeros


@pytest.mark.parametrize("Ns,N", [(7, 12), (50, 13)])
def test_resampling_between_horizons_against_interp(Ns, N):
    """S_k and U0[k] are the piecewise-linear interpolant of the source at tau + (1 - tau) t_k of its time, per entry, to 1e-13"""
    rng = np.random.default_rng(Ns)
    for model_id in (0, 3):
        Xs, Us = random_source(model_id, Ns, rng)
        for tau in (0.0, 0.25, 10 / 49, 0.999):
            X0, U0 = RP.seeded_start(Xs[0], Us[0], tau, np.zeros(Xs.shape[2]), N)
            at = tau + (1 - tau) * np.arange(N) / (N - 1)
            grid = np.arange(Ns) / (Ns - 1)
            S = np.stack([np.interp(at, grid, Xs[0, :, i]) for i in range(Xs.shape[2])], axis=1)
            U = np.stack([np.interp(at, grid, Us[0, :, i]) for i in range(Us.shape[2])], axis=1)
            t = (np.arange(N) / (N - 1))[:, None]
            want = S + (1 - t) * (0.0 - S[0])[None, :]
            assert np.abs(X0[1:] - want[1:]).max() <= 1e-13 and np.abs(U0 - U).max() <= 1e-13


def totals(results, keep):
    rs = [results[q] for q in keep]
    return (sum(bool(r["converged"] and r["successful"]) for r in rs), sum(r["iterations"] for r in rs), max(r["iterations"] for r in rs))


@functools.lru_cache(maxsize=None)
def oracle_study(knot):
    """the first 48 table queries of config 2 from the straight line; the answered ones replanned from X[knot] + p_q with
    tf' = (1 - knot / 49) tf, from the shifted plan and from the straight line.  Returns (answered queries, warm, cold), the
    results as dicts by query"""
    import gusto_oracle as go
    P = g.problems
    x0, glo, ghi, tf = P.freeflyer_batch(STUDY_B)
    o = go.Oracle(go.FREEFLYER_SE2, STUDY_N, boxes=P.freeflyer_env())
    first = []
    for q in range(STUDY_B):
        o.set_problem(x0[q], glo[q], ghi[q], tf[q])
        first.append(o.solve(STUDY_ITERS))
    ok = [q for q in range(STUDY_B) if first[q]["converged"] and first[q]["successful"]]
    warm, cold = {}, {}
    tau = knot / (STUDY_N - 1)
    for q in ok:
        x_now = first[q]["X"][knot] + RP.perturbation(q)
        r = RP.replan(STUDY_N, first[q]["X"][None], first[q]["U"][None], tf[q:q + 1], glo[q:q + 1], ghi[q:q + 1], tau, x_now, [1])
        o.set_problem(x_now, glo[q], ghi[q], r["tf"][0], r["X0"][0], r["U0"][0])
        warm[q] = o.solve(STUDY_ITERS)
        o.set_problem(x_now, glo[q], ghi[q], r["tf"][0])
        cold[q] = o.solve(STUDY_ITERS)
    return ok, warm, cold


@pytest.mark.parametrize("knot", [5, 25])
def test_oracle_study_is_pinned(knot):
    """the shifted plan needs about a third of the straight line's trips and the same queries fail either way (profiles/replan.txt)"""
    ok, warm, cold = oracle_study(knot)
    assert set(range(STUDY_B)) - set(ok) == STUDY_STRAIGHT_FAILS
    assert totals(warm, ok) == STUDY_WARM[knot] and totals(cold, ok) == STUDY_COLD[knot]
    fails = lambda res: {q for q in ok if not (res[q]["converged"] and res[q]["successful"])}
    assert fails(warm) == fails(cold) == STUDY_REPLAN_FAILS[knot]
