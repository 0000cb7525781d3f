"""What the five seeding entries share (csrc/seed.hpp: the decode of a thread, the straight line, the knot-0 tail that replicates
a query into the handle's arrays), under all five at once: multi-start with a zero fan, the trajectory library with an empty
library, an unseeded replan, the roadmap without a keep-out set and the final-time search's begin with seed = "line" each leave
exactly what gusto_set_problems leaves for the replicated inputs -- X and U bit for bit, and x_init, goal_lo, goal_hi and tf as one
gusto_subproblem reads them.  Shapes where an off-by-one in the decode shows: N = 3 and 4, two queries of two starts, the second
query's goal with an unbounded coordinate (its centre is 0), the first one's a point."""
import numpy as np
import pytest

import gusto_jl_amd as g

pytestmark = pytest.mark.gpu

BQ, K = 2, 2
TRUST = (3.0, 1.0, 0.4)     # Delta, omega, toggle of the subproblem: any admissible values, the same on both sides


def same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def reference(s, x_init, lo, hi, tf):
    """X, U and the subproblem of gusto_set_problems on the replicated inputs"""
    rep = [np.repeat(a, K, 0) for a in (x_init, lo, hi)]
    s.set_problems(*rep, tf)
    X, U = s.traj()
    s.set_problems(*rep, tf, X, U)
    return X, U, s.subproblem(X, U, *TRUST)


@pytest.mark.parametrize("N", [3, 4])
@pytest.mark.parametrize("model", [g.FREEFLYER_SE2, g.ASTROBEE_SE3])
def test_every_seeding_entry_leaves_what_set_problems_leaves(model, N):
    n = g._capi.MODEL_DIMS[model][0]
    rng = np.random.default_rng(10 * model + N)
    x_init = rng.uniform(-1, 1, (BQ, n))
    lo = rng.uniform(-1, 1, (BQ, n))
    hi = lo.copy()                                   # query 0: a point goal
    hi[1] = lo[1] + rng.uniform(0.1, 0.3, n)         # query 1: a box, one coordinate unbounded above, one below
    hi[1, 1], lo[1, n - 1] = np.inf, -np.inf
    tf = np.array([30.0, 47.0])
    s = g.BatchSolver(model, N, BQ * K, hist_cap=8)
    Xr, Ur, sub = reference(s, x_init, lo, hi, np.repeat(tf, K))
    assert np.array_equal(Xr[:, 0], np.repeat(x_init, K, 0)) and not Ur.any()
    assert not Xr[2:, -1, 1].any() and not Xr[2:, -1, n - 1].any()         # the centre of an unbounded coordinate: 0

    def check(what, ref=(Xr, Ur, sub)):
        assert s.B == BQ * K, what
        X, U = s.traj()
        assert np.array_equal(X, ref[0]) and np.array_equal(U, ref[1]), what
        assert same(s.subproblem(X, U, *TRUST), ref[2]), what

    s.set_problems_multistart(x_init, lo, hi, tf, np.zeros((K, 2)))
    check("multistart")
    lib = g._capi.TrajLib(model, N, 1)
    s.set_problems_trajlib(lib, x_init, lo, hi, tf, K=K)
    assert (s.trajlib_seeds()["entry"] == -1).all()
    check("trajlib")
    lib.close()
    src = g.BatchSolver(model, N, BQ * K, hist_cap=8)
    src.set_problems(*(np.repeat(a, K, 0) for a in (x_init, lo, hi)), np.repeat(tf, K))
    s.set_problems_replan(0.0, np.repeat(x_init, K, 0), src=src, mask=np.zeros(BQ * K, bool))
    assert not s.replan_info()["seeded"].any()
    check("replan")
    src.close()
    s.set_problems_roadmap(x_init, lo, hi, tf, K=K)
    check("roadmap")
    s.tfsearch_begin(x_init, lo, hi, 5.0, tf, K=K, seed="line")
    cand = s.tfsearch_info()["cand"]
    assert np.array_equal(cand[:, -1], tf)           # (the upper end is always tried)
    X, U = s.traj()
    sub_tf = s.subproblem(X, U, *TRUST)
    assert np.array_equal(X, Xr) and np.array_equal(U, Ur)
    assert same(sub_tf, reference(s, x_init, lo, hi, cand.reshape(-1))[2])
    s.close()
