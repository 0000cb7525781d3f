"""tests/np_trajlib.py, the numpy restatement of the trajectory library, proven without a GPU: the retargeting against
host.init_traj_straightline and against its own definitions, the neighbour rule on hand-made cases, the compaction, the inputs of
the GPU search tests (their sorted distances keep a relative gap above 1e-12), and the study that motivates the feature, pinned on
the CPU oracle (tests/test_gpu_trajlib.py repeats its small case on the device)."""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import np_trajlib as TL
from test_multistart_cpu import host_top

STUDY_ITERS = 30
LIB_FIRST = 100000        # the library problems are the generator's problems LIB_FIRST, LIB_FIRST + 1, ...
# (converged and successful, SCP iterations, IPM iterations, SCP iterations of the longest problem)
FREEFLYER_48 = dict(lib_good=51, cold=(43, 522, 3958, 24), seeded=(48, 182, 1128, 7))
DUBINS_64 = dict(lib_good=171, cold=(37, 1006, 3163, 30), seeded=(56, 760, 1016, 30), seeded_xy=(40, 1246, 1503, 30))
FREEFLYER_16 = dict(lib_good=26, cold=(13, 160, 1316, 24), seeded=(16, 69, 449, 9))      # the case of the GPU test
SEARCH_LS, SEARCH_KS, SEARCH_BQS = (1, 63, 64, 65, 200), (1, 3, 8), (1, 5)


def random_lib(model_id, N, L, rng, **weights):
    n, m = TL.X_DIM[model_id], TL.U_DIM[model_id]
    lib = TL.Lib(model_id, N, **weights)
    c = rng.uniform(-3, 3, (L, n))
    lib.add(rng.uniform(-3, 3, (L, n)), c, c, rng.uniform(10, 50, L), rng.normal(size=(L, N, n)), rng.normal(size=(L, N, m)),
            rng.integers(0, 3, L))
    return lib


# ---- retargeting ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model_id", [0, 1, 2, 3])
def test_no_neighbour_is_the_hosts_straight_line(model_id):
    H = g.host
    model = (H.FreeflyerSE2, H.DubinsCar, H.AstrobeeSE3, H.AstrobeeSE3Manifold)[model_id]()
    rng = np.random.default_rng(model_id)
    n = TL.X_DIM[model_id]
    for N in (3, 4, 50):
        lib = random_lib(model_id, N, 4, rng)
        x_init, x_goal = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
        ref = H.init_traj_straightline(host_top(model, x_init, x_goal, N, 40.0))
        X0, U0 = TL.retarget(lib, -1, x_init, x_goal, x_goal)
        assert np.array_equal(X0, ref.X.T) and not U0.any() and U0.shape == (N, TL.U_DIM[model_id])
        empty = TL.Lib(model_id, N)
        _, _, _, _, X, U, seeds = TL.seeded_problems(empty, [x_init, x_goal], [x_goal, x_init], [x_goal, x_init], 40.0, 3)
        assert (seeds["entry"] == -1).all() and np.isposinf(seeds["dist2"]).all() and not seeds["n_found"].any()
        assert all(np.array_equal(X[j], ref.X.T) for j in range(3)) and not U.any() and X.shape == (6, N, n)


@pytest.mark.parametrize("model_id", [0, 1, 2, 3])
def test_retargeting_ends_and_exact_hit(model_id):
    rng = np.random.default_rng(20 + model_id)
    n = TL.X_DIM[model_id]
    for N in (3, 4, 50):
        lib = random_lib(model_id, N, 5, rng)
        lib.X[:, 0], lib.X[:, -1] = lib.x_init, lib.c        # entries that start and end where their problems do, as solved ones
        x_init, lo = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
        hi = lo + rng.uniform(0, 0.5, n)
        hi[n - 1] = np.inf                                    # (its centre is 0)
        c = TL.goal_centre(lo, hi)
        for e in range(5):
            X0, U0 = TL.retarget(lib, e, x_init, lo, hi)
            assert np.array_equal(X0[0], x_init)              # knot 0 is x_init itself
            assert np.abs(X0[-1] - c).max() <= 4 * 2.0 ** -52 * (np.abs(lib.c[e]) + np.abs(c)).max()
            assert np.array_equal(U0, lib.U[e])
            t = np.arange(N) / (N - 1)
            want = lib.X[e] + np.outer(1 - t, x_init - lib.x_init[e]) + np.outer(t, c - lib.c[e])
            assert np.abs(X0[1:] - want[1:]).max() <= 8 * 2.0 ** -52 * TL.retarget_bound(lib, e, x_init, lo, hi).max()
            # the exact hit: only exact zeros are added
            Xh, Uh = TL.retarget(lib, e, lib.x_init[e], lib.c[e], lib.c[e])
            assert np.array_equal(Xh, lib.X[e]) and np.array_equal(Uh, lib.U[e])


# ---- the neighbour rule ---------------------------------------------------------------------------------------------------------
def test_neighbour_rule():
    nan, inf = np.nan, np.inf
    d = np.array([3.0, 1.5, nan, 1.5, 0.5, inf, 2.0])
    e, dd, nf = TL.neighbours(d, 3)
    assert list(e) == [4, 1, 3] and list(dd) == [0.5, 1.5, 1.5] and nf == 3                 # the tie goes to the lowest entry
    e, dd, nf = TL.neighbours(d, 8)
    assert list(e) == [4, 1, 3, 6, 0, 5, -1, -1] and nf == 6 and dd[5] == inf and np.isposinf(dd[6:]).all()   # +inf is a number, NaN never
    e, dd, nf = TL.neighbours(d, 2, elig=[1, 0, 1, 1, 0, 1, 0])                              # tags: entries 0, 2 (NaN), 3, 5
    assert list(e) == [3, 0] and nf == 2
    e, dd, nf = TL.neighbours(d, 3, elig=[0, 0, 1, 0, 0, 1, 0])                              # fewer eligible than K
    assert list(e) == [5, -1, -1] and nf == 1 and list(dd) == [inf, inf, inf]
    e, dd, nf = TL.neighbours(np.zeros(0), 2)                                                # an empty library
    assert list(e) == [-1, -1] and nf == 0
    e, dd, nf = TL.neighbours([nan, nan], 1)
    assert list(e) == [-1] and nf == 0
    assert list(TL.neighbours([-0.0, 0.0, 0.0], 3)[0]) == [0, 1, 2]                          # -0.0 == 0.0 is a tie


def test_distance_reads_the_positive_weights_only():
    rng = np.random.default_rng(3)
    lib = random_lib(0, 3, 6, rng, w_init=[1, 2, 0, 0, 0, 0], w_goal=0.0, w_tf=0.25)
    assert TL.n_terms(lib) == 3
    lib.x_init[:, 2:] = np.nan                     # never read
    lib.c[:] = np.inf
    xi, c = rng.uniform(-1, 1, 6), rng.uniform(-1, 1, 6)
    d = TL.dist2(lib, xi, c, 20.0)
    want = (xi[0] - lib.x_init[:, 0]) ** 2 + 2 * (xi[1] - lib.x_init[:, 1]) ** 2 + 0.25 * (20.0 - lib.tf) ** 2
    assert np.allclose(d, want, rtol=1e-15, atol=0)
    s = TL.search(lib, [xi, xi], [c, c], [c, c], [20.0, nan_tf()], 2, tag=[int(lib.tag[0]), 7])
    assert s["n_found"][1] == 0 and s["n_found"][0] == min(2, int((lib.tag == lib.tag[0]).sum()))
    assert all(lib.tag[e] == lib.tag[0] for e in s["entry"][0] if e >= 0)


def nan_tf():
    return float("nan")


def test_compaction():
    rng = np.random.default_rng(4)
    B, N = 7, 3
    x, c, tf = rng.normal(size=(B, 6)), rng.normal(size=(B, 6)), rng.uniform(1, 2, B)
    X, U, tag = rng.normal(size=(B, N, 6)), rng.normal(size=(B, N, 3)), np.arange(B) + 10
    lib = TL.Lib(0, N)
    assert lib.add_masked([1, 0, 1, 1, 0, 0, 1], x, c, c, tf, X, U, tag) == 4
    assert lib.add_masked(np.zeros(B), x, c, c, tf, X, U, tag) == 0
    assert lib.add_masked([0, 1, 0, 0, 0, 0, 0], x, c, c, tf, X, U) == 1
    assert list(lib.tag) == [10, 12, 13, 16, 0] and np.array_equal(lib.X, X[[0, 2, 3, 6, 1]]) and np.array_equal(lib.tf, tf[[0, 2, 3, 6, 1]])
    assert np.array_equal(lib.x_init, x[[0, 2, 3, 6, 1]]) and np.array_equal(lib.c, c[[0, 2, 3, 6, 1]]) and np.array_equal(lib.U, U[[0, 2, 3, 6, 1]])


# ---- the inputs of the GPU search tests -------------------------------------------------------------------------------------------
def search_case(model_id, L, seed=0):
    """(lib, x_init, lo, hi, tf) of tests/test_gpu_trajlib.py::test_search_against_the_restatement: a random library of L entries
    (N = 3) and five queries; model 0 also weighs tf, model 2 the positions only"""
    rng = np.random.default_rng(1000 * model_id + L + seed)
    weights = {0: dict(w_tf=0.01), 2: dict(w_init=[2.0] * 3 + [0.0] * 9, w_goal=[0.5] * 3 + [0.0] * 9)}.get(model_id, {})
    lib = random_lib(model_id, 3, L, rng, **weights)
    n = TL.X_DIM[model_id]
    lo = rng.uniform(-3, 3, (5, n))
    return lib, rng.uniform(-3, 3, (5, n)), lo, lo + rng.uniform(0, 0.2, (5, n)), rng.uniform(10, 50, 5)


@pytest.mark.parametrize("model_id", [0, 1, 2, 3])
def test_search_inputs_keep_their_distances_apart(model_id):
    for L in SEARCH_LS:
        lib, x_init, lo, hi, tf = search_case(model_id, L)
        for q in range(5):
            d = TL.dist2(lib, x_init[q], TL.goal_centre(lo[q], hi[q]), tf[q])
            assert TL.min_relative_gap(d, max(SEARCH_KS)) > 1e-12, (L, q)
            for t in range(3):
                assert TL.min_relative_gap(d[lib.tag == t], max(SEARCH_KS)) > 1e-12, (L, q, t)


# ---- the study ----------------------------------------------------------------------------------------------------------------------
def totals(results):
    return (sum(bool(r["converged"] and r["successful"]) for r in results), sum(r["iterations"] for r in results),
            sum(r["total_ipm_iters"] for r in results), max(r["iterations"] for r in results))


@functools.lru_cache(maxsize=None)
def oracle_study(model_id, N, L, Bq, xy_only=False):
    """the library: the generator's problems LIB_FIRST .. LIB_FIRST + L - 1 solved from the straight line on the oracle, the
    converged and successful ones kept; the first Bq problems of the generator from the straight line and from their nearest entry.
    Returns (lib, cold results, seeded results, seeds)"""
    import gusto_oracle as go
    P = g.problems
    gen, env = (P.freeflyer_batch, P.freeflyer_env()) if model_id == 0 else (P.dubins_batch, None)
    o = go.Oracle(model_id, N, boxes=env)
    lx, ll, lh, lt = gen(L, first=LIB_FIRST)
    solved = []
    for b in range(L):
        o.set_problem(lx[b], ll[b], lh[b], lt[b])
        solved.append(o.solve(STUDY_ITERS))
    lib = TL.Lib(model_id, N, **(dict(w_init=[1, 1, 0], w_goal=[1, 1, 0]) if xy_only else {}))
    lib.add_masked([r["converged"] and r["successful"] for r in solved], lx, ll, lh, lt, np.stack([r["X"] for r in solved]),
                   np.stack([r["U"] for r in solved]))
    x0, lo, hi, tf = gen(Bq)
    cold, seeded = [], []
    for b in range(Bq):
        o.set_problem(x0[b], lo[b], hi[b], tf[b])
        cold.append(o.solve(STUDY_ITERS))
    xi, l, h, t, X0, U0, seeds = TL.seeded_problems(lib, x0, lo, hi, tf, 1)
    for b in range(Bq):
        o.set_problem(xi[b], l[b], h[b], t[b], X0[b], U0[b])
        seeded.append(o.solve(STUDY_ITERS))
    return lib, cold, seeded, seeds


def test_freeflyer_study_is_pinned():
    """48 table queries against a library of 64: every query successful, about a third of the SCP iterations, the longest problem
    7 trips instead of 24"""
    lib, cold, seeded, seeds = oracle_study(0, 50, 64, 48)
    assert len(lib) == FREEFLYER_48["lib_good"] and (seeds["n_found"] == 1).all()
    assert totals(cold) == FREEFLYER_48["cold"] and totals(seeded) == FREEFLYER_48["seeded"]


def test_dubins_study_is_pinned():
    """64 queries against a library of 256: with the heading in the distance the seeds help, without it they do harm"""
    lib, cold, seeded, _ = oracle_study(1, 30, 256, 64)
    assert len(lib) == DUBINS_64["lib_good"]
    assert totals(cold) == DUBINS_64["cold"] and totals(seeded) == DUBINS_64["seeded"]
    _, _, seeded_xy, _ = oracle_study(1, 30, 256, 64, xy_only=True)
    assert totals(seeded_xy) == DUBINS_64["seeded_xy"]


def test_small_study_is_pinned():
    """the case tests/test_gpu_trajlib.py repeats on the device: 16 table queries against a library of 32.  The oracle's ratio of
    seeded to cold SCP iterations, 69 / 160, is the reference figure of the device's comparison."""
    lib, cold, seeded, _ = oracle_study(0, 50, 32, 16)
    assert len(lib) == FREEFLYER_16["lib_good"]
    assert totals(cold) == FREEFLYER_16["cold"] and totals(seeded) == FREEFLYER_16["seeded"]
    assert totals(seeded)[1] < totals(cold)[1]
