"""The inputs that tests/test_gpu_roadmap.py sends to the device, and their reference (tests/np_roadmap.py), in one place:
tests/test_roadmap_cpu.py asserts on these very inputs that every decision has a margin of 1e-9 or more, so the device is
never judged on a coin toss.  Shapes: the smallest at which the kernels can go wrong (see the GPU file)."""
import functools

import numpy as np

import np_roadmap as RM

X_DIM = {0: 6, 1: 3, 2: 12, 3: 13}
WS_DIM = {0: 2, 1: 2, 2: 3, 3: 3}
MARGIN = 1e-9
STUDY_B, STUDY_N, STUDY_ITERS = 48, 50, 30
STUDY_OPTS = dict(inflate=0.157 + 0.02, pad=0.03)    # the draft's options: radius + 0.02, 0.03
STUDY_SEED_FAILS = {1, 37}     # what the roadmap seed leaves unanswered on the CPU oracle (tests/test_roadmap_cpu.py pins it)
STUDY_TRIPS = (522, 512)       # GuSTO trips over the 48 queries: straight line, roadmap seed


def scene(WS, C, seed, n_sph=None):
    """C keep-out components on a jittered grid in [0, 6]^WS, boxes then spheres, nothing symmetric: (boxes [nb, 6], spheres [ns, 4])"""
    rng = np.random.default_rng(seed)
    ns = C // 4 if n_sph is None else n_sph
    side = 1
    while side ** WS < C:
        side += 1
    cell = 6.0 / side
    cells = rng.permutation(side ** WS)[:C]
    boxes, spheres = [], []
    for i, c in enumerate(cells):
        ctr = np.array([(c // side ** j) % side for j in range(WS)], float) * cell + 0.5 * cell + rng.uniform(-0.1, 0.1, WS) * cell
        ctr3 = np.concatenate([ctr, rng.uniform(-1, 1, 3 - WS)])
        if i < C - ns:
            half = np.concatenate([rng.uniform(0.12, 0.3, WS) * cell, rng.uniform(0.1, 0.5, 3 - WS)])
            boxes.append(np.concatenate([ctr3 - half, ctr3 + half]))
        else:
            spheres.append(np.concatenate([ctr3, [rng.uniform(0.12, 0.3) * cell]]))
    return np.array(boxes, float).reshape(-1, 6), np.array(spheres, float).reshape(-1, 4)


def queries(model, Bq, seed, open_goal=False):
    """Bq queries across the scene: starts left of it, goals right of it, the other states small; (x_init, goal_lo, goal_hi, tf)"""
    rng = np.random.default_rng(1000 + seed)
    n, WS = X_DIM[model], WS_DIM[model]
    x0, xg = rng.uniform(-0.2, 0.2, (Bq, n)), rng.uniform(-0.2, 0.2, (Bq, n))
    x0[:, 0], xg[:, 0] = rng.uniform(-1.0, -0.5, Bq), rng.uniform(6.5, 7.0, Bq)
    x0[:, 1:WS], xg[:, 1:WS] = rng.uniform(0.5, 5.5, (Bq, WS - 1)), rng.uniform(0.5, 5.5, (Bq, WS - 1))
    lo, hi = xg.copy(), xg.copy()
    if open_goal:   # a box goal and an unconstrained entry: the straight line's rule for the centre
        lo[:, WS] -= 0.05
        hi[:, WS] += 0.07
        lo[:, n - 1], hi[:, n - 1] = -np.inf, np.inf
    return x0, lo, hi, rng.uniform(30.0, 60.0, Bq)


def _case(name, model, N, C, Bq, K, seed, inflate=0.1, pad=0.03, open_goal=False, envs=None, around_last=False):
    x0, lo, hi, tf = queries(model, Bq, seed, open_goal)
    if around_last:   # query 0 from one side of the last component to the other: its corners are on the path
        WS = WS_DIM[model]
        c, R = scene(WS, C, seed)[1][-1][:WS], scene(WS, C, seed)[1][-1][3] + inflate
        x0[0, :WS], lo[0, :WS] = c, c
        x0[0, 0], lo[0, 0] = c[0] - (R + 0.3), c[0] + (R + 0.3)
        x0[0, 1], lo[0, 1] = c[1] + 0.05, c[1] - 0.07
        hi[0, :WS] = lo[0, :WS]
    return dict(name=name, model=model, N=N, Bq=Bq, K=K, x_init=x0, goal_lo=lo, goal_hi=hi, tf=tf,
                envs=scene(WS_DIM[model], C, seed) if envs is None else envs, opts=dict(inflate=inflate, pad=pad))


def _mixed():
    a, b = scene(2, 3, 31), scene(2, 17, 32)
    return [a, b, a, b, b]


CASES = {c["name"]: c for c in (
    _case("plane_c0", 0, 3, 0, 1, 1, 1),
    _case("plane_c1", 0, 4, 1, 5, 3, 2, inflate=0.5),
    _case("plane_c16", 0, 50, 16, 5, 3, 3, open_goal=True),
    _case("plane_c16_k1", 0, 4, 16, 5, 1, 3),
    _case("plane_c17", 0, 50, 17, 5, 3, 4, around_last=True),
    _case("space_c9", 2, 50, 9, 5, 3, 5, inflate=0.3, open_goal=True),
    _case("space_c64", 2, 4, 64, 5, 3, 6, inflate=0.15),
    _case("dubins_c3", 1, 3, 3, 1, 1, 7, inflate=0.4),
    _case("manifold_c9", 3, 4, 9, 1, 3, 8, inflate=0.3),
    _case("plane_mixed", 0, 4, 0, 5, 3, 9, envs=_mixed()),
)}


@functools.lru_cache(maxsize=None)
def reference(name, straight_first=0):
    """np_roadmap on the case: computed once, shared, never written to"""
    c = CASES[name]
    return RM.roadmap_batch(c["x_init"], c["goal_lo"], c["goal_hi"], c["envs"], WS_DIM[c["model"]], c["N"], c["K"],
                            straight_first=straight_first, **c["opts"])


@functools.lru_cache(maxsize=None)
def study_reference():
    """the first 48 table queries with the draft's options, K = 1"""
    import gusto_jl_amd as g
    x0, lo, hi, tf = g.problems.freeflyer_batch(STUDY_B)
    env = (g.problems.freeflyer_env(), np.zeros((0, 4)))
    return RM.roadmap_batch(x0, lo, hi, env, 2, STUDY_N, 1, **STUDY_OPTS), (x0, lo, hi, tf)
