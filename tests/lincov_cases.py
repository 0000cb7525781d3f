"""The inputs of the gusto_lincov tests, shared by tests/test_lincov_cpu.py (which checks their conditioning with the numpy
restatement alone), tests/test_gpu_lincov.py and tools/lincov_errors.py.

Trajectories: np_tvlqr.smooth_batch, B = 5 problems with the DT, MODES, WEIGHTS, dx0 and du0 of tests/sim_cases.py.  Horizons
N = 3, 4 and 50 on all four models: the kernel is one wave per problem with the knots in sequence, so what can go wrong is the
first and the last knot and the prefetch of the next one.  Environments (models 0, 2, 3): sim_cases.env for the whole batch, an
empty set, and a per-problem layout (gusto_set_env_batch) with 0, 1, 31, 33 and 64 components -- with freeflyerSE2's two robot
components 62, 66 and 128 pairs, on both sides of the 64-lane boundary: small spheres scattered away from the batch's line, and
the three components of sim_cases.env, the nearest ones, first.  Start covariances: the default diagonal one and a full one."""
import functools

import numpy as np

import np_lincov as NL
import np_tvlqr as T
import sim_cases as SC

B = SC.B
DT, MODES, WEIGHTS, MODELS = SC.DT, SC.MODES, SC.WEIGHTS, SC.MODELS
HORIZONS = (3, 4, 50)
ENVS = ("sim", "empty", "batch")
BATCH_COUNTS = (0, 1, 31, 33, 64)      # keep-out components of the five problems of the "batch" environment
STARTS = ("default", "full")
GAP = 1e-9            # the inputs keep every decision an exactly compared index rests on further than this from flipping
CASES = [(model, N) for model in MODELS for N in HORIZONS]


def inputs(model, N):
    return SC.inputs(model, N)


def du_white(model, N, mode):
    """actuator noise of a case: 2 % of the controls' size in the second and third roll-out mode; in the first none at N = 3, 4
    and 1 % at N = 50.  Without it the feedback cancels the constant offset along a long horizon: the variances of the rates and
    of the commanded control decay geometrically to rounding noise, and a square root turns a relative 1e-16 of the largest
    variance into 1e-8 of the largest deviation -- no comparison, and no index, can rest on such values
    (tests/test_lincov_cpu.py holds the float64 restatement against the long double one on these inputs)."""
    return (0.02 if mode else (0.01 if N >= 50 else 0.0)) * T._U_SCALE[model]


def bounds(model):
    """(u_lo, u_hi) of the control margins: sim_cases' clipped box (one entry unbounded above)"""
    return SC.bounds(model, 1)


@functools.lru_cache(maxsize=None)
def scattered(model):
    """[61, 4] small spheres at 1.5 .. 3 from the line the trajectories of the batch wind around"""
    rng = np.random.default_rng(4242 + model)
    a, b = T._X_A[model][:3].copy(), T._X_B[model][:3].copy()
    if model == 0:
        a[2] = b[2] = 0.0
    t = (b - a) / np.linalg.norm(b - a)
    out = []
    for _ in range(61):
        v = rng.normal(size=3)
        if model == 0:
            v[2] = 0.0
        v -= (v @ t) * t
        v /= np.linalg.norm(v)
        c = a + rng.uniform(-0.2, 1.2) * (b - a) + rng.uniform(1.5, 3.0) * v
        out.append(np.concatenate([c, [0.03]]))
    out = np.array(out)
    out.setflags(write=False)
    return out


def env(model, which):
    """the keep-out sets of the five problems, a list of (boxes, spheres), and whether they are one shared set (gusto_set_env)
    or per problem (gusto_set_env_batch)"""
    if model == 1 or which == "empty":
        return [(None, None)] * B, True
    boxes, spheres = SC.env(model)
    if which == "sim":
        return [(boxes, spheres)] * B, True
    sets = []
    for c in BATCH_COUNTS:
        if c == 0:
            sets.append((None, None))
        elif c == 1:
            sets.append((boxes, None))
        else:
            sets.append((boxes, np.vstack([spheres, scattered(model)[:c - 3]])))
    return sets, False


@functools.lru_cache(maxsize=None)
def full_S0(model):
    """[B, n + m, n + m]: dense positive semi-definite start covariances of the size of the default one, symmetric to the bit"""
    n, m = NL.MODELS[model].n, NL.MODELS[model].m
    rng = np.random.default_rng(99 + model)
    w = np.concatenate([SC.dx0(model), SC.du0(model)])
    out = []
    for _ in range(B):
        L = 0.5 * w[:, None] * rng.normal(size=(n + m, n + m))
        S = L @ L.T
        out.append(0.5 * (S + S.T))
    out = np.array(out)
    out.setflags(write=False)
    return out


def start(model, which):
    return None if which == "default" else full_S0(model)


@functools.lru_cache(maxsize=None)
def linearisation(model, N, mode):
    """the restatement's own (AB [B, N-1, n, n+m], K [B, N-1, m, n]) with sim_cases' weights"""
    X, U, tf, (Q, R, Qf) = inputs(model, N)
    out = [T.tvlqr(model, X[b], U[b], tf[b], Q, R, Qf, **MODES[mode]) for b in range(B)]
    AB, K = np.stack([o[0] for o in out]), np.stack([o[1] for o in out])
    AB.setflags(write=False)
    K.setflags(write=False)
    return AB, K


def reference(model, N, mode, which_env, which_start, AB=None, K=None, dtype=np.float64):
    """the restatement's results of the five problems (a list of dicts) on AB, K (default: linearisation())"""
    X, U, _, _ = inputs(model, N)
    if AB is None:
        AB, K = linearisation(model, N, mode)
    sets, _ = env(model, which_env)
    S0 = start(model, which_start)
    lo, hi = bounds(model)
    return [NL.lincov(model, X[b], U[b], AB[b], K[b], None if S0 is None else S0[b], SC.dx0(model), SC.du0(model), du_white(model, N, mode),
                      lo, hi, sets[b][0], sets[b][1], dtype=dtype) for b in range(B)]


def options(model, N, mode, **extra):
    """the dict BatchSolver.lincov takes for a case"""
    lo, hi = bounds(model)
    return dict(dx0=SC.dx0(model), du0=SC.du0(model), du_white=du_white(model, N, mode), u_lo=lo, u_hi=hi, **extra)


def _two_smallest_gap(v):
    v = np.sort(np.asarray(v, float)[np.isfinite(v)])
    return np.inf if len(v) < 2 else v[1] - v[0]


def box_switch_gap(q, lo, hi):
    """how far the point q is from the places where the distance to the box [lo, hi] changes its formula: the planes of the
    faces (inside / outside per axis) and, inside, the tie between the two nearest faces"""
    d = len(q)
    lo, hi = np.asarray(lo, float)[:d], np.asarray(hi, float)[:d]
    gap = min(np.abs(q - lo).min(), np.abs(hi - q).min())
    if np.all((q >= lo) & (q <= hi)):
        gap = min(gap, _two_smallest_gap(np.concatenate([q - lo, hi - q])))
    return gap


def decision_gap(model, X, ref, boxes, spheres):
    """the smallest distance of one problem's result `ref` (np_lincov.lincov) from a decision the exactly compared indices rest
    on: the two smallest z_obs and the two smallest per-knot control minima over the knots (obs_knot, ctl_knot), the two smallest
    pair margins at obs_knot (obs_pair) and control margins at ctl_knot (ctl_entry), and every (component, box) point of every
    knot from the box's face / edge switches.  Pairs may tie exactly: the two components of freeflyerSE2 in front of the same face of
    a box have the same distance, normal and deviation, bit for bit; such a tie is decided by the rule (the lowest ordinal), not
    by rounding, and is left out of the gap."""
    import np_verify as V
    gap = min(_two_smallest_gap(ref["z_obs"]), _two_smallest_gap(ref["z_ctl"].min(axis=1)))
    if ref["obs_knot"]:
        k = ref["obs_knot"] - 1
        zp, same = ref["z_pairs"][k], np.ones(len(ref["z_pairs"][k]), bool)
        tie = zp == zp[ref["obs_pair"]]
        # an exact tie of pairs with the same distance and the same deviation is no decision by rounding: the lowest ordinal wins
        same[tie & (ref["d_pairs"][k] == ref["d_pairs"][k][ref["obs_pair"]]) & (ref["sd_pairs"][k] == ref["sd_pairs"][k][ref["obs_pair"]])] = False
        same[ref["obs_pair"]] = True
        gap = min(gap, _two_smallest_gap(zp[same]))
    if ref["ctl_knot"]:
        gap = min(gap, _two_smallest_gap(ref["z_ctl"][ref["ctl_knot"] - 1]))
    bx, _ = V.obstacles(boxes, spheres)
    if model != 1:
        ws = V.WS_DIM[model]
        for x in X:
            for off in V.COMPONENTS[model]:
                for b in bx:
                    gap = min(gap, box_switch_gap(x[:ws] + off, b[0:3], b[3:6]))
    return gap
