"""The inputs of the gusto_simulate tests, shared by tests/test_simulate_cpu.py (which checks their conditioning with the numpy
restatement alone), tests/test_gpu_simulate.py and tools/simulate_errors.py.

Trajectories: np_tvlqr.smooth_batch, B = 5 problems of different tf (the dt of tests/test_gpu_tvlqr.py).  Gains: np_tvlqr.tvlqr
with the uniform WEIGHTS here; the GPU tests take the device's own.  Environment (models 0, 2, 3): two spheres and a box next to
the common straight line of the batch.  A case is (model, N, S, mode, dense_collision, clip, generated): the seams of the
kernel -- S = 1, 63, 64, 65 (wave boundary), 256, 257 (tile boundary, second launch) at N = 3, S = 65 at N = 50 and 65 -- with
the roll-out modes, dense_collision, clipping and the source of the perturbations cycled over them so that every value of every
option meets every model."""
import functools

import numpy as np

import np_simulate as NS
import np_tvlqr as T

B = 5
DT = np.array([0.5, 0.58, 0.45, 0.7, 0.55])       # dt of the five problems; dt_min = 0.2 gives 3, 3, 3, 4, 3 substeps
MODES = (dict(nstep=1), dict(nstep=5), dict(nstep=0, dt_min=0.2))
MODELS = (0, 1, 2, 3)
SHAPES = ((3, 1), (3, 63), (3, 64), (3, 65), (3, 256), (3, 257), (50, 65), (65, 65))
SEED = 2024
WEIGHTS = (100.0, 1.0, 100.0)     # Q, R, Qf of the gains, uniform: smooth_batch is not a trajectory of the models (its knots do not
                                  # follow from one another), the law has a defect of ~0.1 per interval to work against, and tight
                                  # tracking keeps the closed loop inside the range where the models are benign
CLIP = {0: 2.2, 1: 0.95, 2: 0.9, 3: 0.9}   # bounds of the clipped cases in units of np_tvlqr._U_SCALE
BAND = 1e-9          # a sample closer than this to a decision (distance 0, a control bound) is left out of the exact comparisons
CASES = [(model, N, S, (i + model) % 3, (i + model) % 2, ((i + 1) // 2 + model) % 2, (i + 1) % 2)
         for model in MODELS for i, (N, S) in enumerate(SHAPES)]


def dx0(model):
    """half-widths of the start perturbation: a few per cent of the states' ranges"""
    return 0.1 * T._X_AMP[model]


def du0(model):
    return 0.05 * T._U_SCALE[model]


def bounds(model, clip):
    """(u_lo, u_hi): CLIP times the size of the nominal controls when clipping is on (a mixed box: one entry unbounded above)"""
    m = len(T._U_SCALE[model])
    if not clip:
        return np.full(m, -np.inf), np.full(m, np.inf)
    hi = CLIP[model] * T._U_SCALE[model]
    lo = -hi.copy()
    if m > 1:
        hi[-1] = np.inf
    return lo, hi


def env(model):
    """(boxes, spheres) next to the line the trajectories of the batch wind around; None, None for the Dubins car"""
    if model == 1:
        return None, None
    a, b = T._X_A[model][:3].copy(), T._X_B[model][:3].copy()
    if model == 0:
        a[2] = b[2] = 0.0           # (the plane: only the first two coordinates are read)
    mid, q = 0.5 * (a + b), 0.25 * a + 0.75 * b
    r = NS.MODELS[model].r
    off = np.array([0.0, r + 0.1 + (0.255 if model == 0 else 0.27), 0.0])
    spheres = np.array([np.concatenate([mid + off, [0.1]]), np.concatenate([q - off, [0.12]])])
    c = 0.75 * a + 0.25 * b + np.array([r + 0.25 + (0.2 if model == 0 else 0.02), 0.0, 0.0])
    boxes = np.array([np.concatenate([c - 0.2, c + 0.2])])
    return boxes, spheres


@functools.lru_cache(maxsize=None)
def inputs(model, N):
    X, U = T.smooth_batch(model, B, N)
    return X, U, DT * (N - 1), WEIGHTS


@functools.lru_cache(maxsize=None)
def gains(model, N, mode):
    """the restatement's gains [B, N-1, m, n] (the roll-out mode of the gains is the roll-out mode of the case)"""
    X, U, tf, (Q, R, Qf) = inputs(model, N)
    K = np.stack([T.tvlqr(model, X[b], U[b], tf[b], Q, R, Qf, **MODES[mode])[1] for b in range(B)])
    K.setflags(write=False)
    return K


def perturbation(model, S, first_problem=0, nb=B):
    return NS.perturbations(model, nb, S, dx0(model), du0(model), SEED, first_problem)


def reference(case, K=None, dtype=np.float64):
    """the restatement's results of the five problems of a case (a list of dicts), with the gains K (default: gains())"""
    model, N, S, mode, dense, clip, _ = case
    X, U, tf, _ = inputs(model, N)
    K = gains(model, N, mode) if K is None else K
    lo, hi = bounds(model, clip)
    boxes, spheres = env(model)
    P = perturbation(model, S)
    return [NS.simulate(model, X[b], U[b], K[b], tf[b], P[b], lo, hi, boxes, spheres, dense_collision=bool(dense), dtype=dtype,
                        **MODES[mode]) for b in range(B)]


def undecided(ref):
    """[S] mask of one problem's samples within BAND of a decision: |sample_min_dist| or the clip margin"""
    return (np.abs(ref["sample_min_dist"]) < BAND) | (ref["clip_margin"] < BAND)
