"""The inputs of the gusto_simulate_disturbed tests, shared by tests/test_simulate_disturbed_cpu.py (which checks their
conditioning with the numpy restatement alone), tests/test_gpu_simulate_disturbed.py and tools/simulate_errors.py.

Everything gusto_simulate's tests use is kept: the trajectories, tf, weights, environment, bounds and perturbations of
tests/sim_cases.py, B = 5.  A case is (model, N, S, mode, dense_collision, clip, generated pert, plant source, white source) with
the sources 0 = off (zero half-widths, no array), 1 = generated on the device, 2 = supplied by the caller (the array the
generator would have drawn, so both sources mean the same numbers).  Shapes: S = 1, 64, 65 (wave boundary), 257 (tile boundary,
second launch) at N = 3 and S = 65 at N = 50, on each model; the options are cycled so that every source meets every model.
Dispersion: plant_rel = 0.1 on mass, dubins_v and dubins_k, (0.05, 0.1, 0.15) on Jdiag; dw = 0.05 np_tvlqr._U_SCALE."""
import numpy as np

import np_simulate_disturbed as ND
import np_tvlqr as T
import sim_cases as SC

B, SEED, BAND, MODELS, MODES = SC.B, SC.SEED, SC.BAND, SC.MODELS, SC.MODES
SHAPES = ((3, 1), (3, 64), (3, 65), (3, 257), (50, 65))
OFF, GENERATED, SUPPLIED = 0, 1, 2
PLANT_REL = np.array([0.1, 0.05, 0.1, 0.15, 0.1, 0.1])
# (clipping is always on at the real horizon: at N = 3 the bounds of sim_cases clip every sample of the two Astrobee models or
# none, only along 49 intervals do clipped and unclipped samples both occur)
CASES = [(model, N, S, (i + model) % 3, (i + model) % 2, 1 if N == 50 else ((i + 1) // 2 + model) % 2, (i + 1) % 2, (i + model) % 3,
          (2 * i + model) % 3) for model in MODELS for i, (N, S) in enumerate(SHAPES)]
IDS = lambda c: "m%d-N%d-S%d-mode%d-dense%d-clip%d-gen%d-plant%d-white%d" % c   # noqa: E731


def dw(model):
    return 0.05 * T._U_SCALE[model]


def plant_rel(src):
    return PLANT_REL if src != OFF else np.zeros(ND.NPLANT)


def plant(model, S, nominal, src, first_problem=0, nb=B):
    """theta [nb, S, 6] of a case: the nominal plant (off), or what the generator draws"""
    return ND.plants(nominal, nb, S, plant_rel(src), SEED, first_problem)


def white(model, N, S, src, first_problem=0, nb=B):
    """w [nb, N-1, S, m] of a case: zeros (off), or what the generator draws"""
    return ND.whites(model, nb, N, S, dw(model) if src != OFF else 0.0, SEED, first_problem)


def reference(case, K=None, dtype=np.float64, nominal=None):
    """the restatement's results of the five problems of a case (a list of dicts), with the gains K (default: sim_cases.gains())
    and the nominal plant `nominal` (default: np_models' constants)"""
    model, N, S, mode, dense, clip, _, psrc, wsrc = case
    X, U, tf, _ = SC.inputs(model, N)
    K = SC.gains(model, N, mode) if K is None else K
    lo, hi = SC.bounds(model, clip)
    boxes, spheres = SC.env(model)
    P = SC.perturbation(model, S)
    th = plant(model, S, ND.nominal(model) if nominal is None else nominal, psrc)
    W = white(model, N, S, wsrc)
    return [ND.simulate(model, X[b], U[b], K[b], tf[b], P[b], th[b], W[b], lo, hi, boxes, spheres, dense_collision=bool(dense),
                        dtype=dtype, **MODES[mode]) for b in range(B)]


undecided = SC.undecided
