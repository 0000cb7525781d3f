"""The inputs of the long-horizon tests of the post-solve chain (gusto_verify / gusto_interpolate, gusto_tvlqr, gusto_simulate,
gusto_lincov), shared by tests/test_post_horizons_cpu.py (which checks their conditioning and measures the restatements' own
fp64 error, without a GPU) and tests/test_gpu_post_horizons.py.

Trajectories: np_tvlqr.smooth_batch, B = 2 problems with the first two dt of tests/sim_cases.py -- nothing crosses a problem, and
two keep the host references cheap.  DT, WEIGHTS, dx0, du0, env and bounds are sim_cases'; the actuator noise of gusto_lincov
is lincov_cases.du_white of the second and third roll-out mode, 2 % of the controls' size.

Horizons per model, with IPB = 256 // (n + m) the intervals one workgroup of tvlqr_linearise holds:
  N = IPB + 1, IPB + 2, 2 IPB + 1   the last tile full, the last tile with one interval, two full tiles
      (29, 30, 57 for freeflyerSE2; 65, 66, 129 for the Dubins car; 15, 16, 29 for astrobeeSE3; 14, 15, 27 for the manifold model)
  N = 129, 193, 256                 three and four waves of verify_kernel, its dynamic LDS on both sides of 64 KiB, the
                                    one-wave recursions and the per-knot LDS refresh over up to 255 knots in sequence
Roll-out modes (indices into sim_cases.MODES): nstep = 0 with dt_min = 0.2 everywhere (three substeps for both problems); at
the seam horizons and at N = 256 also nstep = 5, one full DENSE_TILE of verify_kernel plus one substep.  gusto_interpolate is
also run with dt_min = 0.27, which gives the two problems 2 and 3 substeps: rows of zeros behind the shorter one.

SEEDS: the smooth_batch seed of a (model, N) whose default trajectories fail a condition of tests/test_post_horizons_cpu.py;
empty -- every case passes them with seed 0."""
import functools

import numpy as np

import gusto_jl_amd as g
import lincov_cases as LC
import np_lincov as NL
import np_simulate as NS
import np_tvlqr as T
import sim_cases as SC

B = 2
DT = SC.DT[:B]
MODELS = SC.MODELS
LONG = (129, 193, 256)
S = 65                         # samples of gusto_simulate: one wave and one lane
MODE_DT, MODE_5 = 2, 1         # sim_cases.MODES: nstep = 0 with dt_min = 0.2; nstep = 5
DT_MIN_UNEVEN = 0.27           # gusto_interpolate: 2 and 3 substeps for the two problems
STARTS = LC.STARTS
SEEDS = {}
# gusto_tvlqr end to end (K, P_1 against the restatement's own AB and recursion) at these horizons: ten times 8.6e-14, rounded up
# to a power of ten -- the figure of tests/test_post_horizons_cpu.py, one fp64 rounding per inexact entry of AB carried through
# the recursion (profiles/tvlqr.txt, section 5).  The float64-against-long-double figure on the SAME AB, 5.8e-15, would by itself
# keep tests/test_gpu_tvlqr.py's 1e-13; it says nothing of what a difference in AB does, which is what this row compares
TOL_TVLQR_END = 1e-12


def ipb(model):
    n, m = g.MODEL_DIMS[model]
    return 256 // (n + m)


def seams(model):
    return (ipb(model) + 1, ipb(model) + 2, 2 * ipb(model) + 1)


def horizons(model):
    return tuple(sorted(set(seams(model) + LONG)))


def modes(model, N):
    return (MODE_DT, MODE_5) if N in seams(model) or N == 256 else (MODE_DT,)


CASES = [(model, N) for model in MODELS for N in horizons(model)]


def verify_lds_bytes(model, N):
    """dynamic LDS of verify_kernel<MODEL, true>: 8 nt DENSE_TILE n with nt = N rounded up to 64 and DENSE_TILE = 4"""
    return 8 * 64 * ((N + 63) // 64) * 4 * g.MODEL_DIMS[model][0]


@functools.lru_cache(maxsize=None)
def inputs(model, N):
    X, U = T.smooth_batch(model, B, N, seed=SEEDS.get((model, N), 0))
    X.setflags(write=False)
    U.setflags(write=False)
    return X, U, DT * (N - 1)


@functools.lru_cache(maxsize=None)
def linearisation(model, N, mode):
    """the restatement's own (AB [B, N-1, n, n+m], K [B, N-1, m, n], P [B, N, n, n]) with sim_cases' weights"""
    X, U, tf = inputs(model, N)
    Q, R, Qf = SC.WEIGHTS
    out = [T.tvlqr(model, X[b], U[b], tf[b], Q, R, Qf, **SC.MODES[mode]) for b in range(B)]
    res = tuple(np.stack([o[i] for o in out]) for i in range(3))
    for a in res:
        a.setflags(write=False)
    return res


def tvlqr_options(mode, **extra):
    Q, R, Qf = SC.WEIGHTS
    return dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode], **extra)


def perturbation(model):
    return SC.perturbation(model, S, nb=B)


def simulate_options(model, mode, **extra):
    """generated perturbations, clipping on, every dense sample checked"""
    lo, hi = SC.bounds(model, 1)
    return dict(n_samples=S, seed=SC.SEED, dx0=SC.dx0(model), du0=SC.du0(model), u_lo=lo, u_hi=hi, dense_collision=1,
                **SC.MODES[mode], **extra)


def simulate_reference(model, N, mode, K=None, dtype=np.float64):
    """the restatement's results of the two problems (a list of dicts) with the gains K (default: linearisation())"""
    X, U, tf = inputs(model, N)
    K = linearisation(model, N, mode)[1] if K is None else K
    lo, hi = SC.bounds(model, 1)
    boxes, spheres = SC.env(model)
    P = perturbation(model)
    return [NS.simulate(model, X[b], U[b], K[b], tf[b], P[b], lo, hi, boxes, spheres, dense_collision=True, dtype=dtype,
                        **SC.MODES[mode]) for b in range(B)]


def start(model, which):
    return None if which == "default" else LC.full_S0(model)[:B]


def lincov_options(model, N, mode, **extra):
    return LC.options(model, N, mode, **extra)


def lincov_reference(model, N, mode, which_start, AB=None, K=None, dtype=np.float64):
    """the restatement's results of the two problems (a list of dicts) on AB, K (default: linearisation()), environment "sim" """
    X, U, _ = inputs(model, N)
    if AB is None:
        AB, K, _ = linearisation(model, N, mode)
    boxes, spheres = SC.env(model)
    S0 = start(model, which_start)
    lo, hi = LC.bounds(model)
    return [NL.lincov(model, X[b], U[b], AB[b], K[b], None if S0 is None else S0[b], SC.dx0(model), SC.du0(model),
                      LC.du_white(model, N, mode), lo, hi, boxes, spheres, dtype=dtype) for b in range(B)]


# ---- the discrete Riccati recursion in any floating-point type ---------------------------------------------------------------
def _solve(A, Bm):
    """A^-1 Bm by Gaussian elimination with partial pivoting, in the type of A (numpy.linalg has no long double)"""
    A, Bm = A.copy(), Bm.copy()
    m = len(A)
    for c in range(m):
        p = c + int(np.argmax(np.abs(A[c:, c])))
        if p != c:
            A[[c, p]], Bm[[c, p]] = A[[p, c]], Bm[[p, c]]
        for r in range(c + 1, m):
            f = A[r, c] / A[c, c]
            A[r, c:] -= f * A[c, c:]
            Bm[r] -= f * Bm[c]
    for c in range(m - 1, -1, -1):
        Bm[c] = (Bm[c] - A[c, c + 1:] @ Bm[c + 1:]) / A[c, c]
    return Bm


def riccati(AB, Q, R, Qf, dtype=np.longdouble):
    """np_tvlqr.riccati, the same formulas, in `dtype`: K [N-1, m, n], P [N, n, n]"""
    AB = np.asarray(AB).astype(dtype)
    Nm1, n, nz = AB.shape
    m = nz - n
    Q, R, Qf = (np.diag(np.broadcast_to(np.asarray(v, float), (d,))).astype(dtype) for v, d in ((Q, n), (R, m), (Qf, n)))
    P = np.zeros((Nm1 + 1, n, n), dtype=dtype)
    K = np.zeros((Nm1, m, n), dtype=dtype)
    P[Nm1] = Qf
    for k in range(Nm1 - 1, -1, -1):
        A, Bd = AB[k, :, :n], AB[k, :, n:]
        K[k] = _solve(R + Bd.T @ P[k + 1] @ Bd, Bd.T @ P[k + 1] @ A)
        Pk = Q + A.T @ P[k + 1] @ (A - Bd @ K[k])
        P[k] = (Pk + Pk.T) / 2
    return K, P


def one_rounding(AB, seed):
    """AB with every inexact entry moved by one unit in the last place of its matrix's largest entry, signs seeded: what a second
    fp64 evaluation of the same Jacobians differs by (test_gpu_tvlqr's AB error is relative to that largest entry).  Entries that
    are exactly 0 or 1 -- the structure of [Ad | Bd], the same in any evaluation -- stay"""
    rng = np.random.default_rng(seed)
    scale = np.abs(AB).max(axis=(-2, -1), keepdims=True)
    moved = AB + np.finfo(np.float64).eps * scale * rng.choice([-1.0, 1.0], size=AB.shape)
    return np.where((AB == 0.0) | (AB == 1.0), AB, moved)
