"""The inputs of the gusto_lincov_dense tests, shared by tests/test_lincov_dense_cpu.py, tests/test_gpu_lincov_dense.py and
tools/lincov_dense_errors.py: tests/lincov_plant_cases.py as it stands (four models, N = 3, 4, 50, B = 5, three roll-out modes,
three environments, two start covariances, the dispersion), the restatement of the dense pass on them, and what the dense pass
adds:

The conditioning of the exactly compared indices: pair_dense of every sample, dense_sample and dense_pair of every problem.
The corner-cut case, built by hand: freeflyerSE2, N = 4, nstep = 5, a straight flight along x at constant speed with one small
  sphere beside the middle of the second interval.  The knots stay 0.9 away from it in x, the sample in the middle of the interval
  passes it at a fraction of that.
The seams of the dense kernel, one wave per interval and four intervals per workgroup: per model a horizon with more than one
  workgroup, a partial last one and N - 1 no multiple of four (N = 7: 6 intervals, 4 + 2); nstep = 64 at N = 3; N = 256 with B = 2."""
import functools

import numpy as np

import lincov_cases as LC
import lincov_plant_cases as PC
import np_lincov_dense as ND
import np_lincov_plant as NP
import np_tvlqr as T
import sim_cases as SC

B = LC.B
GAP = LC.GAP
SEAM_N = 7
SEAM_B = 2
LONG_N = 256
CAP_NSTEP = 64


def dense_reference(model, N, mode, which_env, which_start, AB=None, K=None, Cd=None, dtype=np.float64, disturbed=True, knot=None):
    """the restatement's dense results of the five problems (a list of dicts) behind the knot pass PC.reference(...) on the same
    AB, K, Cd (default: the restatement's own)"""
    X, U, tf, _ = LC.inputs(model, N)
    if knot is None:
        knot = PC.reference(model, N, mode, which_env, which_start, AB, K, Cd, dtype, disturbed)
    if K is None:
        _, K = LC.linearisation(model, N, mode)
    sets, _ = LC.env(model, which_env)
    return [ND.lincov_dense(model, X[b], U[b], K[b], knot[b], tf[b], LC.du_white(model, N, mode), PC.dw(model) if disturbed else 0.0,
                            sets[b][0], sets[b][1], dtype=dtype, **LC.MODES[mode]) for b in range(B)]


def _untied_gap(zp, dp, sp, at):
    """the gap between the two smallest pair margins of a sample, an exact tie of pairs with the same distance and deviation left
    out (lincov_cases.decision_gap: decided by the rule, not by rounding)"""
    same = np.ones(len(zp), bool)
    same[(zp == zp[at]) & (dp == dp[at]) & (sp == sp[at])] = False
    same[at] = True
    return LC._two_smallest_gap(zp[same])


def dense_gap(model, ref, boxes, spheres):
    """the smallest distance of one problem's dense result from a decision an exactly compared index rests on: the two smallest
    pair margins of every sample (pair_dense), the two smallest z_dense (dense_sample) and every (component, box) point of every
    sample from the box's face / edge switches"""
    import np_verify as V
    gap = np.inf
    live = [j for j in range(ref["nfull"]) if ref["z_pairs"][j] is not None]
    z = ref["z_dense"][live]
    if np.isfinite(z).sum() >= 2:
        # z_dense of an i = 0 sample is z_obs of its knot: equal samples do not occur, the runner-up decides
        gap = min(gap, LC._two_smallest_gap(z))
    bx, _ = V.obstacles(boxes, spheres)
    for j in live:
        zp = ref["z_pairs"][j]
        if len(zp) and ref["pair_dense"][j] >= 0:
            gap = min(gap, _untied_gap(zp, ref["d_pairs"][j], ref["sd_pairs"][j], ref["pair_dense"][j]))
        if model != 1:
            ws = V.WS_DIM[model]
            for off in V.COMPONENTS[model]:
                for b in bx:
                    gap = min(gap, LC.box_switch_gap(ref["xbar"][j][:ws] + off[:ws], b[0:3], b[3:6]))
    return gap


# ---- the corner-cut case ---------------------------------------------------------------------------------------------------------
CORNER = dict(model=0, N=4, mode=1, tf=6.0)      # nstep = 5: dt = 2, h = 0.4


@functools.lru_cache(maxsize=None)
def corner_inputs():
    """(X [1, 4, 6], U [1, 4, 3], tf [1], spheres [1, 4]): x from 0 to 5.4 at 0.9 per unit time, y = 0, no rotation, no thrust (the
    flight is a trajectory of the model: the roll-out follows it); the sphere of radius 0.05 at (2.7, 0.45), beside the middle of
    interval 2 -- 0.9 from knots 2 and 3 in x"""
    N, tf = CORNER["N"], CORNER["tf"]
    t = np.linspace(0.0, tf, N)
    X = np.zeros((1, N, 6))
    X[0, :, 0] = 0.9 * t
    X[0, :, 3] = 0.9
    U = np.zeros((1, N, 3))
    spheres = np.array([[2.7, 0.45, 0.0, 0.05]])
    for a in (X, U, spheres):
        a.setflags(write=False)
    return X, U, np.array([tf]), spheres


def corner_options():
    """the options of the corner-cut case: a start deviation of a few centimetres, a little white noise, no bounds"""
    return dict(dx0=np.array([0.03, 0.03, 0.02, 0.01, 0.01, 0.01]), du0=0.0, du_white=0.002)


@functools.lru_cache(maxsize=None)
def corner_reference(dtype=np.float64):
    """(knot pass, dense pass) of the restatement on its own AB, K, Cd"""
    X, U, tf, spheres = corner_inputs()
    model, mode = CORNER["model"], CORNER["mode"]
    Q, R, Qf = LC.WEIGHTS
    o = corner_options()
    AB, K, _ = T.tvlqr(model, X[0], U[0], tf[0], Q, R, Qf, **LC.MODES[mode])
    Cd = NP.sensitivities(model, X[0], U[0], tf[0], **LC.MODES[mode])
    knot = NP.lincov_plant(model, X[0], U[0], AB, K, Cd, None, None, o["dx0"], o["du0"], o["du_white"], PC.dw(model), PC.PLANT_REL,
                           None, None, None, spheres, dtype=dtype)
    dense = ND.lincov_dense(model, X[0], U[0], K, knot, tf[0], o["du_white"], PC.dw(model), None, spheres, dtype=dtype, **LC.MODES[mode])
    return knot, dense


# ---- the seams of the dense kernel -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_inputs(model, N=SEAM_N, nb=SEAM_B):
    X, U = T.smooth_batch(model, nb, N)
    return X, U, SC.DT[:nb] * (N - 1)


def seam_reference(model, X, U, tf, AB, K, Cd, mode_kw, which_env="sim"):
    """knot and dense pass of the restatement for seam inputs on the given AB, K, Cd, with the default starts and the dispersion"""
    sets = SC.env(model) if which_env == "sim" else (None, None)
    N = X.shape[1]
    out = []
    for b in range(len(X)):
        knot = NP.lincov_plant(model, X[b], U[b], AB[b], K[b], Cd[b], None, None, SC.dx0(model), SC.du0(model), LC.du_white(model, N, 1),
                               PC.dw(model), PC.PLANT_REL, None, None, sets[0], sets[1])
        out.append((knot, ND.lincov_dense(model, X[b], U[b], K[b], knot, tf[b], LC.du_white(model, N, 1), PC.dw(model), sets[0], sets[1],
                                          **mode_kw)))
    return out


# ---- two routes to the same covariance: chained one-step maps against the propagation inside the interval ------------------------
# With gains of zero, no noise and full S0 / Sth, sample j of the dense pass on (N = 50, nstep = 5) is knot j + 1 of the knot pass on
# the dense trajectory itself as N' = 246 knots with nstep = 1: the same nominal points, the one-step Jacobians chained by the
# recursion there, carried inside the interval here.
TWO_N, TWO_MODE = 50, 1
TWO_NS = 5


def two_route_dense(model, AB=None, Cd=None):
    """the first route in the restatement: (knot pass, dense pass) per problem with K = 0, du_white = dw = 0, the full starts, "sim" """
    N, mode = TWO_N, TWO_MODE
    X, U, tf, _ = LC.inputs(model, N)
    if AB is None:
        AB, _ = LC.linearisation(model, N, mode)
        Cd = PC.sensitivities(model, N, mode)
    n, m = ND.MODELS[model].n, ND.MODELS[model].m
    K0 = np.zeros((N - 1, m, n))
    sets, _ = LC.env(model, "sim")
    S0, Sth = LC.full_S0(model), PC.full_Sth(model)
    out = []
    for b in range(B):
        knot = NP.lincov_plant(model, X[b], U[b], AB[b], K0, Cd[b], S0[b], Sth[b], boxes=sets[b][0], spheres=sets[b][1])
        out.append((knot, ND.lincov_dense(model, X[b], U[b], K0, knot, tf[b], 0.0, 0.0, sets[b][0], sets[b][1], **LC.MODES[mode])))
    return out


def two_route_chained(model, Xd, Ud, AB=None, Cd=None):
    """the second route in the restatement: the knot pass on the dense trajectories Xd [B, 246, n] with the held controls Ud
    [B, 246, m] and nstep = 1 (AB, Cd: the restatement's own when None)"""
    _, _, tf, _ = LC.inputs(model, TWO_N)
    n, m = ND.MODELS[model].n, ND.MODELS[model].m
    N2 = Xd.shape[1]
    K0 = np.zeros((N2 - 1, m, n))
    sets, _ = LC.env(model, "sim")
    S0, Sth = LC.full_S0(model), PC.full_Sth(model)
    out = []
    for b in range(B):
        ab = T.linearise(model, Xd[b], Ud[b], tf[b], nstep=1) if AB is None else AB[b]
        cd = NP.sensitivities(model, Xd[b], Ud[b], tf[b], nstep=1) if Cd is None else Cd[b]
        out.append(NP.lincov_plant(model, Xd[b], Ud[b], ab, K0, cd, S0[b], Sth[b], boxes=sets[b][0], spheres=sets[b][1]))
    return out


def held_controls(U, ns=TWO_NS):
    """U' [B, (N - 1) ns + 1, m]: U[:, k] held over the ns samples of interval k, the last knot's control behind them"""
    return np.concatenate([np.repeat(U[:, :-1], ns, axis=1), U[:, -1:]], axis=1)
