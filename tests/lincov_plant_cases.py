"""The inputs of the gusto_lincov_disturbed tests, shared by tests/test_lincov_plant_cpu.py, tests/test_gpu_lincov_plant.py and
tools/lincov_plant_errors.py: tests/lincov_cases.py (four models, N = 3, 4, 50, B = 5, three roll-out modes, three environments,
two start covariances) with a dispersion added.

Dispersion: plant_rel = 0.08134 on the mass (the reference free-flyer's 15.36 .. 18.08 kg) and 0.05 on the inertias and the Dubins
constants; half-widths dw of the per-interval noise of 3 % of the controls' size; the start "default" takes the default Stheta of
plant_rel, the start "full" one dense positive semi-definite Sth per problem of the same size, symmetric to the bit, whose
entries on the scalars the model does NOT read are garbage (a NaN among them): they must not be looked at.

The seam cases: one horizon per model at which the N - 1 intervals span two workgroup tiles of the sensitivity kernel with a
partial last one -- 256 lanes over 2 read scalars give 128 intervals per tile (freeflyerSE2, DubinsCar: N = 130), over 4 give 64
(both Astrobee models: N = 66).

The roll-out consistent inputs of the closed-loop sensitivity check: X[:, k+1] = F_k(X[:, k], U[:, k]) under theta_nom in
np_simulate_disturbed's arithmetic, so the nominal sample tracks X exactly."""
import functools

import numpy as np

import lincov_cases as LC
import np_lincov_plant as NP
import np_simulate as NS
import np_simulate_disturbed as NSD
import np_tvlqr as T
import sim_cases as SC

B = LC.B
PLANT_REL = np.array([0.08134, 0.05, 0.05, 0.05, 0.05, 0.05])
SEAM_N = {0: 130, 1: 130, 2: 66, 3: 66}
SEAM_B = 2
EPS_FD = 2e-5     # relative step of the central differences over the plant scalars, where their truncation and rounding errors
#                   balance: against np_lincov_plant on the CONSISTENT cases the worst disagreement is 2.8e-9, 5.1e-9, 2.0e-8, 8.2e-8 at
#                   1e-5, 2e-5, 4e-5, 8e-5 -- the truncation, ~13 eps^2, takes over above 2e-5, the rounding of states of size 40
#                   that a relative change of a scalar moves by 1e-2 or less, 2^-53 x 4e3 / eps, below (CPU only; profiles/lincov_plant.txt)


def dw(model):
    """half-widths of the noise drawn anew in every hold interval"""
    return 0.03 * T._U_SCALE[model]


@functools.lru_cache(maxsize=None)
def full_Sth(model):
    """[B, 6, 6]: dense positive semi-definite covariances of the size of the default one on the scalars the model reads,
    symmetric to the bit; garbage elsewhere (1e3 and, in problem 2, a NaN)"""
    rng = np.random.default_rng(777 + model)
    w = NSD.nominal(model) * PLANT_REL
    r = NP.read_mask(model)
    out = []
    for b in range(B):
        L = 0.5 * w[:, None] * rng.normal(size=(NP.NPLANT, NP.NPLANT))
        S = L @ L.T
        S = 0.5 * (S + S.T)
        S[~(r[:, None] & r[None, :])] = 1e3
        if b == 2:
            j = int(np.flatnonzero(~r)[0])
            S[j, j] = np.nan
        out.append(S)
    out = np.array(out)
    out.setflags(write=False)
    return out


def start_theta(model, which):
    return None if which == "default" else full_Sth(model)


@functools.lru_cache(maxsize=None)
def sensitivities(model, N, mode):
    """the restatement's own Cd [B, N-1, n, 6]"""
    X, U, tf, _ = LC.inputs(model, N)
    Cd = np.stack([NP.sensitivities(model, X[b], U[b], tf[b], **LC.MODES[mode]) for b in range(B)])
    Cd.setflags(write=False)
    return Cd


def reference(model, N, mode, which_env, which_start, AB=None, K=None, Cd=None, dtype=np.float64, disturbed=True):
    """the restatement's results of the five problems (a list of dicts) on AB, K, Cd (default: the restatement's own);
    disturbed = False: zero dispersion"""
    X, U, _, _ = LC.inputs(model, N)
    if AB is None:
        AB, K = LC.linearisation(model, N, mode)
    if Cd is None:
        Cd = sensitivities(model, N, mode)
    sets, _ = LC.env(model, which_env)
    S0 = LC.start(model, which_start)
    Sth = start_theta(model, which_start) if disturbed else None
    lo, hi = LC.bounds(model)
    return [NP.lincov_plant(model, X[b], U[b], AB[b], K[b], Cd[b], None if S0 is None else S0[b], None if Sth is None else Sth[b],
                            SC.dx0(model), SC.du0(model), LC.du_white(model, N, mode), dw(model) if disturbed else 0.0,
                            PLANT_REL if disturbed else 0.0, lo, hi, sets[b][0], sets[b][1], dtype=dtype) for b in range(B)]


def disturb(model):
    """the dict BatchSolver.lincov_disturbed takes as `disturb`"""
    return dict(plant_rel=PLANT_REL, dw=dw(model))


# ---- the seam of the sensitivity kernel -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def seam_inputs(model):
    N = SEAM_N[model]
    X, U = T.smooth_batch(model, SEAM_B, N)
    return X, U, SC.DT[:SEAM_B] * (N - 1)


# ---- roll-out consistent trajectories and the closed-loop sensitivity -----------------------------------------------------------
# (model, N, roll-out mode); astrobeeSE3 stays short: lincov_cases' controls, flown open loop, take its MRP past the unit sphere
CONSISTENT = [(0, 50, 2), (1, 50, 0), (2, 4, 1), (2, 12, 0), (3, 4, 2), (3, 50, 1)]


@functools.lru_cache(maxsize=None)
def consistent_inputs(model, N, mode):
    """(X, U, tf): lincov_cases' U and first knot, every later knot the image of the one before under theta_nom"""
    X, U, tf, _ = LC.inputs(model, N)
    X = X.copy()
    th = NSD.nominal(model)[:, None]
    for b in range(B):
        ns = NS.n_substeps(tf[b], N, **LC.MODES[mode])
        h = np.float64(tf[b]) / np.float64(N - 1) / np.float64(ns)
        for k in range(N - 1):
            x = X[b, k][:, None]
            for _ in range(ns):
                x = NSD.rk4_step(model, x, U[b, k][:, None], h, th)
            X[b, k + 1] = x[:, 0]
    X.setflags(write=False)
    return X, U, tf


def fd_plants(model, eps=EPS_FD):
    """theta [S, 6], S = 1 + 2 |reads|: the nominal plant, then theta_nom (1 + eps e_j) and theta_nom (1 - eps e_j) for every
    scalar j the model reads"""
    th0 = NSD.nominal(model)
    rows = [th0]
    for j in NSD.READS[model]:
        for s in (1.0, -1.0):
            t = th0.copy()
            t[j] = th0[j] * (1.0 + s * eps)
            rows.append(t)
    return np.array(rows)


def fd_sensitivity(model, Xcl, theta):
    """[N, n, 6] central differences of Xcl [N, S, n] of the plants fd_plants() made (theta: the scalars actually used)"""
    N, _, n = Xcl.shape
    out = np.zeros((N, n, NP.NPLANT))
    for c, j in enumerate(NSD.READS[model]):
        out[:, :, j] = (Xcl[:, 1 + 2 * c] - Xcl[:, 2 + 2 * c]) / (theta[1 + 2 * c, j] - theta[2 + 2 * c, j])
    return out


def sens_rel(a, ref, model):
    """the worst over the scalars read of |a - ref|_max / |ref|_max of a column [N, n]"""
    worst = 0.0
    for j in NSD.READS[model]:
        nrm = np.abs(ref[:, :, j]).max()
        worst = max(worst, float(np.abs(a[:, :, j] - ref[:, :, j]).max() / nrm))
    return worst


@functools.lru_cache(maxsize=None)
def consistent_reference(model, N, mode):
    """per problem: (AB, K, Cd, Sth, the restatement's result with S0 = 0, no noise, no bounds, the default Stheta)"""
    X, U, tf = consistent_inputs(model, N, mode)
    Q, R, Qf = LC.WEIGHTS
    n, m = NP.MODELS[model].n, NP.MODELS[model].m
    Sth = NP.default_Sth(model, PLANT_REL)
    out = []
    for b in range(B):
        AB, K, _ = T.tvlqr(model, X[b], U[b], tf[b], Q, R, Qf, **LC.MODES[mode])
        Cd = NP.sensitivities(model, X[b], U[b], tf[b], **LC.MODES[mode])
        r = NP.lincov_plant(model, X[b], U[b], AB, K, Cd, np.zeros((n + m, n + m)), None, plant_rel=PLANT_REL)
        out.append((AB, K, Cd, Sth, r))
    return out
