"""Non-default robot and model scalars, one table for the CPU proofs (tests/test_params_cpu.py) and the GPU tests
(tests/test_gpu_params.py).  With the default, isotropic inertia w x Jw and the six w-w entries of the Jacobian are zero in every
other test of the suite; here they are not.

  aniso        AstrobeeSE3, AstrobeeSE3Manifold: Jdiag = (0.08, 0.11, 0.15), mass 9.3, radius + 3 %, clearance - 5 %
  aniso_tight  aniso with hard_limit_accel and hard_limit_alpha below the peaks of the problem's aniso run (TIGHT, one pair per
               problem: a pair that binds on one problem leaves the other infeasible or untouched): both hard rows bind.  The
               manifold model runs it on a turn of 150 degrees in tf = 7 (tight_problem): on the config problems its angular
               rows carry multipliers of 1e-5 and the interior point method leaves them 1e-5 inside
  freeflyer    freeflyerSE2: Jdiag = (9.0, 7.0, 0.25) -- only [2] may be read --, mass 11.5, radius 0.17, clearance 0.04
  dubins       dubins_car: v = 1.3, k = 0.7, u_max = 4

The linearisation points are trips of oracle runs under the case's parameters -- the second, the middle and the last: from the
straight line, rest to rest, w = 0 and the gyroscopic entries vanish.  tests/test_params_cpu.py proves on the CPU, for exactly the
points listed here, that the certificate accepts the oracle's optimum and rejects the corrupted models."""
import functools

import numpy as np

import gusto_oracle as go
import test_kkt_certificate as T

FF, DUB, SE3, MAN = go.FREEFLYER_SE2, go.DUBINS_CAR, go.ASTROBEE_SE3, go.ASTROBEE_SE3_MANIFOLD
JDIAG = (0.08, 0.11, 0.15)
# the six gyroscopic entries of A as (row, column) offsets inside the w-w block
GYRO = [(0, 1), (0, 2), (1, 0), (1, 2), (2, 0), (2, 1)]
W0 = {SE3: 9, MAN: 10}                     # where w starts in the state


def params(case, model, b=None):
    """the oracle binding's ModelParams of `case` for `model` (T.as_params turns it into the library's); aniso_tight: of problem b"""
    mp = go.default_params(model)[1]
    if case == "default":
        return mp
    if model in (SE3, MAN):
        assert case in ("aniso", "aniso_tight")
        mp.Jdiag[0], mp.Jdiag[1], mp.Jdiag[2] = JDIAG
        mp.mass = 9.3
        mp.radius *= 1.03
        mp.clearance *= 0.95
        if case == "aniso_tight":
            mp.hard_limit_accel, mp.hard_limit_alpha = TIGHT[model][b]
    elif model == FF:
        assert case == "freeflyer"
        mp.Jdiag[0], mp.Jdiag[1], mp.Jdiag[2] = 9.0, 7.0, 0.25
        mp.mass, mp.radius, mp.clearance = 11.5, 0.17, 0.04
    else:
        assert case == "dubins"
        mp.dubins_v, mp.dubins_k, mp.u_max, mp.u_min = 1.3, 0.7, 4.0, -4.0
    return mp


# (hard_limit_accel, hard_limit_alpha) of aniso_tight per problem, from the peaks |F| / mass and |(M_j / J_j)_j| of the oracle's
# aniso run of that problem at N = 16 (astrobeeSE3 problem 1: 0.01729, 0.01879; 2: 0.00876, 0.01477; manifold 1: 0.06914, 0.04429;
# 2: 0.03503, 0.07403).  astrobeeSE3: 0.6 x and 0.45 x -- the trapezoid rule leaves u_N free, so less than the 2/3 of a bang-bang
# profile is still feasible.  The manifold model on tight_problem (peaks 0.0423 / 0.0214 and 0.3165): 0.9 x and 0.81 x; at 0.79 x
# its first subproblem is infeasible.
TIGHT = {SE3: {1: (0.01037, 0.00846), 2: (0.00526, 0.00665)}, MAN: {1: (0.0381, 0.2564), 2: (0.0193, 0.2564)}}
TIGHT_TF, TIGHT_Q, TIGHT_SHRINK = 7.0, np.array([0.25, 0.5, 0.6, 0.6]), 0.3

# tf of the Astrobee problems: short enough that w reaches 0.05 .. 0.15 rad/s on all three axes (config 4 runs tf = 70, config 5
# tf = 40, where w stays below 0.02)
TF = {SE3: 20.0, MAN: 10.0}
# problems of the config set (gusto_jl_amd.problems) the cases use
PROBLEMS = {SE3: (1, 2), MAN: (1, 2), FF: (0, 1), DUB: (0, 3)}     # (dubins 1, 4, 7, 8: infeasible with u_max = 4 at N = 30)
CASES = {"aniso": (SE3, MAN), "aniso_tight": (SE3, MAN), "freeflyer": (FF,), "dubins": (DUB,)}
# the horizons the GPU tests run: one wave and the chain kernels at 16, the first multi-wave horizon 65; freeflyerSE2's
# one-wave kernel (factor_sweep_pg2, the DPP vector sweeps) at 5 and 50
HORIZONS = {SE3: (16, 65), MAN: (16, 65), FF: (5, 50), DUB: (30,)}
# gates that were measured, not reused (the way tests/test_gpu_horizons.py treats freeflyerSE2 at N = 3): none
GATES = {}
RAISE = (1.0, 10.0)                         # every point at the oracle's omega and at omega x 10


def batch(model, B, first=0):
    """the config set of the model at the cases' tf"""
    P = T.P
    if model == SE3:
        return P.astrobee_se3_batch(B, first, tf=TF[SE3])
    if model == MAN:
        return P.astrobee_manifold_batch(B, first, tf=TF[MAN])
    x0, glo, ghi, tf = T.batch(model, B, first)
    if model == FF:             # config 2 starts at theta = 0 at rest and ends there: no moment, no J.  Turn the starts
        x0 = x0.copy()
        x0[:, 2] = 0.9 - 0.5 * np.arange(B)
        x0[:, 5] = 0.04
    return x0, glo, ghi, tf


def tight_problem(x0, glo, ghi):
    """the manifold model's aniso_tight problem from a config problem: 0.3 of the way, a goal attitude 150 degrees from the start,
    tf = 7 -- the rotational cost, and with it the multipliers of the angular rows, is 30 times that of the config problem"""
    glo, ghi = glo.copy(), ghi.copy()
    glo[:3] = ghi[:3] = x0[:3] + TIGHT_SHRINK * (glo[:3] - x0[:3])
    q = TIGHT_Q / np.linalg.norm(TIGHT_Q)
    glo[6:10], ghi[6:10] = q - 1e-4, q + 1e-4
    return x0, glo, ghi, TIGHT_TF


def problem(model, b, case=None):
    x0, glo, ghi, tf = batch(model, b + 1)
    if case == "aniso_tight" and model == MAN:
        return tight_problem(x0[b], glo[b], ghi[b])
    return x0[b], glo[b], ghi[b], tf[b]


@functools.lru_cache(maxsize=None)
def trips(case, model, N, b):
    """[(Xp, Up, Delta, omega)]: the second, middle and last trip of the oracle's run of problem b under the case's parameters"""
    boxes, spheres = T.env(model)
    o = go.Oracle(model, N, boxes=boxes, spheres=spheres, model_params=params(case, model, b))
    o.set_trace(40)
    o.set_problem(*problem(model, b, case))
    r = o.solve(30)
    tr = o.trace()
    n = len(tr)
    assert n >= 2, (case, model, N, b, n)
    return [(tr[t]["Xp"], tr[t]["Up"], float(r["Delta"][t]), float(r["omega"][t])) for t in sorted({1, n // 2, n - 1})]


def groups(case, model, N):
    """[(ModelParams, problems)]: the problems that run under one set of parameters (one handle on the device).  At N = 65, where
    a certificate costs a second on the host, the first problem only."""
    bs = PROBLEMS[model][:1] if N > 50 else PROBLEMS[model]
    if case == "aniso_tight":
        return [(params(case, model, b), (b,)) for b in bs]
    return [(params(case, model), bs)]


def points(case, model, N):
    """every linearisation point of (case, model, N): (ModelParams, prob, Xp, Up, Delta, omega, toggle)"""
    return [(mp, problem(model, b, case), Xp, Up, D, om, D / 8 + mp.clearance)
            for mp, bs in groups(case, model, N) for b in bs for Xp, Up, D, om in trips(case, model, N, b)]


def trip_batches(case, model, N, raise_omega=(1.0,)):
    """points() as the arrays test_gpu_kkt._certify takes, one batch per group: [(ModelParams, prob, Xp, Up, Delta, omega, toggle)],
    every point once per entry of raise_omega (omega times that)"""
    out = []
    for mp, bs in groups(case, model, N):
        pts = [(problem(model, b, case),) + t for b in bs for t in trips(case, model, N, b)]
        pts = [(p, ro) for ro in raise_omega for p in pts]
        prob = tuple(np.stack([np.asarray(p[0][i], float) for p, _ in pts]) for i in range(4))
        D = np.array([p[3] for p, _ in pts])
        out.append((mp, prob, np.stack([p[1] for p, _ in pts]), np.stack([p[2] for p, _ in pts]), D,
                    np.array([ro * p[4] for p, ro in pts]), D / 8 + mp.clearance))
    return out


# ---- post-solve chain ------------------------------------------------------------------------------------------------------
def post_traj(model, B, N, seed=0):
    """np_tvlqr.smooth_batch with the angular rates rescaled so that |w| reaches half of hard_limit_omega on every axis"""
    import np_tvlqr
    X, U = np_tvlqr.smooth_batch(model, B, N, seed)
    w0 = W0[model]
    w = X[..., w0:w0 + 3]
    X[..., w0:w0 + 3] = w * (0.5 * params("aniso", model).hard_limit_omega / np.abs(w).max(axis=1, keepdims=True))
    return np.ascontiguousarray(X), U
