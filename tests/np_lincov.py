"""Numpy restatement of gusto_lincov, written from the definitions of include/gusto_hip.h and from nothing in csrc/: the
covariance S_k of the augmented deviation z = [dx; b] carried through G_k = [Ad_k - Bd_k K_k | Bd_k], the standard deviations of
state and commanded control, the obstacle margins d / sqrt(nh' Sxx[0:WS, 0:WS] nh) over the (component, obstacle) pairs in loop
order, the control margins, the per-problem summaries and the status rules.  The discrete Jacobians AB and the gains K are
INPUTS (np_tvlqr makes them, or the device does); the distances and their normals are np_models' sd_box / sd_sphere, the robot
components np_verify.COMPONENTS.  Works in the dtype passed in (float64, or np.longdouble for the error estimates of
tools/lincov_errors.py; erfc is math.erfc, a double, in both)."""
import math

import numpy as np

import np_models as M
import np_verify as V

MODELS = V.MODELS


def default_S0(model_id, dx0, du0, dtype=np.float64):
    """diag(dx0^2 / 3, du0^2 / 3): the variances of gusto_simulate's uniform draws with the same half-widths"""
    model = MODELS[model_id]
    w = np.concatenate([np.broadcast_to(np.asarray(dx0, float), (model.n,)), np.broadcast_to(np.asarray(du0, float), (model.m,))]).astype(dtype)
    return np.diag(w * w / dtype(3.0))


def sigma_of(var):
    """the standard deviation of a variance (an array): what rounding leaves below zero counts as zero, a NaN stays one"""
    var = np.asarray(var)
    return np.sqrt(np.where(var < 0, var.dtype.type(0), var))


def margin_z(d, sigma):
    """a margin in standard deviations; without any deviation its sign decides"""
    if sigma == 0:
        return np.inf if d >= 0 else -np.inf
    return d / sigma


def pair_margins(model_id, x, Sxx, boxes, spheres, dtype=np.float64):
    """(z, d, sigma_d) of every (component, obstacle) pair at state x, ordinal c n_obs + i; empty for the Dubins car"""
    model, ws = MODELS[model_id], V.WS_DIM[model_id]
    comps = V.COMPONENTS[model_id]
    n_obs = len(boxes) + len(spheres)
    z, dd, sg = [], [], []
    Spos = Sxx[:ws, :ws]
    for c in range(len(comps) if model_id != 1 else 0):
        q = np.asarray(x[:ws], dtype=dtype) + comps[c].astype(dtype)
        for i in range(n_obs):
            if i < len(boxes):
                d, nh = M.sd_box(q, boxes[i, 0:3], boxes[i, 3:6], model.r)
            else:
                s = spheres[i - len(boxes)]
                d, nh = M.sd_sphere(q, s[0:3], s[3], model.r)
            nh = np.asarray(nh, dtype=dtype)
            sd = sigma_of(nh @ (Spos @ nh))[()]
            z.append(margin_z(d, sd))
            dd.append(d)
            sg.append(sd)
    return np.array(z, dtype=dtype), np.array(dd, dtype=dtype), np.array(sg, dtype=dtype)


def _first_min(values):
    """(minimum, index of the first entry that holds it) with a strict <: a NaN never wins; (+inf, -1) when nothing is below +inf"""
    best, at = np.inf, -1
    for i, v in enumerate(values):
        if v < best:
            best, at = v, i
    return best, at


def lincov(model_id, X, U, AB, K, S0=None, dx0=0.01, du0=0.0, du_white=0.0, u_lo=None, u_hi=None, boxes=None, spheres=None,
           dtype=np.float64):
    """One problem: X [N, n], U [N, m], AB [N-1, n, n+m], K [N-1, m, n], S0 [n+m, n+m] or None (default_S0(dx0, du0)).
    Returns every field of gusto_lincov_report for the problem (Sxx included), S [N, n+m, n+m], and for the conditioning checks
    of the tests z_pairs (a list of [pairs] arrays per knot, with d_pairs and sd_pairs) and z_ctl [N-1, m]."""
    model = MODELS[model_id]
    n, m = model.n, model.m
    nz = n + m
    N = len(X)
    boxes, spheres = V.obstacles(boxes, spheres)
    if model_id == 1:
        boxes, spheres = V.obstacles(None, None)
    Xd, Ud, ABd, Kd = (np.asarray(a, float).astype(dtype) for a in (X, U, AB, K))
    S = default_S0(model_id, dx0, du0, dtype) if S0 is None else np.asarray(S0).astype(dtype)
    w2 = np.broadcast_to(np.asarray(du_white, float), (m,)).astype(dtype) ** 2
    lo = np.full(m, -np.inf) if u_lo is None else np.broadcast_to(np.asarray(u_lo, float), (m,))
    hi = np.full(m, np.inf) if u_hi is None else np.broadcast_to(np.asarray(u_hi, float), (m,))
    lo, hi = lo.astype(dtype), hi.astype(dtype)
    out = dict(status=1, fail_knot=0, S=np.zeros((N, nz, nz), dtype=dtype), Sxx=np.zeros((N, n, n), dtype=dtype),
               sigma_x=np.zeros((N, n), dtype=dtype), sigma_u=np.zeros((N - 1, m), dtype=dtype), z_obs=np.zeros(N, dtype=dtype),
               z_ctl=np.full((N - 1, m), np.inf, dtype=dtype), z_pairs=[], d_pairs=[], sd_pairs=[])
    zo, zo_knot, zo_pair, psum = np.inf, 0, -1, 0.0
    zc, zc_knot, zc_entry = np.inf, 0, -1

    def knot_rows(k, S):
        nonlocal zo, zo_knot, zo_pair, psum
        zp, dp, sp = pair_margins(model_id, Xd[k], S[:n, :n], boxes, spheres, dtype)
        zk, pk = _first_min(zp)
        out["z_pairs"].append(zp); out["d_pairs"].append(dp); out["sd_pairs"].append(sp)
        out["S"][k] = S
        out["Sxx"][k] = S[:n, :n]
        out["sigma_x"][k] = sigma_of(np.diag(S)[:n])
        out["z_obs"][k] = zk
        if zk < zo:
            zo, zo_knot, zo_pair = zk, k + 1, pk
        psum += 0.5 * math.erfc(float(zk / np.sqrt(dtype(2.0))))

    with np.errstate(all="ignore"):
        for k in range(N - 1):
            A, Bd = ABd[k, :, :n], ABd[k, :, n:]
            G = np.hstack([A - Bd @ Kd[k], Bd])
            C = np.hstack([-Kd[k], np.eye(m, dtype=dtype)])
            su = sigma_of(np.diag(C @ S @ C.T) + w2)
            Tm = G @ S
            Mx = Tm @ G.T + (Bd * w2) @ Bd.T
            Sxx = np.triu(Mx) + np.triu(Mx, 1).T
            Sxb = Tm[:, n:]
            if not (np.isfinite(Sxx).all() and np.isfinite(Sxb).all() and np.isfinite(su).all()):
                out["status"], out["fail_knot"] = 0, k + 1
                break
            knot_rows(k, S)
            out["sigma_u"][k] = su
            room = np.minimum(hi - Ud[k], Ud[k] - lo)
            zck = np.array([margin_z(room[i], su[i]) for i in range(m)], dtype=dtype)
            out["z_ctl"][k] = zck
            v, e = _first_min(zck)
            if v < zc:
                zc, zc_knot, zc_entry = v, k + 1, e
            Sn = S.copy()
            Sn[:n, :n], Sn[:n, n:], Sn[n:, :n] = Sxx, Sxb, Sxb.T
            S = Sn
        else:
            knot_rows(N - 1, S)
    out.update(obs_knot=zo_knot, obs_pair=zo_pair if zo_knot else -1, ctl_knot=zc_knot, ctl_entry=zc_entry if zc_knot else -1,
               min_z_obs=zo, p_collision_bound=min(1.0, psum), min_z_ctl=zc)
    return out
