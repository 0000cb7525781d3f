"""Numpy restatement of gusto_lincov_disturbed, written from the definitions of include/gusto_hip.h and from nothing in csrc/:
the sensitivity Cd_k = dF_k/dtheta of the discrete roll-out map with respect to the plant scalars, and np_lincov's recursion on
the deviation augmented by the plant deviation, z = [dx; b; theta~].

Cd comes from np_simulate_disturbed.f_cols by COMPLEX STEP (h = 1e-30) through np_simulate_disturbed.rk4_step: f_cols is
complex-safe in theta for all four models (divisions, products, sin / cos of real states), so no finite difference is needed, in
float64 (complex128) or in np.longdouble (np.clongdouble).  All (N - 1) x 6 perturbed roll-outs of a trajectory run side by side
as columns.  Columns of entries the model does not read (np_simulate_disturbed.READS) are zeros by definition, not by
computation.

The recursion is np_lincov.lincov's with the theta terms added BEHIND the terms it has: every product np_lincov forms is formed
here with the same shapes, so with a zero dispersion every field equals np_lincov's bit for bit.  The margins, summaries and
status rules are np_lincov's functions.  Works in the dtype passed in."""
import math

import numpy as np

import np_lincov as NL
import np_simulate as NS
import np_simulate_disturbed as NSD
import np_verify as V

NPLANT = NSD.NPLANT
READS = NSD.READS
MODELS = NL.MODELS
H_CS = 1e-30


def read_mask(model_id):
    m = np.zeros(NPLANT, bool)
    m[list(READS[model_id])] = True
    return m


def sensitivities(model_id, X, U, tf, dt_min=0.1, nstep=0, dtype=np.float64, theta_nom=None):
    """Cd [N-1, n, 6] of one trajectory X [N, n], U [N, m]: the derivative of the roll-out map of np_tvlqr (ns RK4 steps of
    dt / ns under the held control) with respect to theta at theta_nom, by complex step; zeros in the columns not read"""
    model = MODELS[model_id]
    n = model.n
    N = len(X)
    ctype = np.complex128 if dtype == np.float64 else np.clongdouble
    th0 = NSD.nominal(model_id) if theta_nom is None else np.asarray(theta_nom, float)
    ns = NS.n_substeps(tf, N, dt_min, nstep)
    h = dtype(tf) / dtype(N - 1) / dtype(ns)
    reads = list(READS[model_id])
    nr = len(reads)
    x = np.repeat(np.asarray(X[:N - 1], float).astype(dtype).T, nr, axis=1).astype(ctype)      # column k nr + c
    u = np.repeat(np.asarray(U[:N - 1], float).astype(dtype).T, nr, axis=1).astype(ctype)
    th = np.repeat(th0.astype(dtype)[:, None], (N - 1) * nr, axis=1).astype(ctype)
    cols = np.arange((N - 1) * nr)
    th[np.array(reads)[cols % nr], cols] += ctype(1j * H_CS)
    for _ in range(ns):
        x = NSD.rk4_step(model_id, x, u, h, th)
    D = (x.imag / dtype(H_CS)).reshape(n, N - 1, nr).transpose(1, 0, 2)
    Cd = np.zeros((N - 1, n, NPLANT), dtype=dtype)
    Cd[:, :, reads] = D
    return Cd


def default_Sth(model_id, plant_rel, dtype=np.float64, theta_nom=None):
    """diag((theta_nom_j plant_rel_j)^2 / 3) on the entries the model reads, computed as t = nominal * rel; (t * t) / 3"""
    th0 = (NSD.nominal(model_id) if theta_nom is None else np.asarray(theta_nom, float)).astype(dtype)
    t = th0 * np.broadcast_to(np.asarray(plant_rel, float), (NPLANT,)).astype(dtype)
    return np.diag(np.where(read_mask(model_id), (t * t) / dtype(3.0), dtype(0.0)))


def masked_Sth(model_id, Sth, dtype=np.float64):
    """a supplied Sth with the rows and columns of the entries the model does not read set to zero, whatever they hold"""
    r = read_mask(model_id)
    return np.where(r[:, None] & r[None, :], np.asarray(Sth, float), 0.0).astype(dtype)


def lincov_plant(model_id, X, U, AB, K, Cd, S0=None, Sth=None, dx0=0.01, du0=0.0, du_white=0.0, dw=0.0, plant_rel=0.0, u_lo=None,
                 u_hi=None, boxes=None, spheres=None, dtype=np.float64, theta_nom=None):
    """One problem: np_lincov.lincov's arguments, and Cd [N-1, n, 6], Sth [6, 6] or None (default_Sth(plant_rel)), the half-widths
    dw of the per-interval noise.  Returns np_lincov.lincov's fields -- S is [N, n+m+6, n+m+6] -- and Sxt [N, n, 6]."""
    model = MODELS[model_id]
    n, m = model.n, model.m
    nz = n + m
    NZ = nz + NPLANT
    N = len(X)
    boxes, spheres = V.obstacles(boxes, spheres)
    if model_id == 1:
        boxes, spheres = V.obstacles(None, None)
    Xd, Ud, ABd, Kd, Cdd = (np.asarray(a, float).astype(dtype) for a in (X, U, AB, K, Cd))
    S = np.zeros((NZ, NZ), dtype=dtype)
    S[:nz, :nz] = NL.default_S0(model_id, dx0, du0, dtype) if S0 is None else np.asarray(S0).astype(dtype)
    S[nz:, nz:] = default_Sth(model_id, plant_rel, dtype, theta_nom) if Sth is None else masked_Sth(model_id, Sth, dtype)
    w2 = np.broadcast_to(np.asarray(du_white, float), (m,)).astype(dtype) ** 2
    hw = np.broadcast_to(np.asarray(dw, float), (m,)).astype(dtype)
    w2 = w2 + hw * hw / dtype(3.0)
    lo = np.full(m, -np.inf) if u_lo is None else np.broadcast_to(np.asarray(u_lo, float), (m,))
    hi = np.full(m, np.inf) if u_hi is None else np.broadcast_to(np.asarray(u_hi, float), (m,))
    lo, hi = lo.astype(dtype), hi.astype(dtype)
    out = dict(status=1, fail_knot=0, S=np.zeros((N, NZ, NZ), dtype=dtype), Sxx=np.zeros((N, n, n), dtype=dtype),
               Sxt=np.zeros((N, n, NPLANT), dtype=dtype), sigma_x=np.zeros((N, n), dtype=dtype),
               sigma_u=np.zeros((N - 1, m), dtype=dtype), z_obs=np.zeros(N, dtype=dtype),
               z_ctl=np.full((N - 1, m), np.inf, dtype=dtype), z_pairs=[], d_pairs=[], sd_pairs=[])
    zo, zo_knot, zo_pair, psum = np.inf, 0, -1, 0.0
    zc, zc_knot, zc_entry = np.inf, 0, -1

    def knot_rows(k, S):
        nonlocal zo, zo_knot, zo_pair, psum
        zp, dp, sp = NL.pair_margins(model_id, Xd[k], S[:n, :n], boxes, spheres, dtype)
        zk, pk = NL._first_min(zp)
        out["z_pairs"].append(zp); out["d_pairs"].append(dp); out["sd_pairs"].append(sp)
        out["S"][k] = S
        out["Sxx"][k] = S[:n, :n]
        out["Sxt"][k] = S[:n, nz:]
        out["sigma_x"][k] = NL.sigma_of(np.diag(S)[:n])
        out["z_obs"][k] = zk
        if zk < zo:
            zo, zo_knot, zo_pair = zk, k + 1, pk
        psum += 0.5 * math.erfc(float(zk / np.sqrt(dtype(2.0))))

    with np.errstate(all="ignore"):
        for k in range(N - 1):
            A, Bd, Ck = ABd[k, :, :n], ABd[k, :, n:], Cdd[k]
            G = np.hstack([A - Bd @ Kd[k], Bd])
            C = np.hstack([-Kd[k], np.eye(m, dtype=dtype)])
            Sz, Szt, Stt = S[:nz, :nz], S[:nz, nz:], S[nz:, nz:]
            su = NL.sigma_of(np.diag(C @ Sz @ C.T) + w2)                      # dv = [-K I 0] z + w: theta does not enter
            Tz = G @ Sz + Ck @ Szt.T                                         # the terms of np_lincov first, the theta terms after
            Tt = G @ Szt + Ck @ Stt
            Mx = Tz @ G.T + (Bd * w2) @ Bd.T + Tt @ Ck.T
            Sxx = np.triu(Mx) + np.triu(Mx, 1).T
            Sxr = np.hstack([Tz[:, n:], Tt])                                 # S_{x,[b theta]} of the next knot
            if not (np.isfinite(Sxx).all() and np.isfinite(Sxr).all() and np.isfinite(su).all()):
                out["status"], out["fail_knot"] = 0, k + 1
                break
            knot_rows(k, S)
            out["sigma_u"][k] = su
            room = np.minimum(hi - Ud[k], Ud[k] - lo)
            zck = np.array([NL.margin_z(room[i], su[i]) for i in range(m)], dtype=dtype)
            out["z_ctl"][k] = zck
            v, e = NL._first_min(zck)
            if v < zc:
                zc, zc_knot, zc_entry = v, k + 1, e
            Sn = S.copy()
            Sn[:n, :n], Sn[:n, n:], Sn[n:, :n] = Sxx, Sxr, Sxr.T
            S = Sn
        else:
            knot_rows(N - 1, S)
    out.update(obs_knot=zo_knot, obs_pair=zo_pair if zo_knot else -1, ctl_knot=zc_knot, ctl_entry=zc_entry if zc_knot else -1,
               min_z_obs=zo, p_collision_bound=min(1.0, psum), min_z_ctl=zc)
    return out


def closed_loop_sensitivity(r, Sth):
    """dx_k/dtheta_j [N, n, 6] from the Sxt of a run with S0 = 0 and a DIAGONAL Sth and no noise: column j of Sxt_k / Sth_jj;
    zeros where Sth_jj = 0"""
    d = np.diag(np.asarray(Sth))
    with np.errstate(all="ignore"):
        return np.where(d > 0, r["Sxt"] / np.where(d > 0, d, 1), 0.0)
