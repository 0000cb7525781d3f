"""Numpy restatement of gusto_lincov_dense, written from the definitions of include/gusto_hip.h and from nothing in csrc/: the
nominal points xbar_{k,i} inside every hold interval (i RK4 substeps from the knot, every interval restarted at its knot), the
sensitivities Phi, Gamma, C of the map after i substeps with respect to the knot's state, the held control and the plant scalars,
the position covariance Spos_{k,i} = Gp S_k Gp' + Gammap diag(sw2) Gammap' with G = [Phi - Gamma K | Gamma | C], and
np_lincov's pair margins at every dense sample j = k Nstep + i (k 0-based here), knot N last.

Phi, Gamma and C come from np_simulate_disturbed.rk4_step by COMPLEX STEP (h = 1e-30), all (N - 1)(n + m + reads) perturbed
roll-outs of a trajectory side by side as columns; the nominal points from the same step in real arithmetic.  S_k and sw2 are
INPUTS: the knot pass is np_lincov_plant.lincov_plant, whose result is passed in.  Works in the dtype passed in."""
import numpy as np

import np_lincov as NL
import np_lincov_plant as NP
import np_simulate as NS
import np_simulate_disturbed as NSD
import np_verify as V

NPLANT = NP.NPLANT
MODELS = NL.MODELS
H_CS = 1e-30


def interval_maps(model_id, X, U, tf, dt_min=0.1, nstep=0, dtype=np.float64, theta_nom=None):
    """(ns, xbar [N-1, ns+1, n], Phi [N-1, ns+1, n, n], Gamma [N-1, ns+1, n, m], C [N-1, ns+1, n, 6]) of one trajectory X [N, n],
    U [N, m]: entry i is the state after i substeps from knot k and its derivatives; i = ns is the image of the whole interval"""
    model = MODELS[model_id]
    n, m = model.n, model.m
    N = len(X)
    ctype = np.complex128 if dtype == np.float64 else np.clongdouble
    th0 = (NSD.nominal(model_id) if theta_nom is None else np.asarray(theta_nom, float)).astype(dtype)
    ns = NS.n_substeps(tf, N, dt_min, nstep)
    h = dtype(tf) / dtype(N - 1) / dtype(ns)
    reads = list(NSD.READS[model_id])
    nc = n + m + len(reads)
    xr = np.asarray(X[:N - 1], float).astype(dtype).T                       # [n, N-1]
    ur = np.asarray(U[:N - 1], float).astype(dtype).T
    thr = np.repeat(th0[:, None], N - 1, axis=1)
    x = np.repeat(xr, nc, axis=1).astype(ctype)                             # column k nc + j
    u = np.repeat(ur, nc, axis=1).astype(ctype)
    th = np.repeat(thr, nc, axis=1).astype(ctype)
    cols = np.arange((N - 1) * nc)
    j = cols % nc
    step = ctype(1j * H_CS)
    x[j[j < n], cols[j < n]] += step
    cu = (j >= n) & (j < n + m)
    u[j[cu] - n, cols[cu]] += step
    ct = j >= n + m
    th[np.array(reads)[j[ct] - n - m], cols[ct]] += step
    xbar = np.zeros((N - 1, ns + 1, n), dtype=dtype)
    Phi = np.zeros((N - 1, ns + 1, n, n), dtype=dtype)
    Gam = np.zeros((N - 1, ns + 1, n, m), dtype=dtype)
    C = np.zeros((N - 1, ns + 1, n, NPLANT), dtype=dtype)
    for i in range(ns + 1):
        D = (x.imag / dtype(H_CS)).reshape(n, N - 1, nc).transpose(1, 0, 2)  # [N-1, n, nc]
        xbar[:, i] = xr.T
        Phi[:, i], Gam[:, i] = D[:, :, :n], D[:, :, n:n + m]
        C[:, i][:, :, reads] = D[:, :, n + m:]
        if i < ns:
            x = NSD.rk4_step(model_id, x, u, h, th)
            xr = NSD.rk4_step(model_id, xr, ur, h, thr)
    return ns, xbar, Phi, Gam, C


def closed_loop_map(Phi, Gam, C, K):
    """G = [Phi - Gamma K | Gamma | C] of one sample"""
    return np.hstack([Phi - Gam @ K, Gam, C])


def position_covariance(G, S, sw2, n, m, ws):
    """Spos = Gp S Gp' + Gammap diag(sw2) Gammap' on the upper triangle, mirrored"""
    Gp, Gm = G[:ws], G[:ws, n:n + m]
    Mx = Gp @ S @ Gp.T + (Gm * sw2) @ Gm.T
    return np.triu(Mx) + np.triu(Mx, 1).T


def lincov_dense(model_id, X, U, K, knot, tf, du_white=0.0, dw=0.0, boxes=None, spheres=None, dt_min=0.1, nstep=0,
                 dtype=np.float64, theta_nom=None):
    """One problem: X [N, n], U [N, m], K [N-1, m, n]; knot: the result of np_lincov_plant.lincov_plant on the same arguments (its
    S [N, NZ, NZ], status and fail_knot are read).  Returns nfull, z_dense, pair_dense [nfull], Spos [nfull, ws, ws], min_z_dense,
    dense_sample, dense_pair, and for the conditioning checks xbar [nfull, n] and z_pairs / d_pairs / sd_pairs (lists per sample;
    None in the rows a failure leaves zero)."""
    model, ws = MODELS[model_id], V.WS_DIM[model_id]
    n, m = model.n, model.m
    N = len(X)
    boxes, spheres = V.obstacles(boxes, spheres)
    if model_id == 1:
        boxes, spheres = V.obstacles(None, None)
    Kd = np.asarray(K, float).astype(dtype)
    w2 = np.broadcast_to(np.asarray(du_white, float), (m,)).astype(dtype) ** 2
    hw = np.broadcast_to(np.asarray(dw, float), (m,)).astype(dtype)
    w2 = w2 + hw * hw / dtype(3.0)
    ns, xbar, Phi, Gam, C = interval_maps(model_id, X, U, tf, dt_min, nstep, dtype, theta_nom)
    nfull = ns * (N - 1) + 1
    S = np.asarray(knot["S"]).astype(dtype)
    fail = knot["fail_knot"] if knot["status"] == 0 else 0
    live_to = nfull if not fail else (fail - 1) * ns          # the samples before it are covered
    out = dict(nfull=nfull, z_dense=np.zeros(nfull, dtype=dtype), pair_dense=np.zeros(nfull, dtype=np.int64),
               Spos=np.zeros((nfull, ws, ws), dtype=dtype), xbar=np.zeros((nfull, n), dtype=dtype),
               z_pairs=[None] * nfull, d_pairs=[None] * nfull, sd_pairs=[None] * nfull)
    best, at, pair = np.inf, -1, -1
    with np.errstate(all="ignore"):
        for j in range(live_to):
            k, i = (N - 1, 0) if j == nfull - 1 else divmod(j, ns)
            if i == 0:
                x, Sp = np.asarray(X[k], float).astype(dtype), S[k][:ws, :ws]
            else:
                x = xbar[k, i]
                Sp = position_covariance(closed_loop_map(Phi[k, i], Gam[k, i], C[k, i], Kd[k]), S[k], w2, n, m, ws)
            zp, dp, sp = NL.pair_margins(model_id, x, Sp, boxes, spheres, dtype)
            zj, pj = NL._first_min(zp)
            out["z_dense"][j], out["pair_dense"][j], out["Spos"][j], out["xbar"][j] = zj, pj, Sp, x
            out["z_pairs"][j], out["d_pairs"][j], out["sd_pairs"][j] = zp, dp, sp
            if zj < best:
                best, at, pair = zj, j, pj
    out.update(min_z_dense=best, dense_sample=at, dense_pair=pair if at >= 0 else -1)
    return out
