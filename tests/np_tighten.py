"""Numpy restatement of gusto_tighten_env, written from the definitions of include/gusto_hip.h and from nothing in csrc/: the
margins m_i of the base keep-out components from the pair margins of np_lincov (distance, normal and sigma_d as gusto_lincov
defines them), cover over the robot's component offsets (np_verify.COMPONENTS), grow, the report with gusto_lincov's tie rules
on the base set, `blocked`, and the skipped-problem rule.  One problem at a time; Sxx is an INPUT (np_lincov makes it, or the
device does).  Works in the dtype passed in (float64 or np.longdouble)."""
import numpy as np

import np_lincov as NL
import np_models as M
import np_verify as V

DEFAULTS = dict(kappa=3.0, slack=0.0, margin_cap=np.inf, reach=np.inf, cover_components=1, monotone=1)


def cover_offsets(model_id, cover=1, dtype=np.float64):
    """(omax, omin) [WS]: the largest and smallest component offset relative to component 0; zeros with cover off"""
    ws = V.WS_DIM[model_id]
    comps = V.COMPONENTS[model_id].astype(dtype)
    omax, omin = np.zeros(ws, dtype=dtype), np.zeros(ws, dtype=dtype)
    if cover:
        for c in range(1, len(comps)):
            o = comps[c] - comps[0]
            omax, omin = np.maximum(omax, o), np.minimum(omin, o)
    return omax, omin


def tightened(model_id, boxes, spheres, margins, cover=1, dtype=np.float64):
    """the tables of one problem: cover, then grow by margins [n_box + n_sph]; coordinates past WS are copied"""
    ws = V.WS_DIM[model_id]
    boxes, spheres = V.obstacles(boxes, spheres)
    bo, so = boxes.astype(dtype), spheres.astype(dtype)
    omax, omin = cover_offsets(model_id, cover, dtype)
    m = np.asarray(margins).astype(dtype)
    for i in range(len(bo)):
        bo[i, :ws] = (bo[i, :ws] - omax) - m[i]
        bo[i, 3:3 + ws] = (bo[i, 3:3 + ws] - omin) + m[i]
    half = dtype(0.5) * (omax - omin)
    for i in range(len(so)):
        so[i, :ws] = so[i, :ws] - dtype(0.5) * (omax + omin)
        so[i, 3] = (so[i, 3] + np.sqrt(np.sum(half * half))) + m[len(bo) + i]
    return bo, so


def distance0(model_id, q, boxes, spheres, dtype=np.float64):
    """signed distances [n_obs] of robot component 0 at the workspace location q"""
    model = V.MODELS[model_id]
    q = np.asarray(q).astype(dtype) + V.COMPONENTS[model_id][0].astype(dtype)
    out = [M.sd_box(q, b[0:3], b[3:6], model.r)[0] for b in boxes] + [M.sd_sphere(q, s[0:3], s[3], model.r)[0] for s in spheres]
    return np.array(out, dtype=dtype)


def tighten(model_id, X, Sxx, boxes, spheres, x_init, goal_lo, goal_hi, prev=None, skipped=False, dtype=np.float64, **opts):
    """One problem: X [N, n], Sxx [N, n, n], the base tables, prev the previous margins [n_obs] or None (zeros).  Returns the
    fields of gusto_tighten_report for the problem (margin [n_obs]), the tightened tables (boxes, spheres), and for the
    conditioning checks of the tests z_pairs / d_pairs / sd_pairs per knot and m_raw, the margins before cap and monotone."""
    o = dict(DEFAULTS, **opts)
    ws = V.WS_DIM[model_id]
    boxes, spheres = V.obstacles(boxes, spheres)
    bo, so = boxes.astype(dtype), spheres.astype(dtype)
    n_obs = len(bo) + len(so)
    kappa, slack, cap, reach = dtype(o["kappa"]), dtype(o["slack"]), dtype(o["margin_cap"]), dtype(o["reach"])
    prev = np.zeros(n_obs, dtype=dtype) if prev is None else np.asarray(prev).astype(dtype)
    out = dict(status=0 if skipped else 1, min_z_base=0.0, knot=0, pair=0, z_pairs=[], d_pairs=[], sd_pairs=[])
    m_raw = np.zeros(n_obs, dtype=dtype)
    if skipped:
        m = prev.copy()
    else:
        zo, zo_knot, zo_pair = np.inf, 0, -1
        with np.errstate(all="ignore"):
            for k in range(len(X)):
                zp, dp, sp = NL.pair_margins(model_id, np.asarray(X[k]).astype(dtype), np.asarray(Sxx[k]).astype(dtype), bo, so, dtype)
                out["z_pairs"].append(zp); out["d_pairs"].append(dp); out["sd_pairs"].append(sp)
                zk, pk = NL._first_min(zp)
                if zk < zo:
                    zo, zo_knot, zo_pair = zk, k + 1, pk
                for p in range(len(zp)):
                    ks = kappa * sp[p]
                    if dp[p] - ks <= reach:
                        v = max(dtype(0), ks - slack) if not np.isnan(ks) else dtype(0)
                        if v > m_raw[p % n_obs]:
                            m_raw[p % n_obs] = v
        m = np.minimum(m_raw, cap)
        if o["monotone"]:
            m = np.maximum(m, prev)
        out.update(min_z_base=zo, knot=zo_knot, pair=zo_pair if zo_knot else -1)
    tb, ts = tightened(model_id, bo, so, m, o["cover_components"], dtype)
    blocked = bool(n_obs) and bool((distance0(model_id, np.asarray(x_init)[:ws], tb, ts, dtype) < 0).any())
    lo, hi = np.asarray(goal_lo, float)[:ws], np.asarray(goal_hi, float)[:ws]
    if n_obs and np.isfinite(lo).all() and np.isfinite(hi).all():
        blocked = blocked or bool((distance0(model_id, dtype(0.5) * (lo.astype(dtype) + hi.astype(dtype)), tb, ts, dtype) < 0).any())
    out.update(margin=m, m_raw=m_raw, max_margin=m.max() if n_obs else dtype(0), n_grown=int((m > 0).sum()), blocked=int(blocked),
               boxes=tb, spheres=ts)
    return out
