"""A numpy restatement of the roadmap seeds (include/gusto_hip.h, "Roadmap seeds"): blocking sets, nodes, dead flags, visibility,
Dijkstra with its tie rules, the ban rule of the alternates, the arc-length seed and the report -- for one query.

The geometric decisions are made with other formulas than the device's (the smallest L-infinity signed distance along a segment
instead of slabs, the point-to-segment distance for a ball), so that `decision_margin` comes out of the same numbers: the
smallest distance from a boundary of anything that decided a dead flag or a visibility, and the gap between the shortest and
the next-shortest route of every PATH alternate.  Inputs with a margin of 1e-9 or more have one answer in any arithmetic."""
import itertools

import numpy as np

DIRECT, PATH, END_BLOCKED, NO_PATH, TOO_LONG, STRAIGHT = 0, 1, 2, 3, 4, 5
MAX_VIA, MAX_K = 16, 8
_ENV_CACHE = {}
FAR = 0.25   # clearances above this are reported as a lower bound (_box_clearance)


def goal_centre(lo, hi):
    fin = np.isfinite(lo) & np.isfinite(hi)
    return np.where(fin, 0.5 * (np.where(fin, lo, 0.0) + np.where(fin, hi, 0.0)), 0.0)


def straight_line(x_init, lo, hi, N):
    """[N, n]: the expression of init_traj_straightline"""
    xg = goal_centre(lo, hi)
    t = np.arange(N) / (N - 1)
    return (1 - t)[:, None] * x_init[None, :] + t[:, None] * xg[None, :]


def blocking_sets(boxes, spheres, WS, inflate):
    boxes, spheres = np.asarray(boxes, float).reshape(-1, 6), np.asarray(spheres, float).reshape(-1, 4)
    return boxes[:, :WS] - inflate, boxes[:, 3:3 + WS] + inflate, spheres[:, :WS].copy(), spheres[:, 3] + inflate


def env_nodes(blo, bhi, sc, sR, WS, pad):
    """[2^WS C, WS]: corner c of component i at row 2^WS i + c, bit j of c the low or the high side"""
    out = []
    for i in range(len(blo)):
        for c in range(1 << WS):
            out.append([(bhi[i, j] + pad) if (c >> j) & 1 else (blo[i, j] - pad) for j in range(WS)])
    for i in range(len(sc)):
        for c in range(1 << WS):
            out.append([sc[i, j] + (sR[i] + pad) if (c >> j) & 1 else sc[i, j] - (sR[i] + pad) for j in range(WS)])
    return np.array(out, float).reshape(-1, WS)


def edge_length(p, q):
    d = q - p
    s2 = d[..., 0] * d[..., 0]
    for j in range(1, d.shape[-1]):
        s2 = s2 + d[..., j] * d[..., j]
    return np.sqrt(s2)


def _box_clearance(lo, hi, p, q):
    """the smallest L-infinity signed distance to the box [lo, hi] along the segments p[i] -> q[i]: negative = it meets the open box"""
    WS = p.shape[1]
    # far segments: the separation of the segment's bounding box from the box bounds the clearance from below, and is exact
    # enough where it exceeds FAR (the margin is a minimum over much smaller numbers)
    sep = np.maximum(lo - np.maximum(p, q), np.minimum(p, q) - hi).max(axis=1)
    if len(p) > 64 and (sep > FAR).any():
        out = sep.copy()
        near = sep <= FAR
        out[near] = _box_clearance(lo, hi, p[near], q[near])
        return out
    mid, half = 0.5 * (lo + hi), 0.5 * (hi - lo)
    a, d = p - mid, q - p
    cands = [np.zeros(len(p)), np.ones(len(p))]
    with np.errstate(divide="ignore", invalid="ignore"):
        for j in range(WS):
            cands.append(-a[:, j] / d[:, j])
        for i, j in itertools.combinations(range(WS), 2):
            for si, sj in itertools.product((1.0, -1.0), repeat=2):
                cands.append((half[i] - half[j] - si * a[:, i] + sj * a[:, j]) / (si * d[:, i] - sj * d[:, j]))
    t = np.clip(np.nan_to_num(np.stack(cands), nan=0.0, posinf=1.0, neginf=0.0), 0.0, 1.0)   # [cand, M]
    s = np.full(t.shape, -np.inf)
    for j in range(WS):
        s = np.maximum(s, np.abs(a[None, :, j] + t * d[None, :, j]) - half[j])
    return s.min(axis=0)


def _ball_clearance(c, R, p, q):
    d = q - p
    dd = (d * d).sum(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.clip(np.nan_to_num(((c - p) * d).sum(axis=1) / dd, nan=0.0, posinf=0.0, neginf=0.0), 0.0, 1.0)
    return np.linalg.norm(p + t[:, None] * d - c, axis=1) - R


def clearance(sets, p, q):
    """[M]: the smallest clearance of the segments p[i] -> q[i] (points: p == q) over all blocking sets; +inf without sets"""
    blo, bhi, sc, sR = sets
    out = np.full(len(p), np.inf)
    for i in range(len(blo)):
        out = np.minimum(out, _box_clearance(blo[i], bhi[i], p, q))
    for i in range(len(sc)):
        out = np.minimum(out, _ball_clearance(sc[i], sR[i], p, q))
    return out


def build_graph(boxes, spheres, WS, inflate, pad, p0, pg):
    """nodes [V, WS] (0 the start, 1 the goal, then the corners), dead [V], vis [V, V] among the live nodes, and the margin"""
    sets = blocking_sets(boxes, spheres, WS, inflate)
    key = (np.asarray(boxes, float).tobytes(), np.asarray(spheres, float).tobytes(), WS, inflate, pad)
    if key not in _ENV_CACHE:   # the part that belongs to the keep-out set alone
        E = env_nodes(*sets, WS, pad)
        ce = clearance(sets, E, E)
        de = ce < 0
        me = np.abs(ce).min() if len(E) else np.inf
        ve = np.zeros((len(E), len(E)), bool)
        live = np.flatnonzero(~de)
        iu, iv = np.triu_indices(len(live), 1)
        if len(iu):
            cs = clearance(sets, E[live[iu]], E[live[iv]])
            ve[live[iu], live[iv]] = ve[live[iv], live[iu]] = cs >= 0
            me = min(me, np.abs(cs).min())
        _ENV_CACHE[key] = (E, de, ve, float(me))
    E, de, ve, margin = _ENV_CACHE[key]
    P = np.vstack([p0[None, :WS], pg[None, :WS], E])
    V = len(P)
    ends = P[:2]
    cp = clearance(sets, ends, ends)
    dead = np.concatenate([cp < 0, de])
    margin = min(margin, np.abs(cp).min())
    vis = np.zeros((V, V), bool)
    vis[2:, 2:] = ve
    for a in (0, 1):   # the start and the goal against every live node behind them
        if dead[a]:
            continue
        others = np.flatnonzero(~dead[a + 1:]) + a + 1
        if len(others):
            cs = clearance(sets, np.repeat(P[a][None], len(others), axis=0), P[others])
            vis[a, others] = vis[others, a] = cs >= 0
            margin = min(margin, np.abs(cs).min())
    return P, dead, vis, float(margin)


def dijkstra(P, alive, vis, src, stop=None):
    """distances and predecessors from src: the unsettled node of smallest distance next, ties to the lowest index; a
    predecessor changes on a strict < only; stops once `stop` is settled"""
    V = len(P)
    dist, pred, settled = np.full(V, np.inf), np.full(V, -1), np.zeros(V, bool)
    dist[src] = 0.0
    for _ in range(V):
        key = np.where(alive & ~settled, dist, np.inf)
        s = int(np.argmin(key))   # (the first of equal minima)
        if not key[s] < np.inf:
            break
        settled[s] = True
        if s == stop:
            break
        nd = dist[s] + edge_length(P[s][None, :], P)
        upd = vis[s] & alive & ~settled & (nd < dist)
        dist[upd], pred[upd] = nd[upd], s
    return dist, pred, settled


def resample(pts, Lp, N):
    """[N, WS]: the point at arc length t_k Lp on the polyline (rows 0 and N - 1 are not used by the seed)"""
    out = np.zeros((N, pts.shape[1]))
    nseg = len(pts) - 1
    for k in range(N):
        s = (k / (N - 1)) * Lp
        cum, i = 0.0, 0
        ln = edge_length(pts[0], pts[1])
        while i < nseg - 1 and s >= cum + ln:
            cum += ln
            i += 1
            ln = edge_length(pts[i], pts[i + 1])
        f = (s - cum) / ln if ln > 0.0 else 0.0
        out[k] = pts[i] + f * (pts[i + 1] - pts[i])
    return out


def roadmap_query(x_init, goal_lo, goal_hi, boxes, spheres, WS, N, K=1, inflate=0.0, pad=0.03, straight_first=0):
    """One query with K alternates.  A dict of the report rows over the K problems (status, n_via, via [K, 16], length, banned
    [K, 8]), X0 [K, N, n], the polylines `pts` (a list, None for a straight line) and `decision_margin`."""
    x_init, goal_lo, goal_hi = (np.asarray(a, float) for a in (x_init, goal_lo, goal_hi))
    xg = goal_centre(goal_lo, goal_hi)
    line = straight_line(x_init, goal_lo, goal_hi, N)
    P, dead, vis, margin = build_graph(boxes, spheres, WS, inflate, pad, x_init, xg)
    V = len(P)
    comp_of = (np.arange(V) - 2) >> WS
    rows, ban, failed = [], [], None
    KP = K - straight_first
    for j in range(max(KP, 1)):
        if failed is None:
            row = dict(status=PATH, n_via=0, via=[], length=np.inf, banned=list(ban), pts=None)
            if dead[0] or dead[1]:
                row["status"] = END_BLOCKED
            elif vis[0, 1]:
                row["status"], row["length"] = DIRECT, float(edge_length(P[0], P[1]))
            else:
                alive = ~dead & ~((np.arange(V) >= 2) & np.isin(comp_of, ban))
                dist, pred, settled = dijkstra(P, alive, vis, 0, stop=1)
                if not settled[1]:
                    row["status"] = NO_PATH
                else:
                    via, cur = [], pred[1]
                    while cur > 0:
                        via.append(int(cur))
                        cur = pred[cur]
                    via = via[::-1]
                    # the gap to the next-shortest route: every other route uses an edge that is not on this one
                    d0, _, _ = dijkstra(P, alive, vis, 0)
                    d1, _, _ = dijkstra(P, alive, vis, 1)
                    W = np.where(vis & alive[:, None] & alive[None, :], edge_length(P[:, None, :], P[None, :, :]), np.inf)
                    alt = d0[:, None] + W + d1[None, :]
                    path = [0] + via + [1]
                    alt[path[:-1], path[1:]] = np.inf
                    margin = min(margin, float(alt.min() - dist[1]))
                    if len(via) > MAX_VIA:
                        row["status"] = TOO_LONG
                    else:
                        row.update(n_via=len(via), via=via, length=float(dist[1]), pts=P[path])
            if row["status"] != PATH:
                failed = row
            elif via:
                ban.append(int(comp_of[via[0]]))
        if j < KP:
            rows.append(dict(failed) if failed is not None else row)
        if j == 0 and straight_first:
            first = dict(failed) if failed is not None else dict(status=STRAIGHT, n_via=0, via=[], length=np.inf, banned=[], pts=None)
            rows.insert(0, first)
    out = dict(status=np.array([r["status"] for r in rows], np.int32), n_via=np.array([r["n_via"] for r in rows], np.int32),
               via=np.full((K, MAX_VIA), -1, np.int32), length=np.array([r["length"] for r in rows]),
               banned=np.full((K, MAX_K), -1, np.int32), X0=np.repeat(line[None], K, axis=0), pts=[r["pts"] for r in rows],
               decision_margin=margin)
    for k, r in enumerate(rows):
        out["via"][k, :r["n_via"]] = r["via"][:r["n_via"]]
        out["banned"][k, :len(r["banned"])] = r["banned"]
        if r["status"] == PATH:
            out["X0"][k, 1:N - 1, :WS] = resample(r["pts"], r["length"], N)[1:N - 1]
    return out


def roadmap_batch(x_init, goal_lo, goal_hi, envs, WS, N, K=1, **opts):
    """Bq queries; envs: one (boxes, spheres) for all, or a list of Bq.  The rows concatenated over the Bq K problems, the smallest
    margin, and the per-query results under `queries`"""
    Bq = len(x_init)
    per = [roadmap_query(x_init[q], goal_lo[q], goal_hi[q], *(envs if isinstance(envs, tuple) else envs[q]), WS, N, K, **opts)
           for q in range(Bq)]
    out = {k: np.concatenate([p[k] for p in per]) for k in ("status", "n_via", "via", "length", "banned", "X0")}
    out["decision_margin"] = min(p["decision_margin"] for p in per)
    out["queries"] = per
    return out
