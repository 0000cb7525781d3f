"""numpy restatement of the fleet stage (csrc/fleet.hip), written from the definitions in include/gusto_hip.h: the track on the
fleet clock, the departure schedule and the separation report.  Vectorised over the clock samples with the same elementwise
operations in the same order, so the roundings are the device's: tracks, delays and every integer are compared bit for bit."""
import numpy as np

NO_PLAN, SCHEDULED, BLOCKED = 0, 1, 2


def clock_samples(tf, h):
    """J_b = (int)ceil(tf / h) + 1"""
    return int(np.ceil(np.float64(tf) / np.float64(h))) + 1


def track(P, tf, h):
    """Q [J, WS] of the dense positions P [nfull, WS] flown in tf: (1 - w) P_i + w P_{i+1}, the last sample P's last exactly;
    fewer than two dense samples: NaN"""
    P = np.asarray(P, np.float64)
    J = clock_samples(tf, h)
    if len(P) < 2:
        return np.full((J, P.shape[1]), np.nan)
    nf = len(P)
    hb = np.float64(tf) / np.float64(nf - 1)
    tau = np.arange(J - 1, dtype=np.float64) * np.float64(h)
    s = tau / hb
    i = np.minimum(np.floor(s).astype(np.int64), nf - 2)
    w = s - i.astype(np.float64)
    w1 = 1.0 - w
    Q = np.empty((J, P.shape[1]))
    Q[:J - 1] = (w1[:, None] * P[i]) + (w[:, None] * P[i + 1])
    Q[J - 1] = P[nf - 1]
    return Q


def tracks_of_dense(nfull, Xfull, tf, h, ws):
    """the tracks of a handle's dense samples (gusto_get_dense): a list of Q_b"""
    return [track(Xfull[b, :max(int(nfull[b]), 0), :ws], tf[b], h) for b in range(len(tf))]


def pairs_of(comp_off, n_comp, ws, components=1):
    """comp_off[ca] - comp_off[cb] over the component pairs, ca outer and cb inner; components = 0: pair (0, 0) only"""
    nc = max(1, min(int(n_comp), 2)) if components else 1
    off = np.asarray(comp_off, np.float64)
    return np.array([[off[ca][x] - off[cb][x] for x in range(ws)] for ca in range(nc) for cb in range(nc)])


def positions(Q, sigma, jend):
    """p(j; sigma) for j = 0 .. jend"""
    j = np.arange(jend + 1)
    return Q[0][None, :].repeat(jend + 1, 0) if sigma < 0 else Q[np.clip(j - sigma, 0, len(Q) - 1)]


def end_step(sigma, J):
    return 0 if sigma < 0 else sigma + J - 1


def D2(Qa, sa, Qb, sb, doff):
    """D2(a, b, j) for j = 0 .. max(end_a, end_b): the smallest d2 over the component pairs, fmin from +inf"""
    jend = max(end_step(sa, len(Qa)), end_step(sb, len(Qb)))
    pa, pb = positions(Qa, sa, jend), positions(Qb, sb, jend)
    best = np.full(jend + 1, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in doff:
            d2 = np.zeros(jend + 1)
            for x in range(pa.shape[1]):
                dx = (pa[:, x] - pb[:, x]) + d[x]
                d2 = d2 + dx * dx
            best = np.fmin(best, d2)
    return best


def schedule(Q, R, eligible, doff, radius, margin, n_delays=64, stride=10, order=None):
    """the departure schedule of the fleets of R consecutive tracks: status, delay_steps, blocker [B]"""
    B = len(Q)
    thr = 2 * radius + margin
    thr2 = thr * thr
    status, sigma, blocker = np.zeros(B, np.int32), np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    for f in range(B // R):
        od = np.arange(R) if order is None else np.asarray(order).reshape(-1, R)[f]
        placed = []
        for i in od:
            bi = f * R + int(i)
            ok = bool(eligible[bi]) and bool(np.all(np.isfinite(Q[bi])))
            if ok:
                status[bi] = BLOCKED
                for d in range(n_delays):
                    first = next((k for k in placed if np.any(D2(Q[bi], d * stride, Q[f * R + k], int(sigma[f * R + k]), doff) < thr2)), None)
                    if d == 0 and first is not None:
                        blocker[bi] = first
                    if first is None:
                        status[bi], sigma[bi] = SCHEDULED, d * stride
                        break
            placed.append(int(i))
    return status, sigma, blocker


def separation(Q, R, sigma, status, doff, radius, margin):
    """the separation report of the shifts sigma [B] as a dict of the report's arrays (without status, delay_steps, blocker)"""
    B, F = len(Q), len(Q) // R
    thr = 2 * radius + margin
    thr2 = thr * thr
    ps, pt = np.full((F, R, R), np.inf), np.full((F, R, R), -1, np.int32)
    nconf = np.zeros(F, np.int32)
    for f in range(F):
        for a in range(R):
            for b in range(a + 1, R):
                d = D2(Q[f * R + a], int(sigma[f * R + a]), Q[f * R + b], int(sigma[f * R + b]), doff)
                dmin = np.fmin.reduce(d, initial=np.inf)
                if dmin < np.inf:
                    pt[f, a, b] = pt[f, b, a] = int(np.flatnonzero(d == dmin)[0])
                ps[f, a, b] = ps[f, b, a] = np.sqrt(dmin) - 2 * radius
                nconf[f] += dmin < thr2
    min_sep, partner, step = np.full(B, np.inf), np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    for f in range(F):
        for a in range(R):
            row = ps[f, a]
            if np.any(row < np.inf):
                p = int(np.argmin(row))   # (the first of equal minima)
                min_sep[f * R + a], partner[f * R + a], step[f * R + a] = row[p], p, pt[f, a, p]
    st, sg = np.asarray(status).reshape(F, R), np.asarray(sigma).reshape(F, R)
    J = np.array([len(q) for q in Q]).reshape(F, R)
    span = np.array([max([end_step(int(sg[f, a]), int(J[f, a])) for a in range(R) if st[f, a] == SCHEDULED], default=0) for f in range(F)], np.int32)
    return dict(min_sep=min_sep, partner=partner, step=step, pair_min_sep=ps, pair_step=pt, n_conflicts=nconf,
                fleet_min_sep=np.array([ps[f].min() if R > 1 else np.inf for f in range(F)]), makespan_steps=span,
                n_scheduled=(st == SCHEDULED).sum(1).astype(np.int32), n_blocked=(st == BLOCKED).sum(1).astype(np.int32),
                delay=np.where(np.asarray(sigma) < 0, 0.0, np.asarray(sigma, np.float64)))


def report(Q, R, h, eligible, doff, radius, margin, n_delays=64, stride=10, order=None, delay_steps=None):
    """gusto_fleet_schedule (delay_steps None) or gusto_fleet_separation with a caller's delay_steps: the whole report"""
    if delay_steps is None:
        status, sigma, blocker = schedule(Q, R, eligible, doff, radius, margin, n_delays, stride, order)
    else:
        sigma = np.asarray(delay_steps, np.int32)
        status, blocker = np.where(sigma >= 0, SCHEDULED, NO_PLAN).astype(np.int32), np.full(len(Q), -1, np.int32)
    out = separation(Q, R, sigma, status, doff, radius, margin)
    out["delay"] = out["delay"] * np.float64(h)
    out.update(status=status, delay_steps=sigma, blocker=blocker)
    return out


def conflict_scalar(Qa, sa, Qb, sb, doff, thr2):
    """an independent scalar double loop: does any step j = 0 .. max(end) bring any component pair closer than thr2"""
    jend = max(end_step(sa, len(Qa)), end_step(sb, len(Qb)))
    for j in range(jend + 1):
        pa = Qa[0] if sa < 0 else Qa[min(max(j - sa, 0), len(Qa) - 1)]
        pb = Qb[0] if sb < 0 else Qb[min(max(j - sb, 0), len(Qb) - 1)]
        for d in doff:
            d2 = 0.0
            for x in range(len(pa)):
                dx = (float(pa[x]) - float(pb[x])) + float(d[x])
                d2 = d2 + dx * dx
            if d2 < thr2:
                return True
    return False
