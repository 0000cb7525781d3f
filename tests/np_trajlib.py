"""Numpy restatement of the trajectory library, written from the definitions of include/gusto_hip.h and from nothing in csrc/:
the distance, the neighbour rule, the retargeting and the compaction of gusto_trajlib_add.  Plain float64, one rounding per
operation as written (no fused multiply-add)."""
import numpy as np

from np_multistart import U_DIM, X_DIM, goal_centre, straight_line  # noqa: F401

MAX_K = 8


class Lib:
    """the entries of a library as arrays: x_init, c [L, n], tf [L], tag [L], X [L, N, n], U [L, N, m]; w_init, w_goal [n], w_tf"""

    def __init__(self, model_id, N, w_init=None, w_goal=None, w_tf=0.0):
        self.model_id, self.N, self.n, self.m = model_id, N, X_DIM[model_id], U_DIM[model_id]
        self.w_init = np.ones(self.n) if w_init is None else np.broadcast_to(np.asarray(w_init, float), (self.n,)).copy()
        self.w_goal = np.ones(self.n) if w_goal is None else np.broadcast_to(np.asarray(w_goal, float), (self.n,)).copy()
        self.w_tf = float(w_tf)
        self.x_init, self.c = np.zeros((0, self.n)), np.zeros((0, self.n))
        self.tf, self.tag = np.zeros(0), np.zeros(0, np.int32)
        self.X, self.U = np.zeros((0, N, self.n)), np.zeros((0, N, self.m))

    def __len__(self):
        return len(self.tf)

    def add(self, x_init, lo, hi, tf, X, U, tag=None):
        """gusto_trajlib_add_host"""
        x_init, lo, hi = (np.asarray(a, float).reshape(-1, self.n) for a in (x_init, lo, hi))
        cnt = len(x_init)
        tf = np.broadcast_to(np.asarray(tf, float), (cnt,))
        tag = np.zeros(cnt, np.int32) if tag is None else np.broadcast_to(np.asarray(tag, np.int32), (cnt,))
        self.x_init = np.concatenate([self.x_init, x_init])
        self.c = np.concatenate([self.c, goal_centre(lo, hi).reshape(-1, self.n)])
        self.tf, self.tag = np.concatenate([self.tf, tf]), np.concatenate([self.tag, tag])
        self.X = np.concatenate([self.X, np.asarray(X, float).reshape(cnt, self.N, self.n)])
        self.U = np.concatenate([self.U, np.asarray(U, float).reshape(cnt, self.N, self.m)])

    def add_masked(self, mask, x_init, lo, hi, tf, X, U, tag=None):
        """gusto_trajlib_add: the problems whose mask is nonzero, in ascending order"""
        keep = np.flatnonzero(np.asarray(mask))
        tag = np.zeros(len(np.asarray(mask)), np.int32) if tag is None else np.asarray(tag)
        self.add(np.asarray(x_init)[keep], np.asarray(lo)[keep], np.asarray(hi)[keep], np.asarray(tf)[keep], np.asarray(X)[keep],
                 np.asarray(U)[keep], tag[keep])
        return len(keep)


def n_terms(lib):
    """the number of accumulated terms of d2: the positive weights"""
    return int((lib.w_init > 0).sum() + (lib.w_goal > 0).sum() + (lib.w_tf > 0))


def dist2(lib, xi_q, c_q, tf_q):
    """d2 [L] of one query: the positive-weight terms only, accumulated from 0 in the order x_init, centre, tf"""
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.zeros(len(lib))
        for i in range(lib.n):
            if lib.w_init[i] > 0:
                t = xi_q[i] - lib.x_init[:, i]
                d = d + lib.w_init[i] * (t * t)
        for i in range(lib.n):
            if lib.w_goal[i] > 0:
                t = c_q[i] - lib.c[:, i]
                d = d + lib.w_goal[i] * (t * t)
        if lib.w_tf > 0:
            t = tf_q - lib.tf
            d = d + lib.w_tf * (t * t)
    return d


def neighbours(d2, K, elig=None):
    """(entry [K], dist2 [K], n_found): the K smallest eligible entries in ascending (d2, e); a NaN is never a neighbour; the
    starts behind n_found are -1, +inf"""
    d2 = np.asarray(d2, float)
    ok = ~np.isnan(d2) if elig is None else (~np.isnan(d2) & np.asarray(elig, bool))
    cand = sorted((d2[e], e) for e in np.flatnonzero(ok))[:K]
    entry, dist = np.full(K, -1, np.int32), np.full(K, np.inf)
    for j, (d, e) in enumerate(cand):
        entry[j], dist[j] = e, d
    return entry, dist, len(cand)


def search(lib, x_init, lo, hi, tf, K, tag=None):
    """gusto_get_trajlib_seeds of a batch of queries: entry, dist2 [Bq, K], n_found [Bq]"""
    x_init, lo, hi = (np.asarray(a, float).reshape(-1, lib.n) for a in (x_init, lo, hi))
    Bq = len(x_init)
    tf = np.broadcast_to(np.asarray(tf, float), (Bq,))
    out = dict(entry=np.zeros((Bq, K), np.int32), dist2=np.zeros((Bq, K)), n_found=np.zeros(Bq, np.int32))
    for q in range(Bq):
        d = dist2(lib, x_init[q], goal_centre(lo[q], hi[q]), tf[q])
        out["entry"][q], out["dist2"][q], out["n_found"][q] = neighbours(d, K, None if tag is None else lib.tag == np.asarray(tag)[q])
    return out


def retarget(lib, e, x_init, lo, hi):
    """(X0 [N, n], U0 [N, m]) of one start seeded from entry e (-1: the straight line, U0 = 0)"""
    x_init = np.asarray(x_init, float)
    if e < 0:
        return straight_line(x_init, lo, hi, lib.N), np.zeros((lib.N, lib.m))
    t = (np.arange(lib.N) / (lib.N - 1))[:, None]
    dxi, dc = (x_init - lib.x_init[e])[None, :], (goal_centre(lo, hi) - lib.c[e])[None, :]
    X = lib.X[e] + ((1 - t) * dxi + t * dc)
    X[0] = x_init
    return X, lib.U[e].copy()


def retarget_bound(lib, e, x_init, lo, hi):
    """[n]: (|X_e| + |dxi| + |dc|) of the retargeting tolerance, the largest |X_e| over the knots taken per state"""
    return np.abs(lib.X[e]).max(axis=0) + np.abs(np.asarray(x_init, float) - lib.x_init[e]) + np.abs(goal_centre(lo, hi) - lib.c[e])


def seeded_problems(lib, x_init, lo, hi, tf, K, tag=None):
    """gusto_set_problems_trajlib: (x_init, lo, hi [B, n], tf [B], X0 [B, N, n], U0 [B, N, m], seeds) with B = Bq K and problem
    q K + j = neighbour j of query q"""
    x_init, lo, hi = (np.asarray(a, float).reshape(-1, lib.n) for a in (x_init, lo, hi))
    Bq = len(x_init)
    tf = np.broadcast_to(np.asarray(tf, float), (Bq,))
    seeds = search(lib, x_init, lo, hi, tf, K, tag)
    XU = [retarget(lib, seeds["entry"][q, j], x_init[q], lo[q], hi[q]) for q in range(Bq) for j in range(K)]
    rep = lambda a: np.repeat(a, K, axis=0)
    return rep(x_init), rep(lo), rep(hi), rep(tf), np.stack([x for x, _ in XU]), np.stack([u for _, u in XU]), seeds


def min_relative_gap(d2, K):
    """the smallest relative difference between consecutive sorted d2 among the K + 1 smallest: the inputs of a search test
    must keep it above 1e-12, so that the device's roundings cannot reorder neighbours"""
    s = np.sort(np.asarray(d2, float))[:K + 1]
    if len(s) < 2:
        return np.inf
    return float(np.min(np.diff(s) / np.maximum(s[1:], np.finfo(float).tiny)))
