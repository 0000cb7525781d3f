"""Numpy restatement of the multi-start entry points, written from the definitions of include/gusto_hip.h and from nothing in
csrc/: the fan of gusto_set_problems_multistart (frame, tent, replication) and the selection rule of gusto_select_best.  Plain
float64, one rounding per operation as written (no fused multiply-add)."""
import numpy as np

WS_DIM = {0: 2, 1: 2, 2: 3, 3: 3}
X_DIM = {0: 6, 1: 3, 2: 12, 3: 13}
U_DIM = {0: 3, 1: 1, 2: 6, 3: 6}
MAX_STARTS = 64
H_MIN = 1e-9     # the frame's threshold on hypot(e1_x, e1_y)


def goal_centre(lo, hi):
    """(lo + hi) / 2 where both are finite, else 0: the straight line's rule"""
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    fin = np.isfinite(lo) & np.isfinite(hi)
    return np.where(fin, 0.5 * (np.where(fin, lo, 0.0) + np.where(fin, hi, 0.0)), 0.0)


def straight_line(x_init, lo, hi, N):
    """X [N, n]: knot k is (1 - t_k) x_init + t_k centre, t_k = k / (N - 1)"""
    t = np.arange(N) / (N - 1)
    return (1 - t)[:, None] * np.asarray(x_init, float)[None, :] + t[:, None] * goal_centre(lo, hi)[None, :]


def frame(ws, p_i, p_g):
    """(e1, e2) in the plane, (e1, e2, e3) in space, of the direction p_g - p_i"""
    d = np.asarray(p_g, float) - np.asarray(p_i, float)
    L = np.hypot(d[0], d[1]) if ws == 2 else np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    e1 = np.eye(ws)[0] if L == 0 else d / L
    if ws == 2:
        return e1, np.array([-e1[1], e1[0]])
    h = np.hypot(e1[0], e1[1])
    e2 = np.array([-e1[1] / h, e1[0] / h, 0.0]) if h > H_MIN else np.array([1.0, 0.0, 0.0])
    e3 = np.array([e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]])
    return e1, e2, e3


def tent(N):
    """tent(t_k) = 1 - |2 t_k - 1| at the N knots: 0 at both ends"""
    t = np.arange(N) / (N - 1)
    return 1.0 - np.abs(2.0 * t - 1.0)


def detour(model_id, x_init, lo, hi, offset):
    """w = a2 e2 + a3 e3 of one start (a3 is not read in the plane), or None for a start that skips the addition"""
    ws = WS_DIM[model_id]
    a2, a3 = float(offset[0]), (float(offset[1]) if ws == 3 else 0.0)
    if a2 == 0.0 and a3 == 0.0:
        return None
    f = frame(ws, np.asarray(x_init, float)[:ws], goal_centre(lo, hi)[:ws])
    return a2 * f[1] if ws == 2 else a2 * f[1] + a3 * f[2]


def fan_start(model_id, x_init, lo, hi, N, offset):
    """X0 [N, n] of one start of one query"""
    X = straight_line(x_init, lo, hi, N)
    w = detour(model_id, x_init, lo, hi, offset)
    if w is not None:
        X[:, :WS_DIM[model_id]] += tent(N)[:, None] * w[None, :]
    return X


def fan_problems(model_id, x_init, lo, hi, tf, N, fan):
    """gusto_set_problems_multistart: (x_init, lo, hi [B, n], tf [B], X0 [B, N, n], U0 [B, N, m]) with B = Bq K and problem
    q K + j = start j of query q"""
    x_init, lo, hi = (np.asarray(a, float).reshape(-1, X_DIM[model_id]) for a in (x_init, lo, hi))
    fan = np.asarray(fan, float).reshape(-1, 2)
    Bq, K = len(x_init), len(fan)
    tf = np.broadcast_to(np.asarray(tf, float), (Bq,))
    X0 = np.stack([fan_start(model_id, x_init[q], lo[q], hi[q], N, fan[j]) for q in range(Bq) for j in range(K)])
    rep = lambda a: np.repeat(a, K, axis=0)
    return rep(x_init), rep(lo), rep(hi), rep(tf), X0, np.zeros((Bq * K, N, U_DIM[model_id]))


def select_best(K, score, eligible, X=None, U=None):
    """gusto_select_best on score, eligible [B]: the eligible start with the smallest score under a strict < in ascending j; a
    NaN never wins; without a winner -1, -1, +inf and zero rows"""
    score, eligible = np.asarray(score, float), np.asarray(eligible).astype(bool)
    B = len(score)
    assert B % K == 0
    Bq = B // K
    out = dict(winner=np.full(Bq, -1, np.int32), winner_problem=np.full(Bq, -1, np.int32), n_eligible=np.zeros(Bq, np.int32),
               best_score=np.full(Bq, np.inf))
    for q in range(Bq):
        for j in range(K):
            b = q * K + j
            if not eligible[b]:
                continue
            out["n_eligible"][q] += 1
            if np.isnan(score[b]):
                continue
            if out["winner"][q] < 0 or score[b] < out["best_score"][q]:
                out["winner"][q], out["winner_problem"][q], out["best_score"][q] = j, b, score[b]
    for name, A in (("X", X), ("U", U)):
        if A is not None:
            A = np.asarray(A)
            out[name] = np.stack([A[b] if b >= 0 else np.zeros_like(A[0]) for b in out["winner_problem"]])
    return out


def default_inputs(status, history):
    """the score and eligibility gusto_select_best takes when the caller passes none, from a handle's status() and history()"""
    nJ = history["nJ"]
    score = np.array([history["J_true"][b, nJ[b] - 1] if nJ[b] > 0 else np.nan for b in range(len(nJ))])
    return score, np.asarray(status["converged"]).astype(bool) & np.asarray(status["successful"]).astype(bool)
