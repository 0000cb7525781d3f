"""Numpy restatement of the final-time search, written from the definitions of include/gusto_hip.h and from nothing in csrc/: the
candidates, the two seeds and the update rule of gusto_tfsearch_begin / gusto_tfsearch_update, plus search(), which drives any
solve function through the rounds.  Plain float64, one rounding per operation as written (no fused multiply-add)."""
import numpy as np

from np_multistart import U_DIM, X_DIM, goal_centre, straight_line

SEED_LINE, SEED_INCUMBENT = 0, 1
NONE, DONE, FLOOR, NONMONOTONE = 1, 2, 4, 8
FINISHED = NONE | DONE
MAX_STARTS = 64
RATES = {0: (3, 4, 5), 1: (), 2: (3, 4, 5, 9, 10, 11), 3: (3, 4, 5, 10, 11, 12)}   # the entries that scale with 1 / tf


def candidates(lo, hi, K, incumbent):
    """T [K] of one query: lo + (j + 1) (w / K) and hi itself at j = K - 1 without an incumbent, lo + (j + 1) (w / (K + 1)) with"""
    lo, hi = np.float64(lo), np.float64(hi)
    w = hi - lo
    step = w / np.float64(K + 1 if incumbent else K)
    T = lo + np.arange(1, K + 1, dtype=np.float64) * step
    if not incumbent:
        T[K - 1] = hi
    return T


def line_seed(model_id, x_init, lo, hi, N):
    """(X0 [N, n], U0 [N, m]): the straight line"""
    return straight_line(x_init, lo, hi, N), np.zeros((N, U_DIM[model_id]))


def retimed_seed(model_id, x_init, lo, hi, N, tf_best, X_inc, U_inc, T):
    """(X0, U0) of a candidate T from the incumbent (tf_best, X_inc, U_inc): s = tf_best / T; the rate entries become
    s X_inc + (1 - s) L, the others stay, U0 = (s s) U_inc, knot 0 is x_init itself"""
    s = np.float64(tf_best) / np.float64(T)
    s2 = s * s
    L = straight_line(x_init, lo, hi, N)
    X0 = np.array(X_inc, dtype=np.float64, copy=True)
    for i in RATES[model_id]:
        X0[:, i] = s * X0[:, i] + (1 - s) * L[:, i]
    X0[0] = np.asarray(x_init, float)
    return X0, s2 * np.asarray(U_inc, float)


class Search:
    """The state gusto_tfsearch_begin creates for Bq queries x K candidates and gusto_tfsearch_update moves"""

    def __init__(self, model_id, N, K, x_init, goal_lo, goal_hi, tf_lo, tf_hi, rtol=0.01, seed=SEED_INCUMBENT):
        n = X_DIM[model_id]
        self.model_id, self.N, self.K, self.rtol, self.seed = model_id, int(N), int(K), np.float64(rtol), seed
        self.x_init, self.glo, self.ghi = (np.asarray(a, float).reshape(-1, n) for a in (x_init, goal_lo, goal_hi))
        Bq = self.Bq = len(self.x_init)
        self.lo0 = np.broadcast_to(np.asarray(tf_lo, float), (Bq,)).copy()
        self.hi0 = np.broadcast_to(np.asarray(tf_hi, float), (Bq,)).copy()
        assert 1 <= K <= MAX_STARTS and (0 < self.lo0).all() and (self.lo0 < self.hi0).all() and np.isfinite(self.hi0).all()
        self.lo, self.hi = self.lo0.copy(), self.hi0.copy()
        self.tf_best, self.J_best = np.full(Bq, np.nan), np.full(Bq, np.nan)
        self.round_found, self.status, self.n_eligible = np.full(Bq, -1, np.int32), np.zeros(Bq, np.int32), np.zeros(Bq, np.int32)
        self.X, self.U = np.zeros((Bq, N, n)), np.zeros((Bq, N, U_DIM[model_id]))
        self.cand = np.stack([candidates(self.lo[q], self.hi[q], K, False) for q in range(Bq)])
        self.round = 0
        self.parked = np.zeros(Bq, bool)       # done before the last update: the problems stay as they are

    def searching(self):
        return (self.status & FINISHED) == 0

    def report(self):
        return {k: getattr(self, k).copy() for k in ("status", "round_found", "n_eligible", "lo", "hi", "tf_best", "J_best", "cand", "X", "U")}

    def problems(self, prev=None):
        """(x_init, lo, hi [B, n], tf [B], X0 [B, N, n], U0 [B, N, m]) the handle holds after begin or the last update; the rows of a
        parked query come from `prev`, the same tuple one update earlier"""
        K, N = self.K, self.N
        rep = lambda a: np.repeat(a, K, axis=0)
        X0, U0 = np.zeros((self.Bq * K, N, self.X.shape[2])), np.zeros((self.Bq * K, N, self.U.shape[2]))
        tf = self.cand.reshape(-1).copy()
        for q in range(self.Bq):
            for j in range(K):
                b = q * K + j
                if self.parked[q]:
                    tf[b], X0[b], U0[b] = prev[3][b], prev[4][b], prev[5][b]
                elif self.seed == SEED_INCUMBENT and self.round_found[q] >= 0 and self.searching()[q]:
                    X0[b], U0[b] = retimed_seed(self.model_id, self.x_init[q], self.glo[q], self.ghi[q], N, self.tf_best[q], self.X[q],
                                                self.U[q], self.cand[q, j])
                else:
                    X0[b], U0[b] = line_seed(self.model_id, self.x_init[q], self.glo[q], self.ghi[q], N)
        return rep(self.x_init), rep(self.glo), rep(self.ghi), tf, X0, U0

    def update(self, ok, T=None, X=None, U=None, J=None):
        """gusto_tfsearch_update: ok [B] the verdicts, T [B] the problems' final times (None: the candidates), X, U the solved
        trajectories [B, N, .] and J [B] their last true costs (None: zeros / NaN)"""
        K = self.K
        ok = np.asarray(ok).astype(bool).reshape(self.Bq, K)
        T = self.cand.copy() if T is None else np.asarray(T, float).reshape(self.Bq, K)
        for q in range(self.Bq):
            if self.status[q] & FINISHED:
                self.parked[q] = True
                continue
            self.parked[q] = False
            have, lo_old, F = self.round_found[q] >= 0, self.lo[q], self.tf_best[q]
            self.n_eligible[q] = ok[q].sum()
            w = -1
            for j in range(K):                                   # the smallest eligible final time, ties to the lowest j
                if ok[q, j] and (w < 0 or T[q, j] < T[q, w]):
                    w = j
            if w >= 0 and (not have or T[q, w] < F):             # (strict: an equal tf does not replace the incumbent)
                b = q * K + w
                F = self.tf_best[q] = T[q, w]
                self.X[q] = 0.0 if X is None else np.asarray(X)[b]
                self.U[q] = 0.0 if U is None else np.asarray(U)[b]
                self.J_best[q] = np.nan if J is None else np.asarray(J)[b]
                self.round_found[q] = self.round
                have = True
            if have:
                lo = self.lo0[q]
                if lo_old < F:
                    lo = max(lo, lo_old)
                for j in range(K):
                    if not ok[q, j] and T[q, j] < F:
                        lo = max(lo, T[q, j])
                hi = F
            else:
                lo, hi = T[q].max(), self.hi0[q]
            st = self.status[q] & NONMONOTONE
            if not have:
                st |= NONE
            if hi - lo <= self.rtol * hi:
                st |= DONE
            if lo == self.lo0[q]:
                st |= FLOOR
            good, bad = np.flatnonzero(ok[q]), np.flatnonzero(~ok[q])
            if (len(good) and len(bad) and good[0] < bad[-1]) or (have and lo_old >= F):   # some i < j with ok_i and not ok_j
                st |= NONMONOTONE
            self.lo[q], self.hi[q], self.status[q] = lo, hi, st
            self.cand[q] = hi if st & FINISHED else candidates(lo, hi, K, True)
        self.round += 1
        return int(self.searching().sum())


def search(solve, model_id, N, K, x_init, goal_lo, goal_hi, tf_lo, tf_hi, rounds, rtol=0.01, seed=SEED_INCUMBENT):
    """The rounds of a search around `solve(x_init, lo, hi, tf, X0, U0, active) -> (ok [B], X [B, N, n], U [B, N, m], J [B], info)`,
    which solves the active problems of a batch.  Returns (the Search, per round the (candidates, ok, info) of the solves)."""
    S = Search(model_id, N, K, x_init, goal_lo, goal_hi, tf_lo, tf_hi, rtol, seed)
    log, prob = [], None
    for _ in range(rounds):
        prob = S.problems(prob)
        active = np.repeat(S.searching(), K)
        ok, X, U, J, info = solve(*prob, active)
        log.append((S.cand.copy(), np.asarray(ok).astype(bool).reshape(S.Bq, K) & active.reshape(S.Bq, K), info))
        if S.update(np.asarray(ok).astype(bool) & active, prob[3], X, U, J) == 0:
            break
    return S, log
