"""Numpy restatement of the goal timeline, written from the definitions of include/gusto_hip.h and from nothing in csrc/: the
argument check, the leg problems and seeds of gusto_legs_begin, the advance rule and the join of gusto_legs_advance, plus fly(),
which drives any solve function through the rounds.  Plain float64, one rounding per operation as written; the one exception
is device_line, the straight line as the device rounds it."""
from fractions import Fraction

import numpy as np

from np_multistart import U_DIM, X_DIM, goal_centre, straight_line

AUTO, SEQUENTIAL, PARALLEL = 0, 1, 2
FLYING, DONE, FAILED = 1, 2, 4
MAX_STARTS = 64
PER_QUERY = ("status", "failed_leg", "n_done", "J_total")
PER_LEG = ("iterations", "converged", "successful", "stop_reason", "J", "gap", "arrive")
REPORT = PER_QUERY + PER_LEG + ("X", "U", "t")


def device_line(x_init, lo, hi, N):
    """straight_line as csrc/seed.hpp pins its rounding: fma(t, centre, (1 - t) x_init), the sum of the exact product and the
    rounded one, rounded once (exact rational arithmetic; float(Fraction) rounds to nearest even)"""
    x_init, c = np.asarray(x_init, float), goal_centre(lo, hi)
    X = np.zeros((N, len(x_init)))
    for k in range(N):
        t = np.float64(k) / np.float64(N - 1)
        for i in range(len(x_init)):
            X[k, i] = float(Fraction(float(t)) * Fraction(float(c[i])) + Fraction(float((1 - t) * x_init[i])))
    return X


def full_points(glo, ghi, n_legs):
    """every interior goal (l < L_q - 1) of every query pins every entry: lo == hi, finite"""
    Bq, L, _ = glo.shape
    inner = np.arange(L)[None, :] < np.asarray(n_legs)[:, None] - 1
    return bool(((glo == ghi) & np.isfinite(glo)).all(axis=2)[inner].all())


def check_args(n, batch_cap, Bq, L, n_legs, x_init, goal_lo, goal_hi, t_goal, mode=AUTO, trajopt=False):
    """The refusals of gusto_legs_begin, in its order: ValueError with the cause, else the mode taken (never AUTO)"""
    if trajopt:
        raise ValueError("TrajOpt handle")
    if L < 1 or L > MAX_STARTS:
        raise ValueError("L outside 1 .. GUSTO_MAX_STARTS")
    if Bq < 1:
        raise ValueError("need Bq >= 1")
    if any(a is None for a in (x_init, goal_lo, goal_hi, t_goal)):
        raise ValueError("a null array")
    if mode not in (AUTO, SEQUENTIAL, PARALLEL):
        raise ValueError("unknown mode")
    x_init = np.asarray(x_init, float).reshape(Bq, n)
    glo, ghi = (np.asarray(a, float).reshape(Bq, L, n) for a in (goal_lo, goal_hi))
    T = np.asarray(t_goal, float).reshape(Bq, L)
    nl = np.full(Bq, L) if n_legs is None else np.asarray(n_legs).reshape(Bq)
    for q in range(Bq):
        if nl[q] < 1 or nl[q] > L:
            raise ValueError("n_legs outside 1 .. L (query %d)" % q)
        before = 0.0
        for l in range(nl[q]):
            if not (T[q, l] > before and T[q, l] < np.inf):
                raise ValueError("need 0 < T_0 < T_1 < ... < inf (query %d)" % q)
            before = T[q, l]
        if not np.isfinite(x_init[q]).all():
            raise ValueError("x_init must be finite (query %d)" % q)
    points = full_points(glo, ghi, nl)
    if mode == PARALLEL and not points:
        raise ValueError("GUSTO_LEGS_PARALLEL: an interior goal does not pin every entry")
    if mode == AUTO:
        mode = PARALLEL if points else SEQUENTIAL
    if Bq * (L if mode == PARALLEL else 1) > batch_cap:
        raise ValueError("B above batch_cap")
    return mode


def leg_tf(T, l):
    """tf of leg l: T_l - T_{l-1}, one rounded difference; T_0 itself"""
    return np.float64(T[0]) if l == 0 else np.float64(T[l]) - np.float64(T[l - 1])


def leg_times(T, l, N):
    """t [N] of leg l: T_{l-1} + k (tf_l / (N - 1)), T_l itself at k = N - 1"""
    T0 = np.float64(0.0) if l == 0 else np.float64(T[l - 1])
    dt = leg_tf(T, l) / np.float64(N - 1)
    t = T0 + np.arange(N, dtype=np.float64) * dt
    t[N - 1] = T[l]
    return t


def arrive_violation(x, lo, hi):
    """the largest violation of a goal's rows at x: |x - lo| on point entries, max(lo - x, x - hi, 0) on the others"""
    with np.errstate(invalid="ignore"):
        v = np.where(lo == hi, np.abs(x - lo), np.fmax(np.fmax(lo - x, x - hi), 0.0))
    return np.float64(v.max())


class Timeline:
    """The state gusto_legs_begin creates for Bq queries x L legs and gusto_legs_advance moves.  line: the straight line of the
    seeds, straight_line (the host's rounding) or device_line (the device's)"""

    def __init__(self, model_id, N, x_init, goal_lo, goal_hi, t_goal, n_legs=None, mode=AUTO, batch_cap=1 << 30, line=straight_line):
        n, m = X_DIM[model_id], U_DIM[model_id]
        self.model_id, self.N, self.n, self.m, self.line = model_id, int(N), n, m, line
        self.x_init = np.asarray(x_init, float).reshape(-1, n)
        Bq = self.Bq = len(self.x_init)
        self.glo, self.ghi = (np.asarray(a, float).reshape(Bq, -1, n) for a in (goal_lo, goal_hi))
        L = self.L = self.glo.shape[1]
        self.T = np.broadcast_to(np.asarray(t_goal, float), (Bq, L)).copy()
        self.nl = np.full(Bq, L) if n_legs is None else np.asarray(n_legs, int).reshape(Bq)
        self.mode = check_args(n, batch_cap, Bq, L, self.nl, self.x_init, self.glo, self.ghi, self.T, mode)
        self.K = K = L if self.mode == PARALLEL else 1
        self.Nj = Nj = L * (N - 1) + 1
        self.status, self.failed_leg = np.full(Bq, FLYING, np.int32), np.full(Bq, -1, np.int32)
        self.n_done, self.J_total = np.zeros(Bq, np.int32), np.zeros(Bq)
        for k in ("iterations", "converged", "successful", "stop_reason"):
            setattr(self, k, np.zeros((Bq, L), np.int32))
        self.J, self.gap, self.arrive = np.zeros((Bq, L)), np.zeros((Bq, L)), np.zeros((Bq, L))
        self.X, self.U, self.t = np.zeros((Bq, Nj, n)), np.zeros((Bq, Nj, m)), np.zeros((Bq, Nj))
        self.round = 0
        B = self.B = Bq * K
        self.p_xinit, self.p_lo, self.p_hi, self.p_tf = np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n)), np.zeros(B)
        self.p_X, self.p_U, self.active = np.zeros((B, N, n)), np.zeros((B, N, m)), np.ones(B, bool)
        for b in range(B):
            q, j = divmod(b, K)
            l = min(j, self.nl[q] - 1)
            self._seed(b, q, l, self.x_init[q] if l == 0 else self.glo[q, l - 1])
            self.active[b] = j < self.nl[q] or K == 1

    def _seed(self, b, q, l, junction):
        """problem b becomes leg l of query q from `junction`: the straight line, U0 = 0"""
        self.p_xinit[b], self.p_lo[b], self.p_hi[b], self.p_tf[b] = junction, self.glo[q, l], self.ghi[q, l], leg_tf(self.T[q], l)
        self._rest(b)

    def _rest(self, b):
        """problem b becomes the straight line of its own inputs"""
        self.p_X[b], self.p_U[b] = self.line(self.p_xinit[b], self.p_lo[b], self.p_hi[b], self.N), 0.0

    def flying(self):
        return self.status == FLYING

    def n_flying(self):
        return int(self.flying().sum())

    def problems(self):
        """(x_init, lo, hi [B, n], tf [B], X0 [B, N, n], U0 [B, N, m], active [B]) the handle holds after begin or the last advance"""
        return tuple(a.copy() for a in (self.p_xinit, self.p_lo, self.p_hi, self.p_tf, self.p_X, self.p_U, self.active))

    def report(self):
        return {k: getattr(self, k).copy() for k in REPORT}

    def _store(self, q, l, b, X, U, st, last):
        """leg l of query q, solved as problem b, into the joined buffers and the report.  last: it takes its own U[N-1]
        (SEQUENTIAL: every leg does, and the next leg's U[0] is written over it)"""
        N = self.N
        at = l * (N - 1)
        t = leg_times(self.T[q], l, N)
        k0 = 0 if l == 0 else 1                       # a junction's X and t: the last knot of the leg before
        self.X[q, at + k0:at + N], self.t[q, at + k0:at + N] = X[b, k0:], t[k0:]
        self.U[q, at:at + (N if last else N - 1)] = U[b, :N if last else N - 1]
        for k in ("iterations", "converged", "successful", "stop_reason"):
            getattr(self, k)[q, l] = st[k][b]
        self.J[q, l] = st["J"][b]
        self.gap[q, l] = 0.0 if l == 0 else np.abs(X[b, 0] - self.p_xinit[b]).max()
        self.arrive[q, l] = arrive_violation(X[b, N - 1], self.p_lo[b], self.p_hi[b])

    def advance(self, ok, X, U, st):
        """gusto_legs_advance: ok [B] the verdicts, X, U [B, N, .] the handle's trajectories after the solve, st a dict of
        iterations, converged, successful, stop_reason, J [B] (J: the last J_true, NaN when there is none).  Returns n_flying"""
        assert self.n_flying() > 0
        ok = np.asarray(ok).astype(bool).reshape(self.B)
        X, U = np.asarray(X, float), np.asarray(U, float)
        L = self.L
        if self.mode == SEQUENTIAL:
            r = self.round
            for q in np.flatnonzero(self.flying()):
                self._store(q, r, q, X, U, st, True)
                self.J_total[q] = self.J_total[q] + st["J"][q]
                if ok[q] and r + 1 < self.nl[q]:
                    self.n_done[q] = r + 1
                    self._seed(q, q, r + 1, X[q, self.N - 1].copy())      # the junction as stored, copied
                else:
                    if ok[q]:
                        self.n_done[q], self.status[q] = r + 1, DONE
                    else:
                        self.status[q], self.failed_leg[q] = FAILED, r
                    self._rest(q)
                    self.active[q] = False
        else:
            for q in range(self.Bq):
                Jt, failed = np.float64(0.0), -1
                for l in range(self.nl[q]):
                    b = q * L + l
                    self._store(q, l, b, X, U, st, l == self.nl[q] - 1)
                    Jt = Jt + st["J"][b]
                    if failed < 0 and not ok[b]:
                        failed = l
                    self._rest(b)
                self.J_total[q], self.failed_leg[q] = Jt, failed
                self.n_done[q] = self.nl[q] if failed < 0 else failed
                self.status[q] = DONE if failed < 0 else FAILED
            self.active[:] = False
        self.round += 1
        return self.n_flying()


def fly(solve, model_id, N, x_init, goal_lo, goal_hi, t_goal, n_legs=None, mode=AUTO, line=straight_line):
    """The rounds of a timeline around `solve(x_init, lo, hi, tf, X0, U0, active) -> (ok [B], X [B, N, n], U [B, N, m], st, info)`,
    which solves the active problems of a batch and leaves the others as they are; st as Timeline.advance reads it.  Returns (the
    Timeline, per round the (active, ok, info) of the solves)."""
    S = Timeline(model_id, N, x_init, goal_lo, goal_hi, t_goal, n_legs, mode, line=line)
    log = []
    while S.n_flying() > 0:
        prob = S.problems()
        ok, X, U, st, info = solve(*prob)
        log.append((prob[6], np.asarray(ok).astype(bool) & prob[6], info))
        S.advance(ok, X, U, st)
    return S, log
