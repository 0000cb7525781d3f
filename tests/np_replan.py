"""Numpy restatement of receding-horizon replanning, written from the definitions of include/gusto_hip.h and from nothing in
csrc/: the seeded start of gusto_set_problems_replan one knot at a time in the stated order, the unseeded straight line, tf', and
the perturbation rule of the studies.  Plain float64, one rounding per operation as written (no fused multiply-add)."""
import math

import numpy as np

from np_multistart import U_DIM, X_DIM, goal_centre, straight_line  # noqa: F401


def sigma(tau, k, N, Ns):
    """(sigma_k, j, a): the source's knot coordinate of the new knot k"""
    s = (tau * (N - 1 - k) + k) * (Ns - 1) / (N - 1)
    j = min(int(math.floor(s)), Ns - 2)
    return s, j, s - j


def seeded_start(Xs, Us, tau, x_now, N, c_old=None, c_new=None):
    """(X0 [N, n], U0 [N, m]) of one seeded problem from the source rows Xs [Ns, n], Us [Ns, m]; c_old, c_new: the goal centres of
    the source's and of the caller's goals (both None: no goals were passed, the t_k term is skipped)"""
    Xs, Us, x_now = np.asarray(Xs, float), np.asarray(Us, float), np.asarray(x_now, float)
    Ns, n = Xs.shape
    tau = float(tau)
    X0, U0 = np.zeros((N, n)), np.zeros((N, Us.shape[1]))
    _, j0, a0 = sigma(tau, 0, N, Ns)
    S0 = (1 - a0) * Xs[j0] + a0 * Xs[j0 + 1]
    for k in range(N):
        t = k / (N - 1)
        _, j, a = sigma(tau, k, N, Ns)
        if k == N - 1:
            S, U0[k] = Xs[Ns - 1], Us[Ns - 1]
        else:
            S = (1 - a) * Xs[j] + a * Xs[j + 1]
            U0[k] = (1 - a) * Us[j] + a * Us[j + 1]
        d = (1 - t) * (x_now - S0)
        if c_new is not None:
            d = d + t * (np.asarray(c_new, float) - np.asarray(c_old, float))
        X0[k] = x_now if k == 0 else S + d
    return X0, U0


def replan(N, Xs, Us, tf_s, lo_s, hi_s, tau, x_now, seeded, goal_lo=None, goal_hi=None):
    """gusto_set_problems_replan on the source rows Xs [B, Ns, n], Us [B, Ns, m] and the source problems' tf_s [B], lo_s, hi_s
    [B, n]: a dict of x_init, goal_lo, goal_hi [B, n], tf [B], X0 [B, N, n], U0 [B, N, m]"""
    Xs, Us = np.asarray(Xs, float), np.asarray(Us, float)
    B, n, m = len(Xs), Xs.shape[2], Us.shape[2]
    x_now = np.asarray(x_now, float).reshape(B, n)
    tau = np.broadcast_to(np.asarray(tau, float), (B,))
    lo = np.asarray(lo_s if goal_lo is None else goal_lo, float).reshape(B, n)
    hi = np.asarray(hi_s if goal_hi is None else goal_hi, float).reshape(B, n)
    out = dict(x_init=x_now.copy(), goal_lo=lo.copy(), goal_hi=hi.copy(), tf=(1 - tau) * np.asarray(tf_s, float),
               X0=np.zeros((B, N, n)), U0=np.zeros((B, N, m)))
    for b in range(B):
        if not seeded[b]:
            out["X0"][b] = straight_line(x_now[b], lo[b], hi[b], N)
        elif goal_lo is None:
            out["X0"][b], out["U0"][b] = seeded_start(Xs[b], Us[b], tau[b], x_now[b], N)
        else:
            out["X0"][b], out["U0"][b] = seeded_start(Xs[b], Us[b], tau[b], x_now[b], N, goal_centre(np.asarray(lo_s)[b], np.asarray(hi_s)[b]),
                                                      goal_centre(lo[b], hi[b]))
    return out


def perturbation(q):
    """p_q [6] of the freeflyer studies: positions +-0.02 m, velocities +-0.002 m/s, from the first four doubles of the
    splitmix64 stream seeded 0xC0FFEE + q"""
    from gusto_jl_amd import problems
    gen = problems.splitmix64(0xC0FFEE + q)
    r = [next(gen) for _ in range(4)]
    p = np.zeros(6)
    p[0:2] = [0.02 * (2 * r[0] - 1), 0.02 * (2 * r[1] - 1)]
    p[3:5] = [0.002 * (2 * r[2] - 1), 0.002 * (2 * r[3] - 1)]
    return p
