"""KKT certificate of a candidate optimum of one GuSTO convex subproblem, independent of how the candidate was computed.

The rows come from np_models.subproblem_rows (written from the reference's model files, not from the oracle).  The problem is
checked in the slack form the kernel solves, scaled by kappa = 1 / max(1, omega):

  min_{z, s}  kappa cost(z) + sum_i s_i
  s.t.        E z = e                                   (lambda, free)
              c_j h_j(z) <= 0                           (mu_j >= 0;  c_j the row's scale)
              kappa (w g_i(z) - off_i) - s_i <= 0       (nu_i >= 0)
              -s_i <= 0                                 (eta_i >= 0)

The slacks are not inputs: each is set to its optimal value s_i = max(0, kappa (w g_i - off_i)).  Stationarity in s reads
nu_i + eta_i = 1.  Every inequality within `tau` of active is a candidate with a multiplier >= 0, every other one has
multiplier 0; so a penalised row with s_i > tau has nu_i = 1, eta_i = 0 (its gradient moves to the right-hand side), one with
kappa (w g_i - off_i) < -tau has nu_i = 0, eta_i = 1 (it drops out), and only rows in the band keep both multipliers and their
s-equation.  The multipliers are fitted by bounded least squares (scipy lsq_linear, BVLS) on

  stationarity in z     kappa grad cost + E^T lambda + sum mu_j c_j grad h_j + sum nu_i kappa w grad g_i = 0
  stationarity in s     nu_i + eta_i = 1                         (band rows)
  complementarity       value_i * y_i = 0                        (one row per candidate)

The complementarity rows keep the fit from loading a row that is near, but not at, active: without them the fit is not unique
where rows are parallel (the manifold model's +-eps quaternion pair and its slack bounds).

Returned residuals: `eq` the worst |E z - e| (long double), `hard` / `goal` the worst violation of the hard / BoxGoal rows
(scaled), `stat` the fit's residual in z relative to max(1, ||grad objective||_inf) together with the residual of the
s-equations, `comp` sum |y_i value_i| over the candidates, `obj` kappa cost + sum s_i (math.fsum), `n_pairs` the number of
complementarity pairs an interior point method carries for these rows (two per penalised row, one per hard row).

The candidate band tau = 1e-2 is generous on purpose.  Interior point optima keep binding rows slightly inside, and a control bound
2.6e-3 (scaled) from active can still carry a small real multiplier (dubins_car, N = 50, problem 1 of config 3 at omega = 10: with
tau = 1e-3 that row was left out and the fit's stationarity stopped at 3.0e-7; with 1e-2 it is 2.6e-10).  The complementarity rows
keep a far-from-active candidate from carrying a multiplier it does not have."""
import math

import numpy as np
import scipy.optimize as so

TAU_CAND = 1e-2


def _sum_ld(terms):
    return float(np.sum(np.asarray(terms, dtype=np.longdouble)))


def certify(rows, X, U, tau=TAU_CAND):
    R = rows
    N, n, m, nzN, kappa = R["N"], R["n"], R["m"], R["nzN"], R["kappa"]
    z = np.hstack([np.asarray(X, float), np.asarray(U, float)]).ravel()
    assert z.size == nzN

    # ---- primal: |E z - e| in long double, hard rows, BoxGoal rows -------------------------------------------------
    E, e = R["E"], R["e"]
    r_eq = E.astype(np.longdouble) @ z.astype(np.longdouble) - e.astype(np.longdouble)
    eq = float(np.abs(r_eq).max()) if len(r_eq) else 0.0
    hv = [(c * fn(z)[0], fn(z)[1], c, kind) for fn, c, kind in R["hard"]]
    hard = max([0.0] + [v for v, _, _, kd in hv if kd == "hard"])
    goal = max([0.0] + [v for v, _, _, kd in hv if kd == "goal"])

    # ---- penalised rows at the optimal slacks; objective --------------------------------------------------------
    pv = []
    for fn, w, off in R["pen"]:
        val, (idx, gr) = fn(z)
        pv.append((kappa * (w * val - off), idx, kappa * w * np.asarray(gr, float)))
    s = np.array([max(0.0, p[0]) for p in pv])
    u = z[R["uidx"]]
    cost_terms = (kappa * R["wt"][:, None] * u * u).ravel()
    obj = math.fsum(list(cost_terms) + list(s))

    gobj = np.zeros(nzN)                      # gradient of the objective in z (the s-part is all ones)
    gobj[R["uidx"]] = 2 * kappa * R["wt"][:, None] * u
    scale_stat = max(1.0, float(np.abs(gobj).max()))

    # ---- candidates and the least-squares system ---------------------------------------------------------------------
    rhs_z = -gobj.copy()
    cols, vals, kinds = [], [], []             # column vectors in z (sparse: idx, grad), row value, kind
    band = []                                  # (column of nu, column of eta) per band row
    nu = np.zeros(len(pv))                     # multipliers of the penalised rows (filled in after the fit)
    nu_col = {}
    for v, (idx, gr), c, kd in hv:
        if v >= -tau:
            cols.append((idx, c * np.asarray(gr, float))); vals.append(v); kinds.append(kd)
    for i, (p, idx, gr) in enumerate(pv):
        if p > tau:                                           # s_i > tau: nu_i = 1
            np.add.at(rhs_z, idx, -gr)
            nu[i] = 1.0
        elif p >= -tau:                                       # in the band: nu_i and eta_i are candidates
            jn = len(cols)
            nu_col[i] = jn
            cols.append((idx, gr)); vals.append(p - s[i]); kinds.append("pen")
            cols.append((np.array([], int), np.array([]))); vals.append(-s[i]); kinds.append("slack")
            band.append((jn, jn + 1))
        # else: nu_i = 0, eta_i = 1 and the row drops out
    nE, nc, nb = E.shape[0], len(cols), len(band)
    A = np.zeros((nzN + nb + nc, nE + nc))
    A[:nzN, :nE] = E.T
    for j, (idx, gr) in enumerate(cols):
        np.add.at(A[:nzN, nE + j], idx, gr)
    b = np.zeros(nzN + nb + nc)
    b[:nzN] = rhs_z
    for r, (jn, je) in enumerate(band):
        A[nzN + r, nE + jn] = A[nzN + r, nE + je] = 1.0
        b[nzN + r] = 1.0
    for j in range(nc):
        A[nzN + nb + j, nE + j] = vals[j]
    lb = np.concatenate([np.full(nE, -np.inf), np.zeros(nc)])
    fit = so.lsq_linear(A, b, bounds=(lb, np.full(nE + nc, np.inf)), method="bvls", lsmr_tol=None, max_iter=None)
    y = fit.x
    res = A @ y - b
    stat_z = float(np.abs(res[:nzN]).max()) / scale_stat
    worst_z = int(np.abs(res[:nzN]).argmax())
    stat_s = float(np.abs(res[nzN:nzN + nb]).max()) if nb else 0.0
    yc = y[nE:]
    for i, j in nu_col.items():
        nu[i] = yc[j]
    comp = _sum_ld(np.abs(yc * np.array(vals)))
    return dict(eq=eq, hard=hard, goal=goal, stat=max(stat_z, stat_s), stat_z=stat_z, stat_s=stat_s, comp=comp, obj=obj,
                stat_at=divmod(worst_z, n + m), n_pairs=2 * len(pv) + len(hv),
                n_cand=nc, n_band=nb, fit_shape=A.shape, y=yc, kinds=kinds, lam=y[:nE], nu=nu, n_pen=len(pv),
                n_pen_active=int(np.sum(np.array([p[0] for p in pv]) > -tau)) if pv else 0)


# Gates on a certificate, all in the scaled problem (kappa = 1 / max(1, omega) is already in every row and in the objective, so
# no further factor of omega): stationarity, complementarity, |E z - e|, hard / BoxGoal violation.  ALMOST (the interior point
# method's acceptable level) is held to ALMOST_FACTOR x these, the ratio tol_acc / tol = 1e-5 / 1e-8 of the stopping test.
GATES = dict(stat=1e-7, comp=1e-7, eq=1e-9, hard=1e-9, goal=1e-9)
ALMOST_FACTOR = 1e3
# The solvers stop on the MEAN complementarity, mu = sum_i lambda_i t_i / n_pairs <= 0.1 tol = 1e-9; the
# largest pair is not tested.  So the stopping test only guarantees sum_i lambda_i t_i <= n_pairs * STOP_MU, and one pair may
# carry nearly all of it: dubins_car, N = 64, a trip of problem 1 of config 3, has one x_min row 2.3e-4 from active with
# multiplier 3.2e-3 (7.4e-7 of the 8.9e-7 the test allows; device and oracle alike).  The complementarity gate is therefore
# max(1e-7, n_pairs * STOP_MU); the same bound caps the objective gap (primal minus optimal objective is at most the duality gap).
STOP_MU = 0.1 * 1e-8


def comp_gate(c):
    return max(GATES["comp"], c["n_pairs"] * STOP_MU)


def failures(c, factor=1.0):
    """The residuals of certificate `c` above factor x their gate: dict name -> (value, gate)."""
    gates = dict(GATES, comp=comp_gate(c))
    return {k: (c[k], factor * g) for k, g in gates.items() if not c[k] <= factor * g}
