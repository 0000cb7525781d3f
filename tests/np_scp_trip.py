"""One GuSTO trip from any (traj_prev, Delta, omega) under any SCP parameters, on the host: the oracle's pieces (cold subproblem,
convergence_metric, trust_region_ratio, convex_ineq_satisfied, cost_true) composed by a plain restatement of the verdict table of
solve_gusto_jump! (scp_gusto.jl:119-147), written from the Julia source:

    trust_region_satisfied = max_k |x_k - xprev_k|^2 - Delta <= 0           (:34-44; evaluated with the documented slack
                                                                             tr_tol * max(1, Delta), gusto_ipm_opts.tr_tol = 1e-6)
    if trust_region_satisfied:
        rho = trust_region_ratio_gusto(new, prev)                            (:124)
        rho > rho1:  InaccurateModel, reject, Delta <- beta_fail Delta, omega kept                    (:125-129)
        else:        accept, Delta <- rho < rho0 ? min(beta_succ Delta, Delta0) : Delta               (:131-132)
                     rows violated: ViolatesConstraints, omega <- gamma_fail omega; else OK, omega kept  (:133-140)
    else:            TrustRegionViolated, reject, Delta kept, omega <- gamma_fail omega               (:142-147)

The products are formed as one IEEE multiplication each, as on the device, so Delta and omega compare with ==.  `fault` restates
the table wrongly on purpose (tests/test_scp_params_cpu.py shows each fault is seen on the trips the GPU tests run)."""
import numpy as np

TR_TOL = 1e-6
OK, INACCURATE, VIOLATES, TR_VIOLATED = 1, 2, 3, 4
FAULTS = ("rho_swapped", "no_cap", "beta_fail_for_succ")


def verdict(sp, Delta, omega, max_d2, rho, cvx_sat, tr_tol=TR_TOL, fault=None):
    """the verdict table: dict(tr_sat, accept, scp_status, Delta_next, omega_next).  rho is read only where the trust region holds"""
    assert fault is None or fault in FAULTS
    Delta, omega = float(Delta), float(omega)
    rho0, rho1 = (sp.rho1, sp.rho0) if fault == "rho_swapped" else (sp.rho0, sp.rho1)
    beta_succ = sp.beta_fail if fault == "beta_fail_for_succ" else sp.beta_succ
    tr_sat = bool(max_d2 - Delta <= tr_tol * max(1.0, Delta))
    if tr_sat:
        if rho > rho1:
            status, accept, D, w = INACCURATE, False, sp.beta_fail * Delta, omega
        else:
            accept = True
            grown = beta_succ * Delta if fault == "no_cap" else min(beta_succ * Delta, sp.Delta0)
            D = grown if rho < rho0 else Delta
            status, w = (OK, omega) if cvx_sat else (VIOLATES, sp.gamma_fail * omega)
    else:
        status, accept, D, w = TR_VIOLATED, False, Delta, sp.gamma_fail * omega
    return dict(tr_sat=int(tr_sat), accept=int(accept), scp_status=status, Delta_next=float(D), omega_next=float(w))


def pieces(o, clearance, Xp, Up, Delta, omega):
    """everything of the trip that does not depend on the thresholds, from the oracle `o` (its problem set, its eps the set's):
    the cold subproblem around (Xp, Up) with toggle = Delta / 8 + clearance (:76, :156) and the post-solve quantities"""
    Delta, omega = float(Delta), float(omega)
    toggle = Delta / 8 + clearance
    c = o.subproblem(Xp, Up, Delta, omega, toggle)
    out = dict(Delta=Delta, omega=omega, X=c["X"], U=c["U"], obj=c["obj"], ipm_iters=c["iters"], solver_status=c["status"])
    if c["status"] not in (1, 2):
        return out
    X, U = c["X"], c["U"]
    out.update(conv=o.convergence_metric(X, Xp), max_d2=float((np.asarray(X - Xp) ** 2).sum(axis=1).max()),
               cvx_sat=int(o.convex_ineq_satisfied(X, Xp, Up, toggle)), rho=o.trust_region_ratio(X, U, Xp, Up),
               J_true=o.cost_true(U))
    return out


def trip(o, sp, clearance, Xp, Up, Delta, omega, tr_tol=TR_TOL, fault=None):
    """pieces + verdict: one whole trip under `sp` (the oracle `o` must have been created with the same sp: eps enters its rows)"""
    p = pieces(o, clearance, Xp, Up, Delta, omega)
    if p["solver_status"] in (1, 2):
        p.update(verdict(sp, Delta, omega, p["max_d2"], p["rho"], p["cvx_sat"], tr_tol, fault))
    return p
