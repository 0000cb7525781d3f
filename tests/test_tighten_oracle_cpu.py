"""The chance loop of host.solve_SCP_chance_batch restated on the CPU oracle, without a GPU: the first 48 table queries of
problems.freeflyer_batch at N = 50, solved by oracle/ from the straight line, analysed with tests/np_tvlqr.py and
tests/np_lincov.py, tightened with tests/np_tighten.py (kappa = 3, one round: cover, grow, re-solve from the own plan and from the
straight line where that fails).  Asserted: every query reported met has np_lincov's min_z_obs >= kappa over all components on
the base set and no negative distance in np_verify, and strictly more queries are met after the loop than before.  The counts
are printed, not asserted (profiles/tighten.txt)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))

import gusto_jl_amd as g
import gusto_oracle as go
import np_lincov as NL
import np_tighten as NT
import np_tvlqr as T
import np_verify as V

Q, N, KAPPA = 48, 50, 3.0
DX0 = np.array([.02, .02, .02, .002, .002, .002])
DU_WHITE = 0.0074


def analyse(X, U, tf, boxes):
    AB, K, _ = T.tvlqr(0, X, U, tf, np.ones(6), np.ones(3), np.ones(6), dt_min=0.1)
    lc = NL.lincov(0, X, U, AB, K, None, DX0, 0.0, DU_WHITE, boxes=boxes)
    D = V.knot_distances(0, X, *V.obstacles(boxes, None))
    return lc, bool((D >= 0).all())


def solve(x0, lo, hi, tf, boxes, X0=None, U0=None):
    o = go.Oracle(go.FREEFLYER_SE2, N, boxes=boxes)
    o.set_problem(x0, lo, hi, tf, X0, U0)
    r = o.solve(30)
    return (r["converged"] and r["successful"]), r["X"], r["U"], r["stop_reason"]


def test_one_round_of_the_loop_on_the_cpu_oracle():
    P = g.problems
    base = P.freeflyer_env()
    x0, lo, hi, tf = P.freeflyer_batch(Q)
    plans, met0, met1, lost, blocked = {}, [], [], [], []
    for q in range(Q):
        ok, X, U, _ = solve(x0[q], lo[q], hi[q], tf[q], base)
        if ok:
            plans[q] = (X, U)
    for q, (X, U) in plans.items():
        lc, free = analyse(X, U, tf[q], base)
        if lc["min_z_obs"] >= KAPPA and free:
            met0.append(q)
            met1.append(q)
            continue
        t = NT.tighten(0, X, lc["Sxx"], base, None, x0[q], lo[q], hi[q], kappa=KAPPA)
        if t["blocked"]:
            blocked.append(q)
            continue
        ok, X1, U1, _ = solve(x0[q], lo[q], hi[q], tf[q], t["boxes"], X, U)
        if not ok:
            ok, X1, U1, _ = solve(x0[q], lo[q], hi[q], tf[q], t["boxes"])
        if not ok:
            lost.append(q)
            continue
        lc1, free1 = analyse(X1, U1, tf[q], base)
        if lc1["status"] and lc1["min_z_obs"] >= KAPPA and free1:
            met1.append(q)
            D = V.knot_distances(0, X1, *V.obstacles(base, None))
            assert (D >= 0).all() and lc1["min_z_obs"] >= KAPPA
    print(f"answered {len(plans)} of {Q}; met before {len(met0)}, after {len(met1)}; blocked {len(blocked)}, lost re-solves {len(lost)}")
    assert len(met1) > len(met0)
