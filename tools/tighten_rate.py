"""What planning to a margin in standard deviations costs and buys on the GPU, on the BASELINE batch of config 2 (freeflyerSE2,
the table, 4096 queries, N = 50):

  python tools/tighten_rate.py [--queries 4096] [--kappa 3] [--rounds 3] [--max-iter 30] [--commit ID]

host.solve_SCP_chance_batch with dx0 = (.02, .02, .02, .002, .002, .002), du0 = 0, du_white = 0.0074, Q = R = Qf = 1,
dt_min = 0.1: the solve from the straight line, then per round gusto_tvlqr, gusto_lincov (store_S = 1), gusto_tighten_env from the
base table for the answered queries below kappa, the re-solve from the own plans and once more from the straight line for the
ones that pass loses.  Lines of JSON, the first with the date and the commit, then the counts before the first round (answered,
met), one line per round -- tried, blocked, second pass, lost, the queries at or above kappa on the base set when the round
began (done_before), the SCP iterations of the re-solves, and the GPU milliseconds of gusto_tighten_env beside gusto_lincov and
the solves of the same run (HIP events on the handle's stream, one run: the counts are deterministic, the times are not
repeated) -- and the final counts.  profiles/tighten.txt holds them."""
import argparse
import datetime
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import gusto_jl_amd as g  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--kappa", type=float, default=3.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    H, P = g.host, g.problems
    Q = args.queries
    model, env = H.FreeflyerSE2(), H.Environment(P.freeflyer_env())
    x0, glo, _, tf = P.freeflyer_batch(Q)
    TOPs = []
    for b in range(Q):
        gs = H.GoalSet()
        H.add_goal(gs, H.Goal(H.PointGoal(glo[b]), tf[b], model))
        TOPs.append(H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, env, x0[b], gs), 50, tf[b], fixed_final_time=True))
    TOSs = [H.TrajectoryOptimizationSolution(t) for t in TOPs]
    lco = dict(dx0=[.02, .02, .02, .002, .002, .002], du0=0.0, du_white=0.0074)
    out = H.solve_SCP_chance_batch(TOSs, TOPs, kappa=args.kappa, rounds=args.rounds, lincov_opts=lco,
                                   tvlqr_opts=dict(Q=1.0, R=1.0, Qf=1.0, dt_min=0.1), max_iter=args.max_iter)
    print(json.dumps(dict(date=datetime.date.today().isoformat(), commit=args.commit, queries=Q, kappa=args.kappa, rounds=args.rounds,
                          max_iter=args.max_iter)))
    print(json.dumps(dict(stage="before", answered=int(out["answered"].sum()), met=int(out["met_before"].sum()))))
    for i, r in enumerate(out["rounds"]):
        fin = r["min_z_base"][r["min_z_base"] != 0]
        print(json.dumps(dict(stage="round", round=i, tried=int(r["tried"].sum()), blocked=int((r["blocked"] & (r["min_z_base"] != 0)).sum()),
                              second_pass=int(r["second_pass"].sum()), lost=int(r["lost"].sum()),
                              at_or_above_kappa=int((fin >= args.kappa).sum()), analysed=int(len(fin)),
                              scp_iterations=int(r["iterations"].sum()), scp_iterations_max=int(r["iterations"].max()),
                              max_margin=float(r["max_margin"].max()), tighten_ms=round(r["tighten_ms"], 4),
                              lincov_ms=round(r["lincov_ms"], 4), solve_ms=round(r["solve_ms"], 3))))
    zz = out["min_z_obs"][out["met"]]
    print(json.dumps(dict(stage="after", answered=int(out["answered"].sum()), met=int(out["met"].sum()),
                          min_z_obs_of_met=[float(zz.min()), float(np.median(zz)), float(zz.max())] if len(zz) else [],
                          base_restored=bool(len(out["env"][0]) == 1 and np.array_equal(out["env"][0][0], P.freeflyer_env())))))


if __name__ == "__main__":
    main()
