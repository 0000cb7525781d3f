"""What a warm replan buys on the GPU, on the BASELINE batch of config 2 (freeflyerSE2, the table, 4096 queries, N = 50):

  python tools/replan_rate.py [--queries 4096] [--max-iter 30] [--reps 10] [--commit ID]

The queries are solved once from the straight line (the plans).  Then every query is replanned at knot 5 and at knot 25 from
x_now = X[knot] + p_q, p_q = positions +-0.02 m, velocities +-0.002 m/s from the first four doubles of
problems.splitmix64(0xC0FFEE + q), to the same goal in the time that is left, tf' = (1 - knot / 49) tf, two ways:
  warm   gusto_set_problems_replan from the handle that holds the plans + gusto_solve: the answered queries start from their
         shifted plan, the others from the straight line
  cold   gusto_set_problems with X0 = NULL + gusto_solve: every query from the straight line
on a handle of N = 50 and on one of N = 25 (the plans resampled, Ns = 50 -> N = 25).  Per way, over the queries the first solve
answered: the successful count, the SCP and interior-point iterations, the trips of the longest problem, of the median, 90th and
99th percentile problem, the problems that ran into max_iter and the most interior-point iterations of one problem (the batch's
time follows its longest problem); the same counts over all queries (_all); the GPU time of the solve
(gusto_last_solve_ms) and of the warm seeding (gusto_last_replan_ms), HIP events on the handle's stream, each the median of --reps
runs after one warm-up run of the same shapes.  The results of a run do not depend on the repetition (the solves are
deterministic): the counts are asserted equal across them.  Lines of JSON, the first with the date and the commit;
profiles/replan.txt holds them."""
import argparse
import datetime
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import gusto_jl_amd as g  # noqa: E402


def perturbations(Q):
    p = np.zeros((Q, 6))
    for q in range(Q):
        gen = g.problems.splitmix64(0xC0FFEE + q)
        r = [next(gen) for _ in range(4)]
        p[q, 0:2] = [0.02 * (2 * r[0] - 1), 0.02 * (2 * r[1] - 1)]
        p[q, 3:5] = [0.002 * (2 * r[2] - 1), 0.002 * (2 * r[3] - 1)]
    return p


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    P, H = g.problems, g.host
    Q, Ns = args.queries, 50
    env = P.freeflyer_env()
    x0, glo, ghi, tf = P.freeflyer_batch(Q)
    pert = perturbations(Q)
    src = g.BatchSolver(g.FREEFLYER_SE2, Ns, Q, hist_cap=H._hist_cap(args.max_iter), boxes=env)
    src.set_problems(x0, glo, ghi, tf)
    src.solve(args.max_iter)
    st = src.status()
    ok = st["converged"] & st["successful"]
    X, _ = src.traj()
    print(json.dumps(dict(tool="tools/replan_rate.py", date=datetime.date.today().isoformat(), commit=args.commit,
                          device=torch.cuda.get_device_name(0), model="FREEFLYER_SE2", queries=Q, Ns=Ns, max_iter=args.max_iter,
                          reps=args.reps, warmup=1, first_solve=dict(answered=int(ok.sum()), scp_iters=int(st["iterations"].sum()),
                                                                     longest=int(st["iterations"].max()), solve_ms=round(src.last_solve_ms(), 3)))),
          flush=True)

    def figures(s):
        r = s.status()
        return dict(successful=int((r["converged"] & r["successful"])[ok].sum()), scp_iters=int(r["iterations"][ok].sum()),
                    ipm_iters=int(r["ipm_iters"][ok].sum()), longest=int(r["iterations"][ok].max()),
                    trips_p50_p90_p99=[int(v) for v in np.percentile(r["iterations"][ok], [50, 90, 99], method="higher")],
                    at_max_iter=int((r["iterations"][ok] >= args.max_iter).sum()), longest_ipm_iters=int(r["ipm_iters"][ok].max()),
                    successful_all=int((r["converged"] & r["successful"]).sum()), scp_iters_all=int(r["iterations"].sum()),
                    longest_all=int(r["iterations"].max()), solve_ms=s.last_solve_ms())

    for N in (50, 25):
        s = g.BatchSolver(g.FREEFLYER_SE2, N, Q, hist_cap=H._hist_cap(args.max_iter), boxes=env)
        for knot in (5, 25):
            tau = knot / (Ns - 1)
            x_now = X[:, knot] + pert

            def warm():
                s.set_problems_replan(tau, x_now, src=src)
                ms = s.last_replan_ms()
                s.solve(args.max_iter)
                return dict(figures(s), replan_ms=ms, seeded=int(s.replan_info()["seeded"].sum()))

            def cold():
                s.set_problems(x_now, glo, ghi, (1 - tau) * tf)
                s.solve(args.max_iter)
                return dict(figures(s), replan_ms=0.0)

            for name, run in (("warm", warm), ("cold", cold)):
                runs = [run() for _ in range(args.reps + 1)][1:]
                out = dict(runs[0], start=name, N=N, knot=knot)
                for r in runs[1:]:
                    assert all(r[k] == runs[0][k] for k in r if not k.endswith("_ms")), (name, r, runs[0])
                for k in ("solve_ms", "replan_ms"):
                    v = [r[k] for r in runs]
                    out[k] = round(statistics.median(v), 3)
                    out[k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
                print(json.dumps(out), flush=True)
        s.close()
    src.close()


if __name__ == "__main__":
    main()
