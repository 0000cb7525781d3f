"""What a roadmap seed buys and costs on the GPU, on the BASELINE batch of config 2 (freeflyerSE2, the table, 4096 queries, N = 50)
or of config 4 (AstrobeeSE3, the ISS corner, N = 50):

  python tools/roadmap_rate.py [--config 2|4] [--queries 4096] [--max-iter 30] [--reps 10] [--commit ID]

Four ways to answer the same queries, on ONE handle sized for the largest batch:
  straight        gusto_set_problems + gusto_solve: every query from its straight line
  roadmap_k1      gusto_set_problems_roadmap with K = 1 + gusto_solve
  roadmap_k2      ... with K = 2 + gusto_solve + gusto_select_best
  roadmap_retry   roadmap_k1, then the default fan of five for the queries it leaves unanswered
Per way: the queries answered (converged and successful), the GPU time of the solves (gusto_last_solve_ms) and of the seeding
(gusto_last_roadmap_ms and its split into graph, search and seed from the report), each the median of --reps runs after one warm-up
run of the same shapes; the seeds' status counts; the GuSTO trips of all problems.  The results of a run do not depend on the
repetition: the counts are asserted equal across them.  Lines of JSON, the first with the date and the commit;
profiles/roadmap.txt holds them."""
import argparse
import datetime
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import gusto_jl_amd as g  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=2, choices=(2, 4))
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    P, H = g.problems, g.host
    Q, N = args.queries, 50
    if args.config == 2:
        model, name = g.FREEFLYER_SE2, "FREEFLYER_SE2"
        x0, glo, ghi, tf = P.freeflyer_batch(Q)
        boxes, spheres = P.freeflyer_env(), None
    else:
        model, name = g.ASTROBEE_SE3, "ASTROBEE_SE3"
        x0, glo, ghi, tf = P.astrobee_se3_batch(Q)
        boxes, spheres = P.iss_corner_env(True)
    fan = H.default_fan(model)
    Kf = len(fan)
    s = g.BatchSolver(model, N, max(2 * Q, Kf), hist_cap=H._hist_cap(args.max_iter), boxes=boxes, spheres=spheres)
    opts = g.default_roadmap_opts(model)
    ms_keys = ("solve_ms", "roadmap_ms", "graph_ms", "search_ms", "seed_ms")

    def solved():
        s.solve(args.max_iter)
        st = s.status()
        return st["converged"] & st["successful"], int(st["iterations"].sum())

    def straight():
        s.set_problems(x0, glo, ghi, tf)
        ok, trips = solved()
        return dict(answered=int(ok.sum()), problems=Q, trips=trips, solve_ms=s.last_solve_ms(), roadmap_ms=0.0, graph_ms=0.0, search_ms=0.0,
                    seed_ms=0.0)

    def roadmap(K):
        s.set_problems_roadmap(x0, glo, ghi, tf, K=K)
        rep, ms = s.roadmap_info(), s.last_roadmap_ms()
        ok, trips = solved()
        if K > 1:
            ok = s.select_best(K)["winner"] >= 0
        counts = np.bincount(rep["status"], minlength=6)
        return dict(answered=int(ok.sum()), problems=Q * K, trips=trips, solve_ms=s.last_solve_ms(), roadmap_ms=ms, graph_ms=float(rep["stage_ms"][0]),
                    search_ms=float(rep["stage_ms"][1]), seed_ms=float(rep["stage_ms"][2]),
                    seeds={g._capi.ROADMAP_STATUS[i]: int(c) for i, c in enumerate(counts) if c}), ok

    def retry():
        r, ok = roadmap(1)
        again = np.flatnonzero(~ok)
        per = max(1, (2 * Q) // Kf)   # queries per fanned launch on this handle
        for c in range(0, len(again), per):
            qs = again[c:c + per]
            s.set_problems_multistart(x0[qs], glo[qs], ghi[qs], tf[qs], fan)
            s.solve(args.max_iter)
            r["solve_ms"] += s.last_solve_ms()
            r["trips"] += int(s.status()["iterations"].sum())
            r["answered"] += int((s.select_best(Kf)["winner"] >= 0).sum())
        r.update(problems=Q + Kf * len(again), retried_queries=int(len(again)))
        return r

    print(json.dumps(dict(tool="tools/roadmap_rate.py", date=datetime.date.today().isoformat(), commit=args.commit,
                          device=torch.cuda.get_device_name(0), config=args.config, model=name, queries=Q, N=N, max_iter=args.max_iter,
                          inflate=opts.inflate, pad=opts.pad, fan=fan.tolist(), reps=args.reps, warmup=1)), flush=True)
    for pol, run in (("straight", straight), ("roadmap_k1", lambda: roadmap(1)[0]), ("roadmap_k2", lambda: roadmap(2)[0]), ("roadmap_retry", retry)):
        runs = [run() for _ in range(args.reps + 1)][1:]
        out = dict(runs[0], policy=pol)
        for r in runs[1:]:
            assert all(r[k] == runs[0][k] for k in r if not k.endswith("_ms")), (pol, r, runs[0])
        for k in ms_keys:
            v = [r[k] for r in runs]
            out[k] = round(statistics.median(v), 3)
            out[k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
        print(json.dumps(out), flush=True)
    s.close()


if __name__ == "__main__":
    main()
