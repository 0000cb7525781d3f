"""What a fan of starts buys and costs on the GPU, on the BASELINE batch of config 2 (freeflyerSE2, the table, 4096 queries, N = 50):

  python tools/multistart_rate.py [--queries 4096] [--max-iter 30] [--reps 10] [--commit ID]

Three ways to answer the same queries, on ONE handle sized for the fanned batch:
  straight   gusto_set_problems + gusto_solve: every query from its straight line
  all        gusto_set_problems_multistart with the default fan of five + gusto_solve + gusto_select_best
  retry      straight, then the fan for the queries that are not successful only
Per way: the queries answered (converged and successful), the GPU time of the solves (gusto_last_solve_ms, HIP events on the
handle's stream) and of the selection (events on the same stream around gusto_select_best, which ends in a synchronise; its copies
of the report are outside), each the median of --reps runs after one warm-up run of the same shapes; and the wins per start.  The
results of a run do not depend on the repetition (the solves are deterministic): the counts are asserted equal across them.
Lines of JSON, the first with the date and the commit; profiles/multistart.txt holds them."""
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
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    P, H = g.problems, g.host
    Q, N = args.queries, 50
    fan = H.default_fan(g.FREEFLYER_SE2)
    K = len(fan)
    x0, glo, ghi, tf = P.freeflyer_batch(Q)
    s = g.BatchSolver(g.FREEFLYER_SE2, N, Q * K, hist_cap=H._hist_cap(args.max_iter), boxes=P.freeflyer_env())
    stream = torch.cuda.Stream()
    s._chk(s.L.gusto_set_stream(s.h, stream.cuda_stream), "set_stream")

    def timed_select():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        s._chk(s.L.gusto_select_best(s.h, K, None, None), "select_best")
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1), s.get_best(s.B // K)

    def straight():
        s.set_problems(x0, glo, ghi, tf)
        s.solve(args.max_iter)
        st = s.status()
        ok = st["converged"] & st["successful"]
        return dict(answered=int(ok.sum()), solve_ms=s.last_solve_ms(), select_ms=0.0, problems=Q), ok

    def fanned(qs):
        s.set_problems_multistart(x0[qs], glo[qs], ghi[qs], tf[qs], fan)
        s.solve(args.max_iter)
        ms = s.last_solve_ms()
        sel_ms, best = timed_select()
        return ms, sel_ms, best

    def run_all():
        ms, sel_ms, best = fanned(np.arange(Q))
        wins = np.bincount(best["winner"][best["winner"] >= 0], minlength=K)
        return dict(answered=int((best["winner"] >= 0).sum()), solve_ms=ms, select_ms=sel_ms, problems=Q * K, wins_per_start=wins.tolist())

    def run_retry():
        r, ok = straight()
        again = np.flatnonzero(~ok)
        wins = np.zeros(K, dtype=int)
        wins[0] = int(ok.sum())
        if len(again):
            ms, sel_ms, best = fanned(again)
            r["solve_ms"] += ms
            r["select_ms"] += sel_ms
            r["answered"] += int((best["winner"] >= 0).sum())
            wins += np.bincount(best["winner"][best["winner"] >= 0], minlength=K)
        r.update(problems=Q + K * len(again), retried_queries=int(len(again)), wins_per_start=wins.tolist())
        return r

    print(json.dumps(dict(tool="tools/multistart_rate.py", date=datetime.date.today().isoformat(), commit=args.commit,
                          device=torch.cuda.get_device_name(0), model="FREEFLYER_SE2", queries=Q, N=N, max_iter=args.max_iter,
                          fan=fan.tolist(), reps=args.reps, warmup=1)), flush=True)
    for name, run in (("straight", lambda: straight()[0]), ("all", run_all), ("retry", run_retry)):
        runs = [run() for _ in range(args.reps + 1)][1:]
        out = dict(runs[0], policy=name)
        for r in runs[1:]:
            assert all(r[k] == runs[0][k] for k in r if not k.endswith("_ms")), (name, r, runs[0])
        for k in ("solve_ms", "select_ms"):
            v = [r[k] for r in runs]
            out[k] = round(statistics.median(v), 3)
            out[k + "_min_max"] = [round(min(v), 3), round(max(v), 3)]
        print(json.dumps(out), flush=True)
    s.close()


if __name__ == "__main__":
    main()
