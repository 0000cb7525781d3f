"""What the final-time search answers and costs on the GPU, on the BASELINE batch of config 2 (freeflyerSE2, the table, 4096
queries, N = 50), whose every query is solved at tf = 200 s:

  python tools/tfsearch_rate.py [--queries 4096] [--K 4] [--rounds 3] [--lo 4] [--hi 84] [--max-iter 30] [--reps 5] [--commit ID]

gusto_tfsearch_begin, then per round gusto_solve + gusto_tfsearch_update, on ONE handle of queries x K problems, in both seed
modes ("line", "incumbent"), alternated in the same process after one warm-up search of each.  Per mode: the queries answered and
the NONE, FLOOR and NONMONOTONE counts; the quartiles of tf_best; per round the queries still searching, the problems eligible,
the GuSTO trips and interior-point iterations of the round's solves, gusto_last_solve_ms and gusto_last_tfsearch_ms of the update
behind it (copies, update kernel, seed kernel and the status read-back; the library does not report the kernels apart), and
gusto_last_tfsearch_ms of begin: medians of --reps searches, [min, max] next to them.  The counts do not depend on the
repetition (asserted).  Lines of JSON, the first with the date and the commit; profiles/tfsearch.txt holds them."""
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
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lo", type=float, default=4.0)
    ap.add_argument("--hi", type=float, default=84.0)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    P, H, T = g.problems, g.host, g._capi
    Q, K, N = args.queries, args.K, 50
    x0, glo, ghi, tf = P.freeflyer_batch(Q)
    s = g.BatchSolver(g.FREEFLYER_SE2, N, Q * K, hist_cap=H._hist_cap(args.max_iter), boxes=P.freeflyer_env())

    def search(seed):
        s.tfsearch_begin(x0, glo, ghi, args.lo, args.hi, K=K, seed=seed)
        out = dict(begin_ms=s.last_tfsearch_ms(), rounds=[])
        left = Q
        for _ in range(args.rounds):
            s.solve(args.max_iter)
            st = s.status()
            row = dict(searching=left, eligible=int((st["converged"] & st["successful"]).sum()), trips=int(st["iterations"].sum()),
                       ipm_iters=int(st["ipm_iters"].sum()), solve_ms=s.last_solve_ms())
            left = s.tfsearch_update()
            row["update_ms"] = s.last_tfsearch_ms()
            out["rounds"].append(row)
            if left == 0:
                break
        r = s.tfsearch_info()
        have = r["round_found"] >= 0
        out.update(answered=int(have.sum()), none=int(((r["status"] & T.TFSEARCH_NONE) != 0).sum()),
                   done=int(((r["status"] & T.TFSEARCH_DONE) != 0).sum()), floor=int(((r["status"] & T.TFSEARCH_FLOOR) != 0).sum()),
                   nonmonotone=int(((r["status"] & T.TFSEARCH_NONMONOTONE) != 0).sum()),
                   tf_best_quartiles=[round(float(v), 3) for v in np.percentile(r["tf_best"][have], [0, 25, 50, 75, 100])],
                   tf_best_mean=round(float(r["tf_best"][have].mean()), 3),
                   width_max=round(float((r["hi"] - r["lo"])[have].max()), 4))
        return out

    print(json.dumps(dict(tool="tools/tfsearch_rate.py", date=datetime.date.today().isoformat(), commit=args.commit,
                          device=torch.cuda.get_device_name(0), config=2, model="FREEFLYER_SE2", queries=Q, K=K, problems=Q * K, N=N,
                          range=[args.lo, args.hi], rounds=args.rounds, max_iter=args.max_iter, reps=args.reps, tf_of_the_config=float(tf[0]))))
    modes = ("line", "incumbent")
    for m in modes:      # warm-up: every shape once
        search(m)
    runs = {m: [] for m in modes}
    for _ in range(args.reps):
        for m in modes:
            runs[m].append(search(m))
    counts = ("answered", "none", "done", "floor", "nonmonotone", "tf_best_quartiles", "tf_best_mean", "width_max")
    for m in modes:
        first = runs[m][0]
        for o in runs[m][1:]:
            assert all(o[k] == first[k] for k in counts) and len(o["rounds"]) == len(first["rounds"])
            assert all(a[k] == b[k] for a, b in zip(o["rounds"], first["rounds"]) for k in ("searching", "eligible", "trips", "ipm_iters"))
        med = lambda v: dict(median=round(statistics.median(v), 3), min_max=[round(min(v), 3), round(max(v), 3)])
        row = dict(seed=m, **{k: first[k] for k in counts}, begin_ms=med([o["begin_ms"] for o in runs[m]]), per_round=[])
        for i, r0 in enumerate(first["rounds"]):
            row["per_round"].append(dict(round=i, **{k: r0[k] for k in ("searching", "eligible", "trips", "ipm_iters")},
                                         solve_ms=med([o["rounds"][i]["solve_ms"] for o in runs[m]]),
                                         update_ms=med([o["rounds"][i]["update_ms"] for o in runs[m]])))
        row["solve_ms_total"] = round(sum(r["solve_ms"]["median"] for r in row["per_round"]), 3)
        row["tfsearch_ms_total"] = round(row["begin_ms"]["median"] + sum(r["update_ms"]["median"] for r in row["per_round"]), 3)
        print(json.dumps(row))
    s.close()


if __name__ == "__main__":
    main()
