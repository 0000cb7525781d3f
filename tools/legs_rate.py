"""What the goal timeline answers and costs on the GPU, on the BASELINE batch of config 2 (freeflyerSE2, the table, 4096 queries,
N = 50, tf = 200 s) with the timeline of the study (tests/test_legs_cpu.py): waypoint l of query q is the start of query
(q + l + 1) mod Q, L = 3 goals equally spaced in time:

  python tools/legs_rate.py [--queries 4096] [--legs 3] [--max-iter 30] [--reps 5] [--commit ID]

Three runs, alternated in the same process after one warm-up of each, medians of --reps with [min, max] next to them:
  positions/sequential  the waypoints pin the position entries only: gusto_legs_begin, then per round gusto_solve +
                        gusto_legs_advance on ONE handle of `queries` problems
  points/sequential     the waypoints pin the whole start state of that query: the same three launches
  points/parallel       ... and PARALLEL's one launch of queries x legs problems and its one advance
Per run: the queries DONE and the failures per leg; the largest gap and arrive over the DONE queries; per round the queries
flying, the GuSTO trips and interior-point iterations of the round's solve, gusto_last_solve_ms and gusto_last_legs_ms of the
advance behind it (copies, both kernels and the status read-back), and gusto_last_legs_ms of begin.  The counts do not depend on
the repetition (asserted).  Lines of JSON, the first with the date and the commit; profiles/legs.txt holds them."""
import argparse
import datetime
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import gusto_jl_amd as g  # noqa: E402


def timeline(Q, L, full_points):
    """the study's timeline: (x_init [Q, n], lo, hi [Q, L, n], T [Q, L])"""
    x0, glo, ghi, tf = g.problems.freeflyer_batch(Q)
    lo, hi = np.full((Q, L, 6), -np.inf), np.full((Q, L, 6), np.inf)
    for l in range(L - 1):
        w = x0[(np.arange(Q) + l + 1) % Q]
        sel = slice(0, 6) if full_points else slice(0, 2)
        lo[:, l, sel] = hi[:, l, sel] = w[:, sel]
    lo[:, L - 1], hi[:, L - 1] = glo, ghi
    return x0, lo, hi, tf[:, None] * np.arange(1, L + 1)[None, :] / L


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--legs", type=int, default=3)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    P, H, T = g.problems, g.host, g._capi
    Q, L, N = args.queries, args.legs, 50
    s = g.BatchSolver(g.FREEFLYER_SE2, N, Q * L, hist_cap=H._hist_cap(args.max_iter), boxes=P.freeflyer_env())
    lines = {False: timeline(Q, L, False), True: timeline(Q, L, True)}

    def fly(full_points, mode):
        assert s.legs_begin(*lines[full_points], mode=mode) == mode
        out = dict(begin_ms=s.last_legs_ms(), rounds=[])
        left = Q
        while left:
            s.solve(args.max_iter)
            st = s.status()
            row = dict(flying=left, problems=s.B, eligible=int((st["converged"] & st["successful"]).sum()),
                       trips=int(st["iterations"].sum()), ipm_iters=int(st["ipm_iters"].sum()), solve_ms=s.last_solve_ms())
            left = s.legs_advance()
            row["advance_ms"] = s.last_legs_ms()
            out["rounds"].append(row)
        r = s.legs_info()
        done = r["status"] == T.LEGS_DONE
        out.update(done=int(done.sum()), failed_per_leg=[int((r["failed_leg"] == l).sum()) for l in range(L)],
                   max_gap=float(r["gap"][done].max()), max_arrive=float(r["arrive"][done].max()),
                   J_total_mean=round(float(r["J_total"][done].mean()), 6))
        return out

    print(json.dumps(dict(tool="tools/legs_rate.py", date=datetime.date.today().isoformat(), commit=args.commit,
                          device=torch.cuda.get_device_name(0), config=2, model="FREEFLYER_SE2", queries=Q, legs=L, N=N,
                          max_iter=args.max_iter, reps=args.reps, tf_of_the_config=float(lines[False][3][0, -1]))))
    runs = (("positions", False, "sequential"), ("points", True, "sequential"), ("points", True, "parallel"))
    for _, fp, m in runs:      # warm-up: every shape once
        fly(fp, m)
    res = {r: [] for r in runs}
    for _ in range(args.reps):
        for r in runs:
            res[r].append(fly(r[1], r[2]))
    counts = ("done", "failed_per_leg", "max_gap", "max_arrive", "J_total_mean")
    for r in runs:
        first = res[r][0]
        for o in res[r][1:]:
            assert all(o[k] == first[k] for k in counts) and len(o["rounds"]) == len(first["rounds"])
            assert all(a[k] == b[k] for a, b in zip(o["rounds"], first["rounds"]) for k in ("flying", "eligible", "trips", "ipm_iters"))
        med = lambda v: dict(median=round(statistics.median(v), 3), min_max=[round(min(v), 3), round(max(v), 3)])
        row = dict(waypoints=r[0], mode=r[2], **{k: first[k] for k in counts}, begin_ms=med([o["begin_ms"] for o in res[r]]), per_round=[])
        for i, r0 in enumerate(first["rounds"]):
            row["per_round"].append(dict(round=i, **{k: r0[k] for k in ("flying", "problems", "eligible", "trips", "ipm_iters")},
                                         solve_ms=med([o["rounds"][i]["solve_ms"] for o in res[r]]),
                                         advance_ms=med([o["rounds"][i]["advance_ms"] for o in res[r]])))
        row["solve_ms_total"] = round(sum(x["solve_ms"]["median"] for x in row["per_round"]), 3)
        row["legs_ms_total"] = round(row["begin_ms"]["median"] + sum(x["advance_ms"]["median"] for x in row["per_round"]), 3)
        print(json.dumps(row))
    s.close()


if __name__ == "__main__":
    main()
