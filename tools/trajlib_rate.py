"""What seeding from a trajectory library buys and costs on the GPU, on the BASELINE batch of config 2 (freeflyerSE2, the table, 4096
queries, N = 50):

  python tools/trajlib_rate.py [--queries 4096] [--library 4096] [--big 65536] [--max-iter 30] [--reps 10] [--commit ID]

The library: problems.freeflyer_batch(--library, first=100000) solved from the straight line on the device, the converged and
successful ones appended by gusto_trajlib_add.  The queries: problems.freeflyer_batch(--queries).  On ONE handle sized for K = 3:
  cold       gusto_set_problems + gusto_solve: every query from its straight line
  seeded K   gusto_set_problems_trajlib with K = 1 and K = 3 + gusto_solve (+ gusto_select_best for K = 3), with the search kernel
             in both forms (lds_tile = 1: a tile of feature rows shared through LDS, 0: every wavefront reads global memory)
Per way: the queries answered (converged and successful; K = 3: with a winner), the SCP iterations in total and of the longest
problem, the GPU time of the solve (gusto_last_solve_ms) and of the seeding (gusto_last_trajlib_ms, split into search and
retargeting by gusto_dev_trajlib; HIP events on the handle's stream), each the median of --reps runs after one warm-up run of the
same shapes.  The solves are deterministic: the counts are asserted equal across the runs.
Then the search alone at --big entries: the library's entries replicated with a jitter of +-0.05 m on x_init (gusto_trajlib_get,
gusto_trajlib_add_host), both forms of the kernel, K = 1 and 3, and at the weights on the position only (32 B per entry).
Lines of JSON, the first with the date and the commit; profiles/trajlib.txt holds them."""
import argparse
import datetime
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import gusto_jl_amd as g  # noqa: E402


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=4096)
    ap.add_argument("--library", type=int, default=4096)
    ap.add_argument("--big", type=int, default=65536)
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--commit", default="unknown")
    args = ap.parse_args()
    P, H = g.problems, g.host
    Q, N, KMAX = args.queries, 50, 3
    x0, glo, ghi, tf = P.freeflyer_batch(Q)
    s = g.BatchSolver(g.FREEFLYER_SE2, N, max(Q * KMAX, args.library), hist_cap=H._hist_cap(args.max_iter), boxes=P.freeflyer_env())
    print(json.dumps(dict(tool="tools/trajlib_rate.py", date=datetime.date.today().isoformat(), commit=args.commit,
                          device=torch.cuda.get_device_name(0), model="FREEFLYER_SE2", queries=Q, N=N, max_iter=args.max_iter,
                          reps=args.reps, warmup=1)), flush=True)

    # the library
    lx, ll, lh, lt = P.freeflyer_batch(args.library, first=100000)
    s.set_problems(lx, ll, lh, lt)
    s.solve(args.max_iter)
    libs = {1: g.TrajLib(g.FREEFLYER_SE2, N, args.library), 0: g.TrajLib(g.FREEFLYER_SE2, N, args.library, lds_tile=0)}
    add_ms = []
    for lib in libs.values():
        for _ in range(3):
            lib.clear()
            t = time.perf_counter()
            added = lib.add_from(s)
            add_ms.append((time.perf_counter() - t) * 1e3)
    print(json.dumps(dict(stage="library", problems=args.library, entries=added, solve_ms=round(s.last_solve_ms(), 3),
                          add_wall_ms_min=round(min(add_ms), 3), feature_bytes_per_entry=96)), flush=True)

    def counts(K):
        st = s.status()
        if K == 1:
            answered = int((st["converged"].astype(bool) & st["successful"].astype(bool)).sum())
        else:
            answered = int((s.select_best(K)["winner"] >= 0).sum())
        return dict(answered=answered, problems=s.B, scp_iterations=int(st["iterations"].sum()), longest=int(st["iterations"].max()),
                    ipm_iterations=int(st["ipm_iters"].sum()), solve_ms=s.last_solve_ms())

    def cold():
        s.set_problems(x0, glo, ghi, tf)
        s.solve(args.max_iter)
        return dict(counts(1), way="cold")

    def seeded(K, tile):
        def run():
            s.set_problems_trajlib(libs[tile], x0, glo, ghi, tf, K)
            seed_ms, (search_ms, retarget_ms) = s.last_trajlib_ms(), s.trajlib_phase_ms()
            found = int(s.trajlib_seeds()["n_found"].sum())
            s.solve(args.max_iter)
            return dict(counts(K), way="seeded", K=K, lds_tile=tile, seeds_found=found, seed_ms=seed_ms, search_ms=search_ms,
                        retarget_ms=retarget_ms)
        return run

    def median_of(run, reps):
        runs = [run() for _ in range(reps + 1)][1:]
        out = dict(runs[0])
        for r in runs[1:]:
            assert all(r[k] == runs[0][k] for k in r if not k.endswith("_ms")), (r, runs[0])
        for k in [k for k in out if k.endswith("_ms")]:
            v = [r[k] for r in runs]
            out[k] = round(statistics.median(v), 4)
            out[k + "_min_max"] = [round(min(v), 4), round(max(v), 4)]
        return out

    for run in (cold, seeded(1, 1), seeded(1, 0), seeded(3, 1), seeded(3, 0)):
        print(json.dumps(median_of(run, args.reps)), flush=True)

    # the search alone on a large library
    got = libs[1].get()
    L0 = len(got["tf"])
    idx = np.arange(args.big) % L0
    rng = np.random.default_rng(0)
    xi = got["x_init"][idx].copy()
    xi[L0:, :2] += rng.uniform(-0.05, 0.05, (args.big - L0, 2))
    for lib in libs.values():
        lib.close()
    for name, w in (("default", {}), ("position", dict(w_init=[1, 1, 0, 0, 0, 0], w_goal=[1, 1, 0, 0, 0, 0]))):
        for tile in (1, 0):
            big = g.TrajLib(g.FREEFLYER_SE2, N, args.big, lds_tile=tile, **w)
            for c in range(0, args.big, 8192):
                j = idx[c:c + 8192]
                big.add_host(xi[c:c + 8192], got["goal_c"][j], got["goal_c"][j], got["tf"][j], got["X"][j], got["U"][j])
            for K in (1, 3):
                def run():
                    s.set_problems_trajlib(big, x0, glo, ghi, tf, K)
                    a, b = s.trajlib_phase_ms()
                    return dict(stage="search alone", weights=name, feature_bytes_per_entry=96 if name == "default" else 32,
                                entries=len(big), queries=Q, K=K, lds_tile=tile, search_ms=a, retarget_ms=b)
                print(json.dumps(median_of(run, args.reps)), flush=True)
            big.close()
    s.close()


if __name__ == "__main__":
    main()
