"""GPU time of gusto_simulate next to the solve and the verification of the same batch, for BASELINE configs 2 (freeflyerSE2,
4096 problems) and 4 (astrobeeSE3, 8192 problems), N = 50, S = 64 samples per problem:

  python tools/simulate_time.py [--configs 2 4] [--batch B] [--samples 64] [--max-iter 30]

Per config: gusto_last_solve_ms, gusto_last_verify_ms and the median of five warm calls of gusto_last_simulate_ms -- with
dense_collision 1 and 0, and with store_knots -- in the same process, and the time per RK4 step per sample of gusto_simulate
and of gusto_verify (a verify "sample" is one knot interval of one problem): verify's per-step cost is the yardstick the
roll-out kernel is read against, since both do a step and the same distance loop.  One JSON line per config."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import gusto_jl_amd as g  # noqa: E402

CONFIGS = {2: ("FREEFLYER_SE2", 4096), 4: ("ASTROBEE_SE3", 8192)}
N = 50


def problems(cfg, B):
    P = g.problems
    if cfg == 2:
        return P.freeflyer_env(), None, P.freeflyer_batch(B)
    bx, sp = P.iss_corner_env(True)
    return bx, sp, P.astrobee_se3_batch(B)


def median5(s, opts):
    s.simulate(opts)                                   # (the first call allocates and pays the cold instruction caches)
    ms = []
    for _ in range(5):
        s._chk(s.L.gusto_simulate(s.h, None, None, None, None, g._capi.C.byref(s.simulate_opts(opts))), "simulate")
        ms.append(s.last_simulate_ms())
    return statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=0, help="override the config's batch size")
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--max-iter", type=int, default=30)
    args = ap.parse_args()
    for cfg in args.configs:
        name, B = CONFIGS[cfg]
        B = args.batch or B
        model = getattr(g, name)
        boxes, spheres, (x0, glo, ghi, tf) = problems(cfg, B)
        s = g.BatchSolver(model, N, B, hist_cap=64, boxes=boxes, spheres=spheres)
        s.set_problems(x0, glo, ghi, tf)
        s.solve(args.max_iter)
        s.verify()
        ver = []
        for _ in range(5):
            s.verify()
            ver.append(s.last_verify_ms())
        s.tvlqr()
        S = args.samples
        nstep = np.ceil(tf / (N - 1) / 0.1)
        steps = float(nstep.sum()) * (N - 1)            # RK4 steps of one sample of every problem = of one gusto_verify
        dense = median5(s, dict(n_samples=S))
        knots_only = median5(s, dict(n_samples=S, dense_collision=0))
        stored = median5(s, dict(n_samples=S, store_knots=1))
        r = s.get_simulate()
        out = dict(config=cfg, model=name, problems=B, N=N, samples=S, nstep=int(nstep.max()), solve_ms=round(s.last_solve_ms(), 3),
                   verify_median5_ms=round(statistics.median(ver), 3), simulate_median5_ms=round(dense, 3),
                   simulate_dense_collision_0_ms=round(knots_only, 3), simulate_store_knots_ms=round(stored, 3),
                   ns_per_step_per_sample_simulate=round(1e6 * dense / (steps * S), 4),
                   ns_per_step_verify=round(1e6 * statistics.median(ver) / steps, 4),
                   n_free=int(r["n_free"].sum()), n_finite=int(r["n_finite"].sum()))
        print(json.dumps(out), flush=True)
        s.close()


if __name__ == "__main__":
    main()
