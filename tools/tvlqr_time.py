"""GPU time of gusto_tvlqr next to the solve that produced the batch, for BASELINE configs 2 (freeflyerSE2, 4096 problems) and 4
(astrobeeSE3, 8192 problems), N = 50:

  python tools/tvlqr_time.py [--configs 2 4] [--batch B] [--max-iter 30]

Per config and store_P in (0, 1): gusto_last_solve_ms, gusto_last_tvlqr_ms of the FIRST call (it allocates the device buffers
and pays the cold instruction caches) and the median of five later calls, the sizes of the device buffers, and the split of
the later calls between the two launches (linearise / Riccati: gusto_dev_tvlqr, a third event between them; medians).
One JSON line per measurement.  (The Riccati stage is the generic VALU one; the matrix-core variant that was measured
against it with this tool and lost is recorded in profiles/tvlqr.txt.)"""
import argparse
import ctypes as C
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


def call(s, o):
    s._chk(s.L.gusto_tvlqr(s.h, None, None, C.byref(o)), "tvlqr")
    return s.last_tvlqr_ms()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=0, help="override the config's batch size")
    ap.add_argument("--max-iter", type=int, default=30)
    args = ap.parse_args()
    for cfg in args.configs:
        name, B = CONFIGS[cfg]
        B = args.batch or B
        model = getattr(g, name)
        n, m = g.MODEL_DIMS[model]
        boxes, spheres, (x0, glo, ghi, tf) = problems(cfg, B)
        for store_P in (0, 1):
            s = g.BatchSolver(model, N, B, hist_cap=64, boxes=boxes, spheres=spheres)
            s.set_problems(x0, glo, ghi, tf)
            s.solve(args.max_iter)
            o = s.tvlqr_opts(dict(store_P=store_P))
            first = call(s, o)
            later, lin, ric = [], [], []
            for _ in range(5):
                later.append(call(s, o))
                a, b = s.tvlqr_phase_ms()
                lin.append(a)
                ric.append(b)
            st = np.zeros(B, dtype=np.int32)
            s._chk(s.L.gusto_get_tvlqr(s.h, st.ctypes.data, None, None, None, None), "get_tvlqr")
            out = dict(config=cfg, model=name, problems=B, N=N, store_P=store_P, nstep=int(np.ceil(np.max(tf) / (N - 1) / o.dt_min)),
                       solve_ms=round(s.last_solve_ms(), 3), tvlqr_first_ms=round(first, 3),
                       tvlqr_median5_ms=round(statistics.median(later), 3), tvlqr_later_ms=[round(v, 3) for v in later],
                       riccati_stage="generic VALU", status_ok=int(st.sum()),
                       linearise_median5_ms=round(statistics.median(lin), 3), riccati_median5_ms=round(statistics.median(ric), 3),
                       bytes=dict(AB=8 * B * (N - 1) * n * (n + m), K=8 * B * (N - 1) * m * n, P1=8 * B * n * n,
                                  P_all=8 * B * N * n * n * store_P))
            print(json.dumps(out), flush=True)
            s.close()


if __name__ == "__main__":
    main()
