"""GPU time of gusto_lincov next to the stages it follows and the one it stands beside, at the BASELINE batch sizes of the four
models (configs 2 - 5: freeflyerSE2 4096 x N 50, dubins_car 65536 x N 30, astrobeeSE3 8192 x N 50, astrobeeSE3manifold 2048 x N 50):

  python tools/lincov_time.py [--configs 2 3 4 5] [--batch B] [--samples 4096] [--max-iter 30]

Per config, after solve(max_iter): gusto_last_tvlqr_ms (median of five warm calls), gusto_last_lincov_ms of the FIRST call (it
allocates the device buffers and pays the cold instruction caches) and the median of five later calls without and with store_S,
and gusto_last_simulate_ms of one warm call at `samples` samples per problem -- what the same question costs by Monte Carlo
(--samples 0 leaves it out).  One JSON line per config; profiles/lincov.txt holds them."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import gusto_jl_amd as g  # noqa: E402

CONFIGS = {2: ("FREEFLYER_SE2", 4096, 50), 3: ("DUBINS_CAR", 65536, 30), 4: ("ASTROBEE_SE3", 8192, 50), 5: ("ASTROBEE_SE3_MANIFOLD", 2048, 50)}


def problems(cfg, B):
    P = g.problems
    if cfg == 2:
        return P.freeflyer_env(), None, P.freeflyer_batch(B)
    if cfg == 3:
        return None, None, P.dubins_batch(B)
    bx, sp = P.iss_corner_env(True)
    return bx, sp, (P.astrobee_se3_batch(B) if cfg == 4 else P.astrobee_manifold_batch(B))


def median5(call, last):
    ms = []
    for _ in range(5):
        call()
        ms.append(last())
    return statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=sorted(CONFIGS), choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=0, help="override the config's batch size")
    ap.add_argument("--samples", type=int, default=4096, help="samples per problem of the gusto_simulate call (0: none)")
    ap.add_argument("--max-iter", type=int, default=30)
    args = ap.parse_args()
    C = g._capi.C
    for cfg in args.configs:
        name, B, N = CONFIGS[cfg]
        B = args.batch or B
        model = getattr(g, name)
        n, m = g.MODEL_DIMS[model]
        boxes, spheres, (x0, glo, ghi, tf) = problems(cfg, B)
        s = g.BatchSolver(model, N, B, hist_cap=64, boxes=boxes, spheres=spheres)
        s.set_problems(x0, glo, ghi, tf)
        s.solve(args.max_iter)
        cap = max(64, int(np.ceil(np.max(tf) / (N - 1) / 0.1)))
        to = s.tvlqr_opts(dict(nstep_cap=cap))
        s.tvlqr(to)
        tv, _ = median5(lambda: s._chk(s.L.gusto_tvlqr(s.h, None, None, C.byref(to)), "tvlqr"), s.last_tvlqr_ms)
        out = dict(config=cfg, model=name, problems=B, N=N, solve_ms=round(s.last_solve_ms(), 3), tvlqr_median5_ms=round(tv, 3))
        for store_S in (0, 1):
            o = s.lincov_opts(dict(store_S=store_S))
            call = lambda: s._chk(s.L.gusto_lincov(s.h, None, None, None, None, C.byref(o)), "lincov")   # noqa: E731
            call()
            first = s.last_lincov_ms()
            med, each = median5(call, s.last_lincov_ms)
            key = "lincov_store_S_" if store_S else "lincov_"
            out.update({key + "first_ms": round(first, 3), key + "median5_ms": round(med, 3), key + "later_ms": [round(v, 3) for v in each]})
        st = np.zeros(B, dtype=np.int32)
        s._chk(s.L.gusto_get_lincov(s.h, C.byref(g._capi.LincovReport(status=st.ctypes.data))), "get_lincov")
        out.update(status_ok=int(st.sum()), bytes=dict(sigma_x=8 * B * N * n, sigma_u=8 * B * (N - 1) * m, z_obs=8 * B * N, Sxx=8 * B * N * n * n))
        if args.samples:
            so = s.simulate_opts(dict(n_samples=args.samples, nstep_cap=cap))
            sim = lambda: s._chk(s.L.gusto_simulate(s.h, None, None, None, None, C.byref(so)), "simulate")   # noqa: E731
            sim()
            sim()
            out.update(simulate_samples=args.samples, simulate_warm_ms=round(s.last_simulate_ms(), 3))
        print(json.dumps(out), flush=True)
        s.close()


if __name__ == "__main__":
    main()
