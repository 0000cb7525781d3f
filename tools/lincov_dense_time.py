"""GPU time of gusto_lincov_dense next to the stages it stands beside, at the BASELINE shapes of config 2 (freeflyerSE2 4096 x N 50)
and config 4 (astrobeeSE3 8192 x N 50):

  python tools/lincov_dense_time.py [--configs 2 4] [--batch B] [--max-iter 30]

Per config, after solve(max_iter) and one gusto_tvlqr (dt_min 0.1: the roll-out every stage here shares): the median of five warm
gusto_last_lincov_ms of gusto_lincov_dense without and with store_dense, of gusto_lincov_disturbed with the same arguments, the
median of five warm gusto_last_verify_ms, and gusto_last_simulate_ms of one warm gusto_simulate_disturbed at 64 samples; then the
bytes of the buffers the dense call adds.  One JSON line per config; profiles/lincov_dense.txt holds them."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402

import gusto_jl_amd as g  # noqa: E402
from tools.lincov_time import CONFIGS, problems  # noqa: E402

DISTURB = dict(plant_rel=[0.08134, 0.05, 0.05, 0.05, 0.05, 0.05], dw=0.01)


def median5(call, last):
    call()
    ms = []
    for _ in range(5):
        call()
        ms.append(last())
    return round(statistics.median(ms), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=0, help="override the config's batch size")
    ap.add_argument("--max-iter", type=int, default=30)
    args = ap.parse_args()
    C = g._capi.C
    for cfg in args.configs:
        name, B, N = CONFIGS[cfg]
        B = args.batch or B
        model = getattr(g, name)
        n, m = g.MODEL_DIMS[model]
        ws = g._capi.WS_DIM[model]
        boxes, spheres, (x0, glo, ghi, tf) = problems(cfg, B)
        s = g.BatchSolver(model, N, B, hist_cap=64, boxes=boxes, spheres=spheres)
        s.set_problems(x0, glo, ghi, tf)
        s.solve(args.max_iter)
        cap = max(64, int(np.ceil(np.max(tf) / (N - 1) / 0.1)))
        s.tvlqr(dict(nstep_cap=cap))
        o, d = s.lincov_opts(None), s.disturb_opts(DISTURB)
        out = dict(config=cfg, model=name, problems=B, N=N)
        out["verify_median5_ms"] = median5(lambda: s.verify(nstep_cap=cap), s.last_verify_ms)
        out["lincov_disturbed_median5_ms"] = median5(
            lambda: s._chk(s.L.gusto_lincov_disturbed(s.h, None, None, None, None, None, C.byref(o), C.byref(d)), "lincov_disturbed"), s.last_lincov_ms)
        for store in (0, 1):
            out["lincov_dense_store_%d_median5_ms" % store] = median5(
                lambda: s._chk(s.L.gusto_lincov_dense(s.h, None, None, None, None, None, C.byref(o), C.byref(d), store), "lincov_dense"), s.last_lincov_ms)
        rows = C.c_int(0)
        nfull, zmin = np.zeros(B, dtype=np.int32), np.zeros(B)
        rep = g._capi.LincovDenseReport(nfull=nfull.ctypes.data, min_z_dense=zmin.ctypes.data)
        s._chk(s.L.gusto_get_lincov_dense(s.h, C.byref(rep), C.byref(rows)), "get_lincov_dense")
        zobs = s.get_lincov(Sxx=False)["min_z_obs"]
        so = s.simulate_opts(dict(n_samples=64, nstep_cap=cap))
        sim = lambda: s._chk(s.L.gusto_simulate_disturbed(s.h, None, None, None, None, None, None, C.byref(so), C.byref(d)), "simulate_disturbed")   # noqa: E731
        sim()
        sim()
        R, NZ = rows.value, n + m + 6
        out.update(simulate_disturbed_64_warm_ms=round(s.last_simulate_ms(), 3), nfull_max=R, nstep_max=(R - 1) // (N - 1),
                   dense_below_knots=int(np.sum(zmin < zobs)),
                   bytes=dict(S_rows=8 * B * N * n * NZ, S_block=8 * B * (m + 6) ** 2, per_interval=16 * B * (N - 1), z_dense=8 * B * R,
                              pair_dense=4 * B * R, Spos=8 * B * R * ws * ws))
        print(json.dumps(out), flush=True)
        s.close()


if __name__ == "__main__":
    main()
