"""GPU time of gusto_simulate next to the solve and the verification of the same batch, for BASELINE configs 2 (freeflyerSE2,
4096 problems) and 4 (astrobeeSE3, 8192 problems), N = 50, S = 64 samples per problem:

  python tools/simulate_time.py [--configs 2 4] [--batch B] [--samples 64] [--max-iter 30] [--disturbed]

Per config: gusto_last_solve_ms, gusto_last_verify_ms and the median of five warm calls of gusto_last_simulate_ms -- with
dense_collision 1 and 0, and with store_knots -- in the same process, and the time per RK4 step per sample of gusto_simulate
and of gusto_verify (a verify "sample" is one knot interval of one problem): verify's per-step cost is the yardstick the
roll-out kernel is read against, since both do a step and the same distance loop.  One JSON line per config.

--disturbed: instead, per config and per entry of --samples (several may be given), the median, smallest and largest of five warm
gusto_last_simulate_ms of plain gusto_simulate, of gusto_simulate_disturbed with perturbations, plant and noise generated on
the device, and of the same call with all three supplied by the caller, with the ns per RK4 step per sample of each
(profiles/simulate_disturbed.txt)."""
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


def five(call):
    """(median, smallest, largest) of gusto_last_simulate_ms over five warm calls of `call` (one call before them allocates and
    pays the cold instruction caches)"""
    s = call()
    ms = []
    for _ in range(5):
        call()
        ms.append(s.last_simulate_ms())
    return [round(v, 3) for v in (statistics.median(ms), min(ms), max(ms))]


def disturbed(args):
    rng = np.random.default_rng(0)
    for cfg in args.configs:
        name, B = CONFIGS[cfg]
        B = args.batch or B
        model = getattr(g, name)
        boxes, spheres, (x0, glo, ghi, tf) = problems(cfg, B)
        s = g.BatchSolver(model, N, B, hist_cap=64, boxes=boxes, spheres=spheres)
        s.set_problems(x0, glo, ghi, tf)
        s.solve(args.max_iter)
        s.tvlqr()
        n, m = s.n, s.m
        mp = g.default_params(model)[1]
        nominal = np.array([mp.mass, mp.Jdiag[0], mp.Jdiag[1], mp.Jdiag[2], mp.dubins_v, mp.dubins_k])
        rel = np.array([0.1, 0.05, 0.1, 0.15, 0.1, 0.1])
        dw = np.full(m, 1e-3)
        steps = float(np.ceil(tf / (N - 1) / 0.1).sum()) * (N - 1)      # RK4 steps of one sample of every problem
        for S in args.samples:
            o = dict(n_samples=S)
            pert = np.concatenate([rng.uniform(-0.01, 0.01, (B, S, n)), np.zeros((B, S, m))], axis=2)
            plant = nominal * (1 + rel * rng.uniform(-1, 1, (B, S, 6)))
            white = dw * rng.uniform(-1, 1, (B, N - 1, S, m))
            pert[:, 0], plant[:, 0], white[:, :, 0] = 0.0, nominal, 0.0
            rows = dict(plain=five(lambda: s.simulate(o) and s),
                        generated=five(lambda: s.simulate_disturbed(o, dict(plant_rel=rel, dw=dw)) and s),
                        supplied=five(lambda: s.simulate_disturbed(o, None, pert=pert, plant=plant, white=white) and s))
            r = s.get_simulate()
            out = dict(config=cfg, model=name, problems=B, N=N, samples=S, median_min_max_ms=rows,
                       ns_per_step_per_sample={k: round(1e6 * v[0] / (steps * S), 4) for k, v in rows.items()},
                       n_free=int(r["n_free"].sum()), n_finite=int(r["n_finite"].sum()))
            print(json.dumps(out), flush=True)
            del pert, plant, white
        s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    ap.add_argument("--batch", type=int, default=0, help="override the config's batch size")
    ap.add_argument("--samples", type=int, nargs="+", default=[64])
    ap.add_argument("--max-iter", type=int, default=30)
    ap.add_argument("--disturbed", action="store_true", help="plain against gusto_simulate_disturbed, generated and supplied")
    args = ap.parse_args()
    if args.disturbed:
        return disturbed(args)
    args.samples = args.samples[0]
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
