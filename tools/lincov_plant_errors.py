"""The figures behind the gates of tests/test_gpu_lincov_plant.py and the tables of profiles/lincov_plant.txt.

Without arguments, CPU only: the largest relative error of the float64 restatement (tests/np_lincov_plant.py) against the same
restatement in np.longdouble over the cases of tests/lincov_plant_cases.py, one line per quantity -- each gate is ten times its
row's figure, rounded up to a power of ten -- and the closed-loop sensitivity of the two restatements (np_lincov_plant against
central differences of np_simulate_disturbed's roll-outs), whose tenfold is the gate of the same check on the device.

  python tools/lincov_plant_errors.py

With --device (needs the GPU), for information only -- no gate rests on these: the device's own errors against the long double
restatement for the same rows, and with --time the GPU time of gusto_lincov_disturbed next to gusto_lincov's on the same handle at
the BASELINE batches (first call, then the median of five warm calls, without and with store_S).

  python tools/lincov_plant_errors.py --device --time      (--time alone: the timings only)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import lincov_cases as LC  # noqa: E402
import lincov_plant_cases as PC  # noqa: E402
import np_lincov_plant as NP  # noqa: E402
import np_simulate_disturbed as NSD  # noqa: E402

LD = np.longdouble
KNOT_FIELDS = ("sigma_x", "sigma_u", "z_obs", "Sxx", "Sxt")
SUMMARY_FIELDS = ("min_z_obs", "min_z_ctl", "p_collision_bound")
INDEX_FIELDS = ("status", "fail_knot", "obs_knot", "obs_pair", "ctl_knot", "ctl_entry")


def rel(a, ref):
    """tests/test_gpu_lincov.py: rel, without importing a GPU test module"""
    a, ref = np.asarray(a, dtype=LD), np.asarray(ref, dtype=LD)
    fin = np.isfinite(ref)
    if not np.array_equal(a[~fin], ref[~fin], equal_nan=True):
        return np.inf
    if not fin.any():
        return 0.0
    nrm = np.abs(ref[fin]).max()
    err = np.abs(a[fin] - ref[fin]).max()
    return float(err / nrm) if nrm > 0 else float(err)


def cd_rel(a, ref, model):
    """the worst column of Cd [N-1, n, 6] over the scalars the model reads"""
    return max(rel(a[:, :, j], ref[:, :, j]) for j in NSD.READS[model])


def cpu(worst):
    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), float(v))
    for model, N in LC.CASES:
        X, U, tf, _ = LC.inputs(model, N)
        for mode in range(len(LC.MODES)):
            Cd = PC.sensitivities(model, N, mode)
            for b in range(PC.B):
                note("own_Cd", cd_rel(Cd[b], NP.sensitivities(model, X[b], U[b], tf[b], dtype=LD, **LC.MODES[mode]), model))
            for e in LC.ENVS:
                for st in LC.STARTS:
                    r64 = PC.reference(model, N, mode, e, st)
                    rld = PC.reference(model, N, mode, e, st, dtype=LD)
                    for a, r in zip(r64, rld):
                        for f in KNOT_FIELDS + SUMMARY_FIELDS:
                            note("own_" + f, rel(a[f], r[f]))
    import test_lincov_plant_cpu as TC
    for model, N, mode in PC.CONSISTENT:
        X, U, tf = PC.consistent_inputs(model, N, mode)
        n, m = NP.MODELS[model].n, NP.MODELS[model].m
        theta = PC.fd_plants(model)
        for b, (AB, K, Cd, Sth, r) in enumerate(PC.consistent_reference(model, N, mode)):
            sim = NSD.simulate(model, X[b], U[b], K, tf[b], np.zeros((len(theta), n + m)), theta, dense_collision=False, **LC.MODES[mode])
            note("own_closed_loop_sensitivity", PC.sens_rel(PC.fd_sensitivity(model, sim["Xcl"], theta), NP.closed_loop_sensitivity(r, Sth), model))
    assert TC.TOL_SENS >= worst["own_closed_loop_sensitivity"]


def device(worst):
    import test_gpu_lincov_plant as G

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), float(v))
    for model, N in LC.CASES:
        for mode in range(len(LC.MODES)):
            tv, Cd, out = G.device(model, N, mode)
            X, U, tf, _ = LC.inputs(model, N)
            for b in range(PC.B):
                note("device_Cd", cd_rel(Cd[b], NP.sensitivities(model, X[b], U[b], tf[b], dtype=LD, **LC.MODES[mode]), model))
            for e in LC.ENVS:
                for st in LC.STARTS:
                    ref = PC.reference(model, N, mode, e, st, tv.AB, tv.K, Cd, dtype=LD)
                    end = PC.reference(model, N, mode, e, st, dtype=LD) if (e, st) in (("sim", "default"), ("batch", "full")) else None
                    for b in range(PC.B):
                        for f in INDEX_FIELDS:
                            assert out[e, st][f][b] == ref[b][f], (model, N, mode, e, st, b, f)
                        for f in KNOT_FIELDS + SUMMARY_FIELDS:
                            note("device_stage_" + f, rel(out[e, st][f][b], ref[b][f]))
                            if end is not None:
                                note("device_end_" + f, rel(out[e, st][f][b], end[b][f]))
    for model, N, mode in PC.CONSISTENT:
        note("device_closed_loop_sensitivity", G.closed_loop_on_the_device(model, N, mode))


def timing():
    """gusto_lincov and gusto_lincov_disturbed on one handle per BASELINE batch (size, horizon and keep-out set of BASELINE.json's
    configs 2 to 5; the trajectories are np_tvlqr.smooth_batch's, tiled), after one gusto_tvlqr: GPU ms from the events of the
    calls themselves (gusto_last_lincov_ms)"""
    import ctypes

    import gusto_jl_amd as g
    import np_tvlqr as T
    P = g.problems
    for name, model, B, N in (("freeflyerSE2", 0, 4096, 50), ("dubins", 1, 65536, 30), ("astrobeeSE3", 2, 8192, 50), ("manifold", 3, 2048, 50)):
        X, U = T.smooth_batch(model, 8, N)
        X, U = np.tile(X, (B // 8, 1, 1)), np.tile(U, (B // 8, 1, 1))
        tf = np.full(B, 0.5 * (N - 1))
        boxes, spheres = (P.freeflyer_env(), None) if model == 0 else ((None, None) if model == 1 else P.iss_corner_env(True))
        s = g.BatchSolver(model, N, B, hist_cap=16, boxes=boxes, spheres=spheres)
        s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
        s.tvlqr(dict(Q=100.0, R=1.0, Qf=100.0, nstep=5), X, U)
        row = []
        for store in (0, 1):
            for call in ("lincov", "lincov_disturbed"):
                ms = []
                for _ in range(6):
                    if call == "lincov":
                        s.L.gusto_lincov(s.h, None, None, None, None, ctypes.byref(s.lincov_opts(dict(store_S=store)))) and sys.exit("gusto_lincov failed")
                    else:
                        s.L.gusto_lincov_disturbed(s.h, None, None, None, None, None, ctypes.byref(s.lincov_opts(dict(store_S=store))),
                                                   ctypes.byref(s.disturb_opts(PC.disturb(model)))) and sys.exit("gusto_lincov_disturbed failed")
                    ms.append(s.last_lincov_ms())
                row.append("%s store_S=%d first %.3f warm %.3f" % (call, store, ms[0], float(np.median(ms[1:]))))
        s.close()
        print("time_ms %-13s B=%d N=%d nstep=5 | %s" % (name, B, N, " | ".join(row)), flush=True)


def main():
    worst = {}
    if "--device" in sys.argv:
        device(worst)
    elif "--time" not in sys.argv:
        cpu(worst)
    for k, v in sorted(worst.items()):
        print(f"{k:36s} {v:.3e}", flush=True)
    if "--time" in sys.argv:
        timing()


if __name__ == "__main__":
    main()
