"""The figures behind the gates of tests/test_gpu_lincov_dense.py and the tables of profiles/lincov_dense.txt.  CPU only:

  python tools/lincov_dense_errors.py

1. The largest relative error of the float64 restatement (tests/np_lincov_dense.py behind tests/np_lincov_plant.py) against the same
   restatement in np.longdouble -- the roll-out inside the intervals, the sensitivities, the knot pass and the margins all in the
   dtype -- over the cases of tests/lincov_dense_cases.py, one line per quantity.  Each gate is ten times its row's figure,
   rounded up to a power of ten.
2. The disagreement of the restatement's two routes to the covariance at a dense sample (lincov_dense_cases.two_route_*): the
   one-step maps chained by the knot recursion on the dense trajectory against the propagation inside the interval.  Its tenfold,
   rounded up, is the gate of the same check between the two kernel paths on the device.
3. The corner-cut case: the separations its test states.

With --device (needs the GPU), for information only -- no gate rests on these: the device's errors against the long double
restatement for the rows of 1."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import lincov_cases as LC  # noqa: E402
import lincov_dense_cases as DC  # noqa: E402

LD = np.longdouble
DENSE_FIELDS = ("z_dense", "Spos", "min_z_dense")
COMBOS = (("sim", "default"), ("batch", "full"), ("empty", "default"))


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


def two_routes(model, dense, chained):
    """the worst relative disagreement (Spos against the Sxx block, z_dense against z_obs) over the five problems"""
    ws = 2 if model < 2 else 3
    worst = {}
    for (_, d), c in zip(dense, chained):
        worst["Spos"] = max(worst.get("Spos", 0.0), rel(d["Spos"], c["Sxx"][:, :ws, :ws]))
        worst["z_dense"] = max(worst.get("z_dense", 0.0), rel(d["z_dense"], c["z_obs"]))
    return worst


def cpu(worst):
    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), float(v))
    for model, N in LC.CASES:
        for mode in range(len(LC.MODES)):
            for e, st in COMBOS:
                r64 = DC.dense_reference(model, N, mode, e, st)
                rld = DC.dense_reference(model, N, mode, e, st, dtype=LD)
                for a, r in zip(r64, rld):
                    assert a["dense_sample"] == r["dense_sample"] and a["dense_pair"] == r["dense_pair"]
                    assert np.array_equal(a["pair_dense"], r["pair_dense"])
                    for f in DENSE_FIELDS:
                        note("own_" + f, rel(a[f], r[f]))
    for model in LC.MODELS:
        dense = DC.two_route_dense(model)
        Xd = np.stack([d["xbar"] for _, d in dense])
        Ud = DC.held_controls(LC.inputs(model, DC.TWO_N)[1])
        for k, v in two_routes(model, dense, DC.two_route_chained(model, Xd, Ud)).items():
            note("two_routes_" + k, v)
    knot, d = DC.corner_reference()
    z = np.sort(d["z_dense"])
    zp = np.sort(d["z_pairs"][d["dense_sample"]])
    print("corner cut: min_z_obs %.4f (knot %d)  min_z_dense %.4f (sample %d, pair %d)  runner-up sample +%.4f  runner-up pair +%.4f"
          % (knot["min_z_obs"], knot["obs_knot"], d["min_z_dense"], d["dense_sample"], d["dense_pair"], z[1] - z[0], zp[1] - zp[0]))


def device(worst):
    import test_gpu_lincov_dense as G

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), float(v))
    for model, N in LC.CASES:
        for mode in range(len(LC.MODES)):
            tv, Cd, out = G.device(model, N, mode)
            for e, st in COMBOS:
                ref = DC.dense_reference(model, N, mode, e, st, tv.AB, tv.K, Cd, dtype=LD)
                end = DC.dense_reference(model, N, mode, e, st, dtype=LD)
                for b in range(DC.B):
                    for f in DENSE_FIELDS:
                        note("device_stage_" + f, rel(out[e, st][f][b][:ref[b]["nfull"]] if f != "min_z_dense" else out[e, st][f][b], ref[b][f]))
                        note("device_end_" + f, rel(out[e, st][f][b][:end[b]["nfull"]] if f != "min_z_dense" else out[e, st][f][b], end[b][f]))


def main():
    worst = {}
    if "--device" in sys.argv:
        device(worst)
    else:
        cpu(worst)
    for k, v in sorted(worst.items()):
        print(f"{k:36s} {v:.3e}", flush=True)


if __name__ == "__main__":
    main()
