"""The figures behind the tolerance of tests/test_gpu_simulate.py, one line per quantity.

  python tools/simulate_errors.py [--device] [--disturbed]

Without a GPU: over exactly the cases of tests/sim_cases.py, the largest relative difference between the float64 and the
np.longdouble run of the numpy restatement (tests/np_simulate.py) -- what one rounding per operation does to each compared
quantity.  The test gates at 100 x the largest of them, rounded up to a power of ten.  With --device: the device's errors
against the float64 restatement fed with the device's own gains, beside them (profiles/simulate.txt holds both).
With --disturbed: the same for gusto_simulate_disturbed -- tests/sim_disturbed_cases.py, tests/np_simulate_disturbed.py and
tests/test_gpu_simulate_disturbed.py (profiles/simulate_disturbed.txt)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import sim_cases as SC  # noqa: E402

FIELDS = ("sample_min_dist", "x_final", "max_dev", "max_final_dev", "min_dist", "Xcl")


def rel(a, ref):
    """largest |a - ref| over the finite entries of ref, relative to the largest |ref| (equal infinities differ by 0)"""
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    return float(np.abs(a[fin] - ref[fin]).max() / np.abs(ref[fin]).max())


def main():
    worst, dev = {}, {}
    device = "--device" in sys.argv
    cases = SC
    if "--disturbed" in sys.argv:
        import sim_disturbed_cases as cases
    if device:
        G = __import__("test_gpu_simulate_disturbed" if cases is not SC else "test_gpu_simulate")
    for case in cases.CASES:
        lo = cases.reference(case, dtype=np.float64)
        hi = cases.reference(case, dtype=np.longdouble)
        for b in range(SC.B):
            for k in FIELDS:
                worst[k] = max(worst.get(k, 0.0), rel(lo[b][k], hi[b][k]))
        if device:
            r, Xcl, ref = (lambda out: (out[0], out[1], out[-1]))(G.device_and_reference(case))
            for b in range(SC.B):
                for k in FIELDS:
                    got = Xcl[b] if k == "Xcl" else r[k][b]
                    dev[k] = max(dev.get(k, 0.0), rel(got, ref[b][k]))
    for k in FIELDS:
        print(f"{k:16s} float64 against longdouble {worst[k]:.3e}" + (f"   device against float64 {dev[k]:.3e}" if device else ""), flush=True)
    print(f"{'largest':16s} {max(worst.values()):.3e}")


if __name__ == "__main__":
    main()
