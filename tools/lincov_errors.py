"""The largest relative errors of gusto_lincov over the cases of tests/test_gpu_lincov.py -- the figures behind that file's gates
(ten times the value, rounded up to a power of ten) and the first table of profiles/lincov.txt.  Every error is taken against
the numpy restatement (tests/np_lincov.py) in np.longdouble, never against the device; the last row is the cross-check with
gusto_simulate.  One line per quantity.

  python tools/lincov_errors.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import lincov_cases as LC  # noqa: E402
import sim_cases as SC  # noqa: E402
import test_gpu_lincov as G  # noqa: E402


def main():
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), float(v))
    LD = np.longdouble
    for model, N in LC.CASES:
        for mode in range(len(LC.MODES)):
            tv, out = G.device(model, N, mode)
            for e in LC.ENVS:
                for st in LC.STARTS:
                    ref = LC.reference(model, N, mode, e, st, tv.AB, tv.K, dtype=LD)
                    end = LC.reference(model, N, mode, e, st, dtype=LD) if (e, st) in (("sim", "default"), ("batch", "full")) else None
                    for b in range(G.B):
                        for f in G.INDEX_FIELDS:
                            assert out[e, st][f][b] == ref[b][f], (model, N, mode, e, st, b, f)
                        for f in G.KNOT_FIELDS + G.SUMMARY_FIELDS:
                            note("stage_" + f, G.rel(out[e, st][f][b], ref[b][f]))
                            if end is not None:
                                note("end_" + f, G.rel(out[e, st][f][b], end[b][f]))
    # the cross-check with gusto_simulate (tests/test_gpu_lincov.py: test_second_moment_of_gusto_simulate), and next to it the
    # restatement in long double on the device's AB and K against the same second moment of the device's roll-outs
    model, N, mode, S = 0, 50, 2, 257
    X, U, tf, _ = LC.inputs(model, N)
    s = G.solver(model, N, X, U, tf)
    s.tvlqr(G.tvlqr_opts(mode), X, U)
    P = SC.perturbation(model, S)
    s.simulate(dict(n_samples=S, store_knots=1, dense_collision=0, **LC.MODES[mode]), X, U, pert=P)
    Xcl = s.get_simulate_knots()
    D = Xcl - Xcl[:, :, :1]
    M = np.einsum("bksi,bksj->bkij", D, D) / S
    S0 = np.stack([G.second_moment_start(P[b]) for b in range(G.B)])
    r = s.lincov(dict(store_S=1), X, U, S0=S0)
    s.close()
    for b in range(G.B):
        note("simulate_Sxx", max(G.rel(r["Sxx"][b, k], M[b, k]) for k in range(N)))
    for k, v in sorted(worst.items()):
        print(f"{k:28s} {v:.3e}", flush=True)


if __name__ == "__main__":
    main()
