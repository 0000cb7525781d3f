"""The largest relative errors of gusto_tvlqr against the numpy restatement (tests/np_tvlqr.py) over the cases of
tests/test_gpu_tvlqr.py -- the figures behind that file's gates (ten times the value, rounded up to a power of ten) and the
first table of profiles/tvlqr.txt.  One line per quantity.

  python tools/tvlqr_errors.py"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402

import gusto_jl_amd as g  # noqa: E402
import np_tvlqr as T  # noqa: E402
import test_gpu_tvlqr as G  # noqa: E402


def main():
    worst = {}

    def note(k, v):
        worst[k] = max(worst.get(k, 0.0), float(v))
    for model, N in G.CASES:
        n, _ = g.MODEL_DIMS[model]
        X, U, tf, (Q, R, Qf) = G._inputs(model, N)
        for mode in range(len(G.MODES)):
            AB, K, P = G._reference(model, N, mode)
            s = G._solver(model, N, X, U, tf)
            r = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, store_P=1, **G.MODES[mode]), X, U)
            s.close()
            for b in range(G.B):
                note("AB", max(G._rel(r.AB[b, k], AB[b, k]) for k in range(N - 1)))
                Kn, Pn = T.riccati(r.AB[b], Q, R, Qf)
                note("riccati_K", G._rel(r.K[b], Kn))
                note("riccati_P", max(G._rel(r.P[b, k], Pn[k]) for k in range(N)))
                note("end_K", G._rel(r.K[b], K[b]))
                note("end_P1", G._rel(r.P[b, 0], P[b, 0]))
                for k in range(N - 1):
                    A, Bd, Pk = r.AB[b, k, :, :n], r.AB[b, k, :, n:], r.P[b, k]
                    note("identity", np.abs(Pk - (np.diag(Q) + A.T @ r.P[b, k + 1] @ (A - Bd @ r.K[b, k]))).max() / np.abs(Pk).max())
                    note("asymmetry", np.abs(Pk - Pk.T).max())
                    note("min_eig_below_zero", max(0.0, -np.linalg.eigvalsh(Pk).min() / np.abs(Pk).max()))
    for k, v in sorted(worst.items()):
        print(f"{k:20s} {v:.3e}", flush=True)


if __name__ == "__main__":
    main()
