"""The one-wave vector sweeps of freeflyerSE2 (csrc/sweeps.hpp: backward_sweep_dpp / forward_sweep_dpp) run the same sums in the same
order as the v_readlane sweeps they replace (backward_sweep_1w / forward_sweep_1w), so every solve must stay BIT-identical.  The
fixtures tests/golden/sweepdpp_freeflyer_n{N}.npz were recorded on an MI355X with the library that still ran freeflyerSE2 on the
readlane sweeps; the library must reproduce them bit for bit, np.array_equal on every key.

The DPP sweeps walk the horizon in chunks of 8 knots (two groups of 6 lanes in each of the four rows of 16 lanes, rows in the order
0, 1, 3, 2, the vector handed from row to row by a row swap and from the last row back to the first at the chunk boundary); the
backward sweep has N - 1 steps, the forward sweep N.  The horizons are those at which a chunk can go wrong:
  N = 8, 9, 10    one chunk exactly and one step over it, in each direction: the wrap hop is used once
  N = 16, 17, 18  the second chunk boundary
  N = 63          every group busy in every chunk but the last, clamped operands in the last chunk only
and the N = 50 batch of tests/test_gpu_rowstate_layout.py with a sliced schedule (a problem continued in another workspace slot).
Every case is freeflyerSE2, B = 32, the table environment, solve(30).

`python tests/test_gpu_sweep_dpp.py --record` writes the fixtures from the library in the tree."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("X", "U", "iterations", "ipm_iters", "converged")
HORIZONS = (8, 9, 10, 16, 17, 18, 63)


def _freeflyer(N, B=32, schedule=None):
    import gusto_jl_amd as g
    P = g.problems
    s = g.BatchSolver(g.FREEFLYER_SE2, N, B, hist_cap=40, boxes=P.freeflyer_env())
    if schedule is not None:
        s.set_schedule(*schedule)
    s.set_problems(*P.freeflyer_batch(B))
    s.solve(30)
    X, U = s.traj()
    st = s.status()
    s.close()
    return dict(X=X, U=U, iterations=st["iterations"], ipm_iters=st["ipm_iters"], converged=st["converged"])


def _assert_bits(out, d, what):
    for k in KEYS:
        assert out[k].shape == d[k].shape and np.array_equal(out[k], d[k]), (what, k)


@pytest.mark.parametrize("N", HORIZONS)
def test_solve_is_bit_identical_to_the_readlane_sweeps(N):
    d = np.load(os.path.join(GOLDEN, f"sweepdpp_freeflyer_n{N}.npz"))
    assert d["ipm_iters"].min() >= 1 and d["converged"].any()   # (the fixture holds real solves)
    _assert_bits(_freeflyer(N), d, N)


def test_sliced_schedule_is_bit_identical_to_the_readlane_sweeps():
    """N = 50 (six chunks and a step or two) with 2 and 5 probing slices of one SCP iteration each: between slices the problem
    waits in the scheduler's lists and the sweeps of its next subproblem run in whichever workgroup is free.  Against the fixture
    of the unsliced batch that tests/test_gpu_rowstate_layout.py keeps."""
    d = np.load(os.path.join(GOLDEN, "rowstate_freeflyer_n50.npz"))
    for probe in (0, 2, 5):
        _assert_bits(_freeflyer(50, schedule=(probe, 1)), d, ("probe", probe))


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(GOLDEN))
    sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))
    if "--record" in sys.argv:
        for N in HORIZONS:
            out = _freeflyer(N)
            np.savez_compressed(os.path.join(GOLDEN, f"sweepdpp_freeflyer_n{N}.npz"), **{k: out[k] for k in KEYS})
            print(N, "trips", int(out["iterations"].sum()), "kkt", int(out["ipm_iters"].sum()), "min kkt", int(out["ipm_iters"].min()),
                  "converged", int(out["converged"].sum()), "/", len(out["converged"]), flush=True)
