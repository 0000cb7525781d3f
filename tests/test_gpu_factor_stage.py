"""The factor stage of freeflyerSE2 (csrc/factor1w.hpp: factor_sweep_pg2) -- one instruction stream for r_k = P_k c_k and
Pi_k^T c_k, the rows of H_yu, Z_u and Pi laid out for 128-bit reads -- forms every sum in the order the stage formed it before it
had that layout, so every solve must stay BIT-identical.  The fixtures tests/golden/factorstage_freeflyer_{goal}_n{N}.npz were
recorded on an MI355X from the code before that change (a build whose model_0 code object tools/codeobj_diff.py had shown to be
that of the library before it); the library must reproduce them bit for bit, np.array_equal on every key.

The fixtures of the sibling files (test_gpu_sweep_dpp.py, test_gpu_rowstate_layout.py) all have a point goal on every coordinate.
What they leave out of the stage is the last knot's E term of Z = [Phi Gam]^T Pi + E where it differs between the lanes of Z:
  partial   no goal on theta and omega: E is selected on the lanes of four of the six columns of Z only
  box       the same, and a BoxGoal on x for half of the batch: no point goal on x there either (its rows are inequality rows)
both built the way tests/test_gpu_parity.py::test_partial_goal_and_box_goal_freeflyer builds them, at N = 4 and N = 5 -- the
shortest horizons with a middle stage next to the last knot's (E), the first (nothing behind it) and the peeled knot 0 -- and
the partial goal at N = 50 with a sliced schedule (2 and 5 probing slices against the unsliced batch).
Every case is freeflyerSE2, B = 32, the table environment, solve(30).

`python tests/test_gpu_factor_stage.py --record` writes the fixtures from the library in the tree."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("X", "U", "iterations", "ipm_iters", "converged")
CASES = [(goal, N) for goal in ("partial", "box") for N in (4, 5)]
B = 32


def _fixture(goal, N):
    return os.path.join(GOLDEN, f"factorstage_freeflyer_{goal}_n{N}.npz")


def _batch(goal):
    import gusto_jl_amd as g
    x0, glo, ghi, tf = g.problems.freeflyer_batch(B)
    glo[:, 2] = -np.inf; ghi[:, 2] = np.inf            # theta free
    glo[:, 5] = -np.inf; ghi[:, 5] = np.inf            # omega free
    if goal == "box":
        glo[:B // 2, 0] -= 0.05; ghi[:B // 2, 0] += 0.05   # BoxGoal on x for half of the batch
    return x0, glo, ghi, tf


def _freeflyer(goal, N, schedule=None, info=None):
    import gusto_jl_amd as g
    s = g.BatchSolver(g.FREEFLYER_SE2, N, B, hist_cap=40, boxes=g.problems.freeflyer_env())
    if schedule is not None:
        s.set_schedule(*schedule)
    s.set_problems(*_batch(goal))
    s.solve(30)
    X, U = s.traj()
    st = s.status()
    if info is not None:
        info.append(s.launch_info())
    s.close()
    return dict(X=X, U=U, iterations=st["iterations"], ipm_iters=st["ipm_iters"], converged=st["converged"])


def _assert_bits(out, d, what):
    for k in KEYS:
        assert out[k].shape == d[k].shape and np.array_equal(out[k], d[k]), (what, k)


@pytest.mark.parametrize("goal,N", CASES)
def test_last_knot_goal_term_is_bit_identical_to_the_stage_before(goal, N):
    d = np.load(_fixture(goal, N))
    assert d["ipm_iters"].min() >= 1 and d["converged"].any()   # (the fixture holds real solves)
    _assert_bits(_freeflyer(goal, N), d, (goal, N))


def test_sliced_schedule_and_lds_budget_at_n50():
    """N = 50, partial goal, unsliced and with 2 and 5 probing slices of one SCP iteration each (between slices the problem waits in
    the scheduler's lists and its next factor sweep runs in whichever workgroup is free).  The launch must still fit four
    workgroups into a compute unit: 40 960 B of LDS each at the most."""
    d = np.load(_fixture("partial", 50))
    assert d["ipm_iters"].min() >= 1 and d["converged"].any()
    info = []
    for probe in (0, 2, 5):
        _assert_bits(_freeflyer("partial", 50, schedule=(probe, 1), info=info), d, ("probe", probe))
    for slots, lds, per_cu in info:
        assert lds <= 40960 and per_cu == 4, (slots, lds, per_cu)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(GOLDEN))
    sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))
    if "--record" in sys.argv:
        for goal, N in CASES + [("partial", 50)]:
            out = _freeflyer(goal, N, schedule=(0, 1) if N == 50 else None)
            np.savez_compressed(_fixture(goal, N), **{k: out[k] for k in KEYS})
            print(goal, N, "trips", int(out["iterations"].sum()), "kkt", int(out["ipm_iters"].sum()), "min kkt", int(out["ipm_iters"].min()),
                  "converged", int(out["converged"].sum()), "/", len(out["converged"]), flush=True)
