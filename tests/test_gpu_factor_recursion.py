"""The factor stage of freeflyerSE2 (csrc/factor1w.hpp: factor_sweep_pg2) keeps only the recursion on its sequential path: the
stage stores L^-1 where it once stored S^-1 = L^-T L^-1 and V = L^-1 Z_u where it once stored D = L^-T V, and the stage-parallel
mid phase (csrc/ipm.hpp: mid_phase; csrc/common.hpp: kd_holds_linv_v) forms S^-1 and D of its knot with the expressions the stage
used.  No sum and no order of a sum changed, so every solve must stay BIT-identical.  The fixtures
tests/golden/factorrec_freeflyer_{case}_n{N}.npz were recorded on an MI355X from the code before that change (a build whose
model_0 code object tools/codeobj_diff.py had shown to be that of the library before it); the library must reproduce them bit for
bit, np.array_equal on every key.

The sibling files (test_gpu_factor_stage.py, test_gpu_sweep_dpp.py, test_gpu_rowstate_layout.py) hold the stage to those bits with
a point goal on every coordinate, with none on theta and omega, and with a BoxGoal on x.  What they leave out and this change touches:
  nogoal   no point goal on any coordinate (goal_lo = -inf, goal_hi = +inf everywhere): the goalmask == 0 branch of the mid phase,
           where D and mu_g are unused and d_k = d0 = S^-1 lu alone
  xy       a point goal on x and y only: two live columns of D
both at N = 3 -- the shortest horizon: the last knot's stage, one middle stage, the peeled knot 0 -- and N = 4, and
  params   the `freeflyer` case of tests/param_cases.py (mass 11.5, J = 0.25, radius, clearance: the columns of Gam, and with them
           H_uu, differ) on its turned starts, N = 5, set through BatchSolver.set_params on a live handle
Every case is freeflyerSE2, B = 32, the table environment, solve(30).

`python tests/test_gpu_factor_recursion.py --record` writes the fixtures from the library in the tree."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("X", "U", "iterations", "ipm_iters", "converged")
CASES = [(case, N) for case in ("nogoal", "xy") for N in (3, 4)] + [("params", 5)]
B = 32


def _fixture(case, N):
    return os.path.join(GOLDEN, f"factorrec_freeflyer_{case}_n{N}.npz")


def _batch(case):
    import gusto_jl_amd as g
    if case == "params":
        import param_cases as PC
        return PC.batch(PC.FF, B)
    x0, glo, ghi, tf = g.problems.freeflyer_batch(B)
    free = slice(0, None) if case == "nogoal" else slice(2, None)   # xy: the point goal stays on x and y
    glo[:, free] = -np.inf
    ghi[:, free] = np.inf
    return x0, glo, ghi, tf


def _freeflyer(case, N):
    import gusto_jl_amd as g
    s = g.BatchSolver(g.FREEFLYER_SE2, N, B, hist_cap=40, boxes=g.problems.freeflyer_env())
    if case == "params":
        import param_cases as PC
        import test_kkt_certificate as T
        s.set_params(model_params=T.as_params(g.ModelParams, PC.params("freeflyer", PC.FF)))
    s.set_problems(*_batch(case))
    s.solve(30)
    X, U = s.traj()
    st = s.status()
    s.close()
    return dict(X=X, U=U, iterations=st["iterations"], ipm_iters=st["ipm_iters"], converged=st["converged"])


@pytest.mark.parametrize("case,N", CASES)
def test_recursion_only_stage_is_bit_identical_to_the_stage_before(case, N):
    d = np.load(_fixture(case, N))
    assert d["ipm_iters"].min() >= 1 and d["converged"].any()   # (the fixture holds real solves)
    out = _freeflyer(case, N)
    for k in KEYS:
        assert out[k].shape == d[k].shape and np.array_equal(out[k], d[k]), (case, N, k)


if __name__ == "__main__":
    import sys
    root = os.path.dirname(os.path.dirname(GOLDEN))
    for p in (os.path.dirname(GOLDEN), root, os.path.join(root, "oracle")):
        sys.path.insert(0, p)
    if "--record" in sys.argv:
        for case, N in CASES:
            out = _freeflyer(case, N)
            np.savez_compressed(_fixture(case, N), **{k: out[k] for k in KEYS})
            print(case, N, "trips", int(out["iterations"].sum()), "kkt", int(out["ipm_iters"].sum()), "min kkt", int(out["ipm_iters"].min()),
                  "converged", int(out["converged"].sum()), "/", len(out["converged"]), flush=True)
