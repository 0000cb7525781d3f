"""The row state of freeflyerSE2's one-wave kernel in pairs (csrc/common.hpp: RS_PAIR, csrc/rows.hpp: RowState::pair) -- (T, LAM),
(S, LAMB), (DT, DL), (KA, KB) next to each other per knot, one 128-bit access per pair -- changes where a value lives and how many
instructions move it, not one value, sum or order of sums: every solve must stay BIT-identical.  The fixtures
tests/golden/rowpairs_*.npz were recorded on an MI355X from the code before that change (a build whose code objects
tools/codeobj_diff.py had shown to be those of the library before it); the library must reproduce them bit for bit, np.array_equal
on every key: trajectories, status, iteration counts and the histories.

Every case is freeflyerSE2, B = 32, solve(30), the table environment.  The shapes are the smallest at which each access pattern
can go wrong:
  table_n3, table_n4  the first and the last knot, the last knot without control rows, knots with fixed rows only
  obs_n5              Delta0 = 10 (obstacle_toggle_distance = Delta / 8 + clearance = 1.3): knots with 5-8 and with 9 or more active
                      obstacle rows, i.e. two and three obstacle batches and the clamped spare positions of a batch -- asserted from
                      the rows of the first trip (the straight line the handle starts from), not assumed
  box_n4              a BoxGoal on x for half of the batch and no goal on theta, omega (the inputs of tests/test_gpu_factor_stage.py):
                      goal rows through obs_load at goal slots
  params_n5           mass, inertia, radius and clearance of param_cases "freeflyer"
  sliced_n50          N = 50 with 2 probing slices of one trip (gusto_set_schedule(2, 1)): the row state is rebuilt in whichever
                      workspace slot continues the problem
Every fixture holds problems of two and more trips: the first subproblem starts cold, the others warm (both branches of OpInit).

`python tests/test_gpu_rowstate_pairs.py --record` writes the fixtures from the library in the tree."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
B = 32
STATUS = ("iterations", "converged", "successful", "stop_reason", "ipm_iters")
# histories: (first valid entry, the count that bounds them); entries past the count are unset
HIST = {"Delta": (0, "n_hist"), "omega": (0, "n_hist"), "convergence_measure": (1, "n_hist"), "accept_solution": (1, "n_hist"),
        "scp_status": (1, "n_hist"), "solver_status": (1, "n_hist"), "trust_region_satisfied": (1, "n_hist"),
        "convex_ineq_satisfied": (1, "n_hist"), "ipm_iters": (1, "n_hist"), "J_true": (0, "nJ"), "J_full": (0, "nJ"), "rho": (0, "n_rho")}
CASES = ["table_n3", "table_n4", "obs_n5", "box_n4", "params_n5", "sliced_n50"]
OBS_DELTA0 = 10.0


def _fixture(name):
    return os.path.join(GOLDEN, f"rowpairs_freeflyer_{name}.npz")


def _batch(name):
    import gusto_jl_amd as g
    if name == "params_n5":
        import param_cases as PC
        return PC.batch(PC.FF, B)
    x0, glo, ghi, tf = g.problems.freeflyer_batch(B)
    if name == "box_n4":
        glo[:, 2] = -np.inf; ghi[:, 2] = np.inf            # theta free
        glo[:, 5] = -np.inf; ghi[:, 5] = np.inf            # omega free
        glo[:B // 2, 0] -= 0.05; ghi[:B // 2, 0] += 0.05   # BoxGoal on x for half of the batch
    return x0, glo, ghi, tf


def _active_rows(X0, toggle, radius):
    """obstacle rows per knot of the first trip: the boxes closer than `toggle` to the body at the straight-line trajectory"""
    import gusto_jl_amd as g
    P = g.problems
    env = P.freeflyer_env()
    return np.array([[sum(P._sdf_rect2(x[:2], bx[0:2], bx[3:5]) - radius < toggle for bx in env) for x in Xb] for Xb in X0])


def _run(name):
    import gusto_jl_amd as g
    N = int(name.rsplit("_n", 1)[1])
    s = g.BatchSolver(g.FREEFLYER_SE2, N, B, hist_cap=40, boxes=g.problems.freeflyer_env())
    sp, mp = g.default_params(g.FREEFLYER_SE2)
    if name == "params_n5":
        import param_cases as PC
        import test_kkt_certificate as T
        s.set_params(model_params=T.as_params(g.ModelParams, PC.params("freeflyer", PC.FF)))
    if name == "obs_n5":
        sp.Delta0 = OBS_DELTA0
        s.set_params(scp_params=sp)
    if name == "sliced_n50":
        s.set_schedule(2, 1)
    s.set_problems(*_batch(name))
    rows = None
    if name == "obs_n5":
        rows = _active_rows(s.traj()[0], OBS_DELTA0 / 8 + mp.clearance, mp.radius)
    s.solve(30)
    X, U = s.traj()
    st, h = s.status(), s.history()
    s.close()
    out = dict(X=X, U=U, **{k: np.asarray(st[k]) for k in STATUS})
    for k in ("n_hist", "nJ", "n_rho"):
        out["h_" + k] = h[k]
    for k, (lo, cnt) in HIST.items():
        a = np.array(h[k])
        idx = np.arange(a.shape[1])[None, :]
        a[~((idx >= lo) & (idx < h[cnt][:, None]))] = 0
        out["h_" + k] = a
    return out, rows


@pytest.mark.parametrize("name", CASES)
def test_solve_is_bit_identical_to_the_unpaired_build(name):
    d = np.load(_fixture(name))
    # (the fixture holds real solves, a cold and a warm subproblem at least; at N = 3 no problem of the batch converges)
    assert d["iterations"].max() >= 2 and d["ipm_iters"].min() >= 1 and (d["converged"].any() or name == "table_n3")
    out, rows = _run(name)
    if name == "obs_n5":
        print("active obstacle rows per knot, first trip:", np.bincount(rows.ravel()))
        assert (d["h_Delta"][:, 0] == OBS_DELTA0).all()
        assert ((rows >= 5) & (rows <= 8)).any() and (rows >= 9).any(), np.bincount(rows.ravel())
    assert sorted(out) == sorted(d.files)
    for k in sorted(out):
        assert out[k].shape == d[k].shape and np.array_equal(out[k], d[k]), (name, k)


if __name__ == "__main__":
    import sys
    root = os.path.dirname(os.path.dirname(GOLDEN))
    for p in (os.path.dirname(GOLDEN), root, os.path.join(root, "oracle")):
        sys.path.insert(0, p)
    if "--record" in sys.argv:
        for name in CASES:
            out, rows = _run(name)
            np.savez_compressed(_fixture(name), **out)
            print(name, "trips", int(out["iterations"].sum()), "max trips", int(out["iterations"].max()), "kkt", int(out["ipm_iters"].sum()),
                  "min kkt", int(out["ipm_iters"].min()), "converged", int(out["converged"].sum()), "/", B,
                  "" if rows is None else f"rows/knot {np.bincount(rows.ravel())}", flush=True)
