"""The row state of the interior point method (t, lam, s, ... of every inequality row of every knot, csrc/rows.hpp: RowState)
is private to the device code: where a (row, variable, knot) entry lives in the workspace changes no sum and no order of sums, so
every solve must stay BIT-identical across a change of that layout.  The fixtures tests/golden/rowstate_*.npz were recorded on an
MI355X with the build that still addressed `(var * nslot + slot) * N + k` (control rows behind the obstacle rows, run-time
strides); every case here must reproduce them with np.array_equal.

The cases walk the places where the addressing takes another path: the smallest horizon, a padded knot stride that is exactly
full (N = 64) and the first multi-wave size (N = 65), no obstacle rows at all, per-problem obstacle counts (run-time obstacle
slots beside compile-time fixed slots), BoxGoal rows (the manifold model), the helper waves' obstacle rows (two waves per
problem), the TrajOpt row program, and a sliced schedule (the row state is rebuilt per subproblem in the slot workspace).

`python tests/test_gpu_rowstate_layout.py --record` writes the fixtures from the library in the tree."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("X", "U", "iterations", "ipm_iters", "converged")


def _g():
    import gusto_jl_amd as g
    return g


def _out(s):
    X, U = s.traj()
    st = s.status()
    s.close()
    return dict(X=X, U=U, iterations=st["iterations"], ipm_iters=st["ipm_iters"], converged=st["converged"])


def _freeflyer(N, B=32, table=True, schedule=None):
    g = _g()
    P = g.problems
    s = g.BatchSolver(g.FREEFLYER_SE2, N, B, hist_cap=40, boxes=P.freeflyer_env() if table else None)
    if schedule is not None:
        s.set_schedule(*schedule)
    s.set_problems(*P.freeflyer_batch(B))
    s.solve(30)
    return _out(s)


def _freeflyer_env_batch():
    """B = 16, every problem its own keep-out set: 0 to 14 components, boxes and discs (problems.freeflyer_random_layouts), the
    first two problems pinned to the empty set and to the whole table"""
    g = _g()
    P = g.problems
    B = 16
    bl, sl = P.freeflyer_random_layouts(B)
    bl[0], sl[0] = None, None
    bl[1], sl[1] = P.freeflyer_env(), None
    s = g.BatchSolver(g.FREEFLYER_SE2, 50, B, hist_cap=40)
    s.set_env_batch(bl, sl)
    s.set_problems(*P.freeflyer_batch(B))
    s.solve(30)
    return _out(s)


def _dubins():
    g = _g()
    s = g.BatchSolver(g.DUBINS_CAR, 30, 64, hist_cap=40)
    s.set_problems(*g.problems.dubins_batch(64))
    s.solve(30)
    return _out(s)


def _astrobee(manifold, B, decomposition):
    g = _g()
    P = g.problems
    boxes, sph = P.iss_corner_env(True)
    model = g.ASTROBEE_SE3_MANIFOLD if manifold else g.ASTROBEE_SE3
    s = g.BatchSolver(model, 50, B, hist_cap=40, boxes=boxes, spheres=sph)
    s.set_decomposition(decomposition)
    s.set_problems(*(P.astrobee_manifold_batch(B) if manifold else P.astrobee_se3_batch(B)))
    s.solve(30)
    return _out(s)


def _trajopt_freeflyer():
    g = _g()
    P = g.problems
    s = g.TrajOptSolver(g.FREEFLYER_SE2, 50, 8, boxes=P.freeflyer_env())
    s.set_problems(*P.freeflyer_batch(8))
    s.solve(125)
    return _out(s)


CASES = {
    "freeflyer_n3": lambda: _freeflyer(3),
    "freeflyer_n50": lambda: _freeflyer(50),
    "freeflyer_n64": lambda: _freeflyer(64),
    "freeflyer_n65": lambda: _freeflyer(65),
    "freeflyer_n50_no_obstacles": lambda: _freeflyer(50, table=False),
    "freeflyer_n50_env_batch": _freeflyer_env_batch,
    "dubins_n30": _dubins,
    "astrobee_se3_n50": lambda: _astrobee(False, 16, 1),           # one wave per problem
    "astrobee_manifold_n50": lambda: _astrobee(True, 16, 1),
    "astrobee_se3_n50_two_waves": lambda: _astrobee(False, 8, 3),  # GUSTO_DECOMP_WAVE2: the helper wave's row code
    "trajopt_freeflyer_n50": _trajopt_freeflyer,
}


def _golden(name):
    return np.load(os.path.join(GOLDEN, "rowstate_" + name + ".npz"))


def _assert_bits(out, d, what):
    for k in KEYS:
        assert out[k].shape == d[k].shape and np.array_equal(out[k], d[k]), (what, k)


@pytest.mark.parametrize("name", list(CASES))
def test_solve_is_bit_identical_to_the_recorded_one(name):
    d = _golden(name)
    assert d["iterations"].max() > 1 and d["ipm_iters"].min() > 0   # (the fixture holds real solves)
    _assert_bits(CASES[name](), d, name)


def test_sliced_and_unsliced_schedules_are_bit_identical():
    """The same 32 freeflyer problems first come, first served (no slices), with 2 and with 5 probing slices of one SCP iteration
    each (gusto_set_schedule, min_batch = 1).  Between slices a problem waits in the scheduler's lists and whichever workgroup is
    free next continues it, rebuilding the row state in its own workspace slot: nothing of it may be assumed to persist from one
    subproblem to the next.  (32 problems fit the resident workgroups, so a change of slot is possible here, not certain: the test
    below forces it.)"""
    d = _golden("freeflyer_n50")
    runs = [_freeflyer(50, schedule=(probe, 1)) for probe in (0, 2, 5)]
    for r in runs[1:]:
        _assert_bits(r, runs[0], "sliced vs unsliced")
    _assert_bits(runs[0], d, "unsliced vs fixture")


def test_sliced_and_unsliced_with_more_problems_than_workspace_slots():
    """More problems than persistent workgroups (gusto_dev_launch_info), so every slot's row state is reused by one problem after
    another and a sliced problem is continued wherever a slot comes free: sliced and unsliced must agree bit for bit, and the
    first 32 problems with the fixture of the batch of 32 (a problem's result does not depend on its neighbours)."""
    g = _g()
    P = g.problems
    B, runs = 1536, []
    for probe in (0, 2):
        s = g.BatchSolver(g.FREEFLYER_SE2, 50, B, hist_cap=40, boxes=P.freeflyer_env())
        s.set_schedule(probe, 1)
        s.set_problems(*P.freeflyer_batch(B))
        s.solve(30)
        slots = s.launch_info()[0]
        assert 0 < slots < B, (slots, B)
        runs.append(_out(s))
    _assert_bits(runs[1], runs[0], "sliced vs unsliced")
    d = _golden("freeflyer_n50")
    for k in KEYS:
        assert np.array_equal(runs[0][k][:32], d[k]), k


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(GOLDEN))
    sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))
    if "--record" in sys.argv:
        for name, run in CASES.items():
            out = run()
            np.savez_compressed(os.path.join(GOLDEN, "rowstate_" + name + ".npz"), **{k: out[k] for k in KEYS})
            print(name, "trips", int(out["iterations"].sum()), "kkt", int(out["ipm_iters"].sum()), "converged",
                  int(out["converged"].sum()), "/", len(out["converged"]), flush=True)
