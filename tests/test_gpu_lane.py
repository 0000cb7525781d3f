"""What is left of the tests of the lane-per-problem decomposition (GUSTO_DECOMP_LANE: reserved, refused; the kernel and its six
kernel-specific tests are in git history): the one whose body never depended on the kernel -- the history-capacity contract on
dubins_car -- now runs on the shipped wave-per-problem kernel."""
import pytest

pytestmark = pytest.mark.gpu


def test_lane_history_capacity_and_hooks():
    """the history-capacity contract (a handle whose history fills up stops with HIST_FULL, never silently) for dubins_car, as
    tests/test_gpu_parity.py holds it for freeflyerSE2"""
    import gusto_jl_amd as g
    B, N = 64, 30
    x0, glo, ghi, tf = g.problems.dubins_batch(B)
    s = g.BatchSolver(g.DUBINS_CAR, N, B, hist_cap=6)
    s.set_problems(x0, glo, ghi, tf)
    s.solve(30)
    st = s.status()
    assert (st["stop_reason"] != 0).all() and (st["stop_reason"] == 4).any()     # 30 trips cannot fit 6 entries: never MaxIter
    h = s.history()
    assert (h["n_hist"] <= 6).all() and (st["iterations"] <= 5).all()
