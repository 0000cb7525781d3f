"""gusto_set_problems_roadmap on the device against tests/np_roadmap.py.  Every case is an input of tests/roadmap_cases.py, whose
decision margin tests/test_roadmap_cpu.py asserts: status, n_via, via and banned exactly, length to 1e-12 relative, X0 to 1e-11 m
(coordinates below 16 m: a few dozen roundings stay under 1e-13, a wrong node moves a knot by centimetres), DIRECT and every
fallback bit for bit against gusto_set_problems with X0 = NULL.  Shapes: N = 3, 4, 50; Bq = 1 and 5; K = 1 and 3; straight_first
both ways; C = 0, 1, planar 16 (exactly one word: with start and goal a lane owns two nodes), planar 17 (four bits in a second
word), spatial 9 and 64 (512 rows, the limit: nine nodes in lanes 0 and 1); a per-problem batch that mixes C = 3 and C = 17."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import np_roadmap as RM
import roadmap_cases as RC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device(case, straight_first=0, per_problem=False, queries=None):
    """the case (or its `queries`) on a fresh handle: (report, X0, U0, the straight lines of the same problems)"""
    q = np.arange(case["Bq"]) if queries is None else np.asarray(queries)
    K = case["K"]
    s = g.BatchSolver(case["model"], case["N"], len(q) * K, hist_cap=8)
    try:
        envs = case["envs"]
        if isinstance(envs, tuple) and not per_problem:
            s.set_env(*envs)
        else:
            sets = [envs if isinstance(envs, tuple) else envs[i] for i in q for _ in range(K)]
            s.set_env_batch([b for b, _ in sets], [sp for _, sp in sets])
        args = (case["x_init"][q], case["goal_lo"][q], case["goal_hi"][q], case["tf"][q])
        s.set_problems_roadmap(*args, K=K, straight_first=straight_first, **case["opts"])
        rep = s.roadmap_info()
        X, U = s.traj()
        assert s.last_roadmap_ms() > 0 and rep["stage_ms"].sum() <= s.last_roadmap_ms() * (1 + 1e-6) + 1e-6
        s.set_problems(*(np.repeat(a, K, axis=0) for a in args))
        Xs, Us = s.traj()
        with pytest.raises(g.GustoError):
            s.roadmap_info()      # new problems: the report is gone
    finally:
        s.close()
    return rep, X, U, Xs


def compare(rep, X, U, Xs, ref, rows=None):
    rows = np.arange(len(ref["status"])) if rows is None else rows
    for k in ("status", "n_via", "via", "banned"):
        assert np.array_equal(rep[k], ref[k][rows]), (k, rep[k], ref[k][rows])
    ln = ref["length"][rows]
    fin = np.isfinite(ln)
    assert np.array_equal(np.isfinite(rep["length"]), fin) and np.all(rep["length"][~fin] == np.inf)
    assert np.all(np.abs(rep["length"][fin] - ln[fin]) <= 1e-12 * ln[fin])
    assert np.abs(X - ref["X0"][rows]).max() <= 1e-11 and not U.any()
    line = rep["status"] != RM.PATH
    assert np.array_equal(X[line], Xs[line])                      # DIRECT and every fallback: the straight line's bits
    assert np.array_equal(X[:, 0], Xs[:, 0]) and np.array_equal(X[:, -1], Xs[:, -1])   # the end knots: the inputs' own entries


@pytest.mark.parametrize("straight_first", [0, 1])
@pytest.mark.parametrize("name", list(RC.CASES))
def test_device_is_the_restatement(name, straight_first):
    case = RC.CASES[name]
    ref = RC.reference(name, straight_first)
    rep, X, U, Xs = device(case, straight_first)
    compare(rep, X, U, Xs, ref)
    WS = RC.WS_DIM[case["model"]]
    assert np.array_equal(X[:, :, WS:], Xs[:, :, WS:])            # behind the workspace: the straight line's entries


def test_cases_cover_what_they_are_for():
    """the statuses and shapes the cases were built for are really there"""
    st = lambda n, sf=0: set(RC.reference(n, sf)["status"].tolist())
    assert st("plane_c0") == {RM.DIRECT} and RM.NO_PATH in st("plane_c1") and RM.PATH in st("plane_c1")
    assert RM.STRAIGHT in st("plane_c16", 1) and RM.DIRECT in st("space_c9") and RM.PATH in st("space_c64")
    assert (RC.reference("plane_c17")["via"] >= 2 + 64).any()     # a node whose bit lies in the second word
    assert RC.reference("plane_c16")["n_via"].max() >= 3 and (RC.reference("plane_c17")["banned"][:, 1] >= 0).any()


@pytest.mark.parametrize("name", ["plane_c16", "space_c9", "plane_mixed"])
def test_a_query_alone_and_in_a_batch_of_five(name):
    case = RC.CASES[name]
    K = case["K"]
    rep, X, U, _ = device(case)
    for q in (1, 4):
        r1, X1, U1, _ = device(case, queries=[q])
        rows = slice(q * K, (q + 1) * K)
        assert np.array_equal(X1, X[rows]) and all(np.array_equal(r1[k], rep[k][rows]) for k in ("status", "n_via", "via", "length", "banned"))


@pytest.mark.parametrize("name", ["plane_c17", "space_c9"])
def test_one_set_shared_and_the_same_set_per_problem(name):
    case = RC.CASES[name]
    a, b = device(case), device(case, per_problem=True)
    assert np.array_equal(a[1], b[1]) and all(np.array_equal(a[0][k], b[0][k]) for k in ("status", "n_via", "via", "length", "banned"))


def test_refusals_leave_the_handle_untouched():
    case = RC.CASES["plane_c16"]
    K, Bq = case["K"], case["Bq"]
    s = g.BatchSolver(0, case["N"], Bq * K, hist_cap=8, boxes=case["envs"][0], spheres=case["envs"][1])
    t = g.TrajOptSolver(0, case["N"], Bq * K)
    try:
        args = (case["x_init"], case["goal_lo"], case["goal_hi"], case["tf"])
        s.set_problems_roadmap(*args, K=K, **case["opts"])
        rep, (X, U), st = s.roadmap_info(), s.traj(), s.status()
        L, h = s.L, s.h
        p = [a.ctypes.data for a in args]
        ok = g.RoadmapOpts(0.1, 0.03, 0)
        call = lambda Bq_, K_, ptrs, o: L.gusto_set_problems_roadmap(h, Bq_, K_, *ptrs, None if o is None else C.byref(o))
        assert call(Bq, 0, p, ok) == -1 and call(Bq, 9, p, ok) == -1 and call(0, K, p, ok) == -1 and call(Bq + 1, K, p, ok) == -1
        for i in range(4):
            assert call(Bq, K, p[:i] + [None] + p[i + 1:], ok) == -1
        for bad in ((np.nan, 0.03, 0), (-0.01, 0.03, 0), (np.inf, 0.03, 0), (0.1, 0.0, 0), (0.1, np.inf, 0), (0.1, np.nan, 0),
                    (0.1, 0.03, 2), (0.1, 0.03, -1)):
            assert call(Bq, K, p, g.RoadmapOpts(*bad)) == -1, bad
        assert L.gusto_set_problems_roadmap(None, Bq, K, *p, C.byref(ok)) == -1
        assert L.gusto_set_problems_roadmap(t.h, Bq, K, *p, C.byref(ok)) == -1 and b"TrajOpt" in L.gusto_last_error(t.h)
        with pytest.raises(g.GustoError):
            t.set_problems_roadmap(*args)
        assert s.B == Bq * K
        rep2, (X2, U2), st2 = s.roadmap_info(), s.traj(), s.status()
        assert np.array_equal(X, X2) and np.array_equal(U, U2) and all(np.array_equal(rep[k], rep2[k]) for k in rep)
        assert all(np.array_equal(st[k], st2[k]) for k in st)
        # per-problem sets for another number of problems: GUSTO_ERR_STATE, the handle likewise untouched
        s.set_env_batch([case["envs"][0]] * 4, [case["envs"][1]] * 4)
        assert call(Bq, K, p, ok) == -3
        X3, _ = s.traj()
        assert np.array_equal(X, X3)
        ms = C.c_double()
        assert L.gusto_last_roadmap_ms(h, None) == -1 and L.gusto_last_roadmap_ms(None, C.byref(ms)) == -1
        assert L.gusto_default_roadmap_opts(9, C.byref(ok)) == -1 and L.gusto_default_roadmap_opts(0, None) == -1
    finally:
        s.close()
        t.close()
    o = g.default_roadmap_opts(0)
    _, mp = g.default_params(0)
    assert (o.inflate, o.pad, o.straight_first) == (mp.radius + 0.02, 0.03, 0)


def test_study_on_the_device():
    """the first 48 table queries, N = 50, 30 trips: the straight line and the roadmap seed answer what they answer on the oracle"""
    ref, (x0, lo, hi, tf) = RC.study_reference()
    s = g.BatchSolver(0, RC.STUDY_N, RC.STUDY_B, hist_cap=64, boxes=g.problems.freeflyer_env())
    try:
        s.set_problems(x0, lo, hi, tf)
        s.solve(RC.STUDY_ITERS)
        st = s.status()
        straight_fails = set(np.flatnonzero(~(st["converged"] & st["successful"])).tolist())
        s.set_problems_roadmap(x0, lo, hi, tf, K=1, **RC.STUDY_OPTS)
        rep = s.roadmap_info()
        assert np.array_equal(rep["status"], ref["status"]) and np.array_equal(rep["via"], ref["via"])
        s.solve(RC.STUDY_ITERS)
        st = s.status()
        seed_fails = set(np.flatnonzero(~(st["converged"] & st["successful"])).tolist())
    finally:
        s.close()
    assert straight_fails == {1, 5, 7, 37, 40} and seed_fails == RC.STUDY_SEED_FAILS


def test_host_driver():
    """solve_SCP_roadmap_batch: seeds, solves, selects; with a fan the unanswered queries are retried"""
    H = g.host
    ref, (x0, lo, hi, tf) = RC.study_reference()
    qs = [0, 1, 5, 7]
    TOPs = []
    for q in qs:
        gs = H.GoalSet()
        H.add_goal(gs, H.Goal(H.BoxGoal(lo[q], hi[q]), tf[q], H.FreeflyerSE2()))
        PD = H.ProblemDefinition(H.Robot(), H.FreeflyerSE2(), H.Environment(g.problems.freeflyer_env()), x0[q], gs)
        TOPs.append(H.TrajectoryOptimizationProblem(PD, RC.STUDY_N, tf[q], fixed_final_time=True))
    TOSs = [H.TrajectoryOptimizationSolution(t) for t in TOPs]
    out = H.solve_SCP_roadmap_batch(TOSs, TOPs, K=1, roadmap_opts=RC.STUDY_OPTS, max_iter=RC.STUDY_ITERS)
    assert [o["winner"] for o in out] == [0, -1, 0, 0] and [o["status"] for o in out] == [ref["status"][q] for q in qs]
    assert out[1]["source"] is None and out[2]["source"] == "roadmap" and np.isfinite(out[2]["cost"]) and out[0]["roadmap_ms"] > 0
    out = H.solve_SCP_roadmap_batch(TOSs, TOPs, K=2, straight_first=True, fallback_fan=True, roadmap_opts=RC.STUDY_OPTS, max_iter=RC.STUDY_ITERS)
    assert out[1]["source"] == "fan" and out[1]["winner"] > 0 and all(o["winner"] >= 0 for o in out)
    assert all(o["SCPS"].successful and o["SCPS"].converged for o in out)


def test_c_consumer(tmp_path):
    """tests/c/c_abi_roadmap.c, a plain C consumer with checks of its own; the rows it prints are the Python path's"""
    exe = os.path.join(tmp_path, "c_abi_roadmap")
    lib = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_roadmap.c"), "-o", exe, "-L" + lib, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 1 + 6
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.4, 1.3, 0, 0, 0, 0], [0.3, 0.4, 0, 0, 0, 0]], float)
    goal = np.tile([3.0, 1.1, 0, 0.05, -0.05, 0], (3, 1))
    box = np.array([[1.4, 0.9, -0.2, 1.8, 1.5, 0.2]])
    ref = RM.roadmap_batch(x0, goal, goal, (box, np.zeros((0, 4))), 2, 50, 2, inflate=0.177, pad=0.03)
    assert ref["decision_margin"] >= RC.MARGIN
    for b in range(6):
        v = lines[1 + b].split()
        assert [int(v[0]), int(v[1]), int(v[2]), int(v[3])] == [ref["status"][b], ref["n_via"][b], ref["via"][b, 0], ref["banned"][b, 0]]
        assert float(v[4]) == pytest.approx(ref["length"][b], rel=1e-12)
