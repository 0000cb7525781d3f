"""gusto_legs_begin, gusto_legs_advance, gusto_get_legs and gusto_get_legs_dev on the device against tests/np_legs.py, the numpy
restatement (tests/test_legs_cpu.py proves it without a GPU), against gusto_set_problems on the same handle, against the CPU
oracle leg by leg, and end to end through host.solve_SCP_timeline_batch.

Tolerances.  Everything is compared bit for bit -- the seeds with np_legs.device_line, the straight line in the rounding
csrc/seed.hpp pins (one fused multiply-add), and with gusto_set_problems on the same handle -- except
  - the legs against the oracle: the whole-solve gates of tests/test_gpu_parity.py for freeflyerSE2 (_scp_parity, at most one
    diverged problem), applied by that helper to the leg problems;
  - gap and arrive end to end: at most gusto_ipm_opts.tol_acc, the loosest level at which a subproblem is accepted.

Recorded on the MI355X (profiles/legs.txt, section 3)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import np_legs as NL
import np_multistart as MS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPORT = NL.REPORT


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def last_J(h, B):
    return np.array([h["J_true"][b, h["nJ"][b] - 1] if h["nJ"][b] > 0 else np.nan for b in range(B)])


def snapshot(s):
    """what an advance reads of the handle: (X, U, st) with st as np_legs.Timeline.advance takes it"""
    X, U = s.traj()
    st = s.status()
    return X, U, dict(iterations=st["iterations"], converged=st["converged"].astype(np.int32), successful=st["successful"].astype(np.int32),
                      stop_reason=st["stop_reason"], J=last_J(s.history(), s.B))


def check_report(s, S, where):
    r, ref = s.legs_info(), S.report()
    for k in REPORT:
        assert same(r[k], ref[k]), (where, k, r[k], ref[k])
    assert r["round"] == S.round and r["n_flying"] == S.n_flying()
    Xd, Ud, td = s.legs_dev()
    assert np.array_equal(Xd.cpu().numpy(), r["X"]) and np.array_equal(Ud.cpu().numpy(), r["U"]) and np.array_equal(td.cpu().numpy(), r["t"])
    return r


def check_problems(s, S, where):
    """the handle's x_init, goals and tf (gusto_get_problems) and its trajectories are the restatement's, bit for bit"""
    X, U = s.traj()
    ref = S.problems()
    assert s.B == S.B and np.array_equal(X, ref[4]) and np.array_equal(U, ref[5]), where
    for name, a, b in zip(("x_init", "goal_lo", "goal_hi", "tf"), s.problems(), ref[:4]):
        assert np.array_equal(a, b), (where, name, a, b)
    return X, U, ref


def put_traj(s, X, U):
    """X, U onto the handle as a solve would leave them, without one: through the device views of its own buffers"""
    import torch
    Xd, Ud = s.traj_dev()
    Xd.copy_(torch.from_numpy(X))
    Ud.copy_(torch.from_numpy(U))
    torch.cuda.synchronize()


# ---- 1. begin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 4, 50, 65])
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_begin_against_the_restatement(model, N):
    """X0, U0 bit for bit the restatement's and bit for bit what gusto_set_problems with X0 = NULL writes on the same handle for the
    restatement's x_init, goals and tf, in both modes; the report after begin; ragged timelines"""
    from test_legs_cpu import timeline
    rng = np.random.default_rng(100 * model + N)
    shapes = [(1, 1), (3, 2), (3, 5)] + ([(130, 2)] if N == 3 or (model == 0 and N == 65) else [])     # (130 N > 256: more than one block)
    s = g.BatchSolver(model, N, 130 * 2 if len(shapes) > 3 else 15, hist_cap=8)
    for Bq, L in shapes:
        for points in (False, True):
            x_init, lo, hi, T = timeline(model, Bq, L, rng, points=points)
            nl = None if Bq == 1 else np.maximum(1, L - np.arange(Bq) % L)
            for mode in ("sequential", "parallel") if points else ("sequential",):
                took = s.legs_begin(x_init, lo, hi, T, n_legs=nl, mode=mode)
                S = NL.Timeline(model, N, x_init, lo, hi, T, n_legs=nl, mode=g._capi.LEGS_MODE[mode], line=NL.device_line)
                where = (Bq, L, points, mode)
                assert took == mode and s.last_legs_ms() > 0
                check_report(s, S, where)
                X, U, ref = check_problems(s, S, where)
                assert np.array_equal(X[:, 0], ref[0]) and np.array_equal(X[:, -1], MS.goal_centre(ref[1], ref[2])) and not U.any()
                s.set_problems(*ref[:4])                     # the straight lines of the restatement's problems, same handle
                Xs, Us = s.traj()
                assert np.array_equal(X, Xs) and np.array_equal(U, Us), where
            # auto: parallel where every interior goal is a full point
            assert s.legs_begin(x_init, lo, hi, T, n_legs=nl) == ("parallel" if points or L == 1 or (nl is not None and nl.max() == 1) else "sequential")
    s.close()


def leg_times(tf, L, equal):
    """T [Q, L] up to the config's tf: equally spaced, or legs that last 2 : 3 : 4 : ... (every tf_l another number)"""
    w = np.ones(L) if equal else 2.0 + np.arange(L)
    return tf[:, None] * (np.cumsum(w) / w.sum())[None, :]


def real_timeline(model, Q, L, full_points, equal=False):
    """timelines on real numbers, legs of unequal length unless `equal`: the study's for freeflyerSE2 (tests/test_legs_cpu.py); for AstrobeeSE3 (config 4) and the
    manifold model (config 5) the queries of the config with the next queries' starts as waypoints, the config's tf per leg --
    the whole start state with full_points, else the position and, on the manifold, the attitude as the +-1e-4 box the config's
    own goals put on the quaternion (a point goal on it next to the hard norm row is not a problem that model solves)"""
    if model == 0:
        from test_legs_cpu import study_timeline
        x0, lo, hi, T, boxes = study_timeline(Q, L, full_points)
        return x0, lo, hi, leg_times(T[:, -1], L, equal), dict(boxes=boxes)
    P = g.problems
    x0, glo, ghi, tf = {2: P.astrobee_se3_batch, 3: P.astrobee_manifold_batch}[model](Q)
    n = x0.shape[1]
    lo, hi = np.full((Q, L, n), -np.inf), np.full((Q, L, n), np.inf)
    for l in range(L - 1):
        w = x0[(np.arange(Q) + l + 1) % Q]
        sel = slice(0, n) if full_points else slice(0, 3)
        lo[:, l, sel] = hi[:, l, sel] = w[:, sel]
        if model == 3 and not full_points:
            lo[:, l, 6:10], hi[:, l, 6:10] = w[:, 6:10] - 1e-4, w[:, 6:10] + 1e-4
    lo[:, L - 1], hi[:, L - 1] = glo, ghi
    boxes, sph = P.iss_corner_env(True)
    return x0, lo, hi, leg_times(tf * L, L, equal), dict(boxes=boxes, spheres=sph)      # (the config's tf per leg on average)


@pytest.mark.parametrize("mode", ["sequential", "parallel"])
def test_the_first_solve_is_the_plain_solve(mode):
    """the handle's x_init, goals and tf after begin are the restatement's: the solve that follows is bit-identical to the solve
    of gusto_set_problems with them, in X, U, status and histories; with L = 1 those are the plain problems themselves"""
    from test_gpu_parity import _assert_same_runs
    N, Q = 20, 4
    for L in (1, 3):
        x0, lo, hi, T, env = real_timeline(0, Q, L, mode == "parallel")
        nl = [L, max(1, L - 1), L, 1]
        K = L if mode == "parallel" else 1
        s = g.BatchSolver(0, N, Q * K, hist_cap=24, **env)
        s.legs_begin(x0, lo, hi, T, n_legs=nl, mode=mode)
        S = NL.Timeline(0, N, x0, lo, hi, T, n_legs=nl, mode=g._capi.LEGS_MODE[mode], line=NL.device_line)
        ref = S.problems()
        if L == 1:
            assert np.array_equal(ref[0], x0) and np.array_equal(ref[1], lo[:, 0]) and np.array_equal(ref[3], T[:, 0])
        s.solve(4)
        a = (s.traj(), s.status(), s.history())
        p = g.BatchSolver(0, N, Q * K, hist_cap=24, **env)
        p.set_problems(*ref[:4])
        if not ref[6].all():
            p.set_active(ref[6])                             # the problems behind a ragged query's last leg rest
        p.solve(4)
        b = (p.traj(), p.status(), p.history())
        _assert_same_runs(a, b)                              # trajectories, statuses, the set entries of the histories
        assert (a[1]["iterations"][ref[6]] > 0).all() and not a[1]["iterations"][~ref[6]].any()
        s.close(), p.close()


# ---- 2. solve and advance, repeated -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,mode", [(0, "sequential"), (0, "parallel"), (2, "parallel"), (3, "sequential")])
def test_solve_and_advance_against_the_restatement(model, mode):
    """every next x_init is the device's own X[N - 1], bit for bit; the joined X, U, t and the report are the restatement applied
    to the device's per-round trajectories and status words, bit for bit, gap and arrive included"""
    N, Q, L = 10, 5, 3
    x0, lo, hi, T, env = real_timeline(model, Q, L, mode == "parallel")
    nl = [3, 2, 3, 1, 3]
    K = L if mode == "parallel" else 1
    s = g.BatchSolver(model, N, Q * K, hist_cap=24, **env)
    s.legs_begin(x0, lo, hi, T, n_legs=nl, mode=mode)
    S = NL.Timeline(model, N, x0, lo, hi, T, n_legs=nl, mode=g._capi.LEGS_MODE[mode], line=NL.device_line)
    rounds = 0
    while S.n_flying():
        s.solve(6)
        X, U, st = snapshot(s)
        print("model %d, %s, round %d: stop reasons %s, trips %s" % (model, mode, rounds, list(st["stop_reason"][S.active]), list(st["iterations"][S.active])))
        assert rounds > 0 or U[S.active].any()               # (the solve moved something)
        ok = (st["converged"] != 0) & (st["successful"] != 0)
        if rounds == 0 and mode == "sequential":
            ok[:] = True                                     # (six trips need not converge: the caller's verdict keeps every query flying)
            left = s.legs_advance(ok)
        else:
            left = s.legs_advance()
        assert left == S.advance(ok, X, U, st)
        r = check_report(s, S, (model, mode, rounds))
        Xn, Un, ref = check_problems(s, S, (model, mode, rounds))
        if mode == "sequential":
            for q in np.flatnonzero(S.flying()):
                assert np.array_equal(Xn[q, 0], X[q, N - 1])                                   # the junction, copied
                assert np.array_equal(r["X"][q, (rounds + 1) * (N - 1)], X[q, N - 1])
        assert (r["gap"][:, 0] == 0).all() and np.isfinite(r["gap"]).all() and np.isfinite(r["arrive"]).all()
        assert not s.status()["iterations"].any()                                             # the history is reset
        rounds += 1
    assert rounds >= 2 if mode == "sequential" else rounds == 1
    s.close()


# ---- 2a. advance at every shape -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 4, 50, 65])
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_advance_at_every_shape(model, N):
    """begin, then advance after advance on random timelines (goal times of unequal spacing, point, box and unbounded entries,
    ragged) with random trajectories put on the handle and a caller's random verdicts, in both modes, at the horizons where the
    knot rules of the join nearly coincide (3, 4) and past one wave (65), L in {1, 2, 5}, one block and several: the report,
    the joined X, U, t, gap and arrive, the next legs' x_init, goals, tf and seeds equal the restatement bit for bit after
    every advance"""
    from test_legs_cpu import timeline
    rng = np.random.default_rng(1000 + 100 * model + N)
    n, m = MS.X_DIM[model], MS.U_DIM[model]
    big = N in (3, 4) or (model == 0 and N == 65) or (model == 1 and N == 50)          # (130 N > 256: more than one block)
    shapes = [(1, 1), (1, 5), (3, 2), (3, 5)] + ([(130, 2)] if big else [])
    s = g.BatchSolver(model, N, 130 * 2 if big else 15, hist_cap=8)
    for Bq, L in shapes:
        for points in (False, True):
            x_init, lo, hi, T = timeline(model, Bq, L, rng, points=points)
            nl = None if Bq == 1 else np.maximum(1, L - np.arange(Bq) % L)
            for mode in ("sequential", "parallel") if points else ("sequential",):
                where = (Bq, L, points, mode)
                s.legs_begin(x_init, lo, hi, T, n_legs=nl, mode=mode)
                S = NL.Timeline(model, N, x_init, lo, hi, T, n_legs=nl, mode=g._capi.LEGS_MODE[mode], line=NL.device_line)
                check_problems(s, S, where)
                rounds = 0
                while S.n_flying():
                    X, U = s.traj()
                    act = S.active
                    X[act], U[act] = rng.uniform(-2, 2, X[act].shape), rng.uniform(-1, 1, U[act].shape)
                    X[act, 0] = S.p_xinit[act] + 1e-9 * rng.uniform(-1, 1, (int(act.sum()), n)) * (rng.uniform(size=(int(act.sum()), 1)) < 0.5)
                    put_traj(s, X, U)
                    Xh, Uh, st = snapshot(s)
                    assert np.array_equal(Xh, X) and np.array_equal(Uh, U)
                    ok = rng.uniform(size=S.B) < 0.8
                    assert s.legs_advance(ok) == S.advance(ok, X, U, st), where
                    check_report(s, S, where + (rounds,))
                    Xn, _, ref = check_problems(s, S, where + (rounds,))
                    if mode == "sequential":
                        fly = S.flying()
                        assert np.array_equal(ref[0][fly], X[fly, N - 1]) and np.array_equal(Xn[fly, 0], X[fly, N - 1])     # the junction, copied
                    rounds += 1
                assert rounds <= L
    s.close()


# ---- 3. a caller's masks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all_ok", "fail_first", "fail_middle", "fail_last", "ragged", "ragged_fail", "single"])
def test_caller_masks_drive_the_timeline(name):
    """the tables of tests/test_legs_cpu.py on the device, independent of the solver's verdicts: failures, ragged timelines,
    n_flying; a finished query's problem is inactive, untouched by the later solves, and its report by the later advances"""
    from test_legs_cpu import SEQ_TABLES
    nl, L, verdicts, status, failed, n_done, flying = SEQ_TABLES[name]
    Q, N = len(nl), 8
    x0, lo, hi, T, env = real_timeline(0, Q, L, False)
    s = g.BatchSolver(0, N, Q, hist_cap=16, **env)
    s.legs_begin(x0, lo, hi, T, n_legs=nl, mode="sequential")
    S = NL.Timeline(0, N, x0, lo, hi, T, n_legs=nl, mode=NL.SEQUENTIAL, line=NL.device_line)
    for r, v in enumerate(verdicts):
        was = S.flying()
        X0, U0 = s.traj()
        s.solve(2)
        X, U, st = snapshot(s)
        assert (st["iterations"][was] > 0).all() and not st["iterations"][~was].any()
        assert np.array_equal(X[~was], X0[~was]) and np.array_equal(U[~was], U0[~was]) and not np.array_equal(X[was], X0[was])
        before = s.legs_info()
        assert s.legs_advance(v) == S.advance(v, X, U, st) == flying[r]
        rep = check_report(s, S, (name, r))
        for k in REPORT:
            assert same(rep[k][~was], before[k][~was]), (name, r, k)                           # finished before: untouched
        check_problems(s, S, (name, r))
    assert list(rep["status"]) == status and list(rep["failed_leg"]) == failed and list(rep["n_done"]) == n_done
    s.close()


def test_caller_masks_parallel():
    """PARALLEL with a failed middle leg and a ragged query, no solve (a caller's eligibility needs none): every leg is stored"""
    Q, L, N = 3, 3, 8
    x0, lo, hi, T, env = real_timeline(0, Q, L, True)
    nl = [3, 2, 3]
    s = g.BatchSolver(0, N, Q * L, hist_cap=16, **env)
    s.legs_begin(x0, lo, hi, T, n_legs=nl, mode="parallel")
    S = NL.Timeline(0, N, x0, lo, hi, T, n_legs=nl, mode=NL.PARALLEL, line=NL.device_line)
    s.solve(3)
    X, U, st = snapshot(s)
    assert not st["iterations"][5] and np.array_equal(X[5], S.p_X[5])
    ok = np.array([1, 0, 1, 1, 1, 0, 1, 1, 0])
    assert s.legs_advance(ok) == S.advance(ok, X, U, st) == 0
    rep = check_report(s, S, "parallel")
    assert list(rep["status"]) == [NL.FAILED, NL.DONE, NL.FAILED] and list(rep["failed_leg"]) == [1, -1, 2] and list(rep["n_done"]) == [1, 2, 2]
    check_problems(s, S, "parallel")
    with pytest.raises(g.GustoError, match="flying"):
        s.legs_advance(ok)
    s.close()


# ---- 4. batch independence ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_query_env", [False, True])
@pytest.mark.parametrize("mode", ["sequential", "parallel"])
def test_a_query_does_not_depend_on_the_batch(mode, per_query_env):
    """a query alone and inside a batch of 130: report, joined buffers and seeds bit for bit, with one keep-out set for all or
    one per query"""
    P = g.problems
    Q, L, N = 130, 3, 8
    x0, lo, hi, T, env = real_timeline(0, Q, L, mode == "parallel")
    nl = np.where(np.arange(Q) % 7 == 3, 2, 3)
    K = L if mode == "parallel" else 1
    if per_query_env:
        boxes, sph = P.freeflyer_random_layouts(Q)
        env = {}

    def run(qs):
        s = g.BatchSolver(0, N, len(qs) * K, hist_cap=16, **env)
        kw = dict(boxes=[boxes[q] for q in qs], spheres=[sph[q] for q in qs]) if per_query_env else {}
        s.legs_begin(x0[qs], lo[qs], hi[qs], T[qs], n_legs=nl[qs], mode=mode, **kw)
        out, left = [s.traj()], len(qs)
        el = np.ones(len(qs) * K, bool)
        el[(np.asarray(qs) % 5 == 2).repeat(K) & (np.arange(len(qs) * K) % K == K - 1)] = False   # (some fail, by query not by slot)
        while left:
            s.solve(3)
            left = s.legs_advance(el)
            out.append(s.traj())
        rep = s.legs_info()
        s.close()
        return rep, out

    rep, seeds = run(list(range(Q)))
    assert set(rep["status"]) == {NL.DONE, NL.FAILED}
    for q in (3, 57, 129):
        r1, s1 = run([q])
        for k in REPORT:
            assert same(r1[k][0], rep[k][q]), (q, k)
        assert len(s1) <= len(seeds)
        for i, b in enumerate(seeds):                      # (behind its last round a finished query's problems stay as they are)
            a = s1[min(i, len(s1) - 1)]
            assert np.array_equal(a[0], b[0][q * K:(q + 1) * K]) and np.array_equal(a[1], b[1][q * K:(q + 1) * K]), q


# ---- 5. PARALLEL against the oracle -------------------------------------------------------------------------------------------
def test_parallel_legs_against_the_oracle():
    """full-point waypoints: every leg is an ordinary problem.  The plain device solve of the leg problems (x_init, goal, tf)
    passes the whole-solve gates of tests/test_gpu_parity.py against the oracle, through its helper; the legs' solve is that
    solve bit for bit; the join is exact copies of it"""
    from test_gpu_parity import _scp_parity
    N, Q, L = 50, 8, 3
    x0, lo, hi, T, env = real_timeline(0, Q, L, True, equal=True)       # (the study's own timeline)
    S = NL.Timeline(0, N, x0, lo, hi, T, mode=NL.PARALLEL, line=NL.device_line)
    xi, l, h, tf = S.problems()[:4]
    print("legs diverged from the oracle", _scp_parity(g.FREEFLYER_SE2, N, env["boxes"], None, xi, l, h, tf, max_diverged=1))
    p = g.BatchSolver(0, N, Q * L, hist_cap=38, **env)
    p.set_problems(xi, l, h, tf)
    p.solve(30)
    Xp, Up = p.traj()
    stp = p.status()
    p.close()
    s = g.BatchSolver(0, N, Q * L, hist_cap=38, **env)
    assert s.legs_begin(x0, lo, hi, T) == "parallel"
    check_problems(s, S, "oracle, begin")
    s.solve(30)
    X, U, st = snapshot(s)
    assert np.array_equal(X, Xp) and np.array_equal(U, Up) and all(same(s.status()[k], stp[k]) for k in stp)
    assert s.legs_advance() == 0
    S.advance((st["converged"] != 0) & (st["successful"] != 0), X, U, st)
    r = check_report(s, S, "oracle")
    for q in range(Q):
        for j in range(L):
            at = j * (N - 1)
            assert np.array_equal(r["X"][q, at + 1:at + N], X[q * L + j, 1:]) and np.array_equal(r["U"][q, at:at + N - 1], U[q * L + j, :N - 1])
        assert np.array_equal(r["U"][q, -1], U[q * L + L - 1, -1]) and np.array_equal(r["t"][q, ::N - 1], np.concatenate([[0.0], T[q]]))
    print("PARALLEL, %d queries x %d legs: %d DONE, largest gap %.3g, largest arrive %.3g" %
          (Q, L, (r["status"] == NL.DONE).sum(), r["gap"].max(), r["arrive"].max()))
    s.close()


# ---- 6. end to end ------------------------------------------------------------------------------------------------------------
E2E_Q, E2E_N = 16, 20
E2E_FAILED = {False: {}, True: {3: 2}}      # table: query 3's last leg ends at MaxIter, on the CPU oracle too (profiles/legs.txt, section 1)


def e2e_problems(qs, table):
    from test_legs_cpu import study_timeline
    H = g.host
    x0, lo, hi, T, boxes = study_timeline(E2E_Q, 3)
    model = H.FreeflyerSE2()
    env = H.Environment(boxes) if table else H.BlankEnv()
    TOPs = []
    for q in qs:
        gs = H.GoalSet()
        for l in range(2):
            H.add_goal(gs, H.Goal(H.PointGoal(lo[q, l, :2]), T[q, l], [0, 1]))               # two position waypoints
        H.add_goal(gs, H.Goal(H.PointGoal(lo[q, 2]), T[q, 2], model))
        TOPs.append(H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, env, x0[q], gs), E2E_N, T[q, 2], fixed_final_time=True))
    return TOPs, [H.TrajectoryOptimizationSolution(t) for t in TOPs], (x0, lo, hi, T)


@pytest.mark.parametrize("table", [False, True])
def test_end_to_end(table, tmp_path):
    """host.solve_SCP_timeline_batch, freeflyerSE2, N = 20, two position waypoints (SEQUENTIAL), the first 16 queries: every
    query is DONE but query 3 next to the table, whose last leg fails as it does on the CPU oracle (pinned: FAILED at leg 2);
    gap and arrive of the legs that arrived are at most gusto_ipm_opts.tol_acc; the joined plan starts at x_init, passes the waypoints at their times and ends at
    the goal; the plain solve of the same problems ignores the waypoints, as before"""
    H = g.host
    qs = list(range(E2E_Q))
    TOPs, TOSs, (x0, lo, hi, T) = e2e_problems(qs, table)
    out = H.solve_SCP_timeline_batch(TOSs, TOPs, verify=not table)      # (nothing to collide with: verify runs and changes nothing)
    tol = g.default_ipm_opts().tol_acc
    gap, arrive = max(o["gap"][:o["n_done"]].max() for o in out if o["n_done"]), max(o["arrive"][:o["n_done"]].max() for o in out if o["n_done"])
    assert {q: out[q]["failed_leg"] for q in qs if out[q]["status"] != g._capi.LEGS_DONE} == E2E_FAILED[table]
    print("end to end, %s: %d queries, largest gap %.3g, largest arrive %.3g, allowed %.3g; trips per leg %s" %
          ("table" if table else "blank", len(qs), gap, arrive, tol, np.array([o["iterations"] for o in out]).sum(axis=0)))
    N = E2E_N
    for i, q in enumerate(qs):
        o, traj = out[i], TOSs[i].traj
        if q in E2E_FAILED[table]:
            assert o["status"] == g._capi.LEGS_FAILED and o["n_done"] == o["failed_leg"] == E2E_FAILED[table][q], (q, o)
        else:
            assert o["status"] == g._capi.LEGS_DONE and o["failed_leg"] == -1 and o["n_done"] == 3, (q, o)
        assert o is TOSs[i].timeline and len(TOSs[i].SCPS) == 3
        assert [bool(S.converged and S.successful) for S in TOSs[i].SCPS] == [l < o["n_done"] for l in range(3)]
        assert traj.X.shape == (6, 3 * (N - 1) + 1) and traj.U.shape == (3, 3 * (N - 1) + 1) and traj.Tf == T[q, 2]
        assert np.array_equal(traj.t[::N - 1], np.concatenate([[0.0], T[q]])) and (np.diff(traj.t) > 0).all()
        for l in range(3):
            leg = TOSs[i].SCPS[l].traj
            assert np.array_equal(traj.X[:, l * (N - 1) + 1:(l + 1) * (N - 1) + 1], leg.X[:, 1:]) and leg.Tf == o["T"][l] - (o["T"][l - 1] if l else 0.0)
            assert np.array_equal(traj.U[:, l * (N - 1):(l + 1) * (N - 1)], leg.U[:, :N - 1])
        assert np.abs(traj.X[:, 0] - x0[q]).max() <= tol and o["J_total"] == sum(float(j) for j in o["J"])
    assert gap <= tol and arrive <= tol
    tree = g.export.write(str(tmp_path / "joined.npz"), 0, TOSs[0].traj.X.T, TOSs[0].traj.U.T, TOSs[0].traj.Tf, t=TOSs[0].traj.t)
    assert np.array_equal(tree["traj"]["t_traj"], TOSs[0].traj.t)
    # the plain solve keeps ignoring the goals before the final time
    TOP, TOS = TOPs[0], H.TrajectoryOptimizationSolution(TOPs[0])
    H.solve_SCP(TOS, TOP, H.solve_gusto_hip, H.init_traj_straightline)
    assert TOS.traj.X.shape == (6, N) and np.abs(TOS.traj.X[:, -1] - lo[qs[0], 2]).max() <= tol
    with pytest.raises(ValueError):
        H.solve_SCP_timeline_batch(TOSs, TOPs[:2])


# ---- 7. refusals and state errors ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_as_it_was():
    """every GUSTO_ERR_ARG of gusto_legs_begin, before a timeline and with one begun: B, problems, trajectories and the stage
    stay, gusto_last_error names the cause; the GUSTO_ERR_STATE of advance and the getters"""
    from test_legs_cpu import refusal_cases
    n, Bq, L, N = 6, 2, 3, 6
    base, cases = refusal_cases(n, Bq, L)
    s = g.BatchSolver(0, N, Bq * L, hist_cap=8)
    Lb, h = s.L, s.h
    O = g._capi.LegsOpts

    def call(handle=None, **over):
        a = dict(base, **over)
        keep = [None if a[k] is None else np.ascontiguousarray(a[k], float) for k in ("x_init", "goal_lo", "goal_hi", "t_goal")]
        nl = None if a["n_legs"] is None else np.ascontiguousarray(a["n_legs"], np.int32)
        return Lb.gusto_legs_begin(handle or h, a["Bq"], a["L"], None if nl is None else nl.ctypes.data,
                                   *[None if k is None else k.ctypes.data for k in keep], C.byref(O(a["mode"])))

    rep, ms = g._capi.LegsReport(), C.c_double()
    none = lambda: (Lb.gusto_legs_advance(h, None), Lb.gusto_get_legs(h, C.byref(rep), None, None),
                    Lb.gusto_get_legs_dev(h, None, None, None), Lb.gusto_last_legs_ms(h, C.byref(ms)))
    words = {"trajopt": b"TrajOpt", "L_low": b"GUSTO_MAX_STARTS", "L_high": b"GUSTO_MAX_STARTS", "Bq": b"Bq", "mode": b"mode",
             "legs_low": b"n_legs", "legs_high": b"n_legs", "x_nan": b"x_init", "x_inf": b"x_init", "parallel_partial": b"PARALLEL",
             "cap_parallel": b"batch_cap", "cap_sequential": b"batch_cap"}
    assert none() == (-3, -3, -3, -3) and Lb.gusto_legs_begin(None, Bq, L, None, None, None, None, None, None) == -1
    for begun in (False, True):
        if begun:
            assert call() == 0
            s.B, s._legs = Bq * L, (Bq, L)
            before, rep0 = s.traj(), s.legs_info()
        for name, over, _ in cases:
            if name == "trajopt":
                continue
            if name == "cap_parallel":
                over = dict(Bq=Bq + 1, x_init=np.zeros((Bq + 1, n)), goal_lo=np.zeros((Bq + 1, L, n)), goal_hi=np.zeros((Bq + 1, L, n)),
                            t_goal=np.tile(base["t_goal"][:1], (Bq + 1, 1)))
            if name == "cap_sequential":
                over = dict(Bq=Bq * L + 1, x_init=np.zeros((Bq * L + 1, n)), goal_lo=np.zeros((Bq * L + 1, L, n)),
                            goal_hi=np.zeros((Bq * L + 1, L, n)), t_goal=np.tile(base["t_goal"][:1], (Bq * L + 1, 1)), mode=NL.SEQUENTIAL)
            assert call(**over) == -1, name
            err = Lb.gusto_last_error(h)
            assert b"gusto_legs_begin" in err and words.get(name, b"null" if name.startswith("null") else b"T_0") in err, (name, err)
        if not begun:
            assert Lb.gusto_get_traj(h, None, None) == -3 and none() == (-3, -3, -3, -3)     # still without problems
        else:
            after, rep1 = s.traj(), s.legs_info()
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and all(same(rep0[k], rep1[k]) for k in REPORT)
            assert rep1["n_flying"] == Bq and rep1["round"] == 0
    # state errors
    assert Lb.gusto_legs_advance(h, None) == -3 and b"gusto_solve" in Lb.gusto_last_error(h)      # a solve is still needed
    assert s.legs_advance(np.ones(Bq * L)) == 0                                                   # a caller's eligibility needs none
    assert Lb.gusto_legs_advance(h, np.ones(Bq * L, np.int32).ctypes.data) == -3 and b"flying" in Lb.gusto_last_error(h)
    assert s.legs_info()["n_flying"] == 0 and s.last_legs_ms() > 0
    assert call(mode=NL.SEQUENTIAL) == 0
    s.B = Bq
    s.solve(1)
    assert Lb.gusto_legs_advance(h, None) == 0 and Lb.gusto_legs_advance(h, None) == -3           # ... and again after the advance
    s.set_problems(base["x_init"], base["goal_lo"][:, 0], base["goal_hi"][:, 0], base["t_goal"][:, 0])     # other problems: the timeline is gone
    assert none() == (-3, -3, -3, -3)
    assert call() == 0
    s.set_problems_multistart(base["x_init"], base["goal_lo"][:, 0], base["goal_hi"][:, 0], base["t_goal"][:, 0], np.zeros((2, 2)))
    assert none() == (-3, -3, -3, -3)
    s.close()
    t = g._capi.TrajOptSolver(0, N, Bq * L)
    assert call(handle=t.h) == -1 and b"TrajOpt" in t.L.gusto_last_error(t.h)
    t.set_problems(base["x_init"], base["goal_lo"][:, 0], base["goal_hi"][:, 0], base["t_goal"][:, 0])
    assert t.L.gusto_legs_advance(t.h, None) == -1 and t.L.gusto_get_legs(t.h, None, None, None) == -1
    t.close()


# ---- 8. the C consumer --------------------------------------------------------------------------------------------------------
def test_c_consumer(tmp_path):
    """tests/c/c_abi_legs.c, a plain C consumer with checks of its own; the report it prints is the Python path's"""
    exe = os.path.join(tmp_path, "c_abi_legs")
    lib = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "c_abi_legs.c"),
                           "-o", exe, "-L" + lib, "-lgusto_hip", "-lm", "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 3
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.4, 1.9, 0, 0, 0, 0]], float)
    inf = np.inf
    lo = np.array([[[1.0, 2.2, -inf, -inf, -inf, -inf], [3.0, 0.5, 0, 0.05, -0.05, 0]], [[1.2, 0.6, -inf, -inf, -inf, -inf], [3.0, 0.5, 0, 0.05, -0.05, 0]]])
    hi = np.where(np.isinf(lo), inf, lo)
    s = g.BatchSolver(0, 20, 2, hist_cap=64, boxes=np.array([[1.4, 0.9, -0.2, 1.8, 1.5, 0.2]]))
    assert s.legs_begin(x0, lo, hi, [[40.0, 90.0], [50.0, 90.0]]) == "sequential"
    while True:
        s.solve(30)
        if s.legs_advance() == 0:
            break
    r = s.legs_info()
    s.close()
    for q in range(2):
        v = lines[1 + q].split()
        assert (int(v[0]), int(v[1]), int(v[2])) == (r["status"][q], r["failed_leg"][q], r["n_done"][q])
        assert same(np.array([float(x) for x in v[3:]]), np.array([r["J_total"][q], r["gap"][q, 1], r["arrive"][q, 0], r["arrive"][q, 1], r["t"][q, 19], r["t"][q, 20]]))
