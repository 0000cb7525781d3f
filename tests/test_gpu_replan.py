"""Receding-horizon replanning on the device -- gusto_set_problems_replan, gusto_set_problems_replan_knots, gusto_get_replan,
gusto_last_replan_ms -- against tests/np_replan.py, the numpy restatement (tests/test_replan_cpu.py proves it without a GPU),
against gusto_set_problems on a second handle, and on the knot-5 study of the CPU test: the 48 table queries replanned from the
shifted plan and from the straight line.

Tolerances.  Everything is compared bit for bit except the seeded X0, U0 against the restatement:
|dev - np| <= 1e-12 * max(1, max|X_s|, max|x_now|).  The device may contract multiply-adds, and a sigma within an ulp of an integer
may pick the other interval; the interpolant is continuous there, so both choices differ by at most Ns * 2^-52 * max|dX|, which
with Ns <= 256 and entries <= 10 stays well inside the tolerance.
The functional study: over the queries the first solve answered, warm trips (sum) <= 0.5 * cold trips -- the oracle's ratio is
148 / 469 = 0.32 (test_replan_cpu.py), the margin covers device / oracle iteration differences -- and the warm successful count is
at most one below the cold one (equal on the oracle)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import np_replan as RP

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAUS = np.array([0.0, 0.25, 10 / 49, 0.999])
ARG, STATE = -1, -3


def problem_arrays(s):
    """(x_init, goal centre [B, n], tf [B]) of a handle's problems as the device holds them, through a trajectory library"""
    lib = g.TrajLib(s.model, s.N, s.B)
    assert lib.add_from(s, np.ones(s.B)) == s.B
    d = lib.get()
    lib.close()
    return d["x_init"], d["goal_c"], d["tf"]


def random_source(model, Ns, B, rng, cap=None):
    """a handle that holds B random trajectories as its problems' current X, U; (solver, dict of what it holds)"""
    n, m = RP.X_DIM[model], RP.U_DIM[model]
    d = dict(x=rng.uniform(-3, 3, (B, n)), lo=rng.uniform(-3, 3, (B, n)), tf=rng.uniform(20, 60, B), X=rng.uniform(-3, 3, (B, Ns, n)),
             U=rng.normal(size=(B, Ns, m)))
    d["hi"] = d["lo"] + rng.uniform(0, 0.3, (B, n))
    d["hi"][0, n - 1] = np.inf                                  # (its centre is 0)
    s = g.BatchSolver(model, Ns, cap or B, hist_cap=8)
    s.set_problems(d["x"], d["lo"], d["hi"], d["tf"], d["X"], d["U"])
    return s, d


def check_against_restatement(h, d, N, tau, x_now, seeded, goals):
    want = RP.replan(N, d["X"], d["U"], d["tf"], d["lo"], d["hi"], tau, x_now, seeded, *(goals or ()))
    X, U = h.traj()
    tol = 1e-12 * max(1.0, np.abs(d["X"]).max(), np.abs(x_now).max())
    ex, eu = np.abs(X - want["X0"]).max(), np.abs(U - want["U0"]).max()
    print("N = %d: max |X0 - np| = %.3g, max |U0 - np| = %.3g, tolerance %.3g" % (N, ex, eu, tol))
    assert ex <= tol and eu <= tol
    sd = np.asarray(seeded, bool)
    assert np.array_equal(X[:, 0], x_now) and not U[~sd].any()
    xi, c, tf = problem_arrays(h)
    assert np.array_equal(xi, x_now) and np.array_equal(tf, want["tf"]) and np.array_equal(c, RP.goal_centre(want["goal_lo"], want["goal_hi"]))
    info = h.replan_info()
    assert np.array_equal(info["seeded"], sd) and np.array_equal(info["tau"], tau) and np.array_equal(info["x_now"], x_now)
    assert h.last_replan_ms() > 0 and h.B == len(x_now)


def new_goals(d, rng):
    lo = d["lo"] + rng.uniform(-0.5, 0.5, d["lo"].shape)
    hi = lo + rng.uniform(0, 0.3, lo.shape)
    hi[1, 0] = np.inf
    return lo, hi


# ---- 1. restatement parity ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 5, 50, 65])
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_against_the_restatement_in_place(model, N):
    """src = NULL: X0, U0 right after the call, x_init, the goal centres and tf; every tau, seeded and not, with and without goals"""
    rng = np.random.default_rng(100 * model + N)
    B, n = 8, RP.X_DIM[model]
    tau, seeded = np.tile(TAUS, 2), np.array([1, 1, 1, 1, 1, 0, 1, 1])
    for with_goals in (False, True):
        s, d = random_source(model, N, B, rng)
        x_now = rng.uniform(-3, 3, (B, n))
        goals = new_goals(d, rng) if with_goals else None
        s.set_problems_replan(tau, x_now, mask=seeded, **(dict(goal_lo=goals[0], goal_hi=goals[1]) if goals else {}))
        check_against_restatement(s, d, N, tau, x_now, seeded, goals)
        s.close()


@pytest.mark.parametrize("Ns,N", [(7, 12), (7, 13), (50, 12), (50, 13)])
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_against_the_restatement_between_horizons(model, Ns, N):
    rng = np.random.default_rng(1000 * model + 10 * Ns + N)
    B, n = 8, RP.X_DIM[model]
    tau, seeded = np.tile(TAUS, 2), np.array([1, 1, 1, 1, 0, 1, 1, 1])
    s, d = random_source(model, Ns, B, rng)
    h = g.BatchSolver(model, N, B, hist_cap=8)
    for with_goals in (False, True):
        x_now = rng.uniform(-3, 3, (B, n))
        goals = new_goals(d, rng) if with_goals else None
        h.set_problems_replan(tau, x_now, src=s, mask=seeded, **(dict(goal_lo=goals[0], goal_hi=goals[1]) if goals else {}))
        check_against_restatement(h, d, N, tau, x_now, seeded, goals)
    Xs, Us = s.traj()
    assert np.array_equal(Xs, d["X"]) and np.array_equal(Us, d["U"])        # the source is read only
    s.close()
    h.close()


# ---- 2. identity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_identity_returns_the_source_bits(model):
    """tau = 0, Ns = N, x_now = X_s[0], no goals: only exact zeros are added; in place and from a source handle"""
    rng = np.random.default_rng(model)
    for N in (3, 50):
        s, d = random_source(model, N, 5, rng)
        h = g.BatchSolver(model, N, 5, hist_cap=8)
        h.set_problems_replan(0.0, d["X"][:, 0], src=s, mask=np.ones(5))
        s.set_problems_replan(0.0, d["X"][:, 0], mask=np.ones(5))
        for k in (h, s):
            X, U = k.traj()
            assert X.tobytes() == d["X"].tobytes() and U.tobytes() == d["U"].tobytes()
            assert np.array_equal(problem_arrays(k)[2], d["tf"])
            k.close()


# ---- 3. unseeded problems -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_unseeded_problems_are_set_problems_straight_lines(model):
    """mask = 0 and unconverged sources: bit for bit a second handle's gusto_set_problems(x_now, goals, tf', NULL)"""
    rng = np.random.default_rng(40 + model)
    B, n, N = 5, RP.X_DIM[model], 50
    s, d = random_source(model, N, B, rng)
    t = g.BatchSolver(model, N, B, hist_cap=8)
    tau, x_now = rng.uniform(0, 0.9, B), rng.uniform(-3, 3, (B, n))
    nlo, nhi = new_goals(d, rng)
    sp, mp = g.default_params(model)
    for mask in (np.zeros(B), None):                             # (nothing was solved: no source is converged)
        for goals in (None, (nlo, nhi)):
            lo, hi = goals or (d["lo"], d["hi"])
            h = g.BatchSolver(model, N, B, hist_cap=8)
            h.set_problems_replan(tau, x_now, src=s, mask=mask, **(dict(goal_lo=lo, goal_hi=hi) if goals else {}))
            assert not h.replan_info()["seeded"].any()
            t.set_problems(x_now, lo, hi, (1 - tau) * d["tf"])
            (X, U), (Xt, Ut) = h.traj(), t.traj()
            assert X.tobytes() == Xt.tobytes() and U.tobytes() == Ut.tobytes() and not U.any()
            for a, b in zip(problem_arrays(h), problem_arrays(t)):
                assert a.tobytes() == b.tobytes()
            subs = [k.subproblem(X, U, sp.Delta0, sp.omega0, sp.Delta0 / 8 + mp.clearance) for k in (h, t)]   # reads goal_lo and goal_hi
            for f in ("X", "U", "obj", "status", "iters", "dual"):
                assert np.array_equal(subs[0][f], subs[1][f], equal_nan=True), f
            h.close()
    s.close()
    t.close()


# ---- 4. in place ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N", [(0, 50), (1, 3), (2, 65), (3, 5)])
def test_in_place_equals_a_separate_source(model, N):
    rng = np.random.default_rng(7 * model + N)
    B, n = 9, RP.X_DIM[model]
    s, d = random_source(model, N, B, rng, cap=12)
    tau, x_now, mask = rng.uniform(0, 0.999, 6), rng.uniform(-3, 3, (6, n)), np.array([1, 0, 1, 1, 1, 1])
    nlo, nhi = new_goals(d, rng)
    for goals in ({}, dict(goal_lo=nlo[:6], goal_hi=nhi[:6])):
        a, _ = random_source(model, N, B, np.random.default_rng(7 * model + N), cap=12)      # the same trajectories again
        h = g.BatchSolver(model, N, 12, hist_cap=8)
        h.set_problems_replan(tau, x_now, src=s, mask=mask, **goals)                          # B = 6 of the source's 9
        a.set_problems_replan(tau, x_now, mask=mask, **goals)
        (X, U), (Xa, Ua) = h.traj(), a.traj()
        assert a.B == 6 and X.tobytes() == Xa.tobytes() and U.tobytes() == Ua.tobytes()
        for p, q in zip(problem_arrays(h), problem_arrays(a)):
            assert p.tobytes() == q.tobytes()
        h.close()
        a.close()
    s.close()


# ---- 5. batch independence ------------------------------------------------------------------------------------------------------------
def test_a_problems_start_does_not_depend_on_the_batch():
    rng = np.random.default_rng(5)
    B, model, Ns, N = 64, 2, 50, 13
    s, d = random_source(model, Ns, B, rng)
    h = g.BatchSolver(model, N, B, hist_cap=8)
    tau, x_now = rng.uniform(0, 0.999, B), rng.uniform(-3, 3, (B, 12))
    mask = np.arange(B) % 5 != 0
    h.set_problems_replan(tau, x_now, src=s, mask=mask)
    Xb, Ub = h.traj()
    tfb = problem_arrays(h)[2]
    for b in (0, 1, 63):
        one = g.BatchSolver(model, Ns, 1, hist_cap=8)
        one.set_problems(d["x"][b], d["lo"][b], d["hi"][b], d["tf"][b], d["X"][b], d["U"][b])
        h.set_problems_replan(tau[b], x_now[b], src=one, mask=mask[b:b + 1])
        X, U = h.traj()
        assert X[0].tobytes() == Xb[b].tobytes() and U[0].tobytes() == Ub[b].tobytes() and problem_arrays(h)[2][0] == tfb[b]
        one.close()
    s.close()
    h.close()


# ---- 6. from the stored knots ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def flown():
    """8 table queries solved, tracked and flown with two samples and the knots stored (shared; the handle is not written to)"""
    P = g.problems
    x0, lo, hi, tf = P.freeflyer_batch(8)
    s = g.BatchSolver(0, 50, 8, hist_cap=40, boxes=P.freeflyer_env())
    s.set_problems(x0, lo, hi, tf)
    s.solve(30)
    s.tvlqr({})
    s.simulate(dict(n_samples=2, store_knots=1))
    return dict(s=s, Xcl=s.get_simulate_knots(), traj=s.traj(), st=s.status(), q=(x0, lo, hi, tf))


def test_knots_entry_equals_the_general_call():
    d = flown()
    s, Xcl = d["s"], d["Xcl"]
    knot = np.array([5, 0, 48, 25, 5, 1, 47, 10])
    a, b = (g.BatchSolver(0, 50, 8, hist_cap=8) for _ in range(2))
    a.set_problems_replan_knots(knot, 1, src=s)
    x_now = Xcl[np.arange(8), knot, 1]
    b.set_problems_replan(knot / 49, x_now, src=s)
    (Xa, Ua), (Xb, Ub) = a.traj(), b.traj()
    assert Xa.tobytes() == Xb.tobytes() and Ua.tobytes() == Ub.tobytes()
    ia, ib = a.replan_info(), b.replan_info()
    assert all(ia[k].tobytes() == ib[k].tobytes() for k in ia) and ia["x_now"].tobytes() == x_now.tobytes()
    assert np.array_equal(ia["seeded"], d["st"]["converged"] & d["st"]["successful"]) and ia["seeded"].any()
    for p, q in zip(problem_arrays(a), problem_arrays(b)):
        assert p.tobytes() == q.tobytes()
    assert np.array_equal(a._tf, problem_arrays(a)[2])          # the host's record of tf' is the device's
    a.set_problems_replan_knots(5, 0, src=s, B=3)               # sample 0 is the unperturbed one: the plan's own knot
    assert a.B == 3 and np.array_equal(a.replan_info()["x_now"], Xcl[:3, 5, 0])
    (X, U), (Xs, Us) = s.traj(), d["traj"]
    assert X.tobytes() == Xs.tobytes() and U.tobytes() == Us.tobytes()
    a.close()
    b.close()


# ---- 7. GUSTO_REPLAN_BEST -----------------------------------------------------------------------------------------------------------
def test_best_source():
    """multi-start K = 3, solve, select_best with query 2 made to have no winner: the seeded starts against the restatement on
    gusto_get_best's rows, query 2 the straight line bit for bit; src = h gives the same bits as a separate handle"""
    P = g.problems
    K, Bq = 3, 4
    x0, lo, hi, tf = P.freeflyer_batch(Bq)
    tf = tf * np.array([1.0, 0.9, 0.8, 0.7])
    s = g.BatchSolver(0, 50, Bq * K, hist_cap=40, boxes=P.freeflyer_env())
    s.set_problems_multistart(x0, lo, hi, tf, [(0, 0), (0.5, 0), (-0.5, 0)])
    s.solve(30)
    st = s.status()
    elig = st["converged"] & st["successful"]
    elig[2 * K:3 * K] = False
    best = s.select_best(K, eligible=elig)
    won = best["winner"] >= 0
    assert won.sum() >= 2 and not won[2]
    rng = np.random.default_rng(9)
    tau = np.array([0.1, 0.25, 0.5, 10 / 49])
    x_now = best["X"][:, 5] + rng.uniform(-0.02, 0.02, (Bq, 6))
    x_now[2] = x0[2]
    h, t = g.BatchSolver(0, 50, Bq, hist_cap=8), g.BatchSolver(0, 50, 1, hist_cap=8)
    h.set_problems_replan(tau, x_now, src=s, source="best")
    d = dict(X=best["X"], U=best["U"], tf=tf, lo=lo, hi=hi)       # (a query's K starts share tf and goals)
    check_against_restatement(h, d, 50, tau, x_now, won, None)
    t.set_problems(x_now[2], lo[2], hi[2], (1 - tau[2]) * tf[2])
    X, U = h.traj()
    assert X[2].tobytes() == t.traj()[0][0].tobytes() and not U[2].any()
    h.set_problems_replan(tau, x_now, src=s, source="best", mask=[1, 0, 1, 1])     # a mask never seeds a query without a winner
    assert np.array_equal(h.replan_info()["seeded"], won & np.array([1, 0, 1, 1], bool))
    h.set_problems_replan(tau, x_now, src=s, source="best")
    s.set_problems_replan(tau, x_now, source="best")              # in place: B becomes Bq
    (Xh, Uh), (Xs, Us) = h.traj(), s.traj()
    assert s.B == Bq and Xh.tobytes() == Xs.tobytes() and Uh.tobytes() == Us.tobytes()
    assert np.array_equal(problem_arrays(s)[2], (1 - tau) * tf)
    for k in (s, h, t):
        k.close()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals():
    """every refusal returns its code and leaves the handle's trajectories, status and B as they were"""
    P = g.problems
    L = g.lib()
    x0, lo, hi, tf = P.freeflyer_batch(4)
    ptr = lambda a: None if a is None else a.ctypes.data
    s = g.BatchSolver(0, 50, 6, hist_cap=40, boxes=P.freeflyer_env())
    fresh, other, short = g.BatchSolver(0, 50, 6, hist_cap=8), g.BatchSolver(1, 50, 6, hist_cap=8), g.BatchSolver(0, 7, 2, hist_cap=8)
    to = g._capi.TrajOptSolver(0, 50, 6)
    tau, x_now = np.full(6, 0.25), np.ascontiguousarray(np.tile(x0[0], (6, 1)))
    knot = np.full(6, 5, np.int32)

    def call(h=s, src=None, source=0, B=4, tau=tau, x_now=x_now, lo=None, hi=None):
        return L.gusto_set_problems_replan(h.h, None if src is None else src.h, source, B, ptr(tau), ptr(x_now), ptr(lo), ptr(hi), None)

    def knots(h=s, src=None, B=4, knot=knot, sample=1, lo=None, hi=None):
        return L.gusto_set_problems_replan_knots(h.h, None if src is None else src.h, B, ptr(knot), sample, ptr(lo), ptr(hi), None)

    ms = C.c_double()
    # a handle without problems, as source and as destination
    assert call(h=fresh) == STATE and knots(h=fresh) == STATE and call(src=fresh) == STATE
    assert L.gusto_get_replan(fresh.h, None, None, None) == STATE and L.gusto_last_replan_ms(fresh.h, C.byref(ms)) == STATE
    assert L.gusto_get_traj(fresh.h, None, None) == STATE                                    # ... which it still is
    assert L.gusto_set_problems_replan(None, None, 0, 4, ptr(tau), ptr(x_now), None, None, None) == ARG
    assert L.gusto_get_replan(None, None, None, None) == ARG and L.gusto_last_replan_ms(s.h, None) == ARG
    s.set_problems(x0, lo, hi, tf)
    s.solve(30)
    before = s.traj(), s.status()

    def unchanged():
        a = [np.full(6, -7, np.int32) for _ in range(5)]
        assert L.gusto_get_status(s.h, *[x.ctypes.data for x in a]) == 0
        for x, k in zip(a, ("iterations", "converged", "successful", "stop_reason", "ipm_iters")):
            assert np.array_equal(x[:4], before[1][k].astype(np.int32)) and (x[4:] == -7).all(), k     # B is still 4
        X, U = s.traj()
        assert X.tobytes() == before[0][0].tobytes() and U.tobytes() == before[0][1].tobytes()

    bad = lambda i, v: np.ascontiguousarray(np.where(np.arange(6) == i, v, tau))
    bad_x = lambda v: np.ascontiguousarray(np.where(np.arange(36).reshape(6, 6) == 13, v, x_now))
    glo = np.ascontiguousarray(np.tile(lo[0], (6, 1)))
    other.set_problems(np.zeros((4, 3)), np.ones((4, 3)), np.ones((4, 3)), 10.0)
    short.set_problems(x0[:2], lo[:2], hi[:2], tf[:2])
    to.set_problems(x0, lo, hi, tf)
    for rc, want in ((call(B=0), ARG), (call(B=7), ARG), (call(B=5), ARG),                    # 5: above the source's count
                     (call(src=short, B=3), ARG), (call(source=2), ARG), (call(source=-1), ARG), (call(tau=None), ARG),
                     (call(x_now=None), ARG), (call(lo=glo), ARG), (call(hi=glo), ARG), (call(tau=bad(1, -0.1)), ARG),
                     (call(tau=bad(3, 1.0)), ARG), (call(tau=bad(0, np.nan)), ARG), (call(x_now=bad_x(np.inf)), ARG),
                     (call(x_now=bad_x(np.nan)), ARG), (call(src=other), ARG), (call(src=to), ARG), (call(source=1), STATE),
                     (knots(), STATE), (knots(lo=glo), ARG), (knots(knot=None), ARG)):
        assert rc == want, (rc, want, L.gusto_last_error(s.h))
        unchanged()
    assert call(h=to) == ARG and b"TrajOpt" in L.gusto_last_error(to.h) and knots(h=to) == ARG and call(h=other, src=s) == ARG
    with pytest.raises(g.GustoError):
        to.set_problems_replan()
    assert L.gusto_get_replan(s.h, None, None, None) == STATE and L.gusto_last_replan_ms(s.h, C.byref(ms)) == STATE
    # with stored knots: the knot and the sample
    s.tvlqr({})
    s.simulate(dict(n_samples=2, store_knots=1))
    kbad = lambda v: np.ascontiguousarray(np.where(np.arange(6) == 2, v, knot).astype(np.int32))
    for rc in (knots(knot=kbad(-1)), knots(knot=kbad(49)), knots(sample=-1), knots(sample=2), knots(B=5), knots(B=0), knots(B=7)):
        assert rc == ARG, L.gusto_last_error(s.h)
        unchanged()
    assert knots(h=fresh, src=s, knot=kbad(49)) == ARG and L.gusto_get_traj(fresh.h, None, None) == STATE
    s.simulate(dict(n_samples=2))                                                            # a roll-out without stored knots
    assert knots() == STATE
    unchanged()
    assert call() == 0 and L.gusto_get_replan(s.h, None, None, None) == 0                    # and the call itself
    for k in (s, fresh, other, short, to):
        k.close()


# ---- 9. after-effects ---------------------------------------------------------------------------------------------------------------
def test_after_effects_are_those_of_set_problems():
    P = g.problems
    L = g.lib()
    x0, lo, hi, tf = P.freeflyer_batch(4)
    s = g.BatchSolver(0, 50, 8, hist_cap=40, boxes=P.freeflyer_env())
    s.set_problems(np.repeat(x0, 2, 0), np.repeat(lo, 2, 0), np.repeat(hi, 2, 0), np.repeat(tf, 2))
    fresh = s.history()
    s.set_active(np.arange(8) < 2)
    s.solve(30)
    s.set_active(None)
    s.solve(30)
    s.verify(nstep=1)
    s.tvlqr({})
    s.select_best(2)
    vr = C.byref(g._capi.VerifyReport())
    h = s.h
    assert L.gusto_get_verify(h, vr) == 0 and L.gusto_get_best(h, None) == 0 and L.gusto_get_tvlqr(h, None, None, None, None, None) == 0
    X, _ = s.traj()
    s.set_active(np.arange(8) < 2)
    s.set_problems_replan(0.1, X[:6, 5], goal_lo=lo[0] - 0.01, goal_hi=hi[0] + 0.01)
    st, hh = s.status(), s.history()
    assert s.B == 6 and not st["iterations"].any() and not st["converged"].any() and not st["successful"].any()
    for k in ("n_hist", "nJ", "n_rho"):
        assert np.array_equal(hh[k], fresh[k][:6]), k
    assert L.gusto_get_verify(h, vr) == STATE and L.gusto_get_best(h, None) == STATE and L.gusto_get_tvlqr(h, None, None, None, None, None) == STATE
    assert L.gusto_get_replan(h, None, None, None) == 0
    # the box goal reached the device: one subproblem equals that of gusto_set_problems with the same inputs and trajectories
    sp, mp = g.default_params(0)
    X0, U0 = s.traj()
    sub = s.subproblem(X0, U0, sp.Delta0, sp.omega0, sp.Delta0 / 8 + mp.clearance)
    t = g.BatchSolver(0, 50, 8, hist_cap=40, boxes=P.freeflyer_env())
    t.set_problems(X[:6, 5], np.tile(lo[0] - 0.01, (6, 1)), np.tile(hi[0] + 0.01, (6, 1)), s._tf, X0, U0)
    again = t.subproblem(X0, U0, sp.Delta0, sp.omega0, sp.Delta0 / 8 + mp.clearance)
    for f in ("X", "U", "obj", "status", "iters", "dual"):
        assert np.array_equal(sub[f], again[f], equal_nan=True), f
    s.solve(2)
    assert (s.status()["iterations"] >= 1).all()              # the active mask is cleared: every problem iterates
    s.set_problems(x0, lo, hi, tf)
    ms = C.c_double()
    assert L.gusto_get_replan(h, None, None, None) == STATE and L.gusto_last_replan_ms(h, C.byref(ms)) == STATE
    s.close()
    t.close()


# ---- 10. the functional study -------------------------------------------------------------------------------------------------------
def test_warm_replans_need_half_the_trips_of_cold_ones():
    from test_replan_cpu import STUDY_B, STUDY_COLD, STUDY_WARM
    P = g.problems
    env = P.freeflyer_env()
    x0, lo, hi, tf = P.freeflyer_batch(STUDY_B)
    s, w, c = (g.BatchSolver(0, 50, STUDY_B, hist_cap=40, boxes=env) for _ in range(3))
    s.set_problems(x0, lo, hi, tf)
    s.solve(30)
    st = s.status()
    ok = st["converged"] & st["successful"]
    X, _ = s.traj()
    x_now = X[:, 5] + np.stack([RP.perturbation(q) for q in range(STUDY_B)])
    w.set_problems_replan(5 / 49, x_now, src=s)
    assert np.array_equal(w.replan_info()["seeded"], ok)
    c.set_problems(x_now, lo, hi, (1 - 5 / 49) * tf)
    out = {}
    for name, k in (("warm", w), ("cold", c)):
        k.solve(30)
        r = k.status()
        out[name] = (int((r["converged"] & r["successful"])[ok].sum()), int(r["iterations"][ok].sum()), int(r["iterations"][ok].max()),
                     k.last_solve_ms())
    print("first solve answered %d of %d; replanned at knot 5 (successful, SCP trips, longest, solve ms): warm %s, cold %s; oracle: warm %s, cold %s"
          % (ok.sum(), STUDY_B, out["warm"], out["cold"], STUDY_WARM[5], STUDY_COLD[5]))
    assert out["warm"][1] <= 0.5 * out["cold"][1]
    assert out["warm"][0] >= out["cold"][0] - 1
    for k in (s, w, c):
        k.close()


# ---- 11. the host driver ------------------------------------------------------------------------------------------------------------
def test_host_receding_driver():
    """3 steps of 5 knots on 8 queries: each step's x_init is the previous roll-out's state at the knot, tf shrinks by 1 - 5 / 49 per
    step, and the result equals the same sequence of BatchSolver calls made by hand"""
    from test_gpu_multistart import host_problems
    H, P = g.host, g.problems
    TOPs, TOSs = host_problems(8)
    out = H.solve_SCP_receding_batch(TOSs, TOPs, 3, 5)
    x0, lo, hi, tf = P.freeflyer_batch(8)
    sp, mp = g.default_params(0)
    s = g.BatchSolver(0, 50, 8, hist_cap=H._hist_cap(30), boxes=P.freeflyer_env(), scp_params=sp, model_params=mp)
    s.set_problems(x0, lo, hi, tf)
    assert len(out) == 3
    tf_now = tf
    for step in range(3):
        xi, _, tf_dev = problem_arrays(s)
        assert np.array_equal(tf_dev, tf_now) and np.array_equal(s._tf, tf_now)
        tf_last, tf_now = tf_now, (1 - 5 / 49) * tf_now
        if step:
            assert xi.tobytes() == out[step - 1]["x_now"].tobytes()
        s.solve(30)
        st, (X, U) = s.status(), s.traj()
        s.tvlqr({})
        s.simulate_disturbed(dict(n_samples=2, store_knots=1))
        Xcl = s.get_simulate_knots()
        s.set_problems_replan_knots(5, 1)
        o = out[step]
        assert o["x_now"].tobytes() == Xcl[:, 5, 1].tobytes() and np.array_equal(o["tau"], np.full(8, 5 / 49))
        assert np.array_equal(o["seeded"], st["converged"] & st["successful"]) and np.array_equal(o["iterations"], st["iterations"])
        assert np.array_equal(o["converged"], st["converged"]) and np.array_equal(o["successful"], st["successful"])
        assert o["solve_ms"] > 0 and o["replan_ms"] > 0
    for q in range(8):                                            # TOSs take the last plan
        assert np.array_equal(TOSs[q].SCPS.traj.X.T, X[q]) and np.array_equal(TOSs[q].traj.U.T, U[q])
        assert TOSs[q].traj.Tf == tf_last[q]
    with pytest.raises(ValueError, match="0.1"):                  # the reference's Tf >= 0.1
        H.replan_batch(s, 0.9999, Xcl[:, 5, 1])
    info = H.replan_batch(s, 0.5, Xcl[:, 5, 1])
    assert s.B == 8 and np.array_equal(info["tau"], np.full(8, 0.5))
    s.close()


# ---- 12. plain C --------------------------------------------------------------------------------------------------------------------
def test_c_consumer(tmp_path):
    """tests/c/c_abi_replan.c, a plain C consumer with checks of its own; what it prints is the Python path's"""
    exe = os.path.join(tmp_path, "c_abi_replan")
    libdir = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_replan.c"), "-o", exe, "-L" + libdir, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 4
    goal = [3.0, 0.5, 0, 0.05, -0.05, 0]
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.4, 1.9, 0, 0, 0, 0], [0.3, 0.4, 0, 0, 0, 0]], float)
    s = g.BatchSolver(0, 50, 3, hist_cap=64, boxes=np.array([[1.4, 0.9, -0.2, 1.8, 1.5, 0.2]]))
    s.set_problems(x0, np.tile(goal, (3, 1)), np.tile(goal, (3, 1)), [200.0, 150.0, 100.0])
    s.solve(30)
    s.tvlqr({})
    s.simulate(dict(n_samples=2, store_knots=1))
    s.set_problems_replan_knots(5, 1)
    info = s.replan_info()
    s.solve(30)
    it = s.status()["iterations"]
    for b in range(3):
        v = lines[1 + b].split()
        assert (int(v[0]), float(v[1]), float(v[2]), float(v[3]), int(v[4])) == (int(info["seeded"][b]), info["tau"][b], info["x_now"][b, 0],
                                                                                  info["x_now"][b, 1], it[b])
    s.close()
