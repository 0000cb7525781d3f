"""gusto_tfsearch_begin, gusto_tfsearch_update, gusto_get_tfsearch and gusto_get_tfsearch_dev on the device against
tests/np_tfsearch.py, the numpy restatement (tests/test_tfsearch_cpu.py proves it without a GPU), against gusto_set_problems on the
same handle, and on the study that motivates them: the first 12 table queries, searched in [4, 84] s, next to the CPU oracle.

Tolerances.  Everything is compared bit for bit except
  - the retimed seeds: 1e-12 * max(1, max|X0|, max|U0|), what tests/test_gpu_replan.py::check_against_restatement grants seeded
    starts, for the same reason (three roundings and the compiler's contraction); knot 0 bit for bit;
  - the comparison with the oracle: what tests/test_gpu_parity.py grants whole solves of freeflyerSE2 (one differing decision,
    PARITY_MAX_DIVERGED) among the interior round-0 candidates, and what test_gpu_multistart.py asks of winners for the answers.

Recorded on the MI355X (profiles/tfsearch.txt, section 2): all 96 round-0 verdicts of the study equal the oracle's (84 interior, 12
at a threshold); eight of the eleven tf_best are equal to the bit in either seed mode, queries 0, 9 and 11 (answers near 6 s, where
the later rounds are not monotone in tf) end one to nine cells of 0.123 s apart; the retimed seeds are within 1.8e-15 of the restatement."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import np_multistart as MS
import np_tfsearch as TS

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52
PARITY_MAX_DIVERGED = 1      # tests/test_gpu_parity.py: test_scp_parity_freeflyer
REPORT = ("status", "round_found", "n_eligible", "lo", "hi", "tf_best", "J_best", "cand", "X", "U")
FINISHED = TS.NONE | TS.DONE


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def queries(model, Bq, rng):
    """random queries with non-zero end rates; one goal coordinate of query 0 is unbounded (its centre is 0)"""
    n = MS.X_DIM[model]
    x_init, lo = rng.uniform(-2, 2, (Bq, n)), rng.uniform(-2, 2, (Bq, n))
    hi = lo + rng.uniform(0, 0.3, (Bq, n)) * (rng.uniform(size=(Bq, n)) < 0.5)
    hi[0, 1], lo[0, n - 1] = np.inf, -np.inf
    return x_init, lo, hi


# ---- 1. begin -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 4, 50, 64, 65])
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_begin_against_the_restatement(model, N):
    """the candidates bit for bit; X0, U0 bit for bit what gusto_set_problems with X0 = NULL writes on the same handle for the
    replicated inputs; the tf of every problem bit for bit through an update with that candidate alone eligible, which answers
    tf_best = the problem's tf on the device"""
    rng = np.random.default_rng(100 * model + N)
    n = MS.X_DIM[model]
    s = g.BatchSolver(model, N, 320, hist_cap=8)
    seed = "line" if model == 1 else "incumbent"
    for K in (1, 3, 64):
        for Bq in (1, 5):
            x_init, lo, hi = queries(model, Bq, rng)
            tf_lo, tf_hi = rng.uniform(1, 5, Bq), rng.uniform(20, 90, Bq)
            s.tfsearch_begin(x_init, lo, hi, tf_lo, tf_hi, K=K, seed=seed)
            assert s.B == Bq * K
            r = s.tfsearch_info()
            S = TS.Search(model, N, K, x_init, lo, hi, tf_lo, tf_hi, seed=g._capi.TFSEARCH_SEED[seed])
            ref = S.report()
            for k in REPORT:
                assert same(r[k], ref[k]), (K, Bq, k)
            assert r["round"] == 0 and r["n_searching"] == Bq and s.last_tfsearch_ms() > 0
            X, U = s.traj()
            xi, l, h, t, Xr, Ur = S.problems()
            assert np.abs(X - Xr).max() <= 4 * ULP * max(1.0, np.abs(Xr).max()) and not U.any() and U.shape == Ur.shape   # (the device fuses the line's sum)
            assert np.array_equal(X[:, 0], xi) and np.array_equal(X[:, -1], MS.goal_centre(l, h))
            for j in sorted({0, K // 2, K - 1}):          # tf of candidate j of every query
                el = np.zeros((Bq, K), bool)
                el[:, j] = True
                s.tfsearch_begin(x_init, lo, hi, tf_lo, tf_hi, K=K, seed=seed)
                s.tfsearch_update(el.reshape(-1))
                assert np.array_equal(s.tfsearch_info()["tf_best"], S.cand[:, j]), (K, Bq, j)
            s.tfsearch_begin(x_init, lo, hi, tf_lo, tf_hi, K=K, seed=seed)
            s.tfsearch_update(np.zeros(Bq * K))             # nothing eligible: lo = the largest tf of the query
            assert np.array_equal(s.tfsearch_info()["lo"], tf_hi)
            s.set_problems(xi, l, h, t)                     # the straight lines of the replicated inputs, same handle
            Xs, Us = s.traj()
            assert np.array_equal(X, Xs) and np.array_equal(U, Us)
    s.close()


# ---- 2. update with a caller's eligibility ------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", ["line", "incumbent"])
@pytest.mark.parametrize("name", ["k4", "k1", "k64", "ulp"])
def test_update_on_the_tables(name, seed):
    """the tables of tests/test_tfsearch_cpu.py::test_update_rule_on_hand_made_tables, no solve in between: status, bracket,
    round_found, n_eligible and the next candidates bit for bit; the incumbent X, U bit for bit the handle's rows of the winning
    problem (with retimed seeds the rows of a query differ from the second round on); the next seeds against the restatement"""
    from test_tfsearch_cpu import TABLES
    t = TABLES[name]
    K, Bq, N = t["K"], len(t["lo0"]), 5
    rng = np.random.default_rng(K)
    x_init, lo, hi = queries(0, Bq, rng)
    s = g.BatchSolver(0, N, Bq * K, hist_cap=8)
    s.tfsearch_begin(x_init, lo, hi, t["lo0"], t["hi0"], K=K, rtol=t["rtol"], seed=seed)
    S = TS.Search(0, N, K, x_init, lo, hi, t["lo0"], t["hi0"], t["rtol"], g._capi.TFSEARCH_SEED[seed])
    prob = S.problems()
    s2 = g.BatchSolver(0, N, Bq * K, hist_cap=8)          # the straight lines as gusto_set_problems writes them (they do not read tf)
    s2.set_problems(*prob[:4])
    Xline = s2.traj()[0]
    s2.close()
    for rnd, v in enumerate(t["verdicts"]):
        if not S.searching().any():
            break
        X, U = s.traj()
        left = s.tfsearch_update(v)
        assert left == S.update(v, X=X, U=U)
        r, ref = s.tfsearch_info(), S.report()
        for k in REPORT:
            assert same(r[k], ref[k]), (name, rnd, k, r[k], ref[k])
        assert r["round"] == rnd + 1 and r["n_searching"] == left
        for q in np.flatnonzero(r["round_found"] == rnd):
            w = int(np.flatnonzero(v.reshape(Bq, K)[q] & (prob[3].reshape(Bq, K)[q] == r["tf_best"][q]))[0])
            assert np.array_equal(r["X"][q], X[q * K + w]) and np.array_equal(r["U"][q], U[q * K + w])
        Xd, Ud, td = s.tfsearch_dev()
        assert np.array_equal(Xd.cpu().numpy(), r["X"]) and np.array_equal(Ud.cpu().numpy(), r["U"]) and same(td.cpu().numpy(), r["tf_best"])
        prob = S.problems(prob)
        Xn, Un = s.traj()
        scale = 1e-12 * max(1.0, np.abs(prob[4]).max(), np.abs(prob[5]).max())
        assert np.abs(Xn - prob[4]).max() <= scale and np.abs(Un - prob[5]).max() <= scale
        assert np.array_equal(Xn[:, 0], prob[0])
        line = ~np.repeat(S.searching() & (S.round_found >= 0), K) if seed == "incumbent" else np.ones(Bq * K, bool)
        assert np.array_equal(Xn[line], Xline[line]) and not Un[line].any()        # the line seeds: bit for bit
    s.close()


# ---- 3. retimed seeds on real numbers -----------------------------------------------------------------------------------------
def real_problems(model, Bq):
    P = g.problems
    if model == 0:
        x0, glo, ghi, _ = P.freeflyer_batch(Bq)
        return x0, glo, ghi, dict(boxes=P.freeflyer_env()), (4.0, 84.0)
    x0, glo, ghi, _ = P.astrobee_manifold_batch(Bq)
    boxes, sph = P.iss_corner_env(True)
    return x0, glo, ghi, dict(boxes=boxes, spheres=sph), (10.0, 90.0)


def solved_round(model, Bq, K=4, N=10, pick=None):
    """begin, two trips of every candidate, an update with the caller's eligibility (candidates 1 .. K - 1; query 1: none), on the
    handle and on the restatement: (solver, Search, report, next X0, U0, the restatement's problems)"""
    x0, glo, ghi, env, rng_tf = real_problems(model, Bq)
    if pick is not None:
        x0, glo, ghi = x0[pick], glo[pick], ghi[pick]
    Q = len(x0)
    s = g.BatchSolver(model, N, Q * K, hist_cap=16, **env)
    s.tfsearch_begin(x0, glo, ghi, *rng_tf, K=K, seed="incumbent")
    S = TS.Search(model, N, K, x0, glo, ghi, *rng_tf, seed=TS.SEED_INCUMBENT)
    prob = S.problems()
    s.solve(2, False)
    X, U = s.traj()
    h = s.history()
    J = np.array([h["J_true"][b, h["nJ"][b] - 1] if h["nJ"][b] > 0 else np.nan for b in range(Q * K)])
    el = np.tile(np.arange(K) >= 1, Q)
    if pick is None and Q > 1:
        el[K:2 * K] = False
    s.tfsearch_update(el)
    S.update(el, X=X, U=U, J=J)
    Xn, Un = s.traj()
    return s, S, s.tfsearch_info(), Xn, Un, S.problems(prob), (X, U)


@pytest.mark.parametrize("model", [0, 3])
def test_retimed_seeds_on_real_numbers(model):
    s, S, r, Xn, Un, prob, (X, U) = solved_round(model, 3)
    assert U.any() and same(r["J_best"], S.J_best) and np.isfinite(r["J_best"][[0, 2]]).all()
    for k in REPORT:
        assert same(r[k], S.report()[k]), k
    K = 4
    assert list(r["round_found"]) == [0, -1, 0] and np.array_equal(r["X"][0], X[1]) and np.array_equal(r["U"][2], U[2 * K + 1])
    scale = 1e-12 * max(1.0, np.abs(prob[4]).max(), np.abs(prob[5]).max())
    print("retimed seeds, model %d: max |X0 - restatement| %.3g, |U0 - restatement| %.3g, allowed %.3g"
          % (model, np.abs(Xn - prob[4]).max(), np.abs(Un - prob[5]).max(), scale))
    assert np.abs(Xn - prob[4]).max() <= scale and np.abs(Un - prob[5]).max() <= scale
    assert np.array_equal(Xn[:, 0], prob[0])                                  # knot 0: x_init itself
    assert Un[:K].any() and Un[2 * K:].any() and not Un[K:2 * K].any()        # query 1 is NONE: the line at hi
    assert np.array_equal(Xn[K:2 * K], np.repeat(Xn[K:K + 1], K, 0)) and np.array_equal(Xn[K, -1], MS.goal_centre(prob[1][K], prob[2][K]))
    others = [i for i in range(MS.X_DIM[model]) if i not in TS.RATES[model]]
    for q in (0, 2):
        for j in range(K):                                                    # outside the rate set: the incumbent's entries
            assert np.array_equal(Xn[q * K + j, 1:, :][:, others], r["X"][q, 1:, :][:, others])
    s.close()


# ---- 4. batch independence ----------------------------------------------------------------------------------------------------
def test_a_querys_report_and_seeds_do_not_depend_on_the_batch():
    K = 4
    s5, _, r5, X5, U5, _, _ = solved_round(0, 5)
    for q in (2, 4):
        s1, _, r1, X1, U1, _, _ = solved_round(0, 5, pick=[q])
        for k in REPORT:
            assert same(r1[k][0], r5[k][q]), (q, k)
        assert np.array_equal(X1, X5[q * K:(q + 1) * K]) and np.array_equal(U1, U5[q * K:(q + 1) * K])
        s1.close()
    s5.close()


# ---- 5. done queries are inactive ---------------------------------------------------------------------------------------------
def test_done_queries_are_inactive():
    """rtol = 0.5 in [4, 84] with K = 4: query 0 has nothing eligible (NONE), query 2 only 84 s (DONE: 84 - 64 <= 42), query 1 all
    (searching: 24 - 4 > 12).  The next solve iterates the problems of query 1 alone; the others are the straight line at tf = hi"""
    P = g.problems
    K, N = 4, 10
    x0, glo, ghi, _ = P.freeflyer_batch(3)
    s = g.BatchSolver(0, N, 3 * K, hist_cap=16, boxes=P.freeflyer_env())
    s.tfsearch_begin(x0, glo, ghi, 4.0, 84.0, K=K, rtol=0.5)
    s.solve(2)
    el = np.array([0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1])
    assert s.tfsearch_update(el) == 1
    r = s.tfsearch_info()
    assert list(r["status"]) == [TS.NONE | TS.DONE, TS.FLOOR, TS.DONE] and list(r["hi"]) == [84.0, 24.0, 84.0]
    assert np.array_equal(r["cand"][[0, 2]], np.full((2, K), 84.0))
    X0, U0 = s.traj()
    assert not s.status()["iterations"].any()
    s.solve(3)
    X1, U1 = s.traj()
    it = s.status()["iterations"]
    done = np.array([1, 1, 1, 1, 0, 0, 0, 0, 1, 1, 1, 1], bool)
    assert not it[done].any() and (it[~done] > 0).all()
    assert np.array_equal(X1[done], X0[done]) and np.array_equal(U1[done], U0[done]) and not np.array_equal(X1[~done], X0[~done])
    line = MS.straight_line(x0[0], glo[0], ghi[0], N)
    assert np.abs(X1[0] - line).max() <= 4 * ULP * max(1.0, np.abs(line).max()) and not U1[done].any()
    # a later update does not touch the done queries: the same report, the same rows
    assert s.tfsearch_update(np.ones(3 * K)) in (0, 1)
    r2 = s.tfsearch_info()
    for k in REPORT:
        assert same(r2[k][[0, 2]], r[k][[0, 2]]), k
    assert r2["round_found"][1] == 1
    X2, U2 = s.traj()
    assert np.array_equal(X2[done], X0[done]) and np.array_equal(U2[done], U0[done])
    # tf of the done queries' problems is hi: the same rows and verify's dense row count as gusto_set_problems at 84 s
    s.set_active(None)
    nfull = s.interpolate(dt_min=0.5)[0]
    s.set_problems(np.repeat(x0, K, 0), np.repeat(glo, K, 0), np.repeat(ghi, K, 0), np.full(3 * K, 84.0))
    Xs, _ = s.traj()
    assert np.array_equal(Xs[done], X2[done]) and np.array_equal(s.interpolate(dt_min=0.5)[0][done], nfull[done])
    s.close()


# ---- 6. refusals and state errors ---------------------------------------------------------------------------------------------
def test_refusals_and_state_errors():
    P = g.problems
    x0, glo, ghi, _ = P.freeflyer_batch(4)
    s = g.BatchSolver(0, 10, 12, hist_cap=8)
    L, h = s.L, s.h
    ptr = lambda a: None if a is None else np.ascontiguousarray(a, float).ctypes.data
    O = g._capi.TfsearchOpts

    def call(Bq=4, K=3, xi=x0, lo=glo, hi=ghi, tlo=None, thi=None, o=(4.0, 84.0, 0.01, 1)):
        keep = [np.ascontiguousarray(a, float) if a is not None else None for a in (xi, lo, hi, tlo, thi)]
        return L.gusto_tfsearch_begin(h, Bq, K, *[None if a is None else a.ctypes.data for a in keep], C.byref(O(*o)) if o else None)

    rep = g._capi.TfsearchReport()
    ms = C.c_double()
    none = lambda: (L.gusto_tfsearch_update(h, None), L.gusto_get_tfsearch(h, C.byref(rep), None, None),
                    L.gusto_get_tfsearch_dev(h, None, None, None), L.gusto_last_tfsearch_ms(h, C.byref(ms)))
    assert none() == (-3, -3, -3, -3)                                              # before begin
    refusals = [dict(K=0), dict(K=65), dict(Bq=0), dict(Bq=5), dict(Bq=13, K=1), dict(xi=None), dict(lo=None), dict(hi=None),
                dict(o=(0.0, 84.0, 0.01, 1)), dict(o=(4.0, 4.0, 0.01, 1)), dict(o=(4.0, np.inf, 0.01, 1)), dict(o=(np.nan, 84.0, 0.01, 1)),
                dict(o=(-1.0, 84.0, 0.01, 1)), dict(tlo=[4, 4, 0, 4]), dict(thi=[84, 84, 84, 3]), dict(thi=[84, np.inf, 84, 84]),
                dict(tlo=[4, np.nan, 4, 4], thi=[84, 84, 84, 84]), dict(o=(4.0, 84.0, 1.0, 1)), dict(o=(4.0, 84.0, 9e-7, 1)),
                dict(o=(4.0, 84.0, np.nan, 1)), dict(o=(4.0, 84.0, 0.01, 2)), dict(o=(4.0, 84.0, 0.01, -1))]
    for kw in refusals:
        assert call(**kw) == -1, kw
    assert call(tlo=[4, 4, 0, 4]) == -1 and b"query 2" in L.gusto_last_error(h)
    assert L.gusto_tfsearch_begin(None, 4, 3, ptr(x0), ptr(glo), ptr(ghi), None, None, None) == -1
    assert L.gusto_get_traj(h, None, None) == -3 and none() == (-3, -3, -3, -3)     # every refusal left the handle without problems
    assert call() == 0 and call(o=None, tlo=[4] * 4, thi=[84] * 4) == 0 and call(o=(4.0, 84.0, 1e-6, 0)) == 0
    assert call(Bq=12, K=1, xi=np.repeat(x0, 3, 0), lo=np.repeat(glo, 3, 0), hi=np.repeat(ghi, 3, 0)) == 0      # batch_cap itself
    assert call(o=None) == 0                                                         # the library's default range
    s.B, s._tfsearch = 12, (4, 3)
    assert list(s.tfsearch_info()["hi"]) == [100.0] * 4
    assert call() == 0
    before, rep0 = s.traj(), s.tfsearch_info()
    for kw in refusals:                                                              # refused with a search begun: it stays
        assert call(**kw) == -1, kw
    after, rep1 = s.traj(), s.tfsearch_info()
    assert np.array_equal(before[0], after[0]) and all(same(rep0[k], rep1[k]) for k in REPORT)
    assert L.gusto_tfsearch_update(h, None) == -3 and b"gusto_solve" in L.gusto_last_error(h)   # a solve is still needed
    assert all(same(rep0[k], s.tfsearch_info()[k]) for k in REPORT) and np.array_equal(s.traj()[0], before[0])
    s.solve(1)
    assert L.gusto_tfsearch_update(h, None) == 0
    assert L.gusto_tfsearch_update(h, None) == -3                                    # ... and again after the update
    assert call() == 0 and s.tfsearch_update(np.ones(12)) == 4                       # a caller's eligibility needs no solve
    assert L.gusto_tfsearch_update(h, None) == -3 and b"gusto_solve" in L.gusto_last_error(h)
    assert call() == 0 and s.tfsearch_update(np.zeros(12)) == 0                      # nothing eligible: every query NONE
    assert L.gusto_tfsearch_update(h, None) == -3 and b"searching" in L.gusto_last_error(h)
    s.solve(1)
    assert L.gusto_tfsearch_update(h, np.zeros(12, np.int32).ctypes.data) == -3      # no query is searching, solve or not
    assert s.tfsearch_info()["n_searching"] == 0 and s.last_tfsearch_ms() > 0
    s.set_problems(x0, glo, ghi, np.full(4, 50.0))                                   # other problems: the search is gone
    assert none() == (-3, -3, -3, -3)
    assert call() == 0
    s.set_problems_multistart(x0, glo, ghi, np.full(4, 50.0), np.zeros((3, 2)))
    assert none() == (-3, -3, -3, -3)
    s.close()
    d = g.BatchSolver(1, 10, 12, hist_cap=8)
    xd = np.zeros((4, 3))
    od = O(4.0, 84.0, 0.01, 1)
    assert d.L.gusto_tfsearch_begin(d.h, 4, 3, ptr(xd), ptr(xd), ptr(xd), None, None, C.byref(od)) == -1
    assert b"DubinsCar" in d.L.gusto_last_error(d.h)
    assert d.L.gusto_tfsearch_begin(d.h, 4, 3, ptr(xd), ptr(xd), ptr(xd), None, None, None) == 0      # the default there: the line
    d.close()
    t = g._capi.TrajOptSolver(0, 10, 12)
    assert t.L.gusto_tfsearch_begin(t.h, 4, 3, ptr(x0), ptr(glo), ptr(ghi), None, None, None) == -1 and b"TrajOpt" in t.L.gusto_last_error(t.h)
    t.set_problems(x0, glo, ghi, np.full(4, 50.0))
    assert t.L.gusto_tfsearch_update(t.h, None) == -1 and t.L.gusto_get_tfsearch(t.h, None, None, None) == -1
    t.close()


# ---- 7. the study on the device -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def device_study(seed):
    """the 12 queries of the CPU study through the raw calls: (report, per round (candidates, ok, status, X, U), rounds per query)"""
    from test_tfsearch_cpu import STUDY_ITERS, STUDY_K, STUDY_N, STUDY_Q, STUDY_RANGE, STUDY_ROUNDS
    P = g.problems
    x0, glo, ghi, _ = P.freeflyer_batch(STUDY_Q)
    s = g.BatchSolver(0, STUDY_N, STUDY_Q * STUDY_K, hist_cap=4 * STUDY_ITERS + 16, boxes=P.freeflyer_env())
    s.tfsearch_begin(x0, glo, ghi, *STUDY_RANGE, K=STUDY_K, seed=seed)
    log, took_part = [], np.zeros(STUDY_Q, int)
    r = s.tfsearch_info()
    for _ in range(STUDY_ROUNDS):
        cand, active = r["cand"], (r["status"] & FINISHED) == 0
        s.solve(STUDY_ITERS)
        st = s.status()
        X, U = s.traj()
        ok = (st["converged"] & st["successful"]).reshape(STUDY_Q, STUDY_K) & active[:, None]
        left = s.tfsearch_update()
        took_part += active
        r = s.tfsearch_info()
        log.append((cand, ok, st, X, U, s.last_solve_ms(), s.last_tfsearch_ms()))
        if left == 0:
            break
    s.close()
    return r, log, took_part


@pytest.mark.parametrize("seed", ["line", "incumbent"])
def test_the_study_on_the_device(seed):
    from test_tfsearch_cpu import STUDY_K, STUDY_Q, STUDY_RANGE, check_incumbents, oracle_study
    K = STUDY_K
    r, log, took_part = device_study(seed)
    x0, glo, _, _ = g.problems.freeflyer_batch(STUDY_Q)
    have = r["round_found"] >= 0
    # asserted regardless of parity
    for q in np.flatnonzero(have):
        cand, ok, st, X, U, _, _ = log[r["round_found"][q]]
        w = np.flatnonzero(ok[q] & (cand[q] == r["tf_best"][q]))
        assert len(w) and st["converged"][q * K + w[0]] and st["successful"][q * K + w[0]]       # eligible by the device's own status
        assert np.array_equal(r["X"][q], X[q * K + w[0]]) and np.array_equal(r["U"][q], U[q * K + w[0]])
        assert r["tf_best"][q] == r["hi"][q] and r["lo"][q] < r["hi"][q]
        bound = (STUDY_RANGE[1] - STUDY_RANGE[0]) / K / (K + 1) ** (took_part[q] - 1)
        assert r["hi"][q] - r["lo"][q] <= bound + 4 * ULP * took_part[q] * r["hi"][q], (q, r["hi"][q] - r["lo"][q], bound)
    print("worst collocation residual, goal row, v2 excess:", check_incumbents(r["tf_best"], r["X"], r["U"], x0, glo, have))
    for q in range(STUDY_Q):
        assert bool(r["status"][q] & TS.NONE) == (not have[q]) == bool(np.isnan(r["tf_best"][q]))
        assert bool(r["status"][q] & TS.FLOOR) == (r["lo"][q] == STUDY_RANGE[0])
        assert bool(r["status"][q] & TS.DONE) == (r["hi"][q] - r["lo"][q] <= 0.01 * r["hi"][q])
    # round 0 against the oracle: bit-equal candidates, both from the line -- whole solves at eight final times per query
    S, olog = oracle_study(g._capi.TFSEARCH_SEED[seed])
    ocand, ook, _ = olog[0]
    dcand, dok = log[0][0], log[0][1]
    assert np.array_equal(dcand, ocand)
    left_same = np.concatenate([np.ones((STUDY_Q, 1), bool), ook[:, 1:] == ook[:, :-1]], axis=1)
    right_same = np.concatenate([ook[:, :-1] == ook[:, 1:], np.ones((STUDY_Q, 1), bool)], axis=1)
    interior = left_same & right_same            # the oracle gives the candidate and both its neighbours the same verdict
    differ = dok != ook
    print("round 0: %d of %d candidates interior; differing verdicts: %d interior %s, %d at a threshold %s"
          % (interior.sum(), interior.size, (differ & interior).sum(), list(zip(*np.nonzero(differ & interior))),
             (differ & ~interior).sum(), list(zip(*np.nonzero(differ & ~interior)))))
    assert interior.sum() * 4 >= 3 * interior.size
    assert (differ & interior).sum() <= PARITY_MAX_DIVERGED
    # the answers: printed; a flipped verdict near a threshold moves a bracket by a cell, so only the majority is asked for
    overlap = [q for q in range(STUDY_Q) if have[q] and S.round_found[q] >= 0 and r["lo"][q] <= S.hi[q] and S.lo[q] <= r["hi"][q]]
    print("tf_best device", [float(v) for v in r["tf_best"]], "\ntf_best oracle", [float(v) for v in S.tf_best],
          "\noverlapping brackets on", overlap, "equal answers on", [q for q in range(STUDY_Q) if r["tf_best"][q] == S.tf_best[q]])
    print("status device", list(r["status"]), "oracle", list(S.status), "\ntrips per round: device",
          [int(l[2]["iterations"].sum()) for l in log], "oracle", [int(i.sum()) for _, _, i in olog])
    print("solve ms per round", [round(l[5], 3) for l in log], "tfsearch ms per update", [round(l[6], 3) for l in log])
    assert len(overlap) > STUDY_Q // 2


def test_host_driver():
    """host.solve_SCP_min_time_batch answers what the raw calls answer; the solutions are those of the solves that found the incumbents"""
    from test_gpu_multistart import host_problems
    from test_tfsearch_cpu import STUDY_Q, STUDY_RANGE
    H = g.host
    r, log, _ = device_study("incumbent")
    TOPs, TOSs = host_problems(STUDY_Q)
    out = H.solve_SCP_min_time_batch(TOSs, TOPs, *STUDY_RANGE, K=8, rounds=3)
    for q in range(STUDY_Q):
        o = out[q]
        assert same(o["tf"], r["tf_best"][q]) and (o["lo"], o["hi"], o["status"]) == (r["lo"][q], r["hi"][q], r["status"][q])
        assert same(o["J"], r["J_best"][q]) and o["SCPS"] is TOSs[q].SCPS and TOSs[q].traj is o["SCPS"].traj
        if r["round_found"][q] >= 0:
            assert np.array_equal(o["SCPS"].traj.X.T, r["X"][q]) and np.array_equal(o["SCPS"].traj.U.T, r["U"][q])
            assert o["SCPS"].traj.Tf == o["tf"] and o["SCPS"].converged and o["SCPS"].successful and o["SCPS"].J_true[-1] == o["J"]
        else:                                   # NONE: the straight line's solve at tf_hi
            X84 = log[0][3][q * 8 + 7]
            assert o["SCPS"].traj.Tf == STUDY_RANGE[1] and np.array_equal(o["SCPS"].traj.X.T, X84) and not (o["SCPS"].converged and o["SCPS"].successful)
    # a caller's eligibility: the default one, passed as a function, is the same search
    _, TOS2 = host_problems(3)
    a = H.solve_SCP_min_time_batch(TOS2, TOPs[:3], *STUDY_RANGE, K=8, rounds=2, eligible=lambda bs: bs.status()["converged"] & bs.status()["successful"])
    _, TOS3 = host_problems(3)
    b = H.solve_SCP_min_time_batch(TOS3, TOPs[:3], *STUDY_RANGE, K=8, rounds=2)
    assert [(x["tf"], x["lo"], x["status"]) for x in a] == [(x["tf"], x["lo"], x["status"]) for x in b]
    with pytest.raises(ValueError):
        H.solve_SCP_min_time_batch(TOSs, TOPs[:3], *STUDY_RANGE)


# ---- 8. the C consumer --------------------------------------------------------------------------------------------------------
def test_c_consumer(tmp_path):
    """tests/c/c_abi_tfsearch.c, a plain C consumer with checks of its own; the report it prints is the Python path's"""
    exe = os.path.join(tmp_path, "c_abi_tfsearch")
    lib = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_tfsearch.c"), "-o", exe, "-L" + lib, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 4
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.4, 1.9, 0, 0, 0, 0], [0.3, 0.4, 0, 0, 0, 0]], float)
    goal = np.tile([3.0, 0.5, 0, 0.05, -0.05, 0], (3, 1))
    s = g.BatchSolver(0, 50, 12, hist_cap=64, boxes=np.array([[1.4, 0.9, -0.2, 1.8, 1.5, 0.2]]))
    s.tfsearch_begin(x0, goal, goal, 4.0, 84.0, K=4)
    for _ in range(2):
        s.solve(30)
        if s.tfsearch_update() == 0:
            break
    r = s.tfsearch_info()
    s.close()
    for q in range(3):
        v = lines[1 + q].split()
        assert (int(v[0]), int(v[1])) == (r["status"][q], r["round_found"][q])
        assert same(np.array([float(x) for x in v[2:]]), np.array([r["lo"][q], r["hi"][q], r["tf_best"][q], r["J_best"][q]]))
