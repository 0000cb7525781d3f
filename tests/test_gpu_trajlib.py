"""The trajectory library on the device -- gusto_trajlib_*, gusto_set_problems_trajlib, gusto_get_trajlib_seeds -- against
tests/np_trajlib.py, the numpy restatement (tests/test_trajlib_cpu.py proves it without a GPU), against gusto_set_problems on a
second handle, and on the small study of the CPU test: 16 table queries seeded from a library of 32 problems solved on the device,
next to the CPU oracle.

Tolerances.  Everything is compared bit for bit except
  - dist2: 4 ulp per accumulated term, |dev - np| <= 4 * 2^-52 * F * d2 with F the number of positive weights (every term is
    non-negative, so d2 bounds every partial sum); the inputs keep consecutive sorted d2 more than 1e-12 apart
    (test_trajlib_cpu.py::test_search_inputs_keep_their_distances_apart), so the entry lists are expected equal;
  - the retargeted X0: |dev - np| <= 4 * 2^-52 * (|X_e| + |dxi| + |dc|) per entry, three roundings plus the blend's;
  - the comparison with the oracle: what tests/test_gpu_parity.py grants whole solves of freeflyerSE2 (test_scp_parity_freeflyer,
    _scp_parity): one problem whose decisions differ, X and U to 1e-3, J_true, J_full and the convergence measure to 1e-4 relative
    (1e-5 absolute on the latter), rho to 1e-2 relative, all scaled by max(1, omega_max / 1e3)."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import np_trajlib as TL
from test_trajlib_cpu import FREEFLYER_16, LIB_FIRST, SEARCH_BQS, SEARCH_KS, SEARCH_LS, random_lib, search_case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULP = 2.0 ** -52
PARITY_MAX_DIVERGED, PARITY_RTOL, TRAJ_ATOL = 1, 1e-4, 1e-3      # tests/test_gpu_parity.py: test_scp_parity_freeflyer, _scp_parity


def device_lib(ref, cap=None, **kw):
    """the restatement's library on the device, through gusto_trajlib_add_host"""
    lib = g.TrajLib(ref.model_id, ref.N, cap or max(len(ref), 1), w_init=ref.w_init, w_goal=ref.w_goal, w_tf=ref.w_tf, **kw)
    if len(ref):
        lib.add_host(ref.x_init, ref.c, ref.c, ref.tf, ref.X, ref.U, tag=ref.tag)
    return lib


def check_seeds(got, want, F):
    assert np.array_equal(got["entry"], want["entry"]), (got["entry"], want["entry"])
    assert np.array_equal(got["n_found"], want["n_found"])
    inf = np.isposinf(want["dist2"])
    assert np.array_equal(np.isposinf(got["dist2"]), inf)
    err = np.abs(got["dist2"][~inf] - want["dist2"][~inf])
    assert (err <= 4 * ULP * F * want["dist2"][~inf]).all(), (err.max(), F)


# ---- 1. the search ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", SEARCH_LS)
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_search_against_the_restatement(model, L):
    """entry lists equal, dist2 within 4 ulp per term, with and without tags; the two forms of the kernel (lds_tile) agree bit for
    bit"""
    ref, x_init, lo, hi, tf = search_case(model, L)
    F = TL.n_terms(ref)
    libs = [device_lib(ref), device_lib(ref, lds_tile=0)]
    s = g.BatchSolver(model, 3, 40, hist_cap=8)
    tags = np.array([0, 1, 2, 0, 1])
    for K in SEARCH_KS:
        for Bq in SEARCH_BQS:
            for tg in (None, tags[:Bq]):
                want = TL.search(ref, x_init[:Bq], lo[:Bq], hi[:Bq], tf[:Bq], K, tg)
                got = []
                for lib in libs:
                    s.set_problems_trajlib(lib, x_init[:Bq], lo[:Bq], hi[:Bq], tf[:Bq], K, tag=tg)
                    got.append(s.trajlib_seeds())
                    assert s.B == Bq * K and s.last_trajlib_ms() > 0
                check_seeds(got[0], want, F)
                for k in ("entry", "dist2", "n_found"):
                    assert np.array_equal(got[0][k], got[1][k]), k
    s.close()
    for lib in libs:
        lib.close()


def test_ties_go_to_the_lowest_entry():
    """dyadic coordinates: every product and sum is exact, whatever the compiler contracts.  Duplicates at entries (3, 67) and
    (64, 128), the same lane in different strides, and (10, 11), neighbouring lanes"""
    L, n = 200, 6
    q = np.array([0.5, -1.25, 0.25, 0.0, 0.125, -0.5])
    ref = TL.Lib(0, 3)
    x = np.tile(q, (L, 1))
    x[:, 0] += 3.0 + np.arange(L) / 8.0                  # everything else: d2 >= 9
    x[:, 2] -= (np.arange(L) % 7) / 4.0
    for (a, b), (i, off) in (((3, 67), (0, 0.5)), ((64, 128), (1, 1.0)), ((10, 11), (0, -1.5))):
        x[a] = x[b] = q
        x[a, i] = x[b, i] = q[i] + off
    rng = np.random.default_rng(0)
    ref.add(x, np.tile(q, (L, 1)), np.tile(q, (L, 1)), 40.0, rng.normal(size=(L, 3, n)), rng.normal(size=(L, 3, 3)))
    s = g.BatchSolver(0, 3, 16, hist_cap=8)
    for kw in ({}, dict(lds_tile=0)):
        lib = device_lib(ref, **kw)
        for K in (1, 2, 3, 8):
            s.set_problems_trajlib(lib, q, q, q, 40.0, K)
            got, want = s.trajlib_seeds(), TL.search(ref, q, q, q, 40.0, K)
            assert list(got["entry"][0]) == [3, 67, 64, 128, 10, 11, 0, 1][:K]
            for k in ("entry", "dist2", "n_found"):
                assert np.array_equal(got[k], want[k]), (K, k)
            assert list(got["dist2"][0][:6]) == [0.25, 0.25, 1.0, 1.0, 2.25, 2.25][:K][:6]
        lib.close()
    s.close()


def test_tags_nan_and_k_above_the_eligible_count():
    rng = np.random.default_rng(11)
    ref = random_lib(0, 4, 70, rng, w_tf=0.5)
    ref.tag[:] = rng.integers(0, 3, 70)
    ref.tag[[5, 69]] = 7                                   # two entries with tag 7
    lib = device_lib(ref)
    x_init, lo = rng.uniform(-3, 3, (4, 6)), rng.uniform(-3, 3, (4, 6))
    tf = np.array([20.0, 30.0, np.nan, 25.0])              # query 2: every d2 is NaN
    tags = np.array([7, 9, 1, 2])                          # query 1: no entry has its tag
    s = g.BatchSolver(0, 4, 12, hist_cap=8)
    s.set_problems_trajlib(lib, x_init, lo, lo, tf, 3, tag=tags)
    got, want = s.trajlib_seeds(), TL.search(ref, x_init, lo, lo, tf, 3, tags)
    check_seeds(got, want, TL.n_terms(ref))
    assert list(got["n_found"]) == [2, 0, 0, 3] and set(got["entry"][0][:2]) == {5, 69} and got["entry"][0][2] == -1
    assert (got["entry"][1:3] == -1).all() and np.isposinf(got["dist2"][1:3]).all() and np.isposinf(got["dist2"][0, 2])
    X, U = s.traj()
    s.set_problems_trajlib(lib, x_init, lo, lo, tf, 3)     # without tags query 2 still finds nothing: NaN is never a neighbour
    assert list(s.trajlib_seeds()["n_found"]) == [3, 3, 0, 3]
    t = g.BatchSolver(0, 4, 12, hist_cap=8)                # the starts without a neighbour are gusto_set_problems' straight lines
    t.set_problems(np.repeat(x_init, 3, 0), np.repeat(lo, 3, 0), np.repeat(lo, 3, 0), 20.0)      # (tf is not read by the straight line)
    Xs, Us = t.traj()
    for b in (2, 3, 4, 5, 6, 7, 8):
        assert np.array_equal(X[b], Xs[b], equal_nan=True) and not U[b].any()
    assert not np.array_equal(X[0], Xs[0]) and np.array_equal(U[0], ref.U[got["entry"][0, 0]])
    for h in (s, t, lib):
        h.close()


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_empty_library_gives_straight_lines(model):
    """bit for bit the trajectories of a second handle's gusto_set_problems with X0 = NULL"""
    rng = np.random.default_rng(model)
    n = TL.X_DIM[model]
    for N in (3, 50):
        lib = g.TrajLib(model, N, 4)
        x_init, lo = rng.uniform(-3, 3, (3, n)), rng.uniform(-3, 3, (3, n))
        hi = lo + rng.uniform(0, 0.3, (3, n))
        hi[1, 0], lo[2, n - 1] = np.inf, -np.inf
        tf = np.array([20.0, 30.0, 40.0])
        s, t = g.BatchSolver(model, N, 9, hist_cap=8), g.BatchSolver(model, N, 9, hist_cap=8)
        s.set_problems_trajlib(lib, x_init, lo, hi, tf, 3)
        seeds = s.trajlib_seeds()
        assert (seeds["entry"] == -1).all() and np.isposinf(seeds["dist2"]).all() and not seeds["n_found"].any()
        t.set_problems(np.repeat(x_init, 3, 0), np.repeat(lo, 3, 0), np.repeat(hi, 3, 0), np.repeat(tf, 3))
        (X, U), (Xs, Us) = s.traj(), t.traj()
        assert np.array_equal(X, Xs) and np.array_equal(U, Us) and not U.any()
        for h in (s, t, lib):
            h.close()


def test_a_querys_seeds_do_not_depend_on_the_batch():
    ref, x_init, lo, hi, tf = search_case(0, 200)
    lib = device_lib(ref)
    s = g.BatchSolver(0, 3, 40, hist_cap=8)
    s.set_problems_trajlib(lib, x_init, lo, hi, tf, 8)
    batch, (Xb, Ub) = s.trajlib_seeds(), s.traj()
    for q in range(5):
        s.set_problems_trajlib(lib, x_init[q], lo[q], hi[q], tf[q], 8)
        one, (X, U) = s.trajlib_seeds(), s.traj()
        for k in ("entry", "dist2", "n_found"):
            assert np.array_equal(one[k][0], batch[k][q]), (q, k)
        assert np.array_equal(X, Xb[8 * q:8 * q + 8]) and np.array_equal(U, Ub[8 * q:8 * q + 8])
    s.close()
    lib.close()


# ---- 2. the retargeting -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [3, 4, 50])
@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_retargeting_against_the_restatement(model, N):
    """X0, U0 read back before any solve; knot 0 and U0 exact; the exact hit; the replicated x_init, goal_lo, goal_hi and tf through
    one convex subproblem, which reads all four: bit for bit what gusto_set_problems gives for the same trajectories"""
    rng = np.random.default_rng(100 * model + N)
    n = TL.X_DIM[model]
    ref = random_lib(model, N, 70, rng)
    lib = device_lib(ref)
    sp, mp = g.default_params(model)
    s = g.BatchSolver(model, N, 24, hist_cap=8)
    for K, Bq in ((1, 1), (2, 3), (8, 3)):
        x_init, lo = rng.uniform(-3, 3, (Bq, n)), rng.uniform(-3, 3, (Bq, n))
        hi = lo + rng.uniform(0, 0.3, (Bq, n))
        if Bq > 1:
            hi[1, 0] = np.inf
            x_init[2], lo[2], hi[2] = ref.x_init[40], ref.c[40], ref.c[40]          # the exact hit
        tf = rng.uniform(20, 40, Bq)
        s.set_problems_trajlib(lib, x_init, lo, hi, tf, K)
        X, U = s.traj()
        seeds = s.trajlib_seeds()
        xi, l, h, t, Xr, Ur, want = TL.seeded_problems(ref, x_init, lo, hi, tf, K)
        check_seeds(seeds, want, TL.n_terms(ref))
        assert np.array_equal(U, Ur) and np.array_equal(X[:, 0], xi)
        for b in range(Bq * K):
            e = seeds["entry"][b // K, b % K]
            bound = 4 * ULP * (np.abs(ref.X[e]) + np.abs(xi[b] - ref.x_init[e])[None, :] + np.abs(TL.goal_centre(l[b], h[b]) - ref.c[e])[None, :])
            err = np.abs(X[b] - Xr[b])
            assert (err <= bound).all(), (K, b, err.max())
        if Bq > 1:
            assert seeds["entry"][2, 0] == 40 and seeds["dist2"][2, 0] == 0.0
            assert np.array_equal(X[2 * K, 1:], ref.X[40, 1:]) and np.array_equal(X[2 * K, 0], ref.x_init[40]) and np.array_equal(U[2 * K], ref.U[40])
        if K == 2:
            sub = s.subproblem(X, U, sp.Delta0, sp.omega0, sp.Delta0 / 8 + mp.clearance)
            s.set_problems(xi, l, h, t, X, U)
            again = s.subproblem(X, U, sp.Delta0, sp.omega0, sp.Delta0 / 8 + mp.clearance)
            for f in ("X", "U", "obj", "status", "iters", "dual"):
                assert np.array_equal(sub[f], again[f], equal_nan=True), f
    s.close()
    lib.close()


# ---- 3. gusto_trajlib_add -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 64, 65, 130])
def test_add_from_a_handle(B):
    """order and contents under all / none / alternating masks; the features it writes, through a search; the capacity refusal; get
    into add_host of a second library: identical seeds"""
    rng = np.random.default_rng(B)
    model, N = 2, 4
    n, m = TL.X_DIM[model], TL.U_DIM[model]
    x, lo = rng.uniform(-3, 3, (B, n)), rng.uniform(-3, 3, (B, n))
    hi = lo + rng.uniform(0, 0.3, (B, n))
    hi[0, 1] = np.inf
    tf, tag = rng.uniform(20, 40, B), rng.integers(0, 3, B)
    X0, U0 = rng.normal(size=(B, N, n)), rng.normal(size=(B, N, m))
    s = g.BatchSolver(model, N, B, hist_cap=8)
    s.set_problems(x, lo, hi, tf, X0, U0)
    alt = np.arange(B) % 2 == 0
    cap = 2 * B + int(alt.sum())
    lib, ref = g.TrajLib(model, N, cap, w_tf=0.25), TL.Lib(model, N, w_tf=0.25)
    assert lib.add_from(s) == 0 and len(lib) == 0                               # the default mask: nothing is converged
    for mask, tg in ((np.ones(B), tag), (np.zeros(B), tag), (alt, None), (np.ones(B), 5)):
        added = lib.add_from(s, mask, tg)
        assert added == ref.add_masked(mask, x, lo, hi, tf, X0, U0, None if tg is None else np.broadcast_to(tg, (B,))) and len(lib) == len(ref)
    assert len(lib) == cap
    got = lib.get()
    for k, want in (("x_init", ref.x_init), ("goal_c", ref.c), ("tf", ref.tf), ("tag", ref.tag), ("X", ref.X), ("U", ref.U)):
        assert np.array_equal(got[k], want), k
    with pytest.raises(g.GustoError, match="capacity"):                         # full: one more does not fit
        lib.add_from(s, np.arange(B) == B - 1)
    n_added = C.c_int(-1)
    one = np.ones(B, np.int32)
    assert lib.L.gusto_trajlib_add(lib.h, s.h, one.ctypes.data, None, C.byref(n_added)) == -1 and n_added.value == 0
    after = lib.get()
    assert len(lib) == cap and all(np.array_equal(after[k], got[k]) for k in got)
    xq, cq = rng.uniform(-3, 3, (4, n)), rng.uniform(-3, 3, (4, n))
    t = g.BatchSolver(model, N, 32, hist_cap=8)
    t.set_problems_trajlib(lib, xq, cq, cq, 30.0, 8, tag=[0, 1, 2, 5])
    seeds, (X, U) = t.trajlib_seeds(), t.traj()
    check_seeds(seeds, TL.search(ref, xq, cq, cq, 30.0, 8, [0, 1, 2, 5]), TL.n_terms(ref))
    lib2 = g.TrajLib(model, N, cap + 3, w_tf=0.25)
    lib2.add_host(got["x_init"], got["goal_c"], got["goal_c"], got["tf"], got["X"], got["U"], tag=got["tag"])
    t.set_problems_trajlib(lib2, xq, cq, cq, 30.0, 8, tag=[0, 1, 2, 5])
    seeds2, (X2, U2) = t.trajlib_seeds(), t.traj()
    assert all(np.array_equal(seeds[k], seeds2[k]) for k in seeds) and np.array_equal(X, X2) and np.array_equal(U, U2)
    lib.clear()
    assert len(lib) == 0 and lib.add_from(s, alt) == alt.sum()
    for h in (s, t, lib, lib2):
        h.close()


def test_save_and_load(tmp_path):
    rng = np.random.default_rng(8)
    ref = random_lib(1, 5, 9, rng, w_init=[1, 1, 4], w_goal=0.0, w_tf=0.1)
    lib = device_lib(ref, cap=12)
    lib.save(str(tmp_path / "lib.npz"))
    back = g.host.TrajLib.load(str(tmp_path / "lib.npz"))
    a, b = lib.get(), back.get()
    assert len(back) == 9 and all(np.array_equal(a[k], b[k]) for k in a)
    assert list(back.opts.w_init[:3]) == [1, 1, 4] and back.opts.w_tf == 0.1 and not any(back.opts.w_goal[:3])
    s = g.BatchSolver(1, 5, 6, hist_cap=8)
    xq = rng.uniform(-3, 3, (2, 3))
    out = []
    for l in (lib, back):
        s.set_problems_trajlib(l, xq, xq, xq, 12.0, 3)
        out.append((s.trajlib_seeds(), s.traj()))
    assert all(np.array_equal(out[0][0][k], out[1][0][k]) for k in out[0][0]) and np.array_equal(out[0][1][0], out[1][1][0])
    for h in (s, lib, back):
        h.close()


# ---- 4. end to end --------------------------------------------------------------------------------------------------------------------
def snapshot(s):
    X, U = s.traj()
    return dict(X=X, U=U, st=s.status(), h=s.history())


@functools.lru_cache(maxsize=None)
def small_study():
    """32 freeflyer problems solved on the device become the library; the first 16 table queries cold, seeded with K = 1 and with
    K = 3, in the same run (shared, not written to)"""
    P = g.problems
    env = P.freeflyer_env()
    lx, ll, lh, lt = P.freeflyer_batch(32, first=LIB_FIRST)
    s = g.BatchSolver(0, 50, 48, hist_cap=40, boxes=env)
    s.set_problems(lx, ll, lh, lt)
    s.solve(30)
    lib = g.TrajLib(0, 50, 64)
    added = lib.add_from(s)
    st = s.status()
    x0, lo, hi, tf = P.freeflyer_batch(16)
    s.set_problems(x0, lo, hi, tf)
    s.solve(30)
    cold = snapshot(s)
    s.set_problems_trajlib(lib, x0, lo, hi, tf, 1)
    seeds, start = s.trajlib_seeds(), s.traj()
    s.solve(30)
    seeded = snapshot(s)
    s.set_problems_trajlib(lib, x0, lo, hi, tf, 3)
    s.solve(30)
    best3 = s.select_best(3)
    return dict(lib=lib, added=added, lib_status=st, cold=cold, seeds=seeds, start=start, seeded=seeded, best3=best3, solver=s,
                queries=(x0, lo, hi, tf))


def test_seeded_solves_against_the_oracle():
    """per problem against the oracle solved from the restatement's seeds, under the allowances of the whole-solve freeflyer parity
    test; the seeded total of SCP iterations is below the cold total of the same queries in the same run (the oracle's figures for
    this case: 69 against 160, test_trajlib_cpu.py::test_small_study_is_pinned)"""
    import gusto_oracle as go
    d = small_study()
    lib, (x0, lo, hi, tf) = d["lib"], d["queries"]
    ok = d["lib_status"]["converged"].astype(bool) & d["lib_status"]["successful"].astype(bool)
    assert d["added"] == ok.sum() == len(lib)
    print("library: %d of 32 converged and successful on the device (oracle: %d)" % (len(lib), FREEFLYER_16["lib_good"]))
    got = lib.get()
    ref = TL.Lib(0, 50)
    ref.add(got["x_init"], got["goal_c"], got["goal_c"], got["tf"], got["X"], got["U"], got["tag"])
    lx, ll, lh, lt = g.problems.freeflyer_batch(32, first=LIB_FIRST)
    assert np.array_equal(got["x_init"], lx[ok]) and np.array_equal(got["goal_c"], ll[ok]) and np.array_equal(got["tf"], lt[ok])
    xi, l, h, t, X0, U0, want = TL.seeded_problems(ref, x0, lo, hi, tf, 1)
    check_seeds(d["seeds"], want, TL.n_terms(ref))
    assert (d["seeds"]["n_found"] == 1).all()
    assert np.abs(d["start"][0] - X0).max() <= 4 * ULP * 16 and np.array_equal(d["start"][1], U0)
    X, U, st, hh = (d["seeded"][k] for k in ("X", "U", "st", "h"))
    o = go.Oracle(go.FREEFLYER_SE2, 50, boxes=g.problems.freeflyer_env())
    diverged = []
    for b in range(16):
        o.set_problem(xi[b], l[b], h[b], t[b], X0[b], U0[b])
        r = o.solve(30)
        nh = int(hh["n_hist"][b])
        c = min(nh, len(r["omega"]))
        agree = (np.array_equal(hh["scp_status"][b, :c], r["scp_status"][:c]) and np.array_equal(hh["omega"][b, :c], r["omega"][:c])
                 and np.array_equal(hh["Delta"][b, :c], r["Delta"][:c]))
        if not (agree and nh == len(r["omega"])):
            diverged.append(b)
            first = next((i for i in range(c) if hh["scp_status"][b, i] != r["scp_status"][i] or hh["omega"][b, i] != r["omega"][i]
                          or hh["Delta"][b, i] != r["Delta"][i]), c)
            assert first >= 3, (b, first)
            np.testing.assert_allclose(hh["convergence_measure"][b, :first - 1], r["conv"][:first - 1], rtol=1e-3, atol=1e-6)
            continue
        assert bool(st["converged"][b]) == r["converged"] and bool(st["successful"][b]) == r["successful"], b
        assert int(st["iterations"][b]) == r["iterations"] and int(st["stop_reason"][b]) == r["stop_reason"], b
        w = max(1.0, r["omega"].max() / 1e3)
        assert np.abs(X[b] - r["X"]).max() < TRAJ_ATOL * w and np.abs(U[b] - r["U"]).max() < TRAJ_ATOL * w, b
        np.testing.assert_array_equal(hh["accept_solution"][b, :nh], r["accept"])
        nJ = hh["nJ"][b]
        assert nJ == len(r["J_true"])
        np.testing.assert_allclose(hh["J_true"][b, :nJ], r["J_true"], rtol=PARITY_RTOL * w, atol=1e-9)
        np.testing.assert_allclose(hh["J_full"][b, :nJ], r["J_full"], rtol=PARITY_RTOL * w, atol=1e-9)
        np.testing.assert_allclose(hh["convergence_measure"][b, :nh], r["conv"], rtol=PARITY_RTOL * w, atol=1e-5 * w)
        nr = hh["n_rho"][b]
        np.testing.assert_allclose(hh["rho"][b, :nr], r["rho"], rtol=100 * PARITY_RTOL * w, atol=1e-7 * w)
    assert len(diverged) <= PARITY_MAX_DIVERGED, diverged
    cold_it, seeded_it = int(d["cold"]["st"]["iterations"].sum()), int(st["iterations"].sum())
    good = lambda sn: int((sn["st"]["converged"].astype(bool) & sn["st"]["successful"].astype(bool)).sum())
    print("SCP iterations: cold %d, seeded %d (oracle: %d, %d); successful: cold %d, seeded %d (oracle: %d, %d)"
          % (cold_it, seeded_it, FREEFLYER_16["cold"][1], FREEFLYER_16["seeded"][1], good(d["cold"]), good(d["seeded"]),
             FREEFLYER_16["cold"][0], FREEFLYER_16["seeded"][0]))
    assert seeded_it < cold_it


def test_three_neighbours_and_select_best_give_a_winner_per_query():
    d = small_study()
    best = d["best3"]
    assert (best["winner"] >= 0).all() and (best["n_eligible"] >= 1).all() and np.isfinite(best["best_score"]).all()
    assert np.array_equal(best["winner_problem"], np.arange(16) * 3 + best["winner"])


def test_histories_are_reset_and_the_post_solve_getters_refuse():
    """as after gusto_set_problems"""
    d = small_study()
    s, lib, (x0, lo, hi, tf) = d["solver"], d["lib"], d["queries"]
    L, h = s.L, s.h
    s.verify(nstep=1)
    s.tvlqr({})
    s.select_best(3)
    vr = C.byref(g._capi.VerifyReport())
    assert L.gusto_get_verify(h, vr) == 0 and L.gusto_get_best(h, None) == 0 and L.gusto_get_tvlqr(h, None, None, None, None, None) == 0
    assert s.history()["n_hist"].sum() > 0
    s.set_problems(np.repeat(x0[:4], 2, 0), np.repeat(lo[:4], 2, 0), np.repeat(hi[:4], 2, 0), np.repeat(tf[:4], 2))
    fresh = s.history()                                       # what gusto_set_problems leaves
    s.solve(3)
    s.verify(nstep=1)
    s.tvlqr({})
    s.select_best(2)
    s.set_problems_trajlib(lib, x0[:4], lo[:4], hi[:4], tf[:4], 2)
    st, hh = s.status(), s.history()
    assert s.B == 8 and not st["iterations"].any() and not st["converged"].any() and not st["successful"].any()
    for k in ("n_hist", "nJ", "n_rho"):
        assert np.array_equal(hh[k], fresh[k]), k
    assert L.gusto_get_verify(h, vr) == -3 and L.gusto_get_best(h, None) == -3 and L.gusto_get_tvlqr(h, None, None, None, None, None) == -3
    assert L.gusto_get_trajlib_seeds(h, None, None, None) == 0
    s.set_problems(x0[:4], lo[:4], hi[:4], tf[:4])            # ... and the seeds belong to the problems they were found for
    ms = C.c_double()
    assert L.gusto_get_trajlib_seeds(h, None, None, None) == -3 and L.gusto_last_trajlib_ms(h, C.byref(ms)) == -3
    s.set_problems_trajlib(lib, x0, lo, hi, tf, 3)            # (the shared handle as the other tests expect it)
    s.solve(30)


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals():
    P = g.problems
    x0, glo, ghi, tf = P.freeflyer_batch(4)
    L = g.lib()
    ptr = lambda a: np.ascontiguousarray(a, float).ctypes.data
    # creation
    o = g.default_trajlib_opts(0)
    hl = C.c_void_p()
    for model, N, cap in ((9, 50, 4), (0, 2, 4), (0, 257, 4), (0, 50, 0), (0, 50, (1 << 20) + 1)):
        assert L.gusto_trajlib_create(C.byref(hl), model, N, cap, 0, None) == -1 and L.gusto_trajlib_last_error(None)
    assert L.gusto_trajlib_create(None, 0, 50, 4, 0, None) == -1
    for field, i, bad in (("w_init", 0, -1.0), ("w_goal", 5, np.nan), ("w_init", 3, np.inf), ("w_tf", None, -0.5), ("w_tf", None, np.inf),
                          ("lds_tile", None, 2)):
        o = g.default_trajlib_opts(0)
        if i is None:
            setattr(o, field, bad)
        else:
            getattr(o, field)[i] = bad
        assert L.gusto_trajlib_create(C.byref(hl), 0, 50, 4, 0, C.byref(o)) == -1, field
    o = g.default_trajlib_opts(0)
    o.w_init[6] = -1.0                                         # behind x_dim: ignored
    assert L.gusto_trajlib_create(C.byref(hl), 0, 50, 4, 0, C.byref(o)) == 0 and L.gusto_trajlib_destroy(hl) == 0
    for f in (L.gusto_trajlib_destroy, L.gusto_trajlib_clear):
        assert f(None) == -1
    assert L.gusto_trajlib_size(None, None, None) == -1 and L.gusto_trajlib_get(None, None, None, None, None, None, None) == -1
    assert L.gusto_trajlib_add(None, None, None, None, None) == -1 and L.gusto_default_trajlib_opts(0, None) == -1
    # gusto_set_problems_trajlib: the refusals of the multi-start call, and the library's
    lib, lib_n, lib_m = g.TrajLib(0, 50, 8), g.TrajLib(0, 49, 8), g.TrajLib(1, 50, 8)
    s = g.BatchSolver(0, 50, 12, hist_cap=8)
    h = s.h
    call = lambda Bq, K, lb=lib, xi=x0, hs=h: L.gusto_set_problems_trajlib(hs, None if lb is None else lb.h, Bq, K, None if xi is None else ptr(xi),
                                                                            ptr(glo), ptr(ghi), ptr(tf), None)
    assert L.gusto_get_trajlib_seeds(h, None, None, None) == -3                       # no problems
    assert call(4, 0) == -1 and b"GUSTO_TRAJLIB_MAX_K" in L.gusto_last_error(h)
    assert call(1, 9) == -1 and call(0, 3) == -1
    assert call(3, 5) == -1 and b"batch_cap" in L.gusto_last_error(h)                # 15 = batch_cap + 3
    assert call(4, 3, xi=None) == -1 and call(4, 3, lb=None) == -1 and call(4, 3, hs=None) == -1
    assert call(4, 3, lb=lib_n) == -1 and b"differ" in L.gusto_last_error(h) and call(4, 3, lb=lib_m) == -1
    assert L.gusto_get_traj(h, None, None) == -3            # every refusal left the handle as it was: without problems
    assert call(4, 3) == 0                                    # batch_cap itself
    s.B, s._trajlib_K = 12, 3
    before = s.traj()
    assert call(3, 5) == -1 and call(4, 3, lb=lib_n) == -1 and call(4, 9) == -1        # refused with problems set: they stay
    assert np.array_equal(before[0], s.traj()[0]) and L.gusto_get_trajlib_seeds(h, None, None, None) == 0
    # gusto_trajlib_add / _add_host
    n_added = C.c_int(-1)
    assert L.gusto_trajlib_add(lib_n.h, h, None, None, C.byref(n_added)) == -1 and n_added.value == 0 and b"differ" in L.gusto_trajlib_last_error(lib_n.h)
    assert L.gusto_trajlib_add(lib_m.h, h, None, None, None) == -1 and L.gusto_trajlib_add(lib.h, None, None, None, None) == -1
    fresh = g.BatchSolver(0, 50, 4, hist_cap=8)
    assert L.gusto_trajlib_add(lib.h, fresh.h, None, None, None) == -3               # a handle without problems
    X, U = np.zeros((2, 50, 6)), np.zeros((2, 50, 3))
    for name in ("x_init", "tf", "X", "U"):
        a = dict(x_init=x0[:2].copy(), tf=tf[:2].copy(), X=X.copy(), U=U.copy())
        for bad in (np.nan, np.inf):
            a[name].reshape(-1)[-1] = bad
            with pytest.raises(g.GustoError, match="finite"):
                lib.add_host(a["x_init"], glo[:2], ghi[:2], a["tf"], a["X"], a["U"])
    inf_goal = ghi[:2].copy()
    inf_goal[0, 0] = np.inf                                   # a goal bound may be infinite: its centre is 0
    lib.add_host(x0[:2], glo[:2], inf_goal, tf[:2], X, U)
    assert len(lib) == 2 and lib.get()["goal_c"][0, 0] == 0.0
    with pytest.raises(g.GustoError, match="capacity"):
        lib.add_host(np.zeros((7, 6)), np.zeros((7, 6)), np.zeros((7, 6)), np.ones(7), np.zeros((7, 50, 6)), np.zeros((7, 50, 3)))
    assert len(lib) == 2
    t = g._capi.TrajOptSolver(0, 50, 12)
    assert call(4, 3, hs=t.h) == -1 and b"TrajOpt" in L.gusto_last_error(t.h)
    t.set_problems(x0, glo, ghi, tf)
    assert L.gusto_trajlib_add(lib.h, t.h, None, None, None) == -1 and L.gusto_get_trajlib_seeds(t.h, None, None, None) == -1
    with pytest.raises(g._capi.GustoError):
        t.set_problems_trajlib()
    for x in (s, fresh, t, lib, lib_n, lib_m):
        x.close()


# ---- 6. the drivers ---------------------------------------------------------------------------------------------------------------------
def test_host_driver():
    """solve_SCP_trajlib_batch: the seeded winners are the handle's; the fallback fan answers what the library could not; learn
    appends the winners"""
    from test_gpu_multistart import host_problems
    H = g.host
    d = small_study()
    lib0 = d["lib"].get()
    lib = H.TrajLib(0, 50, 64)
    lib.add_host(lib0["x_init"], lib0["goal_c"], lib0["goal_c"], lib0["tf"], lib0["X"], lib0["U"], tag=lib0["tag"])
    TOPs, TOSs = host_problems(16)
    out = H.solve_SCP_trajlib_batch(TOSs, TOPs, lib, K=3)
    best = d["best3"]
    for q in range(16):
        assert out[q]["winner"] == best["winner"][q] and out[q]["cost"] == best["best_score"][q] and out[q]["source"] == "library"
        assert np.array_equal(out[q]["SCPS"].traj.X.T, best["X"][q]) and out[q]["SCPS"] is TOSs[q].SCPS and out[q]["SCPS"].successful
        assert 0 <= out[q]["entry"] < len(lib)
    assert len(lib) == len(lib0["tf"])
    # an empty library: K = 1 is the plain straight-line solve; the fan answers its failures; the winners are learnt
    empty = H.TrajLib(0, 50, 64)
    _, TOSe = host_problems(16)
    oute = H.solve_SCP_trajlib_batch(TOSe, TOPs, empty, K=1, fallback_fan=True, learn=True)
    cold = d["cold"]
    ok = cold["st"]["converged"].astype(bool) & cold["st"]["successful"].astype(bool)
    assert not ok.all()
    for q in range(16):
        assert oute[q]["entry"] == -1
        if ok[q]:
            assert oute[q]["source"] == "library" and oute[q]["winner"] == 0 and np.array_equal(oute[q]["SCPS"].traj.X.T, cold["X"][q])
        else:
            assert oute[q]["source"] in ("fan", None) and (oute[q]["winner"] > 0 or oute[q]["winner"] == -1)
    solved = sum(o["winner"] >= 0 for o in oute)
    assert solved > ok.sum() and len(empty) == solved
    got = empty.get()
    assert np.array_equal(got["X"][:ok.sum()], cold["X"][ok]) and np.array_equal(got["x_init"][:ok.sum()], d["queries"][0][ok])
    with pytest.raises(ValueError):
        H.solve_SCP_trajlib_batch(TOSs, TOPs, H.TrajLib(0, 49, 4))
    lib.close()
    empty.close()


def test_c_consumer(tmp_path):
    """tests/c/c_abi_trajlib.c, a plain C consumer with checks of its own; the seeds and winners it prints are the Python path's"""
    exe = os.path.join(tmp_path, "c_abi_trajlib")
    libdir = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "c", "c_abi_trajlib.c"), "-o", exe, "-L" + libdir, "-lgusto_hip", "-lm",
                           "-Wl,-rpath," + libdir])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and lines[1] == "4" and len(lines) == 5
    goal = [3.0, 0.5, 0, 0.05, -0.05, 0]
    lx = np.array([[0.25, 2.3, 0, 0, 0, 0], [0.5, 1.8, 0, 0, 0, 0], [0.3, 0.5, 0, 0, 0, 0], [1.0, 0.3, 0, 0, 0, 0]], float)
    x0 = np.array([[0.2, 2.4, 0, 0, 0, 0], [0.4, 1.9, 0, 0, 0, 0], [0.3, 0.4, 0, 0, 0, 0]], float)
    s = g.BatchSolver(0, 50, 6, hist_cap=64, boxes=np.array([[1.4, 0.9, -0.2, 1.8, 1.5, 0.2]]))
    s.set_problems(lx, np.tile(goal, (4, 1)), np.tile(goal, (4, 1)), [200.0, 150.0, 100.0, 100.0])
    s.solve(30)
    lib = g.TrajLib(0, 50, 6)
    assert lib.add_from(s, np.ones(4)) == 4
    s.set_problems_trajlib(lib, x0, np.tile(goal, (3, 1)), np.tile(goal, (3, 1)), [200.0, 150.0, 100.0], 2)
    seeds = s.trajlib_seeds()
    s.solve(30)
    r = s.select_best(2)
    for q in range(3):
        v = lines[2 + q].split()
        assert (int(v[0]), int(v[1]), int(v[2])) == (seeds["entry"][q, 0], seeds["entry"][q, 1], seeds["n_found"][q])
        assert float(v[3]) == seeds["dist2"][q, 0] and int(v[4]) == r["winner"][q]
    s.close()
    lib.close()
