"""What tests/test_gpu_shoot.py relies on, proved without a GPU: tests/np_shoot.py (the restatement of gusto_shoot, float64 and
np.longdouble) against the oracle's go_shoot and against scipy, the figures the device tolerances are derived from, and the
conditions the case families of tests/shoot_cases.py state.  tools/shoot_errors.py prints the figures (profiles/shoot_tests.txt).

Figures (this file measures them; the GPU tests take the constants below and this file asserts that they are the derived ones):
  float64 against longdouble, extremals of every roll-out case and of every :Optimal one-step / straggler problem, relative to
  max(1, |value|):                                           dubins 3.7e-14   manifold 2.8e-14
  -> TOL_X = 100 x that, rounded up to a power of ten:       dubins 1e-11     manifold 1e-11
  float64 restatement against the oracle, p0 after one Newton step, conditioned problems, relative to max(1, |p0|_inf):
                                                             dubins 5.5e-9    manifold 2.1e-9
  -> TOL_P0 = 100 x that, rounded up to a power of ten:      dubins 1e-6      manifold 1e-6

Conditioned problems.  An SCP run that fails leaves a dual of 1e2 .. 1e16 (a converged one: below 12), and the one-step cases take the duals as they are (3 of
the 8 dubins problems at N = 5, 2 at N = 30).  From such a seed theta runs through 1e2 .. 1e12 radians within a step of RK4: the
end point of the float64 and of the longdouble extremal differ in every digit (N = 30, substeps = 1, problem 1: theta(tf) = -177
against -1195), a forward difference with h = 1e-6 |p| is noise, and whether the line search finds a decrease is a coin toss --
the oracle takes one step there, both restatements none.  A problem counts as conditioned when the end points of its float64 and
longdouble extremals from the seed agree to CONDITIONED = 1e-9 (three digits below the difference step); status and newton_iters
of the restatement, the oracle and the device must be equal on every conditioned problem, and at least 5 of the 8 problems of every
one-step case are conditioned.  The straggler batches hold conditioned problems only."""
import functools

import numpy as np
import pytest

import np_shoot as NS
import shoot_cases as SC

DUB, MAN = SC.DUB, SC.MAN
TOL_X = {DUB: 1e-11, MAN: 1e-11}
TOL_P0 = {DUB: 1e-6, MAN: 1e-6}
CONDITIONED = 1e-9


def conditioned(inp):
    """[B] bool: the end point of the extremal from the seed is the same in float64 and longdouble to CONDITIONED"""
    X64, Xld = SC.extremal(inp, inp.p0, np.float64)[0], SC.extremal(inp, inp.p0, np.longdouble)[0]
    return np.array([SC.rel_err(X64[b, -1], Xld[b, -1]) <= CONDITIONED for b in range(len(inp.tf))])


@functools.lru_cache(maxsize=None)
def cpu_sides(kind, case):
    """(inputs, oracle, float64 restatement, longdouble restatement, conditioned) of a one-step case or a straggler batch"""
    inp = SC.one_step(case) if kind == "one_step" else SC.stragglers(case)
    return inp, SC.oracle_shoot(inp), SC.restated(inp), SC.restated(inp, np.longdouble), conditioned(inp)


def classes(model):
    """the straggler batch by what the oracle does: (early, late and :Optimal, late and :Diverged) index arrays"""
    ora = cpu_sides("stragglers", model)[1]
    it, st = np.array([o["newton_iters"] for o in ora]), np.array([o["status"] for o in ora])
    late = it > SC.SHOOT_CAP
    return np.flatnonzero(~late), np.flatnonzero(late & (st == 1)), np.flatnonzero(late & (st == 0))


def x_figure(inp, p0s, rows):
    """float64 against longdouble on the extremals from p0s [B, n] over the problems `rows`"""
    if len(rows) == 0:
        return 0.0
    X64, U64 = SC.extremal(inp, p0s, np.float64)
    Xld, Uld = SC.extremal(inp, p0s, np.longdouble)
    return max(SC.rel_err(X64[rows], Xld[rows]), SC.rel_err(U64[rows], Uld[rows]))


def rollout_figure(case):
    inp = SC.rollout(case)
    return x_figure(inp, inp.p0, np.flatnonzero(np.isfinite(inp.p0).all(axis=1)))


def newton_figures(kind, case):
    """(float64 against longdouble on the extremals of the :Optimal problems, float64 restatement against the oracle on p0 and on X
    of the conditioned problems, how many problems were left out of the newton_iters comparison)"""
    inp, ora, r64, rld, cond = cpu_sides(kind, case)
    B = len(ora)
    opt = np.array([b for b in range(B) if r64[b]["status"] == 1], dtype=int)
    fx = x_figure(inp, np.stack([r["p0"] for r in r64]), opt)
    fp = max([SC.rel_inf(r64[b]["p0"], ora[b]["p0"]) for b in range(B) if cond[b] and same_path(ora[b], r64[b])] + [0.0])
    fX = max([SC.rel_err(r64[b]["X"], ora[b]["X"]) for b in opt if cond[b] and ora[b]["status"] == 1] + [0.0])
    return fx, fp, fX, sum(not compared(ora[b], r64[b], rld[b], cond[b]) for b in range(B))


def same_path(a, b):
    return a["status"] == b["status"] and a["newton_iters"] == b["newton_iters"]


def compared(o, r, l, cond):
    """whether newton_iters of this problem is compared: not from an unconditioned seed, and not in a long run that does not
    converge and in which the float64 and the longdouble restatement part ways (the line search fails on a rounding error)"""
    long_diverged = o["status"] == 0 and o["newton_iters"] > SC.SHOOT_CAP
    return bool(cond) and not (long_diverged and r["newton_iters"] != l["newton_iters"])


def model_figures(model):
    """(TOL_X's figure, TOL_P0's figure) of a model over all its cases"""
    fx = [rollout_figure(c) for c in SC.ROLLOUT if c[0] == model]
    nf = [newton_figures("one_step", c) for c in SC.ONE_STEP if c[0] == model] + [newton_figures("stragglers", model)]
    return max(fx + [f[0] for f in nf]), max(f[1] for f in nf[:-1])


# ---- the restatement ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("b", [0, 3])
def test_restated_dubins_extremal_against_scipy(b):
    """RK4 at 16 substeps per interval against an adaptive integration (RK45 at 1e-12) of the ODE as tests/test_shooting.py states it"""
    from scipy.integrate import solve_ivp
    N = 30
    x0, _, _, tf = SC.base(DUB, b + 1)
    p0 = SC.dual(DUB, N, b)
    X, U = NS.extremal(DUB, x0[b], p0, tf[b], N, 16, SC.par(DUB))

    def ode(t, z):
        th, px, py, pth = z[2], z[3], z[4], z[5]
        return [2.0 * np.cos(th), 2.0 * np.sin(th), 0.5 * pth, 0.0, 0.0, px * 2.0 * np.sin(th) - py * 2.0 * np.cos(th)]

    sol = solve_ivp(ode, (0, tf[b]), np.concatenate([x0[b], p0]), rtol=1e-12, atol=1e-14, t_eval=np.linspace(0, tf[b], N))
    assert sol.success and np.abs(sol.y[:3].T - X).max() < 1e-6 and np.abs(0.5 * sol.y[5] - U[:, 0]).max() < 1e-6


def test_restated_manifold_ode_is_the_one_scipy_integrates():
    """the quaternion-algebra statement of tests/np_shoot.py against the component-wise one of tests/test_shooting.py, under the
    anisotropic inertia, at random points"""
    import test_shooting as TS
    rng = np.random.default_rng(5)
    par = SC.par(MAN, "nondefault")
    ode = TS._manifold_ode(par["mass"], par["J"])
    for _ in range(20):
        z = rng.normal(size=26)
        assert np.abs(NS.rhs(MAN, z, par) - ode(0.0, z)).max() < 1e-14 * np.abs(z).max() ** 2


def test_goal_point_and_newton_step():
    lo, hi = np.array([1.0, -np.inf, 2.0, 0.0, np.nan]), np.array([3.0, 5.0, np.inf, 0.0, 1.0])
    assert np.array_equal(NS.goal_point(lo, hi), [2.0, 0.0, 0.0, 0.0, 0.0])
    rng = np.random.default_rng(3)
    for dtype in (np.float64, np.longdouble):
        J, F = rng.normal(size=(3, 3)).astype(dtype), rng.normal(size=3).astype(dtype)
        assert np.abs(J @ NS.newton_step(J, F) + F).max() < 1e-13
        A, F = rng.normal(size=(13, 13)).astype(dtype), rng.normal(size=13).astype(dtype)
        assert np.abs(A @ NS.newton_step(A, F) + F).max() < 1e-11
        v = rng.normal(size=13).astype(dtype)
        v /= np.sqrt(v @ v)
        A1 = A - np.outer(A @ v, v)                       # rank 12: A1 v = 0.  The step solves the 12 pivoted equations
        dp = NS.newton_step(A1, A1 @ F)                   # of a consistent system and leaves one component at 0
        assert (dp == 0).sum() == 1 and np.abs(A1 @ dp + A1 @ F).max() < 1e-9
    assert NS.newton_step(np.zeros((3, 3)), np.ones(3)) is None and NS.newton_step(np.zeros((13, 13)), np.ones(13)) is None
    assert NS.newton_step(np.full((13, 13), np.nan), np.ones(13)) is None


# ---- roll-out cases -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.ROLLOUT, ids=SC.case_id)
def test_rollout_cases_are_what_they_say(case):
    model, B, N, substeps, pcase = case
    inp = SC.rollout(case)
    assert inp.p0.shape == (B, NS.DIMS[model][0]) and (inp.max_newton, inp.ftol) == (0, 1e300)
    fin = np.isfinite(inp.p0).all(axis=1)
    expect = np.ones(B, bool)
    if B >= 33:
        expect[SC.NAN_PROBLEM] = False
    assert np.array_equal(fin, expect)
    assert (np.abs(inp.p0[fin]).max(axis=1) > 0).sum() >= fin.sum() - 1 and (np.abs(inp.p0[fin]) <= SC.SEED_CAP[model] * (1 + 1e-12)).all()
    if B > 1:
        assert (inp.glo[1] < inp.ghi[1]).all() and not np.allclose(NS.goal_point(inp.glo[1], inp.ghi[1]), SC.base(model, B)[1][1])
    if B > 2:
        assert np.isinf(inp.glo[2]).sum() == 1 and np.isinf(inp.ghi[2]).sum() == 1 and NS.goal_point(inp.glo[2], inp.ghi[2])[1] == 0
    Xld, Uld = SC.extremal(inp, inp.p0, np.longdouble)
    assert np.abs(Xld[fin]).max() <= SC.X_BOUND and np.isfinite(Uld[fin]).all()
    if fin.any():                                          # the costates move the state: no roll-out is the one of p0 = 0
        X0 = SC.extremal(inp, np.zeros_like(inp.p0), np.longdouble)[0]
        assert np.abs(Xld[fin] - X0[fin]).max() > 1e-2
    ora = SC.oracle_shoot(inp)                             # the oracle's roll-out, at the tolerance the device gets
    for b in np.flatnonzero(fin):
        assert ora[b]["status"] == 1 and ora[b]["newton_iters"] == 0
        assert SC.rel_err(ora[b]["X"], Xld[b]) <= TOL_X[model] and SC.rel_err(ora[b]["U"], Uld[b]) <= TOL_X[model]
    for b in np.flatnonzero(~fin):
        assert ora[b]["status"] == 0 and ora[b]["newton_iters"] == 0 and np.isnan(ora[b]["resid"])


# ---- one step, stragglers ---------------------------------------------------------------------------------------------------------
def _check_against_the_oracle(kind, case):
    inp, ora, r64, rld, cond = cpu_sides(kind, case)
    left_out = 0
    for b, (o, r, l) in enumerate(zip(ora, r64, rld)):
        if not cond[b]:
            left_out += 1
            continue
        assert r["status"] == o["status"] == l["status"], (case, b)
        if compared(o, r, l, cond[b]):
            assert r["newton_iters"] == o["newton_iters"], (case, b, r["newton_iters"], l["newton_iters"], o["newton_iters"])
        else:
            left_out += 1
    return left_out


@pytest.mark.parametrize("case", SC.ONE_STEP, ids=lambda c: SC.case_id(c))
def test_one_step_restatement_against_the_oracle(case):
    inp, ora, r64, rld, cond = cpu_sides("one_step", case)
    assert len(ora) == SC.ONE_STEP_B == 8 and cond.sum() >= 5 and (inp.max_newton, inp.ftol) == (1, 1e-3)
    assert (np.abs(inp.p0[~cond]).max(axis=1) > 1e2).all()                # the unconditioned seeds are duals of failed SCP runs
    assert _check_against_the_oracle("one_step", case) == (~cond).sum()
    assert max(o["newton_iters"] for o in ora) == 1
    fx, fp, fX, _ = newton_figures("one_step", case)
    print(SC.case_id(case), f"float64 against longdouble {fx:.2e}  restatement against oracle: p0 {fp:.2e} X {fX:.2e}")
    assert fx <= TOL_X[case[0]] / 100 and fp <= TOL_P0[case[0]] / 100


@pytest.mark.parametrize("model", [DUB, MAN], ids=[SC.NAME[DUB], SC.NAME[MAN]])
def test_straggler_batches_are_what_they_say(model):
    inp, ora, r64, rld, cond = cpu_sides("stragglers", model)
    B = len(ora)
    early, late_ok, late_no = classes(model)
    print(SC.NAME[model], "early", [(b, ora[b]["status"], ora[b]["newton_iters"]) for b in early],
          "late :Optimal", [(b, ora[b]["newton_iters"], ora[b]["resid"]) for b in late_ok],
          "late :Diverged", [(b, ora[b]["newton_iters"], ora[b]["resid"]) for b in late_no])
    assert 8 <= B <= 16 and cond.all()
    assert len(late_ok) >= 3 and len(late_no) >= 3 and (len(late_ok) + len(late_no)) % 4 != 0
    assert any(ora[b]["status"] == 1 for b in early) and len(early) >= 3
    assert all(ora[b]["resid"] <= 0.99 * inp.ftol for b in range(B) if ora[b]["status"] == 1)     # no problem converges on the edge
    assert any(ora[b]["newton_iters"] == 100 for b in late_no) or model == DUB
    left_out = _check_against_the_oracle("stragglers", model)
    print(SC.NAME[model], "left out of the newton_iters comparison:", left_out, "of", B)
    assert 4 * left_out <= B
    fx, fp, fX, _ = newton_figures("stragglers", model)
    print(SC.NAME[model], f"float64 against longdouble {fx:.2e}  restatement against oracle: p0 {fp:.2e} X {fX:.2e}")
    assert fx <= TOL_X[model] / 100
    # what max_newton = 0, 1, 8, 9 do to this batch (tests/test_gpu_shoot.py): the oracle stops where the cap says
    for cap in (0, 1, 8, 9):
        capped = SC.oracle_shoot(SC.stragglers(model, cap))
        for b in range(B):
            if ora[b]["newton_iters"] <= cap:
                assert same_path(capped[b], ora[b]) and np.array_equal(capped[b]["p0"], ora[b]["p0"])
            else:
                assert capped[b]["status"] == 0 and capped[b]["newton_iters"] == cap


@pytest.mark.parametrize("model", [DUB, MAN], ids=[SC.NAME[DUB], SC.NAME[MAN]])
def test_the_tolerances_are_the_derived_ones(model):
    fx, fp = model_figures(model)
    print(SC.NAME[model], f"float64 against longdouble {fx:.3e} -> {SC.tol_from(fx):.0e}; restatement against oracle, p0 {fp:.3e} -> {SC.tol_from(fp):.0e}")
    assert SC.tol_from(fx) == TOL_X[model] and SC.tol_from(fp) == TOL_P0[model]
