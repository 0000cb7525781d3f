"""gusto_shoot on the device against tests/np_shoot.py, the numpy restatement of the scheme in np.longdouble; tests/test_shoot_cpu.py
pins the restatement against the oracle and scipy, states which problems are conditioned, and derives the tolerances without a GPU.

Inputs: tests/shoot_cases.py.  Every seed comes from the host (no gusto_solve), so the cases reach N = 3 and N = 256, B = 1 .. 65
(R = N n and B on both sides of the 32 x 32 transposition tiles), box goals, coordinates without a goal, NaN seeds, non-default
dubins_v / dubins_k, anisotropic inertia and non-default mass.

The certificate: whatever path Newton took, the X and U the device returns for an :Optimal problem are the extremal from the p0 it
returns, and resid is the distance of that extremal's end from the goal point.  Both are compared with the longdouble restatement
from the DEVICE's p0, so the tolerance is that of one integration: TOL_X = 100 x the largest float64-against-longdouble difference
over the cases, rounded up to a power of ten, relative to max(1, |value|) (tests/test_shoot_cpu.py: dubins 3.7e-14, manifold
2.8e-14 -> 1e-11).  Measured on an MI355X (tools/shoot_errors.py --device, profiles/shoot_tests.txt): dubins 4.4e-14, manifold 2.8e-14.

One Newton step is also compared with the float64 restatement and the oracle on the conditioned problems: status and newton_iters
equal, p0 to TOL_P0 = 100 x the largest difference between those two CPU implementations on the same cases (5.5e-9 -> 1e-6,
relative to max(1, |p0|_inf)); the device is 6.7e-9 from them."""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import np_shoot as NS
import shoot_cases as SC
import test_shoot_cpu as TC

pytestmark = pytest.mark.gpu

DUB, MAN = SC.DUB, SC.MAN
MODELS = pytest.mark.parametrize("model", [DUB, MAN], ids=[SC.NAME[DUB], SC.NAME[MAN]])
KEYS = ("status", "newton_iters", "resid", "p0")


def solver(inp, B=None, cap=None):
    """a handle of `cap` problems with the first B problems of the inputs"""
    B = B or len(inp.tf)
    s = g.BatchSolver(inp.model, inp.N, cap or B, hist_cap=8, model_params=SC.model_params(g, inp.model, inp.pcase))
    s.set_problems(inp.x0[:B], inp.glo[:B], inp.ghi[:B], inp.tf[:B])
    return s


def shoot(s, inp, B=None, **kw):
    B = B or len(inp.tf)
    return s.shoot(**dict(dict(p0=inp.p0[:B], substeps=inp.substeps, max_newton=inp.max_newton, ftol=inp.ftol), **kw))


def same(a, b, rows=None, what=None):
    """status, newton_iters, resid, p0 of the problems `rows` and X, U of the :Optimal ones among them: bit for bit"""
    rows = np.arange(len(a["status"])) if rows is None else np.asarray(rows)
    for k in KEYS:
        assert np.array_equal(a[k][rows], b[k][rows], equal_nan=True), (what, k)
    ok = rows[a["status"][rows] == 1]
    assert np.array_equal(a["X"][ok], b["X"][ok]) and np.array_equal(a["U"][ok], b["U"][ok]), what


def certify(inp, r, rows=None, what=None):
    """every :Optimal problem of `rows`: X, U are the extremal from the returned p0 and resid its distance from the goal point, to
    TOL_X; every other problem: X and U are zeros.  Returns the largest error seen."""
    B = len(r["status"])
    rows = np.arange(B) if rows is None else np.asarray(rows)
    tol = TC.TOL_X[inp.model]
    sub = SC.Inputs(*[a[:B] if isinstance(a, np.ndarray) else a for a in inp])
    Xr, Ur = SC.extremal(sub, r["p0"], np.longdouble)
    xg = NS.goal_point(sub.glo.astype(np.longdouble), sub.ghi.astype(np.longdouble))
    worst = 0.0
    for b in rows:
        if r["status"][b] != 1:
            assert r["status"][b] == 0 and not r["X"][b].any() and not r["U"][b].any(), (what, b)
            continue
        res = NS.norm_inf(xg[b] - Xr[b, -1])
        e = max(SC.rel_err(r["X"][b], Xr[b]), SC.rel_err(r["U"][b], Ur[b]), SC.rel_err(r["resid"][b], res))
        assert np.isfinite(r["X"][b]).all() and np.isfinite(r["U"][b]).all() and e <= tol, (what, b, e)
        assert r["resid"][b] <= inp.ftol, (what, b)
        assert np.array_equal(r["X"][b, 0], sub.x0[b]), (what, b)
        worst = max(worst, e)
    return worst


# ---- roll-out --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rollout_on_device(case):
    inp = SC.rollout(case)
    s = solver(inp)
    r = shoot(s, inp)
    s.close()
    return r


@pytest.mark.parametrize("case", SC.ROLLOUT, ids=SC.case_id)
def test_rollout_certificate(case):
    """max_newton = 0, ftol = 1e300: integrate, get_control, the knot-major staging and both transposes, nothing else"""
    inp, r = SC.rollout(case), rollout_on_device(case)
    fin = np.isfinite(inp.p0).all(axis=1)
    assert np.array_equal(r["status"], fin.astype(np.int32)) and not r["newton_iters"].any()
    assert np.array_equal(r["p0"].view(np.uint64), inp.p0.view(np.uint64))                   # the seed, bit for bit
    assert np.isnan(r["resid"][~fin]).all() and np.isfinite(r["resid"][fin]).all()
    e = certify(inp, r, what=case)
    # the same against the extremal from the SEED (certify took the returned p0)
    Xr, Ur = SC.extremal(inp, inp.p0, np.longdouble)
    assert SC.rel_err(r["X"][fin], Xr[fin]) <= TC.TOL_X[inp.model] and SC.rel_err(r["U"][fin], Ur[fin]) <= TC.TOL_X[inp.model]
    print(SC.case_id(case), f"device against longdouble {e:.2e}")


# ---- one Newton step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SC.ONE_STEP, ids=SC.case_id)
def test_one_newton_step_against_the_restatement_and_the_oracle(case):
    inp, ora, r64, rld, cond = TC.cpu_sides("one_step", case)
    s = solver(inp)
    r = shoot(s, inp)
    s.close()
    assert ((r["status"] == 0) | (r["status"] == 1)).all() and (r["newton_iters"] <= 1).all()
    worst = 0.0
    for b in np.flatnonzero(cond):
        for ref in (ora[b], r64[b]):
            assert (r["status"][b], r["newton_iters"][b]) == (ref["status"], ref["newton_iters"]), (case, b)
            e = SC.rel_inf(r["p0"][b], ref["p0"])
            assert e <= TC.TOL_P0[inp.model], (case, b, e)
            worst = max(worst, e)
    e = certify(inp, r, what=case)
    print(SC.case_id(case), f"p0: device against restatement / oracle {worst:.2e}; certificate {e:.2e}")


# ---- stragglers ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stragglers_on_device(model):
    """(the straggler batch with the group pass, without it), on one handle"""
    inp = SC.stragglers(model)
    s = solver(inp)
    two, one = shoot(s, inp), shoot(s, inp, group_pass=False)
    s.close()
    return two, one


@MODELS
def test_group_pass_changes_nothing(model):
    """shoot_group_kernel (16 lanes per problem, the Jacobian through LDS) against the lane-per-problem pass alone, bit for bit, on a
    batch whose stragglers do not fill the last wave of the group kernel; and the certificate on every :Optimal problem of both"""
    inp = SC.stragglers(model)
    two, one = stragglers_on_device(model)
    late = two["newton_iters"] > SC.SHOOT_CAP
    print(SC.NAME[model], "stragglers", int(late.sum()), "converged", int((two["status"][late] == 1).sum()), "newton_iters", two["newton_iters"].tolist())
    assert (two["status"][late] == 1).any() and (two["status"][late] == 0).any() and late.sum() % 4 != 0
    assert (two["status"][~late] == 1).any()
    same(two, one, what=model)
    e = max(certify(inp, two, what=(model, "two")), certify(inp, one, what=(model, "one")))
    print(SC.NAME[model], f"certificate {e:.2e}")


@MODELS
@pytest.mark.parametrize("cap", [0, 1, 8, 9])
def test_max_newton_caps(model, cap):
    """max_newton <= 8 takes no group pass, 9 exactly one step of it"""
    inp = SC.stragglers(model, cap)
    full = stragglers_on_device(model)[0]
    s = solver(inp)
    two, one = shoot(s, inp), shoot(s, inp, group_pass=False)
    s.close()
    same(two, one, what=(model, cap))
    assert (two["newton_iters"] <= cap).all()
    done = (full["status"] == 1) & (full["newton_iters"] <= cap)
    same(two, full, np.flatnonzero(done), what=(model, cap, "converged within the cap"))
    assert (two["status"][~done] == 0).all() and (two["newton_iters"][full["newton_iters"] > cap] == cap).all()
    certify(inp, two, what=(model, cap))


@MODELS
def test_mask_together_with_stragglers(model):
    inp = SC.stragglers(model)
    early, late_ok, late_no = TC.classes(model)
    B = len(inp.tf)
    act = np.ones(B, bool)
    act[[early[0], late_ok[0], late_no[0]]] = False
    s = solver(inp)
    full = shoot(s, inp)
    s.set_active(act)
    part = shoot(s, inp)
    s.set_active(None)
    again = shoot(s, inp)
    s.close()
    same(full, stragglers_on_device(model)[0], what=(model, "another handle"))
    same(part, full, np.flatnonzero(act), what=(model, "active"))
    off = ~act
    assert not part["status"][off].any() and not part["newton_iters"][off].any() and np.isnan(part["resid"][off]).all()
    assert np.array_equal(part["p0"][off], inp.p0[off]) and not part["X"][off].any() and not part["U"][off].any()
    certify(inp, part, what=(model, "masked"))
    same(again, full, what=(model, "unmasked again"))


@MODELS
def test_rows_of_problems_that_are_not_optimal(model):
    """gusto_get_shoot after a call in which a problem diverges: its X and U are zeros, not the trajectory an earlier call or an
    earlier batch left in the handle's buffers"""
    inp = SC.stragglers(model)
    B = len(inp.tf)
    s = solver(inp)
    roll = shoot(s, inp, **SC.ROLL_OPTS)                   # every problem :Optimal: every row of the handle's X and U is written
    assert roll["status"].all()
    certify(inp._replace(ftol=SC.ROLL_OPTS["ftol"]), roll, what=(model, "roll-out"))
    r = shoot(s, inp)
    assert (r["status"] == 0).sum() >= 3 and (r["status"] == 1).sum() >= 3
    certify(inp, r, what=(model, "after a roll-out"))      # zeros for the problems that are not :Optimal
    same(r, stragglers_on_device(model)[0], what=(model, "fresh handle"))
    keep = np.flatnonzero(r["status"] == 0)[:2].tolist() + np.flatnonzero(r["status"] == 1)[:3].tolist()
    keep = np.array(sorted(keep))[::-1]                    # a smaller batch, the problems in another order
    sub = SC.Inputs(*[np.ascontiguousarray(a[keep]) if isinstance(a, np.ndarray) else a for a in inp])
    s.set_problems(sub.x0, sub.glo, sub.ghi, sub.tf)
    q = shoot(s, sub)
    s.close()
    assert q["X"].shape[0] == len(keep)
    certify(sub, q, what=(model, "smaller batch"))
    for k in KEYS:
        assert np.array_equal(q[k], r[k][keep], equal_nan=True), (model, k)
    ok = q["status"] == 1
    assert np.array_equal(q["X"][ok], r["X"][keep][ok]) and np.array_equal(q["U"][ok], r["U"][keep][ok])
