"""The device's GuSTO outer loop (csrc/scp.hpp, scp_gusto.jl:123-175) under non-default SCP parameters (tests/scp_param_cases.py).
At the model defaults no lock-step trip of the suite changes Delta; here the runs shrink and grow the trust region, stop at omega_max,
converge at the `iterations > 2` guard and run past convergence.  tests/test_scp_params_cpu.py proves on the CPU that the sets reach
those branches, that the forced states keep their margins and that three wrong tables would be seen on them.

  - natural lock-step trips: test_gpu_parity._lockstep_parity under ladder and ceiling, every trip of 8 problems -- freeflyerSE2 at
    N = 5 and 50, dubins_car at 30, the Astrobee models at N = 16 with one, two and four waves per problem and at N = 65;
  - forced trips: one trip from a chosen Delta (scp_param_cases.forced: grow and split) through the same assertions
    (test_gpu_parity._trip_checks), the reference np_scp_trip's restatement of the verdict table;
  - whole runs at N = 16, 16 problems, under ladder, ceiling and loose; loose from converged trajectories; loose with force = 1;
  - the scheduler's level function under ceiling's omega0 and gamma_fail: results bit-identical to the unscheduled run;
  - gusto_set_params(sp, NULL) on a live handle.
The census of every case is printed (-s); profiles/scp_params.txt holds a run."""
import numpy as np
import pytest

import gusto_jl_amd as g
import scp_param_cases as SC
import test_gpu_parity as TP
import test_kkt_certificate as T
from test_gpu_horizons import LOCKSTEP_ARGS
from test_gpu_kkt import WAVE, WAVE2, WAVE4

pytestmark = pytest.mark.gpu

FF, DUB, SE3, MAN = SC.FF, SC.DUB, SC.SE3, SC.MAN
DEC_NAME = {None: "auto", WAVE: "wave", WAVE2: "wave2", WAVE4: "wave4"}
# (model, N, decomposition): the chain kernels exist for the 12/13-state models below 65 knots
KERNELS = [(m, N, d) for m in SC.MODELS for N in SC.HORIZONS[m]
           for d in ((None,) if m in (FF, DUB) else (WAVE, WAVE2, WAVE4) if N == 16 else (WAVE,))]
# whole runs of the 12/13-state models: as the library chooses the kernel, and with one, two and four waves per problem
RUN_DECS = {FF: (None,), DUB: (None,), SE3: (None, WAVE, WAVE2, WAVE4), MAN: (None, WAVE, WAVE2, WAVE4)}
# arguments of _scp_parity as the whole-run tests of tests/test_gpu_parity.py pass them for the model.  The manifold model's X is
# weakly determined inside the +-1e-4 BoxGoal on q: LOCKSTEP_ARGS gates two solves of one trip at sub_atol = 3e-4 in X, and the
# convergence measure max_k |x_k - xprev_k| / max_k |x_k| is the difference of two such solves over max_k |x_k| >= 9.66 (the 16
# problems at N = 16): 2 x 3e-4 / 9.66.  Measured on the ORACLE alone, cold against warm start of the same 16 runs: 3.3e-5 under
# ceiling (problem 12, third trip: 5.2e-5 against 1.9e-5), 8.7e-6 under ladder, 7.4e-6 under loose; tol / 4: 7.7e-6.
MAN_CONV_ATOL = 2 * LOCKSTEP_ARGS[SC.MAN]["sub_atol"] / 9.66
SCP_ARGS = {FF: {}, DUB: dict(max_diverged=1), SE3: {}, MAN: dict(rtol=1e-3, conv_atol=MAN_CONV_ATOL)}


def _kid(m, N, d):
    return f"{T.NAME[m]}-{N}-{DEC_NAME[d]}"


def _dev(sp):
    return T.as_params(g.ScpParams, sp)


def _decomposition(monkeypatch, dec):
    if dec is not None:
        monkeypatch.setattr(g.BatchSolver, "default_decomposition", dec)


def _trip_census(status, D_before, D_after, sp, pick):
    """census of single trips (entry 0: the state the trip started from)"""
    return SC.total(SC.census(dict(scp_status=[0, status[i]], Delta=[D_before[i], D_after[i]]), sp) for i in np.nonzero(pick)[0])


# ---- natural lock-step trips ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ladder", "ceiling"])
@pytest.mark.parametrize("model,N,dec", [pytest.param(*k, id=_kid(*k)) for k in KERNELS])
def test_lockstep_trips(name, model, N, dec, monkeypatch):
    _decomposition(monkeypatch, dec)
    boxes, sph = T.env(model)
    sp = SC.params(name, model)
    x0, glo, ghi, tf = SC.batch(model)
    out = {}
    info = TP._lockstep_parity(model, N, boxes, sph, x0, glo, ghi, tf, max_iter=SC.MAX_ITER, scp_params=sp, out=out,
                               **{**LOCKSTEP_ARGS[model], **SC.GATES.get((model, N), {})})
    h, same, runs, trips = out["h"], out["same"], out["runs"], out["trips"]
    dev = _trip_census(h["scp_status"][:, 1], h["Delta"][:, 0], h["Delta"][:, 1], sp, same)
    R = lambda k, d: np.array([runs[b][0][k][t + d] for b, t in trips])
    ora = _trip_census(R("scp_status", 1), R("Delta", 0), R("Delta", 1), sp, same)
    print(f"scp_params lockstep {name} {_kid(model, N, dec)}", info, "| device census:", SC.short(dev))
    assert dev == ora, (dev, ora)
    if name == "ladder":                 # what the set is there for (dubins_car, the manifold model and astrobeeSE3 at N = 65 never grow)
        assert dev["shrink"] >= 3, dev
        if (model, N) in ((FF, 5), (FF, 50), (SE3, 16)):
            assert dev["grow"] >= 3 and dev["grow_capped"] >= 1, dev


# ---- forced trips -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N,dec", [pytest.param(*k, id=_kid(*k)) for k in KERNELS])
def test_forced_trips(model, N, dec, monkeypatch):
    """every outcome of the Delta update on every kernel: reject and shrink, keep, grow, grow cut at Delta0"""
    _decomposition(monkeypatch, dec)
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = SC.batch(model, SC.FORCED_B)
    args = LOCKSTEP_ARGS[model]
    forced = SC.forced(model, N)
    dev = dict.fromkeys(SC.CENSUS_KEYS, 0)
    for name in SC.FORCED_SETS:
        sp, pts = forced[name]
        bi = np.array([p["b"] for p in pts])
        A = lambda k: np.array([p[k] for p in pts])
        ref = {k: np.array([p["ref"][kr] for p in pts]) for k, kr in
               dict(conv="conv", obj="obj", iters="ipm_iters", J="J_true", rho="rho", tr_sat="tr_sat", cvx_sat="cvx_sat", accept="accept",
                    scp_status="scp_status", Delta="Delta_next", omega="omega_next").items()}
        s = g.BatchSolver(model, N, len(pts), hist_cap=8, boxes=boxes, spheres=sph, scp_params=_dev(sp))
        s.set_schedule(0, 1)
        s.set_problems(x0[bi], glo[bi], ghi[bi], tf[bi], np.stack(A("Xp")), np.stack(A("Up")))
        s.set_trust_state(A("Delta"), A("omega"))
        s.solve(1)
        h = s.history()
        t2 = TP._trip_checks(h, s.status(), ref, A("omega"), args.get("sub_atol", TP.SUB_ATOL), args.get("max_flag_mismatch", 0.005),
                             [(name, p["b"], p["t"], p["Delta"]) for p in pts])
        s.close()
        assert np.array_equal(h["Delta"][:, 0], A("Delta"))
        c = _trip_census(h["scp_status"][:, 1], h["Delta"][:, 0], h["Delta"][:, 1], sp, np.ones(len(pts), bool))
        print(f"scp_params forced {name} {_kid(model, N, dec)}: {len(pts)} trips, rho1 {sp.rho1:.3g}, flag mismatches "
              f"{int((~t2['same']).sum())}, worst relative rho difference {t2['worst_rho']:.1e} | device census: {SC.short(c)}")
        dev = SC.add(dev, c)
    assert dev["shrink"] >= 3 and dev["grow"] >= 3 and dev["grow_capped"] >= 3, dev


# ---- whole runs -------------------------------------------------------------------------------------------------------------
def _whole(name, model, omega_max=0.1, force=False, max_iter=SC.MAX_ITER, **args):
    boxes, sph = T.env(model)
    sp = SC.params(name, model, omega_max)
    out = {}
    div = TP._scp_parity(model, 16, boxes, sph, *SC.batch(model, 16), max_iter=max_iter, scp_params=sp, force=force, out=out,
                         **{**SCP_ARGS[model], **args})
    st, h = out["st"], out["h"]
    c = SC.total(SC.census({k: h[k][b, :h["n_hist"][b]] for k in ("scp_status", "Delta", "omega")}, sp, st["stop_reason"][b],
                           st["iterations"][b]) for b in range(16))
    print(f"scp_params whole runs {name}{' force' if force else ''} omega_max={sp.omega_max:g} {T.NAME[model]} "
          f"{DEC_NAME[g.BatchSolver.default_decomposition or None]}: diverged {div} | "
          f"device census: {SC.short(c)}")
    return sp, out, c, div


# astrobeeSE3, ladder, problem 9 of the 16: five shrinks, then TrustRegionViolated on every trip, omega x 5 each, until a
# factorisation of the interior point method meets a pivot that is not positive and the run ends SubproblemFailed -- in the
# oracle's run at trip 17 (omega = 4.9e7), on the device two trips later (1.2e9), every entry before that identical.  Which trip
# it is is decided by rounding: on the ORACLE alone, a relative perturbation of 1e-14 of x_init moves the end from trip 17 to 18
# in 1 of 8 draws (1e-12: 1 of 8; 1e-13, 1e-10: 0 of 8).  _scp_parity counts such a run and compares it up to its first difference.
LADDER_ARGS = {SE3: dict(max_diverged=1)}


@pytest.mark.parametrize("model,dec", [pytest.param(m, d, id=f"{T.NAME[m]}-{DEC_NAME[d]}") for m in SC.MODELS for d in RUN_DECS[m]])
def test_whole_runs_ladder(model, dec, monkeypatch):
    _decomposition(monkeypatch, dec)
    sp, out, c, div = _whole("ladder", model, **LADDER_ARGS.get(model, {}))
    assert c["shrink"] >= 3, c
    if model in (FF, SE3):
        assert c["grow"] >= 3 and c["grow_capped"] >= 1, c


@pytest.mark.parametrize("model,omega_max,dec", [pytest.param(m, w, d, id=f"{T.NAME[m]}-{w:g}-{DEC_NAME[d]}") for m in SC.MODELS
                                                 for w in ((0.1,) if m == FF else (0.1, SC.CEILING_LOW)) for d in RUN_DECS[m]])
def test_whole_runs_ceiling(model, omega_max, dec, monkeypatch):
    """GUSTO_STOP_OMEGA_MAX exactly where the oracle stops so, with the history lengths of the oracle's run"""
    _decomposition(monkeypatch, dec)
    sp, out, c, div = _whole("ceiling", model, omega_max)
    st, h = out["st"], out["h"]
    n3 = 0
    for b, r in enumerate(out["oracle"]):
        if b in div:
            continue
        assert (int(st["stop_reason"][b]) == 3) == (r["stop_reason"] == 3), b
        if r["stop_reason"] == 3:
            n3 += 1
            assert r["omega"][-1] > sp.omega_max >= r["omega"][-2], b
            assert (h["n_hist"][b], h["nJ"][b], h["n_rho"][b]) == (len(r["omega"]), len(r["J_true"]), len(r["rho"])), b
            assert h["omega"][b, h["n_hist"][b] - 1] == r["omega"][-1]
    assert n3 >= (2 if omega_max == SC.CEILING_LOW or model == FF else 1), n3


@pytest.mark.parametrize("model,dec", [pytest.param(m, d, id=f"{T.NAME[m]}-{DEC_NAME[d]}") for m in SC.MODELS for d in RUN_DECS[m]])
def test_whole_runs_loose(model, dec, monkeypatch):
    _decomposition(monkeypatch, dec)
    sp, out, c, div = _whole("loose", model)
    st = out["st"]
    n3 = 0
    for b, r in enumerate(out["oracle"]):
        if r["iterations"] == 3 and r["stop_reason"] == 1:
            n3 += 1
            assert int(st["iterations"][b]) == 3 and int(st["stop_reason"][b]) == 1 and st["converged"][b], b
    assert n3 >= (0 if model == DUB else 4), n3           # (dubins_car: test_loose_from_converged_trajectories)


@pytest.mark.parametrize("model", SC.MODELS, ids=lambda m: T.NAME[m])
def test_loose_from_converged_trajectories(model):
    """loose runs started from the converged trajectory of the default run: the first two convergence measures are below the
    threshold already, and `iterations > 2` alone keeps the run going until its third trip -- on every model"""
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = SC.batch(model, SC.FORCED_B)
    runs = SC.restart_runs(model, 16, SC.FORCED_B)
    assert len(runs) >= 4
    bi = np.array([b for b, _, _, _ in runs])
    sp = SC.params("loose", model)
    s = g.BatchSolver(model, 16, len(runs), hist_cap=SC.MAX_ITER + 8, boxes=boxes, spheres=sph, scp_params=_dev(sp))
    s.set_problems(x0[bi], glo[bi], ghi[bi], tf[bi], np.stack([X for _, X, _, _ in runs]), np.stack([U for _, _, U, _ in runs]))
    s.solve(SC.MAX_ITER)
    st, h = s.status(), s.history()
    for i, (b, _, _, q) in enumerate(runs):
        assert q["iterations"] == 3 and q["stop_reason"] == 1
        assert int(st["iterations"][i]) == 3 and int(st["stop_reason"][i]) == 1 and st["converged"][i], b
        assert bool(st["successful"][i]) == q["successful"], b
        cm = h["convergence_measure"][i]
        assert h["n_hist"][i] == 4 and cm[1] + cm[2] <= sp.convergence_threshold, (b, cm[:4])
        assert np.array_equal(h["scp_status"][i, :4], q["scp_status"]) and np.array_equal(h["accept_solution"][i, :4], q["accept"]), b
    print(f"scp_params loose from converged trajectories {T.NAME[model]}: {len(runs)} of {len(runs)} device runs end at iteration 3")


FORCE_ITER = 10


@pytest.mark.parametrize("model", SC.MODELS, ids=lambda m: T.NAME[m])
def test_whole_runs_loose_forced_past_convergence(model):
    """force = 1 against the oracle's solve(max_iter, force=True): a converged run goes on to max_iter with `converged` set"""
    sp, out, c, div = _whole("loose", model, force=True, max_iter=FORCE_ITER)
    st = out["st"]
    past = 0
    for b, r in enumerate(out["oracle"]):
        if b in div:
            continue
        assert bool(st["converged"][b]) == r["converged"] and bool(st["successful"][b]) == r["successful"], b
        if r["converged"] and r["stop_reason"] == 0:
            past += 1
            assert r["iterations"] == FORCE_ITER == int(st["iterations"][b]) and int(st["stop_reason"][b]) == 0, b
    assert past >= 4, past


# ---- the scheduler's level function -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,N", [(FF, 50), (SE3, 16)], ids=["freeflyerSE2", "astrobeeSE3"])
def test_schedule_is_bit_identical_under_ceiling(model, N):
    """the level of a problem is the number of omega raises, counted from omega0 in steps of gamma_fail (csrc/scp.hpp): with
    omega0 = 0.01 and gamma_fail = 4 (and the default omega_max, so that the runs go on) probing, levels and slices still change
    no bit of the results"""
    boxes, sph = T.env(model)
    sp = SC.params("ceiling", model, omega_max=SC.defaults(model).omega_max)
    x0, glo, ghi, tf = SC.batch(model, 48)
    out = []
    for probe in (2, 0):
        s = g.BatchSolver(model, N, 48, hist_cap=SC.MAX_ITER + 8, boxes=boxes, spheres=sph, scp_params=_dev(sp))
        s.set_schedule(probe, 1)
        s.set_problems(x0, glo, ghi, tf)
        s.solve(SC.MAX_ITER)
        out.append((s.traj(), s.status(), s.history()))
        s.close()
    TP._assert_same_runs(out[0], out[1])
    om = out[0][2]["omega"]
    raised = sum(om[b, :n].max() > 1.5 * sp.omega0 for b, n in enumerate(out[0][2]["n_hist"]))
    print(f"scp_params schedule {T.NAME[model]}: {raised} of 48 problems raised omega, iterations {np.bincount(out[0][1]['iterations'])}")
    assert raised >= 8 and (om[:, 0] == sp.omega0).all()


# ---- gusto_set_params(sp, NULL) on a live handle ----------------------------------------------------------------------------
@pytest.mark.parametrize("model,N", [(FF, 50), (MAN, 16)], ids=["freeflyerSE2", "astrobeeSE3manifold"])
def test_set_scp_params_on_a_live_handle(model, N):
    """defaults -> ladder -> ceiling -> defaults on one handle, whole solves of 8 problems: each what a fresh handle returns bit for
    bit, the last the first (a stale copy of the parameters on the device would show), and the sets differ from the defaults"""
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = SC.batch(model)

    def run(s):
        s.set_problems(x0, glo, ghi, tf)
        s.solve(SC.MAX_ITER)
        return s.traj(), s.status(), s.history()

    def fresh(sp):
        s = g.BatchSolver(model, N, 8, hist_cap=SC.MAX_ITER + 8, boxes=boxes, spheres=sph, scp_params=sp)
        r = run(s)
        s.close()
        return r

    sets = [_dev(SC.params(name, model)) for name in ("ladder", "ceiling")]
    s = g.BatchSolver(model, N, 8, hist_cap=SC.MAX_ITER + 8, boxes=boxes, spheres=sph)
    first = run(s)
    live = []
    for sp in sets:
        s.set_params(scp_params=sp)
        live.append(run(s))
    s.set_params(scp_params=g.default_params(model)[0])
    back = run(s)
    s.close()
    TP._assert_same_runs(back, first)
    TP._assert_same_runs(first, fresh(None))
    for sp, r in zip(sets, live):
        TP._assert_same_runs(r, fresh(sp))
        assert not np.array_equal(r[2]["n_hist"], first[2]["n_hist"]) or any(
            not np.array_equal(r[2][k][b, :n], first[2][k][b, :n]) for k in ("Delta", "omega") for b, n in enumerate(first[2]["n_hist"]))
    assert (live[1][2]["omega"][:, 0] == 0.01).all() and (first[2]["omega"][:, 0] == 1.0).all()
