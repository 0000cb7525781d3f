"""CPU proofs for tests/test_gpu_scp_params.py (no GPU): the restatement of the GuSTO verdict table (tests/np_scp_trip.py) against
the oracle's own runs under the non-default SCP parameter sets of tests/scp_param_cases.py; the census conditions that keep those
sets from being vacuous; the margins of the forced states; and the power of the comparison against three wrong tables."""
import pytest

import gusto_oracle as go
import np_scp_trip as NT
import scp_param_cases as SC
import test_kkt_certificate as T

MODELS = pytest.mark.parametrize("model", SC.MODELS, ids=lambda m: T.NAME[m])
FLAGS = ("tr_sat", "cvx_sat", "accept", "scp_status")


def _horizons(model):
    return sorted({16, *SC.HORIZONS[model]})


@MODELS
def test_restatement_reproduces_the_oracle_runs(model):
    """every trip of the ladder, ceiling and loose runs at N = 16, restarted cold from the run's own (Xp, Up, Delta, omega): the
    next history entry -- flags, status, Delta, omega -- exactly, on every trip whose rho (the run's and the cold one) keeps the
    forced states' guard from both thresholds.  The run is warm-started, the restatement cold: a trip inside the guard may differ
    and is counted, at most 2 % per model.  Measured: 0 inside the guard that differ on any model."""
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = SC.batch(model)
    clr = go.default_params(model)[1].clearance
    n_trips = inside = inside_diff = 0
    for name in SC.SETS:
        sp = SC.params(name, model)
        o = go.Oracle(model, 16, boxes=boxes, spheres=sph, scp_params=sp)
        for b, (r, tr) in enumerate(SC.oracle_runs(name, model, 16)):
            o.set_problem(x0[b], glo[b], ghi[b], tf[b])
            assert len(tr) == len(r["Delta"]) - 1
            i_rho = 1                                   # r["rho"][0] the constructor's, [1] ratio(traj, traj); then one per tr_sat trip
            for t, e in enumerate(tr):
                h = t + 1
                c = NT.trip(o, sp, clr, e["Xp"], e["Up"], r["Delta"][t], r["omega"][t])
                assert c["solver_status"] in (1, 2), (name, b, t)
                warm_rho = None
                if r["tr_sat"][h]:
                    i_rho += 1
                    warm_rho = r["rho"][i_rho]
                n_trips += 1
                same = all(c[k] == r[k][h] for k in FLAGS) and c["Delta_next"] == r["Delta"][h] and c["omega_next"] == r["omega"][h]
                guarded = all(SC.margin_ok(x, sp) for x in ([c["rho"]] if c["tr_sat"] else []) + ([warm_rho] if warm_rho is not None else []))
                if not guarded:
                    inside += 1
                    inside_diff += not same
                    continue
                assert same, (name, b, t, {k: (c[k], r[k][h]) for k in FLAGS}, c["Delta_next"], r["Delta"][h], c["omega_next"],
                              r["omega"][h], c["rho"], warm_rho)
            assert i_rho + 1 == len(r["rho"])
    print(f"restatement {T.NAME[model]}: {n_trips} trips, {inside} inside the guard, {inside_diff} of them differ")
    assert n_trips >= 80 and inside <= 0.02 * n_trips, (n_trips, inside)


@MODELS
def test_census_conditions(model):
    """natural runs (ladder, ceiling at both ceilings, loose) and forced states together, at N = 16 and the horizons the GPU tests
    run: enough trips of every branch that the GPU comparison is not vacuous"""
    nat = {name: SC.total(SC.run_census(name, model, N) for N in _horizons(model)) for name in SC.SETS}
    low = SC.total(SC.run_census("ceiling", model, N, omega_max=SC.CEILING_LOW) for N in _horizons(model))
    forced = SC.total(SC.forced_census(model, N) for N in _horizons(model))
    for k, c in list(nat.items()) + [("ceiling_low", low), ("forced", forced)]:
        print(f"census {T.NAME[model]} {k}: {SC.short(c)}")
    both = SC.total([nat["ladder"], nat["ceiling"], nat["loose"], forced])
    for k in ("InaccurateModel", "shrink", "grow", "grow_capped", "TrustRegionViolated"):
        assert both[k] >= 3, (k, both)
    assert both["shrink"] == both["InaccurateModel"]
    assert nat["ceiling"]["stop_OmegaMax"] + low["stop_OmegaMax"] >= 2
    assert max(SC.run_census("ceiling", model, 16)["stop_OmegaMax"],
               SC.run_census("ceiling", model, 16, omega_max=SC.CEILING_LOW)["stop_OmegaMax"]) >= 2
    restart = [q for _, _, _, q in SC.restart_runs(model, 16, SC.FORCED_B)]
    at3 = sum(q["iterations"] == 3 and q["stop_reason"] == 1 for q in restart)
    print(f"census {T.NAME[model]} loose restarted from the converged trajectory: {at3} of {len(restart)} end at iteration 3")
    assert at3 == len(restart)
    assert nat["loose"]["stop_at_3"] + at3 >= 4, (nat["loose"], at3)


def test_loose_runs_end_at_the_iteration_guard():
    """under loose every freeflyerSE2 and astrobeeSE3 run at N = 16 stops at exactly 3 iterations, with the sum of its first two
    convergence measures already below the threshold: `iterations > 2` is what held it"""
    for model in (SC.FF, SC.SE3):
        sp = SC.params("loose", model)
        runs = SC.oracle_runs("loose", model, 16)
        at3 = [r for r, _ in runs if r["iterations"] == 3 and r["stop_reason"] == 1]
        assert len(at3) >= (7 if model == SC.FF else 8), (T.NAME[model], [r["iterations"] for r, _ in runs])
        bound = [r for r in at3 if r["accept"][2] and r["conv"][1] + r["conv"][2] <= sp.convergence_threshold]
        print(f"loose {T.NAME[model]}: {len(at3)} runs end at 3 iterations, {len(bound)} had converged by trip 2")
        assert len(bound) >= 4


@MODELS
def test_forced_states_keep_their_margins(model):
    for N in _horizons(model):
        f = SC.forced(model, N)
        for name in SC.FORCED_SETS:
            sp, pts = f[name]
            nrep, ncand = f["replaced"][name]
            assert nrep <= SC.MAX_REPLACED * ncand, (name, N, nrep, ncand)
            assert len(pts) >= 16
            for p in pts:
                assert p["ref"]["solver_status"] in (1, 2)
                assert SC.margin_ok(p["ref"]["rho"], sp), (name, N, p["b"], p["t"], p["ref"]["rho"], sp.rho0, sp.rho1)
        sp = f["grow"][0]
        assert sp.rho0 == sp.rho1 == SC.defaults(model).rho1
        got = {p["ref"]["Delta_next"] for p in f["grow"][1] if p["ref"]["accept"]}
        assert got == {1.7 * (0.4 * sp.Delta0), sp.Delta0}, got            # 0.68 Delta0 uncapped; 1.36 Delta0 cut to Delta0
        sp = f["split"][0]
        st = [p["ref"] for p in f["split"][1] if p["ref"]["tr_sat"]]
        assert sp.rho0 == sp.rho1 / 4 and sp.rho1 >= SC.SPLIT_RHO1_FLOOR
        assert sum(r["rho"] > sp.rho1 for r in st) >= 3 and sum(r["rho"] < sp.rho0 for r in st) >= 3, N
        assert sum(sp.rho0 <= r["rho"] <= sp.rho1 for r in st) >= 3, N


@MODELS
def test_power_against_wrong_tables(model):
    """rho0 / rho1 swapped, the Delta0 cap removed, beta_fail read for beta_succ: each wrong table disagrees with the right one on
    three or more of the forced trips of every horizon group the GPU tests run, so the GPU comparison would see it"""
    for N in SC.HORIZONS[model]:
        f = SC.forced(model, N)
        for fault in NT.FAULTS:
            n = 0
            for name in SC.FORCED_SETS:
                sp, pts = f[name]
                for p in pts:
                    r = p["ref"]
                    w = NT.verdict(sp, r["Delta"], r["omega"], r["max_d2"], r["rho"], r["cvx_sat"], fault=fault)
                    n += any(w[k] != r[k] for k in ("accept", "scp_status", "Delta_next", "omega_next"))
            print(f"power {T.NAME[model]} N={N} {fault}: {n} trips differ")
            assert n >= 3, (fault, N, n)
