"""The long-horizon cases of the post-solve chain (tests/post_horizon_cases.py) with the numpy restatements alone, no GPU:

  - the conditions the exact comparisons of tests/test_gpu_post_horizons.py rest on: at most 1 % of a case's samples within
    sim_cases.BAND of a decision and every sample finite (gusto_simulate), lincov_cases.decision_gap of at least GAP and the long
    double restatement deciding every index alike (gusto_lincov), status 1 everywhere, the distances of gusto_verify further than
    1e-6 from zero;
  - the restatements' own fp64 error at these horizons, float64 against np.longdouble, each held against the gate the GPU test
    uses by the rule of the file the gate comes from (test_gpu_tvlqr.py and test_gpu_lincov.py: ten times the figure, rounded up
    to a power of ten; test_gpu_simulate.py: a hundred times).  profiles/tvlqr.txt, simulate.txt and lincov.txt hold the figures
    (-s prints them).

gusto_tvlqr: K and P of the float64 recursion against the long double one on the same AB (the Riccati stage): at most 5.8e-15,
which keeps TOL_RICCATI = 1e-13 -- and would, taken alone, keep test_gpu_tvlqr's TOL_END = 1e-13 as well.  The end-to-end row
compares gains that come from two different evaluations of AB, which a same-AB figure does not cover.  So a second figure is
measured for it: the float64 recursion on an AB whose inexact entries are moved by one rounding
(post_horizon_cases.one_rounding; the entries that are exactly 0 or 1 stay) against the long double recursion on the unmoved
AB.  It reaches 8.6e-14 (the Dubins car, N = 256): the end-to-end gate of these horizons is 1e-12, ten times test_gpu_tvlqr's.
gusto_lincov end to end likewise, on the moved AB and the gains that follow from it; its 1e-11 stands."""
import math

import numpy as np
import pytest

import lincov_cases as LC
import np_tvlqr as T
import np_verify as V
import post_horizon_cases as PH
import sim_cases as SC
from test_gpu_lincov import INDEX_FIELDS, KNOT_FIELDS, SUMMARY_FIELDS, TOL_KNOT, TOL_SUMMARY, rel
from test_gpu_lincov import TOL_END as TOL_LINCOV_END
from test_gpu_simulate import TOL as TOL_SIMULATE
from test_gpu_tvlqr import TOL_RICCATI

LD = np.longdouble
SIM_FIELDS = ("sample_min_dist", "x_final", "max_dev", "max_final_dev", "min_dist", "Xcl")   # tools/simulate_errors.py: FIELDS


def gate(figure, factor):
    """`factor` times the figure, rounded up to a power of ten"""
    return 10.0 ** math.ceil(math.log10(factor * figure)) if figure > 0 else 0.0


def test_the_cases_are_the_seams_and_the_long_horizons():
    assert [PH.horizons(m) for m in PH.MODELS] == [(29, 30, 57, 129, 193, 256), (65, 66, 129, 193, 256), (15, 16, 29, 129, 193, 256),
                                                   (14, 15, 27, 129, 193, 256)]
    for model in PH.MODELS:
        assert [N - 1 for N in PH.seams(model)] == [PH.ipb(model), PH.ipb(model) + 1, 2 * PH.ipb(model)]
        assert PH.modes(model, 256) == PH.modes(model, PH.seams(model)[0]) == (PH.MODE_DT, PH.MODE_5)
    assert SC.MODES[PH.MODE_DT] == dict(nstep=0, dt_min=0.2) and SC.MODES[PH.MODE_5] == dict(nstep=5)
    # gusto_interpolate with DT_MIN_UNEVEN: different substep counts in one batch
    assert [V.n_substeps(t, 256, PH.DT_MIN_UNEVEN) for t in PH.DT * 255] == [2, 3]
    # the dynamic LDS of the dense verify kernel on both sides of 64 KiB
    assert PH.verify_lds_bytes(3, 128) == 53248 and PH.verify_lds_bytes(3, 193) == 106496 and PH.verify_lds_bytes(2, 129) == 73728
    assert PH.verify_lds_bytes(0, 256) == 49152 and PH.verify_lds_bytes(2, 256) == 98304      # (6 states: below 64 KiB at every N)


@pytest.mark.parametrize("model,N", PH.CASES)
def test_tvlqr_recursion_against_long_double(model, N):
    Q, R, Qf = SC.WEIGHTS
    worst = dict.fromkeys(("riccati_K", "riccati_P", "end_K", "end_P1"), 0.0)
    for mode in PH.modes(model, N):
        AB, K, P = PH.linearisation(model, N, mode)
        for b in range(PH.B):
            Kl, Pl = PH.riccati(AB[b], Q, R, Qf)
            Km, Pm = T.riccati(PH.one_rounding(AB[b], 7 + b), Q, R, Qf)
            for k, v in (("riccati_K", rel(K[b], Kl)), ("riccati_P", max(rel(P[b, j], Pl[j]) for j in range(N))),
                         ("end_K", rel(Km, Kl)), ("end_P1", rel(Pm[0], Pl[0]))):
                worst[k] = max(worst[k], v)
    print(f"tvlqr model {model} N {N}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert gate(max(worst["riccati_K"], worst["riccati_P"]), 10) <= TOL_RICCATI, worst
    assert gate(max(worst["end_K"], worst["end_P1"]), 10) <= PH.TOL_TVLQR_END, worst


@pytest.mark.parametrize("model,N", PH.CASES)
def test_simulate_conditions_and_float64_against_long_double(model, N):
    worst = dict.fromkeys(SIM_FIELDS, 0.0)
    for mode in PH.modes(model, N):
        lo = PH.simulate_reference(model, N, mode)
        hi = PH.simulate_reference(model, N, mode, dtype=LD)
        und = np.stack([SC.undecided(r) for r in lo])
        assert und.mean() <= 0.01, (model, N, mode, und.sum())
        assert not (np.stack([r["sample_flags"] for r in lo]) & 4).any(), (model, N, mode)
        assert all(np.isfinite(r["Xcl"]).all() for r in lo)
        for b in range(PH.B):
            for k in SIM_FIELDS:
                worst[k] = max(worst[k], rel(lo[b][k], hi[b][k]))
    print(f"simulate model {model} N {N}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert gate(max(worst.values()), 100) <= TOL_SIMULATE, worst


@pytest.mark.parametrize("model,N", PH.CASES)
def test_lincov_conditions_and_float64_against_long_double(model, N):
    Q, R, Qf = SC.WEIGHTS
    X, _, _ = PH.inputs(model, N)
    worst = dict.fromkeys(("knot", "summary", "end_knot", "end_summary"), 0.0)
    for mode in PH.modes(model, N):
        AB, _, _ = PH.linearisation(model, N, mode)
        ABm = np.stack([PH.one_rounding(AB[b], 7 + b) for b in range(PH.B)])
        Km = np.stack([T.riccati(ABm[b], Q, R, Qf)[0] for b in range(PH.B)])
        for st in PH.STARTS:
            ref = PH.lincov_reference(model, N, mode, st)
            ld = PH.lincov_reference(model, N, mode, st, dtype=LD)
            moved = PH.lincov_reference(model, N, mode, st, ABm, Km)
            for b in range(PH.B):
                assert ref[b]["status"] == 1 and ref[b]["fail_knot"] == 0
                assert LC.decision_gap(model, X[b], ref[b], *SC.env(model)) >= LC.GAP, (model, N, mode, st, b)
                for f in INDEX_FIELDS:          # no index rests on rounding
                    assert ref[b][f] == ld[b][f] == moved[b][f], (model, N, mode, st, b, f)
                for fields, k in ((KNOT_FIELDS, "knot"), (SUMMARY_FIELDS, "summary")):
                    for f in fields:
                        worst[k] = max(worst[k], rel(ref[b][f], ld[b][f]))
                        worst["end_" + k] = max(worst["end_" + k], rel(moved[b][f], ld[b][f]))
    print(f"lincov model {model} N {N}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert gate(worst["knot"], 10) <= TOL_KNOT and gate(worst["summary"], 10) <= TOL_SUMMARY, worst
    assert gate(max(worst["end_knot"], worst["end_summary"]), 10) <= TOL_LINCOV_END, worst


@pytest.mark.parametrize("model,N", PH.CASES)
def test_verify_distances_sit_away_from_zero(model, N):
    """no flag of gusto_verify's report can hinge on the last digits of a distance (tests/test_gpu_verify.py compares them exactly)"""
    X, U, tf = PH.inputs(model, N)
    boxes, spheres = SC.env(model)
    for opts in [SC.MODES[mode] for mode in PH.modes(model, N)] + [dict(dt_min=PH.DT_MIN_UNEVEN)]:
        for b in range(PH.B):
            r = V.report(model, X[b], U[b], tf[b], boxes, spheres, **opts)
            assert min(abs(r["min_dist_knots"]), abs(r["min_dist_dense"])) > 1e-6, (model, N, opts, b)
