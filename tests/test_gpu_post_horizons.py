"""The post-solve chain -- gusto_verify / gusto_interpolate, gusto_tvlqr, gusto_simulate, gusto_lincov -- at the horizons the
other files stop short of (tests/post_horizon_cases.py): the tile seams of tvlqr_linearise (N - 1 = IPB, IPB + 1, 2 IPB) and
N = 129, 193, 256 on every model, where the dense verify kernel asks for up to 106 496 bytes of dynamic LDS (above 64 KiB from
N = 129 on for the 12/13-state models) and the one-wave recursions and the per-knot LDS refresh of simulate_kernel run up to 255
knots in sequence.  B = 2 problems of different tf on one handle per (model, N).

Every comparison is the one of the stage's own test file, with its functions and constants: test_gpu_verify._compare,
the four rows of test_gpu_tvlqr.py, test_gpu_simulate.test_against_the_restatement, test_gpu_lincov.compare.  No tolerance comes
from the device: tests/test_post_horizons_cpu.py measures the restatements' own fp64 error at these horizons and holds each
constant against it by its file's rule.  All stand but one: K and P_1 of gusto_tvlqr against the restatement's own AB
(post_horizon_cases.TOL_TVLQR_END, 1e-12; the reasoning is in tests/test_post_horizons_cpu.py).  TOL_AB and TOL_IDENTITY are
per-interval quantities: the intervals here have the dt and the substep counts of test_gpu_tvlqr.py's, whatever their number.
The worst error per stage, model and N is printed (-s); profiles/tvlqr.txt, simulate.txt and lincov.txt hold the values of a run."""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import np_simulate as NS
import np_tvlqr as T
import post_horizon_cases as PH
import sim_cases as SC
import test_gpu_lincov as GL
import test_gpu_simulate as GS
import test_gpu_tvlqr as GT
import test_gpu_verify as GV

pytestmark = pytest.mark.gpu

CASES = [pytest.param(model, N, id=f"m{model}-N{N}") for model, N in PH.CASES]


@functools.lru_cache(maxsize=None)
def device(model, N):
    """one handle, the whole chain per roll-out mode (computed once per case, shared, never written to): {mode: dict}, under
    "uneven" the dense pass whose two problems need different substep counts, at the seams "both" and "alone" (test_tvlqr)"""
    X, U, tf = PH.inputs(model, N)
    boxes, spheres = SC.env(model)
    s = g.BatchSolver(model, N, PH.B, hist_cap=16, boxes=boxes, spheres=spheres)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    out = {}
    for mode in PH.modes(model, N):
        r = {}
        r["dense"] = s.interpolate(X, U, dense_collision=1, **SC.MODES[mode])     # (GUSTO_OK, or _chk raises)
        r["report"] = s.get_verify()
        r["plain"] = s.verify(X, U, dense_collision=1, **SC.MODES[mode])
        r["tvlqr"] = s.tvlqr(PH.tvlqr_options(mode, store_P=1), X, U)
        r["simulate"] = s.simulate(PH.simulate_options(model, mode, store_knots=1), X, U)
        r["Xcl"] = s.get_simulate_knots()
        r["lincov"] = {st: s.lincov(PH.lincov_options(model, N, mode, store_S=1), X, U, S0=PH.start(model, st)) for st in PH.STARTS}
        out[mode] = r
    out["uneven"] = dict(dense=s.interpolate(X, U, dt_min=PH.DT_MIN_UNEVEN), report=s.get_verify())
    if N in PH.seams(model):   # both problems, then problem 0 alone on the same problems: problem 1 keeps every bit it had
        out["both"] = s.tvlqr(PH.tvlqr_options(PH.MODE_DT, store_P=1), X, U)
        s.set_active(np.array([1, 0], bool))
        out["alone"] = s.tvlqr(PH.tvlqr_options(PH.MODE_5, store_P=1), X, U)
        s.set_active(None)
    s.close()
    return out


@pytest.mark.parametrize("model,N", CASES)
def test_verify_and_interpolate(model, N):
    """every field of the report, nfull, Xfull and Ufull with the zeros behind a problem's own rows, under test_gpu_verify's rules"""
    X, U, tf = PH.inputs(model, N)
    env = SC.env(model)
    dev = device(model, N)
    # (gusto_interpolate returned GUSTO_OK, or device() had raised; the size is verify.hip's formula, computed here)
    print(f"verify model {model} N {N}: dynamic LDS of the dense kernel by verify.hip's formula {PH.verify_lds_bytes(model, N)} bytes")
    for mode in PH.modes(model, N):
        r = dev[mode]
        for k in GV.INT_FIELDS + GV.DBL_FIELDS:                # interpolate is verify plus the dense stores
            assert np.array_equal(r["report"][k], r["plain"][k], equal_nan=True), (mode, k)
        assert GV._compare(model, r["report"], X, U, tf, lambda b: env, dense=r["dense"], **SC.MODES[mode]) == 0
    r = dev["uneven"]
    nfull = r["dense"][0]
    assert nfull[0] < nfull[1] == r["dense"][1].shape[1]      # rows of zeros behind problem 0 (asserted in _compare)
    GV._compare(model, r["report"], X, U, tf, lambda b: env, dense=r["dense"], dt_min=PH.DT_MIN_UNEVEN)


@pytest.mark.parametrize("model,N", CASES)
def test_tvlqr(model, N):
    """the four rows of tests/test_gpu_tvlqr.py with store_P = 1: AB against the complex step, K and P on the device's AB, K and
    P_1 end to end, the Riccati identity"""
    n, _ = g.MODEL_DIMS[model]
    Q, R, Qf = SC.WEIGHTS
    worst = dict.fromkeys(("AB", "riccati_K", "riccati_P", "end_K", "end_P1", "identity"), 0.0)
    for mode in PH.modes(model, N):
        AB, K, P = PH.linearisation(model, N, mode)
        r = device(model, N)[mode]["tvlqr"]
        assert r.P.shape == (PH.B, N, n, n) and r.status.all() and not r.fail_knot.any()
        for b in range(PH.B):
            Kd, Pd = T.riccati(r.AB[b], Q, R, Qf)
            assert np.array_equal(r.P[b, N - 1], Qf * np.eye(n))
            worst["AB"] = max(worst["AB"], max(GT._rel(r.AB[b, k], AB[b, k]) for k in range(N - 1)))
            worst["riccati_K"] = max(worst["riccati_K"], GT._rel(r.K[b], Kd))
            worst["riccati_P"] = max(worst["riccati_P"], max(GT._rel(r.P[b, k], Pd[k]) for k in range(N)))
            worst["end_K"] = max(worst["end_K"], GT._rel(r.K[b], K[b]))
            worst["end_P1"] = max(worst["end_P1"], GT._rel(r.P[b, 0], P[b, 0]))
            for k in range(N - 1):
                A, Bd, Pk = r.AB[b, k, :, :n], r.AB[b, k, :, n:], r.P[b, k]
                nrm = np.abs(Pk).max()
                worst["identity"] = max(worst["identity"], np.abs(Pk - (Q * np.eye(n) + A.T @ r.P[b, k + 1] @ (A - Bd @ r.K[b, k]))).max() / nrm)
                assert np.array_equal(Pk, Pk.T), (mode, b, k)
                assert np.linalg.eigvalsh(Pk).min() >= -GT.TOL_IDENTITY * nrm, (mode, b, k)
    print(f"tvlqr model {model} N {N}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    if N in PH.seams(model):
        # the last tile of problem 0 stores its own intervals and nothing behind them: a masked call for problem 0, with another
        # roll-out mode, leaves problem 1's arrays as the unmasked call wrote them -- whatever a store past the tile would hold.
        # (Only N = IPB + 2 has a partial last tile, the other two seams are full tiles; a store past it would show in problem
        # 1's AB alone, since K and P of a masked-out problem are not rewritten.  One horizon per model, which is enough.)
        dev = device(model, N)
        for name in ("K", "P", "AB", "status", "fail_knot"):
            assert np.array_equal(getattr(dev["both"], name), getattr(dev[PH.MODE_DT]["tvlqr"], name)), name
            assert np.array_equal(getattr(dev["alone"], name)[1], getattr(dev["both"], name)[1]), name
            assert np.array_equal(getattr(dev["alone"], name)[0], getattr(dev[PH.MODE_5]["tvlqr"], name)[0]), name
        assert not np.array_equal(dev["alone"].AB[0], dev["both"].AB[0])
    assert worst["AB"] <= GT.TOL_AB, worst
    assert worst["riccati_K"] <= GT.TOL_RICCATI and worst["riccati_P"] <= GT.TOL_RICCATI, worst
    assert worst["end_K"] <= PH.TOL_TVLQR_END and worst["end_P1"] <= PH.TOL_TVLQR_END, worst
    assert worst["identity"] <= GT.TOL_IDENTITY, worst


@pytest.mark.parametrize("model,N", CASES)
def test_simulate(model, N):
    """S = 65 generated perturbations, store_knots, clipping on, as test_gpu_simulate.test_against_the_restatement: the
    perturbations exactly, flags and indices outside the BAND, per-sample arrays and Xcl to TOL, the report as the reduction of the
    device's own arrays"""
    X, _, _ = PH.inputs(model, N)
    n = X.shape[2]
    P = PH.perturbation(model)
    worst = {}
    for mode in PH.modes(model, N):
        d = device(model, N)[mode]
        r, Xcl = d["simulate"], d["Xcl"]
        ref = PH.simulate_reference(model, N, mode, K=d["tvlqr"].K)
        assert np.array_equal(Xcl[:, 0], X[:, None, 0, :] + P[:, :, :n])
        assert np.array_equal(Xcl[:, N - 1], r["x_final"])
        left_out = 0
        for b in range(PH.B):
            q = ref[b]
            ok = ~SC.undecided(q)
            left_out += int((~ok).sum())
            assert np.array_equal(r["sample_flags"][b][ok], q["sample_flags"][ok]), (mode, b)
            assert np.array_equal(r["sample_dense_index"][b][ok], q["sample_dense_index"][ok]), (mode, b)
            if ok.all():
                for k in GS.REPORT_INT:
                    assert r[k][b] == q[k], (mode, b, k, r[k][b], q[k])
            for k in ("sample_min_dist", "x_final", "max_dev", "max_final_dev", "min_dist"):
                worst[k] = max(worst.get(k, 0.0), GS._rel(r[k][b], q[k]))
            worst["Xcl"] = max(worst.get("Xcl", 0.0), GS._rel(Xcl[b], q["Xcl"]))
            own = NS.report(r["sample_min_dist"][b], r["sample_dense_index"][b], r["sample_flags"][b], r["x_final"][b],
                            np.abs(Xcl[b] - X[b][:, None, :]).max(axis=0), X[b, N - 1])
            for k in GS.REPORT_INT:
                assert r[k][b] == own[k], (mode, b, k)
            assert r["min_dist"][b] == own["min_dist"]
            assert np.array_equal(r["max_dev"][b], own["max_dev"]) and np.array_equal(r["max_final_dev"][b], own["max_final_dev"])
            assert np.array_equal((r["sample_flags"][b] & 1) != 0, r["sample_min_dist"][b] < 0)
        assert left_out <= 0.01 * PH.B * PH.S, (mode, left_out)
    print(f"simulate model {model} N {N}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert max(worst.values()) <= GS.TOL, worst


@pytest.mark.parametrize("model,N", CASES)
def test_lincov(model, N):
    """store_S = 1, sim_cases.env, both start covariances: every output through test_gpu_lincov.compare, on the device's AB and K
    and end to end"""
    worst = dict.fromkeys(("knot", "summary", "end"), 0.0)
    rows = []
    for mode in PH.modes(model, N):
        d = device(model, N)[mode]
        tv = d["tvlqr"]
        for st in PH.STARTS:
            out = d["lincov"][st]
            assert np.array_equal(out["Sxx"], np.swapaxes(out["Sxx"], -1, -2))
            ref = PH.lincov_reference(model, N, mode, st, tv.AB, tv.K)
            end = PH.lincov_reference(model, N, mode, st)
            for b in range(PH.B):
                rows.append((out, ref[b], end[b], b, (model, N, mode, st, b)))
                worst["knot"] = max([worst["knot"]] + [GL.rel(out[f][b], ref[b][f]) for f in GL.KNOT_FIELDS])
                worst["summary"] = max([worst["summary"]] + [GL.rel(out[f][b], ref[b][f]) for f in GL.SUMMARY_FIELDS])
                worst["end"] = max([worst["end"]] + [GL.rel(out[f][b], end[b][f]) for f in GL.KNOT_FIELDS + GL.SUMMARY_FIELDS])
    print(f"lincov model {model} N {N}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    for out, ref, end, b, where in rows:
        GL.compare(out, ref, b, GL.TOL_KNOT, GL.TOL_SUMMARY, where)
        GL.compare(out, end, b, GL.TOL_END, GL.TOL_END, where + ("end to end",))
