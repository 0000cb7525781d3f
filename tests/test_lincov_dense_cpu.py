"""tests/np_lincov_dense.py, the numpy restatement the GPU tests of gusto_lincov_dense compare against, pinned without a GPU: float64
against np.longdouble, the sensitivities inside an interval (complex step) against long double central differences, the
second-moment identity on freeflyerSE2's linear closed loop, continuity with the knot recursion at i = Nstep, the conditioning of
the shared inputs (tests/lincov_dense_cases.py), the corner-cut case; then the argument checks of csrc/post.hpp as a stand-alone
host program (tests/c/lincov_dense_args.cpp) and the declarations."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gusto_jl_amd as g
import lincov_cases as LC
import lincov_dense_cases as DC
import lincov_plant_cases as PC
import np_lincov_dense as ND
import np_lincov_plant as NP
import np_simulate as NS
import np_simulate_disturbed as NSD
import sim_cases as SC
from test_lincov_plant_cpu import _hipcc_host_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gusto_lincov_dense", "gusto_get_lincov_dense"]
COMBOS = (("sim", "default"), ("batch", "full"), ("empty", "default"))


def _rel(a, ref):
    fin = np.isfinite(np.asarray(ref, dtype=np.longdouble))
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    assert np.array_equal(a[~fin], ref[~fin])
    return float(np.abs(a[fin] - ref[fin]).max() / np.abs(ref[fin]).max()) if fin.any() else 0.0


@pytest.mark.parametrize("model", LC.MODELS)
def test_float64_against_long_double(model):
    """every dense array of the restatement in float64 against np.longdouble, both behind their own knot pass on the same AB, K,
    Cd; the indices agree exactly.  1e-11: the knot pass's own bound (tests/test_lincov_plant_cpu.py holds sigma_x to 1e-12
    there), with the one more product Gp S Gp' and the margin's square root on top; tools/lincov_dense_errors.py prints the figures"""
    for N, mode in ((4, 2), (50, 1)):
        for e, st in COMBOS[:2]:
            d = DC.dense_reference(model, N, mode, e, st)
            q = DC.dense_reference(model, N, mode, e, st, dtype=np.longdouble)
            for a, b in zip(d, q):
                assert a["nfull"] == b["nfull"] and a["dense_sample"] == b["dense_sample"] and a["dense_pair"] == b["dense_pair"]
                assert np.array_equal(a["pair_dense"], b["pair_dense"])
                for f in ("z_dense", "Spos", "min_z_dense"):
                    assert _rel(a[f], b[f]) <= 1e-11, (model, N, mode, e, st, f, _rel(a[f], b[f]))


def test_interval_sensitivities_by_complex_step_against_long_double_central_differences():
    """Phi, Gamma, C of every sample of every interval (complex step) against central differences of the same roll-out in
    np.longdouble with a step e = 2e-6 (relative for the plant scalars); at i = 0 they are I, 0, 0 exactly.  The bound 1e-9: the
    truncation is e^2 = 4e-12 times a ratio of derivatives of order 1 to 10, the rounding 2^-64 |x| / e = 5e-20 x 40 / 2e-6 = 1e-12"""
    LD = np.longdouble
    e = LD(2e-6)
    for model in LC.MODELS:
        N, mode = 4, 2
        X, U, tf, _ = LC.inputs(model, N)
        n, m = g.MODEL_DIMS[model]
        for b in (0, 3):
            ns, xbar, Phi, Gam, Cc = ND.interval_maps(model, X[b], U[b], tf[b], **LC.MODES[mode])
            assert ns == NS.n_substeps(tf[b], N, **LC.MODES[mode]) and np.array_equal(xbar[:, 0], X[b, :N - 1])
            assert np.array_equal(Phi[:, 0], np.broadcast_to(np.eye(n), (N - 1, n, n))) and not Gam[:, 0].any() and not Cc[:, 0].any()
            assert not Cc[:, :, :, ~NP.read_mask(model)].any()
            h = LD(tf[b]) / LD(N - 1) / LD(ns)
            th0 = NSD.nominal(model).astype(LD)

            def roll(dx, du, dth):
                x = X[b, :N - 1].T.astype(LD) + dx[:, None]
                u = U[b, :N - 1].T.astype(LD) + du[:, None]
                th = np.repeat((th0 + dth)[:, None], N - 1, axis=1)
                out = [x]
                for _ in range(ns):
                    x = NSD.rk4_step(model, x, u, h, th)
                    out.append(x)
                return np.array(out)                      # [ns+1, n, N-1]

            def fd(kind, j, step):
                d = [np.zeros(n, LD), np.zeros(m, LD), np.zeros(6, LD)]
                d[kind][j] = step
                hi = roll(*d)
                d[kind][j] = -step
                lo = roll(*d)
                return ((hi - lo) / (2 * step)).transpose(2, 0, 1)      # [N-1, ns+1, n]

            for kind, M, cols in ((0, Phi, range(n)), (1, Gam, range(m)), (2, Cc, NSD.READS[model])):
                for j in cols:
                    ref = fd(kind, j, e * (th0[j] if kind == 2 else LD(1)))
                    err = np.abs(ref - M[:, :, :, j]).max() / max(np.abs(M[:, :, :, j]).max(), 1e-300)
                    assert err <= 1e-9, (model, b, kind, j, float(err))


def test_second_moment_identity_on_the_linear_closed_loop():
    """freeflyerSE2 is linear in state and control: closed-loop roll-outs x(t) of the law with the nominal plant, from perturbed
    starts, with a constant offset b and a noise w_k per interval, deviate from the nominal points by exactly G_{k,i} z_k +
    Gamma_{k,i} w_k, so the second moment of the position deviations at a dense sample is [Gp Gammap] M [Gp Gammap]' for the
    sample second moment M of [z_k; w_k] -- no statistics, rounding only.  1e-10: 49 intervals of a contracting loop in float64"""
    model, N, mode, S = 0, 50, 1, 24
    n, m = g.MODEL_DIMS[model]
    ws = 2
    X, U, tf, _ = LC.inputs(model, N)
    _, K = LC.linearisation(model, N, mode)
    rng = np.random.default_rng(5)
    th = np.repeat(NSD.nominal(model)[:, None], S, axis=1)
    for b in (1, 4):
        ns, xbar, Phi, Gam, Cc = ND.interval_maps(model, X[b], U[b], tf[b], **LC.MODES[mode])
        h = tf[b] / (N - 1) / ns
        x = X[b, 0][:, None] + SC.dx0(model)[:, None] * rng.uniform(-1, 1, (n, S))
        off = SC.du0(model)[:, None] * rng.uniform(-1, 1, (m, S))
        worst = 0.0
        for k in range(N - 1):
            w = PC.dw(model)[:, None] * rng.uniform(-1, 1, (m, S))
            dxk = x - X[b, k][:, None]
            u = U[b, k][:, None] - K[b, k] @ dxk + off + w
            z = np.vstack([dxk, off, np.zeros((6, S))])
            M = np.vstack([z, w]) @ np.vstack([z, w]).T / S
            for i in range(ns):
                if i:
                    x = NSD.rk4_step(model, x, u, h, th)
                    G = ND.closed_loop_map(Phi[k, i], Gam[k, i], Cc[k, i], K[b, k])
                    L = np.hstack([G[:ws], Gam[k, i][:ws]])
                    dev = x[:ws] - xbar[k, i][:ws, None]
                    worst = max(worst, np.abs(dev @ dev.T / S - L @ M @ L.T).max() / np.abs(dev @ dev.T / S).max())
            x = NSD.rk4_step(model, x, u, h, th)
        assert worst <= 1e-10, (b, worst)


@pytest.mark.parametrize("model", LC.MODELS)
def test_continuity_with_the_knot_recursion(model):
    """the dense formula on all n rows at i = Nstep is the recursion's Sxx_{k+1}: G_{k,Nstep} = [Ad - Bd K | Bd | Cd].  Both are
    complex steps through the same roll-out, taken by two routes (one composite step, or Phi, Gamma apart and the product with K
    after): 1e-11 relative to the largest entry, the size of tests/test_gpu_lincov.py's TOL_END"""
    n, m = g.MODEL_DIMS[model]
    for N, mode in ((4, 2), (50, 1)):
        X, U, tf, _ = LC.inputs(model, N)
        _, K = LC.linearisation(model, N, mode)
        knot = PC.reference(model, N, mode, "empty", "full")
        w2 = LC.du_white(model, N, mode) ** 2 + PC.dw(model) ** 2 / 3.0
        for b in range(LC.B):
            ns, _, Phi, Gam, Cc = ND.interval_maps(model, X[b], U[b], tf[b], **LC.MODES[mode])
            for k in range(N - 1):
                G = ND.closed_loop_map(Phi[k, ns], Gam[k, ns], Cc[k, ns], K[b, k])
                Sn = ND.position_covariance(G, knot[b]["S"][k], w2, n, m, n)
                ref = knot[b]["Sxx"][k + 1]
                assert np.abs(Sn - ref).max() <= 1e-11 * np.abs(ref).max(), (model, N, b, k)


@pytest.mark.parametrize("model,N", LC.CASES)
def test_structure_and_conditioning_of_the_inputs(model, N):
    """z_dense and pair_dense at every i = 0 sample and at knot N are the knot pass's z_obs and pair, Spos there its Sxx block;
    min_z_dense <= min_z_obs; with nstep = 1 the dense summary IS the knot summary; DubinsCar and the empty set give +inf, -1;
    every exactly compared index (pair_dense, dense_sample, dense_pair) is further than GAP from flipping"""
    ws = 2 if model < 2 else 3
    for mode in range(len(LC.MODES)):
        for e, st in COMBOS:
            sets, _ = LC.env(model, e)
            knot = PC.reference(model, N, mode, e, st)
            dense = DC.dense_reference(model, N, mode, e, st)
            for b, (r, d) in enumerate(zip(knot, dense)):
                ns = (d["nfull"] - 1) // (N - 1)
                at = np.arange(N) * ns
                assert np.array_equal(d["z_dense"][at], r["z_obs"]) and np.array_equal(d["Spos"][at], r["Sxx"][:, :ws, :ws])
                assert np.array_equal(d["Spos"], np.swapaxes(d["Spos"], 1, 2))
                assert [d["pair_dense"][j] for j in at] == [NP.NL._first_min(zp)[1] for zp in r["z_pairs"]]
                assert d["min_z_dense"] <= r["min_z_obs"]
                if ns == 1:
                    assert d["min_z_dense"] == r["min_z_obs"] and d["dense_sample"] == r["obs_knot"] - 1 and d["dense_pair"] == r["obs_pair"]
                if model == 1 or e == "empty" or (sets[b][0] is None and sets[b][1] is None):
                    assert np.all(d["z_dense"] == np.inf) and np.all(d["pair_dense"] == -1)
                    assert d["min_z_dense"] == np.inf and d["dense_sample"] == -1 and d["dense_pair"] == -1
                assert DC.dense_gap(model, d, *sets[b]) > DC.GAP, (model, N, mode, e, st, b, DC.dense_gap(model, d, *sets[b]))


def test_corner_cut_case():
    """the hand-built case: the knots see the sphere from 0.9 away, the samples in the middle of interval 2 pass it closely.
    The restatement gives min_z_dense below a third of min_z_obs, at a sample inside the interval, with the runner-up sample and
    the runner-up pair of that sample more than 1 (standard deviation) away: nothing an fp64 kernel could flip"""
    knot, d = DC.corner_reference()
    _, dl = DC.corner_reference(np.longdouble)
    ns = 5
    assert knot["status"] == 1 and d["nfull"] == 3 * ns + 1
    assert d["min_z_dense"] < knot["min_z_obs"] / 3 and d["dense_sample"] % ns != 0
    assert (d["dense_sample"], d["dense_pair"]) == (dl["dense_sample"], dl["dense_pair"]) == (7, 1)
    z = np.sort(d["z_dense"])
    assert z[1] - z[0] > 1.0
    zp = np.sort(d["z_pairs"][d["dense_sample"]])
    assert zp[1] - zp[0] > 1.0
    _, _, _, spheres = DC.corner_inputs()
    assert DC.dense_gap(0, d, None, spheres) > DC.GAP


def test_argument_checks_as_a_sanitized_host_program(tmp_path):
    """tests/c/lincov_dense_args.cpp: csrc/post.hpp's lincov_dense_args_host, and the checks of gusto_lincov and
    gusto_lincov_disturbed under the new call's name, built with the address and undefined-behaviour sanitizers"""
    out = {r["name"]: (r["rc"], r["err"]) for r in _hipcc_host_program(tmp_path, "lincov_dense_args")}
    accepted = ("store_dense_0", "store_dense_1", "dispersion_typical", "Sth_diagonal")
    refused = {"store_dense_2": "store_dense must be 0 or 1", "store_dense_minus_1": "store_dense must be 0 or 1",
               "store_dense_large": "store_dense must be 0 or 1",
               "plant_rel_one": "plant_rel must lie in [0, 1) (entry 3)", "dw_nan": "dw must be finite and >= 0 (entry 0)",
               "Sth_not_symmetric": "Sth must be symmetric to the bit (problem 2, entry 0, 3)",
               "Sth_nan_last_entry": "Sth must be finite (problem 2, entry 3, 3)",
               "du_white_negative": "du_white must be finite and >= 0 (entry 1)", "store_S_2": "store_S must be 0 or 1",
               "S0_negative_diagonal": "S0 has a negative diagonal entry (problem 2, entry 8, 8)"}
    assert set(out) == set(accepted) | set(refused)
    for name in accepted:
        assert out[name] == (0, ""), name
    for name, text in refused.items():
        assert out[name] == (-1, "gusto_lincov_dense: " + text), name


def test_library_declares_and_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    jl = open(os.path.join(ROOT, "gusto.jl_amd", "julia", "GuSTOHIPBatch.jl")).read()
    L = g.lib()
    for s in NEW_SYMBOLS:
        assert s in g._capi.SYMBOLS and re.search(r"\bint %s\(" % s, hdr) and hasattr(L, s) and (":" + s) in jl, s
    doc = hdr[hdr.index("gusto_lincov_disturbed with the obstacle margins at the dense samples"):hdr.index("int gusto_lincov_dense(")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)
    for phrase in ("No counterpart in the reference", "EXACT derivative", "no finite differences", "restarted at its knot",
                   "Gp S_k Gp' + Gammap diag(sw2) Gammap'", "BY DEFINITION", "NO Boole bound", "GUSTO_ERR_STATE", "under any mask"):
        assert phrase in doc, phrase
    assert L.gusto_lincov_dense(None, None, None, None, None, None, None, None, 1) == -1
    assert L.gusto_get_lincov_dense(None, None, None) == -1
    assert C.sizeof(g._capi.LincovDenseReport) == 7 * 8
    assert hasattr(g._capi.BatchSolver, "lincov_dense") and hasattr(g.host, "lincov_dense")
