"""tests/np_lincov_plant.py, the numpy restatement the GPU tests of gusto_lincov_disturbed compare against, pinned without a GPU:
the sensitivities (complex step) against long double central differences, the structure of the augmented recursion and its
reduction to np_lincov, the conditioning of the shared inputs (tests/lincov_plant_cases.py), the closed-loop sensitivity against
np_simulate_disturbed's roll-outs; then the df/dtheta trait of csrc/models.hpp and the argument checks of csrc/post.hpp as
stand-alone host programs (tests/c/plant_sens.cpp, tests/c/lincov_plant_args.cpp), and the declarations."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import lincov_cases as LC
import lincov_plant_cases as PC
import np_lincov as NL
import np_lincov_plant as NP
import np_simulate as NS
import np_simulate_disturbed as NSD
import sim_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gusto_lincov_disturbed", "gusto_get_lincov_plant"]
TOL_SENS = 5.1e-8     # profiles/lincov_plant.txt 1(c): ten times the worst disagreement of the two restatements, 5.09e-9
INDEX_FIELDS = ("status", "fail_knot", "obs_knot", "obs_pair", "ctl_knot", "ctl_entry")


def test_sensitivities_by_complex_step_against_long_double_central_differences():
    """Cd of the restatement (complex step through np_simulate_disturbed.rk4_step) against central differences of the same
    roll-out in np.longdouble with a relative step e = 5e-6; unread columns are zeros.  The bound 1e-9: the truncation of the
    difference is e^2 = 2.5e-11 times a ratio of derivatives of order 1 to 10 (1 / theta: exactly 1); its rounding is
    2^-64 |x| / (e |theta dx/dtheta|) with states of size 3 that a plant scalar moves by as little as 3e-3 per unit of relative
    change: 5e-20 x 1e3 / 5e-6 = 1e-11"""
    LD = np.longdouble
    for model in LC.MODELS:
        N, mode = 4, 2
        X, U, tf, _ = LC.inputs(model, N)
        Cd = PC.sensitivities(model, N, mode)
        assert not Cd[:, :, :, ~NP.read_mask(model)].any()
        th0 = NSD.nominal(model).astype(LD)
        for b in (0, 3):
            ns = NS.n_substeps(tf[b], N, **LC.MODES[mode])
            h = LD(tf[b]) / LD(N - 1) / LD(ns)
            for j in NSD.READS[model]:
                cols = []
                for s in (1, -1):
                    th = th0.copy()
                    th[j] = th0[j] * (1 + LD(s) * LD(5e-6))
                    x = X[b, :N - 1].T.astype(LD)
                    for _ in range(ns):
                        x = NSD.rk4_step(model, x, U[b, :N - 1].T.astype(LD), h, np.repeat(th[:, None], N - 1, axis=1))
                    cols.append((x, th[j]))
                fd = ((cols[0][0] - cols[1][0]) / (cols[0][1] - cols[1][1])).T          # [N-1, n]
                err = np.abs(fd - Cd[b, :, :, j]).max() / np.abs(Cd[b, :, :, j]).max()
                assert err <= 1e-9, (model, b, j, float(err))


@pytest.mark.parametrize("model,N", LC.CASES)
def test_structure_of_the_augmented_recursion_and_conditioning_of_the_inputs(model, N):
    """S_1 = blockdiag(S0, Stheta) with the unread rows of a supplied Sth masked; the [b theta] block constant; Sxx symmetric to
    the bit; unread columns of Cd and Sxt zero; with zero dispersion every field equals np_lincov's; every decision an exactly
    compared index of the GPU tests rests on is further than GAP from flipping, and the long double restatement decides the same"""
    n, m = g.MODEL_DIMS[model]
    nz = n + m
    X, U, _, _ = LC.inputs(model, N)
    unread = ~NP.read_mask(model)
    for mode in range(len(LC.MODES)):
        assert not PC.sensitivities(model, N, mode)[:, :, :, unread].any()
        for e in LC.ENVS:
            sets, _ = LC.env(model, e)
            for st in LC.STARTS:
                ref = PC.reference(model, N, mode, e, st)
                for b, r in enumerate(ref):
                    S0 = NL.default_S0(model, SC.dx0(model), SC.du0(model)) if st == "default" else LC.full_S0(model)[b]
                    Sth = NP.default_Sth(model, PC.PLANT_REL) if st == "default" else NP.masked_Sth(model, PC.full_Sth(model)[b])
                    assert r["status"] == 1 and np.array_equal(r["S"][0, :nz, :nz], S0) and np.array_equal(r["S"][0, nz:, nz:], Sth)
                    assert not r["S"][0, :nz, nz:].any() and not Sth[unread].any() and not Sth[:, unread].any()
                    assert np.all(np.diag(Sth)[~unread] > 0)
                    for k in range(N):
                        S = r["S"][k]
                        assert np.array_equal(S[n:, n:], r["S"][0, n:, n:]) and np.array_equal(S, S.T)
                        assert np.array_equal(S[:n, :n], r["Sxx"][k]) and np.array_equal(S[:n, nz:], r["Sxt"][k])
                        assert not r["Sxt"][k][:, unread].any()
                    assert LC.decision_gap(model, X[b], r, *sets[b]) > LC.GAP, (model, N, mode, e, st, b)
                if e == "sim" or model == 1:
                    for r, rl in zip(ref, PC.reference(model, N, mode, e, st, dtype=np.longdouble)):
                        assert all(r[f] == rl[f] for f in INDEX_FIELDS)
                        for f in ("sigma_x", "sigma_u"):
                            assert np.abs(r[f] - rl[f]).max() <= 1e-12 * np.abs(r[f]).max(), (model, N, mode, e, st, f)
                if (e, st) in (("sim", "default"), ("batch", "full")):
                    zero = PC.reference(model, N, mode, e, st, disturbed=False)
                    plain = LC.reference(model, N, mode, e, st)
                    for z, p in zip(zero, plain):
                        assert all(z[f] == p[f] for f in INDEX_FIELDS + ("min_z_obs", "min_z_ctl", "p_collision_bound"))
                        assert np.array_equal(z["S"][:, :nz, :nz], p["S"]) and not z["S"][:, nz:].any() and not z["S"][:, :, nz:].any()
                        for f in ("Sxx", "sigma_x", "sigma_u", "z_obs", "z_ctl"):
                            assert np.array_equal(z[f], p[f]), f
                    # the dispersion is not lost on the way: it moves the standard deviations
                    assert all(np.abs(r["sigma_x"] - p["sigma_x"]).max() > 1e-6 * np.abs(p["sigma_x"]).max() for r, p in zip(ref, plain))


@pytest.mark.parametrize("model,N,mode", PC.CONSISTENT)
def test_closed_loop_sensitivity_against_the_roll_outs(model, N, mode):
    """roll-out consistent trajectories, S0 = 0, no clipping, no noise: the central difference of np_simulate_disturbed's Xcl over
    the plants theta_nom (1 +- eps e_j) is column j of Sxt_k / Stheta_jj.  Deterministic; the figure goes to
    profiles/lincov_plant.txt (-s prints it)"""
    X, U, tf = PC.consistent_inputs(model, N, mode)
    n, m = g.MODEL_DIMS[model]
    theta = PC.fd_plants(model)
    worst = 0.0
    for b, (AB, K, Cd, Sth, r) in enumerate(PC.consistent_reference(model, N, mode)):
        sim = NSD.simulate(model, X[b], U[b], K, tf[b], np.zeros((len(theta), n + m)), theta, dense_collision=False, **LC.MODES[mode])
        assert np.array_equal(sim["Xcl"][:, 0], X[b])            # the nominal sample tracks X exactly
        assert r["status"] == 1 and not r["Sxx"][0].any()
        worst = max(worst, PC.sens_rel(PC.fd_sensitivity(model, sim["Xcl"], theta), NP.closed_loop_sensitivity(r, Sth), model))
    print("closed-loop sensitivity, model %d N %d mode %d: %.3e" % (model, N, mode, worst))
    assert worst <= TOL_SENS, worst


def _hipcc_host_program(tmp_path, name):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / name)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gusto.jl_amd", "csrc"), "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "c", name + ".cpp"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr + run.stdout
    return json.loads(run.stdout)


def test_df_dtheta_trait_as_a_sanitized_host_program(tmp_path):
    """tests/c/plant_sens.cpp: Dyn<MODEL>::dfdth of every model against central differences of Dyn<MODEL>::f over the plant
    scalar at a handful of points, built with the address and undefined-behaviour sanitizers; entries not read give zeros"""
    rows = _hipcc_host_program(tmp_path, "plant_sens")
    assert sorted({r["model"] for r in rows}) == [0, 1, 2, 3] and len(rows) == 4 * 6
    for r in rows:
        read = r["entry"] in NSD.READS[r["model"]]
        assert r["read"] == int(read) and r["points"] == 5
        if read:
            # central differences with a relative step of 1e-5: truncation 1e-10 |d3f|, rounding 1e-16 / 1e-5
            assert 0 < r["scale"] and r["err"] <= 1e-8 * r["scale"], r
        else:
            assert r["scale"] == 0 and r["err"] == 0, r


def test_argument_checks_as_a_sanitized_host_program(tmp_path):
    """tests/c/lincov_plant_args.cpp: csrc/post.hpp's lincov_plant_args_host (and lincov_args_host under the new call's name) --
    every refusal the header lists that needs no device, with the offending problem and entry in the text, and the accepted edges"""
    out = {r["name"]: (r["rc"], r["err"]) for r in _hipcc_host_program(tmp_path, "lincov_plant_args")}
    accepted = ("zeros", "typical", "plant_rel_just_below_one", "dw_behind_the_model_is_not_read", "Sth_zero", "Sth_diagonal",
                "Sth_garbage_on_unread_entries_freeflyer", "Sth_garbage_on_unread_entries_dubins", "Sth_symmetric_zero_diagonal")
    refused = {"plant_rel_negative": "plant_rel must lie in [0, 1) (entry 0)", "plant_rel_one": "plant_rel must lie in [0, 1) (entry 3)",
               "plant_rel_nan": "plant_rel must lie in [0, 1) (entry 5)", "plant_rel_inf": "plant_rel must lie in [0, 1) (entry 1)",
               "dw_negative": "dw must be finite and >= 0 (entry 1)", "dw_inf": "dw must be finite and >= 0 (entry 2)",
               "dw_nan": "dw must be finite and >= 0 (entry 0)",
               "Sth_nan": "Sth must be finite (problem 2, entry 3, 3)", "Sth_inf": "Sth must be finite (problem 2, entry 0, 3)",
               "Sth_negative_diagonal": "Sth has a negative diagonal entry (problem 1, entry 3, 3)",
               "Sth_not_symmetric_by_one_bit": "Sth must be symmetric to the bit (problem 2, entry 0, 3)",
               "Sth_signed_zero": "Sth must be symmetric to the bit (problem 0, entry 0, 3)",
               "Sth_astrobee_inertia": "Sth must be finite (problem 1, entry 1, 2)",
               "Sth_dubins": "Sth has a negative diagonal entry (problem 0, entry 4, 4)"}
    named = {"lincov_opts_under_the_new_name": "du_white must be finite and >= 0 (entry 1)"}
    assert set(out) == set(accepted) | set(refused) | set(named)
    for name in accepted:
        assert out[name] == (0, ""), name
    for name, text in {**refused, **named}.items():
        assert out[name] == (-1, "gusto_lincov_disturbed: " + text), name


def test_library_declares_and_exports_the_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    jl = open(os.path.join(ROOT, "gusto.jl_amd", "julia", "GuSTOHIPBatch.jl")).read()
    L = g.lib()
    for s in NEW_SYMBOLS:
        assert s in g._capi.SYMBOLS and re.search(r"\bint %s\(" % s, hdr) and hasattr(L, s) and (":" + s) in jl, s
    doc = hdr[hdr.index("gusto_lincov with an uncertain plant"):hdr.index("int gusto_lincov_disturbed(")]
    doc = re.sub(r"\s*\n \*\s*", " ", doc)                   # (the comment's line breaks)
    for phrase in ("No counterpart in the reference", "EXACT derivative", "not a finite difference", "first order", "plant_rel^2",
                   "blockdiag(S0, Stheta)", "(t * t) / 3", "whatever a supplied Sth", "du_white_i^2 + dw_i^2 / 3", "theta terms after them",
                   "GUSTO_ERR_STATE"):
        assert phrase in doc, phrase
    assert "NOT the plant dispersion" not in hdr
    assert L.gusto_lincov_disturbed(None, None, None, None, None, None, None, None) == -1
    assert L.gusto_get_lincov_plant(None, None, None) == -1
    assert C.sizeof(g._capi.DisturbOpts) == (6 + 6) * 8
