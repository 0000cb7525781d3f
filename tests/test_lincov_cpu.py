"""tests/np_lincov.py, the numpy restatement the GPU tests of gusto_lincov compare against, pinned without a GPU: the structure of
the recursion, the exact agreement with np_simulate's closed-loop roll-outs on the linear model, margins and summaries against
direct constructions; the conditioning of the shared inputs (tests/lincov_cases.py); then the declarations, the export of the
standard deviations and the argument checks of the library as a sanitized host program."""
import ctypes as C
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

import gusto_jl_amd as g
import lincov_cases as LC
import np_lincov as NL
import np_simulate as NS
import np_tvlqr as T
import sim_cases as SC
from test_gpu_lincov import TOL_SIMULATE, second_moment_start

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gusto_default_lincov_opts", "gusto_lincov", "gusto_get_lincov", "gusto_last_lincov_ms"]


@pytest.mark.parametrize("model,N", LC.CASES)
def test_structure_of_the_recursion_and_conditioning_of_the_inputs(model, N):
    """S_1 = S0, Sbb constant, Sxx symmetric without an eigenvalue below -1e-12 |Sxx|; the default S0 is the explicit diagonal one,
    bit for bit; and every decision an exactly compared index of the GPU tests rests on is further than GAP from flipping"""
    n = g.MODEL_DIMS[model][0]
    X, U, _, _ = LC.inputs(model, N)
    for mode in range(len(LC.MODES)):
        AB, K = LC.linearisation(model, N, mode)
        for e in LC.ENVS:
            sets, _ = LC.env(model, e)
            for st in LC.STARTS:
                ref = LC.reference(model, N, mode, e, st)
                for b, r in enumerate(ref):
                    S0 = NL.default_S0(model, SC.dx0(model), SC.du0(model)) if st == "default" else LC.full_S0(model)[b]
                    assert r["status"] == 1 and np.array_equal(r["S"][0], S0)
                    for k in range(N):
                        Sxx = r["S"][k, :n, :n]
                        assert np.array_equal(r["S"][k, n:, n:], S0[n:, n:]) and np.array_equal(r["S"][k, :n, n:], r["S"][k, n:, :n].T)
                        assert np.array_equal(Sxx, Sxx.T) and np.array_equal(Sxx, r["Sxx"][k])
                        assert np.linalg.eigvalsh(Sxx).min() >= -1e-12 * np.abs(Sxx).max()
                    assert LC.decision_gap(model, X[b], r, *sets[b]) > LC.GAP, (model, N, mode, e, st, b)
                if e == "sim" or model == 1:   # no index rests on rounding: the long double restatement decides the same
                    for r, rl in zip(ref, LC.reference(model, N, mode, e, st, dtype=np.longdouble)):
                        assert all(r[f] == rl[f] for f in ("status", "fail_knot", "obs_knot", "obs_pair", "ctl_knot", "ctl_entry"))
                        for f in ("sigma_x", "sigma_u"):
                            assert np.abs(r[f] - rl[f]).max() <= 1e-12 * np.abs(r[f]).max(), (model, N, mode, e, st, f)
                if st == "default" and e == "empty":
                    lo, hi = LC.bounds(model)
                    for b in range(LC.B):
                        d = NL.lincov(model, X[b], U[b], AB[b], K[b], NL.default_S0(model, SC.dx0(model), SC.du0(model)),
                                      du_white=LC.du_white(model, N, mode), u_lo=lo, u_hi=hi)
                        for f in ("S", "sigma_x", "sigma_u", "z_obs", "z_ctl"):
                            assert np.array_equal(d[f], ref[b][f]), f


def test_second_moment_of_the_closed_loop_roll_outs():
    """freeflyerSE2, unclipped: the sample second moment of np_simulate's Xcl[:, s] - Xcl[:, 0] is the restatement's Sxx for
    S0 = sym(P'P / S), inside the constant the GPU cross-check uses -- the model is linear, no statistics are involved"""
    model, N, mode, S = 0, 50, 2, 257
    X, U, tf, _ = LC.inputs(model, N)
    AB, K = LC.linearisation(model, N, mode)
    P = SC.perturbation(model, S)
    worst = 0.0
    for b in range(LC.B):
        sim = NS.simulate(model, X[b], U[b], K[b], tf[b], P[b], dense_collision=False, **LC.MODES[mode])
        D = sim["Xcl"] - sim["Xcl"][:, :1]
        M = np.einsum("ksi,ksj->kij", D, D) / S
        r = NL.lincov(model, X[b], U[b], AB[b], K[b], second_moment_start(P[b]))
        worst = max(worst, max(np.abs(r["Sxx"][k] - M[k]).max() / np.abs(M[k]).max() for k in range(N)))
    assert worst <= TOL_SIMULATE, worst


def _one(model, x, sphere=None, box=None, S0=None, dx0=0.01, **kw):
    """a two-knot problem at rest at state x with zero gains and identity dynamics: S_2 = S_1"""
    n, m = g.MODEL_DIMS[model]
    X = np.tile(np.asarray(x, float), (2, 1))
    AB = np.hstack([np.eye(n), np.zeros((n, m))])[None]
    return NL.lincov(model, X, np.zeros((2, m)), AB, np.zeros((1, m, n)), S0, dx0, boxes=box, spheres=sphere, **kw)


def test_margins_against_direct_constructions():
    r_robot = NL.MODELS[2].r
    # one sphere at distance 1 along (1, 2, 2) / 3 from an AstrobeeSE3 at the origin, anisotropic position covariance
    x = np.zeros(12)
    S0 = np.zeros((18, 18))
    S0[0, 0], S0[1, 1], S0[2, 2], S0[0, 1], S0[1, 0] = 4e-4, 1e-4, 9e-4, 1e-4, 1e-4
    c = np.array([1.0, 2.0, 2.0]) / 3 * (1.0 + 0.2 + r_robot)
    r = _one(2, x, sphere=[[*c, 0.2]], S0=S0)
    nh = -np.array([1.0, 2.0, 2.0]) / 3
    sd = math.sqrt(nh @ S0[:3, :3] @ nh)
    assert abs(r["z_obs"][0] - 1.0 / sd) <= 1e-12 / sd and r["obs_knot"] == 1 and r["obs_pair"] == 0
    assert abs(r["p_collision_bound"] - min(1.0, 2 * 0.5 * math.erfc(1.0 / sd / math.sqrt(2)))) <= 1e-15
    # one box face: the point 0.5 - r in front of the face x = lo; only the variance along x counts
    box = [[0.5, -1, -1, 1.5, 1, 1]]
    r = _one(2, x, box=box, S0=S0)
    assert abs(r["z_obs"][0] - (0.5 - r_robot) / 0.02) <= 1e-12 and np.array_equal(r["z_obs"], r["z_obs"][:1].repeat(2))
    # p_collision_bound is Boole's sum of erfc tails, capped at 1
    for scale in (1.0, 25.0, 400.0):
        r = _one(2, x, box=box, S0=scale * S0)
        z = (0.5 - r_robot) / (0.02 * math.sqrt(scale))
        want = min(1.0, 2 * 0.5 * math.erfc(z / math.sqrt(2)))
        assert abs(r["p_collision_bound"] - want) <= 1e-13 * want and abs(r["min_z_obs"] - z) <= 1e-12 * z
    inside = _one(2, np.r_[0.6, np.zeros(11)], box=box, S0=S0)          # 0.1 + r behind the face: two tails above 1/2 each
    assert inside["p_collision_bound"] == 1.0 and abs(inside["min_z_obs"] + (0.1 + r_robot) / 0.02) <= 1e-12
    # no deviation of the position: the sign of the distance decides; inside the box it is -inf
    r = _one(2, x, box=box, S0=np.zeros((18, 18)))
    assert np.all(r["z_obs"] == np.inf) and r["obs_knot"] == 0 and r["obs_pair"] == -1 and r["p_collision_bound"] == 0.0
    r = _one(2, np.r_[1.0, 0, 0, np.zeros(9)], box=box, S0=np.zeros((18, 18)))
    assert np.all(r["z_obs"] == -np.inf) and (r["obs_knot"], r["obs_pair"]) == (1, 0) and r["p_collision_bound"] == 1.0
    # dx0 = 0 on the positions of a moving problem: sigma_d = 0 at knot 1 only
    model, N = 0, 4
    X, U, _, _ = LC.inputs(model, N)
    AB, K = LC.linearisation(model, N, 0)
    w = SC.dx0(model).copy()
    w[:2] = 0.0
    bx, sp = SC.env(model)
    r = NL.lincov(model, X[0], U[0], AB[0], K[0], None, w, SC.du0(model), boxes=bx, spheres=sp)
    assert np.all(r["sd_pairs"][0] == 0) and np.isinf(r["z_obs"][0]) and np.all(r["sd_pairs"][1] > 0) and np.isfinite(r["z_obs"][1:]).all()
    # the Dubins car has no keep-out set
    r = _one(1, np.zeros(3), box=[[0.5, -1, -1, 1.5, 1, 1]])
    assert np.all(r["z_obs"] == np.inf) and r["obs_pair"] == -1


def test_ties_go_to_the_lowest_knot_then_the_lowest_ordinal():
    # two identical spheres, two identical knots: pair 0 of knot 1; freeflyerSE2's two components in front of one box face
    x = np.zeros(12)
    r = _one(2, x, sphere=[[1.0, 0, 0, 0.2], [1.0, 0, 0, 0.2], [0.9, 0, 0, 0.2]])
    assert np.array_equal(r["z_pairs"][0][:1], r["z_pairs"][0][1:2]) and (r["obs_knot"], r["obs_pair"]) == (1, 2)
    r = _one(2, x, sphere=[[2.0, 0, 0, 0.2], [1.0, 0, 0, 0.2], [1.0, 0, 0, 0.2]])
    assert (r["obs_knot"], r["obs_pair"]) == (1, 1) and r["z_obs"][0] == r["z_obs"][1]
    r = _one(0, np.zeros(6), box=[[0.5, -1, -1, 1.5, 1, 1]])
    assert r["z_pairs"][0][0] == r["z_pairs"][0][1] and (r["obs_knot"], r["obs_pair"]) == (1, 0)
    # control margins: entry 1 and 2 tie, the first knot wins; an infinite bound gives +inf; sigma_u = 0 is decided by the sign
    n, m = 12, 6
    S0 = np.zeros((18, 18))
    S0[n:, n:] = np.diag([1e-4] * 3 + [0.0] * 3)
    lo, hi = np.array([-1, -0.5, -0.5, -np.inf, -1, 0.1]), np.array([1, 0.5, 0.5, np.inf, 1, 1])
    r = _one(2, x, S0=S0, u_lo=lo, u_hi=hi)
    assert np.array_equal(r["z_ctl"][0], [100.0, 50.0, 50.0, np.inf, np.inf, -np.inf]) and (r["ctl_knot"], r["ctl_entry"]) == (1, 5)
    assert r["min_z_ctl"] == -np.inf
    r = _one(2, x, S0=S0, u_lo=lo[:5].tolist() + [-1.0], u_hi=hi)
    assert (r["ctl_knot"], r["ctl_entry"], r["min_z_ctl"]) == (1, 1, 50.0)
    r = _one(2, x, S0=S0, du_white=[0, 0, 0, 0.01, 0, 0], u_lo=-np.inf, u_hi=np.inf)
    assert np.all(r["z_ctl"] == np.inf) and (r["ctl_knot"], r["ctl_entry"]) == (0, -1) and r["sigma_u"][0, 3] == 0.01


def test_failure_rows_of_the_restatement():
    """a NaN gain at knot 2: status 0, fail_knot 2, rows of knot 1 only, summaries of knot 1"""
    model, N = 0, 4
    X, U, _, _ = LC.inputs(model, N)
    AB, K = LC.linearisation(model, N, 0)
    bx, sp = SC.env(model)
    lo, hi = LC.bounds(model)
    ok = NL.lincov(model, X[1], U[1], AB[1], K[1], None, SC.dx0(model), SC.du0(model), 0.0, lo, hi, bx, sp)
    Kn = K[1].copy()
    Kn[1, 0, 3] = np.nan
    r = NL.lincov(model, X[1], U[1], AB[1], Kn, None, SC.dx0(model), SC.du0(model), 0.0, lo, hi, bx, sp)
    assert (r["status"], r["fail_knot"], r["obs_knot"], r["ctl_knot"]) == (0, 2, 1, 1) and r["min_z_obs"] == ok["z_obs"][0]
    for f in ("sigma_x", "sigma_u", "z_obs", "Sxx"):
        assert np.array_equal(r[f][:1], ok[f][:1]) and not r[f][1:].any(), f


def test_library_declares_and_exports_the_lincov_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    L = g.lib()
    for s in NEW_SYMBOLS:
        assert s in g._capi.SYMBOLS and re.search(r"\bint %s\(" % s, hdr) and hasattr(L, s), s
    doc = hdr[hdr.index("Linear covariance analysis"):hdr.index("} gusto_lincov_opts;")]
    assert "No counterpart in the reference" in doc and "not a" in doc and "probability" in doc and "that call saw" in doc
    for model, (n, m) in g.MODEL_DIMS.items():
        o = g.default_lincov_opts(model)
        assert list(o.dx0) == [0.01] * n + [0.0] * (13 - n) and list(o.du0) == [0.0] * 6 and list(o.du_white) == [0.0] * 6
        assert list(o.u_lo) == [-np.inf] * 6 and list(o.u_hi) == [np.inf] * 6 and o.store_S == 0
    assert L.gusto_default_lincov_opts(9, C.byref(g.LincovOpts())) == -1 and L.gusto_default_lincov_opts(0, None) == -1
    assert L.gusto_lincov(None, None, None, None, None, None) == -1
    assert L.gusto_get_lincov(None, None) == -1 and L.gusto_last_lincov_ms(None, None) == -1
    assert C.sizeof(g.LincovOpts) == (13 + 4 * 6) * 8 + 8 and C.sizeof(g._capi.LincovReport) == 13 * 8
    # the report mirror has the header's fields in the header's order
    end = hdr.index("} gusto_lincov_report;")
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end):end], flags=re.S)
    assert re.findall(r"\*(\w+)", body) == [k for k, _, _ in g._capi.LINCOV_FIELDS]


def test_export_writes_the_standard_deviations_next_to_the_gains(tmp_path):
    """export.write(..., sigma=): traj/sigma_traj [N][x_dim] in all three formats; without it the tree has no such entry"""
    import h5read
    E = g.export
    X, U = T.smooth_batch(0, 2, 6)
    K = np.arange(2 * 5 * 3 * 6, dtype=float).reshape(2, 5, 3, 6)
    sig = np.arange(2 * 6 * 6, dtype=float).reshape(2, 6, 6) / 7
    tf = np.array([10.0, 12.0])
    for ext in (".npz", ".mat"):
        p = str(tmp_path / ("s" + ext))
        E.write(p, 0, X, U, tf, K=K, sigma=sig)
        tree = E.read(p)["traj"]
        assert np.array_equal(tree["sigma_traj"], sig) and np.array_equal(tree["k_traj"], K)
        E.write(p, 0, X, U, tf, K=K)
        assert "sigma_traj" not in E.read(p)["traj"]
    p = str(tmp_path / "s.h5")
    tree = E.write(p, 0, X[0], U[0], 10.0, sigma=sig[0])
    assert np.array_equal(tree["traj"]["sigma_traj"], sig[0]) and "k_traj" not in tree["traj"]
    assert np.array_equal(np.asarray(h5read.read_h5(p)["traj"]["sigma_traj"]).reshape(6, 6), sig[0])
    assert "sigma_traj" not in E.write(p, 0, X[0], U[0], 10.0)["traj"]
    with pytest.raises(ValueError):
        E.write(p, 0, X[0], U[0], 10.0, sigma=sig[0][:5])


def test_argument_checks_as_a_sanitized_host_program(tmp_path):
    """tests/c/lincov_args.cpp: csrc/post.hpp's lincov_args_host, built with the address and undefined-behaviour sanitizers --
    every refusal the header lists, with the offending problem and entry in the text, and the accepted edges"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "lincov_args")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gusto.jl_amd", "csrc"), "-x", "hip", "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "c", "lincov_args.cpp"), "-o", exe],
                          stderr=subprocess.DEVNULL)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and not run.stderr, run.stderr
    out = {r["name"]: (r["rc"], r["err"]) for r in json.loads(run.stdout)}
    accepted = ("defaults", "zero_widths", "infinite_bounds", "entries_behind_the_model_are_not_read", "store_S_1", "S0_zero",
                "S0_diagonal", "S0_symmetric_zero_diagonal")
    refused = {"dx0_negative": "dx0 must be finite and >= 0 (entry 4)", "dx0_inf": "dx0 must be finite and >= 0 (entry 0)",
               "dx0_nan": "dx0 must be finite and >= 0 (entry 5)", "du0_negative": "du0 must be finite and >= 0 (entry 2)",
               "du0_nan": "du0 must be finite and >= 0 (entry 0)", "du_white_negative": "du_white must be finite and >= 0 (entry 1)",
               "du_white_inf": "du_white must be finite and >= 0 (entry 2)", "u_lo_above_u_hi": "u_lo must not exceed u_hi (entry 2)",
               "u_lo_nan": "u_lo must not exceed u_hi (entry 0)", "u_hi_nan": "u_lo must not exceed u_hi (entry 1)",
               "store_S_2": "store_S must be 0 or 1", "store_S_negative": "store_S must be 0 or 1",
               "S0_nan": "S0 must be finite (problem 2, entry 8, 8)", "S0_inf": "S0 must be finite (problem 2, entry 3, 8)",
               "S0_negative_diagonal": "S0 has a negative diagonal entry (problem 1, entry 8, 8)",
               "S0_not_symmetric_by_one_bit": "S0 must be symmetric to the bit (problem 2, entry 7, 8)",
               "S0_signed_zero": "S0 must be symmetric to the bit (problem 0, entry 0, 1)"}
    assert set(out) == set(accepted) | set(refused)
    for name in accepted:
        assert out[name] == (0, ""), name
    for name, text in refused.items():
        assert out[name] == (-1, "gusto_lincov: " + text), name
