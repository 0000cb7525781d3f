"""gusto_simulate, the part that needs no GPU: tests/np_simulate.py, the numpy restatement the GPU tests compare against, is
pinned -- its generator against the published outputs of splitmix64 and against the header the kernel compiles
(csrc/simrng.hpp, through tests/c/simulate_rng.cpp), its roll-out against closed forms and against np_tvlqr.rollout, its flags
against direct constructions -- and the inputs of the GPU tests (tests/sim_cases.py) are shown to sit away from the decisions
the exact comparisons depend on."""
import os
import subprocess

import numpy as np
import pytest

import np_models as M
import np_simulate as NS
import np_tvlqr as T
import sim_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_generator_is_splitmix64():
    """the first outputs of splitmix64 from seed 0 as published with the algorithm; sample 0 is zero; every draw lies in [-w, w);
    a shard that starts at problem 3 draws what problem 3 of the whole batch draws"""
    assert [int(v) for v in NS.splitmix64(0, np.arange(3))] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F]
    for model in SC.MODELS:
        n = NS.MODELS[model].n
        w = np.concatenate([SC.dx0(model), SC.du0(model)])
        p = NS.perturbations(model, 5, 257, SC.dx0(model), SC.du0(model), SC.SEED)
        assert p.shape == (5, 257, len(w)) and not p[:, 0].any()
        assert (p >= -w).all() and (p < w).all() and np.abs(p[:, 1:, :n]).min() > 0
        assert len(np.unique(p[:, 1:])) == p[:, 1:].size                     # (no counter is used twice)
        q = NS.perturbations(model, 2, 257, SC.dx0(model), SC.du0(model), SC.SEED, first_problem=3)
        assert np.array_equal(q, p[3:5])
    assert not np.array_equal(NS.perturbations(0, 1, 4, 1.0, 1.0, 1), NS.perturbations(0, 1, 4, 1.0, 1.0, 2))


def test_generator_header_draws_numpys_bits(tmp_path):
    """csrc/simrng.hpp, the header host and device code both compile, in a host program of its own: the same table to the bit"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "simulate_rng")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gusto.jl_amd", "csrc"), "-x", "hip",
                           os.path.join(ROOT, "tests", "c", "simulate_rng.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    for model, seed, first, B, S in ((0, 0, 0, 2, 3), (3, SC.SEED, 0, 3, 65), (2, 2 ** 64 - 1, 2 ** 40, 2, 5), (1, 12345, 7, 4, 257)):
        w = np.concatenate([SC.dx0(model), SC.du0(model)])
        out = subprocess.check_output([exe, str(seed), str(first), str(B), str(S), str(len(w))] + [repr(float(v)) for v in w]).decode().split()
        assert [int(v, 16) for v in out[:3]] == [int(v) for v in NS.splitmix64(seed, np.arange(3))]
        bits = np.array([int(v, 16) for v in out[3:]], dtype=np.uint64).reshape(B, S, len(w))
        p = NS.perturbations(model, B, S, SC.dx0(model), SC.du0(model), seed, first)
        assert np.array_equal(bits, p.view(np.uint64))


def test_astrobee_se3_columns_are_np_models_f():
    """f_cols of AstrobeeSE3 (sums along the state axis) against np_models' f, column by column"""
    rng = np.random.default_rng(3)
    x, u = rng.uniform(-1, 1, (12, 9)), rng.uniform(-1, 1, (6, 9))
    F = NS.f_cols(2, x, u)
    for j in range(9):
        assert np.abs(F[:, j] - M.AstrobeeSE3.f(x[:, j], u[:, j])).max() < 1e-15
    assert NS.f_cols(2, x.astype(np.longdouble), u.astype(np.longdouble)).dtype == np.longdouble


def test_linear_model_deviation_obeys_the_closed_loop_recursion():
    """freeflyerSE2 is linear, so without clipping the deviation from the free roll-out obeys d_{k+1} = (Ad - Bd K_k) d_k with the
    restatement's own AB and K.  The nominal of smooth_batch is not a trajectory of the model, so the recursion is stated between
    two samples: the difference of a perturbed and the unperturbed sample."""
    model, N = 0, 50
    X, U, tf, (Q, R, Qf) = SC.inputs(model, N)
    for b, mode in ((0, 0), (3, 2)):
        AB, K, _ = T.tvlqr(model, X[b], U[b], tf[b], Q, R, Qf, **SC.MODES[mode])
        P = SC.perturbation(model, 9)[b]
        P[:, 6:] = 0.0                                   # (a control offset is an input of the recursion, not a deviation)
        r = NS.simulate(model, X[b], U[b], K, tf[b], P, **SC.MODES[mode])
        for s in range(1, 9):
            d = r["Xcl"][:, s] - r["Xcl"][:, 0]
            assert np.array_equal(d[0], (X[b, 0] + P[s, :6]) - X[b, 0])
            for k in range(N - 1):
                want = (AB[k, :, :6] - AB[k, :, 6:] @ K[k]) @ d[k]
                assert np.abs(d[k + 1] - want).max() <= 1e-12 * max(1.0, np.abs(d).max()), (b, s, k)
        assert np.array_equal(r["x_final"], r["Xcl"][N - 1])


@pytest.mark.parametrize("model", SC.MODELS)
def test_without_gains_the_rollout_is_the_chained_open_loop_map(model):
    """K = 0, zero perturbation: every interval's end equals np_tvlqr.rollout chained from knot 1 (no restart at the knots)"""
    N = 7
    X, U, tf, _ = SC.inputs(model, N)
    mod = NS.MODELS[model]
    for mode in range(3):
        b = 3
        ns = T.n_substeps(tf[b], N, **{"dt_min": 0.1, **SC.MODES[mode]})
        r = NS.simulate(model, X[b], U[b], np.zeros((N - 1, mod.m, mod.n)), tf[b], np.zeros((2, mod.n + mod.m)), **SC.MODES[mode])
        assert r["nstep"] == ns
        x = X[b, 0].copy()
        for k in range(N - 1):
            assert np.abs(r["Xcl"][k, 0] - x).max() <= 1e-13 * np.abs(x).max()
            x = T.rollout(mod, x, U[b, k], tf[b] / (N - 1), ns)
        assert np.abs(r["x_final"][1] - x).max() <= 1e-13 * np.abs(x).max()
        assert not r["sample_flags"].any() and r["n_free"] == r["n_finite"] == 2


def test_clip_flag_is_set_exactly_where_the_unclipped_control_leaves_the_box():
    """bit 1 against a direct evaluation of the law along the restatement's own closed-loop states"""
    model, N, S = 2, 50, 40
    X, U, tf, _ = SC.inputs(model, N)
    K = SC.gains(model, N, 0)
    lo, hi = SC.bounds(model, 1)
    b = 0
    P = SC.perturbation(model, S)[b]
    r = NS.simulate(model, X[b], U[b], K[b], tf[b], P, lo, hi, nstep=1)
    want = np.zeros(S, bool)
    for s in range(S):
        for k in range(N - 1):
            v = (U[b, k] - K[b, k] @ (r["Xcl"][k, s] - X[b, k])) + P[s, 12:]
            want[s] |= bool(((v < lo) | (v > hi)).any())
    assert np.array_equal((r["sample_flags"] & 2) != 0, want) and 0 < want.sum() < S
    assert r["n_clipped"] == want.sum()
    free = NS.simulate(model, X[b], U[b], K[b], tf[b], P, nstep=1)
    assert not (free["sample_flags"] & 2).any() and np.isinf(free["clip_margin"]).all()


@pytest.mark.parametrize("model", [0, 2, 3])
def test_sphere_on_the_nominal_path_collides_sample_0(model):
    """a sphere centred on sample 0's own path: bit 0, a negative distance, the dense index of the knot; without it, free"""
    N = 9
    X, U, tf, _ = SC.inputs(model, N)
    K = SC.gains(model, N, 1)
    b = 2
    P = SC.perturbation(model, 3)[b]
    clear = NS.simulate(model, X[b], U[b], K[b], tf[b], P, nstep=5)
    assert np.isinf(clear["sample_min_dist"]).all() and clear["worst_sample"] == -1 and clear["n_free"] == 3
    c = np.zeros(3)
    ws = 2 if model == 0 else 3
    c[:ws] = clear["Xcl"][4, 0, :ws]
    for dense in (True, False):
        r = NS.simulate(model, X[b], U[b], K[b], tf[b], P, spheres=[[*c, 0.05]], nstep=5, dense_collision=dense)
        assert r["sample_flags"][0] & 1 and r["sample_dense_index"][0] == 4 * 5
        assert abs(r["sample_min_dist"][0] + 0.05 + NS.MODELS[model].r) < 1e-12
        assert r["n_free"] == 3 - int((r["sample_flags"] & 1).sum()) and r["min_dist"] == r["sample_min_dist"].min()


def test_nonfinite_samples_stop_and_leave_the_report():
    """gains of 1e200: the perturbed samples overflow, are flagged, keep the state they had, and enter no minimum or maximum"""
    model, N, S = 0, 6, 5
    X, U, tf, _ = SC.inputs(model, N)
    P = SC.perturbation(model, S)[0]
    boxes, spheres = SC.env(model)
    r = NS.simulate(model, X[0], U[0], np.full((N - 1, 3, 6), 1e200), tf[0], P, boxes=boxes, spheres=spheres, nstep=1)
    assert ((r["sample_flags"][1:] & 4) != 0).all() and r["n_finite"] == int(((r["sample_flags"] & 4) == 0).sum())
    bad = (r["sample_flags"] & 4) != 0
    assert not np.isfinite(r["x_final"][bad]).all(axis=1).any() and np.array_equal(r["x_final"], r["Xcl"][N - 1], equal_nan=True)
    assert np.isfinite(r["max_dev"]).all() and np.isfinite(r["max_final_dev"]).all() and not np.isnan(r["min_dist"])
    assert r["n_free"] <= r["n_finite"]


def test_gpu_cases_sit_away_from_the_decisions():
    """tests/sim_cases.py with the restatement alone: over every case at most 1 % of the samples have |sample_min_dist| below 1e-9
    or a control entry within 1e-9 of a finite bound where it decides the clip flag; and the cases exercise what they are for --
    collisions and free samples, clipped and unclipped ones, on every model with obstacles / with clipping"""
    seen = {}
    for case in SC.CASES:
        model, N, S, mode, dense, clip, gen = case
        ref = SC.reference(case)
        und = np.stack([SC.undecided(r) for r in ref])
        assert und.mean() <= 0.01, (case, und.sum())
        fl = np.stack([r["sample_flags"] for r in ref])
        assert not (fl & 4).any(), case
        s = seen.setdefault(model, dict(hit=0, free=0, clipped=0, unclipped=0))
        s["hit"] += int((fl & 1).astype(bool).sum()); s["free"] += int(((fl & 1) == 0).sum())
        if clip:
            s["clipped"] += int((fl & 2).astype(bool).sum()); s["unclipped"] += int(((fl & 2) == 0).sum())
    for model, s in seen.items():
        assert s["clipped"] > 0 and s["unclipped"] > 0, (model, s)
        assert model == 1 or (s["hit"] > 0 and s["free"] > 0), (model, s)
    assert {c[3] for c in SC.CASES} == {0, 1, 2} and {c[4:] for c in SC.CASES} >= {(d, c, g) for d in (0, 1) for c in (0, 1) for g in (0, 1)}
