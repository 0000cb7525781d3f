"""gusto_simulate_disturbed, the part that needs no GPU: tests/np_simulate_disturbed.py, the numpy restatement the GPU tests
compare against, is pinned -- its two generator streams against the header the kernel compiles (csrc/simrng.hpp, through
tests/c/simulate_disturbed_rng.cpp), its dynamics and roll-out against np_simulate's at the nominal plant, against closed forms
of the two models that have them, and its actuator noise against the covariance recursion of np_lincov -- and the inputs of the
GPU tests (tests/sim_disturbed_cases.py) are shown to sit away from the decisions the exact comparisons depend on."""
import functools
import os
import subprocess

import numpy as np
import pytest

import np_lincov as NL
import np_simulate as NS
import np_simulate_disturbed as ND
import np_tvlqr as T
import sim_cases as SC
import sim_disturbed_cases as DC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-11          # 100 x 8.6e-14, the largest float64-against-longdouble difference over sim_disturbed_cases
                     # (tools/simulate_errors.py --disturbed; profiles/simulate_disturbed.txt), rounded up to a power of ten
LINCOV_GATE = 5 * np.sqrt(2 / (4096 - 1))   # five standard errors of a variance estimate from S - 1 = 4095 samples: 0.1105


def test_generator_header_draws_numpys_bits(tmp_path):
    """csrc/simrng.hpp in a host program of its own: the stream seeds, the plant table and the noise table to the bit -- a
    shard that starts at problem 3 among them, and seed 2^64 - 1 with first_problem 2^40; sample 0 is exactly nominal / zero;
    the three streams of one seed share no draw among their first 1000"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "simulate_disturbed_rng")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gusto.jl_amd", "csrc"), "-x", "hip",
                           os.path.join(ROOT, "tests", "c", "simulate_disturbed_rng.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    for model, seed, first, B, S, N in ((0, 0, 0, 2, 3, 3), (3, DC.SEED, 0, 3, 65, 4), (2, 2 ** 64 - 1, 2 ** 40, 2, 5, 7),
                                        (1, 12345, 7, 4, 257, 3), (0, DC.SEED, 3, 2, 65, 5)):
        m = NS.MODELS[model].m
        nom = ND.nominal(model, fill=0.37)
        args = [seed, first, B, S, N, m] + [repr(float(v)) for v in np.concatenate([nom, DC.PLANT_REL, DC.dw(model)])]
        out = subprocess.check_output([exe] + [str(a) for a in args]).decode().split()
        assert [int(v, 16) for v in out[:2]] == list(ND.stream_seeds(seed))
        bits = np.array([int(v, 16) for v in out[2:]], dtype=np.uint64)
        th = ND.plants(nom, B, S, DC.PLANT_REL, seed, first)
        w = ND.whites(model, B, N, S, DC.dw(model), seed, first)
        assert np.array_equal(bits[:th.size].reshape(th.shape), th.view(np.uint64))
        assert np.array_equal(bits[th.size:].reshape(w.shape), w.view(np.uint64))
        assert np.array_equal(th[:, 0], np.tile(nom, (B, 1))) and not w[:, :, 0].any()
        if S > 1:
            assert (np.abs(th[:, 1:] / nom - 1) <= DC.PLANT_REL + 1e-15).all() and len(np.unique(th[:, 1:, 0])) == B * (S - 1)
            assert (w >= -DC.dw(model)).all() and (w < DC.dw(model)).all() and len(np.unique(w[:, :, 1:])) == w[:, :, 1:].size
    # a shard with first_problem = its offset draws what the whole batch draws
    assert np.array_equal(ND.plants(ND.nominal(0), 2, 65, DC.PLANT_REL, DC.SEED, 3), ND.plants(ND.nominal(0), 5, 65, DC.PLANT_REL, DC.SEED)[3:])
    assert np.array_equal(ND.whites(0, 2, 5, 65, DC.dw(0), DC.SEED, 3), ND.whites(0, 5, 5, 65, DC.dw(0), DC.SEED)[3:])
    for seed in (0, DC.SEED, 2 ** 64 - 1):
        sp, sw = ND.stream_seeds(seed)
        idx = np.arange(1000)
        draws = np.concatenate([NS.splitmix64(s, idx) for s in (seed, sp, sw)])
        assert len(np.unique(draws)) == 3000


@pytest.mark.parametrize("model", DC.MODELS)
def test_at_the_nominal_plant_f_and_the_rollout_are_np_simulates(model):
    """f_cols with the nominal theta in every column is np_simulate.f_cols to the bit; with zero dispersion and no noise the
    restatement's outputs equal np_simulate.simulate's"""
    rng = np.random.default_rng(5 + model)
    mod = NS.MODELS[model]
    x, u = rng.uniform(-1, 1, (mod.n, 9)), rng.uniform(-1, 1, (mod.m, 9))
    th = np.tile(ND.nominal(model, fill=np.nan)[:, None], (1, 9))
    assert np.array_equal(ND.f_cols(model, x, u, th), NS.f_cols(model, x, u))
    assert ND.f_cols(model, x.astype(np.longdouble), u.astype(np.longdouble), th.astype(np.longdouble)).dtype == np.longdouble
    N, S, b = 7, 9, 1
    X, U, tf, _ = SC.inputs(model, N)
    K = SC.gains(model, N, 1)
    lo, hi = SC.bounds(model, 1)
    boxes, spheres = SC.env(model)
    P = SC.perturbation(model, S)[b]
    want = NS.simulate(model, X[b], U[b], K[b], tf[b], P, lo, hi, boxes, spheres, nstep=5)
    th = ND.plants(ND.nominal(model, fill=np.nan), 1, S, 0.0, DC.SEED)[0]
    got = ND.simulate(model, X[b], U[b], K[b], tf[b], P, th, ND.whites(model, 1, N, S, 0.0, DC.SEED)[0], lo, hi, boxes, spheres, nstep=5)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k


def test_closed_forms_of_the_two_linear_plants():
    """freeflyerSE2 is linear and RK4 integrates it exactly up to rounding: with K = 0, no perturbation and no noise the velocity
    gained times the sample's mass, and the turn rate gained times its inertia, are the impulse of the nominal controls -- the
    same for every sample.  DubinsCar: the heading gained over k_s likewise."""
    N, S, b = 9, 33, 2
    for model, rows, entry in ((0, slice(3, 5), 0), (0, slice(5, 6), 3), (1, slice(2, 3), 5)):
        X, U, tf, _ = SC.inputs(model, N)
        mod = NS.MODELS[model]
        th = ND.plants(ND.nominal(model), 1, S, DC.PLANT_REL, DC.SEED)[0]
        r = ND.simulate(model, X[b], U[b], np.zeros((N - 1, mod.m, mod.n)), tf[b], np.zeros((S, mod.n + mod.m)), th, nstep=5)
        gained = r["Xcl"][N - 1][:, rows] - r["Xcl"][0][:, rows]            # [S, rows]
        q = gained * th[:, entry:entry + 1] if model == 0 else gained / th[:, entry:entry + 1]
        assert np.abs(gained[1:] - gained[0]).max() > 1e-3 * np.abs(gained).max()       # (the plants do differ)
        assert np.abs(q - q[0]).max() <= TOL * np.abs(q).max(), (model, entry)
        dt = tf[b] / (N - 1)
        u_rows = {(0, 0): slice(0, 2), (0, 3): slice(2, 3), (1, 5): slice(0, 1)}[(model, entry)]
        impulse = dt * U[b][:N - 1, u_rows].sum(axis=0)
        assert np.abs(q[0] - impulse).max() <= 1e-12 * np.abs(impulse).max()


@functools.lru_cache(maxsize=None)
def lincov_inputs():
    """the inputs of the roll-outs-against-lincov tests (also the GPU one's): freeflyerSE2, two problems of 8 knots"""
    model, nb, N = 0, 2, 8
    X, U = T.smooth_batch(model, nb, N)
    tf = SC.DT[:nb] * (N - 1)
    return model, N, X, U, tf, 0.5 * T._U_SCALE[model]


def variance_error(Xcl, Sxx):
    """largest relative error, over knots and states, of the sample variance over samples 1 .. S-1 of Xcl [N, S, n] against
    diag Sxx [N, n, n]"""
    var = Xcl[:, 1:].var(axis=1, ddof=1)
    want = np.einsum("kii->ki", Sxx)
    return float(np.abs(var / want - 1).max())


def test_rollouts_with_actuator_noise_have_the_covariance_of_lincov():
    """freeflyerSE2 is exactly linear: the sample variance of every state at every knot over 4095 perturbed roll-outs is diag Sxx_k
    of np_lincov.lincov(du_white = dw / sqrt(3)) within five standard errors -- and far outside them with the noise left out"""
    model, N, X, U, tf, dw = lincov_inputs()
    S = 4096
    Q, R, Qf = SC.WEIGHTS
    P = NS.perturbations(model, len(X), S, SC.dx0(model), SC.du0(model), 2024)
    W = ND.whites(model, len(X), N, S, dw, 2024)
    th = ND.plants(ND.nominal(model), len(X), S, 0.0, 2024)
    for b in range(len(X)):
        AB, K, _ = T.tvlqr(model, X[b], U[b], tf[b], Q, R, Qf, nstep=5)
        cov = NL.lincov(model, X[b], U[b], AB, K, dx0=SC.dx0(model), du0=SC.du0(model), du_white=dw / np.sqrt(3))
        on = ND.simulate(model, X[b], U[b], K, tf[b], P[b], th[b], W[b], nstep=5)
        off = ND.simulate(model, X[b], U[b], K, tf[b], P[b], th[b], None, nstep=5)
        e_on, e_off = variance_error(on["Xcl"], cov["Sxx"]), variance_error(off["Xcl"], cov["Sxx"])
        print(f"problem {b}: variance error with the noise {e_on:.4f}, without {e_off:.4f}, gate {LINCOV_GATE:.4f}")
        assert e_on <= LINCOV_GATE, (b, e_on)
        assert e_off > LINCOV_GATE, (b, e_off)


def test_gpu_cases_sit_away_from_the_decisions():
    """tests/sim_disturbed_cases.py with the restatement alone: in every case at most 1 % of the samples lie within BAND of a
    decision and every sample is finite; collided and free, clipped and unclipped samples occur on every model that has
    obstacles / in the cases that clip; every source of every disturbance meets every model"""
    seen = {}
    for case in DC.CASES:
        model, N, S, mode, dense, clip, gen, psrc, wsrc = case
        ref = DC.reference(case)
        und = np.stack([DC.undecided(r) for r in ref])
        assert und.mean() <= 0.01, (case, und.sum())
        fl = np.stack([r["sample_flags"] for r in ref])
        assert not (fl & 4).any(), case
        assert all(np.isfinite(r["x_final"]).all() and np.isfinite(r["Xcl"]).all() for r in ref), case
        s = seen.setdefault(model, dict(hit=0, free=0, clipped=0, unclipped=0, plant=set(), white=set()))
        s["hit"] += int((fl & 1).astype(bool).sum()); s["free"] += int(((fl & 1) == 0).sum())
        s["plant"].add(psrc); s["white"].add(wsrc)
        if clip:
            s["clipped"] += int((fl & 2).astype(bool).sum()); s["unclipped"] += int(((fl & 2) == 0).sum())
        else:
            assert not (fl & 2).any(), case
    for model, s in seen.items():
        assert s["clipped"] > 0 and s["unclipped"] > 0, (model, s)
        assert model == 1 or (s["hit"] > 0 and s["free"] > 0), (model, s)
        assert s["plant"] == {0, 1, 2} and s["white"] == {0, 1, 2}, (model, s)
    assert {c[3] for c in DC.CASES} == {0, 1, 2} and {c[4] for c in DC.CASES} == {c[5] for c in DC.CASES} == {c[6] for c in DC.CASES} == {0, 1}
    assert {(c[1], c[2]) for c in DC.CASES} == {(3, 1), (3, 64), (3, 65), (3, 257), (50, 65)}
