"""The post-solve stages share one roll-out (csrc/rollout.hpp: the substep count, the RK4 step of the state, the RK4 step of the
state and one tangent column, the distance loop of the robot, the nominal plant scalars).  Moving those statements into one place
changes where they are written, not one value, sum or order of sums: every output of gusto_verify, gusto_interpolate, gusto_tvlqr,
gusto_simulate(_disturbed) and gusto_lincov(_disturbed, _dense) must stay BIT-identical.  The fixtures
tests/golden/postroll_{model}_{case}.npz were recorded on an MI355X from the code before that change (twice, with equal bytes); the
library must reproduce every key byte for byte (tobytes(): NaN, +-inf and the sign of a zero count).

A fixture holds its own inputs ("in_*": X, U, tf, the environment and every option), so the test runs no solve and draws no random
number on the host; the perturbations, plant scalars and noise of the roll-outs are the device's own, from the recorded seed.
Trajectories: the straight line from a start to a goal state (the pairs of tests/np_tvlqr.py) with a small sinusoidal wiggle per
state and problem, unit quaternions for the manifold model, next to the keep-out set of tests/sim_cases.py so that the margins are
finite.  All four models, B = 3, S = 70 samples (two waves, one partial).  The shapes are the smallest at which the shared pieces can
go wrong:
  n3    N = 3, nstep = 1: one substep, the first and the last interval only; knot N of lincov_dense is taken by the last interval's
        wave.  store_knots, store_S
  n6    N = 6, nstep = 0 with dt_min = 0.2 and dt = 0.35, 0.55, 0.9: 2, 3 and 5 substeps, the count taken from tf on the device;
        nfull differs per problem; lincov_dense has two tiles, one partial.  store_knots, store_S
  tile  N = 256 / (n + m) + 2 (30, 66, 16, 15), nstep = 2: the linearise launch spans two tiles.  No store_knots, no store_S
Stages per case, on one handle, every getter array recorded: verify; interpolate (report and dense arrays); tvlqr; simulate
(dense_collision = 1, clipped controls); simulate_disturbed (and the plant scalars); lincov; lincov_disturbed (and Cd, Sxt);
lincov_dense(store_dense = 1) with the report of its own knot pass.  Arrays are recorded in full up to the fixture's own
"in_full_bytes", the largest entry of FULL_BYTES with which the fixture stays under MAX_BYTES; a larger array is recorded as the
SHA-256 of its dtype, shape and bytes (the closed-loop states of store_knots, [B, N, S, n], are alone larger than a fixture may be;
in full the 12/13-state fixtures come to 140 - 154 KB even without them): the comparison is as strict, a failure names such an array
instead of showing the entry.

`python tests/test_gpu_post_rollout.py --record` writes the fixtures from the library in the tree."""
import hashlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODELS = {0: "freeflyer", 1: "dubins", 2: "astrobee", 3: "manifold"}
CASES = ("n3", "n6", "tile")
B, S, SEED = 3, 70, 2024
DT = {"n3": (0.5, 0.58, 0.45), "n6": (0.35, 0.55, 0.9), "tile": (0.5, 0.58, 0.45)}
ROLL = {"n3": dict(nstep=1, dt_min=0.1), "n6": dict(nstep=0, dt_min=0.2), "tile": dict(nstep=2, dt_min=0.1)}
N6_SUBSTEPS = (2, 3, 5)
MAX_BYTES = 116688          # the largest fixture of tests/golden before these (rowstate_astrobee_manifold_n50.npz)
FULL_BYTES = (1 << 20, 65536, 32768, 16384, 8192)   # --record tries these in turn: arrays up to this size are recorded in full


def _fixture(model, case):
    return os.path.join(GOLDEN, f"postroll_{MODELS[model]}_{case}.npz")


def _horizon(model, case):
    import gusto_jl_amd as g
    n, m = g.MODEL_DIMS[model]
    return {"n3": 3, "n6": 6, "tile": 256 // (n + m) + 2}[case]


def _inputs(model, case):
    """what --record writes under "in_*": the trajectories, tf, the environment and the options of every stage"""
    import gusto_jl_amd as g
    import np_tvlqr as T
    import sim_cases as SC
    from lincov_plant_cases import PLANT_REL
    n, m = g.MODEL_DIMS[model]
    N = _horizon(model, case)
    s = np.linspace(0.0, 1.0, N)[None, :, None]
    b = np.arange(B)[:, None, None]
    i, c = np.arange(n)[None, None, :], np.arange(m)[None, None, :]
    X = T._X_A[model] * (1 - s) + T._X_B[model] * s + 0.25 * T._X_AMP[model] * np.sin(2 * np.pi * (1 + 0.37 * i + 0.21 * b) * s + 0.5 * i + b)
    U = 0.6 * T._U_SCALE[model] * np.sin(2 * np.pi * (0.8 + 0.43 * c + 0.17 * b) * s + 0.9 * c + 2 * b)
    if model == 3:
        X[..., 6:10] /= np.linalg.norm(X[..., 6:10], axis=-1, keepdims=True)
    boxes, spheres = SC.env(model)
    lo, hi = SC.bounds(model, 1)
    return dict(X=np.ascontiguousarray(X), U=np.ascontiguousarray(U), tf=np.array(DT[case]) * (N - 1),
                boxes=np.zeros((0, 6)) if boxes is None else boxes, spheres=np.zeros((0, 4)) if spheres is None else spheres,
                nstep=np.int32(ROLL[case]["nstep"]), dt_min=np.float64(ROLL[case]["dt_min"]), weights=np.array(SC.WEIGHTS),
                dx0=SC.dx0(model), du0=SC.du0(model), u_lo=lo, u_hi=hi, du_white=0.02 * T._U_SCALE[model],
                plant_rel=PLANT_REL, dw=0.03 * T._U_SCALE[model], seed=np.int64(SEED), n_samples=np.int32(S),
                store=np.int32(case != "tile"))


def _pack(out, full_bytes):
    """what a fixture holds of the outputs: arrays up to full_bytes as they are, larger ones as the digest of dtype, shape and bytes"""
    packed = {}
    for k, a in out.items():
        if a.nbytes <= full_bytes:
            packed[k] = a
        else:
            h = hashlib.sha256(f"{a.dtype.str}{a.shape}".encode() + a.tobytes())
            packed[k + "__sha256"] = np.frombuffer(h.digest(), dtype=np.uint8)
    return packed


def _run(model, I):
    """every stage on the inputs I (a dict without the "in_" prefix): {key: array}"""
    import gusto_jl_amd as g
    X, U, tf = I["X"], I["U"], I["tf"]
    N = X.shape[1]
    roll = dict(nstep=int(I["nstep"]), dt_min=float(I["dt_min"]))
    store = int(I["store"])
    s = g.BatchSolver(model, N, B, hist_cap=16)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    s.set_env(I["boxes"] if len(I["boxes"]) else None, I["spheres"] if len(I["spheres"]) else None)
    out = {}

    def put(prefix, d):
        for k, v in d.items():
            if v is not None:
                out[prefix + k] = np.ascontiguousarray(v)

    put("verify_", s.verify(X, U, **roll))
    nfull, Xf, Uf = s.interpolate(X, U, **roll)
    put("interp_", dict(s.get_verify(), nfull=nfull, Xfull=Xf, Ufull=Uf))
    Q, R, Qf = I["weights"]
    tv = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **roll), X, U)
    put("tvlqr_", dict(K=tv.K, P=tv.P, AB=tv.AB, status=tv.status, fail_knot=tv.fail_knot))
    so = dict(n_samples=int(I["n_samples"]), seed=int(I["seed"]), dx0=I["dx0"], du0=I["du0"], u_lo=I["u_lo"], u_hi=I["u_hi"],
              dense_collision=1, store_knots=store, **roll)
    dist = dict(plant_rel=I["plant_rel"], dw=I["dw"])
    put("sim_", s.simulate(so, X, U))
    if store:
        put("sim_", dict(knots=s.get_simulate_knots()))
    put("simd_", dict(s.simulate_disturbed(so, dist, X, U), plant=s.get_simulate_plant()))
    if store:
        put("simd_", dict(knots=s.get_simulate_knots()))
    lo = dict(dx0=I["dx0"], du0=I["du0"], du_white=I["du_white"], u_lo=I["u_lo"], u_hi=I["u_hi"], store_S=store)
    put("lincov_", s.lincov(lo, X, U))
    put("lincovd_", s.lincov_disturbed(lo, dist, X, U))
    Cd, Sxt = s.get_lincov_plant()
    put("lincovd_", dict(Cd=Cd, Sxt=Sxt))
    put("dense_", s.lincov_dense(lo, dist, X, U, store_dense=1))
    put("dense_knot_", s.get_lincov())
    Cd, Sxt = s.get_lincov_plant()
    put("dense_knot_", dict(Cd=Cd, Sxt=Sxt))
    s.close()
    return out


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("model", sorted(MODELS))
def test_every_stage_is_bit_identical_to_the_build_before_the_shared_rollout(model, case):
    assert os.path.getsize(_fixture(model, case)) <= MAX_BYTES
    d = np.load(_fixture(model, case))
    I = {k[3:]: d[k] for k in d.files if k.startswith("in_")}
    ref = {k: d[k] for k in d.files if not k.startswith("in_")}
    N = I["X"].shape[1]
    # the fixture is what the docstring says: the shape, the substep counts, live stages with finite margins
    assert I["X"].shape[0] == B and N == _horizon(model, case)
    steps = (ref["interp_nfull"] - 1) // (N - 1)
    assert tuple(steps) == (N6_SUBSTEPS if case == "n6" else (ROLL[case]["nstep"],) * B)
    assert np.array_equal(ref["dense_nfull"], ref["interp_nfull"])
    assert ref["tvlqr_status"].all() and all(ref[p + "status"].all() for p in ("lincov_", "lincovd_", "dense_knot_"))
    assert (ref["sim_n_finite"] == S).all() and (ref["simd_n_finite"] == S).all()
    if model != 1:
        for k in ("verify_min_dist_dense", "sim_min_dist", "simd_min_dist", "lincov_min_z_obs", "lincovd_min_z_obs", "dense_min_z_dense"):
            assert np.isfinite(ref[k]).all(), k
    out = _pack(_run(model, I), int(I["full_bytes"]))
    assert sorted(out) == sorted(ref)
    bad = []
    for k in sorted(out):
        a, r = out[k], ref[k]
        if a.shape != r.shape or a.dtype != r.dtype:
            bad.append((k, a.shape, a.dtype.str, r.shape, r.dtype.str))
        elif a.tobytes() != r.tobytes():   # the first entry whose bytes differ, and how many do
            w = f"u{a.dtype.itemsize}"
            at = np.flatnonzero(a.ravel().view(w) != r.ravel().view(w))
            bad.append((k, f"{len(at)} of {a.size} entries, first at {np.unravel_index(at[0], a.shape)}: {a.ravel()[at[0]]!r} for {r.ravel()[at[0]]!r}"))
    assert not bad, (MODELS[model], case, bad)


if __name__ == "__main__":
    import sys
    root = os.path.dirname(os.path.dirname(GOLDEN))
    for p in (os.path.dirname(GOLDEN), root, os.path.join(root, "oracle")):
        sys.path.insert(0, p)
    if "--record" in sys.argv:
        for model in sorted(MODELS):
            for case in CASES:
                I = _inputs(model, case)
                out = _run(model, I)
                for full in FULL_BYTES:
                    I["full_bytes"] = np.int32(full)
                    np.savez_compressed(_fixture(model, case), **{"in_" + k: v for k, v in I.items()}, **_pack(out, full))
                    if os.path.getsize(_fixture(model, case)) <= MAX_BYTES:
                        break
                print(MODELS[model], case, "N", I["X"].shape[1], "nfull", list(out["interp_nfull"]), "in full up to", int(I["full_bytes"]), "bytes", os.path.getsize(_fixture(model, case)),
                      "sha256", hashlib.sha256(b"".join(out[k].tobytes() for k in sorted(out))).hexdigest()[:16], flush=True)
