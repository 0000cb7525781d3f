"""The v_readlane vector sweeps (csrc/sweeps.hpp: backward_sweep_1w / forward_sweep_1w, their ring of chunk buffers, the range sweeps
of the wave-per-chain kernels in csrc/segw.hpp, and the costate passes) at their chunk and ring boundaries, BIT for bit: the fixtures
tests/golden/sweepring_{case}_n{N}.npz were recorded on an MI355X, twice with equal results, with the library in which every sweep
still spelled its chain step out for itself (the commit before GUSTO_CHAIN_STEP); the library must reproduce them, np.array_equal on
every key.

A wave holds C = 64 / n groups of n lanes, a group per knot: a chunk is C knots, a round of the ring GUSTO_SWEEP_RING = 4 chunks.  The
backward sweep has N - 1 steps, the forward sweep N, so the horizons are those at which a chunk or a ring round can go wrong -- C,
C + 1, C + 2 (one chunk exactly and a step over it in each direction), 4 C, 4 C + 1, 4 C + 2 (the same for a round) -- and N = 64:
  astrobeeSE3, one wave          n = 12, C = 5, ring                       N = 5, 6, 7, 20, 21, 22, 64
  astrobeeSE3manifold, one wave  n = 13, C = 4, ring                       N = 4, 5, 6, 16, 17, 18, 64
  dubins_car                     n = 3, C = 21, no ring (`ok ? load : 0`)  N = 21, 22, 23, 43, 64
  TrajOpt freeflyerSE2           n = 6, C = 10, no ring, Blk by reference  N = 10, 11, 12, 21, 64
  TrajOpt astrobeeSE3            n = 12, ring, Blk by reference            N = 21, 64
  TrajOpt astrobeeSE3manifold    n = 13, ring, Blk by reference            N = 17, 64
  two and four waves per problem (astrobeeSE3, astrobeeSE3manifold): a range sweep per chain, chain c the stages seg_lo(c) ..
  seg_lo(c + 1) - 1 with seg_lo(c) = N c / NCH.  N = NCH L is the horizon at which every chain is L stages long, N = NCH L + 1 the
  one at which the last chain is L + 1 long; L = C and 4 C, without the N > 64 and the N < NCH GUSTO_SEG_MIN_N (= 4 NCH, refused):
    n = 12: two waves N = 10, 11, 40, 41, 64; four waves N = 20, 21, 64
    n = 13: two waves N = 8, 9, 32, 33, 64;   four waves N = 16, 17, 64 (N = 64: every chain 4 C long)
Every case is B = 8 problems in the model's usual environment (gusto_jl_amd.problems), solve(30).

`python tests/test_gpu_sweep_ring.py --record [DIR]` writes the fixtures from the library in the tree (into DIR instead of tests/golden)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KEYS = ("X", "U", "iterations", "ipm_iters", "converged")
B = 8
WAVE, WAVE2, WAVE4 = 1, 3, 4   # gusto_set_decomposition

# case -> (model, TrajOpt?, decomposition or None, horizons)
CASES = {
    "astrobee_w1": ("ASTROBEE_SE3", False, WAVE, (5, 6, 7, 20, 21, 22, 64)),
    "manifold_w1": ("ASTROBEE_SE3_MANIFOLD", False, WAVE, (4, 5, 6, 16, 17, 18, 64)),
    "dubins": ("DUBINS_CAR", False, None, (21, 22, 23, 43, 64)),
    "trajopt_freeflyer": ("FREEFLYER_SE2", True, None, (10, 11, 12, 21, 64)),
    "trajopt_astrobee": ("ASTROBEE_SE3", True, None, (21, 64)),
    "trajopt_manifold": ("ASTROBEE_SE3_MANIFOLD", True, None, (17, 64)),
    "astrobee_w2": ("ASTROBEE_SE3", False, WAVE2, (10, 11, 40, 41, 64)),
    "astrobee_w4": ("ASTROBEE_SE3", False, WAVE4, (20, 21, 64)),
    "manifold_w2": ("ASTROBEE_SE3_MANIFOLD", False, WAVE2, (8, 9, 32, 33, 64)),
    "manifold_w4": ("ASTROBEE_SE3_MANIFOLD", False, WAVE4, (16, 17, 64)),
}
PARAMS = [(c, N) for c, v in CASES.items() for N in v[3]]


def _solve(case, N):
    import gusto_jl_amd as g
    P = g.problems
    name, trajopt, dec, _ = CASES[case]
    model = getattr(g, name)
    if model == g.DUBINS_CAR:
        env, batch = {}, P.dubins_batch(B)
    elif model == g.FREEFLYER_SE2:
        env, batch = dict(boxes=P.freeflyer_env()), P.freeflyer_batch(B)
    else:
        boxes, sph = P.iss_corner_env(True)
        env = dict(boxes=boxes, spheres=sph)
        batch = P.astrobee_se3_batch(B) if model == g.ASTROBEE_SE3 else P.astrobee_manifold_batch(B)
    s = g.TrajOptSolver(model, N, B, **env) if trajopt else g.BatchSolver(model, N, B, hist_cap=40, **env)
    if dec is not None:
        s.set_decomposition(dec)
    s.set_problems(*batch)
    s.solve(30)
    X, U = s.traj()
    st = s.status()
    s.close()
    return dict(X=X, U=U, iterations=st["iterations"], ipm_iters=st["ipm_iters"], converged=st["converged"])


@pytest.mark.parametrize("case,N", PARAMS, ids=[f"{c}-{N}" for c, N in PARAMS])
def test_solve_is_bit_identical_to_the_recorded_sweeps(case, N):
    d = np.load(os.path.join(GOLDEN, f"sweepring_{case}_n{N}.npz"))
    assert d["ipm_iters"].min() >= 1   # (the fixture holds real solves: every problem ran the sweeps)
    out = _solve(case, N)
    for k in KEYS:
        assert out[k].shape == d[k].shape and np.array_equal(out[k], d[k]), (case, N, k)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(GOLDEN))
    sys.path.insert(0, os.path.dirname(os.path.dirname(GOLDEN)))
    if "--record" in sys.argv:
        at = sys.argv.index("--record")
        out_dir = sys.argv[at + 1] if len(sys.argv) > at + 1 else GOLDEN
        os.makedirs(out_dir, exist_ok=True)
        for case, N in PARAMS:
            out = _solve(case, N)
            np.savez_compressed(os.path.join(out_dir, f"sweepring_{case}_n{N}.npz"), **{k: out[k] for k in KEYS})
            print(case, N, "trips", int(out["iterations"].sum()), "kkt", int(out["ipm_iters"].sum()), "min kkt", int(out["ipm_iters"].min()),
                  "converged", int(out["converged"].sum()), "/", len(out["converged"]), "finite", bool(np.isfinite(out["X"]).all()), flush=True)
