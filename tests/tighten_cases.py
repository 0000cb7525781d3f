"""The inputs of the gusto_tighten_env tests, shared by tests/test_tighten_cpu.py (which checks their conditioning with the numpy
restatements alone) and tests/test_gpu_tighten.py.  Built on tests/lincov_cases.py: its trajectories (B = 5 problems), roll-out
modes, environments ("sim", "empty", and "batch" with 0, 1, 31, 33 and 64 components: with freeflyerSE2's two robot components
62, 66 and 128 pairs) and start covariances, on the models with keep-out sets (0, 2, 3) at N = 3, 4 and 50.  The problems are
those of tests/test_gpu_lincov.py's handle: x_init = X[0], a point goal at X[-1].

Option sets: each makes one rule of include/gusto_hip.h decide at least one component of at least one case
(tests/test_tighten_cpu.py asserts that on the restatement): a finite reach that leaves the far components out, a slack that
takes a part of every margin and, with the reach, all of some, a margin_cap below the largest margin, cover off, a kappa large
enough to block a start, kappa = 0, and SECOND: a second call with a smaller kappa after the default one, where monotone = 1
keeps the first call's margins and monotone = 0 does not."""
import numpy as np

import lincov_cases as LC
import np_tighten as NT
import np_verify as V

B = LC.B
MODELS = (0, 2, 3)
HORIZONS = LC.HORIZONS
ENVS = LC.ENVS
STARTS = LC.STARTS
CASES = [(model, N) for model in MODELS for N in HORIZONS]
MODE = 1              # the roll-out mode of lincov_cases the margins are taken in: actuator noise at every horizon
GAP = LC.GAP
KAPPA = 3.0
# name -> the keyword options of one gusto_tighten_env call; the scales are those of the dispersions (dx0 of sim_cases: a
# standard deviation of 1.2 cm at the first knot, millimetres later) and of the distances (the scattered spheres lie 1.5 .. 3 m away)
OPTION_SETS = {
    "default": dict(kappa=KAPPA),
    "reach": dict(kappa=KAPPA, reach=0.5),
    "slack": dict(kappa=KAPPA, slack=0.01),
    "slack_reach": dict(kappa=KAPPA, slack=0.015, reach=0.5),
    "cap": dict(kappa=KAPPA, margin_cap=0.01),
    "nocover": dict(kappa=KAPPA, cover_components=0),
    "big": dict(kappa=40.0),
    "kappa0": dict(kappa=0.0),
}
SECOND = dict(kappa=1.0)      # after "default": monotone = 1 keeps every margin of the first call, monotone = 0 writes kappa = 1's


def problems(model, N):
    """(x_init, goal_lo, goal_hi) [B, n] of the handle the tests build"""
    X, _, _, _ = LC.inputs(model, N)
    return X[:, 0], X[:, -1], X[:, -1]


def base(model, which_env):
    """(boxes_list, spheres_list) as BatchSolver.tighten_env takes them: one entry for a shared set, else B"""
    sets, shared = LC.env(model, which_env)
    sets = sets[:1] if shared else sets
    return [s[0] for s in sets], [s[1] for s in sets]


def reference(model, N, which_env, which_start, Sxx=None, prev=None, skipped=None, dtype=np.float64, **opts):
    """the restatement's results of the five problems (a list of dicts).  Sxx [B, N, n, n]: the covariances to use (the
    device's), default np_lincov's own on lincov_cases' linearisation; prev: a list of previous margins; skipped: a mask"""
    X, _, _, _ = LC.inputs(model, N)
    if Sxx is None:
        Sxx = [r["Sxx"] for r in LC.reference(model, N, MODE, "empty", which_start, dtype=dtype)]
    sets, _ = LC.env(model, which_env)
    x0, glo, ghi = problems(model, N)
    return [NT.tighten(model, X[b], Sxx[b], sets[b][0], sets[b][1], x0[b], glo[b], ghi[b], None if prev is None else prev[b],
                       bool(skipped[b]) if skipped is not None else False, dtype=dtype, **opts) for b in range(B)]


def decision_gap(model, X, ref, boxes, spheres, x_init, goal, **opts):
    """the smallest distance of one problem's result `ref` (np_tighten.tighten) from a decision its exactly compared indices rest
    on: knot and pair as lincov_cases.decision_gap has them, n_grown (kappa sigma_d from slack and d - kappa sigma_d from reach,
    for every pair), blocked (the component-0 distances of x_init and the goal to the tightened set from zero) and the face /
    edge switches of every box"""
    o = dict(NT.DEFAULTS, **opts)
    gap = np.inf
    if ref["status"]:
        zk = np.array([z.min() if len(z) else np.inf for z in ref["z_pairs"]])
        gap = min(gap, LC._two_smallest_gap(zk))
        if ref["knot"]:
            k = ref["knot"] - 1
            zp, dp, sp = ref["z_pairs"][k], ref["d_pairs"][k], ref["sd_pairs"][k]
            same = np.ones(len(zp), bool)
            same[(zp == zp[ref["pair"]]) & (dp == dp[ref["pair"]]) & (sp == sp[ref["pair"]])] = False   # exact ties: the rule decides
            same[ref["pair"]] = True
            gap = min(gap, LC._two_smallest_gap(zp[same]))
        for dp, sp in zip(ref["d_pairs"], ref["sd_pairs"]):
            if len(dp):
                ks = o["kappa"] * sp
                if np.isfinite(o["reach"]):
                    gap = min(gap, np.abs(dp - ks - o["reach"]).min())
                if o["slack"] > 0:
                    gap = min(gap, np.abs(ks - o["slack"]).min())
    ws = V.WS_DIM[model]
    if len(ref["boxes"]) + len(ref["spheres"]):
        for q in (np.asarray(x_init)[:ws], np.asarray(goal)[:ws]):
            gap = min(gap, np.abs(NT.distance0(model, q, ref["boxes"], ref["spheres"])).min())
    bx, _ = V.obstacles(boxes, spheres)
    for x in X:
        for off in V.COMPONENTS[model]:
            for b in bx:
                gap = min(gap, LC.box_switch_gap(x[:ws] + off, b[0:3], b[3:6]))
    return gap
