"""The KKT certificate (tests/np_kkt.py) on the rows of tests/np_models.py, without a GPU: calibrated on oracle optima of all four
models at N = 50, and shown to reject points that are not optimal.  The certificate shares neither rows nor algorithm with the
oracle or the kernel: the oracle only supplies candidate points and linearisation points here.

Gates (np_kkt.GATES, in the problem scaled by kappa = 1 / max(1, omega)): stationarity 1e-7, complementarity 1e-7, |E z - e| 1e-9,
hard and BoxGoal violation 1e-9.  The objective gap kappa * obj(solver) - objective(certificate) is gated per model at OBJ_GAP:
an interior point method keeps its slacks at the final barrier level, above the optimal slacks the certificate sets."""
import ctypes as C

import numpy as np
import pytest
from scipy.linalg import null_space

import gusto_oracle as go
import np_kkt as K
import np_models as M
import gusto_jl_amd as g

P = g.problems
N = 50

# 10 x the worst gap measured on oracle optima in test_calibration_on_oracle_optima (freeflyer 8.5e-9, dubins 3.4e-8,
# astrobeeSE3 3.9e-8, manifold 2.0e-7: 50 knots x a few penalised rows, each slack about mu_floor above its optimum)
OBJ_GAP = {go.FREEFLYER_SE2: 1e-7, go.DUBINS_CAR: 4e-7, go.ASTROBEE_SE3: 4e-7, go.ASTROBEE_SE3_MANIFOLD: 2e-6}
MODEL = {go.FREEFLYER_SE2: M.FreeflyerSE2, go.DUBINS_CAR: M.Dubins, go.ASTROBEE_SE3: M.AstrobeeSE3,
         go.ASTROBEE_SE3_MANIFOLD: M.AstrobeeSE3Manifold}
NAME = {go.FREEFLYER_SE2: "freeflyerSE2", go.DUBINS_CAR: "dubins_car", go.ASTROBEE_SE3: "astrobeeSE3",
        go.ASTROBEE_SE3_MANIFOLD: "astrobeeSE3manifold"}
BINDING_DELTA = {go.FREEFLYER_SE2: 0.05, go.ASTROBEE_SE3: 0.1}


def env(model):
    """(boxes, spheres) of the model's benchmark environment"""
    if model == go.FREEFLYER_SE2:
        return P.freeflyer_env(), None
    if model == go.DUBINS_CAR:
        return None, None
    return P.iss_corner_env(True)


def batch(model, B, first=0):
    if model == go.FREEFLYER_SE2:
        x0, glo, ghi, tf = P.freeflyer_batch(B, first)
        if first == 0:
            x0[0] = P.FREEFLYER_X_INIT
        return x0, glo, ghi, tf
    if model == go.DUBINS_CAR:
        return P.dubins_batch(B, first)
    if model == go.ASTROBEE_SE3:
        return P.astrobee_se3_batch(B, first)
    return P.astrobee_manifold_batch(B, first)


def as_params(cls, mp):
    """a ModelParams of the oracle's or the library's binding as `cls` (the two structs have one layout); None stays None"""
    return None if mp is None else cls.from_buffer_copy(bytes(mp))


def rows(model, N, prob, Xp, Up, Delta, omega, toggle, boxes, spheres, model_params=None):
    x0, glo, ghi, tf = prob
    with M.model_params(model, model_params):
        return M.subproblem_rows(MODEL[model], N, tf, x0, glo, ghi, Xp, Up, Delta, omega, toggle,
                                 () if boxes is None else boxes, () if spheres is None else spheres)


def obj_gap(model, r_obj, c, kappa):
    """kappa * obj(solver) - objective(certificate), both in the scaled problem"""
    return kappa * r_obj - c["obj"]


def obj_gate(model, c):
    """OBJ_GAP, or the duality gap the solvers' stopping test allows (np_kkt.STOP_MU) where that is larger: the gap is the final
    barrier level summed over the pairs, and a long horizon with many rows ends higher than the calibration set (freeflyerSE2,
    N = 130, problem 7 of the config-2 set from the straight line: 3.7e-7 with mu = 5.5e-10 over 1 612 pairs)"""
    return max(OBJ_GAP[model], c["n_pairs"] * K.STOP_MU)


def oracle_trips(model, N, boxes, spheres, prob, max_iter=30, model_params=None):
    """(Xp, Up, Delta, omega) of the first, second, middle and last trip of an oracle SCP run; an empty list for a run that stops
    before its first trip (SubproblemFailed at the first subproblem: dubins_car at N = 3, where no control reaches the goal)"""
    o = go.Oracle(model, N, boxes=boxes, spheres=spheres, model_params=as_params(go.ModelParams, model_params))
    o.set_trace(max_iter + 2)
    o.set_problem(*prob)
    r = o.solve(max_iter)
    tr = o.trace()
    T = len(tr)
    return [(tr[t]["Xp"], tr[t]["Up"], r["Delta"][t], r["omega"][t]) for t in sorted({0, 1, T // 2, T - 1}) if 0 <= t < T]


def _calibration_points(model):
    """the linearisation points and (Delta, omega, toggle) of the calibration: straight line and oracle trips, (omega, Delta) at
    the model's defaults, omega = 10 and 100, a binding trust region where the model has one, every obstacle row present once"""
    mod = MODEL[model]
    boxes, spheres = env(model)
    x0, glo, ghi, tf = batch(model, 2)
    out = []
    o = go.Oracle(model, N, boxes=boxes, spheres=spheres)
    for b in range(2):
        prob = (x0[b], glo[b], ghi[b], tf[b])
        o.set_problem(*prob)
        Xp, Up = o.init_straightline()
        D0 = mod.Delta0
        settings = [(D0, 1.0), (D0, 10.0), (D0, 100.0)]
        if model in BINDING_DELTA:
            settings.append((BINDING_DELTA[model], 1.0))
        for D, om in settings:
            out.append((prob, Xp, Up, D, om, D / 8 + mod.clearance))
        out.append((prob, Xp, Up, D0, 1.0, 1e3))                      # every obstacle row present
        for Xp, Up, D, om in oracle_trips(model, N, boxes, spheres, prob):
            out.append((prob, Xp, Up, D, om, D / 8 + mod.clearance))
            if model in BINDING_DELTA:
                out.append((prob, Xp, Up, BINDING_DELTA[model], 10.0 * om, BINDING_DELTA[model] / 8 + mod.clearance))
    return out


@pytest.mark.parametrize("model", [go.FREEFLYER_SE2, go.DUBINS_CAR, go.ASTROBEE_SE3, go.ASTROBEE_SE3_MANIFOLD],
                         ids=lambda m: NAME[m])
def test_calibration_on_oracle_optima(model):
    """Oracle optima at N = 50 pass every gate (complementarity: np_kkt.comp_gate).  Worst values measured (scaled problem;
    freeflyerSE2 / dubins_car / astrobeeSE3 / astrobeeSE3manifold): stationarity 8.2e-10 / 5.1e-9 / 1.8e-9 / 2.5e-9, complementarity 9.9e-10 / 1.3e-8 / 6.0e-9 / 5.5e-9,
    |E z - e| 1.0e-14 / 1.1e-11 / 4.9e-15 / 5.1e-14, hard and BoxGoal rows never violated, objective gap 8.5e-9 / 3.4e-8 / 3.9e-8
    / 2.0e-7 (OBJ_GAP is 10x that).  The candidate band is np_kkt.TAU_CAND = 1e-2 (see there)."""
    boxes, spheres = env(model)
    o = go.Oracle(model, N, boxes=boxes, spheres=spheres)
    worst = dict(stat=0.0, comp=0.0, eq=0.0, hard=0.0, goal=0.0, gap=0.0)
    n_active = 0
    for prob, Xp, Up, D, om, tg in _calibration_points(model):
        o.set_problem(*prob)
        r = o.subproblem(Xp, Up, D, om, tg)
        assert r["status"] == 1, (NAME[model], D, om, r["status"])
        R = rows(model, N, prob, Xp, Up, D, om, tg, boxes, spheres)
        c = K.certify(R, r["X"], r["U"])
        assert not K.failures(c), (NAME[model], D, om, tg, K.failures(c))
        gap = obj_gap(model, r["obj"], c, R["kappa"])
        assert abs(gap) <= 0.2 * OBJ_GAP[model], (NAME[model], D, om, gap)
        for k in ("stat", "comp", "eq", "hard", "goal"):
            worst[k] = max(worst[k], c[k])
        worst["gap"] = max(worst["gap"], abs(gap))
        n_active += c["n_pen_active"]
    print(NAME[model], "oracle optima, worst:", {k: f"{v:.1e}" for k, v in worst.items()})
    if model != go.DUBINS_CAR:
        assert n_active > 0          # the set reaches points where penalised rows bind


@pytest.mark.parametrize("model,b,omega,Delta", [(go.FREEFLYER_SE2, 0, 1.0, 3.0), (go.FREEFLYER_SE2, 0, 1.0, 0.05),
                                                 (go.DUBINS_CAR, 2, 1.0, None), (go.ASTROBEE_SE3, 1, 10.0, 0.5),
                                                 (go.ASTROBEE_SE3_MANIFOLD, 0, 1.0, None)], ids=str)
def test_certificate_accepts_slsqp_optima(model, b, omega, Delta):
    """The SLSQP optima of test_oracle_models_slsqp.py's small-N cases pass at ALMOST_FACTOR x the gates: SLSQP stops on a 1e-15
    change of the objective, not on a KKT residual (measured: stationarity up to 3e-9, complementarity up to 1e-6 -- SLSQP leaves
    some slacks about 1e-9 above their optimum at a multiplier near 1)."""
    mod = MODEL[model]
    boxes, spheres = env(model)
    Nn = 8 if model != go.ASTROBEE_SE3_MANIFOLD else 6
    if model == go.ASTROBEE_SE3_MANIFOLD:
        boxes = boxes[:12]
    x0, glo, ghi, tf = batch(model, 3)
    prob = (x0[b], glo[b], ghi[b], tf[b])
    o = go.Oracle(model, Nn, boxes=boxes, spheres=spheres)
    o.set_problem(*prob)
    Xp, Up = o.init_straightline()
    D = Delta or mod.Delta0
    s = M.solve_subproblem(mod, Nn, tf[b], x0[b], glo[b], ghi[b], Xp, Up, D, omega, () if boxes is None else boxes,
                           () if spheres is None else spheres)
    c = K.certify(s["rows"], s["X"], s["U"])
    assert not K.failures(c, K.ALMOST_FACTOR), K.failures(c, K.ALMOST_FACTOR)
    r = o.subproblem(Xp, Up, D, omega, D / 8 + mod.clearance)
    assert abs(c["obj"] / s["rows"]["kappa"] - r["obj"]) <= 1e-6 * max(1.0, abs(r["obj"]))


def _ff_trip():
    """freeflyerSE2, problem 1 of the config-2 set, straight-line start at the model's (Delta, omega): obstacle rows bind"""
    boxes, _ = env(go.FREEFLYER_SE2)
    x0, glo, ghi, tf = batch(go.FREEFLYER_SE2, 2)
    prob = (x0[1], glo[1], ghi[1], tf[1])
    o = go.Oracle(go.FREEFLYER_SE2, N, boxes=boxes)
    o.set_problem(*prob)
    Xp, Up = o.init_straightline()
    return o, prob, boxes, Xp, Up


def test_rejects_a_move_along_the_null_space_of_the_equality_rows():
    """An oracle optimum moved 1e-5 (inf-norm) along a random direction in the null space of E: the equality rows still hold, the
    stationarity residual rejects it (measured 2e-5 .. 7e-5 against 1e-7)."""
    for model in (go.FREEFLYER_SE2, go.ASTROBEE_SE3, go.ASTROBEE_SE3_MANIFOLD):
        boxes, spheres = env(model)
        mod = MODEL[model]
        x0, glo, ghi, tf = batch(model, 1)
        prob = (x0[0], glo[0], ghi[0], tf[0])
        o = go.Oracle(model, N, boxes=boxes, spheres=spheres)
        o.set_problem(*prob)
        Xp, Up = o.init_straightline()
        D, tg = mod.Delta0, mod.Delta0 / 8 + mod.clearance
        r = o.subproblem(Xp, Up, D, 1.0, tg)
        R = rows(model, N, prob, Xp, Up, D, 1.0, tg, boxes, spheres)
        assert not K.failures(K.certify(R, r["X"], r["U"]))
        Z = null_space(R["E"])
        rng = np.random.default_rng(11)
        n = mod.n
        for _ in range(2):
            d = Z @ rng.standard_normal(Z.shape[1])
            z = np.hstack([r["X"], r["U"]]).ravel() + 1e-5 * d / np.abs(d).max()
            Zm = z.reshape(N, -1)
            c = K.certify(R, Zm[:, :n], Zm[:, n:])
            f = K.failures(c)
            assert "stat" in f and c["stat"] > 1e-6 and "eq" not in f, (NAME[model], f)


def test_rejects_an_optimum_solved_without_a_binding_obstacle():
    """The same subproblem solved with the obstacle whose rows carry the largest multiplier left out of the environment: its rows
    are violated at that point, their slacks positive, their multipliers 1, and nothing balances their gradient -- stationarity
    rejects it (measured about 1)."""
    o, prob, boxes, Xp, Up = _ff_trip()
    D, om, tg = 3.0, 1.0, 3.0 / 8 + 0.05
    R = rows(go.FREEFLYER_SE2, N, prob, Xp, Up, D, om, tg, boxes, None)
    r = o.subproblem(Xp, Up, D, om, tg)
    c = K.certify(R, r["X"], r["U"])
    assert not K.failures(c)
    obs = {}
    for nu, tag in zip(c["nu"], R["pen_tag"]):
        if tag[0] == "obs":
            obs[tag[2]] = max(obs.get(tag[2], 0.0), nu)
    i = max(obs, key=obs.get)
    assert obs[i] > 0.1, obs                     # a binding obstacle with a real multiplier
    o2 = go.Oracle(go.FREEFLYER_SE2, N, boxes=np.delete(boxes, i, 0))
    o2.set_problem(*prob)
    r2 = o2.subproblem(Xp, Up, D, om, tg)
    assert r2["status"] == 1
    c2 = K.certify(R, r2["X"], r2["U"])
    f = K.failures(c2)
    assert "stat" in f and c2["stat"] > 1e-2 and set(f) <= {"stat", "comp"}, f


def _oracle_ipm_opts(**kw):
    io = go.IpmOpts()
    L = go.lib()
    L.go_default_ipm_opts.argtypes = [C.c_void_p]
    L.go_default_ipm_opts(C.byref(io))
    for k, v in kw.items():
        setattr(io, k, v)
    return io


def test_rejects_a_loose_interior_point_stop():
    """The oracle with IpmOpts.tol = 1e-3 stops three or four iterations early and reports OPTIMAL: stationarity rejects the
    point (measured 1.4e-6 without a binding trust region, 6e-4 with one; gate 1e-7)."""
    o, prob, boxes, Xp, Up = _ff_trip()
    ol = go.Oracle(go.FREEFLYER_SE2, N, boxes=boxes, ipm_opts=_oracle_ipm_opts(tol=1e-3))
    ol.set_problem(*prob)
    for D, om in ((3.0, 1.0), (0.05, 1.0)):
        tg = D / 8 + 0.05
        r = ol.subproblem(Xp, Up, D, om, tg)
        assert r["status"] == 1 and r["iters"] < o.subproblem(Xp, Up, D, om, tg)["iters"]
        c = K.certify(rows(go.FREEFLYER_SE2, N, prob, Xp, Up, D, om, tg, boxes, None), r["X"], r["U"])
        f = K.failures(c)
        assert "stat" in f and c["stat"] > 1e-6 and "eq" not in f, f


def test_rejects_an_optimum_of_a_smaller_trust_region():
    """Solved with 0.9 Delta where the trust region binds (freeflyer Delta = 0.05), certified against Delta: the point is feasible
    but the trust-region rows sit 0.1 kappa Delta = 5e-3 inside.  They are candidates (band 1e-2), and the fit can only balance
    stationarity by loading them: complementarity rejects it (measured 2.0e-3 against 4e-7; stationarity 4.2e-5 as well).  Certified
    against 0.9 Delta the same point passes.  (The second trip of the oracle's run of problem
    0: from the straight line the trust-region rows at Delta = 0.05 are violated, so their multipliers are 1 at either radius.)"""
    boxes, _ = env(go.FREEFLYER_SE2)
    x0, glo, ghi, tf = batch(go.FREEFLYER_SE2, 1)
    prob = (x0[0], glo[0], ghi[0], tf[0])
    Xp, Up, _, _ = oracle_trips(go.FREEFLYER_SE2, N, boxes, None, prob)[1]
    o = go.Oracle(go.FREEFLYER_SE2, N, boxes=boxes)
    o.set_problem(*prob)
    D, om = 0.05, 1.0
    tg = D / 8 + 0.05
    r = o.subproblem(Xp, Up, D, om, tg)
    R = rows(go.FREEFLYER_SE2, N, prob, Xp, Up, D, om, tg, boxes, None)
    c = K.certify(R, r["X"], r["U"])
    assert not K.failures(c)
    assert sum(nu > 1e-3 for nu, tag in zip(c["nu"], R["pen_tag"]) if tag[0] == "tr") > 0      # the trust region binds
    r9 = o.subproblem(Xp, Up, 0.9 * D, om, tg)
    c9 = K.certify(R, r9["X"], r9["U"])
    f = K.failures(c9)
    assert "comp" in f and c9["comp"] > 1e-4 and set(f) <= {"stat", "comp"}, f
    assert not K.failures(K.certify(rows(go.FREEFLYER_SE2, N, prob, Xp, Up, 0.9 * D, om, tg, boxes, None), r9["X"], r9["U"]))


def test_mean_complementarity_stop_leaves_one_pair_high():
    """A known property of the solvers' stopping test, pinned: it tests the mean complementarity (<= 0.1 tol = 1e-9 over the
    pairs), not the largest pair.  dubins_car, N = 64, problem 1 of config 3 from the straight line: the oracle reports OPTIMAL
    with one x_min row of y 2.3e-4 from active carrying a multiplier of 3.2e-3 -- complementarity 7.4e-7, above the flat 1e-7
    but within n_pairs * STOP_MU = 8.9e-7, the bound np_kkt.failures uses.  SLSQP on the same rows finds an objective 7.2e-7
    lower, which that same bound (the duality gap the stopping test allows) also covers; its point certifies with complementarity
    5e-12.  The device reproduces the oracle's value (tests/test_gpu_kkt.py::test_dubins)."""
    x0, glo, ghi, tf = P.dubins_batch(2)
    prob = (x0[1], glo[1], ghi[1], tf[1])
    o = go.Oracle(go.DUBINS_CAR, 64)
    o.set_problem(*prob)
    Xp, Up = o.init_straightline()
    r = o.subproblem(Xp, Up, 1e4, 1.0, 1e4 / 8 + 0.01)
    assert r["status"] == 1
    R = rows(go.DUBINS_CAR, 64, prob, Xp, Up, 1e4, 1.0, 1e4 / 8 + 0.01, None, None)
    c = K.certify(R, r["X"], r["U"])
    assert 5e-7 < c["comp"] <= K.comp_gate(c) and not K.failures(c), (c["comp"], K.comp_gate(c))
    s = M.solve_subproblem(M.Dubins, 64, tf[1], x0[1], glo[1], ghi[1], Xp, Up, 1e4, 1.0, maxiter=2000, toggle=1e4 / 8 + 0.01)
    cs = K.certify(s["rows"], s["X"], s["U"])
    assert cs["comp"] < 1e-9 and cs["stat"] < 1e-6, (cs["comp"], cs["stat"])
    assert 0 < r["obj"] - s["obj"] <= c["n_pairs"] * K.STOP_MU, (r["obj"], s["obj"])


def test_oracle_trips_of_a_run_that_fails_its_first_subproblem():
    """dubins_car at N = 3: no control reaches the goal in two steps, so the oracle's first subproblem is infeasible (SubproblemFailed
    with no trip traced) -- oracle_trips returns no trips instead of failing on the empty trace"""
    x0, glo, ghi, tf = batch(go.DUBINS_CAR, 2)
    for b in range(2):
        prob = (x0[b], glo[b], ghi[b], tf[b])
        o = go.Oracle(go.DUBINS_CAR, 3)
        o.set_problem(*prob)
        r = o.solve(30)
        assert r["stop_reason"] == 2 and r["iterations"] == 0
        assert oracle_trips(go.DUBINS_CAR, 3, None, None, prob) == []
    assert len(oracle_trips(go.DUBINS_CAR, 4, None, None, (x0[0], glo[0], ghi[0], tf[0]))) == 4
