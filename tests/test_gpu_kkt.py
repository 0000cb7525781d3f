"""KKT certificate (tests/np_kkt.py) of the device's convex subproblem (gusto_subproblem through BatchSolver.subproblem): every
certified problem is checked for feasibility and for multipliers that satisfy the KKT conditions of the rows of tests/np_models.py
-- a statement of the problem that shares neither rows nor algorithm with the kernel or the oracle.  Unlike the parity tests this
does not care whether the optimum is unique (the manifold model's X is weakly determined inside its +-1e-4 BoxGoal).

Gates: np_kkt.failures for OPTIMAL, ALMOST_FACTOR = 1e3 (tol_acc / tol) x those for ALMOST; the objective gap kappa * obj - objective
of the certificate within test_kkt_certificate.obj_gate.  None of the gates depends on the oracle.  A problem the device reports
FAILED must be one the oracle fails as well (infeasible subproblems).  For N <= 16 the objective also matches an SLSQP solve of the
same rows to 1e-6 relative.  A seeded sample of each batch is certified; where the batch is larger than twice the resident
workgroups the sample includes problems past the first round of slots.  The file runs in about a minute on an MI355X."""
import numpy as np
import pytest

import np_kkt as K
import np_models as M
import test_kkt_certificate as T

pytestmark = pytest.mark.gpu

WAVE, WAVE2, WAVE4 = 1, 3, 4


def _mods():
    import gusto_jl_amd as g
    import gusto_oracle as go
    return g, go


def _certify(model, N, boxes, spheres, prob, Xp, Up, Delta, omega, toggle, dec=None, sample=4, seed=0, ipm_opts=None,
             slsqp=True, label="", model_params=None):
    """One batch through the device; certify a seeded sample.  prob = (x0, glo, ghi, tf) [B]; Delta, omega, toggle [B] or scalar.
    model_params (default: the model's own) goes to the solver, to the rows of the certificate and to the oracle alike.
    Returns the worst residuals; asserts every gate."""
    g, _ = _mods()
    x0, glo, ghi, tf = prob
    B = len(x0)
    Delta, omega, toggle = (np.broadcast_to(np.asarray(v, float), (B,)).copy() for v in (Delta, omega, toggle))
    s = g.BatchSolver(model, N, B, hist_cap=8, boxes=boxes, spheres=spheres, ipm_opts=ipm_opts,
                      model_params=T.as_params(g.ModelParams, model_params))
    if dec is not None:
        s.set_decomposition(dec)
    s.set_problems(x0, glo, ghi, tf)
    sub = s.subproblem(Xp, Up, Delta, omega, toggle)
    slots = s.launch_info()[0]
    rng = np.random.default_rng(seed)
    pick = set(rng.choice(B, size=min(sample, B), replace=False).tolist())
    if B > 2 * slots:           # slot reuse: problems that ran in a later round of the persistent workgroups
        pick |= set(rng.choice(np.arange(slots, B), size=2, replace=False).tolist())
    worst = dict(stat=0.0, comp=0.0, eq=0.0, hard=0.0, goal=0.0, gap=0.0)
    certs = []
    for b in sorted(pick):
        st = int(sub["status"][b])
        pb = (x0[b], glo[b], ghi[b], tf[b])
        if st == 3 and ipm_opts is None:        # FAILED: only where the oracle fails on the same subproblem (infeasible ones)
            assert _oracle(model, N, boxes, spheres, pb, Xp[b], Up[b], Delta[b], omega[b], toggle[b],
                           model_params)["status"] == 3, (label, b)
            continue
        assert st in (1, 2), (label, b, st)
        R = T.rows(model, N, pb, Xp[b], Up[b], Delta[b], omega[b], toggle[b], boxes, spheres, model_params)
        c = K.certify(R, sub["X"][b], sub["U"][b])
        certs.append((b, st, c))
        if ipm_opts is not None:
            continue
        f = K.failures(c, 1.0 if st == 1 else K.ALMOST_FACTOR)
        assert not f, (label, b, st, f, c["stat_at"])
        gap = T.obj_gap(model, sub["obj"][b], c, R["kappa"])
        gate = T.obj_gate(model, c) * (1.0 if st == 1 else K.ALMOST_FACTOR)
        assert abs(gap) <= gate, (label, b, gap, gate)
        for k in ("stat", "comp", "eq", "hard", "goal"):
            worst[k] = max(worst[k], c[k])
        worst["gap"] = max(worst["gap"], abs(gap))
        if slsqp and N <= 16 and b == min(pick):       # a second solver that shares nothing with the kernel
            with M.model_params(model, model_params):
                r = M.solve_subproblem(T.MODEL[model], N, tf[b], x0[b], glo[b], ghi[b], Xp[b], Up[b], Delta[b], omega[b],
                                       () if boxes is None else boxes, () if spheres is None else spheres, toggle=toggle[b])
            assert abs(r["obj"] - sub["obj"][b]) <= 1e-6 * max(1.0, abs(sub["obj"][b])), (label, b, r["obj"], sub["obj"][b])
    if ipm_opts is None:
        print(f"kkt {label} N={N} dec={dec} B={B} slots={slots} certified={len(pick)}",
              {k: f"{v:.1e}" for k, v in worst.items()})
    return worst, certs


def _oracle(model, N, boxes, spheres, pb, Xp, Up, Delta, omega, toggle, model_params=None):
    _, go = _mods()
    o = go.Oracle(model, N, boxes=boxes, spheres=spheres, model_params=T.as_params(go.ModelParams, model_params))
    o.set_problem(*pb)
    return o.subproblem(Xp, Up, Delta, omega, toggle)


def _resident(s):
    """workgroups the device keeps resident for the last launch of `s`: per CU x CUs (launch_info()[0] is that, capped at B)"""
    import torch
    return s.launch_info()[2] * torch.cuda.get_device_properties(s.device).multi_processor_count


def _trip_batch(model, N, boxes, spheres, prob, idx, raise_omega=1.0, delta=None, model_params=None):
    """oracle trips (first, second, middle, last) of the problems `idx`: (prob, Xp, Up, Delta, omega) batched"""
    x0, glo, ghi, tf = prob
    rows = []
    for b in idx:
        pb = (x0[b], glo[b], ghi[b], tf[b])
        for Xp, Up, D, om in T.oracle_trips(model, N, boxes, spheres, pb, model_params=model_params):
            rows.append((b, Xp, Up, D if delta is None else delta, raise_omega * om))
    bi = np.array([r[0] for r in rows])
    return ((x0[bi], glo[bi], ghi[bi], tf[bi]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]),
            np.array([r[3] for r in rows]), np.array([r[4] for r in rows]))


# ---- freeflyerSE2 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 37, 50, 64, 65, 130])
@pytest.mark.parametrize("obstacles", [True, False])
def test_freeflyer_straight_line(N, obstacles):
    g, _ = _mods()
    P = g.problems
    boxes = P.freeflyer_env() if obstacles else None
    prob = T.batch(T.go.FREEFLYER_SE2, 12)
    s = g.BatchSolver(g.FREEFLYER_SE2, N, 12, hist_cap=8)
    s.set_problems(*prob)
    Xp, Up = s.traj()
    for i, (om, D) in enumerate([(1.0, 3.0), (10.0, 3.0), (100.0, 0.75), (1.0, 0.05)]):
        _certify(g.FREEFLYER_SE2, N, boxes, None, prob, Xp, Up, D, om, D / 8 + 0.05, sample=3, seed=i, slsqp=(i == 0),
                 label=f"freeflyer straight obstacles={obstacles} omega={om} Delta={D}")


@pytest.mark.parametrize("N", [5, 37, 50, 64, 65, 130])
def test_freeflyer_oracle_trips(N):
    """trips of oracle runs (the (Delta, omega) of the run, and again with Delta = 0.05 binding and omega x 10)"""
    g, _ = _mods()
    boxes = g.problems.freeflyer_env()
    prob = T.batch(T.go.FREEFLYER_SE2, 4)
    for k, (ro, dl) in enumerate([(1.0, None), (10.0, 0.05)]):
        pb, Xp, Up, D, om = _trip_batch(g.FREEFLYER_SE2, N, boxes, None, prob, range(4), ro, dl)
        _certify(g.FREEFLYER_SE2, N, boxes, None, pb, Xp, Up, D, om, D / 8 + 0.05, sample=5, seed=k,
                 label=f"freeflyer trips x{ro} Delta={dl}")


def _tile(B, pb, Xp, Up, D, om):
    """the trip batch repeated to B problems, omega of problem b scaled by 1 + 1e-3 b: no two problems have the same inputs, so a
    workspace left over from whichever problem ran earlier in the same slot cannot pass for the right one"""
    rep = -(-B // len(D))
    tile = lambda a: np.concatenate([a] * rep)[:B]
    return tuple(tile(a) for a in pb), tile(Xp), tile(Up), tile(D), tile(om) * (1.0 + 1e-3 * np.arange(B))


def test_freeflyer_slot_reuse():
    """a batch of more than twice the resident workgroups (oracle trips, tiled and perturbed)"""
    g, _ = _mods()
    boxes = g.problems.freeflyer_env()
    prob = T.batch(T.go.FREEFLYER_SE2, 3)
    pb, Xp, Up, D, om = _trip_batch(g.FREEFLYER_SE2, 50, boxes, None, prob, range(3), 10.0, 0.05)
    s = g.BatchSolver(g.FREEFLYER_SE2, 50, 8, hist_cap=8, boxes=boxes)
    s.set_problems(*[a[:1] for a in pb])
    s.subproblem(Xp[:1], Up[:1], D[:1], om[:1], D[:1] / 8 + 0.05)
    pb, Xp, Up, D, om = _tile(2 * _resident(s) + 37, pb, Xp, Up, D, om)
    _certify(g.FREEFLYER_SE2, 50, boxes, None, pb, Xp, Up, D, om, D / 8 + 0.05, sample=3, seed=5, label="freeflyer slot reuse")


def test_freeflyer_loose_interior_point_stop_is_rejected():
    """ipm_opts.tol = 1e-3: the device stops early and reports OPTIMAL; the certificate rejects every such output on stationarity
    (the oracle with the same options at the same eight trips: 2.7e-7 .. 8.6e-4 against 1e-7)"""
    g, _ = _mods()
    boxes = g.problems.freeflyer_env()
    prob = T.batch(T.go.FREEFLYER_SE2, 4)
    pb, Xp, Up, D, om = _trip_batch(g.FREEFLYER_SE2, 50, boxes, None, prob, range(2))
    io = g.default_ipm_opts()
    io.tol = 1e-3
    _, certs = _certify(g.FREEFLYER_SE2, 50, boxes, None, pb, Xp, Up, D, om, D / 8 + 0.05, sample=len(D), ipm_opts=io)
    print("kkt loose stop: stationarity", [f"{c['stat']:.1e}" for _, _, c in certs])
    optimal = [(b, c) for b, st, c in certs if st == 1]
    assert len(optimal) == len(D) and all("stat" in K.failures(c) for _, c in optimal), [(b, K.failures(c)) for b, c in optimal]


# ---- dubins_car ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [30, 64])
def test_dubins(N):
    g, _ = _mods()
    prob = g.problems.dubins_batch(16)
    prob[0][0] = [2.0, 2.0, 2.0]                 # on the state box as in test_subproblem_parity_dubins
    s = g.BatchSolver(g.DUBINS_CAR, N, 16, hist_cap=8)
    s.set_problems(*prob)
    Xp, Up = s.traj()
    _certify(g.DUBINS_CAR, N, None, None, prob, Xp, Up, 1e4, 1.0, 1e4 / 8 + 0.01, sample=6, label="dubins straight")
    pb, Xp, Up, D, om = _trip_batch(g.DUBINS_CAR, N, None, None, prob, range(3))
    _certify(g.DUBINS_CAR, N, None, None, pb, Xp, Up, D, om, D / 8 + 0.01, sample=6, seed=1, label="dubins trips")


# ---- the 12/13-state models: every decomposition --------------------------------------------------------------------------
_PICKED = {}


def _raised(model):
    """problems of the config set whose penalty weight the oracle raises, first, then the rest (test_gpu_parity._with_raised_penalty)"""
    import test_gpu_parity as tp
    g, _ = _mods()
    if model not in _PICKED:
        boxes, sph = T.env(model)
        _PICKED[model] = tp._with_raised_penalty(model, 50, boxes, sph, T.batch(model, 12), 3, 2)[0]
    return _PICKED[model]


def _decs(N):
    return [WAVE, WAVE2] + ([WAVE4] if N >= 16 else [])


@pytest.mark.parametrize("N", [12, 16, 33, 50, 63, 64])
def test_astrobee_se3(N):
    g, _ = _mods()
    boxes, sph = T.env(g.ASTROBEE_SE3)
    prob = _raised(g.ASTROBEE_SE3)
    for k, (ro, dl) in enumerate([(1.0, None), (10.0, 0.1)]):
        pb, Xp, Up, D, om = _trip_batch(g.ASTROBEE_SE3, N, boxes, sph, prob, range(len(prob[0])), ro, dl)
        for dec in _decs(N):
            _certify(g.ASTROBEE_SE3, N, boxes, sph, pb, Xp, Up, D, om, D / 8 + 0.03, dec=dec, sample=3, seed=k,
                     slsqp=(k == 0 and dec == WAVE), label=f"astrobeeSE3 trips omega x{ro} Delta={dl}")


@pytest.mark.parametrize("N", [12, 16, 50, 63])
def test_astrobee_manifold(N):
    g, _ = _mods()
    P = g.problems
    boxes, sph = T.env(g.ASTROBEE_SE3_MANIFOLD)
    prob = _raised(g.ASTROBEE_SE3_MANIFOLD)
    tf10 = P.astrobee_manifold_batch_tf10(2)         # problem 0 is the notebook's own problem
    for k, (pr, ro) in enumerate([(prob, 1.0), (prob, 10.0), (tf10, 1.0)]):
        pb, Xp, Up, D, om = _trip_batch(g.ASTROBEE_SE3_MANIFOLD, N, boxes, sph, pr, range(len(pr[0])), ro)
        for dec in _decs(N):
            _certify(g.ASTROBEE_SE3_MANIFOLD, N, boxes, sph, pb, Xp, Up, D, om, D / 8 + 0.03, dec=dec, sample=3, seed=k,
                     slsqp=(k == 0 and dec == WAVE), label=f"manifold trips omega x{ro} {'tf10' if pr is tf10 else 'config 5'}")


@pytest.mark.parametrize("model", ["astrobee_se3", "astrobee_se3_manifold"])
@pytest.mark.parametrize("dec", [WAVE, WAVE2, WAVE4])
def test_astrobee_slot_reuse(model, dec):
    """N = 50, a batch of more than twice the resident workgroups of the forced decomposition"""
    g, _ = _mods()
    mid = g.ASTROBEE_SE3 if model == "astrobee_se3" else g.ASTROBEE_SE3_MANIFOLD
    boxes, sph = T.env(mid)
    prob = _raised(mid)
    pb, Xp, Up, D, om = _trip_batch(mid, 50, boxes, sph, prob, range(2))
    s = g.BatchSolver(mid, 50, 1, hist_cap=8, boxes=boxes, spheres=sph)
    s.set_decomposition(dec)
    s.set_problems(*[a[:1] for a in pb])
    s.subproblem(Xp[:1], Up[:1], D[:1], om[:1], D[:1] / 8 + 0.03)
    pb, Xp, Up, D, om = _tile(2 * _resident(s) + 11, pb, Xp, Up, D, om)
    _certify(mid, 50, boxes, sph, pb, Xp, Up, D, om, D / 8 + 0.03, dec=dec, sample=2, seed=7, label=f"{model} slot reuse")
