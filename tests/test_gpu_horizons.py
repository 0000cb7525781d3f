"""Every GuSTO kernel from the shortest horizon to the longest its LDS layout takes (tests/horizons.py), and the refusal one knot past
that.  Above 64 knots a problem runs as 2, 3 or 4 waves with workgroup barriers (scp_kernel<MODEL, false>: the generic multi-wave
factor sweeps and row passes), from about 100 knots one workgroup per CU; the rest of the suite runs those kernels at 65 .. 130
knots of freeflyerSE2 only.

  - subproblems: the KKT certificate of tests/test_gpu_kkt.py (_certify, same gates) on the straight line and on oracle trips at
    N = 3, 4, the first and last N of each wave count and the model's largest N; omega x 10 at one N per wave count.  The
    certificate costs about 20 s per problem at N = 200 on the host, so one problem per case is certified above 100 knots;
  - whole runs: lock-step trips (test_gpu_parity._lockstep_parity) at N = 65 and at the largest N, _scp_parity at one long N;
  - the launch refuses N = limit + 1 (gusto_create already refuses N > 256) and launches nothing; a valid handle of the same
    process still solves.
The worst certificate residuals per model and N are printed (-s)."""
import numpy as np
import pytest

import gusto_jl_amd as g
import horizons as HZ
import np_kkt as K
import test_gpu_parity as TP
import test_kkt_certificate as T
from test_gpu_kkt import WAVE, WAVE2, WAVE4, _certify, _raised, _resident, _tile, _trip_batch

pytestmark = pytest.mark.gpu

FF, DUB, SE3, MAN = g.FREEFLYER_SE2, g.DUBINS_CAR, g.ASTROBEE_SE3, g.ASTROBEE_SE3_MANIFOLD
HORIZONS = {FF: [3, 4, 128, 129, 192, 193, 256], DUB: [3, 4, 65, 128, 129, 193, 256],
            SE3: [3, 4, 65, 128, 129, 192, 193, 200], MAN: [3, 4, 65, 128, 129, 182]}
# omega x 10 on the trips: one N per wave count (1, 2, 3, 4 waves)
RAISED = {FF: {4, 128, 129, 193}, DUB: {4, 65, 129, 256}, SE3: {4, 65, 129, 193}, MAN: {4, 65, 129, 182}}


def _sample(N):
    return 3 if N <= 65 else 1


def _problems(model):
    """the config set of the model; for the 12/13-state models the problems whose penalty the oracle raises come first"""
    return _raised(model) if model in (SE3, MAN) else T.batch(model, 8)


def _trips(model, N, boxes, sph, prob, idx, raise_omega):
    """test_gpu_kkt._trip_batch over the problems of `idx` whose oracle run has trips (T.oracle_trips: none where the first
    subproblem is infeasible); None if no problem has one"""
    x0, glo, ghi, tf = prob
    idx = [b for b in idx if T.oracle_trips(model, N, boxes, sph, (x0[b], glo[b], ghi[b], tf[b]))]
    return _trip_batch(model, N, boxes, sph, prob, idx, raise_omega) if idx else None


def _cases(pairs):
    return [pytest.param(*c, id="-".join([T.NAME[c[0]]] + [str(v) for v in c[1:]])) for c in pairs]


@pytest.mark.parametrize("model,N", _cases([(m, N) for m, Ns in HORIZONS.items() for N in Ns]))
def test_certified_subproblems_at_the_horizon_edges(model, N, monkeypatch):
    mod = T.MODEL[model]
    boxes, sph = T.env(model)
    name = T.NAME[model]
    prob = _problems(model)
    B = len(prob[0])
    s = g.BatchSolver(model, N, B, hist_cap=8, boxes=boxes, spheres=sph)
    s.set_problems(*prob)
    Xp, Up = s.traj()
    D0 = mod.Delta0
    worst = {}
    if model == FF and N == 3:
        # |E z - e| <= 1e-9 is absolute; at N = 3 a freeflyerSE2 step is dt = tf / 2 and the dynamics rows are that much larger.
        # Measured on problem 5 of this set from the straight line: 1.87e-9 for the ORACLE's optimum and the device's alike (the
        # other seven below 4e-10), so the equality gate of this one case is 3e-9; every other gate is unchanged
        monkeypatch.setitem(K.GATES, "eq", 3e-9)
    w, _ = _certify(model, N, boxes, sph, prob, Xp, Up, D0, 1.0, D0 / 8 + mod.clearance, sample=_sample(N),
                    slsqp=False, label=f"{name} horizon straight")
    worst["straight"] = w
    for k, ro in enumerate([1.0] + ([10.0] if N in RAISED[model] else [])):
        tb = _trips(model, N, boxes, sph, prob, range(2), ro)
        if tb is None:
            # dubins_car at N = 3: the oracle fails the first subproblem of every config problem (infeasible) -- the straight-line
            # batch above has then checked that the device reports FAILED on the certified ones (_certify's st == 3 rule)
            assert model == DUB and N == 3, (name, N)
            continue
        pb, Xt, Ut, D, om = tb
        w, _ = _certify(model, N, boxes, sph, pb, Xt, Ut, D, om, D / 8 + mod.clearance, sample=_sample(N), seed=k + 1,
                        slsqp=False, label=f"{name} horizon trips omega x{ro}")
        worst[f"trips x{ro:g}"] = w
    print(f"horizon worst {name} N={N} waves={HZ.waves(N)}:",
          {c: {r: f"{v:.1e}" for r, v in w.items()} for c, w in worst.items()})


def test_astrobee_slot_reuse_at_a_long_horizon():
    """astrobeeSE3, N = 128: one problem per CU; 2 x resident + 7 problems (oracle trips, tiled and perturbed), certified past the
    first round of slots"""
    boxes, sph = T.env(SE3)
    prob = _raised(SE3)
    pb, Xp, Up, D, om = _trip_batch(SE3, 128, boxes, sph, prob, range(2))
    s = g.BatchSolver(SE3, 128, 1, hist_cap=8, boxes=boxes, spheres=sph)
    s.set_problems(*[a[:1] for a in pb])
    s.subproblem(Xp[:1], Up[:1], D[:1], om[:1], D[:1] / 8 + 0.03)
    assert s.launch_info()[2] == 1                               # one workgroup per CU at this horizon
    pb, Xp, Up, D, om = _tile(2 * _resident(s) + 7, pb, Xp, Up, D, om)
    _certify(SE3, 128, boxes, sph, pb, Xp, Up, D, om, D / 8 + 0.03, sample=1, seed=3, label="astrobeeSE3 N=128 slot reuse")


@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobee_se3", "astrobee_se3_manifold"])
def test_chain_decompositions_are_refused_above_one_wave(model):
    """GUSTO_DECOMP_WAVE2 / WAVE4 split the horizon of a ONE-wave problem into chains (csrc/segw.hpp): at N = 65 there is no such
    kernel, and the forced decomposition is refused, not run as something else"""
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = T.batch(model, 2)
    for dec in (WAVE2, WAVE4):
        s = g.BatchSolver(model, 65, 2, hist_cap=8, boxes=boxes, spheres=sph)
        s.set_decomposition(dec)
        s.set_problems(x0, glo, ghi, tf)
        Xp, Up = s.traj()
        with pytest.raises(g.GustoError, match="WAVE2 / WAVE4"):
            s.subproblem(Xp, Up, 10.0, 1.0, 10.0 / 8 + 0.03)
        with pytest.raises(g.GustoError, match="WAVE2 / WAVE4"):
            s.solve(2)
    s = g.BatchSolver(model, 65, 2, hist_cap=8, boxes=boxes, spheres=sph)     # ... while one wave per problem is the 2-wave kernel
    s.set_decomposition(WAVE)
    s.set_problems(x0, glo, ghi, tf)
    Xp, Up = s.traj()
    assert np.isin(s.subproblem(Xp, Up, 10.0, 1.0, 10.0 / 8 + 0.03)["status"], (1, 2)).all()


# ---- whole GuSTO runs ---------------------------------------------------------------------------------------------------------
# the per-model arguments of the lock-step tests of tests/test_gpu_parity.py (measured there at N = 50)
LOCKSTEP_ARGS = {FF: {}, DUB: dict(max_cold_fail=3), SE3: dict(max_flag_mismatch=TP.GATE_FLAGS_SE3),
                 MAN: dict(sub_atol=3e-4, max_flag_mismatch=TP.GATE_FLAGS_MANIFOLD, q_tight=0.5, min_same_iters=0.7)}


@pytest.mark.parametrize("model,N", _cases([(m, N) for m in (FF, DUB, SE3, MAN) for N in (65, HZ.GUSTO[m])]))
def test_lockstep_trips_at_long_horizons(model, N):
    """every trip of 8 problems from the oracle's own state (_lockstep_parity): the subproblem and one trip of the device's state
    machine at N = 65 (the first two-wave horizon) and at the largest N the model's kernel takes"""
    boxes, sph = T.env(model)
    prob = _problems(model)
    x0, glo, ghi, tf = (a[:8] for a in prob)
    if model == DUB:
        x0 = x0.copy(); x0[0] = [2.0, 2.0, 2.0]          # on the state box as in test_lockstep_parity_dubins
    info = TP._lockstep_parity(model, N, boxes, sph, x0, glo, ghi, tf, max_iter=30, **LOCKSTEP_ARGS[model])
    print(f"lockstep {T.NAME[model]} N={N}", info)


@pytest.mark.parametrize("model,N,B", _cases([(SE3, 200, 8), (DUB, 256, 16)]))
def test_whole_runs_at_a_long_horizon(model, N, B):
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = T.batch(model, B)
    if model == DUB:
        x0[0] = [2.0, 2.0, 2.0]
        print("scp dubins N=256 diverged", TP._scp_parity(model, N, None, None, x0, glo, ghi, tf, max_diverged=1))
    else:
        TP._scp_parity(model, N, boxes, sph, x0, glo, ghi, tf, max_iter=10)


# ---- refusal one knot past the limit ------------------------------------------------------------------------------------------
def _assert_refused(s, calls):
    for what, call in calls:
        with pytest.raises(g.GustoError, match="does not fit the 160 KiB LDS") as e:
            call()
        assert "-1" in str(e.value), (what, str(e.value))          # GUSTO_ERR_ARG
    with pytest.raises(g.GustoError, match="nothing launched yet"):
        s.launch_info()                                              # no kernel went out


@pytest.mark.parametrize("trajopt", [False, True], ids=["gusto", "trajopt"])
def test_one_knot_past_the_limit_is_refused(trajopt):
    table = HZ.TRAJOPT if trajopt else HZ.GUSTO
    for model, limit in table.items():
        boxes, sph = T.env(model)
        x0, glo, ghi, tf = T.batch(model, 2)
        if limit == HZ.N_MAX:                                        # past 256 knots gusto_create refuses the handle itself
            with pytest.raises(g.GustoError, match="N <= 256"):
                (g.TrajOptSolver if trajopt else g.BatchSolver)(model, limit + 1, 2, boxes=boxes, spheres=sph)
            continue
        if trajopt:
            s = g.TrajOptSolver(model, limit + 1, 2, boxes=boxes, spheres=sph)
            s.set_problems(x0, glo, ghi, tf)
            Xp, Up = s.traj()
            _assert_refused(s, [("subproblem", lambda: s.subproblem(Xp, Up, 5.0, 0.25)), ("solve", lambda: s.solve(125)),
                                ("solve_async", lambda: s.solve_async(125))])
        else:
            s = g.BatchSolver(model, limit + 1, 2, hist_cap=40, boxes=boxes, spheres=sph)
            s.set_problems(x0, glo, ghi, tf)
            Xp, Up = s.traj()
            _assert_refused(s, [("subproblem", lambda: s.subproblem(Xp, Up, 10.0, 1.0, 10.0 / 8 + 0.03)),
                                ("solve", lambda: s.solve(30)), ("solve_async", lambda: s.solve_async(30))])
        s.close()
    # a valid handle of the same process still solves, and matches the oracle as in the N = 50 parity tests of that model
    import gusto_oracle as go
    if trajopt:
        model = SE3
        boxes, sph = T.env(model)
        x0, glo, ghi, tf = T.batch(model, 4)
        s = g.TrajOptSolver(model, 50, 4, boxes=boxes, spheres=sph)
        s.set_problems(x0, glo, ghi, tf)
        X0, U0 = s.traj()
        r = s.subproblem(X0, U0, 1.0, 1.0)
        o = go.OracleTrajOpt(model, 50, boxes=boxes, spheres=sph)
        for b in range(4):              # (test_gpu_trajopt.test_subproblem_parity's tolerances at mu = 1)
            o.set_problem(x0[b], glo[b], ghi[b], tf[b])
            ro = o.subproblem(X0[b], U0[b], 1.0, 1.0)
            assert r["status"][b] == ro["status"] and ro["status"] in (1, 2), b
            assert np.abs(r["X"][b] - ro["X"]).max() < 5e-5 and np.abs(r["U"][b] - ro["U"]).max() < 5e-5, b
            assert abs(r["obj"][b] - ro["obj"]) <= 1e-6 * max(1.0, abs(ro["obj"])), b
    else:               # (test_gpu_parity.test_subproblem_parity_astrobee_manifold)
        boxes, sph = T.env(MAN)
        x0, glo, ghi, tf = T.batch(MAN, 8)
        TP._sub_parity(MAN, 50, boxes, sph, x0, glo, ghi, tf, 1e3, 1.0, 1e3 / 8 + 0.03, atol=1e-4, u_atol=1e-6)
