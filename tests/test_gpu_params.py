"""Every kernel under non-default robot and model scalars (tests/param_cases.py), above all an anisotropic inertia: with the
default, isotropic one w x Jw and the six w-w entries of A are zero, and the rest of the suite multiplies the gyroscopic part of
the dynamics by nothing else.  tests/test_params_cpu.py proves on the CPU, for the very linearisation points used here, that the
certificate accepts the oracle's optima and rejects each flipped entry, the wrong inertia axis and the default Dubins constants.

  - GuSTO subproblems: the KKT certificate of tests/test_gpu_kkt.py (_certify, same gates; one measured gate, param_cases.GATES)
    with solver, rows and oracle under the case's parameters -- one wave, WAVE2 and WAVE4 at N = 16, the first multi-wave horizon
    N = 65, freeflyerSE2 at N = 5 and 50, dubins_car at N = 30; the oracle's (Delta, omega) and omega x 10;
  - the state machine: test_gpu_parity._lockstep_parity at N = 16 (the device evaluates the nonlinear f in the trust-region ratio);
  - TrajOpt subproblems against OracleTrajOpt, tolerances of test_gpu_trajopt.test_subproblem_parity;
  - the post-solve chain at N = 9 against the numpy restatements with the comparisons and constants of the stages' own files;
  - manifold shooting against the oracle's;
  - gusto_set_params on a live handle: bit for bit what a fresh handle returns, and back.
The worst certificate residuals are printed (-s); profiles/params_anisotropic.txt holds the values of a run."""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import gusto_oracle as go
import lincov_cases as LC
import np_kkt as K
import np_lincov as NL
import np_models as M
import np_simulate as NS
import np_tvlqr as TV
import param_cases as PC
import sim_cases as SC
import test_gpu_lincov as GL
import test_gpu_parity as TP
import test_gpu_simulate as GS
import test_gpu_trajopt as GTO
import test_gpu_tvlqr as GT
import test_gpu_verify as GV
import test_kkt_certificate as T
from test_gpu_horizons import LOCKSTEP_ARGS
from test_gpu_kkt import WAVE, WAVE2, WAVE4, _certify

pytestmark = pytest.mark.gpu

FF, DUB, SE3, MAN = PC.FF, PC.DUB, PC.SE3, PC.MAN
_id = lambda c, m, N: f"{c}-{T.NAME[m]}-{N}"


def _dev(mp):
    return T.as_params(g.ModelParams, mp)


# ---- GuSTO subproblems ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,model,N", [pytest.param(c, m, N, id=_id(c, m, N)) for c, ms in PC.CASES.items() for m in ms
                                          for N in PC.HORIZONS[m]])
def test_certified_subproblems(case, model, N, monkeypatch):
    """batches of 6 .. 8 subproblems (oracle trips of the case; aniso_tight: one handle per problem, both omega in one batch), two
    certified per batch, one at N = 65.  The SLSQP solve of the same rows runs on the CPU (tests/test_params_cpu.py: 30 .. 170 s for
    an Astrobee model at N = 16); here only for freeflyerSE2 at N = 5, where it takes a fraction of a second"""
    boxes, sph = T.env(model)
    for k, v in PC.GATES.get((case, model, N), {}).items():
        monkeypatch.setitem(K.GATES, k, v)
    decs = (None,) if model in (FF, DUB) else ((WAVE, WAVE2, WAVE4) if N == 16 else (WAVE,))
    raises = [PC.RAISE] if case == "aniso_tight" or N > 50 else [(ro,) for ro in PC.RAISE]
    sample = 1 if N > 50 else 2
    first = True
    for ro in raises:
        for g_, (mp, prob, Xp, Up, D, om, tg) in enumerate(PC.trip_batches(case, model, N, ro)):
            assert 4 <= len(D) <= 8 or model in (FF, DUB), len(D)
            for dec in decs:
                _certify(model, N, boxes, sph, prob, Xp, Up, D, om, tg, dec=dec, sample=sample, seed=g_, slsqp=first and model == FF,
                         label=f"params {case} {T.NAME[model]} group {g_} omega x{ro}", model_params=mp)
                first = False


# ---- the state machine ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobeeSE3", "astrobeeSE3manifold"])
def test_lockstep_trips(model):
    """every trip of the first 8 problems of the case's set from the oracle's own state, under aniso: the convex subproblem and one
    trip of the device's state machine -- rho evaluates the nonlinear f, w x Jw included -- with the per-model arguments of
    test_gpu_horizons.LOCKSTEP_ARGS"""
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = PC.batch(model, 8)
    info = TP._lockstep_parity(model, 16, boxes, sph, x0, glo, ghi, tf, max_iter=30, model_params=PC.params("aniso", model),
                               **LOCKSTEP_ARGS[model])
    print(f"params lockstep aniso {T.NAME[model]} N=16", info)


# ---- TrajOpt --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobeeSE3", "astrobeeSE3manifold"])
@pytest.mark.parametrize("mu,s_tr", [(1.0, 1.0), (5.0, 0.25)])
def test_trajopt_subproblems_aniso(model, mu, s_tr):
    """gusto_subproblem_trajopt against OracleTrajOpt around the aniso linearisation points (trips of GuSTO runs: from the straight
    line w = 0 and the gyroscopic entries vanish), N = 16"""
    boxes, sph = T.env(model)
    mp, prob, Xp, Up, _, _, _ = PC.trip_batches("aniso", model, 16)[0]
    GTO._subproblem_parity(model, 16, boxes, sph, prob, mu, s_tr, Xp, Up, model_params=mp)


def test_trajopt_subproblems_freeflyer():
    """the turned starts of the freeflyer case (the config problems never turn: no moment, no J).  The case has power over the
    axis: with Jdiag[1] = 7 read for Jdiag[2] = 0.25 the moment would be 28 times as large, and 27 x the largest moment is more
    than ten times the tolerance"""
    boxes, sph = T.env(FF)
    mp = PC.params("freeflyer", FF)
    for mu, s_tr in ((1.0, 1.0), (5.0, 0.25)):
        r = GTO._subproblem_parity(FF, 16, boxes, sph, PC.batch(FF, 6), mu, s_tr, model_params=mp)
        moment = np.abs(r["U"][:, :, 2]).max()
        print(f"params trajopt freeflyer mu={mu}: largest moment {moment:.2e}")
        assert (mp.Jdiag[1] / mp.Jdiag[2] - 1) * moment > 10 * 5e-5 * max(1.0, mu), moment


# ---- the post-solve chain -------------------------------------------------------------------------------------------------------
POST_N, POST_B = 9, 2
POST_MODES = (0, 2)            # sim_cases.MODES: nstep = 1; nstep = 0 with dt_min = 0.2 (three substeps)
POST_S = 65


@functools.lru_cache(maxsize=None)
def _post_inputs(model):
    X, U = PC.post_traj(model, POST_B, POST_N)
    return X, U, SC.DT[:POST_B] * (POST_N - 1), SC.env(model)


@functools.lru_cache(maxsize=None)
def _post_device(model):
    """one handle under aniso, the whole chain per roll-out mode"""
    X, U, tf, (boxes, spheres) = _post_inputs(model)
    Q, R, Qf = SC.WEIGHTS
    lo, hi = SC.bounds(model, 1)
    s = g.BatchSolver(model, POST_N, POST_B, hist_cap=16, boxes=boxes, spheres=spheres, model_params=_dev(PC.params("aniso", model)))
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    P = SC.perturbation(model, POST_S, nb=POST_B)
    out = {}
    for mode in POST_MODES:
        r = {}
        r["dense"] = s.interpolate(X, U, dense_collision=1, **SC.MODES[mode])
        r["report"] = s.get_verify()
        r["tvlqr"] = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, store_P=1, **SC.MODES[mode]), X, U)
        r["simulate"] = s.simulate(dict(n_samples=POST_S, u_lo=lo, u_hi=hi, dense_collision=1, store_knots=1, **SC.MODES[mode]),
                                   X, U, pert=P)
        r["Xcl"] = s.get_simulate_knots()
        r["lincov"] = s.lincov(LC.options(model, POST_N, mode, store_S=1), X, U)
        out[mode] = r
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def _post_reference(model, mode, aniso=True):
    """the restatement's AB, K, P under aniso (or, for the power assertion, under the default inertia)"""
    X, U, tf, _ = _post_inputs(model)
    Q, R, Qf = SC.WEIGHTS
    with M.model_params(model, PC.params("aniso", model) if aniso else None):
        out = [TV.tvlqr(model, X[b], U[b], tf[b], Q, R, Qf, **SC.MODES[mode]) for b in range(POST_B)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobeeSE3", "astrobeeSE3manifold"])
def test_post_verify_and_interpolate(model):
    X, U, tf, env = _post_inputs(model)
    w0 = PC.W0[model]
    assert (np.abs(X[..., w0:w0 + 3]).max(axis=1) > 0.49 * PC.params("aniso", model).hard_limit_omega).all()
    with M.model_params(model, PC.params("aniso", model)):
        for mode in POST_MODES:
            r = _post_device(model)[mode]
            assert GV._compare(model, r["report"], X, U, tf, lambda b: env, dense=r["dense"], **SC.MODES[mode]) == 0


@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobeeSE3", "astrobeeSE3manifold"])
def test_post_tvlqr(model):
    """the four rows of tests/test_gpu_tvlqr.py with their constants; and the case has power: the device's AB differs from the
    ISOTROPIC restatement's by more than 1e3 x TOL_AB in the w-w block"""
    n, _ = g.MODEL_DIMS[model]
    Q, R, Qf = SC.WEIGHTS
    w0 = PC.W0[model]
    worst = dict.fromkeys(("AB", "riccati_K", "riccati_P", "end_K", "end_P1", "identity"), 0.0)
    for mode in POST_MODES:
        AB, Kr, P = _post_reference(model, mode)
        iso = _post_reference(model, mode, aniso=False)[0]
        r = _post_device(model)[mode]["tvlqr"]
        assert r.P.shape == (POST_B, POST_N, n, n) and r.status.all() and not r.fail_knot.any()
        for b in range(POST_B):
            Kd, Pd = TV.riccati(r.AB[b], Q, R, Qf)
            worst["AB"] = max(worst["AB"], max(GT._rel(r.AB[b, k], AB[b, k]) for k in range(POST_N - 1)))
            worst["riccati_K"] = max(worst["riccati_K"], GT._rel(r.K[b], Kd))
            worst["riccati_P"] = max(worst["riccati_P"], max(GT._rel(r.P[b, k], Pd[k]) for k in range(POST_N)))
            worst["end_K"] = max(worst["end_K"], GT._rel(r.K[b], Kr[b]))
            worst["end_P1"] = max(worst["end_P1"], GT._rel(r.P[b, 0], P[b, 0]))
            for k in range(POST_N - 1):
                A, Bd, Pk = r.AB[b, k, :, :n], r.AB[b, k, :, n:], r.P[b, k]
                worst["identity"] = max(worst["identity"], np.abs(Pk - (Q * np.eye(n) + A.T @ r.P[b, k + 1] @ (A - Bd @ r.K[b, k]))).max()
                                        / np.abs(Pk).max())
                ww = np.abs(r.AB[b, k] - iso[b, k])[w0:w0 + 3, w0:w0 + 3].max() / np.abs(iso[b, k]).max()
                assert ww > 1e3 * GT.TOL_AB, (mode, b, k, ww)
    print(f"params tvlqr {T.NAME[model]}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert worst["AB"] <= GT.TOL_AB, worst
    assert worst["riccati_K"] <= GT.TOL_RICCATI and worst["riccati_P"] <= GT.TOL_RICCATI, worst
    assert worst["end_K"] <= GT.TOL_END and worst["end_P1"] <= GT.TOL_END, worst
    assert worst["identity"] <= GT.TOL_IDENTITY, worst


@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobeeSE3", "astrobeeSE3manifold"])
def test_post_simulate(model):
    """caller-supplied perturbations, clipping on, store_knots: as test_gpu_simulate.test_against_the_restatement, TOL"""
    X, U, tf, (boxes, spheres) = _post_inputs(model)
    n = X.shape[2]
    P = SC.perturbation(model, POST_S, nb=POST_B)
    lo, hi = SC.bounds(model, 1)
    worst = {}
    for mode in POST_MODES:
        d = _post_device(model)[mode]
        r, Xcl = d["simulate"], d["Xcl"]
        assert np.array_equal(Xcl[:, 0], X[:, None, 0, :] + P[:, :, :n])
        left_out = 0
        for b in range(POST_B):
            with M.model_params(model, PC.params("aniso", model)):
                q = NS.simulate(model, X[b], U[b], d["tvlqr"].K[b], tf[b], P[b], lo, hi, boxes, spheres, dense_collision=True,
                                **SC.MODES[mode])
            ok = ~SC.undecided(q)
            left_out += int((~ok).sum())
            assert np.array_equal(r["sample_flags"][b][ok], q["sample_flags"][ok]), (mode, b)
            assert np.array_equal(r["sample_dense_index"][b][ok], q["sample_dense_index"][ok]), (mode, b)
            if ok.all():
                for k in GS.REPORT_INT:
                    assert r[k][b] == q[k], (mode, b, k, r[k][b], q[k])
            for k in ("sample_min_dist", "x_final", "max_dev", "max_final_dev", "min_dist"):
                worst[k] = max(worst.get(k, 0.0), GS._rel(r[k][b], q[k]))
            worst["Xcl"] = max(worst.get("Xcl", 0.0), GS._rel(Xcl[b], q["Xcl"]))
        assert left_out <= 0.01 * POST_B * POST_S, (mode, left_out)
    print(f"params simulate {T.NAME[model]}: " + "  ".join(f"{k} {v:.3e}" for k, v in worst.items()))
    assert max(worst.values()) <= GS.TOL, worst


@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobeeSE3", "astrobeeSE3manifold"])
def test_post_lincov(model):
    """every output through test_gpu_lincov.compare, on the device's AB and K and end to end"""
    X, U, tf, (boxes, spheres) = _post_inputs(model)
    lo, hi = LC.bounds(model)
    for mode in POST_MODES:
        d = _post_device(model)[mode]
        tv, out = d["tvlqr"], d["lincov"]
        AB, Kr, _ = _post_reference(model, mode)
        with M.model_params(model, PC.params("aniso", model)):          # (the robot radius enters the obstacle margins)
            for b in range(POST_B):
                args = (None, SC.dx0(model), SC.du0(model), LC.du_white(model, POST_N, mode), lo, hi, boxes, spheres)
                ref = NL.lincov(model, X[b], U[b], tv.AB[b], tv.K[b], *args)
                end = NL.lincov(model, X[b], U[b], AB[b], Kr[b], *args)
                GL.compare(out, ref, b, GL.TOL_KNOT, GL.TOL_SUMMARY, (model, mode, b))
                GL.compare(out, end, b, GL.TOL_END, GL.TOL_END, (model, mode, b, "end to end"))


# ---- shooting -------------------------------------------------------------------------------------------------------------------
def test_manifold_shooting_aniso():
    """gusto_shoot against the oracle's shooting under aniso, as test_shooting.test_gpu_manifold_shooting_matches_the_oracle at the
    defaults (the costate half of the reference ODE leaves the gyroscopic terms out: as written, on both sides)"""
    B, N = 12, 50
    mp = PC.params("aniso", MAN)
    x0, glo, ghi, tf = PC.batch(MAN, B)               # tf = 10: w reaches 0.1 rad/s (below 0.02 at the config's tf = 40)
    bx, sp = T.env(MAN)
    s = g.BatchSolver(MAN, N, B, hist_cap=40, boxes=bx, spheres=sp, model_params=_dev(mp))
    s.set_problems(x0, glo, ghi, tf)
    s.solve(30)
    duals = s.dual()
    r = s.shoot()
    o = go.Oracle(MAN, N, boxes=bx, spheres=sp, model_params=mp)
    n_opt = 0
    for b in range(B):
        o.set_problem(x0[b], glo[b], ghi[b], tf[b])
        ro = o.shoot(p0=duals[b])
        assert int(r["status"][b]) == ro["status"], b
        if ro["status"] == 1:
            n_opt += 1
            assert int(r["newton_iters"][b]) == ro["newton_iters"], b
            assert np.abs(r["X"][b] - ro["X"]).max() < 1e-4 and np.abs(r["U"][b] - ro["U"]).max() < 1e-4
            assert np.abs(r["X"][b, -1] - glo[b]).max() <= 1e-3
    # (measured: 11 of these 12 end Optimal; the oracle alone, seeded by its own duals: 10, problems 0 and 5 being infeasible at tf = 10)
    print(f"params shooting aniso: {n_opt} of {B} Optimal")
    assert n_opt >= 8, n_opt


# ---- gusto_set_params on a live handle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobeeSE3", "astrobeeSE3manifold"])
def test_set_params_on_a_live_handle(model):
    """defaults -> aniso -> defaults on one handle: the aniso results are a fresh aniso handle's bit for bit, the last results the
    first ones bit for bit (a stale copy of the parameters on the device would show) -- one subproblem batch and one gusto_tvlqr.
    (The fresh handle's parameters go through gusto_set_params too, right after gusto_create: set before any use against set
    after use.)"""
    boxes, sph = T.env(model)
    mp = _dev(PC.params("aniso", model))
    _, prob, Xp, Up, D, om, tg = PC.trip_batches("aniso", model, 16)[0]
    Xt, Ut = PC.post_traj(model, len(D), 16)
    Q, R, Qf = SC.WEIGHTS
    topt = dict(Q=Q, R=R, Qf=Qf, nstep=3, store_P=1)

    def run(s):
        s.set_problems(*prob)
        sub = s.subproblem(Xp, Up, D, om, tg)
        tv = s.tvlqr(topt, Xt, Ut)
        return sub, tv

    def same(a, b):
        for k in ("X", "U", "obj", "status", "iters", "dual"):
            assert np.array_equal(a[0][k], b[0][k]), k
        for k in ("K", "P", "AB", "status", "fail_knot"):
            assert np.array_equal(getattr(a[1], k), getattr(b[1], k)), k

    s = g.BatchSolver(model, 16, len(D), hist_cap=8, boxes=boxes, spheres=sph)
    first = run(s)
    s.set_params(model_params=mp)
    live = run(s)
    s.set_params(model_params=g.default_params(model)[1])
    back = run(s)
    s.close()
    s = g.BatchSolver(model, 16, len(D), hist_cap=8, boxes=boxes, spheres=sph, model_params=mp)
    fresh = run(s)
    s.close()
    same(live, fresh)
    same(back, first)
    assert not np.array_equal(live[0]["U"], first[0]["U"]) and not np.array_equal(live[1].AB, first[1].AB)
