"""The cases of tests/param_cases.py proven on the CPU before any kernel sees them (oracle + numpy only): non-default robot and
model scalars, above all an anisotropic inertia -- with the default, isotropic one w x Jw and the six w-w entries of the Jacobian
are zero everywhere else in the suite.

Per case, for exactly the linearisation points tests/test_gpu_params.py uses (param_cases.points):
  * the oracle's optimum under the case's parameters passes np_kkt.failures on the rows of np_models under the same parameters,
    np_kkt.GATES and test_kkt_certificate.OBJ_GAP unchanged (ALMOST: x ALMOST_FACTOR, as everywhere); for N <= 16 one SLSQP solve
    of the same rows agrees on the objective to 1e-6 relative;
  * power: the same optimum is REJECTED when the numpy model is corrupted -- each of the six gyroscopic entries of A with its sign
    flipped, one at a time (aniso, aniso_tight); Jdiag[0] read in place of Jdiag[2] (freeflyer); v = 2, k = 1 (dubins);
  * aniso_tight: at least one translational and one angular acceleration row active.
The post-solve references (np_tvlqr, np_simulate) are held against finite differences and against np_models' f under aniso."""
import numpy as np
import pytest

import gusto_oracle as go
import np_kkt as K
import np_models as M
import np_simulate as NS
import np_tvlqr as TV
import param_cases as PC
import test_kkt_certificate as T

FF, DUB, SE3, MAN = PC.FF, PC.DUB, PC.SE3, PC.MAN
ACTIVE = -1e-6          # a hard row counts as active when scale * value is above this
# NOT MET: the angular rows of the manifold model at N = 65.  The oracle's optima leave them at -1.5e-6 .. -1.9e-6, and no tighter
# limit is feasible (0.2564 rad/s^2 runs, 0.2535 does not).  A row's multiplier falls with the knot spacing and the interior
# point method's slack grows with it: the same problem holds -4.0e-7 .. -8.3e-7 at N = 16.  There the test asserts what does
# hold -- an angular row is a candidate of the certificate and carries a positive multiplier -- and prints the value.
ACTIVE_NOT_MET = {(MAN, 65)}
SLSQP_MODEL = {"aniso": MAN, "aniso_tight": SE3, "freeflyer": FF}    # one SLSQP solve per case with an N <= 16 (30 .. 170 s for an Astrobee model)
CASE_MODEL_N = [(c, m, N) for c, ms in PC.CASES.items() for m in ms for N in PC.HORIZONS[m]]
_ids = lambda v: T.NAME.get(v, str(v)) if isinstance(v, int) and v < 4 else str(v)


@pytest.fixture(scope="module")
def optima():
    """(case, model, N) -> [(point, oracle result, rows, certificate)] at the oracle's omega, computed once"""
    cache = {}

    def get(case, model, N):
        if (case, model, N) not in cache:
            boxes, spheres = T.env(model)
            out = []
            for pt in PC.points(case, model, N):
                mp, prob, Xp, Up, D, om, tg = pt
                o = go.Oracle(model, N, boxes=boxes, spheres=spheres, model_params=mp)
                o.set_problem(*prob)
                r = o.subproblem(Xp, Up, D, om, tg)
                R = T.rows(model, N, prob, Xp, Up, D, om, tg, boxes, spheres, mp)
                out.append((pt, r, R, K.certify(R, r["X"], r["U"])))
            cache[(case, model, N)] = out
        return cache[(case, model, N)]
    return get


def _factor(r):
    assert r["status"] in (1, 2), r["status"]
    return 1.0 if r["status"] == 1 else K.ALMOST_FACTOR


@pytest.mark.parametrize("case,model,N", [pytest.param(c, m, N, id=f"{c}-{T.NAME[m]}-{N}") for c, m, N in CASE_MODEL_N])
def test_oracle_optima_pass_the_certificate(case, model, N, optima, monkeypatch):
    """At the oracle's omega and at omega x 10.  Worst values measured (scaled problem): profiles/params_anisotropic.txt."""
    boxes, spheres = T.env(model)
    for k, v in PC.GATES.get((case, model, N), {}).items():
        monkeypatch.setitem(K.GATES, k, v)
    worst = dict(stat=0.0, comp=0.0, eq=0.0, hard=0.0, goal=0.0, gap=0.0)
    raised = []
    for (mp, prob, Xp, Up, D, om, tg), _, _, _ in optima(case, model, N):
        o = go.Oracle(model, N, boxes=boxes, spheres=spheres, model_params=mp)
        o.set_problem(*prob)
        r = o.subproblem(Xp, Up, D, 10.0 * om, tg)
        R = T.rows(model, N, prob, Xp, Up, D, 10.0 * om, tg, boxes, spheres, mp)
        raised.append(((mp, prob, Xp, Up, D, 10.0 * om, tg), r, R, K.certify(R, r["X"], r["U"])))
    for i, ((mp, prob, Xp, Up, D, om, tg), r, R, c) in enumerate(optima(case, model, N) + raised):
        fac = _factor(r)
        assert not K.failures(c, fac), (case, T.NAME[model], N, i, K.failures(c, fac))
        gap = T.obj_gap(model, r["obj"], c, R["kappa"])
        assert abs(gap) <= T.obj_gate(model, c) * fac, (case, T.NAME[model], N, i, gap)
        for k in ("stat", "comp", "eq", "hard", "goal"):
            worst[k] = max(worst[k], c[k])
        worst["gap"] = max(worst["gap"], abs(gap))
        if N <= 16 and i == 0 and model == SLSQP_MODEL.get(case):           # a second solver that shares nothing with the oracle
            with M.model_params(model, mp):
                s = M.solve_subproblem(T.MODEL[model], N, prob[3], prob[0], prob[1], prob[2], Xp, Up, D, om,
                                       () if boxes is None else boxes, () if spheres is None else spheres, toggle=tg)
            assert abs(s["obj"] - r["obj"]) <= 1e-6 * max(1.0, abs(r["obj"])), (case, T.NAME[model], N, s["obj"], r["obj"])
    print(f"params oracle {case} {T.NAME[model]} N={N} points={len(optima(case, model, N))}", {k: f"{v:.1e}" for k, v in worst.items()})


def _rejected(model, N, pt, r, corrupt):
    """np_kkt.failures of the oracle's optimum against rows built while `corrupt` (a context manager) holds"""
    mp, prob, Xp, Up, D, om, tg = pt
    boxes, spheres = T.env(model)
    with corrupt:
        R = T.rows(model, N, prob, Xp, Up, D, om, tg, boxes, spheres, mp)
    return K.failures(K.certify(R, r["X"], r["U"]), _factor(r))


class _flipped:
    """np_models.jac with the sign of A[w0 + i, w0 + j] flipped"""

    def __init__(self, w0, i, j):
        self.at = (w0 + i, w0 + j)

    def __enter__(self):
        self.orig = orig = M.jac

        def jac(model, x, u):
            A, B = orig(model, x, u)
            A[self.at] = -A[self.at]
            return A, B
        M.jac = jac

    def __exit__(self, *a):
        M.jac = self.orig


class _attr:
    """setattr for the length of a block (plain Python attributes: a ctypes array field would be read back as a view)"""

    def __init__(self, obj, **kw):
        self.obj, self.kw = obj, kw

    def __enter__(self):
        self.old = {k: getattr(self.obj, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(self.obj, k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            setattr(self.obj, k, v)


@pytest.mark.parametrize("case,model,N", [pytest.param(c, m, N, id=f"{c}-{T.NAME[m]}-{N}") for c, m, N in CASE_MODEL_N
                                          if c in ("aniso", "aniso_tight")])
def test_each_flipped_gyroscopic_entry_is_rejected(case, model, N, optima, monkeypatch):
    """every point, all six entries, one at a time (measured on the aniso points at N = 16: stationarity 5.6e-7 .. 1.8e-5 against
    1e-7, |E z - e| 1.2e-8 .. 6.6e-4 against 1e-9; every point fails at least one of the two)"""
    for k, v in PC.GATES.get((case, model, N), {}).items():
        monkeypatch.setitem(K.GATES, k, v)
    for i, (pt, r, R, c) in enumerate(optima(case, model, N)):
        w = np.abs(pt[2][:, PC.W0[model]:PC.W0[model] + 3]).max(axis=0)
        assert (w > 5e-3).all(), (case, T.NAME[model], N, i, w)          # the linearisation point turns about all three axes
        for (a, b) in PC.GYRO:
            f = _rejected(model, N, pt, r, _flipped(PC.W0[model], a, b))
            # |E z - e| is not scaled by kappa: what rejects the point here rejects it at omega x 10 as well
            assert "eq" in f, (case, T.NAME[model], N, i, (a, b), f)


def test_an_isotropic_model_is_rejected(optima):
    """the aniso optima against the default inertia (|E z - e| about 5e-3)"""
    for model in (SE3, MAN):
        for pt, r, R, c in optima("aniso", model, 16):
            mp, prob, Xp, Up, D, om, tg = pt
            iso = go.ModelParams.from_buffer_copy(bytes(mp))              # (a copy: the points are shared by the module)
            iso.Jdiag = go.default_params(model)[1].Jdiag
            f = K.failures(K.certify(T.rows(model, 16, prob, Xp, Up, D, om, tg, *T.env(model), iso), r["X"], r["U"]), _factor(r))
            assert tuple(mp.Jdiag) == PC.JDIAG and "eq" in f and f["eq"][0] > 1e-4, (T.NAME[model], f)


@pytest.mark.parametrize("model,N", [pytest.param(m, N, id=f"{T.NAME[m]}-{N}") for m in (SE3, MAN) for N in PC.HORIZONS[m]])
def test_tight_limits_bind_on_both_hard_rows(model, N, optima):
    """aniso_tight: at every point at least one translational and one angular acceleration row active (scale * value > -1e-6;
    ACTIVE_NOT_MET: where that does not hold), and at least one row of each kind loaded in the certificate (the hard candidates are the first columns of the fit, in the
    order of the rows)"""
    for i, (pt, r, R, c) in enumerate(optima("aniso_tight", model, N)):
        z = np.hstack([r["X"], r["U"]]).ravel()
        hv = [cc * fn(z)[0] for fn, cc, kd in R["hard"] if kd == "hard"]
        if model == MAN:                   # per knot: the hard half of the quaternion pair, then (k < N - 1) the two control rows
            at = [3 * k + 1 for k in range(N - 1)]
        else:
            at = [2 * k for k in range(N - 1)]
        acc, alp = np.array([hv[j] for j in at]), np.array([hv[j + 1] for j in at])
        print(f"params active {T.NAME[model]} N={N} point {i}: accel {int((acc > ACTIVE).sum())} rows, max {acc.max():.1e}; "
              f"alpha {int((alp > ACTIVE).sum())} rows, max {alp.max():.1e}")
        assert acc.max() > ACTIVE, (T.NAME[model], N, i, acc.max())
        assert alp.max() > ACTIVE or (model, N) in ACTIVE_NOT_MET, (T.NAME[model], N, i, alp.max())
        every = [cc * fn(z)[0] for fn, cc, kd in R["hard"]]
        where = [j for j, (_, _, kd) in enumerate(R["hard"]) if kd == "hard"]
        cand = [j for j, v in enumerate(every) if v >= -K.TAU_CAND]
        y = dict(zip(cand, c["y"]))
        y_acc = max(y.get(where[j], 0.0) for j in at)
        y_alp = max(y.get(where[j + 1], 0.0) for j in at)
        print(f"   multipliers: accel {y_acc:.1e}, alpha {y_alp:.1e}")
        assert y_acc > 1e-8 and y_alp > 1e-8, (T.NAME[model], N, i, y_acc, y_alp)


@pytest.mark.parametrize("N", PC.HORIZONS[FF])
def test_freeflyer_reading_the_wrong_axis_is_rejected(N, optima):
    """the numpy model with Jdiag[0] = 9.0 where Jdiag[2] = 0.25 belongs"""
    for i, (pt, r, R, c) in enumerate(optima("freeflyer", FF, N)):
        f = _rejected(FF, N, pt, r, _attr(M.FreeflyerSE2, J_AXIS=0))
        assert f, (N, i)


@pytest.mark.parametrize("N", PC.HORIZONS[DUB])
def test_dubins_default_speed_and_gain_are_rejected(N, optima):
    """the dubins optima (v = 1.3, k = 0.7) against rows with v = 2, k = 1"""
    for i, (pt, r, R, c) in enumerate(optima("dubins", DUB, N)):
        mp = PC.params("dubins", DUB)
        mp.dubins_v, mp.dubins_k = 2.0, 1.0
        _, prob, Xp, Up, D, om, tg = pt
        Rw = T.rows(DUB, N, prob, Xp, Up, D, om, tg, None, None, mp)
        f = K.failures(K.certify(Rw, r["X"], r["U"]), _factor(r))
        assert f, (N, i)


# ---- the context manager itself -------------------------------------------------------------------------------------------------
def test_model_params_restores_the_defaults():
    before = {c: {k: v for k, v in vars(c).items() if not k.startswith("__") and not isinstance(v, staticmethod)} for c in (M.Astrobee, M.FreeflyerSE2, M.Dubins)}
    for model in (FF, DUB, SE3, MAN):
        case = {FF: "freeflyer", DUB: "dubins"}.get(model, "aniso")
        mp = PC.params(case, model)
        with pytest.raises(ZeroDivisionError):
            with M.model_params(model, mp):
                if model in (SE3, MAN):
                    assert tuple(M.Astrobee.J) == PC.JDIAG and M.Astrobee.mass == 9.3 and M.AstrobeeSE3.r == mp.radius
                elif model == FF:
                    assert M.FreeflyerSE2.J[2] == 0.25 and M.FreeflyerSE2.a_max == mp.hard_limit_accel
                else:
                    assert (M.Dubins.v, M.Dubins.k, M.Dubins.u_max) == (1.3, 0.7, 4.0)
                1 / 0
    for c, d in before.items():
        for k, v in d.items():
            assert np.array_equal(getattr(c, k), v) if isinstance(v, np.ndarray) else getattr(c, k) is v or getattr(c, k) == v, (c, k)


def test_angular_acceleration_row_is_per_axis():
    """sum_j (M_j / J_j)^2 - alpha_max^2 with a vector J: np_models against the oracle's row list at a point with three different
    moments"""
    mp = PC.params("aniso", SE3)
    N = 4
    x0, glo, ghi, tf = PC.problem(SE3, 1)
    o = go.Oracle(SE3, N, model_params=mp)
    o.set_problem(x0, glo, ghi, tf)
    Xp, Up = o.init_straightline()
    R = T.rows(SE3, N, (x0, glo, ghi, tf), Xp, Up, 10.0, 1.0, 1e3, None, None, mp)
    z = np.hstack([Xp, Up]).ravel()
    z[12 + 3:12 + 6] = [0.001, -0.002, 0.003]
    fn, scale, _ = R["hard"][1]
    val, (idx, gr) = fn(z)
    J = np.array(PC.JDIAG)
    assert abs(val - (np.sum((z[15:18] / J) ** 2) - mp.hard_limit_alpha ** 2)) < 1e-18
    assert np.abs(gr - 2 * z[15:18] / J ** 2).max() < 1e-15 and list(idx) == [15, 16, 17]


# ---- post-solve references under aniso ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobeeSE3", "astrobeeSE3manifold"])
@pytest.mark.parametrize("nstep", [1, 3])
def test_tvlqr_jacobians_against_central_differences(model, nstep):
    """np_tvlqr.jacobians (complex step through the roll-out) against (F(z + h_j e_j) - F(z - h_j e_j)) / 2 h_j of np_tvlqr.rollout.
    h_j = 1e-5 for a state, 1e-5 x mass for a force, 1e-5 x J_j for a moment: the same change of the state over the interval.
    Gate per column: truncation h^2 |F'''| / 6, 1e-9 with third derivatives up to 60, plus rounding 4 eps |F|_inf / h_j (positions
    about 11 m: 1e-9 for the states, 1.2e-8 for the moment about x).  The w-w block differs from the isotropic one by more than 1e-3
    at these rates."""
    mp = PC.params("aniso", model)
    X, U = PC.post_traj(model, 2, 9)
    dt = 20.0 / 8
    mod = T.MODEL[model]
    n, m = mod.n, mod.m
    w0 = PC.W0[model]
    with M.model_params(model, mp):
        for b, k in ((0, 0), (1, 4), (1, 7)):
            x, u = X[b, k], U[b, k]
            assert (np.abs(X[b][:, w0:w0 + 3]).max(axis=0) > 0.49 * mp.hard_limit_omega).all()
            AB = TV.jacobians(model, x, u, dt, nstep)
            fd = np.zeros_like(AB)
            hs = 1e-5 * np.concatenate([np.ones(n), np.full(3, mp.mass), PC.JDIAG])
            Fx = np.abs(TV.rollout(mod, x, u, dt, nstep)).max()
            for j in range(n + m):
                zp, zm = np.concatenate([x, u]), np.concatenate([x, u])
                zp[j] += hs[j]; zm[j] -= hs[j]
                fd[:, j] = (TV.rollout(mod, zp[:n], zp[n:], dt, nstep) - TV.rollout(mod, zm[:n], zm[n:], dt, nstep)) / (2 * hs[j])
                gate = 1e-9 + 4 * np.finfo(float).eps * Fx / hs[j]
                assert np.abs(AB[:, j] - fd[:, j]).max() < gate, (b, k, j, np.abs(AB[:, j] - fd[:, j]).max(), gate)
    iso = TV.jacobians(model, X[1, 4], U[1, 4], dt, nstep)                  # the default inertia again
    with M.model_params(model, mp):
        AB = TV.jacobians(model, X[1, 4], U[1, 4], dt, nstep)
    assert np.abs(AB - iso)[w0:w0 + 3, w0:w0 + 3].max() > 1e-3


@pytest.mark.parametrize("model", [SE3, MAN], ids=["astrobeeSE3", "astrobeeSE3manifold"])
def test_simulate_f_against_np_models_f(model):
    """np_simulate.f_cols (its own statement of f for astrobeeSE3; np_models' f on [n, S] arrays for the manifold model) against
    np_models' f one state at a time, |w| up to hard_limit_omega, and its difference from the isotropic f"""
    mp = PC.params("aniso", model)
    mod = T.MODEL[model]
    rng = np.random.default_rng(5)
    S = 9
    x, u = rng.uniform(-1, 1, (mod.n, S)), rng.uniform(-1, 1, (mod.m, S))
    w0 = PC.W0[model]
    x[w0:w0 + 3] *= mp.hard_limit_omega
    iso = NS.f_cols(model, x, u)
    with M.model_params(model, mp):
        F = NS.f_cols(model, x, u)
        for j in range(S):
            assert np.abs(F[:, j] - mod.f(x[:, j], u[:, j])).max() < 1e-15 * max(1.0, np.abs(F[:, j]).max()), j
        assert NS.f_cols(model, x.astype(np.longdouble), u.astype(np.longdouble)).dtype == np.longdouble
    J = np.array(PC.JDIAG)
    w = x[w0:w0 + 3]
    wd = (u[3:6] - np.cross(w.T, (J[:, None] * w).T).T) / J[:, None]
    assert np.abs(F[w0:w0 + 3] - wd).max() < 1e-14 and np.abs(F - iso)[w0:w0 + 3].max() > 1.0


def test_trajopt_restatement_under_the_freeflyer_case():
    """tests/test_oracle_trajopt.py's SLSQP restatement of the TrajOpt subproblem builds its rows from the oracle's ModelParams: the
    same comparison, same tolerances, under the freeflyer case from a turned start (the config problems never turn: no moment,
    no J).  Power over the axis: Jdiag[1] = 7 read for Jdiag[2] = 0.25 would make the moment 28 times as large, and 27 x the moment
    is more than ten times the 5e-4 the controls are compared to"""
    import test_oracle_trajopt as TO
    mp = PC.params("freeflyer", FF)
    r = TO._subproblem_against_slsqp(10, 1.0, 1.0, True, model_params=mp, x_init=PC.problem(FF, 0)[0])
    moment = np.abs(r["U"][:, 2]).max()
    assert (mp.Jdiag[1] / mp.Jdiag[2] - 1) * moment > 10 * 5e-4, moment
