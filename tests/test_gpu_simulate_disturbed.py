"""gusto_simulate_disturbed on the device against tests/np_simulate_disturbed.py, the numpy restatement in float64;
tests/test_simulate_disturbed_cpu.py pins that restatement and the conditioning of the inputs without a GPU.

Inputs: tests/sim_disturbed_cases.py -- the trajectories, environment, bounds and perturbations of tests/sim_cases.py (B = 5),
gains from the device's own gusto_tvlqr; S = 1, 64, 65, 257 at N = 3 and S = 65 at N = 50 on every model, over the roll-out modes,
dense_collision, clipping, and the three sources (off, generated, supplied) of the perturbations, the plant and the noise.

Exact: the plant scalars the kernel reports, the knot-1 states, the flags and the integer fields of every sample whose reference
is not within 1e-9 of a decision (at most 1 % are), and the report as the stated reduction of the device's own per-sample arrays.

Tolerance: TOL is not taken from the device.  tools/simulate_errors.py --disturbed measures on the CPU, over exactly these
cases, the largest relative difference between the float64 and the np.longdouble run of the restatement:
  sample_min_dist 2.6e-14, x_final 4.9e-14, max_dev 2.4e-14, max_final_dev 3.2e-14, min_dist 6.8e-15, Xcl 8.6e-14
TOL is 100 x the largest, rounded up to a power of ten.  The device's own errors against the float64 restatement, measured on an
MI355X (tools/simulate_errors.py --disturbed --device; profiles/simulate_disturbed.txt holds both):
  sample_min_dist 6.9e-15, x_final 5.8e-14, max_dev 2.1e-14, max_final_dev 2.8e-14, min_dist 2.8e-15, Xcl 6.2e-14"""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import np_simulate as NS
import np_simulate_disturbed as ND
import sim_cases as SC
import sim_disturbed_cases as DC
from test_simulate_disturbed_cpu import LINCOV_GATE, lincov_inputs, variance_error

pytestmark = pytest.mark.gpu

TOL = 1e-11         # 100 x 8.6e-14 (tools/simulate_errors.py --disturbed, float64 against longdouble), rounded up to a power of ten
REPORT_INT = ("n_free", "n_finite", "n_clipped", "worst_sample", "worst_dense_sample")


def _rel(a, ref):
    a, ref = np.asarray(a, float), np.asarray(ref, float)
    fin = np.isfinite(ref)
    assert np.array_equal(a[~fin], ref[~fin], equal_nan=True)
    return float(np.abs(a[fin] - ref[fin]).max() / np.abs(ref[fin]).max()) if fin.any() else 0.0


def _same(a, b, what=None):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), (what, k)


def nominal(model):
    """the handle's plant scalars: those of gusto_default_params"""
    mp = g.default_params(model)[1]
    return np.array([mp.mass, mp.Jdiag[0], mp.Jdiag[1], mp.Jdiag[2], mp.dubins_v, mp.dubins_k])


def _solver(model, N, X, U, tf, cap=None):
    boxes, spheres = SC.env(model)
    s = g.BatchSolver(model, N, cap or len(X), hist_cap=16, boxes=boxes, spheres=spheres)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    return s


def _opts(case, **more):
    model, N, S, mode, dense, clip = case[:6]
    lo, hi = SC.bounds(model, clip)
    return dict(dict(n_samples=S, seed=DC.SEED, dx0=SC.dx0(model), du0=SC.du0(model), u_lo=lo, u_hi=hi, dense_collision=dense,
                     **SC.MODES[mode]), **more)


def _disturbances(case, lo=0, hi=DC.B, swap=False):
    """the keyword arguments (disturb, pert, plant, white) of a case for the problems lo .. hi-1 of the batch, with first_problem =
    lo.  swap: generated instead of supplied and the other way round -- the same numbers from the other source."""
    model, N, S, mode, dense, clip, gen, psrc, wsrc = case
    flip = {DC.OFF: DC.OFF, DC.GENERATED: DC.SUPPLIED, DC.SUPPLIED: DC.GENERATED}
    if swap:
        gen, psrc, wsrc = 1 - gen, flip[psrc], flip[wsrc]
    nb = hi - lo
    return dict(disturb=dict(plant_rel=DC.plant_rel(psrc) if psrc == DC.GENERATED else 0.0, dw=DC.dw(model) if wsrc == DC.GENERATED else 0.0),
                pert=None if gen else SC.perturbation(model, S, lo, nb),
                plant=DC.plant(model, S, nominal(model), psrc, lo, nb) if psrc == DC.SUPPLIED else None,
                white=DC.white(model, N, S, wsrc, lo, nb) if wsrc == DC.SUPPLIED else None)


@functools.lru_cache(maxsize=None)
def device_and_reference(case):
    """(the device's report with store_knots, its Xcl, its plant scalars, the restatement's results with the DEVICE's gains),
    computed once per case and shared.  Along the way: store_knots changes no result, and generated and caller-supplied
    perturbations, plants and noises agree bit for bit."""
    model, N, S, mode = case[:4]
    X, U, tf, (Q, R, Qf) = SC.inputs(model, N)
    s = _solver(model, N, X, U, tf)
    K = s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]), X, U).K
    r0 = s.simulate_disturbed(_opts(case), X=X, U=U, **_disturbances(case))
    th0 = s.get_simulate_plant()
    assert s.last_simulate_ms() > 0
    r = s.simulate_disturbed(_opts(case, store_knots=1), X=X, U=U, K=K, **_disturbances(case))
    Xcl, th = s.get_simulate_knots(), s.get_simulate_plant()
    _same(r, r0, (case, "store_knots"))
    other = s.simulate_disturbed(_opts(case), X=X, U=U, **_disturbances(case, swap=True))
    _same(r, other, (case, "sources"))
    assert np.array_equal(th, th0, equal_nan=True) and np.array_equal(th, s.get_simulate_plant(), equal_nan=True)
    s.close()
    return r, Xcl, th, DC.reference(case, K=K, nominal=nominal(model))


@pytest.mark.parametrize("case", DC.CASES, ids=DC.IDS)
def test_against_the_restatement(case):
    model, N, S, mode, dense, clip, gen, psrc, wsrc = case
    r, Xcl, th, ref = device_and_reference(case)
    X = SC.inputs(model, N)[0]
    n = X.shape[2]
    assert np.array_equal(th, DC.plant(model, S, nominal(model), psrc))            # the plant, exactly
    P = SC.perturbation(model, S)
    assert np.array_equal(Xcl[:, 0], X[:, None, 0, :] + P[:, :, :n])                 # knot 1 of every sample is X_1 + p
    assert np.array_equal(Xcl[:, N - 1], r["x_final"])
    left_out = 0
    for b in range(DC.B):
        q = ref[b]
        ok = ~DC.undecided(q)
        left_out += int((~ok).sum())
        assert np.array_equal(r["sample_flags"][b][ok], q["sample_flags"][ok]), (case, b)
        assert np.array_equal(r["sample_dense_index"][b][ok], q["sample_dense_index"][ok]), (case, b)
        if ok.all():
            for k in REPORT_INT:
                assert r[k][b] == q[k], (case, b, k, r[k][b], q[k])
        for k in ("sample_min_dist", "x_final", "max_dev", "max_final_dev", "min_dist"):
            e = _rel(r[k][b], q[k])
            assert e <= TOL, (case, b, k, e)
        e = _rel(Xcl[b], q["Xcl"])
        assert e <= TOL, (case, b, "Xcl", e)
        # the report is the stated reduction of the device's own per-sample arrays
        own = NS.report(r["sample_min_dist"][b], r["sample_dense_index"][b], r["sample_flags"][b], r["x_final"][b],
                        np.abs(Xcl[b] - X[b][:, None, :]).max(axis=0), X[b, N - 1])
        for k in REPORT_INT:
            assert r[k][b] == own[k], (case, b, k)
        assert r["min_dist"][b] == own["min_dist"]
        assert np.array_equal(r["max_dev"][b], own["max_dev"]) and np.array_equal(r["max_final_dev"][b], own["max_final_dev"])
        assert np.array_equal((r["sample_flags"][b] & 1) != 0, r["sample_min_dist"][b] < 0)
    assert left_out <= 0.01 * DC.B * S, (case, left_out)


BITS = [c for c in DC.CASES if (c[1], c[2]) in ((3, 257), (50, 65))]


@pytest.mark.parametrize("case", BITS, ids=lambda c: "m%d-N%d-S%d" % c[:3])
def test_without_dispersion_it_is_gusto_simulate(case):
    """d = NULL (and all zeros), plant = white = NULL; and the nominal plant with zeros as white, supplied: every output equals
    gusto_simulate's as numbers.  A plain gusto_simulate after a disturbed call gives the plain results again, and
    gusto_get_simulate_plant then answers the state error."""
    model, N, S, mode = case[:4]
    gen = case[6]
    X, U, tf, (Q, R, Qf) = SC.inputs(model, N)
    s = _solver(model, N, X, U, tf)
    s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]))
    pert = None if gen else SC.perturbation(model, S)
    o = _opts(case, store_knots=1)
    plain, Xp = s.simulate(o, pert=pert), s.get_simulate_knots()
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_simulate_plant()
    nom = np.tile(nominal(model), (DC.B, S, 1))
    zeros = np.zeros((DC.B, N - 1, S, len(SC.du0(model))))
    for kw in (dict(), dict(disturb=dict(plant_rel=0.0, dw=0.0)), dict(plant=nom, white=zeros), dict(plant=nom), dict(white=zeros)):
        _same(s.simulate_disturbed(o, pert=pert, **kw), plain, (case, sorted(kw)))
        assert np.array_equal(s.get_simulate_knots(), Xp) and np.array_equal(s.get_simulate_plant(), nom)
    d = s.simulate_disturbed(o, pert=pert, **{k: v for k, v in _disturbances(case).items() if k != "pert"})
    if case[7] or case[8]:
        assert not np.array_equal(d["x_final"][:, 1:], plain["x_final"][:, 1:])
    assert np.array_equal(d["x_final"][:, 0], plain["x_final"][:, 0])            # (sample 0: the nominal plant, no noise)
    _same(s.simulate(o, pert=pert), plain, (case, "plain again"))
    assert np.array_equal(s.get_simulate_knots(), Xp)
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        s.get_simulate_plant()
    assert b"gusto_simulate_disturbed" in g.lib().gusto_last_error(s.h)
    s.close()


@pytest.mark.parametrize("case", BITS, ids=lambda c: "m%d-N%d-S%d" % c[:3])
def test_a_result_does_not_depend_on_the_batch_or_the_call(case):
    """a problem alone against the same problem inside the batch; two calls; first_problem sharding (handles of 2 and 3 problems
    against one of 5); an active mask keeps the inactive problems' earlier results, plant scalars among them -- all bit for bit"""
    model, N, S, mode = case[:4]
    X, U, tf, (Q, R, Qf) = SC.inputs(model, N)
    r, _, th, _ = device_and_reference(case)
    parts, plants = [], []
    for lo, hi in ((0, 2), (2, 5)):
        s = _solver(model, N, X[lo:hi], U[lo:hi], tf[lo:hi])
        s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]))
        kw = _disturbances(case, lo, hi)
        parts.append(s.simulate_disturbed(_opts(case, first_problem=lo), **kw))
        plants.append(s.get_simulate_plant())
        again = s.simulate_disturbed(_opts(case, first_problem=lo), **kw)
        _same(again, parts[-1], (case, "again"))
        if lo == 2:   # problems 2 and 4 only, with other bounds and another plant: problem 3 keeps what it had
            s.set_active(np.array([1, 0, 1], bool))
            m = s.simulate_disturbed(_opts(case, first_problem=lo, u_lo=-1e-3, u_hi=1e-3), **dict(kw, plant=2.0 * plants[-1]))
            for k in m:
                assert np.array_equal(m[k][1], again[k][1], equal_nan=True), k
            assert (m["n_clipped"][[0, 2]] == S).all() and not np.array_equal(m["x_final"][0], again["x_final"][0])
            pm = s.get_simulate_plant()
            assert np.array_equal(pm[1], plants[-1][1]) and np.array_equal(pm[[0, 2]], 2.0 * plants[-1][[0, 2]])
            s.set_active(None)
        s.close()
    for k in r:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), r[k], equal_nan=True), k
    assert np.array_equal(np.concatenate(plants), th)
    j = 3
    s = _solver(model, N, X[j:j + 1], U[j:j + 1], tf[j:j + 1])
    s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]))
    one = s.simulate_disturbed(_opts(case, first_problem=j), **_disturbances(case, j, j + 1))
    assert np.array_equal(s.get_simulate_plant()[0], th[j])
    s.close()
    for k in r:
        assert np.array_equal(one[k][0], r[k][j], equal_nan=True), k


def test_a_larger_handle_and_fewer_problems_leak_nothing():
    """a handle created for 8 problems holds the 5 of the batch: the batch's results; gusto_set_problems with the first 2 of them
    afterwards: those 2 problems' results, and plant scalars, and nothing of the other 3"""
    case = next(c for c in DC.CASES if c[:3] == (0, 50, 65))
    model, N, S, mode = case[:4]
    X, U, tf, (Q, R, Qf) = SC.inputs(model, N)
    r, Xcl, th, _ = device_and_reference(case)
    s = _solver(model, N, X, U, tf, cap=8)
    s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]))
    _same(s.simulate_disturbed(_opts(case, store_knots=1), **_disturbances(case)), r, "cap 8")
    assert np.array_equal(s.get_simulate_knots(), Xcl) and np.array_equal(s.get_simulate_plant(), th)
    s.set_problems(X[:2, 0], X[:2, -1], X[:2, -1], tf[:2], X[:2], U[:2])
    for call in (s.get_simulate, s.get_simulate_plant):
        with pytest.raises(g._capi.GustoError, match="-> -3"):
            call()
    s.tvlqr(dict(Q=Q, R=R, Qf=Qf, **SC.MODES[mode]))
    two = s.simulate_disturbed(_opts(case, store_knots=1), **_disturbances(case, 0, 2))
    for k in r:
        assert np.array_equal(two[k], r[k][:2], equal_nan=True), k
    assert np.array_equal(s.get_simulate_knots(), Xcl[:2]) and np.array_equal(s.get_simulate_plant(), th[:2])
    s.close()


def test_refusals():
    """each with its code, nothing launched, and the offending problem, sample and entry in gusto_last_error"""
    N, S = 5, 4
    L = g.lib()
    X, U, tf, (Q, R, Qf) = SC.inputs(0, N)
    t = g._capi.TrajOptSolver(0, N, SC.B)
    t.set_problems(X[:, 0], X[:, -1], X[:, -1], tf)
    with pytest.raises(g._capi.GustoError):
        t.simulate_disturbed()
    assert L.gusto_simulate_disturbed(t.h, None, None, None, None, None, None, None, None) == -1 and b"TrajOpt" in L.gusto_last_error(t.h)
    t.close()
    s = g.BatchSolver(0, N, SC.B, hist_cap=16)
    assert L.gusto_simulate_disturbed(s.h, None, None, None, None, None, None, None, None) == -3
    assert b"gusto_simulate_disturbed: call gusto_set_problems" in L.gusto_last_error(s.h)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], tf, X, U)
    assert L.gusto_simulate_disturbed(s.h, None, None, None, None, None, None, None, None) == -3
    assert b"gusto_simulate_disturbed: no gains" in L.gusto_last_error(s.h)
    assert L.gusto_simulate_disturbed(None, None, None, None, None, None, None, None, None) == -1
    assert L.gusto_get_simulate_plant(None, None) == -1 and L.gusto_default_disturb_opts(None) == -1
    s.close()
    for model in DC.MODELS:
        X, U, tf, (Q, R, Qf) = SC.inputs(model, N)
        m = U.shape[2]
        s = _solver(model, N, X, U, tf)
        s.tvlqr(dict(Q=Q, R=R, Qf=Qf))
        o = dict(n_samples=S, nstep=1)
        nom = np.tile(nominal(model), (SC.B, S, 1))

        def entry(a, idx, v):
            a = a.copy()
            a[idx] = v
            return a
        rel = np.zeros(6)
        bad = [(dict(disturb=dict(plant_rel=entry(rel, 2, 1.0))), b"plant_rel must lie in [0, 1) (entry 2)"),
               (dict(disturb=dict(plant_rel=entry(rel, 5, -1e-3))), b"plant_rel must lie in [0, 1) (entry 5)"),
               (dict(disturb=dict(plant_rel=entry(rel, 0, np.nan))), b"plant_rel must lie in [0, 1) (entry 0)"),
               (dict(disturb=dict(dw=entry(np.zeros(m), m - 1, -1.0))), b"dw must be finite and >= 0 (entry %d)" % (m - 1)),
               (dict(disturb=dict(dw=np.inf)), b"dw must be finite and >= 0 (entry 0)"),
               (dict(white=entry(np.zeros((SC.B, N - 1, S, m)), (3, 2, 1, m - 1), np.nan)),
                b"white must be finite (problem 3, interval 3, sample 1, entry %d)" % (m - 1)),
               (dict(white=entry(np.zeros((SC.B, N - 1, S, m)), (0, 0, 0, 0), -np.inf)), b"white must be finite (problem 0, interval 1, sample 0, entry 0)")]
        for j in ND.READS[model]:
            for v in (np.nan, np.inf) + ((0.0, -1.0) if j < 4 else ()):
                text = b"mass and Jdiag must be finite and > 0" if j < 4 else b"dubins_v and dubins_k must be finite"
                bad.append((dict(plant=entry(nom, (4, 2, j), v)), text + b" (problem 4, sample 2, entry %d)" % j))
        for kw, text in bad:
            with pytest.raises(g._capi.GustoError, match="-> -1"):
                s.simulate_disturbed(o, **kw)
            assert text in L.gusto_last_error(s.h), (model, kw, L.gusto_last_error(s.h))
            assert L.gusto_last_error(s.h).startswith(b"gusto_simulate_disturbed: ")
        with pytest.raises(g._capi.GustoError, match="-> -3"):
            s.get_simulate()                                       # (nothing was launched)
        with pytest.raises(g._capi.GustoError, match="-> -1"):
            s.simulate_disturbed(dict(o, n_samples=0))             # (gusto_simulate's refusals, under the new name)
        assert b"gusto_simulate_disturbed: n_samples" in L.gusto_last_error(s.h)
        # a NaN, or a negative number, in an entry the model does not read is accepted and changes nothing
        ok = s.simulate_disturbed(o, plant=nom)
        loose = nom.copy()
        for j in set(range(6)) - set(ND.READS[model]):
            loose[:, :, j] = np.nan if j % 2 else -1.0
        _same(s.simulate_disturbed(o, plant=loose), ok, (model, "unread entries"))
        assert np.array_equal(s.get_simulate_plant(), loose, equal_nan=True)
        _same(s.simulate(o), ok, (model, "plain"))
        s.close()


@pytest.mark.parametrize("model, rows, entry", [(0, slice(3, 5), 0), (0, slice(5, 6), 3), (1, slice(2, 3), 5)])
def test_closed_forms_of_the_two_linear_plants(model, rows, entry):
    """K = 0, no perturbation, no noise, a generated plant: the velocity gained times the sample's mass (the turn rate gained times
    its inertia; the Dubins car's heading gained over its k) is the same for every sample"""
    N, S = 9, 33
    X, U, tf, _ = SC.inputs(model, N)
    n, m = X.shape[2], U.shape[2]
    s = _solver(model, N, X, U, tf)
    s.simulate_disturbed(dict(n_samples=S, seed=DC.SEED, nstep=5, store_knots=1), dict(plant_rel=DC.PLANT_REL), K=np.zeros((SC.B, N - 1, m, n)),
                         pert=np.zeros((SC.B, S, n + m)))
    Xcl, th = s.get_simulate_knots(), s.get_simulate_plant()
    s.close()
    assert np.array_equal(th, ND.plants(nominal(model), SC.B, S, DC.PLANT_REL, DC.SEED))
    for b in range(SC.B):
        gained = Xcl[b, N - 1][:, rows] - Xcl[b, 0][:, rows]
        q = gained * th[b][:, entry:entry + 1] if model == 0 else gained / th[b][:, entry:entry + 1]
        assert np.abs(gained[1:] - gained[0]).max() > 1e-3 * np.abs(gained).max()
        assert np.abs(q - q[0]).max() <= TOL * np.abs(q).max(), (b, float(np.abs(q - q[0]).max() / np.abs(q).max()))


def test_rollouts_with_actuator_noise_have_the_covariance_of_the_devices_lincov():
    """gusto_tvlqr -> gusto_lincov(store_S, du_white = dw / sqrt(3)) -> gusto_simulate_disturbed(store_knots) at S = 4096 (16 tiles)
    on freeflyerSE2: the sample variance of every state at every knot over samples 1 .. S-1 is diag Sxx_k within five standard
    errors, 0.1105 relative; with the noise left out it is not"""
    model, N, X, U, tf, dw = lincov_inputs()
    S = 4096
    Q, R, Qf = SC.WEIGHTS
    s = _solver(model, N, X, U, tf)
    s.tvlqr(dict(Q=Q, R=R, Qf=Qf, nstep=5))
    cov = s.lincov(dict(dx0=SC.dx0(model), du0=SC.du0(model), du_white=dw / np.sqrt(3), store_S=1))
    o = dict(n_samples=S, seed=2024, dx0=SC.dx0(model), du0=SC.du0(model), nstep=5, store_knots=1)
    r = s.simulate_disturbed(o, dict(dw=dw))
    on = s.get_simulate_knots()
    s.simulate_disturbed(o)
    off = s.get_simulate_knots()
    s.close()
    assert (cov["status"] == 1).all() and (r["n_finite"] == S).all()
    for b in range(len(X)):
        e_on, e_off = variance_error(on[b], cov["Sxx"][b]), variance_error(off[b], cov["Sxx"][b])
        print(f"problem {b}: variance error with the noise {e_on:.4f}, without {e_off:.4f}, gate {LINCOV_GATE:.4f}")
        assert e_on <= LINCOV_GATE, (b, e_on)
        assert e_off > LINCOV_GATE, (b, e_off)


def test_host_mirror_and_batch_option():
    """host.simulate with disturb / plant / white on one trajectory; solve_SCP_batch(..., simulate=, disturb=) over two shards
    draws what one shard draws; disturb without simulate is refused"""
    H, P = g.host, g.problems
    env = P.freeflyer_env()
    x0 = P.freeflyer_random_x_init(4)
    TOPs = []
    for b in range(4):
        model = H.FreeflyerSE2()
        gs = H.GoalSet()
        H.add_goal(gs, H.Goal(H.PointGoal(P.FREEFLYER_X_GOAL), 200.0, model))
        TOPs.append(H.TrajectoryOptimizationProblem(H.ProblemDefinition(H.Robot(), model, H.Environment(env), x0[b], gs), 50, 200.0,
                                                    fixed_final_time=True))
    lq, sim, dist = dict(Q=10.0, R=1.0, Qf=10.0), dict(n_samples=5, seed=3), dict(plant_rel=[0.08134, 0, 0, 0.1, 0, 0], dw=1e-3)
    with pytest.raises(ValueError):
        H.solve_SCP_batch([H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs, max_iter=3, tvlqr=lq, disturb=dist)
    one = H.solve_SCP_batch([H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs, max_iter=3, tvlqr=lq, simulate=sim, disturb=dist)
    two = H.solve_SCP_batch([H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs, max_iter=3, tvlqr=lq, simulate=sim, disturb=dist,
                            devices=[0, 0])
    plain = H.solve_SCP_batch([H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs, max_iter=3, tvlqr=lq, simulate=sim)
    th = ND.plants(nominal(0), 4, 5, dist["plant_rel"], 3)
    for b in range(4):
        _same(one[b].simulate, two[b].simulate, b)
        assert np.array_equal(one[b].simulate["plant"], th[b]) and "plant" not in plain[b].simulate
        assert np.array_equal(one[b].simulate["x_final"][0], plain[b].simulate["x_final"][0])
        assert not np.array_equal(one[b].simulate["x_final"][1:], plain[b].simulate["x_final"][1:])
    traj = H.init_traj_straightline(TOPs[1])
    kw = dict(Q=10.0, R=1.0, Qf=10.0, n_samples=5, seed=3)
    base = H.simulate(traj, H.SCPProblem(TOPs[1]), **kw)
    r = H.simulate(traj, H.SCPProblem(TOPs[1]), disturb=dist, **kw)
    assert r["plant"].shape == (5, 6) and np.array_equal(r["plant"], ND.plants(nominal(0), 1, 5, dist["plant_rel"], 3)[0])
    assert np.array_equal(r["x_final"][0], base["x_final"][0]) and not np.array_equal(r["x_final"][1:], base["x_final"][1:])
    same = H.simulate(traj, H.SCPProblem(TOPs[1]), plant=np.tile(nominal(0), (5, 1)), white=np.zeros((49, 5, 3)), **kw)
    for k in base:
        assert np.array_equal(same[k], base[k], equal_nan=True), k
