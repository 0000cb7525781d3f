"""The fleet stage on the device (csrc/fleet.hip) against the numpy restatement (tests/np_fleet.py).  The inputs are put on the
handle as gusto_interpolate(X, U) of synthetic knot trajectories (positions on a line, the velocity entries constant, U = 0: the
roll-out is that line), a second set comes from the device's own solves.  THE RESTATEMENT IS FED THE DEVICE'S OWN DENSE SAMPLES
(gusto_get_dense) AND tf, so only this stage is compared: tracks, J, delays and every integer bit for bit.  The separations are one square root and one subtraction behind D2; the bound stated for them was
4 * spacing(value + 2 radius).  The device's sqrt proved correctly rounded on every input of this file (all seven schedule cases
printed "bit for bit: True" on an MI355X), so they are held bit for bit as well."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import fleet_cases as FC
import gusto_jl_amd as g
import np_fleet as NF

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_KEYS = ("status", "delay_steps", "blocker", "partner", "step", "pair_step", "n_scheduled", "n_blocked", "n_conflicts", "makespan_steps")
SEP_KEYS = ("min_sep", "pair_min_sep", "fleet_min_sep")
ALL_KEYS = INT_KEYS + SEP_KEYS + ("delay",)


def geometry(model):
    _, mp = g.default_params(model)
    off = np.array([list(mp.comp_off[c]) for c in range(2)])
    return mp.radius, mp.clearance, off, mp.n_robot_comp


def solver_of(lines, tf, model=0, N=3, **interp):
    """a handle whose dense trajectories are the roll-outs of the lines (p0, p1) [B] flown in tf [B]"""
    n = g.MODEL_DIMS[model][0]
    B = len(lines)
    X = np.stack([FC.knots_of_line(p0, p1, N, n, t) for (p0, p1), t in zip(lines, tf)])
    U = np.zeros((B, N, g.MODEL_DIMS[model][1]))
    s = g.BatchSolver(model, N, B, hist_cap=64)
    s.set_problems(X[:, 0], X[:, -1], X[:, -1], np.asarray(tf, float))
    nfull, Xf, _ = s.interpolate(X, U, **interp)
    return s, nfull, Xf


def reference(s, nfull, Xf, R, h=0.1, margin=None, components=1, **kw):
    radius, clearance, off, nc = geometry(s.model)
    ws = g._capi.WS_DIM[s.model]
    Q = NF.tracks_of_dense(nfull, Xf, s._tf, h, ws)
    if kw.get("delay_steps") is None and "eligible" not in kw:
        st = s.status()
        kw["eligible"] = st["converged"] & st["successful"]
    el = kw.pop("eligible", np.ones(len(Q), bool))
    return Q, NF.report(Q, R, h, el, NF.pairs_of(off, nc, ws, components), radius, clearance if margin is None else margin, **kw)


def check(rep, ref, radius, keys=ALL_KEYS):
    exact = True
    for k in keys:
        a, b = np.asarray(rep[k]), np.asarray(ref[k]).reshape(np.shape(rep[k]))
        if k in SEP_KEYS:
            fin = np.isfinite(b)
            assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin]), k
            exact = exact and np.array_equal(a[fin], b[fin])
            assert np.array_equal(a[fin], b[fin]), (k, np.max(np.abs(a[fin] - b[fin]), initial=0.0), 4 * np.spacing(np.abs(b[fin]) + 2 * radius).max())
        else:
            assert a.tobytes() == b.astype(a.dtype).tobytes(), (k, a, b)
    return exact


def random_lines(rng, B, ws, span, tf_lo, tf_hi):
    lines = [(rng.uniform(-span, span, ws), rng.uniform(-span, span, ws)) for _ in range(B)]
    return lines, list(rng.uniform(tf_lo, tf_hi, B))


# ---- 1. tracks and J -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model, N, nstep", [(0, 3, 1), (0, 50, 2), (2, 3, 3), (3, 50, 1), (3, 3, 2)])
def test_tracks_bit_for_bit(model, N, nstep):
    """J_b of 2, 63, 64, 65, 255, 256, 257 (a wave and the track kernel's workgroup, plus and minus one) and 513 in one batch"""
    Js = [2, 63, 64, 65, 255, 256, 257, 513]
    tf = [(J - 1) * 0.1 - 0.05 for J in Js]
    rng = np.random.default_rng(model * 100 + N)
    ws = g._capi.WS_DIM[model]
    lines = [(rng.uniform(-2, 2, ws), rng.uniform(-2, 2, ws)) for _ in Js]
    s, nfull, Xf = solver_of(lines, tf, model, N, nstep=nstep)
    assert np.all(nfull == nstep * (N - 1) + 1)
    s.fleet_separation(1, delay_steps=np.zeros(len(Js), np.int32))
    J, Q = s.fleet_tracks()
    assert list(J) == Js and Q.shape == (len(Js), 513, ws)
    for b, q in enumerate(NF.tracks_of_dense(nfull, Xf, s._tf, 0.1, ws)):
        assert Q[b, :J[b]].tobytes() == q.tobytes(), b
        assert not Q[b, J[b]:].any()
        assert np.array_equal(Q[b, J[b] - 1], Xf[b, nfull[b] - 1, :ws])
    s.close()


# ---- 2. the schedule ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model, R, F, nd, stride, comp, custom", [
    (0, 1, 1, 64, 1, 1, False), (0, 2, 3, 64, 7, 1, True), (0, 5, 3, 1, 7, 0, False), (0, 5, 1, 64, 1, 1, True),
    (0, 64, 1, 8, 7, 1, False), (2, 5, 3, 64, 7, 1, True), (3, 2, 1, 64, 1, 0, False)])
def test_schedule_matches_the_restatement(model, R, F, nd, stride, comp, custom, capsys):
    rng = np.random.default_rng(R * 1000 + F * 10 + nd)
    B, ws = R * F, g._capi.WS_DIM[model]
    big = R == 64
    lines, tf = random_lines(rng, B, ws, 2.0 if big else 0.8, 1.0, 3.85 if big else 9.0)
    s, nfull, Xf = solver_of(lines, tf, model, 3, nstep=4)
    order = np.stack([rng.permutation(R) for _ in range(F)]) if custom else None
    eligible = rng.uniform(size=B) < 0.8 if custom else np.ones(B, bool)
    if custom and F > 1:
        eligible[R:2 * R] = False                     # a fleet with every robot NO_PLAN
    rep = s.fleet_schedule(R, order=order, eligible=eligible, n_delays=nd, delay_stride=stride, components=comp)
    Q, ref = reference(s, nfull, Xf, R, components=comp, eligible=eligible, order=order, n_delays=nd, stride=stride)
    if big:
        assert max(len(q) for q in Q) <= 40
    exact = check(rep, ref, geometry(model)[0])
    with capsys.disabled():
        print(f"\n  fleet R={R} F={F}: scheduled {int(rep['n_scheduled'].sum())} blocked {int(rep['n_blocked'].sum())} "
              f"conflicts {int(rep['n_conflicts'].sum())}; separations bit for bit: {exact}")
    if custom and F > 1:
        assert np.all(rep["status"][R:2 * R] == NF.NO_PLAN) and rep["n_scheduled"][1] == 0 and rep["makespan_steps"][1] == 0
    assert rep["F"] == F and rep["R"] == R and s.last_fleet_ms() > 0 and np.all(rep["stage_ms"] > 0)
    s.close()


def test_default_eligibility_reads_the_status_words():
    """no solve has run: nothing is converged, every robot is NO_PLAN"""
    lines, tf = random_lines(np.random.default_rng(5), 4, 2, 1.0, 2.0, 5.0)
    s, nfull, Xf = solver_of(lines, tf)
    rep = s.fleet_schedule(4)
    assert np.all(rep["status"] == NF.NO_PLAN) and np.all(rep["delay_steps"] == -1)
    check(rep, reference(s, nfull, Xf, 4)[1], FC.RADIUS)
    s.close()


def test_crossing_and_swap_on_the_device():
    lines = [((-2, 0), (2, 0)), ((0, -2), (0, 2)), ((-2, 0), (2, 0)), ((2, 0), (-2, 0))]
    s, nfull, Xf = solver_of(lines, [40.0] * 4, 0, 50)
    el = np.ones(4, bool)
    rep = s.fleet_schedule(2, eligible=el, delay_stride=5)
    assert list(rep["status"]) == [NF.SCHEDULED, NF.SCHEDULED, NF.SCHEDULED, NF.BLOCKED]
    assert list(rep["delay_steps"]) == [0, 70, 0, -1] and list(rep["blocker"]) == [-1, 0, -1, 0]
    check(rep, reference(s, nfull, Xf, 2, eligible=el, stride=5)[1], FC.RADIUS)
    rep = s.fleet_schedule(2, order=[[1, 0], [0, 1]], eligible=el, delay_stride=5)     # reversed: the other robot waits
    assert list(rep["delay_steps"][:2]) == [70, 0]
    s.close()


# ---- 3. the separation report ----------------------------------------------------------------------------------------------------
def test_separation_of_given_shifts_and_minimality():
    rng = np.random.default_rng(11)
    R, F, stride = 5, 2, 7
    lines, tf = [], list(rng.uniform(6.0, 9.0, R * F))          # two stars: every robot crosses the centre, the later ones wait
    for rot, radius in ((0.0, 2.0), (7.0, 1.5)):
        a, b = FC.star_points(R, radius, rot)
        lines += list(zip(a, b))
    s, nfull, Xf = solver_of(lines, tf, 0, 3, nstep=4)
    el = np.ones(R * F, bool)
    sched = s.fleet_schedule(R, eligible=el, delay_stride=stride)
    check(sched, reference(s, nfull, Xf, R, eligible=el, stride=stride)[1], FC.RADIUS)
    again = s.fleet_separation(R, delay_stride=stride)                     # the last schedule's shifts: the same report
    assert all(np.asarray(sched[k]).tobytes() == np.asarray(again[k]).tobytes() for k in ALL_KEYS) and again["stage_ms"][1] == 0
    ds = sched["delay_steps"].copy()
    ds[[1, 7]] = -1
    rep = s.fleet_separation(R, delay_steps=ds)
    check(rep, reference(s, nfull, Xf, R, delay_steps=ds)[1], FC.RADIUS)
    assert list(rep["status"][[1, 7]]) == [NF.NO_PLAN, NF.NO_PLAN] and np.all(rep["blocker"] == -1)
    # minimality on the device: the taken delay minus one stride conflicts with a robot placed earlier
    waited = [b for b in range(R * F) if sched["status"][b] == NF.SCHEDULED and sched["delay_steps"][b] > 0]
    assert waited
    for b in waited:
        ds = sched["delay_steps"].copy()
        ds[b] -= stride
        rep = s.fleet_separation(R, delay_steps=ds)
        f, i = divmod(b, R)
        assert rep["n_conflicts"][f] >= 1 and rep["pair_min_sep"][f, i, :i].min() < geometry(0)[1]
    assert s.fleet_separation(R, delay_stride=stride)["delay_steps"].tobytes() == sched["delay_steps"].tobytes()   # NULL: still the schedule's
    s.close()


# ---- 4. batch independence ---------------------------------------------------------------------------------------------------------
def test_a_fleet_is_the_same_anywhere_in_the_batch():
    rng = np.random.default_rng(21)
    R = 5
    mine, tf_mine = random_lines(rng, R, 2, 0.8, 2.0, 9.0)
    others, tf_o = random_lines(rng, 2 * R, 2, 0.8, 2.0, 20.0)
    outs = []
    for pos in (None, 0, 1, 2):
        fleets = [(mine, tf_mine)] if pos is None else [(others[:R], tf_o[:R]), (others[R:], tf_o[R:])]
        if pos is not None:
            fleets.insert(pos, (mine, tf_mine))
        lines, tf = sum((f[0] for f in fleets), []), sum((f[1] for f in fleets), [])
        s, _, _ = solver_of(lines, tf, 0, 3, nstep=4)
        rep = s.fleet_schedule(R, eligible=np.ones(len(lines), bool), delay_stride=7)
        J, Q = s.fleet_tracks()
        p = pos or 0
        fleet = {k: np.asarray(rep[k]).reshape(len(fleets), -1)[p] for k in ALL_KEYS}
        outs.append((fleet, J[p * R:(p + 1) * R], [Q[p * R + i, :J[p * R + i]] for i in range(R)]))
        s.close()
    for fleet, J, Q in outs[1:]:
        assert all(fleet[k].tobytes() == outs[0][0][k].tobytes() for k in ALL_KEYS) and np.array_equal(J, outs[0][1])
        assert all(a.tobytes() == b.tobytes() for a, b in zip(Q, outs[0][2]))


@pytest.mark.parametrize("span", [0.8, 6.0])
def test_pruning_changes_nothing(span):
    """span 6: most boxes lie apart and are skipped; span 0.8: next to none is"""
    lines, tf = random_lines(np.random.default_rng(int(span * 10)), 32, 2, span, 2.0, 9.0)
    s, _, _ = solver_of(lines, tf, 0, 3, nstep=4)
    el = np.ones(32, bool)
    a = s.fleet_schedule(16, eligible=el, delay_stride=3, prune=1)
    b = s.fleet_schedule(16, eligible=el, delay_stride=3, prune=0)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ALL_KEYS)
    s.close()


# ---- 5. nothing else moves ---------------------------------------------------------------------------------------------------------
def test_the_handle_is_left_alone_and_refusals_change_nothing():
    L = g.lib()
    lines, tf = random_lines(np.random.default_rng(31), 6, 2, 0.8, 2.0, 9.0)
    s, nfull, Xf = solver_of(lines, tf, 0, 3, nstep=4)
    s.set_env(boxes=np.array([[5.0, 5.0, -0.2, 6.0, 6.0, 0.2]]))
    s.interpolate(nstep=4)

    def snapshot():
        X, U = s.traj()
        nf, xf, uf = np.zeros(6, np.int32), np.zeros((6, 9, 6)), np.zeros((6, 8, 3))
        assert L.gusto_get_dense(s.h, nf.ctypes.data, xf.ctypes.data, uf.ctypes.data) == 0
        st, h, env = s.status(), s.history(), s.get_env()
        return [X, U, nf, xf, uf] + [np.asarray(v) for v in st.values()] + [np.asarray(v) for v in h.values()] + list(env[0]) + list(env[1])

    assert L.gusto_get_fleet(s.h, None, None, None) == -3 and L.gusto_get_fleet_tracks(s.h, None, None, None) == -3      # nothing called yet
    assert L.gusto_fleet_separation(s.h, 3, None, None) == -3 and b"gusto_fleet_schedule" in L.gusto_last_error(s.h)
    before = snapshot()
    el = np.ones(6, bool)
    rep = s.fleet_schedule(3, eligible=el, delay_stride=7)
    s.fleet_separation(3, delay_stride=7)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, snapshot()))
    J, Q = s.fleet_tracks()
    o = g.default_fleet_opts(0)
    o.delay_stride = 7
    bad_order, bad_steps = np.array([0, 1, 1, 0, 1, 2], np.int32), np.array([0, 0, -2, 0, 0, 0], np.int32)
    refusals = [lambda: L.gusto_fleet_schedule(s.h, 4, None, None, None), lambda: L.gusto_fleet_schedule(s.h, 0, None, None, None),
                lambda: L.gusto_fleet_schedule(s.h, 3, bad_order.ctypes.data, None, None),
                lambda: L.gusto_fleet_separation(s.h, 3, bad_steps.ctypes.data, None)]
    for field, v in (("dt_clock", 0.0), ("margin", -1.0), ("n_delays", 65), ("delay_stride", 0), ("clock_cap", 10), ("components", 2)):
        bad = g.FleetOpts(*(getattr(o, f) for f, _ in g.FleetOpts._fields_))
        setattr(bad, field, v)
        refusals.append(lambda bad=bad: L.gusto_fleet_schedule(s.h, 3, None, None, bad))
    for call in refusals:
        assert call() == -1
        now = s.fleet_info()
        assert all(np.asarray(now[k]).tobytes() == np.asarray(rep[k]).tobytes() for k in ALL_KEYS)
        J2, Q2 = s.fleet_tracks()
        assert J2.tobytes() == J.tobytes() and Q2.tobytes() == Q.tobytes()
    bad = g.FleetOpts(*(getattr(o, f) for f, _ in g.FleetOpts._fields_))
    bad.clock_cap = int(J.max()) - 1
    assert L.gusto_fleet_schedule(s.h, 3, None, None, bad) == -1 and b"problem %d needs" % int(np.argmax(J >= J.max())) in L.gusto_last_error(s.h)
    assert s.fleet_separation(3, delay_stride=7)["delay_steps"].tobytes() == rep["delay_steps"].tobytes()    # the schedule is still there
    # new problems end the stage, and the dense trajectories it reads
    s.set_problems(np.zeros((6, 6)), np.ones((6, 6)), np.ones((6, 6)), 10.0)
    assert L.gusto_get_fleet(s.h, None, None, None) == -3 and L.gusto_last_fleet_ms(s.h, C.byref(C.c_double())) == -3
    assert L.gusto_fleet_schedule(s.h, 3, None, None, None) == -3 and b"gusto_interpolate" in L.gusto_last_error(s.h)
    s.close()
    d = g.BatchSolver(1, 20, 2)                                   # DubinsCar
    d.set_problems(np.zeros((2, 3)), np.ones((2, 3)), np.ones((2, 3)), 5.0)
    assert L.gusto_fleet_schedule(d.h, 2, None, None, None) == -1 and b"DubinsCar" in L.gusto_last_error(d.h)
    d.close()
    t = g.TrajOptSolver(0, 20, 2)
    assert L.gusto_fleet_schedule(t.h, 2, None, None, None) == -1 and b"TrajOpt" in L.gusto_last_error(t.h)
    t.close()
    assert L.gusto_fleet_schedule(None, 2, None, None, None) == -1


# ---- 6. end to end ---------------------------------------------------------------------------------------------------------------
def fleet_problems(starts, goals, tf, N=20):
    H = g.host
    TOPs = []
    for a, b, t in zip(starts, goals, tf):
        gs = H.GoalSet()
        H.add_goal(gs, H.Goal(H.PointGoal(np.array([b[0], b[1], 0.0, 0.0, 0.0, 0.0])), t, range(0, 6)))
        PD = H.ProblemDefinition(H.Robot(), H.FreeflyerSE2(), H.BlankEnv(), np.array([a[0], a[1], 0.0, 0.0, 0.0, 0.0]), gs)
        TOPs.append(H.TrajectoryOptimizationProblem(PD, N, t, fixed_final_time=True))
    return [H.TrajectoryOptimizationSolution(t) for t in TOPs], TOPs


def test_driver_star_two_fleets():
    s0, e0 = FC.star_points()
    s1, e1 = FC.star_points(rot=10.0)
    TOSs, TOPs = fleet_problems(np.concatenate([s0, s1]), np.concatenate([e0, e1]), [40.0] * 8)
    rep = g.host.solve_SCP_fleet_batch(TOSs, TOPs, 4, park_keepouts=False)
    assert all(r["SCPS"].converged and r["SCPS"].successful for r in rep["robots"])
    assert np.all(rep["status"] == NF.SCHEDULED) and np.all(np.diff(rep["delay_steps"].reshape(2, 4), axis=1) > 0)
    assert np.all(rep["n_conflicts"] == 0) and np.all(rep["fleet_min_sep"] >= FC.CLEARANCE)
    nfull, P = rep["dense"]
    Q = NF.tracks_of_dense(nfull, P, [40.0] * 8, 0.1, 2)
    ref = NF.report(Q, 4, 0.1, np.ones(8, bool), NF.pairs_of(FC.COMP_OFF, 2, 2), FC.RADIUS, FC.CLEARANCE)
    check(rep, ref, FC.RADIUS)
    for q, T in enumerate(TOSs):
        assert T.fleet_status == NF.SCHEDULED and T.delay == rep["delay"][q] and T.traj.t[0] == T.delay and len(T.traj.t) == 20
    uncoordinated = NF.report(Q, 4, 0.1, np.ones(8, bool), NF.pairs_of(FC.COMP_OFF, 2, 2), FC.RADIUS, FC.CLEARANCE, delay_steps=np.zeros(8, np.int32))
    assert list(uncoordinated["n_conflicts"]) == [6, 6]


def test_driver_goal_crossing_with_and_without_parking_spheres():
    starts, goals, tf = [(-2.0, 0.0), (0.1, -2.0)], [(0.0, 0.0), (0.1, 2.0)], [15.0, 40.0]
    TOSs, TOPs = fleet_problems(starts, goals, tf)
    rep = g.host.solve_SCP_fleet_batch(TOSs, TOPs, 2, park_keepouts=False)
    assert list(rep["status"]) == [NF.SCHEDULED, NF.BLOCKED] and rep["blocker"][1] == 0
    TOSs, TOPs = fleet_problems(starts, goals, tf)
    rep = g.host.solve_SCP_fleet_batch(TOSs, TOPs, 2, park_keepouts=True)
    assert all(r["SCPS"].converged and r["SCPS"].successful for r in rep["robots"]) and not rep["park_skipped"]
    assert list(rep["status"]) == [NF.SCHEDULED, NF.SCHEDULED] and list(rep["delay_steps"]) == [0, 0] and rep["min_sep"][1] > FC.CLEARANCE
    with pytest.raises(ValueError):
        g.host.solve_SCP_fleet_batch(TOSs, TOPs + TOPs[:1], 2)


# ---- 7. the C consumer -------------------------------------------------------------------------------------------------------------
def test_c_consumer(tmp_path):
    """tests/c/c_abi_fleet.c, a plain C consumer with checks of its own; the delays it prints are the Python path's"""
    exe = os.path.join(tmp_path, "c_abi_fleet")
    lib = os.path.join(ROOT, "gusto.jl_amd")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "c_abi_fleet.c"),
                           "-o", exe, "-L" + lib, "-lgusto_hip", "-lm", "-Wl,-rpath," + lib])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    lines = out.stdout.strip().split("\n")
    assert lines[0] == "ok" and len(lines) == 2
    s, _, _ = solver_of([((-2, 0), (2, 0)), ((0, -2), (0, 2))], [40.0, 40.0], 0, 20)
    rep = s.fleet_schedule(2, eligible=np.ones(2, bool), delay_stride=5)
    assert [int(v) for v in lines[1].split()[:2]] == list(rep["delay_steps"]) and abs(float(lines[1].split()[2]) - rep["fleet_min_sep"][0]) < 1e-9
    s.close()
