"""The fleet stage without a GPU: the numpy restatement (tests/np_fleet.py) and the inputs (tests/fleet_cases.py) are proved here
-- tracks, the four scenarios of include/gusto_hip.h with their decision margins, invariants on random fleets against an
independent scalar double loop, the star and the goal crossing solved by the CPU oracle, the driver's parking spheres as a pure
function -- and fleet_args_host (csrc/fleet.hpp) compiled into a host program.  tests/test_gpu_fleet.py holds the device against
the same restatement."""
import json
import os
import subprocess

import numpy as np
import pytest

import fleet_cases as FC
import gusto_jl_amd as g
import np_fleet as NF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DOFF = NF.pairs_of(FC.COMP_OFF, 2, 2)
THR2 = (2 * FC.RADIUS + FC.MARGIN) ** 2


def run(P, tf, R, h=FC.H, eligible=None, **kw):
    Q = [NF.track(p, t, h) for p, t in zip(P, tf)]
    el = np.ones(len(Q), bool) if eligible is None else eligible
    return Q, NF.report(Q, R, h, el, DOFF, FC.RADIUS, FC.MARGIN, **kw)


# ---- 1. tracks -----------------------------------------------------------------------------------------------------------------
def test_track_end_points_and_line():
    rng = np.random.default_rng(1)
    for nfull in (2, 3, 17, 400):
        a, b, tf = rng.uniform(-2, 2, 2), rng.uniform(-2, 2, 2), float(rng.uniform(0.5, 30))
        P = FC.line(a, b, nfull)
        Q = NF.track(P, tf, FC.H)
        assert np.array_equal(Q[0], P[0]) and np.array_equal(Q[-1], P[-1])
        # a constant-speed line resampled stays on the line, at the clock's times, to within rounding
        t = np.minimum(np.arange(len(Q)) * FC.H / tf, 1.0)[:, None]
        assert np.max(np.abs(Q - ((1 - t) * a + t * b))) < 1e-13


@pytest.mark.parametrize("tf, J", [(4.0, 41), (4.0 - 1e-9, 41), (4.0 + 1e-9, 42), (0.1, 2), (0.03, 2), (0.25, 4)])
def test_clock_sample_rule(tf, J):
    """J_b = ceil(tf / h) + 1 at tf / h an integer, just below one, just above one, and at tf <= h"""
    assert NF.clock_samples(tf, 0.1) == J
    assert len(NF.track(FC.line((0, 0), (1, 0), 5), tf, 0.1)) == J


# ---- 2. the scenarios ------------------------------------------------------------------------------------------------------------
def test_crossing_decision_margins():
    P, tf = FC.crossing()
    Q, r = run(P, tf, 2, stride=5)
    assert list(r["status"]) == [NF.SCHEDULED, NF.SCHEDULED] and list(r["delay_steps"]) == [0, 70] and list(r["blocker"]) == [-1, 0]
    assert r["delay"][1] == 70 * np.float64(FC.H) and r["n_conflicts"][0] == 0
    sep = lambda s: np.sqrt(NF.D2(Q[1], s, Q[0], 0, DOFF).min()) - 2 * FC.RADIUS
    assert sep(70) - FC.MARGIN > 1e-3 and FC.MARGIN - sep(65) > 1e-3          # measured: +0.025 and -0.010
    assert abs(sep(70) - 0.0750) < 1e-3 and abs(sep(65) - 0.0396) < 1e-3
    assert r["pair_min_sep"][0, 0, 1] == sep(70)
    # reversed order: the other robot waits
    _, r2 = run(P, tf, 2, stride=5, order=[[1, 0]])
    assert list(r2["delay_steps"]) == [70, 0] and list(r2["blocker"]) == [1, -1]


def test_swap_is_blocked():
    P, tf = FC.swap()
    _, r = run(P, tf, 2)
    assert list(r["status"]) == [NF.SCHEDULED, NF.BLOCKED] and list(r["delay_steps"]) == [0, -1] and r["blocker"][1] == 0
    assert r["n_blocked"][0] == 1 and r["makespan_steps"][0] == 400 and r["delay"][1] == 0.0


def test_no_plan_still_blocks_its_start():
    P, tf = FC.crossing()
    P[0] = FC.line((0, 0), (3, 3), 50)      # robot 0 has no plan and sits at (0, 0), on robot 1's path
    _, r = run(P, tf, 2, eligible=np.array([False, True]))
    assert list(r["status"]) == [NF.NO_PLAN, NF.BLOCKED] and r["blocker"][1] == 0 and list(r["delay_steps"]) == [-1, -1]
    # a track with a non-finite entry is NO_PLAN whatever the caller says
    P[0][7, 1] = np.nan
    _, r = run(P, tf, 2)
    assert r["status"][0] == NF.NO_PLAN


def test_star_of_lines():
    s, e = FC.star_points()
    P, tf = [FC.line(a, b, 401) for a, b in zip(s, e)], [40.0] * 4
    Q, r0 = run(P, tf, 4, delay_steps=np.zeros(4, np.int32))
    assert r0["n_conflicts"][0] == 6 and abs(r0["fleet_min_sep"][0] + 2 * FC.RADIUS) < 1e-9     # all four in the centre at once
    _, r = run(P, tf, 4)
    assert np.all(r["status"] == NF.SCHEDULED) and np.all(np.diff(r["delay_steps"]) > 0) and r["n_conflicts"][0] == 0
    assert r["fleet_min_sep"][0] >= FC.MARGIN


# ---- 3. invariants on random fleets ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", [2, 5, 16])
def test_random_fleet_invariants(R):
    rng = np.random.default_rng(100 + R)
    P, tf = FC.random_fleet(rng, R, span=1.0)
    stride, nd = 7, 6
    order = rng.permutation(R)
    Q, r = run(P, tf, R, n_delays=nd, stride=stride, order=order[None, :])
    sig = r["delay_steps"]
    for p, i in enumerate(order):
        before = order[:p]
        hit = lambda s: [k for k in before if NF.conflict_scalar(Q[i], s, Q[k], int(sig[k]), DOFF, THR2)]
        if r["status"][i] == NF.SCHEDULED:
            assert not hit(int(sig[i]))
            assert all(hit(d * stride) for d in range(int(sig[i]) // stride))
        else:
            assert r["status"][i] == NF.BLOCKED and all(hit(d * stride) for d in range(nd))
        first = hit(0)
        assert r["blocker"][i] == (first[0] if first else -1)
    assert np.array_equal(r["pair_min_sep"], r["pair_min_sep"].transpose(0, 2, 1)) and np.array_equal(r["pair_step"], r["pair_step"].transpose(0, 2, 1))
    n = sum(NF.conflict_scalar(Q[a], int(sig[a]), Q[b], int(sig[b]), DOFF, THR2) for a in range(R) for b in range(a + 1, R))
    assert r["n_conflicts"][0] == n


# ---- 4. solved by the CPU oracle -------------------------------------------------------------------------------------------------
def oracle_paths(x0, goal, tf, spheres=None, N=20):
    import gusto_oracle as go
    out = []
    for b in range(len(x0)):
        o = go.Oracle(0, N, spheres=None if spheres is None else spheres[b])
        xi, xg = np.zeros(6), np.zeros(6)
        xi[:2], xg[:2] = x0[b], goal[b]
        o.set_problem(xi, xg, xg, tf[b])
        res = o.solve(30)
        out.append((res["X"][:, :2].copy(), res["converged"] and res["successful"]))
    return out


def test_star_solved_by_the_oracle():
    s, e = FC.star_points()
    sol = oracle_paths(s, e, [40.0] * 4)
    assert all(ok for _, ok in sol)
    P, tf = [p for p, _ in sol], [40.0] * 4
    _, r0 = run(P, tf, 4, delay_steps=np.zeros(4, np.int32))
    assert r0["n_conflicts"][0] == 6
    _, r = run(P, tf, 4)
    assert np.all(r["status"] == NF.SCHEDULED) and np.all(np.diff(r["delay_steps"]) > 0) and r["n_conflicts"][0] == 0


def test_goal_crossing_needs_the_parking_spheres():
    x0, goal, tf = np.array([[-2.0, 0.0], [0.1, -2.0]]), np.array([[0.0, 0.0], [0.1, 2.0]]), [15.0, 40.0]
    sol = oracle_paths(x0, goal, tf)
    _, r = run([p for p, _ in sol], tf, 2)
    assert list(r["status"]) == [NF.SCHEDULED, NF.BLOCKED] and r["blocker"][1] == 0
    sph, skipped = g.host.fleet_park_spheres(x0, goal, 2, FC.RADIUS, FC.MARGIN, FC.COMP_OFF)
    assert not skipped and sph[1].shape == (2, 4) and abs(sph[1][0, 3] - 0.507) < 1e-12
    sol = oracle_paths(x0, goal, tf, spheres=sph)
    assert all(ok for _, ok in sol)
    _, r = run([p for p, _ in sol], tf, 2)
    assert list(r["status"]) == [NF.SCHEDULED, NF.SCHEDULED] and list(r["delay_steps"]) == [0, 0] and r["min_sep"][1] > FC.MARGIN
    assert np.max(np.abs(sol[1][0][:, 0] - 0.1)) > 0.3        # robot 1 bends sideways around robot 0's goal


def test_parking_sphere_rule():
    park = g.host.fleet_park_spheres
    start, goal = np.array([[0.0, 0.0], [3.0, 0.0], [0.2, 0.0], [9.0, 9.0]]), np.array([[1.0, 1.0], [3.0, 3.0], [5.0, 5.0], [8.0, 8.0]])
    sph, skipped = park(start, goal, 2, 0.157, 0.05, FC.COMP_OFF)
    assert [len(s) for s in sph] == [2, 2, 2, 2] and not skipped
    assert np.array_equal(sph[0][:, :3], [[3.0, 0.0, 0.0], [3.0, 3.0, 0.0]]) and np.all(sph[0][:, 3] == 0.157 + 0.05 + 2 * 0.15)
    assert np.array_equal(sph[2][:, :2], [[9.0, 9.0], [8.0, 8.0]])          # fleets do not see each other
    # R = 4: robot 2 starts inside robot 0's start sphere -- that sphere is left out for both, and listed
    sph, skipped = park(start, goal, 4, 0.157, 0.05, FC.COMP_OFF)
    assert (2, 0, "start") in skipped and (0, 2, "start") in skipped and len(skipped) == 2
    assert len(sph[0]) == 5 and len(sph[2]) == 5 and len(sph[1]) == 6
    # one component only: no arm, a smaller sphere
    sph, _ = park(start, goal, 2, 0.157, 0.05, FC.COMP_OFF[:1])
    assert sph[0][0, 3] == 0.157 + 0.05
    # 64 components at the most, refused before anything is set
    with pytest.raises(ValueError, match="64"):
        park(start, goal, 2, 0.157, 0.05, FC.COMP_OFF, n_base=[63, 0, 0, 0])
    park(start, goal, 2, 0.157, 0.05, FC.COMP_OFF, n_base=[62, 0, 0, 0])
    with pytest.raises(ValueError):
        park(start[:3], goal[:3], 2, 0.157, 0.05, FC.COMP_OFF)


# ---- 5. fleet_args_host ----------------------------------------------------------------------------------------------------------
def test_fleet_arguments(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "fleet_args")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "gusto.jl_amd", "csrc"), "-x", "hip",
                           os.path.join(ROOT, "tests", "c", "fleet_args.cpp"), "-o", exe], stderr=subprocess.DEVNULL)
    ARG = -1
    d = dict(model=0, B=8, R=4, dt=0.1, margin=0.05, nd=64, stride=10, cap=8192, comp=1, prune=1, order=0, delay=0, tf=0)

    def case(**kw):
        return ",".join(repr(v) for v in dict(d, **kw).values())

    cases = [
        (case(), (0, "")), (case(order=1, delay=1, tf=1), (0, "")), (case(R=1), (0, "")), (case(R=8), (0, "")),
        (case(B=64, R=64), (0, "")), (case(model=2), (0, "")), (case(model=3), (0, "")), (case(delay=3), (0, "")),
        (case(model=1), (ARG, "who: DubinsCar cannot hold at its start and has no robot geometry")),
        (case(R=0), (ARG, "who: R outside 1 .. GUSTO_MAX_STARTS")), (case(B=130, R=65), (ARG, "who: R outside 1 .. GUSTO_MAX_STARTS")),
        (case(R=3), (ARG, "who: R does not divide B")),
        (case(dt=0.0), (ARG, "who: dt_clock must be positive and finite")), (case(dt=float("inf")), (ARG, "who: dt_clock must be positive and finite")),
        (case(dt=float("nan")), (ARG, "who: dt_clock must be positive and finite")),
        (case(margin=-1e-9), (ARG, "who: margin must be finite and >= 0")), (case(margin=0.0), (0, "")),
        (case(nd=0), (ARG, "who: n_delays outside 1 .. 64")), (case(nd=65), (ARG, "who: n_delays outside 1 .. 64")), (case(nd=1), (0, "")),
        (case(stride=0), (ARG, "who: delay_stride outside 1 .. GUSTO_FLEET_MAX_SHIFT / 64")),
        (case(cap=1), (ARG, "who: clock_cap outside 2 .. GUSTO_FLEET_MAX_SHIFT")),
        (case(comp=2), (ARG, "who: components must be 0 or 1")), (case(prune=-1), (ARG, "who: prune must be 0 or 1")),
        (case(order=2), (ARG, "who: order is not a permutation of 0 .. R - 1 (fleet 1)")),
        (case(order=3), (ARG, "who: order is not a permutation of 0 .. R - 1 (fleet 0)")),
        (case(delay=2), (ARG, "who: delay_steps outside -1 .. GUSTO_FLEET_MAX_SHIFT (problem 3)")),
        # the order of the refusals: the model, R, the options, order, delay_steps, the clock
        (case(model=1, R=0, dt=0.0), (ARG, "who: DubinsCar cannot hold at its start and has no robot geometry")),
        (case(R=3, dt=0.0, order=2), (ARG, "who: R does not divide B")),
        (case(nd=0, order=2, delay=2), (ARG, "who: n_delays outside 1 .. 64")),
        (case(order=2, delay=2, tf=2), (ARG, "who: order is not a permutation of 0 .. R - 1 (fleet 1)")),
        (case(delay=2, tf=2), (ARG, "who: delay_steps outside -1 .. GUSTO_FLEET_MAX_SHIFT (problem 3)")),
    ]
    out = json.loads(subprocess.check_output([exe] + [c for c, _ in cases]).decode().replace("nan", "NaN"))
    for (c, (rc, text)), r in zip(cases, out):
        assert (r["rc"], r["err"]) == (rc, text), (c, r)
    # the clock: J_max of the accepted, the first offending problem of the refused
    clock = [(case(tf=1), 0, 51, None), (case(tf=1, cap=51), 0, 51, None), (case(tf=1, cap=50), ARG, None, "problem 0 needs"),
             (case(tf=2), ARG, None, "problem 2 needs"), (case(tf=3), ARG, None, "problem 1 needs"), (case(tf=4), 0, 2, None),
             (case(tf=1, dt=5.0), 0, 2, None), (case(tf=1, dt=2.5), 0, 3, None)]
    out = json.loads(subprocess.check_output([exe] + [c for c, _, _, _ in clock]).decode().replace("nan", "NaN"))
    for (c, rc, J, text), r in zip(clock, out):
        assert r["rc"] == rc and (J is None or r["J_max"] == J) and (text is None or text in r["err"]), (c, r)
