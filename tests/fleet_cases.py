"""Inputs of the fleet tests (tests/test_fleet_cpu.py, tests/test_gpu_fleet.py): the freeflyerSE2 robot's geometry, straight
lines as dense samples, the four scenarios of include/gusto_hip.h's fleet stage and random fleets."""
import numpy as np

RADIUS, CLEARANCE = 0.157, 0.05                  # freeflyerSE2 defaults
COMP_OFF = np.array([[0.0, 0.0, 0.0], [0.0, 0.15, 0.0]])   # body and arm
MARGIN, H = 0.05, 0.1


def line(p0, p1, nfull):
    """nfull dense positions at constant speed from p0 to p1"""
    t = np.linspace(0.0, 1.0, nfull)[:, None]
    return (1 - t) * np.asarray(p0, float)[None, :] + t * np.asarray(p1, float)[None, :]


def crossing(nfull=401):
    """two constant-speed lines through one point at one time, tf = 40"""
    return [line((-2, 0), (2, 0), nfull), line((0, -2), (0, 2), nfull)], [40.0, 40.0]


def swap(nfull=401):
    """two robots swap places along one line"""
    return [line((-2, 0), (2, 0), nfull), line((2, 0), (-2, 0), nfull)], [40.0, 40.0]


def star_points(R=4, radius=2.0, rot=0.0):
    """starts on a circle at 0, 45, 90, 135 degrees (+ rot), goals at the antipodes"""
    a = np.deg2rad(np.arange(R) * 180.0 / R + rot)
    p = radius * np.stack([np.cos(a), np.sin(a)], axis=1)
    return p, -p


def random_fleet(rng, R, ws=2, span=2.0):
    """R straight tracks of unequal length in a box of side 2 span: (dense positions, tf)"""
    P, tf = [], []
    for _ in range(R):
        a, b = rng.uniform(-span, span, ws), rng.uniform(-span, span, ws)
        tf.append(float(rng.uniform(3.0, 12.0)))
        P.append(line(a, b, int(rng.integers(2, 40))))
    return P, tf


def knots_of_line(p0, p1, N, n, tf):
    """knot trajectories X [N, n], U = 0 whose roll-out is the line p0 -> p1 flown in tf: positions on the line, the velocity
    entries constant (positions first, velocities behind them in every model with robot geometry)"""
    ws = len(p0)
    X = np.zeros((N, n))
    X[:, :ws] = line(p0, p1, N)
    voff = {6: 3, 12: 3, 13: 3}[n]   # freeflyerSE2: (x, y, theta, vx, vy, w); Astrobee: (r, v, ...)
    X[:, voff:voff + ws] = (np.asarray(p1, float) - np.asarray(p0, float)) / tf
    if n == 13:
        X[:, 6] = 1.0                # a unit quaternion
    return X
