"""Inputs of the gusto_shoot tests, one table for the CPU proofs (tests/test_shoot_cpu.py) and the GPU tests
(tests/test_gpu_shoot.py).  No GPU here: the problems are the config sets of gusto_jl_amd.problems, the seeds are scale x the dual
of the oracle's SCP run of the problem at the case's horizon (30 iterations, default parameters, ISS corner with obstacles for the
manifold model), and the GPU tests hand every seed over from the host -- no gusto_solve, every horizon is usable.

  roll-out    max_newton = 0, ftol = 1e300: every problem with a finite end point is :Optimal after zero steps and the call is
              integrate + get_control + the knot-major staging + both transposes, nothing else.  Problem 1 of a batch has a box goal
              (lo < hi on every coordinate, the centre off the point goal), problem 2 one coordinate without a goal, the 33- and
              65-problem batches a NaN in one seed.  An SCP run that fails leaves a dual of any size (1e16); a seed is the dual scaled
              down by one
              factor to |p0_i| <= SEED_CAP_i so that the extremal stays bounded (tests/test_shoot_cpu.py asserts |X| <= 1e3).
  one step    max_newton = 1, default ftol, B = 8, the duals themselves.
  stragglers  one batch per model at one (N, substeps, ftol) that mixes problems which converge within the 8 Newton steps of the
              lane-per-problem pass, converge later, and never do; members are (problem, scale) pairs found by scanning the oracle
              over scales {0, 0.3, 0.6, 1.5, 2, 3, -0.5, 1}, problems 0-15 and N in {5, 8, 12, 20}.  tests/test_shoot_cpu.py
              re-derives what each member does with the oracle."""
import collections
import functools

import numpy as np

import gusto_oracle as go
import gusto_jl_amd as g
import np_shoot as NS

P = g.problems
DUB, MAN = go.DUBINS_CAR, go.ASTROBEE_SE3_MANIFOLD
NAME = {DUB: "dubins", MAN: "manifold"}
ROLL_OPTS = dict(max_newton=0, ftol=1e300)
# per component: the costates of position and velocity of a converged manifold run are 0.01 .. 1, those of the attitude and the
# angular rate 1e-6 .. 1e-4 (1 / (2 J^2) = 43 turns the latter into 4 rad/s^2 per 0.1, and RK4 steps of 5 s follow)
SEED_CAP = {DUB: np.ones(3), MAN: np.array([1.0] * 6 + [1e-3] * 7)}
X_BOUND = 1e3
JDIAG, MASS = (0.08, 0.11, 0.15), 9.3          # tests/param_cases.py: aniso
DUBINS_V, DUBINS_K = 1.3, 0.7                  # tests/param_cases.py: dubins
NAN_PROBLEM = 7                                # the problem whose seed gets a NaN (batches of 33 and 65)

Inputs = collections.namedtuple("Inputs", "model N substeps max_newton ftol x0 glo ghi tf p0 pcase")


def base(model, B):
    return P.dubins_batch(B) if model == DUB else P.astrobee_manifold_batch(B)


def env(model):
    return (None, None) if model == DUB else P.iss_corner_env(True)


def model_params(binding, model, pcase="default"):
    """ModelParams of `binding` (gusto_oracle or gusto_jl_amd: one layout) for the parameter case"""
    mp = binding.default_params(model)[1]
    if pcase == "nondefault":
        if model == DUB:
            mp.dubins_v, mp.dubins_k = DUBINS_V, DUBINS_K
        else:
            mp.Jdiag[0], mp.Jdiag[1], mp.Jdiag[2] = JDIAG
            mp.mass = MASS
    return mp


def par(model, pcase="default"):
    return NS.params(model, model_params(go, model, pcase))


@functools.lru_cache(maxsize=None)
def _scp(model, N):
    boxes, spheres = env(model)
    return go.Oracle(model, N, boxes=boxes, spheres=spheres)


@functools.lru_cache(maxsize=None)
def dual(model, N, b):
    """SCPS.dual of the oracle's run of problem b at horizon N (read-only)"""
    x0, glo, ghi, tf = base(model, b + 1)
    o = _scp(model, N)
    o.set_problem(x0[b], glo[b], ghi[b], tf[b])
    d = o.solve(30)["dual"].copy()
    d.setflags(write=False)
    return d


def duals(model, N, bs):
    return np.stack([dual(model, N, int(b)) for b in bs])


# ---- roll-out ------------------------------------------------------------------------------------------------------------
ROLLOUT = [(DUB, 1, 3, 1, "default"), (DUB, 33, 4, 4, "default"), (DUB, 65, 30, 7, "default"), (DUB, 31, 256, 2, "default"),
           (DUB, 33, 4, 4, "nondefault"), (DUB, 65, 30, 7, "nondefault"),
           (MAN, 1, 3, 4, "default"), (MAN, 3, 3, 4, "default"), (MAN, 33, 5, 1, "default"), (MAN, 65, 50, 4, "default"), (MAN, 5, 256, 2, "default"),
           (MAN, 33, 5, 1, "nondefault"), (MAN, 65, 50, 4, "nondefault")]


def case_id(c):
    return "-".join([NAME[c[0]]] + [str(v) for v in c[1:]])


def capped(model, d):
    """the duals, each scaled down by one factor until |p0_i| <= SEED_CAP_i for every i (a non-finite dual stays what it is)"""
    a = (np.abs(d) / SEED_CAP[model]).max(axis=-1, keepdims=True)
    with np.errstate(all="ignore"):
        return np.where(a > 1, d / a, d)


@functools.lru_cache(maxsize=None)
def rollout(case):
    model, B, N, substeps, pcase = case
    n = NS.DIMS[model][0]
    x0, glo, ghi, tf = base(model, B)
    p0 = capped(model, duals(model, N, range(B)))
    if B > 1:            # a box goal: lo < hi on every coordinate, the centre 0.05 (1 + i) / n above the point goal
        w = 0.1 * (1 + np.arange(n)) / n
        glo[1], ghi[1] = glo[1] - w, ghi[1] + 2 * w
    if B > 2:            # one coordinate without a goal
        glo[2, 1], ghi[2, 1] = -np.inf, np.inf
    if B >= 33:
        p0[NAN_PROBLEM, 1] = np.nan
    return _frozen(Inputs(model, N, substeps, ROLL_OPTS["max_newton"], ROLL_OPTS["ftol"], x0, glo, ghi, tf, p0, pcase))


def _frozen(inp):
    for a in inp:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return inp


# ---- one Newton step -----------------------------------------------------------------------------------------------------
ONE_STEP = [(model, N, substeps) for model, Ns in ((DUB, (5, 30)), (MAN, (5, 12))) for N in Ns for substeps in (1, 4)]
ONE_STEP_B = 8


@functools.lru_cache(maxsize=None)
def one_step(case):
    model, N, substeps = case
    x0, glo, ghi, tf = base(model, ONE_STEP_B)
    return _frozen(Inputs(model, N, substeps, 1, 1e-3, x0, glo, ghi, tf, duals(model, N, range(ONE_STEP_B)), "default"))


# ---- stragglers ----------------------------------------------------------------------------------------------------------
# (problem, scale) per member; what the oracle does with each is in tests/test_shoot_cpu.py and profiles/shoot_tests.txt
STRAGGLERS = {
    DUB: dict(N=5, substeps=4, ftol=1e-3, members=((0, 0.3), (3, 1), (6, 0.6), (5, 1.5), (2, 1), (6, 1), (9, 1), (13, 0.3),
                                                     (5, 1), (3, 1.5), (9, 0.3), (15, 0.6), (13, 1))),
    MAN: dict(N=5, substeps=1, ftol=6e-4, members=((3, 0.6), (1, 1), (5, 1), (4, 1), (6, 1), (0, 1.5), (11, 0.6), (12, 1),
                                                     (2, 0.3), (8, 0.3), (3, 3), (12, 3))),
}
SHOOT_CAP = 8        # Newton steps of the lane-per-problem pass (csrc/shoot.hip)


@functools.lru_cache(maxsize=None)
def stragglers(model, max_newton=100):
    S = STRAGGLERS[model]
    bs = np.array([b for b, _ in S["members"]])
    sc = np.array([s for _, s in S["members"]], dtype=float)
    x0, glo, ghi, tf = (a[bs] for a in base(model, int(bs.max()) + 1))
    p0 = sc[:, None] * duals(model, S["N"], bs)
    return _frozen(Inputs(model, S["N"], S["substeps"], max_newton, S["ftol"], x0, glo, ghi, tf, p0, "default"))


# ---- both sides ----------------------------------------------------------------------------------------------------------
def oracle_shoot(inp):
    """the oracle's go_shoot of every problem of the inputs: [dict]"""
    o = go.Oracle(inp.model, inp.N, model_params=model_params(go, inp.model, inp.pcase))
    out = []
    for b in range(len(inp.tf)):
        o.set_problem(inp.x0[b], inp.glo[b], inp.ghi[b], inp.tf[b])
        out.append(o.shoot(p0=inp.p0[b], substeps=inp.substeps, max_newton=inp.max_newton, ftol=inp.ftol))
    return out


def restated(inp, dtype=np.float64):
    """tests/np_shoot.py on every problem of the inputs: [dict]"""
    pr = par(inp.model, inp.pcase)
    return [NS.shoot(inp.model, inp.x0[b], inp.p0[b], inp.glo[b], inp.ghi[b], inp.tf[b], inp.N, inp.substeps, inp.max_newton,
                     inp.ftol, pr, dtype) for b in range(len(inp.tf))]


def extremal(inp, p0, dtype=np.longdouble):
    """the restated extremals of every problem of the inputs from p0 [B, n]: X [B, N, n], U [B, N, m]"""
    return NS.extremal(inp.model, inp.x0, p0, inp.tf, inp.N, inp.substeps, par(inp.model, inp.pcase), dtype)


def rel_err(a, ref):
    """largest |a - ref| / max(1, |ref|) over the entries where ref is finite"""
    ref = np.asarray(ref)
    a = np.asarray(a, ref.dtype)
    fin = np.isfinite(ref)
    if not fin.any():
        return 0.0
    with np.errstate(all="ignore"):
        e = np.abs(a - ref)[fin] / np.maximum(1, np.abs(ref[fin]))
    return float(np.nan_to_num(e, nan=np.inf).max())


def rel_inf(a, ref):
    """|a - ref|_inf / max(1, |ref|_inf)"""
    return float(np.abs(np.asarray(a) - np.asarray(ref)).max() / max(1.0, np.abs(ref).max()))


def tol_from(figure):
    """100 x the figure, rounded up to a power of ten"""
    return 10.0 ** int(np.ceil(np.log10(100 * figure)))
