"""Batched post-solve verification (gusto_verify / gusto_interpolate), the part that needs no GPU: the numpy restatement the
GPU tests compare against (tests/np_verify.py) is held against the CPU oracle and against closed forms, the inputs of the GPU
tests are shown to sit away from the zero crossing of the signed distance, and the new entry points are checked at the
boundary (exports, argument checks that run before any device call, the Julia mirrors of the new structs)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gusto_jl_amd as g
import gusto_oracle as go
import np_models as M
import np_verify as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = g.problems
N = 50

# first= of the generators for the GPU tests' 256-problem batches (condition (c) below holds for these; none had to be moved)
FIRST = {g.FREEFLYER_SE2: 0, g.ASTROBEE_SE3: 0, g.ASTROBEE_SE3_MANIFOLD: 0}


def batch(model, B, first=0):
    """(x_init, goal_lo, goal_hi, tf, boxes, spheres) of the generator batch of a model"""
    if model == g.FREEFLYER_SE2:
        return P.freeflyer_batch(B, first) + (P.freeflyer_env(), None)
    if model == g.DUBINS_CAR:
        return P.dubins_batch(B, first) + (None, None)
    gen = P.astrobee_se3_batch if model == g.ASTROBEE_SE3 else P.astrobee_manifold_batch
    return gen(B, first) + P.iss_corner_env()


def straight_line(model, x0, glo, ghi, n_knots=N):
    """init_traj_straightline (freeflyer_se2.jl:97-111): LinRange from x_init to the goal's centre, zero controls"""
    n, m = g.MODEL_DIMS[model]
    xg = np.where(np.isfinite(glo) & np.isfinite(ghi), 0.5 * (glo + ghi), 0.0)
    t = (np.arange(n_knots) / (n_knots - 1))[None, :, None]
    return (1 - t) * x0[:, None, :] + t * xg[:, None, :], np.zeros((len(x0), n_knots, m))


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_np_verify_agrees_with_the_oracle_on_straight_line_inits(model):
    """(a) f and the signed distances np_verify is built on, against Oracle.dynamics / Oracle.signed_distance to 1e-12 at every
    knot of the straight-line inits of 64 generator problems; dist_many (the array form used for the dense samples) against the
    one-by-one sd_box / sd_sphere calls."""
    B = 64
    x0, glo, ghi, tf, boxes, spheres = batch(model, B)
    bx, sp = V.obstacles(boxes, spheres)
    o = go.Oracle(model, N, boxes=boxes, spheres=spheres)
    rng = np.random.default_rng(5)
    for b in range(B):
        o.set_problem(x0[b], glo[b], ghi[b], tf[b])
        X, U = o.init_straightline()
        Xs, Us = straight_line(model, x0[b:b + 1], glo[b:b + 1], ghi[b:b + 1])
        assert np.abs(Xs[0] - X).max() < 1e-14 and not U.any()
        Ur = rng.uniform(-0.1, 0.1, U.shape)               # (the init has zero controls: exercise the control terms as well)
        F = V.f_cols(model, X, Ur)
        for k in range(N):
            fo = o.dynamics(X[k], Ur[k])[0]
            assert np.abs(V.MODELS[model].f(X[k], Ur[k]) - fo).max() < 1e-12
            assert np.abs(F[k] - fo).max() < 1e-12
        if model == g.DUBINS_CAR:
            continue
        D = V.knot_distances(model, X, bx, sp)
        for c in range(D.shape[0]):
            for i in range(D.shape[1]):
                for k in range(0, N, 7):
                    assert abs(D[c, i, k] - o.signed_distance(c, X[k, :V.WS_DIM[model]], i)[0]) < 1e-12, (b, c, i, k)
        assert D.shape[0] == o.mp.n_robot_comp
        assert np.abs(V.dist_many(model, X, bx, sp) - D.min(axis=(0, 1))).max() < 1e-14


def test_freeflyer_constant_control_rolls_out_to_the_exact_quadratic():
    """(b) freeflyerSE2 is a double integrator: under a held control RK4 is exact, r(t) = r0 + v0 t + a t^2 / 2."""
    Mo = M.FreeflyerSE2
    Nk, tf = 6, 10.0
    dt = tf / (Nk - 1)
    u = np.array([0.3, -0.2, 0.01])
    a = np.array([u[0] / Mo.mass, u[1] / Mo.mass, u[2] / Mo.J[2]])
    x0 = np.array([0.5, 0.7, 0.1, 0.02, -0.01, 0.003])
    t = dt * np.arange(Nk)[:, None]
    X = np.hstack([x0[:3] + x0[3:] * t + 0.5 * a * t * t, x0[3:] + a * t])
    U = np.tile(u, (Nk, 1))
    Xf, Uf, gap = V.interpolate_traj(0, X, U, tf, dt_min=0.1)
    ns = V.n_substeps(tf, Nk, 0.1)
    assert ns == 20 and Xf.shape == (ns * (Nk - 1) + 1, 6) and Uf.shape == (ns * (Nk - 1), 3)
    tt = (dt / ns) * np.arange(len(Xf))[:, None]
    exact = np.hstack([x0[:3] + x0[3:] * tt + 0.5 * a * tt * tt, x0[3:] + a * tt])
    assert np.abs(Xf - exact).max() < 1e-13 and gap < 1e-13
    assert np.array_equal(Uf, np.tile(u, (len(Xf) - 1, 1))) and np.array_equal(Xf[-1], X[-1])
    # fixed substep count
    assert V.interpolate_traj(0, X, U, tf, nstep=3)[0].shape[0] == 3 * (Nk - 1) + 1


def test_first_hit_follows_the_obstacle_major_order():
    """(b) a straight line that runs through two boxes: the reference loops obstacles outside knots, so the hit it returns is the
    first penetrating knot of the FIRST obstacle in table order, although the second obstacle is met at an earlier knot."""
    Nk = 21
    X = np.zeros((Nk, 12))
    X[:, 0] = np.linspace(0.0, 10.0, Nk)                  # knots every 0.5 m along x
    boxes = np.array([[7.0, -1, -1, 8.0, 1, 1], [2.0, -1, -1, 3.0, 1, 1]])     # table order: the far slab first
    r = M.Astrobee.r
    free, k, d = V.verify_collision_free(2, X, boxes, None)
    k_first = int(np.argmax(X[:, 0] > 7.0 - r)) + 1       # first knot (1-based) whose sphere reaches into the far slab
    assert (free, k) == (False, k_first) and abs(d - ((7.0 - X[k - 1, 0]) - r)) < 1e-15 and d < 0
    assert V.verify_collision_free(2, X, boxes[::-1], None)[1] == int(np.argmax(X[:, 0] > 2.0 - r)) + 1
    assert V.verify_collision_free(2, X[:3], boxes, None) == (True, 0, 0.0)
    rep = V.report(2, X, np.zeros((Nk, 6)), 20.0, boxes, None)
    assert rep["min_dist_knots"] == -0.5 - r and rep["first_knot"] == k_first          # a knot in the middle of a 1 m slab
    # through a table slab of the freeflyer's workspace: the body's disc reaches the x = 12 ft wall first
    Xf = np.zeros((Nk, 6))
    Xf[:, 0] = np.linspace(3.0, 4.0, Nk); Xf[:, 1] = 1.0
    free, k, d = V.verify_collision_free(0, Xf, P.table_stanford_boxes(), None)
    wall = 12.0 * P.FT2M
    assert not free and k == int(np.argmax(Xf[:, 0] + M.FreeflyerSE2.r > wall)) + 1 and d < 0


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_defect_of_an_exact_euler_trajectory_is_zero(model):
    """(b) x_{k+1} = x_k + dt f(x_k, u_k): dynamics_constraint_satisfaction is zero to rounding."""
    rng = np.random.default_rng(11)
    n, m = g.MODEL_DIMS[model]
    Nk, tf = 12, 6.0
    dt = tf / (Nk - 1)
    X, U = np.zeros((Nk, n)), rng.uniform(-0.05, 0.05, (Nk, m))
    X[0] = rng.uniform(-0.2, 0.2, n)
    if model == 3:
        X[0, 6:10] = [1, 0, 0, 0]
    for k in range(Nk - 1):
        X[k + 1] = X[k] + dt * V.MODELS[model].f(X[k], U[k])
    assert V.dynamics_constraint_satisfaction(model, X, U, tf) < 1e-13
    X[5, 0] += 0.1                                          # ... and it sees a knot that is moved: 0.1 / dt on either side
    assert abs(V.dynamics_constraint_satisfaction(model, X, U, tf) - 2 * 0.1 / dt) < 1e-9


@pytest.mark.parametrize("model", [0, 2, 3])
def test_input_condition_of_the_gpu_tests(model):
    """(c) on the straight-line inits of the 256-problem generator batches the reference's own smallest distances, over the knots
    and over the dense samples, stay further than 1e-6 from zero for every problem: the flag and index fields of the GPU
    comparison cannot hinge on the last digits of a distance."""
    B = 256
    x0, glo, ghi, tf, boxes, spheres = batch(model, B, FIRST[model])
    Xs, Us = straight_line(model, x0, glo, ghi)
    worst = np.inf
    for b in range(B):
        r = V.report(model, Xs[b], Us[b], tf[b], boxes, spheres)
        worst = min(worst, abs(r["min_dist_knots"]), abs(r["min_dist_dense"]))
        assert abs(r["min_dist_knots"]) > 1e-6 and abs(r["min_dist_dense"]) > 1e-6, (b, r["min_dist_knots"], r["min_dist_dense"])
    print(f"model {model}: smallest |min distance| of the batch {worst:.3e}")


@pytest.mark.parametrize("model", [0, 2, 3])
def test_solved_trajectories_rarely_sit_on_the_zero_crossing(model):
    """The GPU test of solved trajectories leaves a problem's flags out when its reference |min distance| is below 1e-9 and
    allows 1 % of such problems.  The oracle's solves of the head of each generator batch: a solved trajectory keeps the
    clearance (0.05 / 0.03 m) at its knots, so its distances are nowhere near zero unless the solve failed."""
    B = 12 if model == 0 else 6
    x0, glo, ghi, tf, boxes, spheres = batch(model, B, FIRST[model])
    o = go.Oracle(model, N, boxes=boxes, spheres=spheres)
    close = 0
    for b in range(B):
        o.set_problem(x0[b], glo[b], ghi[b], tf[b])
        r = o.solve(30)
        rep = V.report(model, r["X"], r["U"], tf[b], boxes, spheres)
        close += min(abs(rep["min_dist_knots"]), abs(rep["min_dist_dense"])) <= 1e-9
    assert close <= 0.01 * B, close


NEW_SYMBOLS = ["gusto_default_verify_opts", "gusto_verify", "gusto_get_verify", "gusto_interpolate", "gusto_get_dense",
               "gusto_last_verify_ms"]


def test_library_exports_the_verification_entry_points():
    """(d) the new symbols are in _capi.SYMBOLS, in the header and in the library; the calls that need no device answer as the
    header says."""
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    L = g.lib()
    for s in NEW_SYMBOLS:
        assert s in g._capi.SYMBOLS and hasattr(L, s) and re.search(r"\bint %s\(" % s, hdr), s
    o = g._capi.VerifyOpts()
    assert L.gusto_default_verify_opts(C.byref(o)) == 0
    assert (o.dt_min, o.nstep, o.nstep_cap, o.dense_collision) == (0.1, 0, 64, 1)
    assert L.gusto_default_verify_opts(None) == -1
    assert L.gusto_verify(None, None, None, None) == -1
    assert L.gusto_interpolate(None, None, None, None, None) == -1
    assert L.gusto_get_verify(None, None) == -1 and L.gusto_get_dense(None, None, None, None) == -1
    ms = C.c_double()
    assert L.gusto_last_verify_ms(None, C.byref(ms)) == -1
    assert "TrajOpt handles answer GUSTO_ERR_ARG" in hdr
    assert [k for k, _ in g._capi.VerifyReport._fields_] == [k for k, _ in g._capi.VERIFY_FIELDS]
    with pytest.raises(g._capi.GustoError):
        g._capi.TrajOptSolver.verify(None)


def test_julia_mirrors_of_the_verification_structs():
    """(d) GustoVerifyOpts / GustoVerifyReport have the header's fields in the header's order and types, and every function the
    Julia files ccall is declared and exported (the parser of tests/test_boundary.py)."""
    jl = "".join(open(os.path.join(ROOT, "gusto.jl_amd", "julia", f)).read() for f in ("GuSTOHIP.jl", "GuSTOHIPBatch.jl"))
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    syms = set(re.findall(r"ccall\(\(:(\w+), libgusto_hip\)", jl))
    assert {"gusto_verify", "gusto_get_verify", "gusto_interpolate", "gusto_get_dense"} <= syms
    L = g.lib()
    for s in syms:
        assert hasattr(L, s) and re.search(r"\b%s\(" % s, hdr), s

    def c_fields(name):
        end = hdr.index("} %s;" % name)
        body = hdr[hdr.rindex("typedef struct {", 0, end) + len("typedef struct {"):end]
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if not decl:
                continue
            ctype, rest = decl.split(None, 1)
            for v in rest.split(","):
                v = v.strip()
                out.append((v.lstrip("*"), ctype + ("*" if v.startswith("*") else "")))
        return out

    def jl_fields(name):
        body = re.search(r"struct %s\b[^\n]*\n(.*?)\nend" % name, jl, re.S).group(1)
        out = []
        for f in re.split(r"[;\n]", re.sub(r"#[^\n]*", "", body)):
            f = f.strip()
            if f:
                nm, ty = f.split("::")
                out.append((nm.strip(), ty.strip()))
        return out

    jl_type = {"double": "Cdouble", "int": "Cint", "double*": "Ptr{Cdouble}", "int*": "Ptr{Cint}"}
    for cname, jname, ct in (("gusto_verify_opts", "GustoVerifyOpts", g._capi.VerifyOpts),
                             ("gusto_verify_report", "GustoVerifyReport", g._capi.VerifyReport)):
        cf, jf = c_fields(cname), jl_fields(jname)
        assert [n for n, _ in cf] == [n for n, _ in jf] == [n for n, _ in ct._fields_], (cname, cf, jf)
        assert [jl_type[t] for _, t in cf] == [t for _, t in jf], (cname, cf, jf)
    assert [n for n, _ in c_fields("gusto_verify_report")] == [
        "collision_free", "first_knot", "first_dist", "min_dist_knots", "dyn_defect_l1", "min_dist_dense", "min_dense_sample",
        "max_gap"]


def test_host_mirror_keeps_the_reference_signatures():
    """host.py: interpolate_traj / verify_collision_free / dynamics_constraint_satisfaction take (traj, SCPP) like the
    reference's and need a device to run: without one they raise instead of computing on the CPU."""
    import inspect
    H = g.host
    assert list(inspect.signature(H.interpolate_traj).parameters) == ["traj", "SCPP", "dt_min"]
    assert inspect.signature(H.interpolate_traj).parameters["dt_min"].default == 0.1
    assert list(inspect.signature(H.verify_collision_free).parameters) == ["traj", "SCPP"]
    assert list(inspect.signature(H.dynamics_constraint_satisfaction).parameters) == ["traj", "SCPP"]
    assert inspect.signature(H.solve_SCP_batch).parameters["verify"].default is False
