"""tests/np_tvlqr.py, the numpy restatement the GPU tests of gusto_tvlqr compare against, pinned without a GPU: the roll-out
Jacobians in closed form where one exists, the recursion against the algebraic Riccati equation and against the quadratic
program it solves; then the declarations (header, library, Julia mirror) and the export of the gains."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import scipy.linalg

import gusto_jl_amd as g
import np_models as M
import np_tvlqr as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["gusto_default_tvlqr_opts", "gusto_tvlqr", "gusto_get_tvlqr", "gusto_last_tvlqr_ms"]


@pytest.mark.parametrize("nstep", [1, 3, 8])
def test_freeflyer_rollout_jacobians_in_closed_form(nstep):
    """freeflyerSE2 is a double integrator: RK4 under a held control is exact for any nstep, so Ad = [[I, dt I], [0, I]] and
    Bd = [[dt^2 / 2 Bv], [dt Bv]], Bv = diag(1/m, 1/m, 1/J)."""
    Mo = M.FreeflyerSE2
    X, U = T.smooth_batch(0, 1, 5)
    tf = 7.3
    dt = tf / 4
    AB = T.linearise(0, X[0], U[0], tf, nstep=nstep)
    Bv = np.diag([1 / Mo.mass, 1 / Mo.mass, 1 / Mo.J[2]])
    Ad = np.block([[np.eye(3), dt * np.eye(3)], [np.zeros((3, 3)), np.eye(3)]])
    Bd = np.vstack([0.5 * dt * dt * Bv, dt * Bv])
    for k in range(4):
        assert np.abs(AB[k, :, :6] - Ad).max() <= 1e-14 * dt
        assert np.abs(AB[k, :, 6:] - Bd).max() <= 1e-14 * np.abs(Bd).max()


def test_long_lti_horizon_approaches_the_algebraic_riccati_solution():
    """freeflyerSE2 (time invariant): P of knot 1 of a long horizon is the stabilising solution of the discrete algebraic
    Riccati equation, and the first gain its gain."""
    N, tf = 400, 399.0
    X, U = T.smooth_batch(0, 1, N)
    Q, R, Qf = T.weights(0)
    AB, K, P = T.tvlqr(0, X[0], U[0], tf, Q, R, Qf, nstep=1)
    A, B = AB[0, :, :6], AB[0, :, 6:]
    Pinf = scipy.linalg.solve_discrete_are(A, B, np.diag(Q), np.diag(R))
    assert np.abs(P[0] - Pinf).max() <= 1e-9 * np.abs(Pinf).max()
    Kinf = np.linalg.solve(np.diag(R) + B.T @ Pinf @ B, B.T @ Pinf @ A)
    assert np.abs(K[0] - Kinf).max() <= 1e-9 * np.abs(Kinf).max()
    assert np.abs(np.linalg.eigvals(A - B @ K[0])).max() < 1.0


@pytest.mark.parametrize("model", [0, 1, 2, 3])
def test_two_stage_recursion_is_the_optimum_of_the_quadratic_program(model):
    """N = 3: x1' P_1 x1 = min over (u1, u2) of x1'Q x1 + u1'R u1 + x2'Q x2 + u2'R u2 + x3'Qf x3 along x2 = A1 x1 + B1 u1,
    x3 = A2 x2 + B2 u2 -- solved here as ONE dense least-squares problem in (u1, u2), no recursion."""
    n, m = g.MODEL_DIMS[model]
    X, U = T.smooth_batch(model, 1, 3)
    Q, R, Qf = T.weights(model)
    AB, K, P = T.tvlqr(model, X[0], U[0], 2.0, Q, R, Qf, nstep=2)
    A1, B1, A2, B2 = AB[0, :, :n], AB[0, :, n:], AB[1, :, :n], AB[1, :, n:]
    sQ, sR, sQf = np.diag(np.sqrt(Q)), np.diag(np.sqrt(R)), np.diag(np.sqrt(Qf))
    Z = np.zeros
    # residual rows: sqrt(Q) x1, sqrt(R) u1, sqrt(Q) x2, sqrt(R) u2, sqrt(Qf) x3 as Cx x1 + Mu [u1; u2]
    Cx = np.vstack([sQ, Z((m, n)), sQ @ A1, Z((m, n)), sQf @ A2 @ A1])
    Mu = np.vstack([Z((n, 2 * m)), np.hstack([sR, Z((m, m))]), np.hstack([sQ @ B1, Z((n, m))]), np.hstack([Z((m, m)), sR]),
                    np.hstack([sQf @ A2 @ B1, sQf @ B2])])
    Us = np.linalg.lstsq(Mu, -Cx, rcond=None)[0]
    res = Cx + Mu @ Us
    V = res.T @ res
    assert np.abs(P[0] - V).max() <= 1e-10 * np.abs(V).max()
    assert np.abs(K[0] + Us[:m]).max() <= 1e-9 * max(1.0, np.abs(K[0]).max())      # u1 = -K_1 x1


def test_complex_step_jacobians_against_central_differences():
    """the complex step through the whole roll-out against central differences of the same map (1e-6 relative: what a central
    difference with a 1e-6 step can show), every model"""
    for model in (1, 2, 3):
        X, U = T.smooth_batch(model, 1, 4)
        n, m = g.MODEL_DIMS[model]
        dt, ns = 0.8, 3
        AB = T.jacobians(model, X[0, 1], U[0, 1], dt, ns)
        z0 = np.concatenate([X[0, 1], U[0, 1]])
        for j in range(n + m):
            e = np.zeros(n + m); e[j] = 1e-6
            fp = T.rollout(T.MODELS[model], (z0 + e)[:n], (z0 + e)[n:], dt, ns)
            fm = T.rollout(T.MODELS[model], (z0 - e)[:n], (z0 - e)[n:], dt, ns)
            assert np.abs((fp - fm) / 2e-6 - AB[:, j]).max() <= 1e-6 * max(1.0, np.abs(AB).max())


def test_column_batched_linearisation_is_the_per_column_one():
    """np_tvlqr.linearise runs the perturbed roll-outs of the array-safe models side by side: the same numbers as one
    complex-step roll-out per column"""
    for model in (0, 1, 3):
        X, U = T.smooth_batch(model, 1, 5)
        AB = T.linearise(model, X[0], U[0], 3.0, nstep=2)
        for k in range(4):
            one = T.jacobians(model, X[0, k], U[0, k], 0.75, 2)
            assert np.abs(AB[k] - one).max() <= 1e-15 * np.abs(one).max()


def test_library_declares_and_exports_the_tvlqr_entry_points():
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    L = g.lib()
    for s in NEW_SYMBOLS:
        assert s in g._capi.SYMBOLS and re.search(r"\bint %s\(" % s, hdr) and hasattr(L, s), s
    assert "No counterpart in the reference" in hdr[hdr.index("Time-varying LQR"):hdr.index("} gusto_tvlqr_opts;")]
    # the calls that need no device
    for model, (n, m) in g.MODEL_DIMS.items():
        o = g.default_tvlqr_opts(model)
        assert list(o.Q) == [1.0] * n + [0.0] * (13 - n) and list(o.Qf) == list(o.Q) and list(o.R) == [1.0] * m + [0.0] * (6 - m)
        assert (o.dt_min, o.nstep, o.nstep_cap, o.store_P) == (0.1, 0, 64, 0)
    assert L.gusto_default_tvlqr_opts(9, C.byref(g.TvlqrOpts())) == -1 and L.gusto_default_tvlqr_opts(0, None) == -1
    assert L.gusto_tvlqr(None, None, None, None) == -1
    assert L.gusto_get_tvlqr(None, None, None, None, None, None) == -1
    assert L.gusto_last_tvlqr_ms(None, None) == -1
    assert C.sizeof(g.TvlqrOpts) == (13 + 6 + 13 + 1) * 8 + 3 * 4 + 4


def test_julia_mirror_of_the_tvlqr_options():
    """GustoTvlqrOpts has the header's fields in the header's order and types; tvlqr_batch! calls the three entry points"""
    jl = open(os.path.join(ROOT, "gusto.jl_amd", "julia", "GuSTOHIPBatch.jl")).read()
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    end = hdr.index("} gusto_tvlqr_opts;")
    body = re.sub(r"/\*.*?\*/", "", hdr[hdr.rindex("typedef struct {", 0, end) + len("typedef struct {"):end], flags=re.S)
    cf = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, rest = decl.split(None, 1)
        for v in rest.split(","):
            v = v.strip()
            dim = re.search(r"\[(\w+)\]", v)
            base = {"double": "Cdouble", "int": "Cint"}[ctype]
            cf.append((re.sub(r"\[.*", "", v), "NTuple{%d,%s}" % ({"GUSTO_MAXN": 13, "GUSTO_MAXM": 6}[dim.group(1)], base) if dim else base))
    jbody = re.search(r"struct GustoTvlqrOpts\b[^\n]*\n(.*?)\nend", jl, re.S).group(1)
    jf = [tuple(s.strip() for s in f.split("::")) for f in re.split(r"[;\n]", re.sub(r"#[^\n]*", "", jbody)) if f.strip()]
    assert cf == jf, (cf, jf)
    assert [n for n, _ in cf] == ["Q", "R", "Qf", "dt_min", "nstep", "nstep_cap", "store_P"]
    fn = jl[jl.index("function tvlqr_batch!"):]
    for s in ("gusto_tvlqr", "gusto_get_tvlqr", "gusto_last_tvlqr_ms"):
        assert "ccall((:%s, libgusto_hip)" % s in fn, s


def test_export_writes_the_gains_next_to_the_trajectory(tmp_path):
    """export.write(..., K=): traj/k_traj [N-1][m][n] in all three formats; without K the tree has no such entry"""
    import h5read
    E = g.export
    X, U = T.smooth_batch(0, 2, 6)
    K = np.arange(2 * 5 * 3 * 6, dtype=float).reshape(2, 5, 3, 6)
    tf = np.array([10.0, 12.0])
    for ext in (".npz", ".mat"):
        p = str(tmp_path / ("k" + ext))
        E.write(p, 0, X, U, tf, K=K)
        assert np.array_equal(E.read(p)["traj"]["k_traj"], K)
        E.write(p, 0, X, U, tf)
        assert "k_traj" not in E.read(p)["traj"]
    p = str(tmp_path / "k.h5")
    tree = E.write(p, 0, X[0], U[0], 10.0, K=K[0])
    assert np.array_equal(tree["traj"]["k_traj"], K[0])
    assert np.array_equal(np.asarray(h5read.read_h5(p)["traj"]["k_traj"]).reshape(5, 3, 6), K[0])
    assert "k_traj" not in E.write(p, 0, X[0], U[0], 10.0)["traj"]
    with pytest.raises(ValueError):
        E.write(p, 0, X[0], U[0], 10.0, K=K[0][:4])
