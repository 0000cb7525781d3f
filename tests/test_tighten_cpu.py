"""gusto_tighten_env without a GPU: the guarantee of include/gusto_hip.h on random geometry, the numpy restatement
(tests/np_tighten.py) in float64 against itself in long double on the shared inputs (tests/tighten_cases.py), the conditioning of
those inputs -- every exactly compared index rests on decisions at least GAP from flipping, and every option set makes its rule
decide something --, the ctypes layer's struct, and the Julia wrapper's symbols."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import gusto_jl_amd as g
import lincov_cases as LC
import np_models as M
import np_tighten as NT
import np_verify as V
import tighten_cases as TC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_KNOT = 1e-13    # tests/test_gpu_lincov.py (profiles/lincov.txt): ten times the formulas' own fp64 error at the knots, rounded up


def rel(a, ref):
    a, ref = np.asarray(a, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    if np.array_equal(a, ref):      # (+-inf included)
        return 0.0
    nrm = np.abs(ref).max() if ref.size else 0.0
    err = np.abs(a - ref).max() if ref.size else 0.0
    return float(err / nrm) if nrm > 0 else float(err)


@pytest.mark.parametrize("model", TC.MODELS)
def test_guarantee_on_random_geometry(model):
    """for every location q and robot component c: the component-0 distance of q to the tightened component is at most the
    component-c distance to the base component minus the margin.  Coordinates within +-4: a handful of roundings at that scale,
    1e-14 absolute (8.9e-16 was measured on 20 000 boxes)."""
    rng = np.random.default_rng(1234 + model)
    ws, r = V.WS_DIM[model], V.MODELS[model].r
    comps = [V.COMPONENTS[model], np.vstack([np.zeros(ws), rng.uniform(-0.3, 0.3, size=(1, ws))])]   # the model's, and a random arm
    worst = -np.inf
    for offs in comps:
        for _ in range(3000):
            lo = rng.uniform(-4, 3.5, size=3)
            hi = lo + rng.uniform(0.01, 0.5 + 3.5 * rng.uniform(), size=3)
            hi = np.minimum(hi, 4.0)
            sph = np.concatenate([rng.uniform(-4, 4, size=3), [rng.uniform(0.01, 1.0)]])
            q = rng.uniform(-4, 4, size=ws)
            if rng.uniform() < 0.5:      # near or inside the box
                q = lo[:ws] + (hi - lo)[:ws] * rng.uniform(-0.3, 1.3, size=ws)
            m = rng.uniform(0, 0.3)
            off = offs - offs[0]
            omax, omin = np.maximum(off.max(axis=0), 0), np.minimum(off.min(axis=0), 0)
            tb = np.concatenate([lo, hi])
            tb[:ws] = (lo[:ws] - omax) - m
            tb[3:3 + ws] = (hi[:ws] - omin) + m
            tc = sph.copy()
            tc[:ws] = sph[:ws] - 0.5 * (omax + omin)
            tc[3] = (sph[3] + np.sqrt(np.sum((0.5 * (omax - omin)) ** 2))) + m
            d0b = M.sd_box(q + offs[0], tb[0:3], tb[3:6], r)[0]
            d0s = M.sd_sphere(q + offs[0], tc[0:3], tc[3], r)[0]
            for c in range(len(offs)):
                worst = max(worst, d0b - (M.sd_box(q + offs[c], lo, hi, r)[0] - m), d0s - (M.sd_sphere(q + offs[c], sph[0:3], sph[3], r)[0] - m))
    print(f"model {model}: worst excess {worst:.3g}")
    assert worst <= 1e-14


def test_np_tighten_matches_its_own_cover_for_the_models_offsets():
    """np_tighten.cover_offsets / tightened on the committed component offsets: freeflyerSE2's arm at (0, 0.15)"""
    omax, omin = NT.cover_offsets(0)
    assert np.array_equal(omax, [0.0, 0.15]) and np.array_equal(omin, [0.0, 0.0])
    for model in (2, 3):
        assert not np.any(NT.cover_offsets(model)[0]) and not np.any(NT.cover_offsets(model)[1])
    box, sph = np.array([[1.0, 2.0, -0.2, 1.5, 2.5, 0.2]]), np.array([[0.5, 0.5, 0.1, 0.2]])
    tb, ts = NT.tightened(0, box, sph, [0.1, 0.2])
    assert np.array_equal(tb[0], [1.0 - 0.1, (2.0 - 0.15) - 0.1, -0.2, 1.5 + 0.1, 2.5 + 0.1, 0.2])
    assert np.array_equal(ts[0], [0.5, 0.5 - 0.075, 0.1, (0.2 + 0.075) + 0.2])
    tb, ts = NT.tightened(0, box, sph, [0.0, 0.0], cover=0)
    assert np.array_equal(tb, box) and np.array_equal(ts, sph)       # cover off, no margin: the base bit for bit


@pytest.mark.parametrize("model,N", TC.CASES)
def test_float64_against_long_double_and_decision_gaps(model, N):
    """margins, tables, min_z_base and max_margin of the float64 restatement against the long double one within TOL_KNOT relative
    to the coordinate scale, and every exactly compared index (knot, pair, blocked, n_grown) at least GAP from flipping"""
    X, _, _, _ = LC.inputs(model, N)
    x0, glo, _ = TC.problems(model, N)
    for env in TC.ENVS:
        sets, _ = LC.env(model, env)
        for st in TC.STARTS:
            for name, o in TC.OPTION_SETS.items():
                if env != "batch" and name not in ("default", "reach"):
                    continue
                r64 = TC.reference(model, N, env, st, **o)
                rld = TC.reference(model, N, env, st, dtype=np.longdouble, **o)
                for b in range(TC.B):
                    where = (model, N, env, st, name, b)
                    for f in ("knot", "pair", "blocked", "n_grown", "status"):
                        assert r64[b][f] == rld[b][f], (where, f)
                    scale = max(1.0, np.abs(X[b][:, :V.WS_DIM[model]]).max())
                    for f in ("margin", "boxes", "spheres", "max_margin"):
                        err = np.abs(np.asarray(r64[b][f], np.longdouble) - rld[b][f]).max() if np.size(r64[b][f]) else 0.0
                        assert err <= TOL_KNOT * scale, (where, f, err)
                    assert rel([r64[b]["min_z_base"]], [rld[b]["min_z_base"]]) <= TOL_KNOT, where
                    gap = TC.decision_gap(model, X[b], rld[b], sets[b][0], sets[b][1], x0[b], glo[b], **o)
                    assert gap >= TC.GAP, (where, gap)


def test_every_option_rule_decides_something():
    """on the restatement: each option set differs from the default where its rule is meant to bite"""
    for model in TC.MODELS:
        d = TC.reference(model, 50, "batch", "full")
        reach = TC.reference(model, 50, "batch", "full", **TC.OPTION_SETS["reach"])
        slack = TC.reference(model, 50, "batch", "full", **TC.OPTION_SETS["slack"])
        sr = TC.reference(model, 50, "batch", "full", **TC.OPTION_SETS["slack_reach"])
        cap = TC.reference(model, 50, "batch", "full", **TC.OPTION_SETS["cap"])
        noc = TC.reference(model, 50, "batch", "full", **TC.OPTION_SETS["nocover"])
        big = TC.reference(model, 50, "batch", "full", **TC.OPTION_SETS["big"])
        k0 = TC.reference(model, 50, "batch", "full", **TC.OPTION_SETS["kappa0"])
        b = 4                                                            # 64 components
        assert d[b]["n_grown"] == 64 and len(set(d[b]["margin"])) > 1    # a full start: the margins differ between components
        assert 0 < reach[b]["n_grown"] < 64                              # the far spheres are out of reach
        assert (slack[b]["margin"] < d[b]["margin"]).all() and (slack[b]["margin"] > 0).all()
        if model == 0:                                                   # the slack takes all of some margins that are within reach
            assert 0 < sr[b]["n_grown"] < reach[b]["n_grown"]
        assert (cap[b]["margin"] == 0.01).all() and d[b]["max_margin"] > 0.01
        assert k0[b]["n_grown"] == 0 and k0[b]["min_z_base"] == d[b]["min_z_base"]
        assert any(r["blocked"] for r in big) and not any(r["blocked"] for r in d)
        if model == 0:                                                   # the only model with a second component
            assert not np.array_equal(noc[b]["boxes"], d[b]["boxes"]) and np.array_equal(noc[b]["margin"], d[b]["margin"])
        else:
            assert np.array_equal(noc[b]["boxes"], d[b]["boxes"])
        # monotone across two calls: the smaller kappa's margins are smaller, so monotone = 1 keeps the first call's
        prev = [r["margin"] for r in d]
        keep = TC.reference(model, 50, "batch", "full", prev=prev, **TC.SECOND)
        drop = TC.reference(model, 50, "batch", "full", prev=prev, monotone=0, **TC.SECOND)
        assert np.array_equal(keep[b]["margin"], d[b]["margin"]) and (drop[b]["margin"] < d[b]["margin"]).all()
        # a skipped problem keeps its margins and still gets its tables
        sk = TC.reference(model, 50, "batch", "full", prev=prev, skipped=[0, 0, 0, 0, 1], **TC.SECOND)
        assert sk[b]["status"] == 0 and np.array_equal(sk[b]["margin"], d[b]["margin"]) and np.array_equal(sk[b]["boxes"], d[b]["boxes"])


def test_ctypes_struct_matches_the_header():
    hdr = open(os.path.join(ROOT, "include", "gusto_hip.h")).read()
    body = hdr[:hdr.index("} gusto_tighten_opts;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {") + len("typedef struct {"):], flags=re.S)
    fields = [(d.split()[1], d.split()[0]) for d in body.split(";") if d.strip()]
    ctype = {"double": C.c_double, "int": C.c_int}
    assert [(k, ctype[t]) for k, t in fields] == list(g._capi.TightenOpts._fields_)
    body = hdr[:hdr.index("} gusto_tighten_report;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {") + len("typedef struct {"):], flags=re.S)
    names = [v.strip().lstrip("*") for d in body.split(";") if d.strip() for v in d.strip().split(None, 1)[1].split(",")]
    assert names == [k for k, _, _ in g._capi.TIGHTEN_FIELDS]
    o = g._capi.default_tighten_opts(0)
    assert (o.kappa, o.slack, o.margin_cap, o.reach, o.cover_components, o.monotone) == (3.0, 0.0, np.inf, np.inf, 1, 1)
    with pytest.raises(ValueError):
        g._capi.default_tighten_opts(9)


def test_julia_wrapper_calls_the_new_symbols():
    jl = open(os.path.join(ROOT, "gusto.jl_amd", "julia", "GuSTOHIPBatch.jl")).read()
    for s in ("gusto_tighten_env", "gusto_get_tighten", "gusto_get_env", "gusto_last_tighten_ms"):
        assert re.search(r"ccall\(\(:%s, libgusto_hip\)" % s, jl), s
    assert "function tighten_env!" in jl and "function solve_SCP_chance_batch!" in jl


def test_driver_refuses_a_covariance_without_noise():
    H = g.host
    with pytest.raises(ValueError, match="du_white"):
        H.solve_SCP_chance_batch([None], [None], lincov_opts=dict(dx0=0.02))
