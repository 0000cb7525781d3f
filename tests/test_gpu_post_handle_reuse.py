"""The post-solve chain on a handle larger than its batch, and across batches of changing size on one handle.

Most of the chain lays its buffers out by the handle's batch_cap and copies out by the batch B (verify.hip, simulate.hip,
lincov.hip); tvlqr.hip lays out by the batch of the call that allocated, and lincov.hip reads that back.  With batch_cap == B, as
everywhere else in the suite, all those offsets coincide.  Here: (a) a tight handle (batch_cap = B = 5) runs the chain once;
(b) a handle with batch_cap = 8 runs the same five; (c) then problems 3 and 4 only, also with gains that fail, so that a nonzero
fail_knot travels through those offsets; (d) then eight (the five, then 0, 1, 2 again: the tvlqr-side buffers grow); (e) then an
active mask on the eight with changed options.  Every stage promises that a problem's output does not depend on the batch it
sits in, so every comparison is np.array_equal, no tolerance.  (f) gusto_shoot on a handle with batch_cap = B + 3, under
test_shooting.py's own assertions (its knot-major staging depends on the batch: not bit for bit).

Inputs: tests/sim_cases.py and tests/lincov_cases.py, B = 5; models 0 and 2 at N = 50, models 1 and 3 at N = 4; the per-problem
environment of lincov_cases.env(model, "batch") where the model has obstacles."""
import functools

import numpy as np
import pytest

import gusto_jl_amd as g
import lincov_cases as LC
import sim_cases as SC
from test_shooting import check_dubins_shooting_against_the_oracle

pytestmark = pytest.mark.gpu

CASES = [pytest.param(0, 50, id="m0-N50"), pytest.param(1, 4, id="m1-N4"), pytest.param(2, 50, id="m2-N50"), pytest.param(3, 4, id="m3-N4")]
B, CAP, MODE = LC.B, 8, 2
SAMPLES = (65, 257)            # 65 generated on the device, 257 supplied by the caller
EIGHT = [0, 1, 2, 3, 4, 0, 1, 2]
TV_FIELDS = ("K", "P", "AB", "status", "fail_knot")


def _set(s, model, N, idx):
    """the problems `idx` of the batch of five, with their environments"""
    X, U, tf, _ = LC.inputs(model, N)
    idx = list(idx)
    s.set_problems(X[idx, 0], X[idx, -1], X[idx, -1], tf[idx], X[idx], U[idx])
    return X[idx], U[idx]


def _set_env(s, model, idx):
    sets, shared = LC.env(model, "batch")
    if shared:
        s.set_env(*sets[0])
    else:
        s.set_env_batch([sets[b][0] for b in idx], [sets[b][1] for b in idx])


def _sim_opts(model, S, **more):
    lo, hi = SC.bounds(model, 1)
    return dict(dict(n_samples=S, seed=SC.SEED, dx0=SC.dx0(model), du0=SC.du0(model), u_lo=lo, u_hi=hi, dense_collision=1,
                     store_knots=1, **SC.MODES[MODE]), **more)


def _chain(s, model, N, idx, generated_from=None, store_P=1, tv=None, sim=None, lc=None, stages=("verify", "tvlqr", "simulate", "lincov"),
           samples=SAMPLES):
    """the stages on the handle's problems `idx`; generated_from: first_problem of the S = 65 call (None: its perturbations are
    supplied like those of S = 257); tv, sim, lc: options that replace the defaults of a stage"""
    idx = list(idx)
    out = {}
    if "verify" in stages:
        out["verify"] = s.verify(**SC.MODES[MODE])
        out["dense"] = s.interpolate(**SC.MODES[MODE])
        out["dense_report"] = s.get_verify()
    if "tvlqr" in stages:
        Q, R, Qf = LC.WEIGHTS
        out["tvlqr"] = s.tvlqr(dict(dict(Q=Q, R=R, Qf=Qf, store_P=store_P, **SC.MODES[MODE]), **(tv or {})))
    if "simulate" in stages:
        for S in samples:
            if S == SAMPLES[0] and generated_from is not None:
                out["simulate", S] = s.simulate(_sim_opts(model, S, first_problem=generated_from, **(sim or {})))
            else:
                out["simulate", S] = s.simulate(_sim_opts(model, S, **(sim or {})), pert=SC.perturbation(model, S)[idx])
            out["knots", S] = s.get_simulate_knots()
    if "lincov" in stages:
        out["lincov"] = s.lincov(dict(LC.options(model, N, MODE, store_S=1), **(lc or {})), S0=LC.full_S0(model)[idx])
    return out


def _equal(got, want, rows, nb, what, only=None):
    """every array of every getter: nb rows, and equal to the rows `rows` of the tight reference (only: the rows of `got` looked at)"""
    rows = np.asarray(list(rows))
    pick = np.arange(nb) if only is None else np.asarray(only)

    def eq(a, b, name):
        a, b = np.asarray(a), np.asarray(b)
        assert len(a) == nb, (what, name, a.shape)
        assert np.array_equal(a[pick], b[rows][pick], equal_nan=True), (what, name)
    for key, val in got.items():
        ref = want[key]
        if key == "tvlqr":
            for f in TV_FIELDS:
                a, b = getattr(val, f), getattr(ref, f)
                eq(a, b[:, 0] if f == "P" and a.ndim == 3 and b.ndim == 4 else b, (key, f))
        elif key == "dense":
            for i, name in enumerate(("nfull", "Xfull", "Ufull")):
                eq(val[i], ref[i], (key, name))
        elif isinstance(val, dict):
            assert set(val) == set(ref), (what, key)
            for f in val:
                eq(val[f], ref[f], (key, f))
        else:
            eq(val, ref, key)


NAN_STATE = {1: 2, 2: 10, 3: 10}     # a state the Jacobians depend on: the heading, an angular rate


def _failed_gains(s, model, N, idx):
    """gusto_tvlqr fails for problem 4, then gusto_lincov on those gains: its nonzero fail_knot is written by the kernel at the
    offset tvlqr.hip derives from its buffer, read back by the getter and read by lincov.hip, each through the same expression.
    A NaN in problem 4's state at the start of the last interval (as test_gpu_tvlqr.test_failure_is_data); the Jacobians of
    freeflyerSE2 do not depend on the state, so there Q = 1e308 overflows the recursion of every problem"""
    X, U, _, _ = LC.inputs(model, N)
    idx = list(idx)
    row = idx.index(4)
    Xn = X[idx].copy()
    Q, R, Qf = LC.WEIGHTS
    if model == 0:
        Q = 1e308
    else:
        Xn[row, N - 2, NAN_STATE[model]] = np.nan
    out = dict(tvlqr=s.tvlqr(dict(Q=Q, R=R, Qf=Qf, store_P=1, **SC.MODES[MODE]), Xn, U[idx]))
    out["lincov"] = s.lincov(LC.options(model, N, MODE, store_S=1), X[idx], U[idx], S0=LC.full_S0(model)[idx])
    tv, lc = out["tvlqr"], out["lincov"]
    assert tv.status[row] == 0 and tv.fail_knot[row] > 0 and lc["status"][row] == 0 and lc["fail_knot"][row] == tv.fail_knot[row]
    assert model == 0 or (tv.fail_knot[row] == N - 1 and tv.status.sum() == len(idx) - 1 and not tv.fail_knot[tv.status == 1].any())
    return out


@functools.lru_cache(maxsize=None)
def tight(model, N, changed=False):
    """(a): batch_cap = B = 5, the whole chain once (changed: with the options of (e)); then, under "failed", _failed_gains"""
    s = g.BatchSolver(model, N, B, hist_cap=16)
    _set(s, model, N, range(B))
    _set_env(s, model, range(B))
    out = _chain(s, model, N, range(B), generated_from=0, **(_changed(model) if changed else {}))
    if not changed:
        out["failed"] = _failed_gains(s, model, N, range(B))
    s.close()
    return out


def _changed(model):
    """the options of (e): other weights, tighter control bounds, a wider start, P of knot 1 only"""
    Q, R, Qf = LC.WEIGHTS
    return dict(store_P=0, tv=dict(Q=2 * Q, R=3 * R, Qf=Qf / 2), sim=dict(u_lo=-0.5 * SC.bounds(model, 1)[1][0], u_hi=0.5 * SC.bounds(model, 1)[1][0]),
                lc=dict(dx0=2 * SC.dx0(model)))


def _refused(call, *args, **kw):
    with pytest.raises(g._capi.GustoError, match="-> -3"):
        call(*args, **kw)


@pytest.mark.parametrize("model,N", CASES)
def test_a_larger_handle_and_batches_of_changing_size(model, N):
    ref = dict(tight(model, N))
    failed = ref.pop("failed")
    has_env_batch = not LC.env(model, "batch")[1]
    s = g.BatchSolver(model, N, CAP, hist_cap=16)
    # (b) batch_cap = 8, the same five
    _set(s, model, N, range(B))
    _set_env(s, model, range(B))
    _equal(_chain(s, model, N, range(B), generated_from=0), ref, range(B), B, "(b)")
    assert np.array_equal(s.get_tvlqr(full_P=True).P, ref["tvlqr"].P)
    # (c) the same handle, problems 3 and 4 only
    _set(s, model, N, (3, 4))
    for getter in (s.get_verify, s.get_tvlqr, s.get_simulate, s.get_simulate_knots, s.get_lincov, s.last_verify_ms, s.last_tvlqr_ms,
                   s.last_simulate_ms, s.last_lincov_ms):
        _refused(getter)
    assert s.L.gusto_get_dense(s.h, None, None, None) == -3
    _refused(s.simulate, _sim_opts(model, 65))
    assert b"gusto_tvlqr" in s.L.gusto_last_error(s.h)
    _refused(s.lincov)
    assert b"gusto_tvlqr" in s.L.gusto_last_error(s.h)
    part = _chain(s, model, N, (3, 4), stages=("tvlqr",))
    for getter in (s.get_simulate, s.get_simulate_knots, s.get_lincov):
        _refused(getter)
    if has_env_batch:          # the handle still holds the environments of five problems
        _refused(s.lincov)
        assert b"different number of problems" in s.L.gusto_last_error(s.h)
        _refused(s.verify)
        _refused(s.simulate, _sim_opts(model, 65))
        _refused(s.get_lincov)
    _set_env(s, model, (3, 4))
    _refused(s.get_verify)
    part.update(_chain(s, model, N, (3, 4), generated_from=3, stages=("verify", "simulate", "lincov")))
    _equal(part, ref, (3, 4), 2, "(c)")
    # ... and with gains that failed: status and fail_knot sit at offsets of the five-problem allocation, B = 2 now
    _equal(_failed_gains(s, model, N, (3, 4)), failed, (3, 4), 2, "(c) failed gains")
    # (d) the same handle, eight problems: larger than anything it has held
    _set(s, model, N, EIGHT)
    _set_env(s, model, EIGHT)
    eight = _chain(s, model, N, EIGHT, store_P=0)
    _equal(eight, ref, EIGHT, 8, "(d)")
    assert eight["tvlqr"].P.shape == (8, s.n, s.n)
    _refused(s.get_tvlqr, full_P=True)                      # the smaller batch's P of every knot must not leak
    # (e) an active mask on the eight, changed options: rows 1 and 6 keep (d)'s results, the others follow the options
    act = np.ones(8, bool)
    act[[1, 6]] = False
    s.set_active(act)
    # (gusto_simulate with the n_samples of its last call: another n_samples is another layout, zeros before the launch)
    masked = _chain(s, model, N, EIGHT, **_changed(model), stages=("tvlqr", "simulate", "lincov"), samples=SAMPLES[1:])
    s.set_active(None)
    s.close()
    _equal(masked, ref, EIGHT, 8, "(e) inactive", only=[1, 6])
    _equal(masked, tight(model, N, True), EIGHT, 8, "(e) active", only=np.flatnonzero(act))
    assert not np.array_equal(masked["tvlqr"].K[0], eight["tvlqr"].K[0])
    assert not np.array_equal(masked["lincov"]["sigma_x"][0], eight["lincov"]["sigma_x"][0])


def test_shooting_on_a_handle_larger_than_its_batch():
    """(f) test_shooting.test_gpu_shooting_matches_the_oracle's case and assertions with batch_cap = B + 3"""
    check_dubins_shooting_against_the_oracle(256, 256 + 3)
