"""Non-default SCP parameters for the GuSTO outer loop (scp_gusto.jl:123-175), one table for the CPU proofs
(tests/test_scp_params_cpu.py) and the GPU tests (tests/test_gpu_scp_params.py).  At the model defaults no lock-step trip of the
suite ever changes Delta; these sets make the runs shrink and grow the trust region, stop at omega_max, and converge at the
`iterations > 2` guard.

  ladder   beta_fail = 0.4, beta_succ = 1.7 (no powers of two: equal Delta histories are equal arithmetic), rho1 = LADDER_RHO1,
           rho0 = 0.8 rho1.  Natural freeflyerSE2 and astrobeeSE3 runs shrink AND grow; dubins_car and the manifold model never
           grow naturally (they shrink, then fail or end TrustRegionViolated) and get their grows from the forced states
  ceiling  omega0 = 0.01, gamma_fail = 4, omega_max = 0.1 (CEILING_LOW: 0.03): runs stop as OmegaMaxExceeded after one to three raises
  loose    convergence_threshold x 30, eps x 100: the sum of two convergence measures is below the threshold from the start, so
           `iterations > 2` is what holds a run back until its third trip.  restart_runs: loose from the converged trajectory of
           the default run, which ends at the guard on every model

Forced states (np_scp_trip.trip from a chosen Delta) on traced trips of the default oracle runs -- the second, the middle and the
last, as param_cases.trips -- each under two sets:
  grow     ladder's factors with rho0 = rho1 = the model's default rho1, from Delta = 0.4 Delta0 (accepted: 0.68 Delta0, uncapped)
           and 0.8 Delta0 (accepted: Delta0, since 1.36 Delta0 is cut)
  split    ladder's factors from Delta = 0.5 Delta0 with rho1 between two cold-oracle rho values of the group (split_rho1) and
           rho0 = rho1 / 4: the group holds rejects, keeps and grows
Every forced trip keeps |rho - threshold| >= 100 x (1e-6 rho + 3e-8) (margin_ok: 100 x the rho tolerance of the lock-step
comparison); a point that does not is replaced by the next trip of the same run, at most 10 % of a group."""
import functools

import numpy as np

import gusto_oracle as go
import np_scp_trip as NT
import test_kkt_certificate as T

FF, DUB, SE3, MAN = go.FREEFLYER_SE2, go.DUBINS_CAR, go.ASTROBEE_SE3, go.ASTROBEE_SE3_MANIFOLD
MODELS = (FF, DUB, SE3, MAN)
SETS = ("ladder", "ceiling", "loose")
B = 8                                   # problems per natural batch: T.batch(model, 8) in T.env(model)
FORCED_B = 16                           # ... and per group of forced states (8 leave an Astrobee group without three keeps)
MAX_ITER = 30

# rho1 of ladder.  freeflyerSE2 and astrobeeSE3: where the oracle's runs both shrink and grow.  dubins_car, manifold: where the
# runs shrink and still accept trips (oracle, N = 16: dubins_car at 0.003 .. 0.3 rejects or violates the trust region on every
# trip, at 1.0 it has 49 OK, 6 shrinks, 35 TrustRegionViolated; the manifold model at 0.02 .. 1 never shrinks, at 0.003 7 times)
LADDER_RHO1 = {FF: 0.02, DUB: 1.0, SE3: 0.003, MAN: 0.003}
CEILING_LOW = 0.03
# the horizons the GPU tests run (test_gpu_params: one wave and the chain kernels at 16, the first multi-wave horizon 65;
# freeflyerSE2's one-wave kernel at 5 and 50; dubins_car at 30)
HORIZONS = {FF: (5, 50), DUB: (30,), SE3: (16, 65), MAN: (16, 65)}
# Gates that were measured, not reused.  freeflyerSE2 at N = 5: _lockstep_parity asks that both sides run the same number of
# interior point iterations on 90 % of the trips (measured at N = 50: 0.99).  At N = 5 a solve takes 6 .. 7 iterations and the
# last digits of the linearisation point decide the count -- on the ORACLE alone, a relative perturbation of 1e-14 of (Xp, Up)
# changes it on 11 of the 95 ladder trips and on 11 of the 59 default trips (1e-12, 1e-10: 10, 10 and 9, 8); at N = 50 on 1 of 105.
GATES = {(FF, 5): dict(min_same_iters=0.8)}
FORCED_SETS = ("grow", "split")
GROW_DELTAS = (0.4, 0.8)
SPLIT_DELTA = 0.5
MAX_REPLACED = 0.10


def defaults(model):
    return go.default_params(model)[0]


def _copy(sp, **kw):
    out = go.ScpParams.from_buffer_copy(bytes(sp))
    for k, v in kw.items():
        setattr(out, k, v)
    return out


def params(name, model, omega_max=0.1):
    """the oracle binding's ScpParams of set `name` on top of the model's defaults (T.as_params turns it into the library's)"""
    d = defaults(model)
    if name == "default":
        return d
    if name == "ladder":
        return _copy(d, beta_fail=0.4, beta_succ=1.7, rho1=LADDER_RHO1[model], rho0=0.8 * LADDER_RHO1[model])
    if name == "ceiling":
        return _copy(d, omega0=0.01, gamma_fail=4.0, omega_max=omega_max)
    if name == "loose":
        return _copy(d, convergence_threshold=30.0 * d.convergence_threshold, eps=100.0 * d.eps)
    if name == "grow":
        return _copy(d, beta_fail=0.4, beta_succ=1.7, rho0=d.rho1)
    raise KeyError(name)


# The cold rho of a group spans 1e-14 .. 1 with the median of the Astrobee models near 1e-7, far below the absolute part of the
# guard (100 x 3e-8 = 3e-6): a threshold there would have every point inside its guard.  So rho1 >= SPLIT_RHO1_FLOOR, which puts
# rho0 = rho1 / 4 at 10 x that absolute part or more.
SPLIT_RHO1_FLOOR = 4 * 10 * 100 * 3e-8
SPLIT_MIN = 3


def split_rho1(rho):
    """rho1 of the split set: the geometric mean g of two adjacent values of sorted(rho).  Eligible are the pairs with
    g >= SPLIT_RHO1_FLOOR that leave SPLIT_MIN values above g (rejects) and SPLIT_MIN in [g / 4, g] (keeps: with the widest gap of
    all and rho0 = rho1 / 4 a group can have none, and only a keep tells rho0 from rho1).  Of the eligible pairs in the middle half
    of the list the one with the widest (relative) gap; where the middle half has none, the eligible pair nearest to it"""
    r = np.sort(np.asarray(rho, float))
    n = len(r)
    gm = np.sqrt(r[:-1] * r[1:])
    ok = [i for i in range(n - 1) if gm[i] >= SPLIT_RHO1_FLOOR and (r > gm[i]).sum() >= SPLIT_MIN
          and ((r >= gm[i] / 4) & (r <= gm[i])).sum() >= SPLIT_MIN]
    assert ok, r
    mid = [i for i in ok if n // 4 <= i < (3 * n) // 4]
    i = max(mid, key=lambda i: r[i + 1] / r[i]) if mid else min(ok, key=lambda i: abs(i - n // 2))
    return float(gm[i])


def split_params(model, rho):
    r1 = split_rho1(rho)
    return _copy(defaults(model), beta_fail=0.4, beta_succ=1.7, rho1=r1, rho0=r1 / 4)


def guard(rho):
    """100 x the rho tolerance of test_gpu_parity._lockstep_parity"""
    return 100.0 * (1e-6 * abs(rho) + 3e-8)


def margin_ok(rho, sp):
    return abs(rho - sp.rho0) >= guard(rho) and abs(rho - sp.rho1) >= guard(rho)


# ---- census -----------------------------------------------------------------------------------------------------------------
CENSUS_KEYS = ("OK", "InaccurateModel", "ViolatesConstraints", "TrustRegionViolated", "shrink", "grow", "grow_capped",
               "stop_MaxIter", "stop_Converged", "stop_SubproblemFailed", "stop_OmegaMax", "stop_at_3")


def census(history, sp, stop_reason=None, iterations=None):
    """Counts of ONE run: history = dict(scp_status, Delta, omega) of its n_hist entries (entry 0 is the constructor's).  The four
    scp_status values; shrink = a status-2 entry whose Delta is beta_fail x the one before; grow / grow_capped = an accepted entry
    whose Delta rose to beta_succ x the one before / to Delta0 where beta_succ x Delta is larger; the stop reason, and stop_at_3 =
    Converged with iterations == 3."""
    st, D = np.asarray(history["scp_status"]), np.asarray(history["Delta"], float)
    c = dict.fromkeys(CENSUS_KEYS, 0)
    for h in range(1, len(st)):
        c[go.SCP_STATUS[int(st[h])]] += 1
        if st[h] == 2 and D[h] == sp.beta_fail * D[h - 1] and D[h] < D[h - 1]:
            c["shrink"] += 1
        if st[h] in (1, 3) and D[h] > D[h - 1]:
            if D[h] == sp.beta_succ * D[h - 1] and D[h] < sp.Delta0:
                c["grow"] += 1
            elif D[h] == sp.Delta0 and sp.beta_succ * D[h - 1] > sp.Delta0:
                c["grow_capped"] += 1
    if stop_reason is not None:
        c[("stop_MaxIter", "stop_Converged", "stop_SubproblemFailed", "stop_OmegaMax")[int(stop_reason)]] += 1
        if int(stop_reason) == 1 and int(iterations) == 3:
            c["stop_at_3"] += 1
    return c


def add(a, b):
    return {k: a.get(k, 0) + b[k] for k in b}


def total(censuses):
    out = dict.fromkeys(CENSUS_KEYS, 0)
    for c in censuses:
        out = add(out, c)
    return out


def short(c):
    return " ".join(f"{k}={v}" for k, v in c.items() if v)


# ---- natural runs -----------------------------------------------------------------------------------------------------------
def batch(model, nb=B):
    return T.batch(model, nb)


@functools.lru_cache(maxsize=None)
def oracle_runs(name, model, N, nb=B, omega_max=0.1, force=False):
    """[(result, trace)] of the oracle's runs of the batch under set `name`"""
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = batch(model, nb)
    o = go.Oracle(model, N, boxes=boxes, spheres=sph, scp_params=params(name, model, omega_max))
    out = []
    for b in range(nb):
        o.set_trace(MAX_ITER + 2)
        o.set_problem(x0[b], glo[b], ghi[b], tf[b])
        r = o.solve(MAX_ITER, force=force)
        out.append((r, o.trace()))
    return out


def run_census(name, model, N, nb=B, omega_max=0.1):
    sp = params(name, model, omega_max)
    return total(census(r, sp, r["stop_reason"], r["iterations"]) for r, _ in oracle_runs(name, model, N, nb, omega_max))


@functools.lru_cache(maxsize=None)
def restart_runs(model, N, nb=B):
    """[(b, X0, U0, result)]: the loose run of every problem whose default run converged, started from that run's final trajectory.
    Its first two convergence measures are already below the threshold, so the run has to stop at exactly three iterations: the
    `iterations > 2` guard of scp_gusto.jl:170 on every model (natural loose runs of dubins_car never end there)"""
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = batch(model, nb)
    o = go.Oracle(model, N, boxes=boxes, spheres=sph, scp_params=params("loose", model))
    out = []
    for b, (r, _) in enumerate(oracle_runs("default", model, N, nb)):
        if r["stop_reason"] == 1:
            o.set_problem(x0[b], glo[b], ghi[b], tf[b], r["X"], r["U"])
            out.append((b, r["X"], r["U"], o.solve(MAX_ITER)))
    return out


# ---- forced states ----------------------------------------------------------------------------------------------------------
def _candidates(model, N):
    """(problem, trip index) of the second, middle and last trip of every default run that has two trips or more"""
    out = []
    for b, (r, tr) in enumerate(oracle_runs("default", model, N, FORCED_B)):
        n = len(tr)
        if n >= 2:
            out += [(b, t) for t in sorted({1, n // 2, n - 1})]
    return out


@functools.lru_cache(maxsize=None)
def _cold(model, N, b, t, frac):
    """the cold oracle trip from trip t of problem b's default run at Delta = frac x Delta0 (thresholds play no part in it)"""
    boxes, sph = T.env(model)
    x0, glo, ghi, tf = batch(model, FORCED_B)
    r, tr = oracle_runs("default", model, N, FORCED_B)[b]
    sp, mp = go.default_params(model)
    o = go.Oracle(model, N, boxes=boxes, spheres=sph)
    o.set_problem(x0[b], glo[b], ghi[b], tf[b])
    return NT.pieces(o, mp.clearance, tr[t]["Xp"], tr[t]["Up"], frac * sp.Delta0, float(r["omega"][t]))


@functools.lru_cache(maxsize=None)
def forced(model, N):
    """{set: (ScpParams, [point])} with point = dict(b, t, Xp, Up, Delta, omega, ref = np_scp_trip.trip's dict under the set), plus
    "replaced": {set: (replaced, candidates)}.  A candidate whose cold rho sits inside the guard of a threshold, or whose cold
    subproblem fails, is replaced by the nearest other trip of the same run that does not"""
    runs = oracle_runs("default", model, N, FORCED_B)
    cand = _candidates(model, N)
    d = defaults(model)
    fr = {"grow": GROW_DELTAS, "split": (SPLIT_DELTA,)}
    solved = lambda b, t, f: _cold(model, N, b, t, f)["solver_status"] in (1, 2)
    rho = [_cold(model, N, b, t, SPLIT_DELTA)["rho"] for b, t in cand if solved(b, t, SPLIT_DELTA)]
    sps = {"grow": params("grow", model), "split": split_params(model, rho)}
    out, replaced = {}, {}
    for name in FORCED_SETS:
        sp, pts, nrep, used = sps[name], [], 0, set(cand)
        for b, t in cand:
            ok = lambda t_: all(solved(b, t_, f) and margin_ok(_cold(model, N, b, t_, f)["rho"], sp) for f in fr[name])
            if not ok(t):
                alt = [t_ for t_ in sorted(range(len(runs[b][1])), key=lambda t_: abs(t_ - t)) if (b, t_) not in used and ok(t_)]
                assert alt, (name, model, N, b, t)
                t = alt[0]
                used.add((b, t))
                nrep += 1
            r, tr = runs[b]
            for f in fr[name]:
                c = _cold(model, N, b, t, f)
                pts.append(dict(b=b, t=t, Xp=tr[t]["Xp"], Up=tr[t]["Up"], Delta=f * d.Delta0, omega=float(r["omega"][t]),
                                ref=dict(c, **NT.verdict(sp, c["Delta"], c["omega"], c["max_d2"], c["rho"], c["cvx_sat"]))))
        out[name] = (sp, pts)
        replaced[name] = (nrep, len(cand))
    out["replaced"] = replaced
    return out


def forced_census(model, N):
    f = forced(model, N)
    out = dict.fromkeys(CENSUS_KEYS, 0)
    for name in FORCED_SETS:
        sp, pts = f[name]
        for p in pts:
            r = p["ref"]
            out = add(out, census(dict(scp_status=[0, r["scp_status"]], Delta=[p["Delta"], r["Delta_next"]]), sp))
    return out
