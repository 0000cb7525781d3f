"""Numpy restatement of gusto_simulate, written from the definitions of include/gusto_hip.h and from nothing in csrc/: the
closed-loop roll-out of u = clip((U_k - K_k (x - X_k)) + p_u, u_lo, u_hi) from X_1 + p_x, held over Nstep classical RK4 steps per
interval without a restart at the knots; the signed distance at the dense samples (np_verify.dist_many); the handling of
non-finite samples; the per-problem report as a reduction of the per-sample arrays; and the perturbation generator in uint64
arithmetic (splitmix64 of a counter).  Works in the dtype passed in (float64, or np.longdouble for the error estimate of
tools/simulate_errors.py): the samples of one problem run side by side as columns.

The dynamics are np_models' f; for AstrobeeSE3, whose f sums over whole arrays, f_cols below states the same formulas with the
sums along the state axis (tests/test_simulate_cpu.py holds it against np_models' f column by column)."""
import numpy as np

import np_models as M
import np_verify as V
from np_tvlqr import n_substeps  # noqa: F401  (the shared Nstep rule)

MODELS = V.MODELS
U64 = np.uint64
GOLDEN, MIX1, MIX2 = U64(0x9E3779B97F4A7C15), U64(0xBF58476D1CE4E5B9), U64(0x94D049BB133111EB)


# ---- the generator ----------------------------------------------------------------------------------------------------------
def splitmix64(seed, idx):
    """output number idx (0-based; an array) of splitmix64 started at `seed`, in uint64 arithmetic mod 2^64"""
    with np.errstate(over="ignore"):
        z = U64(seed) + GOLDEN * (np.asarray(idx, dtype=U64) + U64(1))
        z = (z ^ (z >> U64(30))) * MIX1
        z = (z ^ (z >> U64(27))) * MIX2
        return z ^ (z >> U64(31))


def perturbations(model_id, B, S, dx0, du0, seed=0, first_problem=0):
    """pert [B, S, n + m] as gusto_simulate generates it: sample 0 zeros, entry i of sample s >= 1 of problem b uniform in
    [-w_i, w_i), w = (dx0, du0), from output ((first_problem + b) S + s)(n + m) + i of splitmix64(seed)"""
    model = MODELS[model_id]
    n, m = model.n, model.m
    nz = n + m
    w = np.concatenate([np.broadcast_to(np.asarray(dx0, float), (n,)), np.broadcast_to(np.asarray(du0, float), (m,))])
    b, s, i = np.meshgrid(np.arange(B, dtype=U64), np.arange(S, dtype=U64), np.arange(nz, dtype=U64), indexing="ij")
    with np.errstate(over="ignore"):
        idx = ((U64(first_problem) + b) * U64(S) + s) * U64(nz) + i
    r = (splitmix64(seed, idx) >> U64(11)).astype(np.float64) * 2.0 ** -53
    p = (2.0 * r - 1.0) * w
    p[:, 0, :] = 0.0
    return p


# ---- dynamics on columns ----------------------------------------------------------------------------------------------------
def _cross0(a, b):
    return np.stack([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def f_cols(model_id, x, u):
    """f at S points: x [n, S], u [m, S] -> [n, S], in the dtype of x"""
    model = MODELS[model_id]
    if model_id != 2:
        return np.asarray(model.f(x, u))
    v, p, w = x[3:6], x[6:9], x[9:12]              # astrobee_se3.jl:180-190 with quat_functions.jl:253-257 (mrp_derivative)
    pd = 0.25 * ((1 - np.sum(p * p, axis=0)) * w - 2 * _cross0(w, p) + 2 * np.sum(w * p, axis=0) * p)
    J = M._per_axis(M.Astrobee.J, w).astype(x.dtype)
    wd = (u[3:6] - _cross0(w, J * w)) / J
    return np.concatenate([v, u[0:3] / M.Astrobee.mass, pd, wd])


def rk4_step(model_id, x, u, h):
    k1 = f_cols(model_id, x, u)
    k2 = f_cols(model_id, x + 0.5 * h * k1, u)
    k3 = f_cols(model_id, x + 0.5 * h * k2, u)
    k4 = f_cols(model_id, x + h * k3, u)
    return x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)


# ---- the roll-out of one problem --------------------------------------------------------------------------------------------
def simulate(model_id, X, U, K, tf, pert, u_lo=None, u_hi=None, boxes=None, spheres=None, dt_min=0.1, nstep=0,
             dense_collision=True, dtype=np.float64):
    """One problem: X [N, n], U [N, m], K [N-1, m, n], pert [S, n + m].  Returns a dict with the per-sample arrays
    (sample_min_dist, sample_dense_index, sample_flags, x_final), Xcl [N, S, n], the per-problem report (report()), and two
    conditioning figures per sample: clip_margin (see below) and the unclipped controls' history is not kept."""
    model = MODELS[model_id]
    n, m = model.n, model.m
    N, S = len(X), len(pert)
    boxes, spheres = V.obstacles(boxes, spheres)
    if model_id == 1:
        boxes, spheres = V.obstacles(None, None)
    has_obs = len(boxes) + len(spheres) > 0
    Xd, Ud, Kd, pd = (np.asarray(a, float).astype(dtype) for a in (X, U, K, pert))
    lo = np.full(m, -np.inf) if u_lo is None else np.broadcast_to(np.asarray(u_lo, float), (m,))
    hi = np.full(m, np.inf) if u_hi is None else np.broadcast_to(np.asarray(u_hi, float), (m,))
    lo, hi = lo.astype(dtype)[:, None], hi.astype(dtype)[:, None]
    ns = n_substeps(tf, N, dt_min, nstep)
    h = dtype(tf) / dtype(N - 1) / dtype(ns)
    x = Xd[0][:, None] + pd[:, :n].T                       # [n, S]
    pu = pd[:, n:].T                                       # [m, S]
    alive = np.isfinite(x).all(axis=0)
    nonfinite = ~alive
    clipped = np.zeros(S, bool)
    dmin = np.full(S, np.inf, dtype=dtype)
    didx = np.full(S, -1)
    dev = np.zeros((n, S), dtype=dtype)
    Xcl = np.zeros((N, S, n), dtype=dtype)
    # clip_margin: how far the decision "was some entry clipped" is from flipping -- for a clipped sample the largest excess over
    # a bound, for an unclipped one the smallest distance of an entry to a finite bound
    excess = np.zeros(S, dtype=dtype)
    room = np.full(S, np.inf, dtype=dtype)

    def distances(j):
        nonlocal dmin, didx
        if not has_obs or not alive.any():
            return
        d = np.full(S, np.inf, dtype=dtype)
        d[alive] = V.dist_many(model_id, x[:, alive].T, boxes, spheres)
        better = alive & (d < dmin)
        dmin = np.where(better, d, dmin)
        didx = np.where(better, j, didx)

    with np.errstate(all="ignore"):
        for k in range(N - 1):
            d = x - Xd[k][:, None]
            dev = np.where(alive, np.maximum(dev, np.abs(d)), dev)
            Xcl[k] = x.T
            v = (Ud[k][:, None] - Kd[k] @ d) + pu
            over = np.maximum(np.where(v > hi, v - hi, 0), np.where(v < lo, lo - v, 0)).max(axis=0)
            inside = np.minimum(np.where(np.isfinite(hi), np.abs(hi - v), np.inf), np.where(np.isfinite(lo), np.abs(v - lo), np.inf)).min(axis=0)
            is_clipped = ((v < lo) | (v > hi)).any(axis=0)
            clipped |= alive & is_clipped
            excess = np.where(alive & is_clipped, np.maximum(excess, over), excess)
            room = np.where(alive & ~is_clipped, np.minimum(room, inside), room)
            u = np.where(v < lo, lo, np.where(v > hi, hi, v))
            for q in range(ns):
                if dense_collision or q == 0:
                    distances(k * ns + q)
                xn = rk4_step(model_id, x, u, h)
                x = np.where(alive, xn, x)
                bad = alive & ~np.isfinite(x).all(axis=0)
                nonfinite |= bad
                alive &= ~bad
        dev = np.where(alive, np.maximum(dev, np.abs(x - Xd[N - 1][:, None])), dev)
        Xcl[N - 1] = x.T
        distances((N - 1) * ns)
    flags = (dmin < 0).astype(np.int32) | (clipped.astype(np.int32) << 1) | (nonfinite.astype(np.int32) << 2)
    out = dict(sample_min_dist=dmin, sample_dense_index=didx.astype(np.int32), sample_flags=flags, x_final=x.T.copy(), Xcl=Xcl,
               sample_dev=dev.T.copy(), clip_margin=np.where(clipped, excess, room), nstep=ns)
    out.update(report(dmin, out["sample_dense_index"], flags, out["x_final"], out["sample_dev"], Xd[N - 1]))
    return out


def report(sample_min_dist, sample_dense_index, sample_flags, x_final, sample_dev, X_end):
    """The per-problem fields of gusto_simulate_report from the per-sample arrays: non-finite samples enter the counts only;
    ties for the smallest distance go to the lowest sample"""
    fin = (sample_flags & 4) == 0
    n = x_final.shape[1]
    out = dict(n_free=int((fin & ((sample_flags & 1) == 0)).sum()), n_finite=int(fin.sum()), n_clipped=int(((sample_flags & 2) != 0).sum()),
               min_dist=np.inf, worst_sample=-1, worst_dense_sample=-1, max_dev=np.zeros(n, dtype=x_final.dtype),
               max_final_dev=np.zeros(n, dtype=x_final.dtype))
    if fin.any():
        d = np.where(fin, sample_min_dist, np.inf)
        if np.isfinite(d).any() or (d < np.inf).any():
            s = int(np.argmin(d))                      # (the first of equal minima)
            if d[s] < np.inf:
                out.update(min_dist=d[s], worst_sample=s, worst_dense_sample=int(sample_dense_index[s]))
        out["max_dev"] = sample_dev[fin].max(axis=0)
        out["max_final_dev"] = np.abs(x_final[fin] - X_end).max(axis=0)
    return out
