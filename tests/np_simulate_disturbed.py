"""Numpy restatement of gusto_simulate_disturbed, written from the definitions of include/gusto_hip.h and from nothing in csrc/:
the two generator streams (plant, actuator noise) in uint64 arithmetic, the dynamics on columns with the plant scalars of every
column, and the closed-loop roll-out with the noise w_k added to the commanded control of interval k.  Everything else -- the
Nstep rule, the signed distance, the flags, the report, splitmix64 -- is np_simulate's.  Works in the dtype passed in.

theta [.., 6] = (mass, Jdiag[0], Jdiag[1], Jdiag[2], dubins_v, dubins_k); freeflyerSE2 reads mass and Jdiag[2], DubinsCar
dubins_v and dubins_k, both Astrobee models mass and Jdiag[0 .. 2]."""
import numpy as np

import np_models as M
import np_simulate as NS
import np_verify as V

NPLANT = 6
U64 = np.uint64
PLANT_TAG, WHITE_TAG = 0x504C414E54, 0x5748495445
READS = {0: (0, 3), 1: (4, 5), 2: (0, 1, 2, 3), 3: (0, 1, 2, 3)}


def nominal(model_id, fill=1.0):
    """the plant scalars of np_models' constants; entries the model does not read hold `fill`"""
    th = np.full(NPLANT, float(fill))
    if model_id == 1:
        th[4], th[5] = M.Dubins.v, M.Dubins.k
    else:
        cls = M.FreeflyerSE2 if model_id == 0 else M.Astrobee
        th[0], th[1:4] = cls.mass, cls.J
    return th


# ---- the generator ----------------------------------------------------------------------------------------------------------
def stream_seeds(seed):
    """(seed_plant, seed_white): output 0 of splitmix64 started at seed ^ tag"""
    seed = int(seed) % 2 ** 64
    return int(NS.splitmix64(seed ^ PLANT_TAG, 0)), int(NS.splitmix64(seed ^ WHITE_TAG, 0))


def _uniform(seed, idx):
    """2 r - 1 with r = (z >> 11) 2^-53: exact"""
    return 2.0 * ((NS.splitmix64(seed, idx) >> U64(11)).astype(np.float64) * 2.0 ** -53) - 1.0


def plants(nominal_theta, B, S, plant_rel, seed=0, first_problem=0):
    """theta [B, S, 6] as generated: nominal_j (1 + e_j), e_j uniform in [-plant_rel_j, plant_rel_j) from output
    ((first_problem + b) S + s) 6 + j of the plant stream; sample 0 draws e = 0"""
    rel = np.broadcast_to(np.asarray(plant_rel, float), (NPLANT,))
    b, s, j = np.meshgrid(np.arange(B, dtype=U64), np.arange(S, dtype=U64), np.arange(NPLANT, dtype=U64), indexing="ij")
    with np.errstate(over="ignore"):
        idx = ((U64(first_problem) + b) * U64(S) + s) * U64(NPLANT) + j
    e = _uniform(stream_seeds(seed)[0], idx) * rel
    e[:, 0, :] = 0.0
    return np.asarray(nominal_theta, float) * (1.0 + e)


def whites(model_id, B, N, S, dw, seed=0, first_problem=0):
    """w [B, N-1, S, m] as generated: entry i of sample s >= 1 in interval k uniform in [-dw_i, dw_i) from output
    (((first_problem + b) S + s)(N - 1) + (k - 1)) m + i of the noise stream; zeros for sample 0"""
    m = NS.MODELS[model_id].m
    w = np.broadcast_to(np.asarray(dw, float), (m,))
    b, k, s, i = np.meshgrid(np.arange(B, dtype=U64), np.arange(N - 1, dtype=U64), np.arange(S, dtype=U64), np.arange(m, dtype=U64),
                             indexing="ij")
    with np.errstate(over="ignore"):
        idx = (((U64(first_problem) + b) * U64(S) + s) * U64(N - 1) + k) * U64(m) + i
    out = _uniform(stream_seeds(seed)[1], idx) * w
    out[:, :, 0, :] = 0.0
    return out


# ---- dynamics on columns, every column with its own plant ---------------------------------------------------------------------
def f_cols(model_id, x, u, theta):
    """f at S points: x [n, S], u [m, S], theta [6, S] -> [n, S], in the dtype of x"""
    mass, J, dv, dk = theta[0], theta[1:4], theta[4], theta[5]
    if model_id == 0:        # freeflyer_se2.jl:182-206
        return np.concatenate([x[3:6], u[0:2] / mass, u[2:3] / J[2]])
    if model_id == 1:        # dubins_car.jl:161-165
        return np.array([dv * np.cos(x[2]), dv * np.sin(x[2]), dk * u[0]])
    if model_id == 2:        # astrobee_se3.jl:180-190
        v, p, w = x[3:6], x[6:9], x[9:12]
        pd = 0.25 * ((1 - np.sum(p * p, axis=0)) * w - 2 * NS._cross0(w, p) + 2 * np.sum(w * p, axis=0) * p)
        wd = (u[3:6] - NS._cross0(w, J * w)) / J
        return np.concatenate([v, u[0:3] / mass, pd, wd])
    v = x[3:6]               # astrobee_se3_manifold.jl:231-246
    qw, qx, qy, qz = x[6:10]
    wx, wy, wz = x[10:13]
    qd = 0.5 * np.array([-wx * qx - wy * qy - wz * qz, wx * qw - wz * qy + wy * qz, wy * qw + wz * qx - wx * qz,
                         wz * qw - wy * qx + wx * qy])
    w = x[10:13]
    wd = (u[3:6] - NS._cross0(w, J * w)) / J
    return np.concatenate([v, u[0:3] / mass, qd, wd])


def rk4_step(model_id, x, u, h, theta):
    k1 = f_cols(model_id, x, u, theta)
    k2 = f_cols(model_id, x + 0.5 * h * k1, u, theta)
    k3 = f_cols(model_id, x + 0.5 * h * k2, u, theta)
    k4 = f_cols(model_id, x + h * k3, u, theta)
    return x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)


# ---- the roll-out of one problem ------------------------------------------------------------------------------------------------
def simulate(model_id, X, U, K, tf, pert, theta, white=None, u_lo=None, u_hi=None, boxes=None, spheres=None, dt_min=0.1, nstep=0,
             dense_collision=True, dtype=np.float64):
    """One problem: X [N, n], U [N, m], K [N-1, m, n], pert [S, n + m], theta [S, 6], white [N-1, S, m] (None: zeros).  Returns
    what np_simulate.simulate returns: the law is the nominal one, the plant integrated is theta's, and in interval k
    v = ((U_k - K_k (x - X_k)) + p_u) + w_k before the clip, which the clipped flag sees."""
    model = NS.MODELS[model_id]
    n, m = model.n, model.m
    N, S = len(X), len(pert)
    boxes, spheres = V.obstacles(boxes, spheres)
    if model_id == 1:
        boxes, spheres = V.obstacles(None, None)
    has_obs = len(boxes) + len(spheres) > 0
    white = np.zeros((N - 1, S, m)) if white is None else white
    Xd, Ud, Kd, pd, th, wh = (np.asarray(a, float).astype(dtype) for a in (X, U, K, pert, theta, white))
    th = th.T                                              # [6, S]
    lo = np.full(m, -np.inf) if u_lo is None else np.broadcast_to(np.asarray(u_lo, float), (m,))
    hi = np.full(m, np.inf) if u_hi is None else np.broadcast_to(np.asarray(u_hi, float), (m,))
    lo, hi = lo.astype(dtype)[:, None], hi.astype(dtype)[:, None]
    ns = NS.n_substeps(tf, N, dt_min, nstep)
    h = dtype(tf) / dtype(N - 1) / dtype(ns)
    x = Xd[0][:, None] + pd[:, :n].T
    pu = pd[:, n:].T
    alive = np.isfinite(x).all(axis=0)
    nonfinite = ~alive
    clipped = np.zeros(S, bool)
    dmin = np.full(S, np.inf, dtype=dtype)
    didx = np.full(S, -1)
    dev = np.zeros((n, S), dtype=dtype)
    Xcl = np.zeros((N, S, n), dtype=dtype)
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
            v = ((Ud[k][:, None] - Kd[k] @ d) + pu) + wh[k].T
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
                xn = rk4_step(model_id, x, u, h, th)
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
    out.update(NS.report(dmin, out["sample_dense_index"], flags, out["x_final"], out["sample_dev"], Xd[N - 1]))
    return out
