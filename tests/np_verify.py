"""Numpy restatement of the reference's post-solve checks, written from the model files:

  interpolate_traj                   astrobee_se3_manifold.jl:1011-1042, astrobee_se3.jl:495-527
  dynamics_constraint_satisfaction   astrobee_se3_manifold.jl:1044-1055, astrobee_se3.jl:529-540
  verify_collision_free              astrobee_se3_manifold.jl:1057-1077, astrobee_se3.jl:542-560
  get_workspace_location             freeflyer_se2.jl:334-336 ([X[1:2,k]; 0]: the plane), astrobee_se3.jl:319-321 (X[1:3,k])
  robot components                   robot/freeflyer.jl:50-57 (body at the origin, arm cylinder at xb = (0, 0.15, 0)),
                                     robot/astrobee3D.jl (one sphere)

plus the two numbers the reference lacks: the smallest signed distance over all dense samples and the gap between the end
of a rolled-out interval and the next knot.  The dynamics are np_models' f, the distances np_models' sd_box / sd_sphere (the
knots call them one by one; the dense samples, a few thousand per problem, go through dist_many, the same arithmetic on
arrays, which tests/test_verify_cpu.py holds against sd_box / sd_sphere).  Nothing here reads csrc/.

Where interpolate_traj cannot run as written (`Matrix(u_dim, Nfull-1)`, `repmat`, the undefined `Tf` of its return) the
statement it makes is kept: Ufull holds U[:,k] over the Nstep samples of interval k."""
import numpy as np

import np_models as M

MODELS = {0: M.FreeflyerSE2, 1: M.Dubins, 2: M.AstrobeeSE3, 3: M.AstrobeeSE3Manifold}
WS_DIM = {0: 2, 1: 2, 2: 3, 3: 3}
# offsets of the convex robot components in the workspace (translation only: BulletCollision.distance(env, rb_idx, r, env_idx)
# places the compound object at r)
COMPONENTS = {0: np.array([[0.0, 0.0], [0.0, 0.15]]), 1: np.zeros((0, 2)), 2: np.zeros((1, 3)), 3: np.zeros((1, 3))}
_BATCH_SAFE_F = (0, 1, 3)      # np_models' f of these models works on [n, K] arrays as it stands


def obstacles(boxes, spheres):
    boxes = np.zeros((0, 6)) if boxes is None else np.asarray(boxes, float).reshape(-1, 6)
    spheres = np.zeros((0, 4)) if spheres is None else np.asarray(spheres, float).reshape(-1, 4)
    return boxes, spheres


def f_cols(model_id, Xc, Uc):
    """f at K points: Xc [K, n], Uc [K, m] -> [K, n]"""
    model = MODELS[model_id]
    if model_id in _BATCH_SAFE_F:
        return np.asarray(model.f(Xc.T, Uc.T), float).T
    return np.array([model.f(x, u) for x, u in zip(Xc, Uc)])


def dist_one(model_id, x, comp, i, boxes, spheres):
    """signed distance of robot component `comp` at state x to keep-out component i (boxes, then spheres)"""
    model, d = MODELS[model_id], WS_DIM[model_id]
    c = np.asarray(x[:d], float) + COMPONENTS[model_id][comp]
    if i < len(boxes):
        return M.sd_box(c, boxes[i, 0:3], boxes[i, 3:6], model.r)[0]
    s = spheres[i - len(boxes)]
    return M.sd_sphere(c, s[0:3], s[3], model.r)[0]


def dist_many(model_id, Xs, boxes, spheres):
    """min over components and keep-out components of the signed distance at every row of Xs [K, n] -> [K] (+inf without
    obstacles): sd_box / sd_sphere on arrays"""
    model, d = MODELS[model_id], WS_DIM[model_id]
    out = np.full(len(Xs), np.inf)
    for off in COMPONENTS[model_id]:
        c = Xs[:, :d] + off
        for bx in boxes:
            lo, hi = bx[0:d], bx[3:3 + d]
            e = np.where(c < lo, c - lo, np.where(c > hi, c - hi, 0.0))
            outside = np.any(e != 0, axis=1)
            d_out = np.sqrt((e * e).sum(axis=1))
            d_in = -np.minimum((c - lo).min(axis=1), (hi - c).min(axis=1))
            out = np.minimum(out, np.where(outside, d_out, d_in) - model.r)
        for s in spheres:
            v = c - s[:d]
            out = np.minimum(out, np.sqrt((v * v).sum(axis=1)) - s[3] - model.r)
    return out


def knot_distances(model_id, X, boxes, spheres):
    """D[comp, obstacle, k]"""
    nc, no = len(COMPONENTS[model_id]), len(boxes) + len(spheres)
    if model_id == 1:
        nc = no = 0
    D = np.zeros((nc, no, len(X)))
    for c in range(nc):
        for i in range(no):
            for k in range(len(X)):
                D[c, i, k] = dist_one(model_id, X[k], c, i, boxes, spheres)
    return D


def verify_collision_free(model_id, X, boxes=None, spheres=None, D=None):
    """(free, k, dist): the first knot (1-based) below zero in the reference's loop order -- obstacle, then knot; the robot
    components outermost (the reference checks rb_idx = 1 only) --, (True, 0, 0.0) when there is none."""
    boxes, spheres = obstacles(boxes, spheres)
    if D is None:
        D = knot_distances(model_id, X, boxes, spheres)
    for c in range(D.shape[0]):
        for i in range(D.shape[1]):
            for k in range(D.shape[2]):
                if D[c, i, k] < 0:
                    return False, k + 1, float(D[c, i, k])
    return True, 0, 0.0


def dynamics_constraint_satisfaction(model_id, X, U, tf):
    N = len(X)
    dt = tf / (N - 1)
    J = 0.0
    for k in range(N - 1):
        J += np.sum(np.abs((X[k + 1] - X[k]) / dt - MODELS[model_id].f(X[k], U[k])))
    return float(J)


def n_substeps(tf, N, dt_min=0.1, nstep=0):
    return int(nstep) if nstep > 0 else int(np.ceil(tf / (N - 1) / dt_min))


def interpolate_traj(model_id, X, U, tf, dt_min=0.1, nstep=0):
    """(Xfull [Nfull, n], Ufull [Nfull - 1, m], gap): every interval restarts from X[k], holds U[k], Nstep RK4 steps of
    dt / Nstep; Xfull[-1] = X[-1]; gap = max_k |end of interval k - X[k+1]|_inf"""
    N, n = X.shape
    dt = tf / (N - 1)
    Nstep = n_substeps(tf, N, dt_min, nstep)
    Nfull = Nstep * (N - 1) + 1
    dtfull = dt / Nstep
    Xfull = np.zeros((Nfull, n))
    Ufull = np.repeat(U[:N - 1], Nstep, axis=0)
    x, u = X[:N - 1].copy(), U[:N - 1]
    idx = Nstep * np.arange(N - 1)
    for s in range(Nstep):
        Xfull[idx + s] = x
        k1 = f_cols(model_id, x, u)
        x2 = x + 0.5 * dtfull * k1
        k2 = f_cols(model_id, x2, u)
        x3 = x + 0.5 * dtfull * k2
        k3 = f_cols(model_id, x3, u)
        x4 = x + dtfull * k3
        k4 = f_cols(model_id, x4, u)
        x = x + 1 / 6 * dtfull * (k1 + 2 * k2 + 2 * k3 + k4)
    gap = float(np.max(np.abs(x - X[1:]))) if not np.isnan(x).any() else float("nan")
    Xfull[-1] = X[-1]
    return Xfull, Ufull, gap


def report(model_id, X, U, tf, boxes=None, spheres=None, dt_min=0.1, nstep=0, dense_collision=True):
    """Every field of gusto_verify_report for one problem, plus the dense trajectory."""
    boxes, spheres = obstacles(boxes, spheres)
    if model_id == 1:
        boxes, spheres = obstacles(None, None)
    D = knot_distances(model_id, X, boxes, spheres)
    free, k, dist = verify_collision_free(model_id, X, boxes, spheres, D)
    Xfull, Ufull, gap = interpolate_traj(model_id, X, U, tf, dt_min, nstep)
    out = dict(collision_free=free, first_knot=k, first_dist=dist,
               min_dist_knots=float(D.min()) if D.size else float("inf"),
               dyn_defect_l1=dynamics_constraint_satisfaction(model_id, X, U, tf),
               min_dist_dense=float("inf"), min_dense_sample=-1, max_gap=gap, Xfull=Xfull, Ufull=Ufull, nfull=len(Xfull))
    if dense_collision and D.size:
        dd = dist_many(model_id, Xfull, boxes, spheres)
        out["min_dense_sample"] = int(np.argmin(dd))
        out["min_dist_dense"] = float(dd.min())
    return out
