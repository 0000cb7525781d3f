"""numpy restatement of gusto_shoot (include/gusto_hip.h), written from the header's text and the reference's model files
(dubins_car.jl:259-280, astrobee_se3_manifold.jl:831-895), in any floating type numpy has (float64, np.longdouble).

The scheme the header states: classical RK4 with `substeps` steps per knot interval on the state + costate ODE, Newton on
F(p0) = x_goal - x(tf; p0) with a forward-difference Jacobian (h_j = 1e-6 max(1, |p_j|)), the step by Cramer's rule (n = 3) or by
Gaussian elimination with complete pivoting that stops at the numerical rank (pivots <= 1e-6 max|J|; n = 13), a halving line search
a = 1 .. 2^-13 on |F|_inf where the first decrease wins.  Stop rules, in this order: |F|_inf not finite (:Diverged), <= ftol
(:Optimal), max_newton steps taken (:Diverged).

Every function takes leading batch axes: z [..., 2n], x0 [..., n], tf [...].  The ODEs are written with vector algebra (quaternion
products, cross products), not component by component as the kernel and the oracle have them."""
import numpy as np

DUBINS, MANIFOLD = 1, 3                      # the public model ids (gusto_hip.h, gusto_oracle.py)
DIMS = {DUBINS: (3, 1), MANIFOLD: (13, 6)}
N_CAND = 14                                  # a = 2^-c > 1e-4: c = 0 .. 13


def params(model, mp):
    """the scalars the shooting ODE reads from a ModelParams (either binding's)"""
    if model == DUBINS:
        return dict(v=float(mp.dubins_v), k=float(mp.dubins_k))
    return dict(mass=float(mp.mass), J=np.array([mp.Jdiag[0], mp.Jdiag[1], mp.Jdiag[2]], dtype=np.float64))


def _quat(a, b):
    """Hamilton product of quaternions (w, x, y, z) along the last axis"""
    aw, av, bw, bv = a[..., :1], a[..., 1:], b[..., :1], b[..., 1:]
    return np.concatenate([aw * bw - (av * bv).sum(-1, keepdims=True), aw * bv + bw * av + np.cross(av, bv)], axis=-1)


def _conj(q):
    return np.concatenate([q[..., :1], -q[..., 1:]], axis=-1)


def _pure(w):
    return np.concatenate([np.zeros_like(w[..., :1]), w], axis=-1)


def ctrl(model, z, par):
    """get_control: u [..., m] from (x, p) = z [..., 2n]"""
    if model == DUBINS:
        return par["k"] / 2 * z[..., 5:6]                                  # U = k/2 p_theta
    J = par["J"].astype(z.dtype)
    return np.concatenate([z[..., 16:19] / (2 * par["mass"]), z[..., 23:26] / J / 2], axis=-1)   # F = pv / 2m, M = Jinv' pw / 2


def rhs(model, z, par):
    """shooting_ode!: d/dt (x, p)"""
    d = np.zeros_like(z)
    u = ctrl(model, z, par)
    if model == DUBINS:
        v, k = par["v"], par["k"]
        th, px, py = z[..., 2], z[..., 3], z[..., 4]
        head = np.stack([np.cos(th), np.sin(th)], axis=-1)
        d[..., 0:2] = v * head
        d[..., 2] = k * u[..., 0]
        d[..., 5] = v * (px * head[..., 1] - py * head[..., 0])            # -(p_xy x heading) v
        return d
    J = par["J"].astype(z.dtype)
    q, w, pr, pq = z[..., 6:10], z[..., 10:13], z[..., 13:16], z[..., 19:23]
    d[..., 0:3] = z[..., 3:6]
    d[..., 3:6] = u[..., :3] / par["mass"]
    d[..., 6:10] = _quat(_pure(w), q) / 2                                   # qdot = (0, w) q / 2
    d[..., 10:13] = (u[..., 3:] - np.cross(w, J * w)) / J                   # Jinv (M - w x J w)
    d[..., 16:19] = -pr
    d[..., 19:23] = _quat(_pure(w), pq) / 2                                 # the costate of q turns with q
    d[..., 23:26] = -_quat(pq, _conj(q))[..., 1:] / 2                       # -(pq q*)_vec / 2 (the w x J w term is left out at HEAD)
    return d


def _rk4(model, z, h, par):
    k1 = rhs(model, z, par)
    k2 = rhs(model, z + h / 2 * k1, par)
    k3 = rhs(model, z + h / 2 * k2, par)
    k4 = rhs(model, z + h * k3, par)
    return z + h / 6 * (k1 + 2 * (k2 + k3) + k4)


def extremal(model, x0, p0, tf, N, substeps, par, dtype=None):
    """the extremal from (x0, p0) over [0, tf] at the N knots: X [..., N, n], U [..., N, m]"""
    dtype = np.dtype(dtype or np.asarray(p0).dtype)
    n, m = DIMS[model]
    with np.errstate(all="ignore"):
        z = np.concatenate(np.broadcast_arrays(np.asarray(x0, dtype), np.asarray(p0, dtype)), axis=-1)
        h = (np.asarray(tf, dtype) / ((N - 1) * substeps))[..., None]
        X, U = np.zeros(z.shape[:-1] + (N, n), dtype), np.zeros(z.shape[:-1] + (N, m), dtype)
        for k in range(N):
            X[..., k, :], U[..., k, :] = z[..., :n], ctrl(model, z, par)
            if k < N - 1:
                for _ in range(substeps):
                    z = _rk4(model, z, h, par)
    return X, U


def goal_point(lo, hi):
    """ShootingProblem's x_goal (types.jl:219-226): the centre of the goal set, 0 for a coordinate without a finite goal"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    both = np.isfinite(lo) & np.isfinite(hi)
    with np.errstate(all="ignore"):
        return np.where(both, (lo + hi) / 2, np.zeros_like(lo))


def norm_inf(F):
    """|F|_inf along the last axis; NaN if any component is"""
    F = np.asarray(F)
    bad = np.isnan(F).any(-1)
    with np.errstate(all="ignore"):
        return np.where(bad, np.nan, np.abs(np.where(np.isnan(F), 0, F)).max(-1))


def newton_step(J, F):
    """dp with J dp = -F, or None.  n = 3: Cramer's rule.  Otherwise elimination with complete pivoting, stopped at the first
    pivot that is not above 1e-6 max|J|; the components of dp that belong to the columns left over stay 0."""
    J, F = np.array(J), np.asarray(F)
    n = len(F)
    with np.errstate(all="ignore"):
        if n == 3:
            det = _det3(J)
            if not (abs(det) > 1e-300) or not np.isfinite(det):
                return None
            dp = np.zeros(3, J.dtype)
            for j in range(3):
                A = J.copy()
                A[:, j] = F
                dp[j] = -_det3(A) / det
            return dp
        if np.isnan(J).any():
            return None
        jmax = np.abs(J).max()
        if not (jmax > 0) or not np.isfinite(jmax):
            return None
        A, r, cols, rank = J, -F.astype(J.dtype), np.arange(n), 0
        for c in range(n):
            sub = np.abs(A[c:, c:])
            i, j = np.unravel_index(np.argmax(sub), sub.shape)       # the first of equal entries, rows first
            if not (sub[i, j] > 1e-6 * jmax):
                break
            i, j = i + c, j + c
            A[[c, i]], r[[c, i]] = A[[i, c]], r[[i, c]]
            A[:, [c, j]], cols[[c, j]] = A[:, [j, c]], cols[[j, c]]
            f = A[c + 1:, c] / A[c, c]
            A[c + 1:, c:] -= f[:, None] * A[c, c:]
            r[c + 1:] -= f * r[c]
            rank = c + 1
            if np.isnan(A[c + 1:, c + 1:]).any():
                return None
        if rank == 0:
            return None
        y = np.zeros(rank, J.dtype)
        for c in range(rank - 1, -1, -1):
            y[c] = (r[c] - A[c, c + 1:rank] @ y[c + 1:]) / A[c, c]
        dp = np.zeros(n, J.dtype)
        dp[cols[:rank]] = y
        return dp


def _det3(A):
    return (A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0])
            + A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]))


def shoot(model, x0, p0, lo, hi, tf, N, substeps=4, max_newton=100, ftol=1e-3, par=None, dtype=np.float64):
    """gusto_shoot of ONE problem: dict(status, newton_iters, resid, p0, X, U); X, U are None unless status == 1"""
    dtype = np.dtype(dtype)
    n, _ = DIMS[model]
    x0, p, tf = np.asarray(x0, dtype), np.array(p0, dtype), dtype.type(tf)
    xg = goal_point(np.asarray(lo, dtype), np.asarray(hi, dtype))

    def end(ps):
        """F and |F|_inf for every start of ps [..., n]"""
        F = xg - extremal(model, x0, ps, tf, N, substeps, par, dtype)[0][..., N - 1, :]
        return F, norm_inf(F)

    a = dtype.type(0.5) ** np.arange(N_CAND)
    F, nf = end(p)
    it, ok = 0, 0
    with np.errstate(all="ignore"):
        while True:
            if not np.isfinite(nf):
                break
            if nf <= ftol:
                ok = 1
                break
            if it >= max_newton:
                break
            h = dtype.type(1e-6) * np.maximum(1, np.abs(p))
            Fj, _ = end(p + np.diag(h))                                      # row j: the start moved in component j
            dp = newton_step(((Fj - F) / h[:, None]).T, F)
            if dp is None:
                break
            Fc, nc = end(p + a[:, None] * dp)                                # every candidate of the line search
            better = np.flatnonzero(nc < nf)
            if better.size == 0:
                break
            c = better[0]
            p, F, nf = p + a[c] * dp, Fc[c], nc[c]
            it += 1
    X, U = extremal(model, x0, p, tf, N, substeps, par, dtype) if ok else (None, None)
    return dict(status=ok, newton_iters=it, resid=nf[()] if isinstance(nf, np.ndarray) else nf, p0=p, X=X, U=U)
