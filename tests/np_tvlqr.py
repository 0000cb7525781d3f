"""Independent numpy restatement of gusto_tvlqr (include/gusto_hip.h): the zero-order-hold RK4 roll-out map F_k of every knot
interval, its Jacobians Ad_k = dF_k/dx, Bd_k = dF_k/du by complex step through the WHOLE roll-out, and the finite-horizon
discrete Riccati recursion in its plainest form.  numpy only; shares no code with the kernels: the dynamics are np_models' f
(written from the reference's model files, safe for complex arguments), no hand-written Jacobian is used anywhere.

Also here: the deterministic smooth test trajectories of tests/test_gpu_tvlqr.py (a straight line plus seeded sinusoids)."""
import numpy as np

import np_models as M

MODELS = {0: M.FreeflyerSE2, 1: M.Dubins, 2: M.AstrobeeSE3, 3: M.AstrobeeSE3Manifold}
H_CS = 1e-30


def n_substeps(tf, N, dt_min=0.1, nstep=0):
    return int(nstep) if nstep > 0 else int(np.ceil(tf / (N - 1) / dt_min))


def rollout(model, x, u, dt, nstep):
    """F(x, u): nstep classical RK4 steps of dt / nstep under the held control u; x, u may be complex"""
    h = dt / nstep
    f = model.f
    for _ in range(nstep):
        k1 = f(x, u)
        k2 = f(x + 0.5 * h * k1, u)
        k3 = f(x + 0.5 * h * k2, u)
        k4 = f(x + h * k3, u)
        x = x + h / 6.0 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


def jacobians(model_id, x, u, dt, nstep):
    """[Ad | Bd] of one interval, n x (n + m), by complex step (h = 1e-30) through the whole roll-out"""
    model = MODELS[model_id]
    n, m = model.n, model.m
    AB = np.zeros((n, n + m))
    for j in range(n + m):
        xc, uc = np.asarray(x, float).astype(complex), np.asarray(u, float).astype(complex)
        if j < n:
            xc[j] += 1j * H_CS
        else:
            uc[j - n] += 1j * H_CS
        AB[:, j] = rollout(model, xc, uc, dt, nstep).imag / H_CS
    return AB


_BATCH_SAFE_F = (0, 1, 3)      # np_models' f of these models works on [n, K] arrays as it stands (np_verify.py uses the same fact)


def linearise(model_id, X, U, tf, dt_min=0.1, nstep=0):
    """AB [N-1, n, n+m] of one trajectory X [N, n], U [N, m]: `jacobians` of every interval.  Where f takes arrays the
    (N - 1)(n + m) perturbed roll-outs run side by side as columns -- the same arithmetic per column (tests/test_tvlqr_cpu.py)."""
    N = len(X)
    dt = tf / (N - 1)
    ns = n_substeps(tf, N, dt_min, nstep)
    if model_id not in _BATCH_SAFE_F:
        return np.stack([jacobians(model_id, X[k], U[k], dt, ns) for k in range(N - 1)])
    model = MODELS[model_id]
    n, m = model.n, model.m
    nz = n + m
    Xc = np.repeat(np.asarray(X[:N - 1], float).T, nz, axis=1).astype(complex)      # column k nz + j: interval k, perturbation j
    Uc = np.repeat(np.asarray(U[:N - 1], float).T, nz, axis=1).astype(complex)
    cols = np.arange((N - 1) * nz)
    j = cols % nz
    Xc[j[j < n], cols[j < n]] += 1j * H_CS
    Uc[j[j >= n] - n, cols[j >= n]] += 1j * H_CS
    D = rollout(model, Xc, Uc, dt, ns).imag / H_CS                                   # [n, (N-1) nz]
    return np.ascontiguousarray(D.reshape(n, N - 1, nz).transpose(1, 0, 2))


def riccati(AB, Q, R, Qf):
    """K [N-1, m, n], P [N, n, n] (P[N-1] = diag(Qf)) from AB [N-1, n, n+m] and the diagonal weights:
    K = solve(R + B'PB, B'PA), P = Q + A'P(A - BK), symmetrised"""
    Nm1, n, nz = AB.shape
    m = nz - n
    Q, R, Qf = (np.diag(np.broadcast_to(np.asarray(v, float), (d,))) for v, d in ((Q, n), (R, m), (Qf, n)))
    P = np.zeros((Nm1 + 1, n, n))
    K = np.zeros((Nm1, m, n))
    P[Nm1] = Qf
    for k in range(Nm1 - 1, -1, -1):
        A, B = AB[k, :, :n], AB[k, :, n:]
        K[k] = np.linalg.solve(R + B.T @ P[k + 1] @ B, B.T @ P[k + 1] @ A)
        Pk = Q + A.T @ P[k + 1] @ (A - B @ K[k])
        P[k] = 0.5 * (Pk + Pk.T)
    return K, P


def tvlqr(model_id, X, U, tf, Q, R, Qf, dt_min=0.1, nstep=0):
    AB = linearise(model_id, X, U, tf, dt_min, nstep)
    K, P = riccati(AB, Q, R, Qf)
    return AB, K, P


# ---- test inputs ----------------------------------------------------------------------------------------------------------
# controls of the size of the models' limits (mass a_max, J alpha_max; the Dubins turn rate), states inside the models' ranges
_U_SCALE = {0: np.array([0.37, 0.37, 0.59]), 1: np.array([1.0]),
            2: np.array([0.7, 0.7, 0.7, 0.09, 0.09, 0.09]), 3: np.array([0.7, 0.7, 0.7, 0.09, 0.09, 0.09])}
_X_A = {0: np.array([0.3, 2.2, 0.1, 0.02, -0.03, 0.05]), 1: np.array([0.0, 0.0, 0.2]),
        2: np.array([10.0, -0.5, 5.0, 0.02, 0.03, -0.02, 0.05, -0.1, 0.1, 0.05, -0.04, 0.03]),
        3: np.array([10.0, -0.5, 5.0, 0.02, 0.03, -0.02, 0.9, 0.1, -0.3, 0.2, 0.05, -0.04, 0.03])}
_X_B = {0: np.array([3.0, 0.5, 1.2, 0.05, -0.05, -0.02]), 1: np.array([8.0, 5.0, 1.5]),
        2: np.array([11.0, 3.0, 5.5, -0.03, 0.02, 0.04, -0.2, 0.25, 0.1, -0.05, 0.06, 0.02]),
        3: np.array([11.0, 3.0, 5.5, -0.03, 0.02, 0.04, 0.6, -0.4, 0.5, 0.3, -0.05, 0.06, 0.02])}
_X_AMP = {0: np.array([0.2, 0.2, 0.3, 0.03, 0.03, 0.05]), 1: np.array([0.5, 0.5, 0.4]),
          2: np.array([0.2, 0.2, 0.2, 0.05, 0.05, 0.05, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]),
          3: np.array([0.2, 0.2, 0.2, 0.05, 0.05, 0.05, 0.2, 0.2, 0.2, 0.2, 0.1, 0.1, 0.1])}


def smooth_batch(model_id, B, N, seed=0):
    """X [B, N, n], U [B, N, m]: a straight line between two fixed states plus seeded sinusoids, controls of the size of the
    model's limits; the manifold model's quaternion is normalised at the knots"""
    rng = np.random.default_rng(1000 * model_id + seed)
    model = MODELS[model_id]
    n, m = model.n, model.m
    s = np.linspace(0.0, 1.0, N)[None, :, None]
    X = _X_A[model_id] * (1 - s) + _X_B[model_id] * s + np.zeros((B, 1, 1))
    for _ in range(2):
        w, ph = rng.uniform(0.5, 3.0, (B, 1, n)), rng.uniform(0, 2 * np.pi, (B, 1, n))
        X = X + 0.5 * _X_AMP[model_id] * rng.uniform(-1, 1, (B, 1, n)) * np.sin(2 * np.pi * w * s + ph)
    w, ph = rng.uniform(0.5, 3.0, (B, 1, m)), rng.uniform(0, 2 * np.pi, (B, 1, m))
    U = _U_SCALE[model_id] * rng.uniform(0.3, 1.0, (B, 1, m)) * np.sin(2 * np.pi * w * s + ph)
    if model_id == 3:
        X[..., 6:10] /= np.linalg.norm(X[..., 6:10], axis=-1, keepdims=True)
    return np.ascontiguousarray(X), np.ascontiguousarray(U)


def weights(model_id, seed=0):
    """non-uniform diagonal Q, R, Qf: different per entry, spanning 1e-2 .. 1e2"""
    model = MODELS[model_id]
    rng = np.random.default_rng(77 + 10 * model_id + seed)

    def span(d):
        e = np.linspace(-2.0, 2.0, d) if d > 1 else np.array([0.5])
        return 10.0 ** rng.permutation(e)
    return span(model.n), span(model.m), span(model.n)
