"""Independent numpy restatement of the convex subproblem of ONE GuSTO trip for all four models, written straight from
the reference's model files -- NOT through the oracle's row list:

  dynamics f            freeflyer_se2.jl:182-206, dubins_car.jl:161-165, astrobee_se3.jl:180-190 (+ quat_functions.jl:253-257),
                        astrobee_se3_manifold.jl:231-246
  Jacobians A, B        complex-step derivatives of f (no hand-written Jacobian table is shared with the oracle)
  trapezoid rows        dubins_car.jl:134-146, astrobee_se3_manifold.jl:169-195
  constraint registry   freeflyer_se2.jl:338-390, dubins_car.jl:184-226, astrobee_se3.jl:322-379, astrobee_se3_manifold.jl:533-608
  row functions         dynamics.jl:56-81, astrobee_se3.jl:244-263,282-305,308-311, astrobee_se3_manifold.jl:308-340,481-504
  penalisation          scp_gusto.jl:253-314 (incl. the +-eps pair of the convex_state_eq category, :297-311)
  signed distance       sphere vs AABB / sphere vs sphere in 3-D, disc vs AABB / disc in the plane for the freeflyer
                        (stands in for BulletCollision.distance)

subproblem_rows states the rows; solve_subproblem hands them to scipy SLSQP in the full slack form (variables X, U and one
slack per penalised row); np_kkt.certify checks a candidate point against them."""
import contextlib

import numpy as np
import scipy.optimize as so

PI = np.pi


# ---- robots / models (constants from robot/astrobee3D.jl:15-33, dubins_car.jl:22-33) ------------------------------
class Dubins:
    n, m = 3, 1
    v, k = 2.0, 1.0
    x_max, u_max = np.array([100.0, 100.0, 2 * PI]), 10.0
    Delta0, eps, clearance = 1e4, 1e-6, 0.01
    has_tr = False

    @staticmethod
    def f(x, u):
        return np.array([Dubins.v * np.cos(x[2]), Dubins.v * np.sin(x[2]), Dubins.k * u[0]])


class Astrobee:
    mass, J = 7.0, np.array([0.1083, 0.1083, 0.1083])       # J: the diagonal of the inertia
    r = np.sqrt(3.0) * 0.5 * 0.305
    v_max, a_max, w_max, al_max = 0.5, 0.1, 45 * PI / 180, 50 * PI / 180
    clearance = 0.03


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _per_axis(J, w):
    """the diagonal J shaped to scale the rows of w ([3] or [3, K])"""
    return np.reshape(J, (3,) + (1,) * (np.ndim(w) - 1))


class AstrobeeSE3(Astrobee):
    n, m = 12, 6
    Delta0, eps = 10.0, 1e-6
    has_tr = True

    @staticmethod
    def f(x, u):
        v, p, w = x[3:6], x[6:9], x[9:12]
        F, M = u[0:3], u[3:6]
        pd = 0.25 * ((1 - np.sum(p * p)) * w - 2 * _cross(w, p) + 2 * np.sum(w * p) * p)      # mrp_derivative
        J = _per_axis(Astrobee.J, w)
        wd = (M - _cross(w, J * w)) / J
        return np.concatenate([v, F / Astrobee.mass, pd, wd])


class AstrobeeSE3Manifold(Astrobee):
    n, m = 13, 6
    Delta0, eps = 1e3, 1e-1
    has_tr = False

    @staticmethod
    def f(x, u):
        v = x[3:6]
        qw, qx, qy, qz = x[6:10]
        wx, wy, wz = x[10:13]
        F, M = u[0:3], u[3:6]
        qd = 0.5 * np.array([-wx * qx - wy * qy - wz * qz, wx * qw - wz * qy + wy * qz, wy * qw + wz * qx - wx * qz,
                             wz * qw - wy * qx + wx * qy])
        w = x[10:13]
        J = _per_axis(Astrobee.J, w)
        wd = (M - _cross(w, J * w)) / J
        return np.concatenate([v, F / Astrobee.mass, qd, wd])


class FreeflyerSE2:
    """freeflyer_se2.jl:15-21,160-214 with robot/freeflyer.jl:28-62; state (r, theta, v, omega), control (F, M).  Its registry
    (freeflyer_se2.jl:338-390) has the penalised velocity rows, the trust region and the BODY obstacle rows (a disc of radius r
    against the keep-out components in the plane); the arm component (freeflyer.jl:55-57) enters trust_region_ratio_gusto only --
    ncsi_arm_obstacle_avoidance_constraints_convexified is written but not registered."""
    n, m = 6, 3
    mass, J = 0.5 * (15.36 + 18.08), np.array([0.184, 0.184, 0.184])    # the plane turns about z: J[2] (freeflyer.jl Jinv)
    r, clearance = 0.157, 0.05
    v_max, w_max = 0.2, 20 * PI / 180
    a_max, al_max = 2 * 0.185 / (0.5 * (15.36 + 18.08)), 0.593 / (0.184 / 6.43)
    Delta0, eps = 3.0, 1e-2
    has_tr = True
    J_AXIS = 2

    @staticmethod
    def f(x, u):
        return np.concatenate([x[3:6], u[0:2] / FreeflyerSE2.mass, u[2:3] / FreeflyerSE2.J[FreeflyerSE2.J_AXIS]])


def jac(model, x, u):
    """complex-step Jacobians of f"""
    n, m, h = model.n, model.m, 1e-30
    A, B = np.zeros((n, n)), np.zeros((n, m))
    for j in range(n):
        xc = x.astype(complex); xc[j] += 1j * h
        A[:, j] = model.f(xc, u.astype(complex)).imag / h
    for j in range(m):
        uc = u.astype(complex); uc[j] += 1j * h
        B[:, j] = model.f(x.astype(complex), uc).imag / h
    return A, B


# ---- non-default robot constants -----------------------------------------------------------------------------------------
_ROBOT = {0: FreeflyerSE2, 1: Dubins, 2: Astrobee, 3: Astrobee}


@contextlib.contextmanager
def model_params(model_id, mp):
    """Run a block with the robot constants of a ModelParams (the oracle's or the library's ctypes struct: the fields are read by
    name) in place of the defaults above -- mass, J, radius, clearance and the four hard limits; the Dubins car's v, k, u_max and
    clearance -- and put the defaults back afterwards.  mp = None leaves everything as it is."""
    cls = _ROBOT[model_id]
    if mp is None:
        yield
        return
    if cls is Dubins:
        new = dict(v=mp.dubins_v, k=mp.dubins_k, u_max=mp.u_max, clearance=mp.clearance)
    else:
        new = dict(mass=mp.mass, J=np.array([mp.Jdiag[0], mp.Jdiag[1], mp.Jdiag[2]]), r=mp.radius, clearance=mp.clearance,
                   v_max=mp.hard_limit_vel, a_max=mp.hard_limit_accel, w_max=mp.hard_limit_omega, al_max=mp.hard_limit_alpha)
    old = {k: getattr(cls, k) for k in new}
    for k, v in new.items():
        setattr(cls, k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            setattr(cls, k, v)


# ---- signed distance of a sphere (a disc in 2-D) of radius r centred at c ---------------------------------------------
def sd_box(c, lo, hi, r):
    d = len(c)
    lo, hi = np.asarray(lo)[:d], np.asarray(hi)[:d]
    e = np.where(c < lo, c - lo, np.where(c > hi, c - hi, 0.0))
    if np.any(e != 0):
        dist = np.linalg.norm(e)
        return dist - r, e / dist
    a, b = c - lo, hi - c          # inside: nearest face
    i = int(np.argmin(np.concatenate([a, b])))
    nh = np.zeros(d)
    if i < d:
        nh[i] = -1.0
        return -a[i] - r, nh
    nh[i - d] = 1.0
    return -b[i - d] - r, nh


def sd_sphere(c, cs, rs, r):
    v = c - np.asarray(cs)[:len(c)]
    d = np.linalg.norm(v)
    return d - rs - r, v / d


def subproblem_rows(model, N, tf, x_init, goal_lo, goal_hi, Xp, Up, Delta, omega, toggle=None, boxes=(), spheres=()):
    """The rows of one trip's convex subproblem (scp_gusto.jl:178-314) around (Xp, Up), on z = [x_0, u_0, x_1, u_1, ...]:

      E z = e                         init, trapezoid collocation, point-goal rows (dense E)
      hard[j](z) <= 0                 entries (fn, scale, kind): kind "goal" for BoxGoal rows, "hard" for the rest; `scale` > 0
                                      states the row in the units the certificate (np_kkt.py) measures it in -- the
                                      acceleration / control bounds relative to their limit, the hard half of the manifold's
                                      +-eps pair scaled by kappa like the penalised rows.  SLSQP sees the rows unscaled.
      kappa (w g_i(z) - off_i) <= s_i, s_i >= 0    penalised rows: entries (fn, w, off) of `pen`, tags in `pen_tag`
      minimise kappa sum_k wt_k |u_k|^2 + sum_i s_i,  kappa = 1 / max(1, omega), wt = trapezoid weights

    Every fn maps z to (value, (indices, gradient)).  `toggle` is the obstacle toggle distance (default Delta / 8 + clearance,
    what scp_gusto.jl:76 sets)."""
    n, m = model.n, model.m
    nz = n + m
    dt = tf / (N - 1)
    kappa = 1.0 / max(1.0, omega)
    if toggle is None:
        toggle = Delta / 8 + model.clearance
    nzN = nz * N
    ix = lambda k, i: nz * k + i
    iu = lambda k, i: nz * k + n + i

    # ---- equality rows: init, trapezoid collocation, goal points --------------------------------------------------
    rows, rhs = [], []
    for i in range(n):
        R = np.zeros(nzN); R[ix(0, i)] = 1.0
        rows.append(R); rhs.append(x_init[i])
    lin = [(model.f(Xp[k], Up[k]),) + jac(model, Xp[k], Up[k]) for k in range(N)]
    for k in range(1, N):
        (f0, A0, B0), (f1, A1, B1) = lin[k - 1], lin[k]
        R = np.zeros((n, nzN))
        R[:, nz * (k - 1):nz * (k - 1) + n] = np.eye(n) + 0.5 * dt * A0
        R[:, nz * (k - 1) + n:nz * k] = 0.5 * dt * B0
        R[:, nz * k:nz * k + n] = -np.eye(n) + 0.5 * dt * A1
        R[:, nz * k + n:nz * (k + 1)] = 0.5 * dt * B1
        c = 0.5 * dt * (f0 - A0 @ Xp[k - 1] - B0 @ Up[k - 1] + f1 - A1 @ Xp[k] - B1 @ Up[k])
        rows.extend(R); rhs.extend(-c)
    for i in range(n):
        if goal_lo[i] == goal_hi[i]:
            R = np.zeros(nzN); R[ix(N - 1, i)] = 1.0
            rows.append(R); rhs.append(goal_lo[i])
    E, e = np.array(rows), np.array(rhs, float)

    # ---- inequality rows as (value, gradient) callables of z; hard: g <= 0; penalised: kappa (w g - off) <= s ------
    hard, pen, pen_tag = [], [], []

    def quad(idx, coef, c0):     # sum coef_i z_i^2 + c0
        idx, coef = np.array(idx), np.array(coef, float)
        return lambda z: (float(np.sum(coef * z[idx] ** 2) + c0), (idx, 2 * coef * z[idx]))

    def lin_(idx, coef, c0):
        idx, coef = np.array(idx), np.array(coef, float)
        return lambda z: (float(np.sum(coef * z[idx]) + c0), (idx, coef))

    def quad_about(idx, ctr):    # sum (z_i - ctr_i)^2
        idx, ctr = np.array(idx), np.array(ctr, float)
        return lambda z: (float(np.sum((z[idx] - ctr) ** 2)), (idx, 2 * (z[idx] - ctr)))

    def add_pen(tag, fn, wt, off):
        pen.append((fn, wt, off)); pen_tag.append(tag)

    comps = [("b", b) for b in (boxes if boxes is not None else ())] + \
            [("s", s) for s in (spheres if spheres is not None else ())]
    for k in range(N):
        if model is Dubins:
            for i in range(n):      # csi_max/min_bound_constraints (dynamics.jl:56-64): penalised
                add_pen(("x_max", k, i), lin_([ix(k, i)], [1.0], -model.x_max[i]), omega, 0.0)
            for i in range(n):
                add_pen(("x_min", k, i), lin_([ix(k, i)], [-1.0], -model.x_max[i]), omega, 0.0)
            if k < N - 1:           # cci_max/min_bound_constraints (dynamics.jl:73-81): hard, k = 1..N-1
                hard.append((lin_([iu(k, 0)], [1.0], -model.u_max), 1 / model.u_max, "hard"))
                hard.append((lin_([iu(k, 0)], [-1.0], -model.u_max), 1 / model.u_max, "hard"))
            continue
        man = model is AstrobeeSE3Manifold
        se2 = model is FreeflyerSE2
        iv, nv = 3, (2 if se2 else 3)                     # velocity block
        iw, nw = (5, 1) if se2 else ((10, 3) if man else (9, 3))
        if model.has_tr:            # stri_state_trust_region: omega * ||x - xp||^2 - Delta <= s
            add_pen(("tr", k), quad_about([ix(k, i) for i in range(n)], Xp[k]), omega, Delta)
        if man:
            qp = Xp[k, 6:10]
            qn = np.linalg.norm(qp)
            # cse_quaternion_norm h = |qp| + qp.(q - qp)/|qp| - 1, penalised as the +-eps pair (scp_gusto.jl:297-311):
            #   j = 1:  -w h - eps <= -s1   (s1 >= 0 is minimised, so this is the HARD bound w h + eps >= 0)
            #   j = 2:   w h - eps <=  s2   (the L1 penalty on h > eps / w)
            hfun = lin_([ix(k, 6 + j) for j in range(4)], qp / qn, qn - np.sum(qp * qp) / qn - 1.0)
            hard.append(((lambda z, hf=hfun: (lambda v, g: (-(omega * v) - model.eps, (g[0], -omega * g[1])))(*hf(z))),
                         kappa, "hard"))
            add_pen(("qnorm", k), hfun, omega, model.eps)
            add_pen(("qw", k), lin_([ix(k, 6)], [-1.0], 0.0), omega, 0.0)           # csi_orientation_sign: -qw
        add_pen(("v", k), quad([ix(k, iv + j) for j in range(nv)], [1.0] * nv, -model.v_max ** 2), omega, 0.0)
        add_pen(("w", k), quad([ix(k, iw + j) for j in range(nw)], [1.0] * nw, -model.w_max ** 2), omega, 0.0)
        d_ws = 2 if se2 else 3      # workspace: the plane for the freeflyer (its obstacles are AABBs / spheres seen as discs)
        r0 = Xp[k, 0:d_ws]
        for i, (kind, o) in enumerate(comps):       # ncsi_*_obstacle_avoidance_..._convexified, body component
            d, nh = sd_box(r0, o[0:3], o[3:6], model.r) if kind == "b" else sd_sphere(r0, o[0:3], o[3], model.r)
            if d < toggle:
                add_pen(("obs", k, i), lin_([ix(k, j) for j in range(d_ws)], -nh, model.clearance - d + nh @ r0), omega, 0.0)
        if k < N - 1:               # cci_translational/angular_accel_bound: hard, k = 1..N-1
            nf, im, nm = (2, 2, 1) if se2 else (3, 3, 3)
            hard.append((quad([iu(k, j) for j in range(nf)], [1 / model.mass ** 2] * nf, -model.a_max ** 2),
                         1 / model.a_max ** 2, "hard"))
            Jm = [model.J[model.J_AXIS]] if se2 else model.J              # 1 / J_j^2 per axis
            hard.append((quad([iu(k, im + j) for j in range(nm)], [1 / Jm[j] ** 2 for j in range(nm)], -model.al_max ** 2),
                         1 / model.al_max ** 2, "hard"))
    for i in range(n):              # csbci_goal_constraints (BoxGoal): hard
        if goal_lo[i] != goal_hi[i]:
            if np.isfinite(goal_hi[i]):
                hard.append((lin_([ix(N - 1, i)], [1.0], -goal_hi[i]), 1.0, "goal"))
            if np.isfinite(goal_lo[i]):
                hard.append((lin_([ix(N - 1, i)], [-1.0], goal_lo[i]), 1.0, "goal"))

    wt = np.full(N, dt); wt[0] = wt[-1] = 0.5 * dt
    uidx = np.array([[iu(k, j) for j in range(m)] for k in range(N)])
    return dict(n=n, m=m, N=N, nzN=nzN, kappa=kappa, omega=omega, E=E, e=e, hard=hard, pen=pen, pen_tag=pen_tag,
                wt=wt, uidx=uidx)


def solve_subproblem(model, N, tf, x_init, goal_lo, goal_hi, Xp, Up, Delta, omega, boxes=(), spheres=(), maxiter=400,
                     toggle=None):
    """One trip's convex subproblem (subproblem_rows) by SLSQP in its full slack form.  Returns X, U, objective (unscaled)."""
    R = subproblem_rows(model, N, tf, x_init, goal_lo, goal_hi, Xp, Up, Delta, omega, toggle, boxes, spheres)
    n, m, nzN, kappa, E, e = R["n"], R["m"], R["nzN"], R["kappa"], R["E"], R["e"]
    pen, hard = R["pen"], [h[0] for h in R["hard"]]
    ns = len(pen)
    w, uidx = R["wt"], R["uidx"]

    def obj(z):
        return kappa * float(np.sum(w[:, None] * z[uidx] ** 2)) + float(z[nzN:].sum())

    def obj_grad(z):
        g = np.zeros_like(z)
        g[uidx] = 2 * kappa * w[:, None] * z[uidx]
        g[nzN:] = 1.0
        return g

    def ineq(z):                    # >= 0
        out = [z[nzN + j] - kappa * (wt * fn(z)[0] - off) for j, (fn, wt, off) in enumerate(pen)]
        out += [-fn(z)[0] for fn in hard]
        return np.array(out)

    def ineq_jac(z):
        Jm = np.zeros((ns + len(hard), len(z)))
        for j, (fn, wt, off) in enumerate(pen):
            idx, gr = fn(z)[1]
            Jm[j, idx] = -kappa * wt * gr
            Jm[j, nzN + j] = 1.0
        for j, fn in enumerate(hard):
            idx, gr = fn(z)[1]
            Jm[ns + j, idx] = -gr
        return Jm

    z0 = np.concatenate([np.hstack([Xp, Up]).ravel(), np.ones(ns)])
    Epad = np.hstack([E, np.zeros((E.shape[0], ns))])
    res = so.minimize(obj, z0, jac=obj_grad, method="SLSQP",
                      constraints=[{"type": "eq", "fun": lambda z: Epad @ z - e, "jac": lambda z: Epad},
                                   {"type": "ineq", "fun": ineq, "jac": ineq_jac}],
                      bounds=[(None, None)] * nzN + [(0, None)] * ns, options={"ftol": 1e-15, "maxiter": maxiter})
    Z = res.x[:nzN].reshape(N, n + m)
    return dict(X=Z[:, :n], U=Z[:, n:], obj=res.fun / kappa, res=res, n_pen=ns, n_hard=len(hard), rows=R,
                eq_violation=float(np.abs(Epad @ res.x - e).max()), ineq_min=float(ineq(res.x).min()))
