// rk4_tangent.inc -- one classical RK4 step of h of the state AND one tangent column, d' = A(x) d + g: rk4_step (rollout.hpp) with
// forward-mode differentiation carried through its four stages.  Included into the substep loop of tvlqr_linearise (tvlqr.hip),
// lincov_plant_sens and lincov_dense (lincov.hip).  Text, not a function: rollout.hpp says why.
// In scope at the include:
//   MODEL, D = Dyn<MODEL>, n = MT<MODEL>::n, P (the kernel's KParams: the dynamics are evaluated with P.mp)
//   double x[n], d[n]   the state and the tangent column; both are advanced by the step
//   double u[m], h      the held control, the step
//   RK4_TANGENT_SOURCE(xp, g)   an expression the includer defines: the source term at the stage point xp as a const double* --
//                               a vector the includer holds (B e_j), or the scratch double g[n] after filling it
//                               (df/dtheta_j(xp, u)).  Undefined again at the end of this text
{
    [[maybe_unused]] double g[n];   // (an includer whose source is a vector of its own never touches it)
    double A[n * n], w[n], dw[n], k1[n], kk[n], kd1[n], kdk[n], xs[n], ds[n];
    D::f(P.mp, x, u, k1);
    D::A(P.mp, x, u, A);
    tangent<MODEL>(A, d, RK4_TANGENT_SOURCE(x, g), kd1);
#pragma unroll
    for (int i = 0; i < n; i++) { xs[i] = k1[i]; ds[i] = kd1[i]; w[i] = x[i] + 0.5 * h * k1[i]; dw[i] = d[i] + 0.5 * h * kd1[i]; }
    D::f(P.mp, w, u, kk);
    D::A(P.mp, w, u, A);
    tangent<MODEL>(A, dw, RK4_TANGENT_SOURCE(w, g), kdk);
#pragma unroll
    for (int i = 0; i < n; i++) { xs[i] += 2 * kk[i]; ds[i] += 2 * kdk[i]; w[i] = x[i] + 0.5 * h * kk[i]; dw[i] = d[i] + 0.5 * h * kdk[i]; }
    D::f(P.mp, w, u, kk);
    D::A(P.mp, w, u, A);
    tangent<MODEL>(A, dw, RK4_TANGENT_SOURCE(w, g), kdk);
#pragma unroll
    for (int i = 0; i < n; i++) { xs[i] += 2 * kk[i]; ds[i] += 2 * kdk[i]; w[i] = x[i] + h * kk[i]; dw[i] = d[i] + h * kdk[i]; }
    D::f(P.mp, w, u, kk);
    D::A(P.mp, w, u, A);
    tangent<MODEL>(A, dw, RK4_TANGENT_SOURCE(w, g), kdk);
#pragma unroll
    for (int i = 0; i < n; i++) {
        x[i] = x[i] + 1.0 / 6.0 * h * (xs[i] + kk[i]);
        d[i] = d[i] + 1.0 / 6.0 * h * (ds[i] + kdk[i]);
    }
}
#undef RK4_TANGENT_SOURCE
