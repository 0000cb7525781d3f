// rk4_step.inc -- one classical RK4 step of h of the state under the held control: the statements of rk4_step (rollout.hpp), which
// is this text in a function.  simulate_kernel (simulate.hip) includes it instead of calling: rollout.hpp says why.
// In scope at the include:
//   D = Dyn<MODEL>, n = MT<MODEL>::n
//   double x[n]       the state, advanced by the step
//   double u[m], h    the held control, the step
//   RK4_STEP_MP       the model parameters f is evaluated with (gusto_simulate_disturbed: a lane's own plant)
//   RK4_STEP_NEW(i)   a statement behind the update of x[i] (simulate_kernel: its finiteness test; rk4_step: nothing)
//                     Both are undefined again at the end of this text
{
    double k1[n], kk[n], w[n], xs[n];
    D::f(RK4_STEP_MP, x, u, k1);
#pragma unroll
    for (int i = 0; i < n; i++) { xs[i] = k1[i]; w[i] = x[i] + 0.5 * h * k1[i]; }
    D::f(RK4_STEP_MP, w, u, kk);
#pragma unroll
    for (int i = 0; i < n; i++) { xs[i] += 2 * kk[i]; w[i] = x[i] + 0.5 * h * kk[i]; }
    D::f(RK4_STEP_MP, w, u, kk);
#pragma unroll
    for (int i = 0; i < n; i++) { xs[i] += 2 * kk[i]; w[i] = x[i] + h * kk[i]; }
    D::f(RK4_STEP_MP, w, u, kk);
#pragma unroll
    for (int i = 0; i < n; i++) {
        x[i] = x[i] + 1.0 / 6.0 * h * (xs[i] + kk[i]);
        RK4_STEP_NEW(i);
    }
}
#undef RK4_STEP_MP
#undef RK4_STEP_NEW
