// rollout.hpp -- THE roll-out of the post-solve stages (verify.hip, tvlqr.hip, simulate.hip, lincov.hip; nothing else includes it):
// Nstep classical RK4 steps of dt / Nstep per knot interval under the held control, as include/gusto_hip.h defines it.  The
// Jacobians of gusto_tvlqr and the sensitivities of gusto_lincov_disturbed are the derivative of what gusto_verify and
// gusto_simulate integrate because both are written here once: a change of the integrator is made in rk4_step.inc and in
// rk4_tangent.inc, nowhere else.  (shoot.hip integrates the reference's costate ODE with h / 6.0 * (...), which rounds
// differently, and keeps its own text.)
//   rollout_nstep, tangent, robot_min_distance: functions.
//   the RK4 step of the state: rk4_step.inc.  verify_kernel calls it as the function rk4_step (astrobeeSE3 156 -> 142 VGPRs,
//     manifold 166 -> 150).  simulate_kernel includes the text, with its finiteness test inside the update loop: that keeps its
//     instruction bytes, and so its bits, what they were; as a call it did not (profiles/post_rollout.txt 3(c)).
//   the RK4 step of the state AND one tangent column: rk4_tangent.inc, included text like scp_body.inc.  As a function the
//     three linearising kernels lose the sharing between f and A at a stage point: tvlqr_linearise<dubins> 100 -> 138 VGPRs,
//     lincov_dense<astrobeeSE3> 169 -> 434, lincov_plant_sens<astrobeeSE3> 250 -> 366 (profiles/post_rollout.txt 3(a)).  As
//     text the kernels' instruction bytes are those they had.
#pragma once
#include "models.hpp"

namespace gusto {

constexpr int NO_HIT = 1 << 30;    // robot_min_distance: no penetrating pair (ordinals stay below 2 * 64)

// substeps per knot interval: the caller's count, or ceil(dt / dt_min).  The host has checked 1 <= Nstep <= nstep_cap before any
// launch (post.hpp: resolve_nstep; gusto_lincov* reads the options gusto_tvlqr checked and kept)
GD int rollout_nstep(double dt, int nstep, double dt_min) { return nstep > 0 ? nstep : (int)ceil(dt / dt_min); }

// one classical RK4 step of h of the state x under the held control u, with the model parameters mp (gusto_simulate_disturbed: a
// lane's own plant).  The stage sum is accumulated left to right, k1 + 2 k2 + 2 k3 + k4
template <int MODEL> GD void rk4_step(const gusto_model_params& mp, double* x, const double* u, double h) {
    using D = Dyn<MODEL>;
    constexpr int n = MT<MODEL>::n;
#define RK4_STEP_MP mp
#define RK4_STEP_NEW(i)
#include "rk4_step.inc"
}

// kd = A d + g over the structural nonzeros of A (MT<MODEL>::Anz: the loops are unrolled, so the pattern is a compile-time
// choice per product -- a product with a constant 0.0 is not something the compiler may drop on its own in IEEE arithmetic)
template <int MODEL> GD void tangent(const double* A, const double* d, const double* g, double* kd) {
    constexpr int n = MT<MODEL>::n;
#pragma unroll
    for (int i = 0; i < n; i++) {
        double s = g[i];
#pragma unroll
        for (int j = 0; j < n; j++)
            if (MT<MODEL>::Anz(i, j)) s += A[i * n + j] * d[j];
        kd[i] = s;
    }
}

// smallest signed distance of the robot at state x over components and obstacles.  HIT: with a non-null `hit` also the first
// penetrating pair in loop order (its ordinal component n_obs + obstacle and its distance; *hit starts as NO_HIT).  The form is
// measured, not chosen: verify_kernel instantiates HIT for its dense samples too and passes nulls -- with the bookkeeping
// compiled out there gusto_interpolate of 8192 astrobeeSE3 problems ran 1.1 % slower -- and without HIT there is no local for
// the distance, which keeps simulate_kernel's instruction bytes what they were (profiles/post_rollout.txt 3(d))
template <int MODEL, bool HIT = false>
GD double robot_min_distance(const KParams& P, const Env& E, const double* x, int* hit = nullptr, double* hit_d = nullptr) {
    using T = MT<MODEL>;
    double dmin = INFINITY;
    for (int c = 0; c < P.mp.n_robot_comp; c++)
        for (int i = 0; i < E.n_obs; i++) {
            double nh[T::WS];
            if constexpr (HIT) {
                const double d = signed_distance<T::WS>(P, E, c, x, i, nh);
                dmin = fmin(dmin, d);
                if (hit && d < 0 && *hit == NO_HIT) { *hit = c * E.n_obs + i; *hit_d = d; }
            } else {
                dmin = fmin(dmin, signed_distance<T::WS>(P, E, c, x, i, nh));
            }
        }
    return dmin;
}

}  // namespace gusto
