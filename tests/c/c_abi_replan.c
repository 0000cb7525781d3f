/* c_abi_replan.c -- plain C through include/gusto_hip.h: the replanning entry points.
 * Three freeflyerSE2 problems (N = 50) next to one box: solved, tracked (gusto_tvlqr), flown (gusto_simulate, two samples,
 * store_knots = 1), then replanned at knot 5 from the second sample -- in place with gusto_set_problems_replan_knots and, on a
 * second handle, with gusto_set_problems_replan from the same states fetched by gusto_get_simulate_knots: the same start bit for
 * bit.  Two refusals, gusto_get_replan, gusto_last_replan_ms and the state errors after gusto_set_problems, with checks of its
 * own; then one line "ok" and, per problem, seeded, tau, x_now[0], x_now[1] and the SCP iterations of the replanned solve, which
 * tests/test_gpu_replan.py compares with the Python path.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_replan.c -o c_abi_replan -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 50, B = 3, S = 2, NX = 6, NU = 3, KNOT = 5 };
    gusto_handle h = 0, h2 = 0;
    const double box[6] = {1.4, 0.9, -0.2, 1.8, 1.5, 0.2};
    const double x_init[B * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.4, 1.9, 0, 0, 0, 0, 0.3, 0.4, 0, 0, 0, 0};
    const double goal[B * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    const double tf[B] = {200.0, 150.0, 100.0};
    const int knot[B] = {KNOT, KNOT, KNOT}, bad_knot[B] = {KNOT, N - 1, KNOT};
    static double X[B * N * NX], U[B * N * NU], X2[B * N * NX], U2[B * N * NU], Xcl[B * N * S * NX];
    double tau[B] = {0}, x_now[B * NX] = {0}, tau_g[B], x_g[B * NX], bad_tau[B], ms = -1.0;
    int seeded[B], seeded2[B], conv[B], succ[B], iters[B];
    gusto_tvlqr_opts to;
    gusto_simulate_opts so;

    REQUIRE(gusto_set_problems_replan(0, 0, GUSTO_REPLAN_TRAJ, B, tau, x_now, 0, 0, 0) == GUSTO_ERR_ARG);
    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 64, 0));
    CHECK(gusto_create(&h2, GUSTO_FREEFLYER_SE2, N, B, 64, 0));
    CHECK(gusto_set_env(h, 1, box, 0, 0));
    CHECK(gusto_set_env(h2, 1, box, 0, 0));
    REQUIRE(gusto_set_problems_replan(h, 0, GUSTO_REPLAN_TRAJ, B, tau, x_now, 0, 0, 0) == GUSTO_ERR_STATE);   /* no source problems */
    REQUIRE(gusto_get_replan(h, seeded, tau_g, x_g) == GUSTO_ERR_STATE);
    CHECK(gusto_set_problems(h, B, x_init, goal, goal, tf, 0, 0));
    CHECK(gusto_solve(h, 30, 0));
    CHECK(gusto_get_status(h, 0, conv, succ, 0, 0));
    REQUIRE(gusto_set_problems_replan_knots(h, 0, B, knot, 1, 0, 0, 0) == GUSTO_ERR_STATE);                   /* no stored knots */
    CHECK(gusto_default_tvlqr_opts(GUSTO_FREEFLYER_SE2, &to));
    CHECK(gusto_tvlqr(h, 0, 0, &to));
    CHECK(gusto_default_simulate_opts(GUSTO_FREEFLYER_SE2, &so));
    so.n_samples = S; so.store_knots = 1;
    CHECK(gusto_simulate(h, 0, 0, 0, 0, &so));
    CHECK(gusto_get_simulate_knots(h, Xcl));
    CHECK(gusto_get_traj(h, X, U));

    /* the general call on a second handle, from the host's copy of the same states */
    for (int b = 0; b < B; b++) {
        tau[b] = (double)KNOT / (double)(N - 1);
        bad_tau[b] = b == 1 ? 1.0 : tau[b];
        memcpy(x_now + b * NX, Xcl + (((size_t)b * N + KNOT) * S + 1) * NX, sizeof(double) * NX);
    }
    REQUIRE(gusto_set_problems_replan(h2, h, GUSTO_REPLAN_TRAJ, B, bad_tau, x_now, 0, 0, 0) == GUSTO_ERR_ARG);   /* tau = 1 */
    REQUIRE(strstr(gusto_last_error(h2), "tau"));
    REQUIRE(gusto_get_traj(h2, X2, U2) == GUSTO_ERR_STATE);                          /* the refusal left h2 without problems */
    CHECK(gusto_set_problems_replan(h2, h, GUSTO_REPLAN_TRAJ, B, tau, x_now, 0, 0, 0));
    CHECK(gusto_get_traj(h2, X2, U2));
    CHECK(gusto_get_replan(h2, seeded2, tau_g, x_g));
    REQUIRE(!memcmp(tau_g, tau, sizeof(tau)) && !memcmp(x_g, x_now, sizeof(x_now)));
    for (int b = 0; b < B; b++) {
        REQUIRE(seeded2[b] == (conv[b] && succ[b]));
        REQUIRE(!memcmp(X2 + (size_t)b * N * NX, x_now + b * NX, sizeof(double) * NX));                       /* knot 0 is x_now */
        if (seeded2[b]) {                                                                                    /* the source's last knot */
            REQUIRE(!memcmp(X2 + ((size_t)b * N + N - 1) * NX, X + ((size_t)b * N + N - 1) * NX, sizeof(double) * NX));
            REQUIRE(!memcmp(U2 + ((size_t)b * N + N - 1) * NU, U + ((size_t)b * N + N - 1) * NU, sizeof(double) * NU));
        }
    }
    /* in place, from the stored knots */
    REQUIRE(gusto_set_problems_replan_knots(h, 0, B, bad_knot, 1, 0, 0, 0) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_replan_knots(h, 0, B, knot, S, 0, 0, 0) == GUSTO_ERR_ARG);
    CHECK(gusto_set_problems_replan_knots(h, 0, B, knot, 1, 0, 0, 0));
    CHECK(gusto_get_traj(h, X, U));
    REQUIRE(!memcmp(X, X2, sizeof(X)) && !memcmp(U, U2, sizeof(U)));
    CHECK(gusto_get_replan(h, seeded, tau_g, x_g));
    REQUIRE(!memcmp(seeded, seeded2, sizeof(seeded)) && !memcmp(tau_g, tau, sizeof(tau)) && !memcmp(x_g, x_now, sizeof(x_now)));
    CHECK(gusto_last_replan_ms(h, &ms));
    REQUIRE(ms > 0.0);
    REQUIRE(gusto_get_simulate_knots(h, Xcl) == GUSTO_ERR_STATE);                    /* new problems: the roll-outs are gone */
    CHECK(gusto_solve(h, 30, 0));
    CHECK(gusto_get_status(h, iters, conv, succ, 0, 0));

    CHECK(gusto_set_problems(h2, B, x_init, goal, goal, tf, 0, 0));                  /* set by another call */
    REQUIRE(gusto_get_replan(h2, 0, 0, 0) == GUSTO_ERR_STATE && gusto_last_replan_ms(h2, &ms) == GUSTO_ERR_STATE);

    printf("ok\n");
    for (int b = 0; b < B; b++) printf("%d %.17g %.17g %.17g %d\n", seeded[b], tau_g[b], x_g[b * NX], x_g[b * NX + 1], iters[b]);
    CHECK(gusto_destroy(h2));
    CHECK(gusto_destroy(h));
    return 0;
}
