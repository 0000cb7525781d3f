/* c_abi_tighten.c -- plain C through include/gusto_hip.h: the risk-tightened keep-out sets.
 * Three freeflyerSE2 problems (N = 50) next to one box: solved, tracked (gusto_tvlqr), analysed (gusto_lincov with actuator noise
 * and store_S = 1), then gusto_tighten_env from the base box with kappa = 3, the tables read back with gusto_get_env, and a
 * re-solve from the own plans (gusto_set_problems_replan, tau = 0).  Refusals before and after, each leaving the handle's tables
 * as they were, gusto_get_tighten, gusto_last_tighten_ms, with checks of its own; then one line "ok" and, per problem, status,
 * knot, pair, n_grown, blocked, min_z_base, the margin and the four tightened corners of the box in the plane, which
 * tests/test_gpu_tighten.py compares with the Python path.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_tighten.c -o c_abi_tighten -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 50, B = 3, NX = 6, NU = 3 };
    gusto_handle h = 0;
    const double box[6] = {1.4, 0.9, -0.2, 1.8, 1.5, 0.2};
    const double bad_box[6] = {1.4, 0.9, -0.2, 1.8, INFINITY, 0.2};
    const double x_init[B * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.4, 1.9, 0, 0, 0, 0, 0.3, 0.4, 0, 0, 0, 0};
    const double goal[B * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    const double tf[B] = {200.0, 150.0, 100.0}, tau[B] = {0, 0, 0};
    const int one = 1, zero = 0, many = 65, two[2] = {1, 1};
    int n_env = -1, nb[B], ns[B], n_obs_max = -1, conv[B], succ[B];
    int status[B], knot[B], pair[B], n_grown[B], blocked[B], lc_knot[B], lc_pair[B];
    double tb[B * 6], margin[B], min_z[B], max_m[B], lc_z[B], ms = -1.0, env0[6];
    gusto_tvlqr_opts to;
    gusto_lincov_opts lo;
    gusto_tighten_opts o;
    gusto_tighten_report rep;
    gusto_lincov_report lrep;

    REQUIRE(gusto_default_tighten_opts(GUSTO_FREEFLYER_SE2, 0) == GUSTO_ERR_ARG);
    REQUIRE(gusto_default_tighten_opts(9, &o) == GUSTO_ERR_ARG);
    CHECK(gusto_default_tighten_opts(GUSTO_FREEFLYER_SE2, &o));
    REQUIRE(o.kappa == 3.0 && o.slack == 0.0 && isinf(o.margin_cap) && isinf(o.reach) && o.cover_components == 1 && o.monotone == 1);
    REQUIRE(gusto_tighten_env(0, 1, &one, box, &zero, 0, &o) == GUSTO_ERR_ARG);
    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 64, 0));
    CHECK(gusto_get_env(h, &n_env, nb, 0, ns, 0));
    REQUIRE(n_env == 1 && nb[0] == 0 && ns[0] == 0);                                  /* before any gusto_set_env */
    CHECK(gusto_set_env(h, 1, box, 0, 0));
    REQUIRE(gusto_tighten_env(h, 1, &one, box, &zero, 0, &o) == GUSTO_ERR_STATE);     /* no problems */
    CHECK(gusto_set_problems(h, B, x_init, goal, goal, tf, 0, 0));
    REQUIRE(gusto_tighten_env(h, 1, &one, box, &zero, 0, &o) == GUSTO_ERR_STATE);     /* no covariances */
    REQUIRE(gusto_get_tighten(h, 0, &n_obs_max) == GUSTO_ERR_STATE);
    CHECK(gusto_solve(h, 30, 0));
    CHECK(gusto_get_status(h, 0, conv, succ, 0, 0));
    CHECK(gusto_default_tvlqr_opts(GUSTO_FREEFLYER_SE2, &to));
    CHECK(gusto_tvlqr(h, 0, 0, &to));
    CHECK(gusto_default_lincov_opts(GUSTO_FREEFLYER_SE2, &lo));
    for (int i = 0; i < NU; i++) lo.du_white[i] = 0.0074;
    CHECK(gusto_lincov(h, 0, 0, 0, 0, &lo));
    REQUIRE(gusto_tighten_env(h, 1, &one, box, &zero, 0, &o) == GUSTO_ERR_STATE);     /* store_S = 0 */
    lo.store_S = 1;
    CHECK(gusto_lincov(h, 0, 0, 0, 0, &lo));
    memset(&lrep, 0, sizeof(lrep));
    lrep.min_z_obs = lc_z; lrep.obs_knot = lc_knot; lrep.obs_pair = lc_pair;
    CHECK(gusto_get_lincov(h, &lrep));

    /* refusals: the handle's tables stay the shared box */
    REQUIRE(gusto_tighten_env(h, 2, two, box, two, 0, &o) == GUSTO_ERR_ARG);          /* n_env neither 1 nor B */
    REQUIRE(gusto_tighten_env(h, 1, &many, box, &zero, 0, &o) == GUSTO_ERR_ARG);      /* 65 components */
    REQUIRE(gusto_tighten_env(h, 1, &one, bad_box, &zero, 0, &o) == GUSTO_ERR_ARG);   /* a non-finite entry */
    o.kappa = -1.0;
    REQUIRE(gusto_tighten_env(h, 1, &one, box, &zero, 0, &o) == GUSTO_ERR_ARG);
    REQUIRE(strstr(gusto_last_error(h), "kappa"));
    o.kappa = 3.0; o.monotone = 2;
    REQUIRE(gusto_tighten_env(h, 1, &one, box, &zero, 0, &o) == GUSTO_ERR_ARG);
    o.monotone = 1;
    CHECK(gusto_get_env(h, &n_env, nb, env0, ns, 0));
    REQUIRE(n_env == 1 && nb[0] == 1 && ns[0] == 0 && !memcmp(env0, box, sizeof(box)));

    CHECK(gusto_tighten_env(h, 1, &one, box, &zero, 0, &o));
    CHECK(gusto_get_tighten(h, 0, &n_obs_max));
    REQUIRE(n_obs_max == 1);
    memset(&rep, 0, sizeof(rep));
    rep.status = status; rep.knot = knot; rep.pair = pair; rep.n_grown = n_grown; rep.blocked = blocked;
    rep.min_z_base = min_z; rep.max_margin = max_m; rep.margin = margin;
    CHECK(gusto_get_tighten(h, &rep, 0));
    CHECK(gusto_last_tighten_ms(h, &ms));
    REQUIRE(ms > 0.0);
    CHECK(gusto_get_env(h, &n_env, 0, 0, 0, 0));
    REQUIRE(n_env == B);
    CHECK(gusto_get_env(h, 0, nb, tb, ns, 0));
    for (int b = 0; b < B; b++) {
        REQUIRE(nb[b] == 1 && ns[b] == 0 && status[b] == 1);
        REQUIRE(knot[b] == lc_knot[b] && pair[b] == lc_pair[b]);                      /* the base is the set gusto_lincov saw */
        REQUIRE(fabs(min_z[b] - lc_z[b]) <= 1e-11 * fabs(lc_z[b]));
        REQUIRE(margin[b] > 0.0 && margin[b] == max_m[b] && n_grown[b] == 1);
        /* cover (the arm at (0, 0.15): omax = (0, 0.15), omin = 0), then grow; the third coordinate is copied */
        REQUIRE(tb[b * 6 + 0] == (box[0] - 0.0) - margin[b] && tb[b * 6 + 1] == (box[1] - 0.15) - margin[b]);
        REQUIRE(tb[b * 6 + 3] == (box[3] - 0.0) + margin[b] && tb[b * 6 + 4] == (box[4] - 0.0) + margin[b]);
        REQUIRE(tb[b * 6 + 2] == box[2] && tb[b * 6 + 5] == box[5]);
    }
    /* the re-solve from the own plans reads the tightened tables; the margins outlive it */
    CHECK(gusto_set_problems_replan(h, 0, GUSTO_REPLAN_TRAJ, B, tau, x_init, 0, 0, 0));
    REQUIRE(gusto_get_tighten(h, &rep, 0) == GUSTO_ERR_STATE);                        /* new problems: the report is gone */
    CHECK(gusto_solve(h, 30, 0));
    CHECK(gusto_set_env(h, 1, box, 0, 0));                                            /* back to the base */
    CHECK(gusto_get_env(h, &n_env, nb, env0, ns, 0));
    REQUIRE(n_env == 1 && nb[0] == 1 && !memcmp(env0, box, sizeof(box)));

    printf("ok\n");
    for (int b = 0; b < B; b++)
        printf("%d %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g\n", status[b], knot[b], pair[b], n_grown[b], blocked[b], min_z[b],
               margin[b], tb[b * 6], tb[b * 6 + 1], tb[b * 6 + 3], tb[b * 6 + 4]);
    CHECK(gusto_destroy(h));
    return 0;
}
