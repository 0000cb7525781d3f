/* c_abi_roadmap.c -- plain C through include/gusto_hip.h: the roadmap entry points.
 * Three freeflyerSE2 queries (N = 50) next to one box, two alternates each: the defaults, the refusals of
 * gusto_set_problems_roadmap, the seeds' replicated inputs and end knots, the report's invariants, the state errors of the getters
 * and a solve from the seeds, with checks of its own; then one line "ok" and, per problem, status, n_via, via[0], banned[0] and
 * length, which tests/test_gpu_roadmap.py compares with the numpy restatement.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_roadmap.c -o c_abi_roadmap -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 50, BQ = 3, K = 2, B = BQ * K, NX = 6, NU = 3, V = GUSTO_ROADMAP_MAX_VIA, NB = GUSTO_ROADMAP_MAX_K };
    gusto_handle h = 0, ht = 0;
    gusto_roadmap_opts o, bad;
    gusto_roadmap_report rep;
    gusto_scp_params sp;
    gusto_model_params mp;
    const double box[6] = {1.4, 0.9, -0.2, 1.8, 1.5, 0.2};
    const double x_init[BQ * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.4, 1.3, 0, 0, 0, 0, 0.3, 0.4, 0, 0, 0, 0};
    const double goal[BQ * NX] = {3.0, 1.1, 0, 0.05, -0.05, 0, 3.0, 1.1, 0, 0.05, -0.05, 0, 3.0, 1.1, 0, 0.05, -0.05, 0};
    const double tf[BQ] = {200.0, 150.0, 100.0};
    static double X[B * N * NX], U[B * N * NU];
    int status[B], n_via[B], via[B * V], banned[B * NB], conv[B], succ[B], n_path = 0;
    double length[B], stage[3], ms = 0.0;

    REQUIRE(gusto_default_roadmap_opts(GUSTO_FREEFLYER_SE2, 0) == GUSTO_ERR_ARG);
    REQUIRE(gusto_default_roadmap_opts(17, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_default_roadmap_opts(GUSTO_FREEFLYER_SE2, &o) == GUSTO_OK);
    REQUIRE(gusto_default_params(GUSTO_FREEFLYER_SE2, &sp, &mp) == GUSTO_OK);
    REQUIRE(o.inflate == mp.radius + 0.02 && o.pad == 0.03 && o.straight_first == 0);
    o.inflate = 0.177;

    REQUIRE(gusto_set_problems_roadmap(0, BQ, K, x_init, goal, goal, tf, &o) == GUSTO_ERR_ARG);
    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 64, 0));
    CHECK(gusto_set_env(h, 1, box, 0, 0));
    memset(&rep, 0, sizeof(rep));
    REQUIRE(gusto_get_roadmap(h, &rep) == GUSTO_ERR_STATE);                         /* nothing set yet */
    REQUIRE(gusto_last_roadmap_ms(h, &ms) == GUSTO_ERR_STATE);
    REQUIRE(gusto_set_problems_roadmap(h, BQ, 0, x_init, goal, goal, tf, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_roadmap(h, 1, GUSTO_ROADMAP_MAX_K + 1, x_init, goal, goal, tf, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_roadmap(h, BQ + 1, K, x_init, goal, goal, tf, &o) == GUSTO_ERR_ARG);   /* 8 > batch_cap */
    REQUIRE(gusto_set_problems_roadmap(h, BQ, K, x_init, goal, goal, 0, &o) == GUSTO_ERR_ARG);
    bad = o; bad.inflate = NAN;
    REQUIRE(gusto_set_problems_roadmap(h, BQ, K, x_init, goal, goal, tf, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.pad = 0.0;
    REQUIRE(gusto_set_problems_roadmap(h, BQ, K, x_init, goal, goal, tf, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.straight_first = 2;
    REQUIRE(gusto_set_problems_roadmap(h, BQ, K, x_init, goal, goal, tf, &bad) == GUSTO_ERR_ARG);
    REQUIRE(gusto_get_traj(h, X, U) == GUSTO_ERR_STATE);                            /* the refusals left the handle without problems */

    CHECK(gusto_set_problems_roadmap(h, BQ, K, x_init, goal, goal, tf, &o));
    CHECK(gusto_get_traj(h, X, U));
    for (int b = 0; b < B; b++) {
        const double* x = X + (size_t)b * N * NX;
        for (int i = 0; i < NX; i++) REQUIRE(x[i] == x_init[(b / K) * NX + i] && x[(N - 1) * NX + i] == goal[(b / K) * NX + i]);
    }
    for (int i = 0; i < B * N * NU; i++) REQUIRE(U[i] == 0.0);
    CHECK(gusto_get_roadmap(h, 0));
    rep.status = status; rep.n_via = n_via; rep.via = via; rep.length = length; rep.banned = banned; rep.stage_ms = stage;
    CHECK(gusto_get_roadmap(h, &rep));
    CHECK(gusto_last_roadmap_ms(h, &ms));
    REQUIRE(ms > 0.0 && stage[0] >= 0.0 && stage[1] > 0.0 && stage[2] > 0.0);
    for (int b = 0; b < B; b++) {
        REQUIRE(status[b] >= GUSTO_ROADMAP_DIRECT && status[b] <= GUSTO_ROADMAP_TOO_LONG);
        REQUIRE(n_via[b] >= 0 && n_via[b] <= V && (status[b] == GUSTO_ROADMAP_PATH) == (n_via[b] > 0));
        for (int i = 0; i < V; i++) REQUIRE(i < n_via[b] ? (via[b * V + i] >= 2 && via[b * V + i] < 2 + 4) : via[b * V + i] == -1);
        REQUIRE((status[b] == GUSTO_ROADMAP_PATH || status[b] == GUSTO_ROADMAP_DIRECT) == (length[b] < INFINITY));
        REQUIRE(b % K == 0 ? banned[b * NB] == -1 : 1);                             /* alternate 0 has no ban */
        n_path += status[b] == GUSTO_ROADMAP_PATH;
    }
    REQUIRE(n_path >= 1);
    CHECK(gusto_solve(h, 30, 0));
    CHECK(gusto_get_status(h, 0, conv, succ, 0, 0));
    CHECK(gusto_get_roadmap(h, &rep));                                              /* a solve leaves the report */
    CHECK(gusto_set_problems(h, BQ, x_init, goal, goal, tf, 0, 0));                 /* new problems: the report is gone */
    REQUIRE(gusto_get_roadmap(h, &rep) == GUSTO_ERR_STATE);
    REQUIRE(gusto_last_roadmap_ms(h, &ms) == GUSTO_ERR_STATE);
    CHECK(gusto_set_problems_roadmap(h, BQ, K, x_init, goal, goal, tf, 0));         /* NULL: the defaults */

    CHECK(gusto_create_trajopt(&ht, GUSTO_FREEFLYER_SE2, N, B, 272, 0));
    REQUIRE(gusto_set_problems_roadmap(ht, BQ, K, x_init, goal, goal, tf, &o) == GUSTO_ERR_ARG && strstr(gusto_last_error(ht), "TrajOpt"));
    gusto_destroy(ht);

    printf("ok\n");
    for (int b = 0; b < B; b++) printf("%d %d %d %d %.17g\n", status[b], n_via[b], via[b * V], banned[b * NB], length[b]);
    CHECK(gusto_destroy(h));
    return 0;
}
