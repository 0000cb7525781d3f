/* c_abi_trajlib.c -- plain C through include/gusto_hip.h: the trajectory library.
 * Four freeflyerSE2 problems (N = 50) next to one box are solved from the straight line and become the library
 * (gusto_trajlib_add); three queries are seeded from their two nearest entries
 * (gusto_set_problems_trajlib), solved, and answered by gusto_select_best.  On the way: the refusals, the empty library (straight
 * lines), gusto_trajlib_get into gusto_trajlib_add_host of a second library (the same seeds), the state errors of the getter, with
 * checks of its own; then one line "ok", one line with the library's fill and, per query, entry 0, entry 1, n_found, dist2 of
 * entry 0 and the winner, which tests/test_gpu_trajlib.py compares with the Python path.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_trajlib.c -o c_abi_trajlib -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s | %s\n", #call, rc_, gusto_last_error(h), gusto_trajlib_last_error(lib)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 50, BL = 4, BQ = 3, K = 2, B = BQ * K, NX = 6, NU = 3, CAP = 6 };
    gusto_handle h = 0, ht = 0;
    gusto_trajlib lib = 0, lib2 = 0, libn = 0;
    gusto_trajlib_opts o;
    gusto_best_report rep;
    const double box[6] = {1.4, 0.9, -0.2, 1.8, 1.5, 0.2};
    const double lx[BL * NX] = {0.25, 2.3, 0, 0, 0, 0, 0.5, 1.8, 0, 0, 0, 0, 0.3, 0.5, 0, 0, 0, 0, 1.0, 0.3, 0, 0, 0, 0};
    const double lgoal[BL * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0,
                                   3.0, 0.5, 0, 0.05, -0.05, 0};
    const double ltf[BL] = {200.0, 150.0, 100.0, 100.0};
    const double x_init[BQ * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.4, 1.9, 0, 0, 0, 0, 0.3, 0.4, 0, 0, 0, 0};
    const double goal[BQ * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    const double tf[BQ] = {200.0, 150.0, 100.0};
    static double X[B * N * NX], U[B * N * NU], Xs[B * N * NX], Us[B * N * NU];
    static double gx[CAP * NX], gc[CAP * NX], gtf[CAP], gX[CAP * N * NX], gU[CAP * N * NU];
    int gtag[CAP], conv[BL], succ[BL], entry[B], entry2[B], nf[BQ], winner[BQ], count = -1, cap = -1, added = -1;
    const int all[BL] = {1, 1, 1, 1};
    double d2[B], d2b[B], ms = -1.0;

    REQUIRE(gusto_default_trajlib_opts(9, &o) == GUSTO_ERR_ARG);
    CHECK(gusto_default_trajlib_opts(GUSTO_FREEFLYER_SE2, &o));
    REQUIRE(o.w_init[0] == 1.0 && o.w_goal[5] == 1.0 && o.w_init[6] == 0.0 && o.w_tf == 0.0 && o.lds_tile == 1);
    REQUIRE(gusto_trajlib_create(&libn, GUSTO_FREEFLYER_SE2, N, 0, 0, 0) == GUSTO_ERR_ARG && strstr(gusto_trajlib_last_error(0), "cap"));
    REQUIRE(gusto_trajlib_create(&libn, GUSTO_FREEFLYER_SE2, N, GUSTO_TRAJLIB_MAX_CAP + 1, 0, 0) == GUSTO_ERR_ARG);
    o.w_goal[1] = -1.0;
    REQUIRE(gusto_trajlib_create(&libn, GUSTO_FREEFLYER_SE2, N, CAP, 0, &o) == GUSTO_ERR_ARG);
    o.w_goal[1] = 1.0;
    CHECK(gusto_trajlib_create(&lib, GUSTO_FREEFLYER_SE2, N, CAP, 0, &o));
    CHECK(gusto_trajlib_create(&libn, GUSTO_FREEFLYER_SE2, N - 1, CAP, 0, 0));     /* another horizon */
    CHECK(gusto_trajlib_size(lib, &count, &cap));
    REQUIRE(count == 0 && cap == CAP);

    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 64, 0));
    CHECK(gusto_set_env(h, 1, box, 0, 0));
    REQUIRE(gusto_trajlib_add(lib, h, 0, 0, &added) == GUSTO_ERR_STATE && added == 0);        /* no problems yet */
    REQUIRE(gusto_get_trajlib_seeds(h, entry, d2, nf) == GUSTO_ERR_STATE);
    /* the refusals of gusto_set_problems_trajlib leave the handle without problems */
    REQUIRE(gusto_set_problems_trajlib(0, lib, BQ, K, x_init, goal, goal, tf, 0) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_trajlib(h, 0, BQ, K, x_init, goal, goal, tf, 0) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_trajlib(h, libn, BQ, K, x_init, goal, goal, tf, 0) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_trajlib(h, lib, BQ, 0, x_init, goal, goal, tf, 0) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_trajlib(h, lib, 1, GUSTO_TRAJLIB_MAX_K + 1, x_init, goal, goal, tf, 0) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_trajlib(h, lib, BQ + 1, K, x_init, goal, goal, tf, 0) == GUSTO_ERR_ARG);   /* 8 > batch_cap */
    REQUIRE(gusto_set_problems_trajlib(h, lib, BQ, K, x_init, goal, 0, tf, 0) == GUSTO_ERR_ARG);
    REQUIRE(gusto_get_traj(h, X, U) == GUSTO_ERR_STATE);

    /* an empty library: K straight lines per query, what gusto_set_problems writes for the replicated inputs */
    CHECK(gusto_set_problems_trajlib(h, lib, BQ, K, x_init, goal, goal, tf, 0));
    CHECK(gusto_get_trajlib_seeds(h, entry, d2, nf));
    CHECK(gusto_get_traj(h, X, U));
    for (int b = 0; b < B; b++) REQUIRE(entry[b] == -1 && d2[b] == INFINITY && nf[b / K] == 0);
    {
        static double rx[B * NX], rg[B * NX], rt[B];
        for (int b = 0; b < B; b++) {
            memcpy(rx + b * NX, x_init + (b / K) * NX, sizeof(double) * NX);
            memcpy(rg + b * NX, goal + (b / K) * NX, sizeof(double) * NX);
            rt[b] = tf[b / K];
        }
        CHECK(gusto_set_problems(h, B, rx, rg, rg, rt, 0, 0));
        CHECK(gusto_get_traj(h, Xs, Us));
        REQUIRE(!memcmp(X, Xs, sizeof(X)) && !memcmp(U, Us, sizeof(U)));
        REQUIRE(gusto_get_trajlib_seeds(h, entry, d2, nf) == GUSTO_ERR_STATE);      /* problems set by another call */
    }

    /* the library: four problems solved from the straight line */
    CHECK(gusto_set_problems(h, BL, lx, lgoal, lgoal, ltf, 0, 0));
    REQUIRE(gusto_trajlib_add(libn, h, 0, 0, &added) == GUSTO_ERR_ARG && added == 0);        /* another horizon */
    CHECK(gusto_trajlib_add(lib, h, 0, 0, &added));                                           /* nothing converged yet */
    REQUIRE(added == 0);
    CHECK(gusto_solve(h, 30, 0));
    CHECK(gusto_get_status(h, 0, conv, succ, 0, 0));
    CHECK(gusto_trajlib_add(lib, h, 0, 0, &added));                                           /* the default mask */
    CHECK(gusto_trajlib_size(lib, &count, 0));
    REQUIRE(count == added && added == (conv[0] && succ[0]) + (conv[1] && succ[1]) + (conv[2] && succ[2]) + (conv[3] && succ[3]));
    CHECK(gusto_trajlib_clear(lib));
    CHECK(gusto_trajlib_add(lib, h, all, 0, &added));                                         /* all four, whatever their status */
    CHECK(gusto_trajlib_size(lib, &count, 0));
    REQUIRE(count == BL && added == BL);
    REQUIRE(gusto_trajlib_add(lib, h, all, 0, &added) == GUSTO_ERR_ARG && added == 0);        /* 4 more do not fit */
    CHECK(gusto_trajlib_size(lib, &cap, 0));
    REQUIRE(cap == count);
    CHECK(gusto_trajlib_get(lib, gx, gc, gtf, gtag, gX, gU));
    for (int e = 0; e < count; e++) {
        REQUIRE(gtag[e] == 0 && gc[e * NX] == 3.0 && gc[e * NX + 3] == 0.05 && gtf[e] == ltf[e]);
        for (int i = 0; i < NX; i++) REQUIRE(gx[e * NX + i] == lx[e * NX + i]);
    }

    /* the seeded queries */
    CHECK(gusto_set_problems_trajlib(h, lib, BQ, K, x_init, goal, goal, tf, 0));
    CHECK(gusto_last_trajlib_ms(h, &ms));
    REQUIRE(ms >= 0.0);
    CHECK(gusto_get_trajlib_seeds(h, entry, d2, nf));
    CHECK(gusto_get_traj(h, X, U));
    for (int q = 0; q < BQ; q++) {
        REQUIRE(nf[q] == K && entry[q * K] >= 0 && entry[q * K] < count && entry[q * K + 1] >= 0 && entry[q * K] != entry[q * K + 1]);
        REQUIRE(d2[q * K] <= d2[q * K + 1]);
        for (int j = 0; j < K; j++) {
            const int b = q * K + j, e = entry[b];
            double want = 0.0;
            for (int i = 0; i < NX; i++) {
                const double t = x_init[q * NX + i] - gx[e * NX + i], u = goal[q * NX + i] - gc[e * NX + i];
                want += t * t + u * u;
                REQUIRE(X[(size_t)b * N * NX + i] == x_init[q * NX + i]);                      /* knot 0 is x_init itself */
            }
            REQUIRE(fabs(d2[b] - want) <= 2e-14 * want);
            REQUIRE(!memcmp(U + (size_t)b * N * NU, gU + (size_t)e * N * NU, sizeof(double) * N * NU));
        }
    }
    /* the same library through the host arrays: the same seeds */
    CHECK(gusto_trajlib_create(&lib2, GUSTO_FREEFLYER_SE2, N, CAP, 0, 0));
    gX[7] = NAN;
    REQUIRE(gusto_trajlib_add_host(lib2, count, gx, gc, gc, gtf, gtag, gX, gU) == GUSTO_ERR_ARG);
    CHECK(gusto_trajlib_get(lib, 0, 0, 0, 0, gX, 0));
    REQUIRE(gusto_trajlib_add_host(lib2, CAP + 1, gx, gc, gc, gtf, gtag, gX, gU) == GUSTO_ERR_ARG);
    CHECK(gusto_trajlib_add_host(lib2, count, gx, gc, gc, gtf, gtag, gX, gU));
    CHECK(gusto_set_problems_trajlib(h, lib2, BQ, K, x_init, goal, goal, tf, gtag));
    CHECK(gusto_get_trajlib_seeds(h, entry2, d2b, 0));
    CHECK(gusto_get_traj(h, Xs, Us));
    REQUIRE(!memcmp(entry, entry2, sizeof(entry)) && !memcmp(d2, d2b, sizeof(d2)) && !memcmp(X, Xs, sizeof(X)) && !memcmp(U, Us, sizeof(U)));
    CHECK(gusto_trajlib_clear(lib2));
    CHECK(gusto_trajlib_size(lib2, &cap, 0));
    REQUIRE(cap == 0);

    CHECK(gusto_solve(h, 30, 0));
    CHECK(gusto_select_best(h, K, 0, 0));
    memset(&rep, 0, sizeof(rep));
    rep.winner = winner;
    CHECK(gusto_get_best(h, &rep));

    CHECK(gusto_create_trajopt(&ht, GUSTO_FREEFLYER_SE2, N, B, 272, 0));
    REQUIRE(gusto_set_problems_trajlib(ht, lib, BQ, K, x_init, goal, goal, tf, 0) == GUSTO_ERR_ARG && strstr(gusto_last_error(ht), "TrajOpt"));
    CHECK(gusto_set_problems(ht, BQ, x_init, goal, goal, tf, 0, 0));
    REQUIRE(gusto_trajlib_add(lib, ht, 0, 0, 0) == GUSTO_ERR_ARG && strstr(gusto_trajlib_last_error(lib), "TrajOpt"));
    gusto_destroy(ht);

    printf("ok\n%d\n", count);
    for (int q = 0; q < BQ; q++) printf("%d %d %d %.17g %d\n", entry[q * K], entry[q * K + 1], nf[q], d2[q * K], winner[q]);
    CHECK(gusto_trajlib_destroy(lib2));
    CHECK(gusto_trajlib_destroy(libn));
    CHECK(gusto_trajlib_destroy(lib));
    REQUIRE(gusto_trajlib_destroy(0) == GUSTO_ERR_ARG);
    CHECK(gusto_destroy(h));
    return 0;
}
