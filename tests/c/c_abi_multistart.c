/* c_abi_multistart.c -- plain C through include/gusto_hip.h: the multi-start entry points.
 * Three freeflyerSE2 queries (N = 50) next to one box, a fan of three starts each (0, +0.5 m, -0.5 m): the refusals of
 * gusto_set_problems_multistart, the fan's replicated inputs and end knots, gusto_solve, gusto_select_best with the default score
 * and eligibility and with the caller's, gusto_get_best against gusto_get_traj, the state errors of the getters, with checks of
 * its own; then one line "ok" and, per query, winner, winner_problem, n_eligible and best_score, which
 * tests/test_gpu_multistart.py compares with the Python path.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_multistart.c -o c_abi_multistart -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 50, BQ = 3, K = 3, B = BQ * K, NX = 6, NU = 3 };
    gusto_handle h = 0, ht = 0;
    gusto_best_report rep;
    const double box[6] = {1.4, 0.9, -0.2, 1.8, 1.5, 0.2};
    const double x_init[BQ * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.4, 1.9, 0, 0, 0, 0, 0.3, 0.4, 0, 0, 0, 0};
    const double goal[BQ * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    const double tf[BQ] = {200.0, 150.0, 100.0};
    const double fan[K * 2] = {0.0, 0.0, 0.5, 0.0, -0.5, 0.0};
    double bad_fan[K * 2];
    static double fan65[65 * 2];
    static double X[B * N * NX], U[B * N * NU], Xb[BQ * N * NX], Ub[BQ * N * NU];
    int winner[BQ], wp[BQ], ne[BQ], w2[BQ], conv[B], succ[B], elig[B];
    double best[BQ], score[B];

    REQUIRE(gusto_set_problems_multistart(0, BQ, K, x_init, goal, goal, tf, fan) == GUSTO_ERR_ARG);
    REQUIRE(gusto_select_best(0, K, 0, 0) == GUSTO_ERR_ARG);
    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 64, 0));
    CHECK(gusto_set_env(h, 1, box, 0, 0));
    memset(&rep, 0, sizeof(rep));
    REQUIRE(gusto_select_best(h, K, 0, 0) == GUSTO_ERR_STATE);                      /* nothing set yet */
    REQUIRE(gusto_get_best(h, &rep) == GUSTO_ERR_STATE);
    REQUIRE(gusto_set_problems_multistart(h, BQ, 0, x_init, goal, goal, tf, fan) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_multistart(h, 1, 65, x_init, goal, goal, tf, fan65) == GUSTO_ERR_ARG);
    REQUIRE(gusto_set_problems_multistart(h, BQ + 1, K, x_init, goal, goal, tf, fan) == GUSTO_ERR_ARG);   /* 12 > batch_cap */
    REQUIRE(gusto_set_problems_multistart(h, BQ, K, x_init, goal, goal, tf, 0) == GUSTO_ERR_ARG);
    memcpy(bad_fan, fan, sizeof(fan));
    bad_fan[3] = NAN;
    REQUIRE(gusto_set_problems_multistart(h, BQ, K, x_init, goal, goal, tf, bad_fan) == GUSTO_ERR_ARG);
    REQUIRE(gusto_get_traj(h, X, U) == GUSTO_ERR_STATE);                            /* the refusals left the handle without problems */

    CHECK(gusto_set_problems_multistart(h, BQ, K, x_init, goal, goal, tf, fan));
    CHECK(gusto_get_traj(h, X, U));
    for (int b = 0; b < B; b++) {
        const double* x = X + (size_t)b * N * NX;
        for (int i = 0; i < NX; i++) REQUIRE(x[i] == x_init[(b / K) * NX + i] && x[(N - 1) * NX + i] == goal[(b / K) * NX + i]);
    }
    for (int i = 0; i < B * N * NU; i++) REQUIRE(U[i] == 0.0);
    REQUIRE(gusto_get_best(h, &rep) == GUSTO_ERR_STATE);                            /* no selection yet */
    REQUIRE(gusto_select_best(h, 2, 0, 0) == GUSTO_ERR_ARG);                        /* 2 does not divide 9 */
    CHECK(gusto_solve(h, 30, 0));
    CHECK(gusto_get_traj(h, X, U));
    CHECK(gusto_get_status(h, 0, conv, succ, 0, 0));

    CHECK(gusto_select_best(h, K, 0, 0));
    rep.winner = winner; rep.winner_problem = wp; rep.n_eligible = ne; rep.best_score = best; rep.X = Xb; rep.U = Ub;
    CHECK(gusto_get_best(h, &rep));
    for (int q = 0; q < BQ; q++) {
        int cnt = 0;
        for (int j = 0; j < K; j++) cnt += conv[q * K + j] && succ[q * K + j];
        REQUIRE(ne[q] == cnt && (cnt == 0) == (winner[q] < 0));
        if (winner[q] < 0) {
            REQUIRE(wp[q] == -1 && best[q] == INFINITY);
            for (int i = 0; i < N * NX; i++) REQUIRE(Xb[(size_t)q * N * NX + i] == 0.0);
        } else {
            REQUIRE(wp[q] == q * K + winner[q] && conv[wp[q]] && succ[wp[q]]);
            REQUIRE(!memcmp(Xb + (size_t)q * N * NX, X + (size_t)wp[q] * N * NX, sizeof(double) * N * NX));
            REQUIRE(!memcmp(Ub + (size_t)q * N * NU, U + (size_t)wp[q] * N * NU, sizeof(double) * N * NU));
        }
    }
    /* the caller's score and eligibility: the last start of every query, whatever its cost */
    for (int b = 0; b < B; b++) { score[b] = (double)(B - b); elig[b] = 1; }
    elig[2 * K + 2] = 0;
    memset(&rep, 0, sizeof(rep));
    rep.winner = w2;
    CHECK(gusto_select_best(h, K, score, elig));
    CHECK(gusto_get_best(h, &rep));
    REQUIRE(w2[0] == 2 && w2[1] == 2 && w2[2] == 1);
    CHECK(gusto_set_problems(h, BQ, x_init, goal, goal, tf, 0, 0));                 /* new problems: the selection is gone */
    REQUIRE(gusto_get_best(h, &rep) == GUSTO_ERR_STATE);
    REQUIRE(gusto_get_best_dev(h, 0, 0, 0) == GUSTO_ERR_STATE);

    CHECK(gusto_create_trajopt(&ht, GUSTO_FREEFLYER_SE2, N, B, 272, 0));
    REQUIRE(gusto_set_problems_multistart(ht, BQ, K, x_init, goal, goal, tf, fan) == GUSTO_ERR_ARG && strstr(gusto_last_error(ht), "TrajOpt"));
    REQUIRE(gusto_select_best(ht, K, 0, 0) == GUSTO_ERR_ARG);
    gusto_destroy(ht);

    printf("ok\n");
    for (int q = 0; q < BQ; q++) printf("%d %d %d %.17g\n", winner[q], wp[q], ne[q], best[q]);
    CHECK(gusto_destroy(h));
    return 0;
}
