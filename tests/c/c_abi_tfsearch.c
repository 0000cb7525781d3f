/* c_abi_tfsearch.c -- plain C through include/gusto_hip.h: the final-time search.
 * Three freeflyerSE2 queries (N = 50) next to one box, four candidate final times each in [4, 84]: the refusals of
 * gusto_tfsearch_begin, its candidates, replicated inputs and line seeds, then begin, solve, update, solve, update, get, with
 * checks of its own on the report after every update; then one line "ok" and, per query, status, round_found, lo, hi, tf_best and
 * J_best, which tests/test_gpu_tfsearch.py compares with the Python path.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_tfsearch.c -o c_abi_tfsearch -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 50, BQ = 3, K = 4, B = BQ * K, NX = 6, NU = 3 };
    gusto_handle h = 0, ht = 0, hd = 0;
    gusto_tfsearch_opts o, bad;
    gusto_tfsearch_report rep;
    const double box[6] = {1.4, 0.9, -0.2, 1.8, 1.5, 0.2};
    const double x_init[BQ * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.4, 1.9, 0, 0, 0, 0, 0.3, 0.4, 0, 0, 0, 0};
    const double goal[BQ * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    const double tf_lo[BQ] = {4.0, 4.0, 4.0}, tf_hi[BQ] = {84.0, 84.0, 84.0}, bad_hi[BQ] = {84.0, 4.0, 84.0};
    static double X[B * N * NX], U[B * N * NU], Xb[BQ * N * NX], Ub[BQ * N * NU];
    int status[BQ], found[BQ], ne[BQ], conv[B], succ[B], round = -1, searching = -1;
    double lo[BQ], hi[BQ], tfb[BQ], Jb[BQ], cand[B], cand0[B], ms = -1.0;
    const double *Xd = 0, *Ud = 0, *Td = 0;

    REQUIRE(gusto_default_tfsearch_opts(GUSTO_FREEFLYER_SE2, 0) == GUSTO_ERR_ARG && gusto_default_tfsearch_opts(9, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_default_tfsearch_opts(GUSTO_FREEFLYER_SE2, &o) == GUSTO_OK);
    REQUIRE(o.rtol == 0.01 && o.seed == GUSTO_TFSEARCH_SEED_INCUMBENT && o.tf_lo > 0 && o.tf_lo < o.tf_hi);
    REQUIRE(gusto_tfsearch_begin(0, BQ, K, x_init, goal, goal, tf_lo, tf_hi, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_tfsearch_update(0, 0) == GUSTO_ERR_ARG);
    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 64, 0));
    CHECK(gusto_set_env(h, 1, box, 0, 0));
    memset(&rep, 0, sizeof(rep));
    REQUIRE(gusto_tfsearch_update(h, 0) == GUSTO_ERR_STATE);                          /* nothing begun yet */
    REQUIRE(gusto_get_tfsearch(h, &rep, 0, 0) == GUSTO_ERR_STATE && gusto_last_tfsearch_ms(h, &ms) == GUSTO_ERR_STATE);
    REQUIRE(gusto_tfsearch_begin(h, BQ, 0, x_init, goal, goal, tf_lo, tf_hi, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_tfsearch_begin(h, BQ, GUSTO_MAX_STARTS + 1, x_init, goal, goal, tf_lo, tf_hi, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_tfsearch_begin(h, BQ + 1, K, x_init, goal, goal, tf_lo, tf_hi, &o) == GUSTO_ERR_ARG);   /* 16 > batch_cap */
    REQUIRE(gusto_tfsearch_begin(h, BQ, K, 0, goal, goal, tf_lo, tf_hi, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_tfsearch_begin(h, BQ, K, x_init, goal, goal, tf_lo, bad_hi, &o) == GUSTO_ERR_ARG && strstr(gusto_last_error(h), "query 1"));
    bad = o; bad.rtol = 1.0;
    REQUIRE(gusto_tfsearch_begin(h, BQ, K, x_init, goal, goal, tf_lo, tf_hi, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.seed = 2;
    REQUIRE(gusto_tfsearch_begin(h, BQ, K, x_init, goal, goal, tf_lo, tf_hi, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.tf_lo = 0.0;
    REQUIRE(gusto_tfsearch_begin(h, BQ, K, x_init, goal, goal, 0, tf_hi, &bad) == GUSTO_ERR_ARG);
    REQUIRE(gusto_get_traj(h, X, U) == GUSTO_ERR_STATE);                            /* the refusals left the handle without problems */

    o.tf_lo = 4.0;                                                                  /* the lower ends from the options */
    CHECK(gusto_tfsearch_begin(h, BQ, K, x_init, goal, goal, 0, tf_hi, &o));
    rep.cand = cand0;
    CHECK(gusto_get_tfsearch(h, &rep, &round, &searching));
    REQUIRE(round == 0 && searching == BQ);
    for (int q = 0; q < BQ; q++)
        for (int j = 0; j < K; j++) REQUIRE(cand0[q * K + j] == 24.0 + 20.0 * j);
    CHECK(gusto_get_traj(h, X, U));
    for (int b = 0; b < B; b++) {
        const double* x = X + (size_t)b * N * NX;
        for (int i = 0; i < NX; i++) REQUIRE(x[i] == x_init[(b / K) * NX + i] && x[(N - 1) * NX + i] == goal[(b / K) * NX + i]);
    }
    for (int i = 0; i < B * N * NU; i++) REQUIRE(U[i] == 0.0);
    REQUIRE(gusto_tfsearch_update(h, 0) == GUSTO_ERR_STATE && strstr(gusto_last_error(h), "gusto_solve"));   /* a solve comes first */

    rep.status = status; rep.round_found = found; rep.n_eligible = ne; rep.lo = lo; rep.hi = hi; rep.tf_best = tfb; rep.J_best = Jb;
    rep.cand = cand; rep.X = Xb; rep.U = Ub;
    for (int r = 0; r < 2 && searching > 0; r++) {
        gusto_tfsearch_report rc;
        memset(&rc, 0, sizeof(rc));
        rc.cand = cand0;                                                            /* the candidates of this round */
        CHECK(gusto_get_tfsearch(h, &rc, 0, 0));
        CHECK(gusto_solve(h, 30, 0));
        CHECK(gusto_get_traj(h, X, U));
        CHECK(gusto_get_status(h, 0, conv, succ, 0, 0));
        CHECK(gusto_tfsearch_update(h, 0));
        CHECK(gusto_get_tfsearch(h, &rep, &round, &searching));
        CHECK(gusto_last_tfsearch_ms(h, &ms));
        REQUIRE(round == r + 1 && ms > 0.0);
        for (int q = 0; q < BQ; q++) {
            const int done = (status[q] & (GUSTO_TFSEARCH_NONE | GUSTO_TFSEARCH_DONE)) != 0;
            if (found[q] == r) {                                                    /* the incumbent is a solve of this round */
                int w = -1;
                for (int j = K - 1; j >= 0; j--)
                    if (conv[q * K + j] && succ[q * K + j] && cand0[q * K + j] == tfb[q]) w = j;
                REQUIRE(w >= 0);
                for (int j = 0; j < K; j++) REQUIRE(!(conv[q * K + j] && succ[q * K + j]) || cand0[q * K + j] >= tfb[q]);
                REQUIRE(!memcmp(Xb + (size_t)q * N * NX, X + (size_t)(q * K + w) * N * NX, sizeof(double) * N * NX));
                REQUIRE(!memcmp(Ub + (size_t)q * N * NU, U + (size_t)(q * K + w) * N * NU, sizeof(double) * N * NU));
                REQUIRE(Jb[q] == Jb[q]);
            }
            if (found[q] >= 0) REQUIRE(hi[q] == tfb[q] && lo[q] < hi[q] && !(status[q] & GUSTO_TFSEARCH_NONE));
            else REQUIRE((status[q] & GUSTO_TFSEARCH_NONE) && tfb[q] != tfb[q] && lo[q] == 84.0 && hi[q] == 84.0);
            REQUIRE(((status[q] & GUSTO_TFSEARCH_FLOOR) != 0) == (lo[q] == 4.0));
            REQUIRE(((status[q] & GUSTO_TFSEARCH_DONE) != 0) == (hi[q] - lo[q] <= o.rtol * hi[q]));
            for (int j = 0; j < K; j++) REQUIRE(done ? cand[q * K + j] == hi[q] : (cand[q * K + j] > lo[q] && cand[q * K + j] < hi[q]));
        }
    }
    CHECK(gusto_get_tfsearch_dev(h, &Xd, &Ud, &Td));
    REQUIRE(Xd && Ud && Td);
    CHECK(gusto_set_problems(h, BQ, x_init, goal, goal, tf_hi, 0, 0));                /* new problems: the search is gone */
    REQUIRE(gusto_get_tfsearch(h, 0, 0, 0) == GUSTO_ERR_STATE && gusto_tfsearch_update(h, 0) == GUSTO_ERR_STATE);
    REQUIRE(gusto_get_tfsearch_dev(h, 0, 0, 0) == GUSTO_ERR_STATE);

    CHECK(gusto_create_trajopt(&ht, GUSTO_FREEFLYER_SE2, N, B, 272, 0));
    REQUIRE(gusto_tfsearch_begin(ht, BQ, K, x_init, goal, goal, tf_lo, tf_hi, &o) == GUSTO_ERR_ARG && strstr(gusto_last_error(ht), "TrajOpt"));
    gusto_destroy(ht);
    CHECK(gusto_create(&hd, GUSTO_DUBINS_CAR, N, B, 64, 0));
    REQUIRE(gusto_tfsearch_begin(hd, BQ, K, x_init, goal, goal, tf_lo, tf_hi, &o) == GUSTO_ERR_ARG && strstr(gusto_last_error(hd), "DubinsCar"));
    gusto_destroy(hd);

    printf("ok\n");
    for (int q = 0; q < BQ; q++) printf("%d %d %.17g %.17g %.17g %.17g\n", status[q], found[q], lo[q], hi[q], tfb[q], Jb[q]);
    CHECK(gusto_destroy(h));
    return 0;
}
