/* c_abi_legs.c -- plain C through include/gusto_hip.h: the goal timeline.
 * Two freeflyerSE2 queries (N = 20) next to one box, each with a position-only waypoint before its goal: two refusals of
 * gusto_legs_begin, its mode, replicated inputs and line seeds, then begin, solve, advance, solve, advance, get, with checks of
 * its own on the report and the joined buffers after every advance; then one line "ok" and, per query, status, failed_leg,
 * n_done, J_total, gap of leg 1, arrive of both legs and the times of knots 19 and 20, which tests/test_gpu_legs.py compares
 * with the Python path.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_legs.c -o c_abi_legs -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 20, BQ = 2, L = 2, NX = 6, NU = 3, NJ = L * (N - 1) + 1 };
    gusto_handle h = 0;
    gusto_legs_opts o, bad;
    gusto_legs_report rep;
    const double box[6] = {1.4, 0.9, -0.2, 1.8, 1.5, 0.2};
    const double x_init[BQ * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.4, 1.9, 0, 0, 0, 0};
    const double t_goal[BQ * L] = {40.0, 90.0, 50.0, 90.0}, bad_t[BQ * L] = {40.0, 90.0, 50.0, 50.0};
    double lo[BQ * L * NX] = {1.0, 2.2, 0, 0, 0, 0, 3.0, 0.5, 0, 0.05, -0.05, 0, 1.2, 0.6, 0, 0, 0, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    double hi[BQ * L * NX];
    static double X[BQ * N * NX], U[BQ * N * NU], X1[BQ * N * NX], U1[BQ * N * NU], Xj[BQ * NJ * NX], Uj[BQ * NJ * NU], tj[BQ * NJ];
    int status[BQ], failed[BQ], ndone[BQ], its[BQ * L], conv[BQ * L], succ[BQ * L], stop[BQ * L], round = -1, flying = -1;
    double Jt[BQ], J[BQ * L], gap[BQ * L], arrive[BQ * L], ms = -1.0;
    const double *Xd = 0, *Ud = 0, *Td = 0;

    memcpy(hi, lo, sizeof(lo));
    for (int q = 0; q < BQ; q++)                       /* the waypoints: positions only */
        for (int i = 2; i < NX; i++) { lo[(q * L) * NX + i] = -INFINITY; hi[(q * L) * NX + i] = INFINITY; }
    REQUIRE(gusto_default_legs_opts(GUSTO_FREEFLYER_SE2, 0) == GUSTO_ERR_ARG && gusto_default_legs_opts(9, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_default_legs_opts(GUSTO_FREEFLYER_SE2, &o) == GUSTO_OK && o.mode == GUSTO_LEGS_AUTO);
    REQUIRE(gusto_legs_begin(0, BQ, L, 0, x_init, lo, hi, t_goal, &o) == GUSTO_ERR_ARG && gusto_legs_advance(0, 0) == GUSTO_ERR_ARG);
    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, BQ * L, 64, 0));
    CHECK(gusto_set_env(h, 1, box, 0, 0));
    memset(&rep, 0, sizeof(rep));
    REQUIRE(gusto_legs_advance(h, 0) == GUSTO_ERR_STATE && gusto_get_legs(h, &rep, 0, 0) == GUSTO_ERR_STATE);   /* nothing begun yet */
    REQUIRE(gusto_legs_begin(h, BQ, L, 0, x_init, lo, hi, bad_t, &o) == GUSTO_ERR_ARG && strstr(gusto_last_error(h), "query 1"));
    bad = o; bad.mode = GUSTO_LEGS_PARALLEL;           /* a position-only waypoint leaves the junction partly free */
    REQUIRE(gusto_legs_begin(h, BQ, L, 0, x_init, lo, hi, t_goal, &bad) == GUSTO_ERR_ARG && strstr(gusto_last_error(h), "PARALLEL"));
    REQUIRE(gusto_get_traj(h, X, U) == GUSTO_ERR_STATE);                             /* the refusals left the handle without problems */

    CHECK(gusto_legs_begin(h, BQ, L, 0, x_init, lo, hi, t_goal, 0));                  /* the defaults: AUTO, here SEQUENTIAL */
    CHECK(gusto_get_legs(h, 0, &round, &flying));
    REQUIRE(round == 0 && flying == BQ);
    CHECK(gusto_get_traj(h, X, U));                                                   /* B = BQ problems: the first legs */
    for (int q = 0; q < BQ; q++)
        for (int i = 0; i < NX; i++) {
            const double c = i < 2 ? lo[(q * L) * NX + i] : 0.0;                     /* the centre of an unbounded entry is 0 */
            REQUIRE(X[(q * N) * NX + i] == x_init[q * NX + i] && X[(q * N + N - 1) * NX + i] == c);
        }
    for (int i = 0; i < BQ * N * NU; i++) REQUIRE(U[i] == 0.0);
    REQUIRE(gusto_legs_advance(h, 0) == GUSTO_ERR_STATE && strstr(gusto_last_error(h), "gusto_solve"));   /* a solve comes first */

    rep.status = status; rep.failed_leg = failed; rep.n_done = ndone; rep.J_total = Jt; rep.iterations = its; rep.converged = conv;
    rep.successful = succ; rep.stop_reason = stop; rep.J = J; rep.gap = gap; rep.arrive = arrive; rep.X = Xj; rep.U = Uj; rep.t = tj;
    for (int r = 0; r < L && flying > 0; r++) {
        int c[BQ], s[BQ];
        CHECK(gusto_solve(h, 30, 0));
        CHECK(gusto_get_traj(h, X, U));
        CHECK(gusto_get_status(h, 0, c, s, 0, 0));
        CHECK(gusto_legs_advance(h, 0));
        CHECK(gusto_get_legs(h, &rep, &round, &flying));
        CHECK(gusto_last_legs_ms(h, &ms));
        CHECK(gusto_get_traj(h, X1, U1));
        REQUIRE(round == r + 1 && ms > 0.0);
        for (int q = 0; q < BQ; q++) {
            const double* x = X + (size_t)q * N * NX;
            const double* xj = Xj + ((size_t)q * NJ + (size_t)r * (N - 1)) * NX;
            if (ndone[q] + (failed[q] >= 0) <= r) continue;                           /* finished before this round */
            REQUIRE(conv[q * L + r] == c[q] && succ[q * L + r] == s[q]);
            REQUIRE(!memcmp(xj + NX, x + NX, sizeof(double) * (N - 1) * NX));         /* leg r: knots 1 .. N - 1 */
            REQUIRE(!memcmp(Uj + ((size_t)q * NJ + (size_t)r * (N - 1)) * NU, U + (size_t)q * N * NU, sizeof(double) * N * NU));
            REQUIRE(tj[q * NJ + (r + 1) * (N - 1)] == t_goal[q * L + r]);
            if (c[q] && s[q] && r + 1 < L) {                                          /* the next leg starts where this one arrived */
                REQUIRE(status[q] == GUSTO_LEGS_FLYING && ndone[q] == r + 1);
                REQUIRE(!memcmp(X1 + (size_t)q * N * NX, x + (size_t)(N - 1) * NX, sizeof(double) * NX));
            } else {
                REQUIRE(status[q] == (c[q] && s[q] ? GUSTO_LEGS_DONE : GUSTO_LEGS_FAILED) && failed[q] == (c[q] && s[q] ? -1 : r));
            }
        }
    }
    REQUIRE(flying == 0);
    for (int q = 0; q < BQ; q++) REQUIRE(status[q] == GUSTO_LEGS_DONE && gap[q * L] == 0.0 && gap[q * L + 1] < 1e-6 && arrive[q * L + 1] < 1e-6);
    CHECK(gusto_get_legs_dev(h, &Xd, &Ud, &Td));
    REQUIRE(Xd && Ud && Td);
    REQUIRE(gusto_legs_advance(h, 0) == GUSTO_ERR_STATE && strstr(gusto_last_error(h), "flying"));
    CHECK(gusto_set_problems(h, BQ, x_init, lo + NX, hi + NX, t_goal, 0, 0));          /* new problems: the timeline is gone */
    REQUIRE(gusto_get_legs(h, 0, 0, 0) == GUSTO_ERR_STATE && gusto_legs_advance(h, 0) == GUSTO_ERR_STATE);
    REQUIRE(gusto_get_legs_dev(h, 0, 0, 0) == GUSTO_ERR_STATE);

    printf("ok\n");
    for (int q = 0; q < BQ; q++)
        printf("%d %d %d %.17g %.17g %.17g %.17g %.17g %.17g\n", status[q], failed[q], ndone[q], Jt[q], gap[q * L + 1], arrive[q * L],
               arrive[q * L + 1], tj[q * NJ + 19], tj[q * NJ + 20]);
    CHECK(gusto_destroy(h));
    return 0;
}
