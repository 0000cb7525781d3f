/* c_abi_fleet.c -- plain C through include/gusto_hip.h: fleet coordination.
 * Two freeflyerSE2 robots (N = 20) on constant-speed lines that cross at one point at one time, put on the handle as
 * gusto_interpolate(X, U): the getters and gusto_fleet_separation(NULL) before any call, the refusals of gusto_fleet_schedule
 * (R, the options, the order, the clock cap), then schedule, get, tracks, separation of the schedule's shifts and of a caller's,
 * with checks of its own; then one line "ok" and the two delays and the fleet's smallest separation, which
 * tests/test_gpu_fleet.py compares with the Python path.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_fleet.c -o c_abi_fleet -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 20, B = 2, R = 2, NX = 6, NU = 3, JMAX = 401 };
    gusto_handle h = 0;
    gusto_fleet_opts o, bad;
    gusto_fleet_report rep;
    const double p0[B][2] = {{-2, 0}, {0, -2}}, p1[B][2] = {{2, 0}, {0, 2}}, tf[B] = {40.0, 40.0};
    static double X[B * N * NX], U[B * N * NU], Q[B * JMAX * 2];
    double x0[B * NX], xg[B * NX], delay[B], min_sep[B], pair_sep[R * R], fleet_sep[1], stage_ms[3], ms = -1.0;
    int status[B], steps[B], blocker[B], partner[B], step[B], pair_step[R * R], n_s[1], n_b[1], n_c[1], span[1], J[B];
    int F = -1, Rr = -1, jmax = -1, nfull_max = 0, order_bad[B] = {1, 1}, order_rev[B] = {1, 0}, el[B] = {1, 1}, forced[B] = {0, 65};

    for (int b = 0; b < B; b++)
        for (int k = 0; k < N; k++) {
            const double t = (double)k / (N - 1);
            double* x = X + ((size_t)b * N + k) * NX;
            for (int i = 0; i < 2; i++) { x[i] = (1 - t) * p0[b][i] + t * p1[b][i]; x[3 + i] = (p1[b][i] - p0[b][i]) / tf[b]; }
        }
    memcpy(x0, X, sizeof(double) * NX); memcpy(x0 + NX, X + N * NX, sizeof(double) * NX);
    memcpy(xg, X + (N - 1) * NX, sizeof(double) * NX); memcpy(xg + NX, X + (2 * N - 1) * NX, sizeof(double) * NX);
    REQUIRE(gusto_default_fleet_opts(GUSTO_FREEFLYER_SE2, 0) == GUSTO_ERR_ARG && gusto_default_fleet_opts(9, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_default_fleet_opts(GUSTO_FREEFLYER_SE2, &o) == GUSTO_OK);
    REQUIRE(o.dt_clock == 0.1 && o.margin == 0.05 && o.n_delays == 64 && o.delay_stride == 10 && o.clock_cap == 8192 && o.components == 1 && o.prune == 1);
    REQUIRE(gusto_fleet_schedule(0, R, 0, 0, &o) == GUSTO_ERR_ARG && gusto_fleet_separation(0, R, 0, &o) == GUSTO_ERR_ARG);
    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 64, 0));
    REQUIRE(gusto_fleet_schedule(h, R, 0, el, &o) == GUSTO_ERR_STATE);                       /* no problems */
    CHECK(gusto_set_problems(h, B, x0, xg, xg, tf, 0, 0));
    REQUIRE(gusto_fleet_schedule(h, R, 0, el, &o) == GUSTO_ERR_STATE && strstr(gusto_last_error(h), "gusto_interpolate"));
    CHECK(gusto_interpolate(h, X, U, 0, &nfull_max));
    memset(&rep, 0, sizeof(rep));
    REQUIRE(gusto_get_fleet(h, &rep, 0, 0) == GUSTO_ERR_STATE && gusto_get_fleet_tracks(h, 0, 0, &jmax) == GUSTO_ERR_STATE);
    REQUIRE(gusto_last_fleet_ms(h, &ms) == GUSTO_ERR_STATE);
    REQUIRE(gusto_fleet_separation(h, R, 0, &o) == GUSTO_ERR_STATE);                         /* no schedule yet */
    o.delay_stride = 5;
    REQUIRE(gusto_fleet_schedule(h, 3, 0, el, &o) == GUSTO_ERR_ARG && gusto_fleet_schedule(h, 65, 0, el, &o) == GUSTO_ERR_ARG);
    bad = o; bad.n_delays = 0;
    REQUIRE(gusto_fleet_schedule(h, R, 0, el, &bad) == GUSTO_ERR_ARG && strstr(gusto_last_error(h), "n_delays"));
    bad = o; bad.dt_clock = -0.1;
    REQUIRE(gusto_fleet_schedule(h, R, 0, el, &bad) == GUSTO_ERR_ARG);
    REQUIRE(gusto_fleet_schedule(h, R, order_bad, el, &o) == GUSTO_ERR_ARG && strstr(gusto_last_error(h), "fleet 0"));
    bad = o; bad.clock_cap = 400;
    REQUIRE(gusto_fleet_schedule(h, R, 0, el, &bad) == GUSTO_ERR_ARG && strstr(gusto_last_error(h), "problem 0"));
    REQUIRE(gusto_get_fleet(h, 0, 0, 0) == GUSTO_ERR_STATE);                                 /* the refusals left no report */

    CHECK(gusto_fleet_schedule(h, R, 0, el, &o));
    rep.status = status; rep.delay_steps = steps; rep.delay = delay; rep.blocker = blocker; rep.min_sep = min_sep; rep.partner = partner;
    rep.step = step; rep.pair_min_sep = pair_sep; rep.pair_step = pair_step; rep.n_scheduled = n_s; rep.n_blocked = n_b;
    rep.n_conflicts = n_c; rep.fleet_min_sep = fleet_sep; rep.makespan_steps = span; rep.stage_ms = stage_ms;
    CHECK(gusto_get_fleet(h, &rep, &F, &Rr));
    CHECK(gusto_last_fleet_ms(h, &ms));
    REQUIRE(F == 1 && Rr == R && ms > 0.0 && stage_ms[0] > 0.0 && stage_ms[1] > 0.0 && stage_ms[2] > 0.0);
    REQUIRE(status[0] == GUSTO_FLEET_SCHEDULED && status[1] == GUSTO_FLEET_SCHEDULED && steps[0] == 0 && steps[1] == 70);
    REQUIRE(blocker[0] == -1 && blocker[1] == 0 && delay[0] == 0.0 && delay[1] == 70 * o.dt_clock);
    REQUIRE(n_s[0] == 2 && n_b[0] == 0 && n_c[0] == 0 && span[0] == 70 + 400 && partner[0] == 1 && partner[1] == 0);
    REQUIRE(fleet_sep[0] > o.margin && fleet_sep[0] == min_sep[0] && min_sep[0] == min_sep[1] && pair_sep[1] == pair_sep[2]);
    REQUIRE(isinf(pair_sep[0]) && pair_step[0] == -1 && pair_step[1] == step[0]);
    CHECK(gusto_get_fleet_tracks(h, 0, 0, &jmax));                                           /* the size query */
    REQUIRE(jmax == JMAX);
    CHECK(gusto_get_fleet_tracks(h, J, Q, 0));
    REQUIRE(J[0] == JMAX && J[1] == JMAX && Q[0] == -2.0 && Q[1] == 0.0 && Q[(JMAX - 1) * 2] == X[(N - 1) * NX]);
    {
        const double first = fleet_sep[0];
        CHECK(gusto_fleet_separation(h, R, 0, &o));                                          /* the schedule's shifts again */
        CHECK(gusto_get_fleet(h, &rep, 0, 0));
        REQUIRE(fleet_sep[0] == first && steps[1] == 70 && stage_ms[1] == 0.0);
        CHECK(gusto_fleet_separation(h, R, forced, &o));                                     /* one candidate earlier: a conflict */
        CHECK(gusto_get_fleet(h, &rep, 0, 0));
        REQUIRE(n_c[0] == 1 && fleet_sep[0] < o.margin && steps[1] == 65 && blocker[1] == -1);
        forced[1] = -2;
        REQUIRE(gusto_fleet_separation(h, R, forced, &o) == GUSTO_ERR_ARG && strstr(gusto_last_error(h), "problem 1"));
        CHECK(gusto_fleet_schedule(h, R, order_rev, el, &o));                                /* reversed: robot 0 waits */
        CHECK(gusto_get_fleet(h, &rep, 0, 0));
        REQUIRE(steps[0] == 70 && steps[1] == 0 && blocker[0] == 1);
        CHECK(gusto_fleet_schedule(h, R, 0, el, &o));
        CHECK(gusto_get_fleet(h, &rep, 0, 0));
        REQUIRE(fleet_sep[0] == first);
    }
    printf("ok\n%d %d %.17g\n", steps[0], steps[1], fleet_sep[0]);
    CHECK(gusto_set_problems(h, B, x0, xg, xg, tf, 0, 0));                                   /* new problems: the stage's state is gone */
    REQUIRE(gusto_get_fleet(h, 0, 0, 0) == GUSTO_ERR_STATE && gusto_fleet_separation(h, R, 0, &o) == GUSTO_ERR_STATE);
    CHECK(gusto_destroy(h));
    return 0;
}
