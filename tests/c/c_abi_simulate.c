/* c_abi_simulate.c -- plain C through include/gusto_hip.h: the closed-loop roll-out entry points.
 * Two freeflyerSE2 problems (N = 50, tf = 200 and 100) on their straight-line inits beside one keep-out box:
 * gusto_default_simulate_opts, gusto_tvlqr then gusto_simulate on the handle's own trajectories and gains and on the same ones
 * passed as arrays (the same bits), generated against caller-supplied zero perturbations, gusto_get_simulate with null
 * pointers, gusto_get_simulate_knots, the refusals, with checks of its own; then one line "ok" and, per problem, x_final of
 * sample 7, min_dist, n_free and n_clipped, which tests/test_gpu_simulate.py compares with its numpy restatement.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_simulate.c -o c_abi_simulate -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 50, B = 2, NX = 6, NU = 3, S = 8 };
    gusto_handle h = 0, ht = 0;
    gusto_simulate_opts o, bad;
    REQUIRE(gusto_default_simulate_opts(GUSTO_FREEFLYER_SE2, &o) == GUSTO_OK);
    REQUIRE(o.n_samples == 64 && o.seed == 0 && o.first_problem == 0 && o.dt_min == 0.1 && o.nstep == 0 && o.nstep_cap == 64);
    REQUIRE(o.dense_collision == 1 && o.store_knots == 0);
    for (int i = 0; i < GUSTO_MAXN; i++) REQUIRE(o.dx0[i] == (i < NX ? 0.01 : 0.0));
    for (int i = 0; i < GUSTO_MAXM; i++) REQUIRE(o.du0[i] == 0.0 && o.u_lo[i] == -INFINITY && o.u_hi[i] == INFINITY);
    REQUIRE(gusto_default_simulate_opts(11, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_simulate(0, 0, 0, 0, 0, 0) == GUSTO_ERR_ARG);

    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 16, 0));
    REQUIRE(gusto_simulate(h, 0, 0, 0, 0, 0) == GUSTO_ERR_STATE);                  /* nothing set yet */
    const double box[6] = {1.0, 0.6, -1.0, 1.2, 0.8, 1.0};                          /* one keep-out box beside the paths */
    CHECK(gusto_set_env(h, 1, box, 0, 0));
    const double x_init[B * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.6, 0.9, 0, 0, 0, 0};
    const double goal[B * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    const double tf[B] = {200.0, 100.0};
    CHECK(gusto_set_problems(h, B, x_init, goal, goal, tf, 0, 0));                /* straight-line inits */
    static double X[B * N * NX], U[B * N * NU], K[B * (N - 1) * NU * NX];
    CHECK(gusto_get_traj(h, X, U));
    REQUIRE(gusto_simulate(h, 0, 0, 0, 0, 0) == GUSTO_ERR_STATE && strstr(gusto_last_error(h), "gusto_tvlqr"));   /* no gains yet */
    gusto_tvlqr_opts lq;
    CHECK(gusto_default_tvlqr_opts(GUSTO_FREEFLYER_SE2, &lq));
    CHECK(gusto_tvlqr(h, 0, 0, &lq));
    CHECK(gusto_get_tvlqr(h, 0, 0, K, 0, 0));

    static double dA[B * S], dB[B * S], xA[B * S * NX], xB[B * S * NX], Xcl[B * N * S * NX], dev[B * NX], fdev[B * NX], mind[B];
    static int fA[B * S], fB[B * S], nfree[B], nfin[B], nclip[B], worst[B], wdense[B];
    gusto_simulate_report rep;
    double ms = -1.0;
    memset(&rep, 0, sizeof(rep));
    REQUIRE(gusto_get_simulate(h, &rep) == GUSTO_ERR_STATE && gusto_last_simulate_ms(h, &ms) == GUSTO_ERR_STATE);
    o.n_samples = S; o.seed = 11;
    for (int i = 0; i < NU; i++) { o.u_lo[i] = -0.05; o.u_hi[i] = 0.05; }
    CHECK(gusto_simulate(h, 0, 0, 0, 0, &o));                                      /* the handle's own trajectories and gains */
    rep.sample_min_dist = dA; rep.sample_flags = fA; rep.x_final = xA;
    rep.n_free = nfree; rep.n_finite = nfin; rep.n_clipped = nclip; rep.worst_sample = worst; rep.worst_dense_sample = wdense;
    rep.min_dist = mind; rep.max_dev = dev; rep.max_final_dev = fdev;
    CHECK(gusto_get_simulate(h, &rep));
    CHECK(gusto_last_simulate_ms(h, &ms));
    REQUIRE(ms >= 0.0);
    REQUIRE(gusto_get_simulate_knots(h, Xcl) == GUSTO_ERR_STATE);                  /* not asked for */
    for (int b = 0; b < B; b++) {
        REQUIRE(nfin[b] == S && nfree[b] <= S && nclip[b] >= 0 && nclip[b] <= S);
        int free_ = 0;
        double m = INFINITY;
        for (int s = 0; s < S; s++) {
            REQUIRE(((fA[b * S + s] & 1) != 0) == (dA[b * S + s] < 0) && !(fA[b * S + s] & 4));
            free_ += !(fA[b * S + s] & 1);
            if (dA[b * S + s] < m) m = dA[b * S + s];
        }
        REQUIRE(free_ == nfree[b] && m == mind[b] && dA[b * S + worst[b]] == m && wdense[b] >= 0);
        for (int i = 0; i < NX; i++) REQUIRE(fdev[b * NX + i] <= dev[b * NX + i] && dev[b * NX + i] >= (i < 3 ? 0.0 : 0.0));
    }
    o.store_knots = 1;
    CHECK(gusto_simulate(h, X, U, K, 0, &o));                                      /* the same as arrays, with the knots */
    memset(&rep, 0, sizeof(rep));
    rep.sample_min_dist = dB; rep.sample_flags = fB; rep.x_final = xB;
    CHECK(gusto_get_simulate(h, &rep));
    REQUIRE(!memcmp(dA, dB, sizeof(dA)) && !memcmp(fA, fB, sizeof(fA)) && !memcmp(xA, xB, sizeof(xA)));
    CHECK(gusto_get_simulate_knots(h, Xcl));
    for (int b = 0; b < B; b++) {
        REQUIRE(!memcmp(Xcl + ((size_t)(b * N + N - 1) * S) * NX, xA + (size_t)b * S * NX, sizeof(double) * S * NX));   /* knot N */
        REQUIRE(!memcmp(Xcl + ((size_t)(b * N) * S) * NX, X + (size_t)b * N * NX, sizeof(double) * NX));                /* sample 0 starts at X_1 */
    }
    static double X2[B * N * NX], U2[B * N * NU], K2[B * (N - 1) * NU * NX];
    CHECK(gusto_get_traj(h, X2, U2));                                             /* untouched */
    CHECK(gusto_get_tvlqr(h, 0, 0, K2, 0, 0));
    REQUIRE(!memcmp(X, X2, sizeof(X)) && !memcmp(U, U2, sizeof(U)) && !memcmp(K, K2, sizeof(K)));

    bad = o; bad.n_samples = 0;
    REQUIRE(gusto_simulate(h, 0, 0, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.n_samples = 4097;
    REQUIRE(gusto_simulate(h, 0, 0, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.u_lo[1] = 0.06;
    REQUIRE(gusto_simulate(h, 0, 0, 0, 0, &bad) == GUSTO_ERR_ARG && strstr(gusto_last_error(h), "u_lo"));
    bad = o; bad.dx0[2] = -0.01;
    REQUIRE(gusto_simulate(h, 0, 0, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.nstep_cap = 40;                                                  /* 41 needed: refused, not clamped */
    REQUIRE(gusto_simulate(h, 0, 0, 0, 0, &bad) == GUSTO_ERR_ARG);
    REQUIRE(gusto_simulate(h, X, 0, 0, 0, &o) == GUSTO_ERR_ARG);
    memset(&rep, 0, sizeof(rep));
    rep.sample_min_dist = dB;
    CHECK(gusto_get_simulate(h, &rep));                                           /* a refused call leaves the last result */
    REQUIRE(!memcmp(dA, dB, sizeof(dA)));

    CHECK(gusto_create_trajopt(&ht, GUSTO_FREEFLYER_SE2, N, B, 272, 0));
    REQUIRE(gusto_set_problems(ht, B, x_init, goal, goal, tf, 0, 0) == GUSTO_OK);
    REQUIRE(gusto_simulate(ht, 0, 0, 0, 0, 0) == GUSTO_ERR_ARG && strstr(gusto_last_error(ht), "TrajOpt"));
    gusto_destroy(ht);

    printf("ok\n");
    for (int b = 0; b < B; b++) {
        const double* x7 = xA + ((size_t)b * S + 7) * NX;
        printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g %d %d\n", x7[0], x7[1], x7[2], x7[3], x7[4], x7[5], mind[b], nfree[b], nclip[b]);
    }
    CHECK(gusto_destroy(h));
    return 0;
}
