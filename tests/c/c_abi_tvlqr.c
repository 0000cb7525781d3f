/* c_abi_tvlqr.c -- plain C through include/gusto_hip.h: the time-varying LQR entry points.
 * Two freeflyerSE2 problems (N = 50, tf = 200 and 100) on their straight-line inits: gusto_default_tvlqr_opts, gusto_tvlqr on the
 * handle's own trajectories and on the same ones passed as arrays, gusto_get_tvlqr with and without store_P, the refusals
 * (weights, substep cap, X without U, TrajOpt handle, calls before gusto_set_problems), with checks of its own -- the double
 * integrator's [Ad | Bd] in closed form among them; then one line "ok" and, per problem, the first gain row and P_1[0][0] that
 * tests/test_gpu_tvlqr.py compares with its numpy restatement.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_tvlqr.c -o c_abi_tvlqr -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(void) {
    enum { N = 50, B = 2, NX = 6, NU = 3, NZ = NX + NU };
    gusto_handle h = 0, ht = 0;
    gusto_tvlqr_opts o, bad;
    REQUIRE(gusto_default_tvlqr_opts(GUSTO_FREEFLYER_SE2, &o) == GUSTO_OK);
    REQUIRE(o.dt_min == 0.1 && o.nstep == 0 && o.nstep_cap == 64 && o.store_P == 0);
    for (int i = 0; i < GUSTO_MAXN; i++) REQUIRE(o.Q[i] == (i < NX ? 1.0 : 0.0) && o.Qf[i] == o.Q[i]);
    for (int i = 0; i < GUSTO_MAXM; i++) REQUIRE(o.R[i] == (i < NU ? 1.0 : 0.0));
    REQUIRE(gusto_default_tvlqr_opts(11, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_tvlqr(0, 0, 0, 0) == GUSTO_ERR_ARG);

    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 16, 0));
    REQUIRE(gusto_tvlqr(h, 0, 0, 0) == GUSTO_ERR_STATE);                          /* nothing set yet */
    const double x_init[B * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.6, 0.9, 0, 0, 0, 0};
    const double goal[B * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    const double tf[B] = {200.0, 100.0};
    CHECK(gusto_set_problems(h, B, x_init, goal, goal, tf, 0, 0));                /* straight-line inits */
    static double X[B * N * NX], U[B * N * NU], X2[B * N * NX], U2[B * N * NU];
    CHECK(gusto_get_traj(h, X, U));

    static double KA[B * (N - 1) * NU * NX], KB[B * (N - 1) * NU * NX], AB[B * (N - 1) * NX * NZ];
    static double P1[B * NX * NX], Pall[B * N * NX * NX];
    int st[B], fk[B];
    double ms = -1.0;
    REQUIRE(gusto_get_tvlqr(h, st, fk, KA, 0, 0) == GUSTO_ERR_STATE);             /* no gains yet */
    REQUIRE(gusto_last_tvlqr_ms(h, &ms) == GUSTO_ERR_STATE);
    o.Q[0] = 4.0; o.R[2] = 0.5; o.Qf[5] = 9.0;
    o.nstep_cap = 41;                                                             /* dt = 200 / 49: 41 substeps of at most 0.1 s */
    CHECK(gusto_tvlqr(h, 0, 0, &o));                                              /* the handle's own trajectories */
    CHECK(gusto_get_tvlqr(h, st, fk, KA, P1, AB));
    CHECK(gusto_last_tvlqr_ms(h, &ms));
    REQUIRE(ms >= 0.0);
    for (int b = 0; b < B; b++) {
        REQUIRE(st[b] == 1 && fk[b] == 0);
        const double dt = tf[b] / (N - 1);
        for (int k = 0; k < N - 1; k++) {                                         /* Ad = [[I, dt I], [0, I]], Bd rows 3..5 = dt Bv */
            const double* M = AB + ((size_t)(b * (N - 1) + k)) * NX * NZ;
            for (int i = 0; i < NX; i++)
                for (int j = 0; j < NX; j++) {
                    const double want = i == j ? 1.0 : (j == i + 3 ? dt : 0.0);
                    REQUIRE(fabs(M[i * NZ + j] - want) <= 1e-12 * dt);
                }
            REQUIRE(fabs(M[0 * NZ + NX] - 0.5 * dt * M[3 * NZ + NX]) <= 1e-12 * dt * dt && M[3 * NZ + NX] > 0.0);
        }
        for (int i = 0; i < NX; i++)
            for (int j = 0; j < NX; j++) REQUIRE(P1[(b * NX + i) * NX + j] == P1[(b * NX + j) * NX + i]);
    }
    o.store_P = 1;
    CHECK(gusto_tvlqr(h, X, U, &o));                                              /* the same trajectories as arrays, every P */
    CHECK(gusto_get_tvlqr(h, 0, 0, KB, Pall, 0));
    REQUIRE(!memcmp(KA, KB, sizeof(KA)));
    for (int b = 0; b < B; b++) {
        REQUIRE(!memcmp(Pall + (size_t)b * N * NX * NX, P1 + (size_t)b * NX * NX, sizeof(double) * NX * NX));
        const double* PN = Pall + ((size_t)b * N + N - 1) * NX * NX;               /* P_N = diag(Qf) */
        for (int i = 0; i < NX * NX; i++) REQUIRE(PN[i] == (i / NX == i % NX ? o.Qf[i / NX] : 0.0));
    }
    CHECK(gusto_get_traj(h, X2, U2));                                             /* untouched */
    REQUIRE(!memcmp(X, X2, sizeof(X)) && !memcmp(U, U2, sizeof(U)));

    bad = o; bad.R[1] = 0.0;
    REQUIRE(gusto_tvlqr(h, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.Q[3] = -1.0;
    REQUIRE(gusto_tvlqr(h, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.Qf[0] = NAN;
    REQUIRE(gusto_tvlqr(h, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.nstep_cap = 40;                                                  /* 41 needed: refused, not clamped */
    REQUIRE(gusto_tvlqr(h, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.nstep = 65; bad.nstep_cap = 64;
    REQUIRE(gusto_tvlqr(h, 0, 0, &bad) == GUSTO_ERR_ARG);
    REQUIRE(gusto_tvlqr(h, X, 0, &o) == GUSTO_ERR_ARG);
    CHECK(gusto_get_tvlqr(h, st, fk, KB, 0, 0));                                  /* a refused call leaves the last result */
    REQUIRE(!memcmp(KA, KB, sizeof(KA)));

    CHECK(gusto_create_trajopt(&ht, GUSTO_FREEFLYER_SE2, N, B, 272, 0));
    REQUIRE(gusto_set_problems(ht, B, x_init, goal, goal, tf, 0, 0) == GUSTO_OK);
    REQUIRE(gusto_tvlqr(ht, 0, 0, 0) == GUSTO_ERR_ARG && strstr(gusto_last_error(ht), "TrajOpt"));
    gusto_destroy(ht);

    printf("ok\n");
    for (int b = 0; b < B; b++) {
        const double* K1 = KA + (size_t)b * (N - 1) * NU * NX;
        printf("%.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", K1[0], K1[1], K1[2], K1[3], K1[4], K1[5], P1[(size_t)b * NX * NX]);
    }
    CHECK(gusto_destroy(h));
    return 0;
}
