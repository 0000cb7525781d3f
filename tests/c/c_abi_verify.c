/* c_abi_verify.c -- plain C through include/gusto_hip.h: the post-solve verification entry points.
 * Two freeflyerSE2 problems (N = 50, tf = 200) on their straight-line inits: gusto_verify on the handle's own trajectories and on
 * the same ones passed as arrays, gusto_get_verify, gusto_interpolate / gusto_get_dense, the refusals (substep cap, TrajOpt
 * handle, calls before gusto_set_problems), with checks of its own; then one line "ok" and the report of both problems that
 * tests/test_gpu_verify.py compares with its numpy restatement.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_verify.c -o c_abi_verify -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd
 *   ./c_abi_verify boxes.txt      (boxes.txt: n_box, then 6 doubles per box: min xyz, max xyz)                        */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "gusto_hip.h"

#define CHECK(call) do { int rc_ = (call); if (rc_ != GUSTO_OK) { \
    fprintf(stderr, "%s -> %d: %s\n", #call, rc_, gusto_last_error(h)); return 2; } } while (0)
#define REQUIRE(cond) do { if (!(cond)) { fprintf(stderr, "line %d: %s\n", __LINE__, #cond); return 3; } } while (0)

int main(int argc, char** argv) {
    enum { N = 50, B = 2, NX = 6, NU = 3 };
    gusto_handle h = 0, ht = 0;
    int n_box = 0;
    if (argc < 2) { fprintf(stderr, "usage: c_abi_verify boxes.txt\n"); return 1; }
    FILE* f = fopen(argv[1], "r");
    if (!f || fscanf(f, "%d", &n_box) != 1) { fprintf(stderr, "cannot read %s\n", argv[1]); return 1; }
    double* boxes = (double*)malloc(sizeof(double) * 6 * (size_t)n_box);
    for (int i = 0; i < 6 * n_box; i++)
        if (fscanf(f, "%lf", &boxes[i]) != 1) { fprintf(stderr, "short box table\n"); return 1; }
    fclose(f);

    gusto_verify_opts o;
    REQUIRE(gusto_default_verify_opts(&o) == GUSTO_OK && o.dt_min == 0.1 && o.nstep == 0 && o.nstep_cap == 64 && o.dense_collision == 1);
    REQUIRE(gusto_verify(0, 0, 0, 0) == GUSTO_ERR_ARG);

    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 16, 0));
    CHECK(gusto_set_env(h, n_box, boxes, 0, 0));
    REQUIRE(gusto_verify(h, 0, 0, 0) == GUSTO_ERR_STATE);                         /* nothing set yet */
    const double x_init[B * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.6, 0.9, 0, 0, 0, 0};
    const double goal[B * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    const double tf[B] = {200.0, 100.0};
    CHECK(gusto_set_problems(h, B, x_init, goal, goal, tf, 0, 0));               /* straight-line inits */
    static double X[B * N * NX], U[B * N * NU], X2[B * N * NX], U2[B * N * NU];
    CHECK(gusto_get_traj(h, X, U));

    int freeA[B], knotA[B], sampA[B], freeB[B], knotB[B], sampB[B];
    double distA[B], dkA[B], defA[B], ddA[B], gapA[B], distB[B], dkB[B], defB[B], ddB[B], gapB[B], ms = -1.0;
    gusto_verify_report ra = {freeA, knotA, distA, dkA, defA, ddA, sampA, gapA}, rb = {freeB, knotB, distB, dkB, defB, ddB, sampB, gapB};
    REQUIRE(gusto_get_verify(h, &ra) == GUSTO_ERR_STATE);                         /* no report yet */
    CHECK(gusto_verify(h, 0, 0, 0));                                             /* the handle's own trajectories, default options */
    CHECK(gusto_get_verify(h, &ra));
    CHECK(gusto_last_verify_ms(h, &ms));
    REQUIRE(ms >= 0.0);
    CHECK(gusto_verify(h, X, U, &o));                                            /* the same trajectories as arrays */
    CHECK(gusto_get_verify(h, &rb));
    for (int b = 0; b < B; b++)
        REQUIRE(freeA[b] == freeB[b] && knotA[b] == knotB[b] && sampA[b] == sampB[b] && distA[b] == distB[b] && dkA[b] == dkB[b] &&
                defA[b] == defB[b] && ddA[b] == ddB[b] && gapA[b] == gapB[b]);
    CHECK(gusto_get_traj(h, X2, U2));                                            /* untouched */
    REQUIRE(!memcmp(X, X2, sizeof(X)) && !memcmp(U, U2, sizeof(U)));
    gusto_verify_report some = {0};                                              /* NULL = skip */
    some.max_gap = gapB;
    CHECK(gusto_get_verify(h, &some));

    /* dt = 200 / 49 and 100 / 49: 41 and 21 substeps of at most 0.1 s */
    int nfull_max = 0, nfull[B];
    REQUIRE(gusto_get_dense(h, nfull, 0, 0) == GUSTO_ERR_STATE);
    CHECK(gusto_interpolate(h, 0, 0, &o, &nfull_max));
    REQUIRE(nfull_max == 41 * (N - 1) + 1);
    double* Xf = (double*)malloc(sizeof(double) * B * (size_t)nfull_max * NX);
    double* Uf = (double*)malloc(sizeof(double) * B * (size_t)(nfull_max - 1) * NU);
    CHECK(gusto_get_dense(h, nfull, Xf, Uf));
    REQUIRE(nfull[0] == 41 * (N - 1) + 1 && nfull[1] == 21 * (N - 1) + 1);
    for (int b = 0; b < B; b++) {
        const int ns = (nfull[b] - 1) / (N - 1);
        const double* xf = Xf + (size_t)b * nfull_max * NX;
        for (int k = 0; k < N; k++)                                              /* every knot is a dense sample */
            REQUIRE(!memcmp(xf + (size_t)k * ns * NX, X + ((size_t)b * N + k) * NX, sizeof(double) * NX));
        for (int j = nfull[b] * NX; j < nfull_max * NX; j++) REQUIRE(xf[j] == 0.0);
    }
    o.nstep_cap = 40;                                                            /* 41 needed: refused, not clamped */
    REQUIRE(gusto_verify(h, 0, 0, &o) == GUSTO_ERR_ARG);
    o.nstep_cap = 64; o.nstep = 65;
    REQUIRE(gusto_verify(h, 0, 0, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_verify(h, X, 0, 0) == GUSTO_ERR_ARG);

    CHECK(gusto_create_trajopt(&ht, GUSTO_FREEFLYER_SE2, N, B, 272, 0));
    REQUIRE(gusto_set_problems(ht, B, x_init, goal, goal, tf, 0, 0) == GUSTO_OK);
    REQUIRE(gusto_verify(ht, 0, 0, 0) == GUSTO_ERR_ARG && strstr(gusto_last_error(ht), "TrajOpt"));
    REQUIRE(gusto_interpolate(ht, 0, 0, 0, 0) == GUSTO_ERR_ARG);
    gusto_destroy(ht);

    printf("ok\n");
    for (int b = 0; b < B; b++)
        printf("%d %d %.17g %.17g %.17g %.17g %d %.17g\n", freeA[b], knotA[b], distA[b], dkA[b], defA[b], ddA[b], sampA[b], gapA[b]);
    free(Xf); free(Uf); free(boxes);
    CHECK(gusto_destroy(h));
    return 0;
}
