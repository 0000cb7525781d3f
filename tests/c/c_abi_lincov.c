/* c_abi_lincov.c -- plain C through include/gusto_hip.h: the linear covariance entry points.
 * Two freeflyerSE2 problems (N = 50, tf = 200 and 100) on their straight-line inits next to one box: gusto_default_lincov_opts,
 * gusto_tvlqr, gusto_lincov on the handle's own trajectories and on the same ones passed as arrays with the gains passed back,
 * gusto_get_lincov with and without store_S, the refusals (options, S0, X without U, no gusto_tvlqr yet, TrajOpt handle, calls
 * before gusto_set_problems), with checks of its own -- S_1 = S0, Sxx symmetric, the summaries against the per-knot rows; then
 * one line "ok" and, per problem, the indices, the summaries and the last sigma_x[0] and sigma_u[2] that
 * tests/test_gpu_lincov.py compares with its numpy restatement.
 *   gcc -std=c99 -Iinclude tests/c/c_abi_lincov.c -o c_abi_lincov -L gusto.jl_amd -lgusto_hip -lm -Wl,-rpath,$PWD/gusto.jl_amd */
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
    gusto_lincov_opts o, bad;
    gusto_tvlqr_opts to;
    gusto_lincov_report rep;
    REQUIRE(gusto_default_lincov_opts(GUSTO_FREEFLYER_SE2, &o) == GUSTO_OK);
    REQUIRE(o.store_S == 0);
    for (int i = 0; i < GUSTO_MAXN; i++) REQUIRE(o.dx0[i] == (i < NX ? 0.01 : 0.0));
    for (int i = 0; i < GUSTO_MAXM; i++) REQUIRE(o.du0[i] == 0.0 && o.du_white[i] == 0.0 && o.u_lo[i] == -INFINITY && o.u_hi[i] == INFINITY);
    REQUIRE(gusto_default_lincov_opts(11, &o) == GUSTO_ERR_ARG);
    REQUIRE(gusto_lincov(0, 0, 0, 0, 0, 0) == GUSTO_ERR_ARG);

    CHECK(gusto_create(&h, GUSTO_FREEFLYER_SE2, N, B, 16, 0));
    REQUIRE(gusto_lincov(h, 0, 0, 0, 0, 0) == GUSTO_ERR_STATE);                   /* nothing set yet */
    const double box[6] = {1.4, 0.2, -0.2, 1.8, 0.6, 0.2};
    CHECK(gusto_set_env(h, 1, box, 0, 0));
    const double x_init[B * NX] = {0.2, 2.4, 0, 0, 0, 0, 0.6, 0.9, 0, 0, 0, 0};
    const double goal[B * NX] = {3.0, 0.5, 0, 0.05, -0.05, 0, 3.0, 0.5, 0, 0.05, -0.05, 0};
    const double tf[B] = {200.0, 100.0};
    CHECK(gusto_set_problems(h, B, x_init, goal, goal, tf, 0, 0));                /* straight-line inits */
    static double X[B * N * NX], U[B * N * NU], K[B * (N - 1) * NU * NX];
    CHECK(gusto_get_traj(h, X, U));
    REQUIRE(gusto_lincov(h, 0, 0, 0, 0, 0) == GUSTO_ERR_STATE && strstr(gusto_last_error(h), "gusto_tvlqr"));   /* no Jacobians yet */
    CHECK(gusto_default_tvlqr_opts(GUSTO_FREEFLYER_SE2, &to));
    CHECK(gusto_tvlqr(h, 0, 0, &to));
    CHECK(gusto_get_tvlqr(h, 0, 0, K, 0, 0));

    static double sx[B * N * NX], su[B * (N - 1) * NU], zo[B * N], Sxx[B * N * NX * NX], sx2[B * N * NX], zo2[B * N];
    int st[B], fk[B], ok_[B], op[B], ck[B], ce[B];
    double mzo[B], pb[B], mzc[B], mzo2[B], ms = -1.0;
    memset(&rep, 0, sizeof(rep));
    rep.status = st;
    REQUIRE(gusto_get_lincov(h, &rep) == GUSTO_ERR_STATE);                        /* no result yet */
    REQUIRE(gusto_last_lincov_ms(h, &ms) == GUSTO_ERR_STATE);
    CHECK(gusto_default_lincov_opts(GUSTO_FREEFLYER_SE2, &o));
    for (int i = 0; i < NX; i++) o.dx0[i] = 0.02;
    for (int i = 0; i < NU; i++) { o.du0[i] = 0.01; o.du_white[i] = 0.005; o.u_lo[i] = -0.3 + 0.05 * i; o.u_hi[i] = 0.4; }
    CHECK(gusto_lincov(h, 0, 0, 0, 0, &o));                                       /* the handle's own trajectories and gains */
    CHECK(gusto_last_lincov_ms(h, &ms));
    REQUIRE(ms >= 0.0);
    rep.fail_knot = fk; rep.obs_knot = ok_; rep.obs_pair = op; rep.ctl_knot = ck; rep.ctl_entry = ce;
    rep.min_z_obs = mzo; rep.p_collision_bound = pb; rep.min_z_ctl = mzc; rep.sigma_x = sx; rep.sigma_u = su; rep.z_obs = zo;
    CHECK(gusto_get_lincov(h, &rep));
    rep.Sxx = Sxx;
    REQUIRE(gusto_get_lincov(h, &rep) == GUSTO_ERR_STATE);                        /* no Sxx without store_S */
    for (int b = 0; b < B; b++) {
        REQUIRE(st[b] == 1 && fk[b] == 0);
        double zmin = INFINITY, psum = 0.0;
        int kmin = 0;
        for (int k = 0; k < N; k++) {
            if (zo[b * N + k] < zmin) { zmin = zo[b * N + k]; kmin = k + 1; }
            psum += 0.5 * erfc(zo[b * N + k] / sqrt(2.0));
        }
        REQUIRE(zmin == mzo[b] && kmin == ok_[b] && op[b] >= 0 && op[b] < 2);     /* two components, one box */
        REQUIRE(fabs(pb[b] - (psum < 1.0 ? psum : 1.0)) <= 1e-12);
        REQUIRE(ck[b] >= 1 && ck[b] <= N - 1 && ce[b] >= 0 && ce[b] < NU && mzc[b] < INFINITY);
        for (int i = 0; i < NX; i++) REQUIRE(fabs(sx[b * N * NX + i] - sqrt(0.02 * 0.02 / 3.0)) <= 1e-17);
    }
    o.store_S = 1;
    rep.sigma_x = sx2; rep.z_obs = zo2; rep.min_z_obs = mzo2;
    CHECK(gusto_lincov(h, X, U, K, 0, &o));                                       /* the same as arrays, every Sxx */
    CHECK(gusto_get_lincov(h, &rep));
    REQUIRE(!memcmp(sx, sx2, sizeof(sx)) && !memcmp(zo, zo2, sizeof(zo)) && !memcmp(mzo, mzo2, sizeof(mzo)));
    for (int b = 0; b < B; b++)
        for (int k = 0; k < N; k++) {
            const double* S = Sxx + ((size_t)b * N + k) * NX * NX;
            for (int i = 0; i < NX; i++) {
                REQUIRE(fabs(sqrt(S[i * NX + i] > 0.0 ? S[i * NX + i] : 0.0) - sx[((size_t)b * N + k) * NX + i]) <= 1e-15 * sx[((size_t)b * N + k) * NX + i]);
                for (int j = 0; j < NX; j++) {
                    REQUIRE(S[i * NX + j] == S[j * NX + i]);
                    if (k == 0) REQUIRE(S[i * NX + j] == (i == j ? 0.02 * 0.02 / 3.0 : 0.0));   /* S_1 = S0 */
                }
            }
        }

    bad = o; bad.dx0[2] = -1.0;
    REQUIRE(gusto_lincov(h, 0, 0, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.du_white[1] = NAN;
    REQUIRE(gusto_lincov(h, 0, 0, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.u_lo[0] = 0.5;
    REQUIRE(gusto_lincov(h, 0, 0, 0, 0, &bad) == GUSTO_ERR_ARG);
    bad = o; bad.store_S = 3;
    REQUIRE(gusto_lincov(h, 0, 0, 0, 0, &bad) == GUSTO_ERR_ARG);
    static double S0[B * NZ * NZ];
    for (int b = 0; b < B; b++) for (int i = 0; i < NZ; i++) S0[(b * NZ + i) * NZ + i] = 1e-4;
    S0[(1 * NZ + 2) * NZ + 5] = 1e-5;                                             /* not symmetric */
    REQUIRE(gusto_lincov(h, 0, 0, 0, S0, &o) == GUSTO_ERR_ARG && strstr(gusto_last_error(h), "problem 1"));
    S0[(1 * NZ + 5) * NZ + 2] = 1e-5;
    CHECK(gusto_lincov(h, 0, 0, 0, S0, &o));
    REQUIRE(gusto_lincov(h, X, 0, 0, 0, &o) == GUSTO_ERR_ARG);
    o.store_S = 0;
    CHECK(gusto_lincov(h, 0, 0, 0, 0, &o));                                       /* the first result again */
    rep.Sxx = 0;
    CHECK(gusto_get_lincov(h, &rep));
    REQUIRE(!memcmp(sx, sx2, sizeof(sx)));

    CHECK(gusto_create_trajopt(&ht, GUSTO_FREEFLYER_SE2, N, B, 272, 0));
    REQUIRE(gusto_set_problems(ht, B, x_init, goal, goal, tf, 0, 0) == GUSTO_OK);
    REQUIRE(gusto_lincov(ht, 0, 0, 0, 0, 0) == GUSTO_ERR_ARG && strstr(gusto_last_error(ht), "TrajOpt"));
    gusto_destroy(ht);

    printf("ok\n");
    for (int b = 0; b < B; b++)
        printf("%d %d %d %d %.17g %.17g %.17g %.17g %.17g\n", ok_[b], op[b], ck[b], ce[b], mzo[b], pb[b], mzc[b],
               sx[((size_t)b * N + N - 1) * NX], su[((size_t)b * (N - 1) + N - 2) * NU + 2]);
    CHECK(gusto_destroy(h));
    return 0;
}
