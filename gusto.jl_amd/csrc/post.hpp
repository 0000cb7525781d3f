// post.hpp -- the host path of the post-solve stages (shoot.hip, verify.hip, tvlqr.hip, simulate.hip, lincov.hip, tighten.hip);
// seed.hpp, the host path of the seeding stages, builds on it, and nothing else includes it.  Plain
// functions that answer a GUSTO_* code and leave the text in h->err: `if (int rc = ...) return rc;` at the call site.  A new
// stage starts from these, from a struct of its own next to ShootState / VerifyState / TvlqrState / SimulateState / LincovState
// (handle.hpp) and, on the device, from rollout.hpp: the roll-out every stage but shoot.hip shares.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "handle.hpp"

// a refusal: "<who>: <what>" in h->err, and the code
static inline int refuse(gusto_handle h, const std::string& who, const std::string& what, int rc = GUSTO_ERR_ARG) {
    h->err = who + ": " + what;
    return rc;
}

// the refusals every stage begins with (a stage without X, U passes nulls), then the handle's device and its enqueued solve
static inline int post_enter(gusto_handle h, const char* who, const double* X, const double* U) {
    if (!h) return GUSTO_ERR_ARG;
    const std::string w(who);
    if (h->trajopt) { h->err = w + ": TrajOpt handle (its controls carry the defect variables; not supported)"; return GUSTO_ERR_ARG; }
    if (!h->have_problems) { h->err = w + ": call gusto_set_problems first"; return GUSTO_ERR_STATE; }
    if ((X == nullptr) != (U == nullptr)) { h->err = w + ": X and U are given together or not at all"; return GUSTO_ERR_ARG; }
    HIPCHK(h, hipSetDevice(h->device));
    return gusto_finish(h);
}

// the roll-out options of gusto_verify_opts / gusto_tvlqr_opts (false: the caller's "bad options")
static inline bool nstep_opts_ok(double dt_min, int nstep, int nstep_cap) {
    return nstep >= 0 && nstep_cap >= 1 && (nstep > 0 || dt_min > 0);
}
// Nstep of every problem, never clamped: nstep, or ceil(dt / dt_min) and the largest of them in *nstep_max; outside
// 1 .. nstep_cap: GUSTO_ERR_ARG and the text, which names the first such problem, in *err.  No device, no handle.
static inline int resolve_nstep_host(const double* tf, size_t B, int N, double dt_min, int nstep, int nstep_cap, const char* who,
                                     int* nstep_max, std::string* err) {
    *nstep_max = nstep;
    if (nstep > nstep_cap) { *err = std::string(who) + ": nstep above nstep_cap"; return GUSTO_ERR_ARG; }
    for (size_t b = 0; nstep == 0 && b < B; b++) {
        const double q = ceil(tf[b] / (double)(N - 1) / dt_min);
        if (!(q >= 1 && q <= (double)nstep_cap)) {
            *err = std::string(who) + ": problem " + std::to_string(b) + " needs ceil(dt / dt_min) = " + std::to_string(q) + " substeps, outside 1 .. nstep_cap";
            return GUSTO_ERR_ARG;
        }
        *nstep_max = std::max(*nstep_max, (int)q);
    }
    return GUSTO_OK;
}
// ... of the handle's problems: tf comes back from the device when the count depends on it
static inline int resolve_nstep(gusto_handle h, const char* who, double dt_min, int nstep, int nstep_cap, int* nstep_max) {
    std::vector<double> tf(nstep == 0 ? h->B : 0);
    if (!tf.empty()) {
        HIPCHK(h, hipMemcpyAsync(tf.data(), h->d_tf, sizeof(double) * tf.size(), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return resolve_nstep_host(tf.data(), tf.size(), h->N, dt_min, nstep, nstep_cap, who, nstep_max, &h->err);
}

// The arguments of gusto_lincov for a model of n states and m controls: the options, and the caller's S0 [B][n + m][n + m]
// (null: the default start).  GUSTO_ERR_ARG and the text, which names the offending entry (and problem), in *err.  Whether S0
// is positive semi-definite is the caller's business.  No device, no handle.
static inline int lincov_args_host(int n, int m, size_t B, const gusto_lincov_opts* o, const double* S0, std::string* err,
                                   const char* who = "gusto_lincov") {
    const std::string w = std::string(who) + ": ";
    const auto width_ok = [](double v) { return v >= 0 && v < INFINITY; };
    if (o->store_S != 0 && o->store_S != 1) { *err = w + "store_S must be 0 or 1"; return GUSTO_ERR_ARG; }
    for (int i = 0; i < n; i++)
        if (!width_ok(o->dx0[i])) { *err = w + "dx0 must be finite and >= 0 (entry " + std::to_string(i) + ")"; return GUSTO_ERR_ARG; }
    for (int i = 0; i < m; i++) {
        if (!width_ok(o->du0[i])) { *err = w + "du0 must be finite and >= 0 (entry " + std::to_string(i) + ")"; return GUSTO_ERR_ARG; }
        if (!width_ok(o->du_white[i])) { *err = w + "du_white must be finite and >= 0 (entry " + std::to_string(i) + ")"; return GUSTO_ERR_ARG; }
        if (!(o->u_lo[i] <= o->u_hi[i])) { *err = w + "u_lo must not exceed u_hi (entry " + std::to_string(i) + ")"; return GUSTO_ERR_ARG; }
    }
    const size_t nz = (size_t)(n + m);
    for (size_t b = 0; S0 && b < B; b++) {
        const double* S = S0 + b * nz * nz;
        const auto where = [&](size_t i, size_t j) {
            return " (problem " + std::to_string(b) + ", entry " + std::to_string(i) + ", " + std::to_string(j) + ")";
        };
        for (size_t i = 0; i < nz; i++)
            for (size_t j = 0; j < nz; j++) {
                const double v = S[i * nz + j];
                if (!(fabs(v) < INFINITY)) { *err = w + "S0 must be finite" + where(i, j); return GUSTO_ERR_ARG; }
                if (i == j && v < 0) { *err = w + "S0 has a negative diagonal entry" + where(i, j); return GUSTO_ERR_ARG; }
                if (j > i && memcmp(&S[i * nz + j], &S[j * nz + i], sizeof(double)) != 0) {
                    *err = w + "S0 must be symmetric to the bit" + where(i, j);
                    return GUSTO_ERR_ARG;
                }
            }
    }
    return GUSTO_OK;
}

// which of the GUSTO_NPLANT scalars (mass, Jdiag[0 .. 2], dubins_v, dubins_k) the f of the public model `model` reads
constexpr bool plant_entry_read(int model, int j) {
    return model == GUSTO_DUBINS_CAR ? j >= 4 : (model == GUSTO_FREEFLYER_SE2 ? (j == 0 || j == 3) : j < 4);
}

// their nominal values, from the handle's model parameters (device code: simulate.hip, lincov.hip)
struct PlantNominal {
    double v[GUSTO_NPLANT];
    GD explicit PlantNominal(const gusto_model_params& mp) : v{mp.mass, mp.Jdiag[0], mp.Jdiag[1], mp.Jdiag[2], mp.dubins_v, mp.dubins_k} {}
};

// The arguments of gusto_lincov_disturbed that gusto_lincov does not have: the dispersion d and the caller's Sth
// [B][GUSTO_NPLANT][GUSTO_NPLANT] (null: the default), of which only the entries the model reads are looked at.  GUSTO_ERR_ARG
// and the text, which names the offending entry (and problem), in *err.  No device, no handle.
static inline int lincov_plant_args_host(int model, int m, size_t B, const gusto_disturb_opts* d, const double* Sth, std::string* err,
                                         const char* who = "gusto_lincov_disturbed") {
    const std::string w = std::string(who) + ": ";
    constexpr size_t NT = GUSTO_NPLANT;
    for (size_t j = 0; j < NT; j++)
        if (!(d->plant_rel[j] >= 0 && d->plant_rel[j] < 1)) { *err = w + "plant_rel must lie in [0, 1) (entry " + std::to_string(j) + ")"; return GUSTO_ERR_ARG; }
    for (int i = 0; i < m; i++)
        if (!(d->dw[i] >= 0 && d->dw[i] < INFINITY)) { *err = w + "dw must be finite and >= 0 (entry " + std::to_string(i) + ")"; return GUSTO_ERR_ARG; }
    for (size_t b = 0; Sth && b < B; b++) {
        const double* S = Sth + b * NT * NT;
        const auto where = [&](size_t i, size_t j) {
            return " (problem " + std::to_string(b) + ", entry " + std::to_string(i) + ", " + std::to_string(j) + ")";
        };
        for (size_t i = 0; i < NT; i++)
            for (size_t j = 0; j < NT; j++) {
                if (!plant_entry_read(model, (int)i) || !plant_entry_read(model, (int)j)) continue;
                const double v = S[i * NT + j];
                if (!(fabs(v) < INFINITY)) { *err = w + "Sth must be finite" + where(i, j); return GUSTO_ERR_ARG; }
                if (i == j && v < 0) { *err = w + "Sth has a negative diagonal entry" + where(i, j); return GUSTO_ERR_ARG; }
                if (j > i && memcmp(&S[i * NT + j], &S[j * NT + i], sizeof(double)) != 0) {
                    *err = w + "Sth must be symmetric to the bit" + where(i, j);
                    return GUSTO_ERR_ARG;
                }
            }
    }
    return GUSTO_OK;
}

// The argument of gusto_lincov_dense that gusto_lincov_disturbed does not have (its others go through the two checks above,
// under this call's name).  No device, no handle.
static inline int lincov_dense_args_host(int store_dense, std::string* err) {
    if (store_dense != 0 && store_dense != 1) { *err = "gusto_lincov_dense: store_dense must be 0 or 1"; return GUSTO_ERR_ARG; }
    return GUSTO_OK;
}

// KParams of a kernel that reads trajectories: zeros but for the sizes, the model parameters and tf
static inline gusto::KParams post_params(gusto_handle h) {
    gusto::KParams P;
    memset(&P, 0, sizeof(P));
    P.N = h->N; P.B = h->B; P.mp = h->mp; P.tf = h->d_tf;
    return P;
}
// The trajectories a stage reads: the handle's, or copies of the caller's X, U in the stage's dX, dU (room for `slots`
// problems, grow-only: a constant `slots` allocates once); the handle's own stay as they are
static inline int stage_traj(gusto_handle h, const double* X, const double* U, size_t slots, DevBuf<double>& dX, DevBuf<double>& dU,
                             const double** Xd, const double** Ud) {
    *Xd = h->d_X; *Ud = h->d_U;
    if (!X) return GUSTO_OK;
    const size_t B = h->B, N = h->N, n = h->n, m = h->m;
    HIPCHK(h, dX.ensure(slots * N * n)); HIPCHK(h, dU.ensure(slots * N * m));
    HIPCHK(h, hipMemcpyAsync(dX, X, sizeof(double) * B * N * n, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(dU, U, sizeof(double) * B * N * m, hipMemcpyHostToDevice, h->stream));
    *Xd = dX; *Ud = dU;
    return GUSTO_OK;
}
// gusto_set_active: null = every problem, else the mask [B]
static inline const int* active_mask(gusto_handle h) { return h->n_active >= 0 ? h->d_active.get() : nullptr; }

// f(std::integral_constant<int, MODEL>{}), which answers a GUSTO_* code, for the public model id `model`
template <class F> static int for_model(int model, F&& f) {
    switch (model) {
    case GUSTO_FREEFLYER_SE2: return f(std::integral_constant<int, GUSTO_FREEFLYER_SE2>{});
    case GUSTO_DUBINS_CAR: return f(std::integral_constant<int, GUSTO_DUBINS_CAR>{});
    case GUSTO_ASTROBEE_SE3: return f(std::integral_constant<int, GUSTO_ASTROBEE_SE3>{});
    case GUSTO_ASTROBEE_SE3_MANIFOLD: return f(std::integral_constant<int, GUSTO_ASTROBEE_SE3_MANIFOLD>{});
    }
    return GUSTO_ERR_ARG;
}
// a getter's array: `count` elements to the caller's dst (null: not asked for)
template <class T> static int copy_out(gusto_handle h, T* dst, const std::common_type_t<T>* src, size_t count) {
    if (dst) HIPCHK(h, hipMemcpy(dst, src, sizeof(T) * count, hipMemcpyDeviceToHost));
    return GUSTO_OK;
}
