// tighten.hip -- risk-tightened keep-out sets: from the covariances of the last gusto_lincov (store_S = 1) and a caller's base
// keep-out tables, per-problem tables in which every component is extended over the robot's component offsets (so that clearing
// it with component 0, the only one the solver's obstacle rows look at, clears the original with every component) and grown by
// kappa standard deviations of that problem's own dispersion along the normal.  The tables go where gusto_set_env_batch puts its
// own: the next gusto_solve reads them, and no solve kernel changes.  No counterpart in the reference; include/gusto_hip.h states
// the definitions (pair, margin, cover, grow, report, skipped problems).
//   gusto_default_tighten_opts, gusto_tighten_env, gusto_get_tighten, gusto_get_env, gusto_last_tighten_ms
// One launch, one wave per problem (four problems per workgroup of 256, nothing shared between the waves: no LDS, no barrier),
// lane i = keep-out component i (at most 64: exactly one wave).  A lane holds its base component in registers and walks the
// knots and, inside, the robot components; the knot's position and its WS x WS covariance block are wave-uniform loads.  The
// distance is signed_distance<WS> (models.hpp) on registers: sdf_box and the sphere expression as they stand there.  sigma_of and
// margin_z are restated from lincov.hip (three lines each) so that file's code stays where it is.  A lane keeps its running
// largest margin and its smallest (z, knot, component) -- strict <, knots outermost: the lowest knot, then the lowest component, of
// equal minima.  At the end one wave_reduce each for the minimum, its lowest knot and the lowest ordinal there (gusto_lincov's
// tie rule), for the largest margin, the count of grown components and `blocked`; then the lane writes its own tightened
// component.  No atomics, nothing crosses a problem: a problem's outputs are the same bit for bit in any batch.
#include <hip/hip_runtime.h>

#include "models.hpp"
#include "post.hpp"

using namespace gusto;

namespace {

constexpr int TG_LANES = 64;       // components per problem, the row length of the margins
constexpr int TG_WAVES = 4;        // problems per workgroup
constexpr double TG_NONE = 4e9;    // (knots and ordinals stay far below)

struct TgArgs {
    const double *X, *Sxx;         // [B][N][n], [B][N][n][n]: what the last gusto_lincov saw and stored
    const int* lc_status;          // [B]: its status
    const int* active;             // gusto_set_active: null = every problem, else the mask [B]
    const double *bbox, *bsph;     // the base tables
    const int *rec_in, *rec_out;   // [B][4] box offset, n_box, sphere offset, n_sph: in the base tables, in the tightened ones
    const int* keep;               // [B]: the margins in M belong to this problem with these counts
    const double *x_init, *goal_lo, *goal_hi;   // [B][n]
    double kappa, slack, margin_cap, reach;
    int cover, monotone;
    double *obox, *osph;           // the tightened tables
    double* M;                     // [B][TG_LANES]
    int *status, *knot, *pair, *n_grown, *blocked;   // [B]
    double *min_z_base, *max_margin;                 // [B]
};

// (lincov.hip) the standard deviation of a variance: what rounding leaves below zero counts as zero (a NaN stays one)
GD double sigma_of(double var) { return sqrt(var < 0.0 ? 0.0 : var); }
// (lincov.hip) a margin in standard deviations; without any deviation the sign of the margin decides
GD double margin_z(double d, double sigma) {
    if (sigma == 0.0) return d >= 0.0 ? INFINITY : -INFINITY;
    return d / sigma;
}

// signed_distance<WS> (models.hpp) of the point q to a component held in registers: g = (min xyz, max xyz) or (centre xyz, radius)
template <int WS> GD double comp_distance(double radius, const double* q, bool is_box, const double* g, double* nh) {
    if (is_box) return sdf_box<WS>(q, g, g + 3, nh) - radius;
    double v[WS], s2 = 0;
#pragma unroll
    for (int j = 0; j < WS; j++) { v[j] = q[j] - g[j]; s2 += v[j] * v[j]; }
    const double nrm = sqrt(s2);
#pragma unroll
    for (int j = 0; j < WS; j++) nh[j] = v[j] / nrm;
    return nrm - g[3] - radius;
}

template <int MODEL> __global__ void __launch_bounds__(TG_WAVES * 64) tighten_kernel(const KParams P, const TgArgs V) {
    using T = MT<MODEL>;
    constexpr int n = T::n, WS = T::WS, NPF = n * n;
    const int lane = threadIdx.x & 63, b = blockIdx.x * TG_WAVES + (threadIdx.x >> 6), N = P.N;
    if (b >= P.B) return;   // (the whole wave; the waves of a workgroup share nothing)
    const int* ri = V.rec_in + 4 * (size_t)b;
    const int* ro = V.rec_out + 4 * (size_t)b;
    const int nb = ri[1], n_obs = nb + ri[3], ncomp = P.mp.n_robot_comp;
    const bool have = lane < n_obs, is_box = lane < nb;
    const bool skip = (V.active && !V.active[b]) || !V.lc_status[b];   // (wave-uniform)

    // the lane's base component
    double g[6] = {0, 0, 0, 0, 0, 0};
    if (have) {
        if (is_box) {
            const double* s = V.bbox + 6 * ((size_t)ri[0] + lane);
#pragma unroll
            for (int j = 0; j < 6; j++) g[j] = s[j];
        } else {
            const double* s = V.bsph + 4 * ((size_t)ri[2] + (lane - nb));
#pragma unroll
            for (int j = 0; j < 4; j++) g[j] = s[j];
        }
    }
    const double prev = (have && V.keep[b]) ? V.M[(size_t)b * TG_LANES + lane] : 0.0;

    double mrun = 0.0, zb = INFINITY;
    int kb = 0, cb = 0;
    if (!skip) {
        const double* Xb = V.X + (size_t)b * N * n;
        const double* Sb = V.Sxx + (size_t)b * N * NPF;
        for (int k = 0; k < N; k++) {
            double x[WS], S[WS][WS];
#pragma unroll
            for (int j = 0; j < WS; j++) x[j] = Xb[(size_t)k * n + j];
#pragma unroll
            for (int a = 0; a < WS; a++)
#pragma unroll
                for (int j = 0; j < WS; j++) S[a][j] = Sb[(size_t)k * NPF + a * n + j];
            for (int c = 0; c < ncomp; c++) {
                if (!have) continue;
                double q[WS], nh[WS];
#pragma unroll
                for (int j = 0; j < WS; j++) q[j] = x[j] + P.mp.comp_off[c][j];
                const double d = comp_distance<WS>(P.mp.radius, q, is_box, g, nh);
                double var = 0.0;
#pragma unroll
                for (int a = 0; a < WS; a++) {
                    double s = 0.0;
#pragma unroll
                    for (int j = 0; j < WS; j++) s += S[a][j] * nh[j];
                    var += nh[a] * s;
                }
                const double sd = sigma_of(var);
                const double z = margin_z(d, sd);
                if (z < zb) { zb = z; kb = k + 1; cb = c; }   // (strict: the lowest knot, then component; a NaN never wins)
                const double ks = V.kappa * sd;
                if (d - ks <= V.reach) {
                    double v = ks - V.slack;
                    v = v > 0.0 ? v : 0.0;
                    if (v > mrun) mrun = v;                   // (a NaN never wins)
                }
            }
        }
    }
    double m = mrun < V.margin_cap ? mrun : V.margin_cap;
    if (V.monotone && prev > m) m = prev;
    if (skip) m = prev;
    if (!have) m = 0.0;
    V.M[(size_t)b * TG_LANES + lane] = m;   // (zeros behind the problem's own count)

    // the tightened component: cover over the component offsets (relative to component 0), then grow
    double omax[WS], omin[WS];
#pragma unroll
    for (int j = 0; j < WS; j++) { omax[j] = 0.0; omin[j] = 0.0; }
    if (V.cover)
        for (int c = 1; c < ncomp; c++)
#pragma unroll
            for (int j = 0; j < WS; j++) {
                const double o = P.mp.comp_off[c][j] - P.mp.comp_off[0][j];
                omax[j] = o > omax[j] ? o : omax[j];
                omin[j] = o < omin[j] ? o : omin[j];
            }
    double t[6];
#pragma unroll
    for (int j = 0; j < 6; j++) t[j] = g[j];
    if (is_box) {
#pragma unroll
        for (int j = 0; j < WS; j++) { t[j] = (g[j] - omax[j]) - m; t[3 + j] = (g[3 + j] - omin[j]) + m; }
    } else {
        double h2 = 0.0;
#pragma unroll
        for (int j = 0; j < WS; j++) {
            const double hj = 0.5 * (omax[j] - omin[j]);
            h2 += hj * hj;
            t[j] = g[j] - 0.5 * (omax[j] + omin[j]);
        }
        t[3] = (g[3] + sqrt(h2)) + m;
    }
    if (have) {
        if (is_box) {
            double* o = V.obox + 6 * ((size_t)ro[0] + lane);
#pragma unroll
            for (int j = 0; j < 6; j++) o[j] = t[j];
        } else {
            double* o = V.osph + 4 * ((size_t)ro[2] + (lane - nb));
#pragma unroll
            for (int j = 0; j < 4; j++) o[j] = t[j];
        }
    }

    // blocked: x_init, or the goal centre where its workspace entries are finite, inside the problem's own tightened set
    bool inside = false;
    if (have) {
        double q[WS], nh[WS];
        bool gfin = true;
#pragma unroll
        for (int j = 0; j < WS; j++) q[j] = V.x_init[(size_t)b * n + j] + P.mp.comp_off[0][j];
        inside = comp_distance<WS>(P.mp.radius, q, is_box, t, nh) < 0.0;
#pragma unroll
        for (int j = 0; j < WS; j++) {
            const double lo = V.goal_lo[(size_t)b * n + j], hi = V.goal_hi[(size_t)b * n + j];
            gfin = gfin && isfinite(lo) && isfinite(hi);
            q[j] = 0.5 * (lo + hi) + P.mp.comp_off[0][j];
        }
        if (gfin) inside = inside || comp_distance<WS>(P.mp.radius, q, is_box, t, nh) < 0.0;
    }

    // the report: gusto_lincov's tie rule -- the lowest knot of equal minima, then the lowest ordinal component n_obs + obstacle
    const bool cand = have && kb > 0;
    const double zmin = wave_reduce(cand ? zb : INFINITY, OpMin());
    const double kmin = wave_reduce((cand && zb == zmin) ? (double)kb : TG_NONE, OpMin());
    const double omin_ord = wave_reduce((cand && zb == zmin && (double)kb == kmin) ? (double)(cb * n_obs + lane) : TG_NONE, OpMin());
    const double mmax = wave_reduce(m, OpMax());
    const double ngrown = wave_reduce(m > 0.0 ? 1.0 : 0.0, OpSum());   // (integers: exact in any order)
    const double blk = wave_reduce(inside ? 1.0 : 0.0, OpMax());
    if (lane == 0) {
        const bool none = kmin == TG_NONE;   // nothing below +inf
        V.status[b] = skip ? 0 : 1;
        V.min_z_base[b] = skip ? 0.0 : zmin;
        V.knot[b] = (skip || none) ? 0 : (int)kmin;
        V.pair[b] = skip ? 0 : (none ? -1 : (int)omin_ord);
        V.max_margin[b] = mmax;
        V.n_grown[b] = (int)ngrown;
        V.blocked[b] = (int)blk;
    }
}

}  // namespace

extern "C" {

int gusto_default_tighten_opts(int model_id, gusto_tighten_opts* o) {
    if (!o || !model_info(model_id)) return GUSTO_ERR_ARG;
    memset(o, 0, sizeof(*o));
    o->kappa = 3.0; o->slack = 0.0; o->margin_cap = INFINITY; o->reach = INFINITY;
    o->cover_components = 1; o->monotone = 1;
    return GUSTO_OK;
}

int gusto_tighten_env(gusto_handle h, int n_env, const int* n_box, const double* box, const int* n_sph, const double* sph,
                      const gusto_tighten_opts* opts) {
    const char* who = "gusto_tighten_env";
    if (int rc = post_enter(h, who, nullptr, nullptr)) return rc;
    if (!model_info(h->model)->has_obs) return refuse(h, who, "the model has no keep-out sets");
    gusto_tighten_opts o;
    gusto_default_tighten_opts(h->model, &o);
    if (opts) o = *opts;
    if (!(o.kappa >= 0 && o.kappa < INFINITY)) return refuse(h, who, "kappa must be finite and >= 0");
    if (!(o.slack >= 0 && o.slack < INFINITY)) return refuse(h, who, "slack must be finite and >= 0");
    if (!(o.margin_cap >= 0)) return refuse(h, who, "margin_cap must be >= 0 (it may be +inf)");
    if (o.reach != o.reach) return refuse(h, who, "reach is a NaN");
    if ((o.cover_components != 0 && o.cover_components != 1) || (o.monotone != 0 && o.monotone != 1))
        return refuse(h, who, "cover_components and monotone must be 0 or 1");
    const size_t B = h->B, Bc = h->batch_cap;
    if (n_env != 1 && n_env != (int)B) return refuse(h, who, "n_env must be 1 or the B of gusto_set_problems");
    if (!n_box || !n_sph) return refuse(h, who, "a null n_box or n_sph");
    size_t tb = 0, ts = 0;
    for (int e = 0; e < n_env; e++) {
        if (n_box[e] < 0 || n_sph[e] < 0 || n_box[e] + n_sph[e] > TG_LANES)
            return refuse(h, who, "between 0 and 64 keep-out components per problem (set " + std::to_string(e) + ")");
        tb += n_box[e]; ts += n_sph[e];
    }
    if ((tb && !box) || (ts && !sph)) return refuse(h, who, "a null table");
    for (size_t i = 0; i < 6 * tb; i++)
        if (!(fabs(box[i]) < INFINITY)) return refuse(h, who, "box_min_max must be finite (box " + std::to_string(i / 6) + ")");
    for (size_t i = 0; i < 4 * ts; i++)
        if (!(fabs(sph[i]) < INFINITY)) return refuse(h, who, "sph_c_r must be finite (sphere " + std::to_string(i / 4) + ")");
    const LincovState& L = h->lincov;
    if (!L.have || !L.store_S || !L.have_Sxx)
        return refuse(h, who, "no covariances: call gusto_lincov with store_S = 1 first", GUSTO_ERR_STATE);

    // the records of every problem in the base tables and in the tightened ones, and whether its remembered margins hold
    TightenState& S = h->tighten;
    std::vector<int> rec(9 * Bc, 0), cnt(2 * B);
    int *rin = rec.data(), *rout = rec.data() + 4 * Bc, *keep = rec.data() + 8 * Bc;
    size_t ob = 0, os = 0, ib = 0, is = 0;
    int mx = 0;
    for (size_t b = 0; b < B; b++) {
        const int e = n_env == 1 ? 0 : (int)b;
        if (n_env != 1 && b) { ib += n_box[b - 1]; is += n_sph[b - 1]; }
        rin[4 * b] = (int)ib; rin[4 * b + 1] = n_box[e]; rin[4 * b + 2] = (int)is; rin[4 * b + 3] = n_sph[e];
        rout[4 * b] = (int)ob; rout[4 * b + 1] = n_box[e]; rout[4 * b + 2] = (int)os; rout[4 * b + 3] = n_sph[e];
        ob += n_box[e]; os += n_sph[e];
        mx = std::max(mx, n_box[e] + n_sph[e]);
        cnt[2 * b] = n_box[e]; cnt[2 * b + 1] = n_sph[e];
        keep[b] = S.mem && S.mem_B == (int)B && S.cnt[2 * b] == n_box[e] && S.cnt[2 * b + 1] == n_sph[e];
    }
    if (ob > (size_t)INT_MAX / 8 || os > (size_t)INT_MAX / 8) return refuse(h, who, "tables too large");

    // the tightened tables are built beside the handle's and take their place once the launch is through
    DevBuf<double> nbox, nsph;
    DevBuf<int> nenv;
    HIPCHK(h, nbox.alloc(6 * ob)); HIPCHK(h, nsph.alloc(4 * os)); HIPCHK(h, nenv.alloc(4 * B));
    HIPCHK(h, S.Bbox.ensure(6 * tb)); HIPCHK(h, S.Bsph.ensure(4 * ts)); HIPCHK(h, S.Rec.ensure(9 * Bc));
    HIPCHK(h, S.M.ensure_zeroed(Bc * TG_LANES, h->stream));
    HIPCHK(h, S.I.ensure_zeroed(5 * Bc, h->stream)); HIPCHK(h, S.D.ensure_zeroed(2 * Bc, h->stream));
    HIPCHK(h, S.t0.record(h->stream));
    if (tb) HIPCHK(h, hipMemcpyAsync(S.Bbox, box, sizeof(double) * 6 * tb, hipMemcpyHostToDevice, h->stream));
    if (ts) HIPCHK(h, hipMemcpyAsync(S.Bsph, sph, sizeof(double) * 4 * ts, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(S.Rec, rec.data(), sizeof(int) * rec.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(nenv, S.Rec.get() + 4 * Bc, sizeof(int) * 4 * B, hipMemcpyDeviceToDevice, h->stream));
    KParams P = post_params(h);
    TgArgs V{};
    V.X = L.staged ? L.X.get() : h->d_X.get();
    V.Sxx = L.Sxx; V.lc_status = L.I; V.active = active_mask(h);
    V.bbox = S.Bbox; V.bsph = S.Bsph; V.rec_in = S.Rec; V.rec_out = S.Rec.get() + 4 * Bc; V.keep = S.Rec.get() + 8 * Bc;
    V.x_init = h->d_xinit; V.goal_lo = h->d_glo; V.goal_hi = h->d_ghi;
    V.kappa = o.kappa; V.slack = o.slack; V.margin_cap = o.margin_cap; V.reach = o.reach;
    V.cover = o.cover_components; V.monotone = o.monotone;
    V.obox = nbox; V.osph = nsph; V.M = S.M;
    V.status = S.I; V.knot = S.I + Bc; V.pair = S.I + 2 * Bc; V.n_grown = S.I + 3 * Bc; V.blocked = S.I + 4 * Bc;
    V.min_z_base = S.D; V.max_margin = S.D + Bc;
    if (int rc = for_model(h->model, [&](auto M) -> int {
            if constexpr (MT<decltype(M)::value>::HAS_OBS) {
                hipLaunchKernelGGL(tighten_kernel<decltype(M)::value>, dim3((unsigned)((B + TG_WAVES - 1) / TG_WAVES)), dim3(TG_WAVES * 64), 0,
                                   h->stream, P, V);
                HIPCHK(h, hipGetLastError());
            }
            return GUSTO_OK;
        }))
        return rc;
    HIPCHK(h, S.t1.record(h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, event_ms(S.t0, S.t1, &S.last_ms));
    h->d_box = std::move(nbox); h->d_sph = std::move(nsph); h->d_env = std::move(nenv);
    h->env_B = (int)B; h->n_obs_max = mx; h->n_box = 0; h->n_sph = 0;
    S.cnt = std::move(cnt); S.mem_B = (int)B; S.mem = true; S.n_obs_max = mx; S.have = true;
    return GUSTO_OK;
}

int gusto_get_tighten(gusto_handle h, gusto_tighten_report* out, int* n_obs_max) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    const TightenState& S = h->tighten;
    if (!S.have) { h->err = "gusto_get_tighten: call gusto_tighten_env first"; return GUSTO_ERR_STATE; }
    if (n_obs_max) *n_obs_max = S.n_obs_max;
    if (!out) return GUSTO_OK;
    const size_t B = h->B, Bc = h->batch_cap, w = S.n_obs_max;
    if (int rc = copy_out(h, out->status, S.I, B)) return rc;
    if (int rc = copy_out(h, out->knot, S.I + Bc, B)) return rc;
    if (int rc = copy_out(h, out->pair, S.I + 2 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->n_grown, S.I + 3 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->blocked, S.I + 4 * Bc, B)) return rc;
    if (int rc = copy_out(h, out->min_z_base, S.D, B)) return rc;
    if (int rc = copy_out(h, out->max_margin, S.D + Bc, B)) return rc;
    if (out->margin && w)   // the first n_obs_max entries of every row of M
        HIPCHK(h, hipMemcpy2D(out->margin, sizeof(double) * w, S.M, sizeof(double) * TG_LANES, sizeof(double) * w, B, hipMemcpyDeviceToHost));
    return GUSTO_OK;
}

int gusto_get_env(gusto_handle h, int* n_env, int* n_box, double* box, int* n_sph, double* sph) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    size_t tb = h->n_box, ts = h->n_sph;
    if (!h->d_env) {
        if (n_env) *n_env = 1;
        if (n_box) n_box[0] = h->n_box;
        if (n_sph) n_sph[0] = h->n_sph;
    } else {
        const size_t E = h->env_B;
        std::vector<int> rec(4 * E);
        HIPCHK(h, hipMemcpy(rec.data(), h->d_env, sizeof(int) * rec.size(), hipMemcpyDeviceToHost));
        tb = ts = 0;
        for (size_t e = 0; e < E; e++) {
            if (n_box) n_box[e] = rec[4 * e + 1];
            if (n_sph) n_sph[e] = rec[4 * e + 3];
            tb += rec[4 * e + 1]; ts += rec[4 * e + 3];
        }
        if (n_env) *n_env = (int)E;
    }
    if (int rc = copy_out(h, tb ? box : nullptr, h->d_box, 6 * tb)) return rc;
    return copy_out(h, ts ? sph : nullptr, h->d_sph, 4 * ts);
}

int gusto_last_tighten_ms(gusto_handle h, double* ms) {
    if (!h || !ms) return GUSTO_ERR_ARG;
    if (!h->tighten.have) { h->err = "gusto_last_tighten_ms: call gusto_tighten_env first"; return GUSTO_ERR_STATE; }
    *ms = h->tighten.last_ms;
    return GUSTO_OK;
}

}  // extern "C"
