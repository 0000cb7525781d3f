// trajlib.hip -- the trajectory library: solved trajectories kept on the device, and every query of a batch seeded from its K
// nearest entries.  No counterpart in the reference, whose GuSTO loop is warm-started at its own previous iterate
// (scp_gusto.jl:100-102); the definitions are stated in include/gusto_hip.h.
//   gusto_trajlib_create / _destroy / _size / _clear / _add / _add_host / _get   the library
//   gusto_set_problems_trajlib     Bq queries x K neighbours become the B = Bq K problems of the handle, problem q K + j seeded
//                                  from neighbour j of query q (the layout of gusto_set_problems_multistart)
//   gusto_get_trajlib_seeds, gusto_last_trajlib_ms, gusto_dev_trajlib
// Search kernel: the shape of select_kernel (multistart.hip) taken further, a wavefront per query, four queries per workgroup.
// Lane l visits the entries l, l + 64, ... in ascending order and keeps its K best in registers, sorted by (d2, e): a strict
// `<` on d2 keeps the earlier entry of a tie in front.  The K smallest of the whole library are among the lanes' lists, so K
// rounds of the two-reduction argmin idiom (the smallest head d2, then the lowest entry among the lanes whose head holds it) pop
// them in ascending (d2, e); the winning lane drops its head.  d2 of a pair is one lane's sum in the order of the definition,
// whatever batch the query sits in.  No atomics.
// The feature rows are feature-major ([F][cap]), so the 64 lanes of a load read 512 consecutive bytes.  With lds_tile the four
// wavefronts of a workgroup stage a tile of TL_TILE entries in LDS ([F][TL_TILE], lane-consecutive: no bank conflicts) and all
// read it there: a quarter of the L2 reads; without, every wavefront reads the rows from global memory.  The arithmetic is the
// same function of the same numbers.  Measured: profiles/trajlib.txt.
// Retarget kernel: a thread per (problem, knot), the shape of fan_kernel.  A start without a neighbour evaluates straight_line()
// of seed.hpp, as init_straightline_kernel (scp.hpp) does: that kernel's output bit for bit.
// Compaction kernel (gusto_trajlib_add): a wavefront per problem.  Its lanes count the selected problems before it (integers: any
// order gives the same sum), which is its row behind the library's count; a selected problem's wavefront then copies its
// trajectory lane-consecutively and writes centre and features.
#include <hip/hip_runtime.h>

#include "seed.hpp"

using namespace gusto;

namespace {

constexpr int TL_WAVES = 4, TL_TILE = 256;   // queries per workgroup of the search; entries per LDS tile

struct FeatMap {
    int F;
    int fmap[TRAJLIB_MAX_F];
    double w[TRAJLIB_MAX_F];
};

struct SearchArgs {
    QueryDev Q;                          // the queries; extra: tf [Bq]
    const int* qtag;                     // [Bq], null: tags ignored
    const double* feat;                  // [F][cap]
    const int* etag;                     // [cap]
    size_t cap;
    int L, Bq, n;
    FeatMap M;
    int* entry; double* dist2; int* n_found;   // [Bq][K], [Bq][K], [Bq]
};

template <int K, bool TILED> __global__ void __launch_bounds__(64 * TL_WAVES) search_kernel(const SearchArgs A) {
    extern __shared__ double sm[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, F = A.M.F;
    const int q = blockIdx.x * TL_WAVES + wave;
    const bool valid = q < A.Bq;   // (a wavefront behind the last query takes part in the tile loads and barriers only)
    double* qf = sm + wave * TRAJLIB_MAX_F;
    double* tile = sm + TL_WAVES * TRAJLIB_MAX_F;
    if (valid && lane < F) {
        const int kind = A.M.fmap[lane] >> 4, i = A.M.fmap[lane] & 15;
        const size_t at = (size_t)q * A.n + i;
        qf[lane] = kind == 0 ? A.Q.xi[at] : (kind == 1 ? goal_centre(A.Q.glo[at], A.Q.ghi[at]) : A.Q.extra[q]);
    }
    const int tq = (valid && A.qtag) ? A.qtag[q] : 0;
    double bd[K];
    int be[K];
#pragma unroll
    for (int j = 0; j < K; j++) { bd[j] = INFINITY; be[j] = -1; }   // (be < 0: an empty slot; they stay behind the filled ones)
    __syncthreads();
    for (int t0 = 0; t0 < A.L; t0 += TL_TILE) {
        if constexpr (TILED) {
            for (int idx = threadIdx.x; idx < F * TL_TILE; idx += 64 * TL_WAVES) {
                const int f = idx / TL_TILE, e = t0 + idx % TL_TILE;
                tile[idx] = e < A.L ? A.feat[(size_t)f * A.cap + e] : 0.0;
            }
            __syncthreads();
        }
        for (int r = lane; r < TL_TILE; r += 64) {
            const int e = t0 + r;
            if (valid && e < A.L && (!A.qtag || A.etag[e] == tq)) {
                double d = 0.0;
                for (int f = 0; f < F; f++) {
                    const double x = TILED ? tile[f * TL_TILE + r] : A.feat[(size_t)f * A.cap + e];
                    const double t = qf[f] - x;
                    d += A.M.w[f] * (t * t);
                }
                if (!isnan(d) && (be[K - 1] < 0 || d < bd[K - 1])) {
                    bd[K - 1] = d; be[K - 1] = e;
#pragma unroll
                    for (int j = K - 1; j > 0; j--) {
                        if (be[j - 1] < 0 || bd[j] < bd[j - 1]) {
                            const double td = bd[j]; bd[j] = bd[j - 1]; bd[j - 1] = td;
                            const int te = be[j]; be[j] = be[j - 1]; be[j - 1] = te;
                        }
                    }
                }
            }
        }
        if constexpr (TILED) __syncthreads();
    }
    int nf = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
        const bool cand = be[0] >= 0;
        const double dmin = wave_reduce(cand ? bd[0] : INFINITY, OpMin());
        const double ew = wave_reduce((cand && bd[0] == dmin) ? (double)be[0] : 4e9, OpMin());   // ties: the lowest entry
        const bool found = ew < 4e9;
        if (valid && lane == 0) {
            A.entry[(size_t)q * K + j] = found ? (int)ew : -1;
            A.dist2[(size_t)q * K + j] = found ? dmin : INFINITY;
        }
        nf += found ? 1 : 0;
        if (cand && (double)be[0] == ew) {   // the winning lane drops its head
#pragma unroll
            for (int i = 0; i + 1 < K; i++) { bd[i] = bd[i + 1]; be[i] = be[i + 1]; }
            bd[K - 1] = INFINITY; be[K - 1] = -1;
        }
    }
    if (valid && lane == 0) A.n_found[q] = nf;
}

struct RetargetArgs {
    QueryDev Q;                         // the queries; extra: tf [Bq]
    const int* entry;                   // [B]
    const double *lxi, *lc, *lX, *lU;   // the library's rows
    SeedOut out;
    int B, K, N;
};

template <int MODEL> __global__ void retarget_kernel(const RetargetArgs A) {
    using T = MT<MODEL>;
    constexpr int n = T::n, m = T::m;
    KnotId id;
    if (!knot_id(A.B, A.K, A.N, id)) return;
    const int b = id.b, k = id.k;
    const double t = id.t;
    const double *xi = A.Q.xi + (size_t)id.q * n, *glo = A.Q.glo + (size_t)id.q * n, *ghi = A.Q.ghi + (size_t)id.q * n;   // the query's rows
    const int e = A.entry[b];
    double* Xo = A.out.X + ((size_t)b * A.N + k) * n;
    double* Uo = A.out.U + ((size_t)b * A.N + k) * m;
    if (e < 0) {
#pragma unroll
        for (int i = 0; i < n; i++) Xo[i] = straight_line(t, xi[i], glo[i], ghi[i]);
#pragma unroll
        for (int i = 0; i < m; i++) Uo[i] = 0.0;
    } else {
        const double* Xe = A.lX + ((size_t)e * A.N + k) * n;
        const double* Ue = A.lU + ((size_t)e * A.N + k) * m;
#pragma unroll
        for (int i = 0; i < n; i++) {
            const double xq = xi[i];
            const double cq = goal_centre(glo[i], ghi[i]);
            const double dxi = xq - A.lxi[(size_t)e * n + i], dc = cq - A.lc[(size_t)e * n + i];
            Xo[i] = k == 0 ? xq : Xe[i] + ((1 - t) * dxi + t * dc);
        }
#pragma unroll
        for (int i = 0; i < m; i++) Uo[i] = Ue[i];
    }
    if (k == 0) seed_problem_tail<MODEL>(A.out, b, xi, glo, ghi, A.Q.extra[id.q]);
}

struct CompactArgs {
    const int *mask, *tag;                                // [B] each
    const double *X, *U, *x_init, *goal_lo, *goal_hi, *tf;   // the handle's arrays
    int B, n, nx, nu, base;                               // nx = N n, nu = N m; base: the library's count
    size_t cap;
    FeatMap M;
    double *lxi, *lc, *ltf, *lX, *lU, *feat;
    int* ltag;
};

__global__ void __launch_bounds__(64) compact_kernel(const CompactArgs A) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int cnt = 0;
    for (int i = lane; i < b; i += 64) cnt += A.mask[i] != 0;
    const size_t e = (size_t)A.base + (size_t)wave_reduce((double)cnt, OpSum());   // (integers below 2^53: exact in any order)
    if (A.mask[b] == 0) return;
    for (int i = lane; i < A.nx; i += 64) A.lX[e * A.nx + i] = A.X[(size_t)b * A.nx + i];
    for (int i = lane; i < A.nu; i += 64) A.lU[e * A.nu + i] = A.U[(size_t)b * A.nu + i];
    if (lane < A.n) {
        const size_t at = (size_t)b * A.n + lane;
        A.lxi[e * A.n + lane] = A.x_init[at];
        A.lc[e * A.n + lane] = goal_centre(A.goal_lo[at], A.goal_hi[at]);
    }
    if (lane < A.M.F) {
        const int kind = A.M.fmap[lane] >> 4, i = A.M.fmap[lane] & 15;
        const size_t at = (size_t)b * A.n + i;
        A.feat[(size_t)lane * A.cap + e] = kind == 0 ? A.x_init[at] : (kind == 1 ? goal_centre(A.goal_lo[at], A.goal_hi[at]) : A.tf[b]);
    }
    if (lane == 0) { A.ltf[e] = A.tf[b]; A.ltag[e] = A.tag[b]; }
}

thread_local std::string g_lib_err;   // a failed gusto_trajlib_create

int lib_refuse(gusto_trajlib lib, const char* who, const std::string& what) {
    lib->err = std::string(who) + ": " + what;
    return GUSTO_ERR_ARG;
}

#define LIBCHK(lib, call)                                                              \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            (lib)->err = std::string(#call) + ": " + hipGetErrorString(e_);            \
            return GUSTO_ERR_HIP;                                                      \
        }                                                                              \
    } while (0)

FeatMap feat_map(const gusto_trajlib_s* lib) {
    FeatMap M;
    M.F = lib->F;
    memcpy(M.fmap, lib->fmap, sizeof(M.fmap));
    memcpy(M.w, lib->w, sizeof(M.w));
    return M;
}

bool all_finite(const double* a, size_t count) {
    for (size_t i = 0; i < count; i++)
        if (!(fabs(a[i]) < INFINITY)) return false;
    return true;
}

template <int K> void launch_search(const SearchArgs& A, bool tiled, hipStream_t s) {
    const dim3 grid((A.Bq + TL_WAVES - 1) / TL_WAVES), block(64 * TL_WAVES);
    const size_t qf = sizeof(double) * TL_WAVES * TRAJLIB_MAX_F;
    if (tiled) hipLaunchKernelGGL((search_kernel<K, true>), grid, block, qf + sizeof(double) * A.M.F * TL_TILE, s, A);
    else hipLaunchKernelGGL((search_kernel<K, false>), grid, block, qf, s, A);
}

}  // namespace

extern "C" {

int gusto_default_trajlib_opts(int model, gusto_trajlib_opts* o) {
    const ModelInfo* mi = model_info(model);
    if (!mi || !o) return GUSTO_ERR_ARG;
    memset(o, 0, sizeof(*o));
    for (int i = 0; i < mi->n; i++) o->w_init[i] = o->w_goal[i] = 1.0;
    o->lds_tile = 1;
    return GUSTO_OK;
}

int gusto_trajlib_create(gusto_trajlib* out, int model, int N, int cap, int device, const gusto_trajlib_opts* opts) {
    const ModelInfo* mi = model_info(model);
    if (!out || !mi || N < 3 || N > 256 || cap < 1 || cap > GUSTO_TRAJLIB_MAX_CAP) {
        g_lib_err = "gusto_trajlib_create: bad argument (need a known model, 3 <= N <= 256, 1 <= cap <= GUSTO_TRAJLIB_MAX_CAP)";
        return GUSTO_ERR_ARG;
    }
    gusto_trajlib_opts o;
    gusto_default_trajlib_opts(model, &o);
    if (opts) o = *opts;
    const auto weight_ok = [](double v) { return v >= 0 && v < INFINITY; };
    bool ok = weight_ok(o.w_tf) && (o.lds_tile == 0 || o.lds_tile == 1);
    for (int i = 0; i < mi->n; i++) ok = ok && weight_ok(o.w_init[i]) && weight_ok(o.w_goal[i]);
    if (!ok) {
        g_lib_err = "gusto_trajlib_create: the weights must be finite and >= 0, lds_tile 0 or 1";
        return GUSTO_ERR_ARG;
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        g_lib_err = "gusto_trajlib_create: no usable HIP device (libgusto_hip has no CPU fallback)";
        return GUSTO_ERR_NO_DEVICE;
    }
    gusto_trajlib lib = new gusto_trajlib_s();
    lib->model = model; lib->n = mi->n; lib->m = mi->m; lib->N = N; lib->cap = cap; lib->device = device; lib->lds_tile = o.lds_tile;
    for (int kind = 0; kind < 2; kind++)
        for (int i = 0; i < mi->n; i++) {
            const double w = kind == 0 ? o.w_init[i] : o.w_goal[i];
            if (w > 0) { lib->fmap[lib->F] = kind * 16 + i; lib->w[lib->F++] = w; }
        }
    if (o.w_tf > 0) { lib->fmap[lib->F] = 2 * 16; lib->w[lib->F++] = o.w_tf; }
    const size_t c = cap, n = mi->n, m = mi->m;
    hipError_t e = hipSetDevice(device);
    if (e == hipSuccess) e = lib->xi.alloc(c * n);
    if (e == hipSuccess) e = lib->c.alloc(c * n);
    if (e == hipSuccess) e = lib->tf.alloc(c);
    if (e == hipSuccess) e = lib->tag.alloc(c);
    if (e == hipSuccess) e = lib->X.alloc(c * N * n);
    if (e == hipSuccess) e = lib->U.alloc(c * N * m);
    if (e == hipSuccess) e = lib->Feat.alloc(c * lib->F);
    if (e != hipSuccess) {
        g_lib_err = std::string("gusto_trajlib_create: ") + hipGetErrorString(e);
        delete lib;
        return GUSTO_ERR_HIP;
    }
    *out = lib;
    return GUSTO_OK;
}

int gusto_trajlib_destroy(gusto_trajlib lib) {
    if (!lib) return GUSTO_ERR_ARG;
    hipSetDevice(lib->device);
    delete lib;
    return GUSTO_OK;
}

const char* gusto_trajlib_last_error(gusto_trajlib lib) { return lib ? lib->err.c_str() : g_lib_err.c_str(); }

int gusto_trajlib_size(gusto_trajlib lib, int* count, int* cap) {
    if (!lib) return GUSTO_ERR_ARG;
    if (count) *count = lib->count;
    if (cap) *cap = lib->cap;
    return GUSTO_OK;
}

int gusto_trajlib_clear(gusto_trajlib lib) {
    if (!lib) return GUSTO_ERR_ARG;
    lib->count = 0;
    return GUSTO_OK;
}

int gusto_trajlib_add(gusto_trajlib lib, gusto_handle h, const int* mask, const int* tag, int* n_added) {
    const char* who = "gusto_trajlib_add";
    if (n_added) *n_added = 0;
    if (!lib) return GUSTO_ERR_ARG;
    if (!h) return lib_refuse(lib, who, "a null handle");
    if (h->trajopt) return lib_refuse(lib, who, "TrajOpt handle (not supported)");
    if (h->model_pub != lib->model || h->N != lib->N || h->device != lib->device)
        return lib_refuse(lib, who, "the handle's model, N or device differ from the library's");
    if (int rc = getter_enter(h, true)) {
        lib->err = std::string(who) + ": " + (rc == GUSTO_ERR_STATE && h->err.empty() ? "the handle has no problems" : h->err);
        return rc;
    }
    const size_t B = h->B;
    std::vector<int> mt(2 * B, 0);   // mask | tag: one copy
    if (mask) {
        for (size_t b = 0; b < B; b++) mt[b] = mask[b] != 0;
    } else {
        std::vector<int> st(B * ST_NI);
        LIBCHK(lib, hipMemcpy(st.data(), h->d_sti, sizeof(int) * st.size(), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; b++) mt[b] = st[b * ST_NI + ST_CONV] != 0 && st[b * ST_NI + ST_SUCC] != 0;
    }
    if (tag) memcpy(mt.data() + B, tag, sizeof(int) * B);
    size_t sel = 0;
    for (size_t b = 0; b < B; b++) sel += mt[b];
    if (sel > (size_t)(lib->cap - lib->count))
        return lib_refuse(lib, who, "the selection (" + std::to_string(sel) + " problems) does not fit the remaining capacity (" +
                                        std::to_string(lib->cap - lib->count) + ")");
    if (sel == 0) return GUSTO_OK;
    TrajlibState& S = h->trajlib;
    LIBCHK(lib, S.Mask.ensure(2 * B));
    LIBCHK(lib, hipMemcpyAsync(S.Mask, mt.data(), sizeof(int) * 2 * B, hipMemcpyHostToDevice, h->stream));
    CompactArgs A;
    A.mask = S.Mask; A.tag = S.Mask + B;
    A.X = h->d_X; A.U = h->d_U; A.x_init = h->d_xinit; A.goal_lo = h->d_glo; A.goal_hi = h->d_ghi; A.tf = h->d_tf;
    A.B = (int)B; A.n = lib->n; A.nx = lib->N * lib->n; A.nu = lib->N * lib->m; A.base = lib->count; A.cap = lib->cap;
    A.M = feat_map(lib);
    A.lxi = lib->xi; A.lc = lib->c; A.ltf = lib->tf; A.lX = lib->X; A.lU = lib->U; A.feat = lib->Feat; A.ltag = lib->tag;
    hipLaunchKernelGGL(compact_kernel, dim3((unsigned)B), dim3(64), 0, h->stream, A);
    LIBCHK(lib, hipGetLastError());
    LIBCHK(lib, hipStreamSynchronize(h->stream));   // (`mt` is read by then)
    lib->count += (int)sel;
    if (n_added) *n_added = (int)sel;
    return GUSTO_OK;
}

int gusto_trajlib_add_host(gusto_trajlib lib, int cnt, const double* x_init, const double* glo, const double* ghi, const double* tf,
                           const int* tag, const double* X, const double* U) {
    const char* who = "gusto_trajlib_add_host";
    if (!lib) return GUSTO_ERR_ARG;
    if (cnt < 0 || cnt > lib->cap - lib->count) return lib_refuse(lib, who, "n is negative or above the remaining capacity");
    if (cnt == 0) return GUSTO_OK;
    if (!x_init || !glo || !ghi || !tf || !X || !U) return lib_refuse(lib, who, "a null array");
    const size_t c = cnt, n = lib->n, nx = (size_t)lib->N * lib->n, nu = (size_t)lib->N * lib->m, at = lib->count;
    if (!all_finite(x_init, c * n) || !all_finite(tf, c) || !all_finite(X, c * nx) || !all_finite(U, c * nu))
        return lib_refuse(lib, who, "x_init, tf, X and U must be finite");
    std::vector<double> cen(c * n), feat(c);
    for (size_t i = 0; i < c * n; i++) cen[i] = (std::isfinite(glo[i]) && std::isfinite(ghi[i])) ? 0.5 * (glo[i] + ghi[i]) : 0.0;
    std::vector<int> tg(c, 0);
    if (tag) memcpy(tg.data(), tag, sizeof(int) * c);
    LIBCHK(lib, hipSetDevice(lib->device));
    LIBCHK(lib, hipMemcpy(lib->xi + at * n, x_init, sizeof(double) * c * n, hipMemcpyHostToDevice));
    LIBCHK(lib, hipMemcpy(lib->c + at * n, cen.data(), sizeof(double) * c * n, hipMemcpyHostToDevice));
    LIBCHK(lib, hipMemcpy(lib->tf + at, tf, sizeof(double) * c, hipMemcpyHostToDevice));
    LIBCHK(lib, hipMemcpy(lib->tag + at, tg.data(), sizeof(int) * c, hipMemcpyHostToDevice));
    LIBCHK(lib, hipMemcpy(lib->X + at * nx, X, sizeof(double) * c * nx, hipMemcpyHostToDevice));
    LIBCHK(lib, hipMemcpy(lib->U + at * nu, U, sizeof(double) * c * nu, hipMemcpyHostToDevice));
    for (int f = 0; f < lib->F; f++) {
        const int kind = lib->fmap[f] >> 4, i = lib->fmap[f] & 15;
        for (size_t e = 0; e < c; e++) feat[e] = kind == 0 ? x_init[e * n + i] : (kind == 1 ? cen[e * n + i] : tf[e]);
        LIBCHK(lib, hipMemcpy(lib->Feat + (size_t)f * lib->cap + at, feat.data(), sizeof(double) * c, hipMemcpyHostToDevice));
    }
    lib->count += cnt;
    return GUSTO_OK;
}

int gusto_trajlib_get(gusto_trajlib lib, double* x_init, double* goal_c, double* tf, int* tag, double* X, double* U) {
    if (!lib) return GUSTO_ERR_ARG;
    const size_t c = lib->count, n = lib->n, nx = (size_t)lib->N * lib->n, nu = (size_t)lib->N * lib->m;
    if (c == 0) return GUSTO_OK;
    LIBCHK(lib, hipSetDevice(lib->device));
    if (x_init) LIBCHK(lib, hipMemcpy(x_init, lib->xi, sizeof(double) * c * n, hipMemcpyDeviceToHost));
    if (goal_c) LIBCHK(lib, hipMemcpy(goal_c, lib->c, sizeof(double) * c * n, hipMemcpyDeviceToHost));
    if (tf) LIBCHK(lib, hipMemcpy(tf, lib->tf, sizeof(double) * c, hipMemcpyDeviceToHost));
    if (tag) LIBCHK(lib, hipMemcpy(tag, lib->tag, sizeof(int) * c, hipMemcpyDeviceToHost));
    if (X) LIBCHK(lib, hipMemcpy(X, lib->X, sizeof(double) * c * nx, hipMemcpyDeviceToHost));
    if (U) LIBCHK(lib, hipMemcpy(U, lib->U, sizeof(double) * c * nu, hipMemcpyDeviceToHost));
    return GUSTO_OK;
}

int gusto_set_problems_trajlib(gusto_handle h, gusto_trajlib lib, int Bq, int K, const double* x_init, const double* glo,
                               const double* ghi, const double* tf, const int* tag) {
    const char* who = "gusto_set_problems_trajlib";
    if (int rc = seed_enter(h, who, Bq, K, GUSTO_TRAJLIB_MAX_K, "GUSTO_TRAJLIB_MAX_K", {x_init, glo, ghi, tf}, [&]() -> int {
            if (!lib) return refuse(h, who, "a null library");
            if (lib->model != h->model_pub || lib->N != h->N || lib->device != h->device)
                return refuse(h, who, "the library's model, N or device differ from the handle's");
            return GUSTO_OK;
        }))
        return rc;
    const size_t n = h->n, q = Bq, B = q * K;
    const std::vector<double> in = pack_queries(q, n, x_init, glo, ghi, {{tf, q}});
    TrajlibState& S = h->trajlib;
    HIPCHK(h, S.In.ensure(in.size())); HIPCHK(h, S.Tag.ensure(q));
    HIPCHK(h, S.Entry.ensure(B)); HIPCHK(h, S.Dist.ensure(B)); HIPCHK(h, S.Found.ensure(q));
    seed_set_B(h, B);
    HIPCHK(h, hipMemcpyAsync(S.In, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, h->stream));
    if (tag) HIPCHK(h, hipMemcpyAsync(S.Tag, tag, sizeof(int) * q, hipMemcpyHostToDevice, h->stream));
    SearchArgs A;
    A.Q = query_dev(S.In, q, n);
    A.qtag = tag ? S.Tag.get() : nullptr;
    A.feat = lib->Feat; A.etag = lib->tag; A.cap = lib->cap; A.L = lib->count; A.Bq = Bq; A.n = (int)n;
    A.M = feat_map(lib);
    A.entry = S.Entry; A.dist2 = S.Dist; A.n_found = S.Found;
    HIPCHK(h, S.t0.record(h->stream));
    const bool tiled = lib->lds_tile != 0;
    switch (K) {
    case 1: launch_search<1>(A, tiled, h->stream); break;
    case 2: launch_search<2>(A, tiled, h->stream); break;
    case 3: launch_search<3>(A, tiled, h->stream); break;
    case 4: launch_search<4>(A, tiled, h->stream); break;
    case 5: launch_search<5>(A, tiled, h->stream); break;
    case 6: launch_search<6>(A, tiled, h->stream); break;
    case 7: launch_search<7>(A, tiled, h->stream); break;
    default: launch_search<8>(A, tiled, h->stream); break;
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, S.mid.record(h->stream));
    const RetargetArgs R{A.Q, S.Entry, lib->xi, lib->c, lib->X, lib->U, seed_out(h), h->B, K, h->N};
    if (int rc = launch_per_knot(h, R, [](auto M) { return retarget_kernel<decltype(M)::value>; })) return rc;
    HIPCHK(h, S.t1.record(h->stream));
    if (int rc = gusto_problems_loaded(h, false)) return rc;   // (waits for the stream: `in` and `tag` are read by then)
    HIPCHK(h, event_ms(S.t0, S.t1, &S.last_ms));
    HIPCHK(h, event_ms(S.t0, S.mid, &S.search_ms));
    HIPCHK(h, event_ms(S.mid, S.t1, &S.retarget_ms));
    S.K = K; S.Bq = Bq; S.have = true;
    return GUSTO_OK;
}

int gusto_get_trajlib_seeds(gusto_handle h, int* entry, double* dist2, int* n_found) {
    if (int rc = post_enter(h, "gusto_get_trajlib_seeds", nullptr, nullptr)) return rc;
    const TrajlibState& S = h->trajlib;
    if (!S.have) { h->err = "gusto_get_trajlib_seeds: call gusto_set_problems_trajlib first"; return GUSTO_ERR_STATE; }
    if (int rc = copy_out(h, entry, S.Entry.get(), (size_t)S.Bq * S.K)) return rc;
    if (int rc = copy_out(h, dist2, S.Dist.get(), (size_t)S.Bq * S.K)) return rc;
    return copy_out(h, n_found, S.Found.get(), (size_t)S.Bq);
}

int gusto_last_trajlib_ms(gusto_handle h, double* ms) {
    return stage_last_ms(h, &gusto_handle_s::trajlib, ms, "gusto_last_trajlib_ms", "call gusto_set_problems_trajlib first");
}

int gusto_dev_trajlib(gusto_handle h, double* search_ms, double* retarget_ms) {
    if (!h) return GUSTO_ERR_ARG;
    if (!h->trajlib.have) { h->err = "gusto_dev_trajlib: call gusto_set_problems_trajlib first"; return GUSTO_ERR_STATE; }
    if (search_ms) *search_ms = h->trajlib.search_ms;
    if (retarget_ms) *retarget_ms = h->trajlib.retarget_ms;
    return GUSTO_OK;
}

}  // extern "C"
