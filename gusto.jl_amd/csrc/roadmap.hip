// roadmap.hip -- roadmap seeds: every query of a batch starts from a shortest collision-free polyline through the corners of
// its inflated keep-out set (a visibility graph), found on the device before the first solve; the alternates of a query are
// the shortest paths of other homotopy classes, one banned component at a time.  No counterpart in the reference, whose
// init_traj_straightline (freeflyer_se2.jl:97-111) is what a query with an unblocked line still gets; include/gusto_hip.h
// states the definitions (blocking sets, nodes, edges, status, alternates, seed, report).
//   gusto_default_roadmap_opts, gusto_set_problems_roadmap, gusto_get_roadmap, gusto_last_roadmap_ms
// Graph kernel: once per keep-out set.  A wave is (set, node u, block of 64 nodes v), lane = v.  The set's components are staged
// into LDS already inflated; a lane rebuilds the two nodes from them (no wave reads what another writes), loops over the
// components (uniform LDS reads) and __ballot forms the 64-bit word that one lane stores.  The waves of u = 0 also write the
// node coordinates and the dead flags.  The full symmetric matrix is stored: the search reads whole rows.
// Search kernel: one wave per query, its alternates in sequence.  Node coordinates, components and predecessors live in LDS; a
// lane owns the nodes lane, lane + 64, ... (at most RM_SLOTS = 9) with their distances in registers.  Start and goal
// visibility are computed here.  A round is two wave_reduce calls (the smallest distance, then the lowest index among its
// holders: the idiom of select_kernel in multistart.hip), then every lane relaxes its nodes against the bit row of the settled
// node, the edge length recomputed from the coordinates.  Lane 0 walks the predecessors back and writes the path as points.
// Seed kernel: a thread per (problem, knot), the shape of fan_kernel (multistart.hip): the polyline resampled by arc length on
// the workspace entries, straight_line() of seed.hpp elsewhere, and the [Bq] inputs replicated into the handle's [B] arrays.
// No atomics, every reduction in a fixed order, nothing crosses a query: a query's outputs are the same bit for bit in any batch.
#include <hip/hip_runtime.h>

#include "seed.hpp"

using namespace gusto;

namespace {

constexpr int RM_MAXC = 64;                        // keep-out components per set (gusto_set_env*)
constexpr int RM_VIA = GUSTO_ROADMAP_MAX_VIA;      // interior nodes of a path
constexpr int RM_PTS = RM_VIA + 2;                 // points of a polyline
constexpr int RM_BAN = GUSTO_ROADMAP_MAX_K;        // row length of `banned`
constexpr int RM_SLOTS = 9;                        // nodes per lane: 2 + 2^3 64 = 514 nodes over 64 lanes
constexpr double RM_NONE = 4e9;                    // (node indices stay far below)

// A component's blocking set in LDS, 2 WS doubles: an open box (lo - inflate, hi + inflate) as lo', hi'; an open ball as centre,
// then R + inflate.  A lane of the wave stages component `lane` from the set's tables (boxes then spheres).
template <int WS> GD void stage_components(double* cg, const int* rec, const double* box, const double* sph, double inflate, int lane) {
    const int nb = rec[1], C = nb + rec[3];
    if (lane < C) {
        double* g = cg + lane * 2 * WS;
        if (lane < nb) {
            const double* s = box + 6 * ((size_t)rec[0] + lane);
#pragma unroll
            for (int j = 0; j < WS; j++) { g[j] = s[j] - inflate; g[WS + j] = s[3 + j] + inflate; }
        } else {
            const double* s = sph + 4 * ((size_t)rec[2] + (lane - nb));
#pragma unroll
            for (int j = 0; j < WS; j++) { g[j] = s[j]; g[WS + j] = 0.0; }
            g[WS] = s[3] + inflate;
        }
    }
}

// corner `e & (2^WS - 1)` of component `e >> WS`: bit j chooses the low or the high side, `pad` outside the blocking set
template <int WS> GD void env_node(const double* cg, int nb, double pad, int e, double* p) {
    const int c = e >> WS;
    const double* g = cg + c * 2 * WS;
#pragma unroll
    for (int j = 0; j < WS; j++) {
        const bool high = (e >> j) & 1;
        if (c < nb) p[j] = high ? g[WS + j] + pad : g[j] - pad;
        else p[j] = high ? g[j] + (g[WS] + pad) : g[j] - (g[WS] + pad);
    }
}

// p strictly inside the blocking set
template <int WS> GD bool point_inside(bool is_box, const double* g, const double* p) {
    if (is_box) {
        bool in = true;
#pragma unroll
        for (int j = 0; j < WS; j++) in = in && g[j] < p[j] && p[j] < g[WS + j];
        return in;
    }
    double s2 = 0.0;
#pragma unroll
    for (int j = 0; j < WS; j++) { const double v = p[j] - g[j]; s2 += v * v; }
    return s2 < g[WS] * g[WS];
}

// the segment p -> q meets the blocking set: slabs for the open box, the closest point for the open ball
template <int WS> GD bool seg_hits(bool is_box, const double* g, const double* p, const double* q) {
    if (is_box) {
        double L = -INFINITY, H = INFINITY;
#pragma unroll
        for (int j = 0; j < WS; j++) {
            const double d = q[j] - p[j];
            if (d == 0.0) {
                if (!(g[j] < p[j] && p[j] < g[WS + j])) L = INFINITY;
            } else {
                const double t1 = (g[j] - p[j]) / d, t2 = (g[WS + j] - p[j]) / d;
                L = fmax(L, fmin(t1, t2));
                H = fmin(H, fmax(t1, t2));
            }
        }
        return fmax(L, 0.0) < fmin(H, 1.0);
    }
    double dd = 0.0, cd = 0.0;
#pragma unroll
    for (int j = 0; j < WS; j++) { const double d = q[j] - p[j]; dd += d * d; cd += (g[j] - p[j]) * d; }
    double t = dd > 0.0 ? cd / dd : 0.0;
    t = fmin(fmax(t, 0.0), 1.0);
    double s2 = 0.0;
#pragma unroll
    for (int j = 0; j < WS; j++) { const double v = (p[j] + t * (q[j] - p[j])) - g[j]; s2 += v * v; }
    return s2 < g[WS] * g[WS];
}

// sqrt(sum d_j^2) in coordinate order
template <int WS> GD double edge_length(const double* p, const double* q) {
    double s2 = 0.0;
#pragma unroll
    for (int j = 0; j < WS; j++) { const double d = q[j] - p[j]; s2 += d * d; }
    return sqrt(s2);
}

struct GraphArgs {
    const int* rec;              // [n_env][4] box offset, n_box, sphere offset, n_sph in the handle's tables
    const double *box, *sph;     // the handle's tables
    double inflate, pad;
    int VeMax, W;                // rows of a set, 64-bit words of a row: sized from the call's largest component count
    double* nodes;               // [n_env][VeMax][WS]
    int* dead;                   // [n_env][VeMax] (1 behind a set's own count)
    unsigned long long* vis;     // [n_env][VeMax][W]
};

template <int WS> __global__ void __launch_bounds__(64) graph_kernel(const GraphArgs A) {
    __shared__ double cg[RM_MAXC * 2 * WS];
    const int lane = threadIdx.x;
    const size_t g = blockIdx.x;
    const int w = (int)(g % A.W), u = (int)((g / A.W) % A.VeMax);
    const size_t e = g / ((size_t)A.W * A.VeMax);
    const int* rec = A.rec + 4 * e;
    const int nb = rec[1], C = nb + rec[3], Ve = C << WS, v = w * 64 + lane;
    stage_components<WS>(cg, rec, A.box, A.sph, A.inflate, lane);
    __syncthreads();
    const bool uin = u < Ve, vin = v < Ve;
    double pu[WS], pv[WS];
#pragma unroll
    for (int j = 0; j < WS; j++) { pu[j] = 0.0; pv[j] = 0.0; }
    if (uin) env_node<WS>(cg, nb, A.pad, u, pu);
    if (vin) env_node<WS>(cg, nb, A.pad, v, pv);
    bool du = false, dv = false, hit = false;
    for (int c = 0; c < C; c++) {
        const double* gc = cg + c * 2 * WS;
        const bool is_box = c < nb;
        if (uin) du = du || point_inside<WS>(is_box, gc, pu);
        if (vin) dv = dv || point_inside<WS>(is_box, gc, pv);
        if (uin && vin) hit = hit || seg_hits<WS>(is_box, gc, pu, pv);
    }
    const bool see = uin && vin && !du && !dv && !hit && u != v;
    const unsigned long long word = __ballot(see);
    if (lane == 0) A.vis[(e * A.VeMax + u) * A.W + w] = word;
    if (u == 0 && v < A.VeMax) {
#pragma unroll
        for (int j = 0; j < WS; j++) A.nodes[(e * A.VeMax + v) * WS + j] = pv[j];
        A.dead[e * A.VeMax + v] = vin ? (dv ? 1 : 0) : 1;
    }
}

struct SearchArgs {
    const double *xi, *glo, *ghi;    // the queries [Bq][n]
    const int* rec;                  // [n_env][4]
    const double *box, *sph;
    double inflate;
    int n_env, VeMax, W, K, straight_first;
    const double* nodes;
    const int* dead;
    const unsigned long long* vis;
    int *status, *n_via, *via, *banned;   // [B], [B], [B][RM_VIA], [B][RM_BAN]
    double *length, *pts;                 // [B], [B][RM_PTS][3]
};

// the report row of problem b (lane 0): a straight line of status st, or the path held in via[0 .. nv)
GD void write_row(const SearchArgs& A, size_t b, int st, int nv, const int* via, double len, int nban, const int* ban) {
    A.status[b] = st;
    A.n_via[b] = nv;
    for (int i = 0; i < RM_VIA; i++) A.via[b * RM_VIA + i] = i < nv ? via[i] : -1;
    A.length[b] = len;
    for (int i = 0; i < RM_BAN; i++) A.banned[b * RM_BAN + i] = i < nban ? ban[i] : -1;
}

template <int MODEL> __global__ void __launch_bounds__(64) search_kernel(const SearchArgs A) {
    using T = MT<MODEL>;
    constexpr int n = T::n, WS = T::WS;
    __shared__ double cg[RM_MAXC * 2 * WS];
    __shared__ double P[(2 + (RM_MAXC << WS)) * WS];
    __shared__ int pred[2 + (RM_MAXC << WS)];
    __shared__ int walk[4 + RM_VIA];          // status, n_via, first component, -, via
    const int lane = threadIdx.x, K = A.K, sf = A.straight_first;
    const size_t q = blockIdx.x, e = A.n_env == 1 ? 0 : q;
    const int* rec = A.rec + 4 * e;
    const int nb = rec[1], C = nb + rec[3], V = 2 + (C << WS);
    stage_components<WS>(cg, rec, A.box, A.sph, A.inflate, lane);
    for (int idx = lane; idx < V; idx += 64) {
#pragma unroll
        for (int j = 0; j < WS; j++) {
            double x;
            if (idx == 0) x = A.xi[q * n + j];
            else if (idx == 1) x = goal_centre(A.glo[q * n + j], A.ghi[q * n + j]);
            else x = A.nodes[(e * A.VeMax + (idx - 2)) * WS + j];
            P[idx * WS + j] = x;
        }
    }
    __syncthreads();
    double p0[WS], pg[WS];
#pragma unroll
    for (int j = 0; j < WS; j++) { p0[j] = P[j]; pg[j] = P[WS + j]; }

    // per owned node: dead by geometry, seen from the start, seen from the goal (bit s = slot s)
    int deadm = 0, v0m = 0, v1m = 0;
#pragma unroll
    for (int s = 0; s < RM_SLOTS; s++) {
        const int idx = lane + 64 * s;
        if (idx >= V) continue;
        double p[WS];
#pragma unroll
        for (int j = 0; j < WS; j++) p[j] = P[idx * WS + j];
        bool dd = idx >= 2 && A.dead[e * A.VeMax + (idx - 2)] != 0, h0 = false, h1 = false;
        for (int c = 0; c < C; c++) {
            const double* gc = cg + c * 2 * WS;
            const bool is_box = c < nb;
            if (idx < 2) dd = dd || point_inside<WS>(is_box, gc, p);
            h0 = h0 || seg_hits<WS>(is_box, gc, p0, p);
            h1 = h1 || seg_hits<WS>(is_box, gc, pg, p);
        }
        deadm |= (dd ? 1 : 0) << s;
        v0m |= (h0 ? 0 : 1) << s;
        v1m |= (h1 ? 0 : 1) << s;
    }
    const bool dead0 = __shfl(deadm & 1, 0) != 0, dead1 = __shfl(deadm & 1, 1) != 0;
    const bool direct = __shfl(v0m & 1, 1) != 0;   // node 1 seen from node 0
    const double len01 = edge_length<WS>(p0, pg);

    int nban = 0, ban[RM_BAN];
    unsigned long long banmask = 0;
#pragma unroll
    for (int i = 0; i < RM_BAN; i++) ban[i] = -1;
    const int KP = K - sf;                  // alternates that are searches
    bool failed = false;
    int fst = 0;
    double flen = INFINITY;
    for (int jp = 0; jp < (KP > 0 ? KP : 1); jp++) {
        const size_t b = q * K + jp + sf;
        const bool out = jp < KP;
        int st = fst;
        double len = flen;
        if (!failed) {
            if (dead0 || dead1) { st = GUSTO_ROADMAP_END_BLOCKED; len = INFINITY; }
            else if (direct) { st = GUSTO_ROADMAP_DIRECT; len = len01; }
            else {
                // Dijkstra from node 0 under the ban list
                double dist[RM_SLOTS];
                int alive = 0, settled = 0;
#pragma unroll
                for (int s = 0; s < RM_SLOTS; s++) {
                    const int idx = lane + 64 * s;
                    dist[s] = idx == 0 ? 0.0 : INFINITY;
                    bool al = idx < V && !((deadm >> s) & 1);
                    if (al && idx >= 2 && ((banmask >> ((idx - 2) >> WS)) & 1)) al = false;
                    alive |= (al ? 1 : 0) << s;
                    if (idx < V) pred[idx] = -1;
                }
                bool found = false;
                for (int round = 0; round < V; round++) {
                    double dl = INFINITY;
                    int il = -1;
#pragma unroll
                    for (int s = 0; s < RM_SLOTS; s++)
                        if (((alive & ~settled) >> s) & 1)
                            if (dist[s] < dl) { dl = dist[s]; il = lane + 64 * s; }   // (strict: the lowest of the lane's equal minima)
                    const double dmin = wave_reduce(dl, OpMin());
                    if (!(dmin < INFINITY)) break;
                    const int sn = (int)wave_reduce((il >= 0 && dl == dmin) ? (double)il : RM_NONE, OpMin());   // ties: the lowest index
                    if ((sn & 63) == lane) settled |= 1 << (sn >> 6);
                    if (sn == 1) { found = true; break; }
                    double ps[WS];
#pragma unroll
                    for (int j = 0; j < WS; j++) ps[j] = P[sn * WS + j];
                    // does the settled node see the goal: its owner knows
                    const int sgoal = __shfl((v1m >> (sn >> 6)) & 1, sn & 63);
                    const unsigned long long* row = A.vis + (e * A.VeMax + (sn >= 2 ? sn - 2 : 0)) * A.W;
#pragma unroll
                    for (int s = 0; s < RM_SLOTS; s++) {
                        const int idx = lane + 64 * s;
                        if (!(((alive & ~settled) >> s) & 1)) continue;
                        bool adj;
                        if (sn == 0) adj = (v0m >> s) & 1;
                        else if (idx == 1) adj = sgoal != 0;
                        else if (idx == 0) adj = false;
                        else { const int ev = idx - 2; adj = (row[ev >> 6] >> (ev & 63)) & 1; }
                        if (!adj) continue;
                        double p[WS];
#pragma unroll
                        for (int j = 0; j < WS; j++) p[j] = P[idx * WS + j];
                        const double nd = dmin + edge_length<WS>(ps, p);
                        if (nd < dist[s]) { dist[s] = nd; pred[idx] = sn; }   // (strict: the first predecessor of equal lengths stays)
                    }
                }
                const double dgoal = __shfl(dist[0], 1);
                __syncthreads();
                if (lane == 0) {
                    int stw = GUSTO_ROADMAP_NO_PATH, cnt = 0;
                    if (found) {
                        int cur = pred[1];
                        while (cur > 0 && cnt <= RM_VIA) { cnt++; cur = pred[cur]; }
                        stw = cur == 0 && cnt <= RM_VIA ? GUSTO_ROADMAP_PATH : GUSTO_ROADMAP_TOO_LONG;
                        if (stw == GUSTO_ROADMAP_PATH) {
                            cur = pred[1];
                            for (int i = cnt - 1; i >= 0; i--) { walk[4 + i] = cur; cur = pred[cur]; }
                        }
                    }
                    walk[0] = stw;
                    walk[1] = stw == GUSTO_ROADMAP_PATH ? cnt : 0;
                    walk[2] = stw == GUSTO_ROADMAP_PATH && cnt > 0 ? (walk[4] - 2) >> WS : -1;
                }
                __syncthreads();
                st = walk[0];
                len = st == GUSTO_ROADMAP_PATH ? dgoal : INFINITY;
            }
        }
        if (st == GUSTO_ROADMAP_PATH) {
            const int nv = walk[1];
            if (lane == 0 && out) {
                write_row(A, b, st, nv, walk + 4, len, nban, ban);
                double* pt = A.pts + b * RM_PTS * 3;
                for (int i = 0; i < nv + 2; i++) {
                    const int idx = i == 0 ? 0 : (i == nv + 1 ? 1 : walk[4 + i - 1]);
#pragma unroll
                    for (int j = 0; j < WS; j++) pt[i * 3 + j] = P[idx * WS + j];
                }
            }
            if (lane == 0 && sf && jp == 0) write_row(A, q * K, GUSTO_ROADMAP_STRAIGHT, 0, walk + 4, INFINITY, 0, ban);
            // the component of the first interior node joins the ban list
            const int fc = walk[2];
            if (fc >= 0 && nban < RM_BAN) {
#pragma unroll
                for (int i = 0; i < RM_BAN; i++) if (i == nban) ban[i] = fc;
                nban++;
                banmask |= 1ull << fc;
            }
            __syncthreads();   // (walk is rewritten by the next alternate)
        } else {
            // this alternate and all later ones: the straight line with this status
            if (!failed) { failed = true; fst = st; flen = len; }
            if (lane == 0 && out) write_row(A, b, st, 0, walk + 4, len, nban, ban);
            if (lane == 0 && sf && jp == 0) write_row(A, q * K, st, 0, walk + 4, len, nban, ban);
        }
    }
}

struct SeedArgs {
    QueryDev Q;                    // the queries; extra: tf [Bq]
    const int *status, *n_via;     // [B]
    const double *length, *pts;    // [B], [B][RM_PTS][3]
    SeedOut out;
    int B, K, N;
};

template <int MODEL> __global__ void seed_kernel(const SeedArgs A) {
    using T = MT<MODEL>;
    constexpr int n = T::n, m = T::m, WS = T::WS;
    KnotId id;
    if (!knot_id(A.B, A.K, A.N, id)) return;
    const int b = id.b, k = id.k;
    const double t = id.t;
    const size_t qn = (size_t)id.q * n;   // the query's row of xi, glo, ghi
    double* Xo = A.out.X + ((size_t)b * A.N + k) * n;
    double x[WS];   // the workspace entries; the others are the line's and go out at once
#pragma unroll
    for (int i = 0; i < n; i++) {
        const double xl = straight_line(t, A.Q.xi[qn + i], A.Q.glo[qn + i], A.Q.ghi[qn + i]);
        if (i < WS) x[i] = xl;
        else Xo[i] = xl;
    }
    if (A.status[b] == GUSTO_ROADMAP_PATH && k > 0 && k < A.N - 1) {
        // the point at arc length t Lp: the first segment whose end lies beyond it (the last one otherwise)
        const double* pt = A.pts + (size_t)b * RM_PTS * 3;
        const int nseg = A.n_via[b] + 1;
        const double s = t * A.length[b];
        double cum = 0.0, len = edge_length<WS>(pt, pt + 3);
        int i = 0;
        while (i < nseg - 1 && s >= cum + len) {
            cum += len;
            i++;
            len = edge_length<WS>(pt + 3 * i, pt + 3 * i + 3);
        }
        const double f = len > 0.0 ? (s - cum) / len : 0.0;
#pragma unroll
        for (int j = 0; j < WS; j++) x[j] = pt[3 * i + j] + f * (pt[3 * i + 3 + j] - pt[3 * i + j]);
    }
#pragma unroll
    for (int i = 0; i < WS; i++) Xo[i] = x[i];
#pragma unroll
    for (int i = 0; i < m; i++) A.out.U[((size_t)b * A.N + k) * m + i] = 0.0;
    if (k == 0) seed_problem_tail<MODEL>(A.out, b, A.Q.xi + qn, A.Q.glo + qn, A.Q.ghi + qn, A.Q.extra[id.q]);
}

}  // namespace

extern "C" {

int gusto_default_roadmap_opts(int model_id, gusto_roadmap_opts* o) {
    if (!o || !model_info(model_id)) return GUSTO_ERR_ARG;
    gusto_scp_params sp;
    gusto_model_params mp;
    if (int rc = gusto_default_params(model_id, &sp, &mp)) return rc;
    memset(o, 0, sizeof(*o));
    o->inflate = mp.radius + 0.02;   // (placeholders from the table study: gusto_hip.h)
    o->pad = 0.03;
    o->straight_first = 0;
    return GUSTO_OK;
}

int gusto_set_problems_roadmap(gusto_handle h, int Bq, int K, const double* x_init, const double* glo, const double* ghi,
                               const double* tf, const gusto_roadmap_opts* opts) {
    const char* who = "gusto_set_problems_roadmap";
    gusto_roadmap_opts o;
    if (int rc = seed_enter(h, who, Bq, K, GUSTO_ROADMAP_MAX_K, "GUSTO_ROADMAP_MAX_K", {x_init, glo, ghi, tf}, [&]() -> int {
            if (opts) o = *opts;
            else {
                o.inflate = h->mp.radius + 0.02; o.pad = 0.03; o.straight_first = 0;   // the defaults, on the handle's own radius
            }
            if (!(o.inflate >= 0 && o.inflate < INFINITY)) return refuse(h, who, "inflate must be finite and >= 0");
            if (!(o.pad > 0 && o.pad < INFINITY)) return refuse(h, who, "pad must be finite and > 0");
            if (o.straight_first != 0 && o.straight_first != 1) return refuse(h, who, "straight_first must be 0 or 1");
            return GUSTO_OK;
        }))
        return rc;

    // the keep-out set of every query: the shared one, or the set of problem q K
    const size_t n = h->n, q = Bq, B = q * K;
    const int n_env = h->d_env ? Bq : 1;
    std::vector<int> rec(4 * (size_t)n_env);
    int Cmax = 0;
    if (h->d_env) {
        if ((size_t)h->env_B != B) return refuse(h, who, "the handle holds per-problem keep-out sets for another number of problems than Bq K", GUSTO_ERR_STATE);
        std::vector<int> all(4 * B);
        HIPCHK(h, hipMemcpy(all.data(), h->d_env, sizeof(int) * all.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < q; i++) memcpy(&rec[4 * i], &all[4 * i * K], sizeof(int) * 4);
    } else {
        rec[0] = 0; rec[1] = h->n_box; rec[2] = 0; rec[3] = h->n_sph;
    }
    for (int e = 0; e < n_env; e++) {
        if (rec[4 * e + 1] < 0 || rec[4 * e + 3] < 0 || rec[4 * e + 1] + rec[4 * e + 3] > RM_MAXC)
            return refuse(h, who, "more than 64 keep-out components in a set", GUSTO_ERR_STATE);
        Cmax = std::max(Cmax, rec[4 * e + 1] + rec[4 * e + 3]);
    }
    int WS = 0;
    if (int rc = for_model(h->model_pub, [&](auto M) -> int { WS = MT<decltype(M)::value>::WS; return GUSTO_OK; })) return rc;
    const size_t VeMax = (size_t)Cmax << WS, W = (VeMax + 63) / 64;

    RoadmapState& S = h->roadmap;
    const std::vector<double> in = pack_queries(q, n, x_init, glo, ghi, {{tf, q}});
    HIPCHK(h, S.In.ensure(in.size())); HIPCHK(h, S.Rec.ensure(rec.size()));
    HIPCHK(h, S.Nodes.ensure((size_t)n_env * VeMax * WS)); HIPCHK(h, S.Dead.ensure((size_t)n_env * VeMax));
    HIPCHK(h, S.Vis.ensure((size_t)n_env * VeMax * W));
    HIPCHK(h, S.I.ensure(B * (2 + RM_VIA + RM_BAN))); HIPCHK(h, S.Len.ensure(B)); HIPCHK(h, S.Pts.ensure(B * RM_PTS * 3));
    if ((size_t)n_env * VeMax * W > (size_t)INT_MAX) return refuse(h, who, "keep-out sets too large");

    S.have = false;
    seed_set_B(h, B);
    HIPCHK(h, S.t0.record(h->stream));
    HIPCHK(h, hipMemcpyAsync(S.In, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(S.Rec, rec.data(), sizeof(int) * rec.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemsetAsync(S.Pts, 0, sizeof(double) * B * RM_PTS * 3, h->stream));
    GraphArgs G{};
    G.rec = S.Rec; G.box = h->d_box; G.sph = h->d_sph; G.inflate = o.inflate; G.pad = o.pad;
    G.VeMax = (int)VeMax; G.W = (int)W; G.nodes = S.Nodes; G.dead = S.Dead; G.vis = S.Vis;
    SearchArgs Q{};
    const QueryDev D = query_dev(S.In, q, n);
    Q.xi = D.xi; Q.glo = D.glo; Q.ghi = D.ghi;
    Q.rec = S.Rec; Q.box = h->d_box; Q.sph = h->d_sph; Q.inflate = o.inflate;
    Q.n_env = n_env; Q.VeMax = (int)VeMax; Q.W = (int)W; Q.K = K; Q.straight_first = o.straight_first;
    Q.nodes = S.Nodes; Q.dead = S.Dead; Q.vis = S.Vis;
    Q.status = S.I; Q.n_via = S.I + B; Q.via = S.I + 2 * B; Q.banned = S.I + (2 + RM_VIA) * B;
    Q.length = S.Len; Q.pts = S.Pts;
    const SeedArgs A{D, Q.status, Q.n_via, S.Len, S.Pts, seed_out(h), h->B, K, h->N};
    if (int rc = for_model(h->model_pub, [&](auto M) -> int {
            constexpr int MODEL = decltype(M)::value, WSM = MT<MODEL>::WS;
            if (VeMax) {
                hipLaunchKernelGGL(graph_kernel<WSM>, dim3((unsigned)((size_t)n_env * VeMax * W)), dim3(64), 0, h->stream, G);
                HIPCHK(h, hipGetLastError());
            }
            HIPCHK(h, S.t1.record(h->stream));
            hipLaunchKernelGGL(search_kernel<MODEL>, dim3((unsigned)q), dim3(64), 0, h->stream, Q);
            HIPCHK(h, hipGetLastError());
            HIPCHK(h, S.t2.record(h->stream));
            return GUSTO_OK;
        }))
        return rc;
    if (int rc = launch_per_knot(h, A, [](auto M) { return seed_kernel<decltype(M)::value>; })) return rc;
    HIPCHK(h, S.t3.record(h->stream));
    if (int rc = gusto_problems_loaded(h, false)) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));   // (`in` and `rec` are read by then)
    HIPCHK(h, event_ms(S.t0, S.t3, &S.last_ms));
    HIPCHK(h, event_ms(S.t0, S.t1, &S.stage_ms[0]));
    HIPCHK(h, event_ms(S.t1, S.t2, &S.stage_ms[1]));
    HIPCHK(h, event_ms(S.t2, S.t3, &S.stage_ms[2]));
    S.K = K; S.Bq = Bq; S.have = true;
    return GUSTO_OK;
}

int gusto_get_roadmap(gusto_handle h, gusto_roadmap_report* out) {
    if (!h) return GUSTO_ERR_ARG;
    if (int rc = getter_enter(h, false)) return rc;
    const RoadmapState& S = h->roadmap;
    if (!S.have) { h->err = "gusto_get_roadmap: call gusto_set_problems_roadmap first"; return GUSTO_ERR_STATE; }
    if (!out) return GUSTO_OK;
    const size_t B = (size_t)S.Bq * S.K;
    if (int rc = copy_out(h, out->status, S.I.get(), B)) return rc;
    if (int rc = copy_out(h, out->n_via, S.I.get() + B, B)) return rc;
    if (int rc = copy_out(h, out->via, S.I.get() + 2 * B, B * RM_VIA)) return rc;
    if (int rc = copy_out(h, out->length, S.Len.get(), B)) return rc;
    if (int rc = copy_out(h, out->banned, S.I.get() + (2 + RM_VIA) * B, B * RM_BAN)) return rc;
    if (out->stage_ms) memcpy(out->stage_ms, S.stage_ms, sizeof(S.stage_ms));
    return GUSTO_OK;
}

int gusto_last_roadmap_ms(gusto_handle h, double* ms) {
    return stage_last_ms(h, &gusto_handle_s::roadmap, ms, "gusto_last_roadmap_ms", "call gusto_set_problems_roadmap first");
}

}  // extern "C"
