// replan.hip -- receding-horizon replanning: a batch restarted from where each plan is.  A solved plan, shifted in time by the
// fraction tau already flown and bent to the measured state (and to a moved goal), is the start of the new solve, as GuSTO is
// warm-started at its own previous iterate (scp_gusto.jl:100-102); no counterpart in the reference.  The definitions are stated
// in include/gusto_hip.h.
//   gusto_set_problems_replan         tau and x_now from the caller
//   gusto_set_problems_replan_knots   tau = knot / (Ns - 1), x_now gathered on the device from the stored closed-loop knots
//   gusto_get_replan, gusto_last_replan_ms
// Replan kernel: a thread per (problem, knot), the shape of fan_kernel (multistart.hip) and retarget_kernel (trajlib.hip);
// consecutive threads write consecutive knots.  The thread of knot 0 also writes the problem's x_init, goal_lo, goal_hi and tf.
// A thread of knot k reads the source knots j and j + 1 (and those of knot 0), which other threads may be writing when source
// and destination are the same handle: the source rows are then read from a staging copy made on the stream, device to
// device.  An unseeded problem evaluates straight_line() of seed.hpp, as init_straightline_kernel (scp.hpp) does: that
// kernel's output bit for bit.  No atomics, nothing crosses a problem: a problem's output is the same bit for bit in any batch.
// Gather kernel: a thread per (problem, state entry) copies x_now out of Xcl [B][Ns][S][n].
#include <hip/hip_runtime.h>

#include "seed.hpp"

using namespace gusto;

namespace {

struct ReplanArgs {
    const double *tau, *xnow;                            // [B], [B][n]
    const double *nlo, *nhi;                             // the caller's goals [B][n], null: the source's
    const int *seeded, *sp;                              // [B]: seeded, the source problem (tf and goals)
    const double *Xs, *Us;                               // the source rows, row b [Ns][n], [Ns][m]
    const double *stf, *sglo, *sghi;                     // the source's problems
    SeedOut out;
    int B, N, Ns;
};

template <int MODEL> __global__ void replan_kernel(const ReplanArgs A) {
    using T = MT<MODEL>;
    constexpr int n = T::n, m = T::m;
    KnotId id;
    if (!knot_id(A.B, 1, A.N, id)) return;
    const int b = id.b, k = id.k, s = A.sp[b];
    const double t = id.t;
    const double* xn = A.xnow + (size_t)b * n;
    const double* lo_p = A.nlo ? A.nlo + (size_t)b * n : A.sglo + (size_t)s * n;
    const double* hi_p = A.nlo ? A.nhi + (size_t)b * n : A.sghi + (size_t)s * n;
    double* Xo = A.out.X + ((size_t)b * A.N + k) * n;
    double* Uo = A.out.U + ((size_t)b * A.N + k) * m;
    double glo[n], ghi[n];
#pragma unroll
    for (int i = 0; i < n; i++) { glo[i] = lo_p[i]; ghi[i] = hi_p[i]; }
    if (!A.seeded[b]) {
#pragma unroll
        for (int i = 0; i < n; i++) Xo[i] = straight_line(t, xn[i], glo[i], ghi[i]);
#pragma unroll
        for (int i = 0; i < m; i++) Uo[i] = 0.0;
    } else {
        const double tau = A.tau[b], scale = (double)(A.Ns - 1), span = (double)(A.N - 1);
        const double sig = (tau * (double)(A.N - 1 - k) + (double)k) * scale / span;
        const double sig0 = (tau * span + 0.0) * scale / span;
        const int j = min((int)floor(sig), A.Ns - 2), j0 = min((int)floor(sig0), A.Ns - 2);
        const double a = sig - (double)j, a0 = sig0 - (double)j0;
        const bool last = k == A.N - 1;   // the source's last knot itself
        const double* Xr = A.Xs + (size_t)b * A.Ns * n;
        const double* Ur = A.Us + (size_t)b * A.Ns * m;
#pragma unroll
        for (int i = 0; i < n; i++) {
            const double S = last ? Xr[(size_t)(A.Ns - 1) * n + i] : (1 - a) * Xr[(size_t)j * n + i] + a * Xr[(size_t)(j + 1) * n + i];
            const double S0 = (1 - a0) * Xr[(size_t)j0 * n + i] + a0 * Xr[(size_t)(j0 + 1) * n + i];
            double d = (1 - t) * (xn[i] - S0);
            if (A.nlo) d = d + t * (goal_centre(glo[i], ghi[i]) - goal_centre(A.sglo[(size_t)s * n + i], A.sghi[(size_t)s * n + i]));
            Xo[i] = k == 0 ? xn[i] : S + d;
        }
#pragma unroll
        for (int i = 0; i < m; i++)
            Uo[i] = last ? Ur[(size_t)(A.Ns - 1) * m + i] : (1 - a) * Ur[(size_t)j * m + i] + a * Ur[(size_t)(j + 1) * m + i];
    }
    if (k == 0) seed_problem_tail<MODEL>(A.out, b, xn, glo, ghi, (1 - A.tau[b]) * A.stf[s]);
}

// x_now[b][i] = Xcl[b][knot[b]][sample][i]
__global__ void gather_knots_kernel(const double* Xcl, const int* knot, double* xnow, int B, int Ns, int S, int sample, int n) {
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= B * n) return;
    const int b = gid / n, i = gid % n;
    xnow[gid] = Xcl[(((size_t)b * Ns + knot[b]) * S + sample) * n + i];
}

// the refusals both entry points share, up to the source's problems; *src becomes h for a null source.  Afterwards both
// handles' enqueued solves are complete and the device is current
int replan_enter(gusto_handle h, gusto_handle* src, const char* who, int B, const double* glo, const double* ghi) {
    if (!h) return GUSTO_ERR_ARG;
    if (!*src) *src = h;
    gusto_handle s = *src;
    if (h->trajopt || s->trajopt) return refuse(h, who, "TrajOpt handle (not supported)");
    if (s->model_pub != h->model_pub || s->device != h->device) return refuse(h, who, "the source's model or device differ from the handle's");
    if (B < 1 || B > h->batch_cap) return refuse(h, who, "need 1 <= B <= batch_cap");
    if ((glo == nullptr) != (ghi == nullptr)) return refuse(h, who, "goal_lo and goal_hi are given together or not at all");
    if (!s->have_problems) return refuse(h, who, "the source has no problems", GUSTO_ERR_STATE);
    HIPCHK(h, hipSetDevice(h->device));
    if (int rc = gusto_finish(s)) {
        if (s != h) h->err = std::string(who) + ": the source: " + s->err;
        return rc;
    }
    return s == h ? GUSTO_OK : gusto_complete(h);
}

int replan_impl(gusto_handle h, gusto_handle src, int source, int B, const double* tau, const double* x_now, const double* glo,
                const double* ghi, const int* mask, const char* who) {
    const bool best = source == GUSTO_REPLAN_BEST;
    if (source != GUSTO_REPLAN_TRAJ && !best) return refuse(h, who, "source must be GUSTO_REPLAN_TRAJ or GUSTO_REPLAN_BEST");
    if (!tau || !x_now) return refuse(h, who, "a null tau or x_now");
    if (best && !src->select.have) return refuse(h, who, "GUSTO_REPLAN_BEST: call gusto_select_best on the source first", GUSTO_ERR_STATE);
    const int count = best ? src->select.Bq : src->B;
    if (B > count) return refuse(h, who, "B above the source's count (" + std::to_string(count) + ")");
    const size_t n = h->n, m = h->m, nb = B, Bs = src->B, Ns = src->N;
    for (size_t b = 0; b < nb; b++)
        if (!(tau[b] >= 0 && tau[b] < 1)) return refuse(h, who, "tau must lie in [0, 1) (problem " + std::to_string(b) + ")");
    for (size_t i = 0; i < nb * n; i++)
        if (!(fabs(x_now[i]) < INFINITY)) return refuse(h, who, "x_now must be finite (problem " + std::to_string(i / n) + ")");
    // seeded, and the source problem of every new one
    std::vector<int> meta(2 * nb);
    int *seeded = meta.data(), *sp = meta.data() + nb;
    if (best) {
        const int K = src->select.K;
        std::vector<int> wp(nb);
        HIPCHK(h, hipMemcpy(wp.data(), src->select.Rep.get() + src->select.Bq, sizeof(int) * nb, hipMemcpyDeviceToHost));
        for (size_t b = 0; b < nb; b++) {
            seeded[b] = wp[b] >= 0 && (!mask || mask[b] != 0);
            sp[b] = wp[b] >= 0 ? wp[b] : (int)b * K;
        }
    } else {
        std::vector<int> st(mask ? 0 : nb * ST_NI);
        if (!mask) HIPCHK(h, hipMemcpy(st.data(), src->d_sti, sizeof(int) * st.size(), hipMemcpyDeviceToHost));
        for (size_t b = 0; b < nb; b++) {
            seeded[b] = mask ? mask[b] != 0 : (st[b * ST_NI + ST_CONV] != 0 && st[b * ST_NI + ST_SUCC] != 0);
            sp[b] = (int)b;
        }
    }
    std::vector<double> in(nb * (1 + n) + (glo ? 2 * nb * n : 0));   // tau | x_now | goal_lo | goal_hi: one copy
    memcpy(in.data(), tau, sizeof(double) * nb);
    memcpy(in.data() + nb, x_now, sizeof(double) * nb * n);
    if (glo) {
        memcpy(in.data() + nb * (1 + n), glo, sizeof(double) * nb * n);
        memcpy(in.data() + nb * (1 + 2 * n), ghi, sizeof(double) * nb * n);
    }
    ReplanState& R = h->replan;
    const bool shared = src == h;   // the kernel writes what it would read: staging copies
    HIPCHK(h, R.In.ensure(in.size())); HIPCHK(h, R.Meta.ensure(2 * nb));
    if (shared) HIPCHK(h, R.G.ensure(Bs * (1 + 2 * n)));
    if (shared && !best) { HIPCHK(h, R.Xs.ensure(nb * Ns * n)); HIPCHK(h, R.Us.ensure(nb * Ns * m)); }
    ReplanArgs A;
    A.stf = src->d_tf; A.sglo = src->d_glo; A.sghi = src->d_ghi;
    A.Xs = best ? src->select.X.get() : src->d_X.get();
    A.Us = best ? src->select.U.get() : src->d_U.get();
    seed_set_B(h, B);
    HIPCHK(h, R.t0.record(h->stream));
    HIPCHK(h, hipMemcpyAsync(R.In, in.data(), sizeof(double) * in.size(), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(R.Meta, meta.data(), sizeof(int) * meta.size(), hipMemcpyHostToDevice, h->stream));
    if (shared) {
        double* G = R.G;
        HIPCHK(h, hipMemcpyAsync(G, src->d_tf, sizeof(double) * Bs, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(G + Bs, src->d_glo, sizeof(double) * Bs * n, hipMemcpyDeviceToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(G + Bs * (1 + n), src->d_ghi, sizeof(double) * Bs * n, hipMemcpyDeviceToDevice, h->stream));
        A.stf = G; A.sglo = G + Bs; A.sghi = G + Bs * (1 + n);
        if (!best) {
            HIPCHK(h, hipMemcpyAsync(R.Xs, src->d_X, sizeof(double) * nb * Ns * n, hipMemcpyDeviceToDevice, h->stream));
            HIPCHK(h, hipMemcpyAsync(R.Us, src->d_U, sizeof(double) * nb * Ns * m, hipMemcpyDeviceToDevice, h->stream));
            A.Xs = R.Xs; A.Us = R.Us;
        }
    }
    A.tau = R.In; A.xnow = A.tau + nb;
    A.nlo = glo ? A.xnow + nb * n : nullptr; A.nhi = glo ? A.nlo + nb * n : nullptr;
    A.seeded = R.Meta; A.sp = R.Meta + nb;
    A.out = seed_out(h);
    A.B = B; A.N = h->N; A.Ns = (int)Ns;
    if (int rc = launch_per_knot(h, A, [](auto M) { return replan_kernel<decltype(M)::value>; })) return rc;
    HIPCHK(h, R.t1.record(h->stream));
    if (int rc = gusto_problems_loaded(h, false)) return rc;   // (waits for the stream: `in` and `meta` are read by then)
    HIPCHK(h, event_ms(R.t0, R.t1, &R.last_ms));
    R.seeded.assign(seeded, seeded + nb);
    R.tau.assign(tau, tau + nb);
    R.x_now.assign(x_now, x_now + nb * n);
    R.have = true;
    return GUSTO_OK;
}

}  // namespace

extern "C" {

int gusto_set_problems_replan(gusto_handle h, gusto_handle src, int source, int B, const double* tau, const double* x_now,
                              const double* goal_lo, const double* goal_hi, const int* mask) {
    const char* who = "gusto_set_problems_replan";
    if (int rc = replan_enter(h, &src, who, B, goal_lo, goal_hi)) return rc;
    return replan_impl(h, src, source, B, tau, x_now, goal_lo, goal_hi, mask, who);
}

int gusto_set_problems_replan_knots(gusto_handle h, gusto_handle src, int B, const int* knot, int sample, const double* goal_lo,
                                    const double* goal_hi, const int* mask) {
    const char* who = "gusto_set_problems_replan_knots";
    if (int rc = replan_enter(h, &src, who, B, goal_lo, goal_hi)) return rc;
    if (!knot) return refuse(h, who, "a null knot");
    const SimulateState& S = src->simulate;
    if (!S.have || !S.have_knots) return refuse(h, who, "the source has no stored knots (gusto_simulate with store_knots = 1)", GUSTO_ERR_STATE);
    if (B > src->B) return refuse(h, who, "B above the source's count (" + std::to_string(src->B) + ")");
    if (sample < 0 || sample >= S.S) return refuse(h, who, "sample outside 0 .. n_samples - 1");
    const size_t nb = B, n = h->n;
    const int Ns = src->N;
    std::vector<double> tau(nb), x_now(nb * n);
    for (size_t b = 0; b < nb; b++) {
        if (knot[b] < 0 || knot[b] > Ns - 2) return refuse(h, who, "knot outside 0 .. Ns - 2 (problem " + std::to_string(b) + ")");
        tau[b] = (double)knot[b] / (double)(Ns - 1);
    }
    ReplanState& R = h->replan;
    HIPCHK(h, R.Meta.ensure(2 * nb)); HIPCHK(h, R.Xnow.ensure(nb * n));
    HIPCHK(h, hipMemcpyAsync(R.Meta, knot, sizeof(int) * nb, hipMemcpyHostToDevice, h->stream));
    const int tot = (int)(nb * n);
    hipLaunchKernelGGL(gather_knots_kernel, dim3((tot + 255) / 256), dim3(256), 0, h->stream, S.Knots.get(), R.Meta.get(), R.Xnow.get(), B, Ns,
                       S.S, sample, (int)n);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(x_now.data(), R.Xnow, sizeof(double) * nb * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < nb * n; i++)
        if (!(fabs(x_now[i]) < INFINITY))
            return refuse(h, who, "the stored state of problem " + std::to_string(i / n) + " is not finite (a sample flagged non-finite)");
    return replan_impl(h, src, GUSTO_REPLAN_TRAJ, B, tau.data(), x_now.data(), goal_lo, goal_hi, mask, who);
}

int gusto_get_replan(gusto_handle h, int* seeded, double* tau, double* x_now) {
    if (!h) return GUSTO_ERR_ARG;
    const ReplanState& R = h->replan;
    if (!R.have) { h->err = "gusto_get_replan: the handle's problems were not set by gusto_set_problems_replan"; return GUSTO_ERR_STATE; }
    if (seeded) memcpy(seeded, R.seeded.data(), sizeof(int) * R.seeded.size());
    if (tau) memcpy(tau, R.tau.data(), sizeof(double) * R.tau.size());
    if (x_now) memcpy(x_now, R.x_now.data(), sizeof(double) * R.x_now.size());
    return GUSTO_OK;
}

int gusto_last_replan_ms(gusto_handle h, double* ms) {
    return stage_last_ms(h, &gusto_handle_s::replan, ms, "gusto_last_replan_ms", "the handle's problems were not set by gusto_set_problems_replan");
}

}  // extern "C"
