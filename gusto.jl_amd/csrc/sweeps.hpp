// sweeps.hpp -- the vector sweeps of the condensed KKT system (ipm.hpp) and the costate passes: the one-wave sweeps on v_readlane
// (backward_sweep_1w / forward_sweep_1w; segw.hpp has them over a range of knots), on the fp64 DPP broadcast (freeflyerSE2:
// backward_sweep_dpp / forward_sweep_dpp), costate_pass_1w and adjoint_sweep_1w of the 12/13-state models, and the multi-wave
// sweeps of a problem of more than 64 knots.  Included by ipm.hpp, which holds the views (Blk, SweepView) they run on.
// Reference path: the convex subproblem handed to JuMP.optimize!, scp_gusto.jl:104,178-314.
#pragma once

namespace gusto {

// Affine vector recurrences of the one-wave path.  The wave is split into C = 64/n groups of n lanes; group g
// holds the operands of knot (k0 -+ g) of the current chunk of C knots, so ONE batch of global loads feeds C knots
// of the dependency chain (the recurrences are memory-latency bound otherwise), and the next chunk is fetched
// while the current one computes.  The n-vector travels between groups with v_readlane (no LDS on the chain).
//
// One step of that chain, the one definition every readlane sweep expands (here and in segw.hpp): every lane forms
// rhs + sum_l c[l] v[lane l of group gs - 1] (of group C - 1 at gs = 0: the vector the chunk before ended with) and the lanes of
// group gs keep it in v.  Uses n, C, g and the step gs of the sweep it stands in; PS_ = 1, or 4 independent partial sums
// (12/13-state models: the n dependent FMAs of one dot product were most of the time per knot).
// The 2 n v_readlane of a step come first, into n scalar pairs of their own, then the FMAs: left alone hipcc reuses ONE scalar
// pair -- readlane, readlane, s_nop, fmac, n times over -- and every fmac waits for its two readlanes, which wait for the fmac
// before them to have read the pair (24 cycles per element, 12 of them avoidable).
// TEXT, not a function (like scp_body.inc): as a force-inlined function template the step is optimised on its own before it is
// inlined, and the sweeps around it come out with other registers and copies (TrajOpt freeflyerSE2, backward sweep: 3044 -> 3036
// bytes) -- the same arithmetic, but kernels that would have to be measured again instead of compared byte for byte.
#define GUSTO_CHAIN_STEP(v, rhs, c, PS_)                                                          \
    {                                                                                             \
        const int sg = (gs == 0) ? C - 1 : gs - 1;                                                \
        double acc[PS_];                                                                          \
        _Pragma("unroll") for (int q = 0; q < PS_; q++) acc[q] = (q == 0) ? (rhs) : 0.0;          \
        double pb[n];                                                                             \
        _Pragma("unroll") for (int l = 0; l < n; l++) pb[l] = readlane_f64(v, sg * n + l);        \
        __builtin_amdgcn_sched_barrier(0);                                                        \
        _Pragma("unroll") for (int l = 0; l < n; l++) acc[l % PS_] += (c)[l] * pb[l];             \
        const double s = (PS_ == 4) ? (acc[0] + acc[1]) + (acc[2] + acc[PS_ - 1]) : acc[0];       \
        v = (g == gs) ? s : v;                                                                    \
    }

// chunk buffers of the 12/13-state sweeps and costate passes: RING - 1 fetches in flight (backward_sweep_1w says why)
#ifndef GUSTO_SWEEP_RING
#define GUSTO_SWEEP_RING 4
#endif

// backward: pt_{k-1} = Phicl_k^T pt_k + qq_k, k = N-1..1, pt := p + r (so qq_k = qt_k + r_{k-1}), pt_{N-1} = r_{N-1}.
//           pv[k] holds qq_k on entry and pt_k on exit.
template <class BLKA> GD void backward_sweep_1w(BLKA K) {
    using BLK = std::remove_cv_t<std::remove_reference_t<BLKA>>;   // (a SweepView by value, or a Blk by reference)
    constexpr int n = BLK::n, C = 64 / n, PS = n > 8 ? 4 : 1;
    constexpr bool XL = n > 8;   // 12/13-state models: operands from HBM through the ring below
    double* ex = K.sHh;
    const int tid = K.tid, N = K.N;
    const int g = (tid < C * n) ? tid / n : C - 1, i = (tid < C * n) ? tid % n : 0;
    // DEAD, and kept: nothing reads phc (it was an operand of the branch that rebuilt Phicl from K, which went to the DPP sweeps).
    // Without these lines hipcc emits the same instructions with g and i formed in another order (seen in astrobeeSE3 and in TrajOpt freeflyerSE2 / astrobeeSE3),
    // and the device code would no longer be the byte-for-byte copy it is checked to be (tools/codeobj_diff.py).
    auto phi_e = [&](int r_, int c_) { return (r_ == c_) ? 1.0 : ((c_ == r_ + n / 2) ? K.dt : 0.0); };
    double phc[n];
#pragma unroll
    for (int l = 0; l < n; l++) phc[l] = phi_e(l, i);
    double col[n], coln[n], qv, qvn = 0, pval;
    auto fetch = [&](int k0, double* c, double& q) {
        // (clamped, unconditional loads: a group past the end of the sweep never has its step executed -- the steps are
        // guarded wave-uniformly below -- so its operands only need to be loadable.  As `ok ? load : 0` every load sat
        // in a branch of its own.)
        const int kk = (k0 - g >= 1) ? k0 - g : 1;
        if constexpr (n <= 4) {
            const bool ok = k0 - g >= 1;
#pragma unroll
            for (int l = 0; l < n; l++) c[l] = ok ? K.Phicl[(size_t)kk * BLK::SPH + l * n + i] : 0.0;
            q = ok ? K.pv[kk * n + i] : 0.0;
            return;
        } else {
#pragma unroll
            for (int l = 0; l < n; l++) c[l] = K.Phicl[(size_t)kk * BLK::SPH + l * n + i];
        }
        q = K.pv[kk * n + i];
    };
    // 12/13-state models: the operands come from the workspace in HBM (~3 k cycles away; 540 MB of slot workspaces do not
    // fit the caches), and one chunk of work (~1.2 k cycles) in front of a fetch does not cover that: a ring of RING chunk
    // buffers keeps RING - 1 fetches in flight.  (No buffer is ever copied: a copy waits for the newest fetch.)
    constexpr int RING = XL ? GUSTO_SWEEP_RING : 1;
    static_assert(!BLK::C::PHI_FROM_K, "the kernel whose sweeps rebuild Phicl from K (ONE && PG2) runs backward_sweep_dpp");
    static_assert(!XL || !BLK::C::KD_LDS, "n > 8 always takes the ring: KD_LDS needs n <= 8");
    if constexpr (RING > 1) {
        double cb[RING][n], qb[RING];
#pragma unroll
        for (int d = 0; d < RING - 1; d++) fetch(N - 1 - d * C, cb[d], qb[d]);
        pval = K.rv[(N - 1) * n + i];
        ex[tid] = pval;   // (nothing in this sweep reads it: the vector goes from group to group by v_readlane)
        K.sync();
        if (tid < n) K.pv[(N - 1) * n + tid] = pval;
        for (int kb = N - 1; kb >= 1; kb -= RING * C) {
            static_for<0, RING>([&](auto DD) {
                constexpr int d = decltype(DD)::value;
                const int k0 = kb - d * C;
                fetch(k0 - (RING - 1) * C, cb[(d + RING - 1) % RING], qb[(d + RING - 1) % RING]);   // (clamped: always loadable)
                if (k0 >= 1) {
#pragma unroll
                    for (int gs = 0; gs < C; gs++) {
                        if (k0 - gs >= 1) GUSTO_CHAIN_STEP(pval, qb[d], cb[d], PS)
                    }
                    const int kk = k0 - g;
                    if (tid < C * n && kk >= 1) K.pv[(kk - 1) * n + i] = pval;
                }
            });
        }
        K.sync();
        return;
    }
    fetch(N - 1, col, qv);
    pval = K.rv[(N - 1) * n + i];       // every group starts from pt_{N-1}; only group C-1 is read at step 0
    K.sync();
    if (tid < n) K.pv[(N - 1) * n + tid] = pval;
    for (int k0 = N - 1; k0 >= 1; k0 -= C) {
        if (k0 - C >= 1) fetch(k0 - C, coln, qvn);
#pragma unroll
        for (int gs = 0; gs < C; gs++) {
            if (k0 - gs >= 1) GUSTO_CHAIN_STEP(pval, qv, col, PS)
        }
        {   // group g produced pt_{kk-1}, kk = k0 - g
            const int kk = k0 - g;
            if (tid < C * n && kk >= 1) K.pv[(kk - 1) * n + i] = pval;
        }
#pragma unroll
        for (int l = 0; l < n; l++) col[l] = coln[l];
        qv = qvn;
    }
    K.sync();
}

// forward: dy_k = Phicl_k dy_{k-1} + ct_k, k = 0..N-1; dY[k] holds ct_k on entry and dy_k on exit
template <class BLKA> GD void forward_sweep_1w(BLKA K) {
    using BLK = std::remove_cv_t<std::remove_reference_t<BLKA>>;   // (a SweepView by value, or a Blk by reference)
    constexpr int n = BLK::n, C = 64 / n, PS = n > 8 ? 4 : 1;
    constexpr bool XL = n > 8;
    double* ex = K.sHh;
    const int tid = K.tid, N = K.N;
    const int g = (tid < C * n) ? tid / n : C - 1, i = (tid < C * n) ? tid % n : 0;
    // (DEAD, and kept: as phc in backward_sweep_1w)
    auto phi_e = [&](int r_, int c_) { return (r_ == c_) ? 1.0 : ((c_ == r_ + n / 2) ? K.dt : 0.0); };
    double phr[n];
#pragma unroll
    for (int l = 0; l < n; l++) phr[l] = phi_e(i, l);
    double row[n], rown[n], cv, cvn = 0, yval = 0.0;
    auto fetch = [&](int k0, double* r, double& c) {
        const int kk = (k0 + g < N) ? k0 + g : N - 1;   // (clamped, unconditional loads: as in backward_sweep_1w's fetch)
        if constexpr (n <= 4) {
            const bool ok = k0 + g < N;
#pragma unroll
            for (int l = 0; l < n; l++) r[l] = ok ? K.Phicl[(size_t)kk * BLK::SPH + i * n + l] : 0.0;
            c = ok ? K.dY[kk * n + i] : 0.0;
            return;
        } else {
#pragma unroll
            for (int l = 0; l < n; l++) r[l] = K.Phicl[(size_t)kk * BLK::SPH + i * n + l];
        }
        c = K.dY[kk * n + i];
    };
    constexpr int RING = XL ? GUSTO_SWEEP_RING : 1;
    static_assert(!BLK::C::PHI_FROM_K, "the kernel whose sweeps rebuild Phicl from K (ONE && PG2) runs forward_sweep_dpp");
    static_assert(!XL || !BLK::C::KD_LDS, "n > 8 always takes the ring: KD_LDS needs n <= 8");
    if constexpr (RING > 1) {
        double rb[RING][n], qb[RING];
#pragma unroll
        for (int d = 0; d < RING - 1; d++) fetch(d * C, rb[d], qb[d]);
        ex[tid] = yval;   // (nothing in this sweep reads it, as in backward_sweep_1w)
        K.sync();
        for (int kb = 0; kb < N; kb += RING * C) {
            static_for<0, RING>([&](auto DD) {
                constexpr int d = decltype(DD)::value;
                const int k0 = kb + d * C;
                fetch(k0 + (RING - 1) * C, rb[(d + RING - 1) % RING], qb[(d + RING - 1) % RING]);   // (clamped: always loadable)
                if (k0 < N) {
#pragma unroll
                    for (int gs = 0; gs < C; gs++) {
                        if (k0 + gs < N) GUSTO_CHAIN_STEP(yval, qb[d], rb[d], PS)
                    }
                    const int kk = k0 + g;
                    if (tid < C * n && kk < N) K.dY[kk * n + i] = yval;
                }
            });
        }
        K.sync();
        return;
    }
    fetch(0, row, cv);
    K.sync();
    for (int k0 = 0; k0 < N; k0 += C) {
        if (k0 + C < N) fetch(k0 + C, rown, cvn);
#pragma unroll
        for (int gs = 0; gs < C; gs++) {
            if (k0 + gs < N) GUSTO_CHAIN_STEP(yval, cv, row, PS)
        }
        {
            const int kk = k0 + g;
            if (tid < C * n && kk < N) K.dY[kk * n + i] = yval;
        }
#pragma unroll
        for (int l = 0; l < n; l++) row[l] = rown[l];
        cv = cvn;
    }
    K.sync();
}

// The vector sweeps of the double integrator (n = 6, operands rebuilt from K: LdsC::PHI_FROM_K) on the fp64 DPP broadcast gfx950
// has, `v_fmac_f64_dpp ... row_newbcast:L` (every lane of a row of 16 multiplies by lane L of ITS row), instead of 2 n v_readlane
// per step: in isolation a step is 6 dependent fmac_dpp, 64 cycles against 128 (tools/ub/dpp.hip).  A row holds TWO knot groups,
// A = lanes 0..5 and B = lanes 8..13 (lanes 6, 7, 14, 15 idle on clamped operands): group B takes the vector of the knot before from
// group A's lanes (L = 0..5) and group A from group B's (L = 8..13), no transfer instruction at all.  After B's step the vector hops
// to the B lanes of the next row by one row swap per dword (v_permlane16_swap / v_permlane32_swap, row_hop); the rows take their
// turns in the order 0, 1, 3, 2 -- each of the four hops, the wrap 2 -> 0 at the end of the chunk included, is one of the two
// halves of one swap.  Four rows are 8 groups: a chunk is 8 knots, and as in the readlane sweep lane i of a group forms ITS column
// (row) of Phicl = Phi - Gam K for the group's knot ONCE PER CHUNK, the next chunk's K read from LDS while this one runs.  Every lane
// executes every step; only the group whose turn it is computes on the right vector, the others on stale ones whose results
// nobody reads: the chain register takes the sum unconditionally and the value a group stores is selected OFF the chain.
// Same sums in the same order as backward_sweep_1w / forward_sweep_1w (acc = q, acc = fma(p_l, col_l, acc), l = 0..5): bit-identical.
// (Round 4 built the sweep with the vector REPLICATED in every row, which needs no hops but has every lane form its column per
// knot -- 3 LDS reads, 6 FMAs and the right-hand side, ~29 cycles per knot on top of a 67-cycle step: bit-identical and 35.9 ms
// against 34.1 ms.  The variant without per-knot operands, Phi^T p - K^T (Gam^T p), subtracts two large terms that Phi - Gam K
// cancels entry by entry first: 1.5 % more interior point iterations, lock-step tolerances missed.  Numbers of this version:
// profiles/r08_dpp_sweeps.txt.)
// HOP 0: row 0 -> 1, 1: row 1 -> 3, 2: row 3 -> 2, 3: row 2 -> 0.  x is the vector, g any value that is dead (the vector of the
// step before): the rows that are not a target keep what g held, so no copy of x is made.
template <int HOP> GD double row_hop(double x, double g) {
    const unsigned long long ux = __builtin_bit_cast(unsigned long long, x), ug = __builtin_bit_cast(unsigned long long, g);
    const unsigned xl = (unsigned)ux, xh = (unsigned)(ux >> 32), gl = (unsigned)ug, gh = (unsigned)(ug >> 32);
    unsigned lo, hi;
    if constexpr (HOP == 0) { lo = __builtin_amdgcn_permlane16_swap(gl, xl, false, false)[0]; hi = __builtin_amdgcn_permlane16_swap(gh, xh, false, false)[0]; }
    if constexpr (HOP == 1) { lo = __builtin_amdgcn_permlane32_swap(gl, xl, false, false)[0]; hi = __builtin_amdgcn_permlane32_swap(gh, xh, false, false)[0]; }
    if constexpr (HOP == 2) { lo = __builtin_amdgcn_permlane16_swap(xl, gl, false, false)[1]; hi = __builtin_amdgcn_permlane16_swap(xh, gh, false, false)[1]; }
    if constexpr (HOP == 3) { lo = __builtin_amdgcn_permlane32_swap(xl, gl, false, false)[1]; hi = __builtin_amdgcn_permlane32_swap(xh, gh, false, false)[1]; }
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// q + sum_l p[lane 8 HALF + l of the row] c[l], l = 0..5 in this order.  (One asm block: the fp64 DPP form has no builtin, and the
// 2 wait states between the VALU write of p -- the step before, or the hop -- and its first DPP read are the s_nop in the string.)
template <int HALF> GD double dpp_step6(double p, double q, const double* c) {
    double acc = q;
    if constexpr (HALF == 0)
        asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\tv_fmac_f64_dpp %0, %1, %3 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f64_dpp %0, %1, %4 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\tv_fmac_f64_dpp %0, %1, %5 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f64_dpp %0, %1, %6 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\tv_fmac_f64_dpp %0, %1, %7 row_newbcast:5 row_mask:0xf bank_mask:0xf"
            : "+v"(acc) : "v"(p), "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]));
    else
        asm("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:8 row_mask:0xf bank_mask:0xf\n\tv_fmac_f64_dpp %0, %1, %3 row_newbcast:9 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f64_dpp %0, %1, %4 row_newbcast:10 row_mask:0xf bank_mask:0xf\n\tv_fmac_f64_dpp %0, %1, %5 row_newbcast:11 row_mask:0xf bank_mask:0xf\n\t"
            "v_fmac_f64_dpp %0, %1, %6 row_newbcast:12 row_mask:0xf bank_mask:0xf\n\tv_fmac_f64_dpp %0, %1, %7 row_newbcast:13 row_mask:0xf bank_mask:0xf"
            : "+v"(acc) : "v"(p), "v"(c[0]), "v"(c[1]), "v"(c[2]), "v"(c[3]), "v"(c[4]), "v"(c[5]));
    return acc;
}
// one chunk of up to 8 steps: step gs is group gs's (2 turn + half), from the vector group gs - 1 left -- group 7 of the chunk before
// at gs = 0.  `live(gs)` is wave-uniform: the steps past the end of the sweep are not executed.
template <class LIVE> GD void dpp_chunk(double& p, double& keep, double q, const double* c, int g, LIVE live) {
    static_for<0, 8>([&](auto GS) {
        constexpr int gs = decltype(GS)::value;
        if (live(gs)) {
            const double acc = dpp_step6<(gs & 1) ? 0 : 1>(p, q, c);
            keep = (g == gs) ? acc : keep;
            if constexpr (gs & 1) p = row_hop<gs / 2>(acc, p); else p = acc;
        }
    });
}
// pt_{k-1} = Phicl_k^T pt_k + q_k, k = N-1..1 (the recurrence of backward_sweep_1w, in its order of loads and stores)
template <class BLKA> GD void backward_sweep_dpp(BLKA K) {
    using BLK = std::remove_cv_t<std::remove_reference_t<BLKA>>;
    constexpr int n = BLK::n, m = BLK::m, C = 8;
    static_assert(n == 6 && BLK::C::PHI_FROM_K, "two groups of 6 lanes per row, operands from K");
    const int tid = K.tid, N = K.N;
    const int row = tid >> 4, j = tid & 15;
    const bool act = (j & 7) < n;
    const int g = 2 * (row ^ (row >> 1)) + (j >> 3), i = act ? (j & 7) : 0;   // (turn of the rows 0, 1, 3, 2: 0, 1, 2, 3)
    double gl[n];
    auto phi_e = [&](int r_, int c_) { return (r_ == c_) ? 1.0 : ((c_ == r_ + n / 2) ? K.dt : 0.0); };
    {
        double Bd[n * m];
        Dyn<BLK::MODEL_ID>::B(*K.mpp, Bd);
        const double h = 0.5 * K.dt;
#pragma unroll
        for (int l = 0; l < n; l++) {
            const int c_ = l % m;
            const double hb = h * Bd[(c_ + n / 2) * m + c_];
            gl[l] = (l < n / 2) ? 2.0 * (h * hb) : 2.0 * hb;
        }
    }
    double phc[n];   // column i of Phi
#pragma unroll
    for (int l = 0; l < n; l++) phc[l] = phi_e(l, i);
    double col[n], kc[m], qv, qvn, p, keep = 0.0;
    // the operands of a chunk in two halves: the LDS reads (clamped, unconditional: always loadable) are issued a whole chunk
    // ahead, the FMAs that form the column from them come behind the chunk's steps -- in front of them they waited out the LDS
    // round trip once per chunk
    auto load = [&](int k0, double& q) {
        const int kk = (k0 - g >= 1) ? k0 - g : 1;
#pragma unroll
        for (int a = 0; a < m; a++) kc[a] = K.kdl[kk * BLK::C::KDS + a * n + i];
        q = K.pv[kk * n + i];
    };
    auto form = [&]() {
#pragma unroll
        for (int l = 0; l < n; l++) col[l] = phc[l] - gl[l] * kc[l % m];
    };
    load(N - 1, qv);
    form();
    p = K.rv[(N - 1) * n + i];          // every group starts from pt_{N-1}; step 0 reads the B lanes of row 0
    K.sync();
    if (tid < n) K.pv[(N - 1) * n + tid] = p;
    for (int k0 = N - 1; k0 >= 1; k0 -= C) {
        load(k0 - C, qvn);
        if (k0 - (C - 1) >= 1) dpp_chunk(p, keep, qv, col, g, [](int) { return true; });   // (a whole chunk: no branch per step)
        else dpp_chunk(p, keep, qv, col, g, [&](int gs) { return k0 - gs >= 1; });
        {   // group g produced pt_{kk-1}, kk = k0 - g
            const int kk = k0 - g;
            if (act && kk >= 1) K.pv[(kk - 1) * n + i] = keep;
        }
        __builtin_amdgcn_sched_barrier(0);
        form();
        qv = qvn;
    }
    K.sync();
}
// dy_k = Phicl_k dy_{k-1} + ct_k, k = 0..N-1, dy_{-1} = 0 (the recurrence of forward_sweep_1w)
template <class BLKA> GD void forward_sweep_dpp(BLKA K) {
    using BLK = std::remove_cv_t<std::remove_reference_t<BLKA>>;
    constexpr int n = BLK::n, m = BLK::m, C = 8;
    static_assert(n == 6 && BLK::C::PHI_FROM_K, "two groups of 6 lanes per row, operands from K");
    const int tid = K.tid, N = K.N;
    const int row = tid >> 4, j = tid & 15;
    const bool act = (j & 7) < n;
    const int g = 2 * (row ^ (row >> 1)) + (j >> 3), i = act ? (j & 7) : 0;   // (see backward_sweep_dpp)
    double gi = 0.0;
    auto phi_e = [&](int r_, int c_) { return (r_ == c_) ? 1.0 : ((c_ == r_ + n / 2) ? K.dt : 0.0); };
    {
        double Bd[n * m];
        Dyn<BLK::MODEL_ID>::B(*K.mpp, Bd);
        const double h = 0.5 * K.dt;
#pragma unroll
        for (int l = 0; l < n; l++) {   // Gam[i][i mod m] of this lane's row
            const int c_ = l % m;
            const double hb = h * Bd[(c_ + n / 2) * m + c_];
            const double gv = (l < n / 2) ? 2.0 * (h * hb) : 2.0 * hb;
            gi = (i == l) ? gv : gi;
        }
    }
    double phr[n];   // row i of Phi
#pragma unroll
    for (int l = 0; l < n; l++) phr[l] = phi_e(i, l);
    double rw[n], kr[n], cv, cvn, p = 0.0, keep = 0.0;
    auto load = [&](int k0, double& c) {   // (see backward_sweep_dpp)
        const int kk = (k0 + g < N) ? k0 + g : N - 1;
        const int ic = (i < m) ? i : i - m;
#pragma unroll
        for (int l = 0; l < n; l++) kr[l] = K.kdl[kk * BLK::C::KDS + ic * n + l];
        c = K.dY[kk * n + i];
    };
    auto form = [&]() {
#pragma unroll
        for (int l = 0; l < n; l++) rw[l] = phr[l] - gi * kr[l];
    };
    load(0, cv);
    form();
    K.sync();
    for (int k0 = 0; k0 < N; k0 += C) {
        load(k0 + C, cvn);
        if (k0 + C - 1 < N) dpp_chunk(p, keep, cv, rw, g, [](int) { return true; });
        else dpp_chunk(p, keep, cv, rw, g, [&](int gs) { return k0 + gs < N; });
        {
            const int kk = k0 + g;
            if (act && kk < N) K.dY[kk * n + i] = keep;
        }
        __builtin_amdgcn_sched_barrier(0);
        form();
        cv = cvn;
    }
    K.sync();
}

// nu_{k+1} = P_k dy_k + p_k + Pi_k mu_g of every knot (the new costates of the corrector), for the 12/13-state models by
// groups of n lanes: lane i of group g forms row i for knot k0 + g from ITS rows of the P_k and Pi_k records (stored transposed:
// the lanes of a group read consecutive doubles), the next chunk's rows in flight while this one is summed.  A load
// instruction then touches one line of each of C = 64 / n records; with a
// lane per knot (step_phase) each of the 2 n^2 loads of the walk touched 50 records -- ~230 cycles apiece through the
// texture addresser, 80 k of the 1.08 M cycles of a KKT solve.  Same sums in the same order as step_phase.
template <int MODEL> GD void costate_pass_1w(SweepView<MODEL> K, const double* mugn) {
    using T = MT<MODEL>;
    using R = Rec<MODEL>;
    constexpr int n = T::n, C = 64 / n;
    const int tid = K.tid, N = K.N;
    const int g = (tid < C * n) ? tid / n : C - 1, i = (tid < C * n) ? tid % n : 0;
    double mg[n];
#pragma unroll
    for (int l = 0; l < n; l++) mg[l] = mugn[l];
    constexpr int RING = GUSTO_SWEEP_RING;   // chunk buffers: RING - 1 fetches in flight (backward_sweep_1w says why)
    double pr[RING][n], pi[RING][n];
    auto fetch = [&](int k0, double* a, double* b) {
        const int k = (k0 + g + 1 < N) ? k0 + g : N - 2;   // (clamped: no load under a branch)
        // (records stored transposed by factor_sweep_mfma: entry (i, l) at l n + i; row-major by the VALU sweep of a
        // -DGUSTO_USE_MFMA=false build)
        const double* pa = K.Paft + (size_t)k * R::SNN + (T::MFMA ? i : i * n);
        const double* pb = K.Piaft + (size_t)k * R::SNN + (T::MFMA ? i : i * n);
#pragma unroll
        for (int l = 0; l < n; l++) { a[l] = pa[T::MFMA ? l * n : l]; b[l] = pb[T::MFMA ? l * n : l]; }
    };
#pragma unroll
    for (int d = 0; d < RING - 1; d++) fetch(d * C, pr[d], pi[d]);
    for (int kb = 0; kb + 1 < N; kb += RING * C) {
        static_for<0, RING>([&](auto DD) {
            constexpr int d = decltype(DD)::value;
            const int k0 = kb + d * C;
            fetch(k0 + (RING - 1) * C, pr[(d + RING - 1) % RING], pi[(d + RING - 1) % RING]);
            if (k0 + 1 < N) {
                const bool ok = tid < C * n && k0 + g + 1 < N;
                const int k = (k0 + g + 1 < N) ? k0 + g : N - 2;
                double s = K.pv[k * n + i] - K.rv[k * n + i];
#pragma unroll
                for (int l = 0; l < n; l++) s += pr[d][l] * K.dY[k * n + l] + pi[d][l] * mg[l];
                if (ok) K.nun[(k + 1) * n + i] = s;
            }
        });
    }
    K.sync();
}

// Adjoint recursion of the new costates (costate_adjoint): nu_k = Phi_k^T nu_{k+1} + v_k, k = N-2 .. 1, nu_{N-1} = v_{N-1};
// nun[k] holds v_k on entry (step_phase) and nu_k on exit.  Phi_k = 2 M_k - I is the block linearize() stored; of its column
// i only the structural nonzeros are fetched (x = (r, v, attitude, w): M is block upper triangular, MT::Mnz -- one or two
// entries for a position / velocity column, the attitude and rate rows for the others): 36 / 46 doubles per knot instead
// of the 2 n^2 of the P | Pi records.  Groups of n lanes hold consecutive knots as in backward_sweep_1w; the n-vector travels
// between groups through 64 doubles of LDS (each lane needs ITS rows of it: a per-lane address, not a broadcast).
template <int MODEL> constexpr bool adjoint_pattern_ok() {   // the column pattern adjoint_sweep_1w assumes IS MT::Mnz
    using T = MT<MODEL>;
    constexpr int n = T::n, q = n - 9;
    for (int i = 0; i < n; i++)
        for (int l = 0; l < n; l++) {
            const bool want = (i < 6) ? (l == i || (i >= 3 && l == i - 3)) : (l >= 6 && l < ((i < 6 + q) ? 6 + q : n));
            if (want != T::Mnz(l, i)) return false;
        }
    return true;
}
template <int MODEL> GD void adjoint_sweep_1w(SweepView<MODEL> K) {
    using T = MT<MODEL>;
    constexpr int n = T::n, NZ = T::n + T::m, C = 64 / n, q = n - 9, NR = n - 6;
    static_assert(adjoint_pattern_ok<MODEL>(), "column pattern of M of the astrobee models");
    const int tid = K.tid, N = K.N;
    const int g = (tid < C * n) ? tid / n : C - 1, i = (tid < C * n) ? tid % n : 0;
    // rows of column i: {i} and {i - 3} below the attitude block, else rows 6 .. hi - 1, hi = 6 + q for an attitude column, n for a rate column
    int rl[NR];
    bool rok[NR];
    const int hi = (i < 6 + q) ? 6 + q : n;
#pragma unroll
    for (int j = 0; j < NR; j++) {
        rl[j] = (i < 6) ? ((j == 1 && i >= 3) ? i - 3 : i) : 6 + j;
        rok[j] = (i < 6) ? (j == 0 || (j == 1 && i >= 3)) : (6 + j < hi);
        if (!rok[j]) rl[j] = i;
    }
    // where those entries sit in the compact record (SpPG: Phi column by column, rows ascending): column start + rank
    int cs = 0, pj[NR];
#pragma unroll
    for (int i2 = 0; i2 < n; i2++) cs = (i == i2) ? SpPG<MODEL>::pos_phi(0, i2) : cs;
#pragma unroll
    for (int j = 0; j < NR; j++) pj[j] = (i < 6) ? ((i >= 3) ? (j == 1 ? 0 : (j == 0 ? 1 : 0)) : 0) : (rok[j] ? j : 0);
    double* ex = K.sHh;
    constexpr int RING = GUSTO_SWEEP_RING;
    double cb[RING][NR], vb[RING];
    auto fetch = [&](int k0, double* c, double& v) {
        const int kk = (k0 - g >= 1) ? k0 - g : 1;      // (clamped: always loadable, never used past the end)
        const auto pg = K.PGS + (size_t)kk * SpPG<MODEL>::S + cs;   // (column i of Phi_kk: consecutive entries of the compact record)
#pragma unroll
        for (int j = 0; j < NR; j++) { const double a = pg[pj[j]]; c[j] = rok[j] ? a : 0.0; }
        v = K.nun[kk * n + i];
    };
#pragma unroll
    for (int d = 0; d < RING - 1; d++) fetch(N - 2 - d * C, cb[d], vb[d]);
    double val = K.nun[(N - 1) * n + i];       // every group starts from nu_{N-1}; only group C - 1 is read at step 0
    ex[tid] = val;
    K.sync();
    for (int kb = N - 2; kb >= 1; kb -= RING * C) {
        static_for<0, RING>([&](auto DD) {
            constexpr int d = decltype(DD)::value;
            const int k0 = kb - d * C;
            fetch(k0 - (RING - 1) * C, cb[(d + RING - 1) % RING], vb[(d + RING - 1) % RING]);
            if (k0 >= 1) {
#pragma unroll
                for (int gs = 0; gs < C; gs++) {
                    if (k0 - gs >= 1) {
                        const int sg = (gs == 0) ? C - 1 : gs - 1;
                        double pb[NR];
#pragma unroll
                        for (int j = 0; j < NR; j++) pb[j] = ex[sg * n + rl[j]];
                        double s = vb[d];
#pragma unroll
                        for (int j = 0; j < NR; j++) s += cb[d][j] * pb[j];
                        val = (g == gs) ? s : val;
                        ex[tid] = val;
                    }
                }
                const int kk = k0 - g;
                if (tid < C * n && kk >= 1) K.nun[kk * n + i] = val;
            }
        });
    }
    K.sync();
}

// p_{k-1} = Phicl_k^T (p_k + r_k) + qt_k, k = N-1..1; pv[k] holds qt_k on entry and p_k on exit
template <class BLK> GD void backward_sweep_mw(BLK& K) {
    // pt_{k-1} = Phicl_k^T pt_k + qq_k (pt = p + r, qq_k = qt_k + r_{k-1}); pv[k]: qq_k on entry, pt_k on exit
    constexpr int n = BLK::n;
    using R = typename BLK::R;
    const int tid = K.tid, N = K.N;
    double p = 0.0, col[n], coln[n];
#pragma unroll
    for (int l = 0; l < n; l++) { col[l] = 0; coln[l] = 0; }
    if (tid < n) {
#pragma unroll
        for (int l = 0; l < n; l++) col[l] = K.Phicl[(size_t)(N - 1) * R::SNN + l * n + tid];
        p = K.rv[(N - 1) * n + tid];
    }
    for (int k = N - 1; k >= 1; k--) {
        double* buf = K.sT + (k & 1) * n;
        if (tid < n) {
            if (k > 1) {
#pragma unroll
                for (int l = 0; l < n; l++) coln[l] = K.Phicl[(size_t)(k - 1) * R::SNN + l * n + tid];
            }
            buf[tid] = p;
        }
        K.sync();
        if (tid < n) {
            double s = K.pv[k * n + tid], v[n];
#pragma unroll
            for (int l = 0; l < n; l++) v[l] = buf[l];
            __builtin_amdgcn_sched_barrier(0);
            K.pv[k * n + tid] = p;
#pragma unroll
            for (int l = 0; l < n; l++) s += col[l] * v[l];
            p = s;
#pragma unroll
            for (int l = 0; l < n; l++) col[l] = coln[l];
        }
    }
    if (tid < n) K.pv[tid] = p;
    K.sync();
}

// dy_k = Phicl_k dy_{k-1} + ct_k, k = 0..N-1; dY[k] holds ct_k on entry and dy_k on exit
template <class BLK> GD void forward_sweep_mw(BLK& K) {
    constexpr int n = BLK::n;
    using R = typename BLK::R;
    const int tid = K.tid, N = K.N;
    double y = 0.0, row[n], rown[n];
#pragma unroll
    for (int l = 0; l < n; l++) { row[l] = 0; rown[l] = 0; }
    if (tid < n) {
#pragma unroll
        for (int l = 0; l < n; l++) row[l] = K.Phicl[(size_t)tid * n + l];
    }
    for (int k = 0; k < N; k++) {
        double* buf = K.sT + (k & 1) * n;
        if (tid < n) {
            if (k + 1 < N) {
#pragma unroll
                for (int l = 0; l < n; l++) rown[l] = K.Phicl[(size_t)(k + 1) * R::SNN + tid * n + l];
            }
            buf[tid] = y;
        }
        K.sync();
        if (tid < n) {
            double s = K.dY[k * n + tid], v[n];
#pragma unroll
            for (int l = 0; l < n; l++) v[l] = buf[l];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int l = 0; l < n; l++) s += row[l] * v[l];
            y = s;
            K.dY[k * n + tid] = y;
#pragma unroll
            for (int l = 0; l < n; l++) row[l] = rown[l];
        }
    }
    K.sync();
}
}  // namespace gusto
