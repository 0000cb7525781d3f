#include <hip/hip_runtime.h>
#include <cstdio>
// one wave: cycles per instruction of the fp64 DPP forms gfx950 has (v_fmac_f64_dpp row_newbcast, v_mov_b64_dpp row_shr / row_newbcast)
// against plain fma and the v_readlane pair they replace; and (kernel k2) what a vector sweep on them needs to move its n-vector
// from one row of 16 lanes to the next: the gfx950 row swaps (v_permlane16_swap / v_permlane32_swap) against a round trip through
// LDS, and a whole 8-knot chunk of the sweep -- two groups of 6 lanes per row, rows in the order 0, 1, 3, 2 -- against 8 steps of
// the readlane form.  Exits non-zero if a hop does not land where the sweep expects it.
#define T0() asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); __builtin_amdgcn_sched_barrier(0); t0 = clock64(); __builtin_amdgcn_sched_barrier(0)
#define T1(slot) asm volatile("" : "+v"(a), "+v"(b), "+v"(c), "+v"(d)); __builtin_amdgcn_sched_barrier(0); t1 = clock64(); __builtin_amdgcn_sched_barrier(0); if (t == 0) out[slot] = t1 - t0
__global__ void k(long long* out, double* sink, double x0) {
    const int t = threadIdx.x;
    double a = x0 + t * 1e-3, b = x0 * 1.1, c = x0 * 1.2, d = x0 * 1.3, m = 1.0000001, q = 1e-9;
    long long t0, t1;
    T0();   // 0: 256 dependent plain fma
#pragma unroll
    for (int i = 0; i < 256; i++) a = __builtin_fma(a, m, q);
    T1(0);
    T0();   // 1: 256 dependent fmac_dpp (acc chain, source b constant): acc += bcast(b, 3) * m
#pragma unroll
    for (int i = 0; i < 256; i++) asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(a) : "v"(b), "v"(m));
    T1(1);
    T0();   // 2: 256 fmac_dpp, 4 independent accumulators
#pragma unroll
    for (int i = 0; i < 64; i++) {
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(a) : "v"(q), "v"(m));
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:2 row_mask:0xf bank_mask:0xf" : "+v"(b) : "v"(q), "v"(m));
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:1 row_mask:0xf bank_mask:0xf" : "+v"(c) : "v"(q), "v"(m));
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf" : "+v"(d) : "v"(q), "v"(m));
    }
    T1(2);
    T0();   // 3: 128 steps of the recurrence pattern: the DPP source is the previous result (write -> s_nop 1 -> dpp read)
#pragma unroll
    for (int i = 0; i < 128; i++) {
        double acc = q;
        asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(m));
        a = acc;
    }
    T1(3);
    T0();   // 4: 128 x (v_mov_b64_dpp row_shr:3 then fma with it), dependent
#pragma unroll
    for (int i = 0; i < 128; i++) {
        unsigned long long u = __builtin_bit_cast(unsigned long long, a);
        unsigned lo = (unsigned)u, hi = (unsigned)(u >> 32), lo2, hi2;
        asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %2 row_shr:3 row_mask:0xf bank_mask:0xf\n\tv_mov_b32_dpp %1, %3 row_shr:3 row_mask:0xf bank_mask:0xf" : "=&v"(lo2), "=&v"(hi2) : "v"(lo), "v"(hi));
        a = __builtin_fma(__builtin_bit_cast(double, ((unsigned long long)hi2 << 32) | lo2), m, q);
    }
    T1(4);
    T0();   // 5: 128 x (two v_readlane + fma), dependent: what the sweeps do today
#pragma unroll
    for (int i = 0; i < 128; i++) {
        unsigned long long u = __builtin_bit_cast(unsigned long long, a);
        unsigned lo = __builtin_amdgcn_readlane((int)(u & 0xffffffffu), 3), hi = __builtin_amdgcn_readlane((int)(u >> 32), 3);
        a = __builtin_fma(b, __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo), q);
    }
    T1(5);
    T0();   // 6: one recurrence step of n = 6 as the sweep would issue it, 64 times: 6 fmac_dpp on one accumulator from the previous vector
#pragma unroll
    for (int i = 0; i < 64; i++) {
        double acc = q;
        asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:0 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(m));
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:1 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(b));
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:2 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(c));
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(d));
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:4 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(m));
        asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:5 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(a), "v"(b));
        a = acc * 1e-3;
    }
    T1(6);
    T0();   // 7: the same step with 12 readlanes + 6 fma
#pragma unroll
    for (int i = 0; i < 64; i++) {
        double acc = q;
#pragma unroll
        for (int l = 0; l < 6; l++) {
            unsigned long long u = __builtin_bit_cast(unsigned long long, a);
            unsigned lo = __builtin_amdgcn_readlane((int)(u & 0xffffffffu), l), hi = __builtin_amdgcn_readlane((int)(u >> 32), l);
            acc = __builtin_fma(l & 1 ? b : m, __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo), acc);
        }
        a = acc * 1e-3;
    }
    T1(7);
    sink[t] = a + b + c + d;
    // correctness of the broadcast: every lane of a row gets lane L of ITS row
    double v = (double)t, r = 0.0;
    asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:5 row_mask:0xf bank_mask:0xf" : "+v"(r) : "v"(v), "v"(m));
    sink[64 + t] = r;
}

// ---- the row hops ----
// With vdst = G (anything) and src = X:  permlane16_swap: r[0] rows 1, 3 = X rows 0, 2;  r[1] (vdst = X, src = G) rows 0, 2 = X rows 1, 3
//                                        permlane32_swap: r[0] rows 2, 3 = X rows 0, 1;  r[1] (vdst = X, src = G) rows 0, 1 = X rows 2, 3
// HOP 0: row 0 -> 1 (and 2 -> 3), 1: row 1 -> 3 (and 0 -> 2), 2: row 3 -> 2 (and 1 -> 0), 3: row 2 -> 0 (and 3 -> 1).  The rows that are
// not a target keep what G held: no copy of X is needed, and G (the vector of the step before) is dead anyway.
template <int HOP> __device__ __forceinline__ double hop(double x, double g) {
    const unsigned long long ux = __builtin_bit_cast(unsigned long long, x), ug = __builtin_bit_cast(unsigned long long, g);
    const unsigned xl = (unsigned)ux, xh = (unsigned)(ux >> 32), gl = (unsigned)ug, gh = (unsigned)(ug >> 32);
    unsigned lo, hi;
    if constexpr (HOP == 0) { lo = __builtin_amdgcn_permlane16_swap(gl, xl, false, false)[0]; hi = __builtin_amdgcn_permlane16_swap(gh, xh, false, false)[0]; }
    if constexpr (HOP == 1) { lo = __builtin_amdgcn_permlane32_swap(gl, xl, false, false)[0]; hi = __builtin_amdgcn_permlane32_swap(gh, xh, false, false)[0]; }
    if constexpr (HOP == 2) { lo = __builtin_amdgcn_permlane16_swap(xl, gl, false, false)[1]; hi = __builtin_amdgcn_permlane16_swap(xh, gh, false, false)[1]; }
    if constexpr (HOP == 3) { lo = __builtin_amdgcn_permlane32_swap(xl, gl, false, false)[1]; hi = __builtin_amdgcn_permlane32_swap(xh, gh, false, false)[1]; }
    return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);
}
// one step of the sweep: acc = q + sum_l bcast(p, lane 8 HALF + l of the row) * c[l], l = 0..5 in this order
template <int HALF> __device__ __forceinline__ double step6(double p, double q, const double* c) {
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
// a chunk of 8 knots: group gs = 2 turn + half (turn of the rows 0, 1, 3, 2 = 0, 1, 2, 3) does step gs from the vector group gs - 1 left
// (group 7 of the chunk before at gs = 0: the wrap hop closes the chunk)
__device__ __forceinline__ void chunk8(double& p, double& keep, double q, const double* c, int g) {
    double acc;
#define STEP(gs) acc = step6<((gs) & 1) ? 0 : 1>(p, q, c); keep = (g == (gs)) ? acc : keep
    STEP(0); p = acc; STEP(1); p = hop<0>(acc, p);
    STEP(2); p = acc; STEP(3); p = hop<1>(acc, p);
    STEP(4); p = acc; STEP(5); p = hop<2>(acc, p);
    STEP(6); p = acc; STEP(7); p = hop<3>(acc, p);
#undef STEP
}
#define U0() asm volatile("" : "+v"(a), "+v"(b)); __builtin_amdgcn_sched_barrier(0); t0 = clock64(); __builtin_amdgcn_sched_barrier(0)
#define U1(slot) asm volatile("" : "+v"(a), "+v"(b)); __builtin_amdgcn_sched_barrier(0); t1 = clock64(); __builtin_amdgcn_sched_barrier(0); if (t == 0) out[slot] = t1 - t0
#define DPP1(acc, src) asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %1, %2 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(m))
__global__ void k2(long long* out, double* sink, double x0) {
    __shared__ double ex[64];
    const int t = threadIdx.x;
    double a = x0 + t * 1e-3, b = x0 * 1.1 + t, m = 1.0000001, q = 1e-9;
    long long t0, t1;
    // 0: the chain without a hop: VALU write (fma) -> DPP read (fmac_dpp), 64 times
    U0();
#pragma unroll
    for (int i = 0; i < 64; i++) { a = __builtin_fma(a, m, q); double acc = q; DPP1(acc, a); b = a; a = acc; }
    U1(0);
    // 1..4: the same with hop 0..3 between the write and the DPP read
#define HOPT(H) U0(); _Pragma("unroll") for (int i = 0; i < 64; i++) { a = __builtin_fma(a, m, q); const double h = hop<H>(a, b); double acc = q; DPP1(acc, h); b = h; a = acc; } U1(1 + H)
    HOPT(0); HOPT(1); HOPT(2); HOPT(3);
    // 5: the hop through LDS: one ds_write_b64, one ds_read_b64 of the lane 16 below (what the 12/13-state sweeps pay per knot)
    U0();
#pragma unroll
    for (int i = 0; i < 64; i++) {
        a = __builtin_fma(a, m, q);
        *(volatile double*)&ex[t] = a;
        const double h = *(volatile double*)&ex[(t + 48) & 63];
        double acc = q; DPP1(acc, h); b = h; a = acc;
    }
    U1(5);
    sink[t] = a + b;
    // 6: 16 chunks of 8 knots as proposed (6 fmac_dpp per step, a hop every second step, the stored value selected off the chain)
    const int row = t >> 4, j = t & 15, g = 2 * (row == 0 ? 0 : row == 1 ? 1 : row == 3 ? 2 : 3) + (j >> 3);
    double c[6];
#pragma unroll
    for (int l = 0; l < 6; l++) c[l] = x0 * 0.1 + 1e-3 * l + 1e-4 * t;
    double p = a * 1e-3, keep = 0.0;
    a = p;
    U0(); p = a;
    for (int i = 0; i < 16; i++) chunk8(p, keep, q, c, g);
    a = p; U1(6);
    sink[64 + t] = a + keep;
    // 7: 128 steps of the readlane form (10 groups of 6 lanes: 12 v_readlane into scalar pairs, 6 dependent fma, a select)
    const int g10 = t < 60 ? t / 6 : 9;
    double pval = a * 1e-3;
    a = pval;
    U0(); pval = a;
    for (int i = 0; i < 16; i++) {
#pragma unroll
        for (int gs = 0; gs < 8; gs++) {
            const int sg = gs == 0 ? 9 : gs - 1;
            double pb[6], acc = q;
            const unsigned long long u = __builtin_bit_cast(unsigned long long, pval);
#pragma unroll
            for (int l = 0; l < 6; l++)
                pb[l] = __builtin_bit_cast(double, ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(u >> 32), sg * 6 + l) << 32) |
                                                    (unsigned)__builtin_amdgcn_readlane((int)(u & 0xffffffffu), sg * 6 + l));
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int l = 0; l < 6; l++) acc += c[l] * pb[l];
            pval = (g10 == gs) ? acc : pval;
        }
    }
    a = pval; U1(7);
    sink[128 + t] = a;
    // lane-id checks.  sink[192 + 64 H + t]: hop H of the lane ids (the other operand: -1)
    {
        const double v = (double)t, G = -1.0;
        sink[192 + t] = hop<0>(v, G); sink[256 + t] = hop<1>(v, G); sink[320 + t] = hop<2>(v, G); sink[384 + t] = hop<3>(v, G);
    }
    // ... and the chain of two chunks with unit operands: lane i of a group takes element i of the vector before and adds 1, so group
    // gs of chunk ch must end with 8 ch + gs + 1 in its six lanes -- the vector went 0A 0B 1A 1B 3A 3B 2A 2B and back to 0A
    {
        const int i = (j & 7) < 6 ? (j & 7) : 0;
        double e[6];
#pragma unroll
        for (int l = 0; l < 6; l++) e[l] = (l == i) ? 1.0 : 0.0;
        double pp = 0.0, k0 = -1.0, k1 = -1.0;
        chunk8(pp, k0, 1.0, e, g);
        chunk8(pp, k1, 1.0, e, g);
        sink[448 + t] = k0; sink[512 + t] = k1;
    }
}
// ---- k3: six doubles of a row to every lane of the row (H_uu to the Cholesky of the factor stage) ----
// One round hands the six doubles held by lanes 0 .. 5 of each row of 16 to every lane of that row and runs three dependent FMAs on
// them; the value the next round hands on is that result, so eight rounds are one dependent chain.  V = 0: 12 v_readlane_b32 (lanes
// 39 .. 44 of the wave, what factor_sweep_pg2 does), 1: six v_mov_b64_dpp row_newbcast:q, 2: 12 v_mov_b32_dpp row_newbcast:q as
// __builtin_amdgcn_update_dpp(.., 0x150 + q, ..) emits them (hazards and order left to the compiler).
template <int Q> __device__ __forceinline__ double bcast_b32x2(double x) {
    const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
    const int lo = (int)(u & 0xffffffffu), hi = (int)(u >> 32);
    const unsigned rl = (unsigned)__builtin_amdgcn_update_dpp(0, lo, 0x150 + Q, 0xf, 0xf, true);
    const unsigned rh = (unsigned)__builtin_amdgcn_update_dpp(0, hi, 0x150 + Q, 0xf, 0xf, true);
    return __builtin_bit_cast(double, ((unsigned long long)rh << 32) | rl);
}
template <int V> __device__ __forceinline__ void six(double x, double* s) {
    if constexpr (V == 0) {
        const unsigned long long u = __builtin_bit_cast(unsigned long long, x);
#pragma unroll
        for (int q = 0; q < 6; q++)
            s[q] = __builtin_bit_cast(double, ((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(u >> 32), 39 + q) << 32) |
                                               (unsigned)__builtin_amdgcn_readlane((int)(u & 0xffffffffu), 39 + q));
    } else if constexpr (V == 1) {
        asm("s_nop 1\n\tv_mov_b64_dpp %0, %6 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\tv_mov_b64_dpp %1, %6 row_newbcast:1 row_mask:0xf bank_mask:0xf\n\t"
            "v_mov_b64_dpp %2, %6 row_newbcast:2 row_mask:0xf bank_mask:0xf\n\tv_mov_b64_dpp %3, %6 row_newbcast:3 row_mask:0xf bank_mask:0xf\n\t"
            "v_mov_b64_dpp %4, %6 row_newbcast:4 row_mask:0xf bank_mask:0xf\n\tv_mov_b64_dpp %5, %6 row_newbcast:5 row_mask:0xf bank_mask:0xf"
            : "=&v"(s[0]), "=&v"(s[1]), "=&v"(s[2]), "=&v"(s[3]), "=&v"(s[4]), "=&v"(s[5]) : "v"(x));
    } else {
        s[0] = bcast_b32x2<0>(x); s[1] = bcast_b32x2<1>(x); s[2] = bcast_b32x2<2>(x);
        s[3] = bcast_b32x2<3>(x); s[4] = bcast_b32x2<4>(x); s[5] = bcast_b32x2<5>(x);
    }
}
template <int V> __device__ __forceinline__ double rounds8(double x, double w) {
#pragma unroll
    for (int r = 0; r < 8; r++) {
        double s[6];
        six<V>(x, s);
        double f = __builtin_fma(s[0], s[1], s[2]);
        f = __builtin_fma(f, s[3], s[4]);
        x = __builtin_fma(f, w, s[5]);   // (every lane's next value: the chain goes on through all six)
    }
    return x;
}
__global__ void k3(long long* out, double* sink, double x0) {
    const int t = threadIdx.x;
    double a = x0 + t * 1e-3, b = 1e-3;
    long long t0, t1;
    U0(); a = rounds8<0>(a, b); U1(0);
    U0(); a = rounds8<1>(a, b); U1(1);
    U0(); a = rounds8<2>(a, b); U1(2);
    sink[t] = a;
    // where the values land: the six doubles of the lane ids
    double s[6];
    const double v = (double)t;
    six<0>(v, s);
#pragma unroll
    for (int q = 0; q < 6; q++) sink[64 * (1 + q) + t] = s[q];
    six<1>(v, s);
#pragma unroll
    for (int q = 0; q < 6; q++) sink[64 * (7 + q) + t] = s[q];
    six<2>(v, s);
#pragma unroll
    for (int q = 0; q < 6; q++) sink[64 * (13 + q) + t] = s[q];
}
int main() {
    long long* out; double* sink;
    hipMalloc(&out, 16 * sizeof(long long)); hipMalloc(&sink, 1280 * sizeof(double));
    for (int rep = 0; rep < 2; rep++) hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, out, sink, 1.0);
    hipDeviceSynchronize();
    long long h[16]; double s[128];
    hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost); hipMemcpy(s, sink, sizeof(s), hipMemcpyDeviceToHost);
    const char* nm[] = {"256 dep fma", "256 dep fmac_dpp (acc chain)", "256 fmac_dpp, 4 accumulators", "128 recurrence fmac_dpp (src = prev result)",
                        "128 x (2 mov_b32_dpp row_shr + fma)", "128 x (2 readlane + fma)", "64 steps n=6: 6 fmac_dpp", "64 steps n=6: 12 readlane + 6 fma"};
    const int cnt[] = {256, 256, 256, 128, 128, 128, 64, 64};
    for (int i = 0; i < 8; i++) printf("%-48s %6lld cycles  %.1f per item\n", nm[i], h[i], (double)h[i] / cnt[i]);
    printf("row_newbcast:5 of lane ids: lane 0 -> %.7g, lane 17 -> %.7g, lane 40 -> %.7g, lane 63 -> %.7g (expect 5 21 37 53 x 1.0000001)\n", s[64], s[64 + 17], s[64 + 40], s[64 + 63]);
    // ---- k2: hops and whole chunks ----
    for (int rep = 0; rep < 2; rep++) hipLaunchKernelGGL(k2, dim3(1), dim3(64), 0, 0, out, sink, 1.0);
    hipDeviceSynchronize();
    static double s2[576];
    hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost); hipMemcpy(s2, sink, sizeof(s2), hipMemcpyDeviceToHost);
    const char* nm2[] = {"64 x (fma -> fmac_dpp), no hop", "64 x (fma -> hop 0: permlane16_swap r[0], row 0 -> 1 -> fmac_dpp)", "64 x (fma -> hop 1: permlane32_swap r[0], row 1 -> 3 -> fmac_dpp)",
                         "64 x (fma -> hop 2: permlane16_swap r[1], row 3 -> 2 -> fmac_dpp)", "64 x (fma -> hop 3: permlane32_swap r[1], row 2 -> 0 -> fmac_dpp)",
                         "64 x (fma -> ds_write_b64, ds_read_b64 -> fmac_dpp)", "128 steps n=6: 16 chunks of 8 knots, DPP + 4 hops", "128 steps n=6: readlane form (12 readlane + 6 fma + select)"};
    const int cnt2[] = {64, 64, 64, 64, 64, 64, 128, 128};
    for (int i = 0; i < 8; i++) printf("%-72s %6lld cycles  %.1f per item\n", nm2[i], h[i], (double)h[i] / cnt2[i]);
    for (int i = 1; i < 6; i++) printf("  hop cost of line %d over the chain without a hop: %.1f cycles\n", i, (double)(h[i] - h[0]) / 64);
    // where the hops land: target row of hop H <- source row
    const int from[4] = {0, 1, 3, 2}, to[4] = {1, 3, 2, 0};
    int bad = 0;
    for (int H = 0; H < 4; H++) {
        int ok = 1;
        for (int l = 0; l < 16; l++) ok &= s2[192 + 64 * H + 16 * to[H] + l] == (double)(16 * from[H] + l);
        printf("hop %d: row %d -> row %d %s (lane %d holds %.0f)\n", H, from[H], to[H], ok ? "ok" : "WRONG", 16 * to[H], s2[192 + 64 * H + 16 * to[H]]);
        bad += !ok;
    }
    const int turn[4] = {0, 1, 3, 2};
    int okc = 1;
    for (int gs = 0; gs < 8; gs++)
        for (int l = 0; l < 6; l++) {
            const int lane = 16 * turn[gs >> 1] + 8 * (gs & 1) + l;
            okc &= s2[448 + lane] == gs + 1.0 && s2[512 + lane] == gs + 9.0;
        }
    printf("two chunks with unit operands: %s (group 7 of chunk 1 holds %.0f, expect 16)\n", okc ? "ok" : "WRONG", s2[512 + 16 * 2 + 8]);
    bad += !okc;
    // ---- k3: six doubles of a row to the whole row ----
    for (int rep = 0; rep < 2; rep++) hipLaunchKernelGGL(k3, dim3(1), dim3(64), 0, 0, out, sink, 1.0);
    hipDeviceSynchronize();
    static double s3[1216];
    hipMemcpy(h, out, sizeof(h), hipMemcpyDeviceToHost); hipMemcpy(s3, sink, sizeof(s3), hipMemcpyDeviceToHost);
    const char* nm3[] = {"8 rounds: 12 v_readlane_b32 + 3 fma", "8 rounds: 6 v_mov_b64_dpp row_newbcast + 3 fma", "8 rounds: 12 v_mov_b32_dpp row_newbcast (update_dpp) + 3 fma"};
    for (int i = 0; i < 3; i++) printf("%-72s %6lld ticks  %.1f per round\n", nm3[i], h[i], (double)h[i] / 8);
    for (int i = 1; i < 3; i++) printf("  line %d against the readlane form: %+.1f ticks per round\n", i, (double)(h[i] - h[0]) / 8);
    int ok3 = 1;
    for (int q = 0; q < 6; q++)
        for (int l = 0; l < 64; l++)
            ok3 &= s3[64 * (1 + q) + l] == 39.0 + q && s3[64 * (7 + q) + l] == (double)((l & 48) + q) && s3[64 * (13 + q) + l] == (double)((l & 48) + q);
    printf("six doubles of a row: %s (readlane: lane 17 holds %.0f, expect 39; b64 dpp q = 5: lane 17 holds %.0f, lane 63 %.0f, expect 21 53; b32 dpp: %.0f %.0f)\n",
           ok3 ? "ok" : "WRONG", s3[64 + 17], s3[64 * 12 + 17], s3[64 * 12 + 63], s3[64 * 18 + 17], s3[64 * 18 + 63]);
    bad += !ok3;
    return bad ? 1 : 0;
}
