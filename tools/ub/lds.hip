#include <hip/hip_runtime.h>
#include <cstdio>
// one wave: throughput of back-to-back LDS instructions (32 independent ops, one wait at the end)
#define REP4(x) x x x x
#define REP32(x) REP4(REP4(x)) REP4(REP4(x))
template <int MODE> __device__ long long run(double* lds, int t) {
    double v0, v1, v2, v3;
    unsigned a = (unsigned)(size_t)lds;   // LDS byte address
    unsigned addr = a + 8 * t;            // conflict free
    if (MODE == 1) addr = a;              // broadcast
    if (MODE == 4) addr = a + 8 * (t & 15) * 32;   // 16-way bank conflict
    if (MODE == 7) addr = a + 16 * t;     // b128
    long long t0, t1;
    __builtin_amdgcn_sched_barrier(0);
    t0 = clock64();
    __builtin_amdgcn_sched_barrier(0);
    if (MODE == 0 || MODE == 1 || MODE == 4) {
        REP32(asm volatile("ds_read_b64 %0, %1" : "=v"(v0) : "v"(addr) : "memory");)
    } else if (MODE == 2) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        d2 w;
        REP32(asm volatile("ds_read2_b64 %0, %1 offset0:0 offset1:64" : "=v"(w) : "v"(addr) : "memory");)
        v0 = w.x;
    } else if (MODE == 3) {
        if (t < 16) { REP32(asm volatile("ds_read_b64 %0, %1" : "=v"(v0) : "v"(addr) : "memory");) }
    } else if (MODE == 5) {
        v0 = t;
        REP32(asm volatile("ds_write_b64 %1, %0" : : "v"(v0), "v"(addr) : "memory");)
    } else if (MODE == 6) {
        if (t < 6) { REP32(asm volatile("ds_read_b64 %0, %1" : "=v"(v0) : "v"(addr) : "memory");) }
    } else if (MODE == 7) {
        typedef double d2 __attribute__((ext_vector_type(2)));
        d2 w;
        REP32(asm volatile("ds_read_b128 %0, %1" : "=v"(w) : "v"(addr) : "memory");)
        v0 = w.x;
    } else if (MODE == 8) {
        float f0;
        REP32(asm volatile("ds_read_b32 %0, %1" : "=v"(f0) : "v"(addr) : "memory");)
        v0 = f0;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    t1 = clock64();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" :: "v"(v0));
    return t1 - t0;
}
__global__ void k(long long* out) {
    __shared__ double lds[4096];
    const int t = threadIdx.x;
    for (int i = t; i < 4096; i += 64) lds[i] = i;
    __syncthreads();
    long long r[9];
    r[0] = run<0>(lds, t); r[1] = run<1>(lds, t); r[2] = run<2>(lds, t); r[3] = run<3>(lds, t); r[4] = run<4>(lds, t);
    r[5] = run<5>(lds, t); r[6] = run<6>(lds, t); r[7] = run<7>(lds, t); r[8] = run<8>(lds, t);
    if (t == 0) for (int i = 0; i < 9; i++) out[i] = r[i];
}
// ---- the factor stage's H_uu hand-over and its wide accesses (profiles/r09_factor_stage_lds.txt) -------------------------------
// (a) six lanes hold the upper triangle of a 3 x 3 matrix; every lane needs all six values for a dependent FMA chain:
//     LDS route   ds_write_b64 by the six lanes -> 3 broadcast ds_read_b128 of the same 48 bytes -> FMA
//     lane route  12 v_readlane_b32 -> FMA
//     each as a chain of 8 dependent rounds, alone and with 25 independent FMAs placed between the reads and the first use
typedef double d2v __attribute__((ext_vector_type(2)));
template <bool LDSR, bool FILL> __device__ long long huu(double* lds, int t, double* sink) {
    const double seed = *sink + (LDSR ? 0.5 : 0.25) + (FILL ? 0.125 : 0.0);   // (run-time value per variant: nothing is shared between them)
    double v = seed + 1e-3 * t, f[5] = {seed, seed + 0.1, seed + 0.2, seed + 0.3, seed + 0.4};
    const double g = 1.0 + 1e-9 * t;
    double* w = lds + (t < 6 ? t : 64 + (t & 15));
    __builtin_amdgcn_sched_barrier(0);
    const long long t0 = clock64();
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        double s[6];
        if (LDSR) {
            *w = v;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        if (LDSR) {
            const d2v a = *(const d2v*)(lds), b = *(const d2v*)(lds + 2), c = *(const d2v*)(lds + 4);
            s[0] = a.x; s[1] = a.y; s[2] = b.x; s[3] = b.y; s[4] = c.x; s[5] = c.y;
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        } else {
#pragma unroll
            for (int e = 0; e < 6; e++) {
                const unsigned lo = __builtin_amdgcn_readlane((unsigned)__double2loint(v), e), hi = __builtin_amdgcn_readlane((unsigned)__double2hiint(v), e);
                s[e] = __hiloint2double((int)hi, (int)lo);
            }
        }
        if (FILL) {
#pragma unroll
            for (int q = 0; q < 5; q++)
#pragma unroll
                for (int c = 0; c < 5; c++) f[c] = fma(f[c], g, g);
        }
        v = fma(s[0], s[1], fma(s[2], s[3], fma(s[4], s[5], g))) * 0.25;
        __builtin_amdgcn_sched_barrier(0);
    }
    const long long t1 = clock64();
    __builtin_amdgcn_sched_barrier(0);
    *sink = v + f[0] + f[1] + f[2] + f[3] + f[4];
    return t1 - t0;
}
// (b) 32 two-address accesses of adjacent doubles against 32 128-bit accesses; (c) 9 against 6 back-to-back ds_read_b128
template <int MODE> __device__ long long wide(double* lds, int t) {
    d2v w = {1.0 * t, 2.0};
    const unsigned addr = (unsigned)(size_t)lds + 16 * t;
    __builtin_amdgcn_sched_barrier(0);
    const long long t0 = clock64();
    __builtin_amdgcn_sched_barrier(0);
    if (MODE == 0) { REP32(asm volatile("ds_read2_b64 %0, %1 offset0:0 offset1:1" : "=v"(w) : "v"(addr) : "memory");) }
    else if (MODE == 1) { REP32(asm volatile("ds_read_b128 %0, %1" : "=v"(w) : "v"(addr) : "memory");) }
    else if (MODE == 2) { REP32(asm volatile("ds_write2_b64 %1, %0, %2 offset0:0 offset1:1" : : "v"(w.x), "v"(addr), "v"(w.y) : "memory");) }
    else if (MODE == 3) { REP32(asm volatile("ds_write_b128 %1, %0" : : "v"(w), "v"(addr) : "memory");) }
    else if (MODE == 4) { REP4(asm volatile("ds_read_b128 %0, %1" : "=v"(w) : "v"(addr) : "memory");) REP4(asm volatile("ds_read_b128 %0, %1" : "=v"(w) : "v"(addr) : "memory");) asm volatile("ds_read_b128 %0, %1" : "=v"(w) : "v"(addr) : "memory"); }
    else if (MODE == 5) { REP4(asm volatile("ds_read_b128 %0, %1" : "=v"(w) : "v"(addr) : "memory");) asm volatile("ds_read_b128 %0, %1" : "=v"(w) : "v"(addr) : "memory"); asm volatile("ds_read_b128 %0, %1" : "=v"(w) : "v"(addr) : "memory"); }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    const long long t1 = clock64();
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" :: "v"(w));
    return t1 - t0;
}
__global__ void k2(long long* out, double* sink) {
    __shared__ __attribute__((aligned(16))) double lds[2048];
    const int t = threadIdx.x;
    for (int i = t; i < 2048; i += 64) lds[i] = 1.0 + 1e-6 * i;
    __syncthreads();
    long long r[10];
    r[0] = huu<true, false>(lds, t, sink + t); r[1] = huu<false, false>(lds, t, sink + t);
    r[2] = huu<true, true>(lds, t, sink + t); r[3] = huu<false, true>(lds, t, sink + t);
    r[4] = wide<0>(lds, t); r[5] = wide<1>(lds, t); r[6] = wide<2>(lds, t); r[7] = wide<3>(lds, t); r[8] = wide<4>(lds, t); r[9] = wide<5>(lds, t);
    if (t == 0) for (int i = 0; i < 10; i++) out[i] = r[i];
}
int main() {
    long long* o; (void)hipMalloc(&o, 64 * 8);
    for (int r = 0; r < 2; r++) hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, o);
    long long h[16]; (void)hipMemcpy(h, o, 16 * 8, hipMemcpyDeviceToHost);
    const char* nm[] = {"32 ds_read_b64 conflict-free", "32 ds_read_b64 broadcast", "32 ds_read2_b64", "32 ds_read_b64, 16 lanes active", "32 ds_read_b64 16-way conflict",
                        "32 ds_write_b64", "32 ds_read_b64, 6 lanes active", "32 ds_read_b128", "32 ds_read_b32"};
    for (int i = 0; i < 9; i++) printf("%-36s %6lld ticks  (%.1f per op)\n", nm[i], h[i], (h[i] - 40) / 32.0);
    double* sink; (void)hipMalloc(&sink, 64 * 8); (void)hipMemset(sink, 0, 64 * 8);
    for (int r = 0; r < 2; r++) hipLaunchKernelGGL(k2, dim3(1), dim3(64), 0, 0, o, sink);
    (void)hipMemcpy(h, o, 16 * 8, hipMemcpyDeviceToHost);
    const char* nm2[] = {"H_uu by LDS: write, 3 bcast b128, FMA", "H_uu by 12 v_readlane_b32, FMA", "H_uu by LDS, 25 FMAs inside", "H_uu by v_readlane, 25 FMAs inside",
                         "32 ds_read2_b64 adjacent", "32 ds_read_b128", "32 ds_write2_b64 adjacent", "32 ds_write_b128", "9 ds_read_b128", "6 ds_read_b128"};
    const int per[] = {8, 8, 8, 8, 32, 32, 32, 32, 9, 6};
    for (int i = 0; i < 10; i++) printf("%-38s %6lld ticks  (%.1f per %s)\n", nm2[i], h[i], (h[i] - 40) / (double)per[i], i < 4 ? "round" : "op");
    return 0;
}
