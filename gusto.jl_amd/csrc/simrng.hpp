// simrng.hpp -- the generated perturbations of gusto_simulate (include/gusto_hip.h states the definition): splitmix64 of a
// counter, integers only up to the last two steps, so host code, device code and numpy draw the same bits.  Compiled by the
// kernel (simulate.hip) and by a stand-alone host program (tests/c/simulate_rng.cpp); includes nothing of the library.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SIMRNG_HD __host__ __device__ inline
#else
#define SIMRNG_HD inline
#endif

// output number idx (0-based) of splitmix64 started at `seed`
SIMRNG_HD uint64_t simrng_u64(uint64_t seed, uint64_t idx) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * (idx + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
// entry i of the perturbation of sample s of problem b (first_problem already added to b): uniform in [-w, w), 0 for sample 0.
// r has 53 bits, 2 r - 1 is exact, the product rounds once: a fused multiply-add changes nothing
SIMRNG_HD double simrng_pert(uint64_t seed, uint64_t problem, uint64_t S, uint64_t s, uint64_t nz, uint64_t i, double w) {
    if (s == 0) return 0.0;
    const uint64_t z = simrng_u64(seed, (problem * S + s) * nz + i);
    const double r = (double)(z >> 11) * 0x1.0p-53;
    return (2.0 * r - 1.0) * w;
}
