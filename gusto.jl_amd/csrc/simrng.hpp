// simrng.hpp -- the generated perturbations of gusto_simulate (include/gusto_hip.h states the definition): splitmix64 of a
// counter, integers only up to the last two steps, so host code, device code and numpy draw the same bits.  Compiled by the
// kernel (simulate.hip) and by stand-alone host programs (tests/c/simulate_rng.cpp, tests/c/simulate_disturbed_rng.cpp);
// includes nothing of the library.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SIMRNG_HD __host__ __device__ inline
#else
#define SIMRNG_HD inline
#endif

// the floating-point operations of the enclosing block are not contracted with their neighbours (a x + b stays two roundings)
#if defined(__clang__)
#define SIMRNG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define SIMRNG_NO_CONTRACT
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

// gusto_simulate_disturbed: two more streams of the caller's seed, for the plant and for the actuator noise.  Seeds that
// differ by a multiple of the golden constant give shifted copies of one sequence, so the stream seeds are hashed
SIMRNG_HD uint64_t simrng_plant_seed(uint64_t seed) { return simrng_u64(seed ^ 0x504C414E54ull, 0); }
SIMRNG_HD uint64_t simrng_white_seed(uint64_t seed) { return simrng_u64(seed ^ 0x5748495445ull, 0); }
// scalar j (of np = 6) of the plant of sample s of problem b: nominal (1 + e), e uniform in [-rel, rel); sample 0 draws e = 0.
// One rounding for e, one for the sum, one for the product: e's product must not be fused into the sum
SIMRNG_HD double simrng_plant(uint64_t seed_plant, uint64_t problem, uint64_t S, uint64_t s, uint64_t np, uint64_t j, double nominal,
                              double rel) {
    SIMRNG_NO_CONTRACT
    const double e = simrng_pert(seed_plant, problem, S, s, np, j, rel);
    const double g = 1.0 + e;
    return nominal * g;
}
// entry i (of m) of the actuator noise of sample s of problem b in hold interval k (0-based, of ni = N - 1): uniform in
// [-w, w), 0 for sample 0.  The caller adds it to the commanded control: the product rounds here, on its own, as a caller's
// array of the same numbers would have it
SIMRNG_HD double simrng_white(uint64_t seed_white, uint64_t problem, uint64_t S, uint64_t s, uint64_t ni, uint64_t k, uint64_t m,
                              uint64_t i, double w) {
    SIMRNG_NO_CONTRACT
    if (s == 0) return 0.0;
    const uint64_t z = simrng_u64(seed_white, ((problem * S + s) * ni + k) * m + i);
    const double r = (double)(z >> 11) * 0x1.0p-53;
    return (2.0 * r - 1.0) * w;
}
