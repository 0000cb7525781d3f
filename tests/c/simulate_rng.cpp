// simulate_rng.cpp -- the perturbation generator of gusto_simulate (csrc/simrng.hpp) without a device: the header the kernel
// compiles, compiled here into a host program.  Arguments: seed first_problem B S nz, then nz half-widths.  Prints the three
// first outputs of splitmix64(seed) in hex, then the table pert[b][s][i], one entry per line as the 16 hex digits of its bits
// (tests/test_simulate_cpu.py holds it against numpy's uint64 arithmetic).  Host code only.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simrng.hpp"

int main(int argc, char** argv) {
    if (argc < 6) return 1;
    const uint64_t seed = strtoull(argv[1], nullptr, 0), first = strtoull(argv[2], nullptr, 0);
    const uint64_t B = strtoull(argv[3], nullptr, 0), S = strtoull(argv[4], nullptr, 0), nz = strtoull(argv[5], nullptr, 0);
    if ((uint64_t)argc != 6 + nz) return 1;
    std::vector<double> w;
    for (uint64_t i = 0; i < nz; i++) w.push_back(strtod(argv[6 + i], nullptr));
    for (uint64_t i = 0; i < 3; i++) printf("%016" PRIX64 "\n", simrng_u64(seed, i));
    for (uint64_t b = 0; b < B; b++)
        for (uint64_t s = 0; s < S; s++)
            for (uint64_t i = 0; i < nz; i++) {
                const double p = simrng_pert(seed, first + b, S, s, nz, i, w[i]);
                uint64_t bits;
                memcpy(&bits, &p, sizeof(bits));
                printf("%016" PRIX64 "\n", bits);
            }
    return 0;
}
