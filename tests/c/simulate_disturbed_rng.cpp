// simulate_disturbed_rng.cpp -- the two generator streams of gusto_simulate_disturbed (csrc/simrng.hpp) without a device: the
// header the kernel compiles, compiled here into a host program.  Arguments: seed first_problem B S N m, then 6 nominal plant
// scalars, 6 relative half-widths, m noise half-widths.  Prints the two stream seeds in hex, then the table plant[b][s][j] and
// the table white[b][k][s][i], one entry per line as the 16 hex digits of its bits (tests/test_simulate_disturbed_cpu.py holds
// them against numpy's uint64 arithmetic).  Host code only.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "simrng.hpp"

static void put(double v) {
    uint64_t bits;
    memcpy(&bits, &v, sizeof(bits));
    printf("%016" PRIX64 "\n", bits);
}

int main(int argc, char** argv) {
    if (argc < 7) return 1;
    const uint64_t seed = strtoull(argv[1], nullptr, 0), first = strtoull(argv[2], nullptr, 0);
    const uint64_t B = strtoull(argv[3], nullptr, 0), S = strtoull(argv[4], nullptr, 0), N = strtoull(argv[5], nullptr, 0);
    const uint64_t m = strtoull(argv[6], nullptr, 0), np = 6;
    if ((uint64_t)argc != 7 + 2 * np + m || N < 2) return 1;
    std::vector<double> v;
    for (int i = 7; i < argc; i++) v.push_back(strtod(argv[i], nullptr));
    const double *nominal = v.data(), *rel = nominal + np, *dw = rel + np;
    const uint64_t sp = simrng_plant_seed(seed), sw = simrng_white_seed(seed);
    printf("%016" PRIX64 "\n%016" PRIX64 "\n", sp, sw);
    for (uint64_t b = 0; b < B; b++)
        for (uint64_t s = 0; s < S; s++)
            for (uint64_t j = 0; j < np; j++) put(simrng_plant(sp, first + b, S, s, np, j, nominal[j], rel[j]));
    for (uint64_t b = 0; b < B; b++)
        for (uint64_t k = 0; k + 1 < N; k++)
            for (uint64_t s = 0; s < S; s++)
                for (uint64_t i = 0; i < m; i++) put(simrng_white(sw, first + b, S, s, N - 1, k, m, i, dw[i]));
    return 0;
}
