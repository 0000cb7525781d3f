// seed_args.cpp -- the arguments every query entry of the seeding stages checks (csrc/seed.hpp: query_args_host) without a
// device.  Every argument is one case, "Bq,K,k_max,batch_cap,null_mask": bit i of null_mask makes array i of four a null pointer.
// The program prints a JSON list with, per case, the code and the error text (tests/test_seed_cpu.py holds them against the rule
// of include/gusto_hip.h).  Host code only.
#include <cstdio>
#include <cstdlib>

#include "seed.hpp"

thread_local std::string g_err;

int main(int argc, char** argv) {
    static const double some[1] = {0.0};
    printf("[");
    for (int c = 1; c < argc; c++) {
        long long v[5];
        char* p = argv[c];
        for (int i = 0; i < 5; i++) {
            v[i] = strtoll(p, &p, 10);
            if (*p == ',') p++;
        }
        const void* a[4];
        for (int i = 0; i < 4; i++) a[i] = (v[4] >> i) & 1 ? nullptr : some;
        std::string err;
        const int rc = query_args_host((int)v[0], (int)v[1], (int)v[2], "LIMIT", (int)v[3], {a[0], a[1], a[2], a[3]}, "who", &err);
        printf("%s{\"rc\": %d, \"err\": \"%s\"}", c > 1 ? ", " : "", rc, err.c_str());
    }
    printf("]\n");
    return 0;
}
