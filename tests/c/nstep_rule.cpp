// nstep_rule.cpp -- the Nstep rule of the post-solve stages (csrc/post.hpp: nstep_opts_ok, resolve_nstep_host) without a device.
// Every argument is one case, "N,dt_min,nstep,nstep_cap,tf_0,tf_1,...": the program prints a JSON list with, per case, whether
// the caller's option check passes and -- if it does -- the resolver's code, nstep_max and error text (tests/test_post_cpu.py
// holds them against its own ceil(tf / (N - 1) / dt_min)).  Host code only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "post.hpp"

thread_local std::string g_err;

int main(int argc, char** argv) {
    printf("[");
    for (int c = 1; c < argc; c++) {
        std::vector<double> v;
        for (char* p = argv[c]; *p;) {
            v.push_back(strtod(p, &p));
            if (*p == ',') p++;
        }
        if (v.size() < 4) return 1;
        const int N = (int)v[0], nstep = (int)v[2], cap = (int)v[3];
        const bool ok = nstep_opts_ok(v[1], nstep, cap);
        printf("%s{\"opts_ok\": %s", c > 1 ? ", " : "", ok ? "true" : "false");
        if (ok) {
            int nstep_max = -1;
            std::string err;
            const int rc = resolve_nstep_host(v.data() + 4, v.size() - 4, N, v[1], nstep, cap, "who", &nstep_max, &err);
            printf(", \"rc\": %d, \"nstep_max\": %d, \"err\": \"%s\"", rc, nstep_max, err.c_str());
        }
        printf("}");
    }
    printf("]\n");
    return 0;
}
