// fleet_args.cpp -- the arguments gusto_fleet_schedule / gusto_fleet_separation check (csrc/fleet.hpp: fleet_args_host) without a
// device.  Every argument is one case, "model,B,R,dt_clock,margin,n_delays,delay_stride,clock_cap,components,prune,order,delay,tf":
// order 0 = null, 1 = index order, 2 = a repeated robot in fleet 1, 3 = an index out of range in fleet 0; delay 0 = null, 1 = zeros,
// 2 = -2 at problem 3, 3 = -1 everywhere; tf 0 = null, 1 = 5.0 everywhere, 2 = 1e6 at problem 2, 3 = NaN at problem 1, 4 = 0.05.
// The program prints a JSON list with, per case, the code, J_max and the error text (tests/test_fleet_cpu.py holds them against
// the rule of include/gusto_hip.h).  Host code only.
#include <cstdio>
#include <cstdlib>

#include "fleet.hpp"

int main(int argc, char** argv) {
    printf("[");
    for (int c = 1; c < argc; c++) {
        double v[13];
        char* p = argv[c];
        for (int i = 0; i < 13; i++) {
            v[i] = strtod(p, &p);
            if (*p == ',') p++;
        }
        const int model = (int)v[0], B = (int)v[1], R = (int)v[2];
        gusto_fleet_opts o = {v[3], v[4], (int)v[5], (int)v[6], (int)v[7], (int)v[8], (int)v[9]};
        const int nB = B > 0 ? B : 1, nR = R > 0 ? R : 1;
        std::vector<int> order(nB), delay(nB, (int)v[11] == 3 ? -1 : 0);
        std::vector<double> tf(nB, (int)v[12] == 4 ? 0.05 : 5.0);
        for (int b = 0; b < nB; b++) order[b] = b % nR;
        if ((int)v[10] == 2 && nB >= 2 * nR && nR >= 2) order[nR + 1] = order[nR];
        if ((int)v[10] == 3) order[0] = nR;
        if ((int)v[11] == 2 && nB > 3) delay[3] = -2;
        if ((int)v[12] == 2 && nB > 2) tf[2] = 1e6;
        if ((int)v[12] == 3 && nB > 1) tf[1] = NAN;
        std::string err;
        int Jmax = -1;
        const int rc = fleet_args_host(model, B, R, &o, (int)v[10] ? order.data() : nullptr, (int)v[11] ? delay.data() : nullptr,
                                       (int)v[12] ? tf.data() : nullptr, &Jmax, "who", &err);
        printf("%s{\"rc\": %d, \"J_max\": %d, \"err\": \"%s\"}", c > 1 ? ", " : "", rc, Jmax, err.c_str());
    }
    printf("]\n");
    return 0;
}
