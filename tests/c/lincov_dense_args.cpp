// lincov_dense_args.cpp -- the argument check gusto_lincov_dense adds (csrc/post.hpp: lincov_dense_args_host) without a device or
// a handle, and the checks of gusto_lincov and gusto_lincov_disturbed under the new call's name.  B = 3 problems of freeflyerSE2
// (6 states, 3 controls; reads mass and Jdiag[2], entries 0 and 3).  The program prints a JSON list of {"name", "rc", "err"};
// tests/test_lincov_dense_cpu.py builds it with the address and undefined-behaviour sanitizers and holds the list against what it
// expects.  Host code only.
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

#include "post.hpp"

thread_local std::string g_err;

namespace {
constexpr int NT = GUSTO_NPLANT, N_X = 6, N_U = 3, NZ0 = N_X + N_U;
constexpr size_t B = 3;
const char* WHO = "gusto_lincov_dense";
bool first = true;

void report(const char* name, int rc, const std::string& err) {
    printf("%s{\"name\": \"%s\", \"rc\": %d, \"err\": \"%s\"}", first ? "" : ", ", name, rc, err.c_str());
    first = false;
}
// exactly B problems of d x d doubles on the heap: a read past the end is the sanitizer's
std::vector<double> diagonal(int d, double v) {
    std::vector<double> S(B * d * d, 0.0);
    for (size_t b = 0; b < B; b++)
        for (int i = 0; i < d; i++) S[(b * d + i) * d + i] = v;
    return S;
}
void store(const char* name, int store_dense) {
    std::string err;
    const int rc = lincov_dense_args_host(store_dense, &err);
    report(name, rc, err);
}
void plant(const char* name, const gusto_disturb_opts& d, const std::vector<double>* Sth) {
    std::string err;
    const int rc = lincov_plant_args_host(GUSTO_FREEFLYER_SE2, N_U, B, &d, Sth ? Sth->data() : nullptr, &err, WHO);
    report(name, rc, err);
}
void plain(const char* name, const gusto_lincov_opts& o, const std::vector<double>* S0) {
    std::string err;
    const int rc = lincov_args_host(N_X, N_U, B, &o, S0 ? S0->data() : nullptr, &err, WHO);
    report(name, rc, err);
}
}  // namespace

int main() {
    const double nan = std::numeric_limits<double>::quiet_NaN();
    printf("[");
    store("store_dense_0", 0);
    store("store_dense_1", 1);
    store("store_dense_2", 2);
    store("store_dense_minus_1", -1);
    store("store_dense_large", std::numeric_limits<int>::max());
    gusto_disturb_opts zero;
    memset(&zero, 0, sizeof(zero));
    gusto_disturb_opts d = zero;
    d.plant_rel[0] = 0.08134; d.plant_rel[3] = 0.05; d.dw[0] = d.dw[1] = 0.01; d.dw[2] = 0.02;
    plant("dispersion_typical", d, nullptr);
    d = zero; d.plant_rel[3] = 1.0;
    plant("plant_rel_one", d, nullptr);
    d = zero; d.dw[0] = nan;
    plant("dw_nan", d, nullptr);
    const std::vector<double> eye = diagonal(NT, 1e-4);
    plant("Sth_diagonal", zero, &eye);
    std::vector<double> s = eye;
    s[(2 * NT + 0) * NT + 3] = 1e-6; s[(2 * NT + 3) * NT + 0] = std::nextafter(1e-6, 1.0);
    plant("Sth_not_symmetric", zero, &s);
    s = eye; s[(2 * NT + 3) * NT + 3] = nan;   // the last read entry of the last problem: the whole array is walked
    plant("Sth_nan_last_entry", zero, &s);
    gusto_lincov_opts o;
    memset(&o, 0, sizeof(o));
    for (int i = 0; i < GUSTO_MAXM; i++) { o.u_lo[i] = -INFINITY; o.u_hi[i] = INFINITY; }
    gusto_lincov_opts bad = o;
    bad.du_white[1] = -1.0;
    plain("du_white_negative", bad, nullptr);
    bad = o; bad.store_S = 2;
    plain("store_S_2", bad, nullptr);
    std::vector<double> s0 = diagonal(NZ0, 1e-4);
    s0[(2 * NZ0 + 8) * NZ0 + 8] = -1e-12;
    plain("S0_negative_diagonal", o, &s0);
    printf("]\n");
    return 0;
}
