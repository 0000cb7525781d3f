// lincov_args.cpp -- the argument checks of gusto_lincov (csrc/post.hpp: lincov_args_host) without a device or a handle.
// The cases are built here, for a model of 6 states and 3 controls and B = 3 problems: every refusal the header lists and the
// accepted edges.  The program prints a JSON list of {"name", "rc", "err"}; tests/test_lincov_cpu.py builds it with the address
// and undefined-behaviour sanitizers and holds the list against what it expects.  Host code only.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "post.hpp"

thread_local std::string g_err;

namespace {
constexpr int n = 6, m = 3, nz = n + m;
constexpr size_t B = 3;
bool first = true;

gusto_lincov_opts defaults() {
    gusto_lincov_opts o;
    memset(&o, 0, sizeof(o));
    for (int i = 0; i < n; i++) o.dx0[i] = 0.01;
    for (int i = 0; i < GUSTO_MAXM; i++) { o.u_lo[i] = -INFINITY; o.u_hi[i] = INFINITY; }
    return o;
}
// exactly B problems of nz x nz doubles on the heap: a read past the end is the sanitizer's
std::vector<double> identity(double v) {
    std::vector<double> S(B * nz * nz, 0.0);
    for (size_t b = 0; b < B; b++)
        for (int i = 0; i < nz; i++) S[(b * nz + i) * nz + i] = v;
    return S;
}
void run(const char* name, const std::function<void(gusto_lincov_opts&)>& edit, const std::vector<double>* S0) {
    gusto_lincov_opts o = defaults();
    edit(o);
    std::string err;
    const int rc = lincov_args_host(n, m, B, &o, S0 ? S0->data() : nullptr, &err);
    printf("%s{\"name\": \"%s\", \"rc\": %d, \"err\": \"%s\"}", first ? "" : ", ", name, rc, err.c_str());
    first = false;
}
}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const auto none = [](gusto_lincov_opts&) {};
    printf("[");
    // accepted
    run("defaults", none, nullptr);
    run("zero_widths", [](gusto_lincov_opts& o) { for (int i = 0; i < n; i++) o.dx0[i] = 0; }, nullptr);
    run("infinite_bounds", [&](gusto_lincov_opts& o) { o.u_lo[1] = -inf; o.u_hi[1] = inf; o.u_lo[0] = 0.5; o.u_hi[0] = 0.5; }, nullptr);
    run("entries_behind_the_model_are_not_read", [&](gusto_lincov_opts& o) { o.dx0[n] = -1; o.du0[m] = nan; o.du_white[m] = -1; o.u_lo[m] = 1; o.u_hi[m] = 0; }, nullptr);
    run("store_S_1", [](gusto_lincov_opts& o) { o.store_S = 1; }, nullptr);
    const std::vector<double> zero = identity(0.0), eye = identity(1e-4);
    run("S0_zero", none, &zero);
    run("S0_diagonal", none, &eye);
    std::vector<double> zd = identity(0.0);   // symmetric, zero diagonal, off-diagonal entries (not PSD: the caller's business)
    zd[(1 * nz + 2) * nz + 7] = zd[(1 * nz + 7) * nz + 2] = -3e-5;
    run("S0_symmetric_zero_diagonal", none, &zd);
    // refused options
    run("dx0_negative", [](gusto_lincov_opts& o) { o.dx0[4] = -1e-300; }, nullptr);
    run("dx0_inf", [&](gusto_lincov_opts& o) { o.dx0[0] = inf; }, nullptr);
    run("dx0_nan", [&](gusto_lincov_opts& o) { o.dx0[5] = nan; }, nullptr);
    run("du0_negative", [](gusto_lincov_opts& o) { o.du0[2] = -1; }, nullptr);
    run("du0_nan", [&](gusto_lincov_opts& o) { o.du0[0] = nan; }, nullptr);
    run("du_white_negative", [](gusto_lincov_opts& o) { o.du_white[1] = -0.5; }, nullptr);
    run("du_white_inf", [&](gusto_lincov_opts& o) { o.du_white[2] = inf; }, nullptr);
    run("u_lo_above_u_hi", [](gusto_lincov_opts& o) { o.u_lo[2] = 1; o.u_hi[2] = 0.5; }, nullptr);
    run("u_lo_nan", [&](gusto_lincov_opts& o) { o.u_lo[0] = nan; }, nullptr);
    run("u_hi_nan", [&](gusto_lincov_opts& o) { o.u_hi[1] = nan; }, nullptr);
    run("store_S_2", [](gusto_lincov_opts& o) { o.store_S = 2; }, nullptr);
    run("store_S_negative", [](gusto_lincov_opts& o) { o.store_S = -1; }, nullptr);
    // refused S0: the last entry of the last problem, so the whole array is walked
    std::vector<double> s = eye;
    s[B * nz * nz - 1] = nan;
    run("S0_nan", none, &s);
    s = eye; s[(2 * nz + 3) * nz + 8] = inf; s[(2 * nz + 8) * nz + 3] = inf;
    run("S0_inf", none, &s);
    s = eye; s[(1 * nz + 8) * nz + 8] = -1e-12;
    run("S0_negative_diagonal", none, &s);
    s = eye; s[(2 * nz + 7) * nz + 8] = 1e-6; s[(2 * nz + 8) * nz + 7] = std::nextafter(1e-6, 1.0);
    run("S0_not_symmetric_by_one_bit", none, &s);
    s = eye; s[(0 * nz + 0) * nz + 1] = 0.0; s[(0 * nz + 1) * nz + 0] = -0.0;
    run("S0_signed_zero", none, &s);
    printf("]\n");
    return 0;
}
