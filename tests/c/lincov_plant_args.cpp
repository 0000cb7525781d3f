// lincov_plant_args.cpp -- the argument checks gusto_lincov_disturbed adds to gusto_lincov's (csrc/post.hpp:
// lincov_plant_args_host) without a device or a handle, and gusto_lincov's own under the new call's name.
// The cases are built here, for B = 3 problems of freeflyerSE2 (3 controls; reads mass and Jdiag[2], entries 0 and 3), and one
// each of an Astrobee model and the Dubins car: every refusal the header lists that needs no device and the accepted edges.  The
// program prints a JSON list of {"name", "rc", "err"}; tests/test_lincov_plant_cpu.py builds it with the address and
// undefined-behaviour sanitizers and holds the list against what it expects.  Host code only.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "post.hpp"

thread_local std::string g_err;

namespace {
constexpr int NT = GUSTO_NPLANT;
constexpr size_t B = 3;
bool first = true;

void report(const char* name, int rc, const std::string& err) {
    printf("%s{\"name\": \"%s\", \"rc\": %d, \"err\": \"%s\"}", first ? "" : ", ", name, rc, err.c_str());
    first = false;
}
// exactly B problems of NT x NT doubles on the heap: a read past the end is the sanitizer's
std::vector<double> diagonal(double v) {
    std::vector<double> S(B * NT * NT, 0.0);
    for (size_t b = 0; b < B; b++)
        for (int i = 0; i < NT; i++) S[(b * NT + i) * NT + i] = v;
    return S;
}
void run(const char* name, const std::function<void(gusto_disturb_opts&)>& edit, const std::vector<double>* Sth,
         int model = GUSTO_FREEFLYER_SE2, int m = 3) {
    gusto_disturb_opts d;
    memset(&d, 0, sizeof(d));
    edit(d);
    std::string err;
    const int rc = lincov_plant_args_host(model, m, B, &d, Sth ? Sth->data() : nullptr, &err);
    report(name, rc, err);
}
}  // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const auto none = [](gusto_disturb_opts&) {};
    printf("[");
    // accepted
    run("zeros", none, nullptr);
    run("typical", [](gusto_disturb_opts& d) { d.plant_rel[0] = 0.08134; d.plant_rel[3] = 0.05; d.dw[0] = d.dw[1] = 0.01; d.dw[2] = 0.02; }, nullptr);
    run("plant_rel_just_below_one", [](gusto_disturb_opts& d) { d.plant_rel[2] = std::nextafter(1.0, 0.0); }, nullptr);
    run("dw_behind_the_model_is_not_read", [&](gusto_disturb_opts& d) { d.dw[3] = -1; d.dw[5] = nan; }, nullptr);
    const std::vector<double> zero = diagonal(0.0), eye = diagonal(1e-4);
    run("Sth_zero", none, &zero);
    run("Sth_diagonal", none, &eye);
    std::vector<double> s = eye;   // freeflyerSE2 reads entries 0 and 3: everything else may hold anything
    for (size_t b = 0; b < B; b++)
        for (int i = 0; i < NT; i++)
            for (int j = 0; j < NT; j++)
                if (!((i == 0 || i == 3) && (j == 0 || j == 3))) s[(b * NT + i) * NT + j] = (i + j) % 3 == 0 ? nan : ((i + j) % 3 == 1 ? -inf : -1.0 - i);
    run("Sth_garbage_on_unread_entries_freeflyer", none, &s);
    s = eye;
    for (size_t b = 0; b < B; b++)
        for (int i = 0; i < NT; i++)
            for (int j = 0; j < NT; j++)
                if (i < 4 || j < 4) s[(b * NT + i) * NT + j] = i == j ? -1.0 : nan;
    run("Sth_garbage_on_unread_entries_dubins", none, &s, GUSTO_DUBINS_CAR, 1);
    s = zero; s[(1 * NT + 0) * NT + 3] = s[(1 * NT + 3) * NT + 0] = -3e-5;   // (not PSD: the caller's business)
    run("Sth_symmetric_zero_diagonal", none, &s);
    // refused options
    run("plant_rel_negative", [](gusto_disturb_opts& d) { d.plant_rel[0] = -1e-300; }, nullptr);
    run("plant_rel_one", [](gusto_disturb_opts& d) { d.plant_rel[3] = 1.0; }, nullptr);
    run("plant_rel_nan", [&](gusto_disturb_opts& d) { d.plant_rel[5] = nan; }, nullptr);
    run("plant_rel_inf", [&](gusto_disturb_opts& d) { d.plant_rel[1] = inf; }, nullptr);
    run("dw_negative", [](gusto_disturb_opts& d) { d.dw[1] = -0.5; }, nullptr);
    run("dw_inf", [&](gusto_disturb_opts& d) { d.dw[2] = inf; }, nullptr);
    run("dw_nan", [&](gusto_disturb_opts& d) { d.dw[0] = nan; }, nullptr);
    // refused Sth: the last read entry of the last problem, so the whole array is walked
    s = eye; s[(2 * NT + 3) * NT + 3] = nan;
    run("Sth_nan", none, &s);
    s = eye; s[(2 * NT + 0) * NT + 3] = inf; s[(2 * NT + 3) * NT + 0] = inf;
    run("Sth_inf", none, &s);
    s = eye; s[(1 * NT + 3) * NT + 3] = -1e-12;
    run("Sth_negative_diagonal", none, &s);
    s = eye; s[(2 * NT + 0) * NT + 3] = 1e-6; s[(2 * NT + 3) * NT + 0] = std::nextafter(1e-6, 1.0);
    run("Sth_not_symmetric_by_one_bit", none, &s);
    s = eye; s[(0 * NT + 0) * NT + 3] = 0.0; s[(0 * NT + 3) * NT + 0] = -0.0;
    run("Sth_signed_zero", none, &s);
    s = eye; s[(1 * NT + 1) * NT + 2] = nan; s[(1 * NT + 2) * NT + 1] = nan;   // read by the Astrobee models, not by freeflyerSE2
    run("Sth_astrobee_inertia", none, &s, GUSTO_ASTROBEE_SE3, 6);
    s = eye; s[(0 * NT + 4) * NT + 4] = -1.0;
    run("Sth_dubins", none, &s, GUSTO_DUBINS_CAR, 1);
    // gusto_lincov's own checks speak under the name of the call they were made for
    {
        gusto_lincov_opts o;
        memset(&o, 0, sizeof(o));
        for (int i = 0; i < GUSTO_MAXM; i++) { o.u_lo[i] = -INFINITY; o.u_hi[i] = INFINITY; }
        o.du_white[1] = -1.0;
        std::string err;
        const int rc = lincov_args_host(6, 3, B, &o, nullptr, &err, "gusto_lincov_disturbed");
        report("lincov_opts_under_the_new_name", rc, err);
    }
    printf("]\n");
    return 0;
}
