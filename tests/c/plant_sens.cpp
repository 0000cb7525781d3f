// plant_sens.cpp -- the df/dtheta trait of csrc/models.hpp (Dyn<MODEL>::dfdth, which gusto_lincov_disturbed carries through the
// RK4 stages) against central differences of Dyn<MODEL>::f over the plant scalar, on the host: no device, no handle.
// For every model and every entry j of theta = (mass, Jdiag[0], Jdiag[1], Jdiag[2], dubins_v, dubins_k), at POINTS points
// (x, u) drawn by a small generator and an anisotropic plant: the largest |dfdth - (f(theta_j (1 + e)) - f(theta_j (1 - e))) /
// (2 e theta_j)| with e = 1e-5, and the largest |dfdth| as its scale.  An entry the model does not read must give zeros on
// both sides.  The program prints a JSON list of {"model", "entry", "read", "points", "scale", "err"};
// tests/test_lincov_plant_cpu.py builds it with the address and undefined-behaviour sanitizers and holds the list against
// what it expects.  Host code only.
#include <cmath>
#include <cstdio>

#include "models.hpp"

using namespace gusto;

namespace {
constexpr int POINTS = 5;
bool first = true;
unsigned long long state = 0x9E3779B97F4A7C15ull;

double draw() {   // uniform in [-1, 1)
    state = state * 6364136223846793005ull + 1442695040888963407ull;
    return 2.0 * (double)(state >> 11) * 0x1p-53 - 1.0;
}

double* entry(gusto_model_params& mp, int j) {
    return j == 0 ? &mp.mass : (j < 4 ? &mp.Jdiag[j - 1] : (j == 4 ? &mp.dubins_v : &mp.dubins_k));
}

template <int MODEL> void run(bool (*reads)(int)) {
    using D = Dyn<MODEL>;
    constexpr int n = D::n, m = D::m;
    gusto_model_params mp{};
    mp.mass = 7.2; mp.Jdiag[0] = 0.11; mp.Jdiag[1] = 0.15; mp.Jdiag[2] = 0.19; mp.dubins_v = 2.0; mp.dubins_k = 1.5;
    for (int j = 0; j < GUSTO_NPLANT; j++) {
        double scale = 0.0, err = 0.0;
        for (int p = 0; p < POINTS; p++) {
            double x[n], u[m], g[n], fp[n], fm[n];
            for (int i = 0; i < n; i++) x[i] = draw();
            for (int i = 0; i < m; i++) u[i] = draw();
            D::dfdth(mp, x, u, j, g);
            gusto_model_params a = mp, b = mp;
            const double t = *entry(mp, j), e = 1e-5;
            *entry(a, j) = t * (1.0 + e);
            *entry(b, j) = t * (1.0 - e);
            D::f(a, x, u, fp);
            D::f(b, x, u, fm);
            for (int i = 0; i < n; i++) {
                const double fd = (fp[i] - fm[i]) / (*entry(a, j) - *entry(b, j));
                scale = fmax(scale, fabs(g[i]));
                err = fmax(err, fabs(g[i] - fd));
            }
        }
        printf("%s{\"model\": %d, \"entry\": %d, \"read\": %d, \"points\": %d, \"scale\": %.17g, \"err\": %.17g}", first ? "" : ", ", MODEL, j,
               reads(j) ? 1 : 0, POINTS, scale, err);
        first = false;
    }
}
}  // namespace

int main() {
    printf("[");
    run<GUSTO_FREEFLYER_SE2>([](int j) { return j == 0 || j == 3; });
    run<GUSTO_DUBINS_CAR>([](int j) { return j >= 4; });
    run<GUSTO_ASTROBEE_SE3>([](int j) { return j < 4; });
    run<GUSTO_ASTROBEE_SE3_MANIFOLD>([](int j) { return j < 4; });
    printf("]\n");
    return 0;
}
