// Host-side probe of the LDS bytes a workgroup of each kernel asks for (csrc/common.hpp: make_lds_layout, the layout launch_scp /
// launch_trajopt size the launch by), compiled and run by tests/test_boundary.py::test_horizon_limits_of_the_lds_layouts (no GPU
// needed: prints one JSON object, {"<model>": [bytes at N = 3, 4, ..., 256]} for the internal model ids 0-6).
#include "common.hpp"
#include <cstdio>
using namespace gusto;
template <int MODEL> static void model(bool last) {
    printf("\"%d\": [", MODEL);
    for (int N = 3; N <= 256; N++)
        printf("%zu%s", (size_t)make_lds_layout<MODEL>(N).total * sizeof(double), N == 256 ? "" : ", ");
    printf("]%s", last ? "" : ", ");
}
int main() {
    printf("{");
    model<0>(false);
    model<1>(false);
    model<2>(false);
    model<3>(false);
    model<4>(false);
    model<5>(false);
    model<6>(true);
    printf("}\n");
    return 0;
}
