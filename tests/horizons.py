"""The largest horizon N each kernel accepts: the single table the tests use (include/gusto_hip.h states the same numbers).

gusto_create / gusto_create_trajopt accept 3 <= N <= 256; the launch then refuses (GUSTO_ERR_ARG, "does not fit the 160 KiB LDS")
any N whose workgroup layout, make_lds_layout<MODEL>(N) of csrc/common.hpp, is larger than a CU's 160 KiB of LDS.
tests/test_boundary.py::test_horizon_limits_of_the_lds_layouts checks this table against the layouts themselves (tests/c/lds_limits.hip)."""
import gusto_jl_amd as g

N_MIN, N_MAX = 3, 256
LDS_BYTES = 160 * 1024

# public model id -> largest N of the GuSTO kernel (gusto_create)
GUSTO = {g.FREEFLYER_SE2: 256, g.DUBINS_CAR: 256, g.ASTROBEE_SE3: 200, g.ASTROBEE_SE3_MANIFOLD: 182}
# public model id -> largest N of the TrajOpt kernel (gusto_create_trajopt; dubins_car has no TrajOpt variant)
TRAJOPT = {g.FREEFLYER_SE2: 256, g.ASTROBEE_SE3: 157, g.ASTROBEE_SE3_MANIFOLD: 139}
# the internal model id whose layout the TrajOpt kernel of a public model uses (csrc/common.hpp: GUSTO_TO_*)
TRAJOPT_INTERNAL = {g.FREEFLYER_SE2: 4, g.ASTROBEE_SE3: 5, g.ASTROBEE_SE3_MANIFOLD: 6}


def waves(N):
    """wavefronts per workgroup of a GuSTO problem (launch.hpp: launch_waves) and of a TrajOpt problem: one per 64 knots"""
    return (N + 63) // 64
