// model_6.hip -- instantiates the TrajOpt kernels of the internal model variant 6 (common.hpp: GUSTO_TO_*)
#include "launch.hpp"

GUSTO_MODEL_OPS(6, nullptr, &launch_trajopt<6>)
