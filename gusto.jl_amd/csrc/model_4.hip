// model_4.hip -- instantiates the TrajOpt kernels of the internal model variant 4 (common.hpp: GUSTO_TO_*)
#include "launch.hpp"

GUSTO_MODEL_OPS(4, nullptr, &launch_trajopt<4>)
