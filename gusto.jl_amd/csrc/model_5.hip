// model_5.hip -- instantiates the TrajOpt kernels of the internal model variant 5 (common.hpp: GUSTO_TO_*)
#include "launch.hpp"

GUSTO_MODEL_OPS(5, nullptr, &launch_trajopt<5>)
