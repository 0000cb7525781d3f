// model_0.hip -- instantiates the SCP kernels for gusto_model_id 0
#include "launch.hpp"

GUSTO_MODEL_OPS(0, &launch_scp<0>, nullptr)
