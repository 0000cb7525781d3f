// model_1.hip -- instantiates the SCP kernels for gusto_model_id 1
#include "launch.hpp"

GUSTO_MODEL_OPS(1, &launch_scp<1>, nullptr)
