// model_2.hip -- instantiates the SCP kernels for gusto_model_id 2
#include "launch.hpp"

GUSTO_MODEL_OPS(2, &launch_scp<2>, nullptr)
