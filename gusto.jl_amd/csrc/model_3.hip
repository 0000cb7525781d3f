// model_3.hip -- instantiates the SCP kernels for gusto_model_id 3
#include "launch.hpp"

GUSTO_MODEL_OPS(3, &launch_scp<3>, nullptr)
