// What fedavg_kernels.hip calls of route_kernels.hip. Library-internal: none of it is exported.
#pragma once

#include "robust_internal.h"

// route_kernels.hip
FEDAVG_INTERNAL int32_t fedavg_internal_route_constant(const char* name, int64_t* out);
