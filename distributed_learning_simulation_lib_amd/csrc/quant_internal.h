// What quant_kernels.hip needs of a context beyond robust_internal.h's view, and what
// fedavg_kernels.hip calls of quant_kernels.hip. Library-internal: none of it is exported.
#pragma once

#include "robust_internal.h"

// fedavg_kernels.hip: the context's slot for quant_kernels.hip's per-context state
FEDAVG_INTERNAL int32_t fedavg_internal_quant_slot(fedavg_ctx* ctx, void*** slot);
// quant_kernels.hip
FEDAVG_INTERNAL int32_t fedavg_internal_quant_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL void fedavg_internal_quant_release(int32_t device, void* state);
