// What robust_kernels.hip needs of a context (the struct lives in fedavg_kernels.hip) and what
// fedavg_kernels.hip calls of robust_kernels.hip. Library-internal: none of it is exported.
#pragma once

#include <stdint.h>

#include "../../include/fedavg_hip.h"

#define FEDAVG_INTERNAL extern "C" __attribute__((visibility("hidden")))

struct fedavg_robust_view {
  int32_t device;
  int32_t num_segments;
  const int64_t* seg_numel;  // [num_segments], owned by the context
  uint32_t* d_flag;          // device alias of the context's NaN words (0 acc, 1 result, 2 input)
  int32_t busy;              // a dynamic wave is open: no other launch on the context
  void** state;              // the context's slot for robust_kernels.hip's per-context state
};

// fedavg_kernels.hip
FEDAVG_INTERNAL int32_t fedavg_internal_robust_view(fedavg_ctx* ctx, fedavg_robust_view* out);
// sets fedavg_last_error (C++ linkage: the definition personalized_kernels.hip already shares)
__attribute__((visibility("hidden"))) int32_t fedavg_internal_fail(int32_t code, const char* msg);
// robust_kernels.hip
FEDAVG_INTERNAL int32_t fedavg_internal_robust_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL void fedavg_internal_robust_release(int32_t device, void* state);
