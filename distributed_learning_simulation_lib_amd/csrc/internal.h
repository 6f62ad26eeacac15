// What the side modules (<module>_kernels.hip beside fedavg_kernels.hip) need of a context, whose
// struct lives in fedavg_kernels.hip, and what fedavg_kernels.hip calls of them. Library-internal:
// none of it is exported.
#pragma once

#include <stdint.h>

#include "../../include/fedavg_hip.h"

#define FEDAVG_INTERNAL extern "C" __attribute__((visibility("hidden")))

// The side modules, in the order fedavg_kernel_constant asks them and fedavg_ctx_destroy releases
// them. A context holds one state pointer per module; route keeps its state in its own handle.
enum fedavg_module {
  FEDAVG_MODULE_ROBUST,
  FEDAVG_MODULE_KRUM,
  FEDAVG_MODULE_POINT,
  FEDAVG_MODULE_CLIP,
  FEDAVG_MODULE_TRUST,
  FEDAVG_MODULE_OPT,
  FEDAVG_MODULE_SPARSE,
  FEDAVG_MODULE_ROUTE,
  FEDAVG_MODULE_QUANT,
  FEDAVG_MODULE_DP,
  FEDAVG_MODULE_TOPK,
  FEDAVG_MODULES
};

struct fedavg_robust_view {
  int32_t device;
  int32_t num_segments;
  const int64_t* seg_numel;  // [num_segments], owned by the context
  uint32_t* d_flag;          // device alias of the context's NaN words (0 acc, 1 result, 2 input)
  int32_t busy;              // a dynamic wave is open: no other launch on the context
};

// fedavg_kernels.hip
FEDAVG_INTERNAL int32_t fedavg_internal_robust_view(fedavg_ctx* ctx, fedavg_robust_view* out);
// the context's slot for a module's per-context state
FEDAVG_INTERNAL int32_t fedavg_internal_module_slot(fedavg_ctx* ctx, int32_t module, void*** slot);
// sets fedavg_last_error (C++ linkage: the definition personalized_kernels.hip already shares)
__attribute__((visibility("hidden"))) int32_t fedavg_internal_fail(int32_t code, const char* msg);

// <module>_kernels.hip: its fedavg_kernel_constant names (FEDAVG_ERR_INVALID for any other name) and
// the teardown of its per-context state
FEDAVG_INTERNAL int32_t fedavg_internal_robust_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_krum_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_point_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_clip_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_trust_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_opt_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_sparse_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_route_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_quant_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_dp_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL int32_t fedavg_internal_topk_constant(const char* name, int64_t* out);
FEDAVG_INTERNAL void fedavg_internal_robust_release(int32_t device, void* state);
FEDAVG_INTERNAL void fedavg_internal_krum_release(int32_t device, void* state);
FEDAVG_INTERNAL void fedavg_internal_point_release(int32_t device, void* state);
FEDAVG_INTERNAL void fedavg_internal_clip_release(int32_t device, void* state);
FEDAVG_INTERNAL void fedavg_internal_trust_release(int32_t device, void* state);
FEDAVG_INTERNAL void fedavg_internal_opt_release(int32_t device, void* state);
FEDAVG_INTERNAL void fedavg_internal_sparse_release(int32_t device, void* state);
FEDAVG_INTERNAL void fedavg_internal_quant_release(int32_t device, void* state);
FEDAVG_INTERNAL void fedavg_internal_dp_release(int32_t device, void* state);
FEDAVG_INTERNAL void fedavg_internal_topk_release(int32_t device, void* state);
