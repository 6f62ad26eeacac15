// Host-side plumbing the side modules (<module>_kernels.hip) share: error helpers, the span list of
// a layout, and the two-slot ring that carries a call's tables to the device.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "internal.h"

#define FEDAVG_TRY_HIP(expr)                                                                          \
  do {                                                                                                \
    hipError_t e_ = (expr);                                                                           \
    if (e_ != hipSuccess)                                                                             \
      return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string(#expr) + ": " + hipGetErrorString(e_)).c_str()); \
  } while (0)

#define FEDAVG_TRY(expr)            \
  do {                              \
    int32_t r_ = (expr);            \
    if (r_ != FEDAVG_OK) return r_; \
  } while (0)

__attribute__((visibility("hidden"))) inline int32_t invalid(const std::string& msg) {
  return fedavg_internal_fail(FEDAVG_ERR_INVALID, msg.c_str());
}

// FEDAVG_OK, or FEDAVG_ERR_HIP with "<what>: <the error's text>"
__attribute__((visibility("hidden"))) inline int32_t hip_status(const char* what, hipError_t e) {
  if (e == hipSuccess) return FEDAVG_OK;
  return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string(what) + ": " + hipGetErrorString(e)).c_str());
}

__attribute__((visibility("hidden"))) inline bool misaligned(const void* p, uintptr_t bytes) {
  return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0;
}

// One workgroup's share of a layout: a module's tile or chunk.
struct Span {
  int32_t seg;
  int32_t count;  // elements in this span (the module's span length except at a segment's end)
  int64_t start;  // first element, relative to the segment
};

// Cuts the layout, segment by segment, into spans of `span` elements (a segment's last span is
// shorter) and uploads the list. Fails with "layout too large for one <what>" or "<table>: <HIP error>".
__attribute__((visibility("hidden"))) int32_t span_table(const int64_t* seg_numel, int32_t num_segments, int span,
                                                         const char* what, const char* table, Span** out_dev,
                                                         int64_t* out_count);

// A call's tables (pointer lists, coefficients, ...) go to the device through one of two pinned
// slots, so the next call can fill its image while the launches of this one still read theirs. A
// slot is reused once the event recorded after the launches that read it has completed, and is
// freed and regrown (to twice the bytes asked for, at least 64 KiB) only after that wait.
struct __attribute__((visibility("hidden"))) TableRing {
  struct Slot {
    char* host = nullptr;  // pinned image of a call's tables
    char* dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;  // the launches that read `dev` finished
    bool used = false;
  } slots[2];
  int next = 0;

  hipError_t create();  // the events
  void release();       // waits for the launches in flight, then frees the slots and the events

  // The next slot, idle and at least `bytes` large. A call is then: fill sl.host, submit, launch, retire.
  int32_t acquire(size_t bytes, Slot** out);
  int32_t submit(Slot& sl, size_t bytes, hipStream_t s);  // the copy of sl.host to sl.dev
  int32_t retire(Slot& sl, hipStream_t s);                // the event after the call's launches

  // The same for a call that keeps its slot until the event is on the stream: peek() leaves `next`
  // on the slot, so a call that fails before commit() is followed by a call on the same slot;
  // commit() records the event and moves on, or drains the stream where the record fails.
  int32_t peek(size_t bytes, Slot** out);
  hipError_t commit(Slot& sl, hipStream_t s);
};
