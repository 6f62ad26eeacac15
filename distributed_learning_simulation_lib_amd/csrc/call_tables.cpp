// The span list of a layout and the two-slot table ring of the side modules (call_tables.h).
#include "call_tables.h"

#include <vector>

int32_t span_table(const int64_t* seg_numel, int32_t num_segments, int span, const char* what, const char* table,
                   Span** out_dev, int64_t* out_count) {
  std::vector<Span> spans;
  for (int32_t t = 0; t < num_segments; ++t) {
    for (int64_t s = 0; s < seg_numel[t]; s += span) {
      const int64_t left = seg_numel[t] - s;
      spans.push_back(Span{t, static_cast<int32_t>(left < span ? left : span), s});
    }
  }
  if (spans.empty() || spans.size() > 0x7fffffffull) return invalid(std::string("layout too large for one ") + what);
  Span* dev = nullptr;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), sizeof(Span) * spans.size());
  if (e == hipSuccess) e = hipMemcpy(dev, spans.data(), sizeof(Span) * spans.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    if (dev) (void)hipFree(dev);
    return hip_status(table, e);
  }
  *out_dev = dev;
  *out_count = static_cast<int64_t>(spans.size());
  return FEDAVG_OK;
}

hipError_t TableRing::create() {
  hipError_t e = hipSuccess;
  for (auto& sl : slots)
    if (e == hipSuccess) e = hipEventCreateWithFlags(&sl.done, hipEventDisableTiming);
  return e;
}

void TableRing::release() {
  for (auto& sl : slots) {
    if (sl.used) (void)hipEventSynchronize(sl.done);
    if (sl.host) (void)hipHostFree(sl.host);
    if (sl.dev) (void)hipFree(sl.dev);
    if (sl.done) (void)hipEventDestroy(sl.done);
  }
}

namespace {

int32_t grow(TableRing::Slot& sl, size_t bytes) {
  if (sl.cap < bytes) {
    if (sl.host) FEDAVG_TRY_HIP(hipHostFree(sl.host));
    if (sl.dev) FEDAVG_TRY_HIP(hipFree(sl.dev));
    sl.host = sl.dev = nullptr;
    sl.cap = 0;
    const size_t cap = bytes * 2 < 64 * 1024 ? 64 * 1024 : bytes * 2;
    FEDAVG_TRY_HIP(hipHostMalloc(reinterpret_cast<void**>(&sl.host), cap, hipHostMallocDefault));
    FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&sl.dev), cap));
    sl.cap = cap;
  }
  return FEDAVG_OK;
}

}  // namespace

int32_t TableRing::acquire(size_t bytes, Slot** out) {
  Slot& sl = slots[next];
  next ^= 1;
  *out = &sl;
  if (sl.used) FEDAVG_TRY_HIP(hipEventSynchronize(sl.done));  // the launches that read this slot's tables
  return grow(sl, bytes);
}

int32_t TableRing::submit(Slot& sl, size_t bytes, hipStream_t s) {
  FEDAVG_TRY_HIP(hipMemcpyAsync(sl.dev, sl.host, bytes, hipMemcpyHostToDevice, s));
  return FEDAVG_OK;
}

int32_t TableRing::retire(Slot& sl, hipStream_t s) {
  FEDAVG_TRY_HIP(hipEventRecord(sl.done, s));
  sl.used = true;
  return FEDAVG_OK;
}

int32_t TableRing::peek(size_t bytes, Slot** out) {
  Slot& sl = slots[next];
  *out = &sl;
  if (sl.used) FEDAVG_TRY_HIP(hipEventSynchronize(sl.done));  // the launches that read this slot's tables
  sl.used = false;
  return grow(sl, bytes);
}

hipError_t TableRing::commit(Slot& sl, hipStream_t s) {
  // the copy is on the stream whatever became of the launches: the slot is guarded either way
  const hipError_t er = hipEventRecord(sl.done, s);
  if (er == hipSuccess) {
    sl.used = true;
    next ^= 1;
  } else {
    (void)hipStreamSynchronize(s);  // no event to wait for: leave the slot idle before it is reused
  }
  return er;
}
