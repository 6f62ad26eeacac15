// sparse_kernels.hip — gfx950 (MI355X) kernels of the sparse delta fold
// (fedavg_sparse_aggregate_delta, include/fedavg_hip.h): FedAvg over clients that send, per tensor,
// nnz (index, value) pairs of a parameter diff instead of the dense diff. A sparse delta is a
// DeltaParameterMessage whose missing entries are +0.0, so the result is the reference's restore()
// (message.py:40-61) followed by FedAVGAlgorithm (fed_avg_algorithm.py:43-99) on the densified
// delta; the contract is DESIGN.md §5n and tests/sparse_reference.py restates it in numpy.
//
// Per element e, with b the fp64 base: d_i = the value client i stores for e, converted exactly to
// fp64, or +0.0; x_i = b + d_i; p_i = x_i * w_i; acc = p_0 then acc = acc + p_i in table order;
// out = acc / W. Each is a separately rounded fp64 operation, NO FMA (the library is built with
// -ffp-contract=off), the add is performed even for d = +0.0 (b = -0.0 gives +0.0) and the first
// product starts the sum. An element's result depends on its base value, the entries that name it,
// the weights and W alone. No atomics.
//
//   * The layout is cut, segment by segment, into tiles of kSpTile elements (a segment's last tile
//     is shorter). A 256-lane workgroup owns one tile: grid = tiles. Lane t owns the elements
//     t, t + 256, ...: kSpTile / 256 = 8, whose base values and accumulators stay in registers.
//   * Prologue: lane t finds, for the clients t, t + 256, ..., the range [lo, lo + cnt) of the
//     client's entries that fall into the tile by two lower-bound searches over its sorted indices
//     (the second inside the window [lo, lo + count]: strictly increasing indices put at most
//     `count` entries into a tile). The ranges stay in LDS.
//   * The clients are folded in batches of kSpBatch, with kSpBatch LDS planes of kSpTile fp64. The
//     lanes walk the batch's entries as one flat range with coalesced loads; an entry is written
//     into its plane only after its index has been checked to lie inside the tile, otherwise it is
//     dropped. After a barrier every lane folds the batch's clients in table order into its own
//     elements and writes +0.0 back over the plane words it read, so the planes are clean for the
//     next batch. Two barriers per batch; the batch size does not enter the result.
//   * Every global access is one element per lane (consecutive lanes, consecutive addresses): no
//     alignment beyond the element's own is assumed of the index, value, base or output storage.
//   * sparse_check_kernel walks every index array once in the same call and latches a word of the
//     sparse state when an index is negative, >= the tensor's element count or not greater than its
//     predecessor (fedavg_sparse_index_errors reports it). The fold is safe whatever the indices
//     are: the searches and the walk stay inside [0, nnz), the plane write is range-checked, and
//     nothing but the tile's own output elements is written.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kSpThreads = 256;  // lanes per workgroup
constexpr int kSpTile = 2048;    // elements per workgroup
constexpr int kSpBatch = 4;      // clients between two pairs of barriers: kSpBatch planes of kSpTile fp64
constexpr int kSpPerLane = kSpTile / kSpThreads;
constexpr int kSpMaxClients = FEDAVG_POINT_MAX_CLIENTS;
constexpr int kSpCheckSlices = 4;  // workgroups per (client, tensor) index array in the check
static_assert(kSpPerLane * kSpThreads == kSpTile && kSpTile <= 65535, "tile geometry");


struct SArgs {
  const Span* tiles;
  const int32_t* const* idx;   // [n][num_segments]; NULL only where nnz == 0
  const void* const* val;      // [n][num_segments]
  const int32_t* nnz;          // [n][num_segments], 0 <= nnz <= numel
  const double* const* base;   // [num_segments]
  void* const* outs;           // [num_segments]
  const double* w;             // [n]
  const int32_t* numel;        // [num_segments]
  double divisor;
  uint32_t* flag;              // the context's NaN words (0 acc, 1 result, 2 input)
  uint32_t* bad;               // the sparse state's index-violation word
  int32_t num_segments;
  int32_t n;
};

// entry j of a client's value array -> fp64, exactly
template <typename V>
__device__ __forceinline__ double sp_value(const void* p, int j);
template <>
__device__ __forceinline__ double sp_value<float>(const void* p, int j) {
  return static_cast<double>(((const float FEDAVG_AS_GLOBAL*)p)[j]);
}
template <>
__device__ __forceinline__ double sp_value<__half>(const void* p, int j) {
  const uint16_t h = ((const uint16_t FEDAVG_AS_GLOBAL*)p)[j];
  return static_cast<double>(__half2float(__ushort_as_half(static_cast<unsigned short>(h))));
}
template <>
__device__ __forceinline__ double sp_value<bf16_t>(const void* p, int j) {
  const uint32_t h = ((const uint16_t FEDAVG_AS_GLOBAL*)p)[j];
  return static_cast<double>(__uint_as_float(h << 16));
}
template <>
__device__ __forceinline__ double sp_value<double>(const void* p, int j) {
  return ((const double FEDAVG_AS_GLOBAL*)p)[j];
}

// first position in [lo, hi) whose index is >= key (hi if none); reads inside [lo, hi) only
__device__ __forceinline__ int sp_lower_bound(const int32_t* p, int lo, int hi, int64_t key) {
  const int32_t FEDAVG_AS_GLOBAL* q = (const int32_t FEDAVG_AS_GLOBAL*)p;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (static_cast<int64_t>(q[mid]) < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---------------------------------------------------------------------------------------
// the fold: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
template <typename V, typename O>
__global__ __launch_bounds__(kSpThreads) void sparse_fold_kernel(SArgs a) {
  constexpr int B = kSpBatch;
  constexpr int K = kSpPerLane;
  __shared__ double plane[B * kSpTile];
  __shared__ int32_t slo[kSpMaxClients];   // first entry of client c inside the tile
  __shared__ uint16_t scnt[kSpMaxClients]; // entries of client c inside the tile (<= count)

  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63;
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg;
  const int32_t count = tp->count;
  const int64_t start = tp->start;
  const int n = a.n;
  const int T = a.num_segments;

  for (int i = t; i < B * kSpTile; i += kSpThreads) plane[i] = 0.0;

  // every client's entries inside [start, start + count)
  for (int c = t; c < n; c += kSpThreads) {
    const int64_t e = static_cast<int64_t>(c) * T + seg;
    const int nz = a.nnz[e];
    int lo = 0, cnt = 0;
    if (nz > 0) {
      const int32_t* const ip = a.idx[e];
      lo = sp_lower_bound(ip, 0, nz, start);
      const int room = nz - lo < count ? nz - lo : count;
      cnt = sp_lower_bound(ip, lo, lo + room, start + count) - lo;
    }
    slo[c] = lo;
    scnt[c] = static_cast<uint16_t>(cnt);
  }

  // the lane's base values, kept for the whole tile (+0.0 past the tile's end)
  double b[K];
  {
    const double FEDAVG_AS_GLOBAL* pb = (const double FEDAVG_AS_GLOBAL*)a.base[seg] + start;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e = k * kSpThreads + t;
      b[k] = e < count ? pb[e] : 0.0;
    }
  }
  __syncthreads();  // the planes are clean, slo and scnt complete

  bool nan_in = false;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.0;

#pragma unroll 1
  for (int c0 = 0; c0 < n; c0 += B) {
    // the batch's entries as one flat range [0, off[B]): client q owns [off[q], off[q + 1])
    const int32_t* ip[B];
    const void* vp[B];
    int lo[B], off[B + 1];
    off[0] = 0;
#pragma unroll
    for (int q = 0; q < B; ++q) {
      const int c = c0 + q;
      const bool live = c < n;
      const int64_t e = static_cast<int64_t>(live ? c : 0) * T + seg;
      const int cnt = live ? static_cast<int>(scnt[c]) : 0;
      lo[q] = live ? slo[c] : 0;
      ip[q] = a.idx[e];
      vp[q] = a.val[e];
      off[q + 1] = off[q] + cnt;
    }
    for (int f = t; f < off[B]; f += kSpThreads) {
      int q = 0, o = 0, l = lo[0];
      const int32_t* ipq = ip[0];
      const void* vpq = vp[0];
#pragma unroll
      for (int r = 1; r < B; ++r) {
        if (f >= off[r]) {
          q = r;
          o = off[r];
          l = lo[r];
          ipq = ip[r];
          vpq = vp[r];
        }
      }
      const int j = l + (f - o);
      const int64_t rel = static_cast<int64_t>(((const int32_t FEDAVG_AS_GLOBAL*)ipq)[j]) - start;
      // into the plane only when the index lies inside this tile; otherwise the entry is dropped
      if (rel >= 0 && rel < count) plane[q * kSpTile + static_cast<int>(rel)] = sp_value<V>(vpq, j);
    }
    __syncthreads();
    // the batch's clients in table order: x = b + d, p = x * w, acc = acc + p (client 0: acc = p)
#pragma unroll
    for (int q = 0; q < B; ++q) {
      const int c = c0 + q;
      if (c < n) {
        const double w = a.w[c];
        const bool first = c == 0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          double* const cell = &plane[q * kSpTile + k * kSpThreads + t];
          const double d = *cell;
          *cell = 0.0;
          const double x = b[k] + d;
          nan_in |= x != x;
          const double p = x * w;
          acc[k] = first ? p : acc[k] + p;
        }
      }
    }
    __syncthreads();
  }

  // out = acc / W
  bool nan_acc = false, nan_out = false;
  O FEDAVG_AS_GLOBAL* po = (O FEDAVG_AS_GLOBAL*)a.outs[seg] + start;
  const double divisor = a.divisor;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = k * kSpThreads + t;
    if (e < count) {
      const double s = acc[k];
      nan_acc |= s != s;
      const double r = s / divisor;
      nan_out |= r != r;
      po[e] = static_cast<O>(r);
    }
  }
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
  if (__ballot(nan_acc) != 0ull && lane == 0) raise_flag(a.flag, 0);
  if (__ballot(nan_out) != 0ull && lane == 0) raise_flag(a.flag, 1);
}

// ---------------------------------------------------------------------------------------
// the index check: blockIdx.x = client * num_segments + segment, blockIdx.y = slice
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpThreads) void sparse_check_kernel(SArgs a) {
  const int64_t pair = blockIdx.x;
  const int nz = a.nnz[pair];
  if (nz <= 0) return;
  const int32_t FEDAVG_AS_GLOBAL* ip = (const int32_t FEDAVG_AS_GLOBAL*)a.idx[pair];
  const int32_t numel = a.numel[pair % a.num_segments];
  const int t = static_cast<int>(threadIdx.x);
  bool bad = false;
  for (int64_t j = static_cast<int64_t>(blockIdx.y) * kSpThreads + t; j < nz;
       j += static_cast<int64_t>(kSpThreads) * kSpCheckSlices) {
    const int32_t i = ip[j];
    bad |= i < 0 || i >= numel || (j > 0 && i <= ip[j - 1]);
  }
  if (__ballot(bad) != 0ull && (t & 63) == 0) raise_flag(a.bad, 0);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct SparseState {
  Span* d_tiles = nullptr;
  int64_t num_tiles = 0;
  int32_t* d_numel = nullptr;  // [num_segments]
  uint32_t* d_bad = nullptr;   // latched by sparse_check_kernel, cleared by fedavg_sparse_index_errors
  TableRing ring;
  ~SparseState() {
    ring.release();
    if (d_tiles) (void)hipFree(d_tiles);
    if (d_numel) (void)hipFree(d_numel);
    if (d_bad) (void)hipFree(d_bad);
  }
};

int32_t ensure_state(const fedavg_robust_view& v, void** slot, SparseState** out) {
  if (*slot == nullptr) {
    std::vector<int32_t> numel(static_cast<size_t>(v.num_segments));
    for (int32_t t = 0; t < v.num_segments; ++t)
      numel[t] = static_cast<int32_t>(v.seg_numel[t]);  // <= INT32_MAX: checked by the caller
    SparseState* st = new SparseState();
    int32_t r = span_table(v.seg_numel, v.num_segments, kSpTile, "sparse fold", "sparse tile table", &st->d_tiles,
                           &st->num_tiles);
    if (r == FEDAVG_OK) {
      hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->d_numel), sizeof(int32_t) * numel.size());
      if (e == hipSuccess) e = hipMemcpy(st->d_numel, numel.data(), sizeof(int32_t) * numel.size(), hipMemcpyHostToDevice);
      if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&st->d_bad), sizeof(uint32_t));
      if (e == hipSuccess) e = hipMemset(st->d_bad, 0, sizeof(uint32_t));
      if (e == hipSuccess) e = hipDeviceSynchronize();  // the word is clear before any stream's first check
      if (e == hipSuccess) e = st->ring.create();
      r = hip_status("sparse tile table", e);
    }
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<SparseState*>(*slot);
  return FEDAVG_OK;
}

template <typename O>
void launch(int32_t value_dtype, dim3 grid, dim3 block, hipStream_t s, const SArgs& a) {
  switch (value_dtype) {
    case FEDAVG_F32: hipLaunchKernelGGL((sparse_fold_kernel<float, O>), grid, block, 0, s, a); break;
    case FEDAVG_F16: hipLaunchKernelGGL((sparse_fold_kernel<__half, O>), grid, block, 0, s, a); break;
    case FEDAVG_BF16: hipLaunchKernelGGL((sparse_fold_kernel<bf16_t, O>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((sparse_fold_kernel<double, O>), grid, block, 0, s, a); break;
  }
}

}  // namespace

int32_t fedavg_internal_sparse_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "sparse_tile") *out = kSpTile;
  else if (n == "sparse_threads") *out = kSpThreads;
  else if (n == "sparse_batch") *out = kSpBatch;
  else if (n == "sparse_max_clients") *out = kSpMaxClients;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_sparse_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<SparseState*>(state);
}

extern "C" int32_t fedavg_sparse_aggregate_delta(fedavg_ctx* ctx, const int32_t* const* index_ptrs,
                                                 const void* const* value_ptrs, const int64_t* nnz,
                                                 int32_t value_dtype, const double* weights, int32_t num_clients,
                                                 double divisor, const double* const* base_ptrs,
                                                 void* const* out_ptrs, int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_SPARSE, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (value_dtype != FEDAVG_F32 && value_dtype != FEDAVG_F16 && value_dtype != FEDAVG_BF16 && value_dtype != FEDAVG_F64)
    return invalid("the sparse fold reads fp32 / fp16 / bf16 / fp64 values (no records)");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("the sparse fold writes fp32 or fp64");
  if (index_ptrs == nullptr || value_ptrs == nullptr || nnz == nullptr || weights == nullptr ||
      base_ptrs == nullptr || out_ptrs == nullptr)
    return invalid("null index table, value table, nnz, weights, base or outputs");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kSpMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the sparse fold takes at most " +
                   std::to_string(kSpMaxClients));
  if (!(std::isfinite(divisor) && divisor > 0)) return invalid("the divisor must be finite and > 0");
  for (int32_t i = 0; i < num_clients; ++i)
    if (!std::isfinite(weights[i])) return invalid("weight " + std::to_string(i) + " is not finite");
  const int T = v.num_segments;
  for (int t = 0; t < T; ++t)
    if (v.seg_numel[t] > 0x7fffffffll)
      return invalid("segment " + std::to_string(t) + " holds more than 2^31 - 1 elements: sparse indices are int32");
  const size_t elem_bytes = value_dtype == FEDAVG_F64 ? 8 : value_dtype == FEDAVG_F32 ? 4 : 2;
  const size_t out_bytes = out_dtype == FEDAVG_F64 ? 8 : 4;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  // the message is built only on a refusal: this loop runs n * T times on every call
  const auto where = [T](size_t i) {
    return "client " + std::to_string(i / T) + ", segment " + std::to_string(i % T);
  };
  const uintptr_t elem_mask = static_cast<uintptr_t>(elem_bytes - 1);
  for (int32_t c = 0; c < num_clients; ++c) {
    const size_t row = static_cast<size_t>(c) * static_cast<size_t>(T);
    for (int t = 0; t < T; ++t) {
      const size_t i = row + static_cast<size_t>(t);
      if (nnz[i] < 0 || nnz[i] > v.seg_numel[t])
        return invalid(where(i) + ": nnz " + std::to_string(nnz[i]) + " outside [0, " + std::to_string(v.seg_numel[t]) + "]");
      if (nnz[i] > 0 && (index_ptrs[i] == nullptr || value_ptrs[i] == nullptr))
        return invalid(where(i) + ": null index or value array with nnz > 0");
      if ((reinterpret_cast<uintptr_t>(index_ptrs[i]) & 3u) != 0) return invalid(where(i) + ": index array not aligned to int32");
      if ((reinterpret_cast<uintptr_t>(value_ptrs[i]) & elem_mask) != 0)
        return invalid(where(i) + ": value array not aligned to its element size");
    }
  }
  for (int t = 0; t < T; ++t) {
    if (base_ptrs[t] == nullptr) return invalid("the base lacks segment " + std::to_string(t));
    if (reinterpret_cast<uintptr_t>(base_ptrs[t]) % 8 != 0) return invalid("base tensor not aligned to fp64");
    if (out_ptrs[t] == nullptr) return invalid("null output pointer for segment " + std::to_string(t));
    if (reinterpret_cast<uintptr_t>(out_ptrs[t]) % out_bytes != 0) return invalid("output tensor not aligned to its element size");
    if (static_cast<const void*>(out_ptrs[t]) == static_cast<const void*>(base_ptrs[t]))
      return invalid("segment " + std::to_string(t) + ": the fold is not in-place (out == base)");
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  SparseState* st = nullptr;
  const int32_t re = ensure_state(v, slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: [n][T] index pointers, [n][T] value pointers, [T] base pointers, [T] output
  // pointers, [n] weights, [n][T] entry counts (int32: nnz <= numel <= INT32_MAX)
  const size_t ptr_bytes = sizeof(void*) * entries;
  const size_t seg_bytes = sizeof(void*) * static_cast<size_t>(T);
  const size_t w_bytes = sizeof(double) * static_cast<size_t>(num_clients);
  const size_t nnz_bytes = sizeof(int32_t) * entries;
  const size_t bytes = 2 * ptr_bytes + 2 * seg_bytes + w_bytes + nnz_bytes;
  // `next` advances only once work that reads this slot has been enqueued and its event recorded: a
  // call that fails before that leaves the slot idle and is simply followed by a call on the same slot
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  const size_t o_val = ptr_bytes, o_base = 2 * ptr_bytes, o_out = o_base + seg_bytes, o_w = o_out + seg_bytes,
               o_nnz = o_w + w_bytes;
  std::memcpy(sl.host, index_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_val, value_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_base, base_ptrs, seg_bytes);
  std::memcpy(sl.host + o_out, out_ptrs, seg_bytes);
  std::memcpy(sl.host + o_w, weights, w_bytes);
  int32_t* const h_nnz = reinterpret_cast<int32_t*>(sl.host + o_nnz);
  for (size_t i = 0; i < entries; ++i) h_nnz[i] = static_cast<int32_t>(nnz[i]);
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  SArgs a;
  a.tiles = st->d_tiles;
  a.idx = reinterpret_cast<const int32_t* const*>(sl.dev);
  a.val = reinterpret_cast<const void* const*>(sl.dev + o_val);
  a.nnz = reinterpret_cast<const int32_t*>(sl.dev + o_nnz);
  a.base = reinterpret_cast<const double* const*>(sl.dev + o_base);
  a.outs = reinterpret_cast<void* const*>(sl.dev + o_out);
  a.w = reinterpret_cast<const double*>(sl.dev + o_w);
  a.numel = st->d_numel;
  a.divisor = divisor;
  a.flag = v.d_flag;
  a.bad = st->d_bad;
  a.num_segments = T;
  a.n = num_clients;
  const dim3 block(kSpThreads);
  hipLaunchKernelGGL(sparse_check_kernel, dim3(static_cast<unsigned>(entries), kSpCheckSlices), block, 0, s, a);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    const dim3 grid(static_cast<unsigned>(st->num_tiles));
    if (out_dtype == FEDAVG_F32) launch<float>(value_dtype, grid, block, s, a);
    else launch<double>(value_dtype, grid, block, s, a);
    e = hipGetLastError();
  }
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("sparse fold launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_sparse_index_errors(fedavg_ctx* ctx, void* stream, int32_t* out) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_SPARSE, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (out == nullptr) return invalid("null out");
  *out = 0;
  SparseState* st = static_cast<SparseState*>(*slot);
  if (st == nullptr) return FEDAVG_OK;  // no sparse fold has run on this context
  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  FEDAVG_TRY_HIP(hipStreamSynchronize(s));
  uint32_t word = 0;
  FEDAVG_TRY_HIP(hipMemcpy(&word, st->d_bad, sizeof(word), hipMemcpyDeviceToHost));
  if (word != 0) {  // reported once: the context stays usable (cleared on the stream, before its next launch)
    FEDAVG_TRY_HIP(hipMemsetAsync(st->d_bad, 0, sizeof(word), s));
    FEDAVG_TRY_HIP(hipStreamSynchronize(s));
  }
  *out = word != 0 ? 1 : 0;
  return FEDAVG_OK;
}
