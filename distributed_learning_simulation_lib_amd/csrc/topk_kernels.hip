// topk_kernels.hip — gfx950 (MI355X) kernels of the client-side top-k step with error feedback
// (fedavg_topk_sparsify, include/fedavg_hip.h): what sparse.topk_sparsify computes with two sorts,
// for all tensors of a model in a fixed number of streaming launches. The contract is DESIGN.md §5s;
// the oracle is the CPU path of sparse.topk_sparsify (torch's stable sort).
//
// t[e] = delta[e] + error[e] rounded once into the dtype (delta[e] itself where there is no error);
// key(t[e]) = its bits without the sign, every NaN on the one largest key; the `keep` elements of
// largest (key, -index) are sent, in index order, and leave +0.0 in the residual. No sort:
//   * topk_hist_kernel, once per digit of the key from the top: a workgroup owns one chunk of kKChunk
//     consecutive tiles of one tensor and counts the digit of every element whose higher digits equal
//     the tensor's prefix so far into an LDS histogram (integer adds: any order gives the same
//     counts), then stores the histogram as its partial. The first of them also forms t and stores
//     it to the residual, which is what every later pass reads.
//   * topk_select_kernel after each: one workgroup per tensor sums the partials of its chunks and
//     scans from the top bin to the digit that holds the element still wanted; the prefix grows by
//     that digit and `want` shrinks by the count above it. After the last digit the prefix is the
//     threshold key tau and `want` is r, the number of key == tau elements to send.
//   * topk_count_kernel: per tile #(key > tau) and #(key == tau).
//   * topk_scan_kernel: one workgroup per tensor, the exclusive scan of both over its tiles.
//   * topk_write_kernel: one workgroup per tile. An element is sent if key > tau, or key == tau and
//     fewer than r such elements precede it in its tensor; its place in the output is the number of
//     sent elements before it, from the tile's two prefixes and a scan inside the tile, so the
//     indices come out ascending.
// No atomics on global memory, no floating-point reductions, no host round trip.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kKThreads = 256;  // lanes per workgroup
constexpr int kKWaves = kKThreads / 64;
constexpr int kKTile = 2048;    // elements per tile: the unit of the counts and of the write pass
constexpr int kKChunk = 8;      // tiles per workgroup of the histogram and count passes
constexpr int kKBins = 2048;    // bins of a partial histogram (the widest digit has 11 bits)
// Copies of the LDS histogram, chosen by the lane: gradients cluster on a few exponents, so many
// lanes of a wave add to one bin; copy c of bin b lies at word b * kKCopies + c, on another bank.
constexpr int kKCopies = 4;
constexpr int kKMaxTensors = 1 << 20;
constexpr int kKMaxPasses = 6;
static_assert(kKTile % (kKThreads * 8) == 0, "a tile is whole rows of one 16-byte group per lane");
static_assert(kKTile <= 0xffff, "a tile's two counts share one 32-bit word");

struct KTensor {
  const void* delta;
  const void* error;  // NULL: no residual yet
  void* residual;
  int32_t* indices;
  void* values;
  int64_t numel;
  int64_t keep;
  int32_t first_tile;   // of the call's tile counts
  int32_t first_chunk;  // of the call's chunk list
  int32_t num_chunks;
  int32_t pad;
};

// A tensor's select state: the key digits fixed so far, and how many elements are still wanted
// among those that share them. After the last digit: tau and r. keep == 0: tau above every key.
struct KState {
  uint64_t prefix;
  uint32_t want;
  uint32_t pad;
};

struct KArgs {
  const Span* chunks;      // the chunks of every tensor, in list order
  const KTensor* tensors;  // [T]
  uint32_t* part;          // [chunks][kKBins]
  KState* state;           // [T]
  uint32_t* counts;        // [tiles][2]: #(key > tau), #(key == tau); after the scan their prefixes
  int32_t shift;           // bits below this pass's digit
  int32_t bits;            // width of this pass's digit
  int32_t first;           // this is the first digit
};

// ---------------------------------------------------------------------------------------
// keys and sums
// ---------------------------------------------------------------------------------------
template <typename T>
struct KKey;
template <>
struct KKey<float> {
  using K = uint32_t;
  static constexpr int kPasses = 3;
  static constexpr int kDigits[kKMaxPasses] = {11, 10, 10, 0, 0, 0};
  __device__ __forceinline__ static K key(const u32x4& raw, int i) {
    const uint32_t k = raw[i] & 0x7fffffffu;
    return k > 0x7f800000u ? 0x7fffffffu : k;
  }
  __device__ __forceinline__ static void add(u32x4& d, const u32x4& e) {
#pragma unroll
    for (int i = 0; i < 4; ++i) d[i] = __float_as_uint(__uint_as_float(d[i]) + __uint_as_float(e[i]));
  }
};
template <>
struct KKey<__half> {
  using K = uint32_t;
  static constexpr int kPasses = 2;
  static constexpr int kDigits[kKMaxPasses] = {8, 7, 0, 0, 0, 0};
  __device__ __forceinline__ static K key(const u32x4& raw, int i) {
    const uint32_t k = (raw[i / 2] >> (16 * (i % 2))) & 0x7fffu;
    return k > 0x7c00u ? 0x7fffu : k;
  }
  // the fp32 sum rounded to fp16 is the correctly rounded sum: 24 >= 2 * 11 + 2
  __device__ __forceinline__ static uint32_t add1(uint32_t a, uint32_t b) {
    const float s = __half2float(__ushort_as_half(static_cast<unsigned short>(a))) +
                    __half2float(__ushort_as_half(static_cast<unsigned short>(b)));
    return __half_as_ushort(__float2half_rn(s));
  }
  __device__ __forceinline__ static void add(u32x4& d, const u32x4& e) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      d[i] = add1(d[i] & 0xffffu, e[i] & 0xffffu) | (add1(d[i] >> 16, e[i] >> 16) << 16);
  }
};
template <>
struct KKey<bf16_t> {
  using K = uint32_t;
  static constexpr int kPasses = 2;
  static constexpr int kDigits[kKMaxPasses] = {8, 7, 0, 0, 0, 0};
  __device__ __forceinline__ static K key(const u32x4& raw, int i) {
    const uint32_t k = (raw[i / 2] >> (16 * (i % 2))) & 0x7fffu;
    return k > 0x7f80u ? 0x7fffu : k;
  }
  // the fp32 sum rounded to nearest even into bf16: 24 >= 2 * 8 + 2
  __device__ __forceinline__ static uint32_t add1(uint32_t a, uint32_t b) {
    const float s = __uint_as_float(a << 16) + __uint_as_float(b << 16);
    const uint32_t u = __float_as_uint(s);
    return s == s ? (u + 0x7fffu + ((u >> 16) & 1u)) >> 16 : 0x7fc0u;
  }
  __device__ __forceinline__ static void add(u32x4& d, const u32x4& e) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      d[i] = add1(d[i] & 0xffffu, e[i] & 0xffffu) | (add1(d[i] >> 16, e[i] >> 16) << 16);
  }
};
template <>
struct KKey<double> {
  using K = uint64_t;
  static constexpr int kPasses = 6;
  static constexpr int kDigits[kKMaxPasses] = {11, 11, 11, 10, 10, 10};
  __device__ __forceinline__ static K key(const u32x4& raw, int i) {
    const uint64_t k = (static_cast<uint64_t>(raw[2 * i]) | (static_cast<uint64_t>(raw[2 * i + 1]) << 32)) &
                       0x7fffffffffffffffull;
    return k > 0x7ff0000000000000ull ? 0x7fffffffffffffffull : k;
  }
  __device__ __forceinline__ static void add(u32x4& d, const u32x4& e) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const double s = Format<double>::value(d, i) + Format<double>::value(e, i);
      const uint64_t b = static_cast<uint64_t>(__double_as_longlong(s));
      d[2 * i] = static_cast<uint32_t>(b);
      d[2 * i + 1] = static_cast<uint32_t>(b >> 32);
    }
  }
};

// the group of N elements from element e of `base`: one 16-byte load where it is complete and aligned
template <typename T>
__device__ __forceinline__ u32x4 k_load(const void* base, int64_t e, int have) {
  const char* p = static_cast<const char*>(base) + e * static_cast<int64_t>(sizeof(T));
  if (have == Format<T>::N && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) return *(const u32x4 FEDAVG_AS_GLOBAL*)p;
  return load_guarded<T>(base, e, have);
}

template <typename T>
__device__ __forceinline__ void k_store(void* base, int64_t e, int have, const u32x4& raw) {
  char* p = static_cast<char*>(base) + e * static_cast<int64_t>(sizeof(T));
  if (have == Format<T>::N && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) *(u32x4 FEDAVG_AS_GLOBAL*)p = raw;
  else store_guarded<T>(base, e, have, raw);
}

// The exclusive prefix of v over the workgroup's lanes in lane order, and the total. Integer sums.
template <typename V>
__device__ __forceinline__ V k_scan(V v, V* sm, V& total) {
  const int t = static_cast<int>(threadIdx.x), lane = t & 63, w = t >> 6;
  V inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const V o = __shfl_up(inc, off);
    if (lane >= off) inc += o;
  }
  __syncthreads();  // the previous scan's readers are done with sm
  if (lane == 63) sm[w] = inc;
  __syncthreads();
  V base = 0;
  total = 0;
#pragma unroll
  for (int i = 0; i < kKWaves; ++i) {
    const V s = sm[i];
    if (i < w) base += s;
    total += s;
  }
  return base + inc - v;
}

// ---------------------------------------------------------------------------------------
// the digit histogram of one chunk: blockIdx.x = chunk
// ---------------------------------------------------------------------------------------
template <typename T, bool kFirst>
__global__ __launch_bounds__(kKThreads) void topk_hist_kernel(KArgs a) {
  constexpr int N = Format<T>::N;
  using K = typename KKey<T>::K;
  __shared__ uint32_t hist[kKBins * kKCopies];
  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* cp = (const Span FEDAVG_AS_CONST*)(a.chunks + blockIdx.x);
  const int32_t seg = cp->seg, count = cp->count;
  const int64_t start = cp->start;
  const KTensor FEDAVG_AS_CONST* tp = (const KTensor FEDAVG_AS_CONST*)(a.tensors + seg);
  const void* const delta = tp->delta;
  const void* const error = tp->error;
  void* const residual = tp->residual;
  const int bins = 1 << a.bits;
  for (int b = t; b < bins * kKCopies; b += kKThreads) hist[b] = 0u;
  __syncthreads();
  const K prefix = kFirst ? K(0) : static_cast<K>(a.state[seg].prefix);
  const int above = a.shift + a.bits;  // < the key's width except in the first pass
  const uint32_t mask = static_cast<uint32_t>(bins - 1);
  uint32_t* const mine = hist + (t & (kKCopies - 1));
  for (int g = t; g * N < count; g += kKThreads) {
    const int64_t e = start + static_cast<int64_t>(g) * N;
    const int have = count - g * N < N ? count - g * N : N;
    u32x4 raw;
    if (kFirst) {
      raw = k_load<T>(delta, e, have);
      if (error != nullptr) KKey<T>::add(raw, k_load<T>(error, e, have));
      k_store<T>(residual, e, have, raw);
    } else {
      raw = k_load<T>(residual, e, have);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i >= have) continue;
      const K key = KKey<T>::key(raw, i);
      if (kFirst || (key >> above) == prefix)
        atomicAdd(mine + (static_cast<uint32_t>(key >> a.shift) & mask) * kKCopies, 1u);
    }
  }
  __syncthreads();
  uint32_t* const part = a.part + static_cast<size_t>(blockIdx.x) * kKBins;
  for (int b = t; b < bins; b += kKThreads) {
    uint32_t s = 0;
#pragma unroll
    for (int c = 0; c < kKCopies; ++c) s += hist[b * kKCopies + c];
    part[b] = s;
  }
}

// ---------------------------------------------------------------------------------------
// the digit that holds the element still wanted: blockIdx.x = tensor
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kKThreads) void topk_select_kernel(KArgs a) {
  __shared__ uint32_t tot[kKBins];
  __shared__ uint32_t sm[kKWaves];
  const int t = static_cast<int>(threadIdx.x);
  const int seg = static_cast<int>(blockIdx.x);
  const KTensor FEDAVG_AS_CONST* tp = (const KTensor FEDAVG_AS_CONST*)(a.tensors + seg);
  const int64_t keep = tp->keep;
  if (keep == 0) {  // nothing is sent: a threshold above every key (the same for the whole workgroup)
    if (t == 0) a.state[seg] = KState{~0ull, 0u, 0u};
    return;
  }
  const int bins = 1 << a.bits;
  const uint32_t* const part = a.part + static_cast<size_t>(tp->first_chunk) * kKBins;
  const int chunks = tp->num_chunks;
  for (int b = t; b < bins; b += kKThreads) {
    uint32_t s = 0;
    for (int c = 0; c < chunks; ++c) s += part[static_cast<size_t>(c) * kKBins + b];
    tot[b] = s;
  }
  __syncthreads();
  const uint64_t prefix = a.first ? 0ull : a.state[seg].prefix;
  const uint32_t want = a.first ? static_cast<uint32_t>(keep) : a.state[seg].want;
  // lane t owns `per` bins from bin (bins - 1 - t * per) downwards; lanes past the bins own none
  const int per = bins >= kKThreads ? bins / kKThreads : 1;
  const int hi = bins - 1 - t * per;
  uint32_t my = 0;
  if (hi >= 0)
    for (int j = 0; j < per; ++j) my += tot[hi - j];
  uint32_t total;
  uint32_t above = k_scan<uint32_t>(my, sm, total);
  if (above < want && want <= above + my) {  // one lane: the counts sum to at least `want`
    for (int j = 0; j < per; ++j) {
      const uint32_t c = tot[hi - j];
      if (want <= above + c) {
        a.state[seg] = KState{(prefix << a.bits) | static_cast<uint64_t>(hi - j), want - above, 0u};
        break;
      }
      above += c;
    }
  }
}

// ---------------------------------------------------------------------------------------
// per tile #(key > tau) and #(key == tau): blockIdx.x = chunk
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kKThreads) void topk_count_kernel(KArgs a) {
  constexpr int N = Format<T>::N;
  using K = typename KKey<T>::K;
  __shared__ uint32_t sm[kKWaves];
  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* cp = (const Span FEDAVG_AS_CONST*)(a.chunks + blockIdx.x);
  const int32_t seg = cp->seg, count = cp->count;
  const int64_t start = cp->start;
  const KTensor FEDAVG_AS_CONST* tp = (const KTensor FEDAVG_AS_CONST*)(a.tensors + seg);
  const void* const residual = tp->residual;
  const uint64_t tau64 = a.state[seg].prefix;
  const bool none = tau64 == ~0ull;
  const K tau = static_cast<K>(tau64);
  const int64_t tile0 = tp->first_tile + start / kKTile;
  for (int off = 0; off < count; off += kKTile) {
    const int n = count - off < kKTile ? count - off : kKTile;
    uint32_t c = 0;  // gt in the low half, eq in the high half: at most kKTile each
    if (!none) {
      for (int g = t; g * N < n; g += kKThreads) {
        const int have = n - g * N < N ? n - g * N : N;
        const u32x4 raw = k_load<T>(residual, start + off + static_cast<int64_t>(g) * N, have);
#pragma unroll
        for (int i = 0; i < N; ++i) {
          if (i >= have) continue;
          const K key = KKey<T>::key(raw, i);
          c += (key > tau ? 1u : 0u) + (key == tau ? 0x10000u : 0u);
        }
      }
    }
    uint32_t total;
    (void)k_scan<uint32_t>(c, sm, total);
    if (t == 0) {
      uint32_t* const o = a.counts + 2 * (tile0 + off / kKTile);
      o[0] = total & 0xffffu;
      o[1] = total >> 16;
    }
  }
}

// ---------------------------------------------------------------------------------------
// the exclusive scan of a tensor's tile counts, in place: blockIdx.x = tensor
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kKThreads) void topk_scan_kernel(KArgs a) {
  __shared__ uint64_t sm[kKWaves];
  const int t = static_cast<int>(threadIdx.x);
  const KTensor FEDAVG_AS_CONST* tp = (const KTensor FEDAVG_AS_CONST*)(a.tensors + blockIdx.x);
  const int64_t tiles = (tp->numel + kKTile - 1) / kKTile;
  uint32_t* const counts = a.counts + 2 * static_cast<int64_t>(tp->first_tile);
  uint64_t carry = 0;  // gt in the low word, eq in the high word: each below 2^31 in all
  for (int64_t i0 = 0; i0 < tiles; i0 += kKThreads) {
    const int64_t i = i0 + t;
    uint64_t v = 0;
    if (i < tiles) v = static_cast<uint64_t>(counts[2 * i]) | (static_cast<uint64_t>(counts[2 * i + 1]) << 32);
    uint64_t total;
    const uint64_t ex = carry + k_scan<uint64_t>(v, sm, total);
    if (i < tiles) {
      counts[2 * i] = static_cast<uint32_t>(ex);
      counts[2 * i + 1] = static_cast<uint32_t>(ex >> 32);
    }
    carry += total;
  }
}

// ---------------------------------------------------------------------------------------
// the sent entries and the zeros they leave: blockIdx.x = chunk * kKChunk + tile of the chunk
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kKThreads) void topk_write_kernel(KArgs a) {
  constexpr int N = Format<T>::N;
  constexpr int W = sizeof(T) == 2 ? 1 : sizeof(T) / 4;  // 32-bit words per element (fp32, fp64)
  using K = typename KKey<T>::K;
  __shared__ uint32_t sm[kKWaves];
  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* cp = (const Span FEDAVG_AS_CONST*)(a.chunks + blockIdx.x / kKChunk);
  const int off = static_cast<int>(blockIdx.x % kKChunk) * kKTile;
  const int32_t seg = cp->seg;
  if (off >= cp->count) return;  // the chunk at a tensor's end has fewer tiles
  const int n = cp->count - off < kKTile ? cp->count - off : kKTile;
  const int64_t start = cp->start + off;
  const KTensor FEDAVG_AS_CONST* tp = (const KTensor FEDAVG_AS_CONST*)(a.tensors + seg);
  const uint64_t tau64 = a.state[seg].prefix;
  if (tau64 == ~0ull) return;  // keep == 0
  const K tau = static_cast<K>(tau64);
  const uint32_t r = a.state[seg].want;
  const uint32_t keep = static_cast<uint32_t>(tp->keep);
  void* const residual = tp->residual;
  int32_t* const indices = tp->indices;
  uint16_t FEDAVG_AS_GLOBAL* const values16 = (uint16_t FEDAVG_AS_GLOBAL*)tp->values;
  uint32_t FEDAVG_AS_GLOBAL* const values32 = (uint32_t FEDAVG_AS_GLOBAL*)tp->values;
  uint16_t FEDAVG_AS_GLOBAL* const res16 = (uint16_t FEDAVG_AS_GLOBAL*)residual;
  uint32_t FEDAVG_AS_GLOBAL* const res32 = (uint32_t FEDAVG_AS_GLOBAL*)residual;
  const uint32_t* const pre = a.counts + 2 * (tp->first_tile + start / kKTile);
  uint32_t gt_base = pre[0], eq_base = pre[1];
  // once r equal keys have gone and no larger key is left in the tensor the rest is residual; the
  // loop still runs to its end: its bounds are the same for every lane
  for (int row = 0; row < n; row += kKThreads * N) {
    const int p = row + t * N;
    const int have = n - p < 0 ? 0 : (n - p < N ? n - p : N);
    u32x4 raw = {0u, 0u, 0u, 0u};
    if (have > 0) raw = k_load<T>(residual, start + p, have);
    uint32_t c = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i >= have) continue;
      const K key = KKey<T>::key(raw, i);
      c += (key > tau ? 1u : 0u) + (key == tau ? 0x10000u : 0u);
    }
    uint32_t total;
    const uint32_t ex = k_scan<uint32_t>(c, sm, total);
    uint32_t gt = gt_base + (ex & 0xffffu), eq = eq_base + (ex >> 16);
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i >= have) continue;
      const K key = KKey<T>::key(raw, i);
      const bool g = key > tau, q = key == tau;
      const bool sent = g || (q && eq < r);
      if (sent) {
        const uint32_t pos = gt + (eq < r ? eq : r);
        if (pos < keep) {  // always: the counts of the passes before say so
          const int64_t e = start + p + i;
          indices[pos] = static_cast<int32_t>(e);
          if constexpr (sizeof(T) == 2) {
            values16[pos] = static_cast<uint16_t>(raw[i / 2] >> (16 * (i % 2)));
            res16[e] = 0;
          } else {
#pragma unroll
            for (int w = 0; w < W; ++w) {
              values32[static_cast<int64_t>(pos) * W + w] = raw[i * W + w];
              res32[e * W + w] = 0u;
            }
          }
        }
      }
      gt += g ? 1u : 0u;
      eq += q ? 1u : 0u;
    }
    gt_base += total & 0xffffu;
    eq_base += total >> 16;
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct TopkState {
  char* d_work = nullptr;  // the partials, the select states and the tile counts of the call in flight
  size_t work_cap = 0;
  TableRing ring;
  ~TopkState() {
    ring.release();
    if (d_work) (void)hipFree(d_work);
  }
};

int32_t ensure_state(void** slot, TopkState** out) {
  if (*slot == nullptr) {
    TopkState* st = new TopkState();
    const int32_t r = hip_status("top-k state", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<TopkState*>(*slot);
  return FEDAVG_OK;
}

// hipFree waits for the device: no launch still reads the old buffer
int32_t grow(TopkState* st, size_t need) {
  if (st->work_cap >= need) return FEDAVG_OK;
  if (st->d_work) FEDAVG_TRY_HIP(hipFree(st->d_work));
  st->d_work = nullptr;
  st->work_cap = 0;
  const size_t n = need * 2 < (size_t(1) << 16) ? (size_t(1) << 16) : need * 2;
  FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&st->d_work), n));
  st->work_cap = n;
  return FEDAVG_OK;
}

size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

template <typename T>
void launch_all(unsigned chunks, unsigned tensors, hipStream_t s, KArgs a) {
  const dim3 block(kKThreads);
  int shift = 0;
  for (int p = 0; p < KKey<T>::kPasses; ++p) shift += KKey<T>::kDigits[p];
  for (int p = 0; p < KKey<T>::kPasses; ++p) {
    a.bits = KKey<T>::kDigits[p];
    shift -= a.bits;
    a.shift = shift;
    a.first = p == 0;
    if (chunks > 0) {
      if (p == 0) hipLaunchKernelGGL((topk_hist_kernel<T, true>), dim3(chunks), block, 0, s, a);
      else hipLaunchKernelGGL((topk_hist_kernel<T, false>), dim3(chunks), block, 0, s, a);
    }
    hipLaunchKernelGGL(topk_select_kernel, dim3(tensors), block, 0, s, a);
  }
  if (chunks > 0) {
    hipLaunchKernelGGL((topk_count_kernel<T>), dim3(chunks), block, 0, s, a);
    hipLaunchKernelGGL(topk_scan_kernel, dim3(tensors), block, 0, s, a);
    hipLaunchKernelGGL((topk_write_kernel<T>), dim3(chunks * kKChunk), block, 0, s, a);
  }
}

}  // namespace

int32_t fedavg_internal_topk_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "topk_tile") *out = kKTile;
  else if (n == "topk_chunk") *out = kKChunk;
  else if (n == "topk_threads") *out = kKThreads;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_topk_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<TopkState*>(state);
}

extern "C" int32_t fedavg_topk_sparsify(fedavg_ctx* ctx, int32_t dtype, const void* const* delta_ptrs,
                                        const void* const* error_ptrs, const int64_t* numels, const int64_t* keeps,
                                        int32_t num_tensors, int32_t* const* index_ptrs, void* const* value_ptrs,
                                        void* const* residual_ptrs, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_TOPK, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (dtype != FEDAVG_F32 && dtype != FEDAVG_F16 && dtype != FEDAVG_BF16 && dtype != FEDAVG_F64)
    return invalid("the top-k step takes fp32, fp16, bf16 or fp64 tensors");
  if (delta_ptrs == nullptr || numels == nullptr || keeps == nullptr || index_ptrs == nullptr ||
      value_ptrs == nullptr || residual_ptrs == nullptr)
    return invalid("null delta, count, index, value or residual table");
  if (num_tensors < 1 || num_tensors > kKMaxTensors)
    return invalid("the top-k step takes between 1 and " + std::to_string(kKMaxTensors) + " tensors");
  const int T = num_tensors;
  const size_t esize = dtype == FEDAVG_F64 ? 8 : (dtype == FEDAVG_F32 ? 4 : 2);
  constexpr int64_t kChunkElems = static_cast<int64_t>(kKChunk) * kKTile;
  uint64_t num_tiles = 0, num_chunks = 0;
  for (int t = 0; t < T; ++t) {
    const std::string who = "tensor " + std::to_string(t);
    if (numels[t] < 0 || keeps[t] < 0) return invalid(who + ": negative element count or keep count");
    if (numels[t] > 0x7fffffffll) return invalid(who + ": more than 2^31 - 1 elements (the indices are int32)");
    if (keeps[t] > numels[t]) return invalid(who + ": keeps more entries than it has elements");
    if (numels[t] > 0 && (delta_ptrs[t] == nullptr || residual_ptrs[t] == nullptr))
      return invalid(who + ": null delta or residual");
    if (keeps[t] > 0 && (index_ptrs[t] == nullptr || value_ptrs[t] == nullptr))
      return invalid(who + ": null index or value buffer");
    if (misaligned(delta_ptrs[t], esize) || misaligned(residual_ptrs[t], esize) || misaligned(value_ptrs[t], esize) ||
        (error_ptrs != nullptr && misaligned(error_ptrs[t], esize)) || misaligned(index_ptrs[t], sizeof(int32_t)))
      return invalid(who + ": a buffer is not aligned to its element size");
    num_tiles += (static_cast<uint64_t>(numels[t]) + kKTile - 1) / kKTile;
    num_chunks += (static_cast<uint64_t>(numels[t]) + kChunkElems - 1) / kChunkElems;
  }
  if (num_chunks * kKChunk > 0x7fffffffull) return invalid("layout too large for one top-k call");

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  TopkState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the workspace: [chunks][kKBins] partials, [T] states, [tiles][2] counts
  const size_t part_bytes = align16(sizeof(uint32_t) * kKBins * num_chunks);
  const size_t state_bytes = align16(sizeof(KState) * static_cast<size_t>(T));
  const size_t count_bytes = align16(sizeof(uint32_t) * 2 * num_tiles);
  FEDAVG_TRY(grow(st, part_bytes + state_bytes + count_bytes));

  // the call's tables: the chunks, then one KTensor per tensor
  const size_t chunk_bytes = align16(sizeof(Span) * num_chunks);
  const size_t bytes = chunk_bytes + align16(sizeof(KTensor) * static_cast<size_t>(T));
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memset(sl.host, 0, bytes);
  Span* const h_chunks = reinterpret_cast<Span*>(sl.host);
  KTensor* const h_tensors = reinterpret_cast<KTensor*>(sl.host + chunk_bytes);
  size_t k = 0;
  uint64_t tile = 0;
  for (int t = 0; t < T; ++t) {
    KTensor& kt = h_tensors[t];
    kt.delta = delta_ptrs[t];
    kt.error = error_ptrs != nullptr ? error_ptrs[t] : nullptr;
    kt.residual = residual_ptrs[t];
    kt.indices = index_ptrs[t];
    kt.values = value_ptrs[t];
    kt.numel = numels[t];
    kt.keep = keeps[t];
    kt.first_tile = static_cast<int32_t>(tile);
    kt.first_chunk = static_cast<int32_t>(k);
    for (int64_t b = 0; b < numels[t]; b += kChunkElems) {
      const int64_t left = numels[t] - b;
      h_chunks[k++] = Span{t, static_cast<int32_t>(left < kChunkElems ? left : kChunkElems), b};
    }
    kt.num_chunks = static_cast<int32_t>(k) - kt.first_chunk;
    tile += (static_cast<uint64_t>(numels[t]) + kKTile - 1) / kKTile;
  }
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  KArgs a;
  a.chunks = reinterpret_cast<const Span*>(sl.dev);
  a.tensors = reinterpret_cast<const KTensor*>(sl.dev + chunk_bytes);
  a.part = reinterpret_cast<uint32_t*>(st->d_work);
  a.state = reinterpret_cast<KState*>(st->d_work + part_bytes);
  a.counts = reinterpret_cast<uint32_t*>(st->d_work + part_bytes + state_bytes);
  a.shift = a.bits = a.first = 0;
  const unsigned g1 = static_cast<unsigned>(num_chunks), g2 = static_cast<unsigned>(T);
  if (dtype == FEDAVG_F32) launch_all<float>(g1, g2, s, a);
  else if (dtype == FEDAVG_F16) launch_all<__half>(g1, g2, s, a);
  else if (dtype == FEDAVG_BF16) launch_all<bf16_t>(g1, g2, s, a);
  else launch_all<double>(g1, g2, s, a);
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("top-k launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}
