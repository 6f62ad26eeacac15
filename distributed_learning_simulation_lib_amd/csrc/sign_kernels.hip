// sign_kernels.hip — gfx950 (MI355X) kernels of 1-bit sign compression with error feedback
// (EF-signSGD: Karimireddy, Rebjock, Stich, Jaggi, ICML 2019): the client step fedavg_sign_compress
// and the server fold fedavg_sign_aggregate_delta (include/fedavg_hip.h). The contract is DESIGN.md
// §5w; the oracle of the client step is the CPU path of sign.sign_compress, the oracle of the fold is
// fedavg_aggregate_delta on the densified deltas.
//
// A sign delta of a tensor is one bit per element and one magnitude: element e is bit e % 64 of the
// 64-bit word e / 64, and stands for -scale where the bit is set and +scale elsewhere. A 64-bit word
// is therefore a wave's lane mask of 64 consecutive elements: both kernels are built on that.
//
// The client step, three launches whatever the number of tensors:
//   * sign_abs_kernel: total = delta + error rounded once into the dtype, a = |total| widened to
//     fp64, and the sum of a over a piece of kDTile elements in the pinned order of fedavg_dp_noise
//     (lane j of 256 owns the 16-byte groups j, j + 256, ... and adds their elements in increasing
//     index, then the adjacent-pair tree). All arithmetic is fp64: the fp64 sum of two fp32 / fp16 /
//     bf16 values rounded to nearest even into the dtype is the correctly rounded sum (53 >= 2 * 24 + 2).
//   * sign_scale_kernel: one workgroup per tensor adds the tensor's piece partials (lane j the
//     partials j, j + 256, ..., the same tree), divides by the element count and rounds into the dtype.
//   * sign_apply_kernel: a 64-lane wave owns one piece = 64 words. Lane l holds element 64 k + l of
//     word k, so __ballot(sign bit) IS word k; the wave loads kGUnroll words' worth of elements per
//     lane (each load one coalesced wave access of 64 elements) before the first ballot, keeps ballot k
//     in lane k, and stores the piece's words with one 8-byte-per-lane store. The residual is written
//     by the lane that read the element; lanes past the tensor's end vote 0, so the last word's
//     padding bits are 0.
//
// The fold: a 256-lane workgroup owns a tile of kSgTile elements, a wave kSgWords consecutive words
// of it: lane l holds the kSgWords elements 64 k + l, their fp64 base values and accumulators in
// registers. The clients go through in batches of kSgBatch: the batch's words of the tile (16 bytes
// per lane and load), its scales widened to fp64 and its weights are staged in LDS; a wave then reads
// word (i, k) as an LDS broadcast, moves it into a scalar register pair and uses it as the lane mask
// of one select on the high word of the scale: d = bit ? -s : +s. Per client and element that is the
// select and three fp64 operations: x = b + d, p = x * w, acc = acc + p. acc starts at -0.0, which
// is the identity of the IEEE add for every p (signed zeros included), so the first product starts
// the sum bit for bit. No atomics.
//
// The majority vote (signSGD with majority vote: Bernstein, Wang, Azizzadenesheli, Anandkumar, ICML
// 2018; fedavg_sign_majority_vote) has no floating point until its last step. A
// workgroup is one wave and owns a tile of kVtTile elements = 64 words; lane l owns word l, that is
// 64 consecutive elements, and keeps their 64 vote counts bit-sliced: plane p is a 64-bit register
// pair that holds bit p of all 64 counts. A client's word is loaded by the lane that owns it (8 bytes
// per lane, one contiguous 512-byte line per wave and client, kVtLoads clients in flight) and the
// clients go into the planes kVtGroup at a time through a carry-save adder tree (Harley-Seal), so the
// carry ripples through the upper planes once per group. A bit-serial comparator against n / 2 then
// gives the lane's two masks (2c > n, 2c == n), which are the packed outputs as they stand. For the
// dense model the masks change hands: word k goes from lane k into a scalar register pair and is the
// wave's lane mask of the elements 64 k + l, so the base loads and the output stores are whole
// coalesced wave accesses and one select takes b itself on a tie. No LDS, no barrier, no atomics.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>

#include "call_tables.h"
#include "device_common.h"

namespace {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------------------
constexpr int kGWaves = kDThreads / 64;    // pieces per workgroup of the apply pass
constexpr int kGWords = kDTile / 64;       // words of a piece: one per lane of the wave that owns it
constexpr int kGUnroll = 8;                // words whose elements a lane loads before the first ballot
constexpr int kGMaxTensors = 1 << 20;
static_assert(kGWords == 64, "a wave keeps word k of its piece in lane k");
static_assert(kGWords % kGUnroll == 0, "whole rounds of loads");

constexpr int kSgThreads = 256;
constexpr int kSgWaves = kSgThreads / 64;
// K and the batch are -D overridable for tuning builds (build.py `defines`); DESIGN.md §5w has the runs
#ifndef FEDAVG_SIGN_WORDS
#define FEDAVG_SIGN_WORDS 4
#endif
#ifndef FEDAVG_SIGN_BATCH
#define FEDAVG_SIGN_BATCH 64
#endif
constexpr int kSgWords = FEDAVG_SIGN_WORDS;          // K: words (= elements per lane) of a wave
constexpr int kSgTileWords = kSgWaves * kSgWords;    // words of a tile
constexpr int kSgTile = kSgTileWords * 64;           // elements per workgroup
constexpr int kSgBatch = FEDAVG_SIGN_BATCH;          // clients staged in LDS between two pairs of barriers
constexpr int kSgMaxClients = FEDAVG_POINT_MAX_CLIENTS;
static_assert(kSgWords % 2 == 0, "a client's words are staged and read 16 bytes at a time");
static_assert(kSgBatch <= kSgThreads, "one lane stages one client's scale and weight");

// ---------------------------------------------------------------------------------------
// one element in and out, through the shared 16-byte image helpers
// ---------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ u32x4 g_load(const void* base, int64_t e) {
  u32x4 raw = {0u, 0u, 0u, 0u};
  if constexpr (sizeof(T) == 2) raw[0] = ((const uint16_t FEDAVG_AS_GLOBAL*)base)[e];
  else if constexpr (sizeof(T) == 4) raw[0] = ((const uint32_t FEDAVG_AS_GLOBAL*)base)[e];
  else {
    const uint64_t b = ((const uint64_t FEDAVG_AS_GLOBAL*)base)[e];
    raw[0] = static_cast<uint32_t>(b);
    raw[1] = static_cast<uint32_t>(b >> 32);
  }
  return raw;
}

template <typename T>
__device__ __forceinline__ void g_store(void* base, int64_t e, const u32x4& raw) {
  if constexpr (sizeof(T) == 2) ((uint16_t FEDAVG_AS_GLOBAL*)base)[e] = static_cast<uint16_t>(raw[0]);
  else if constexpr (sizeof(T) == 4) ((uint32_t FEDAVG_AS_GLOBAL*)base)[e] = raw[0];
  else ((uint64_t FEDAVG_AS_GLOBAL*)base)[e] = static_cast<uint64_t>(raw[0]) | (static_cast<uint64_t>(raw[1]) << 32);
}

// RNE(o) into T as a one-element image
template <typename T>
__device__ __forceinline__ u32x4 g_round(double o) {
  u32x4 raw = {0u, 0u, 0u, 0u};
  dp_put<T>(raw, 0, o);
  return raw;
}

// the sign bit of element 0 of an image
template <typename T>
__device__ __forceinline__ bool g_negative(const u32x4& raw) {
  if constexpr (sizeof(T) == 2) return (raw[0] & 0x8000u) != 0;
  else if constexpr (sizeof(T) == 4) return (raw[0] >> 31) != 0;
  else return (raw[1] >> 31) != 0;
}

// total[e] as an image: delta[e] itself, or delta[e] + error[e] rounded once into T
template <typename T>
__device__ __forceinline__ u32x4 g_total(const u32x4& d, const u32x4& e, bool has_error, int i) {
  if (!has_error) {
    u32x4 one = {0u, 0u, 0u, 0u};
    if constexpr (sizeof(T) == 2) one[0] = (d[i / 2] >> (16 * (i % 2))) & 0xffffu;
    else if constexpr (sizeof(T) == 4) one[0] = d[i];
    else {
      one[0] = d[2 * i];
      one[1] = d[2 * i + 1];
    }
    return one;
  }
  const double s = Format<T>::value(d, i) + Format<T>::value(e, i);
  return g_round<T>(s);
}

struct GTensor {
  const void* delta;
  const void* error;  // NULL: no residual yet
  void* residual;
  uint64_t* bits;     // ceil(numel / 64) words
  void* scale;        // one element of the dtype
  int64_t numel;
  int32_t first_piece;  // of the call's piece list
  int32_t num_pieces;
};

struct GArgs {
  const Span* pieces;      // the pieces of every tensor, in list order
  const GTensor* tensors;  // [T]
  double* part;            // [pieces]
  double* scale64;         // [T]: the scales, widened
  uint32_t* flag;          // the context's NaN words (0 acc, 1 result, 2 input)
  int64_t num_pieces;
};

// ---------------------------------------------------------------------------------------
// client pass 1: the piece partials of sum |total|; blockIdx.x = piece
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kDThreads) void sign_abs_kernel(GArgs a) {
  constexpr int N = Format<T>::N;
  __shared__ double sm[kDThreads / 64];
  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* pp = (const Span FEDAVG_AS_CONST*)(a.pieces + blockIdx.x);
  const int32_t count = pp->count;
  const int64_t first = pp->start;
  const GTensor FEDAVG_AS_CONST* tp = (const GTensor FEDAVG_AS_CONST*)(a.tensors + pp->seg);
  const void* const delta = tp->delta;
  const void* const error = tp->error;
  const bool has_error = error != nullptr;
  double acc = 0.0;
  bool bad = false;
  for (int g = t; g * N < count; g += kDThreads) {
    const int64_t e = first + static_cast<int64_t>(g) * N;
    const int have = count - g * N < N ? count - g * N : N;
    const char* const pd = static_cast<const char*>(delta) + e * static_cast<int64_t>(sizeof(T));
    u32x4 d, r = {0u, 0u, 0u, 0u};
    if (have == N && (reinterpret_cast<uintptr_t>(pd) & 15u) == 0) d = *(const u32x4 FEDAVG_AS_GLOBAL*)pd;
    else d = load_guarded<T>(delta, e, have);
    if (has_error) {
      const char* const pe = static_cast<const char*>(error) + e * static_cast<int64_t>(sizeof(T));
      if (have == N && (reinterpret_cast<uintptr_t>(pe) & 15u) == 0) r = *(const u32x4 FEDAVG_AS_GLOBAL*)pe;
      else r = load_guarded<T>(error, e, have);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {  // past `have`: +0.0, which changes nothing
      const u32x4 tot = g_total<T>(d, r, has_error, i);
      const double x = __builtin_fabs(Format<T>::value(tot, 0));
      bad |= !(x < __builtin_huge_val());
      acc = acc + x;
    }
  }
  acc = dp_tree(acc, kDThreads, sm);
  if (t == 0) a.part[blockIdx.x] = acc;
  if (__ballot(bad) != 0ull && (t & 63) == 0) raise_flag(a.flag, 2);
}

// ---------------------------------------------------------------------------------------
// client pass 2: scale = RNE((sum of the partials) / numel); blockIdx.x = tensor
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kDThreads) void sign_scale_kernel(GArgs a) {
  __shared__ double sm[kDThreads / 64];
  const int t = static_cast<int>(threadIdx.x);
  const GTensor FEDAVG_AS_CONST* tp = (const GTensor FEDAVG_AS_CONST*)(a.tensors + blockIdx.x);
  const double* const part = a.part + tp->first_piece;
  const int k = tp->num_pieces;
  double acc = 0.0;
  for (int i = t; i < k; i += kDThreads) acc = acc + part[i];
  acc = dp_tree(acc, kDThreads, sm);
  if (t == 0) {
    const double s64 = acc / static_cast<double>(tp->numel);  // numel < 2^31: exact
    const u32x4 img = g_round<T>(s64);
    g_store<T>(tp->scale, 0, img);
    a.scale64[blockIdx.x] = Format<T>::value(img, 0);
  }
}

// ---------------------------------------------------------------------------------------
// client pass 3: the bits and the residual; wave w of workgroup b owns piece b * kGWaves + w
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kDThreads) void sign_apply_kernel(GArgs a) {
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int64_t piece = static_cast<int64_t>(blockIdx.x) * kGWaves + (static_cast<int>(threadIdx.x) >> 6);
  if (piece >= a.num_pieces) return;  // the same for the whole wave; the kernel has no barrier
  const Span FEDAVG_AS_CONST* pp = (const Span FEDAVG_AS_CONST*)(a.pieces + piece);
  const int32_t seg = pp->seg, count = pp->count;
  const int64_t start = pp->start;  // a multiple of kDTile: the piece's first word is start / 64
  const GTensor FEDAVG_AS_CONST* tp = (const GTensor FEDAVG_AS_CONST*)(a.tensors + seg);
  const void* const delta = tp->delta;
  const void* const error = tp->error;
  void* const residual = tp->residual;
  const bool has_error = error != nullptr;
  const double scale = a.scale64[seg];
  const double minus = -scale;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  uint64_t word = 0;  // lane k: word k of the piece
#pragma unroll 1
  for (int k0 = 0; k0 * 64 < count; k0 += kGUnroll) {
    u32x4 d[kGUnroll], r[kGUnroll];
#pragma unroll
    for (int u = 0; u < kGUnroll; ++u) {  // all loads of the round before its first ballot
      const int p = (k0 + u) * 64 + lane;
      const bool live = p < count;
      d[u] = live ? g_load<T>(delta, start + p) : zero;
      r[u] = (live && has_error) ? g_load<T>(error, start + p) : zero;
    }
#pragma unroll
    for (int u = 0; u < kGUnroll; ++u) {
      const int p = (k0 + u) * 64 + lane;
      const bool live = p < count;
      const u32x4 tot = g_total<T>(d[u], r[u], has_error, 0);
      const bool neg = live && g_negative<T>(tot);
      const uint64_t vote = __ballot(neg);
      if (lane == k0 + u) word = vote;
      if (live) {
        const double o = Format<T>::value(tot, 0) - (neg ? minus : scale);
        g_store<T>(residual, start + p, g_round<T>(o));
      }
    }
  }
  if (lane * 64 < count) ((uint64_t FEDAVG_AS_GLOBAL*)tp->bits)[start / 64 + lane] = word;
}

// ---------------------------------------------------------------------------------------
// the fold: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
struct SgArgs {
  const Span* tiles;
  const uint64_t* const* bits;  // [n][num_segments]
  const void* const* scales;    // [n][num_segments]: one scalar of the scale dtype each
  const double* const* base;    // [num_segments]
  void* const* outs;            // [num_segments]
  const double* w;              // [n]
  double divisor;
  uint32_t* flag;               // the context's NaN words (0 acc, 1 result, 2 input)
  int32_t num_segments;
  int32_t n;
  int32_t scale_dtype;
};

__device__ __forceinline__ double sg_scale(const void* p, int32_t dtype) {
  if (dtype == FEDAVG_F64) return *(const double FEDAVG_AS_GLOBAL*)p;
  if (dtype == FEDAVG_F32) return static_cast<double>(*(const float FEDAVG_AS_GLOBAL*)p);
  const uint32_t h = *(const uint16_t FEDAVG_AS_GLOBAL*)p;
  if (dtype == FEDAVG_F16) return static_cast<double>(__half2float(__ushort_as_half(static_cast<unsigned short>(h))));
  return static_cast<double>(__uint_as_float(h << 16));
}

// The clients [0, m) of the staged batch into the wave's accumulators, in table order. kCheck: a
// staged scale is not finite, so x can be NaN where the base is not: look at every x.
template <bool kCheck>
__device__ __forceinline__ void sg_fold_batch(int m, const uint64_t* words, const double* ss, const double* ws,
                                              const double (&b)[kSgWords], double (&acc)[kSgWords], bool& nan_in) {
#pragma unroll 2
  for (int i = 0; i < m; ++i) {
    const double s = ss[i], w = ws[i];  // LDS broadcasts
    const uint64_t sb = static_cast<uint64_t>(__double_as_longlong(s));
    const uint32_t lo = static_cast<uint32_t>(sb), hi = static_cast<uint32_t>(sb >> 32);
    const uint32_t hi_neg = hi ^ 0x80000000u;
    const u64x2* const row = reinterpret_cast<const u64x2*>(words + i * kSgTileWords);
#pragma unroll
    for (int k = 0; k < kSgWords; k += 2) {
      const u64x2 pair = row[k / 2];  // every lane of the wave reads the same 16 bytes
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        // the word as the wave's lane mask, in a scalar register pair
        const uint32_t mlo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(pair[h]));
        const uint32_t mhi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(pair[h] >> 32));
        const bool neg = __builtin_amdgcn_inverse_ballot_w64((static_cast<uint64_t>(mhi) << 32) | mlo);
        const uint32_t dh = neg ? hi_neg : hi;
        const double d = __longlong_as_double(static_cast<long long>((static_cast<uint64_t>(dh) << 32) | lo));
        const double x = b[k + h] + d;
        if (kCheck) nan_in |= x != x;
        const double p = x * w;
        acc[k + h] = acc[k + h] + p;
      }
    }
  }
}

template <typename O>
__global__ __launch_bounds__(kSgThreads) void sign_fold_kernel(SgArgs a) {
  constexpr int K = kSgWords;
  constexpr int B = kSgBatch;
  constexpr int kUnits = kSgTileWords / 2;  // 16-byte units of a client's words of the tile
  __shared__ __attribute__((aligned(16))) uint64_t words[B * kSgTileWords];
  __shared__ double ss[B];
  __shared__ double ws[B];
  // set by a staging lane that meets a non-finite scale and never cleared: every later batch of the
  // workgroup then also compares each x, which costs time but changes no result
  __shared__ int careful;

  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63, wave = t >> 6;
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg, count = tp->count;
  const int64_t start = tp->start;  // a multiple of kSgTile
  const int n = a.n, T = a.num_segments;
  const int nw = (count + 63) >> 6;  // words of the tile that exist
  const int64_t word0 = start >> 6;
  if (t == 0) careful = 0;

  // the lane's elements: (wave * K + k) * 64 + lane; past the segment's end neither read nor written
  double b[K], acc[K];
  const double FEDAVG_AS_GLOBAL* pb = (const double FEDAVG_AS_GLOBAL*)a.base[seg] + start;
  bool nan_in = false;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = (wave * K + k) * 64 + lane;
    b[k] = e < count ? pb[e] : 0.0;
    nan_in |= b[k] != b[k];  // n >= 1: x_0 = b + d_0 is NaN
    acc[k] = -0.0;           // -0.0 + p == p bit for bit: the first product starts the sum
  }

#pragma unroll 1
  for (int c0 = 0; c0 < n; c0 += B) {
    const int m = n - c0 < B ? n - c0 : B;
    __syncthreads();  // the batch before has been folded (first batch: `careful` is clear)
    for (int j = t; j < m * kUnits; j += kSgThreads) {
      const int i = j / kUnits, u = j - i * kUnits;
      const uint64_t* const p = a.bits[static_cast<int64_t>(c0 + i) * T + seg] + word0 + 2 * u;
      u64x2 v = {0ull, 0ull};
      if (2 * u + 1 < nw && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
        v = *(const u64x2 FEDAVG_AS_GLOBAL*)p;
      } else {
        if (2 * u < nw) v[0] = ((const uint64_t FEDAVG_AS_GLOBAL*)p)[0];
        if (2 * u + 1 < nw) v[1] = ((const uint64_t FEDAVG_AS_GLOBAL*)p)[1];
      }
      *reinterpret_cast<u64x2*>(words + i * kSgTileWords + 2 * u) = v;
    }
    if (t < m) {
      const double s = sg_scale(a.scales[static_cast<int64_t>(c0 + t) * T + seg], a.scale_dtype);
      ss[t] = s;
      ws[t] = a.w[c0 + t];
      if (!(__builtin_fabs(s) < __builtin_huge_val())) careful = 1;
    }
    __syncthreads();
    const uint64_t* const mine = words + wave * K;
    if (careful) sg_fold_batch<true>(m, mine, ss, ws, b, acc, nan_in);
    else sg_fold_batch<false>(m, mine, ss, ws, b, acc, nan_in);
  }

  // out = acc / W
  bool nan_acc = false, nan_out = false, any = false;
  O FEDAVG_AS_GLOBAL* po = (O FEDAVG_AS_GLOBAL*)a.outs[seg] + start;
  const double divisor = a.divisor;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e = (wave * K + k) * 64 + lane;
    if (e < count) {
      any = true;
      const double s = acc[k];
      nan_acc |= s != s;
      const double r = s / divisor;
      nan_out |= r != r;
      po[e] = static_cast<O>(r);
    }
  }
  if (__ballot(nan_in && any) != 0ull && lane == 0) raise_flag(a.flag, 2);
  if (__ballot(nan_acc) != 0ull && lane == 0) raise_flag(a.flag, 0);
  if (__ballot(nan_out) != 0ull && lane == 0) raise_flag(a.flag, 1);
}

// ---------------------------------------------------------------------------------------
// the majority vote: blockIdx.x = tile, one wave per tile
// ---------------------------------------------------------------------------------------
constexpr int kVtThreads = 64;              // one wave: lane l owns word l of the tile
constexpr int kVtTile = kVtThreads * 64;    // elements per workgroup
constexpr int kVtGroup = 8;                 // clients a carry-save tree takes before one ripple
constexpr int kVtLoads = 16;                // clients whose words a lane has in flight
constexpr int kVtApply = 8;                 // words whose base values a lane has in flight
// planes of the three cases: n < 2^planes, so the count fits and n / 2 < 2^(planes - 1)
constexpr int kVtPlanesSmall = 3, kVtPlanesMid = 7, kVtPlanesAll = 11;
static_assert(kVtLoads % kVtGroup == 0 && kVtThreads % kVtApply == 0, "whole groups, whole rounds");
static_assert(kVtPlanesSmall >= 3, "the tree's ones, twos and fours are the planes 0, 1 and 2");
static_assert((1 << kVtPlanesAll) > kSgMaxClients, "the top plane holds the count of every client");

struct VtArgs {
  const Span* tiles;
  const uint64_t* const* bits;  // [n][num_segments]
  const double* const* base;    // [num_segments]
  void* const* outs;            // [num_segments]
  uint64_t* const* neg;         // [num_segments], or NULL: not asked for
  uint64_t* const* tie;         // [num_segments], or NULL
  const double* steps;          // [num_segments]
  uint32_t* flag;               // the context's NaN words (2: input)
  int32_t num_segments;
  int32_t n;
};

// a + b + c bit by bit: `lo` the sums, `hi` the carries
__device__ __forceinline__ void vt_csa(uint64_t& hi, uint64_t& lo, uint64_t a, uint64_t b, uint64_t c) {
  const uint64_t u = a ^ b;
  hi = (a & b) | (u & c);
  lo = u ^ c;
}

// The words w[G0 .. G0 + 8) of eight clients into the planes: seven carry-save adders leave the
// planes 0, 1, 2 and one word of weight 8, which ripples through the planes from 3 up. A word of a
// client past n is 0 and adds nothing. The carry out of the top plane is 0 because n < 2^P.
template <int P, int G0>
__device__ __forceinline__ void vt_add_group(uint64_t (&pl)[P], const uint64_t (&w)[kVtLoads]) {
  uint64_t ones = pl[0], twos = pl[1], fours = pl[2];
  uint64_t ta, tb, fa, fb, carry;
  vt_csa(ta, ones, ones, w[G0 + 0], w[G0 + 1]);
  vt_csa(tb, ones, ones, w[G0 + 2], w[G0 + 3]);
  vt_csa(fa, twos, twos, ta, tb);
  vt_csa(ta, ones, ones, w[G0 + 4], w[G0 + 5]);
  vt_csa(tb, ones, ones, w[G0 + 6], w[G0 + 7]);
  vt_csa(fb, twos, twos, ta, tb);
  vt_csa(carry, fours, fours, fa, fb);
  pl[0] = ones;
  pl[1] = twos;
  pl[2] = fours;
#pragma unroll
  for (int p = 3; p < P; ++p) {
    const uint64_t t = pl[p] & carry;
    pl[p] ^= carry;
    carry = t;
  }
}

// word `k` of the wave (held by lane k) as the lane mask of the elements 64 k + lane
__device__ __forceinline__ bool vt_bit_of_word(uint32_t lo, uint32_t hi, int k) {
  const uint32_t mlo = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(lo), k));
  const uint32_t mhi = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(hi), k));
  return __builtin_amdgcn_inverse_ballot_w64((static_cast<uint64_t>(mhi) << 32) | mlo);
}

template <typename O, int P>
__global__ __launch_bounds__(kVtThreads) void sign_vote_kernel(VtArgs a) {
  const int lane = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg, count = tp->count;
  const int64_t start = tp->start;  // a multiple of kVtTile
  const int n = a.n, T = a.num_segments;
  const int nw = (count + 63) >> 6;  // words of the tile that exist: lanes past them load and store nothing
  const int64_t word0 = start >> 6;
  const bool mine = lane < nw;

  // the counts of the lane's 64 elements, bit-sliced
  uint64_t pl[P];
#pragma unroll
  for (int p = 0; p < P; ++p) pl[p] = 0ull;
#pragma unroll 1
  for (int c0 = 0; c0 < n; c0 += kVtLoads) {
    uint64_t w[kVtLoads];
#pragma unroll
    for (int i = 0; i < kVtLoads; ++i) {  // all loads of the round before its first adder
      w[i] = 0ull;
      if (c0 + i < n) {  // the same for the whole wave
        const uint64_t* const p = a.bits[static_cast<int64_t>(c0 + i) * T + seg] + word0;
        if (mine) w[i] = ((const uint64_t FEDAVG_AS_GLOBAL*)p)[lane];
      }
    }
    vt_add_group<P, 0>(pl, w);
    if (c0 + kVtGroup < n) vt_add_group<P, kVtGroup>(pl, w);
  }

  // c > h and c == h with h = floor(n / 2), from the top plane down: 2c > n is c > h for either
  // parity of n, 2c == n is c == h for an even n and never holds for an odd one
  const uint32_t h = static_cast<uint32_t>(n) >> 1;
  uint64_t gt = 0ull, eq = ~0ull;
#pragma unroll
  for (int p = P - 1; p >= 0; --p) {
    const uint64_t hb = ((h >> p) & 1u) ? ~0ull : 0ull;  // in scalar registers
    gt |= eq & pl[p] & ~hb;
    eq &= ~(pl[p] ^ hb);
  }
  // the bits past the tensor's end (garbage in the clients' words) are cleared
  const int left = count - lane * 64;
  const uint64_t valid = left >= 64 ? ~0ull : (left <= 0 ? 0ull : (1ull << left) - 1ull);
  const uint64_t neg = gt & valid;
  const uint64_t tie = (n & 1) ? 0ull : (eq & valid);
  if (mine) {
    if (a.neg != nullptr) ((uint64_t FEDAVG_AS_GLOBAL*)a.neg[seg])[word0 + lane] = neg;
    if (a.tie != nullptr) ((uint64_t FEDAVG_AS_GLOBAL*)a.tie[seg])[word0 + lane] = tie;
  }

  // the dense model: word k's masks go to every lane, lane l takes element 64 k + l
  const double s = a.steps[seg];
  const double minus = -s;
  const double FEDAVG_AS_GLOBAL* pb = (const double FEDAVG_AS_GLOBAL*)a.base[seg] + start;
  O FEDAVG_AS_GLOBAL* po = (O FEDAVG_AS_GLOBAL*)a.outs[seg] + start;
  const uint32_t nlo = static_cast<uint32_t>(neg), nhi = static_cast<uint32_t>(neg >> 32);
  const uint32_t tlo = static_cast<uint32_t>(tie), thi = static_cast<uint32_t>(tie >> 32);
  bool nan_in = false;
  // A round is kVtApply words. kFull: every element of the round exists, so the round has no branch
  // and its loads and stores are waited for one by one; the tensor's last round checks every element.
  auto round = [&](int k0, auto full) {
    constexpr bool kFull = decltype(full)::value;
    double b[kVtApply];
#pragma unroll
    for (int u = 0; u < kVtApply; ++u) {  // all loads of the round before its first store
      const int e = (k0 + u) * 64 + lane;
      b[u] = (kFull || e < count) ? pb[e] : 0.0;
    }
#pragma unroll
    for (int u = 0; u < kVtApply; ++u) {  // k0 + u <= 63: a word past nw has empty masks
      const int e = (k0 + u) * 64 + lane;
      const bool is_neg = vt_bit_of_word(nlo, nhi, k0 + u);
      const bool is_tie = vt_bit_of_word(tlo, thi, k0 + u);
      nan_in |= b[u] != b[u];
      const double r = b[u] + (is_neg ? minus : s);  // b + (-s) is b - s bit for bit
      const double o = is_tie ? b[u] : r;            // a tie keeps b itself: -0.0 stays -0.0
      if (kFull || e < count) po[e] = static_cast<O>(o);
    }
  };
  int k0 = 0;
#pragma unroll 1
  for (; (k0 + kVtApply) * 64 <= count; k0 += kVtApply) round(k0, std::true_type{});
  if (k0 < nw) round(k0, std::false_type{});  // fewer than kVtApply words are left
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct SignState {
  Span* d_tiles = nullptr;  // the fold's tiles of the context's layout
  int64_t num_tiles = 0;
  Span* d_vote_tiles = nullptr;  // the vote's
  int64_t num_vote_tiles = 0;
  char* d_work = nullptr;   // the piece partials and the widened scales of the compress call in flight
  size_t work_cap = 0;
  TableRing ring;
  ~SignState() {
    ring.release();
    if (d_tiles) (void)hipFree(d_tiles);
    if (d_vote_tiles) (void)hipFree(d_vote_tiles);
    if (d_work) (void)hipFree(d_work);
  }
};

int32_t ensure_state(void** slot, SignState** out) {
  if (*slot == nullptr) {
    SignState* st = new SignState();
    const int32_t r = hip_status("sign state", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<SignState*>(*slot);
  return FEDAVG_OK;
}

// hipFree waits for the device: no launch still reads the old buffer
int32_t grow(SignState* st, size_t need) {
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
void launch_compress(unsigned pieces, unsigned tensors, hipStream_t s, const GArgs& a) {
  const dim3 block(kDThreads);
  hipLaunchKernelGGL((sign_abs_kernel<T>), dim3(pieces), block, 0, s, a);
  hipLaunchKernelGGL((sign_scale_kernel<T>), dim3(tensors), block, 0, s, a);
  hipLaunchKernelGGL((sign_apply_kernel<T>), dim3((pieces + kGWaves - 1) / kGWaves), block, 0, s, a);
}

}  // namespace

int32_t fedavg_internal_sign_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "sign_tile") *out = kSgTile;
  else if (n == "sign_batch") *out = kSgBatch;
  else if (n == "sign_words") *out = kSgWords;
  else if (n == "sign_threads") *out = kSgThreads;
  else if (n == "vote_tile") *out = kVtTile;
  else if (n == "vote_threads") *out = kVtThreads;
  else if (n == "vote_group") *out = kVtGroup;
  else if (n == "vote_loads") *out = kVtLoads;
  else if (n == "vote_small_clients") *out = (1 << kVtPlanesSmall) - 1;
  else if (n == "vote_mid_clients") *out = (1 << kVtPlanesMid) - 1;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_sign_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<SignState*>(state);
}

extern "C" int32_t fedavg_sign_compress(fedavg_ctx* ctx, int32_t dtype, const void* const* delta_ptrs,
                                        const void* const* error_ptrs, const int64_t* numels, int32_t num_tensors,
                                        void* const* bit_ptrs, void* const* scale_ptrs, void* const* residual_ptrs,
                                        void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_SIGN, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (dtype != FEDAVG_F32 && dtype != FEDAVG_F16 && dtype != FEDAVG_BF16 && dtype != FEDAVG_F64)
    return invalid("the sign step takes fp32, fp16, bf16 or fp64 tensors");
  if (delta_ptrs == nullptr || numels == nullptr || bit_ptrs == nullptr || scale_ptrs == nullptr ||
      residual_ptrs == nullptr)
    return invalid("null delta, count, bit, scale or residual table");
  if (num_tensors < 1 || num_tensors > kGMaxTensors)
    return invalid("the sign step takes between 1 and " + std::to_string(kGMaxTensors) + " tensors");
  const int T = num_tensors;
  const size_t esize = dtype == FEDAVG_F64 ? 8 : (dtype == FEDAVG_F32 ? 4 : 2);
  uint64_t num_pieces = 0;
  for (int t = 0; t < T; ++t) {
    const std::string who = "tensor " + std::to_string(t);
    if (numels[t] < 1) return invalid(who + ": no elements (an empty tensor has scale +0.0 and no bits: the caller's)");
    if (numels[t] > 0x7fffffffll) return invalid(who + ": more than 2^31 - 1 elements");
    if (delta_ptrs[t] == nullptr || residual_ptrs[t] == nullptr || bit_ptrs[t] == nullptr || scale_ptrs[t] == nullptr)
      return invalid(who + ": null delta, residual, bit or scale buffer");
    if (misaligned(delta_ptrs[t], esize) || misaligned(residual_ptrs[t], esize) || misaligned(scale_ptrs[t], esize) ||
        (error_ptrs != nullptr && misaligned(error_ptrs[t], esize)))
      return invalid(who + ": a buffer is not aligned to its element size");
    if (misaligned(bit_ptrs[t], 8)) return invalid(who + ": the bit buffer is not 8-byte aligned");
    num_pieces += (static_cast<uint64_t>(numels[t]) + kDTile - 1) / kDTile;
  }
  if (num_pieces > 0x7fffffffull) return invalid("layout too large for one sign call");

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  SignState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the workspace: [pieces] partials, [T] widened scales
  const size_t part_bytes = align16(sizeof(double) * num_pieces);
  FEDAVG_TRY(grow(st, part_bytes + align16(sizeof(double) * static_cast<size_t>(T))));

  // the call's tables: the pieces, then one GTensor per tensor
  const size_t piece_bytes = align16(sizeof(Span) * num_pieces);
  const size_t bytes = piece_bytes + align16(sizeof(GTensor) * static_cast<size_t>(T));
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memset(sl.host, 0, bytes);
  Span* const h_pieces = reinterpret_cast<Span*>(sl.host);
  GTensor* const h_tensors = reinterpret_cast<GTensor*>(sl.host + piece_bytes);
  size_t k = 0;
  for (int t = 0; t < T; ++t) {
    GTensor& g = h_tensors[t];
    g.delta = delta_ptrs[t];
    g.error = error_ptrs != nullptr ? error_ptrs[t] : nullptr;
    g.residual = residual_ptrs[t];
    g.bits = static_cast<uint64_t*>(bit_ptrs[t]);
    g.scale = scale_ptrs[t];
    g.numel = numels[t];
    g.first_piece = static_cast<int32_t>(k);
    for (int64_t b = 0; b < numels[t]; b += kDTile) {
      const int64_t left = numels[t] - b;
      h_pieces[k++] = Span{t, static_cast<int32_t>(left < kDTile ? left : kDTile), b};
    }
    g.num_pieces = static_cast<int32_t>(k) - g.first_piece;
  }
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  GArgs a;
  a.pieces = reinterpret_cast<const Span*>(sl.dev);
  a.tensors = reinterpret_cast<const GTensor*>(sl.dev + piece_bytes);
  a.part = reinterpret_cast<double*>(st->d_work);
  a.scale64 = reinterpret_cast<double*>(st->d_work + part_bytes);
  a.flag = v.d_flag;
  a.num_pieces = static_cast<int64_t>(num_pieces);
  const unsigned g1 = static_cast<unsigned>(num_pieces), g2 = static_cast<unsigned>(T);
  if (dtype == FEDAVG_F32) launch_compress<float>(g1, g2, s, a);
  else if (dtype == FEDAVG_F16) launch_compress<__half>(g1, g2, s, a);
  else if (dtype == FEDAVG_BF16) launch_compress<bf16_t>(g1, g2, s, a);
  else launch_compress<double>(g1, g2, s, a);
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("sign compress launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_sign_aggregate_delta(fedavg_ctx* ctx, const void* const* bit_ptrs,
                                               const void* const* scale_ptrs, int32_t scale_dtype,
                                               const double* weights, int32_t num_clients, double divisor,
                                               const double* const* base_ptrs, void* const* out_ptrs,
                                               int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_SIGN, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (scale_dtype != FEDAVG_F32 && scale_dtype != FEDAVG_F16 && scale_dtype != FEDAVG_BF16 && scale_dtype != FEDAVG_F64)
    return invalid("the sign fold reads fp32 / fp16 / bf16 / fp64 scales");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("the sign fold writes fp32 or fp64");
  if (bit_ptrs == nullptr || scale_ptrs == nullptr || weights == nullptr || base_ptrs == nullptr || out_ptrs == nullptr)
    return invalid("null bit table, scale table, weights, base or outputs");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kSgMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the sign fold takes at most " + std::to_string(kSgMaxClients));
  if (!(std::isfinite(divisor) && divisor > 0)) return invalid("the divisor must be finite and > 0");
  for (int32_t i = 0; i < num_clients; ++i)
    if (!std::isfinite(weights[i])) return invalid("weight " + std::to_string(i) + " is not finite");
  const int T = v.num_segments;
  const size_t scale_bytes = scale_dtype == FEDAVG_F64 ? 8 : scale_dtype == FEDAVG_F32 ? 4 : 2;
  const size_t out_bytes = out_dtype == FEDAVG_F64 ? 8 : 4;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (size_t i = 0; i < entries; ++i) {
    // the message is built only on a refusal: this loop runs n * T times on every call
    const auto where = [T, i] { return "client " + std::to_string(i / T) + ", segment " + std::to_string(i % T); };
    if (bit_ptrs[i] == nullptr || scale_ptrs[i] == nullptr) return invalid(where() + ": null bit buffer or scale");
    if (misaligned(bit_ptrs[i], 8)) return invalid(where() + ": the bit buffer is not 8-byte aligned");
    if (misaligned(scale_ptrs[i], scale_bytes)) return invalid(where() + ": the scale is not aligned to its element size");
  }
  for (int t = 0; t < T; ++t) {
    if (base_ptrs[t] == nullptr) return invalid("the base lacks segment " + std::to_string(t));
    if (misaligned(base_ptrs[t], 8)) return invalid("base tensor not aligned to fp64");
    if (out_ptrs[t] == nullptr) return invalid("null output pointer for segment " + std::to_string(t));
    if (misaligned(out_ptrs[t], out_bytes)) return invalid("output tensor not aligned to its element size");
    if (static_cast<const void*>(out_ptrs[t]) == static_cast<const void*>(base_ptrs[t]))
      return invalid("segment " + std::to_string(t) + ": the fold is not in-place (out == base)");
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  SignState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  if (st->d_tiles == nullptr)
    FEDAVG_TRY(span_table(v.seg_numel, v.num_segments, kSgTile, "sign fold", "sign tile table", &st->d_tiles,
                          &st->num_tiles));
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: [n][T] bit pointers, [n][T] scale pointers, [T] base pointers, [T] output
  // pointers, [n] weights
  const size_t ptr_bytes = sizeof(void*) * entries;
  const size_t seg_bytes = sizeof(void*) * static_cast<size_t>(T);
  const size_t w_bytes = sizeof(double) * static_cast<size_t>(num_clients);
  const size_t o_scale = ptr_bytes, o_base = 2 * ptr_bytes, o_out = o_base + seg_bytes, o_w = o_out + seg_bytes;
  const size_t bytes = o_w + w_bytes;
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, bit_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_scale, scale_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_base, base_ptrs, seg_bytes);
  std::memcpy(sl.host + o_out, out_ptrs, seg_bytes);
  std::memcpy(sl.host + o_w, weights, w_bytes);
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  SgArgs a;
  a.tiles = st->d_tiles;
  a.bits = reinterpret_cast<const uint64_t* const*>(sl.dev);
  a.scales = reinterpret_cast<const void* const*>(sl.dev + o_scale);
  a.base = reinterpret_cast<const double* const*>(sl.dev + o_base);
  a.outs = reinterpret_cast<void* const*>(sl.dev + o_out);
  a.w = reinterpret_cast<const double*>(sl.dev + o_w);
  a.divisor = divisor;
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  a.scale_dtype = scale_dtype;
  const dim3 grid(static_cast<unsigned>(st->num_tiles)), block(kSgThreads);
  if (st->num_tiles > 0) {
    if (out_dtype == FEDAVG_F32) hipLaunchKernelGGL((sign_fold_kernel<float>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((sign_fold_kernel<double>), grid, block, 0, s, a);
  }
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("sign fold launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}

namespace {

template <typename O>
void launch_vote(int n, unsigned tiles, hipStream_t s, const VtArgs& a) {
  const dim3 grid(tiles), block(kVtThreads);
  if (n < (1 << kVtPlanesSmall)) hipLaunchKernelGGL((sign_vote_kernel<O, kVtPlanesSmall>), grid, block, 0, s, a);
  else if (n < (1 << kVtPlanesMid)) hipLaunchKernelGGL((sign_vote_kernel<O, kVtPlanesMid>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((sign_vote_kernel<O, kVtPlanesAll>), grid, block, 0, s, a);
}

}  // namespace

extern "C" int32_t fedavg_sign_majority_vote(fedavg_ctx* ctx, const void* const* bit_ptrs, int32_t num_clients,
                                             const double* steps, const double* const* base_ptrs,
                                             void* const* out_ptrs, int32_t out_dtype, void* const* neg_ptrs,
                                             void* const* tie_ptrs, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_SIGN, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("the sign vote writes fp32 or fp64");
  if (bit_ptrs == nullptr || steps == nullptr || base_ptrs == nullptr || out_ptrs == nullptr)
    return invalid("null bit table, steps, base or outputs");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kSgMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the sign vote takes at most " + std::to_string(kSgMaxClients));
  const int T = v.num_segments;
  const size_t out_bytes = out_dtype == FEDAVG_F64 ? 8 : 4;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (size_t i = 0; i < entries; ++i) {
    // the message is built only on a refusal: this loop runs n * T times on every call
    const auto where = [T, i] { return "client " + std::to_string(i / T) + ", segment " + std::to_string(i % T); };
    if (bit_ptrs[i] == nullptr) return invalid(where() + ": null bit buffer");
    if (misaligned(bit_ptrs[i], 8)) return invalid(where() + ": the bit buffer is not 8-byte aligned");
  }
  for (int t = 0; t < T; ++t) {
    const std::string who = "segment " + std::to_string(t);
    if (!(std::isfinite(steps[t]) && steps[t] >= 0)) return invalid(who + ": the step must be finite and >= 0");
    if (base_ptrs[t] == nullptr) return invalid("the base lacks segment " + std::to_string(t));
    if (misaligned(base_ptrs[t], 8)) return invalid("base tensor not aligned to fp64");
    if (out_ptrs[t] == nullptr) return invalid("null output pointer for segment " + std::to_string(t));
    if (misaligned(out_ptrs[t], out_bytes)) return invalid("output tensor not aligned to its element size");
    if (static_cast<const void*>(out_ptrs[t]) == static_cast<const void*>(base_ptrs[t]))
      return invalid(who + ": the vote is not in-place (out == base)");
    for (void* const* masks : {neg_ptrs, tie_ptrs}) {
      if (masks == nullptr) continue;
      if (masks[t] == nullptr) return invalid(who + ": null mask buffer");
      if (misaligned(masks[t], 8)) return invalid(who + ": the mask buffer is not 8-byte aligned");
    }
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  SignState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  if (st->d_vote_tiles == nullptr)
    FEDAVG_TRY(span_table(v.seg_numel, v.num_segments, kVtTile, "sign vote", "sign vote tile table", &st->d_vote_tiles,
                          &st->num_vote_tiles));
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: [n][T] bit pointers, then [T] each: base, output, neg mask, tie mask pointers
  // (the masks' places stay empty where a table is not asked for), steps
  const size_t ptr_bytes = sizeof(void*) * entries;
  const size_t seg_bytes = sizeof(void*) * static_cast<size_t>(T);
  const size_t o_base = ptr_bytes, o_out = o_base + seg_bytes, o_neg = o_out + seg_bytes, o_tie = o_neg + seg_bytes;
  const size_t o_steps = o_tie + seg_bytes;
  const size_t bytes = o_steps + sizeof(double) * static_cast<size_t>(T);
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, bit_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_base, base_ptrs, seg_bytes);
  std::memcpy(sl.host + o_out, out_ptrs, seg_bytes);
  if (neg_ptrs != nullptr) std::memcpy(sl.host + o_neg, neg_ptrs, seg_bytes);
  if (tie_ptrs != nullptr) std::memcpy(sl.host + o_tie, tie_ptrs, seg_bytes);
  std::memcpy(sl.host + o_steps, steps, sizeof(double) * static_cast<size_t>(T));
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  VtArgs a;
  a.tiles = st->d_vote_tiles;
  a.bits = reinterpret_cast<const uint64_t* const*>(sl.dev);
  a.base = reinterpret_cast<const double* const*>(sl.dev + o_base);
  a.outs = reinterpret_cast<void* const*>(sl.dev + o_out);
  a.neg = neg_ptrs != nullptr ? reinterpret_cast<uint64_t* const*>(sl.dev + o_neg) : nullptr;
  a.tie = tie_ptrs != nullptr ? reinterpret_cast<uint64_t* const*>(sl.dev + o_tie) : nullptr;
  a.steps = reinterpret_cast<const double*>(sl.dev + o_steps);
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  if (st->num_vote_tiles > 0) {
    if (out_dtype == FEDAVG_F32) launch_vote<float>(num_clients, static_cast<unsigned>(st->num_vote_tiles), s, a);
    else launch_vote<double>(num_clients, static_cast<unsigned>(st->num_vote_tiles), s, a);
  }
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("sign vote launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}
