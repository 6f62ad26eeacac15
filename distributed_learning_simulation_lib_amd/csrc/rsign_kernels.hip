// rsign_kernels.hip — gfx950 (MI355X) kernels of randomly rotated 1-bit updates (DRIVE: Vargaftik et
// al., NeurIPS 2021; the random rotation of Suresh et al., ICML 2017): the client step
// fedavg_rsign_compress and the server fold fedavg_rsign_aggregate_delta (include/fedavg_hip.h). The
// contract is DESIGN.md §5ad; the oracle of both is the numpy restatement in rotated.py.
//
// A rotated sign delta of a tensor of n elements is cut into blocks of B = min(4096, max(64,
// next_pow2(n))) elements, the last one padded with +0.0: one bit per padded element, the sign of the
// block's randomised Walsh-Hadamard transform y = H_B (D u), and one magnitude per block. D is a
// diagonal of +-1 cut from a Philox4x32-10 stream that the server can restate; H_B is unnormalised and
// its levels h = 1, 2, 4, ..., B / 2 run in that order, every butterfly (a + b, a - b) two separately
// rounded fp64 operations, so the result does not depend on how the work is laid out.
//
// Both kernels share one layout. A 256-lane workgroup owns a tile of 4096 padded elements of one
// tensor, that is 4096 / B blocks, and keeps them in registers as fp64, 16 per lane: lane l of wave w
// holds the elements 1024 w + 64 k + l, k = 0 .. 15. A 64-bit word of bits is then the lane mask of
// one k (as in sign_kernels.hip), and the twelve levels fall into three kinds of exchange in
// ascending order:
//   * h = 1 .. 32, across the lanes of a wave: the partner's value comes by two 32-bit moves (DPP
//     quad_perm for 1 and 2, DPP row_ror:8 for 8, ds_swizzle for 4 and 16, ds_bpermute for 32) and the
//     butterfly is one add, new = other + (upper lane ? -own : own), which is a + b below and a - b
//     above bit for bit;
//   * h = 64 .. 512, inside a lane: the pairs (k, k + h / 64) of its own registers;
//   * h = 1024, 2048, across the waves: the tile goes through 32 KB of LDS once, at index
//     1024 w + 64 k + l, so every access is 64 consecutive doubles of one row and needs no padding
//     against bank conflicts; a lane reads the other three waves' values of its (k, l) and does both
//     levels from them (three adds for two levels).
// Levels h >= B are skipped (B is uniform in a workgroup). The diagonal of a word is itself a lane
// mask: the elements 128 j .. 128 j + 127 of a tensor take the bits of Philox block j, so the words 2 j
// and 2 j + 1 are the two 64-bit halves of one block, which every lane of the wave computes from
// wave-uniform values. No matrix instruction: a +-1 butterfly in fp64 with a pinned rounding order is
// not a product the MFMA unit can restate, its accumulation order being its own.
//
// The client step, one launch whatever the number of tensors: total = delta + error stays in
// registers from the load to the residual. After the first transform the 32 per-lane values |y_k| and
// y_k * y_k are added over the wave by a halving exchange (at lane bit j the lanes of a pair keep one
// half of the values each and send the other: 16 + 8 + 4 + 2 + 1 + 1 moves instead of 6 * 32), which is
// the adjacent-pair tree over the element index, the word sums go through LDS to wave 0, whose lane j
// finishes the tree of word j's block by cross-lane adds, forms the scale and hands it back through
// LDS. The bits are ballots, stored as whole 64-bit words by the lanes 0 .. 15 of a wave. Then
// v = -+scale goes through the same transform and the lane that read an element writes its residual.
//
// The fold, one launch for the layout: the clients go through in batches of kRsBatch; a batch's words
// of the tile, its scales (widened to fp64, one slot per word) and its weights are staged in LDS in
// one coalesced pass between two barriers, in the 32 KB that carry the cross-wave levels afterwards.
// Per client and word a wave reads the word as an LDS broadcast into a scalar register pair and uses
// it as the lane mask of one select on the sign of p = s * w ((-s) * w is -(s * w) bit for bit), so an
// element costs one fp64 add per client. acc starts at -0.0, the identity of the IEEE add. After the
// last batch m = acc / divisor goes through the transform once and out = base + D z. No atomics.
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
constexpr int kRsThreads = 256;
constexpr int kRsWaves = kRsThreads / 64;
constexpr int kRsTile = 4096;                    // padded elements per workgroup, both kernels
constexpr int kRsPer = kRsTile / kRsThreads;     // elements (= words of its wave) per lane
constexpr int kRsWords = kRsTile / 64;           // words of a tile
constexpr int kRsWaveSpan = kRsTile / kRsWaves;  // consecutive elements of a wave
constexpr int kRsMinBlock = 64;
// the batch is -D overridable for tuning builds (build.py `defines`)
#ifndef FEDAVG_RSIGN_BATCH
#define FEDAVG_RSIGN_BATCH 32
#endif
constexpr int kRsBatch = FEDAVG_RSIGN_BATCH;     // clients staged in LDS between two pairs of barriers
constexpr int kRsMaxClients = FEDAVG_POINT_MAX_CLIENTS;
constexpr int kRsMaxTensors = 1 << 20;
static_assert(kRsPer == 16 && kRsWaves == 4, "the levels 64 .. 512 are a lane's own, 1024 and 2048 the waves'");
static_assert(kRsBatch >= 1 && kRsBatch * 2 * kRsWords <= kRsTile, "a batch's words and scales fit the exchange buffer");
static_assert(kRsBatch <= kRsThreads, "one lane stages one client's weight");

// log2 of the block size of the tensor that the span (start, count) of kRsTile elements belongs to: a
// tensor with a second tile, or with more than 2048 elements, has blocks of 4096
__device__ __forceinline__ int rs_lg_block(int64_t start, int32_t count) {
  if (start > 0 || count > kRsTile / 2) return 12;
  return count <= kRsMinBlock ? 6 : 32 - __builtin_clz(static_cast<uint32_t>(count - 1));
}

// ---------------------------------------------------------------------------------------
// the value of lane (l ^ H): two 32-bit moves
// ---------------------------------------------------------------------------------------
template <int H>
__device__ __forceinline__ int rs_xor32(int v) {
  if constexpr (H == 1) return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);        // quad_perm:[1,0,3,2]
  else if constexpr (H == 2) return __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);   // quad_perm:[2,3,0,1]
  else if constexpr (H == 8) return __builtin_amdgcn_update_dpp(0, v, 0x128, 0xF, 0xF, false);  // row_ror:8
  else if constexpr (H == 4 || H == 16) return __builtin_amdgcn_ds_swizzle(v, 0x1F | (H << 10));  // and 31, xor H
  else return __shfl_xor(v, 32);
}

template <int H>
__device__ __forceinline__ double rs_xor(double v) {
  return __hiloint2double(rs_xor32<H>(__double2hiint(v)), rs_xor32<H>(__double2loint(v)));
}

// -v where `flip` is 0x80000000, v where it is 0
__device__ __forceinline__ double rs_flip(double v, uint32_t flip) {
  return __hiloint2double(__double2hiint(v) ^ static_cast<int>(flip), __double2loint(v));
}

// ---------------------------------------------------------------------------------------
// the transform of the tile's blocks, in place
// ---------------------------------------------------------------------------------------
template <int H>
__device__ __forceinline__ void rs_lane_level(double (&v)[kRsPer], int lane) {
  const uint32_t flip = (lane & H) ? 0x80000000u : 0u;
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) v[k] = rs_xor<H>(v[k]) + rs_flip(v[k], flip);
}

template <int J>
__device__ __forceinline__ void rs_reg_level(double (&v)[kRsPer]) {
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) {
    if ((k & (1 << J)) == 0) {
      const double a = v[k], b = v[k + (1 << J)];
      v[k] = a + b;
      v[k + (1 << J)] = a - b;
    }
  }
}

// xs: kRsTile doubles of LDS that no lane of the workgroup still reads for another purpose once it
// has reached this call's first barrier. lg is the same for the whole workgroup.
__device__ __forceinline__ void rs_transform(double (&v)[kRsPer], int lg, int lane, int wave, double* xs) {
  rs_lane_level<1>(v, lane);
  rs_lane_level<2>(v, lane);
  rs_lane_level<4>(v, lane);
  rs_lane_level<8>(v, lane);
  rs_lane_level<16>(v, lane);
  rs_lane_level<32>(v, lane);
  if (lg > 6) rs_reg_level<0>(v);
  if (lg > 7) rs_reg_level<1>(v);
  if (lg > 8) rs_reg_level<2>(v);
  if (lg > 9) rs_reg_level<3>(v);
  if (lg > 10) {
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kRsPer; ++k) xs[wave * kRsWaveSpan + k * 64 + lane] = v[k];
    __syncthreads();
    const uint32_t flip1 = (wave & 1) ? 0x80000000u : 0u, flip2 = (wave & 2) ? 0x80000000u : 0u;
    const double* const x1 = xs + (wave ^ 1) * kRsWaveSpan + lane;
    const double* const x2 = xs + (wave ^ 2) * kRsWaveSpan + lane;
    const double* const x3 = xs + (wave ^ 3) * kRsWaveSpan + lane;
    if (lg > 11) {
#pragma unroll
      for (int k = 0; k < kRsPer; ++k) {
        const double mine = x1[k * 64] + rs_flip(v[k], flip1);         // level 1024 of this wave
        const double other = x3[k * 64] + rs_flip(x2[k * 64], flip1);  // and of wave ^ 2, whose bit 0 is the same
        v[k] = other + rs_flip(mine, flip2);                           // level 2048
      }
    } else {
#pragma unroll
      for (int k = 0; k < kRsPer; ++k) v[k] = x1[k * 64] + rs_flip(v[k], flip1);
    }
  }
}

// bit k: D is -1 at the lane's element k. `first` is the tensor index of the wave's element 0, a
// multiple of 1024, so the words 2 j and 2 j + 1 of the wave are Philox block first / 128 + j.
__device__ __forceinline__ uint32_t rs_diagonal(int64_t first, uint32_t tid, uint32_t draw, uint32_t k0, uint32_t k1,
                                                int lane) {
  const uint64_t block0 = static_cast<uint64_t>(first) >> 7;
  uint32_t dm = 0u;
#pragma unroll
  for (int j = 0; j < kRsPer / 2; ++j) {
    const uint64_t block = block0 + j;
    const QWords q = q_philox(static_cast<uint32_t>(block), static_cast<uint32_t>(block >> 32), tid, draw, k0, k1);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint32_t word = (lane & 32) ? q.w[2 * h + 1] : q.w[2 * h];
      dm |= ((word >> (lane & 31)) & 1u) << (2 * j + h);
    }
  }
  return dm;
}

// ---------------------------------------------------------------------------------------
// one element in and out
// ---------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ double rs_load(const void* base, int64_t e) {
  if constexpr (sizeof(T) == 8) return ((const double FEDAVG_AS_GLOBAL*)base)[e];
  else if constexpr (sizeof(T) == 4) return static_cast<double>(((const float FEDAVG_AS_GLOBAL*)base)[e]);
  else {
    u32x4 raw = {0u, 0u, 0u, 0u};
    raw[0] = ((const uint16_t FEDAVG_AS_GLOBAL*)base)[e];
    return Format<T>::value(raw, 0);
  }
}

// RNE(o) into T at element e
template <typename T>
__device__ __forceinline__ void rs_store(void* base, int64_t e, double o) {
  u32x4 raw = {0u, 0u, 0u, 0u};
  dp_put<T>(raw, 0, o);
  if constexpr (sizeof(T) == 2) ((uint16_t FEDAVG_AS_GLOBAL*)base)[e] = static_cast<uint16_t>(raw[0]);
  else if constexpr (sizeof(T) == 4) ((uint32_t FEDAVG_AS_GLOBAL*)base)[e] = raw[0];
  else ((double FEDAVG_AS_GLOBAL*)base)[e] = o;
}

// o rounded once into T, as an fp64
template <typename T>
__device__ __forceinline__ double rs_round(double o) {
  if constexpr (sizeof(T) == 8) return o;
  u32x4 raw = {0u, 0u, 0u, 0u};
  dp_put<T>(raw, 0, o);
  return Format<T>::value(raw, 0);
}

struct RsTensor {
  const void* delta;
  const void* error;  // NULL: no residual yet
  void* residual;
  uint64_t* bits;     // n_pad / 64 words
  void* scales;       // one per block: fp64 for fp64 tensors, fp32 otherwise
  uint32_t id;        // the tensor's word of the Philox counter
};

struct RsEncArgs {
  const Span* pieces;       // the tiles of every tensor, in list order
  const RsTensor* tensors;  // [T]
  uint32_t* flag;           // the context's NaN words (0 acc, 1 result, 2 input)
  uint32_t k0, k1, draw;    // the two halves of the seed, the draw
  int32_t mode;
};

// One halving step of the wave sum at lane bit log2(H): of the 2 * M values the lower lane keeps the
// first M, the upper lane the last M, each adding its partner's copy.
template <int H, int M>
__device__ __forceinline__ void rs_halve(double (&a)[2 * kRsPer], int lane) {
  const bool up = (lane & H) != 0;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    const double send = up ? a[i] : a[i + M];
    const double keep = up ? a[i + M] : a[i];
    a[i] = keep + rs_xor<H>(send);
  }
}

// ---------------------------------------------------------------------------------------
// the client step; blockIdx.x = tile
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kRsThreads) void rsign_encode_kernel(RsEncArgs a) {
  using S = typename std::conditional<sizeof(T) == 8, double, float>::type;
  __shared__ double xs[kRsTile];
  __shared__ double sums[2 * kRsWords];  // the word sums of |y|, then of y * y
  __shared__ double sc[kRsWords];        // the scale of every word's block, widened
  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const Span FEDAVG_AS_CONST* pp = (const Span FEDAVG_AS_CONST*)(a.pieces + blockIdx.x);
  const int32_t count = pp->count;
  const int64_t start = pp->start;  // a multiple of kRsTile
  const RsTensor FEDAVG_AS_CONST* tp = (const RsTensor FEDAVG_AS_CONST*)(a.tensors + pp->seg);
  const void* const delta = tp->delta;
  const void* const error = tp->error;
  void* const residual = tp->residual;
  const bool has_error = error != nullptr;
  const int lg = rs_lg_block(start, count);
  const int padded = ((count + (1 << lg) - 1) >> lg) << lg;  // the tile's blocks are whole in the payload
  const int e0 = wave * kRsWaveSpan + lane;                  // the lane's element k is e0 + 64 k
  const uint32_t dm = rs_diagonal(start + wave * kRsWaveSpan, tp->id, a.draw, a.k0, a.k1, lane);

  // total, and u = D total (+0.0 past the tensor's end)
  double tot[kRsPer], v[kRsPer];
  bool bad = false;
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) {
    const int e = e0 + 64 * k;
    const bool live = e < count;
    double x = live ? rs_load<T>(delta, start + e) : 0.0;
    if (live && has_error) x = rs_round<T>(x + rs_load<T>(error, start + e));
    bad |= !(__builtin_fabs(x) < __builtin_huge_val());
    tot[k] = x;
    v[k] = rs_flip(x, live ? ((dm >> k) & 1u) << 31 : 0u);
  }
  rs_transform(v, lg, lane, wave, xs);

  // the bits: word k of the wave is the ballot of k, kept in lane k
  uint64_t word = 0ull;
  uint32_t neg = 0u;
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) {
    const bool n = __double2hiint(v[k]) < 0;
    const uint64_t vote = __ballot(n);
    if (lane == k) word = vote;
    neg |= (n ? 1u : 0u) << k;
  }
  if (lane < kRsPer && (wave * kRsPer + lane) * 64 < padded)
    ((uint64_t FEDAVG_AS_GLOBAL*)tp->bits)[(start >> 6) + wave * kRsPer + lane] = word;

  // the word sums of |y| and y * y: lane bits 0 .. 5 of the adjacent-pair tree
  {
    double s[2 * kRsPer];
#pragma unroll
    for (int k = 0; k < kRsPer; ++k) {
      s[k] = __builtin_fabs(v[k]);
      s[kRsPer + k] = v[k] * v[k];
    }
    rs_halve<1, 16>(s, lane);
    rs_halve<2, 8>(s, lane);
    rs_halve<4, 4>(s, lane);
    rs_halve<8, 2>(s, lane);
    rs_halve<16, 1>(s, lane);
    const double sum = s[0] + rs_xor<32>(s[0]);
    // the lane holds the sum (lane bit 0: of y * y) of the word whose bits 3, 2, 1, 0 are its bits 1, 2, 3, 4
    const int k = ((lane >> 1) & 1) * 8 + ((lane >> 2) & 1) * 4 + ((lane >> 3) & 1) * 2 + ((lane >> 4) & 1);
    if (lane < 32) sums[(lane & 1) * kRsWords + wave * kRsPer + k] = sum;
  }
  __syncthreads();
  if (wave == 0) {  // lane j: word j; the tree goes on over the words of a block
    const int m = 1 << (lg - 6);
    double l1 = sums[lane], l2 = sums[kRsWords + lane];
    if (m > 1) { l1 = l1 + rs_xor<1>(l1); l2 = l2 + rs_xor<1>(l2); }
    if (m > 2) { l1 = l1 + rs_xor<2>(l1); l2 = l2 + rs_xor<2>(l2); }
    if (m > 4) { l1 = l1 + rs_xor<4>(l1); l2 = l2 + rs_xor<4>(l2); }
    if (m > 8) { l1 = l1 + rs_xor<8>(l1); l2 = l2 + rs_xor<8>(l2); }
    if (m > 16) { l1 = l1 + rs_xor<16>(l1); l2 = l2 + rs_xor<16>(l2); }
    if (m > 32) { l1 = l1 + rs_xor<32>(l1); l2 = l2 + rs_xor<32>(l2); }
    const double B = static_cast<double>(1 << lg);
    const double sigma = a.mode == FEDAVG_RSIGN_UNBIASED ? l2 / l1 : l1 / B;
    const double s = l1 == 0.0 ? 0.0 : sigma / B;
    const S narrow = static_cast<S>(s);
    sc[lane] = static_cast<double>(narrow);
    if ((lane & (m - 1)) == 0 && lane * 64 < padded)
      ((S FEDAVG_AS_GLOBAL*)tp->scales)[(start >> lg) + (lane >> (lg - 6))] = narrow;
  }
  __syncthreads();

  // sent = D H (-+scale), residual = total - sent
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) v[k] = rs_flip(sc[wave * kRsPer + k], ((neg >> k) & 1u) << 31);
  rs_transform(v, lg, lane, wave, xs);
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) {
    const int e = e0 + 64 * k;
    if (e < count) {
      const double sent = rs_round<T>(rs_flip(v[k], ((dm >> k) & 1u) << 31));
      rs_store<T>(residual, start + e, tot[k] - sent);
    }
  }
  if (__ballot(bad) != 0ull && lane == 0) raise_flag(a.flag, 2);
}

// ---------------------------------------------------------------------------------------
// the fold: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
struct RsFoldArgs {
  const Span* tiles;
  const uint64_t* const* bits;  // [n][num_segments]
  const void* const* scales;    // [n][num_segments]: one per block
  const double* const* base;    // [num_segments]
  void* const* outs;            // [num_segments]
  const double* w;              // [n]
  const uint32_t* ids;          // [num_segments]
  double divisor;
  uint32_t* flag;               // the context's NaN words (0 acc, 1 result, 2 input)
  uint32_t k0, k1, draw;
  int32_t num_segments;
  int32_t n;
  int32_t scale_f64;
};

// The clients [0, m) of the staged batch into the wave's accumulators, in table order. kWide: the
// wave's 1024 elements lie in one block, so a client has one scale for all of them.
template <bool kWide>
__device__ __forceinline__ void rs_fold_batch(int m, const uint64_t* words, const double* ss, const double* ws,
                                              double (&acc)[kRsPer]) {
#pragma unroll 2
  for (int i = 0; i < m; ++i) {
    const double w = ws[i];  // LDS broadcasts
    const u64x2* const row = reinterpret_cast<const u64x2*>(words + i * kRsWords);
    double p = kWide ? ss[i * kRsWords] * w : 0.0;
#pragma unroll
    for (int k = 0; k < kRsPer; k += 2) {
      const u64x2 pair = row[k / 2];  // every lane of the wave reads the same 16 bytes
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (!kWide) p = ss[i * kRsWords + k + h] * w;
        // the word as the wave's lane mask, in a scalar register pair
        const uint32_t mlo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(pair[h]));
        const uint32_t mhi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(pair[h] >> 32));
        const bool neg = __builtin_amdgcn_inverse_ballot_w64((static_cast<uint64_t>(mhi) << 32) | mlo);
        acc[k + h] = acc[k + h] + rs_flip(p, neg ? 0x80000000u : 0u);  // (-s) * w is -(s * w) bit for bit
      }
    }
  }
}

template <typename O>
__global__ __launch_bounds__(kRsThreads) void rsign_fold_kernel(RsFoldArgs a) {
  // a batch's words and scales while the clients go through, the exchange buffer after them
  __shared__ __attribute__((aligned(16))) double xs[kRsTile];
  __shared__ double ws[kRsBatch];
  uint64_t* const words = reinterpret_cast<uint64_t*>(xs);  // [kRsBatch][kRsWords]
  double* const ss = xs + kRsBatch * kRsWords;              // [kRsBatch][kRsWords]: the scale of the word's block

  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63, wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg, count = tp->count;
  const int64_t start = tp->start;  // a multiple of kRsTile
  const int n = a.n, T = a.num_segments;
  const int lg = rs_lg_block(start, count);
  const int padded = ((count + (1 << lg) - 1) >> lg) << lg;
  const int nw = padded >> 6;  // words of the tile that exist
  const int64_t word0 = start >> 6, block0 = start >> lg;
  const int e0 = wave * kRsWaveSpan + lane;

  double acc[kRsPer];
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) acc[k] = -0.0;  // -0.0 + p == p bit for bit: the first product starts the sum
  bool nan_in = false;

#pragma unroll 1
  for (int c0 = 0; c0 < n; c0 += kRsBatch) {
    const int m = n - c0 < kRsBatch ? n - c0 : kRsBatch;
    __syncthreads();  // the batch before has been folded
    for (int j = t; j < m * kRsWords; j += kRsThreads) {
      const int i = j / kRsWords, u = j - i * kRsWords;
      uint64_t bits = 0ull;
      double s = 0.0;
      if (u < nw) {  // the word and its block exist
        const int64_t entry = static_cast<int64_t>(c0 + i) * T + seg;
        bits = ((const uint64_t FEDAVG_AS_GLOBAL*)a.bits[entry])[word0 + u];
        const int64_t block = block0 + (u >> (lg - 6));
        s = a.scale_f64 ? ((const double FEDAVG_AS_GLOBAL*)a.scales[entry])[block]
                        : static_cast<double>(((const float FEDAVG_AS_GLOBAL*)a.scales[entry])[block]);
        nan_in |= s != s;
      }
      words[j] = bits;
      ss[j] = s;
    }
    if (t < m) ws[t] = a.w[c0 + t];
    __syncthreads();
    if (lg >= 10) rs_fold_batch<true>(m, words + wave * kRsPer, ss + wave * kRsPer, ws, acc);
    else rs_fold_batch<false>(m, words + wave * kRsPer, ss + wave * kRsPer, ws, acc);
  }

  // m = acc / W, z = H m, out = base + D z
  const uint32_t dm = rs_diagonal(start + wave * kRsWaveSpan, a.ids[seg], a.draw, a.k0, a.k1, lane);
  const double FEDAVG_AS_GLOBAL* pb = (const double FEDAVG_AS_GLOBAL*)a.base[seg] + start;
  double b[kRsPer];
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) b[k] = e0 + 64 * k < count ? pb[e0 + 64 * k] : 0.0;
  bool nan_acc = false, nan_out = false;
  const double divisor = a.divisor;
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) {
    nan_acc |= (e0 + 64 * k < padded) & (acc[k] != acc[k]);
    acc[k] = acc[k] / divisor;
  }
  rs_transform(acc, lg, lane, wave, xs);  // its first barrier: every wave has folded its last batch
  O FEDAVG_AS_GLOBAL* po = (O FEDAVG_AS_GLOBAL*)a.outs[seg] + start;
#pragma unroll
  for (int k = 0; k < kRsPer; ++k) {
    const int e = e0 + 64 * k;
    if (e < count) {
      const double r = b[k] + rs_flip(acc[k], ((dm >> k) & 1u) << 31);
      nan_out |= r != r;
      po[e] = static_cast<O>(r);
    }
  }
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
  if (__ballot(nan_acc) != 0ull && lane == 0) raise_flag(a.flag, 0);
  if (__ballot(nan_out) != 0ull && lane == 0) raise_flag(a.flag, 1);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct RsState {
  Span* d_tiles = nullptr;  // the fold's tiles of the context's layout
  int64_t num_tiles = 0;
  TableRing ring;
  ~RsState() {
    ring.release();
    if (d_tiles) (void)hipFree(d_tiles);
  }
};

int32_t ensure_state(void** slot, RsState** out) {
  if (*slot == nullptr) {
    RsState* st = new RsState();
    const int32_t r = hip_status("rsign state", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<RsState*>(*slot);
  return FEDAVG_OK;
}

size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

}  // namespace

int32_t fedavg_internal_rsign_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "rsign_tile") *out = kRsTile;
  else if (n == "rsign_min_block") *out = kRsMinBlock;
  else if (n == "rsign_threads") *out = kRsThreads;
  else if (n == "rsign_batch") *out = kRsBatch;
  else if (n == "rsign_max_clients") *out = kRsMaxClients;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_rsign_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<RsState*>(state);
}

extern "C" int32_t fedavg_rsign_compress(fedavg_ctx* ctx, int32_t dtype, int32_t mode, uint64_t seed, uint32_t draw,
                                         const uint32_t* tensor_ids, const void* const* delta_ptrs,
                                         const void* const* error_ptrs, const int64_t* numels, int32_t num_tensors,
                                         void* const* bit_ptrs, void* const* scale_ptrs, void* const* residual_ptrs,
                                         void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_RSIGN, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (dtype != FEDAVG_F32 && dtype != FEDAVG_F16 && dtype != FEDAVG_BF16 && dtype != FEDAVG_F64)
    return invalid("the rotated sign step takes fp32, fp16, bf16 or fp64 tensors");
  if (mode != FEDAVG_RSIGN_UNBIASED && mode != FEDAVG_RSIGN_MSE)
    return invalid("the rotated sign step's mode is FEDAVG_RSIGN_UNBIASED or FEDAVG_RSIGN_MSE");
  if (tensor_ids == nullptr || delta_ptrs == nullptr || numels == nullptr || bit_ptrs == nullptr ||
      scale_ptrs == nullptr || residual_ptrs == nullptr)
    return invalid("null id, delta, count, bit, scale or residual table");
  if (num_tensors < 1 || num_tensors > kRsMaxTensors)
    return invalid("the rotated sign step takes between 1 and " + std::to_string(kRsMaxTensors) + " tensors");
  const int T = num_tensors;
  const size_t esize = dtype == FEDAVG_F64 ? 8 : (dtype == FEDAVG_F32 ? 4 : 2);
  const size_t ssize = dtype == FEDAVG_F64 ? 8 : 4;
  uint64_t num_pieces = 0;
  for (int t = 0; t < T; ++t) {
    const std::string who = "tensor " + std::to_string(t);
    if (numels[t] < 1) return invalid(who + ": no elements (an empty tensor has no bits and no scales: the caller's)");
    if (numels[t] > 0x7fffffffll) return invalid(who + ": more than 2^31 - 1 elements");
    if (delta_ptrs[t] == nullptr || residual_ptrs[t] == nullptr || bit_ptrs[t] == nullptr || scale_ptrs[t] == nullptr)
      return invalid(who + ": null delta, residual, bit or scale buffer");
    if (misaligned(delta_ptrs[t], esize) || misaligned(residual_ptrs[t], esize) || misaligned(scale_ptrs[t], ssize) ||
        (error_ptrs != nullptr && misaligned(error_ptrs[t], esize)))
      return invalid(who + ": a buffer is not aligned to its element size");
    if (misaligned(bit_ptrs[t], 8)) return invalid(who + ": the bit buffer is not 8-byte aligned");
    num_pieces += (static_cast<uint64_t>(numels[t]) + kRsTile - 1) / kRsTile;
  }
  if (num_pieces > 0x7fffffffull) return invalid("layout too large for one rotated sign call");

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  RsState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: the tiles, then one RsTensor per tensor
  const size_t piece_bytes = align16(sizeof(Span) * num_pieces);
  const size_t bytes = piece_bytes + align16(sizeof(RsTensor) * static_cast<size_t>(T));
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memset(sl.host, 0, bytes);
  Span* const h_pieces = reinterpret_cast<Span*>(sl.host);
  RsTensor* const h_tensors = reinterpret_cast<RsTensor*>(sl.host + piece_bytes);
  size_t k = 0;
  for (int t = 0; t < T; ++t) {
    RsTensor& g = h_tensors[t];
    g.delta = delta_ptrs[t];
    g.error = error_ptrs != nullptr ? error_ptrs[t] : nullptr;
    g.residual = residual_ptrs[t];
    g.bits = static_cast<uint64_t*>(bit_ptrs[t]);
    g.scales = scale_ptrs[t];
    g.id = tensor_ids[t];
    for (int64_t b = 0; b < numels[t]; b += kRsTile) {
      const int64_t left = numels[t] - b;
      h_pieces[k++] = Span{t, static_cast<int32_t>(left < kRsTile ? left : kRsTile), b};
    }
  }
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  RsEncArgs a;
  a.pieces = reinterpret_cast<const Span*>(sl.dev);
  a.tensors = reinterpret_cast<const RsTensor*>(sl.dev + piece_bytes);
  a.flag = v.d_flag;
  a.k0 = static_cast<uint32_t>(seed);
  a.k1 = static_cast<uint32_t>(seed >> 32);
  a.draw = draw;
  a.mode = mode;
  const dim3 grid(static_cast<unsigned>(num_pieces)), block(kRsThreads);
  if (dtype == FEDAVG_F32) hipLaunchKernelGGL((rsign_encode_kernel<float>), grid, block, 0, s, a);
  else if (dtype == FEDAVG_F16) hipLaunchKernelGGL((rsign_encode_kernel<__half>), grid, block, 0, s, a);
  else if (dtype == FEDAVG_BF16) hipLaunchKernelGGL((rsign_encode_kernel<bf16_t>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((rsign_encode_kernel<double>), grid, block, 0, s, a);
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("rotated sign compress launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_rsign_aggregate_delta(fedavg_ctx* ctx, const void* const* bit_ptrs,
                                                const void* const* scale_ptrs, int32_t scale_dtype, uint64_t seed,
                                                uint32_t draw, const uint32_t* tensor_ids, const double* weights,
                                                int32_t num_clients, double divisor, const double* const* base_ptrs,
                                                void* const* out_ptrs, int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_RSIGN, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (scale_dtype != FEDAVG_F32 && scale_dtype != FEDAVG_F64) return invalid("the rotated sign fold reads fp32 or fp64 scales");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("the rotated sign fold writes fp32 or fp64");
  if (bit_ptrs == nullptr || scale_ptrs == nullptr || tensor_ids == nullptr || weights == nullptr ||
      base_ptrs == nullptr || out_ptrs == nullptr)
    return invalid("null bit table, scale table, ids, weights, base or outputs");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kRsMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the rotated sign fold takes at most " +
                   std::to_string(kRsMaxClients));
  if (!(std::isfinite(divisor) && divisor > 0)) return invalid("the divisor must be finite and > 0");
  for (int32_t i = 0; i < num_clients; ++i)
    if (!std::isfinite(weights[i])) return invalid("weight " + std::to_string(i) + " is not finite");
  const int T = v.num_segments;
  const size_t scale_bytes = scale_dtype == FEDAVG_F64 ? 8 : 4;
  const size_t out_bytes = out_dtype == FEDAVG_F64 ? 8 : 4;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (size_t i = 0; i < entries; ++i) {
    // the message is built only on a refusal: this loop runs n * T times on every call
    const auto where = [T, i] { return "client " + std::to_string(i / T) + ", segment " + std::to_string(i % T); };
    if (bit_ptrs[i] == nullptr || scale_ptrs[i] == nullptr) return invalid(where() + ": null bit or scale buffer");
    if (misaligned(bit_ptrs[i], 8)) return invalid(where() + ": the bit buffer is not 8-byte aligned");
    if (misaligned(scale_ptrs[i], scale_bytes)) return invalid(where() + ": the scales are not aligned to their element size");
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
  RsState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  if (st->d_tiles == nullptr)
    FEDAVG_TRY(span_table(v.seg_numel, v.num_segments, kRsTile, "rotated sign fold", "rotated sign tile table",
                          &st->d_tiles, &st->num_tiles));
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: [n][T] bit pointers, [n][T] scale pointers, [T] base pointers, [T] output
  // pointers, [n] weights, [T] tensor ids
  const size_t ptr_bytes = sizeof(void*) * entries;
  const size_t seg_bytes = sizeof(void*) * static_cast<size_t>(T);
  const size_t w_bytes = sizeof(double) * static_cast<size_t>(num_clients);
  const size_t o_scale = ptr_bytes, o_base = 2 * ptr_bytes, o_out = o_base + seg_bytes, o_w = o_out + seg_bytes;
  const size_t o_ids = o_w + w_bytes;
  const size_t bytes = o_ids + sizeof(uint32_t) * static_cast<size_t>(T);
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, bit_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_scale, scale_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_base, base_ptrs, seg_bytes);
  std::memcpy(sl.host + o_out, out_ptrs, seg_bytes);
  std::memcpy(sl.host + o_w, weights, w_bytes);
  std::memcpy(sl.host + o_ids, tensor_ids, sizeof(uint32_t) * static_cast<size_t>(T));
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  RsFoldArgs a;
  a.tiles = st->d_tiles;
  a.bits = reinterpret_cast<const uint64_t* const*>(sl.dev);
  a.scales = reinterpret_cast<const void* const*>(sl.dev + o_scale);
  a.base = reinterpret_cast<const double* const*>(sl.dev + o_base);
  a.outs = reinterpret_cast<void* const*>(sl.dev + o_out);
  a.w = reinterpret_cast<const double*>(sl.dev + o_w);
  a.ids = reinterpret_cast<const uint32_t*>(sl.dev + o_ids);
  a.divisor = divisor;
  a.flag = v.d_flag;
  a.k0 = static_cast<uint32_t>(seed);
  a.k1 = static_cast<uint32_t>(seed >> 32);
  a.draw = draw;
  a.num_segments = T;
  a.n = num_clients;
  a.scale_f64 = scale_dtype == FEDAVG_F64 ? 1 : 0;
  const dim3 grid(static_cast<unsigned>(st->num_tiles)), block(kRsThreads);
  if (st->num_tiles > 0) {
    if (out_dtype == FEDAVG_F32) hipLaunchKernelGGL((rsign_fold_kernel<float>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((rsign_fold_kernel<double>), grid, block, 0, s, a);
  }
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("rotated sign fold launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}
