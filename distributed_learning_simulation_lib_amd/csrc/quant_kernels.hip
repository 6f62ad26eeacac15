// quant_kernels.hip — gfx950 (MI355X) kernels of the broadcast encoder (fedavg_quant_encode,
// include/fedavg_hip.h): the `send` half of the reference's StochasticQuantServerEndpoint /
// NNADQServerEndpoint (simulation_lib/topology/quantized_endpoint.py:79-96). The aggregated model is
// turned into QSGD or NNADQ records (the layouts of FEDAVG_QSGD_F32 / FEDAVG_NNADQ_F32) where it lies,
// on the device. The contract is DESIGN.md §5p; tests/quant_encode_reference.py restates it in numpy
// on top of oracle/qsgd_oracle.py and oracle/nnadq_oracle.py.
//
// Every arithmetic line is one separately rounded operation in the codec's dtype F (fp32 or fp64):
// no FMA (the library is built with -ffp-contract=off), no reciprocal, IEEE division.
//   QSGD:  norm = max|x|;  q = |x| / norm;  r = q * level;  fl = floor(r);  d = r - fl;
//          slot = fl + (u < d), 0 where norm == 0, clamped to [0, level];  sign bit = !(x < 0)
//   NNADQ: lo = min x, hi = max x;  L = levels(lo, hi, weight) in fp64;  step = (hi - lo) / L;
//          code = clamp(rint((x - lo) / step), 0, L), 0 where step is not positive and finite
// u is the element's uniform of the Philox4x32-10 stream below. No atomics; three launches whatever
// the number of tensors:
//   * The ragged list of tensors is cut, tensor by tensor, into tiles of kQTile elements (a tensor's
//     last tile is shorter), so a tile starts at a multiple of kQTile (and of 128) elements of its
//     tensor: no 16-byte group of slots and no sign byte belongs to two workgroups.
//   * quant_minmax_kernel: one 256-lane workgroup per tile, one element per lane and load
//     (consecutive lanes, consecutive addresses: only the element's own alignment is assumed). It
//     reduces the total-order keys of the values (so -0.0 < +0.0) to the tile's minimum and maximum
//     and raises the context's input flag at a non-finite element.
//   * quant_header_kernel: one workgroup per tensor reduces the tile partials, derives norm or
//     lo / step / L on the device and writes the whole header, its gaps included.
//   * quant_encode_kernel: over the same tiles; a lane owns 16 consecutive elements: one 16-byte
//     store of slots or codes and one 2-byte store of sign bits, both aligned because records are
//     16-byte aligned and tiles start at multiples of 128. The padding of the slot / code area and of
//     the sign area is written as zeros by the lanes whose 16 elements reach past the tensor's end.
//     The inputs are read by 16-byte loads where the lane's 16 elements are complete and so aligned,
//     else element by element.
//
// The record decoder (fedavg_quant_decode) is the way back: the `get` half of the
// reference's QuantClientEndpoint (quantized_endpoint.py:32-39) and the dequantisation of
// QuantServerEndpoint.get (:69-77) for consumers of dense tensors. One launch over the same tiles:
//   QSGD:  a = norm * sign;  b = a * slot;  x = b / level        NNADQ: t = code * step;  x = t + lo
// each line one rounding in F, the formulas of oracle/qsgd_oracle.py:dequantize and
// oracle/nnadq_oracle.py:dequantize and of the fold's in-kernel dequantisation, for every byte pattern.
//   * quant_decode_kernel: a lane owns the same 16 consecutive elements: one 16-byte load of slots or
//     codes and one 2-byte load of sign bits (both aligned, both inside the record's padded areas),
//     the header read by every workgroup for itself (wave-uniform loads). The outputs are aligned to
//     their element only: a complete lane stores single elements up to the first 16-byte boundary,
//     16-byte vectors from there and single elements after the last boundary; an incomplete lane (a
//     tensor's end) stores element by element. An fp32 codec can write the exact fp64 widening of the
//     same values to a second output in the same pass. A header whose level lies outside [1, 255] and
//     a decoded element that is not finite raise the context's input flag.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kQThreads = 256;                  // lanes per workgroup
constexpr int kQPerLane = 16;                   // consecutive elements of one lane in the encode pass
constexpr int kQTile = kQThreads * kQPerLane;   // elements per workgroup
constexpr int kQMaxTensors = 1 << 20;
static_assert(kQTile % 128 == 0, "tile starts are multiples of 128 elements");

struct QArgs {
  const Span* tiles;
  const void* const* in;      // [T]; NULL only where numel == 0
  uint8_t* const* rec;        // [T], 16-byte aligned
  const int64_t* numel;       // [T]
  const uint32_t* ids;        // [T]: the tensor's counter word of the uniform stream
  const int32_t* tile_first;  // [T + 1]: tensor t owns the tiles [tile_first[t], tile_first[t + 1])
  uint64_t* part;             // [2 * tiles]: minimum key, maximum key of every tile
  uint32_t* flag;             // the context's NaN words (0 acc, 1 result, 2 input)
  double weight;
  uint32_t key0, key1, draw;
  int32_t level;
};

template <typename F>
struct QT;
template <>
struct QT<float> {
  using U = uint32_t;
  static constexpr U kSign = 0x80000000u;
  static constexpr U kExp = 0x7f800000u;
  static __device__ __forceinline__ U bits(float x) { return __float_as_uint(x); }
  static __device__ __forceinline__ float value(U b) { return __uint_as_float(b); }
};
template <>
struct QT<double> {
  using U = uint64_t;
  static constexpr U kSign = 0x8000000000000000ull;
  static constexpr U kExp = 0x7ff0000000000000ull;
  static __device__ __forceinline__ U bits(double x) { return static_cast<U>(__double_as_longlong(x)); }
  static __device__ __forceinline__ double value(U b) { return __longlong_as_double(static_cast<long long>(b)); }
};

// The IEEE total order as an unsigned key: -inf < ... < -0.0 < +0.0 < ... < +inf.
template <typename F>
__device__ __forceinline__ uint64_t q_key(typename QT<F>::U b) {
  using U = typename QT<F>::U;
  const U k = (b & QT<F>::kSign) ? static_cast<U>(~b) : static_cast<U>(b | QT<F>::kSign);
  return static_cast<uint64_t>(k);
}
template <typename F>
__device__ __forceinline__ F q_unkey(uint64_t key) {
  using U = typename QT<F>::U;
  const U k = static_cast<U>(key);
  return QT<F>::value((k & QT<F>::kSign) ? static_cast<U>(k ^ QT<F>::kSign) : static_cast<U>(~k));
}

// minimum and maximum over the workgroup; the result is valid in thread 0
__device__ __forceinline__ void q_block_minmax(uint64_t& mn, uint64_t& mx, uint64_t* smn, uint64_t* smx) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long omn = __shfl_xor(static_cast<unsigned long long>(mn), off);
    const unsigned long long omx = __shfl_xor(static_cast<unsigned long long>(mx), off);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
  }
  const int t = static_cast<int>(threadIdx.x);
  if ((t & 63) == 0) {
    smn[t >> 6] = mn;
    smx[t >> 6] = mx;
  }
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int w = 1; w < kQThreads / 64; ++w) {
      mn = smn[w] < mn ? smn[w] : mn;
      mx = smx[w] > mx ? smx[w] : mx;
    }
  }
}

// ---------------------------------------------------------------------------------------
// pass 1: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
template <typename F>
__global__ __launch_bounds__(kQThreads) void quant_minmax_kernel(QArgs a) {
  using U = typename QT<F>::U;
  __shared__ uint64_t smn[kQThreads / 64], smx[kQThreads / 64];
  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg;
  const int32_t count = tp->count;
  const U FEDAVG_AS_GLOBAL* p = (const U FEDAVG_AS_GLOBAL*)a.in[seg] + tp->start;
  uint64_t mn = ~0ull, mx = 0ull;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < kQPerLane; ++k) {
    const int e = k * kQThreads + t;
    if (e < count) {
      const U b = p[e];
      bad |= (b & QT<F>::kExp) == QT<F>::kExp;
      const uint64_t key = q_key<F>(b);
      mn = key < mn ? key : mn;
      mx = key > mx ? key : mx;
    }
  }
  q_block_minmax(mn, mx, smn, smx);
  if (t == 0) {
    a.part[2 * static_cast<int64_t>(blockIdx.x)] = mn;
    a.part[2 * static_cast<int64_t>(blockIdx.x) + 1] = mx;
  }
  if (__ballot(bad) != 0ull && (t & 63) == 0) raise_flag(a.flag, 2);
}

// ---------------------------------------------------------------------------------------
// pass 2: blockIdx.x = tensor
// ---------------------------------------------------------------------------------------
template <typename F, bool NNADQ>
__global__ __launch_bounds__(kQThreads) void quant_header_kernel(QArgs a) {
  __shared__ uint64_t smn[kQThreads / 64], smx[kQThreads / 64];
  const int t = static_cast<int>(threadIdx.x);
  const int seg = static_cast<int>(blockIdx.x);
  const int first = a.tile_first[seg], last = a.tile_first[seg + 1];
  uint64_t mn = ~0ull, mx = 0ull;
  for (int i = first + t; i < last; i += kQThreads) {
    const uint64_t pmn = a.part[2 * static_cast<int64_t>(i)], pmx = a.part[2 * static_cast<int64_t>(i) + 1];
    mn = pmn < mn ? pmn : mn;
    mx = pmx > mx ? pmx : mx;
  }
  q_block_minmax(mn, mx, smn, smx);
  if (t != 0) return;
  const bool empty = first == last;
  const F lo = empty ? static_cast<F>(0) : q_unkey<F>(mn);
  const F hi = empty ? static_cast<F>(0) : q_unkey<F>(mx);
  ulonglong2* const h = reinterpret_cast<ulonglong2*>(a.rec[seg]);
  if (!NNADQ) {
    // max|x| = max(-lo, hi); a zero norm is +0.0 (|x| has no negative zero)
    const F nlo = -lo;
    F norm = nlo > hi ? nlo : hi;
    if (norm == static_cast<F>(0)) norm = static_cast<F>(0);
    ulonglong2 w;
    w.x = static_cast<unsigned long long>(__double_as_longlong(static_cast<double>(norm)));
    w.y = static_cast<unsigned long long>(static_cast<uint32_t>(a.level));  // level, then four zero bytes
    h[0] = w;
  } else {
    const double dlo = static_cast<double>(lo), dhi = static_cast<double>(hi);
    const double alo = __builtin_fabs(dlo), ahi = __builtin_fabs(dhi);
    const double amax = alo > ahi ? alo : ahi;
    int32_t levels = 1;
    if (amax > 0.0 && a.weight > 0.0) {
      const double den = a.weight * amax;
      const double num = dhi - dlo;
      const double r = num / den;
      if (r > 0.0 && r < __builtin_huge_val()) {  // finite and positive (false for NaN)
        const double c = __builtin_ceil(r);
        levels = c >= 255.0 ? 255 : (c <= 1.0 ? 1 : static_cast<int32_t>(c));
      }
    }
    const F span = hi - lo;
    const F step = empty ? static_cast<F>(0) : span / static_cast<F>(levels);
    ulonglong2 w0, w1;
    w0.x = static_cast<unsigned long long>(__double_as_longlong(dlo));
    w0.y = static_cast<unsigned long long>(__double_as_longlong(static_cast<double>(step)));
    w1.x = static_cast<unsigned long long>(static_cast<uint32_t>(levels));  // L, then twelve zero bytes
    w1.y = 0ull;
    h[0] = w0;
    h[1] = w1;
  }
}

// ---------------------------------------------------------------------------------------
// the uniform stream: Philox4x32-10 (q_philox, device_common.h), key = the seed's two halves,
// counter = (block low, block high, tensor id, draw)
// ---------------------------------------------------------------------------------------
// the uniforms of the aligned group of 4 (fp32) or 2 (fp64) elements that starts at element e
template <typename F>
struct QUniform;
template <>
struct QUniform<float> {
  static constexpr int kGroup = 4;
  static __device__ __forceinline__ void draw(const QArgs& a, uint32_t id, int64_t e, float* u) {
    const uint64_t block = static_cast<uint64_t>(e) >> 2;
    const QWords o = q_philox(static_cast<uint32_t>(block), static_cast<uint32_t>(block >> 32), id, a.draw, a.key0,
                              a.key1);
#pragma unroll
    for (int i = 0; i < 4; ++i) u[i] = static_cast<float>(o.w[i] >> 8) * 0x1p-24f;
  }
};
template <>
struct QUniform<double> {
  static constexpr int kGroup = 2;
  static __device__ __forceinline__ void draw(const QArgs& a, uint32_t id, int64_t e, double* u) {
    const uint64_t block = static_cast<uint64_t>(e) >> 1;
    const QWords o = q_philox(static_cast<uint32_t>(block), static_cast<uint32_t>(block >> 32), id, a.draw, a.key0,
                              a.key1);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const uint64_t m = (static_cast<uint64_t>(o.w[2 * i + 1] >> 5) << 26) | static_cast<uint64_t>(o.w[2 * i] >> 6);
      u[i] = static_cast<double>(m) * 0x1p-53;
    }
  }
};

template <typename F>
__device__ __forceinline__ F q_floor(F x);
template <>
__device__ __forceinline__ float q_floor<float>(float x) { return __builtin_floorf(x); }
template <>
__device__ __forceinline__ double q_floor<double>(double x) { return __builtin_floor(x); }
template <typename F>
__device__ __forceinline__ F q_abs(F x);
template <>
__device__ __forceinline__ float q_abs<float>(float x) { return __builtin_fabsf(x); }
template <>
__device__ __forceinline__ double q_abs<double>(double x) { return __builtin_fabs(x); }
template <typename F>
__device__ __forceinline__ F q_rint(F x);
template <>
__device__ __forceinline__ float q_rint<float>(float x) { return __builtin_rintf(x); }
template <>
__device__ __forceinline__ double q_rint<double>(double x) { return __builtin_rint(x); }

// clamp to [0, top] and narrow; a NaN (a refused, non-finite input) gives 0
template <typename F>
__device__ __forceinline__ uint32_t q_byte(F s, F top) {
  const F c = s > static_cast<F>(0) ? (s < top ? s : top) : static_cast<F>(0);
  return static_cast<uint32_t>(static_cast<int32_t>(c));
}

// the lane's 16 elements: element i of the tile-relative chunk [16 * t, 16 * t + 16), +0.0 past `have`
template <typename F>
__device__ __forceinline__ void q_load16(const F* src, int have, F* x);
template <>
__device__ __forceinline__ void q_load16<float>(const float* src, int have, float* x) {
  if (have == kQPerLane && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
    const f32x4 FEDAVG_AS_GLOBAL* p = (const f32x4 FEDAVG_AS_GLOBAL*)src;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const f32x4 v = p[j];
      x[4 * j] = v.x;
      x[4 * j + 1] = v.y;
      x[4 * j + 2] = v.z;
      x[4 * j + 3] = v.w;
    }
  } else {
    const float FEDAVG_AS_GLOBAL* p = (const float FEDAVG_AS_GLOBAL*)src;
#pragma unroll
    for (int i = 0; i < kQPerLane; ++i) x[i] = i < have ? p[i] : 0.0f;
  }
}
template <>
__device__ __forceinline__ void q_load16<double>(const double* src, int have, double* x) {
  if (have == kQPerLane && (reinterpret_cast<uintptr_t>(src) & 15u) == 0) {
    const f64x2 FEDAVG_AS_GLOBAL* p = (const f64x2 FEDAVG_AS_GLOBAL*)src;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const f64x2 v = p[j];
      x[2 * j] = v.x;
      x[2 * j + 1] = v.y;
    }
  } else {
    const double FEDAVG_AS_GLOBAL* p = (const double FEDAVG_AS_GLOBAL*)src;
#pragma unroll
    for (int i = 0; i < kQPerLane; ++i) x[i] = i < have ? p[i] : 0.0;
  }
}

// ---------------------------------------------------------------------------------------
// pass 3: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
template <typename F, bool NNADQ>
__global__ __launch_bounds__(kQThreads) void quant_encode_kernel(QArgs a) {
  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg;
  const int32_t count = tp->count;
  const int64_t start = tp->start;
  const int64_t n = a.numel[seg];
  uint8_t* const rec = a.rec[seg];
  const int64_t e0 = start + static_cast<int64_t>(t) * kQPerLane;  // the lane's first element in the tensor
  const int64_t area = (n + 15) & ~static_cast<int64_t>(15);       // bytes of the slot / code area
  const int left = count - t * kQPerLane;
  const int have = left < 0 ? 0 : (left > kQPerLane ? kQPerLane : left);

  F x[kQPerLane];
  if (have > 0) {
    q_load16<F>(static_cast<const F*>(a.in[seg]) + e0, have, x);
  } else {
#pragma unroll
    for (int i = 0; i < kQPerLane; ++i) x[i] = static_cast<F>(0);
  }

  uint32_t pk[4] = {0u, 0u, 0u, 0u};
  if (!NNADQ) {
    const ulonglong2 h = *reinterpret_cast<const ulonglong2*>(rec);  // written by the header pass
    const F norm = static_cast<F>(__longlong_as_double(static_cast<long long>(h.x)));  // exact: it was widened from F
    const F level = static_cast<F>(a.level);
    const bool live = norm > static_cast<F>(0);
    const uint32_t id = a.ids[seg];
    uint32_t sign = 0u;
    constexpr int G = QUniform<F>::kGroup;
    if (have > 0) {
#pragma unroll
      for (int g = 0; g < kQPerLane / G; ++g) {
        F u[G];
        QUniform<F>::draw(a, id, e0 + g * G, u);
#pragma unroll
        for (int j = 0; j < G; ++j) {
          const int i = g * G + j;
          const F v = x[i];
          const F m = q_abs<F>(v);
          const F q = m / norm;
          const F r = q * level;
          const F fl = q_floor<F>(r);
          const F d = r - fl;
          const F s = fl + (u[j] < d ? static_cast<F>(1) : static_cast<F>(0));
          const uint32_t b = (live && i < have) ? q_byte<F>(s, level) : 0u;
          pk[i >> 2] |= b << (8 * (i & 3));
          // numpy.packbits: element i of a byte's eight is bit 7 - i; byte 1 follows byte 0
          if (i < have && !(v < static_cast<F>(0))) sign |= 1u << ((i & 8) + 7 - (i & 7));
        }
      }
    }
    const int64_t sign_area = (((n + 7) >> 3) + 15) & ~static_cast<int64_t>(15);
    const int64_t sb = e0 >> 3;
    if (sb < sign_area) *(uint16_t FEDAVG_AS_GLOBAL*)(rec + 16 + area + sb) = static_cast<uint16_t>(sign);
    if (e0 < area) *(u32x4 FEDAVG_AS_GLOBAL*)(rec + 16 + e0) = u32x4{pk[0], pk[1], pk[2], pk[3]};
  } else {
    const ulonglong2 h0 = *reinterpret_cast<const ulonglong2*>(rec);
    const ulonglong2 h1 = *reinterpret_cast<const ulonglong2*>(rec + 16);
    const F lo = static_cast<F>(__longlong_as_double(static_cast<long long>(h0.x)));
    const F step = static_cast<F>(__longlong_as_double(static_cast<long long>(h0.y)));
    const F top = static_cast<F>(static_cast<int32_t>(static_cast<uint32_t>(h1.x)));
    const bool live = step > static_cast<F>(0) && step < static_cast<F>(__builtin_huge_val());
#pragma unroll
    for (int i = 0; i < kQPerLane; ++i) {
      const F y = x[i] - lo;
      const F q = y / step;
      const F c = q_rint<F>(q);
      const uint32_t b = (live && i < have) ? q_byte<F>(c, top) : 0u;
      pk[i >> 2] |= b << (8 * (i & 3));
    }
    if (e0 < area) *(u32x4 FEDAVG_AS_GLOBAL*)(rec + 32 + e0) = u32x4{pk[0], pk[1], pk[2], pk[3]};
  }
}

// ---------------------------------------------------------------------------------------
// the decoder: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
struct DArgs {
  const Span* tiles;
  const uint8_t* const* rec;  // [T], 16-byte aligned; NULL only where numel == 0
  void* const* out;           // [T], dtype F, aligned to the element
  void* const* out64;         // [T] fp64 (the WIDE kernels), else unused
  const int64_t* numel;       // [T]
  uint32_t* flag;             // the context's NaN words (0 acc, 1 result, 2 input)
};

template <typename F>
struct QVec;
template <>
struct QVec<float> {
  using T = f32x4;
};
template <>
struct QVec<double> {
  using T = f64x2;
};

// A complete lane's 16 values with H single elements before the first 16-byte boundary of dst:
// 16-byte stores from there, single elements after the last boundary.
template <typename F, int H>
__device__ __forceinline__ void q_store_peeled(F* dst, const F* x) {
  using V = typename QVec<F>::T;
  constexpr int N = 16 / static_cast<int>(sizeof(F));
  F FEDAVG_AS_GLOBAL* p = (F FEDAVG_AS_GLOBAL*)dst;
#pragma unroll
  for (int i = 0; i < H; ++i) p[i] = x[i];
  constexpr int kVecs = (kQPerLane - H) / N;
#pragma unroll
  for (int j = 0; j < kVecs; ++j) {
    V v;
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = x[H + j * N + k];
    *(V FEDAVG_AS_GLOBAL*)(p + H + j * N) = v;
  }
#pragma unroll
  for (int i = H + kVecs * N; i < kQPerLane; ++i) p[i] = x[i];
}

// the lane's values x[0 .. have) to dst[0 .. have); dst is aligned to the element only
template <typename F>
__device__ __forceinline__ void q_store16(F* dst, int have, const F* x) {
  if (have == kQPerLane) {
    // elements before the first 16-byte boundary: 0 .. 3 (fp32), 0 .. 1 (fp64)
    const unsigned h = ((16u - (static_cast<unsigned>(reinterpret_cast<uintptr_t>(dst)) & 15u)) & 15u) /
                       static_cast<unsigned>(sizeof(F));
    if (h == 0u) q_store_peeled<F, 0>(dst, x);
    else if (h == 1u) q_store_peeled<F, 1>(dst, x);
    else if constexpr (sizeof(F) == 4) {
      if (h == 2u) q_store_peeled<F, 2>(dst, x);
      else q_store_peeled<F, 3>(dst, x);
    }
  } else {
    F FEDAVG_AS_GLOBAL* p = (F FEDAVG_AS_GLOBAL*)dst;
#pragma unroll
    for (int i = 0; i < kQPerLane; ++i) {
      if (i < have) p[i] = x[i];
    }
  }
}

template <typename F, bool NNADQ, bool WIDE>
__global__ __launch_bounds__(kQThreads) void quant_decode_kernel(DArgs a) {
  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg;
  const int32_t count = tp->count;
  const int64_t start = tp->start;
  const uint8_t* const rec = a.rec[seg];
  const int64_t e0 = start + static_cast<int64_t>(t) * kQPerLane;  // the lane's first element in the tensor
  const int left = count - t * kQPerLane;
  const int have = left < 0 ? 0 : (left > kQPerLane ? kQPerLane : left);

  F x[kQPerLane];
#pragma unroll
  for (int i = 0; i < kQPerLane; ++i) x[i] = static_cast<F>(0);
  bool bad;
  // e0 < numel where have > 0, and e0 is a multiple of 16: the lane's 16 bytes lie inside the slot /
  // code area (numel rounded up to 16), its 2 sign bytes inside the sign area (likewise)
  if (!NNADQ) {
    const ulonglong2 h = *reinterpret_cast<const ulonglong2*>(rec);
    const F norm = static_cast<F>(__longlong_as_double(static_cast<long long>(h.x)));
    const int32_t ilevel = static_cast<int32_t>(static_cast<uint32_t>(h.y));
    const F level = static_cast<F>(ilevel);
    bad = ilevel < 1 || ilevel > 255;
    if (have > 0) {
      const int64_t n = a.numel[seg];
      const int64_t area = (n + 15) & ~static_cast<int64_t>(15);
      const u32x4 c = *(const u32x4 FEDAVG_AS_GLOBAL*)(rec + 16 + e0);
      const uint32_t sw = *(const uint16_t FEDAVG_AS_GLOBAL*)(rec + 16 + area + (e0 >> 3));
#pragma unroll
      for (int i = 0; i < kQPerLane; ++i) {
        const uint32_t slot = (c[i >> 2] >> (8 * (i & 3))) & 0xffu;
        // numpy.packbits: element i of a byte's eight is bit 7 - i; byte 1 follows byte 0
        const bool plus = ((sw >> ((i & 8) + 7 - (i & 7))) & 1u) != 0u;
        const F sign = plus ? static_cast<F>(1) : static_cast<F>(-1);
        const F ns = norm * sign;
        const F p = ns * static_cast<F>(slot);
        x[i] = p / level;
      }
    }
  } else {
    const ulonglong2 h0 = *reinterpret_cast<const ulonglong2*>(rec);
    const unsigned long long h1 = *reinterpret_cast<const unsigned long long*>(rec + 16);
    const F lo = static_cast<F>(__longlong_as_double(static_cast<long long>(h0.x)));
    const F step = static_cast<F>(__longlong_as_double(static_cast<long long>(h0.y)));
    const int32_t levels = static_cast<int32_t>(static_cast<uint32_t>(h1));
    bad = levels < 1 || levels > 255;
    if (have > 0) {
      const u32x4 c = *(const u32x4 FEDAVG_AS_GLOBAL*)(rec + 32 + e0);
#pragma unroll
      for (int i = 0; i < kQPerLane; ++i) {
        const uint32_t code = (c[i >> 2] >> (8 * (i & 3))) & 0xffu;
        const F p = static_cast<F>(code) * step;
        x[i] = p + lo;
      }
    }
  }
#pragma unroll
  for (int i = 0; i < kQPerLane; ++i) bad |= i < have && (QT<F>::bits(x[i]) & QT<F>::kExp) == QT<F>::kExp;

  if (have > 0) {
    q_store16<F>(static_cast<F*>(a.out[seg]) + e0, have, x);
    if (WIDE) {
      double w[kQPerLane];
#pragma unroll
      for (int i = 0; i < kQPerLane; ++i) w[i] = static_cast<double>(x[i]);  // exact
      q_store16<double>(static_cast<double*>(a.out64[seg]) + e0, have, w);
    }
  }
  if (__ballot(bad) != 0ull && (t & 63) == 0) raise_flag(a.flag, 2);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct QuantState {
  uint64_t* d_part = nullptr;  // the tile partials of the call in flight
  size_t part_cap = 0;         // in tiles
  TableRing ring;
  ~QuantState() {
    ring.release();
    if (d_part) (void)hipFree(d_part);
  }
};

int32_t ensure_state(void** slot, QuantState** out) {
  if (*slot == nullptr) {
    QuantState* st = new QuantState();
    const int32_t r = hip_status("quant state", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<QuantState*>(*slot);
  return FEDAVG_OK;
}

size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

// The tile table: tensor by tensor, tiles of kQTile elements (a tensor's last tile is shorter);
// first[t] (where asked for) is tensor t's first tile, first[T] the number of tiles.
void cut_tiles(const int64_t* numels, int T, Span* tiles, int32_t* first) {
  size_t k = 0;
  for (int t = 0; t < T; ++t) {
    if (first) first[t] = static_cast<int32_t>(k);
    for (int64_t b = 0; b < numels[t]; b += kQTile) {
      const int64_t left = numels[t] - b;
      tiles[k++] = Span{t, static_cast<int32_t>(left < kQTile ? left : kQTile), b};
    }
  }
  if (first) first[T] = static_cast<int32_t>(k);
}

template <typename F>
void launch_all(bool nnadq, unsigned tiles, unsigned tensors, hipStream_t s, const QArgs& a) {
  const dim3 block(kQThreads);
  if (tiles > 0) hipLaunchKernelGGL((quant_minmax_kernel<F>), dim3(tiles), block, 0, s, a);
  if (nnadq) {
    hipLaunchKernelGGL((quant_header_kernel<F, true>), dim3(tensors), block, 0, s, a);
    if (tiles > 0) hipLaunchKernelGGL((quant_encode_kernel<F, true>), dim3(tiles), block, 0, s, a);
  } else {
    hipLaunchKernelGGL((quant_header_kernel<F, false>), dim3(tensors), block, 0, s, a);
    if (tiles > 0) hipLaunchKernelGGL((quant_encode_kernel<F, false>), dim3(tiles), block, 0, s, a);
  }
}

}  // namespace

int32_t fedavg_internal_quant_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "quant_tile") *out = kQTile;
  else if (n == "quant_threads") *out = kQThreads;
  else if (n == "quant_per_lane") *out = kQPerLane;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_quant_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<QuantState*>(state);
}

extern "C" int32_t fedavg_quant_encode(fedavg_ctx* ctx, int32_t codec, const void* const* in_ptrs,
                                       const int64_t* numels, const uint32_t* tensor_ids, int32_t num_tensors,
                                       void* const* record_ptrs, int32_t level, double weight, uint64_t seed,
                                       uint32_t draw, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_QUANT, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (codec != FEDAVG_QSGD_F32 && codec != FEDAVG_QSGD_F64 && codec != FEDAVG_NNADQ_F32 && codec != FEDAVG_NNADQ_F64)
    return invalid("the encoder writes QSGD or NNADQ records of fp32 or fp64 tensors");
  const bool nnadq = codec == FEDAVG_NNADQ_F32 || codec == FEDAVG_NNADQ_F64;
  const bool f64 = codec == FEDAVG_QSGD_F64 || codec == FEDAVG_NNADQ_F64;
  if (in_ptrs == nullptr || numels == nullptr || record_ptrs == nullptr)
    return invalid("null input table, element counts or record table");
  if (num_tensors < 1 || num_tensors > kQMaxTensors)
    return invalid("the encoder takes between 1 and " + std::to_string(kQMaxTensors) + " tensors");
  if (!nnadq && (level < 1 || level > 255)) return invalid("the quantisation level must lie in [1, 255]");
  if (nnadq && !(std::isfinite(weight) && weight > 0)) return invalid("the NNADQ weight must be finite and > 0");
  const int T = num_tensors;
  const uintptr_t elem_mask = f64 ? 7u : 3u;
  uint64_t num_tiles = 0;
  for (int t = 0; t < T; ++t) {
    if (numels[t] < 0) return invalid("tensor " + std::to_string(t) + ": negative element count");
    if (numels[t] > 0 && in_ptrs[t] == nullptr) return invalid("tensor " + std::to_string(t) + ": null input");
    if ((reinterpret_cast<uintptr_t>(in_ptrs[t]) & elem_mask) != 0)
      return invalid("tensor " + std::to_string(t) + ": input not aligned to its element size");
    if (record_ptrs[t] == nullptr) return invalid("tensor " + std::to_string(t) + ": null record");
    if ((reinterpret_cast<uintptr_t>(record_ptrs[t]) & 15u) != 0)
      return invalid("tensor " + std::to_string(t) + ": record not aligned to 16 bytes");
    num_tiles += (static_cast<uint64_t>(numels[t]) + kQTile - 1) / kQTile;
  }
  if (num_tiles > 0x7fffffffull) return invalid("layout too large for one encode call");

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  QuantState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  if (st->part_cap < num_tiles) {  // hipFree waits for the device: no launch still reads the old buffer
    if (st->d_part) FEDAVG_TRY_HIP(hipFree(st->d_part));
    st->d_part = nullptr;
    st->part_cap = 0;
    const size_t cap = num_tiles * 2 < 1024 ? 1024 : num_tiles * 2;
    FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&st->d_part), cap * 2 * sizeof(uint64_t)));
    st->part_cap = cap;
  }

  // the call's tables: the tiles, [T] input pointers, [T] record pointers, [T] element counts,
  // [T] stream ids, [T + 1] first tile of every tensor
  const size_t tile_bytes = align16(sizeof(Span) * num_tiles);
  const size_t ptr_bytes = align16(sizeof(void*) * static_cast<size_t>(T));
  const size_t id_bytes = align16(sizeof(uint32_t) * static_cast<size_t>(T));
  const size_t first_bytes = align16(sizeof(int32_t) * (static_cast<size_t>(T) + 1));
  const size_t o_in = tile_bytes, o_rec = o_in + ptr_bytes, o_numel = o_rec + ptr_bytes, o_id = o_numel + ptr_bytes,
               o_first = o_id + id_bytes;
  const size_t bytes = o_first + first_bytes;
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memset(sl.host, 0, bytes);
  Span* const h_tiles = reinterpret_cast<Span*>(sl.host);
  int32_t* const h_first = reinterpret_cast<int32_t*>(sl.host + o_first);
  uint32_t* const h_ids = reinterpret_cast<uint32_t*>(sl.host + o_id);
  for (int t = 0; t < T; ++t) h_ids[t] = tensor_ids ? tensor_ids[t] : static_cast<uint32_t>(t);
  cut_tiles(numels, T, h_tiles, h_first);
  std::memcpy(sl.host + o_in, in_ptrs, sizeof(void*) * static_cast<size_t>(T));
  std::memcpy(sl.host + o_rec, record_ptrs, sizeof(void*) * static_cast<size_t>(T));
  std::memcpy(sl.host + o_numel, numels, sizeof(int64_t) * static_cast<size_t>(T));
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  QArgs a;
  a.tiles = reinterpret_cast<const Span*>(sl.dev);
  a.in = reinterpret_cast<const void* const*>(sl.dev + o_in);
  a.rec = reinterpret_cast<uint8_t* const*>(sl.dev + o_rec);
  a.numel = reinterpret_cast<const int64_t*>(sl.dev + o_numel);
  a.ids = reinterpret_cast<const uint32_t*>(sl.dev + o_id);
  a.tile_first = reinterpret_cast<const int32_t*>(sl.dev + o_first);
  a.part = st->d_part;
  a.flag = v.d_flag;
  a.weight = weight;
  a.key0 = static_cast<uint32_t>(seed & 0xffffffffull);
  a.key1 = static_cast<uint32_t>(seed >> 32);
  a.draw = draw;
  a.level = nnadq ? 0 : level;
  if (f64) launch_all<double>(nnadq, static_cast<unsigned>(num_tiles), static_cast<unsigned>(T), s, a);
  else launch_all<float>(nnadq, static_cast<unsigned>(num_tiles), static_cast<unsigned>(T), s, a);
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("quant encode launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_quant_decode(fedavg_ctx* ctx, int32_t codec, const void* const* record_ptrs,
                                       const int64_t* numels, int32_t num_tensors, void* const* out_ptrs,
                                       void* const* out64_ptrs, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_QUANT, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (codec != FEDAVG_QSGD_F32 && codec != FEDAVG_QSGD_F64 && codec != FEDAVG_NNADQ_F32 && codec != FEDAVG_NNADQ_F64)
    return invalid("the decoder reads QSGD or NNADQ records of fp32 or fp64 tensors");
  const bool nnadq = codec == FEDAVG_NNADQ_F32 || codec == FEDAVG_NNADQ_F64;
  const bool f64 = codec == FEDAVG_QSGD_F64 || codec == FEDAVG_NNADQ_F64;
  const bool wide = out64_ptrs != nullptr;
  if (record_ptrs == nullptr || numels == nullptr || out_ptrs == nullptr)
    return invalid("null record table, element counts or output table");
  if (wide && f64) return invalid("the fp64 copy is offered for the fp32 codecs: an fp64 codec's output is fp64");
  if (num_tensors < 1 || num_tensors > kQMaxTensors)
    return invalid("the decoder takes between 1 and " + std::to_string(kQMaxTensors) + " tensors");
  const int T = num_tensors;
  const uintptr_t elem = f64 ? 8u : 4u;
  uint64_t num_tiles = 0;
  for (int t = 0; t < T; ++t) {
    if (numels[t] < 0) return invalid("tensor " + std::to_string(t) + ": negative element count");
    if (numels[t] > 0 && record_ptrs[t] == nullptr) return invalid("tensor " + std::to_string(t) + ": null record");
    if (misaligned(record_ptrs[t], 16))
      return invalid("tensor " + std::to_string(t) + ": record not aligned to 16 bytes");
    if (numels[t] > 0 && out_ptrs[t] == nullptr) return invalid("tensor " + std::to_string(t) + ": null output");
    if (misaligned(out_ptrs[t], elem))
      return invalid("tensor " + std::to_string(t) + ": output not aligned to its element size");
    if (wide) {
      if (numels[t] > 0 && out64_ptrs[t] == nullptr)
        return invalid("tensor " + std::to_string(t) + ": null fp64 output");
      if (misaligned(out64_ptrs[t], 8))
        return invalid("tensor " + std::to_string(t) + ": fp64 output not aligned to 8 bytes");
    }
    num_tiles += (static_cast<uint64_t>(numels[t]) + kQTile - 1) / kQTile;
  }
  if (num_tiles > 0x7fffffffull) return invalid("layout too large for one decode call");
  if (num_tiles == 0) return FEDAVG_OK;  // nothing but empty tensors: nothing to write

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  QuantState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: the tiles, [T] record pointers, [T] output pointers, [T] fp64 output pointers
  // (zeros without them), [T] element counts
  const size_t tile_bytes = align16(sizeof(Span) * num_tiles);
  const size_t ptr_bytes = align16(sizeof(void*) * static_cast<size_t>(T));
  const size_t o_rec = tile_bytes, o_out = o_rec + ptr_bytes, o_out64 = o_out + ptr_bytes,
               o_numel = o_out64 + ptr_bytes;
  const size_t bytes = o_numel + ptr_bytes;
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memset(sl.host, 0, bytes);
  cut_tiles(numels, T, reinterpret_cast<Span*>(sl.host), nullptr);
  std::memcpy(sl.host + o_rec, record_ptrs, sizeof(void*) * static_cast<size_t>(T));
  std::memcpy(sl.host + o_out, out_ptrs, sizeof(void*) * static_cast<size_t>(T));
  if (wide) std::memcpy(sl.host + o_out64, out64_ptrs, sizeof(void*) * static_cast<size_t>(T));
  std::memcpy(sl.host + o_numel, numels, sizeof(int64_t) * static_cast<size_t>(T));
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  DArgs a;
  a.tiles = reinterpret_cast<const Span*>(sl.dev);
  a.rec = reinterpret_cast<const uint8_t* const*>(sl.dev + o_rec);
  a.out = reinterpret_cast<void* const*>(sl.dev + o_out);
  a.out64 = reinterpret_cast<void* const*>(sl.dev + o_out64);
  a.numel = reinterpret_cast<const int64_t*>(sl.dev + o_numel);
  a.flag = v.d_flag;
  const dim3 grid(static_cast<unsigned>(num_tiles)), block(kQThreads);
  if (f64) {
    if (nnadq) hipLaunchKernelGGL((quant_decode_kernel<double, true, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((quant_decode_kernel<double, false, false>), grid, block, 0, s, a);
  } else if (wide) {
    if (nnadq) hipLaunchKernelGGL((quant_decode_kernel<float, true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((quant_decode_kernel<float, false, true>), grid, block, 0, s, a);
  } else {
    if (nnadq) hipLaunchKernelGGL((quant_decode_kernel<float, true, false>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((quant_decode_kernel<float, false, false>), grid, block, 0, s, a);
  }
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("quant decode launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}
