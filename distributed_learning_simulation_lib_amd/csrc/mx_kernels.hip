// mx_kernels.hip — gfx950 (MI355X) kernels of OCP Microscaling (MX) client updates: the client step
// fedavg_mx_compress and the server fold fedavg_mx_aggregate_delta (include/fedavg_hip.h). The
// contract is DESIGN.md §5ab; the oracle of the client step is mx._mx_compress_torch, the oracle of the
// fold is fedavg_aggregate_delta on the densified deltas.
//
// An MX delta of a tensor is one code per element (FP8 E4M3, one byte, or FP4 E2M1, one nibble, the
// even element in the low one) and one E8M0 scale byte per block of 32 consecutive elements: element
// e is code_value[e] * 2^(scales[e / 32] - 127).
//
// The client step, one launch whatever the number of tensors: a 256-lane workgroup owns a piece of
// kMxTile elements of one tensor and walks it 1024 elements at a time. A lane owns 4 consecutive
// elements (one 16-byte load of fp32, 8 bytes of fp16 / bf16, two 16-byte loads of fp64; element by
// element where the tensor's storage is not that well aligned or the tensor ends), so a block is 8
// adjacent lanes of one wave and its amax is three cross-lane maxima: no LDS, no barrier, no second
// pass. All arithmetic is fp64, where every step of the contract but the two roundings into the dtype
// is exact: total = RNE(delta + error), q = total * 2^-E by an assembled power of two, the code by
// one v_rndne_f64 of q scaled so that the element format's quantum is 1 (normal and subnormal codes
// then come out of the same integer expression), sent = m * 2^(e - mant + E), residual = RNE(total -
// sent). The lane stores its 4 codes as one 32-bit (FP8) or 16-bit (FP4) word, the block's first
// lane its scale byte, and the lane that read an element writes its residual, so the residual may be
// the error or the delta itself. The hardware's v_cvt_scalef32_pk_fp8_* / _fp4_* are not used by the
// encoder: DESIGN.md §5ab says why.
//
// The fold, one launch for the layout: a workgroup owns a tile of kMxTile elements = 128 blocks. A
// lane owns kLane consecutive elements, 16 for FP8 and 32 for FP4, that is 16 bytes of a client's
// codes: one non-temporal 16-byte load per lane and client, a wave's loads one contiguous KiB, the
// next client's load in flight while this one's is decoded. Base values and accumulators stay in fp64
// registers across the clients. The clients go through in batches of kMxBatch: the batch's scale
// bytes of the tile (128 per client, read four to a load where the client's buffer allows it) and its
// weights are staged in LDS in one coalesced pass between two barriers; a lane then reads its block's
// byte back (two FP8 lanes share one) and assembles 2^(s - 127) as an fp64 from integer operations.
// Codes are decoded two to an instruction by v_cvt_scalef32_pk_f32_fp8 / _fp4 at scale 1.0, which is
// exact in fp32, widened to fp64 and multiplied by the power of two: the product is exact and always a
// normal fp64 (or a zero that keeps its sign). Then per client and element the three rounded
// operations x = b + d, p = x * w, acc = acc + p; acc starts at -0.0, the identity of the IEEE add.
// A full tile looks for NaN inputs without a compare per element: the base once, the scale byte 255
// once per client and lane, an E4M3 NaN code by one carry trick per four codes. Only the tile that
// holds a tensor's end runs the guarded variant, which compares every x of an element that exists.
// No atomics.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "call_tables.h"
#include "device_common.h"

namespace {

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------
// geometry and formats
// ---------------------------------------------------------------------------------------
constexpr int kMxBlock = 32;                      // elements that share a scale byte
constexpr int kMxThreads = 256;                   // lanes of an encoder workgroup and of an FP8 fold workgroup
constexpr int kMxTile = 4096;                     // elements per workgroup, both kernels
constexpr int kMxTileBlocks = kMxTile / kMxBlock; // scale bytes of a tile
constexpr int kMxQuad = 4;                        // consecutive elements of an encoder lane
constexpr int kMxStep = kMxThreads * kMxQuad;     // elements an encoder workgroup takes at a time
// the batch is -D overridable for tuning builds (build.py `defines`)
#ifndef FEDAVG_MX_BATCH
#define FEDAVG_MX_BATCH 32
#endif
constexpr int kMxBatch = FEDAVG_MX_BATCH;         // clients whose scale bytes are staged between two pairs of barriers
constexpr int kMxMaxClients = FEDAVG_POINT_MAX_CLIENTS;
constexpr int kMxMaxTensors = 1 << 20;
static_assert(kMxTile % kMxStep == 0 && kMxTileBlocks % 4 == 0, "whole steps, whole 4-byte units of scale bytes");
static_assert(kMxBatch >= 1 && kMxBatch <= 128, "one lane of the narrowest fold workgroup stages one client's weight");
static_assert(kMxBlock % kMxQuad == 0 && (kMxBlock / kMxQuad) == 8, "a block is 8 adjacent lanes of a wave");

template <int F>
struct Mx;
template <>
struct Mx<FEDAVG_MXFP8> {  // E4M3 "FN": bias 7, subnormals, 448 the largest, S.1111.111 NaN
  static constexpr int kMant = 3, kEmin = -6, kEmax = 8, kSign = 7, kLane = 16;
  static constexpr double kMax = 448.0;
};
template <>
struct Mx<FEDAVG_MXFP4> {  // E2M1: bias 1, +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}
  static constexpr int kMant = 1, kEmin = 0, kEmax = 2, kSign = 3, kLane = 32;
  static constexpr double kMax = 6.0;
};

// 2^k as an fp64, -1022 <= k <= 1023, from integer operations
__device__ __forceinline__ double mx_pow2(int k) {
  return __longlong_as_double(static_cast<long long>(static_cast<uint64_t>(1023 + k) << 52));
}

__device__ __forceinline__ uint32_t mx_high(double v) {
  return static_cast<uint32_t>(static_cast<uint64_t>(__double_as_longlong(v)) >> 32);
}

// ---------------------------------------------------------------------------------------
// the encoder's element access: 4 consecutive elements of T as fp64 values and back
// ---------------------------------------------------------------------------------------
template <typename T>
struct QuadIO {
  static constexpr int kImgs = sizeof(T) == 8 ? 2 : 1;  // 16-byte images of the 4 elements
  static constexpr int kPer = kMxQuad / kImgs;          // elements of an image
  static constexpr uintptr_t kAlign = sizeof(T) == 2 ? 8 : 16;

  // elements [e, e + have) of `base`; the rest +0.0
  __device__ __forceinline__ static void load(const void* base, int64_t e, int have, double (&v)[kMxQuad]) {
    const char* const p = static_cast<const char*>(base) + e * static_cast<int64_t>(sizeof(T));
    const bool vec = have == kMxQuad && (reinterpret_cast<uintptr_t>(p) & (kAlign - 1)) == 0;
#pragma unroll
    for (int g = 0; g < kImgs; ++g) {
      u32x4 raw = {0u, 0u, 0u, 0u};
      if (vec) {
        if constexpr (sizeof(T) == 2) {
          const u32x2 h = *(const u32x2 FEDAVG_AS_GLOBAL*)p;
          raw[0] = h[0];
          raw[1] = h[1];
        } else {
          raw = *(const u32x4 FEDAVG_AS_GLOBAL*)(p + 16 * g);
        }
      } else {
        const int left = have - g * kPer;
        raw = load_guarded<T>(base, e + g * kPer, left < kPer ? left : kPer);
      }
#pragma unroll
      for (int i = 0; i < kPer; ++i) v[g * kPer + i] = Format<T>::value(raw, i);
    }
  }

  // RNE(v[i]) into T at elements [e, e + have); returns nothing, writes nothing else
  __device__ __forceinline__ static void store(void* base, int64_t e, int have, const double (&v)[kMxQuad]) {
    char* const p = static_cast<char*>(base) + e * static_cast<int64_t>(sizeof(T));
    const bool vec = have == kMxQuad && (reinterpret_cast<uintptr_t>(p) & (kAlign - 1)) == 0;
#pragma unroll
    for (int g = 0; g < kImgs; ++g) {
      u32x4 raw = {0u, 0u, 0u, 0u};
#pragma unroll
      for (int i = 0; i < kPer; ++i) dp_put<T>(raw, i, v[g * kPer + i]);
      if (vec) {
        if constexpr (sizeof(T) == 2) {
          const u32x2 h = {raw[0], raw[1]};
          *(u32x2 FEDAVG_AS_GLOBAL*)p = h;
        } else {
          *(u32x4 FEDAVG_AS_GLOBAL*)(p + 16 * g) = raw;
        }
      } else {
        const int left = have - g * kPer;
        store_guarded<T>(base, e + g * kPer, left < kPer ? left : kPer, raw);
      }
    }
  }
};

// v rounded once into T, as an fp64
template <typename T>
__device__ __forceinline__ double mx_round(double v) {
  if constexpr (sizeof(T) == 8) return v;
  u32x4 raw = {0u, 0u, 0u, 0u};
  dp_put<T>(raw, 0, v);
  return Format<T>::value(raw, 0);
}

struct MxTensor {
  const void* delta;
  const void* error;  // NULL: no residual yet
  void* residual;
  uint8_t* codes;     // 32 * ceil(numel / 32) bytes (FP8) or half of that (FP4), 16-byte aligned
  uint8_t* scales;    // ceil(numel / 32) bytes
  int64_t numel;
};

struct MxEncArgs {
  const Span* pieces;       // the pieces of every tensor, in list order
  const MxTensor* tensors;  // [T]
  uint32_t* flag;           // the context's NaN words (0 acc, 1 result, 2 input)
};

// ---------------------------------------------------------------------------------------
// the client step; blockIdx.x = piece
// ---------------------------------------------------------------------------------------
template <typename T, int F>
__global__ __launch_bounds__(kMxThreads) void mx_encode_kernel(MxEncArgs a) {
  using M = Mx<F>;
  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* pp = (const Span FEDAVG_AS_CONST*)(a.pieces + blockIdx.x);
  const int32_t count = pp->count;
  const int64_t start = pp->start;  // a multiple of kMxTile
  const MxTensor FEDAVG_AS_CONST* tp = (const MxTensor FEDAVG_AS_CONST*)(a.tensors + pp->seg);
  const void* const delta = tp->delta;
  const void* const error = tp->error;
  void* const residual = tp->residual;
  uint8_t* const codes = tp->codes;
  uint8_t* const scales = tp->scales;
  const bool has_error = error != nullptr;
  const int padded = (count + kMxBlock - 1) & ~(kMxBlock - 1);  // the piece's last block is whole in the payload
  bool bad = false;
#pragma unroll 1
  for (int e0 = t * kMxQuad; e0 - t * kMxQuad < count; e0 += kMxStep) {  // the same trips for every lane
    const int left = count - e0;
    const int have = left < 0 ? 0 : (left < kMxQuad ? left : kMxQuad);
    double tot[kMxQuad];
    QuadIO<T>::load(delta, start + e0, have, tot);
    if (has_error) {
      double err[kMxQuad];
      QuadIO<T>::load(error, start + e0, have, err);
#pragma unroll
      for (int i = 0; i < kMxQuad; ++i) tot[i] = mx_round<T>(tot[i] + err[i]);
    }
    // the block's amax: the lane's four, then the 8 lanes of the block
    double amax = 0.0;
#pragma unroll
    for (int i = 0; i < kMxQuad; ++i) {
      const double x = __builtin_fabs(tot[i]);
      bad |= !(x < __builtin_huge_val());
      amax = x > amax ? x : amax;
    }
#pragma unroll
    for (int off = 1; off < kMxBlock / kMxQuad; off <<= 1) {
      const double o = __shfl_xor(amax, off);
      amax = o > amax ? o : amax;
    }
    // E = floor(log2 amax) - emax in [-127, 127]; a zero or fp64-subnormal amax has field 0 and clamps
    int E = static_cast<int>((mx_high(amax) >> 20) & 0x7ffu) - 1023 - M::kEmax;
    E = E < -127 ? -127 : (E > 127 ? 127 : E);
    const double down = mx_pow2(-E), up = mx_pow2(E);
    uint32_t word = 0u;
    double res[kMxQuad];
#pragma unroll
    for (int i = 0; i < kMxQuad; ++i) {
      const double q = __builtin_fabs(tot[i]) * down;  // exact (or an overflow that saturates)
      const double c = q < M::kMax ? q : M::kMax;
      int e = static_cast<int>(mx_high(c) >> 20) - 1023;
      e = e < M::kEmin ? M::kEmin : e;
      const double r = __builtin_rint(c * mx_pow2(M::kMant - e));  // ties to even; 2^(mant+1) carries into e + 1
      const uint32_t code = (static_cast<uint32_t>(e - M::kEmin) << M::kMant) + static_cast<uint32_t>(static_cast<int>(r));
      const uint32_t neg = mx_high(tot[i]) >> 31;
      constexpr int kBits = M::kSign + 1;
      word |= (code | (neg << M::kSign)) << (kBits * i);
      const double mag = (r * mx_pow2(e - M::kMant)) * up;  // exact
      const double sent = mx_round<T>(neg ? -mag : mag);
      res[i] = tot[i] - sent;
    }
    if (e0 < padded) {
      if constexpr (F == FEDAVG_MXFP8) *(uint32_t FEDAVG_AS_GLOBAL*)(codes + start + e0) = word;
      else *(uint16_t FEDAVG_AS_GLOBAL*)(codes + ((start + e0) >> 1)) = static_cast<uint16_t>(word);
      if ((t & (kMxBlock / kMxQuad - 1)) == 0)
        *(uint8_t FEDAVG_AS_GLOBAL*)(scales + ((start + e0) >> 5)) = static_cast<uint8_t>(E + 127);
    }
    if (have > 0) QuadIO<T>::store(residual, start + e0, have, res);
  }
  if (__ballot(bad) != 0ull && (t & 63) == 0) raise_flag(a.flag, 2);
}

// ---------------------------------------------------------------------------------------
// the fold: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
struct MxFoldArgs {
  const Span* tiles;
  const uint8_t* const* codes;   // [n][num_segments]
  const uint8_t* const* scales;  // [n][num_segments]
  const double* const* base;     // [num_segments]
  void* const* outs;             // [num_segments]
  const double* w;               // [n]
  double divisor;
  uint32_t* flag;                // the context's NaN words (0 acc, 1 result, 2 input)
  int32_t num_segments;
  int32_t n;
};

// the two code values of the low (kHigh = false) or high half of `v` (FP8), or of byte `kSel` (FP4)
template <int F, int kSel>
__device__ __forceinline__ f32x2 mx_pair(uint32_t v) {
  if constexpr (F == FEDAVG_MXFP8) return __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(v, 1.0f, kSel != 0);
  else return __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v, 1.0f, kSel);
}

// One client into the lane's accumulators. kGuard: the tile holds its tensor's end, so only the
// lane's first `mine` elements exist and every x of those is compared.
template <int F, bool kGuard>
__device__ __forceinline__ void mx_fold_client(const u32x4& cur, uint32_t s, double w, int mine,
                                               const double (&b)[Mx<F>::kLane], double (&acc)[Mx<F>::kLane],
                                               bool& nan_in) {
  constexpr int L = Mx<F>::kLane;
  constexpr int kPerWord = L / 4;   // elements of a 32-bit word of codes
  constexpr int kPairs = kPerWord / 2;
  // 2^(s - 127): the exponent field s + 896 is never 0 or 2047, so the value is a normal fp64; 255 is NaN
  const uint64_t sbits = s == 255u ? 0x7ff8000000000000ull : static_cast<uint64_t>(s + 896u) << 52;
  const double scale = __longlong_as_double(static_cast<long long>(sbits));
  if (!kGuard) {
    nan_in |= s == 255u;
    if constexpr (F == FEDAVG_MXFP8) {
#pragma unroll
      for (int j = 0; j < 4; ++j)  // a byte whose low 7 bits are all set carries into its bit 7
        nan_in |= (((cur[j] & 0x7f7f7f7fu) + 0x01010101u) & 0x80808080u) != 0u;
    }
  }
  auto one = [&](int k, float f) {
    const double d = static_cast<double>(f) * scale;  // exact
    const double x = b[k] + d;
    if (kGuard) nan_in |= (k < mine) & (x != x);
    const double p = x * w;
    acc[k] = acc[k] + p;
  };
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const uint32_t v = cur[j];
    f32x2 f[kPairs];
    f[0] = mx_pair<F, 0>(v);
    f[1] = mx_pair<F, 1>(v);
    if constexpr (kPairs == 4) {
      f[2] = mx_pair<F, 2>(v);
      f[3] = mx_pair<F, 3>(v);
    }
#pragma unroll
    for (int h = 0; h < kPairs; ++h) {
      one(j * kPerWord + 2 * h, f[h][0]);
      one(j * kPerWord + 2 * h + 1, f[h][1]);
    }
  }
}

// The clients [c0, c0 + m) of the staged batch, in table order; `lp` is the lane's byte offset into a
// client's codes of the segment, `live` whether the lane's block exists.
template <int F, bool kGuard>
__device__ __forceinline__ void mx_fold_batch(const MxFoldArgs& a, int c0, int m, int32_t seg, int64_t lp, bool live,
                                              const uint8_t* sc, const double* ws, int mine,
                                              const double (&b)[Mx<F>::kLane], double (&acc)[Mx<F>::kLane],
                                              bool& nan_in) {
  const int T = a.num_segments;
  const u32x4 zero = {0u, 0u, 0u, 0u};
  auto fetch = [&](int i) -> u32x4 {
    const uint8_t* const p = a.codes[static_cast<int64_t>(c0 + i) * T + seg] + lp;
    return live ? __builtin_nontemporal_load((const u32x4 FEDAVG_AS_GLOBAL*)p) : zero;
  };
  u32x4 nxt = fetch(0);
#pragma unroll 2
  for (int i = 0; i < m; ++i) {
    const u32x4 cur = nxt;
    if (i + 1 < m) nxt = fetch(i + 1);  // in flight while `cur` is decoded
    mx_fold_client<F, kGuard>(cur, sc[i * kMxTileBlocks], ws[i], mine, b, acc, nan_in);
  }
}

template <int F, typename O>
__global__ __launch_bounds__(kMxTile / Mx<F>::kLane) void mx_fold_kernel(MxFoldArgs a) {
  constexpr int L = Mx<F>::kLane;
  constexpr int kThreads = kMxTile / L;
  constexpr int kUnits = kMxTileBlocks / 4;  // 4-byte units of a client's scale bytes of the tile
  __shared__ __attribute__((aligned(4))) uint8_t sc[kMxBatch * kMxTileBlocks];
  __shared__ double ws[kMxBatch];

  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg, count = tp->count;
  const int64_t start = tp->start;  // a multiple of kMxTile
  const int n = a.n, T = a.num_segments;
  const int nb = (count + kMxBlock - 1) / kMxBlock;  // blocks of the tile that exist
  const int64_t block0 = start / kMxBlock;
  const bool full = count == kMxTile;

  // the lane's elements: [t * L, t * L + L); past the segment's end neither read nor written
  const int e0 = t * L;
  const int mine = count - e0 < 0 ? 0 : (count - e0 < L ? count - e0 : L);
  const bool live = e0 < nb * kMxBlock;  // the lane's 16 bytes of codes are inside every client's payload
  const int64_t lp = (start + e0) * 16 / L;  // FP8: one byte per element; FP4: two elements per byte
  double b[L], acc[L];
  const double FEDAVG_AS_GLOBAL* pb = (const double FEDAVG_AS_GLOBAL*)a.base[seg] + start + e0;
  bool nan_in = false;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    b[k] = k < mine ? pb[k] : 0.0;
    nan_in |= b[k] != b[k];  // n >= 1: x_0 = b + d_0 is NaN
    acc[k] = -0.0;           // -0.0 + p == p bit for bit: the first product starts the sum
  }

#pragma unroll 1
  for (int c0 = 0; c0 < n; c0 += kMxBatch) {
    const int m = n - c0 < kMxBatch ? n - c0 : kMxBatch;
    __syncthreads();  // the batch before has been folded
    for (int j = t; j < m * kUnits; j += kThreads) {
      const int i = j / kUnits, u = j - i * kUnits;
      const uint8_t* const p = a.scales[static_cast<int64_t>(c0 + i) * T + seg] + block0 + 4 * u;
      uint32_t v = 0u;
      if (4 * u + 3 < nb && (reinterpret_cast<uintptr_t>(p) & 3u) == 0) {
        v = *(const uint32_t FEDAVG_AS_GLOBAL*)p;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (4 * u + q < nb) v |= static_cast<uint32_t>(((const uint8_t FEDAVG_AS_GLOBAL*)p)[q]) << (8 * q);
        }
      }
      *reinterpret_cast<uint32_t*>(sc + i * kMxTileBlocks + 4 * u) = v;
    }
    if (t < m) ws[t] = a.w[c0 + t];
    __syncthreads();
    const uint8_t* const my_scale = sc + e0 / kMxBlock;
    if (full) mx_fold_batch<F, false>(a, c0, m, seg, lp, live, my_scale, ws, mine, b, acc, nan_in);
    else mx_fold_batch<F, true>(a, c0, m, seg, lp, live, my_scale, ws, mine, b, acc, nan_in);
  }

  // out = acc / W
  bool nan_acc = false, nan_out = false;
  O FEDAVG_AS_GLOBAL* po = (O FEDAVG_AS_GLOBAL*)a.outs[seg] + start + e0;
  const double divisor = a.divisor;
#pragma unroll
  for (int k = 0; k < L; ++k) {
    if (k < mine) {
      const double s = acc[k];
      nan_acc |= s != s;
      const double r = s / divisor;
      nan_out |= r != r;
      po[k] = static_cast<O>(r);
    }
  }
  const int lane = t & 63;
  if (__ballot(nan_in && mine > 0) != 0ull && lane == 0) raise_flag(a.flag, 2);
  if (__ballot(nan_acc) != 0ull && lane == 0) raise_flag(a.flag, 0);
  if (__ballot(nan_out) != 0ull && lane == 0) raise_flag(a.flag, 1);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct MxState {
  Span* d_tiles = nullptr;  // the fold's tiles of the context's layout
  int64_t num_tiles = 0;
  TableRing ring;
  ~MxState() {
    ring.release();
    if (d_tiles) (void)hipFree(d_tiles);
  }
};

int32_t ensure_state(void** slot, MxState** out) {
  if (*slot == nullptr) {
    MxState* st = new MxState();
    const int32_t r = hip_status("mx state", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<MxState*>(*slot);
  return FEDAVG_OK;
}

size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

bool mx_format(int32_t format) { return format == FEDAVG_MXFP8 || format == FEDAVG_MXFP4; }

template <typename T>
void launch_encode(int32_t format, unsigned pieces, hipStream_t s, const MxEncArgs& a) {
  const dim3 grid(pieces), block(kMxThreads);
  if (format == FEDAVG_MXFP8) hipLaunchKernelGGL((mx_encode_kernel<T, FEDAVG_MXFP8>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((mx_encode_kernel<T, FEDAVG_MXFP4>), grid, block, 0, s, a);
}

template <int F>
void launch_fold(int32_t out_dtype, unsigned tiles, hipStream_t s, const MxFoldArgs& a) {
  const dim3 grid(tiles), block(kMxTile / Mx<F>::kLane);
  if (out_dtype == FEDAVG_F32) hipLaunchKernelGGL((mx_fold_kernel<F, float>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((mx_fold_kernel<F, double>), grid, block, 0, s, a);
}

}  // namespace

int32_t fedavg_internal_mx_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "mx_block") *out = kMxBlock;
  else if (n == "mx_tile") *out = kMxTile;
  else if (n == "mx_threads") *out = kMxThreads;
  else if (n == "mx_batch") *out = kMxBatch;
  else if (n == "mx_max_clients") *out = kMxMaxClients;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_mx_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<MxState*>(state);
}

extern "C" int32_t fedavg_mx_compress(fedavg_ctx* ctx, int32_t dtype, int32_t format, const void* const* delta_ptrs,
                                      const void* const* error_ptrs, const int64_t* numels, int32_t num_tensors,
                                      void* const* code_ptrs, void* const* scale_ptrs, void* const* residual_ptrs,
                                      void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_MX, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (dtype != FEDAVG_F32 && dtype != FEDAVG_F16 && dtype != FEDAVG_BF16 && dtype != FEDAVG_F64)
    return invalid("the mx step takes fp32, fp16, bf16 or fp64 tensors");
  if (!mx_format(format)) return invalid("the mx step writes FEDAVG_MXFP8 or FEDAVG_MXFP4");
  if (delta_ptrs == nullptr || numels == nullptr || code_ptrs == nullptr || scale_ptrs == nullptr ||
      residual_ptrs == nullptr)
    return invalid("null delta, count, code, scale or residual table");
  if (num_tensors < 1 || num_tensors > kMxMaxTensors)
    return invalid("the mx step takes between 1 and " + std::to_string(kMxMaxTensors) + " tensors");
  const int T = num_tensors;
  const size_t esize = dtype == FEDAVG_F64 ? 8 : (dtype == FEDAVG_F32 ? 4 : 2);
  uint64_t num_pieces = 0;
  for (int t = 0; t < T; ++t) {
    const std::string who = "tensor " + std::to_string(t);
    if (numels[t] < 1) return invalid(who + ": no elements (an empty tensor has no codes and no scales: the caller's)");
    if (numels[t] > 0x7fffffffll) return invalid(who + ": more than 2^31 - 1 elements");
    if (delta_ptrs[t] == nullptr || residual_ptrs[t] == nullptr || code_ptrs[t] == nullptr || scale_ptrs[t] == nullptr)
      return invalid(who + ": null delta, residual, code or scale buffer");
    if (misaligned(delta_ptrs[t], esize) || misaligned(residual_ptrs[t], esize) ||
        (error_ptrs != nullptr && misaligned(error_ptrs[t], esize)))
      return invalid(who + ": a buffer is not aligned to its element size");
    if (misaligned(code_ptrs[t], 16)) return invalid(who + ": the code buffer is not 16-byte aligned");
    num_pieces += (static_cast<uint64_t>(numels[t]) + kMxTile - 1) / kMxTile;
  }
  if (num_pieces > 0x7fffffffull) return invalid("layout too large for one mx call");

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  MxState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: the pieces, then one MxTensor per tensor
  const size_t piece_bytes = align16(sizeof(Span) * num_pieces);
  const size_t bytes = piece_bytes + align16(sizeof(MxTensor) * static_cast<size_t>(T));
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memset(sl.host, 0, bytes);
  Span* const h_pieces = reinterpret_cast<Span*>(sl.host);
  MxTensor* const h_tensors = reinterpret_cast<MxTensor*>(sl.host + piece_bytes);
  size_t k = 0;
  for (int t = 0; t < T; ++t) {
    MxTensor& g = h_tensors[t];
    g.delta = delta_ptrs[t];
    g.error = error_ptrs != nullptr ? error_ptrs[t] : nullptr;
    g.residual = residual_ptrs[t];
    g.codes = static_cast<uint8_t*>(code_ptrs[t]);
    g.scales = static_cast<uint8_t*>(scale_ptrs[t]);
    g.numel = numels[t];
    for (int64_t b = 0; b < numels[t]; b += kMxTile) {
      const int64_t left = numels[t] - b;
      h_pieces[k++] = Span{t, static_cast<int32_t>(left < kMxTile ? left : kMxTile), b};
    }
  }
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  MxEncArgs a;
  a.pieces = reinterpret_cast<const Span*>(sl.dev);
  a.tensors = reinterpret_cast<const MxTensor*>(sl.dev + piece_bytes);
  a.flag = v.d_flag;
  const unsigned g1 = static_cast<unsigned>(num_pieces);
  if (dtype == FEDAVG_F32) launch_encode<float>(format, g1, s, a);
  else if (dtype == FEDAVG_F16) launch_encode<__half>(format, g1, s, a);
  else if (dtype == FEDAVG_BF16) launch_encode<bf16_t>(format, g1, s, a);
  else launch_encode<double>(format, g1, s, a);
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("mx compress launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_mx_aggregate_delta(fedavg_ctx* ctx, const void* const* code_ptrs,
                                             const void* const* scale_ptrs, int32_t format, const double* weights,
                                             int32_t num_clients, double divisor, const double* const* base_ptrs,
                                             void* const* out_ptrs, int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_MX, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (!mx_format(format)) return invalid("the mx fold reads FEDAVG_MXFP8 or FEDAVG_MXFP4");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("the mx fold writes fp32 or fp64");
  if (code_ptrs == nullptr || scale_ptrs == nullptr || weights == nullptr || base_ptrs == nullptr || out_ptrs == nullptr)
    return invalid("null code table, scale table, weights, base or outputs");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kMxMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the mx fold takes at most " + std::to_string(kMxMaxClients));
  if (!(std::isfinite(divisor) && divisor > 0)) return invalid("the divisor must be finite and > 0");
  for (int32_t i = 0; i < num_clients; ++i)
    if (!std::isfinite(weights[i])) return invalid("weight " + std::to_string(i) + " is not finite");
  const int T = v.num_segments;
  const size_t out_bytes = out_dtype == FEDAVG_F64 ? 8 : 4;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (size_t i = 0; i < entries; ++i) {
    // the message is built only on a refusal: this loop runs n * T times on every call
    const auto where = [T, i] { return "client " + std::to_string(i / T) + ", segment " + std::to_string(i % T); };
    if (code_ptrs[i] == nullptr || scale_ptrs[i] == nullptr) return invalid(where() + ": null code or scale buffer");
    if (misaligned(code_ptrs[i], 16)) return invalid(where() + ": the code buffer is not 16-byte aligned");
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
  MxState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  if (st->d_tiles == nullptr)
    FEDAVG_TRY(span_table(v.seg_numel, v.num_segments, kMxTile, "mx fold", "mx tile table", &st->d_tiles,
                          &st->num_tiles));
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: [n][T] code pointers, [n][T] scale pointers, [T] base pointers, [T] output
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
  std::memcpy(sl.host, code_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_scale, scale_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_base, base_ptrs, seg_bytes);
  std::memcpy(sl.host + o_out, out_ptrs, seg_bytes);
  std::memcpy(sl.host + o_w, weights, w_bytes);
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  MxFoldArgs a;
  a.tiles = st->d_tiles;
  a.codes = reinterpret_cast<const uint8_t* const*>(sl.dev);
  a.scales = reinterpret_cast<const uint8_t* const*>(sl.dev + o_scale);
  a.base = reinterpret_cast<const double* const*>(sl.dev + o_base);
  a.outs = reinterpret_cast<void* const*>(sl.dev + o_out);
  a.w = reinterpret_cast<const double*>(sl.dev + o_w);
  a.divisor = divisor;
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  if (st->num_tiles > 0) {
    if (format == FEDAVG_MXFP8) launch_fold<FEDAVG_MXFP8>(out_dtype, static_cast<unsigned>(st->num_tiles), s, a);
    else launch_fold<FEDAVG_MXFP4>(out_dtype, static_cast<unsigned>(st->num_tiles), s, a);
  }
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("mx fold launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}
