// dp_kernels.hip — gfx950 (MI355X) kernels of the clip-and-noise pass (fedavg_dp_noise,
// include/fedavg_hip.h): the arithmetic of the reference's add_dp_noise / add_dp_noise_to_parameter
// (simulation_lib/dp.py:13-47) on tensors that lie in HBM. The contract is DESIGN.md §5r;
// tests/dp_reference.py restates it in numpy.
//
// Every arithmetic line is one separately rounded fp64 operation after the exact widening of the
// element: no FMA (the library is built with -ffp-contract=off), no reciprocal, IEEE division, the
// correctly rounded square root.
//   q = x * x;  acc = acc + q                                   (from +0.0, in the order below)
//   norm = sqrt(acc);  t = norm / C;  s = (t < 1) ? 1 : t       (a NaN t stays NaN)
//   y = x / s;  n = z * noise_scale;  o = y + n;  out = RNE(o) into the dtype (one rounding)
// z is the element's normal deviate (dp_normal_pair below). No atomics; three launches:
//   * dp_sumsq_kernel: a sum (the whole list, or one row) is cut into pieces of kDTile elements:
//     whole-list mode cuts every tensor from its start, row mode every row from its start. With G =
//     the elements of 16 bytes, lane j of 256 owns the piece's groups j, j + 256, ... of G consecutive
//     elements and adds their squares in increasing index; the 256 lane sums combine by the
//     adjacent-pair tree ((l0 + l1) + (l2 + l3)) + ... . All terms are >= +0.0, so a lane that owns
//     nothing holds +0.0 and changes no bit: a row shorter than a piece is summed by a team of
//     W = 2^k >= ceil(L / G) lanes and 256 / W rows share a workgroup. Raises the context's input
//     flag at a non-finite element.
//   * dp_scale_kernel: lane j of 256 adds the sum's piece partials j, j + 256, ... in increasing
//     index (whole-list mode: all pieces of all tensors in list order), the same tree combines the
//     lanes, and the lines of norm, t, s follow: one s per row, or one in all.
//   * dp_apply_kernel: over tiles of kDTile elements of every tensor (a tile starts at a multiple
//     of kDTile elements of its tensor, so at an even index: a Box-Muller pair never belongs to two
//     workgroups). A lane owns 16-byte groups: one 16-byte load and store where the group is
//     complete and 16-byte aligned in both the input and the output; the groups are shifted to the
//     tensor's alignment where that keeps pairs whole, which leaves a head and a tail that go
//     element by element, as does a tensor whose 16-byte boundaries fall on odd elements. An element
//     is read and then written by the same lane: out[t] == in[t] is allowed.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kDThreads = 256;   // lanes per workgroup
constexpr int kDTile = 4096;     // elements per piece of a sum and per tile of the apply pass
constexpr int kDMaxTensors = 1 << 20;
static_assert(kDTile % (kDThreads * 8) == 0, "every lane owns whole groups of a full tile");

struct DArgs {
  const Span* tiles;       // the tiles of every tensor, in list order
  const void* const* in;   // [T]; NULL only where numel == 0
  void* const* out;        // [T]
  const uint32_t* ids;     // [T]: the tensor's counter word of the normal stream
  double* part;            // the piece partials
  double* scale;           // s: [rows], or [1]
  uint32_t* flag;          // the context's NaN words (0 acc, 1 result, 2 input)
  int64_t row_len;         // 0: whole-list mode
  int64_t rows;
  int64_t row_pieces;      // pieces per row
  int64_t num_parts;       // whole-list mode: pieces of all tensors
  int32_t team;            // row mode: lanes that sum one row's piece
  double C, noise_scale;
  uint32_t key0, key1, draw;
};

// ---------------------------------------------------------------------------------------
// the normal stream (include/fedavg_hip.h): one Philox block, one Box-Muller pair
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double d_from_bits(uint64_t b) { return __longlong_as_double(static_cast<long long>(b)); }

// ln(v * 2^-53) for an integer v in [1, 2^53]: <= 0, and -0.0 only at v = 2^53
__device__ __forceinline__ double dp_ln(uint64_t v) {
  const double d = static_cast<double>(static_cast<long long>(v));  // exact
  const uint64_t bits = static_cast<uint64_t>(__double_as_longlong(d));
  const uint64_t frac = bits & 0x000fffffffffffffull;
  const int up = frac >= 0x6a09e667f3bcdull ? 1 : 0;  // the mantissa is >= sqrt(2)
  const int e = static_cast<int>(bits >> 52) - 1023 - 53 + up;
  const double m = d_from_bits(frac | (static_cast<uint64_t>(1023 - up) << 52));  // in [sqrt(1/2), sqrt(2))
  const double f = m - 1.0;  // exact
  const double g = 2.0 + f;
  const double s = f / g;
  const double w = s * s;
  double p = 0x1.8618618618618p-5;  // 1/21
  p = p * w;
  p = p + 0x1.af286bca1af28p-5;  // 1/19
  p = p * w;
  p = p + 0x1.e1e1e1e1e1e1ep-5;  // 1/17
  p = p * w;
  p = p + 0x1.1111111111111p-4;  // 1/15
  p = p * w;
  p = p + 0x1.3b13b13b13b14p-4;  // 1/13
  p = p * w;
  p = p + 0x1.745d1745d1746p-4;  // 1/11
  p = p * w;
  p = p + 0x1.c71c71c71c71cp-4;  // 1/9
  p = p * w;
  p = p + 0x1.2492492492492p-3;  // 1/7
  p = p * w;
  p = p + 0x1.999999999999ap-3;  // 1/5
  p = p * w;
  p = p + 0x1.5555555555555p-2;  // 1/3
  p = p * w;
  p = p * s;
  const double q = s + p;
  const double lm = q + q;
  const double ek = static_cast<double>(e);
  const double el = ek * 0x1.62e42fefa39efp-1;  // ln 2
  return el + lm;
}

// sin and cos of x = g * pi/4, g in [0, 1]
__device__ __forceinline__ void dp_sincos(double g, double& sn, double& cs) {
  const double x = g * 0x1.921fb54442d18p-1;  // pi / 4
  const double w = x * x;
  double p = 0x1.952c77030ad4ap-49;  // 1/17!
  p = p * w;
  p = p + -0x1.ae7f3e733b81fp-41;  // -1/15!
  p = p * w;
  p = p + 0x1.6124613a86d09p-33;  // 1/13!
  p = p * w;
  p = p + -0x1.ae64567f544e4p-26;  // -1/11!
  p = p * w;
  p = p + 0x1.71de3a556c734p-19;  // 1/9!
  p = p * w;
  p = p + -0x1.a01a01a01a01ap-13;  // -1/7!
  p = p * w;
  p = p + 0x1.1111111111111p-7;  // 1/5!
  p = p * w;
  p = p + -0x1.5555555555555p-3;  // -1/3!
  p = p * w;
  p = p * x;
  sn = x + p;
  double c = 0x1.ae7f3e733b81fp-45;  // 1/16!
  c = c * w;
  c = c + -0x1.93974a8c07c9dp-37;  // -1/14!
  c = c * w;
  c = c + 0x1.1eed8eff8d898p-29;  // 1/12!
  c = c * w;
  c = c + -0x1.27e4fb7789f5cp-22;  // -1/10!
  c = c * w;
  c = c + 0x1.a01a01a01a01ap-16;  // 1/8!
  c = c * w;
  c = c + -0x1.6c16c16c16c17p-10;  // -1/6!
  c = c * w;
  c = c + 0x1.5555555555555p-5;  // 1/4!
  c = c * w;
  c = c + -0x1.0p-1;  // -1/2!
  c = c * w;
  cs = 1.0 + c;
}

// z[2 * block], z[2 * block + 1] of tensor `id`
__device__ __forceinline__ void dp_normal_pair(const DArgs& a, uint32_t id, uint64_t block, double& z0, double& z1) {
  const QWords o = q_philox(static_cast<uint32_t>(block), static_cast<uint32_t>(block >> 32), id, a.draw, a.key0, a.key1);
  const uint64_t ia = (static_cast<uint64_t>(o.w[1] >> 5) << 26) | static_cast<uint64_t>(o.w[0] >> 6);
  const uint64_t ib = (static_cast<uint64_t>(o.w[3] >> 5) << 26) | static_cast<uint64_t>(o.w[2] >> 6);
  const double lu = dp_ln(ia + 1);
  const double t = lu * -2.0;
  const double r = __builtin_sqrt(t);  // correctly rounded (opt_kernels.hip, opt_sqrt)
  // 8 * u2 = k + fi * 2^-50 exactly: the octant and the position in it
  const uint32_t k = static_cast<uint32_t>(ib >> 50);
  const uint64_t fi = ib & ((1ull << 50) - 1);
  const uint64_t gi = (k & 1u) ? (1ull << 50) - fi : fi;
  const double g = static_cast<double>(static_cast<long long>(gi)) * 0x1p-50;  // exact
  double sn, cs;
  dp_sincos(g, sn, cs);
  const bool swap = ((k + 1u) >> 1) & 1u;
  double c = swap ? sn : cs;
  double s = swap ? cs : sn;
  if (((k + 2u) >> 2) & 1u) c = -c;
  if (k >> 2) s = -s;
  z0 = r * c;
  z1 = r * s;
}

// ---------------------------------------------------------------------------------------
// elements in and out of a 16-byte image
// ---------------------------------------------------------------------------------------
// elements [lo, hi) of the group that starts at element `elem`; the rest stay +0.0
template <typename T>
__device__ __forceinline__ u32x4 dp_load_part(const void* base, int64_t elem, int lo, int hi) {
  constexpr int N = Format<T>::N;
  u32x4 raw = {0u, 0u, 0u, 0u};
  if constexpr (sizeof(T) == 2) {
    const uint16_t FEDAVG_AS_GLOBAL* p = (const uint16_t FEDAVG_AS_GLOBAL*)base + elem;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i >= lo && i < hi) raw[i / 2] |= static_cast<uint32_t>(p[i]) << (16 * (i % 2));
    }
  } else {
    constexpr int W = sizeof(T) / 4;  // 32-bit words per element
    const uint32_t FEDAVG_AS_GLOBAL* p = (const uint32_t FEDAVG_AS_GLOBAL*)base + elem * W;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i >= lo && i < hi) {
#pragma unroll
        for (int w = 0; w < W; ++w) raw[i * W + w] = p[i * W + w];
      }
    }
  }
  return raw;
}

template <typename T>
__device__ __forceinline__ void dp_store_part(void* base, int64_t elem, int lo, int hi, const u32x4& raw) {
  constexpr int N = Format<T>::N;
  if constexpr (sizeof(T) == 2) {
    uint16_t FEDAVG_AS_GLOBAL* p = (uint16_t FEDAVG_AS_GLOBAL*)base + elem;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i >= lo && i < hi) p[i] = static_cast<uint16_t>(raw[i / 2] >> (16 * (i % 2)));
    }
  } else {
    constexpr int W = sizeof(T) / 4;
    uint32_t FEDAVG_AS_GLOBAL* p = (uint32_t FEDAVG_AS_GLOBAL*)base + elem * W;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i >= lo && i < hi) {
#pragma unroll
        for (int w = 0; w < W; ++w) p[i * W + w] = raw[i * W + w];
      }
    }
  }
}

// The float nearest to o that is odd where o is no float ("round to odd"): rounding it to a
// narrower format (at most 22 bits) gives what one rounding of o gives.
__device__ __forceinline__ uint32_t dp_odd_float_bits(double o) {
  const float f = static_cast<float>(o);
  uint32_t u = __float_as_uint(f);
  if (o == o && static_cast<double>(f) != o) {
    if (__builtin_fabs(static_cast<double>(f)) > __builtin_fabs(o)) u -= 1u;  // towards zero (from infinity too)
    u |= 1u;
  }
  return u;
}

// RNE(o) into T, as the bits of element i of the image
template <typename T>
__device__ __forceinline__ void dp_put(u32x4& raw, int i, double o);
template <>
__device__ __forceinline__ void dp_put<float>(u32x4& raw, int i, double o) {
  raw[i] = __float_as_uint(static_cast<float>(o));
}
template <>
__device__ __forceinline__ void dp_put<double>(u32x4& raw, int i, double o) {
  const uint64_t b = static_cast<uint64_t>(__double_as_longlong(o));
  raw[2 * i] = static_cast<uint32_t>(b);
  raw[2 * i + 1] = static_cast<uint32_t>(b >> 32);
}
template <>
__device__ __forceinline__ void dp_put<__half>(u32x4& raw, int i, double o) {
  const __half h = __float2half_rn(__uint_as_float(dp_odd_float_bits(o)));
  raw[i / 2] |= static_cast<uint32_t>(__half_as_ushort(h)) << (16 * (i % 2));
}
template <>
__device__ __forceinline__ void dp_put<bf16_t>(u32x4& raw, int i, double o) {
  const uint32_t u = dp_odd_float_bits(o);
  const uint32_t b = (o == o) ? (u + 0x7fffu + ((u >> 16) & 1u)) >> 16 : 0x7fc0u;
  raw[i / 2] |= b << (16 * (i % 2));
}

// the adjacent-pair tree over the first `width` (a power of two) lanes of every aligned block of
// `width` lanes; the block's sum is valid in its first lane
__device__ __forceinline__ double dp_tree(double v, int width, double* sm) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    if (off < width) v = v + __shfl_xor(v, off);
  }
  if (width > 64) {  // the same for every lane of the workgroup
    const int t = static_cast<int>(threadIdx.x);
    if ((t & 63) == 0) sm[t >> 6] = v;
    __syncthreads();
    const double a = sm[0] + sm[1], b = sm[2] + sm[3];
    v = width == 128 ? ((t & 128) ? b : a) : a + b;
  }
  return v;
}

// ---------------------------------------------------------------------------------------
// pass 1: the piece partials
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kDThreads) void dp_sumsq_kernel(DArgs a) {
  constexpr int N = Format<T>::N;
  __shared__ double sm[kDThreads / 64];
  const int t = static_cast<int>(threadIdx.x);
  const void* base = nullptr;
  int64_t first = 0, unit = 0;
  int count = 0, j = t, width = kDThreads;
  bool live = true;
  if (a.row_len == 0) {
    const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
    base = a.in[tp->seg];
    first = tp->start;
    count = tp->count;
    unit = blockIdx.x;
  } else {
    width = a.team;
    unit = static_cast<int64_t>(blockIdx.x) * (kDThreads / width) + t / width;
    j = t % width;
    live = unit < a.rows * a.row_pieces;
    if (live) {
      const int64_t row = unit / a.row_pieces, piece = unit - row * a.row_pieces;
      const int64_t left = a.row_len - piece * kDTile;
      base = a.in[0];
      first = row * a.row_len + piece * kDTile;
      count = static_cast<int>(left < kDTile ? left : kDTile);
    }
  }
  double acc = 0.0;
  bool bad = false;
  if (live) {
    for (int g = j; g * N < count; g += width) {
      const int64_t e = first + static_cast<int64_t>(g) * N;
      const int have = count - g * N < N ? count - g * N : N;
      const char* p = static_cast<const char*>(base) + e * static_cast<int64_t>(sizeof(T));
      u32x4 raw;
      if (have == N && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) raw = *(const u32x4 FEDAVG_AS_GLOBAL*)p;
      else raw = load_guarded<T>(base, e, have);
#pragma unroll
      for (int i = 0; i < N; ++i) {  // past `have`: +0.0, which changes nothing
        const double x = Format<T>::value(raw, i);
        bad |= !(__builtin_fabs(x) < __builtin_huge_val());
        const double q = x * x;
        acc = acc + q;
      }
    }
  }
  acc = dp_tree(acc, width, sm);
  if (live && j == 0) a.part[unit] = acc;
  if (__ballot(bad) != 0ull && (t & 63) == 0) raise_flag(a.flag, 2);
}

// ---------------------------------------------------------------------------------------
// pass 2: one s per row, or one in all
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ double dp_finish(double acc, double C) {
  const double norm = __builtin_sqrt(acc);
  const double t = norm / C;
  return t < 1.0 ? 1.0 : t;  // a NaN t stays NaN
}

__global__ __launch_bounds__(kDThreads) void dp_scale_kernel(DArgs a) {
  __shared__ double sm[kDThreads / 64];
  const int t = static_cast<int>(threadIdx.x);
  if (a.row_len != 0 && a.row_pieces == 1) {  // a row's one partial is its sum: a lane per row
    const int64_t row = static_cast<int64_t>(blockIdx.x) * kDThreads + t;
    if (row < a.rows) a.scale[row] = dp_finish(a.part[row], a.C);
    return;
  }
  const int64_t first = a.row_len != 0 ? static_cast<int64_t>(blockIdx.x) * a.row_pieces : 0;
  const int64_t k = a.row_len != 0 ? a.row_pieces : a.num_parts;
  double acc = 0.0;
  for (int64_t i = t; i < k; i += kDThreads) acc = acc + a.part[first + i];
  acc = dp_tree(acc, kDThreads, sm);
  if (t == 0) a.scale[blockIdx.x] = dp_finish(acc, a.C);
}

// ---------------------------------------------------------------------------------------
// pass 3: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kDThreads) void dp_apply_kernel(DArgs a) {
  constexpr int N = Format<T>::N;
  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg;
  const int32_t count = tp->count;
  const int64_t start = tp->start;
  const void* const in = a.in[seg];
  void* const out = a.out[seg];
  const uint32_t id = a.ids[seg];
  // elements up to the input's first 16-byte boundary at or after the tile's start; the groups are
  // shifted to it where it is even (kDTile is a multiple of N: the same shift in every tile)
  const uintptr_t addr0 = reinterpret_cast<uintptr_t>(in) + static_cast<uintptr_t>(start) * sizeof(T);
  const int head = static_cast<int>(((16u - (addr0 & 15u)) & 15u) / sizeof(T));
  const int shift = (head != 0 && head % 2 == 0) ? N - head : 0;
  const int slots = kDTile / N + (shift != 0 ? 1 : 0);
  const bool by_row = a.row_len != 0;
  const double s_all = by_row ? 1.0 : a.scale[0];

  for (int slot = t; slot < slots; slot += kDThreads) {
    const int p = slot * N - shift;  // the group's first element in the tile: even, < 0 for a head
    const int lo = p < 0 ? -p : 0;
    const int hi = count - p < N ? count - p : N;  // the group holds elements [lo, hi) of its N
    if (lo >= hi) continue;
    const int64_t e = start + p;
    const char* const pi = static_cast<const char*>(in) + e * static_cast<int64_t>(sizeof(T));
    char* const po = static_cast<char*>(out) + e * static_cast<int64_t>(sizeof(T));
    const bool vec = lo == 0 && hi == N && ((reinterpret_cast<uintptr_t>(pi) | reinterpret_cast<uintptr_t>(po)) & 15u) == 0;
    u32x4 raw;
    if (vec) raw = *(const u32x4 FEDAVG_AS_GLOBAL*)pi;
    else raw = dp_load_part<T>(in, e, lo, hi);

    int64_t row = 0, rem = 0;
    double s = s_all;
    if (by_row) {
      row = (e + lo) / a.row_len;
      rem = (e + lo) - row * a.row_len;
      s = a.scale[row];
    }
    u32x4 res = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int pr = 0; pr < N / 2; ++pr) {
      if (2 * pr + 1 < lo || 2 * pr >= hi) continue;  // no element of the pair is here
      double z[2];
      dp_normal_pair(a, id, static_cast<uint64_t>(e + 2 * pr) >> 1, z[0], z[1]);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int i = 2 * pr + h;
        if (i < lo || i >= hi) continue;
        const double x = Format<T>::value(raw, i);
        const double y = x / s;
        const double n = z[h] * a.noise_scale;
        const double o = y + n;
        dp_put<T>(res, i, o);
        if (by_row && ++rem == a.row_len) {
          rem = 0;
          ++row;
          if (row < a.rows) s = a.scale[row];
        }
      }
    }
    if (vec) *(u32x4 FEDAVG_AS_GLOBAL*)po = res;
    else dp_store_part<T>(out, e, lo, hi, res);
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct DpState {
  double* d_part = nullptr;   // the piece partials of the call in flight
  size_t part_cap = 0;
  double* d_scale = nullptr;  // its s values
  size_t scale_cap = 0;
  TableRing ring;
  ~DpState() {
    ring.release();
    if (d_part) (void)hipFree(d_part);
    if (d_scale) (void)hipFree(d_scale);
  }
};

int32_t ensure_state(void** slot, DpState** out) {
  if (*slot == nullptr) {
    DpState* st = new DpState();
    const int32_t r = hip_status("dp state", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<DpState*>(*slot);
  return FEDAVG_OK;
}

// hipFree waits for the device: no launch still reads the old buffer
int32_t grow(double** buf, size_t* cap, size_t need) {
  if (*cap >= need) return FEDAVG_OK;
  if (*buf) FEDAVG_TRY_HIP(hipFree(*buf));
  *buf = nullptr;
  *cap = 0;
  const size_t n = need * 2 < 1024 ? 1024 : need * 2;
  FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(buf), n * sizeof(double)));
  *cap = n;
  return FEDAVG_OK;
}

size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

template <typename T>
void launch_all(unsigned sum_grid, unsigned scale_grid, unsigned tiles, hipStream_t s, const DArgs& a) {
  const dim3 block(kDThreads);
  if (sum_grid > 0) hipLaunchKernelGGL((dp_sumsq_kernel<T>), dim3(sum_grid), block, 0, s, a);
  hipLaunchKernelGGL(dp_scale_kernel, dim3(scale_grid), block, 0, s, a);
  if (tiles > 0) hipLaunchKernelGGL((dp_apply_kernel<T>), dim3(tiles), block, 0, s, a);
}

}  // namespace

int32_t fedavg_internal_dp_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "dp_tile") *out = kDTile;
  else if (n == "dp_threads") *out = kDThreads;
  else if (n == "dp_ae_f32") *out = Format<float>::N;
  else if (n == "dp_ae_f16") *out = Format<__half>::N;
  else if (n == "dp_ae_bf16") *out = Format<bf16_t>::N;
  else if (n == "dp_ae_f64") *out = Format<double>::N;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_dp_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<DpState*>(state);
}

extern "C" int32_t fedavg_dp_noise(fedavg_ctx* ctx, int32_t dtype, const void* const* in_ptrs, const int64_t* numels,
                                   const uint32_t* tensor_ids, int32_t num_tensors, void* const* out_ptrs,
                                   int64_t row_len, double C, double noise_scale, uint64_t seed, uint32_t draw,
                                   void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_DP, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (dtype != FEDAVG_F32 && dtype != FEDAVG_F16 && dtype != FEDAVG_BF16 && dtype != FEDAVG_F64)
    return invalid("the clip-and-noise pass takes fp32, fp16, bf16 or fp64 tensors");
  if (in_ptrs == nullptr || numels == nullptr || out_ptrs == nullptr)
    return invalid("null input table, element counts or output table");
  if (num_tensors < 1 || num_tensors > kDMaxTensors)
    return invalid("the clip-and-noise pass takes between 1 and " + std::to_string(kDMaxTensors) + " tensors");
  if (!(std::isfinite(C) && C > 0)) return invalid("the clipping norm C must be finite and > 0");
  if (!(std::isfinite(noise_scale) && noise_scale >= 0)) return invalid("the noise scale must be finite and >= 0");
  if (row_len < 0) return invalid("negative row length");
  if (row_len > 0 && num_tensors != 1) return invalid("row mode takes one tensor");
  const int T = num_tensors;
  const size_t esize = dtype == FEDAVG_F64 ? 8 : (dtype == FEDAVG_F32 ? 4 : 2);
  const int group = static_cast<int>(16 / esize);
  uint64_t num_tiles = 0;
  for (int t = 0; t < T; ++t) {
    if (numels[t] < 0) return invalid("tensor " + std::to_string(t) + ": negative element count");
    if (numels[t] > 0 && (in_ptrs[t] == nullptr || out_ptrs[t] == nullptr))
      return invalid("tensor " + std::to_string(t) + ": null input or output");
    if (misaligned(in_ptrs[t], esize) || misaligned(out_ptrs[t], esize))
      return invalid("tensor " + std::to_string(t) + ": input or output not aligned to its element size");
    num_tiles += (static_cast<uint64_t>(numels[t]) + kDTile - 1) / kDTile;
  }
  if (row_len > 0 && numels[0] % row_len != 0) return invalid("the row length does not divide the tensor");
  if (num_tiles > 0x7fffffffull) return invalid("layout too large for one clip-and-noise call");
  const int64_t rows = row_len > 0 ? numels[0] / row_len : 0;
  const int64_t row_pieces = row_len > 0 ? (row_len + kDTile - 1) / kDTile : 0;
  int team = kDThreads;
  if (row_len > 0) {
    const int64_t groups = ((row_len < kDTile ? row_len : kDTile) + group - 1) / group;
    team = 1;
    while (team < kDThreads && team < groups) team <<= 1;
  }
  uint64_t sum_grid = num_tiles, scale_grid = 1, parts = num_tiles, scales = 1;
  if (row_len > 0) {
    if (rows == 0) return FEDAVG_OK;  // an empty tensor: nothing to read or write
    const uint64_t units = static_cast<uint64_t>(rows) * static_cast<uint64_t>(row_pieces);
    const uint64_t per = static_cast<uint64_t>(kDThreads / team);
    sum_grid = (units + per - 1) / per;
    scale_grid = row_pieces == 1 ? (static_cast<uint64_t>(rows) + kDThreads - 1) / kDThreads : static_cast<uint64_t>(rows);
    parts = units;
    scales = static_cast<uint64_t>(rows);
    if (sum_grid > 0x7fffffffull || scale_grid > 0x7fffffffull) return invalid("too many rows for one clip-and-noise call");
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  DpState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);
  FEDAVG_TRY(grow(&st->d_part, &st->part_cap, parts));
  FEDAVG_TRY(grow(&st->d_scale, &st->scale_cap, scales));

  // the call's tables: the tiles, [T] input pointers, [T] output pointers, [T] stream ids
  const size_t tile_bytes = align16(sizeof(Span) * num_tiles);
  const size_t ptr_bytes = align16(sizeof(void*) * static_cast<size_t>(T));
  const size_t id_bytes = align16(sizeof(uint32_t) * static_cast<size_t>(T));
  const size_t o_in = tile_bytes, o_out = o_in + ptr_bytes, o_id = o_out + ptr_bytes;
  const size_t bytes = o_id + id_bytes;
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memset(sl.host, 0, bytes);
  Span* const h_tiles = reinterpret_cast<Span*>(sl.host);
  uint32_t* const h_ids = reinterpret_cast<uint32_t*>(sl.host + o_id);
  size_t k = 0;
  for (int t = 0; t < T; ++t) {
    h_ids[t] = tensor_ids ? tensor_ids[t] : static_cast<uint32_t>(t);
    for (int64_t b = 0; b < numels[t]; b += kDTile) {
      const int64_t left = numels[t] - b;
      h_tiles[k++] = Span{t, static_cast<int32_t>(left < kDTile ? left : kDTile), b};
    }
  }
  std::memcpy(sl.host + o_in, in_ptrs, sizeof(void*) * static_cast<size_t>(T));
  std::memcpy(sl.host + o_out, out_ptrs, sizeof(void*) * static_cast<size_t>(T));
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  DArgs a;
  a.tiles = reinterpret_cast<const Span*>(sl.dev);
  a.in = reinterpret_cast<const void* const*>(sl.dev + o_in);
  a.out = reinterpret_cast<void* const*>(sl.dev + o_out);
  a.ids = reinterpret_cast<const uint32_t*>(sl.dev + o_id);
  a.part = st->d_part;
  a.scale = st->d_scale;
  a.flag = v.d_flag;
  a.row_len = row_len;
  a.rows = rows;
  a.row_pieces = row_pieces;
  a.num_parts = static_cast<int64_t>(num_tiles);
  a.team = team;
  a.C = C;
  a.noise_scale = noise_scale;
  a.key0 = static_cast<uint32_t>(seed & 0xffffffffull);
  a.key1 = static_cast<uint32_t>(seed >> 32);
  a.draw = draw;
  const unsigned g1 = static_cast<unsigned>(sum_grid), g2 = static_cast<unsigned>(scale_grid),
                 g3 = static_cast<unsigned>(num_tiles);
  if (dtype == FEDAVG_F32) launch_all<float>(g1, g2, g3, s, a);
  else if (dtype == FEDAVG_F16) launch_all<__half>(g1, g2, g3, s, a);
  else if (dtype == FEDAVG_BF16) launch_all<bf16_t>(g1, g2, g3, s, a);
  else launch_all<double>(g1, g2, g3, s, a);
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("dp noise launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}
