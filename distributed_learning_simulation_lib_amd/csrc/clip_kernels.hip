// clip_kernels.hip — gfx950 (MI355X) kernel of the fold about a point (fedavg_fold_about_point,
// include/fedavg_hip.h): the device half of centred clipping's step
//   out[e] = z[e] + ( sum_i c_i * (x_i[e] - z[e]) ) / divisor
// with the clients fp32 / fp16 / bf16 / fp64 beside an fp64 point. Not an algorithm of the
// reference: the contract is DESIGN.md §5j and tests/clip_reference.py restates it in numpy.
//
// Per element, every value converted exactly to fp64: d = x - z, p = c * d, acc = p_0 then
// acc = acc + p_i in table order, r = acc / divisor (IEEE division), out = z + r. Each is a
// separately rounded fp64 operation, NO FMA (the library is built with -ffp-contract=off), and the
// first product starts the sum (no leading 0 +), so numpy and torch restate it bit for bit. An
// element's result depends on its own values, the coefficients and the divisor alone.
//
// A memory-bound stream (n x P client bytes and 8 P point bytes read once, P results written):
//   * The layout is cut, segment by segment, into tiles of kClipTile elements (a segment's last
//     tile is shorter). A 256-lane workgroup owns one tile: grid = tiles.
//   * With N = the elements of one 16-byte load of the client dtype ("clip_ae_<d>"), lane t owns
//     the vectors t, t + 256, ...: kClipTile / 256 = 8 elements, whose point values and
//     accumulators stay in registers for the whole tile. The tile's client pointers and the
//     coefficients are cached in LDS once.
//   * The clients are walked in table order with 16-byte non-temporal loads; client c + 1's loads
//     are in flight while client c is folded. A vector that would cross the tile's end, client or
//     output storage that is not 16-byte aligned and a point segment that is only 8-byte aligned
//     take an element-wise path under a guard; nothing outside a tensor is read or written.
//   * Results leave with plain vector stores. No atomics, no workspace, no second kernel.
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

constexpr int kClipThreads = 256;  // lanes per workgroup
constexpr int kClipTile = 2048;    // elements per workgroup: 8 per lane for every client dtype
constexpr int kClipMaxClients = FEDAVG_POINT_MAX_CLIENTS;


struct CArgs {
  const Span* tiles;
  const void* const* ptrs;      // [n][num_segments], every entry non-NULL
  const double* const* point;   // [num_segments]
  void* const* outs;            // [num_segments]
  const double* coef;           // [n]
  double divisor;
  uint32_t* flag;
  int32_t num_segments;
  int32_t n;
};

// One vector's N results to out[elem ..]: `vec` says the 16-byte stores are aligned and inside.
template <typename O, int N>
__device__ __forceinline__ void clip_store(void* base, int64_t elem, const double (&r)[N], int have, bool vec) {
  O FEDAVG_AS_GLOBAL* o = (O FEDAVG_AS_GLOBAL*)base + elem;
  if (vec) {
    if constexpr (sizeof(O) == 8) {
#pragma unroll
      for (int i = 0; i < N; i += 2) {
        const f64x2 v = {r[i], r[i + 1]};
        *(f64x2 FEDAVG_AS_GLOBAL*)(o + i) = v;
      }
    } else if constexpr (N == 2) {  // elem is even and the base 16-byte aligned: an aligned 8-byte store
      const f32x2 v = {static_cast<float>(r[0]), static_cast<float>(r[1])};
      *(f32x2 FEDAVG_AS_GLOBAL*)o = v;
    } else {
#pragma unroll
      for (int i = 0; i < N; i += 4) {
        const f32x4 v = {static_cast<float>(r[i]), static_cast<float>(r[i + 1]), static_cast<float>(r[i + 2]),
                         static_cast<float>(r[i + 3])};
        *(f32x4 FEDAVG_AS_GLOBAL*)(o + i) = v;
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i < have) o[i] = static_cast<O>(r[i]);
    }
  }
}

// ---------------------------------------------------------------------------------------
// the kernel: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
template <typename T, typename O>
__global__ __launch_bounds__(kClipThreads) void clip_fold_kernel(CArgs a) {
  using F = Format<T>;
  constexpr int N = F::N;
  constexpr int K = kClipTile / (N * kClipThreads);  // 16-byte vectors per lane and client
  static_assert(K >= 1 && K * N * kClipThreads == kClipTile && N % 2 == 0, "tile geometry");

  __shared__ const void* sptr[kClipMaxClients];
  __shared__ double scoef[kClipMaxClients];

  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63;
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg;
  const int32_t count = tp->count;
  const int64_t start = tp->start;
  const int n = a.n;

  // the tile's client pointers and the coefficients
  for (int c = t; c < n; c += kClipThreads) {
    sptr[c] = a.ptrs[static_cast<int64_t>(c) * a.num_segments + seg];
    scoef[c] = a.coef[c];
  }

  // the lane's point values, kept for the whole tile (+0.0 past the tile's end)
  bool nan_in = false;
  double z[K][N];
  const double* const pz = a.point[seg];
  const bool pz_vec = (reinterpret_cast<uintptr_t>(pz) & 15u) == 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e0 = (k * kClipThreads + t) * N;  // tile-relative
    const int have = count - e0;
#pragma unroll
    for (int i = 0; i < N; ++i) z[k][i] = 0.0;
    if (have > 0) {
      const double FEDAVG_AS_GLOBAL* q = (const double FEDAVG_AS_GLOBAL*)pz + (start + e0);
      if (have >= N && pz_vec) {  // start and e0 are even: 16-byte aligned with the segment
#pragma unroll
        for (int i = 0; i < N; i += 2) {
          const f64x2 v = *(const f64x2 FEDAVG_AS_GLOBAL*)(q + i);
          z[k][i] = v[0];
          z[k][i + 1] = v[1];
        }
      } else {
#pragma unroll
        for (int i = 0; i < N; ++i) {
          if (i < have) z[k][i] = q[i];
        }
      }
#pragma unroll
      for (int i = 0; i < N; ++i) nan_in |= z[k][i] != z[k][i];
    }
  }
  __syncthreads();  // sptr and scoef are complete

  auto fetch = [&](u32x4(&dst)[K], int c) __attribute__((always_inline)) {
    const void* const p = sptr[c];
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (k * kClipThreads + t) * N;
      const int have = count - e0;
      u32x4 r = {0u, 0u, 0u, 0u};
      if (have > 0) {
        if (have >= N && vec) {
          const u32x4 FEDAVG_AS_GLOBAL* q = (const u32x4 FEDAVG_AS_GLOBAL*)((const T FEDAVG_AS_GLOBAL*)p + (start + e0));
          r = __builtin_nontemporal_load(q);
        } else {
          r = load_guarded<T>(p, start + e0, have);
        }
      }
      dst[k] = r;
    }
  };

  // one client into the lane's accumulators: d = x - z, p = c * d, acc = acc + p (client 0: acc = p)
  double acc[K][N];
  auto fold = [&](const u32x4(&src)[K], int c, bool first) __attribute__((always_inline)) {
    const double w = scoef[c];
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const double x = F::value(src[k], i);
        nan_in |= x != x;
        const double d = x - z[k][i];
        const double p = w * d;
        acc[k][i] = first ? p : acc[k][i] + p;
      }
    }
  };

  u32x4 bufa[K], bufb[K];
  fetch(bufa, 0);
  if (n > 1) fetch(bufb, 1);  // in flight while client 0 is folded
  fold(bufa, 0, true);
#pragma unroll 1
  for (int c = 1; c < n; c += 2) {
    if (c + 1 < n) fetch(bufa, c + 1);
    fold(bufb, c, false);
    if (c + 1 < n) {
      if (c + 2 < n) fetch(bufb, c + 2);
      fold(bufa, c + 1, false);
    }
  }

  // out = z + acc / divisor
  bool nan_acc = false, nan_out = false;
  void* const po = a.outs[seg];
  const bool po_vec = (reinterpret_cast<uintptr_t>(po) & 15u) == 0;
  const double divisor = a.divisor;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e0 = (k * kClipThreads + t) * N;
    const int have = count - e0;
    if (have > 0) {
      double r[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const double s = acc[k][i];
        nan_acc |= s != s;
        const double q = s / divisor;
        const double o = z[k][i] + q;
        nan_out |= o != o;
        r[i] = o;
      }
      clip_store<O, N>(po, start + e0, r, have, have >= N && po_vec);
    }
  }
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
  if (__ballot(nan_acc) != 0ull && lane == 0) raise_flag(a.flag, 0);
  if (__ballot(nan_out) != 0ull && lane == 0) raise_flag(a.flag, 1);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct ClipState {
  Span* d_tiles = nullptr;
  int64_t num_tiles = 0;
  TableRing ring;  // a call's tables: clients, point, outs, coefficients
  ~ClipState() {
    ring.release();
    if (d_tiles) (void)hipFree(d_tiles);
  }
};

int32_t ensure_state(const fedavg_robust_view& v, void** slot, ClipState** out) {
  if (*slot == nullptr) {
    ClipState* st = new ClipState();
    int32_t r = span_table(v.seg_numel, v.num_segments, kClipTile, "fold about a point", "clip tile table", &st->d_tiles,
                           &st->num_tiles);
    if (r == FEDAVG_OK) r = hip_status("clip tile table", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<ClipState*>(*slot);
  return FEDAVG_OK;
}

template <typename O>
void launch(int32_t in_dtype, dim3 grid, dim3 block, hipStream_t s, const CArgs& a) {
  switch (in_dtype) {
    case FEDAVG_F32: hipLaunchKernelGGL((clip_fold_kernel<float, O>), grid, block, 0, s, a); break;
    case FEDAVG_F16: hipLaunchKernelGGL((clip_fold_kernel<__half, O>), grid, block, 0, s, a); break;
    case FEDAVG_BF16: hipLaunchKernelGGL((clip_fold_kernel<bf16_t, O>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((clip_fold_kernel<double, O>), grid, block, 0, s, a); break;
  }
}

}  // namespace

int32_t fedavg_internal_clip_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "clip_tile") *out = kClipTile;
  else if (n == "clip_threads") *out = kClipThreads;
  else if (n == "clip_max_clients") *out = kClipMaxClients;
  else if (n == "clip_ae_f32") *out = Format<float>::N;
  else if (n == "clip_ae_f16") *out = Format<__half>::N;
  else if (n == "clip_ae_bf16") *out = Format<bf16_t>::N;
  else if (n == "clip_ae_f64") *out = Format<double>::N;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_clip_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<ClipState*>(state);
}

extern "C" int32_t fedavg_fold_about_point(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                           const double* coefficients, int32_t num_clients, double divisor,
                                           const double* const* point_ptrs, void* const* out_ptrs,
                                           int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_CLIP, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (in_dtype != FEDAVG_F32 && in_dtype != FEDAVG_F16 && in_dtype != FEDAVG_BF16 && in_dtype != FEDAVG_F64)
    return invalid("the fold about a point reads dense fp32 / fp16 / bf16 / fp64 tensors (no records)");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("the fold about a point writes fp32 or fp64");
  if (client_ptrs == nullptr || coefficients == nullptr || point_ptrs == nullptr || out_ptrs == nullptr)
    return invalid("null client table, coefficients, point or outputs");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kClipMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the fold about a point takes at most " +
                   std::to_string(kClipMaxClients));
  if (!(std::isfinite(divisor) && divisor > 0)) return invalid("the divisor must be finite and > 0");
  for (int32_t i = 0; i < num_clients; ++i)
    if (!std::isfinite(coefficients[i])) return invalid("coefficient " + std::to_string(i) + " is not finite");
  const int T = v.num_segments;
  const size_t elem_bytes = in_dtype == FEDAVG_F64 ? 8 : in_dtype == FEDAVG_F32 ? 4 : 2;
  const size_t out_bytes = out_dtype == FEDAVG_F64 ? 8 : 4;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (size_t i = 0; i < entries; ++i) {
    const void* p = client_ptrs[i];
    if (p == nullptr)
      return invalid("client " + std::to_string(i / T) + " lacks segment " + std::to_string(i % T) +
                     ": the fold about a point takes whole updates");
    if (reinterpret_cast<uintptr_t>(p) % elem_bytes != 0) return invalid("client tensor not aligned to its element size");
  }
  for (int t = 0; t < T; ++t) {
    if (point_ptrs[t] == nullptr) return invalid("the point lacks segment " + std::to_string(t));
    if (reinterpret_cast<uintptr_t>(point_ptrs[t]) % 8 != 0) return invalid("point tensor not aligned to fp64");
    if (out_ptrs[t] == nullptr) return invalid("null output pointer for segment " + std::to_string(t));
    if (reinterpret_cast<uintptr_t>(out_ptrs[t]) % out_bytes != 0) return invalid("output tensor not aligned to its element size");
    if (static_cast<const void*>(out_ptrs[t]) == static_cast<const void*>(point_ptrs[t]))
      return invalid("segment " + std::to_string(t) + ": the step is not in-place (out == point); ping-pong two buffers");
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  ClipState* st = nullptr;
  const int32_t re = ensure_state(v, slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: [n][T] client pointers, [T] point pointers, [T] output pointers, [n] coefficients
  const size_t client_bytes = sizeof(void*) * entries;
  const size_t seg_bytes = sizeof(void*) * static_cast<size_t>(T);
  const size_t coef_bytes = sizeof(double) * static_cast<size_t>(num_clients);
  const size_t bytes = client_bytes + 2 * seg_bytes + coef_bytes;
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.acquire(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, client_ptrs, client_bytes);
  std::memcpy(sl.host + client_bytes, point_ptrs, seg_bytes);
  std::memcpy(sl.host + client_bytes + seg_bytes, out_ptrs, seg_bytes);
  std::memcpy(sl.host + client_bytes + 2 * seg_bytes, coefficients, coef_bytes);
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  CArgs a;
  a.tiles = st->d_tiles;
  a.ptrs = reinterpret_cast<const void* const*>(sl.dev);
  a.point = reinterpret_cast<const double* const*>(sl.dev + client_bytes);
  a.outs = reinterpret_cast<void* const*>(sl.dev + client_bytes + seg_bytes);
  a.coef = reinterpret_cast<const double*>(sl.dev + client_bytes + 2 * seg_bytes);
  a.divisor = divisor;
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  const dim3 grid(static_cast<unsigned>(st->num_tiles));
  const dim3 block(kClipThreads);
  if (out_dtype == FEDAVG_F32) launch<float>(in_dtype, grid, block, s, a);
  else launch<double>(in_dtype, grid, block, s, a);
  FEDAVG_TRY_HIP(hipGetLastError());
  return st->ring.retire(sl, s);
}
