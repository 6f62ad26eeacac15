// opt_kernels.hip — gfx950 (MI355X) kernel of the server optimiser step (fedavg_server_opt_step,
// include/fedavg_hip.h): the fold about a point with the FedOpt epilogue (Reddi et al., "Adaptive
// Federated Optimization", ICLR 2021: FedAvgM, FedAdagrad, FedYogi, FedAdam) fused onto it
//   delta[e] = ( sum_i c_i * (x_i[e] - z[e]) ) / divisor
//   (m', v')[e] = moments(m[e], v[e], delta[e]);  out[e] = z[e] + lr * m'[e] / (sqrt(v'[e]) + tau)
// with the clients fp32 / fp16 / bf16 / fp64 beside an fp64 point and fp64 moments. Not an
// algorithm of the reference: the contract is DESIGN.md §5m and tests/opt_reference.py restates it
// in numpy.
//
// Per element, every value converted exactly to fp64: d = x - z, p = c * d, acc = p_0 then
// acc = acc + p_i in table order, delta = acc / divisor (IEEE division) — so far bit for bit the r
// of clip_kernels.hip — then the mode's lines of opt_epilogue below, each a separately rounded
// fp64 operation, NO FMA (the library is built with -ffp-contract=off), no reciprocal, and a
// correctly rounded square root (opt_sqrt). An element's results depend on its own values, the
// coefficients, the divisor and the hyper-parameters alone.
//
// The tile walk is clip_kernels.hip's (its helpers are restated here so that file's device code
// stays byte for byte what it was):
//   * The layout is cut, segment by segment, into tiles of kOptTile elements (a segment's last
//     tile is shorter). A 256-lane workgroup owns one tile: grid = tiles.
//   * With N = the elements of one 16-byte load of the client dtype ("opt_ae_<d>"), lane t owns the
//     vectors t, t + 256, ...: kOptTile / 256 = 8 elements, whose point values and accumulators
//     stay in registers for the whole tile. The tile's client pointers and the coefficients are
//     cached in LDS once.
//   * The clients are walked in table order with 16-byte non-temporal loads; client c + 1's loads
//     are in flight while client c is folded. A vector that would cross the tile's end, client or
//     output storage that is not 16-byte aligned and point or moment segments that are only 8-byte
//     aligned take an element-wise path under a guard; nothing outside a tensor is read or written.
//   * m and v are needed by the epilogue alone. They are loaded after the last client is folded
//     (FEDAVG_OPT_STATE_EARLY=1 loads them at the tile's start instead, at 32 more live registers
//     through the client loop; DESIGN.md §5m has the measurement).
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

#ifndef FEDAVG_OPT_STATE_EARLY
#define FEDAVG_OPT_STATE_EARLY 0
#endif

namespace {

constexpr int kOptThreads = 256;  // lanes per workgroup
constexpr int kOptTile = 2048;    // elements per workgroup: 8 per lane for every client dtype
constexpr int kOptMaxClients = FEDAVG_POINT_MAX_CLIENTS;


struct OArgs {
  const Span* tiles;
  const void* const* ptrs;      // [n][num_segments], every entry non-NULL
  const double* const* point;   // [num_segments]
  const double* const* m_in;    // [num_segments]
  const double* const* v_in;    // [num_segments]; unused for FEDAVG_OPT_AVGM
  double* const* m_out;         // [num_segments]
  double* const* v_out;         // [num_segments]; unused for FEDAVG_OPT_AVGM
  void* const* outs;            // [num_segments]
  const double* coef;           // [n]
  double divisor;
  double lr, beta1, one_minus_beta1, beta2, one_minus_beta2, tau;
  uint32_t* flag;
  int32_t num_segments;
  int32_t n;
  int32_t mode;
};

// N fp64 values of a point or moment segment from base[elem ..]: `vec` says 16-byte loads are
// aligned and inside; otherwise only elements below `have` are read and the rest stay +0.0.
template <int N>
__device__ __forceinline__ void opt_load_f64(const double* base, int64_t elem, double (&dst)[N], int have, bool vec) {
  const double FEDAVG_AS_GLOBAL* q = (const double FEDAVG_AS_GLOBAL*)base + elem;
  if (vec) {
#pragma unroll
    for (int i = 0; i < N; i += 2) {
      const f64x2 v = *(const f64x2 FEDAVG_AS_GLOBAL*)(q + i);
      dst[i] = v[0];
      dst[i + 1] = v[1];
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) dst[i] = i < have ? q[i] : 0.0;
  }
}

// One vector's N results to out[elem ..]: `vec` says the 16-byte stores are aligned and inside.
template <typename O, int N>
__device__ __forceinline__ void opt_store(void* base, int64_t elem, const double (&r)[N], int have, bool vec) {
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

// The correctly rounded fp64 square root: RN(sqrt(x)) for every x (sqrt(-0) = -0, x < 0 = NaN),
// subnormals included. The compiler's expansion of the IEEE square root for gfx950 (v_rsq_f64, a
// Goldschmidt refinement in FMAs, scaling of inputs below 2^-767) returned numpy's bits on the whole
// edge set of tests/test_gpu_opt_contract.py (zero, subnormals, DBL_MIN, k^2 and its neighbours
// across binades, squares of rounding midpoints and their neighbours, DBL_MAX), so no residual
// correction follows it. This helper is the one place the step takes a root.
__device__ __forceinline__ double opt_sqrt(double x) { return __builtin_sqrt(x); }

// The optimiser lines on one element: delta, m, v -> m', v', u. One rounded operation per line.
__device__ __forceinline__ void opt_epilogue(const OArgs& a, double delta, double m, double v, double& m_new,
                                             double& v_new, double& u) {
  const double am = a.beta1 * m;
  if (a.mode == FEDAVG_OPT_AVGM) {
    m_new = am + delta;
    v_new = 0.0;
    u = a.lr * m_new;
    return;
  }
  const double b = a.one_minus_beta1 * delta;
  m_new = am + b;
  const double q = delta * delta;
  if (a.mode == FEDAVG_OPT_ADAGRAD) {
    v_new = v + q;
  } else if (a.mode == FEDAVG_OPT_ADAM) {
    const double e = a.beta2 * v;
    const double f = a.one_minus_beta2 * q;
    v_new = e + f;
  } else {  // FEDAVG_OPT_YOGI
    const double g = v - q;
    const double s = g > 0.0 ? 1.0 : (g < 0.0 ? -1.0 : 0.0);
    const double f = a.one_minus_beta2 * q;
    const double h = f * s;
    v_new = v - h;
  }
  const double r = opt_sqrt(v_new);
  const double den = r + a.tau;
  const double num = a.lr * m_new;
  u = num / den;
}

// ---------------------------------------------------------------------------------------
// the kernel: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
template <typename T, typename O>
__global__ __launch_bounds__(kOptThreads) void opt_step_kernel(OArgs a) {
  using F = Format<T>;
  constexpr int N = F::N;
  constexpr int K = kOptTile / (N * kOptThreads);  // 16-byte vectors per lane and client
  static_assert(K >= 1 && K * N * kOptThreads == kOptTile && N % 2 == 0, "tile geometry");

  __shared__ const void* sptr[kOptMaxClients];
  __shared__ double scoef[kOptMaxClients];

  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63;
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg;
  const int32_t count = tp->count;
  const int64_t start = tp->start;
  const int n = a.n;
  const bool adaptive = a.mode != FEDAVG_OPT_AVGM;

  // the tile's client pointers and the coefficients
  for (int c = t; c < n; c += kOptThreads) {
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
    const int e0 = (k * kOptThreads + t) * N;  // tile-relative
    const int have = count - e0;
#pragma unroll
    for (int i = 0; i < N; ++i) z[k][i] = 0.0;
    if (have > 0) {
      opt_load_f64<N>(pz, start + e0, z[k], have, have >= N && pz_vec);  // start and e0 are even
#pragma unroll
      for (int i = 0; i < N; ++i) nan_in |= z[k][i] != z[k][i];
    }
  }

  // the lane's moments (+0.0 past the tile's end, and v for FEDAVG_OPT_AVGM)
  double m[K][N], v[K][N];
  auto load_state = [&]() __attribute__((always_inline)) {
    const double* const pm = a.m_in[seg];
    const double* const pv = adaptive ? a.v_in[seg] : nullptr;
    const bool pm_vec = (reinterpret_cast<uintptr_t>(pm) & 15u) == 0;
    const bool pv_vec = (reinterpret_cast<uintptr_t>(pv) & 15u) == 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (k * kOptThreads + t) * N;
      const int have = count - e0;
#pragma unroll
      for (int i = 0; i < N; ++i) m[k][i] = v[k][i] = 0.0;
      if (have > 0) {
        opt_load_f64<N>(pm, start + e0, m[k], have, have >= N && pm_vec);
        if (adaptive) opt_load_f64<N>(pv, start + e0, v[k], have, have >= N && pv_vec);
#pragma unroll
        for (int i = 0; i < N; ++i) nan_in |= (m[k][i] != m[k][i]) | (v[k][i] != v[k][i]);
      }
    }
  };
#if FEDAVG_OPT_STATE_EARLY
  load_state();
#endif
  __syncthreads();  // sptr and scoef are complete

  auto fetch = [&](u32x4(&dst)[K], int c) __attribute__((always_inline)) {
    const void* const p = sptr[c];
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (k * kOptThreads + t) * N;
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
#if !FEDAVG_OPT_STATE_EARLY
  load_state();
#endif

  // delta = acc / divisor, the optimiser lines, out = z + u
  bool nan_acc = false, nan_out = false;
  void* const po = a.outs[seg];
  double* const pmo = a.m_out[seg];
  double* const pvo = adaptive ? a.v_out[seg] : nullptr;
  const bool po_vec = (reinterpret_cast<uintptr_t>(po) & 15u) == 0;
  const bool pmo_vec = (reinterpret_cast<uintptr_t>(pmo) & 15u) == 0;
  const bool pvo_vec = (reinterpret_cast<uintptr_t>(pvo) & 15u) == 0;
  const double divisor = a.divisor;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e0 = (k * kOptThreads + t) * N;
    const int have = count - e0;
    if (have > 0) {
      double r[N], mn[N], vn[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const double s = acc[k][i];
        nan_acc |= s != s;
        const double delta = s / divisor;
        double u;
        opt_epilogue(a, delta, m[k][i], v[k][i], mn[i], vn[i], u);
        const double o = z[k][i] + u;
        nan_out |= (o != o) | (mn[i] != mn[i]) | (vn[i] != vn[i]);
        r[i] = o;
      }
      opt_store<O, N>(po, start + e0, r, have, have >= N && po_vec);
      opt_store<double, N>(pmo, start + e0, mn, have, have >= N && pmo_vec);
      if (adaptive) opt_store<double, N>(pvo, start + e0, vn, have, have >= N && pvo_vec);
    }
  }
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
  if (__ballot(nan_acc) != 0ull && lane == 0) raise_flag(a.flag, 0);
  if (__ballot(nan_out) != 0ull && lane == 0) raise_flag(a.flag, 1);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct OptState {
  Span* d_tiles = nullptr;
  int64_t num_tiles = 0;
  TableRing ring;  // a call's tables: clients, point, moments, outs, coefficients
  ~OptState() {
    ring.release();
    if (d_tiles) (void)hipFree(d_tiles);
  }
};

int32_t ensure_state(const fedavg_robust_view& v, void** slot, OptState** out) {
  if (*slot == nullptr) {
    OptState* st = new OptState();
    int32_t r = span_table(v.seg_numel, v.num_segments, kOptTile, "server optimiser step", "opt tile table", &st->d_tiles,
                           &st->num_tiles);
    if (r == FEDAVG_OK) r = hip_status("opt tile table", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<OptState*>(*slot);
  return FEDAVG_OK;
}

template <typename O>
void launch(int32_t in_dtype, dim3 grid, dim3 block, hipStream_t s, const OArgs& a) {
  switch (in_dtype) {
    case FEDAVG_F32: hipLaunchKernelGGL((opt_step_kernel<float, O>), grid, block, 0, s, a); break;
    case FEDAVG_F16: hipLaunchKernelGGL((opt_step_kernel<__half, O>), grid, block, 0, s, a); break;
    case FEDAVG_BF16: hipLaunchKernelGGL((opt_step_kernel<bf16_t, O>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((opt_step_kernel<double, O>), grid, block, 0, s, a); break;
  }
}

}  // namespace

int32_t fedavg_internal_opt_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "opt_tile") *out = kOptTile;
  else if (n == "opt_threads") *out = kOptThreads;
  else if (n == "opt_max_clients") *out = kOptMaxClients;
  else if (n == "opt_ae_f32") *out = Format<float>::N;
  else if (n == "opt_ae_f16") *out = Format<__half>::N;
  else if (n == "opt_ae_bf16") *out = Format<bf16_t>::N;
  else if (n == "opt_ae_f64") *out = Format<double>::N;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_opt_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<OptState*>(state);
}

extern "C" int32_t fedavg_server_opt_step(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                          const double* coefficients, int32_t num_clients, double divisor,
                                          const double* const* point_ptrs, const double* const* m_in,
                                          const double* const* v_in, double* const* m_out, double* const* v_out,
                                          int32_t mode, double lr, double beta1, double one_minus_beta1,
                                          double beta2, double one_minus_beta2, double tau, void* const* out_ptrs,
                                          int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_OPT, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (in_dtype != FEDAVG_F32 && in_dtype != FEDAVG_F16 && in_dtype != FEDAVG_BF16 && in_dtype != FEDAVG_F64)
    return invalid("the server optimiser step reads dense fp32 / fp16 / bf16 / fp64 tensors (no records)");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("the server optimiser step writes fp32 or fp64");
  if (mode != FEDAVG_OPT_AVGM && mode != FEDAVG_OPT_ADAGRAD && mode != FEDAVG_OPT_YOGI && mode != FEDAVG_OPT_ADAM)
    return invalid("unknown server optimiser mode " + std::to_string(mode));
  const bool adaptive = mode != FEDAVG_OPT_AVGM;
  if (client_ptrs == nullptr || coefficients == nullptr || point_ptrs == nullptr || out_ptrs == nullptr)
    return invalid("null client table, coefficients, point or outputs");
  if (m_in == nullptr || m_out == nullptr) return invalid("null first-moment tables");
  if (adaptive && (v_in == nullptr || v_out == nullptr))
    return invalid("null second-moment tables: only FEDAVG_OPT_AVGM keeps no second moment");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kOptMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the server optimiser step takes at most " +
                   std::to_string(kOptMaxClients));
  if (!(std::isfinite(divisor) && divisor > 0)) return invalid("the divisor must be finite and > 0");
  if (!(std::isfinite(lr) && lr > 0)) return invalid("the learning rate must be finite and > 0");
  if (!(beta1 >= 0 && beta1 < 1)) return invalid("beta1 must lie in [0, 1)");
  if (!(beta2 >= 0 && beta2 < 1)) return invalid("beta2 must lie in [0, 1)");
  if (!std::isfinite(one_minus_beta1) || !std::isfinite(one_minus_beta2))
    return invalid("1 - beta1 and 1 - beta2 must be finite");
  if (adaptive && !(std::isfinite(tau) && tau > 0)) return invalid("tau must be finite and > 0 in the adaptive modes");
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
                     ": the server optimiser step takes whole updates");
    if (reinterpret_cast<uintptr_t>(p) % elem_bytes != 0) return invalid("client tensor not aligned to its element size");
  }
  for (int t = 0; t < T; ++t) {
    const std::string at = "segment " + std::to_string(t);
    if (point_ptrs[t] == nullptr) return invalid("the point lacks " + at);
    if (reinterpret_cast<uintptr_t>(point_ptrs[t]) % 8 != 0) return invalid("point tensor not aligned to fp64");
    if (out_ptrs[t] == nullptr) return invalid("null output pointer for " + at);
    if (reinterpret_cast<uintptr_t>(out_ptrs[t]) % out_bytes != 0) return invalid("output tensor not aligned to its element size");
    if (static_cast<const void*>(out_ptrs[t]) == static_cast<const void*>(point_ptrs[t]))
      return invalid(at + ": the step is not in-place (out == point); ping-pong two buffers");
    if (m_in[t] == nullptr || m_out[t] == nullptr) return invalid("null first-moment pointer for " + at);
    if (reinterpret_cast<uintptr_t>(m_in[t]) % 8 != 0 || reinterpret_cast<uintptr_t>(m_out[t]) % 8 != 0)
      return invalid("first-moment tensor not aligned to fp64");
    if (m_out[t] == m_in[t]) return invalid(at + ": the step is not in-place (m_out == m_in); ping-pong two buffers");
    if (adaptive) {
      if (v_in[t] == nullptr || v_out[t] == nullptr) return invalid("null second-moment pointer for " + at);
      if (reinterpret_cast<uintptr_t>(v_in[t]) % 8 != 0 || reinterpret_cast<uintptr_t>(v_out[t]) % 8 != 0)
        return invalid("second-moment tensor not aligned to fp64");
      if (v_out[t] == v_in[t]) return invalid(at + ": the step is not in-place (v_out == v_in); ping-pong two buffers");
    }
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  OptState* st = nullptr;
  const int32_t re = ensure_state(v, slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: [n][T] client pointers, six [T] pointer tables (point, m_in, v_in, m_out,
  // v_out, outs; the v tables stay zero for FEDAVG_OPT_AVGM), [n] coefficients
  const size_t client_bytes = sizeof(void*) * entries;
  const size_t seg_bytes = sizeof(void*) * static_cast<size_t>(T);
  const size_t coef_bytes = sizeof(double) * static_cast<size_t>(num_clients);
  const size_t bytes = client_bytes + 6 * seg_bytes + coef_bytes;
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.acquire(bytes, &slp));
  TableRing::Slot& sl = *slp;
  const void* const seg_tables[6] = {point_ptrs, m_in, adaptive ? v_in : nullptr, m_out, adaptive ? v_out : nullptr,
                                     out_ptrs};
  std::memcpy(sl.host, client_ptrs, client_bytes);
  for (int k = 0; k < 6; ++k) {
    char* dst = sl.host + client_bytes + k * seg_bytes;
    if (seg_tables[k] != nullptr) std::memcpy(dst, seg_tables[k], seg_bytes);
    else std::memset(dst, 0, seg_bytes);
  }
  std::memcpy(sl.host + client_bytes + 6 * seg_bytes, coefficients, coef_bytes);
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  char* const segs = sl.dev + client_bytes;
  OArgs a;
  a.tiles = st->d_tiles;
  a.ptrs = reinterpret_cast<const void* const*>(sl.dev);
  a.point = reinterpret_cast<const double* const*>(segs);
  a.m_in = reinterpret_cast<const double* const*>(segs + seg_bytes);
  a.v_in = reinterpret_cast<const double* const*>(segs + 2 * seg_bytes);
  a.m_out = reinterpret_cast<double* const*>(segs + 3 * seg_bytes);
  a.v_out = reinterpret_cast<double* const*>(segs + 4 * seg_bytes);
  a.outs = reinterpret_cast<void* const*>(segs + 5 * seg_bytes);
  a.coef = reinterpret_cast<const double*>(segs + 6 * seg_bytes);
  a.divisor = divisor;
  a.lr = lr;
  a.beta1 = beta1;
  a.one_minus_beta1 = one_minus_beta1;
  a.beta2 = beta2;
  a.one_minus_beta2 = one_minus_beta2;
  a.tau = tau;
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  a.mode = mode;
  const dim3 grid(static_cast<unsigned>(st->num_tiles));
  const dim3 block(kOptThreads);
  if (out_dtype == FEDAVG_F32) launch<float>(in_dtype, grid, block, s, a);
  else launch<double>(in_dtype, grid, block, s, a);
  FEDAVG_TRY_HIP(hipGetLastError());
  return st->ring.retire(sl, s);
}
