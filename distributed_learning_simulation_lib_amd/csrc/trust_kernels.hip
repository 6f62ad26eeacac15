// trust_kernels.hip — gfx950 (MI355X) kernels of the two moments of every client's whole update
// about one fp64 point (fedavg_moments_about_point, include/fedavg_hip.h): the inner product of
// x_i - v with one fp64 direction g and the squared norm of x_i - v, from the same client bytes in
// one pass. The device half of FLTrust's trust scores. Not an algorithm of the reference: the
// contract is DESIGN.md §5l and tests/trust_reference.py restates it in numpy.
//
//   out[i]     = T_i = sum over all elements e of all segments of (x_i[e] - v[e]) * g[e]
//   out[n + i] = S_i = sum over all elements e of all segments of (x_i[e] - v[e])^2
// every value converted exactly to fp64, then d = x - v, q = d * d, p = d * g, S = S + q, T = T + p:
// five separately rounded fp64 operations, NO FMA (the library is built with -ffp-contract=off).
//
// The geometry and the summation order are point_kernels.hip's, so S_i is bit for
// bit fedavg_sqdist_to_point on the same table and point:
//   * The layout is cut, segment by segment, into chunks of kTrustChunk elements (== point_chunk; a
//     segment's last chunk is shorter). A 256-lane workgroup owns one chunk: grid = chunks.
//   * With N = the elements of one 16-byte load of the client dtype ("trust_ae_<d>"), lane t owns
//     vectors t, t + 256, t + 512, ... of the chunk and keeps their centre AND direction values in
//     registers (16 + 16 doubles) for the whole chunk. Positions past the chunk's end hold
//     x = v = g = +0.0: d = +0.0, q = p = +0.0, and adding +0.0 changes no bit of an accumulator
//     that started at +0.0 (such an accumulator is never -0.0: DESIGN.md §5l).
//   * The clients are walked in table order with 16-byte non-temporal loads; client c + 1's loads
//     are in flight while client c is reduced. A vector that would cross the chunk's end, client
//     storage that is not 16-byte aligned and a centre or direction segment that is only 8-byte
//     aligned are read element by element under a guard; nothing outside a tensor is read.
//   * Per client the lane adds its elements in ascending order into ONE accumulator per sum from
//     +0.0; the 64 lanes of a wave are combined by the halving butterfly (off = 32, 16, ..., 1);
//     lane 0 of each wave parks the wave's two sums in LDS and, once per batch of kTrustBatch
//     clients, one lane per client and sum adds the 4 waves in wave order and stores the chunk
//     partial to the workspace [chunk][2n] (dots, then squared norms).
//   * trust_reduce_kernel, ordered after it by the stream (no spin-wait), adds each of the 2n
//     columns sequentially from +0.0 in layout order, writes out[] and latches the accumulator flag
//     for a NaN output (inf - inf, 0 * inf, +inf + -inf). The input-NaN flag is latched at the load.
// Summation order (the determinism contract): it depends on the layout and, through N, on the
// client dtype — not on the client count, the client's row, the other clients, the batch size, the
// CU count or timing. No floating-point atomics.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kTrustThreads = 256;  // lanes per workgroup
constexpr int kTrustWaves = kTrustThreads / 64;
constexpr int kTrustChunk = 4096;   // elements per workgroup: point_chunk, or S loses its bit-identity
constexpr int kTrustBatch = 64;     // clients whose wave sums are parked in LDS between two barriers
constexpr int kTrustMaxClients = FEDAVG_POINT_MAX_CLIENTS;
constexpr int kTrustRedCols = 16;   // reduce kernel: columns per workgroup
constexpr int kTrustRedTile = 256;  // reduce kernel: chunk partials staged in LDS per step
static_assert(kTrustThreads % 64 == 0 && 2 * kTrustBatch <= kTrustThreads, "geometry");
static_assert(kTrustRedCols * (kTrustThreads / kTrustRedCols) == kTrustThreads &&
              kTrustRedTile % (kTrustThreads / kTrustRedCols) == 0, "reduce geometry");


struct TArgs {
  const Span* chunks;
  const void* const* ptrs;         // [n][num_segments], every entry non-NULL
  const double* const* centre;     // [num_segments], or NULL: the origin
  const double* const* direction;  // [num_segments]
  double* ws;                      // [chunks][2n]
  uint32_t* flag;
  int32_t num_segments;
  int32_t n;
};

// ---------------------------------------------------------------------------------------
// the chunk kernel: blockIdx.x = chunk
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kTrustThreads) void trust_chunk_kernel(TArgs a) {
  using F = Format<T>;
  constexpr int N = F::N;
  constexpr int K = kTrustChunk / (N * kTrustThreads);  // 16-byte vectors per lane and client
  static_assert(K >= 1 && K * N * kTrustThreads == kTrustChunk && N % 2 == 0, "chunk geometry");

  __shared__ const void* sptr[kTrustMaxClients];
  __shared__ double part[2][kTrustBatch][kTrustWaves];  // [dot | squared norm]

  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63, wave = t >> 6;
  const Span FEDAVG_AS_CONST* cp = (const Span FEDAVG_AS_CONST*)(a.chunks + blockIdx.x);
  const int32_t seg = cp->seg;
  const int32_t count = cp->count;
  const int64_t start = cp->start;
  const int n = a.n;

  // the chunk's client pointers
  for (int c = t; c < n; c += kTrustThreads) sptr[c] = a.ptrs[static_cast<int64_t>(c) * a.num_segments + seg];

  // the lane's centre and direction values, kept for the whole chunk (+0.0 for the origin and past
  // the chunk's end)
  bool nan_in = false;
  double v[K][N], g[K][N];
  const double* const pv = a.centre != nullptr ? a.centre[seg] : nullptr;
  const double* const pg = a.direction[seg];
  const bool pv_vec = (reinterpret_cast<uintptr_t>(pv) & 15u) == 0;
  const bool pg_vec = (reinterpret_cast<uintptr_t>(pg) & 15u) == 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e0 = (k * kTrustThreads + t) * N;  // chunk-relative
    const int have = count - e0;
    load_f64<N>(v[k], pv, start + e0, have, pv_vec);
    load_f64<N>(g[k], pg, start + e0, have, pg_vec);
#pragma unroll
    for (int i = 0; i < N; ++i) nan_in |= (v[k][i] != v[k][i]) | (g[k][i] != g[k][i]);
  }
  __syncthreads();  // sptr is complete

  auto fetch = [&](u32x4(&dst)[K], int c) __attribute__((always_inline)) {
    const void* const p = sptr[c];
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (k * kTrustThreads + t) * N;
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

  // one client: the lane's elements in ascending order into one accumulator per sum, the wave's
  // butterfly, and at a batch's end the waves in wave order -> ws[chunk][client], ws[chunk][n + client]
  auto reduce = [&](const u32x4(&src)[K], int c) __attribute__((always_inline)) {
    double sq = 0.0, dot = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const double x = F::value(src[k], i);
        nan_in |= x != x;
        const double d = x - v[k][i];
        const double q = d * d;
        const double p = d * g[k][i];
        sq = sq + q;
        dot = dot + p;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      sq = sq + __shfl_xor(sq, off, 64);
      dot = dot + __shfl_xor(dot, off, 64);
    }
    const int slot = c % kTrustBatch;
    if (lane == 0) {
      part[0][slot][wave] = dot;
      part[1][slot][wave] = sq;
    }
    if (slot == kTrustBatch - 1 || c == n - 1) {  // uniform over the workgroup
      __syncthreads();
      const int which = t / kTrustBatch, r = t % kTrustBatch;  // which < 2 for the lanes that store
      if (which < 2 && r <= slot) {
        double s = part[which][r][0];
#pragma unroll
        for (int w = 1; w < kTrustWaves; ++w) s = s + part[which][r][w];
        a.ws[static_cast<int64_t>(blockIdx.x) * (2 * n) + which * n + (c - slot + r)] = s;
      }
      __syncthreads();  // part is free for the next batch
    }
  };

  u32x4 bufa[K], bufb[K];
  fetch(bufa, 0);
#pragma unroll 1
  for (int c = 0; c < n; c += 2) {
    if (c + 1 < n) fetch(bufb, c + 1);  // in flight while client c is reduced
    reduce(bufa, c);
    if (c + 1 < n) {
      if (c + 2 < n) fetch(bufa, c + 2);
      reduce(bufb, c + 1);
    }
  }
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
}

// A workgroup owns kTrustRedCols of the 2n columns: it stages kTrustRedTile chunk partials of each
// in LDS (the next tile's loads in flight meanwhile) and one lane per column adds them sequentially
// from +0.0 in chunk order.
__global__ __launch_bounds__(kTrustThreads) void trust_reduce_kernel(const double* ws, int32_t num_chunks,
                                                                      int32_t cols, double* out, uint32_t* flag) {
  constexpr int kRows = kTrustThreads / kTrustRedCols;  // chunk rows loaded per pass
  constexpr int kLoads = kTrustRedTile / kRows;         // loads per lane and tile
  __shared__ double tile[kTrustRedTile][kTrustRedCols];

  const int t = static_cast<int>(threadIdx.x);
  const int col = t % kTrustRedCols, row = t / kTrustRedCols;
  const int column = static_cast<int>(blockIdx.x) * kTrustRedCols + col;
  double v[kLoads];
  auto fetch = [&](int base) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < kLoads; ++j) {
      const int r = base + j * kRows + row;
      v[j] = (r < num_chunks && column < cols) ? ws[static_cast<int64_t>(r) * cols + column] : 0.0;
    }
  };
  double s = 0.0;
  fetch(0);
#pragma unroll 1
  for (int base = 0; base < num_chunks; base += kTrustRedTile) {
    __syncthreads();  // the previous tile has been added
#pragma unroll
    for (int j = 0; j < kLoads; ++j) tile[j * kRows + row][col] = v[j];
    __syncthreads();
    if (base + kTrustRedTile < num_chunks) fetch(base + kTrustRedTile);
    if (t < kTrustRedCols) {
      const int cnt = num_chunks - base < kTrustRedTile ? num_chunks - base : kTrustRedTile;
#pragma unroll 8
      for (int r = 0; r < cnt; ++r) s = s + tile[r][t];
    }
  }
  const int mine = static_cast<int>(blockIdx.x) * kTrustRedCols + t;
  if (t < kTrustRedCols && mine < cols) {
    out[mine] = s;
    if (s != s) raise_flag(flag, 0);  // inf - inf, 0 * inf, +inf + -inf (or a NaN input, flagged at the load too)
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct TrustState {
  Span* d_chunks = nullptr;
  int64_t num_chunks = 0;
  double* ws = nullptr;  // grown lazily to the largest client count seen
  size_t ws_bytes = 0;
  TableRing ring;  // a call's tables: clients, direction, centre
  ~TrustState() {
    ring.release();
    if (d_chunks) (void)hipFree(d_chunks);
    if (ws) (void)hipFree(ws);
  }
};

int32_t ensure_state(const fedavg_robust_view& v, void** slot, TrustState** out) {
  if (*slot == nullptr) {
    TrustState* st = new TrustState();
    int32_t r = span_table(v.seg_numel, v.num_segments, kTrustChunk, "moments launch", "trust chunk table", &st->d_chunks,
                           &st->num_chunks);
    if (r == FEDAVG_OK) r = hip_status("trust chunk table", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<TrustState*>(*slot);
  return FEDAVG_OK;
}

}  // namespace

int32_t fedavg_internal_trust_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "trust_chunk") *out = kTrustChunk;
  else if (n == "trust_threads") *out = kTrustThreads;
  else if (n == "trust_batch") *out = kTrustBatch;
  else if (n == "trust_max_clients") *out = kTrustMaxClients;
  else if (n == "trust_ae_f32") *out = Format<float>::N;
  else if (n == "trust_ae_f16") *out = Format<__half>::N;
  else if (n == "trust_ae_bf16") *out = Format<bf16_t>::N;
  else if (n == "trust_ae_f64") *out = Format<double>::N;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_trust_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<TrustState*>(state);
}

extern "C" int32_t fedavg_moments_about_point(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                              int32_t num_clients, const double* const* centre_ptrs,
                                              const double* const* direction_ptrs, double* out, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_TRUST, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (in_dtype != FEDAVG_F32 && in_dtype != FEDAVG_F16 && in_dtype != FEDAVG_BF16 && in_dtype != FEDAVG_F64)
    return invalid("moments about a point read dense fp32 / fp16 / bf16 / fp64 tensors (no records)");
  if (client_ptrs == nullptr || out == nullptr) return invalid("null client table or output");
  if (direction_ptrs == nullptr) return invalid("null direction table");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kTrustMaxClients)
    return invalid(std::to_string(num_clients) + " clients: moments about a point take at most " +
                   std::to_string(kTrustMaxClients));
  if (reinterpret_cast<uintptr_t>(out) % 8 != 0) return invalid("output not aligned to fp64");
  const int T = v.num_segments;
  const size_t elem_bytes = in_dtype == FEDAVG_F64 ? 8 : in_dtype == FEDAVG_F32 ? 4 : 2;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (size_t i = 0; i < entries; ++i) {
    const void* p = client_ptrs[i];
    if (p == nullptr)
      return invalid("client " + std::to_string(i / T) + " lacks segment " + std::to_string(i % T) +
                     ": moments compare whole updates");
    if (reinterpret_cast<uintptr_t>(p) % elem_bytes != 0) return invalid("client tensor not aligned to its element size");
  }
  for (int t = 0; t < T; ++t) {
    if (direction_ptrs[t] == nullptr) return invalid("the direction lacks segment " + std::to_string(t));
    if (reinterpret_cast<uintptr_t>(direction_ptrs[t]) % 8 != 0) return invalid("direction tensor not aligned to fp64");
  }
  if (centre_ptrs != nullptr) {
    for (int t = 0; t < T; ++t) {
      if (centre_ptrs[t] == nullptr) return invalid("the centre lacks segment " + std::to_string(t));
      if (reinterpret_cast<uintptr_t>(centre_ptrs[t]) % 8 != 0) return invalid("centre tensor not aligned to fp64");
    }
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  TrustState* st = nullptr;
  const int32_t re = ensure_state(v, slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  const size_t ws_bytes =
      sizeof(double) * static_cast<size_t>(st->num_chunks) * 2 * static_cast<size_t>(num_clients);
  if (st->ws_bytes < ws_bytes) {
    if (st->ws) FEDAVG_TRY_HIP(hipFree(st->ws));  // synchronises with the launches that used it
    st->ws = nullptr;
    st->ws_bytes = 0;
    FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&st->ws), ws_bytes));
    st->ws_bytes = ws_bytes;
  }

  // the call's pointer tables: [n][T] client pointers, [T] direction pointers, then [T] centre pointers
  const size_t client_bytes = sizeof(void*) * entries;
  const size_t seg_bytes = sizeof(void*) * static_cast<size_t>(T);
  const size_t bytes = client_bytes + seg_bytes + (centre_ptrs != nullptr ? seg_bytes : 0);
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.acquire(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, client_ptrs, client_bytes);
  std::memcpy(sl.host + client_bytes, direction_ptrs, seg_bytes);
  if (centre_ptrs != nullptr) std::memcpy(sl.host + client_bytes + seg_bytes, centre_ptrs, seg_bytes);
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  TArgs a;
  a.chunks = st->d_chunks;
  a.ptrs = reinterpret_cast<const void* const*>(sl.dev);
  a.direction = reinterpret_cast<const double* const*>(sl.dev + client_bytes);
  a.centre = centre_ptrs != nullptr ? reinterpret_cast<const double* const*>(sl.dev + client_bytes + seg_bytes) : nullptr;
  a.ws = st->ws;
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  const dim3 grid(static_cast<unsigned>(st->num_chunks));
  const dim3 block(kTrustThreads);
  switch (in_dtype) {
    case FEDAVG_F32: hipLaunchKernelGGL(trust_chunk_kernel<float>, grid, block, 0, s, a); break;
    case FEDAVG_F16: hipLaunchKernelGGL(trust_chunk_kernel<__half>, grid, block, 0, s, a); break;
    case FEDAVG_BF16: hipLaunchKernelGGL(trust_chunk_kernel<bf16_t>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(trust_chunk_kernel<double>, grid, block, 0, s, a); break;
  }
  FEDAVG_TRY_HIP(hipGetLastError());
  const int32_t cols = 2 * num_clients;
  const unsigned groups = (static_cast<unsigned>(cols) + kTrustRedCols - 1) / kTrustRedCols;
  hipLaunchKernelGGL(trust_reduce_kernel, dim3(groups), block, 0, s, st->ws, static_cast<int32_t>(st->num_chunks),
                     cols, out, v.d_flag);
  FEDAVG_TRY_HIP(hipGetLastError());
  return st->ring.retire(sl, s);
}
