// point_kernels.hip — gfx950 (MI355X) kernels of the squared distance of every client's whole
// update to one fp64 point (fedavg_sqdist_to_point, include/fedavg_hip.h): the device half of the
// geometric median's Weiszfeld iteration, and with no point the clients' squared norms. Not an
// algorithm of the reference: the contract is DESIGN.md §5i and tests/geomed_reference.py restates
// it in numpy.
//
//   out[i] = sum over all elements e of all segments of (x_i[e] - z[e])^2,
// every value converted exactly to fp64, then d = x - z, q = d * d, acc = acc + q: three separately
// rounded fp64 operations, NO FMA (the library is built with -ffp-contract=off). The distances
// become continuous weights of the next fold, so numpy and torch must be able to restate them bit
// for bit. All terms are non-negative: any order is within (P + 2) * 2^-53 relative.
//
// A memory-bound stream (n x P client bytes read once, the point once per chunk, n doubles out):
//   * The layout is cut, segment by segment, into chunks of kPointChunk elements (a segment's last
//     chunk is shorter). A 256-lane workgroup owns one chunk: grid = chunks.
//   * With N = the elements of one 16-byte load of the client dtype ("point_ae_<d>"), the chunk is
//     kPointChunk / N vectors; lane t owns vectors t, t + 256, t + 512, ... and keeps their point
//     values in registers (16 doubles) for the whole chunk: 8 bytes per element read once per
//     chunk, not once per client. Positions past the chunk's end hold x = z = +0.0 and add +0.0,
//     which changes no bit of a non-negative sum.
//   * The clients are walked in table order with 16-byte non-temporal loads; client c + 1's loads
//     are in flight while client c is reduced. A vector that would cross the chunk's end, client
//     storage that is not 16-byte aligned and a point segment that is only 8-byte aligned are read
//     element by element under a guard; nothing outside a tensor is read.
//   * Per client the lane adds its elements in ascending order into ONE accumulator from +0.0; the
//     64 lanes of a wave are combined by a butterfly (a <- a + a[lane ^ off], off = 32, 16, ..., 1:
//     lane 0 ends with the halving tree (l, l + off)); lane 0 of each wave parks the wave's sum in
//     LDS and, once per batch of kPointBatch clients, one lane per client adds the 4 waves in wave
//     order ((w0 + w1) + w2) + w3 and stores the chunk partial to the workspace [chunk][n].
//   * point_reduce_kernel, ordered after it by the stream (no spin-wait), adds each client's chunk
//     partials sequentially from +0.0 in layout order, writes out[i] and latches the accumulator
//     flag for a NaN distance (inf - inf). The input-NaN flag is latched at the load.
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

constexpr int kPointThreads = 256;  // lanes per workgroup
constexpr int kPointWaves = kPointThreads / 64;
constexpr int kPointChunk = 4096;   // elements per workgroup
constexpr int kPointBatch = 64;     // clients whose wave sums are parked in LDS between two barriers
constexpr int kPointMaxClients = FEDAVG_POINT_MAX_CLIENTS;
constexpr int kPointRedClients = 16;   // reduce kernel: clients per workgroup
constexpr int kPointRedTile = 256;     // reduce kernel: chunk partials staged in LDS per step
static_assert(kPointThreads % 64 == 0 && kPointBatch <= kPointThreads, "geometry");
static_assert(kPointRedClients * (kPointThreads / kPointRedClients) == kPointThreads &&
              kPointRedTile % (kPointThreads / kPointRedClients) == 0, "reduce geometry");


struct PArgs {
  const Span* chunks;
  const void* const* ptrs;      // [n][num_segments], every entry non-NULL
  const double* const* point;   // [num_segments], or NULL: the origin
  double* ws;                   // [chunks][n]
  uint32_t* flag;
  int32_t num_segments;
  int32_t n;
};

// ---------------------------------------------------------------------------------------
// the chunk kernel: blockIdx.x = chunk
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kPointThreads) void point_chunk_kernel(PArgs a) {
  using F = Format<T>;
  constexpr int N = F::N;
  constexpr int K = kPointChunk / (N * kPointThreads);  // 16-byte vectors per lane and client
  static_assert(K >= 1 && K * N * kPointThreads == kPointChunk && N % 2 == 0, "chunk geometry");

  __shared__ const void* sptr[kPointMaxClients];
  __shared__ double part[kPointBatch][kPointWaves];

  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63, wave = t >> 6;
  const Span FEDAVG_AS_CONST* cp = (const Span FEDAVG_AS_CONST*)(a.chunks + blockIdx.x);
  const int32_t seg = cp->seg;
  const int32_t count = cp->count;
  const int64_t start = cp->start;
  const int n = a.n;

  // the chunk's client pointers
  for (int c = t; c < n; c += kPointThreads) sptr[c] = a.ptrs[static_cast<int64_t>(c) * a.num_segments + seg];

  // the lane's point values, kept for the whole chunk (+0.0 for the origin and past the chunk's end)
  bool nan_in = false;
  double z[K][N];
  const double* const pz = a.point != nullptr ? a.point[seg] : nullptr;
  const bool pz_vec = (reinterpret_cast<uintptr_t>(pz) & 15u) == 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const int e0 = (k * kPointThreads + t) * N;  // chunk-relative
    const int have = count - e0;
#pragma unroll
    for (int i = 0; i < N; ++i) z[k][i] = 0.0;
    if (pz != nullptr && have > 0) {
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
  __syncthreads();  // sptr is complete

  auto fetch = [&](u32x4(&dst)[K], int c) __attribute__((always_inline)) {
    const void* const p = sptr[c];
    const bool vec = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const int e0 = (k * kPointThreads + t) * N;
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

  // one client: the lane's elements in ascending order into one accumulator, the wave's butterfly,
  // and at a batch's end the waves in wave order -> ws[chunk][client]
  auto reduce = [&](const u32x4(&src)[K], int c) __attribute__((always_inline)) {
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const double x = F::value(src[k], i);
        nan_in |= x != x;
        const double d = x - z[k][i];
        const double q = d * d;
        acc = acc + q;
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off, 64);
    const int slot = c % kPointBatch;
    if (lane == 0) part[slot][wave] = acc;
    if (slot == kPointBatch - 1 || c == n - 1) {  // uniform over the workgroup
      __syncthreads();
      if (t <= slot) {
        double s = part[t][0];
#pragma unroll
        for (int w = 1; w < kPointWaves; ++w) s = s + part[t][w];
        a.ws[static_cast<int64_t>(blockIdx.x) * n + (c - slot + t)] = s;
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

// A workgroup owns kPointRedClients clients: it stages kPointRedTile chunk partials of each in LDS
// (the next tile's loads in flight meanwhile) and one lane per client adds them sequentially from
// +0.0 in chunk order.
__global__ __launch_bounds__(kPointThreads) void point_reduce_kernel(const double* ws, int32_t num_chunks, int32_t n,
                                                                      double* out, uint32_t* flag) {
  constexpr int kRows = kPointThreads / kPointRedClients;  // chunk rows loaded per pass
  constexpr int kLoads = kPointRedTile / kRows;            // loads per lane and tile
  __shared__ double tile[kPointRedTile][kPointRedClients];

  const int t = static_cast<int>(threadIdx.x);
  const int col = t % kPointRedClients, row = t / kPointRedClients;
  const int client = static_cast<int>(blockIdx.x) * kPointRedClients + col;
  double v[kLoads];
  auto fetch = [&](int base) __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < kLoads; ++j) {
      const int r = base + j * kRows + row;
      v[j] = (r < num_chunks && client < n) ? ws[static_cast<int64_t>(r) * n + client] : 0.0;
    }
  };
  double s = 0.0;
  fetch(0);
#pragma unroll 1
  for (int base = 0; base < num_chunks; base += kPointRedTile) {
    __syncthreads();  // the previous tile has been added
#pragma unroll
    for (int j = 0; j < kLoads; ++j) tile[j * kRows + row][col] = v[j];
    __syncthreads();
    if (base + kPointRedTile < num_chunks) fetch(base + kPointRedTile);
    if (t < kPointRedClients) {
      const int cnt = num_chunks - base < kPointRedTile ? num_chunks - base : kPointRedTile;
#pragma unroll 8
      for (int r = 0; r < cnt; ++r) s = s + tile[r][t];
    }
  }
  if (t < kPointRedClients && client < n) {
    out[client] = s;
    if (s != s) raise_flag(flag, 0);  // inf - inf in some element (or a NaN input, flagged at the load too)
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct PointState {
  Span* d_chunks = nullptr;
  int64_t num_chunks = 0;
  double* ws = nullptr;  // grown lazily to the largest client count seen
  size_t ws_bytes = 0;
  TableRing ring;  // a call's tables: clients, then the point
  ~PointState() {
    ring.release();
    if (d_chunks) (void)hipFree(d_chunks);
    if (ws) (void)hipFree(ws);
  }
};

int32_t ensure_state(const fedavg_robust_view& v, void** slot, PointState** out) {
  if (*slot == nullptr) {
    PointState* st = new PointState();
    int32_t r = span_table(v.seg_numel, v.num_segments, kPointChunk, "distance launch", "point chunk table", &st->d_chunks,
                           &st->num_chunks);
    if (r == FEDAVG_OK) r = hip_status("point chunk table", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<PointState*>(*slot);
  return FEDAVG_OK;
}

}  // namespace

int32_t fedavg_internal_point_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "point_chunk") *out = kPointChunk;
  else if (n == "point_threads") *out = kPointThreads;
  else if (n == "point_batch") *out = kPointBatch;
  else if (n == "point_max_clients") *out = kPointMaxClients;
  else if (n == "point_ae_f32") *out = Format<float>::N;
  else if (n == "point_ae_f16") *out = Format<__half>::N;
  else if (n == "point_ae_bf16") *out = Format<bf16_t>::N;
  else if (n == "point_ae_f64") *out = Format<double>::N;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_point_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<PointState*>(state);
}

extern "C" int32_t fedavg_sqdist_to_point(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                          int32_t num_clients, const double* const* point_ptrs, double* out,
                                          void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_POINT, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (in_dtype != FEDAVG_F32 && in_dtype != FEDAVG_F16 && in_dtype != FEDAVG_BF16 && in_dtype != FEDAVG_F64)
    return invalid("distances to a point read dense fp32 / fp16 / bf16 / fp64 tensors (no records)");
  if (client_ptrs == nullptr || out == nullptr) return invalid("null client table or output");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kPointMaxClients)
    return invalid(std::to_string(num_clients) + " clients: distances to a point take at most " +
                   std::to_string(kPointMaxClients));
  if (reinterpret_cast<uintptr_t>(out) % 8 != 0) return invalid("output not aligned to fp64");
  const int T = v.num_segments;
  const size_t elem_bytes = in_dtype == FEDAVG_F64 ? 8 : in_dtype == FEDAVG_F32 ? 4 : 2;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (size_t i = 0; i < entries; ++i) {
    const void* p = client_ptrs[i];
    if (p == nullptr)
      return invalid("client " + std::to_string(i / T) + " lacks segment " + std::to_string(i % T) +
                     ": distances compare whole updates");
    if (reinterpret_cast<uintptr_t>(p) % elem_bytes != 0) return invalid("client tensor not aligned to its element size");
  }
  if (point_ptrs != nullptr) {
    for (int t = 0; t < T; ++t) {
      if (point_ptrs[t] == nullptr) return invalid("the point lacks segment " + std::to_string(t));
      if (reinterpret_cast<uintptr_t>(point_ptrs[t]) % 8 != 0) return invalid("point tensor not aligned to fp64");
    }
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  PointState* st = nullptr;
  const int32_t re = ensure_state(v, slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  const size_t ws_bytes = sizeof(double) * static_cast<size_t>(st->num_chunks) * static_cast<size_t>(num_clients);
  if (st->ws_bytes < ws_bytes) {
    if (st->ws) FEDAVG_TRY_HIP(hipFree(st->ws));  // synchronises with the launches that used it
    st->ws = nullptr;
    st->ws_bytes = 0;
    FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&st->ws), ws_bytes));
    st->ws_bytes = ws_bytes;
  }

  // the call's pointer tables: [n][T] client pointers, then [T] point pointers
  const size_t client_bytes = sizeof(void*) * entries;
  const size_t bytes = client_bytes + (point_ptrs != nullptr ? sizeof(void*) * static_cast<size_t>(T) : 0);
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.acquire(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, client_ptrs, client_bytes);
  if (point_ptrs != nullptr) std::memcpy(sl.host + client_bytes, point_ptrs, bytes - client_bytes);
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  PArgs a;
  a.chunks = st->d_chunks;
  a.ptrs = reinterpret_cast<const void* const*>(sl.dev);
  a.point = point_ptrs != nullptr ? reinterpret_cast<const double* const*>(sl.dev + client_bytes) : nullptr;
  a.ws = st->ws;
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  const dim3 grid(static_cast<unsigned>(st->num_chunks));
  const dim3 block(kPointThreads);
  switch (in_dtype) {
    case FEDAVG_F32: hipLaunchKernelGGL(point_chunk_kernel<float>, grid, block, 0, s, a); break;
    case FEDAVG_F16: hipLaunchKernelGGL(point_chunk_kernel<__half>, grid, block, 0, s, a); break;
    case FEDAVG_BF16: hipLaunchKernelGGL(point_chunk_kernel<bf16_t>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(point_chunk_kernel<double>, grid, block, 0, s, a); break;
  }
  FEDAVG_TRY_HIP(hipGetLastError());
  const unsigned groups = (static_cast<unsigned>(num_clients) + kPointRedClients - 1) / kPointRedClients;
  hipLaunchKernelGGL(point_reduce_kernel, dim3(groups), block, 0, s, st->ws, static_cast<int32_t>(st->num_chunks),
                     num_clients, out, v.d_flag);
  FEDAVG_TRY_HIP(hipGetLastError());
  return st->ring.retire(sl, s);
}
