// krum_kernels.hip — gfx950 (MI355X) kernels of the pairwise squared distances between the
// clients' whole updates (fedavg_pairwise_sqdist, include/fedavg_hip.h), the device half of Krum
// and Multi-Krum. Not an algorithm of the reference: the contract is DESIGN.md §5h and
// tests/krum_reference.py restates it in torch.
//
//   D[i][j] = sum over all elements e of all segments of (x_i[e] - x_j[e])^2,
// every value converted exactly to fp64, one fp64 subtraction, then d * d + acc as one fp64 FMA.
// Never the norm / inner-product form: updates are a common model plus small changes, and that
// form cancels. All terms are non-negative, so any order is within (P + 2) * 2^-53 relative.
//
// This is a symmetric rank-P update with M = N <= 64 per block and a huge K, so K is split:
//   * The layout is cut, segment by segment, into chunks of kKrumChunk elements (a segment's last
//     chunk is shorter). A 256-lane workgroup owns one chunk for one pair of 64-client blocks
//     (I, J), I <= J: grid = (chunks, block pairs).
//   * The chunk is walked in steps of kKrumTile elements. Per step every lane issues 16-byte
//     non-temporal loads (consecutive lanes: consecutive vectors of one client), converts to fp64
//     and parks the values in LDS as [element][client]; the loads of step s + 1 are in flight while
//     step s is computed. A vector that would cross the chunk's end, or whose client storage is not
//     16-byte aligned, is read element by element under a guard; nothing outside a tensor is read.
//   * Lanes map to pairs, not to elements: a lane owns a 4 x 4 block of the 64 x 64 pair matrix in
//     16 fp64 accumulators and reads, per element, its 4 row values and 4 column values from LDS
//     (two 16-byte reads each). A diagonal block pair (I == J) gives lanes only to the 136 blocks on
//     or above the diagonal; an off-diagonal one uses all 256.
//   * At the chunk's end the lane stores its 16 partial sums to the workspace
//     [block pair][chunk][64 x 64] (vector stores; no atomics).
//   * krum_reduce_kernel, ordered after it by the stream, adds each pair's chunk partials in
//     ascending chunk order, mirrors the triangle, writes +0.0 on the diagonal and latches the
//     accumulator flag for a NaN distance (inf - inf). The input-NaN flag is latched at the load.
// Summation order (the determinism contract): within a chunk ascending element order into one
// accumulator per pair, chunks in layout order (segment by segment, ascending offset). It depends
// on the layout alone — not on the client count, the CU count or timing.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kKrumThreads = 256;   // lanes per workgroup
constexpr int kKrumBlock = 64;      // clients per row / column block
constexpr int kKrumReg = 4;         // a lane owns kKrumReg x kKrumReg pairs
constexpr int kKrumTile = 32;       // elements staged in LDS per step
constexpr int kKrumChunk = 8192;    // elements per workgroup
constexpr int kKrumMaxClients = FEDAVG_KRUM_MAX_CLIENTS;
constexpr int kKrumBlocksPerSide = kKrumBlock / kKrumReg;                             // 16
constexpr int kKrumDiagBlocks = kKrumBlocksPerSide * (kKrumBlocksPerSide + 1) / 2;    // 136
constexpr int kKrumPairs = kKrumBlock * kKrumBlock;  // workspace doubles per (block pair, chunk)
// doubles per staged element row: 64 clients + 2 of padding, which spreads the staging writes
// over the banks and keeps every row 16-byte aligned for the paired reads
constexpr int kKrumStride = kKrumBlock + 2;
static_assert(kKrumChunk % kKrumTile == 0 && kKrumBlocksPerSide * kKrumBlocksPerSide == kKrumThreads, "geometry");
static_assert(kKrumStride % 2 == 0, "16-byte aligned rows");


struct KArgs {
  const Span* chunks;
  const void* const* ptrs;  // [n][num_segments], every entry non-NULL
  double* ws;               // [block pairs][chunks][kKrumPairs]
  uint32_t* flag;
  int32_t num_segments;
  int32_t n;
  int32_t num_chunks;
  int32_t pad_;
};

// Block pair index of (I, J), I <= J, with NB blocks per side: row-major over the upper triangle.
__host__ __device__ __forceinline__ int krum_block_pair(int I, int J, int NB) {
  return I * NB - I * (I - 1) / 2 + (J - I);
}

// ---------------------------------------------------------------------------------------
// the chunk kernel: blockIdx.x = chunk, blockIdx.y = block pair
// ---------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kKrumThreads) void krum_chunk_kernel(KArgs a) {
  using F = Format<T>;
  constexpr int N = F::N;
  constexpr int kVecs = kKrumTile / N;                           // 16-byte vectors per client per step
  constexpr int kLoads = kKrumBlock * kVecs / kKrumThreads;      // vectors per lane per step and side
  static_assert(kKrumTile % N == 0 && (kKrumBlock * kVecs) % kKrumThreads == 0 && kLoads >= 1, "staging geometry");

  __shared__ __attribute__((aligned(16))) double stage[2][kKrumTile * kKrumStride];
  __shared__ const void* sptr[2 * kKrumBlock];

  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* cp = (const Span FEDAVG_AS_CONST*)(a.chunks + blockIdx.x);
  const int32_t seg = cp->seg;
  const int32_t count = cp->count;
  const int64_t start = cp->start;
  const int n = a.n;
  const int NB = (n + kKrumBlock - 1) / kKrumBlock;
  int I = 0, rem = static_cast<int>(blockIdx.y);
  while (rem >= NB - I) {
    rem -= NB - I;
    ++I;
  }
  const int J = I + rem;
  const bool diag = I == J;
  const int nrows = (n - I * kKrumBlock) < kKrumBlock ? (n - I * kKrumBlock) : kKrumBlock;
  const int ncols = (n - J * kKrumBlock) < kKrumBlock ? (n - J * kKrumBlock) : kKrumBlock;

  // the chunk's client pointers (rows, then columns); slots past the block's clients stay NULL and
  // stage zeros
  if (t < 2 * kKrumBlock) {
    const int side = t / kKrumBlock, c = t % kKrumBlock;
    const int nb = side ? ncols : nrows;
    const int client = (side ? J : I) * kKrumBlock + c;
    sptr[t] = c < nb ? a.ptrs[static_cast<int64_t>(client) * a.num_segments + seg] : nullptr;
  }
  __syncthreads();

  // the lane's 4 x 4 block (bi, bj) of the pair matrix
  int bi, bj;
  bool active;
  if (diag) {
    int r = t;
    bi = 0;
    while (bi < kKrumBlocksPerSide && r >= kKrumBlocksPerSide - bi) {
      r -= kKrumBlocksPerSide - bi;
      ++bi;
    }
    bj = bi + r;
    active = bi < kKrumBlocksPerSide;
  } else {
    bi = t / kKrumBlocksPerSide;
    bj = t % kKrumBlocksPerSide;
    active = true;
  }
  active = active && kKrumReg * bi < nrows && kKrumReg * bj < ncols;

  const int sides = diag ? 1 : 2;
  u32x4 raw[2][kLoads];
  auto fetch = [&](int step) __attribute__((always_inline)) {
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      if (side < sides) {
#pragma unroll
        for (int k = 0; k < kLoads; ++k) {
          const int idx = t + k * kKrumThreads;
          const int c = idx / kVecs, v = idx % kVecs;
          const int e0 = step * kKrumTile + v * N;  // chunk-relative
          const int have = count - e0;
          const void* p = sptr[side * kKrumBlock + c];
          u32x4 r = {0u, 0u, 0u, 0u};
          if (p != nullptr && have > 0) {
            if (have >= N && (reinterpret_cast<uintptr_t>(p) & 15u) == 0) {
              const u32x4 FEDAVG_AS_GLOBAL* q = (const u32x4 FEDAVG_AS_GLOBAL*)((const T FEDAVG_AS_GLOBAL*)p + (start + e0));
              r = __builtin_nontemporal_load(q);
            } else {
              r = load_guarded<T>(p, start + e0, have);
            }
          }
          raw[side][k] = r;
        }
      }
    }
  };

  double acc[kKrumReg][kKrumReg];
#pragma unroll
  for (int r = 0; r < kKrumReg; ++r)
#pragma unroll
    for (int c = 0; c < kKrumReg; ++c) acc[r][c] = 0.0;

  bool nan_in = false;
  const int steps = (count + kKrumTile - 1) / kKrumTile;
  const double* const rowv = stage[0] + kKrumReg * bi;
  const double* const colv = stage[diag ? 0 : 1] + kKrumReg * bj;
  fetch(0);
#pragma unroll 1
  for (int step = 0; step < steps; ++step) {
    __syncthreads();  // the previous step's values have been read by every lane
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      if (side < sides) {
#pragma unroll
        for (int k = 0; k < kLoads; ++k) {
          const int idx = t + k * kKrumThreads;
          const int c = idx / kVecs, v = idx % kVecs;
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const double x = F::value(raw[side][k], i);
            nan_in |= x != x;
            stage[side][(v * N + i) * kKrumStride + c] = x;
          }
        }
      }
    }
    __syncthreads();
    if (step + 1 < steps) fetch(step + 1);  // in flight while this step is computed
    if (active) {
#pragma unroll 4
      for (int e = 0; e < kKrumTile; ++e) {
        const f64x2 a01 = *reinterpret_cast<const f64x2*>(rowv + e * kKrumStride);
        const f64x2 a23 = *reinterpret_cast<const f64x2*>(rowv + e * kKrumStride + 2);
        const f64x2 b01 = *reinterpret_cast<const f64x2*>(colv + e * kKrumStride);
        const f64x2 b23 = *reinterpret_cast<const f64x2*>(colv + e * kKrumStride + 2);
        const double av[kKrumReg] = {a01[0], a01[1], a23[0], a23[1]};
        const double bv[kKrumReg] = {b01[0], b01[1], b23[0], b23[1]};
#pragma unroll
        for (int r = 0; r < kKrumReg; ++r) {
#pragma unroll
          for (int c = 0; c < kKrumReg; ++c) {
            const double d = av[r] - bv[c];
            acc[r][c] = __builtin_fma(d, d, acc[r][c]);
          }
        }
      }
    }
  }

  if (active) {
    const int bp = static_cast<int>(blockIdx.y);
    double* const w = a.ws + (static_cast<int64_t>(bp) * a.num_chunks + static_cast<int64_t>(blockIdx.x)) * kKrumPairs +
                      (kKrumReg * bi) * kKrumBlock + kKrumReg * bj;
#pragma unroll
    for (int r = 0; r < kKrumReg; ++r) {
      const f64x2 lo = {acc[r][0], acc[r][1]}, hi = {acc[r][2], acc[r][3]};
      *reinterpret_cast<f64x2*>(w + r * kKrumBlock) = lo;
      *reinterpret_cast<f64x2*>(w + r * kKrumBlock + 2) = hi;
    }
  }
  if (__ballot(nan_in) != 0ull && (t & 63) == 0) raise_flag(a.flag, 2);
}

// One lane per (i, j), i <= j: the pair's chunk partials added in ascending chunk order, the
// result mirrored; the diagonal is +0.0.
__global__ __launch_bounds__(kKrumThreads) void krum_reduce_kernel(const double* ws, int32_t num_chunks, int32_t n,
                                                                   double* out, uint32_t* flag) {
  const int idx = static_cast<int>(blockIdx.x) * kKrumThreads + static_cast<int>(threadIdx.x);
  if (idx >= n * n) return;
  const int i = idx / n, j = idx % n;
  if (i > j) return;
  if (i == j) {
    out[idx] = 0.0;
    return;
  }
  const int NB = (n + kKrumBlock - 1) / kKrumBlock;
  const int bp = krum_block_pair(i / kKrumBlock, j / kKrumBlock, NB);
  const double* p = ws + static_cast<int64_t>(bp) * num_chunks * kKrumPairs + (i % kKrumBlock) * kKrumBlock + (j % kKrumBlock);
  double s = 0.0;
#pragma unroll 8
  for (int c = 0; c < num_chunks; ++c) s += p[static_cast<int64_t>(c) * kKrumPairs];
  out[static_cast<int64_t>(i) * n + j] = s;
  out[static_cast<int64_t>(j) * n + i] = s;
  if (s != s) raise_flag(flag, 0);  // inf - inf in some element (or a NaN input, flagged at the load too)
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct KrumState {
  Span* d_chunks = nullptr;
  int64_t num_chunks = 0;
  double* ws = nullptr;  // grown lazily to the largest client count seen
  size_t ws_bytes = 0;
  TableRing ring;  // a call's tables: the client pointers
  ~KrumState() {
    ring.release();
    if (d_chunks) (void)hipFree(d_chunks);
    if (ws) (void)hipFree(ws);
  }
};

int32_t ensure_state(const fedavg_robust_view& v, void** slot, KrumState** out) {
  if (*slot == nullptr) {
    KrumState* st = new KrumState();
    int32_t r = span_table(v.seg_numel, v.num_segments, kKrumChunk, "distance launch", "krum chunk table", &st->d_chunks,
                           &st->num_chunks);
    if (r == FEDAVG_OK) r = hip_status("krum chunk table", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<KrumState*>(*slot);
  return FEDAVG_OK;
}

}  // namespace

int32_t fedavg_internal_krum_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "krum_chunk") *out = kKrumChunk;
  else if (n == "krum_tile") *out = kKrumTile;
  else if (n == "krum_block") *out = kKrumBlock;
  else if (n == "krum_reg") *out = kKrumReg;
  else if (n == "krum_threads") *out = kKrumThreads;
  else if (n == "krum_max_clients") *out = kKrumMaxClients;
  else if (n == "krum_ae_f32") *out = Format<float>::N;
  else if (n == "krum_ae_f16") *out = Format<__half>::N;
  else if (n == "krum_ae_bf16") *out = Format<bf16_t>::N;
  else if (n == "krum_ae_f64") *out = Format<double>::N;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_krum_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<KrumState*>(state);
}

extern "C" int32_t fedavg_pairwise_sqdist(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                          int32_t num_clients, double* out, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_KRUM, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (in_dtype != FEDAVG_F32 && in_dtype != FEDAVG_F16 && in_dtype != FEDAVG_BF16 && in_dtype != FEDAVG_F64)
    return invalid("pairwise distances read dense fp32 / fp16 / bf16 / fp64 tensors (no records)");
  if (client_ptrs == nullptr || out == nullptr) return invalid("null client table or output");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kKrumMaxClients)
    return invalid(std::to_string(num_clients) + " clients: pairwise distances take at most " +
                   std::to_string(kKrumMaxClients));
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

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  KrumState* st = nullptr;
  const int32_t re = ensure_state(v, slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  const int NB = (num_clients + kKrumBlock - 1) / kKrumBlock;
  const int num_bp = NB * (NB + 1) / 2;
  const size_t ws_bytes = sizeof(double) * static_cast<size_t>(num_bp) * static_cast<size_t>(st->num_chunks) * kKrumPairs;
  if (st->ws_bytes < ws_bytes) {
    if (st->ws) FEDAVG_TRY_HIP(hipFree(st->ws));  // synchronises with the launches that used it
    st->ws = nullptr;
    st->ws_bytes = 0;
    FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&st->ws), ws_bytes));
    st->ws_bytes = ws_bytes;
  }

  const size_t bytes = sizeof(void*) * entries;
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.acquire(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, client_ptrs, bytes);
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  KArgs a;
  a.chunks = st->d_chunks;
  a.ptrs = reinterpret_cast<const void* const*>(sl.dev);
  a.ws = st->ws;
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  a.num_chunks = static_cast<int32_t>(st->num_chunks);
  a.pad_ = 0;
  const dim3 grid(static_cast<unsigned>(st->num_chunks), static_cast<unsigned>(num_bp));
  const dim3 block(kKrumThreads);
  switch (in_dtype) {
    case FEDAVG_F32: hipLaunchKernelGGL(krum_chunk_kernel<float>, grid, block, 0, s, a); break;
    case FEDAVG_F16: hipLaunchKernelGGL(krum_chunk_kernel<__half>, grid, block, 0, s, a); break;
    case FEDAVG_BF16: hipLaunchKernelGGL(krum_chunk_kernel<bf16_t>, grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL(krum_chunk_kernel<double>, grid, block, 0, s, a); break;
  }
  FEDAVG_TRY_HIP(hipGetLastError());
  const unsigned cells = static_cast<unsigned>(num_clients) * static_cast<unsigned>(num_clients);
  hipLaunchKernelGGL(krum_reduce_kernel, dim3((cells + kKrumThreads - 1) / kKrumThreads), block, 0, s, st->ws,
                     static_cast<int32_t>(st->num_chunks), num_clients, out, v.d_flag);
  FEDAVG_TRY_HIP(hipGetLastError());
  return st->ring.retire(sl, s);
}
