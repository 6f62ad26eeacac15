// gram_kernels.hip — gfx950 (MI355X) kernels of the Gram matrix of the clients' whole updates about
// one fp64 point (fedavg_gram_about_point, include/fedavg_hip.h), the device half of FoolsGold. Not
// an algorithm of the reference: the contract is DESIGN.md §5y and tests/foolsgold_reference.py
// restates it in numpy.
//
//   G[i][j] = sum over all elements e of all segments of r_i[e] * r_j[e],
//   r_i[e] = d_i[e] = x_i[e] - v[e]            without history,
//   r_i[e] = h_i[e] = history_in_i[e] + d_i[e] with it (h is stored to history_out_i[e]);
// every value converted exactly to fp64, the subtract and the add separately rounded. The products
// are summed by v_mfma_f64_16x16x4_f64, the fp64 matrix instruction: fused into the sum, in the
// hardware's order inside one instruction. The rows are small updates about v, so the inner-product
// form does not cancel the way it would for Krum's distances.
//
// A symmetric rank-P update with M = N <= 64 per block and a huge K, so K is split as in
// krum_kernels.hip:
//   * The layout is cut, segment by segment, into chunks of kGramChunk elements. A 256-lane
//     workgroup (4 waves) owns one chunk for one pair of 64-client blocks (I, J), I <= J:
//     grid = (chunks, block pairs).
//   * The chunk is walked in steps of kGramTile = 32 elements. Per step every lane issues 16-byte
//     non-temporal client loads (consecutive lanes: consecutive vectors of one client) and the
//     matching point and history loads, converts, subtracts, adds and parks r in LDS as
//     [element][client] with a row stride of 66 doubles; the loads of step s + 1 are in flight while
//     step s is multiplied. The diagonal pair (I == J) alone stores h to history_out, so every
//     history element is written by exactly one lane of one workgroup. A vector that would cross the
//     chunk's end, or storage that is not 16-byte aligned, is read and written element by element
//     under a guard; nothing outside a tensor is touched.
//   * The 64 x 64 block of G is 4 x 4 tiles of 16 x 16. Wave w of an off-diagonal pair owns the tile
//     row w; the waves of a diagonal pair share the 10 tiles on or above the diagonal (3, 3, 2, 2).
//     A tile whose strip lies past the block's last client is skipped. A tile's 16 x 16 fp64 sums live
//     in 4 accumulator doubles per lane for the whole chunk.
//   * The matrix instruction takes A[i][k] from lane 16 k + i and B[k][j] from lane 16 k + j: for a
//     Gram matrix both are "client l % 16 of a strip at the k-slot l / 16", so one LDS read pattern
//     serves both and a diagonal tile passes one register twice. Which element a k-slot holds is
//     free (the sum runs over all of them): k-step s of a tile step gives slot g the staged row
//     8 g + s. With the 66-double stride the two rows a half-wave reads are 16 doubles apart modulo
//     the 32 double-wide banks, and the staging writes of one instruction spread over all of them.
//   * D[i][j] comes back in register v of lane l with i = 4 v + l / 16, j = l % 16. At the chunk's
//     end the lanes store their tiles to the workspace [block pair][chunk][64 x 64] (vector stores;
//     no atomics).
//   * gram_reduce_kernel, ordered after it by the stream, adds each entry's chunk partials in
//     ascending chunk order, mirrors the triangle and latches the accumulator flag for a NaN entry.
//     The input-NaN flag is latched at the load.
// Rows past a chunk's end and clients past the block's last stage +0.0: a 0 * inf of such a slot
// lands in a padding row or column of the block, which the reduce kernel never reads.
// Determinism: k-steps ascending inside a chunk, chunks in layout order. It depends on the layout
// and on the block a client falls in — not on the CU count or timing.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kGramThreads = 256;  // lanes per workgroup
constexpr int kGramBlock = 64;     // clients per row / column block
constexpr int kGramEdge = 16;      // edge of a matrix-instruction tile
constexpr int kGramK = 4;          // elements one matrix instruction contracts
constexpr int kGramTile = 32;      // elements staged in LDS per step
constexpr int kGramChunk = 8192;   // elements per workgroup
constexpr int kGramMaxClients = FEDAVG_GRAM_MAX_CLIENTS;
constexpr int kGramStrips = kGramBlock / kGramEdge;  // 4
constexpr int kGramKSteps = kGramTile / kGramK;      // 8 matrix instructions per tile and step
constexpr int kGramSlots = 4;                        // tiles a wave owns at most
constexpr int kGramPairs = kGramBlock * kGramBlock;  // workspace doubles per (block pair, chunk)
// doubles per staged element row: 64 clients + 2. 66 = 2 mod 32, so rows 8 apart sit 16 double-wide
// banks apart (the fragment reads) and rows 4, 8 or 2 apart sit 8, 16 or 4 apart (the staging writes
// of fp32, 2-byte and fp64 clients)
constexpr int kGramStride = kGramBlock + 2;
static_assert(kGramChunk % kGramTile == 0 && kGramThreads == 64 * kGramStrips, "geometry");
static_assert(kGramKSteps * kGramStrips == kGramTile && kGramK * 16 == 64, "one k-slot per 16 lanes");

typedef double f64x4 __attribute__((ext_vector_type(4)));

struct GArgs {
  const Span* chunks;
  const void* const* ptrs;      // [n][num_segments], every entry non-NULL
  const double* const* point;   // [num_segments], or NULL: the origin
  const double* const* hin;     // [n][num_segments], or NULL
  double* const* hout;          // [n][num_segments], or NULL
  double* ws;                   // [block pairs][chunks][kGramPairs]
  uint32_t* flag;
  int32_t num_segments;
  int32_t n;
  int32_t num_chunks;
  int32_t pad_;
};

// Block pair index of (I, J), I <= J, with NB blocks per side: row-major over the upper triangle.
__host__ __device__ __forceinline__ int gram_block_pair(int I, int J, int NB) {
  return I * NB - I * (I - 1) / 2 + (J - I);
}

// The tiles (R, C), R <= C, of a diagonal block pair, by wave and slot: 3, 3, 2, 2.
__device__ __forceinline__ void gram_diag_tile(int wave, int slot, int& R, int& C, bool& owned) {
  const int first = wave < 2 ? 3 * wave : 6 + 2 * (wave - 2);
  const int many = wave < 2 ? 3 : 2;
  owned = slot < many;
  int r = first + slot;  // index into the row-major upper triangle of the 4 x 4 tiles
  R = 0;
  while (R < kGramStrips - 1 && r >= kGramStrips - R) {
    r -= kGramStrips - R;
    ++R;
  }
  C = R + r;
}

// ---------------------------------------------------------------------------------------
// the chunk kernel: blockIdx.x = chunk, blockIdx.y = block pair
// ---------------------------------------------------------------------------------------
// Without history the kernel fits 4 workgroups on a CU with no scratch once the compiler is told to
// aim for them; with history (two more fp64 operands per staged value) it is left its own budget.
template <typename T, bool kHist>
__global__ __launch_bounds__(kGramThreads) __attribute__((amdgpu_waves_per_eu(kHist ? 1 : 4, kHist ? 8 : 4)))
void gram_chunk_kernel(GArgs a) {
  using F = Format<T>;
  constexpr int N = F::N;
  constexpr int kVecs = kGramTile / N;                       // 16-byte vectors per client per step
  constexpr int kLoads = kGramBlock * kVecs / kGramThreads;  // vectors per lane per step and side
  constexpr int kH = kHist ? kLoads : 1;
  static_assert(kGramTile % N == 0 && (kGramBlock * kVecs) % kGramThreads == 0 && kLoads >= 1 && N % 2 == 0,
                "staging geometry");

  __shared__ __attribute__((aligned(16))) double stage[2][kGramTile * kGramStride];
  __shared__ const void* sptr[2 * kGramBlock];
  __shared__ const double* shin[2 * kGramBlock];
  __shared__ double* shout[kGramBlock];

  const int t = static_cast<int>(threadIdx.x);
  const Span FEDAVG_AS_CONST* cp = (const Span FEDAVG_AS_CONST*)(a.chunks + blockIdx.x);
  const int32_t seg = cp->seg;
  const int32_t count = cp->count;
  const int64_t start = cp->start;
  const int n = a.n;
  const int NB = (n + kGramBlock - 1) / kGramBlock;
  int I = 0, rem = static_cast<int>(blockIdx.y);
  while (rem >= NB - I) {
    rem -= NB - I;
    ++I;
  }
  const int J = I + rem;
  const bool diag = I == J;
  const int nrows = (n - I * kGramBlock) < kGramBlock ? (n - I * kGramBlock) : kGramBlock;
  const int ncols = (n - J * kGramBlock) < kGramBlock ? (n - J * kGramBlock) : kGramBlock;

  // the chunk's client and history pointers (rows, then columns); slots past the block's clients
  // stay NULL and stage +0.0
  if (t < 2 * kGramBlock) {
    const int side = t / kGramBlock, c = t % kGramBlock;
    const int nb = side ? ncols : nrows;
    const int64_t entry = static_cast<int64_t>((side ? J : I) * kGramBlock + c) * a.num_segments + seg;
    const bool live = c < nb;
    sptr[t] = live ? a.ptrs[entry] : nullptr;
    if constexpr (kHist) {
      shin[t] = live ? a.hin[entry] : nullptr;
      if (side == 0) shout[c] = live ? a.hout[entry] : nullptr;
    }
  }
  const double* const pv = a.point != nullptr ? a.point[seg] : nullptr;
  const bool pv_vec = (reinterpret_cast<uintptr_t>(pv) & 15u) == 0;
  __syncthreads();

  // the wave's tiles: LDS offsets of its A and B fragments (doubles), wave-uniform
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int g = lane >> 4, j = lane & 15;  // the lane's k-slot and its client inside a strip
  int tR[kGramSlots], tC[kGramSlots];
  bool live[kGramSlots];
#pragma unroll
  for (int s = 0; s < kGramSlots; ++s) {
    if (diag) {
      gram_diag_tile(wave, s, tR[s], tC[s], live[s]);
    } else {
      tR[s] = wave;
      tC[s] = s;
      live[s] = true;
    }
    live[s] = live[s] && kGramEdge * tR[s] < nrows && kGramEdge * tC[s] < ncols;
  }

  const int sides = diag ? 1 : 2;
  u32x4 raw[2][kLoads];
  double pt[kLoads][N];
  double hist[2][kH][N];
  auto fetch = [&](int step) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const int idx = t + k * kGramThreads;
      const int c = idx / kVecs, v = idx % kVecs;
      const int e0 = step * kGramTile + v * N;  // chunk-relative
      const int have = count - e0;
      load_f64<N>(pt[k], pv, start + e0, have, pv_vec);
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        if (side < sides) {
          const void* p = sptr[side * kGramBlock + c];
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
          if constexpr (kHist) {
            const double* hp = shin[side * kGramBlock + c];  // NULL (a padding client): +0.0
            load_f64<N>(hist[side][k], hp, start + e0, have, (reinterpret_cast<uintptr_t>(hp) & 15u) == 0);
          }
        }
      }
    }
  };

  f64x4 acc[kGramSlots];
#pragma unroll
  for (int s = 0; s < kGramSlots; ++s) acc[s] = f64x4{0.0, 0.0, 0.0, 0.0};

  bool nan_in = false;
  const int steps = (count + kGramTile - 1) / kGramTile;
  fetch(0);
#pragma unroll 1
  for (int step = 0; step < steps; ++step) {
    __syncthreads();  // the previous step's values have been read by every wave
#pragma unroll
    for (int k = 0; k < kLoads; ++k) {
      const int idx = t + k * kGramThreads;
      const int c = idx / kVecs, v = idx % kVecs;
      const int e0 = step * kGramTile + v * N;
      const int have = count - e0;
#pragma unroll
      for (int i = 0; i < N; ++i) nan_in |= pt[k][i] != pt[k][i];
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        if (side < sides) {
          const bool present = sptr[side * kGramBlock + c] != nullptr;
          double r[N];
#pragma unroll
          for (int i = 0; i < N; ++i) {
            const double x = F::value(raw[side][k], i);
            nan_in |= x != x;
            double d = present ? x - pt[k][i] : 0.0;
            if constexpr (kHist) {
              const double h = hist[side][k][i];
              nan_in |= h != h;
              d = h + d;
            }
            r[i] = d;
            stage[side][(v * N + i) * kGramStride + c] = d;
          }
          if constexpr (kHist) {
            // the diagonal pair's rows are every client of block I once: the one writer of history_out
            if (diag && side == 0 && present && have > 0) {
              double FEDAVG_AS_GLOBAL* q = (double FEDAVG_AS_GLOBAL*)shout[c] + (start + e0);
              if (have >= N && (reinterpret_cast<uintptr_t>(shout[c]) & 15u) == 0) {
#pragma unroll
                for (int i = 0; i < N; i += 2) *(f64x2 FEDAVG_AS_GLOBAL*)(q + i) = f64x2{r[i], r[i + 1]};
              } else {
#pragma unroll
                for (int i = 0; i < N; ++i) {
                  if (i < have) q[i] = r[i];
                }
              }
            }
          }
        }
      }
    }
    __syncthreads();
    if (step + 1 < steps) fetch(step + 1);  // in flight while this step is multiplied
    const double* const rows = stage[0] + (kGramKSteps * g) * kGramStride + j;
    const double* const cols = stage[diag ? 0 : 1] + (kGramKSteps * g) * kGramStride + j;
#pragma unroll 2
    for (int ks = 0; ks < kGramKSteps; ++ks) {
#pragma unroll
      for (int s = 0; s < kGramSlots; ++s) {
        if (live[s]) {  // wave-uniform
          const double av = rows[ks * kGramStride + kGramEdge * tR[s]];
          const double bv = (diag && tR[s] == tC[s]) ? av : cols[ks * kGramStride + kGramEdge * tC[s]];
          acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[s], 0, 0, 0);
        }
      }
    }
  }

  double* const w = a.ws + (static_cast<int64_t>(blockIdx.y) * a.num_chunks + static_cast<int64_t>(blockIdx.x)) * kGramPairs;
#pragma unroll
  for (int s = 0; s < kGramSlots; ++s) {
    if (live[s]) {
#pragma unroll
      for (int v = 0; v < 4; ++v)
        w[(kGramEdge * tR[s] + 4 * v + g) * kGramBlock + kGramEdge * tC[s] + j] = acc[s][v];
    }
  }
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
}

// One lane per (i, j), i <= j: the entry's chunk partials added in ascending chunk order, the result
// mirrored.
__global__ __launch_bounds__(kGramThreads) void gram_reduce_kernel(const double* ws, int32_t num_chunks, int32_t n,
                                                                   double* out, uint32_t* flag) {
  const int idx = static_cast<int>(blockIdx.x) * kGramThreads + static_cast<int>(threadIdx.x);
  if (idx >= n * n) return;
  const int i = idx / n, j = idx % n;
  if (i > j) return;
  const int NB = (n + kGramBlock - 1) / kGramBlock;
  const int bp = gram_block_pair(i / kGramBlock, j / kGramBlock, NB);
  const double* p = ws + static_cast<int64_t>(bp) * num_chunks * kGramPairs + (i % kGramBlock) * kGramBlock + (j % kGramBlock);
  double s = 0.0;
#pragma unroll 8
  for (int c = 0; c < num_chunks; ++c) s += p[static_cast<int64_t>(c) * kGramPairs];
  out[static_cast<int64_t>(i) * n + j] = s;
  out[static_cast<int64_t>(j) * n + i] = s;
  if (s != s) raise_flag(flag, 0);  // 0 * inf or +inf + -inf in some element (or a NaN input, flagged at the load too)
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct GramState {
  Span* d_chunks = nullptr;
  int64_t num_chunks = 0;
  double* ws = nullptr;  // grown lazily to the largest client count seen
  size_t ws_bytes = 0;
  TableRing ring;  // a call's tables: clients, point, history in and out
  ~GramState() {
    ring.release();
    if (d_chunks) (void)hipFree(d_chunks);
    if (ws) (void)hipFree(ws);
  }
};

int32_t ensure_state(const fedavg_robust_view& v, void** slot, GramState** out) {
  if (*slot == nullptr) {
    GramState* st = new GramState();
    int32_t r = span_table(v.seg_numel, v.num_segments, kGramChunk, "Gram launch", "gram chunk table", &st->d_chunks,
                           &st->num_chunks);
    if (r == FEDAVG_OK) r = hip_status("gram chunk table", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<GramState*>(*slot);
  return FEDAVG_OK;
}

// Does a history_out row share a byte with a history_in row or with another history_out row?
bool history_overlaps(const fedavg_robust_view& v, int n, const double* const* hin, double* const* hout) {
  struct Range {
    uintptr_t lo, hi;
    bool out;
  };
  std::vector<Range> r;
  r.reserve(2 * static_cast<size_t>(n) * v.num_segments);
  for (int i = 0; i < n; ++i) {
    for (int t = 0; t < v.num_segments; ++t) {
      const uintptr_t bytes = 8u * static_cast<uintptr_t>(v.seg_numel[t]);
      if (bytes == 0) continue;
      const size_t e = static_cast<size_t>(i) * v.num_segments + t;
      r.push_back({reinterpret_cast<uintptr_t>(hin[e]), reinterpret_cast<uintptr_t>(hin[e]) + bytes, false});
      r.push_back({reinterpret_cast<uintptr_t>(hout[e]), reinterpret_cast<uintptr_t>(hout[e]) + bytes, true});
    }
  }
  std::sort(r.begin(), r.end(), [](const Range& x, const Range& y) { return x.lo < y.lo; });
  uintptr_t any_end = 0, out_end = 0;  // the furthest end of the ranges so far: of all, of the outputs
  for (const Range& x : r) {
    if (x.lo < (x.out ? any_end : out_end)) return true;
    any_end = std::max(any_end, x.hi);
    if (x.out) out_end = std::max(out_end, x.hi);
  }
  return false;
}

template <typename T>
void launch_chunks(bool hist, dim3 grid, hipStream_t s, const GArgs& a) {
  const dim3 block(kGramThreads);
  if (hist) hipLaunchKernelGGL((gram_chunk_kernel<T, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((gram_chunk_kernel<T, false>), grid, block, 0, s, a);
}

}  // namespace

int32_t fedavg_internal_gram_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "gram_chunk") *out = kGramChunk;
  else if (n == "gram_tile") *out = kGramTile;
  else if (n == "gram_block") *out = kGramBlock;
  else if (n == "gram_threads") *out = kGramThreads;
  else if (n == "gram_max_clients") *out = kGramMaxClients;
  else if (n == "gram_ae_f32") *out = Format<float>::N;
  else if (n == "gram_ae_f16") *out = Format<__half>::N;
  else if (n == "gram_ae_bf16") *out = Format<bf16_t>::N;
  else if (n == "gram_ae_f64") *out = Format<double>::N;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_gram_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<GramState*>(state);
}

extern "C" int32_t fedavg_gram_about_point(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                           int32_t num_clients, const double* const* point_ptrs,
                                           const double* const* history_in, double* const* history_out, double* out,
                                           void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_GRAM, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (in_dtype != FEDAVG_F32 && in_dtype != FEDAVG_F16 && in_dtype != FEDAVG_BF16 && in_dtype != FEDAVG_F64)
    return invalid("the Gram matrix reads dense fp32 / fp16 / bf16 / fp64 tensors (no records)");
  if (client_ptrs == nullptr || out == nullptr) return invalid("null client table or output");
  if ((history_in == nullptr) != (history_out == nullptr))
    return invalid("history_in and history_out come together or not at all");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kGramMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the Gram matrix takes at most " +
                   std::to_string(kGramMaxClients));
  if (reinterpret_cast<uintptr_t>(out) % 8 != 0) return invalid("output not aligned to fp64");
  const int T = v.num_segments;
  const size_t elem_bytes = in_dtype == FEDAVG_F64 ? 8 : in_dtype == FEDAVG_F32 ? 4 : 2;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (size_t i = 0; i < entries; ++i) {
    const void* p = client_ptrs[i];
    if (p == nullptr)
      return invalid("client " + std::to_string(i / T) + " lacks segment " + std::to_string(i % T) +
                     ": the Gram matrix compares whole updates");
    if (reinterpret_cast<uintptr_t>(p) % elem_bytes != 0) return invalid("client tensor not aligned to its element size");
  }
  if (point_ptrs != nullptr) {
    for (int t = 0; t < T; ++t) {
      if (point_ptrs[t] == nullptr) return invalid("the point lacks segment " + std::to_string(t));
      if (reinterpret_cast<uintptr_t>(point_ptrs[t]) % 8 != 0) return invalid("point tensor not aligned to fp64");
    }
  }
  const bool hist = history_in != nullptr;
  if (hist) {
    for (size_t i = 0; i < entries; ++i) {
      if (history_in[i] == nullptr || history_out[i] == nullptr)
        return invalid("the history of client " + std::to_string(i / T) + " lacks segment " + std::to_string(i % T));
      if (reinterpret_cast<uintptr_t>(history_in[i]) % 8 != 0 || reinterpret_cast<uintptr_t>(history_out[i]) % 8 != 0)
        return invalid("history tensor not aligned to fp64");
    }
    if (history_overlaps(v, num_clients, history_in, history_out))
      return invalid("a history_out tensor shares storage with a history_in tensor or with another history_out "
                     "tensor: other workgroups read history_in while it is written");
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  GramState* st = nullptr;
  const int32_t re = ensure_state(v, slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  const int NB = (num_clients + kGramBlock - 1) / kGramBlock;
  const int num_bp = NB * (NB + 1) / 2;
  const size_t ws_bytes = sizeof(double) * static_cast<size_t>(num_bp) * static_cast<size_t>(st->num_chunks) * kGramPairs;
  if (st->ws_bytes < ws_bytes) {
    if (st->ws) FEDAVG_TRY_HIP(hipFree(st->ws));  // synchronises with the launches that used it
    st->ws = nullptr;
    st->ws_bytes = 0;
    FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&st->ws), ws_bytes));
    st->ws_bytes = ws_bytes;
  }

  // the call's pointer tables: [n][T] clients, then [T] point, [n][T] history in, [n][T] history out
  const size_t client_bytes = sizeof(void*) * entries;
  const size_t point_bytes = point_ptrs != nullptr ? sizeof(void*) * static_cast<size_t>(T) : 0;
  const size_t bytes = client_bytes + point_bytes + (hist ? 2 * client_bytes : 0);
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.acquire(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, client_ptrs, client_bytes);
  if (point_ptrs != nullptr) std::memcpy(sl.host + client_bytes, point_ptrs, point_bytes);
  if (hist) {
    std::memcpy(sl.host + client_bytes + point_bytes, history_in, client_bytes);
    std::memcpy(sl.host + 2 * client_bytes + point_bytes, history_out, client_bytes);
  }
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  GArgs a;
  a.chunks = st->d_chunks;
  a.ptrs = reinterpret_cast<const void* const*>(sl.dev);
  a.point = point_ptrs != nullptr ? reinterpret_cast<const double* const*>(sl.dev + client_bytes) : nullptr;
  a.hin = hist ? reinterpret_cast<const double* const*>(sl.dev + client_bytes + point_bytes) : nullptr;
  a.hout = hist ? reinterpret_cast<double* const*>(sl.dev + 2 * client_bytes + point_bytes) : nullptr;
  a.ws = st->ws;
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  a.num_chunks = static_cast<int32_t>(st->num_chunks);
  a.pad_ = 0;
  const dim3 grid(static_cast<unsigned>(st->num_chunks), static_cast<unsigned>(num_bp));
  switch (in_dtype) {
    case FEDAVG_F32: launch_chunks<float>(hist, grid, s, a); break;
    case FEDAVG_F16: launch_chunks<__half>(hist, grid, s, a); break;
    case FEDAVG_BF16: launch_chunks<bf16_t>(hist, grid, s, a); break;
    default: launch_chunks<double>(hist, grid, s, a); break;
  }
  FEDAVG_TRY_HIP(hipGetLastError());
  const unsigned cells = static_cast<unsigned>(num_clients) * static_cast<unsigned>(num_clients);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((cells + kGramThreads - 1) / kGramThreads), dim3(kGramThreads), 0, s,
                     st->ws, static_cast<int32_t>(st->num_chunks), num_clients, out, v.d_flag);
  FEDAVG_TRY_HIP(hipGetLastError());
  return st->ring.retire(sl, s);
}
