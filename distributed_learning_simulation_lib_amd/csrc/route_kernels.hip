// route_kernels.hip — gfx950 (MI355X) kernels of the routed row gather (fedavg_route_rows,
// include/fedavg_hip.h): the server half of the reference's graph embedding exchange
// (graph_embedding_algorithm.py:38-59). S workers send row blocks whose rows carry node ids; N
// workers each want a strictly increasing list of node ids and receive, packed at the front of the
// list's own output slot, the ids that somebody sent and those nodes' rows, byte for byte. The
// contract is DESIGN.md §5o and tests/graph_reference.py restates it in numpy.
//
// A routed copy and nothing else: no arithmetic touches a row, so the result is bit-identical to the
// reference's torch.stack by construction. No atomics; four launches on the caller's stream:
//
//   1. route_scatter_kernel: table[src_ids[r]] = r for every sent row r of the concatenation. The
//      table is a dense int32 map node -> concatenated row held by the handle, -1 where empty. An id
//      outside [0, node_space) is not written (and latches error word 2).
//   2. route_rank_kernel, two kinds of workgroup in one launch. The first `id_blocks` re-read the
//      table for every sent row (write-then-verify): table[src_ids[r]] != r means another row wrote
//      the same node, a duplicate (error word 0). The others own one chunk of kRtChunk wanted ids of
//      one list each: a lane looks its ids up (an id outside [0, node_space) is a miss and never
//      reaches the table), the hits of a wave are ranked by ballot and popcount, the waves and the
//      passes of a chunk are combined through LDS, and the hit's source row is stored compacted at
//      the front of the chunk's own range of the workspace; the chunk's hit count goes to
//      chunk_count. The same walk checks that a list is strictly increasing (error word 1).
//   3. route_scan_kernel, again two kinds. One wave per list adds the list's chunk counts up with a
//      wave prefix (the small scan), writes every chunk's base inside the list's slot and the list's
//      out_count. The other workgroups un-scatter: table[src_ids[r]] = -1, so the table is empty
//      again before the call's work on the stream ends, whatever the error words say.
//   4. route_gather_kernel<T>: workgroup (chunk, part) copies its part of the chunk's hit rows as one
//      flat range of T-sized units (T = 16 bytes when row_bytes and every pointer allow it, else the
//      element), so consecutive lanes store consecutive addresses of the packed output. A hit's
//      source pointer is recovered once per hit from the S + 1 row offsets held in LDS (binary
//      search) and kept in LDS for the copy loop. out_ids is written by the part that holds a row's
//      first unit.
//
// Nothing outside [want_off[j], want_off[j] + count_j) of an output is written, nothing outside
// [0, node_space) of the table is touched, and nothing of an earlier call survives in the table.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kRtThreads = 256;                     // lanes per workgroup
constexpr int kRtWaves = kRtThreads / 64;
constexpr int kRtPasses = 2;                        // wanted ids per lane and chunk
constexpr int kRtChunk = kRtThreads * kRtPasses;    // wanted ids per workgroup of the rank walk
constexpr int kRtMaxSources = 1024;
constexpr int64_t kRtMaxNodeSpace = int64_t(1) << 28;  // a 1 GiB table
constexpr int64_t kRtSplitBytes = 64 * 1024;        // bytes one gather workgroup aims at
constexpr int kRtMaxSplit = 64;                     // parts of one chunk's gather

struct RChunk {
  int32_t list;
  int32_t start;  // first wanted id of the chunk, relative to its list
};

struct RArgs {
  int32_t* table;             // [>= node_space], -1 = empty
  int64_t node_space;
  const int64_t* src_ids;     // [R]
  const int64_t* want_ids;    // [B]
  const int32_t* want_off;    // [N + 1]
  const int32_t* chunk_off;   // [N + 1]: list j owns the chunks [chunk_off[j], chunk_off[j + 1])
  const RChunk* chunks;       // [num_chunks]
  int32_t* ws_src;            // [B]: per chunk, the source rows of its hits, compacted
  int32_t* chunk_count;       // [num_chunks]
  int32_t* chunk_base;        // [num_chunks]: hits of the list's earlier chunks
  const void* const* src_ptrs;  // [S]
  const int32_t* row_off;     // [S + 1]
  int64_t row_bytes;
  void* out_rows;
  int64_t* out_ids;
  int32_t* out_count;
  uint32_t* err;              // 0 duplicate sent id, 1 list not increasing, 2 sent id out of range
  int32_t R;
  int32_t N;
  int32_t S;
  int32_t num_chunks;
  int32_t id_blocks;          // workgroups that walk the sent ids in a mixed launch
};

// ---------------------------------------------------------------------------------------
// 1. the map: blockIdx.x * kRtThreads + lane = sent row
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRtThreads) void route_scatter_kernel(RArgs a) {
  const int64_t r = static_cast<int64_t>(blockIdx.x) * kRtThreads + threadIdx.x;
  bool bad = false;
  if (r < a.R) {
    const int64_t id = a.src_ids[r];
    if (id >= 0 && id < a.node_space) a.table[id] = static_cast<int32_t>(r);
    else bad = true;
  }
  if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) raise_flag(a.err, 2);
}

// ---------------------------------------------------------------------------------------
// 2. verify the map (blockIdx.x < id_blocks) and rank the hits (one chunk per other workgroup)
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRtThreads) void route_rank_kernel(RArgs a) {
  __shared__ int32_t wcount[kRtPasses * kRtWaves];
  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63;
  const int wave = t >> 6;
  if (static_cast<int32_t>(blockIdx.x) < a.id_blocks) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * kRtThreads + t;
    bool dup = false;
    if (r < a.R) {
      const int64_t id = a.src_ids[r];
      if (id >= 0 && id < a.node_space) dup = a.table[id] != static_cast<int32_t>(r);
    }
    if (__ballot(dup) != 0ull && lane == 0) raise_flag(a.err, 0);
    return;
  }
  const int32_t c = static_cast<int32_t>(blockIdx.x) - a.id_blocks;
  const RChunk ch = a.chunks[c];
  const int32_t lo = a.want_off[ch.list];
  const int32_t left = a.want_off[ch.list + 1] - lo - ch.start;
  const int32_t n = left < kRtChunk ? left : kRtChunk;
  const int32_t g0 = lo + ch.start;  // the chunk's first wanted id, and its range of ws_src

  int32_t row[kRtPasses];
  int32_t prefix[kRtPasses];
  bool disorder = false;
#pragma unroll
  for (int p = 0; p < kRtPasses; ++p) {
    const int e = p * kRtThreads + t;
    int32_t r = -1;
    if (e < n) {
      const int64_t id = a.want_ids[g0 + e];
      if (ch.start + e > 0) disorder |= id <= a.want_ids[g0 + e - 1];
      if (id >= 0 && id < a.node_space) {
        r = a.table[id];
        if (r >= a.R) r = -1;  // the table holds -1 or a sent row: never trusted past R
      }
    }
    const unsigned long long mask = __ballot(r >= 0);
    row[p] = r;
    prefix[p] = __popcll(mask & ((1ull << lane) - 1ull));
    if (lane == 0) wcount[p * kRtWaves + wave] = __popcll(mask);
  }
  __syncthreads();
  int32_t total = 0;
#pragma unroll
  for (int p = 0; p < kRtPasses; ++p) {
    int32_t base = 0;
#pragma unroll
    for (int q = 0; q < kRtPasses * kRtWaves; ++q) {
      const int32_t v = wcount[q];
      if (q < p * kRtWaves + wave) base += v;
      if (p == 0) total += v;
    }
    if (row[p] >= 0) a.ws_src[g0 + base + prefix[p]] = row[p];
  }
  if (t == 0) a.chunk_count[c] = total;
  if (__ballot(disorder) != 0ull && lane == 0) raise_flag(a.err, 1);
}

// ---------------------------------------------------------------------------------------
// 3. one wave per list: the chunks' bases and the list's count; the other workgroups
//    (blockIdx.x >= list_blocks) put the table back to empty
// ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(kRtThreads) void route_scan_kernel(RArgs a, int32_t list_blocks) {
  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63;
  if (static_cast<int32_t>(blockIdx.x) >= list_blocks) {
    const int64_t r = static_cast<int64_t>(static_cast<int32_t>(blockIdx.x) - list_blocks) * kRtThreads + t;
    if (r < a.R) {
      const int64_t id = a.src_ids[r];
      if (id >= 0 && id < a.node_space) a.table[id] = -1;
    }
    return;
  }
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kRtWaves + (t >> 6);
  if (j >= a.N) return;  // the whole wave
  const int32_t c0 = a.chunk_off[j], c1 = a.chunk_off[j + 1];
  int32_t running = 0;
  for (int32_t i = c0; i < c1; i += 64) {
    const int32_t c = i + lane;
    const int32_t v = c < c1 ? a.chunk_count[c] : 0;
    int32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int32_t o = __shfl_up(incl, d, 64);
      if (lane >= d) incl += o;
    }
    if (c < c1) a.chunk_base[c] = running + incl - v;
    running += __shfl(incl, 63, 64);
  }
  if (lane == 0) a.out_count[j] = running;
}

// ---------------------------------------------------------------------------------------
// 4. the rows: blockIdx.x = chunk, blockIdx.y = part of the chunk's flat range of units
// ---------------------------------------------------------------------------------------
template <typename T, typename I>
__device__ __forceinline__ void rt_copy(const uint64_t* sptr, T FEDAVG_AS_GLOBAL* dst, I u0, I u1, I upr, int t) {
  // dst is the chunk's first output row; unit u of the flat range is unit u % upr of hit u / upr
  constexpr int U = 4;
  I u = u0 + static_cast<I>(t);
  for (; u + static_cast<I>((U - 1) * kRtThreads) < u1; u += static_cast<I>(U * kRtThreads)) {
    T v[U];
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const I uu = u + static_cast<I>(q * kRtThreads);
      const I k = uu / upr;
      v[q] = ((const T FEDAVG_AS_GLOBAL*)sptr[k])[uu - k * upr];
    }
#pragma unroll
    for (int q = 0; q < U; ++q) dst[u + static_cast<I>(q * kRtThreads)] = v[q];
  }
  for (; u < u1; u += static_cast<I>(kRtThreads)) {
    const I k = u / upr;
    dst[u] = ((const T FEDAVG_AS_GLOBAL*)sptr[k])[u - k * upr];
  }
}

template <typename T>
__global__ __launch_bounds__(kRtThreads) void route_gather_kernel(RArgs a) {
  __shared__ int32_t soff[kRtMaxSources + 1];
  __shared__ uint64_t sptr[kRtChunk];  // address of hit k's source row
  const int32_t c = static_cast<int32_t>(blockIdx.x);
  const int32_t cnt = a.chunk_count[c];
  if (cnt <= 0) return;
  const int t = static_cast<int>(threadIdx.x);
  const int64_t upr = a.row_bytes / static_cast<int64_t>(sizeof(T));  // units per row
  const int64_t total = static_cast<int64_t>(cnt) * upr;
  const int64_t per = (total + gridDim.y - 1) / gridDim.y;
  const int64_t u0 = static_cast<int64_t>(blockIdx.y) * per;
  const int64_t u1 = u0 + per < total ? u0 + per : total;
  if (u0 >= u1) return;
  const int32_t k0 = static_cast<int32_t>(u0 / upr);
  const int32_t k1 = static_cast<int32_t>((u1 - 1) / upr) + 1;  // <= cnt <= kRtChunk

  const RChunk ch = a.chunks[c];
  const int32_t lo = a.want_off[ch.list];
  const int32_t g0 = lo + ch.start;
  const int64_t dst0 = static_cast<int64_t>(lo) + a.chunk_base[c];  // the chunk's first output row
  const int S = a.S;
  for (int i = t; i <= S; i += kRtThreads) soff[i] = a.row_off[i];
  __syncthreads();
  for (int32_t k = k0 + t; k < k1; k += kRtThreads) {
    const int32_t r = a.ws_src[g0 + k];
    // the last source s with row_off[s] <= r: sources without rows share an offset with their successor
    int s0 = 0, s1 = S;
    while (s1 - s0 > 1) {
      const int mid = (s0 + s1) >> 1;
      if (soff[mid] <= r) s0 = mid;
      else s1 = mid;
    }
    sptr[k] = reinterpret_cast<uint64_t>(a.src_ptrs[s0]) +
              static_cast<uint64_t>(r - soff[s0]) * static_cast<uint64_t>(a.row_bytes);
    // the part that holds the row's first unit names it
    if (static_cast<int64_t>(k) * upr >= u0) a.out_ids[dst0 + k] = a.src_ids[r];
  }
  __syncthreads();
  T FEDAVG_AS_GLOBAL* const dst = (T FEDAVG_AS_GLOBAL*)a.out_rows + dst0 * upr;
  if (total <= 0x7fffffffll)
    rt_copy<T, uint32_t>(sptr, dst, static_cast<uint32_t>(u0), static_cast<uint32_t>(u1), static_cast<uint32_t>(upr), t);
  else
    rt_copy<T, int64_t>(sptr, dst, u0, u1, upr, t);
}

}  // namespace

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------

struct fedavg_route {
  int32_t device = 0;
  int32_t* d_table = nullptr;  // [table_cap], -1 everywhere between calls
  int64_t table_cap = 0;
  bool dirty = false;          // a call scattered and could not enqueue its un-scatter
  uint32_t* d_err = nullptr;   // 3 words, latched by the kernels, cleared by fedavg_route_errors
  char* d_ws = nullptr;        // ws_src, chunk_count, chunk_base of the call in flight
  size_t ws_cap = 0;
  TableRing ring;
};

int32_t fedavg_internal_route_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "route_chunk") *out = kRtChunk;
  else if (n == "route_threads") *out = kRtThreads;
  else if (n == "route_max_sources") *out = kRtMaxSources;
  else if (n == "route_max_node_space") *out = kRtMaxNodeSpace;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_route_destroy(fedavg_route* p) {
  if (p == nullptr) return FEDAVG_OK;
  (void)hipSetDevice(p->device);
  (void)hipDeviceSynchronize();
  p->ring.release();
  if (p->d_table) (void)hipFree(p->d_table);
  if (p->d_err) (void)hipFree(p->d_err);
  if (p->d_ws) (void)hipFree(p->d_ws);
  delete p;
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_route_create(fedavg_route** out, int32_t device) {
  if (out == nullptr) return invalid("null out");
  *out = nullptr;
  if (device < 0) return invalid("bad device");
  FEDAVG_TRY_HIP(hipSetDevice(device));
  fedavg_route* p = new fedavg_route();
  p->device = device;
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&p->d_err), 3 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipMemset(p->d_err, 0, 3 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipDeviceSynchronize();  // the words are clear before any stream's first call
  if (e == hipSuccess) e = p->ring.create();
  if (e != hipSuccess) {
    fedavg_route_destroy(p);
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("route state: ") + hipGetErrorString(e)).c_str());
  }
  *out = p;
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_route_rows(fedavg_route* p, const void* const* src_ptrs, const int64_t* src_rows,
                                     int32_t num_sources, int64_t row_bytes, int32_t elem_bytes,
                                     const int64_t* src_ids, const int64_t* want_ids, const int64_t* want_off,
                                     int32_t num_lists, int64_t node_space, void* out_rows, int64_t* out_ids,
                                     int32_t* out_count, void* stream) {
  if (p == nullptr) return invalid("null route handle");
  const int S = num_sources, N = num_lists;
  if (S < 0 || S > kRtMaxSources)
    return invalid(std::to_string(S) + " sources: a routing takes 0 to " + std::to_string(kRtMaxSources));
  if (N < 1) return invalid("no want list");
  if (S > 0 && (src_ptrs == nullptr || src_rows == nullptr)) return invalid("null source table");
  if (want_off == nullptr || out_count == nullptr) return invalid("null want offsets or out_count");
  if (elem_bytes != 1 && elem_bytes != 2 && elem_bytes != 4 && elem_bytes != 8)
    return invalid("the element size is 1, 2, 4 or 8 bytes");
  if (row_bytes < 1 || row_bytes % elem_bytes != 0)
    return invalid("row_bytes must be a positive multiple of the element size");
  if (node_space < 0 || node_space > kRtMaxNodeSpace)
    return invalid("node_space outside [0, 2^28]");
  const uintptr_t eb = static_cast<uintptr_t>(elem_bytes);
  int64_t R = 0;
  bool vec = row_bytes % 16 == 0 && !misaligned(out_rows, 16);
  for (int s = 0; s < S; ++s) {
    if (src_rows[s] < 0) return invalid("source " + std::to_string(s) + ": negative row count");
    R += src_rows[s];
    if (R > 0x7fffffffll) return invalid("2^31 or more sent rows");
    if (src_rows[s] > 0 && src_ptrs[s] == nullptr) return invalid("source " + std::to_string(s) + ": null rows");
    if (misaligned(src_ptrs[s], eb)) return invalid("source " + std::to_string(s) + ": rows not aligned to the element");
    if (src_rows[s] > 0 && misaligned(src_ptrs[s], 16)) vec = false;
  }
  if (want_off[0] != 0) return invalid("want_off must start at 0");
  for (int j = 0; j < N; ++j) {
    if (want_off[j + 1] < want_off[j]) return invalid("want_off decreases at list " + std::to_string(j));
    if (want_off[j + 1] > 0x7fffffffll) return invalid("2^31 or more wanted ids");
  }
  const int64_t B = want_off[N];
  if (R > 0 && src_ids == nullptr) return invalid("null src_ids");
  if (B > 0 && (want_ids == nullptr || out_rows == nullptr || out_ids == nullptr))
    return invalid("null want_ids, out_rows or out_ids");
  if (misaligned(src_ids, 8) || misaligned(want_ids, 8) || misaligned(out_ids, 8))
    return invalid("src_ids, want_ids and out_ids are int64 arrays: not aligned");
  if (misaligned(out_count, 4)) return invalid("out_count not aligned to int32");
  if (misaligned(out_rows, eb)) return invalid("out_rows not aligned to the element");

  // the rank walk's chunks: list by list, kRtChunk wanted ids each (a list's last chunk is shorter)
  std::vector<int32_t> chunk_off(static_cast<size_t>(N) + 1);
  int64_t C = 0;
  for (int j = 0; j < N; ++j) {
    chunk_off[j] = static_cast<int32_t>(C);
    C += (want_off[j + 1] - want_off[j] + kRtChunk - 1) / kRtChunk;
  }
  if (C > 0x7fffffffll) return invalid("too many want lists");
  chunk_off[N] = static_cast<int32_t>(C);

  FEDAVG_TRY_HIP(hipSetDevice(p->device));
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the table: grown on demand, empty (-1) between calls
  if (p->table_cap < node_space && R > 0) {
    int64_t cap = p->table_cap * 2 > node_space ? p->table_cap * 2 : node_space;
    if (cap < 4096) cap = 4096;
    if (cap > kRtMaxNodeSpace) cap = kRtMaxNodeSpace;
    if (p->d_table) {
      FEDAVG_TRY_HIP(hipStreamSynchronize(s));
      FEDAVG_TRY_HIP(hipFree(p->d_table));
      p->d_table = nullptr;
      p->table_cap = 0;
    }
    FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_table), sizeof(int32_t) * static_cast<size_t>(cap)));
    p->table_cap = cap;
    p->dirty = true;
  }
  if (p->dirty && p->d_table != nullptr) {
    FEDAVG_TRY_HIP(hipMemsetAsync(p->d_table, 0xff, sizeof(int32_t) * static_cast<size_t>(p->table_cap), s));
    p->dirty = false;
  }

  // the workspace of the call in flight: ws_src[B], chunk_count[C], chunk_base[C]
  const size_t ws_bytes = sizeof(int32_t) * (static_cast<size_t>(B) + 2 * static_cast<size_t>(C));
  if (p->ws_cap < ws_bytes) {
    if (p->d_ws) {
      FEDAVG_TRY_HIP(hipStreamSynchronize(s));
      FEDAVG_TRY_HIP(hipFree(p->d_ws));
      p->d_ws = nullptr;
      p->ws_cap = 0;
    }
    const size_t cap = ws_bytes * 2 < 64 * 1024 ? 64 * 1024 : ws_bytes * 2;
    FEDAVG_TRY_HIP(hipMalloc(reinterpret_cast<void**>(&p->d_ws), cap));
    p->ws_cap = cap;
  }

  // the call's tables: [S] source pointers, [C] chunks, [S + 1] row offsets, [N + 1] want offsets,
  // [N + 1] chunk offsets
  const size_t ptr_bytes = sizeof(void*) * static_cast<size_t>(S);
  const size_t chunk_bytes = sizeof(RChunk) * static_cast<size_t>(C);
  const size_t roff_bytes = sizeof(int32_t) * (static_cast<size_t>(S) + 1);
  const size_t list_bytes = sizeof(int32_t) * (static_cast<size_t>(N) + 1);
  const size_t o_chunks = ptr_bytes, o_roff = o_chunks + chunk_bytes, o_woff = o_roff + roff_bytes,
               o_coff = o_woff + list_bytes, bytes = o_coff + list_bytes;
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(p->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  if (S > 0) std::memcpy(sl.host, src_ptrs, ptr_bytes);
  RChunk* const h_chunks = reinterpret_cast<RChunk*>(sl.host + o_chunks);
  int32_t* const h_roff = reinterpret_cast<int32_t*>(sl.host + o_roff);
  int32_t* const h_woff = reinterpret_cast<int32_t*>(sl.host + o_woff);
  h_roff[0] = 0;
  for (int i = 0; i < S; ++i) h_roff[i + 1] = h_roff[i] + static_cast<int32_t>(src_rows[i]);
  for (int j = 0; j <= N; ++j) h_woff[j] = static_cast<int32_t>(want_off[j]);
  for (int j = 0; j < N; ++j) {
    const int32_t len = h_woff[j + 1] - h_woff[j];
    RChunk* q = h_chunks + chunk_off[j];
    for (int32_t st = 0; st < len; st += kRtChunk) *q++ = RChunk{j, st};
  }
  std::memcpy(sl.host + o_coff, chunk_off.data(), list_bytes);
  FEDAVG_TRY(p->ring.submit(sl, bytes, s));

  RArgs a;
  a.table = p->d_table;
  a.node_space = R > 0 ? node_space : 0;  // nothing sent: every wanted id misses before the table
  a.src_ids = src_ids;
  a.want_ids = want_ids;
  a.want_off = reinterpret_cast<const int32_t*>(sl.dev + o_woff);
  a.chunk_off = reinterpret_cast<const int32_t*>(sl.dev + o_coff);
  a.chunks = reinterpret_cast<const RChunk*>(sl.dev + o_chunks);
  a.ws_src = reinterpret_cast<int32_t*>(p->d_ws);
  a.chunk_count = a.ws_src + B;
  a.chunk_base = a.chunk_count + C;
  a.src_ptrs = reinterpret_cast<const void* const*>(sl.dev);
  a.row_off = reinterpret_cast<const int32_t*>(sl.dev + o_roff);
  a.row_bytes = row_bytes;
  a.out_rows = out_rows;
  a.out_ids = out_ids;
  a.out_count = out_count;
  a.err = p->d_err;
  a.R = static_cast<int32_t>(R);
  a.N = N;
  a.S = S;
  a.num_chunks = static_cast<int32_t>(C);
  a.id_blocks = static_cast<int32_t>((R + kRtThreads - 1) / kRtThreads);

  const dim3 block(kRtThreads);
  hipError_t e = hipSuccess;
  bool scattered = false;
  if (a.id_blocks > 0) {
    p->dirty = true;  // until the un-scatter is on the stream
    hipLaunchKernelGGL(route_scatter_kernel, dim3(static_cast<unsigned>(a.id_blocks)), block, 0, s, a);
    e = hipGetLastError();
    scattered = e == hipSuccess;
    if (!scattered) p->dirty = false;  // nothing was written
  }
  if (e == hipSuccess && a.id_blocks + C > 0) {
    hipLaunchKernelGGL(route_rank_kernel, dim3(static_cast<unsigned>(a.id_blocks + C)), block, 0, s, a);
    e = hipGetLastError();
  }
  // the un-scatter goes out whatever became of the rank launch
  const int32_t list_blocks = e == hipSuccess ? (N + kRtWaves - 1) / kRtWaves : 0;
  if (list_blocks + (scattered ? a.id_blocks : 0) > 0) {
    hipLaunchKernelGGL(route_scan_kernel, dim3(static_cast<unsigned>(list_blocks + (scattered ? a.id_blocks : 0))),
                       block, 0, s, a, list_blocks);
    const hipError_t eu = hipGetLastError();
    if (eu == hipSuccess) p->dirty = false;
    if (e == hipSuccess) e = eu;
  }
  if (e == hipSuccess && C > 0 && R > 0) {
    // parts per chunk: a full chunk of hits cut into pieces of about kRtSplitBytes
    int64_t split = (static_cast<int64_t>(kRtChunk) * row_bytes + kRtSplitBytes - 1) / kRtSplitBytes;
    split = split < 1 ? 1 : split > kRtMaxSplit ? kRtMaxSplit : split;
    const dim3 grid(static_cast<unsigned>(C), static_cast<unsigned>(split));
    if (vec) hipLaunchKernelGGL(route_gather_kernel<u32x4>, grid, block, 0, s, a);
    else if (elem_bytes == 8) hipLaunchKernelGGL(route_gather_kernel<uint64_t>, grid, block, 0, s, a);
    else if (elem_bytes == 4) hipLaunchKernelGGL(route_gather_kernel<uint32_t>, grid, block, 0, s, a);
    else if (elem_bytes == 2) hipLaunchKernelGGL(route_gather_kernel<uint16_t>, grid, block, 0, s, a);
    else hipLaunchKernelGGL(route_gather_kernel<uint8_t>, grid, block, 0, s, a);
    e = hipGetLastError();
  }
  const hipError_t er = p->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("route launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_route_errors(fedavg_route* p, void* stream, int32_t* out) {
  if (p == nullptr || out == nullptr) return invalid("null route handle or out");
  *out = 0;
  FEDAVG_TRY_HIP(hipSetDevice(p->device));
  hipStream_t s = static_cast<hipStream_t>(stream);
  FEDAVG_TRY_HIP(hipStreamSynchronize(s));
  uint32_t words[3] = {0, 0, 0};
  FEDAVG_TRY_HIP(hipMemcpy(words, p->d_err, sizeof(words), hipMemcpyDeviceToHost));
  if ((words[0] | words[1] | words[2]) != 0) {  // reported once: the handle stays usable
    FEDAVG_TRY_HIP(hipMemsetAsync(p->d_err, 0, sizeof(words), s));
    FEDAVG_TRY_HIP(hipStreamSynchronize(s));
  }
  *out = (words[0] ? 1 : 0) | (words[1] ? 2 : 0) | (words[2] ? 4 : 0);
  return FEDAVG_OK;
}
