// lowrank_kernels.hip — gfx950 (MI355X) kernel of FedAvg over low-rank deltas
// (fedavg_lowrank_aggregate_delta, include/fedavg_hip.h): a client sends a weight matrix's delta as
// two thin factors, D = L R with L [m x r] and R [r x n] (the structured updates of Konecny et al.
// 2016, the PowerSGD compressor of Vogels et al. 2019). Not an algorithm of the reference: the
// contract is DESIGN.md §5aa and tests/lowrank_reference.py restates it in numpy.
//
//   a_c[i][j] = fl64(w_c * L_c[i][j])                     the factor converted exactly, one rounding
//   S[i][e]   = sum over c, j of a_c[i][j] * R_c[j][e]    summed by v_mfma_f64_16x16x4_f64
//   out[i][e] = fl(b[i][e] + fl(S[i][e] / W))
// The products are fused into the sum; inside one instruction the order is the hardware's, across
// instructions it is ascending k = c * r + j. Per tensor the round is one [m x K] [K x n] product
// with K = N r: a grouped GEMM with a huge M x N, a small K and many tensors of different shapes,
// the opposite of gram_kernels.hip.
//
// Work split:
//   * The host cuts every tensor of the layout into output tiles of kLrTM x kLrTN = 64 x 64 and
//     uploads one list (LrTile: segment, row and column origin, live extents, n, r). It is rebuilt
//     only when the rows or ranks of a call differ from the call before. One launch,
//     grid = tiles, whatever the number of tensors.
//   * A 256-lane workgroup owns one tile. Wave w owns the strip of the four 16 x 16
//     matrix-instruction tiles of the rows [16 w, 16 w + 16): 4 accumulators of 4 doubles per lane,
//     in registers for the whole K loop. A wave whose strip lies past the tile's last row, and a
//     tile column past its last column, issues no matrix instruction.
//   * K is walked in steps of kLrKStep = 16 slots = 4 matrix instructions per 16 x 16 tile;
//     instruction ks of a step contracts the slots 4 ks .. 4 ks + 3, so k ascends across
//     instructions.
//   * Rows past m, columns past n and slots past K stage +0.0 on BOTH operands: a padding slot is
//     0 * 0, and the 0 * inf of a padding row or column lands in an element that is never stored
//     or looked at.
// Data movement:
//   * Per step the A panel (a_c rows, [slot][row]) and the B panel (R_c columns, [slot][column])
//     are parked in LDS as fp64; the conversion and the one weight multiplication happen there.
//   * A: wave q stages the slots 4 q .. 4 q + 3 of the step, lane i the tile row i, so the client
//     and j of a slot, its pointer and its weight are wave-uniform (scalar loads). Where r % 4 == 0
//     the four slots are four consecutive elements of one client's row: one load of 4 elements
//     (16 bytes for fp32, 2 x 16 for fp64, 8 for fp16 / bf16) where the address allows, and
//     consecutive lanes read consecutive rows, that is consecutive memory. Otherwise guarded
//     element loads.
//   * B: a lane loads one 16-byte non-temporal vector of one slot's row of R_c (consecutive lanes:
//     consecutive vectors) where the address is 16-byte aligned and the vector ends inside the tile
//     and the tensor, and guarded elements otherwise.
//   * Two LDS buffers per panel: the global loads of step s + 1 are issued before the matrix
//     instructions of step s, converted and parked in the other buffer after them; one barrier per
//     step.
//   * Row stride kLrStride = 80 doubles. The matrix instruction takes A[i][k] from lane 16 k + i and
//     B[k][j] from lane 16 k + j, so a half-wave reads 16 consecutive doubles of the two staged rows
//     4 ks + g, 4 ks + g + 1: 80 = 16 mod 32, so the two runs sit 16 double-wide banks apart and
//     cover all 32 once. The A staging writes of one instruction are 64 consecutive doubles of one
//     row; the B staging writes of 16 (fp32), 32 (fp64) or 8 (2-byte) consecutive lanes are one row
//     of 64 consecutive doubles and the next row starts 16 banks further on.
// Epilogue: D[i][j] comes back in register v of lane l with i = 4 v + l / 16, j = l % 16, so for one
// register the 16 lanes of a quarter-wave hold 16 consecutive columns of one row: the base loads
// (issued before the K loop) and the result stores are 128-byte runs (64 for fp32 out). Vector
// stores, no atomics, nothing outside the outputs is written.
// Flags: input NaN at the load (a factor, the base), accumulator NaN for a NaN S of a live element
// (0 * inf, inf - inf), result NaN for a NaN output.
// Determinism: the result depends on the layout, the client order and the rank alone: a tile's K
// loop is one wave's, in ascending k; no CU count, no timing.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kLrThreads = 256;  // lanes per workgroup
constexpr int kLrTM = 64;        // rows of an output tile
constexpr int kLrTN = 64;        // columns of an output tile
constexpr int kLrEdge = 16;      // edge of a matrix-instruction tile
constexpr int kLrK = 4;          // slots one matrix instruction contracts
constexpr int kLrKStep = 16;     // slots staged in LDS per step
constexpr int kLrMaxRank = FEDAVG_LOWRANK_MAX_RANK;
constexpr int kLrMaxClients = FEDAVG_POINT_MAX_CLIENTS;
constexpr int kLrWaves = kLrThreads / 64;
constexpr int kLrColTiles = kLrTN / kLrEdge;  // accumulators of a wave
constexpr int kLrInstr = kLrKStep / kLrK;     // matrix instructions per 16 x 16 tile and step
// doubles per staged slot row: 64 + 16. 80 = 16 mod 32: consecutive rows sit 16 double-wide banks apart
constexpr int kLrStride = kLrTN + 16;
static_assert(kLrTM == kLrWaves * kLrEdge, "wave w owns the tile rows [16 w, 16 w + 16)");
static_assert(kLrTM == 64 && kLrKStep == kLrWaves * kLrK, "A staging: lane = row, wave = slot quad");
static_assert(kLrTM <= kLrTN + 16 && kLrK * 16 == 64, "one stride for both panels; one k-slot per 16 lanes");

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// One output tile. 32 bytes.
struct LrTile {
  int32_t seg;
  int32_t r;     // the tensor's rank
  int32_t row0;  // origin
  int32_t col0;
  int32_t rows;  // live extents: min(64, m - row0), min(64, n - col0)
  int32_t cols;
  int64_t n;     // the tensor's column count: the row stride of R_c, the base and the output
};

struct LrArgs {
  const LrTile* tiles;
  const void* const* left;    // [n][num_segments]: L_c, [m x r] row-major
  const void* const* right;   // [n][num_segments]: R_c, [r x n] row-major
  const double* const* base;  // [num_segments]
  void* const* outs;          // [num_segments]
  const double* w;            // [n]
  double divisor;
  uint32_t* flag;             // the context's NaN words (0 acc, 1 result, 2 input)
  int32_t num_segments;
  int32_t n;
};

// One element's bits, zero-extended, and their exact fp64 value.
template <typename T>
using LrRaw = std::conditional_t<sizeof(T) == 8, uint64_t, uint32_t>;

template <typename T>
__device__ __forceinline__ LrRaw<T> lr_load(const void* base, int64_t e) {
  if constexpr (sizeof(T) == 2) return ((const uint16_t FEDAVG_AS_GLOBAL*)base)[e];
  else if constexpr (sizeof(T) == 4) return ((const uint32_t FEDAVG_AS_GLOBAL*)base)[e];
  else return ((const uint64_t FEDAVG_AS_GLOBAL*)base)[e];
}

template <typename T>
__device__ __forceinline__ double lr_widen(LrRaw<T> bits) {
  if constexpr (std::is_same_v<T, double>) return __longlong_as_double(static_cast<long long>(bits));
  else if constexpr (std::is_same_v<T, float>) return static_cast<double>(__uint_as_float(bits));
  else if constexpr (std::is_same_v<T, __half>)
    return static_cast<double>(__half2float(__ushort_as_half(static_cast<unsigned short>(bits))));
  else return static_cast<double>(__uint_as_float(bits << 16));
}

// ---------------------------------------------------------------------------------------
// the fold: blockIdx.x = tile
// ---------------------------------------------------------------------------------------
// Told to aim for 4 workgroups on a CU (the LDS allows it) the compiler keeps the kernel within 128
// registers with no scratch; left alone it spends 231 on hoisted address arithmetic.
template <typename T, typename O>
__global__ __launch_bounds__(kLrThreads) __attribute__((amdgpu_waves_per_eu(4, 4)))
void lowrank_fold_kernel(LrArgs a) {
  using F = Format<T>;
  constexpr int N = F::N;
  constexpr int kVecs = kLrTN / N;                                 // 16-byte vectors per slot row of the B panel
  constexpr int kBTotal = kLrKStep * kVecs;                        // vectors of the B panel
  constexpr int kBLoads = (kBTotal + kLrThreads - 1) / kLrThreads;  // per lane: 1 (fp32, 2-byte: half the lanes), 2 (fp64)
  constexpr uintptr_t kAMask = (4 * sizeof(T) < 16 ? 4 * sizeof(T) : 16) - 1;  // alignment of the 4-element A load
  static_assert(kLrTN % N == 0, "whole vectors per row");

  __shared__ __attribute__((aligned(16))) double sA[2][kLrKStep * kLrStride];
  __shared__ __attribute__((aligned(16))) double sB[2][kLrKStep * kLrStride];

  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int g = lane >> 4, j16 = lane & 15;  // the lane's k-slot of an instruction and its row / column of a 16 x 16 tile
  const LrTile FEDAVG_AS_CONST* tp = (const LrTile FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg, r = tp->r, row0 = tp->row0, col0 = tp->col0, rows = tp->rows, cols = tp->cols;
  const int64_t n = tp->n;
  const int T_ = a.num_segments;
  const int K = a.n * r;  // <= 1024 * 16
  const int steps = (K + kLrKStep - 1) / kLrKStep;
  const bool wave_live = kLrEdge * wave < rows;
  bool nan_in = false;

  // the lane's base values: element (16 wave + 4 v + g, 16 c + j16) of the tile, loaded up front
  double bv[kLrColTiles][4];
  const double FEDAVG_AS_GLOBAL* const pb = (const double FEDAVG_AS_GLOBAL*)a.base[seg];
#pragma unroll
  for (int c = 0; c < kLrColTiles; ++c) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = kLrEdge * wave + 4 * v + g, col = kLrEdge * c + j16;
      const bool live = row < rows && col < cols;
      bv[c][v] = live ? pb[static_cast<int64_t>(row0 + row) * n + (col0 + col)] : 0.0;
    }
  }

  // what a step's loads leave in registers until the step before has been multiplied
  LrRaw<T> araw[kLrK];
  double aw[kLrK];
  bool avec = false;  // 2-byte factors: araw[0], araw[1] hold the four elements packed
  u32x4 braw[kBLoads];

  auto fetch = [&](int step) __attribute__((always_inline)) {
    // A: wave `wave` stages the slots kb .. kb + 3, lane i the tile row i
    const int kb = step * kLrKStep + kLrK * wave;
    avec = false;
#pragma unroll
    for (int u = 0; u < kLrK; ++u) {
      araw[u] = 0;
      aw[u] = kb + u < K ? a.w[(kb + u) / r] : 0.0;
    }
    if (lane < rows && kb < K) {
      if ((r & 3) == 0) {  // kb % 4 == 0: the four slots are the elements j .. j + 3 of client c's row
        const int c = kb / r, j = kb - c * r;
        const T* const p = static_cast<const T*>(a.left[static_cast<int64_t>(c) * T_ + seg]) +
                           (static_cast<int64_t>(row0 + lane) * r + j);
        if ((reinterpret_cast<uintptr_t>(p) & kAMask) == 0) {
          avec = true;
          if constexpr (sizeof(T) == 4) {
            const u32x4 q = __builtin_nontemporal_load((const u32x4 FEDAVG_AS_GLOBAL*)p);
#pragma unroll
            for (int u = 0; u < kLrK; ++u) araw[u] = q[u];
          } else if constexpr (sizeof(T) == 8) {
            const u32x4 q0 = __builtin_nontemporal_load((const u32x4 FEDAVG_AS_GLOBAL*)p);
            const u32x4 q1 = __builtin_nontemporal_load((const u32x4 FEDAVG_AS_GLOBAL*)p + 1);
            araw[0] = static_cast<uint64_t>(q0[0]) | (static_cast<uint64_t>(q0[1]) << 32);
            araw[1] = static_cast<uint64_t>(q0[2]) | (static_cast<uint64_t>(q0[3]) << 32);
            araw[2] = static_cast<uint64_t>(q1[0]) | (static_cast<uint64_t>(q1[1]) << 32);
            araw[3] = static_cast<uint64_t>(q1[2]) | (static_cast<uint64_t>(q1[3]) << 32);
          } else {
            const u32x2 q = __builtin_nontemporal_load((const u32x2 FEDAVG_AS_GLOBAL*)p);
            araw[0] = q[0];
            araw[1] = q[1];
          }
        }
      }
      if (!avec) {
#pragma unroll
        for (int u = 0; u < kLrK; ++u) {
          const int k = kb + u;
          if (k < K) {  // wave-uniform
            const int c = k / r, j = k - c * r;
            araw[u] = lr_load<T>(a.left[static_cast<int64_t>(c) * T_ + seg], static_cast<int64_t>(row0 + lane) * r + j);
          }
        }
      }
    }
    // B: vector idx of the panel is vector idx % kVecs of slot idx / kVecs
#pragma unroll
    for (int q = 0; q < kBLoads; ++q) {
      const int idx = t + q * kLrThreads;
      u32x4 raw = {0u, 0u, 0u, 0u};
      if (idx < kBTotal) {
        const int k = step * kLrKStep + idx / kVecs, v = idx % kVecs;
        const int have = cols - v * N;
        if (k < K && have > 0) {
          const int c = k / r, j = k - c * r;
          const void* const p = a.right[static_cast<int64_t>(c) * T_ + seg];
          const int64_t e = static_cast<int64_t>(j) * n + (col0 + v * N);
          const T* const pe = static_cast<const T*>(p) + e;
          if (have >= N && (reinterpret_cast<uintptr_t>(pe) & 15u) == 0)
            raw = __builtin_nontemporal_load((const u32x4 FEDAVG_AS_GLOBAL*)pe);
          else
            raw = load_guarded<T>(p, e, have);
        }
      }
      braw[q] = raw;
    }
  };

  // converts what fetch(step) left and parks it in buffer `buf`
  auto park = [&](int step, int buf) __attribute__((always_inline)) {
    const int kb = step * kLrKStep + kLrK * wave;
#pragma unroll
    for (int u = 0; u < kLrK; ++u) {
      double x = 0.0;  // a row past m or a slot past K: +0.0, not w * 0
      if (lane < rows && kb + u < K) {
        LrRaw<T> bits = araw[u];
        if constexpr (sizeof(T) == 2) {
          if (avec) bits = (araw[u / 2] >> (16 * (u % 2))) & 0xffffu;
        }
        const double v = lr_widen<T>(bits);
        nan_in |= v != v;
        x = aw[u] * v;
      }
      sA[buf][(kLrK * wave + u) * kLrStride + lane] = x;
    }
#pragma unroll
    for (int q = 0; q < kBLoads; ++q) {
      const int idx = t + q * kLrThreads;
      if (idx < kBTotal) {
        double* const dst = sB[buf] + (idx / kVecs) * kLrStride + (idx % kVecs) * N;
#pragma unroll
        for (int i = 0; i < N; i += 2) {  // zero bits (a column past n, a slot past K) are +0.0
          const double x0 = F::value(braw[q], i), x1 = F::value(braw[q], i + 1);
          nan_in |= x0 != x0 || x1 != x1;
          *reinterpret_cast<f64x2*>(dst + i) = f64x2{x0, x1};
        }
      }
    }
  };

  f64x4 acc[kLrColTiles];
#pragma unroll
  for (int c = 0; c < kLrColTiles; ++c) acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};

  fetch(0);
  park(0, 0);
  __syncthreads();
#pragma unroll 1
  for (int step = 0; step < steps; ++step) {
    const int cur = step & 1;
    const bool more = step + 1 < steps;
    if (more) fetch(step + 1);  // in flight while this step is multiplied
    if (wave_live) {
      const double* const pa = sA[cur] + g * kLrStride + kLrEdge * wave + j16;
      const double* const pc = sB[cur] + g * kLrStride + j16;
#pragma unroll
      for (int ks = 0; ks < kLrInstr; ++ks) {
        const double av = pa[kLrK * ks * kLrStride];
#pragma unroll
        for (int c = 0; c < kLrColTiles; ++c) {
          if (kLrEdge * c < cols) {  // wave-uniform
            const double cv = pc[kLrK * ks * kLrStride + kLrEdge * c];
            acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, cv, acc[c], 0, 0, 0);
          }
        }
      }
    }
    // the other buffer was last read in step - 1, and every wave has passed that step's barrier
    if (more) park(step + 1, cur ^ 1);
    __syncthreads();
  }

  // out = b + S / W
  bool nan_acc = false, nan_out = false;
  O FEDAVG_AS_GLOBAL* const po = (O FEDAVG_AS_GLOBAL*)a.outs[seg];
  const double divisor = a.divisor;
#pragma unroll
  for (int c = 0; c < kLrColTiles; ++c) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = kLrEdge * wave + 4 * v + g, col = kLrEdge * c + j16;
      if (row < rows && col < cols) {
        const double s = acc[c][v];
        const double b = bv[c][v];
        nan_in |= b != b;
        nan_acc |= s != s;
        const double o = b + s / divisor;
        nan_out |= o != o;
        po[static_cast<int64_t>(row0 + row) * n + (col0 + col)] = static_cast<O>(o);
      }
    }
  }
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
  if (__ballot(nan_acc) != 0ull && lane == 0) raise_flag(a.flag, 0);
  if (__ballot(nan_out) != 0ull && lane == 0) raise_flag(a.flag, 1);
}

// ---------------------------------------------------------------------------------------
// the client step (fedavg_lowrank_compress): one power-iteration step per tensor
// ---------------------------------------------------------------------------------------
//   M = fl64(delta) + fl64(error), recomputed wherever it is needed, never stored
//   P = M Q^T, P^ = P orthonormalised, R = P^^T M, left = round(P^), right = round(R),
//   residual = round(M - fl64(left) fl64(right))
// Five launches for a whole diff, each over one host-built tile list (LcTile):
//   1 lowrank_project_kernel      a workgroup owns 64 rows x one chunk of kLcCW columns; the chunk is
//                                 walked in steps of kLcStep columns: the 64 x 32 piece of M is loaded
//                                 with 16-byte non-temporal loads, added and widened into LDS row-major
//                                 (stride 34 doubles: the 16 rows x 2 columns a half-wave reads cover
//                                 the 32 double-wide banks once), the 16 x 32 piece of Q beside it in
//                                 the same shape; wave w owns the rows [16 w, 16 w + 16) and two
//                                 accumulators (even and odd instructions of a step, added at the
//                                 end); two buffers, one barrier per step. Partials: [chunk][m][16].
//   2 lowrank_ortho_kernel        one workgroup of 512 lanes per tensor; lane t owns the rows
//                                 t, t + 512, ...: it adds their chunk partials in ascending order and
//                                 keeps P column-major, in LDS for m <= kLcLdsRows and in the
//                                 workspace otherwise. Column j: twice (all dots against the columns
//                                 before it in one workgroup reduction, then the subtraction in
//                                 ascending order), then the norm. A reduction is the xor tree of a
//                                 wave, then the eight wave sums in a fixed tree.
//   3 lowrank_backproject_kernel  a workgroup owns 64 columns x one chunk of kLcCH rows, walked in
//                                 steps of kLcStep rows: the 32 x 64 piece of M goes through LDS
//                                 row-major (stride 80, as the fold's B panel), the 16 x 32 piece of
//                                 P^ beside it; wave w owns the columns [16 w, 16 w + 16).
//                                 Partials: [chunk][16][n].
//   4 lowrank_right_kernel        a lane owns a column: the partials in ascending chunk order, rounded.
//   5 lowrank_residual_kernel     64 x 64 tiles, K = r: the rounded factors straight from global
//                                 memory (they are small and cached), no LDS; M - acc rounded once.
// Rows past m, columns past n and slots past r are +0.0 on both operands. No atomics; a chunk is a
// compile-time width, so the result depends on the shapes alone.
constexpr int kLcCW = 256;                 // columns of one chunk of P = M Q^T
constexpr int kLcCH = 256;                 // rows of one chunk of R = P^^T M
constexpr int kLcStep = 32;                // columns (rows) of M staged per step
constexpr int kLcInstr = kLcStep / kLrK;   // matrix instructions per step
constexpr int kLcPStride = kLcStep + 2;    // doubles per staged row of a [.. x 32] panel: 34 = 2 mod 32
constexpr int kLcOrthoThreads = 512;
constexpr int kLcOrthoWaves = kLcOrthoThreads / 64;
constexpr int kLcLdsRows = 480;            // rows of P the orthonormaliser keeps in LDS: 480 * 16 * 8 = 60 KiB
constexpr int kLcMaxTensors = 1 << 20;
static_assert(kLcCW % kLcStep == 0 && kLcCH % kLcStep == 0 && kLcCW % kLrTN == 0 && kLcCH % kLrTM == 0, "whole steps");
static_assert(kLrEdge * kLcStep == 2 * kLrThreads, "two elements of the thin panel per lane");
static_assert(kLcOrthoWaves == 8, "the fixed tree of reduce()");

struct LcTensor {
  const void* delta;
  const void* error;  // or null
  const void* q;      // [r x n]: T, or fp64 where q_f64
  void* left;         // [m x r]
  void* right;        // [r x n]
  void* residual;     // [m x n]
  int64_t p_off;      // workspace, in doubles: the chunk partials of P, [p_chunks][m][16]
  int64_t ph_off;     //   P^, [16][ldp]
  int64_t r_off;      //   the chunk partials of R, [r_chunks][16][n]
  int32_t m, n, r, q_f64;
  int32_t p_chunks, r_chunks, ldp, pad_;
};

struct LcTile {
  int32_t t;
  int32_t row0;
  int32_t col0;
  int32_t chunk;
};

struct LcArgs {
  const LcTile* tiles;
  const LcTensor* tensors;
  double* ws;
  uint32_t* flag;
};

__device__ __forceinline__ int lc_min(int a, int b) { return a < b ? a : b; }
__device__ __forceinline__ bool lc_bad(double x) { return (x - x) != 0.0; }  // inf or NaN

// RNE(o) into element e
template <typename T>
__device__ __forceinline__ void lc_store(void* base, int64_t e, double o) {
  if constexpr (std::is_same_v<T, double>) ((double FEDAVG_AS_GLOBAL*)base)[e] = o;
  else if constexpr (std::is_same_v<T, float>) ((float FEDAVG_AS_GLOBAL*)base)[e] = static_cast<float>(o);
  else {
    u32x4 raw = {0u, 0u, 0u, 0u};
    dp_put<T>(raw, 0, o);
    ((uint16_t FEDAVG_AS_GLOBAL*)base)[e] = static_cast<uint16_t>(raw[0]);
  }
}

// An R x C piece of M = delta + error on its way into LDS (row-major, stride S doubles).
template <typename T, int R, int C, int S>
struct LcStage {
  using F = Format<T>;
  static constexpr int N = F::N;
  static constexpr int kVecs = C / N;  // 16-byte vectors per row
  static constexpr int kTotal = R * kVecs;
  static constexpr int kLoads = (kTotal + kLrThreads - 1) / kLrThreads;
  static_assert(C % N == 0 && S % 2 == 0, "whole vectors per row; rows start 16-byte aligned");
  u32x4 d[kLoads], e[kLoads];

  __device__ __forceinline__ static u32x4 load(const void* base, int64_t elem, int have) {
    const T* const pe = static_cast<const T*>(base) + elem;
    if (have >= N && (reinterpret_cast<uintptr_t>(pe) & 15u) == 0)
      return __builtin_nontemporal_load((const u32x4 FEDAVG_AS_GLOBAL*)pe);
    return load_guarded<T>(base, elem, have);
  }

  // the live rows x cols elements from (row0, col0) of the [.. x n] matrices; everything else +0.0
  __device__ __forceinline__ void fetch(const void* delta, const void* error, int64_t n, int row0, int col0, int rows,
                                        int cols, int t) {
#pragma unroll
    for (int q = 0; q < kLoads; ++q) {
      const int idx = t + q * kLrThreads;
      d[q] = u32x4{0u, 0u, 0u, 0u};
      e[q] = u32x4{0u, 0u, 0u, 0u};
      if (idx < kTotal) {
        const int row = idx / kVecs, v = idx % kVecs;
        const int have = cols - v * N;
        if (row < rows && have > 0) {
          const int64_t elem = static_cast<int64_t>(row0 + row) * n + (col0 + v * N);
          d[q] = load(delta, elem, have);
          if (error != nullptr) e[q] = load(error, elem, have);
        }
      }
    }
  }

  __device__ __forceinline__ void park(double* dst, int t, bool& bad) const {
#pragma unroll
    for (int q = 0; q < kLoads; ++q) {
      const int idx = t + q * kLrThreads;
      if (idx < kTotal) {
        double* const p = dst + (idx / kVecs) * S + (idx % kVecs) * N;
#pragma unroll
        for (int i = 0; i < N; i += 2) {
          const double x0 = F::value(d[q], i) + F::value(e[q], i);
          const double x1 = F::value(d[q], i + 1) + F::value(e[q], i + 1);
          bad |= lc_bad(x0) || lc_bad(x1);
          *reinterpret_cast<f64x2*>(p + i) = f64x2{x0, x1};
        }
      }
    }
  }
};

// 1: P = M Q^T. blockIdx.x = (tensor, 64 rows, chunk of kLcCW columns)
template <typename T>
__global__ __launch_bounds__(kLrThreads) void lowrank_project_kernel(LcArgs a) {
  __shared__ __attribute__((aligned(16))) double sM[2][kLrTM * kLcPStride];
  __shared__ __attribute__((aligned(16))) double sQ[2][kLrEdge * kLcPStride];
  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int g = lane >> 4, j16 = lane & 15;
  const LcTile tile = a.tiles[blockIdx.x];
  const LcTensor& ten = a.tensors[tile.t];
  const int m = ten.m, n = ten.n, r = ten.r;
  const int row0 = tile.row0, col0 = tile.col0;
  const int rows = lc_min(kLrTM, m - row0), width = lc_min(kLcCW, n - col0);
  const int steps = (width + kLcStep - 1) / kLcStep;
  const bool wave_live = kLrEdge * wave < rows;
  const bool q_f64 = ten.q_f64 != 0;
  bool bad = false;

  LcStage<T, kLrTM, kLcStep, kLcPStride> st;
  double qv[2];
  auto fetch = [&](int step) __attribute__((always_inline)) {
    const int c0 = col0 + step * kLcStep;
    const int cols = lc_min(kLcStep, col0 + width - c0);
    st.fetch(ten.delta, ten.error, n, row0, c0, rows, cols, t);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = t + u * kLrThreads, slot = idx / kLcStep, c = idx % kLcStep;
      qv[u] = 0.0;
      if (slot < r && c < cols) {
        const int64_t e = static_cast<int64_t>(slot) * n + (c0 + c);
        qv[u] = q_f64 ? ((const double FEDAVG_AS_GLOBAL*)ten.q)[e] : lr_widen<T>(lr_load<T>(ten.q, e));
      }
    }
  };
  auto park = [&](int buf) __attribute__((always_inline)) {
    st.park(sM[buf], t, bad);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = t + u * kLrThreads;
      bad |= lc_bad(qv[u]);
      sQ[buf][(idx / kLcStep) * kLcPStride + idx % kLcStep] = qv[u];
    }
  };

  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  fetch(0);
  park(0);
  __syncthreads();
#pragma unroll 1
  for (int step = 0; step < steps; ++step) {
    const int cur = step & 1;
    const bool more = step + 1 < steps;
    if (more) fetch(step + 1);
    if (wave_live) {
      // A[i][k] = M[16 w + i][4 ks + k], B[k][j] = Q[j][4 ks + k]: both panels are read the same way
      const double* const pa = sM[cur] + (kLrEdge * wave + j16) * kLcPStride + g;
      const double* const pq = sQ[cur] + j16 * kLcPStride + g;
#pragma unroll
      for (int ks = 0; ks < kLcInstr; ks += 2) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kLrK * ks], pq[kLrK * ks], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kLrK * (ks + 1)], pq[kLrK * (ks + 1)], acc1, 0, 0, 0);
      }
    }
    if (more) park(cur ^ 1);
    __syncthreads();
  }
  if (wave_live) {  // D[i][j]: register v of lane l holds i = 4 v + l / 16, j = l % 16
    double FEDAVG_AS_GLOBAL* const out =
        (double FEDAVG_AS_GLOBAL*)(a.ws + ten.p_off) +
        (static_cast<int64_t>(tile.chunk) * m + row0 + kLrEdge * wave) * kLrEdge;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = 4 * v + g;
      if (kLrEdge * wave + row < rows) out[row * kLrEdge + j16] = acc0[v] + acc1[v];
    }
  }
  if (__ballot(bad) != 0ull && lane == 0) raise_flag(a.flag, 2);
}

// 2: P^ = orthonormalise(sum of the chunk partials). blockIdx.x = tensor
template <typename T>
__global__ __launch_bounds__(kLcOrthoThreads) void lowrank_ortho_kernel(LcArgs a) {
  __shared__ __attribute__((aligned(16))) double sP[kLrEdge * kLcLdsRows];
  __shared__ double sRed[2][kLcOrthoWaves * kLrEdge];
  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63, wave = t >> 6;
  const LcTensor& ten = a.tensors[blockIdx.x];
  const int m = ten.m, r = ten.r, chunks = ten.p_chunks;
  const bool in_lds = m <= kLcLdsRows;
  double* const gP = a.ws + ten.ph_off;
  double* const P = in_lds ? sP : gP;  // column-major: P[k * ld + i]; lane t touches the rows t, t + 512, .. only
  const int64_t ld = in_lds ? kLcLdsRows : ten.ldp;

  const double* const part = a.ws + ten.p_off;
  for (int i = t; i < m; i += kLcOrthoThreads) {
    double s[kLrEdge];
    for (int c = 0; c < chunks; ++c) {  // ascending chunk order
      const f64x2* const row = reinterpret_cast<const f64x2*>(part + (static_cast<int64_t>(c) * m + i) * kLrEdge);
#pragma unroll
      for (int k = 0; k < kLrEdge; k += 2) {
        const f64x2 v = row[k / 2];
        s[k] = c == 0 ? v[0] : s[k] + v[0];
        s[k + 1] = c == 0 ? v[1] : s[k + 1] + v[1];
      }
    }
#pragma unroll
    for (int k = 0; k < kLrEdge; ++k) {
      if (k < r) P[k * ld + i] = s[k];
    }
  }

  // the first `count` values of d summed over the workgroup, in every lane: the xor tree of a wave,
  // then the eight wave sums pairwise. Two scratch buffers in turn: one barrier per reduction.
  int buf = 0;
  auto reduce = [&](double (&d)[kLrEdge], int count) __attribute__((always_inline)) {
#pragma unroll
    for (int k = 0; k < kLrEdge; ++k) {
      if (k < count) {
        double v = d[k];
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off);
        if (lane == 0) sRed[buf][wave * kLrEdge + k] = v;
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kLrEdge; ++k) {
      if (k < count) {
        const double* const p = sRed[buf] + k;
        d[k] = ((p[0] + p[kLrEdge]) + (p[2 * kLrEdge] + p[3 * kLrEdge])) +
               ((p[4 * kLrEdge] + p[5 * kLrEdge]) + (p[6 * kLrEdge] + p[7 * kLrEdge]));
      }
    }
    buf ^= 1;
  };

  for (int j = 0; j < r; ++j) {
    double* const pj = P + j * ld;
    double d[kLrEdge];
    if (j > 0) {
      for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int k = 0; k < kLrEdge; ++k) d[k] = 0.0;
        for (int i = t; i < m; i += kLcOrthoThreads) {
          const double v = pj[i];
#pragma unroll
          for (int k = 0; k < kLrEdge; ++k) {
            if (k < j) d[k] = __builtin_fma(P[k * ld + i], v, d[k]);
          }
        }
        reduce(d, j);
        for (int i = t; i < m; i += kLcOrthoThreads) {
          double v = pj[i];
#pragma unroll
          for (int k = 0; k < kLrEdge; ++k) {
            if (k < j) v = v - d[k] * P[k * ld + i];
          }
          pj[i] = v;
        }
      }
    }
    d[0] = 0.0;
    for (int i = t; i < m; i += kLcOrthoThreads) d[0] = __builtin_fma(pj[i], pj[i], d[0]);
    reduce(d, 1);
    const double norm = __builtin_sqrt(d[0]);
    for (int i = t; i < m; i += kLcOrthoThreads) pj[i] = norm > 0.0 ? pj[i] / norm : 0.0;  // a vanished column stays 0
  }

  for (int i = t; i < m; i += kLcOrthoThreads) {
#pragma unroll
    for (int k = 0; k < kLrEdge; ++k) {
      if (k < r) {
        const double v = P[k * ld + i];
        if (in_lds) gP[static_cast<int64_t>(k) * ten.ldp + i] = v;
        lc_store<T>(ten.left, static_cast<int64_t>(i) * r + k, v);
      }
    }
  }
}

// 3: R = P^^T M. blockIdx.x = (tensor, 64 columns, chunk of kLcCH rows)
template <typename T>
__global__ __launch_bounds__(kLrThreads) void lowrank_backproject_kernel(LcArgs a) {
  __shared__ __attribute__((aligned(16))) double sM[2][kLcStep * kLrStride];
  __shared__ __attribute__((aligned(16))) double sP[2][kLrEdge * kLcPStride];
  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int g = lane >> 4, j16 = lane & 15;
  const LcTile tile = a.tiles[blockIdx.x];
  const LcTensor& ten = a.tensors[tile.t];
  const int m = ten.m, n = ten.n, r = ten.r;
  const int row0 = tile.row0, col0 = tile.col0;
  const int cols = lc_min(kLrTN, n - col0), height = lc_min(kLcCH, m - row0);
  const int steps = (height + kLcStep - 1) / kLcStep;
  const bool wave_live = kLrEdge * wave < cols;
  const double FEDAVG_AS_GLOBAL* const ph = (const double FEDAVG_AS_GLOBAL*)(a.ws + ten.ph_off);
  const int64_t ldp = ten.ldp;
  bool unused = false;

  LcStage<T, kLcStep, kLrTN, kLrStride> st;
  double pv[2];
  auto fetch = [&](int step) __attribute__((always_inline)) {
    const int r0 = row0 + step * kLcStep;
    const int live = lc_min(kLcStep, row0 + height - r0);
    st.fetch(ten.delta, ten.error, n, r0, col0, live, cols, t);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = t + u * kLrThreads, slot = idx / kLcStep, i = idx % kLcStep;
      pv[u] = (slot < r && i < live) ? ph[slot * ldp + (r0 + i)] : 0.0;
    }
  };
  auto park = [&](int buf) __attribute__((always_inline)) {
    st.park(sM[buf], t, unused);
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int idx = t + u * kLrThreads;
      sP[buf][(idx / kLcStep) * kLcPStride + idx % kLcStep] = pv[u];
    }
  };

  f64x4 acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
  fetch(0);
  park(0);
  __syncthreads();
#pragma unroll 1
  for (int step = 0; step < steps; ++step) {
    const int cur = step & 1;
    const bool more = step + 1 < steps;
    if (more) fetch(step + 1);
    if (wave_live) {
      // A[i][k] = P^[4 ks + k][i], B[k][j] = M[4 ks + k][16 w + j]
      const double* const pa = sP[cur] + j16 * kLcPStride + g;
      const double* const pb = sM[cur] + g * kLrStride + kLrEdge * wave + j16;
#pragma unroll
      for (int ks = 0; ks < kLcInstr; ks += 2) {
        acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kLrK * ks], pb[kLrK * ks * kLrStride], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[kLrK * (ks + 1)], pb[kLrK * (ks + 1) * kLrStride], acc1, 0, 0, 0);
      }
    }
    if (more) park(cur ^ 1);
    __syncthreads();
  }
  if (wave_live && kLrEdge * wave + j16 < cols) {
    double FEDAVG_AS_GLOBAL* const out = (double FEDAVG_AS_GLOBAL*)(a.ws + ten.r_off) +
                                         static_cast<int64_t>(tile.chunk) * kLrEdge * n + (col0 + kLrEdge * wave + j16);
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int slot = 4 * v + g;
      if (slot < r) out[static_cast<int64_t>(slot) * n] = acc0[v] + acc1[v];
    }
  }
}

// 4: right = round(sum of the chunk partials of R). blockIdx.x = (tensor, kLrThreads columns)
template <typename T>
__global__ __launch_bounds__(kLrThreads) void lowrank_right_kernel(LcArgs a) {
  const LcTile tile = a.tiles[blockIdx.x];
  const LcTensor& ten = a.tensors[tile.t];
  const int n = ten.n, r = ten.r, chunks = ten.r_chunks;
  const int col = tile.col0 + static_cast<int>(threadIdx.x);
  if (col >= n) return;
  const double FEDAVG_AS_GLOBAL* const part = (const double FEDAVG_AS_GLOBAL*)(a.ws + ten.r_off) + col;
  for (int slot = 0; slot < r; ++slot) {
    double s = part[static_cast<int64_t>(slot) * n];
    for (int c = 1; c < chunks; ++c) s = s + part[(static_cast<int64_t>(c) * kLrEdge + slot) * n];
    lc_store<T>(ten.right, static_cast<int64_t>(slot) * n + col, s);
  }
}

// 5: residual = M - left right. blockIdx.x = (tensor, 64 x 64 tile); no barrier in this kernel
template <typename T>
__global__ __launch_bounds__(kLrThreads) void lowrank_residual_kernel(LcArgs a) {
  const int t = static_cast<int>(threadIdx.x);
  const int lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int g = lane >> 4, j16 = lane & 15;
  const LcTile tile = a.tiles[blockIdx.x];
  const LcTensor& ten = a.tensors[tile.t];
  const int m = ten.m, n = ten.n, r = ten.r;
  const int row0 = tile.row0, col0 = tile.col0;
  const int rows = lc_min(kLrTM, m - row0), cols = lc_min(kLrTN, n - col0);
  if (kLrEdge * wave >= rows) return;  // wave-uniform
  const int instr = (r + kLrK - 1) / kLrK;

  double mv[kLrColTiles][4];
#pragma unroll
  for (int c = 0; c < kLrColTiles; ++c) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = kLrEdge * wave + 4 * v + g, col = kLrEdge * c + j16;
      mv[c][v] = 0.0;
      if (row < rows && col < cols) {
        const int64_t e = static_cast<int64_t>(row0 + row) * n + (col0 + col);
        mv[c][v] = lr_widen<T>(lr_load<T>(ten.delta, e));
        if (ten.error != nullptr) mv[c][v] = mv[c][v] + lr_widen<T>(lr_load<T>(ten.error, e));
      }
    }
  }
  double av[kLrInstr];
#pragma unroll
  for (int ks = 0; ks < kLrInstr; ++ks) {
    const int slot = kLrK * ks + g, row = kLrEdge * wave + j16;
    av[ks] = (slot < r && row < rows) ? lr_widen<T>(lr_load<T>(ten.left, static_cast<int64_t>(row0 + row) * r + slot)) : 0.0;
  }
  f64x4 acc[kLrColTiles];
#pragma unroll
  for (int c = 0; c < kLrColTiles; ++c) {
    acc[c] = f64x4{0.0, 0.0, 0.0, 0.0};
    if (kLrEdge * c < cols) {  // wave-uniform
#pragma unroll
      for (int ks = 0; ks < kLrInstr; ++ks) {
        if (ks < instr) {  // wave-uniform
          const int slot = kLrK * ks + g, col = kLrEdge * c + j16;
          const double bv =
              (slot < r && col < cols) ? lr_widen<T>(lr_load<T>(ten.right, static_cast<int64_t>(slot) * n + (col0 + col))) : 0.0;
          acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[ks], bv, acc[c], 0, 0, 0);
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kLrColTiles; ++c) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int row = kLrEdge * wave + 4 * v + g, col = kLrEdge * c + j16;
      if (row < rows && col < cols)
        lc_store<T>(ten.residual, static_cast<int64_t>(row0 + row) * n + (col0 + col), mv[c][v] - acc[c][v]);
    }
  }
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct LowRankState {
  LrTile* d_tiles = nullptr;  // the tiles of the layout under `shape`
  int64_t num_tiles = 0;
  std::vector<int32_t> shape;  // the rows, then the ranks, the tile list was built for
  double* d_ws = nullptr;      // the client step's workspace: grows on demand
  size_t ws_doubles = 0;
  TableRing ring;
  ~LowRankState() {
    ring.release();
    if (d_tiles) (void)hipFree(d_tiles);
    if (d_ws) (void)hipFree(d_ws);
  }
};

int32_t ensure_state(void** slot, LowRankState** out) {
  if (*slot == nullptr) {
    LowRankState* st = new LowRankState();
    const int32_t r = hip_status("low-rank state", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<LowRankState*>(*slot);
  return FEDAVG_OK;
}

// The tile list of the layout with rows[t] x (seg_numel[t] / rows[t]) tensors of rank ranks[t]. A call
// with the shape of the call before keeps the list; hipFree waits for the launches that read the old one.
int32_t ensure_tiles(LowRankState* st, const fedavg_robust_view& v, const int32_t* rows, const int32_t* ranks) {
  const int T = v.num_segments;
  std::vector<int32_t> shape(rows, rows + T);
  shape.insert(shape.end(), ranks, ranks + T);
  if (st->d_tiles != nullptr && shape == st->shape) return FEDAVG_OK;
  std::vector<LrTile> tiles;
  for (int t = 0; t < T; ++t) {
    const int64_t m = rows[t], n = v.seg_numel[t] / m;
    for (int64_t r0 = 0; r0 < m; r0 += kLrTM) {
      for (int64_t c0 = 0; c0 < n; c0 += kLrTN) {
        LrTile x;
        x.seg = t;
        x.r = ranks[t];
        x.row0 = static_cast<int32_t>(r0);
        x.col0 = static_cast<int32_t>(c0);
        x.rows = static_cast<int32_t>(m - r0 < kLrTM ? m - r0 : kLrTM);
        x.cols = static_cast<int32_t>(n - c0 < kLrTN ? n - c0 : kLrTN);
        x.n = n;
        tiles.push_back(x);
      }
    }
  }
  if (tiles.size() > 0x7fffffffull) return invalid("layout too large for one low-rank fold");
  if (st->d_tiles) FEDAVG_TRY_HIP(hipFree(st->d_tiles));
  st->d_tiles = nullptr;
  st->num_tiles = 0;
  st->shape.clear();
  if (!tiles.empty()) {
    LrTile* dev = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&dev), sizeof(LrTile) * tiles.size());
    if (e == hipSuccess) e = hipMemcpy(dev, tiles.data(), sizeof(LrTile) * tiles.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      if (dev) (void)hipFree(dev);
      return hip_status("low-rank tile table", e);
    }
    st->d_tiles = dev;
    st->num_tiles = static_cast<int64_t>(tiles.size());
    st->shape = std::move(shape);
  }
  return FEDAVG_OK;
}

template <typename T>
void launch_fold(int32_t out_dtype, dim3 grid, hipStream_t s, const LrArgs& a) {
  const dim3 block(kLrThreads);
  if (out_dtype == FEDAVG_F32) hipLaunchKernelGGL((lowrank_fold_kernel<T, float>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((lowrank_fold_kernel<T, double>), grid, block, 0, s, a);
}

// The client step's workspace, at least `doubles` large; hipFree waits for the launches that read the old one.
int32_t ensure_workspace(LowRankState* st, size_t doubles) {
  if (doubles <= st->ws_doubles) return FEDAVG_OK;
  if (st->d_ws) FEDAVG_TRY_HIP(hipFree(st->d_ws));
  st->d_ws = nullptr;
  st->ws_doubles = 0;
  const size_t grown = doubles + doubles / 2;
  FEDAVG_TRY(hip_status("low-rank workspace", hipMalloc(reinterpret_cast<void**>(&st->d_ws), sizeof(double) * grown)));
  st->ws_doubles = grown;
  return FEDAVG_OK;
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

template <typename T>
void launch_compress(const unsigned (&grid)[5], hipStream_t s, LcArgs a, const LcTile* const (&lists)[5]) {
  const dim3 block(kLrThreads);
  a.tiles = lists[0];
  hipLaunchKernelGGL((lowrank_project_kernel<T>), dim3(grid[0]), block, 0, s, a);
  a.tiles = nullptr;  // one workgroup per tensor
  hipLaunchKernelGGL((lowrank_ortho_kernel<T>), dim3(grid[1]), dim3(kLcOrthoThreads), 0, s, a);
  a.tiles = lists[2];
  hipLaunchKernelGGL((lowrank_backproject_kernel<T>), dim3(grid[2]), block, 0, s, a);
  a.tiles = lists[3];
  hipLaunchKernelGGL((lowrank_right_kernel<T>), dim3(grid[3]), block, 0, s, a);
  a.tiles = lists[4];
  hipLaunchKernelGGL((lowrank_residual_kernel<T>), dim3(grid[4]), block, 0, s, a);
}

}  // namespace

int32_t fedavg_internal_lowrank_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "lowrank_tm") *out = kLrTM;
  else if (n == "lowrank_chunk_cols") *out = kLcCW;
  else if (n == "lowrank_chunk_rows") *out = kLcCH;
  else if (n == "lowrank_ortho_lds_rows") *out = kLcLdsRows;
  else if (n == "lowrank_ortho_threads") *out = kLcOrthoThreads;
  else if (n == "lowrank_tn") *out = kLrTN;
  else if (n == "lowrank_kstep") *out = kLrKStep;
  else if (n == "lowrank_threads") *out = kLrThreads;
  else if (n == "lowrank_max_rank") *out = kLrMaxRank;
  else if (n == "lowrank_max_clients") *out = kLrMaxClients;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_lowrank_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<LowRankState*>(state);
}

extern "C" int32_t fedavg_lowrank_aggregate_delta(fedavg_ctx* ctx, const void* const* left_ptrs,
                                                  const void* const* right_ptrs, int32_t dtype, const int32_t* rows,
                                                  const int32_t* ranks, const double* weights, int32_t num_clients,
                                                  double divisor, const double* const* base_ptrs,
                                                  void* const* out_ptrs, int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_LOWRANK, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (dtype != FEDAVG_F32 && dtype != FEDAVG_F16 && dtype != FEDAVG_BF16 && dtype != FEDAVG_F64)
    return invalid("the low-rank fold reads fp32 / fp16 / bf16 / fp64 factors");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("the low-rank fold writes fp32 or fp64");
  if (left_ptrs == nullptr || right_ptrs == nullptr || rows == nullptr || ranks == nullptr || weights == nullptr ||
      base_ptrs == nullptr || out_ptrs == nullptr)
    return invalid("null factor table, rows, ranks, weights, base or outputs");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kLrMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the low-rank fold takes at most " +
                   std::to_string(kLrMaxClients));
  if (!(std::isfinite(divisor) && divisor > 0)) return invalid("the divisor must be finite and > 0");
  for (int32_t i = 0; i < num_clients; ++i)
    if (!std::isfinite(weights[i])) return invalid("weight " + std::to_string(i) + " is not finite");
  const int T = v.num_segments;
  const size_t esize = dtype == FEDAVG_F64 ? 8 : dtype == FEDAVG_F32 ? 4 : 2;
  const size_t out_bytes = out_dtype == FEDAVG_F64 ? 8 : 4;
  for (int t = 0; t < T; ++t) {
    const std::string who = "segment " + std::to_string(t);
    if (rows[t] < 1 || v.seg_numel[t] % rows[t] != 0)
      return invalid(who + ": " + std::to_string(rows[t]) + " rows do not divide its " +
                     std::to_string(v.seg_numel[t]) + " elements");
    if (v.seg_numel[t] / rows[t] > 0x7fffffffll) return invalid(who + ": more than 2^31 - 1 columns");
    if (ranks[t] < 1 || ranks[t] > kLrMaxRank)
      return invalid(who + ": rank " + std::to_string(ranks[t]) + " is not in 1 .. " + std::to_string(kLrMaxRank));
    if (base_ptrs[t] == nullptr) return invalid("the base lacks " + who);
    if (misaligned(base_ptrs[t], 8)) return invalid("base tensor not aligned to fp64");
    if (out_ptrs[t] == nullptr) return invalid("null output pointer for " + who);
    if (misaligned(out_ptrs[t], out_bytes)) return invalid("output tensor not aligned to its element size");
    if (static_cast<const void*>(out_ptrs[t]) == static_cast<const void*>(base_ptrs[t]))
      return invalid(who + ": the fold is not in-place (out == base)");
  }
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (size_t i = 0; i < entries; ++i) {
    // the message is built only on a refusal: this loop runs n * T times on every call
    const auto where = [T, i] { return "client " + std::to_string(i / T) + ", segment " + std::to_string(i % T); };
    if (left_ptrs[i] == nullptr || right_ptrs[i] == nullptr) return invalid(where() + ": null factor");
    if (misaligned(left_ptrs[i], esize) || misaligned(right_ptrs[i], esize))
      return invalid(where() + ": a factor is not aligned to its element size");
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  LowRankState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  FEDAVG_TRY(ensure_tiles(st, v, rows, ranks));
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: [n][T] left pointers, [n][T] right pointers, [T] base pointers, [T] output
  // pointers, [n] weights
  const size_t ptr_bytes = sizeof(void*) * entries;
  const size_t seg_bytes = sizeof(void*) * static_cast<size_t>(T);
  const size_t w_bytes = sizeof(double) * static_cast<size_t>(num_clients);
  const size_t o_right = ptr_bytes, o_base = 2 * ptr_bytes, o_out = o_base + seg_bytes, o_w = o_out + seg_bytes;
  const size_t bytes = o_w + w_bytes;
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, left_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_right, right_ptrs, ptr_bytes);
  std::memcpy(sl.host + o_base, base_ptrs, seg_bytes);
  std::memcpy(sl.host + o_out, out_ptrs, seg_bytes);
  std::memcpy(sl.host + o_w, weights, w_bytes);
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  LrArgs a;
  a.tiles = st->d_tiles;
  a.left = reinterpret_cast<const void* const*>(sl.dev);
  a.right = reinterpret_cast<const void* const*>(sl.dev + o_right);
  a.base = reinterpret_cast<const double* const*>(sl.dev + o_base);
  a.outs = reinterpret_cast<void* const*>(sl.dev + o_out);
  a.w = reinterpret_cast<const double*>(sl.dev + o_w);
  a.divisor = divisor;
  a.flag = v.d_flag;
  a.num_segments = T;
  a.n = num_clients;
  if (st->num_tiles > 0) {
    const dim3 grid(static_cast<unsigned>(st->num_tiles));
    switch (dtype) {
      case FEDAVG_F32: launch_fold<float>(out_dtype, grid, s, a); break;
      case FEDAVG_F16: launch_fold<__half>(out_dtype, grid, s, a); break;
      case FEDAVG_BF16: launch_fold<bf16_t>(out_dtype, grid, s, a); break;
      default: launch_fold<double>(out_dtype, grid, s, a); break;
    }
  }
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("low-rank fold launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_lowrank_compress(fedavg_ctx* ctx, int32_t dtype, const void* const* delta_ptrs,
                                           const void* const* error_ptrs, const void* const* q_ptrs,
                                           const int32_t* q_dtypes, const int32_t* rows, const int32_t* cols,
                                           const int32_t* ranks, int32_t num_tensors, void* const* left_ptrs,
                                           void* const* right_ptrs, void* const* residual_ptrs, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_LOWRANK, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (dtype != FEDAVG_F32 && dtype != FEDAVG_F16 && dtype != FEDAVG_BF16 && dtype != FEDAVG_F64)
    return invalid("the low-rank step takes fp32, fp16, bf16 or fp64 tensors");
  if (delta_ptrs == nullptr || q_ptrs == nullptr || q_dtypes == nullptr || rows == nullptr || cols == nullptr ||
      ranks == nullptr || left_ptrs == nullptr || right_ptrs == nullptr || residual_ptrs == nullptr)
    return invalid("null delta, start, start dtype, rows, columns, ranks, left, right or residual table");
  if (num_tensors < 1 || num_tensors > kLcMaxTensors)
    return invalid("the low-rank step takes between 1 and " + std::to_string(kLcMaxTensors) + " tensors");
  const int T = num_tensors;
  const size_t esize = dtype == FEDAVG_F64 ? 8 : (dtype == FEDAVG_F32 ? 4 : 2);
  // the tile lists: project, (ortho: one workgroup per tensor), backproject, right, residual
  uint64_t count[5] = {0, static_cast<uint64_t>(T), 0, 0, 0};
  uint64_t ws_doubles = 0;
  for (int t = 0; t < T; ++t) {
    const std::string who = "tensor " + std::to_string(t);
    if (rows[t] < 1 || cols[t] < 1) return invalid(who + ": fewer than 1 row or column");
    if (ranks[t] < 1 || ranks[t] > kLrMaxRank)
      return invalid(who + ": rank " + std::to_string(ranks[t]) + " is not in 1 .. " + std::to_string(kLrMaxRank));
    const int64_t m = rows[t], n = cols[t], r = ranks[t];
    if (m * n > 0x7fffffffll) return invalid(who + ": more than 2^31 - 1 elements");
    if (r * (m + n) >= m * n)
      return invalid(who + ": rank " + std::to_string(r) + " factors would not make a " + std::to_string(m) + " x " +
                     std::to_string(n) + " matrix smaller");
    if (q_dtypes[t] != dtype && q_dtypes[t] != FEDAVG_F64) return invalid(who + ": the start is of the tensors' dtype or fp64");
    if (delta_ptrs[t] == nullptr || q_ptrs[t] == nullptr || left_ptrs[t] == nullptr || right_ptrs[t] == nullptr ||
        residual_ptrs[t] == nullptr)
      return invalid(who + ": null delta, start, left, right or residual buffer");
    if (misaligned(delta_ptrs[t], esize) || misaligned(left_ptrs[t], esize) || misaligned(right_ptrs[t], esize) ||
        misaligned(residual_ptrs[t], esize) || (error_ptrs != nullptr && misaligned(error_ptrs[t], esize)) ||
        misaligned(q_ptrs[t], q_dtypes[t] == FEDAVG_F64 ? 8 : esize))
      return invalid(who + ": a buffer is not aligned to its element size");
    const int64_t rt = ceil_div(m, kLrTM), ct = ceil_div(n, kLrTN), pc = ceil_div(n, kLcCW), rc = ceil_div(m, kLcCH);
    count[0] += static_cast<uint64_t>(rt * pc);
    count[2] += static_cast<uint64_t>(ct * rc);
    count[3] += static_cast<uint64_t>(ceil_div(n, kLrThreads));
    count[4] += static_cast<uint64_t>(rt * ct);
    ws_doubles += static_cast<uint64_t>(pc * m * kLrEdge + kLrEdge * (m + (m & 1)) + rc * kLrEdge * n);
  }
  for (int k = 0; k < 5; ++k)
    if (count[k] > 0x7fffffffull) return invalid("layout too large for one low-rank step");

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  LowRankState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  FEDAVG_TRY(ensure_workspace(st, static_cast<size_t>(ws_doubles)));
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: one LcTensor per tensor, then the four tile lists
  const size_t tensor_bytes = align16(sizeof(LcTensor) * static_cast<size_t>(T));
  size_t list_off[5] = {0, 0, 0, 0, 0};
  size_t bytes = tensor_bytes;
  for (int k = 0; k < 5; ++k) {
    if (k == 1) continue;
    list_off[k] = bytes;
    bytes += align16(sizeof(LcTile) * static_cast<size_t>(count[k]));
  }
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memset(sl.host, 0, bytes);
  LcTensor* const h_tensors = reinterpret_cast<LcTensor*>(sl.host);
  LcTile* h_list[5];
  size_t fill[5] = {0, 0, 0, 0, 0};
  for (int k = 0; k < 5; ++k) h_list[k] = reinterpret_cast<LcTile*>(sl.host + list_off[k]);
  int64_t ws_off = 0;
  for (int t = 0; t < T; ++t) {
    const int32_t m = rows[t], n = cols[t];
    LcTensor& g = h_tensors[t];
    g.delta = delta_ptrs[t];
    g.error = error_ptrs != nullptr ? error_ptrs[t] : nullptr;
    g.q = q_ptrs[t];
    g.left = left_ptrs[t];
    g.right = right_ptrs[t];
    g.residual = residual_ptrs[t];
    g.m = m;
    g.n = n;
    g.r = ranks[t];
    g.q_f64 = (q_dtypes[t] == FEDAVG_F64 && dtype != FEDAVG_F64) ? 1 : 0;
    g.p_chunks = static_cast<int32_t>(ceil_div(n, kLcCW));
    g.r_chunks = static_cast<int32_t>(ceil_div(m, kLcCH));
    g.ldp = m + (m & 1);  // even: every part of the workspace starts 16-byte aligned
    g.p_off = ws_off;
    ws_off += static_cast<int64_t>(g.p_chunks) * m * kLrEdge;
    g.ph_off = ws_off;
    ws_off += static_cast<int64_t>(kLrEdge) * g.ldp;
    g.r_off = ws_off;
    ws_off += static_cast<int64_t>(g.r_chunks) * kLrEdge * n;
    for (int32_t r0 = 0; r0 < m; r0 += kLrTM) {
      for (int32_t c = 0; c < g.p_chunks; ++c) h_list[0][fill[0]++] = LcTile{t, r0, c * kLcCW, c};
      for (int32_t c0 = 0; c0 < n; c0 += kLrTN) h_list[4][fill[4]++] = LcTile{t, r0, c0, 0};
    }
    for (int32_t c0 = 0; c0 < n; c0 += kLrTN)
      for (int32_t c = 0; c < g.r_chunks; ++c) h_list[2][fill[2]++] = LcTile{t, c * kLcCH, c0, c};
    for (int32_t c0 = 0; c0 < n; c0 += kLrThreads) h_list[3][fill[3]++] = LcTile{t, 0, c0, 0};
  }
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  LcArgs a;
  a.tiles = nullptr;
  a.tensors = reinterpret_cast<const LcTensor*>(sl.dev);
  a.ws = st->d_ws;
  a.flag = v.d_flag;
  const LcTile* lists[5];
  unsigned grid[5];
  for (int k = 0; k < 5; ++k) {
    lists[k] = reinterpret_cast<const LcTile*>(sl.dev + list_off[k]);
    grid[k] = static_cast<unsigned>(count[k]);
  }
  switch (dtype) {
    case FEDAVG_F32: launch_compress<float>(grid, s, a, lists); break;
    case FEDAVG_F16: launch_compress<__half>(grid, s, a, lists); break;
    case FEDAVG_BF16: launch_compress<bf16_t>(grid, s, a, lists); break;
    default: launch_compress<double>(grid, s, a, lists); break;
  }
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP,
                                (std::string("low-rank compress launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}
