// secagg_kernels.hip — gfx950 (MI355X) kernels of secure aggregation by pairwise masking (Bonawitz et
// al., CCS 2017): fedavg_secagg_mask (a client's fixed-point encoding plus its masks) and
// fedavg_secagg_unmask (the server's sum of the masked words, minus the masks it can regenerate,
// decoded). Not an algorithm of the reference: the contract is in include/fedavg_hip.h and DESIGN.md
// §5z, and tests/secagg_reference.py restates it in numpy.
//
// Everything is addition in Z/2^64, which is associative and commutative: the kernels split and
// reorder the work freely and still owe the restatement the same bits. The cost is the generator,
// not the bytes: one Philox4x32-10 block (20 32 x 32 -> 64 products) per seed entry and two elements.
//
//   * The block is the unit. A Philox block is the mask of elements 2b and 2b + 1 of a tensor: one
//     16-byte vector of masked words. A lane owns kSaBlocks blocks, lane l's k-th being block
//     64 k + l of its wave's tile (consecutive lanes: consecutive vectors), and keeps their
//     2 * kSaBlocks ring accumulators in registers while it loops over the seed entries. The blocks of
//     a lane are independent chains for the integer multiplier.
//   * Uniform keys. The seed table is read through the constant address space at a wave-uniform
//     index, so a seed's two key words and the ten round keys derived from them live in scalar
//     registers and the key schedule runs on the scalar unit.
//   * One product per multiplication. sa_philox writes a round's two multiplications as
//     32 x 32 -> 64 products (v_mad_u64_u32: hi and lo from one instruction) and gives the words of
//     q_philox (device_common.h), which stays as it is for the modules whose code is pinned.
//   * The signs cost nothing. The host sorts the table, the entries that are added first: the kernel
//     runs one adding and one subtracting loop.
//   * The tile is one wave's share: kSaTile = 64 * kSaBlocks * 2 elements. With a short seed table a
//     256-lane workgroup owns four tiles, one per wave: no LDS, no barrier. From kSaSplit entries on
//     (a dropout round has |A| (1 + |D|)) a workgroup owns ONE tile and its four waves take every
//     fourth seed entry (and, in unmask, every fourth client); the partial accumulators meet in LDS
//     (16 KiB) and wave w finishes block w of every lane.
//   * unmask loads a client's vector with one non-temporal 16-byte load, kSaLoads clients (times
//     kSaBlocks blocks) in flight per lane. Storage that is 8-byte but not 16-byte aligned, and a
//     segment's last odd element, go element by element under a guard (half of that block's words
//     are unused). The decode, the division and the optional base add happen in the same pass.
//   * Nothing outside a tensor is read or written, the accumulator is not touched, no atomics apart
//     from raise_flag, no scratch.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kSaThreads = 256;
constexpr int kSaWaves = kSaThreads / 64;
constexpr int kSaBlocks = 4;                  // Philox blocks a lane owns
constexpr int kSaTile = 64 * kSaBlocks * 2;   // elements of a wave's tile
constexpr int kSaLoads = 4;                   // clients whose vectors a lane has in flight
constexpr int kSaSplit = 96;                  // seed entries from which a workgroup shares one tile
constexpr int kSaMaxClients = FEDAVG_SECAGG_MAX_CLIENTS;
constexpr int kSaMaxSeeds = 1 << 20;
constexpr int kSaMaxTensors = 1 << 20;
static_assert(kSaBlocks == kSaWaves, "in a shared tile wave w finishes block w of every lane");

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

struct SaSeed {
  uint32_t k0, k1;  // the Philox key: seed & 0xffffffff, seed >> 32
};

// Philox4x32-10 of counter (c0, c1, c2, c3) under key (k0, k1): the words of q_philox, as the mask
// words of the block's even element (w0 | w1 << 32) and of its odd element (w2 | w3 << 32).
__device__ __forceinline__ void sa_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                          uint64_t& even, uint64_t& odd) {
  constexpr uint64_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u;
  constexpr uint32_t kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = kM0 * c0, p1 = kM1 * c2;
    c0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    c1 = static_cast<uint32_t>(p1);
    c2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c3 = static_cast<uint32_t>(p0);
    k0 += kW0;
    k1 += kW1;
  }
  even = c0 | (static_cast<uint64_t>(c1) << 32);
  odd = c2 | (static_cast<uint64_t>(c3) << 32);
}

// The masks of seed entries first, first + step, ... below last, added to (or subtracted from) the
// lane's accumulators. first, last and step are wave-uniform: the keys are scalar loads.
template <bool kSub>
__device__ __forceinline__ void sa_seeds(const SaSeed* seeds, int first, int last, int step, int64_t block0,
                                         uint32_t tensor, uint32_t draw, uint64_t (&acc)[2 * kSaBlocks]) {
  const SaSeed FEDAVG_AS_CONST* sp = (const SaSeed FEDAVG_AS_CONST*)seeds;
#pragma unroll 1
  for (int s = first; s < last; s += step) {
    const uint32_t k0 = sp[s].k0, k1 = sp[s].k1;
#pragma unroll
    for (int k = 0; k < kSaBlocks; ++k) {
      const uint64_t b = static_cast<uint64_t>(block0 + 64 * k);
      uint64_t even, odd;
      sa_philox(static_cast<uint32_t>(b), static_cast<uint32_t>(b >> 32), tensor, draw, k0, k1, even, odd);
      if (kSub) {
        acc[2 * k] -= even;
        acc[2 * k + 1] -= odd;
      } else {
        acc[2 * k] += even;
        acc[2 * k + 1] += odd;
      }
    }
  }
}

// The plus entries [0, num_plus), then the minus entries [num_plus, num_seeds); wave `part` of `parts`.
__device__ __forceinline__ void sa_masks(const SaSeed* seeds, int num_plus, int num_seeds, int part, int parts,
                                         int64_t block0, uint32_t tensor, uint32_t draw,
                                         uint64_t (&acc)[2 * kSaBlocks]) {
  sa_seeds<false>(seeds, part, num_plus, parts, block0, tensor, draw, acc);
  sa_seeds<true>(seeds, num_plus + part, num_seeds, parts, block0, tensor, draw, acc);
}

// The waves' partial accumulators of a shared tile meet in LDS; wave w leaves with the sums of
// block w of every lane in acc[0], acc[1].
__device__ __forceinline__ void sa_combine(u64x2 (&sm)[kSaWaves][kSaBlocks][64], int wave, int lane,
                                           uint64_t (&acc)[2 * kSaBlocks]) {
#pragma unroll
  for (int k = 0; k < kSaBlocks; ++k) {
    const u64x2 v = {acc[2 * k], acc[2 * k + 1]};
    sm[wave][k][lane] = v;
  }
  __syncthreads();
  u64x2 s = sm[0][wave][lane];
#pragma unroll
  for (int w = 1; w < kSaWaves; ++w) s += sm[w][wave][lane];
  acc[0] = s[0];
  acc[1] = s[1];
}

// `have` (0, 1 or 2) ring words at p[e]: one 16-byte access where `vec` says the storage allows it
__device__ __forceinline__ u64x2 sa_load_words(const uint64_t* p, int64_t e, int have, bool vec) {
  const uint64_t FEDAVG_AS_GLOBAL* q = (const uint64_t FEDAVG_AS_GLOBAL*)p + e;
  u64x2 v = {0u, 0u};
  if (have == 2 && vec) {
    v = __builtin_nontemporal_load((const u64x2 FEDAVG_AS_GLOBAL*)q);
  } else {
    if (have > 0) v[0] = __builtin_nontemporal_load(q);
    if (have > 1) v[1] = __builtin_nontemporal_load(q + 1);
  }
  return v;
}

__device__ __forceinline__ void sa_store_words(uint64_t* p, int64_t e, int have, bool vec, const u64x2& v) {
  uint64_t FEDAVG_AS_GLOBAL* q = (uint64_t FEDAVG_AS_GLOBAL*)p + e;
  if (have == 2 && vec) {
    *(u64x2 FEDAVG_AS_GLOBAL*)q = v;
  } else {
    if (have > 0) q[0] = v[0];
    if (have > 1) q[1] = v[1];
  }
}

// ---------------------------------------------------------------------------------------
// the client side
// ---------------------------------------------------------------------------------------
struct SaTensor {
  const void* in;
  uint64_t* out;
};

struct SaMaskArgs {
  const Span* tiles;         // the tiles of every tensor, in list order
  const SaTensor* tensors;   // [T]
  const SaSeed* seeds;       // [num_seeds]: the added entries, then the subtracted ones
  uint32_t* flag;            // the context's NaN words (0 acc, 1 result, 2 input)
  int64_t num_tiles;
  double scale;              // 2^frac_bits
  double limit;              // 2^value_bits
  uint32_t weight;
  uint32_t draw;
  int32_t num_plus;
  int32_t num_seeds;
};

// q = (uint64)(int64)rint(x * 2^f) * w mod 2^64; out of range (not finite, or |r| >= 2^value_bits): `bad`
__device__ __forceinline__ uint64_t sa_encode(double x, double scale, double limit, uint32_t w, bool& bad) {
  const double r = __builtin_rint(x * scale);  // the scaling is exact; to nearest, ties to even
  const bool ok = __builtin_fabs(r) < limit;   // false for a NaN and for an infinity
  bad |= !ok;
  const int64_t i = static_cast<int64_t>(ok ? r : 0.0);
  return static_cast<uint64_t>(i) * w;
}

// Block `j` of the tile (elements 2 j, 2 j + 1 of it): encode, add the masks, store.
template <typename T>
__device__ __forceinline__ bool sa_mask_finish(const SaMaskArgs& a, const void* in, uint64_t* out, int64_t start,
                                               int count, int j, uint64_t even, uint64_t odd) {
  const int left = count - 2 * j;
  const int have = left < 0 ? 0 : (left > 2 ? 2 : left);
  bool bad = false;
  if (have > 0) {
    const int64_t e = start + 2 * j;
    const u32x4 raw = load_guarded<T>(in, e, have);  // past `have`: +0.0, never stored
    u64x2 y;
    y[0] = sa_encode(Format<T>::value(raw, 0), a.scale, a.limit, a.weight, bad) + even;
    y[1] = sa_encode(Format<T>::value(raw, 1), a.scale, a.limit, a.weight, bad) + odd;
    sa_store_words(out, e, have, (reinterpret_cast<uintptr_t>(out) & 15u) == 0, y);
  }
  return bad;
}

// kShare false: wave w of workgroup b owns tile 4 b + w. kShare true: workgroup b owns tile b.
template <typename T, bool kShare>
__global__ __launch_bounds__(kSaThreads) void secagg_mask_kernel(SaMaskArgs a) {
  __shared__ u64x2 sm[kShare ? kSaWaves : 1][kSaBlocks][64];
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t tile = kShare ? static_cast<int64_t>(blockIdx.x) : static_cast<int64_t>(blockIdx.x) * kSaWaves + wave;
  if (tile >= a.num_tiles) return;  // the same for the whole wave; only the shared tile has a barrier
  const Span FEDAVG_AS_CONST* pp = (const Span FEDAVG_AS_CONST*)(a.tiles + tile);
  const int32_t seg = pp->seg, count = pp->count;
  const int64_t start = pp->start;  // a multiple of kSaTile: the tile's first block is start / 2
  const SaTensor FEDAVG_AS_CONST* tp = (const SaTensor FEDAVG_AS_CONST*)(a.tensors + seg);
  const void* const in = tp->in;
  uint64_t* const out = tp->out;
  uint64_t acc[2 * kSaBlocks] = {};
  sa_masks(a.seeds, a.num_plus, a.num_seeds, kShare ? wave : 0, kShare ? kSaWaves : 1, start / 2 + lane,
           static_cast<uint32_t>(seg), a.draw, acc);
  bool bad = false;
  if constexpr (kShare) {
    sa_combine(sm, wave, lane, acc);
    bad = sa_mask_finish<T>(a, in, out, start, count, 64 * wave + lane, acc[0], acc[1]);
  } else {
#pragma unroll
    for (int k = 0; k < kSaBlocks; ++k)
      bad |= sa_mask_finish<T>(a, in, out, start, count, 64 * k + lane, acc[2 * k], acc[2 * k + 1]);
  }
  if (__ballot(bad) != 0ull && lane == 0) raise_flag(a.flag, 2);
}

// ---------------------------------------------------------------------------------------
// the server side
// ---------------------------------------------------------------------------------------
struct SaUnmaskArgs {
  const Span* tiles;                 // the tiles of the context's layout
  const uint64_t* const* clients;    // [n][num_segments]
  const double* const* base;         // [num_segments], or NULL
  void* const* outs;                 // [num_segments]
  const SaSeed* seeds;
  uint32_t* flag;
  int64_t num_tiles;
  double inv_scale;                  // 2^-frac_bits
  double W;
  int32_t num_segments;
  int32_t n;
  int32_t num_plus;
  int32_t num_seeds;
  uint32_t draw;
  uint32_t pad_;
};

// The masked words of clients first, first + step, ... below n, added to the lane's accumulators,
// kSaLoads clients' vectors in flight.
__device__ __forceinline__ void sa_clients(const SaUnmaskArgs& a, int seg, int first, int step, int64_t start,
                                           int count, int lane, uint64_t (&acc)[2 * kSaBlocks]) {
  const uint64_t* const FEDAVG_AS_CONST* table = (const uint64_t* const FEDAVG_AS_CONST*)a.clients;
#pragma unroll 1
  for (int i0 = first; i0 < a.n; i0 += step * kSaLoads) {
    u64x2 v[kSaLoads][kSaBlocks];
#pragma unroll
    for (int u = 0; u < kSaLoads; ++u) {
      const int i = i0 + u * step;
      const bool live = i < a.n;
      const uint64_t* const p = live ? table[static_cast<int64_t>(i) * a.num_segments + seg] : nullptr;
      const bool vec = (reinterpret_cast<uintptr_t>(p) & 15u) == 0;
#pragma unroll
      for (int k = 0; k < kSaBlocks; ++k) {
        const int j = 64 * k + lane;
        const int left = count - 2 * j;
        const int have = !live || left < 0 ? 0 : (left > 2 ? 2 : left);
        v[u][k] = sa_load_words(p, start + 2 * j, have, vec);
      }
    }
#pragma unroll
    for (int u = 0; u < kSaLoads; ++u) {
#pragma unroll
      for (int k = 0; k < kSaBlocks; ++k) {
        acc[2 * k] += v[u][k][0];
        acc[2 * k + 1] += v[u][k][1];
      }
    }
  }
}

// Block `j` of the tile: decode the two sums, divide, add the base, store. Returns the flags to
// latch: bit 0 a NaN quotient, bit 1 a NaN in the base.
template <typename O>
__device__ __forceinline__ int sa_unmask_finish(const SaUnmaskArgs& a, const double* base, void* out, int64_t start,
                                                int count, int j, uint64_t even, uint64_t odd) {
  const int left = count - 2 * j;
  const int have = left < 0 ? 0 : (left > 2 ? 2 : left);
  if (have == 0) return 0;
  const int64_t e = start + 2 * j;
  const uint64_t S[2] = {even, odd};
  double b[2];
  load_f64<2>(b, base, e, have, (reinterpret_cast<uintptr_t>(base) & 15u) == 0);
  double o[2];
  int bad = 0;
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const double v = static_cast<double>(static_cast<int64_t>(S[i]));  // one rounding to nearest even
    const double g = (v * a.inv_scale) / a.W;
    if (i < have && g != g) bad |= 1;
    if (i < have && b[i] != b[i]) bad |= 2;
    o[i] = base != nullptr ? b[i] + g : g;
  }
  if constexpr (sizeof(O) == 8) {
    double FEDAVG_AS_GLOBAL* q = (double FEDAVG_AS_GLOBAL*)out + e;
    if (have == 2 && (reinterpret_cast<uintptr_t>(out) & 15u) == 0) {
      const f64x2 w = {o[0], o[1]};
      *(f64x2 FEDAVG_AS_GLOBAL*)q = w;
    } else {
      q[0] = o[0];
      if (have > 1) q[1] = o[1];
    }
  } else {
    float FEDAVG_AS_GLOBAL* q = (float FEDAVG_AS_GLOBAL*)out + e;
    if (have == 2 && (reinterpret_cast<uintptr_t>(out) & 7u) == 0) {
      const f32x2 w = {static_cast<float>(o[0]), static_cast<float>(o[1])};
      *(f32x2 FEDAVG_AS_GLOBAL*)q = w;
    } else {
      q[0] = static_cast<float>(o[0]);
      if (have > 1) q[1] = static_cast<float>(o[1]);
    }
  }
  return bad;
}

template <typename O, bool kShare>
__global__ __launch_bounds__(kSaThreads) void secagg_unmask_kernel(SaUnmaskArgs a) {
  __shared__ u64x2 sm[kShare ? kSaWaves : 1][kSaBlocks][64];
  const int lane = static_cast<int>(threadIdx.x) & 63;
  const int wave = __builtin_amdgcn_readfirstlane(static_cast<int>(threadIdx.x) >> 6);
  const int64_t tile = kShare ? static_cast<int64_t>(blockIdx.x) : static_cast<int64_t>(blockIdx.x) * kSaWaves + wave;
  if (tile >= a.num_tiles) return;  // the same for the whole wave; only the shared tile has a barrier
  const Span FEDAVG_AS_CONST* pp = (const Span FEDAVG_AS_CONST*)(a.tiles + tile);
  const int32_t seg = pp->seg, count = pp->count;
  const int64_t start = pp->start;
  const double* const base =
      a.base != nullptr ? ((const double* const FEDAVG_AS_CONST*)a.base)[seg] : nullptr;
  void* const out = ((void* const FEDAVG_AS_CONST*)a.outs)[seg];
  const int part = kShare ? wave : 0, parts = kShare ? kSaWaves : 1;
  uint64_t acc[2 * kSaBlocks] = {};
  sa_clients(a, seg, part, parts, start, count, lane, acc);
  sa_masks(a.seeds, a.num_plus, a.num_seeds, part, parts, start / 2 + lane, static_cast<uint32_t>(seg), a.draw, acc);
  int bad = 0;
  if constexpr (kShare) {
    sa_combine(sm, wave, lane, acc);
    bad = sa_unmask_finish<O>(a, base, out, start, count, 64 * wave + lane, acc[0], acc[1]);
  } else {
#pragma unroll
    for (int k = 0; k < kSaBlocks; ++k)
      bad |= sa_unmask_finish<O>(a, base, out, start, count, 64 * k + lane, acc[2 * k], acc[2 * k + 1]);
  }
  if (__ballot((bad & 1) != 0) != 0ull && lane == 0) raise_flag(a.flag, 1);
  if (__ballot((bad & 2) != 0) != 0ull && lane == 0) raise_flag(a.flag, 2);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct SecaggState {
  Span* d_tiles = nullptr;  // unmask's tiles of the context's layout
  int64_t num_tiles = 0;
  TableRing ring;
  ~SecaggState() {
    ring.release();
    if (d_tiles) (void)hipFree(d_tiles);
  }
};

int32_t ensure_state(void** slot, SecaggState** out) {
  if (*slot == nullptr) {
    SecaggState* st = new SecaggState();
    const int32_t r = hip_status("secagg state", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<SecaggState*>(*slot);
  return FEDAVG_OK;
}

size_t align16(size_t n) { return (n + 15) & ~static_cast<size_t>(15); }

int32_t check_seeds(const uint64_t* seeds, const int32_t* signs, int32_t num_seeds, int32_t least) {
  if (num_seeds < least || num_seeds > kSaMaxSeeds)
    return invalid("the seed table holds between " + std::to_string(least) + " and " + std::to_string(kSaMaxSeeds) +
                   " entries");
  if (num_seeds > 0 && (seeds == nullptr || signs == nullptr)) return invalid("null seed or sign table");
  for (int32_t s = 0; s < num_seeds; ++s)
    if (signs[s] != 1 && signs[s] != -1) return invalid("seed entry " + std::to_string(s) + ": the sign is +1 or -1");
  return FEDAVG_OK;
}

// The device image of the seed table: the added entries first. Returns their count.
int32_t sort_seeds(const uint64_t* seeds, const int32_t* signs, int32_t num_seeds, SaSeed* dst) {
  int32_t k = 0, plus = 0;
  for (int pass = 0; pass < 2; ++pass) {
    for (int32_t s = 0; s < num_seeds; ++s)
      if ((signs[s] > 0) == (pass == 0))
        dst[k++] = SaSeed{static_cast<uint32_t>(seeds[s]), static_cast<uint32_t>(seeds[s] >> 32)};
    if (pass == 0) plus = k;
  }
  return plus;
}

// a shared tile per workgroup, or one tile per wave
unsigned grid_of(bool share, int64_t tiles) {
  return static_cast<unsigned>(share ? tiles : (tiles + kSaWaves - 1) / kSaWaves);
}

template <typename T>
void launch_mask(bool share, hipStream_t s, const SaMaskArgs& a) {
  const dim3 grid(grid_of(share, a.num_tiles)), block(kSaThreads);
  if (share) hipLaunchKernelGGL((secagg_mask_kernel<T, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((secagg_mask_kernel<T, false>), grid, block, 0, s, a);
}

template <typename O>
void launch_unmask(bool share, hipStream_t s, const SaUnmaskArgs& a) {
  const dim3 grid(grid_of(share, a.num_tiles)), block(kSaThreads);
  if (share) hipLaunchKernelGGL((secagg_unmask_kernel<O, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((secagg_unmask_kernel<O, false>), grid, block, 0, s, a);
}

}  // namespace

int32_t fedavg_internal_secagg_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "secagg_tile") *out = kSaTile;
  else if (n == "secagg_blocks") *out = kSaBlocks;
  else if (n == "secagg_loads") *out = kSaLoads;
  else if (n == "secagg_split") *out = kSaSplit;
  else if (n == "secagg_threads") *out = kSaThreads;
  else if (n == "secagg_max_seeds") *out = kSaMaxSeeds;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_secagg_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<SecaggState*>(state);
}

extern "C" int32_t fedavg_secagg_mask(fedavg_ctx* ctx, int32_t dtype, const void* const* in_ptrs,
                                      const int64_t* numels, int32_t num_tensors, int64_t weight, int32_t frac_bits,
                                      int32_t value_bits, uint32_t draw, const uint64_t* seeds, const int32_t* signs,
                                      int32_t num_seeds, void* const* out_ptrs, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_SECAGG, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (dtype != FEDAVG_F32 && dtype != FEDAVG_F16 && dtype != FEDAVG_BF16 && dtype != FEDAVG_F64)
    return invalid("the masking step takes fp32, fp16, bf16 or fp64 tensors");
  if (in_ptrs == nullptr || numels == nullptr || out_ptrs == nullptr) return invalid("null input, count or output table");
  if (num_tensors < 1 || num_tensors > kSaMaxTensors)
    return invalid("the masking step takes between 1 and " + std::to_string(kSaMaxTensors) + " tensors");
  if (weight < 0 || weight >= (int64_t(1) << 31)) return invalid("the weight is an integer in 0 .. 2^31 - 1");
  if (frac_bits < 0 || frac_bits > 52) return invalid("frac_bits is in 0 .. 52");
  if (value_bits < 1 || value_bits > 62) return invalid("value_bits is in 1 .. 62");
  FEDAVG_TRY(check_seeds(seeds, signs, num_seeds, 1));
  const int T = num_tensors;
  const size_t esize = dtype == FEDAVG_F64 ? 8 : (dtype == FEDAVG_F32 ? 4 : 2);
  uint64_t num_tiles = 0;
  for (int t = 0; t < T; ++t) {
    const std::string who = "tensor " + std::to_string(t);
    if (numels[t] < 1) return invalid(who + ": no elements");
    if (numels[t] > 0x7fffffffll) return invalid(who + ": more than 2^31 - 1 elements");
    if (in_ptrs[t] == nullptr || out_ptrs[t] == nullptr) return invalid(who + ": null input or output buffer");
    if (misaligned(in_ptrs[t], esize)) return invalid(who + ": the input is not aligned to its element size");
    if (misaligned(out_ptrs[t], 8)) return invalid(who + ": the output is not 8-byte aligned");
    if (in_ptrs[t] == static_cast<const void*>(out_ptrs[t])) return invalid(who + ": the output is its input");
    num_tiles += (static_cast<uint64_t>(numels[t]) + kSaTile - 1) / kSaTile;
  }
  if (num_tiles > 0x7fffffffull) return invalid("layout too large for one masking call");

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  SecaggState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: the tiles, one SaTensor per tensor, the seeds
  const size_t tile_bytes = align16(sizeof(Span) * num_tiles);
  const size_t tensor_bytes = align16(sizeof(SaTensor) * static_cast<size_t>(T));
  const size_t bytes = tile_bytes + tensor_bytes + align16(sizeof(SaSeed) * static_cast<size_t>(num_seeds));
  // `next` advances only once work that reads this slot has been enqueued and its event recorded
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memset(sl.host, 0, bytes);
  Span* const h_tiles = reinterpret_cast<Span*>(sl.host);
  SaTensor* const h_tensors = reinterpret_cast<SaTensor*>(sl.host + tile_bytes);
  size_t k = 0;
  for (int t = 0; t < T; ++t) {
    h_tensors[t] = SaTensor{in_ptrs[t], static_cast<uint64_t*>(out_ptrs[t])};
    for (int64_t b = 0; b < numels[t]; b += kSaTile) {
      const int64_t left = numels[t] - b;
      h_tiles[k++] = Span{t, static_cast<int32_t>(left < kSaTile ? left : kSaTile), b};
    }
  }
  const int32_t plus = sort_seeds(seeds, signs, num_seeds, reinterpret_cast<SaSeed*>(sl.host + tile_bytes + tensor_bytes));
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  SaMaskArgs a;
  a.tiles = reinterpret_cast<const Span*>(sl.dev);
  a.tensors = reinterpret_cast<const SaTensor*>(sl.dev + tile_bytes);
  a.seeds = reinterpret_cast<const SaSeed*>(sl.dev + tile_bytes + tensor_bytes);
  a.flag = v.d_flag;
  a.num_tiles = static_cast<int64_t>(num_tiles);
  a.scale = std::ldexp(1.0, frac_bits);
  a.limit = std::ldexp(1.0, value_bits);
  a.weight = static_cast<uint32_t>(weight);
  a.draw = draw;
  a.num_plus = plus;
  a.num_seeds = num_seeds;
  const bool share = num_seeds >= kSaSplit;
  if (dtype == FEDAVG_F32) launch_mask<float>(share, s, a);
  else if (dtype == FEDAVG_F16) launch_mask<__half>(share, s, a);
  else if (dtype == FEDAVG_BF16) launch_mask<bf16_t>(share, s, a);
  else launch_mask<double>(share, s, a);
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("secagg mask launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}

extern "C" int32_t fedavg_secagg_unmask(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t num_clients,
                                        const uint64_t* seeds, const int32_t* signs, int32_t num_seeds, uint32_t draw,
                                        int32_t frac_bits, double total_weight, const double* const* base_ptrs,
                                        void* const* out_ptrs, int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rs = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_SECAGG, &slot);
  if (rs != FEDAVG_OK) return rs;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("the unmasking step writes fp32 or fp64");
  if (client_ptrs == nullptr || out_ptrs == nullptr) return invalid("null client table or outputs");
  if (num_clients < 1) return invalid("empty client table");
  if (num_clients > kSaMaxClients)
    return invalid(std::to_string(num_clients) + " clients: the unmasking step takes at most " +
                   std::to_string(kSaMaxClients));
  if (frac_bits < 0 || frac_bits > 52) return invalid("frac_bits is in 0 .. 52");
  if (!(total_weight >= 0 && std::isfinite(total_weight))) return invalid("the total weight is finite and >= 0");
  FEDAVG_TRY(check_seeds(seeds, signs, num_seeds, 0));
  const int T = v.num_segments;
  const size_t out_bytes = out_dtype == FEDAVG_F64 ? 8 : 4;
  const size_t entries = static_cast<size_t>(num_clients) * static_cast<size_t>(T);
  for (int t = 0; t < T; ++t) {
    if (out_ptrs[t] == nullptr) return invalid("null output pointer for segment " + std::to_string(t));
    if (misaligned(out_ptrs[t], out_bytes)) return invalid("output tensor not aligned to its element size");
    if (base_ptrs != nullptr) {
      if (base_ptrs[t] == nullptr) return invalid("the base lacks segment " + std::to_string(t));
      if (misaligned(base_ptrs[t], 8)) return invalid("base tensor not aligned to fp64");
      if (static_cast<const void*>(out_ptrs[t]) == static_cast<const void*>(base_ptrs[t]))
        return invalid("segment " + std::to_string(t) + ": the output is its base");
    }
  }
  for (size_t i = 0; i < entries; ++i) {
    // the message is built only on a refusal: this loop runs n * T times on every call
    const auto where = [T, i] { return "client " + std::to_string(i / T) + ", segment " + std::to_string(i % T); };
    if (client_ptrs[i] == nullptr) return invalid(where() + ": null tensor (a masked update is whole)");
    if (misaligned(client_ptrs[i], 8)) return invalid(where() + ": the masked words are not 8-byte aligned");
    if (client_ptrs[i] == static_cast<const void*>(out_ptrs[i % T])) return invalid(where() + ": the output is a client");
  }

  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  SecaggState* st = nullptr;
  const int32_t re = ensure_state(slot, &st);
  if (re != FEDAVG_OK) return re;
  if (st->d_tiles == nullptr)
    FEDAVG_TRY(span_table(v.seg_numel, v.num_segments, kSaTile, "secagg launch", "secagg tile table", &st->d_tiles,
                          &st->num_tiles));
  hipStream_t s = static_cast<hipStream_t>(stream);

  // the call's tables: [n][T] client pointers, [T] base pointers, [T] output pointers, the seeds
  const size_t ptr_bytes = sizeof(void*) * entries;
  const size_t seg_bytes = sizeof(void*) * static_cast<size_t>(T);
  const size_t o_base = ptr_bytes, o_out = o_base + seg_bytes, o_seed = align16(o_out + seg_bytes);
  const size_t bytes = o_seed + align16(sizeof(SaSeed) * static_cast<size_t>(num_seeds));
  TableRing::Slot* slp = nullptr;
  FEDAVG_TRY(st->ring.peek(bytes, &slp));
  TableRing::Slot& sl = *slp;
  std::memcpy(sl.host, client_ptrs, ptr_bytes);
  if (base_ptrs != nullptr) std::memcpy(sl.host + o_base, base_ptrs, seg_bytes);
  else std::memset(sl.host + o_base, 0, seg_bytes);
  std::memcpy(sl.host + o_out, out_ptrs, seg_bytes);
  const int32_t plus = sort_seeds(seeds, signs, num_seeds, reinterpret_cast<SaSeed*>(sl.host + o_seed));
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));

  SaUnmaskArgs a;
  a.tiles = st->d_tiles;
  a.clients = reinterpret_cast<const uint64_t* const*>(sl.dev);
  a.base = base_ptrs != nullptr ? reinterpret_cast<const double* const*>(sl.dev + o_base) : nullptr;
  a.outs = reinterpret_cast<void* const*>(sl.dev + o_out);
  a.seeds = reinterpret_cast<const SaSeed*>(sl.dev + o_seed);
  a.flag = v.d_flag;
  a.num_tiles = st->num_tiles;
  a.inv_scale = std::ldexp(1.0, -frac_bits);
  a.W = total_weight;
  a.num_segments = T;
  a.n = num_clients;
  a.num_plus = plus;
  a.num_seeds = num_seeds;
  a.draw = draw;
  a.pad_ = 0;
  const bool share = num_seeds >= kSaSplit;
  if (st->num_tiles > 0) {
    if (out_dtype == FEDAVG_F32) launch_unmask<float>(share, s, a);
    else launch_unmask<double>(share, s, a);
  }
  hipError_t e = hipGetLastError();
  const hipError_t er = st->ring.commit(sl, s);
  if (e == hipSuccess) e = er;
  if (e != hipSuccess)
    return fedavg_internal_fail(FEDAVG_ERR_HIP, (std::string("secagg unmask launch: ") + hipGetErrorString(e)).c_str());
  return FEDAVG_OK;
}
