// robust_kernels.hip — gfx950 (MI355X) kernels of the coordinate-wise trimmed mean and median
// (fedavg_robust_aggregate, include/fedavg_hip.h). Not an algorithm of the reference: the
// contract is DESIGN.md "Robust rules" and tests/robust_reference.py restates it in torch.
//
// Unlike the weighted mean these rules need an element's n client values together, so this is
// not a variant of the fold: every lane keeps the n values of its elements in registers as
// order-preserving integer keys and sorts them with a compile-time sorting network.
//   * A segment is cut into tiles of kRobustTile elements; one 64-lane workgroup owns a tile and
//     walks it in passes of 64 x 16 bytes. Per pass a lane issues one 16-byte load per client
//     (all of them before the network starts) and parks the raw words in LDS — 64 clients x 16
//     bytes would not fit the register file next to the keys — then sorts its elements one after
//     the other, each with its n keys in registers.
//   * Key: the sign-flip map of the value's bits (negative: all bits inverted, else the sign bit
//     set), which orders -inf < ... < -0.0 < +0.0 < ... < +inf as unsigned integers. fp32 / fp16 /
//     bf16 values are widened exactly to fp32 and sort as 32-bit keys, fp64 as 64-bit keys.
//   * The network is Batcher's odd-even merge sort for NPAD in {2, 4, ..., 64} slots, generated at
//     compile time; every register index is a constant, so nothing lives in scratch. Slots past
//     the segment's n hold the maximum key and sort to the end.
//   * The kept range [k, n - k) is runtime per segment: the sum starts at s_k and adds s_j in
//     ascending order under wave-uniform predicates over the unrolled index — never a zero in a
//     dropped value's place (-0.0 + 0.0 would flip a sign). Then one IEEE division by n - 2k.
//   * NaN: negative NaNs sort below -inf and positive ones above +inf, so s_0 and s_{n-1} tell
//     whether any input was NaN; the result's NaN check is one compare. Both latch the context's
//     host-coherent flag words.
// mam_tile_kernel (fedavg_mean_around_median; tests/bulyan_reference.py) shares the
// staging, the keys and the network and differs after the sort: see the comment above it.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "call_tables.h"
#include "device_common.h"

namespace {

constexpr int kRobustLanes = 64;                           // one wave per workgroup
constexpr int kRobustTile = 512;                           // elements per tile (all dtypes)
constexpr int kRobustMaxClients = FEDAVG_ROBUST_MAX_CLIENTS;  // the widest network


struct RSeg {      // one segment of a call
  void* out;
  int32_t first;   // index of the segment's first client pointer in the dense pointer list
  int32_t n;       // clients that sent the segment
  int32_t k;       // values dropped at each end (mam_tile_kernel: beta, the values averaged)
  int32_t vec;     // every client pointer and the output are 16-byte aligned
  int64_t pad_;
};

struct RArgs {
  const Span* tiles;
  const RSeg* segs;
  const void* const* ptrs;  // per segment n dense client pointers (missing clients compacted away)
  uint32_t* flag;
  int32_t out_f32;
};

// the loop bodies below are lambdas over a compile-time index; they must be inlined for the
// register arrays they touch to stay registers
#define ROBUST_INLINE __attribute__((always_inline))

// ---------------------------------------------------------------------------------------
// compile-time loops and the sorting network
// ---------------------------------------------------------------------------------------
template <typename F, size_t... I>
__device__ __forceinline__ void static_for_impl(F&& f, std::index_sequence<I...>) {
  const int d[] = {(f(std::integral_constant<int, static_cast<int>(I)>{}), 0)...};
  (void)d;
}
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(static_cast<F&&>(f), std::make_index_sequence<N>{});
}

constexpr int ilog2(int n) { return n <= 1 ? 0 : 1 + ilog2(n / 2); }

// Batcher's odd-even merge sort on N = 2^p slots as a list of compare-exchanges (a[i] < b[i],
// minimum to slot a[i]): 1 / 3 / 19 / 63 / 191 / 543 of them for N = 2 ... 64.
template <int N>
struct Network {
  static constexpr int kCap = N * ilog2(N) * (ilog2(N) + 1) / 4 + 1;
  int a[kCap] = {};
  int b[kCap] = {};
  int count = 0;
};

template <int N>
constexpr Network<N> make_network() {
  Network<N> net;
  for (int p = 1; p < N; p <<= 1) {
    for (int k = p; k >= 1; k >>= 1) {
      for (int j = k % p; j <= N - 1 - k; j += 2 * k) {
        const int lim = (k - 1 < N - j - k - 1) ? k - 1 : N - j - k - 1;
        for (int i = 0; i <= lim; ++i) {
          if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
            net.a[net.count] = i + j;
            net.b[net.count] = i + j + k;
            ++net.count;
          }
        }
      }
    }
  }
  return net;
}

template <int N>
struct NetworkOf {
  static constexpr Network<N> value = make_network<N>();
};

template <int A, int B, typename K, int N>
__device__ __forceinline__ void compare_exchange(K (&s)[N]) {
  const K x = s[A], y = s[B];
  const bool swap = y < x;
  s[A] = swap ? y : x;  // v_min_u32 / v_max_u32 for 32-bit keys
  s[B] = swap ? x : y;
}

template <int N, typename K, size_t... I>
__device__ __forceinline__ void sort_impl(K (&s)[N], std::index_sequence<I...>) {
  const int d[] = {(compare_exchange<NetworkOf<N>::value.a[I], NetworkOf<N>::value.b[I]>(s), 0)...};
  (void)d;
}
template <int N, typename K>
__device__ __forceinline__ void sort_network(K (&s)[N]) {
  sort_impl<N>(s, std::make_index_sequence<NetworkOf<N>::value.count>{});
}

// ---------------------------------------------------------------------------------------
// input formats: a client's 16 staged bytes -> keys, keys -> fp64 values
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t key32(uint32_t bits) {
  const uint32_t m = static_cast<uint32_t>(static_cast<int32_t>(bits) >> 31);
  return bits ^ (m | 0x80000000u);
}
__device__ __forceinline__ uint32_t bits32(uint32_t key) {
  const uint32_t m = static_cast<uint32_t>(static_cast<int32_t>(key) >> 31);
  return key ^ (~m | 0x80000000u);
}
__device__ __forceinline__ uint64_t key64(uint64_t bits) {
  const uint64_t m = static_cast<uint64_t>(static_cast<int64_t>(bits) >> 63);
  return bits ^ (m | 0x8000000000000000ull);
}
__device__ __forceinline__ uint64_t bits64(uint64_t key) {
  const uint64_t m = static_cast<uint64_t>(static_cast<int64_t>(key) >> 63);
  return key ^ (~m | 0x8000000000000000ull);
}

template <typename K>
struct KeyLimits;
template <>
struct KeyLimits<uint32_t> {
  static constexpr uint32_t kMax = 0xffffffffu;
  static constexpr uint32_t kNegInf = 0x007fffffu;  // key32(0xff800000)
  static constexpr uint32_t kPosInf = 0xff800000u;  // key32(0x7f800000)
  __device__ __forceinline__ static double value(uint32_t key) {
    return static_cast<double>(__uint_as_float(bits32(key)));
  }
};
template <>
struct KeyLimits<uint64_t> {
  static constexpr uint64_t kMax = 0xffffffffffffffffull;
  static constexpr uint64_t kNegInf = 0x000fffffffffffffull;
  static constexpr uint64_t kPosInf = 0xfff0000000000000ull;
  __device__ __forceinline__ static double value(uint64_t key) {
    return __longlong_as_double(static_cast<long long>(bits64(key)));
  }
};

template <typename T>
struct KeyFormat;
template <>
struct KeyFormat<float> {
  using Key = uint32_t;
  static constexpr int N = 4;
  template <int J>
  __device__ __forceinline__ static Key key(const uint32_t* col, int e) {
    return key32(col[(J * 4 + e) * kRobustLanes]);
  }
};
template <>
struct KeyFormat<__half> {
  using Key = uint32_t;
  static constexpr int N = 8;
  template <int J>
  __device__ __forceinline__ static Key key(const uint32_t* col, int e) {
    const uint32_t h = (col[(J * 4 + e / 2) * kRobustLanes] >> (16 * (e % 2))) & 0xffffu;
    return key32(__float_as_uint(__half2float(__ushort_as_half(static_cast<unsigned short>(h)))));
  }
};
template <>
struct KeyFormat<bf16_t> {
  using Key = uint32_t;
  static constexpr int N = 8;
  template <int J>
  __device__ __forceinline__ static Key key(const uint32_t* col, int e) {
    const uint32_t w = col[(J * 4 + e / 2) * kRobustLanes];
    return key32((w >> (16 * (e % 2))) << 16);
  }
};
template <>
struct KeyFormat<double> {
  using Key = uint64_t;
  static constexpr int N = 2;
  template <int J>
  __device__ __forceinline__ static Key key(const uint32_t* col, int e) {
    const uint64_t lo = col[(J * 4 + 2 * e) * kRobustLanes], hi = col[(J * 4 + 2 * e + 1) * kRobustLanes];
    return key64(lo | (hi << 32));
  }
};

template <typename O, int N>
__device__ __forceinline__ void store_results(void* out, int64_t elem, const double (&res)[N], bool vec, int have) {
  O FEDAVG_AS_GLOBAL* o = (O FEDAVG_AS_GLOBAL*)out + elem;
  if (vec) {
    if constexpr (sizeof(O) == 8) {
#pragma unroll
      for (int i = 0; i < N; i += 2) {
        f64x2 v = {res[i], res[i + 1]};
        __builtin_nontemporal_store(v, (f64x2 FEDAVG_AS_GLOBAL*)(o + i));
      }
    } else if constexpr (N >= 4) {
#pragma unroll
      for (int i = 0; i < N; i += 4) {
        f32x4 v = {static_cast<float>(res[i]), static_cast<float>(res[i + 1]), static_cast<float>(res[i + 2]),
                   static_cast<float>(res[i + 3])};
        __builtin_nontemporal_store(v, (f32x4 FEDAVG_AS_GLOBAL*)(o + i));
      }
    } else {
      f32x2 v = {static_cast<float>(res[0]), static_cast<float>(res[1])};
      __builtin_nontemporal_store(v, (f32x2 FEDAVG_AS_GLOBAL*)o);
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i < have) o[i] = static_cast<O>(res[i]);
    }
  }
}

// ---------------------------------------------------------------------------------------
// the kernel: one tile per workgroup, NPAD >= the launch's largest client count
// ---------------------------------------------------------------------------------------
template <typename T, int NPAD>
__global__ __attribute__((amdgpu_flat_work_group_size(kRobustLanes, kRobustLanes))) void robust_tile_kernel(RArgs a) {
  using F = KeyFormat<T>;
  using Key = typename F::Key;
  using L = KeyLimits<Key>;
  constexpr int N = F::N;
  constexpr int kPass = kRobustLanes * N;  // elements per pass
  static_assert(kRobustTile % kPass == 0, "tile geometry");

  // wave-uniform descriptors through the constant address space (scalar loads)
  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg;
  const int32_t count = tp->count;
  const int64_t start = tp->start;
  const RSeg FEDAVG_AS_CONST* sp = (const RSeg FEDAVG_AS_CONST*)(a.segs + seg);
  void* const out = sp->out;
  const int32_t n = sp->n;
  const int32_t k = sp->k;
  const bool seg_vec = sp->vec != 0;
  const void* const FEDAVG_AS_CONST* ptrs = (const void* const FEDAVG_AS_CONST*)(a.ptrs + sp->first);
  const double divisor = static_cast<double>(n - 2 * k);
  const int lane = static_cast<int>(threadIdx.x);

  // The lane's raw words of a pass, word w of client j at col[(j * 4 + w) * 64]: a lane reads
  // back only what it wrote (no barrier), and both directions are conflict-free.
  __shared__ uint32_t stage[NPAD * 4 * kRobustLanes];
  uint32_t* const col = stage + lane;
  __shared__ double results[8 * kRobustLanes];  // a pass's results, element e of a lane at [e * 64]
  double* const rcol = results + lane;
  static_assert(N <= 8, "results staging");
  constexpr int kBatch = NPAD < 16 ? NPAD : 16;

  bool nan_in = false, nan_out = false;
#pragma unroll 1
  for (int base = 0; base < count; base += kPass) {
    const int e0 = base + lane * N;        // the lane's first element of this pass, tile-relative
    const int have = count - e0;           // elements of the tile from there on (may be <= 0)
    const int64_t elem = start + e0;
    // whole 16-byte vectors for every lane of the wave, or the guarded element path for all
    const bool vec = seg_vec && (count - base >= kPass);

    // stage the pass's client vectors in LDS, kBatch loads in flight per lane
    static_for<NPAD / kBatch>([&](auto B) ROBUST_INLINE {
      constexpr int b = decltype(B)::value;
      u32x4 raw[kBatch];
      if (vec) {
        static_for<kBatch>([&](auto I) ROBUST_INLINE {
          constexpr int j = b * kBatch + decltype(I)::value;
          if (j < n) {
            const u32x4 FEDAVG_AS_GLOBAL* p =
                (const u32x4 FEDAVG_AS_GLOBAL*)((const T FEDAVG_AS_GLOBAL*)ptrs[j] + elem);
            raw[j - b * kBatch] = __builtin_nontemporal_load(p);
          }
        });
      } else {
        static_for<kBatch>([&](auto I) ROBUST_INLINE {
          constexpr int j = b * kBatch + decltype(I)::value;
          if (j < n) raw[j - b * kBatch] = load_guarded<T>(ptrs[j], elem, have);
        });
      }
      static_for<kBatch>([&](auto I) ROBUST_INLINE {
        constexpr int j = b * kBatch + decltype(I)::value;
        if (j < n) {
#pragma unroll
          for (int w = 0; w < 4; ++w) col[(j * 4 + w) * kRobustLanes] = raw[j - b * kBatch][w];
        }
      });
      // a batch is parked before the next one's loads issue: hoisted, all NPAD x 4 words would be
      // in registers at once
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    });

    // the words are read back from LDS, not forwarded from the load registers (which would keep
    // all NPAD x 4 of them live through every element's network)
    asm volatile("" ::: "memory");

    // One element after the other, in a loop that is not unrolled: the staged words are addressed
    // by the element at run time, so one copy of the network serves all N and only one element's
    // keys are live. The results wait in LDS for the pass's vector store.
#pragma unroll 1
    for (int e = 0; e < N; ++e) {
      asm volatile("" ::: "memory");
      Key s[NPAD];
      static_for<NPAD>([&](auto J) ROBUST_INLINE {
        constexpr int j = decltype(J)::value;
        s[j] = (j < n) ? F::template key<j>(col, e) : L::kMax;
      });
      sort_network<NPAD>(s);
      // NaNs sort to the ends of the real values: s_0 below -inf or s_{n-1} above +inf
      nan_in |= s[0] < L::kNegInf;
      double sum = 0.0;  // assigned at j == k before it is read
      static_for<NPAD>([&](auto J) ROBUST_INLINE {
        constexpr int j = decltype(J)::value;
        if (j == n - 1) nan_in |= s[j] > L::kPosInf;
        if (j == k) {
          sum = L::value(s[j]);
        } else if (j > k && j < n - k) {
          sum = sum + L::value(s[j]);
        }
      });
      const double r = sum / divisor;
      rcol[e * kRobustLanes] = r;
      nan_out |= r != r;  // elements past the tile's end are zeros here: never NaN
    }
    asm volatile("" ::: "memory");
    double res[N];
#pragma unroll
    for (int e = 0; e < N; ++e) res[e] = rcol[e * kRobustLanes];

    if (a.out_f32) {
      store_results<float, N>(out, elem, res, vec, have);
    } else {
      store_results<double, N>(out, elem, res, vec, have);
    }
  }
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
  if (__ballot(nan_out) != 0ull && lane == 0) raise_flag(a.flag, 1);
}

// ---------------------------------------------------------------------------------------
// mean around the median (fedavg_mean_around_median): the mean of the beta sorted values closest
// to the lower median. The window's start differs from lane to lane, and a register array indexed
// by a lane's value would live in scratch, so after the network the sorted values go back into
// the element's own staged bytes, in the input format (every value came from there, so it is
// representable), and the window is walked in LDS: slot i of a lane is at col[(i * 4 + w) * 64],
// congruent to the lane modulo 64 words whatever i is — no bank conflict for a lane-varying i.
// ---------------------------------------------------------------------------------------
template <typename T>
struct Sorted;  // slot i of element e in the lane's column: put a key's value there / read it as fp64
template <>
struct Sorted<float> {
  __device__ __forceinline__ static void put(uint32_t* col, int i, int e, uint32_t key) {
    col[(i * 4 + e) * kRobustLanes] = bits32(key);
  }
  __device__ __forceinline__ static double get(const uint32_t* col, int i, int e) {
    return static_cast<double>(__uint_as_float(col[(i * 4 + e) * kRobustLanes]));
  }
};
template <>
struct Sorted<__half> {
  __device__ __forceinline__ static void put(uint32_t* col, int i, int e, uint32_t key) {
    // the key is a widened fp16 value: narrowing it is exact; the element's neighbour in the word
    // (not sorted yet, or sorted already) keeps its 16 bits
    const __half h = __float2half(__uint_as_float(bits32(key)));
    reinterpret_cast<uint16_t*>(col + (i * 4 + e / 2) * kRobustLanes)[e % 2] = __half_as_ushort(h);
  }
  __device__ __forceinline__ static double get(const uint32_t* col, int i, int e) {
    const uint16_t h = reinterpret_cast<const uint16_t*>(col + (i * 4 + e / 2) * kRobustLanes)[e % 2];
    return static_cast<double>(__half2float(__ushort_as_half(h)));
  }
};
template <>
struct Sorted<bf16_t> {
  __device__ __forceinline__ static void put(uint32_t* col, int i, int e, uint32_t key) {
    reinterpret_cast<uint16_t*>(col + (i * 4 + e / 2) * kRobustLanes)[e % 2] = static_cast<uint16_t>(bits32(key) >> 16);
  }
  __device__ __forceinline__ static double get(const uint32_t* col, int i, int e) {
    const uint32_t h = reinterpret_cast<const uint16_t*>(col + (i * 4 + e / 2) * kRobustLanes)[e % 2];
    return static_cast<double>(__uint_as_float(h << 16));
  }
};
template <>
struct Sorted<double> {
  __device__ __forceinline__ static void put(uint32_t* col, int i, int e, uint64_t key) {
    const uint64_t b = bits64(key);
    col[(i * 4 + 2 * e) * kRobustLanes] = static_cast<uint32_t>(b);
    col[(i * 4 + 2 * e + 1) * kRobustLanes] = static_cast<uint32_t>(b >> 32);
  }
  __device__ __forceinline__ static double get(const uint32_t* col, int i, int e) {
    const uint64_t lo = col[(i * 4 + 2 * e) * kRobustLanes], hi = col[(i * 4 + 2 * e + 1) * kRobustLanes];
    return __longlong_as_double(static_cast<long long>(lo | (hi << 32)));
  }
};

// One tile per workgroup like robust_tile_kernel, with the same staging; RSeg::k is beta, the
// number of values averaged (1 <= beta <= n).
template <typename T, int NPAD>
__global__ __attribute__((amdgpu_flat_work_group_size(kRobustLanes, kRobustLanes))) void mam_tile_kernel(RArgs a) {
  using F = KeyFormat<T>;
  using Key = typename F::Key;
  using L = KeyLimits<Key>;
  using S = Sorted<T>;
  constexpr int N = F::N;
  constexpr int kPass = kRobustLanes * N;
  static_assert(kRobustTile % kPass == 0, "tile geometry");

  const Span FEDAVG_AS_CONST* tp = (const Span FEDAVG_AS_CONST*)(a.tiles + blockIdx.x);
  const int32_t seg = tp->seg;
  const int32_t count = tp->count;
  const int64_t start = tp->start;
  const RSeg FEDAVG_AS_CONST* sp = (const RSeg FEDAVG_AS_CONST*)(a.segs + seg);
  void* const out = sp->out;
  const int32_t n = sp->n;
  const int32_t beta = sp->k;
  const bool seg_vec = sp->vec != 0;
  const void* const FEDAVG_AS_CONST* ptrs = (const void* const FEDAVG_AS_CONST*)(a.ptrs + sp->first);
  const double divisor = static_cast<double>(beta);
  const int32_t mid = (n - 1) >> 1;  // the lower median's slot
  const int lane = static_cast<int>(threadIdx.x);

  __shared__ uint32_t stage[NPAD * 4 * kRobustLanes];
  uint32_t* const col = stage + lane;
  __shared__ double results[8 * kRobustLanes];
  double* const rcol = results + lane;
  static_assert(N <= 8, "results staging");
  constexpr int kBatch = NPAD < 16 ? NPAD : 16;

  bool nan_in = false, nan_out = false;
#pragma unroll 1
  for (int base = 0; base < count; base += kPass) {
    const int e0 = base + lane * N;
    const int have = count - e0;
    const int64_t elem = start + e0;
    const bool vec = seg_vec && (count - base >= kPass);

    static_for<NPAD / kBatch>([&](auto B) ROBUST_INLINE {
      constexpr int b = decltype(B)::value;
      u32x4 raw[kBatch];
      if (vec) {
        static_for<kBatch>([&](auto I) ROBUST_INLINE {
          constexpr int j = b * kBatch + decltype(I)::value;
          if (j < n) {
            const u32x4 FEDAVG_AS_GLOBAL* p =
                (const u32x4 FEDAVG_AS_GLOBAL*)((const T FEDAVG_AS_GLOBAL*)ptrs[j] + elem);
            raw[j - b * kBatch] = __builtin_nontemporal_load(p);
          }
        });
      } else {
        static_for<kBatch>([&](auto I) ROBUST_INLINE {
          constexpr int j = b * kBatch + decltype(I)::value;
          if (j < n) raw[j - b * kBatch] = load_guarded<T>(ptrs[j], elem, have);
        });
      }
      static_for<kBatch>([&](auto I) ROBUST_INLINE {
        constexpr int j = b * kBatch + decltype(I)::value;
        if (j < n) {
#pragma unroll
          for (int w = 0; w < 4; ++w) col[(j * 4 + w) * kRobustLanes] = raw[j - b * kBatch][w];
        }
      });
      asm volatile("" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
    });
    asm volatile("" ::: "memory");

#pragma unroll 1
    for (int e = 0; e < N; ++e) {
      asm volatile("" ::: "memory");
      Key s[NPAD];
      static_for<NPAD>([&](auto J) ROBUST_INLINE {
        constexpr int j = decltype(J)::value;
        s[j] = (j < n) ? F::template key<j>(col, e) : L::kMax;
      });
      sort_network<NPAD>(s);
      nan_in |= s[0] < L::kNegInf;
      // the sorted values replace the element's raw ones (slots below n only: the lane owns them)
      static_for<NPAD>([&](auto J) ROBUST_INLINE {
        constexpr int j = decltype(J)::value;
        if (j == n - 1) nan_in |= s[j] > L::kPosInf;
        if (j < n) S::put(col, j, e, s[j]);
      });
      asm volatile("" ::: "memory");
      const double med = S::get(col, mid, e);
      // the window's start: the steps t at which the value beta slots up lies closer to the median
      // than s_t (a prefix of t: rounding is monotone). One rounded subtraction on each side; the
      // comparison is false on NaN (inf - inf), and a tie keeps the lower value.
      int32_t first = 0;
#pragma unroll 4
      for (int t = 0; t < n - beta; ++t) {
        const double lo = S::get(col, t, e), hi = S::get(col, t + beta, e);
        first += ((hi - med) < (med - lo)) ? 1 : 0;
      }
      double sum = S::get(col, first, e);  // never a leading zero: -0.0 + 0.0 would flip a sign
#pragma unroll 4
      for (int j = 1; j < beta; ++j) sum = sum + S::get(col, first + j, e);
      const double r = sum / divisor;
      rcol[e * kRobustLanes] = r;
      nan_out |= r != r;  // elements past the tile's end are zeros here: never NaN
    }
    asm volatile("" ::: "memory");
    double res[N];
#pragma unroll
    for (int e = 0; e < N; ++e) res[e] = rcol[e * kRobustLanes];

    if (a.out_f32) {
      store_results<float, N>(out, elem, res, vec, have);
    } else {
      store_results<double, N>(out, elem, res, vec, have);
    }
  }
  if (__ballot(nan_in) != 0ull && lane == 0) raise_flag(a.flag, 2);
  if (__ballot(nan_out) != 0ull && lane == 0) raise_flag(a.flag, 1);
}

// ---------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------
struct RobustState {
  Span* d_tiles = nullptr;
  int64_t num_tiles = 0;
  TableRing ring;  // a call's tables: RSeg[T], then the pointer list
  ~RobustState() {
    if (d_tiles) (void)hipFree(d_tiles);
    ring.release();
  }
};

int32_t ensure_state(const fedavg_robust_view& v, void** slot, RobustState** out) {
  if (*slot == nullptr) {
    RobustState* st = new RobustState();
    int32_t r = span_table(v.seg_numel, v.num_segments, kRobustTile, "robust launch", "robust tile table", &st->d_tiles,
                           &st->num_tiles);
    if (r == FEDAVG_OK) r = hip_status("robust tile table", st->ring.create());
    if (r != FEDAVG_OK) {
      delete st;
      return r;
    }
    *slot = st;
  }
  *out = static_cast<RobustState*>(*slot);
  return FEDAVG_OK;
}

template <typename T>
void launch_npad(int npad, dim3 grid, hipStream_t s, const RArgs& a) {
  const dim3 block(kRobustLanes);
  switch (npad) {
    case 2: hipLaunchKernelGGL((robust_tile_kernel<T, 2>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((robust_tile_kernel<T, 4>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((robust_tile_kernel<T, 8>), grid, block, 0, s, a); break;
    case 16: hipLaunchKernelGGL((robust_tile_kernel<T, 16>), grid, block, 0, s, a); break;
    case 32: hipLaunchKernelGGL((robust_tile_kernel<T, 32>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((robust_tile_kernel<T, 64>), grid, block, 0, s, a); break;
  }
}

template <typename T>
void launch_mam_npad(int npad, dim3 grid, hipStream_t s, const RArgs& a) {
  const dim3 block(kRobustLanes);
  switch (npad) {
    case 2: hipLaunchKernelGGL((mam_tile_kernel<T, 2>), grid, block, 0, s, a); break;
    case 4: hipLaunchKernelGGL((mam_tile_kernel<T, 4>), grid, block, 0, s, a); break;
    case 8: hipLaunchKernelGGL((mam_tile_kernel<T, 8>), grid, block, 0, s, a); break;
    case 16: hipLaunchKernelGGL((mam_tile_kernel<T, 16>), grid, block, 0, s, a); break;
    case 32: hipLaunchKernelGGL((mam_tile_kernel<T, 32>), grid, block, 0, s, a); break;
    default: hipLaunchKernelGGL((mam_tile_kernel<T, 64>), grid, block, 0, s, a); break;
  }
}

// A call's tables: per segment the dense list of its non-NULL client pointers (missing clients
// compacted away) and RSeg::k from k_of(t, n, &k), which returns FEDAVG_OK or has failed.
template <typename KOf>
int32_t collect_segments(const fedavg_robust_view& v, const void* const* client_ptrs, int32_t num_clients,
                         size_t elem_bytes, void* const* out_ptrs, KOf&& k_of, std::vector<RSeg>* segs,
                         std::vector<const void*>* list, int* nmax) {
  const int T = v.num_segments;
  segs->assign(T, RSeg{});
  list->reserve(static_cast<size_t>(T) * static_cast<size_t>(num_clients < kRobustMaxClients ? num_clients : kRobustMaxClients));
  *nmax = 0;
  for (int t = 0; t < T; ++t) {
    if (out_ptrs[t] == nullptr) return invalid("null output pointer");
    RSeg& sg = (*segs)[t];
    sg.out = out_ptrs[t];
    sg.first = static_cast<int32_t>(list->size());
    sg.vec = reinterpret_cast<uintptr_t>(out_ptrs[t]) % 16 == 0;
    sg.pad_ = 0;
    int n = 0;
    for (int c = 0; c < num_clients; ++c) {
      const void* p = client_ptrs[static_cast<int64_t>(c) * T + t];
      if (p == nullptr) continue;
      if (reinterpret_cast<uintptr_t>(p) % elem_bytes != 0) return invalid("client tensor not aligned to its element size");
      if (reinterpret_cast<uintptr_t>(p) % 16 != 0) sg.vec = 0;
      if (++n > kRobustMaxClients)
        return invalid("segment " + std::to_string(t) + ": more than " + std::to_string(kRobustMaxClients) +
                       " clients (the register-resident sort holds at most 64 values per element)");
      list->push_back(p);
    }
    if (n == 0)
      return fedavg_internal_fail(FEDAVG_ERR_STATE, ("segment " + std::to_string(t) + " has no client data").c_str());
    int32_t k = 0;
    const int32_t rk = k_of(t, n, &k);
    if (rk != FEDAVG_OK) return rk;
    sg.n = n;
    sg.k = k;
    *nmax = n > *nmax ? n : *nmax;
  }
  return FEDAVG_OK;
}

// The tables go through one of two pinned slots to the device (a slot is reused once the launch
// that read it has finished); *a is ready for the launch, which the caller records in *slot.
int32_t upload_tables(const fedavg_robust_view& v, void** state_slot, const std::vector<RSeg>& segs,
                      const std::vector<const void*>& list, int32_t out_dtype, hipStream_t s, RobustState** state,
                      TableRing::Slot** slot, RArgs* a) {
  FEDAVG_TRY_HIP(hipSetDevice(v.device));
  RobustState* st = nullptr;
  FEDAVG_TRY(ensure_state(v, state_slot, &st));
  const size_t seg_bytes = sizeof(RSeg) * segs.size();
  const size_t bytes = seg_bytes + sizeof(void*) * list.size();
  FEDAVG_TRY(st->ring.acquire(bytes, slot));
  TableRing::Slot& sl = **slot;
  std::memcpy(sl.host, segs.data(), seg_bytes);
  std::memcpy(sl.host + seg_bytes, list.data(), sizeof(void*) * list.size());
  FEDAVG_TRY(st->ring.submit(sl, bytes, s));
  a->tiles = st->d_tiles;
  a->segs = reinterpret_cast<const RSeg*>(sl.dev);
  a->ptrs = reinterpret_cast<const void* const*>(sl.dev + seg_bytes);
  a->flag = v.d_flag;
  a->out_f32 = out_dtype == FEDAVG_F32 ? 1 : 0;
  *state = st;
  return FEDAVG_OK;
}

int npad_for(int nmax) {
  int npad = 2;
  while (npad < nmax) npad *= 2;
  return npad;
}

}  // namespace

int32_t fedavg_internal_robust_constant(const char* name, int64_t* out) {
  const std::string n(name);
  if (n == "robust_tile") *out = kRobustTile;
  else if (n == "robust_lanes") *out = kRobustLanes;
  else if (n == "robust_max_clients") *out = kRobustMaxClients;
  else if (n == "robust_ae_f32") *out = KeyFormat<float>::N;
  else if (n == "robust_ae_f16") *out = KeyFormat<__half>::N;
  else if (n == "robust_ae_bf16") *out = KeyFormat<bf16_t>::N;
  else if (n == "robust_ae_f64") *out = KeyFormat<double>::N;
  else if (n == "mam_tile") *out = kRobustTile;
  else if (n == "mam_lanes") *out = kRobustLanes;
  else if (n == "mam_ae_f32") *out = KeyFormat<float>::N;
  else if (n == "mam_ae_f16") *out = KeyFormat<__half>::N;
  else if (n == "mam_ae_bf16") *out = KeyFormat<bf16_t>::N;
  else if (n == "mam_ae_f64") *out = KeyFormat<double>::N;
  else return FEDAVG_ERR_INVALID;
  return FEDAVG_OK;
}

void fedavg_internal_robust_release(int32_t device, void* state) {
  if (state == nullptr) return;
  (void)hipSetDevice(device);
  delete static_cast<RobustState*>(state);
}

extern "C" int32_t fedavg_robust_aggregate(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                           int32_t num_clients, int32_t mode, const int32_t* trim_k,
                                           void* const* out_ptrs, int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rm = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_ROBUST, &slot);
  if (rm != FEDAVG_OK) return rm;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (in_dtype != FEDAVG_F32 && in_dtype != FEDAVG_F16 && in_dtype != FEDAVG_BF16 && in_dtype != FEDAVG_F64)
    return invalid("robust aggregation reads dense fp32 / fp16 / bf16 / fp64 tensors (no records)");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("out dtype must be FEDAVG_F32 or FEDAVG_F64");
  if (mode != FEDAVG_ROBUST_TRIMMED_MEAN && mode != FEDAVG_ROBUST_MEDIAN)
    return invalid("mode must be FEDAVG_ROBUST_TRIMMED_MEAN or FEDAVG_ROBUST_MEDIAN");
  if (num_clients <= 0 || client_ptrs == nullptr) return invalid("null or empty client table");
  if (out_ptrs == nullptr) return invalid("null out table");
  if (mode == FEDAVG_ROBUST_TRIMMED_MEAN && trim_k == nullptr) return invalid("trimmed mean needs trim_k");

  const size_t elem_bytes = in_dtype == FEDAVG_F64 ? 8 : in_dtype == FEDAVG_F32 ? 4 : 2;
  std::vector<RSeg> segs;
  std::vector<const void*> list;
  int nmax = 0;
  const int32_t rc = collect_segments(
      v, client_ptrs, num_clients, elem_bytes, out_ptrs,
      [&](int t, int n, int32_t* k) -> int32_t {
        *k = mode == FEDAVG_ROBUST_MEDIAN ? (n - 1) / 2 : trim_k[t];
        if (*k < 0 || 2 * *k >= n)
          return invalid("segment " + std::to_string(t) + ": trim_k " + std::to_string(*k) + " keeps no value of " +
                         std::to_string(n));
        return FEDAVG_OK;
      },
      &segs, &list, &nmax);
  if (rc != FEDAVG_OK) return rc;
  const int npad = npad_for(nmax);

  hipStream_t s = static_cast<hipStream_t>(stream);
  RobustState* st = nullptr;
  TableRing::Slot* sl = nullptr;
  RArgs a;
  const int32_t ru = upload_tables(v, slot, segs, list, out_dtype, s, &st, &sl, &a);
  if (ru != FEDAVG_OK) return ru;
  const dim3 grid(static_cast<unsigned>(st->num_tiles));
  switch (in_dtype) {
    case FEDAVG_F32: launch_npad<float>(npad, grid, s, a); break;
    case FEDAVG_F16: launch_npad<__half>(npad, grid, s, a); break;
    case FEDAVG_BF16: launch_npad<bf16_t>(npad, grid, s, a); break;
    default: launch_npad<double>(npad, grid, s, a); break;
  }
  FEDAVG_TRY_HIP(hipGetLastError());
  return st->ring.retire(*sl, s);
}

extern "C" int32_t fedavg_mean_around_median(fedavg_ctx* ctx, const void* const* client_ptrs, int32_t in_dtype,
                                             int32_t num_clients, const int32_t* keep, void* const* out_ptrs,
                                             int32_t out_dtype, void* stream) {
  fedavg_robust_view v;
  const int32_t rv = fedavg_internal_robust_view(ctx, &v);
  if (rv != FEDAVG_OK) return rv;
  void** slot = nullptr;
  const int32_t rm = fedavg_internal_module_slot(ctx, FEDAVG_MODULE_ROBUST, &slot);
  if (rm != FEDAVG_OK) return rm;
  if (v.busy) return fedavg_internal_fail(FEDAVG_ERR_STATE, "a dynamic wave is open on this context");
  if (in_dtype != FEDAVG_F32 && in_dtype != FEDAVG_F16 && in_dtype != FEDAVG_BF16 && in_dtype != FEDAVG_F64)
    return invalid("the mean around the median reads dense fp32 / fp16 / bf16 / fp64 tensors (no records)");
  if (out_dtype != FEDAVG_F32 && out_dtype != FEDAVG_F64) return invalid("out dtype must be FEDAVG_F32 or FEDAVG_F64");
  if (num_clients <= 0 || client_ptrs == nullptr) return invalid("null or empty client table");
  if (out_ptrs == nullptr) return invalid("null out table");
  if (keep == nullptr) return invalid("the mean around the median needs keep");

  const size_t elem_bytes = in_dtype == FEDAVG_F64 ? 8 : in_dtype == FEDAVG_F32 ? 4 : 2;
  std::vector<RSeg> segs;
  std::vector<const void*> list;
  int nmax = 0;
  const int32_t rc = collect_segments(
      v, client_ptrs, num_clients, elem_bytes, out_ptrs,
      [&](int t, int n, int32_t* k) -> int32_t {
        *k = keep[t];
        if (*k < 1 || *k > n)
          return invalid("segment " + std::to_string(t) + ": keep " + std::to_string(*k) + " is not in [1, " +
                         std::to_string(n) + "]");
        return FEDAVG_OK;
      },
      &segs, &list, &nmax);
  if (rc != FEDAVG_OK) return rc;
  const int npad = npad_for(nmax);

  hipStream_t s = static_cast<hipStream_t>(stream);
  RobustState* st = nullptr;
  TableRing::Slot* sl = nullptr;
  RArgs a;
  const int32_t ru = upload_tables(v, slot, segs, list, out_dtype, s, &st, &sl, &a);
  if (ru != FEDAVG_OK) return ru;
  const dim3 grid(static_cast<unsigned>(st->num_tiles));
  switch (in_dtype) {
    case FEDAVG_F32: launch_mam_npad<float>(npad, grid, s, a); break;
    case FEDAVG_F16: launch_mam_npad<__half>(npad, grid, s, a); break;
    case FEDAVG_BF16: launch_mam_npad<bf16_t>(npad, grid, s, a); break;
    default: launch_mam_npad<double>(npad, grid, s, a); break;
  }
  FEDAVG_TRY_HIP(hipGetLastError());
  return st->ring.retire(*sl, s);
}
