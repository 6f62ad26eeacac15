// Device-side helpers the side modules (<module>_kernels.hip) share: the 16-byte vector types, the
// staged-bytes-to-fp64 formats, the guarded loads, the NaN-flag store and the Philox block. Everything here is
// inlined into the kernel that calls it; fedavg_kernels.hip and personalized_kernels.hip keep their own.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdint>

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
struct bf16_t {
  uint16_t bits;
};

#define FEDAVG_AS_GLOBAL __attribute__((address_space(1)))
#define FEDAVG_AS_CONST __attribute__((address_space(4)))

// A client's 16 staged bytes -> fp64 values, exactly.
template <typename T>
struct Format;
template <>
struct Format<float> {
  static constexpr int N = 4;
  __device__ __forceinline__ static double value(const u32x4& raw, int i) {
    return static_cast<double>(__uint_as_float(raw[i]));
  }
};
template <>
struct Format<__half> {
  static constexpr int N = 8;
  __device__ __forceinline__ static double value(const u32x4& raw, int i) {
    const uint32_t h = (raw[i / 2] >> (16 * (i % 2))) & 0xffffu;
    return static_cast<double>(__half2float(__ushort_as_half(static_cast<unsigned short>(h))));
  }
};
template <>
struct Format<bf16_t> {
  static constexpr int N = 8;
  __device__ __forceinline__ static double value(const u32x4& raw, int i) {
    return static_cast<double>(__uint_as_float((raw[i / 2] >> (16 * (i % 2))) << 16));
  }
};
template <>
struct Format<double> {
  static constexpr int N = 2;
  __device__ __forceinline__ static double value(const u32x4& raw, int i) {
    const uint64_t lo = raw[2 * i], hi = raw[2 * i + 1];
    return __longlong_as_double(static_cast<long long>(lo | (hi << 32)));
  }
};

// The 16 bytes element by element: only elements below `have` are read (a span's last vector at a
// segment's end, or client storage that is not 16-byte aligned); the rest stay +0.0.
template <typename T>
__device__ __forceinline__ u32x4 load_guarded(const void* base, int64_t elem, int have) {
  constexpr int N = Format<T>::N;
  u32x4 raw = {0u, 0u, 0u, 0u};
  if constexpr (sizeof(T) == 2) {
    const uint16_t FEDAVG_AS_GLOBAL* p = (const uint16_t FEDAVG_AS_GLOBAL*)base + elem;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i < have) raw[i / 2] |= static_cast<uint32_t>(p[i]) << (16 * (i % 2));
    }
  } else {
    constexpr int W = sizeof(T) / 4;  // 32-bit words per element
    const uint32_t FEDAVG_AS_GLOBAL* p = (const uint32_t FEDAVG_AS_GLOBAL*)base + elem * W;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i < have) {
#pragma unroll
        for (int w = 0; w < W; ++w) raw[i * W + w] = p[i * W + w];
      }
    }
  }
  return raw;
}

// The counterpart of load_guarded: only elements below `have` of the 16-byte image are written.
template <typename T>
__device__ __forceinline__ void store_guarded(void* base, int64_t elem, int have, const u32x4& raw) {
  constexpr int N = Format<T>::N;
  if constexpr (sizeof(T) == 2) {
    uint16_t FEDAVG_AS_GLOBAL* p = (uint16_t FEDAVG_AS_GLOBAL*)base + elem;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i < have) p[i] = static_cast<uint16_t>(raw[i / 2] >> (16 * (i % 2)));
    }
  } else {
    constexpr int W = sizeof(T) / 4;
    uint32_t FEDAVG_AS_GLOBAL* p = (uint32_t FEDAVG_AS_GLOBAL*)base + elem * W;
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i < have) {
#pragma unroll
        for (int w = 0; w < W; ++w) p[i * W + w] = raw[i * W + w];
      }
    }
  }
}

// N fp64 values of a point segment (a centre, a direction) from element `elem`: only elements below
// `have` are read, the rest stay +0.0, and a NULL base is the origin; 16-byte loads where `vec` says
// the segment is 16-byte aligned.
template <int N>
__device__ __forceinline__ void load_f64(double (&dst)[N], const double* base, int64_t elem, int have, bool vec) {
#pragma unroll
  for (int i = 0; i < N; ++i) dst[i] = 0.0;
  if (base == nullptr || have <= 0) return;
  const double FEDAVG_AS_GLOBAL* q = (const double FEDAVG_AS_GLOBAL*)base + elem;
  if (have >= N && vec) {  // elem is even: 16-byte aligned with the segment
#pragma unroll
    for (int i = 0; i < N; i += 2) {
      const f64x2 v = *(const f64x2 FEDAVG_AS_GLOBAL*)(q + i);
      dst[i] = v[0];
      dst[i + 1] = v[1];
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) {
      if (i < have) dst[i] = q[i];
    }
  }
}

// Latches word `word` of a flag block (the context's NaN words, a module's error words).
__device__ __forceinline__ void raise_flag(uint32_t* flag, int word) {
  __hip_atomic_store(flag + word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

// The pinned sum of fedavg_dp_noise (include/fedavg_hip.h, "The order of the sum"), which
// fedavg_sign_compress shares: its geometry, the one rounding of an fp64 value into a tensor's dtype
// and the adjacent-pair tree.
constexpr int kDThreads = 256;   // lanes per workgroup
constexpr int kDTile = 4096;     // elements per piece of a sum and per tile of the apply pass

// The float nearest to o that is odd where o is no float ("round to odd"): rounding it to a
// narrower format (at most 22 bits) gives what one rounding of o gives.
__device__ __forceinline__ uint32_t dp_odd_float_bits(double o) {
  const float f = static_cast<float>(o);
  uint32_t u = __float_as_uint(f);
  if (o == o && static_cast<double>(f) != o) {
    if (__builtin_fabs(static_cast<double>(f)) > __builtin_fabs(o)) u -= 1u;  // towards zero (from infinity too)
    u |= 1u;
  }
  return u;
}

// RNE(o) into T, as the bits of element i of the image
template <typename T>
__device__ __forceinline__ void dp_put(u32x4& raw, int i, double o);
template <>
__device__ __forceinline__ void dp_put<float>(u32x4& raw, int i, double o) {
  raw[i] = __float_as_uint(static_cast<float>(o));
}
template <>
__device__ __forceinline__ void dp_put<double>(u32x4& raw, int i, double o) {
  const uint64_t b = static_cast<uint64_t>(__double_as_longlong(o));
  raw[2 * i] = static_cast<uint32_t>(b);
  raw[2 * i + 1] = static_cast<uint32_t>(b >> 32);
}
template <>
__device__ __forceinline__ void dp_put<__half>(u32x4& raw, int i, double o) {
  const __half h = __float2half_rn(__uint_as_float(dp_odd_float_bits(o)));
  raw[i / 2] |= static_cast<uint32_t>(__half_as_ushort(h)) << (16 * (i % 2));
}
template <>
__device__ __forceinline__ void dp_put<bf16_t>(u32x4& raw, int i, double o) {
  const uint32_t u = dp_odd_float_bits(o);
  const uint32_t b = (o == o) ? (u + 0x7fffu + ((u >> 16) & 1u)) >> 16 : 0x7fc0u;
  raw[i / 2] |= b << (16 * (i % 2));
}

// the adjacent-pair tree over the first `width` (a power of two) lanes of every aligned block of
// `width` lanes; the block's sum is valid in its first lane
__device__ __forceinline__ double dp_tree(double v, int width, double* sm) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    if (off < width) v = v + __shfl_xor(v, off);
  }
  if (width > 64) {  // the same for every lane of the workgroup
    const int t = static_cast<int>(threadIdx.x);
    if ((t & 63) == 0) sm[t >> 6] = v;
    __syncthreads();
    const double a = sm[0] + sm[1], b = sm[2] + sm[3];
    v = width == 128 ? ((t & 128) ? b : a) : a + b;
  }
  return v;
}

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11): the block of counter (c0, c1, c2, c3) under key
// (k0, k1). The streams of the broadcast encoder and of the clip-and-noise pass are cut from it.
struct QWords {
  uint32_t w[4];
};

__device__ __forceinline__ QWords q_philox(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                           uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(kM0, c0), lo0 = kM0 * c0;
    const uint32_t hi1 = __umulhi(kM1, c2), lo1 = kM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kW0;
    k1 += kW1;
  }
  QWords o;
  o.w[0] = c0;
  o.w[1] = c1;
  o.w[2] = c2;
  o.w[3] = c3;
  return o;
}
