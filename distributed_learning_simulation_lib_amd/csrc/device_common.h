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
