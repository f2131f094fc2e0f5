// The bf16 pieces of an f32 (lenet_fast.hip, lenet_net_split.hip; gpd_hip_bf16_split3 is their host statement):
// a = h + m + l with h = bf16(a), m = bf16(a - h), l = bf16(a - h - m), round to nearest even, the residuals exact in f32.
#pragma once
#include <cstdint>
#include <cstring>

#include <hip/hip_runtime.h>

namespace gpd {

struct Bf3 {
  unsigned short h, m, l;
};
__host__ __device__ inline unsigned short bf16_bits(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const __bf16 b = (__bf16)x;
  unsigned short u;
  __builtin_memcpy(&u, &b, 2);
  return u;
#else
  uint32_t u;
  memcpy(&u, &x, 4);
  if ((u & 0x7f800000u) == 0x7f800000u) return (unsigned short)((u >> 16) | ((u & 0xffffu) ? 0x40u : 0u));  // inf / nan
  u += 0x7fffu + ((u >> 16) & 1u);
  return (unsigned short)(u >> 16);
#endif
}
__host__ __device__ inline float bf16_value(unsigned short b) {
  const uint32_t u = (uint32_t)b << 16;
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_memcpy(&f, &u, 4);
#else
  memcpy(&f, &u, 4);
#endif
  return f;
}
__host__ __device__ inline Bf3 bf16_split3(float a) {
  Bf3 r;
  r.h = bf16_bits(a);
  const float r1 = a - bf16_value(r.h);
  r.m = bf16_bits(r1);
  const float r2 = r1 - bf16_value(r.m);
  r.l = bf16_bits(r2);
  return r;
}

// bf16_split3 of TWO values at once: v_cvt_pk_bf16_f32 rounds both (the same round to nearest even per element) and leaves the
// pair packed as the planes want it; a piece's value for the residual is its half of the pair, shifted or masked into place
__host__ __device__ inline uint32_t bf16_pair_bits(float x0, float x1) {
#if defined(__HIP_DEVICE_COMPILE__)
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(uint32_t, __builtin_convertvector(f32x2{x0, x1}, bf16x2));
#else
  return bf16_bits(x0) | ((uint32_t)bf16_bits(x1) << 16);
#endif
}
__host__ __device__ inline void bf16_split3_pair(float a0, float a1, uint32_t &h, uint32_t &m, uint32_t &l) {
  h = bf16_pair_bits(a0, a1);
  float r0 = a0 - bf16_value((unsigned short)h), r1 = a1 - bf16_value((unsigned short)(h >> 16));
  m = bf16_pair_bits(r0, r1);
  r0 -= bf16_value((unsigned short)m);
  r1 -= bf16_value((unsigned short)(m >> 16));
  l = bf16_pair_bits(r0, r1);
}

}  // namespace gpd
