// Device pieces the radius searches (search.hip) and the k-nearest-neighbour search (refine.hip) share: the cell of a
// coordinate in the cloud's uniform grid, and the in-register bitonic sort of (d2 bits, index) keys.
#pragma once
#include <hip/hip_runtime.h>

#include "gpd_internal.h"

namespace gpd {

__device__ inline int grid_coord(const GridView &g, int axis, float v) {
  int k = (int)floorf((v - g.lo[axis]) / g.cell);
  return k < 0 ? 0 : (k > g.dim[axis] - 1 ? g.dim[axis] - 1 : k);
}

// Bitonic sort of 64 K keys held K per lane, element e = lane * K + r, ascending — in the formulation whose every
// compare-exchange puts the minimum at the lower index: a merge of width k starts with the "flip" step (partner e ^ (k - 1))
// and goes on with partners e ^ j, j = k / 4 .. 1.  Partners inside a lane exchange registers (v_min_f64 + v_max_f64: the keys
// are compared AS DOUBLES — sign bit clear, never a NaN, so the order is the order of the bit patterns — at the full f64 rate,
// where a 64-bit integer compare plus selects costs four times as much); partners in another lane come through ds_bpermute.
// (d2 bits, index) ascending = FLANN's result order; positive floats order as their bit patterns.
__device__ __forceinline__ double key_min(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));  // (no canonicalisation of the operands: they are never NaNs)
  return r;
}
__device__ __forceinline__ double key_max(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
constexpr unsigned long long NL_PAD_KEY = 0x7fefffffffffffffull;  // above every key, and a finite double
template <int K>
__device__ __forceinline__ void wave_sort_regs(double (&key)[K], int lane) {
  auto from_lane = [&](double v, int xor_mask) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    const unsigned lo = __shfl_xor((unsigned)b, xor_mask), hi = __shfl_xor((unsigned)(b >> 32), xor_mask);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
  };
#pragma unroll
  for (int k = 2; k <= 64 * K; k <<= 1) {
    // ---- the flip step: partner e ^ (k - 1)
    if (k <= K) {
#pragma unroll
      for (int r = 0; r < K; r++)
        if ((r & (k >> 1)) == 0) {  // the lower half of its block of k
          const int r2 = r ^ (k - 1);
          const double a = key[r], b = key[r2];
          key[r] = key_min(a, b);
          key[r2] = key_max(a, b);
        }
    } else {
      const int lm = k / K - 1;                       // lanes of a block of k elements: flip them all, and r within the lane
      const bool lower = (lane & (k / K / 2)) == 0;   // the lower half of the block holds the minima
      double other[K];
#pragma unroll
      for (int r = 0; r < K; r++) other[r] = from_lane(key[K - 1 - r], lm);
#pragma unroll
      for (int r = 0; r < K; r++) key[r] = ((other[r] < key[r]) == lower) ? other[r] : key[r];
    }
    // ---- partners e ^ j
#pragma unroll
    for (int j = k >> 2; j > 0; j >>= 1) {
      if (j >= K) {
        const int lj = j / K;
        const bool lower = (lane & lj) == 0;
#pragma unroll
        for (int r = 0; r < K; r++) {
          const double other = from_lane(key[r], lj);
          key[r] = ((other < key[r]) == lower) ? other : key[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < K; r++)
          if ((r & j) == 0) {
            const double a = key[r], b = key[r | j];
            key[r] = key_min(a, b);
            key[r | j] = key_max(a, b);
          }
      }
    }
  }
}

}  // namespace gpd
