// Device pieces the grid build (cloud.hip), the radius searches (search.hip, normals.hip) and the k-nearest-neighbour
// search (refine.hip) share: the cell of a coordinate in the cloud's uniform grid, the visit of the cells around a query,
// the in-register bitonic sort of (d2 bits, index) keys, and the test that certifies an order-free fp64 sum of floats.
#pragma once
#include <hip/hip_runtime.h>

#include "gpd_internal.h"

namespace gpd {

__device__ inline int grid_coord(const GridView &g, int axis, float v) {
  int k = (int)floorf((v - g.lo[axis]) / g.cell);
  return k < 0 ? 0 : (k > g.dim[axis] - 1 ? g.dim[axis] - 1 : k);
}

// Visits every point of the cells overlapping the cube of half-edge `reach` around q: calls
// visit(original index, x, y, z).  Wave w takes (x, y) cell columns w, w + nwaves, ...; a column's
// cells are contiguous in memory (z fastest), its lanes stride the point range.  All lanes of a
// wave run the same number of iterations, so `visit` may use wave-wide operations.
template <class Visit>
__device__ inline void grid_visit(const GridView &g, float qx, float qy, float qz, float reach, int wave, int nwaves, int lane,
                                  Visit visit) {
  const int x0 = grid_coord(g, 0, qx - reach), x1 = grid_coord(g, 0, qx + reach);
  const int y0 = grid_coord(g, 1, qy - reach), y1 = grid_coord(g, 1, qy + reach);
  const int z0 = grid_coord(g, 2, qz - reach), z1 = grid_coord(g, 2, qz + reach);
  const int ny = y1 - y0 + 1;
  const int ncol = (x1 - x0 + 1) * ny;
  for (int col = wave; col < ncol; col += nwaves) {
    const int cx = x0 + col / ny, cy = y0 + col % ny;
    const int cbase = (cx * g.dim[1] + cy) * g.dim[2];
    const int b = g.start[cbase + z0], e = g.start[cbase + z1 + 1];
    for (int t0 = b; t0 < e; t0 += 64) {
      const int t = t0 + lane;
      const bool in = t < e;
      const int tt = in ? t : b;
      const float4 p = g.p[tt];
      visit(in, __float_as_int(p.w), p.x, p.y, p.z);
    }
  }
}

// Is the fp64 sum of n floats exact in every order?  emin / emax: smallest / largest biased exponent among the non-zero addends
// (denormals count as exponent 1; no non-zero addend: emin = 255 > emax = 0).  Every addend is a multiple of 2^(emin - 150) and
// below 2^(emax - 126) in magnitude, so every partial sum of every subset is a multiple of the former below n 2^(emax - 126);
// fp64 holds every multiple of 2^L below 2^(L + 53): exact when ceil(log2 n) + emax - 126 <= emin - 150 + 53.  One more bit is
// left as margin; infinities / NaNs (emax = 255) never pass.
__host__ __device__ inline bool centre_exact(int emin, int emax, int n) {
  if (emax == 0) return true;  // nothing but zeros
  if (emax >= 255) return false;
  int lg = 0;
  while ((1ll << lg) < (long long)n) lg++;
  return lg + emax - emin <= 28;
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
