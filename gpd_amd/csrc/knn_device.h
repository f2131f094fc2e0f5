// The k-nearest-neighbour search of one point on the cloud's uniform grid, a WAVE per point: what knn_kernel (refine.hip) and
// outlier_dist_kernel (outliers.hip) run ahead of their epilogues.  The grid is visited in square shells of cells around the
// point's cell.  Every visited point's (d2 bits, index) key that beats the current k-th key goes to the wave's LDS row; the
// row is sorted in registers by the normals path's bitonic network (grid_sort.h) and cut to k whenever it fills and after
// every shell.  The search stops when the k-th key's d2 is below refine::ring_bound of the shell — a lower bound of the
// float d2 of every point not visited yet — or the shells have covered the grid.
#pragma once
#include "gpd_internal.h"
#include "grid_sort.h"
#include "refine_model.h"

namespace gpd {

constexpr int KN_WAVES = 4;     // points per workgroup of a kernel that searches
constexpr int KN_BUF = 1024;    // keys a wave's LDS row holds (cut back to k <= kRefineKCap whenever it fills)
constexpr int KN_SHELLS = 257;  // ring_bound of shells 0 .. 256 (a grid has at most 256 cells per axis)
static_assert(KN_BUF - kRefineKCap >= 64, "a cut row must take the next 64 candidates");

struct KnnSearch {
  GridView grid;
  int num_points;
  int k;                    // 1 <= k <= min(kRefineKCap, num_points)
  float bound[KN_SHELLS];   // refine::ring_bound(R, cell)
};
inline void knn_search_fill(KnnSearch &s, const Cloud &c, int k) {
  s.grid = grid_view(c);
  s.num_points = c.num_points;
  s.k = k;
  for (int R = 0; R < KN_SHELLS; R++) s.bound[R] = refine::ring_bound(R, c.g_cell);
}

// the LDS of a workgroup of KN_WAVES searching waves
struct KnnLds {
  unsigned long long keys[KN_WAVES][KN_BUF];
  int beg[KN_WAVES][128], off[KN_WAVES][128];  // the point ranges of a batch of 64 cell columns, two per column
};

// sort the n keys of the row through registers and keep the first `keep` (n <= 64 K)
template <int K>
__device__ __forceinline__ void knn_cut(unsigned long long *keys, int n, int keep, int lane) {
  double key[K];
#pragma unroll
  for (int r = 0; r < K; r++) key[r] = __longlong_as_double((long long)(lane * K + r < n ? keys[lane * K + r] : NL_PAD_KEY));
  wave_sort_regs<K>(key, lane);
#pragma unroll
  for (int r = 0; r < K; r++)
    if (lane * K + r < keep) keys[lane * K + r] = (unsigned long long)__double_as_longlong(key[r]);
}

// The search of the point at cell-order position w (< P.num_points, wave-uniform) by the calling wave: returns n, the keys
// found (min(k, num_points): the shells end by covering the grid), sorted ascending in keys[0 .. n) and visible to every lane
// of the wave.  keys: KN_BUF entries, beg / off: 128 ints each, the wave's own.
__device__ __forceinline__ int knn_search_row(const KnnSearch &P, int w, int lane, unsigned long long *keys, int *beg, int *off) {
  const GridView &g = P.grid;
  const float4 q4 = g.p[w];
  const float qx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q4.x))),
              qy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q4.y))),
              qz = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q4.z)));
  const int cx = grid_coord(g, 0, qx), cy = grid_coord(g, 1, qy), cz = grid_coord(g, 2, qz);
  const int k = P.k;
  int n = 0;                           // wave-uniform: keys in the row
  bool sorted = true;                  // the row is sorted and holds at most k keys
  unsigned long long kth = ~0ull;      // the k-th key once k are known: a candidate must beat it
  auto sync_row = [&]() {
    __threadfence_block();  // the row was written by other lanes of this wave
    __builtin_amdgcn_wave_barrier();
  };
  auto cut = [&]() {
    sync_row();
    const int keep = n < k ? n : k;
    if (n <= 256)
      knn_cut<4>(keys, n, keep, lane);
    else if (n <= 512)
      knn_cut<8>(keys, n, keep, lane);
    else
      knn_cut<16>(keys, n, keep, lane);
    sync_row();
    n = keep;
    sorted = true;
    if (n == k) kth = keys[k - 1];
  };
  for (int R = 0;; R++) {
    const int xa = max(0, cx - R), xb = min(g.dim[0] - 1, cx + R);
    const int ya = max(0, cy - R), yb = min(g.dim[1] - 1, cy + R);
    const int za = max(0, cz - R), zb = min(g.dim[2] - 1, cz + R);
    const int nyc = yb - ya + 1, ncol = (xb - xa + 1) * nyc;
    // the shell: border columns whole (za .. zb), inner columns their bottom and top cells; a lane per column, 64 at a time
    for (int col0 = 0; col0 < ncol; col0 += 64) {
      const int col = col0 + lane;
      int b0 = 0, l0 = 0, b1 = 0, l1 = 0;
      if (col < ncol) {
        const int x = xa + col / nyc, y = ya + col % nyc;
        const int base = (x * g.dim[1] + y) * g.dim[2];
        if (abs(x - cx) == R || abs(y - cy) == R) {
          b0 = g.start[base + za];
          l0 = g.start[base + zb + 1] - b0;
        } else {
          if (cz - R >= 0) {
            b0 = g.start[base + cz - R];
            l0 = g.start[base + cz - R + 1] - b0;
          }
          if (cz + R <= g.dim[2] - 1) {
            b1 = g.start[base + cz + R];
            l1 = g.start[base + cz + R + 1] - b1;
          }
        }
      }
      int incl = l0 + l1;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(incl, o);
        if (lane >= o) incl += x;
      }
      const int excl = incl - (l0 + l1);
      const int T = __builtin_amdgcn_readlane(incl, 63);
      sync_row();  // the previous batch's lanes are done with the range table
      beg[2 * lane] = b0;
      beg[2 * lane + 1] = b1;
      off[2 * lane] = excl;
      off[2 * lane + 1] = excl + l0;
      sync_row();
      for (int t0 = 0; t0 < T; t0 += 64) {
        if (n + 64 > KN_BUF) cut();
        const int t = t0 + lane;
        const bool in = t < T;
        int r = 0;  // the last range that starts at or before t (it is not empty)
#pragma unroll
        for (int step = 64; step > 0; step >>= 1)
          if (off[r + step] <= t) r += step;
        const float4 p = g.p[in ? beg[r] + (t - off[r]) : 0];
        float d = qx - p.x;  // FLANN L2_Simple<float>: d2 accumulated over x, y, z
        float d2 = 0.f;
        d2 += d * d;
        d = qy - p.y;
        d2 += d * d;
        d = qz - p.z;
        d2 += d * d;
        const unsigned long long kv = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)__float_as_int(p.w);
        const bool hit = in && kv < kth;
        const unsigned long long ballot = __ballot(hit);
        if (hit) keys[n + __popcll(ballot & ((1ull << lane) - 1ull))] = kv;
        const int add = __popcll(ballot);
        n += add;
        sorted = sorted && add == 0;
      }
    }
    if (!sorted) cut();
    const bool all = cx - R <= 0 && cx + R >= g.dim[0] - 1 && cy - R <= 0 && cy + R >= g.dim[1] - 1 && cz - R <= 0 && cz + R >= g.dim[2] - 1;
    if (all || (n == k && __uint_as_float((unsigned)(kth >> 32)) < P.bound[R < KN_SHELLS ? R : KN_SHELLS - 1])) break;
  }
  return n;
}

}  // namespace gpd
