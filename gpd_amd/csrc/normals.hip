// Surface normals of the uploaded cloud on gfx950.
//
// normals_*_kernel       Cloud::calculateNormals (util/cloud.cpp:451-604): count, scan, lists, finish.
//
// All fp64 expressions are evaluated unfused, left to right (-ffp-contract=off),
// exactly as oracle/gpd_oracle.cpp defines them.
#include <algorithm>
#include <cstring>

#include "buffers.h"
#include "eigen3.h"
#include "gpd_internal.h"
#include "grid_sort.h"

namespace gpd {

// ---------------------------------------------------------------------------
// Cloud::calculateNormals (util/cloud.cpp:451-476): the radius-search normal estimation of calculateNormalsOMP
// (:497-535, pcl::NormalEstimationOMP) followed by reverseNormals (:573-604).  Per point: the neighbours within the
// radius in FLANN order (d2, index), centroid and covariance as sequential fp64 sums IN THAT ORDER (the oracle's
// definition: nine serial chains as long as the neighbourhood), Eigen's 3x3 eigensolver, eigenvector of the smallest
// eigenvalue, flipped towards the view point of the first camera that sees the point, then the reference's reversal rule.
//
// Rounds 1-3 gave every point a workgroup of its own that did all of this behind barriers: 1.40 ms per 30k points, 75 % of
// it three lanes walking the chains one LDS round trip per step, the eigensolver on one lane of 256.  Now every part runs
// where it is parallel:
//   normals_list_kernel    a WAVE per point (cell order: neighbouring waves share grid cells in L1): the hits' (d2 bits,
//                          index) keys go to the wave's LDS, then into registers — 4, 8 or 16 keys per lane — for a bitonic
//                          network that never touches memory (in-lane stages on registers, cross-lane stages through
//                          ds_bpermute); the sorted indices leave as 16-byte stores into the point's row.  No workgroup
//                          barrier anywhere.  A point with more than 1024 neighbours is queued
//   normals_list_big_kernel  the queued points (un-voxelised scans), a workgroup each: keys sorted in LDS (up to 8192) or
//                          in the point's own slice of an arena in global memory — ANY size: no capacity
//   normals_finish_kernel  a LANE per point: the nine chains of 64 points side by side in one wave (every lane useful, nine
//                          independent chains per lane against the add latency), coordinates gathered from the L2-resident
//                          point table with 32 rows in flight per lane, then 64 eigensolvers side by side, flips, store
// ---------------------------------------------------------------------------
constexpr int NL_CAP = 1024;       // neighbours a wave sorts in registers (voxelised clouds at radius 0.03: ~340, up to ~950)
constexpr int NL_WAVES = 4;        // points per workgroup of the wave-per-point kernel
constexpr int NL_BIG_LDS = 8192;   // keys the big kernel sorts in LDS (64 KB); longer lists are sorted in their arena slice
struct NormalsParams {
  GridView grid;
  const float4 *pxyz;              // [P] by original index
  int num_points;
  const int32_t *cam_source;
  int num_cams;
  double view_points[3 * kMaxCams];
  float r2;
  float reach;
  int32_t *count;                  // [P] by cell-order position
  int w0, w1;                      // the tile of this pass: cell-order positions [w0, w1), w0 a multiple of 64
  float4 *lists;                   // [(w1 - w0) / 64][NL_CAP][64] neighbour coordinates in FLANN order, transposed per block of 64 points
  int32_t *big;                    // [0] number of queued points, [1 ..] their cell-order positions
  long long *big_off;              // [P] slice of a queued point in the arena (8-byte units)
  unsigned long long *arena;       // sort space + sorted indices of the queued points
  unsigned long long *arena_top;   // bump allocator (8-byte units)
  long long arena_cap;
  int32_t *status;                 // bit 0: the arena is too small (the host grows it and runs again)
  float *out;                      // AoS [P][3] by original index
  double *cent;                    // [P][3] by cell-order position: the centroid of a point's list when its order-free sum is certified
                                   // exact (centre_exact), NaN where it is not (normals_finish_kernel then walks the chain)
};

// the hits of one query among the cells around it, a wave at work: hit(is a hit, index, d2) for every candidate, 64 at a time
template <typename Hit>
__device__ inline void normals_visit(const NormalsParams &P, float qx, float qy, float qz, int lane, Hit hit) {
  auto test = [&](bool in, int i, float x, float y, float z) {
    float d = qx - x;  // FLANN L2_Simple<float>: d2 accumulated over x, y, z, strict <
    float d2 = 0.f;
    d2 += d * d;
    d = qy - y;
    d2 += d * d;
    d = qz - z;
    d2 += d * d;
    hit(in && d2 < P.r2, i, d2);
  };
  const GridView &g = P.grid;
  const int x0 = grid_coord(g, 0, qx - P.reach), x1 = grid_coord(g, 0, qx + P.reach);
  const int y0 = grid_coord(g, 1, qy - P.reach), y1 = grid_coord(g, 1, qy + P.reach);
  const int z0 = grid_coord(g, 2, qz - P.reach), z1 = grid_coord(g, 2, qz + P.reach);
  const int ny = y1 - y0 + 1;
  const int ncol = (x1 - x0 + 1) * ny;
  if (ncol <= 64) {
    // the point ranges of all (x, y) cell columns in one round trip (a lane per column); then the first 64 points of
    // EIGHT columns are requested before any of them is tested — a column of a voxelised cloud holds ~45 points, so
    // a 4 x 4-column neighbourhood costs three dependent round trips instead of nine (the kernel waits for memory, not
    // for its ALUs: 30k waves of a few hundred instructions each)
    int cbv = 0, cev = 0;
    if (lane < ncol) {
      const int cx = x0 + lane / ny, cy = y0 + lane % ny;
      const int cbase = (cx * g.dim[1] + cy) * g.dim[2];
      cbv = g.start[cbase + z0];
      cev = g.start[cbase + z1 + 1];
    }
    for (int c0 = 0; c0 < ncol; c0 += 8) {
      int cb[8], cn[8];
      float4 p[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int c = c0 + u < ncol ? c0 + u : c0;
        cb[u] = __builtin_amdgcn_readlane(cbv, c);
        cn[u] = c0 + u < ncol ? __builtin_amdgcn_readlane(cev, c) - cb[u] : 0;
      }
#pragma unroll
      for (int u = 0; u < 8; u++) p[u] = g.p[lane < cn[u] ? cb[u] + lane : 0];
#pragma unroll
      for (int u = 0; u < 8; u++)
        if (cn[u] > 0) test(lane < cn[u], __float_as_int(p[u].w), p[u].x, p[u].y, p[u].z);
#pragma unroll
      for (int u = 0; u < 8; u++)  // fuller columns (a wall seen edge-on, an un-voxelised scan): the rest, 64 at a time
        for (int t0 = 64; t0 < cn[u]; t0 += 64) {
          const bool in = t0 + lane < cn[u];
          const float4 pt = g.p[in ? cb[u] + t0 + lane : 0];
          test(in, __float_as_int(pt.w), pt.x, pt.y, pt.z);
        }
    }
  } else {
    grid_visit(g, qx, qy, qz, P.reach, 0, 1, lane, test);
  }
}

// sort the n keys of the wave's LDS row through registers, fetch the coordinates and store the list TRANSPOSED: entry e of
// the p-th point of a block of 64 points at [block][e][p], so that normals_finish_kernel — a lane per point — reads one
// contiguous kilobyte per step and wave
template <int K>
__device__ __forceinline__ void normals_sort_store(const NormalsParams &P, const unsigned long long *keys, int n, int lane, int w, const float4 &q) {
  double key[K];
#pragma unroll
  for (int r = 0; r < K; r++) key[r] = __longlong_as_double((long long)(lane * K + r < n ? keys[lane * K + r] : NL_PAD_KEY));
  wave_sort_regs<K>(key, lane);
  float4 *col = P.lists + (size_t)((w - P.w0) >> 6) * NL_CAP * 64 + (w & 63);
  // (round 6) the centroid on the way: the coordinates pass through this wave's registers anyway.  The sum of floats in fp64 is
  // the same in EVERY order when centre_exact's certificate holds (two exponents per coordinate), so the order-free sum taken
  // here — a lane its entries, then the wave — is the sequential one of the oracle; normals_finish_kernel then reads the lists
  // ONCE (covariance) instead of twice: it moved 447 MB per 30k points, 3.8 TB/s.  A list that fails the certificate (a neighbour
  // micrometres from a coordinate plane) gets NaN and its chain is walked there, as before.
  // The certificate's two exponents per coordinate: every neighbour lies within the search radius of the query, so when the
  // query is farther than that from the coordinate plane (wave-uniform: three neighbourhoods in four on the benchmark clouds)
  // |q| - r <= |x| <= |q| + r bounds them without looking at a single entry; only a neighbourhood that reaches a coordinate
  // plane tracks its smallest non-zero and its largest |x| entry by entry (as unsigned bit patterns: |x| orders like its bits,
  // and bits - 1 sends a zero to the far end of a minimum).
  const float qv[3] = {q.x, q.y, q.z};
  const float rad = sqrtf(P.r2) * 1.0001f;
  const bool track = !(fabsf(qv[0]) > 2.f * rad && fabsf(qv[1]) > 2.f * rad && fabsf(qv[2]) > 2.f * rad);
  double cs[3] = {0.0, 0.0, 0.0};
  unsigned umax[3] = {0u, 0u, 0u}, umin[3] = {~0u, ~0u, ~0u};
  auto take = [&](const float4 &v, bool on) {
    const float x[3] = {on ? v.x : 0.f, on ? v.y : 0.f, on ? v.z : 0.f};
#pragma unroll
    for (int a = 0; a < 3; a++) {
      cs[a] += (double)x[a];
      if (track) {
        const unsigned b = __float_as_uint(x[a]) & 0x7fffffffu;
        umax[a] = max(umax[a], b);
        umin[a] = min(umin[a], b - 1u);
      }
    }
  };
#pragma unroll
  for (int r0 = 0; r0 < K; r0 += 4) {  // four gathers in flight, then their four stores
    const int e = lane * K + r0;
    const float4 v0 = P.pxyz[e + 0 < n ? (unsigned)__double_as_longlong(key[r0 + 0]) : 0u];
    const float4 v1 = P.pxyz[e + 1 < n ? (unsigned)__double_as_longlong(key[r0 + 1]) : 0u];
    const float4 v2 = P.pxyz[e + 2 < n ? (unsigned)__double_as_longlong(key[r0 + 2]) : 0u];
    const float4 v3 = P.pxyz[e + 3 < n ? (unsigned)__double_as_longlong(key[r0 + 3]) : 0u];
    if (e + 0 < n) col[(size_t)(e + 0) * 64] = v0;
    if (e + 1 < n) col[(size_t)(e + 1) * 64] = v1;
    if (e + 2 < n) col[(size_t)(e + 2) * 64] = v2;
    if (e + 3 < n) col[(size_t)(e + 3) * 64] = v3;
    take(v0, e + 0 < n);
    take(v1, e + 1 < n);
    take(v2, e + 2 < n);
    take(v3, e + 3 < n);
  }
#pragma unroll
  for (int a = 0; a < 3; a++) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      cs[a] += __shfl_xor(cs[a], o);
      if (track) {
        umax[a] = max(umax[a], (unsigned)__shfl_xor((int)umax[a], o));
        umin[a] = min(umin[a], (unsigned)__shfl_xor((int)umin[a], o));
      }
    }
  }
  if (lane < 3) {
    const double sum = lane == 0 ? cs[0] : (lane == 1 ? cs[1] : cs[2]);
    auto bexp = [](unsigned bits) {  // biased exponent of |x| given as bits, a denormal's as 1 (its ulp is that of exponent 1)
      const int e = (int)((bits >> 23) & 0xffu);
      return e ? e : 1;
    };
    int emin, emax;
    if (track) {
      const unsigned hi = lane == 0 ? umax[0] : (lane == 1 ? umax[1] : umax[2]), lo = lane == 0 ? umin[0] : (lane == 1 ? umin[1] : umin[2]);
      emax = hi ? bexp(hi) : 0;  // (no non-zero addend: emax = 0, the sum is exact)
      emin = hi ? bexp(lo + 1u) : 255;
    } else {
      const float aq = fabsf(lane == 0 ? qv[0] : (lane == 1 ? qv[1] : qv[2]));
      emax = bexp(__float_as_uint(aq + rad));       // |x| <= |q| + r: its exponent bounds every entry's from above ...
      emin = bexp(__float_as_uint(aq - rad)) - 1;   // ... |x| >= |q| - r > r from below (one binade of slack for the float subtraction)
    }
    P.cent[3 * (size_t)w + lane] = centre_exact(emin, emax, n) ? sum / (double)n : __longlong_as_double(0x7ff8000000000000ll);
  }
}

__global__ __launch_bounds__(64 * NL_WAVES) void normals_list_kernel(NormalsParams P) {
  __shared__ unsigned long long s_keys[NL_WAVES][NL_CAP];
  const int lane = threadIdx.x & 63;
  // the point of this wave, told to the compiler as what it is — wave-uniform: the cell ranges, column counts and loop
  // bounds derived from it then live in scalar registers and the visit's control flow is scalar branches (left as
  // per-lane values they became exec-mask regions with a vmcnt(0) at every join: the loads of a column batch were waited
  // for one by one)
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int w = P.w0 + blockIdx.x * NL_WAVES + wv;
  if (w >= P.w1) return;
  unsigned long long *keys = s_keys[wv];
  const float4 q4 = P.grid.p[w];
  const float qx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q4.x))),
              qy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q4.y))),
              qz = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(q4.z)));
  int n = 0;  // wave-uniform: the hits so far
  normals_visit(P, qx, qy, qz, lane, [&](bool hit, int i, float d2) {
    const unsigned long long ballot = __ballot(hit);
    const int pos = n + __popcll(ballot & ((1ull << lane) - 1ull));
    if (hit && pos < NL_CAP) keys[pos] = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)i;
    n += __popcll(ballot);
  });
  if (lane == 0) P.count[w] = n;
  if (n > NL_CAP) {  // a neighbourhood for the big kernel (it searches again)
    if (lane == 0) P.big[1 + atomicAdd(P.big, 1)] = w;
    return;
  }
  __threadfence_block();  // the keys were written by other lanes of this wave
  __builtin_amdgcn_wave_barrier();
  if (n <= 256)
    normals_sort_store<4>(P, keys, n, lane, w, q4);
  else if (n <= 512)
    normals_sort_store<8>(P, keys, n, lane, w, q4);
  else
    normals_sort_store<16>(P, keys, n, lane, w, q4);
}

// The queued points: a workgroup each (a persistent launch walks the queue, whose length stays on the device).  The list
// length is known from the first kernel; a slice of m = 2^ceil(log2 n) eight-byte units is drawn from the arena, the keys
// are sorted in LDS (m <= 8192) or in the slice itself, and the sorted indices are written over the slice's first 4 n
// bytes from the front: index t lands on key t / 2, which has been read by then.
__global__ __launch_bounds__(256) void normals_list_big_kernel(NormalsParams P) {
  __shared__ unsigned long long s_big[NL_BIG_LDS];
  __shared__ int s_count;
  __shared__ long long s_off;
  const int tid = threadIdx.x, lane = tid & 63;
  const int queued = P.big[0];
  for (int b = blockIdx.x; b < queued; b += gridDim.x) {
    const int w = P.big[1 + b];
    const int n = P.count[w];
    int m = 1;
    while (m < n) m <<= 1;
    __syncthreads();
    if (tid == 0) {
      s_count = 0;
      const long long off = (long long)atomicAdd(P.arena_top, (unsigned long long)m);
      s_off = off;
      P.big_off[w] = off;
      if (off + m > P.arena_cap) atomicOr(P.status, 1);
    }
    __syncthreads();
    const long long off = s_off;
    if (off + m > P.arena_cap) continue;  // the host grows the arena and runs again
    unsigned long long *slice = P.arena + off;
    unsigned long long *keys = m <= NL_BIG_LDS ? s_big : slice;
    const float4 q = P.grid.p[w];
    grid_visit(P.grid, q.x, q.y, q.z, P.reach, tid >> 6, 4, lane, [&](bool in, int i, float x, float y, float z) {
      float d = q.x - x;
      float d2 = 0.f;
      d2 += d * d;
      d = q.y - y;
      d2 += d * d;
      d = q.z - z;
      d2 += d * d;
      const bool hit = in && d2 < P.r2;
      const unsigned long long ballot = __ballot(hit);
      if (ballot) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_count, __popcll(ballot));
        base = __builtin_amdgcn_readfirstlane(base);
        if (hit) keys[base + __popcll(ballot & ((1ull << lane) - 1ull))] = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)i;
      }
    });
    for (int t = n + tid; t < m; t += 256) keys[t] = ~0ull;
    __threadfence_block();
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (m >> 1); t += 256) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int hi = lo | j;
          const bool up = (lo & k) == 0;
          const unsigned long long ka = keys[lo], kb = keys[hi];
          if ((ka > kb) == up) {
            keys[lo] = kb;
            keys[hi] = ka;
          }
        }
        __threadfence_block();
        __syncthreads();
      }
    int32_t *row = reinterpret_cast<int32_t *>(slice);
    for (int t0 = 0; t0 < n; t0 += 256) {
      const int t = t0 + tid;
      const int idx = t < n ? (int)(unsigned)keys[t] : 0;
      __syncthreads();  // every key of this batch has been read
      if (t < n) row[t] = idx;
      __threadfence_block();
      __syncthreads();
    }
  }
}

__global__ __launch_bounds__(64) void normals_finish_kernel(NormalsParams P) {
  const int w = P.w0 + blockIdx.x * 64 + threadIdx.x;
  if (w >= P.w1) return;
  if (*P.status & 1) return;  // the arena was too small: this run is repeated
  const int n = P.count[w];
  const float4 q = P.grid.p[w];
  const int pi = __float_as_int(q.w);
  constexpr int B = 16;  // list entries per batch; the next batch is requested before this one is summed
  // centroid: three sequential sums in neighbour order; covariance entries 00, 10, 11, 20, 21, 22 about it: six more
  double c0 = 0.0, c1 = 0.0, c2 = 0.0;
  double m00 = 0.0, m10 = 0.0, m11 = 0.0, m20 = 0.0, m21 = 0.0, m22 = 0.0;
  const float4 *col = P.lists + (size_t)((w - P.w0) >> 6) * NL_CAP * 64 + (w & 63);  // this point's column of its block's transposed lists
  int nmax = n;  // the longest list of this wave: the loop below is uniform, shorter lists are masked out arithmetically
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) nmax = max(nmax, __shfl_xor(nmax, o));
  nmax = __builtin_amdgcn_readfirstlane(nmax);
  if (nmax <= NL_CAP) {
    // The common case, straight-line: every lane's list is a column of the block's transposed array, so entry t of all 64
    // points is ONE contiguous kilobyte.  Two batches of 16 entries are in flight while one is summed; nothing in the loop
    // depends on a lane (addresses are clamped, a list that has ended adds +0.0 — exact: no sum here can be -0.0), so the
    // loads are counted, not waited for at branch joins.
    auto load = [&](int t0, float4 (&v)[B]) {
#pragma unroll
      for (int i = 0; i < B; i++) v[i] = col[(size_t)min(t0 + i, NL_CAP - 1) * 64];
    };
    // neighbouring points have neighbourhoods of similar size: up to the shortest list of the wave (rounded down to whole
    // rounds of three batches) no entry needs a mask — the masks are two v_cndmask per double, as many instructions as the
    // sums themselves, and this kernel is ONE wave per SIMD: its time is its instruction count
    int nmin = n;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) nmin = min(nmin, __shfl_xor(nmin, o));
    const int tfull = __builtin_amdgcn_readfirstlane(nmin) / (3 * B) * (3 * B);
    float4 ba[B], bb[B], bc[B];
    auto sum0 = [&](int t0, const float4 (&v)[B], bool masked) {
#pragma unroll
      for (int i = 0; i < B; i++) {
        const bool on = !masked || t0 + i < n;
        c0 += on ? (double)v[i].x : 0.0;
        c1 += on ? (double)v[i].y : 0.0;
        c2 += on ? (double)v[i].z : 0.0;
      }
    };
    auto sum1 = [&](int t0, const float4 (&v)[B], bool masked) {
#pragma unroll
      for (int i = 0; i < B; i++) {
        const bool on = !masked || t0 + i < n;
        const double d0 = on ? (double)v[i].x - c0 : 0.0, d1 = on ? (double)v[i].y - c1 : 0.0, d2 = on ? (double)v[i].z - c2 : 0.0;
        m00 += d0 * d0;
        m10 += d1 * d0;
        m11 += d1 * d1;
        m20 += d2 * d0;
        m21 += d2 * d1;
        m22 += d2 * d2;
      }
    };
#define NL_ROUND(SUM, MASKED)    \
  load(t0 + 2 * B, bc);          \
  SUM(t0, ba, MASKED);           \
  load(t0 + 3 * B, ba);          \
  SUM(t0 + B, bb, MASKED);       \
  load(t0 + 4 * B, bb);          \
  SUM(t0 + 2 * B, bc, MASKED);
    // (round 6) the centroid comes from normals_list_kernel, which summed it order-free under centre_exact's certificate; a lane
    // whose list failed it holds NaN, and only a wave with such a lane walks the three centroid chains (this pass read 223 of
    // the kernel's 447 MB per 30k points)
    c0 = P.cent[3 * (size_t)w + 0];
    c1 = P.cent[3 * (size_t)w + 1];
    c2 = P.cent[3 * (size_t)w + 2];
    int t0 = 0;
    if (__builtin_amdgcn_ballot_w64(c0 != c0 || c1 != c1 || c2 != c2) != 0ull) {
      const double k0 = c0, k1 = c1, k2 = c2;
      c0 = c1 = c2 = 0.0;
      load(0, ba);
      load(B, bb);
      for (; t0 < tfull; t0 += 3 * B) { NL_ROUND(sum0, false) }
      for (; t0 < nmax; t0 += 3 * B) { NL_ROUND(sum0, true) }
      c0 = k0 != k0 ? c0 / (double)n : k0;
      c1 = k1 != k1 ? c1 / (double)n : k1;
      c2 = k2 != k2 ? c2 / (double)n : k2;
    }
    load(0, ba);
    load(B, bb);
    for (t0 = 0; t0 < tfull; t0 += 3 * B) { NL_ROUND(sum1, false) }
    for (; t0 < nmax; t0 += 3 * B) { NL_ROUND(sum1, true) }
#undef NL_ROUND
  } else {
    // a wave with a queued point (more than NL_CAP neighbours): per-lane walks, each lane at its own pace
    const bool small = n <= NL_CAP;
    const int32_t *row = small ? nullptr : reinterpret_cast<const int32_t *>(P.arena + P.big_off[w]);
    auto at = [&](int t) { return small ? col[(size_t)t * 64] : P.pxyz[row[t]]; };
    for (int t = 0; t < n; t++) {
      const float4 v = at(t);
      c0 += (double)v.x;
      c1 += (double)v.y;
      c2 += (double)v.z;
    }
    c0 /= (double)n;
    c1 /= (double)n;
    c2 /= (double)n;
    for (int t = 0; t < n; t++) {
      const float4 v = at(t);
      const double d0 = (double)v.x - c0, d1 = (double)v.y - c1, d2 = (double)v.z - c2;
      m00 += d0 * d0;
      m10 += d1 * d0;
      m11 += d1 * d1;
      m20 += d2 * d0;
      m21 += d2 * d1;
      m22 += d2 * d2;
    }
  }
  double ev[3], Q[9];
  eigen3(m00, m10, m11, m20, m21, m22, ev, Q);
  int mn = 0;
  for (int k = 1; k < 3; k++)
    if (ev[k] < ev[mn]) mn = k;
  const double nx = mn == 0 ? Q[0] : (mn == 1 ? Q[1] : Q[2]), ny = mn == 0 ? Q[3] : (mn == 1 ? Q[4] : Q[5]),
               nz = mn == 0 ? Q[6] : (mn == 1 ? Q[7] : Q[8]);
  float o0 = 0.f, o1 = 0.f, o2 = 0.f;
  // estimated once, with the view point of the FIRST camera that sees the point (convertCameraSourceMatrixToLists,
  // cloud.cpp:606-620: `== 1` and a break); NormalEstimation::setViewPoint takes floats (cloud.cpp:513)
  for (int cam = 0; cam < P.num_cams; cam++) {
    if (P.cam_source[(size_t)cam * P.num_points + pi] != 1) continue;
    const double *vp = P.view_points + 3 * cam;
    const double dot = ((double)(float)vp[0] - (double)q.x) * nx + ((double)(float)vp[1] - (double)q.y) * ny + ((double)(float)vp[2] - (double)q.z) * nz;
    o0 = (float)(dot < 0 ? -nx : nx);
    o1 = (float)(dot < 0 ? -ny : ny);
    o2 = (float)(dot < 0 ? -nz : nz);
    break;
  }
  bool needs_reverse = true;  // reverseNormals (cloud.cpp:573-604)
  for (int cam = 0; cam < P.num_cams && needs_reverse; cam++) {
    if (P.cam_source[(size_t)cam * P.num_points + pi] != 1) continue;
    const double *vp = P.view_points + 3 * cam;
    const double d = (double)o0 * ((double)q.x - vp[0]) + (double)o1 * ((double)q.y - vp[1]) + (double)o2 * ((double)q.z - vp[2]);
    if (d < 0) needs_reverse = false;
  }
  if (needs_reverse) {
    o0 = (float)((double)o0 * -1.0);
    o1 = (float)((double)o1 * -1.0);
    o2 = (float)((double)o2 * -1.0);
  }
  P.out[3 * (size_t)pi + 0] = o0;
  P.out[3 * (size_t)pi + 1] = o1;
  P.out[3 * (size_t)pi + 2] = o2;
}

void normals_free(NormalsScratch &s) {
  device_release(s.d_count, s.d_lists, s.d_big, s.d_big_off, s.d_arena, s.d_ctl, s.d_out, s.d_cent);
  s = NormalsScratch();
}

// Host wrapper: normals of the uploaded cloud, result to the host and into the context's device copy.  Nothing waits
// for the device between the three kernels; the arena of the large neighbourhoods grows when a cloud needs more (the
// status word comes back with the result, and the run is repeated once with the size the first one asked for).
constexpr int kNormalsTile = 65536;  // points per pass of the normals kernels (a multiple of 64): their transposed lists are 1 GB

int normals_run(Cloud &c, double radius, float *normals_out, hipStream_t stream) {
  NormalsScratch &s = c.normals;
  const int P = c.num_points;
  if (P > s.cap_points) {
    note_alloc(__func__);
    unsigned long long *arena = s.d_arena;
    const long long arena_cap = s.arena_cap;
    s.d_arena = nullptr;
    normals_free(s);
    s.d_arena = arena;
    s.arena_cap = arena_cap;
    const int cap = slack_cap(P, 4);
    HIP_RET(device_alloc(s.d_count, (size_t)cap));
    // the transposed lists take 16 KB per point (1024 entries of 16 bytes; a point touches 16 B per neighbour): a tile of at
    // most kNormalsTile points at a time shares ONE such array (1 GB), whatever the size of the cloud — sized per point of
    // the whole cloud it was 10 GB for a 500k-point raw scan
    const size_t tile_pts = std::min<size_t>(((size_t)cap + 63) / 64 * 64, kNormalsTile);
    HIP_RET(device_alloc(s.d_lists, tile_pts * NL_CAP));
    HIP_RET(device_alloc(s.d_big, (size_t)cap + 1));
    HIP_RET(device_alloc(s.d_big_off, (size_t)cap));
    HIP_RET(device_alloc(s.d_ctl, 4));  // [0] arena top, [1] status
    HIP_RET(device_alloc(s.d_out, (size_t)cap * 3));
    HIP_RET(device_alloc(s.d_cent, (size_t)cap * 3));
    s.cap_points = cap;
  }
  if (!s.d_arena) {
    note_alloc(__func__);
    const long long want = 1ll << 20;  // 8 MB: a voxelised cloud needs none of it
    HIP_RET(device_alloc(s.d_arena, (size_t)want));
    s.arena_cap = want;
  }
  NormalsParams np;
  np.grid = grid_view(c);
  np.pxyz = c.pxyz;
  np.num_points = P;
  np.cam_source = c.cam_source;
  np.num_cams = c.num_cams;
  std::memcpy(np.view_points, c.view_points, sizeof(np.view_points));
  np.r2 = (float)(radius * radius);
  np.reach = (float)radius * 1.001f + 1e-5f;
  np.count = s.d_count;
  np.lists = s.d_lists;
  np.big = s.d_big;
  np.big_off = s.d_big_off;
  np.arena_top = s.d_ctl;
  np.status = reinterpret_cast<int32_t *>(s.d_ctl + 1);
  np.out = s.d_out;
  np.cent = s.d_cent;
  struct {
    unsigned long long top, status;
  } h = {0, 0};
  int32_t queued = 0;
  const int tiles = (P + kNormalsTile - 1) / kNormalsTile;
  std::vector<int32_t> tile_queued((size_t)tiles, 0);
  int attempts = 0;
  for (int attempt = 0; attempt < 2; attempt++) {
    attempts = attempt + 1;
    np.arena = s.d_arena;
    np.arena_cap = s.arena_cap;
    HIP_RET(hipMemsetAsync(s.d_out, 0, (size_t)P * 3 * sizeof(float), stream));
    unsigned long long top_max = 0, status_any = 0;
    queued = 0;
    for (int t = 0; t < tiles; t++) {
      // one tile of points: its lists, the queue of its large neighbourhoods and their arena slices, its sums — the lists array
      // and the arena are the next tile's again
      np.w0 = t * kNormalsTile;
      np.w1 = std::min(P, np.w0 + kNormalsTile);
      const int tp = np.w1 - np.w0;
      HIP_RET(hipMemsetAsync(s.d_ctl, 0, 2 * sizeof(unsigned long long), stream));
      HIP_RET(hipMemsetAsync(s.d_big, 0, sizeof(int32_t), stream));
      normals_list_kernel<<<(tp + NL_WAVES - 1) / NL_WAVES, 64 * NL_WAVES, 0, stream>>>(np);
      normals_list_big_kernel<<<256, 256, 0, stream>>>(np);
      normals_finish_kernel<<<(tp + 63) / 64, 64, 0, stream>>>(np);
      HIP_RET(hipGetLastError());
      if (tiles > 1 || t == tiles - 1) {
        HIP_RET(hipMemcpyAsync(&h, s.d_ctl, sizeof(h), hipMemcpyDeviceToHost, stream));
        HIP_RET(hipMemcpyAsync(&tile_queued[(size_t)t], s.d_big, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
        if (t == tiles - 1 && normals_out) HIP_RET(hipMemcpyAsync(normals_out, s.d_out, (size_t)P * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
        if (t == tiles - 1) {
          // the device copy of the cloud (planes nx, ny, nz) behind the last tile, before the ONE wait of the call (round 6: it
          // was a second launch + wait after this one); a run that has to be repeated for a larger arena rewrites it
          const int rc = cloud_set_normals(c, s.d_out, stream);
          if (rc) return rc;
        }
        HIP_RET(hipStreamSynchronize(stream));  // (several tiles: the control words are the next tile's)
        top_max = std::max(top_max, h.top);
        status_any |= h.status;
        queued += tile_queued[(size_t)t];
      }
    }
    h.top = top_max;
    h.status = status_any;
    if (!(h.status & 1)) break;
    // more / larger neighbourhoods beyond a wave's reach than the arena holds: grow it to what this run asked for
    note_alloc(__func__);
    device_release(s.d_arena);
    s.arena_cap = 0;
    const long long want = slack_cap((long long)h.top, 8);
    if (attempt == 1 || device_alloc(s.d_arena, (size_t)want) != hipSuccess) {
      (void)hipGetLastError();
      set_error("normals: the neighbour lists of this cloud (%llu sort slots within %.3f m) do not fit the device memory", h.top, radius);
      return GPD_ERR_CAPACITY;
    }
    s.arena_cap = want;
  }
  s.last_queued = queued;
  s.last_points = P;
  s.last_tiles = tiles;
  s.last_attempts = attempts;
  c.generation++;
  s.last_generation = c.generation;
  return GPD_OK;
}

// gpd_hip_last_normals_routes (tests only): what the last normals_run left on the device, read after the fact — the counts by
// cell-order position (every tile writes its own range of d_count and d_cent, so both hold the whole cloud), carried to the
// original index through the grid's point table, and the routes that follow from them by the kernels' own rules.  The stream
// has been waited for.
int normals_routes(const Cloud &c, int32_t *count, int n_room, long long info[8]) {
  const NormalsScratch &s = c.normals;
  const int P = s.last_points;
  if (P <= 0 || P != c.num_points || s.last_generation != c.generation) {
    set_error("gpd_hip_last_normals_routes: no gpd_hip_estimate_normals ran on the cloud the context holds");
    return GPD_ERR_STATE;
  }
  if (n_room < P) {
    set_error("gpd_hip_last_normals_routes: room for %d points, the last run had %d", n_room, P);
    return GPD_ERR_INVALID;
  }
  std::vector<int32_t> n((size_t)P);
  std::vector<float4> gp((size_t)P);
  std::vector<double> cent((size_t)P * 3);
  HIP_RET(hipMemcpy(n.data(), s.d_count, n.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  HIP_RET(hipMemcpy(gp.data(), c.g_p, gp.size() * sizeof(float4), hipMemcpyDeviceToHost));
  HIP_RET(hipMemcpy(cent.data(), s.d_cent, cent.size() * sizeof(double), hipMemcpyDeviceToHost));
  long long in_lds = 0, in_arena = 0, chains = 0;
  for (int w = 0; w < P; w++) {
    int32_t pi;
    std::memcpy(&pi, &gp[(size_t)w].w, sizeof(pi));
    if (pi < 0 || pi >= P) {
      set_error("gpd_hip_last_normals_routes: cell-order position %d holds the index %d (points: %d)", w, pi, P);
      return GPD_ERR_STATE;
    }
    count[pi] = n[(size_t)w];
    if (n[(size_t)w] > NL_CAP) {  // normals_list_big_kernel's choice of sort space
      long long m = 1;
      while (m < n[(size_t)w]) m <<= 1;
      (m <= NL_BIG_LDS ? in_lds : in_arena)++;
    } else {
      const double *k = &cent[3 * (size_t)w];
      chains += k[0] != k[0] || k[1] != k[1] || k[2] != k[2];
    }
  }
  info[0] = P;
  info[1] = s.last_tiles;
  info[2] = s.last_queued;
  info[3] = in_lds;
  info[4] = in_arena;
  info[5] = s.last_attempts;
  info[6] = s.arena_cap;
  info[7] = chains;
  return GPD_OK;
}

}  // namespace gpd
