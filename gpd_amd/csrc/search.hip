// Candidate search on gfx950: radius neighbourhoods and local frames, and the drivers of the search, of the
// ground-truth re-evaluation and of a label_view round.  (The cloud and its grid: cloud.hip; the normals: normals.hip;
// the hand kernels the drivers enqueue: hands.hip.)
//
// Replaces HandSearch::searchHands (candidate/hand_search.cpp:24-64, 144-188), FrameEstimator::calculateFrame
// (candidate/frame_estimator.cpp:66-86) and LocalFrame::findAverageNormalAxis (candidate/local_frame.cpp:14-41).
//
// neighbourhood_kernel   one workgroup per sample: visits the cells of a uniform 2 cm grid
//     around the sample (instead of walking PCL's k-d tree), collects the points with
//     d2 < r^2 (r = the largest of the hand / image / frame radii) in LDS and sorts them
//     by (d2, index) — FLANN's order — with a 1024-bucket counting sort whose buckets are
//     ordered through registers (bitonic sort in place for the 16384-entry retry); writes
//     the sorted neighbourhood gathered as SoA.  The three neighbourhoods are prefixes of
//     this list (same query point, same float d2, same sort).  Lane 0 then forms
//     M = sum n n^T in neighbour order and runs the 3x3 symmetric QR eigensolver
//     (Eigen's SelfAdjointEigenSolver algorithm, fp64, unfused: eigen3.h).
// centre_kernel          centre of the image neighbourhood, one lane per serial fp64 chain.
//
// All fp64 expressions are evaluated unfused, left to right (-ffp-contract=off),
// exactly as oracle/gpd_oracle.cpp defines them.
#include <cmath>
#include <cstdio>

#include "buffers.h"
#include "eigen3.h"
#include "gpd_internal.h"
#include "grid_sort.h"

namespace gpd {

// ---------------------------------------------------------------------------
// neighbourhood_kernel
// ---------------------------------------------------------------------------
struct NbParams {
  const float *px, *py, *pz, *nx, *ny, *nz;
  const float4 *pxyz, *pnrm;  // AoS copies: one 16-byte load per random access
  int num_points;
  const int32_t *sample_idx;
  const double *sample_xyz;  // non-null: samples by coordinates; the query is their float cast (eigenVectorToPcl)
  float r2_all, r2_hands, r2_images, r2_frames;  // r2_all = the largest: one search, the three neighbourhoods are prefixes
  int cap;  // list capacity; a power of two in bitonic mode
  int bucket;  // 1: bucket sort (keys + u16 slot table + 2 x 1024 counters in LDS), 0: in-place bitonic sort
  int32_t *counts;  // [S][8]: N_hands, N_images, k_frames, found, mask of cameras that see the image neighbourhood, -, -, -
  int32_t *nn_idx;
  float *nn;
  double *frames;
  double *centers;  // [S][3] mean of the image neighbourhood (hand_set.cpp:131-133)
  const int32_t *cam_source;
  int num_cams;
  GridView grid;
  float reach;  // half-edge of the cube of cells to visit (radius + margin)
  unsigned long long *dbg;  // profiling aid (GPD_NB_TIMING=1): per-phase cycle sums of wave 0
  // the height list of the hand search (the crop shared by a sample's orientations, see hl_note below), built by the
  // frame wave once the frame is known; hl == nullptr: not wanted (re-evaluation)
  float4 *hl;                       // [S][cap]: x, y, z, rank bits of the points that can be in-height for some orientation
  int hl_slots;
  double hl_col[GPD_MAX_SLOTS][3];  // third column of rot_binormal * rot[slot]: the slot's hand axis in the local frame
  double hl_height, hl_radius;
};

// ---- bucket sort of the (d2, index) keys -------------------------------------------------
// d2 < r2 maps monotonically to one of NB_BUCKETS buckets (about 3-5 keys each at the reference's
// radii); a counting sort groups the point indices bucket by bucket and every bucket is ordered
// through registers.  LDS holds two u32 arrays (visit order / bucket order of the indices; after
// the sort: d2 bits / indices, both sorted) — the same 64 KB as the u64 keys of the bitonic path,
// d2 is recomputed from the coordinates (bit-identical, L2 hits) instead of being stored twice.
// Five barriers instead of the 78 barrier-separated bitonic stages (648 of the kernel's 1320 us).
constexpr int NB_BUCKETS = 1024;
// 512 threads: sixteen waves per CU at two workgroups (72 KB of LDS each) — the kernel waits on dependent global
// loads (cell bounds -> points) and on its barriers, more waves in flight is what hides them
constexpr int NB_THREADS = 512, NB_WAVES = NB_THREADS / 64;
// The keys — (d2 bits << 32) | index, or ~0 for padding — are compared as DOUBLES: a d2 below r2 has float bits under
// 0x3f800000, so the key is the bit pattern of a non-negative finite (possibly denormal: f64 denormals are kept) double,
// and those order like the 64-bit integers; the padding must be a number too (a NaN would be dropped by both v_min_f64 and
// v_max_f64 in favour of the key, which would then appear twice): the largest finite double.  One compare-exchange = v_min_f64 + v_max_f64 instead of v_cmp_gt_u64 + four v_cndmask_b32.
template <int N>
__device__ inline void sort_regs64(unsigned long long (&k)[N]) {
  double d[N];
#pragma unroll
  for (int i = 0; i < N; i++) d[i] = __longlong_as_double((long long)k[i]);
#pragma unroll
  for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (int i = 0; i < N; i++) {
        const int j = i ^ stride;
        if (j > i) {
          const bool up = (i & size) == 0;
          const double lo = __builtin_fmin(d[i], d[j]), hi = __builtin_fmax(d[i], d[j]);
          d[i] = up ? lo : hi;
          d[j] = up ? hi : lo;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) k[i] = (unsigned long long)__double_as_longlong(d[i]);
}
// GLOBAL: the slow path for neighbourhoods beyond the LDS list capacities (the reference has no limit:
// hand_search.cpp:178 takes whatever radiusSearch returns).  The same bucket sort with the two index arrays in
// global memory — they live in the output rows themselves (sorted indices in nn_idx, d2 bits in the last nn row until
// the gather overwrites it) — and, LDS being free, 8192 buckets.
template <bool GLOBAL>
__global__ __launch_bounds__(NB_THREADS) void neighbourhood_kernel(NbParams P) {
  constexpr int NBK = GLOBAL ? 8192 : NB_BUCKETS;  // buckets
  constexpr int PER = NBK / NB_THREADS;           // per lane in the scan
  // workgroup-wide hand-over of the index arrays: a barrier, plus a fence when they are global memory
  auto hand_over = [] {
    if constexpr (GLOBAL) __threadfence_block();
    __syncthreads();
  };
  extern __shared__ __attribute__((aligned(16))) unsigned long long s_keys[];
  __shared__ int s_count;
  __shared__ int s_bounds[3];
  __shared__ int s_seen;
  __shared__ double s_csum[NB_WAVES][3];  // centre of the image neighbourhood: the waves' partial sums ...
  __shared__ int s_cexp[NB_WAVES][6];     // ... and the smallest / largest biased exponent among their non-zero addends
  __shared__ double s_hl_axis[4];  // height list: hand axis of slot 0 and the limit h + margin (published by the frame wave)
  __shared__ int s_hl_ready, s_hl_next, s_hl_count;
  __shared__ int s_ncrowd;
  // the frame wave's own list of the frame neighbourhood (d2 < r2_frames): keys (d2 bits, index) in visit order, the point
  // indices in FLANN order; s_fkf = their number once the frame is done (more than FCAP: -1, the frame waits for the workgroup's sorted list)
  constexpr int FCAP = 160;
  __shared__ unsigned long long s_fk[FCAP];
  __shared__ int s_fidx[FCAP];
  __shared__ int s_fkf;
  const int s = blockIdx.x;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  unsigned long long t_last = __builtin_readcyclecounter();
#define NTICK(k_)                                                    \
  do {                                                              \
    if (P.dbg && tid == 0) {                                        \
      const unsigned long long now_ = __builtin_readcyclecounter(); \
      atomicAdd(&P.dbg[k_], now_ - t_last);                         \
      t_last = now_;                                                \
    }                                                               \
  } while (0)
  float qx, qy, qz;
  double sx, sy, sz;  // the sample the hand frame keeps (frame_estimator.cpp:20-22, 53-54)
  if (P.sample_xyz) {
    sx = P.sample_xyz[3 * (size_t)s + 0];
    sy = P.sample_xyz[3 * (size_t)s + 1];
    sz = P.sample_xyz[3 * (size_t)s + 2];
    qx = (float)sx;
    qy = (float)sy;
    qz = (float)sz;
  } else {
    const int sidx = P.sample_idx[s];
    qx = P.px[sidx];
    qy = P.py[sidx];
    qz = P.pz[sidx];
    sx = (double)qx;
    sy = (double)qy;
    sz = (double)qz;
  }
  if (tid == 0) {
    s_count = 0;
    s_bounds[0] = 0;
    s_bounds[1] = 0;
    s_bounds[2] = 0;
    s_seen = 0;
    s_hl_ready = 0;
    s_hl_next = 0;
    s_hl_count = 0;
    s_ncrowd = 0;
    s_fkf = -1;
  }
  // bucket mode: two u32 arrays in the key storage, counters behind them
  uint32_t *s_a, *s_b;  // indices in visit order, then sorted d2 bits / indices in bucket order, then sorted
  int *s_hist;
  if constexpr (GLOBAL) {
    s_a = reinterpret_cast<uint32_t *>(P.nn + ((size_t)s * 6 + 5) * P.cap);
    s_b = reinterpret_cast<uint32_t *>(P.nn_idx + (size_t)s * P.cap);
    s_hist = reinterpret_cast<int *>(s_keys);
  } else {
    s_a = reinterpret_cast<uint32_t *>(s_keys);
    s_b = s_a + P.cap;
    s_hist = reinterpret_cast<int *>(s_keys + P.cap);
  }
  int *s_start = s_hist + NBK;  // NBK + 1 entries
  auto d2_of = [&](int i) {  // FLANN L2_Simple<float>, the same operation order as in the visit
    const float4 p = P.pxyz[i];
    float d = qx - p.x;
    float d2 = 0.f;
    d2 += d * d;
    d = qy - p.y;
    d2 += d * d;
    d = qz - p.z;
    d2 += d * d;
    return d2;
  };
  const float bscale = (float)NBK / P.r2_all;
  auto bucket_of = [&](float d2) {
    const int b = (int)(d2 * bscale);
    return b < NBK - 1 ? b : NBK - 1;
  };
  if (P.bucket)
    for (int i = tid; i < NBK; i += NB_THREADS) s_hist[i] = 0;
  __syncthreads();
  constexpr int VW = NB_WAVES - 1;  // visiting waves
  // frames (frame_estimator.cpp:66-86 + local_frame.cpp:14-41) from the kf nearest neighbours in FLANN order, idx_of(t) =
  // point index of the t-th; one whole wave.  M = sum n n^T and sum n are nine sequential fp64 chains in neighbour
  // order: the normals come in ONE round trip per 64 — lane t asks for the t-th neighbour's — and are handed to the
  // nine chain lanes through v_readlane (the same adds in the same order per chain); the wave's first lane runs the
  // eigensolver, stores the frame and, for the height list, publishes the hand axis of slot 0 and the limit.
  auto frame_of = [&](int kf, auto idx_of) {
    const int cp = lane == 0 ? 0 : lane == 1 ? 1 : lane == 2 ? 1 : lane == 3 ? 2 : lane == 4 ? 2 : lane == 5 ? 2 : lane == 6 ? 0 : lane == 7 ? 1 : 2;
    const int cq = lane == 0 ? 0 : lane == 1 ? 0 : lane == 2 ? 1 : lane == 3 ? 0 : lane == 4 ? 1 : lane == 5 ? 2 : -1;
    double acc = 0.0;
    for (int base = 0; base < kf; base += 64) {
      const int tl = base + lane;
      const float4 nl = P.pnrm[idx_of(tl < kf ? tl : base)];
      const int m = kf - base < 64 ? kf - base : 64;
      for (int u = 0; u < m; u++) {
        const float ux = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nl.x), u));
        const float uy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nl.y), u));
        const float uz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(nl.z), u));
        const float xs = cp == 0 ? ux : (cp == 1 ? uy : uz);
        const float ys = cq == 0 ? ux : (cq == 1 ? uy : uz);
        const double x = (double)xs;
        const double y = cq >= 0 ? (double)ys : 1.0;
        if (lane < 9) acc += x * y;
      }
    }
    auto chain = [&](int c) {
      const unsigned long long b = (unsigned long long)__double_as_longlong(acc);
      const unsigned lo = __shfl((unsigned)b, c), hi = __shfl((unsigned)(b >> 32), c);
      return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    };
    double m00 = chain(0), m10 = chain(1), m11 = chain(2), m20 = chain(3), m21 = chain(4), m22 = chain(5);
    double a0 = chain(6), a1 = chain(7), a2 = chain(8);
    double *f = P.frames + 12 * (size_t)s;
    if (lane == 0) {
      f[0] = sx;
      f[1] = sy;
      f[2] = sz;
      if (kf > 0) {
        double ev[3], Q[9];
        eigen3(m00, m10, m11, m20, m21, m22, ev, Q);
        int mn = 0, mx = 0;
        for (int i = 1; i < 3; i++) {
          if (ev[i] < ev[mn]) mn = i;
          if (ev[i] > ev[mx]) mx = i;
        }
        double curv[3], nor[3];
        for (int r = 0; r < 3; r++) {
          curv[r] = Q[3 * r + mn];
          nor[r] = Q[3 * r + mx];
        }
        const double nrm = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
        a0 /= nrm;
        a1 /= nrm;
        a2 /= nrm;
        const double dot = a0 * nor[0] + a1 * nor[1] + a2 * nor[2];
        if (dot < 0)
          for (int r = 0; r < 3; r++) nor[r] *= -1.0;
        f[3] = nor[0];
        f[4] = nor[1];
        f[5] = nor[2];
        f[6] = curv[1] * nor[2] - curv[2] * nor[1];
        f[7] = curv[2] * nor[0] - curv[0] * nor[2];
        f[8] = curv[0] * nor[1] - curv[1] * nor[0];
        f[9] = curv[0];
        f[10] = curv[1];
        f[11] = curv[2];
      }
    }
    // hl_note.  The height crop shared by the orientations of a sample: cropByHandHeight (point_list.cpp:35-55) keeps the
    // points whose coordinate along the hand frame's third axis lies in (-h, h); that axis is the one the orientations
    // rotate about, so the frames of a sample's slots have the same third column up to rounding.  The points with
    // |z| < h + margin for the axis of slot 0 — margin = (largest deviation of any slot's axis from it) x radius + 1e-12,
    // a superset of every orientation's exact crop, which hand_eval_kernel then decides with its own frame — are listed
    // in this kernel, by the gathering waves as they pass (coordinates in registers; order of the list: none, the entries
    // carry their rank).  This was a kernel of its own that read the gathered rows back from HBM (110 MB per 2564
    // samples), then a pass of its own behind the frame.
    if (P.hl && kf > 0) {
      auto bc = [&](double v) {  // lane 0's value to the wave
        const unsigned long long b = (unsigned long long)__double_as_longlong(v);
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)b), hi = __builtin_amdgcn_readfirstlane((unsigned)(b >> 32));
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
      };
      // lane 0 holds the frame it has just stored: F = [normal | binormal | curvature] (hand_set.cpp:39-40)
      double F[9];
      __threadfence_block();
#pragma unroll
      for (int r = 0; r < 3; r++) {
        F[3 * r + 0] = bc(lane == 0 ? f[3 + r] : 0.0);
        F[3 * r + 1] = bc(lane == 0 ? f[6 + r] : 0.0);
        F[3 * r + 2] = bc(lane == 0 ? f[9 + r] : 0.0);
      }
      double axis[3] = {0.0, 0.0, 0.0}, dev = 0.0;
      for (int slot = 0; slot < P.hl_slots; slot++) {
        double a[3];
#pragma unroll
        for (int r = 0; r < 3; r++)
          a[r] = F[3 * r] * P.hl_col[slot][0] + F[3 * r + 1] * P.hl_col[slot][1] + F[3 * r + 2] * P.hl_col[slot][2];
        if (slot == 0) {
          axis[0] = a[0];
          axis[1] = a[1];
          axis[2] = a[2];
        }
        dev = fmax(dev, fabs(a[0] - axis[0]) + fabs(a[1] - axis[1]) + fabs(a[2] - axis[2]));
      }
      if (lane == 0) {
        s_hl_axis[0] = axis[0];
        s_hl_axis[1] = axis[1];
        s_hl_axis[2] = axis[2];
        s_hl_axis[3] = P.hl_height + dev * P.hl_radius + 1e-12;
      }
    }
  };
  auto early_frame = [&] {
    // the cells within the frame radius (same distance arithmetic as the visit), hits appended to s_fk in visit order
    const float rfr = sqrtf(P.r2_frames) * 1.001f + 1e-5f;
    int fn = 0;  // hits so far: the same in every lane (it only ever grows by a ballot's population)
    auto visit_f = [&](bool in, int i, float x, float y, float z) {
      float d = qx - x;
      float d2 = 0.f;
      d2 += d * d;
      d = qy - y;
      d2 += d * d;
      d = qz - z;
      d2 += d * d;
      const bool hit = in && d2 < P.r2_frames;
      const unsigned long long ballot = __ballot(hit);
      if (hit) {
        const int pos = fn + __popcll(ballot & ((1ull << lane) - 1ull));
        if (pos < FCAP) s_fk[pos] = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)i;
      }
      fn += __popcll(ballot);
    };
    {
      const GridView &g = P.grid;
      const int x0 = grid_coord(g, 0, qx - rfr), x1 = grid_coord(g, 0, qx + rfr);
      const int y0 = grid_coord(g, 1, qy - rfr), y1 = grid_coord(g, 1, qy + rfr);
      const int z0 = grid_coord(g, 2, qz - rfr), z1 = grid_coord(g, 2, qz + rfr);
      const int ny = y1 - y0 + 1;
      const int ncol = (x1 - x0 + 1) * ny;
      if (ncol <= 64) {
        // the point ranges of all columns in one round trip (a lane per column), then four columns' points at a time
        int cbv = 0, cev = 0;
        if (lane < ncol) {
          const int cx = x0 + lane / ny, cy = y0 + lane % ny;
          const int cbase = (cx * g.dim[1] + cy) * g.dim[2];
          cbv = g.start[cbase + z0];
          cev = g.start[cbase + z1 + 1];
        }
        for (int c0 = 0; c0 < ncol; c0 += 4) {
          int cb[4], ce[4];
          float4 p[4];
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int col = c0 + q < ncol ? c0 + q : c0;
            cb[q] = __builtin_amdgcn_readlane(cbv, col);
            ce[q] = c0 + q < ncol ? __builtin_amdgcn_readlane(cev, col) : cb[q];
          }
#pragma unroll
          for (int q = 0; q < 4; q++) {
            const int t = cb[q] + lane;
            p[q] = g.p[t < ce[q] ? t : 0];
          }
#pragma unroll
          for (int q = 0; q < 4; q++)
            if (cb[q] < ce[q]) visit_f(cb[q] + lane < ce[q], __float_as_int(p[q].w), p[q].x, p[q].y, p[q].z);
#pragma unroll
          for (int q = 0; q < 4; q++)
            for (int t0 = cb[q] + 64; t0 < ce[q]; t0 += 64) {
              const int t = t0 + lane;
              const bool in = t < ce[q];
              const float4 pt = g.p[in ? t : cb[q]];
              visit_f(in, __float_as_int(pt.w), pt.x, pt.y, pt.z);
            }
        }
      } else {
        grid_visit(g, qx, qy, qz, rfr, 0, 1, lane, visit_f);
      }
    }
    const int kf = fn;
    if (kf > FCAP) return;  // left to the sorted list (the late path below)
    __threadfence_block();  // the keys were written by other lanes of this wave
    __builtin_amdgcn_wave_barrier();
    // FLANN's order, (d2, index) ascending: the rank of a key is the number of smaller keys (they are distinct)
    constexpr int KPL = (FCAP + 63) / 64;
    unsigned long long mine[KPL];
    int rank[KPL];
#pragma unroll
    for (int q = 0; q < KPL; q++) {
      mine[q] = lane + 64 * q < kf ? s_fk[lane + 64 * q] : ~0ull;
      rank[q] = 0;
    }
    for (int u = 0; u < kf; u++) {
      const unsigned long long ku = s_fk[u];
#pragma unroll
      for (int q = 0; q < KPL; q++) rank[q] += ku < mine[q] ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < KPL; q++)
      if (lane + 64 * q < kf) s_fidx[rank[q]] = (int)(unsigned)mine[q];
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    frame_of(kf, [&](int t) { return s_fidx[t]; });
    if (lane == 0) s_fkf = kf;
  };
  // 1. visit the grid cells around the sample; FLANN L2_Simple<float>: d2 accumulated over x,y,z, strict <.
  //    The point ranges of the (x, y) cell columns are fetched up front, one column per lane, into LDS (a column holds
  //    ~45 points: one dependent global round trip less per column and wave).
  auto visit = [&](bool in, int i, float x, float y, float z) {
    float d = qx - x;
    float d2 = 0.f;
    d2 += d * d;
    d = qy - y;
    d2 += d * d;
    d = qz - z;
    d2 += d * d;
    const bool hit = in && d2 < P.r2_all;
    const unsigned long long ballot = __ballot(hit);
    if (ballot) {
      int base = 0;
      if (lane == 0) base = atomicAdd(&s_count, __popcll(ballot));
      base = __builtin_amdgcn_readfirstlane(base);  // every lane is active here and lane 0 holds it
      if (hit) {
        const int pos = base + __popcll(ballot & ((1ull << lane) - 1ull));
        if (pos < P.cap) {
          if (P.bucket) {
            if constexpr (GLOBAL) {
              s_a[pos] = (uint32_t)i;  // d2 is recomputed by the scatter (a thread's entries do not fit its registers)
            } else {
              s_a[pos] = __float_as_uint(d2);  // visit order; the scatter below re-orders both arrays in place
              s_b[pos] = (uint32_t)i;
            }
            atomicAdd(&s_hist[bucket_of(d2)], 1);
          } else {
            s_keys[pos] = ((unsigned long long)__float_as_uint(d2) << 32) | (unsigned)i;
          }
        }
      }
    }
  };
  {
    const GridView &g = P.grid;
    const int x0 = grid_coord(g, 0, qx - P.reach), x1 = grid_coord(g, 0, qx + P.reach);
    const int y0 = grid_coord(g, 1, qy - P.reach), y1 = grid_coord(g, 1, qy + P.reach);
    const int z0 = grid_coord(g, 2, qz - P.reach), z1 = grid_coord(g, 2, qz + P.reach);
    const int ny = y1 - y0 + 1;
    const int ncol = (x1 - x0 + 1) * ny;
    __shared__ int s_cb[NB_THREADS], s_ce[NB_THREADS];
    if (ncol <= NB_THREADS) {
      if (tid < ncol) {
        const int cx = x0 + tid / ny, cy = y0 + tid % ny;
        const int cbase = (cx * g.dim[1] + cy) * g.dim[2];
        s_cb[tid] = g.start[cbase + z0];
        s_ce[tid] = g.start[cbase + z1 + 1];
      }
      __syncthreads();
      // four columns of the wave at a time: the first 64 points of each are requested together, then visited (a column per
      // iteration was one dependent global round trip per column, 18 in a row per wave: 30 of the kernel's ~110 kcycles);
      // the few columns with more than 64 points finish in the tail loop.  The visit order is free: the list is sorted.
      constexpr int CU_ = 4;
      if ((tid >> 6) < VW)
      for (int c0 = tid >> 6; c0 < ncol; c0 += CU_ * VW) {
        int cb[CU_], ce[CU_];
        float4 p[CU_];
#pragma unroll
        for (int q = 0; q < CU_; q++) {
          const int col = c0 + q * VW;
          cb[q] = col < ncol ? s_cb[col] : 0;
          ce[q] = col < ncol ? s_ce[col] : 0;
        }
#pragma unroll
        for (int q = 0; q < CU_; q++) {
          const int t = cb[q] + lane;
          p[q] = g.p[t < ce[q] ? t : 0];
        }
#pragma unroll
        for (int q = 0; q < CU_; q++)
          if (cb[q] < ce[q]) visit(cb[q] + lane < ce[q], __float_as_int(p[q].w), p[q].x, p[q].y, p[q].z);
#pragma unroll
        for (int q = 0; q < CU_; q++)
          for (int t0 = cb[q] + 64; t0 < ce[q]; t0 += 64) {
            const int t = t0 + lane;
            const bool in = t < ce[q];
            const float4 pt = g.p[in ? t : cb[q]];
            visit(in, __float_as_int(pt.w), pt.x, pt.y, pt.z);
          }
      }
    } else if ((tid >> 6) < VW) {
      grid_visit(g, qx, qy, qz, P.reach, tid >> 6, VW, lane, visit);
    }
  }
  // The last wave does not visit: it finds the frame neighbourhood on its own (the few cells within the frame radius,
  // ~40 points), orders it and computes the local frame while the other seven walk the 144 cell columns — the 3 x 3
  // eigensolver is a chain of ~2-3 k dependent f64 instructions on one lane, and started after the sort it kept the
  // gathering waves waiting at the end of the kernel (GPD_NB_TIMING: 7 of 108 kcycles) and the height list behind it.
  if ((tid >> 6) == VW) early_frame();
  hand_over();
  NTICK(0);
  const int found = s_count;
  const int n = found < P.cap ? found : P.cap;
  if (P.bucket) {
    // 2. bucket sort: exclusive scan of the counters (PER buckets per lane) ...
    __shared__ int s_wsum[NB_WAVES];
    int c4[PER], sum = 0;
#pragma unroll
    for (int q = 0; q < PER; q++) {
      c4[q] = s_hist[PER * tid + q];
      sum += c4[q];
    }
    int incl = sum;  // wave-wide inclusive prefix sum through DPP (row_shr 1 / 2 / 4 / 8, then the row totals by row_bcast)
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x111, 0xf, 0xf, false);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x112, 0xf, 0xf, false);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x114, 0xf, 0xf, false);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x118, 0xf, 0xf, false);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x142, 0xa, 0xf, false);
    incl += __builtin_amdgcn_update_dpp(0, incl, 0x143, 0xc, 0xf, false);
    if (lane == 63) s_wsum[tid >> 6] = incl;
    __syncthreads();
    int run = incl - sum;
    for (int w = 0; w < (tid >> 6); w++) run += s_wsum[w];
#pragma unroll
    for (int q = 0; q < PER; q++) {
      s_start[PER * tid + q] = run;
      s_hist[PER * tid + q] = run;  // the scatter cursor
      run += c4[q];
    }
    if (tid == NB_THREADS - 1) s_start[NBK] = run;
    __syncthreads();
    NTICK(1);
    // ... entries grouped bucket by bucket ...
    if constexpr (GLOBAL) {
      for (int t = tid; t < n; t += NB_THREADS) {
        const uint32_t i = s_a[t];
        const int pos = atomicAdd(&s_hist[bucket_of(d2_of((int)i))], 1);
        if (pos < n) s_b[pos] = i;  // always true (the counters come from the same d2 values); keeps a corrupted table out of memory
      }
    } else {
      // in place: a thread takes its (at most 16) entries into registers, everybody waits, then they go to their bucket
      // positions in the same two arrays — no second look at the coordinates
      constexpr int EPT = 8192 / NB_THREADS;
      uint32_t rd[EPT], ri[EPT];
#pragma unroll
      for (int q = 0; q < EPT; q++) {
        const int t = tid + q * NB_THREADS;
        rd[q] = t < n ? s_a[t] : 0u;
        ri[q] = t < n ? s_b[t] : 0u;
      }
      __syncthreads();
#pragma unroll
      for (int q = 0; q < EPT; q++) {
        const int t = tid + q * NB_THREADS;
        if (t < n) {
          const int pos = atomicAdd(&s_hist[bucket_of(__uint_as_float(rd[q]))], 1);
          if (pos < n) {
            s_a[pos] = rd[q];
            s_b[pos] = ri[q];
          }
        }
      }
    }
    hand_over();
    NTICK(2);
    // ... and every bucket ordered by (d2 bits, index); non-negative floats order as unsigned.  The d2 bits are
    // in s_a already (LDS mode) or recomputed into it (GLOBAL).
    auto d2bits_of_entry = [&](int x) {
      if constexpr (GLOBAL) return __float_as_uint(d2_of((int)s_b[x]));
      else return s_a[x];
    };
    for (int b = tid; b < NBK; b += NB_THREADS) {
      const int st = s_start[b], nb = s_start[b + 1] - st;
      if (nb <= 0) continue;
      auto run = [&](auto tag) {
        constexpr int N = decltype(tag)::value;
        unsigned long long k[N];
#pragma unroll
        for (int q = 0; q < N; q++) {
          const int x = st + (q < nb ? q : 0);
          k[q] = q < nb ? ((unsigned long long)d2bits_of_entry(x) << 32) | s_b[x] : 0x7fefffffffffffffull;  // padding: the largest finite double
        }
        sort_regs64<N>(k);
#pragma unroll
        for (int q = 0; q < N; q++)
          if (q < nb) {
            s_a[st + q] = (uint32_t)(k[q] >> 32);
            s_b[st + q] = (uint32_t)k[q];
          }
      };
      if (nb <= 4)
        run(std::integral_constant<int, 4>());
      else if (nb <= 8)
        run(std::integral_constant<int, 8>());
      else if (nb <= 16)
        run(std::integral_constant<int, 16>());
      else {
        // crowded bucket (lattice clouds put dozens of points at exactly the same distance): left
        // to a whole wave below
        const int c = atomicAdd(&s_ncrowd, 1);
        if (c < NBK) s_hist[c] = b;  // the scatter cursors are dead: their storage lists the crowded buckets
      }
    }
    __syncthreads();
    NTICK(3);
    const int ncrowd = s_ncrowd < NBK ? s_ncrowd : NBK;
    for (int c = tid >> 6; c < ncrowd; c += NB_WAVES) {
      const int b = s_hist[c];
      const int st = s_start[b], nb = s_start[b + 1] - st;
      if (nb <= 64) {
        // one key per lane, bitonic network across the wave
        unsigned long long k = lane < nb ? ((unsigned long long)d2bits_of_entry(st + lane) << 32) | s_b[st + lane] : ~0ull;
#pragma unroll
        for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
          for (int stride = size >> 1; stride > 0; stride >>= 1) {
            const unsigned lo = __shfl_xor((unsigned)k, stride), hi = __shfl_xor((unsigned)(k >> 32), stride);
            const unsigned long long other = ((unsigned long long)hi << 32) | lo;
            const bool keep_min = ((lane & stride) == 0) == ((lane & size) == 0);
            k = keep_min ? (k < other ? k : other) : (k > other ? k : other);
          }
        }
        if (lane < nb) {
          s_a[st + lane] = (uint32_t)(k >> 32);
          s_b[st + lane] = (uint32_t)k;
        }
      } else {
        // more than 64 keys in one bucket (dense clouds; lattice clouds put many points at exactly the same distance):
        // the d2 column first, then a bitonic network over the two arrays by the whole wave.  Every comparison
        // sorts upwards (the first step of each merge pairs x with its mirror image), so positions past the end
        // would hold +inf and never move: those comparisons are simply left out.
        if constexpr (GLOBAL)
          for (int x = lane; x < nb; x += 64) s_a[st + x] = __float_as_uint(d2_of((int)s_b[st + x]));
        int m = 1;
        while (m < nb) m <<= 1;
        auto exchange = [&](int lo, int hi) {
          if (hi < nb) {
            const unsigned long long klo = ((unsigned long long)s_a[st + lo] << 32) | s_b[st + lo];
            const unsigned long long khi = ((unsigned long long)s_a[st + hi] << 32) | s_b[st + hi];
            if (klo > khi) {
              s_a[st + lo] = (uint32_t)(khi >> 32);
              s_b[st + lo] = (uint32_t)khi;
              s_a[st + hi] = (uint32_t)(klo >> 32);
              s_b[st + hi] = (uint32_t)klo;
            }
          }
        };
        auto wave_sync = [] {
          __threadfence_block();
          __builtin_amdgcn_wave_barrier();
        };
        for (int size = 2; size <= m; size <<= 1) {
          wave_sync();
          const int half = size >> 1;
          for (int t = lane; t < (m >> 1); t += 64) {
            const int blk = t / half, off = t - blk * half;
            exchange(blk * size + off, blk * size + size - 1 - off);
          }
          for (int stride = size >> 2; stride > 0; stride >>= 1) {
            wave_sync();
            for (int t = lane; t < (m >> 1); t += 64) {
              const int lo = ((t & ~(stride - 1)) << 1) | (t & (stride - 1));
              exchange(lo, lo + stride);
            }
          }
        }
      }
    }
    hand_over();
    NTICK(4);
  } else {
    int m = 1;
    while (m < n) m <<= 1;
    for (int i = n + tid; i < m; i += NB_THREADS) s_keys[i] = ~0ull;
    __syncthreads();
    // 2. bitonic sort ascending by (d2 bits, index); non-negative floats order as unsigned
    for (int k = 2; k <= m; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (m >> 1); t += NB_THREADS) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
          const int hi = lo | j;
          const bool up = (lo & k) == 0;
          const unsigned long long a = s_keys[lo], b = s_keys[hi];
          if ((a > b) == up) {
            s_keys[lo] = b;
            s_keys[hi] = a;
          }
        }
        __syncthreads();
      }
    }
  }
  // sorted position t -> d2 bits / point index
  auto d2bits_at = [&](int t) { return P.bucket ? s_a[t] : (unsigned)(s_keys[t] >> 32); };
  auto index_at = [&](int t) { return P.bucket ? (int)s_b[t] : (int)(unsigned)(s_keys[t] & 0xffffffffull); };
  // 3. prefix lengths of the image, frame and hand-search neighbourhoods
  const unsigned ri = __float_as_uint(P.r2_images), rf = __float_as_uint(P.r2_frames), rh = __float_as_uint(P.r2_hands);
  for (int t = tid; t < n; t += NB_THREADS) {
    const unsigned d = d2bits_at(t);
    const unsigned dn = (t + 1 < n) ? d2bits_at(t + 1) : 0xffffffffu;
    if (d < ri && dn >= ri) s_bounds[0] = t + 1;
    if (d < rf && dn >= rf) s_bounds[1] = t + 1;
    if (d < rh && dn >= rh) s_bounds[2] = t + 1;
  }
  __syncthreads();
  NTICK(5);
  // 4. sorted index list + gathered SoA neighbourhood, and the height list of the hand search on the way
  // (the sorted index list itself has no reader on the device: nn_idx is the GLOBAL mode's scratch only — 43 MB of the
  //  303 MB this phase used to write per 2564 samples)
  float *on = P.nn + (size_t)s * 6 * P.cap;
  const int n_img = s_bounds[0], kf = s_bounds[1], Nh = s_bounds[2];
  // the frame wave's own neighbourhood must be the sorted list's prefix; when it is not there (more than FCAP points
  // inside the frame radius) or differs, the frame is computed from the sorted list after the gather, as it used to be
  const bool late = s_fkf != kf;
  if (tid == 0) {
    P.counts[8 * s + 0] = Nh;
    P.counts[8 * s + 1] = n_img;
    P.counts[8 * s + 2] = kf;
    P.counts[8 * s + 3] = found;
  }
  const bool list_here = P.hl && !late && kf > 0 && Nh > 0;
  const double ax0 = s_hl_axis[0], ax1 = s_hl_axis[1], ax2 = s_hl_axis[2], lim = s_hl_axis[3];  // (read by list_here only)
  float4 *hl_out = P.hl ? P.hl + (size_t)s * P.cap : nullptr;
  int seen = 0;
  // Two entries per thread and round, and the loads of round r + 1 are requested BEFORE the stores of round r go out
  // (two register sets, A and B): gfx9 counts loads and stores in one in-order counter, so a round that stores first and
  // then asks for the next points waits for its 14 store acknowledgements before it sees them.  The first camera's
  // flag comes with the coordinates (pxyz.w).
  constexpr int GT = NB_THREADS;  // every wave gathers
  // Centre of the image neighbourhood (HandSet::calculateShadow, hand_set.cpp:131-133: points.rowwise().sum() / size; the oracle
  // defines the sum sequentially in neighbour order, Eigen reduces in packets).  The addends are floats: when every addend is
  // a multiple of 2^L and n x max|x| < 2^(L + 53), EVERY partial sum of EVERY summation order is exact in fp64 — the
  // sequential chain, Eigen's, and the order-free one taken here on the way (each thread its entries, then the waves, then
  // the workgroup).  The certificate is two exponents per coordinate (see centre_exact); a sample that fails it — a point within
  // micrometres of a coordinate plane among points decimetres away — is flagged and gets its serial chain from centre_kernel.
  // (That kernel used to walk all 3 S chains from the gathered rows: 93 MB read back, 0.12-0.13 ms on a side stream.)
  double csum[3] = {0.0, 0.0, 0.0};
  int cemin[3] = {255, 255, 255}, cemax[3] = {0, 0, 0};
  auto centre_add = [&](const float4 &a) {
    const float v[3] = {a.x, a.y, a.z};
#pragma unroll
    for (int c = 0; c < 3; c++) {
      csum[c] += (double)v[c];
      const int e = (int)((__float_as_uint(v[c]) >> 23) & 0xffu);
      const bool nz = (__float_as_uint(v[c]) & 0x7fffffffu) != 0u;
      const int el = e ? e : 1;  // a denormal's ulp is that of exponent 1
      cemin[c] = nz && el < cemin[c] ? el : cemin[c];
      cemax[c] = nz && el > cemax[c] ? el : cemax[c];
    }
  };
  struct Rnd {
    int t0, i0, i1, c0, c1;
    float4 a0, b0, a1, b1;
  };
  auto fetch = [&](int t0, Rnd &r) {
    r.t0 = t0;
    const int t1 = t0 + GT;
    r.i0 = index_at(t0 < n ? t0 : 0);
    r.i1 = index_at(t1 < n ? t1 : 0);
    r.a0 = P.pxyz[r.i0];
    r.b0 = P.pnrm[r.i0];
    r.a1 = P.pxyz[r.i1];
    r.b1 = P.pnrm[r.i1];
    r.c0 = __float_as_int(r.a0.w);  // the first camera's flag (split_soa_kernel)
    r.c1 = __float_as_int(r.a1.w);
  };
  auto put = [&](const Rnd &r) {  // (wave-uniform control flow around the ballots)
    const int t0 = r.t0, t1 = r.t0 + GT;
    const bool one = t0 < n, two = t1 < n;
    if (one) {
      on[0 * P.cap + t0] = r.a0.x;
      on[1 * P.cap + t0] = r.a0.y;
      on[2 * P.cap + t0] = r.a0.z;
      on[3 * P.cap + t0] = r.b0.x;
      on[4 * P.cap + t0] = r.b0.y;
      on[5 * P.cap + t0] = r.b0.z;
      if (t0 < n_img) {
        seen |= (int)(r.c0 != 0);
        centre_add(r.a0);
      }
    }
    if (two) {
      on[0 * P.cap + t1] = r.a1.x;
      on[1 * P.cap + t1] = r.a1.y;
      on[2 * P.cap + t1] = r.a1.z;
      on[3 * P.cap + t1] = r.b1.x;
      on[4 * P.cap + t1] = r.b1.y;
      on[5 * P.cap + t1] = r.b1.z;
      if (t1 < n_img) {
        seen |= (int)(r.c1 != 0);
        centre_add(r.a1);
      }
    }
    for (int cam = 1; cam < P.num_cams; cam++) {  // further cameras: not pipelined
      if (one && t0 < n_img) seen |= (int)((unsigned)(P.cam_source[(size_t)cam * P.num_points + r.i0] != 0) << cam);
      if (two && t1 < n_img) seen |= (int)((unsigned)(P.cam_source[(size_t)cam * P.num_points + r.i1] != 0) << cam);
    }
    if (list_here && (t0 & ~63) < Nh) {  // uniform: some entry of the wave's first row is a hand-search neighbour
      bool ina = false, inb = false;
      if (t0 < Nh) {
        const double za = ax0 * ((double)r.a0.x - sx) + ax1 * ((double)r.a0.y - sy) + ax2 * ((double)r.a0.z - sz);
        ina = za > -lim && za < lim;
      }
      if (t1 < Nh) {
        const double zb = ax0 * ((double)r.a1.x - sx) + ax1 * ((double)r.a1.y - sy) + ax2 * ((double)r.a1.z - sz);
        inb = zb > -lim && zb < lim;
      }
      const unsigned long long ba = __ballot(ina), bb = __ballot(inb);
      if (ba | bb) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_hl_count, __popcll(ba) + __popcll(bb));
        base = __builtin_amdgcn_readfirstlane(base);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (ina) hl_out[base + __popcll(ba & below)] = make_float4(r.a0.x, r.a0.y, r.a0.z, __int_as_float(t0));
        if (inb) hl_out[base + __popcll(ba) + __popcll(bb & below)] = make_float4(r.a1.x, r.a1.y, r.a1.z, __int_as_float(t1));
      }
    }
  };
  if (n > 0) {
    Rnd A, B;
    fetch(tid, A);
    for (int t0 = tid; (t0 & ~63) < n; t0 += 4 * GT) {  // whole waves stay in the loop (the ballots in put)
      fetch(t0 + 2 * GT, B);
      __builtin_amdgcn_sched_barrier(0);
      put(A);
      __builtin_amdgcn_sched_barrier(0);
      fetch(t0 + 4 * GT, A);
      __builtin_amdgcn_sched_barrier(0);
      put(B);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  if (seen) atomicOr(&s_seen, seen);
  {  // the wave's share of the centre sums (exact under the certificate, discarded otherwise)
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        csum[c] += __shfl_xor(csum[c], o);
        cemin[c] = min(cemin[c], __shfl_xor(cemin[c], o));
        cemax[c] = max(cemax[c], __shfl_xor(cemax[c], o));
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        s_csum[tid >> 6][c] = csum[c];
        s_cexp[tid >> 6][c] = cemin[c];
        s_cexp[tid >> 6][3 + c] = cemax[c];
      }
    }
  }
  NTICK(6);
  if (late) {
    // 5'. the frame from the sorted list (more than FCAP points inside the frame radius), then the height list as a pass
    //     of its own: every wave takes chunks of 128 hand-search neighbours until none is left
    if ((tid >> 6) == VW) {
      frame_of(kf, index_at);
      __threadfence_block();
      if (lane == 0) *(volatile int *)&s_hl_ready = 1;
    }
    if (P.hl) {
      while (*(volatile int *)&s_hl_ready == 0) __builtin_amdgcn_s_sleep(2);
      __threadfence_block();
      NTICK(8);
      const double lx0 = s_hl_axis[0], lx1 = s_hl_axis[1], lx2 = s_hl_axis[2], llim = s_hl_axis[3];
      while (kf > 0 && Nh > 0) {
        int chunk = 0;
        if (lane == 0) chunk = atomicAdd(&s_hl_next, 1);
        const int e0 = __builtin_amdgcn_readfirstlane(chunk) * 128;
        if (e0 >= Nh) break;
        const int ea = e0 + lane, eb = e0 + 64 + lane;  // two entries per lane: their loads are in flight together
        const float4 pa = P.pxyz[index_at(ea < Nh ? ea : Nh - 1)], pb = P.pxyz[index_at(eb < Nh ? eb : Nh - 1)];
        const double za = lx0 * ((double)pa.x - sx) + lx1 * ((double)pa.y - sy) + lx2 * ((double)pa.z - sz);
        const double zb = lx0 * ((double)pb.x - sx) + lx1 * ((double)pb.y - sy) + lx2 * ((double)pb.z - sz);
        const bool ina = ea < Nh && za > -llim && za < llim, inb = eb < Nh && zb > -llim && zb < llim;
        const unsigned long long ba = __ballot(ina), bb = __ballot(inb);
        int base = 0;
        if (lane == 0) base = atomicAdd(&s_hl_count, __popcll(ba) + __popcll(bb));
        base = __builtin_amdgcn_readfirstlane(base);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (ina) hl_out[base + __popcll(ba & below)] = make_float4(pa.x, pa.y, pa.z, __int_as_float(ea));
        if (inb) hl_out[base + __popcll(ba) + __popcll(bb & below)] = make_float4(pb.x, pb.y, pb.z, __int_as_float(eb));
      }
      NTICK(9);
    }
  }
  __syncthreads();
  NTICK(7);
  if (tid == 0) {
    P.counts[8 * s + 4] = s_seen;
    if (P.hl) P.counts[8 * s + 6] = s_hl_count;
  }
  if (tid < 3) {
    double acc = 0.0;
    int emin = 255, emax = 0;
    for (int w = 0; w < NB_WAVES; w++) {
      acc += s_csum[w][tid];
      emin = min(emin, s_cexp[w][tid]);
      emax = max(emax, s_cexp[w][tid + 3]);
    }
    const bool exact = centre_exact(emin, emax, n_img);
    if (exact) P.centers[3 * (size_t)s + tid] = n_img > 0 ? acc / (double)n_img : 0.0;
    // counts[8 s + 5]: bit c set -> coordinate c of the centre still needs its serial chain (centre_kernel)
    const unsigned long long todo = __ballot(!exact);
    if (tid == 0) P.counts[8 * s + 5] = (int)(todo & 7ull);
  }
#undef NTICK
}

// centre of the image neighbourhood (HandSet::calculateShadow, hand_set.cpp:131-133): sequential
// fp64 sums in neighbour order.  The chain is serial, so one LANE per (sample, coordinate) walks it
// and the whole batch runs side by side (inside neighbourhood_kernel the three chains of a sample
// kept a 256-thread workgroup waiting: 390 of its 1320 us).  Since round 6 only for the (sample, coordinate) pairs whose
// sum neighbourhood_kernel could not certify as exact in every order (counts[8 s + 5]): on the benchmark clouds none.
__global__ __launch_bounds__(64) void centre_kernel(const float *__restrict__ nn, const int32_t *__restrict__ counts, int cap,
                                                    int num_samples, double *__restrict__ centers) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= 3 * num_samples) return;
  const int s = g / 3, c = g - 3 * s;
  if (!((counts[8 * s + 5] >> c) & 1)) return;  // neighbourhood_kernel's order-free sum was exact: the centre is written
  const int n_img = counts[8 * s + 1];
  const float *row = nn + ((size_t)s * 6 + c) * cap;
  double acc = 0.0;
  int t = 0;
  for (; t + 16 <= n_img; t += 16) {  // four 16-byte loads in flight, adds in order
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = *reinterpret_cast<const float4 *>(row + t + 4 * i);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      acc += (double)v[i].x;
      acc += (double)v[i].y;
      acc += (double)v[i].z;
      acc += (double)v[i].w;
    }
  }
  for (; t < n_img; t++) acc += (double)row[t];
  centers[g] = n_img > 0 ? acc / (double)n_img : 0.0;
}

// Sample indices that never were on the host (raw scans of gpd_hip_detect_batch): out[i] = list ? list[pos[i]] : pos[i] —
// `pos` the draw positions of Cloud::subsample (sample_model.h, computed on the host from a count), `list` the points above
// the support plane as the fit left them on the device.  A position outside the list gives -1, which the neighbourhood
// kernel never sees: the host draws positions below the list's size only.
__global__ __launch_bounds__(256) void sample_gather_kernel(const int32_t *__restrict__ list, int list_size, const int32_t *__restrict__ pos, int n,
                                                            int32_t *__restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int q = pos[i];
  int32_t v = q;
  if (list) v = (q >= 0 && q < list_size) ? list[q] : -1;
  out[i] = v;
}

// ---------------------------------------------------------------------------
// Host side
// ---------------------------------------------------------------------------
void search_free(SearchState &s) {
  // hipFree waits for the device: the side stream is idle as well
  device_release(s.d_sample_idx, s.d_sample_xyz, s.d_counts, s.d_nn_idx, s.d_nn, s.d_frames, s.d_centers, s.d_hands, s.d_fvalid, s.d_hl, s.d_labels);
  if (s.ev_fork) (void)hipEventDestroy(s.ev_fork);
  if (s.ev_join) (void)hipEventDestroy(s.ev_join);
  if (s.aux) (void)hipStreamDestroy(s.aux);
  s = SearchState();
}

static int search_reserve(SearchState &s, int S, int cap, int slots) {
  if (S <= s.capacity_samples && cap == s.nn_cap) return GPD_OK;
  int newS = S > s.capacity_samples ? S + S / 8 : s.capacity_samples;  // slack: the clouds of a batch differ a little
  // (a list-capacity change keeps the sample capacity the lane was sized for — while the lists are the LDS-sorted sizes: the
  //  global-memory lists of a dense scan cost 44 bytes per entry and sample, up to 46 MB per sample at 2^20 entries, and are
  //  sized for the call at hand only: 2884 reserved samples x 200k entries would be 25 GB)
  if (newS < s.min_samples && cap <= 16384) newS = s.min_samples;
  {
    // 44 bytes per list entry and sample (gathered rows, index scratch, height list): with the large lists of a dense
    // scan that is what bounds a call, and it should say so rather than fail inside hipMalloc
    size_t free_b = 0, total_b = 0;
    const size_t want = (size_t)newS * (size_t)cap * 44u;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && want > free_b + (size_t)s.capacity_samples * (size_t)s.nn_cap * 44u) {
      set_error("search: %d samples with neighbourhood lists of %d entries need %.1f GB of device memory (%.1f GB free): pass fewer samples per call",
                newS, cap, want / 1e9, free_b / 1e9);
      return GPD_ERR_CAPACITY;
    }
  }
  note_alloc(__func__);
  const uint64_t seen = s.seen_generation;
  search_free(s);
  s.seen_generation = seen;  // (search_free resets the whole state; the cloud the lists belong to is still the same)
  HIP_RET(device_alloc(s.d_sample_idx, (size_t)newS));
  HIP_RET(device_alloc(s.d_sample_xyz, (size_t)newS * 3));
  HIP_RET(device_alloc(s.d_counts, (size_t)newS * 8));
  HIP_RET(device_alloc(s.d_nn_idx, (size_t)newS * cap));
  HIP_RET(device_alloc(s.d_nn, (size_t)newS * 6 * cap));
  HIP_RET(device_alloc(s.d_frames, (size_t)newS * 12));
  HIP_RET(device_alloc(s.d_centers, (size_t)newS * 3));
  HIP_RET(device_alloc(s.d_hands, (size_t)newS * slots));
  HIP_RET(device_alloc(s.d_fvalid, (size_t)newS * slots));
  HIP_RET(device_alloc(s.d_hl, (size_t)newS * cap));
  HIP_RET(device_alloc(s.d_labels, (size_t)newS));
  s.capacity_samples = newS;
  s.nn_cap = cap;
  return GPD_OK;
}

int search_reserve_samples(SearchState &s, int S, int slots) { return search_reserve(s, S, s.nn_cap ? s.nn_cap : 8192, slots); }

// the main stream waits for the centre sums of the last run_neighbourhoods
int search_join(SearchState &s, hipStream_t stream) {
  if (s.ev_join) HIP_RET(hipStreamWaitEvent(stream, s.ev_join, 0));
  return GPD_OK;
}

static int run_neighbourhoods(const gpd_params &p, const Cloud &c, SearchState &s, const HostConsts &hc, int S, int cap,
                              const double *d_xyz /* device; null: by index */, int slots, bool want_height_list, hipStream_t stream,
                              bool sync_counts) {
  NbParams np;
  np.px = c.px; np.py = c.py; np.pz = c.pz; np.nx = c.nx; np.ny = c.ny; np.nz = c.nz;
  np.pxyz = c.pxyz;
  np.pnrm = c.pnrm;
  np.num_points = c.num_points;
  np.sample_idx = s.d_sample_idx;
  np.sample_xyz = d_xyz;
  // pcl::KdTreeFLANN::radiusSearch passes (float)(radius*radius) to FLANN
  const double r_all = std::fmax(hc.nn_radius_hands, std::fmax(hc.nn_radius_images, p.nn_radius_frames));
  np.r2_all = (float)(r_all * r_all);
  np.r2_hands = (float)(hc.nn_radius_hands * hc.nn_radius_hands);
  np.r2_images = (float)(hc.nn_radius_images * hc.nn_radius_images);
  np.r2_frames = (float)(p.nn_radius_frames * p.nn_radius_frames);
  np.cap = cap;
  np.counts = s.d_counts;
  np.nn_idx = s.d_nn_idx;
  np.nn = s.d_nn;
  np.frames = s.d_frames;
  np.centers = s.d_centers;
  np.cam_source = c.cam_source;
  np.num_cams = c.num_cams;
  np.grid = grid_view(c);
  np.reach = (float)r_all * 1.001f + 1e-5f;
  np.hl = want_height_list ? s.d_hl : nullptr;
  np.hl_slots = slots;
  for (int slot = 0; slot < slots && slot < GPD_MAX_SLOTS; slot++)
    for (int r = 0; r < 3; r++)  // third column of rot_binormal * rot[slot]
      np.hl_col[slot][r] = hc.rot_binormal[3 * r] * hc.rot[slot][2] + hc.rot_binormal[3 * r + 1] * hc.rot[slot][5] +
                           hc.rot_binormal[3 * r + 2] * hc.rot[slot][8];
  np.hl_height = p.hand_height;
  np.hl_radius = hc.nn_radius_hands * 1.001 + 1e-6;
  static unsigned long long *d_nbdbg = nullptr;
  np.dbg = nullptr;
  if (prof_env("GPD_NB_TIMING")) {
    if (!d_nbdbg) HIP_RET(hipMalloc(&d_nbdbg, 10 * sizeof(unsigned long long)));
    HIP_RET(hipMemsetAsync(d_nbdbg, 0, 10 * sizeof(unsigned long long), stream));
    np.dbg = d_nbdbg;
  }
  // 8192-entry lists are bucket-sorted (64 + 8 KB of LDS: two workgroups per CU); the 16384-entry
  // retry of an overfull neighbourhood sorts in place (bitonic, 128 KB); anything larger (up to kNnCapMax) is
  // bucket-sorted in global memory
  if (cap > 16384) {
    np.bucket = 1;
    const size_t lds = (size_t)(2 * 8192 + 1) * sizeof(int);
    HIP_RET(hipFuncSetAttribute(reinterpret_cast<const void *>(neighbourhood_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    neighbourhood_kernel<true><<<S, NB_THREADS, lds, stream>>>(np);
  } else {
    np.bucket = cap < 16384 ? 1 : 0;
    const size_t lds = (size_t)cap * sizeof(unsigned long long) + (np.bucket ? (2 * NB_BUCKETS + 1) * sizeof(int) : 0);
    HIP_RET(hipFuncSetAttribute(reinterpret_cast<const void *>(neighbourhood_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)lds));
    neighbourhood_kernel<false><<<S, NB_THREADS, lds, stream>>>(np);
  }
  HIP_RET(hipGetLastError());
  if (np.dbg) {
    unsigned long long h[10];
    HIP_RET(hipMemcpyAsync(h, d_nbdbg, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_RET(hipStreamSynchronize(stream));
    static const char *names[10] = {"visit", "scan", "scatter", "bucket sort", "crowded buckets", "prefix lengths", "gather",
                                    "last barrier", "wait for the frame", "height list"};
    for (int i = 0; i < 10; i++) fprintf(stderr, "[nb-timing] %-16s %8.1f kcycles/sample\n", names[i], (double)h[i] / S / 1e3);
  }
  // the centre sums fork off to the side stream; search_join() brings them back
  if (!s.aux) {
    HIP_RET(hipStreamCreate(&s.aux));
    HIP_RET(hipEventCreateWithFlags(&s.ev_fork, hipEventDisableTiming));
    HIP_RET(hipEventCreateWithFlags(&s.ev_join, hipEventDisableTiming));
  }
  HIP_RET(hipEventRecord(s.ev_fork, stream));
  HIP_RET(hipStreamWaitEvent(s.aux, s.ev_fork, 0));
  centre_kernel<<<(3 * S + 63) / 64, 64, 0, s.aux>>>(s.d_nn, s.d_counts, cap, S, s.d_centers);
  HIP_RET(hipGetLastError());
  HIP_RET(hipEventRecord(s.ev_join, s.aux));
  s.h_counts.clear();
  if (sync_counts) {
    s.h_counts.resize((size_t)S * 8);
    HIP_RET(hipMemcpyAsync(s.h_counts.data(), s.d_counts, (size_t)S * 8 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_RET(hipStreamSynchronize(stream));
  }
  return GPD_OK;
}

// The list capacity a run on cloud c starts with.  A new cloud starts from the LDS-sorted list size again: the large lists one
// dense cloud needed are not carried into the next one (they come back through the caller's retry if it needs them too).
static int start_capacity(SearchState &s, const Cloud &c, int *cap) {
  if (s.seen_generation != c.generation) {
    s.seen_generation = c.generation;
    if (s.nn_cap > 16384) {
      const int rc = search_force_capacity(s, 8192);
      if (rc) return rc;
    }
  }
  *cap = s.nn_cap ? s.nn_cap : 8192;
  return GPD_OK;
}

// neighbourhoods of S samples (by index or by coordinates), list capacity grown once if needed
static int neighbourhoods(const gpd_params &p, const Cloud &c, SearchState &s, const HostConsts &hc, const int32_t *sample_idx,
                          const double *sample_xyz, int S, int slots, int *cap_out, hipStream_t stream, bool sync_counts = true,
                          bool want_height_list = true, const SampleGather *resident = nullptr) {
  int cap = 0;
  int rc = start_capacity(s, c, &cap);
  if (rc) return rc;
  rc = search_reserve(s, S, cap, slots);
  if (rc) return rc;
  for (;;) {
    if (resident && resident->d_xyz) {
      // coordinates on the device already: read where they are (a retry reads them again)
    } else if (resident) {  // the indices are on the device already (and stay where they were: a retry gathers them again)
      sample_gather_kernel<<<(S + 255) / 256, 256, 0, stream>>>(resident->d_list, resident->list_size, resident->d_pos, S, s.d_sample_idx);
      HIP_RET(hipGetLastError());
    } else if (sample_xyz) {
      HIP_RET(hipMemcpyAsync(s.d_sample_xyz, sample_xyz, (size_t)S * 3 * sizeof(double), hipMemcpyHostToDevice, stream));
    } else {
      HIP_RET(hipMemcpyAsync(s.d_sample_idx, sample_idx, (size_t)S * sizeof(int32_t), hipMemcpyHostToDevice, stream));
    }
    rc = run_neighbourhoods(p, c, s, hc, S, cap, resident && resident->d_xyz ? resident->d_xyz : (sample_xyz ? s.d_sample_xyz : nullptr), slots,
                            want_height_list, stream, sync_counts);
    if (rc) return rc;
    if (!sync_counts) break;  // the caller reads `worst found` from the plan summary and retries (search_next_capacity)
    int worst = 0;
    for (int i = 0; i < S; i++) worst = s.h_counts[8 * i + 3] > worst ? s.h_counts[8 * i + 3] : worst;
    if (worst <= cap) break;
    // the first run's centre_kernel may still read d_nn / d_counts and write d_centers on the side stream: the lists are
    // rebuilt (and reallocated) only after it
    rc = search_join(s, stream);
    if (rc) return rc;
    cap = search_next_capacity(s, worst);
    if (!cap) {
      set_error("search: a neighbourhood holds %d points, more than the list capacity %d", worst, kNnCapMax);
      return GPD_ERR_CAPACITY;
    }
    rc = search_reserve(s, S, cap, slots);
    if (rc) return rc;
  }
  *cap_out = cap;
  return GPD_OK;
}

int search_next_capacity(const SearchState &s, int worst) {
  if (worst <= s.nn_cap) return s.nn_cap;
  if (worst <= 16384) return 16384;  // in-place bitonic sort, 128 KB of LDS per workgroup
  if (worst > kNnCapMax) return 0;
  const int cap = (worst + 4095) / 4096 * 4096;  // global-memory lists
  return cap < kNnCapMax ? cap : kNnCapMax;
}
int search_force_capacity(SearchState &s, int cap) {
  if (cap == s.nn_cap) return GPD_OK;
  const int keep = s.capacity_samples > s.min_samples ? s.capacity_samples : s.min_samples;
  const uint64_t seen = s.seen_generation;
  search_free(s);
  s.seen_generation = seen;
  s.nn_cap = cap;  // search_reserve allocates on the next run (capacity_samples is 0 now) ...
  s.min_samples = keep;  // ... for at least as many samples as before: a lane sized by gpd_hip_reserve stays sized
  return GPD_OK;
}

int search_run(const gpd_params &p, const Cloud &c, SearchState &s, const int32_t *sample_idx, const double *sample_xyz, int S,
               hipStream_t stream, bool sync_counts, const SampleGather *resident) {
  const int slots = p.num_hand_axes * p.num_orientations;
  HostConsts hc;
  host_consts(p, hc);
  int cap = 0;
  int rc = neighbourhoods(p, c, s, hc, sample_idx, resident ? nullptr : sample_xyz, S, slots, &cap, stream, sync_counts, true, resident);
  if (rc) return rc;
  rc = hands_enqueue_eval(p, hc, s, cap, S, stream);
  if (rc) return rc;
  rc = search_join(s, stream);
  if (rc) return rc;
  s.num_samples = S;
  s.cloud_generation = c.generation;
  return GPD_OK;
}

int reevaluate_run(const gpd_params &p, const Cloud &c, SearchState &s, gpd_hand *hands, int n, int32_t *labels, hipStream_t stream) {
  const int slots = p.num_hand_axes * p.num_orientations;
  HostConsts hc;
  host_consts(p, hc);
  s.num_samples = 0;  // the buffers are reused: hands of an earlier search can no longer be imaged
  s.h_set_sample.clear();
  s.h_samples.clear();
  std::vector<double> xyz((size_t)n * 3);
  for (int i = 0; i < n; i++)
    for (int r = 0; r < 3; r++) xyz[3 * (size_t)i + r] = hands[i].sample[r];
  int cap = 0;
  int rc = neighbourhoods(p, c, s, hc, nullptr, xyz.data(), n, slots, &cap, stream, true, /*want_height_list=*/false);
  if (rc) return rc;
  HIP_RET(hipMemcpyAsync(s.d_hands, hands, (size_t)n * sizeof(gpd_hand), hipMemcpyHostToDevice, stream));
  rc = hands_enqueue_reeval(p, hc, s, cap, n, stream);
  if (rc) return rc;
  rc = search_join(s, stream);
  if (rc) return rc;
  HIP_RET(hipMemcpyAsync(hands, s.d_hands, (size_t)n * sizeof(gpd_hand), hipMemcpyDeviceToHost, stream));
  HIP_RET(hipMemcpyAsync(labels, s.d_labels, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_RET(hipStreamSynchronize(stream));
  return GPD_OK;
}

// gpd_hip_images_given: the neighbourhood lists of S samples given by coordinates, through the capacity retry, and nothing
// else — no hand is evaluated (no height list either).  The centre sums are joined: the caller goes on to write into d_counts.
int given_lists_run(const gpd_params &p, const Cloud &c, SearchState &s, const double *sample_xyz, int S, hipStream_t stream) {
  const int slots = p.num_hand_axes * p.num_orientations;
  HostConsts hc;
  host_consts(p, hc);
  s.num_samples = 0;  // the buffers are reused: hands of an earlier search can no longer be imaged
  s.h_set_sample.clear();
  s.h_samples.clear();
  int cap = 0;
  int rc = neighbourhoods(p, c, s, hc, nullptr, sample_xyz, S, slots, &cap, stream, true, /*want_height_list=*/false);
  if (rc) return rc;
  return search_join(s, stream);
}

// gpd_hip_label_view, one round: reevaluateHypotheses of the n candidate records d_recs (device, set-major) against the ground
// truth `gt`, one neighbourhood list per hand set with a candidate (`lists` of them: the plan's live sets).  Rewrites the records'
// flags, writes d_labels8 [n]; only 8 bytes (largest neighbourhood — or the capacity flags d_img_status[0] of the round's image kernels,
// *img_status —, positives) come back per attempt — an attempt is repeated
// with the next list capacity when a neighbourhood overflowed, as the search does.
int label_round(const gpd_params &p, const Cloud &gt, SearchState &gs, gpd_hand *d_recs, uint8_t *d_labels8, int n, int lists,
                int32_t *d_cand_list, int32_t *d_meta, int32_t *h_meta, const int32_t *d_img_status, int *img_status, int *positives,
                long long *d2h_bytes, hipStream_t stream) {
  *img_status = 0;
  const int slots = p.num_hand_axes * p.num_orientations;
  HostConsts hc;
  host_consts(p, hc);
  gs.num_samples = 0;
  int cap = 0;
  int rc = start_capacity(gs, gt, &cap);
  if (rc) return rc;
  for (;;) {
    rc = search_reserve(gs, lists, cap, slots);
    if (rc) return rc;
    rc = hands_enqueue_label_sets(d_recs, n, d_cand_list, gs.d_sample_xyz, d_meta, stream);
    if (rc) return rc;
    rc = run_neighbourhoods(p, gt, gs, hc, lists, cap, gs.d_sample_xyz, slots, /*want_height_list=*/false, stream, /*sync_counts=*/false);
    if (rc) return rc;
    rc = hands_enqueue_label(p, hc, gs, cap, lists, d_recs, n, d_cand_list, d_labels8, stream);
    if (rc) return rc;
    rc = hands_enqueue_label_meta(gs.d_counts, lists, d_labels8, n, d_img_status, d_meta, stream);
    if (rc) return rc;
    rc = search_join(gs, stream);
    if (rc) return rc;
    HIP_RET(hipMemcpyAsync(h_meta, d_meta, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_RET(hipStreamSynchronize(stream));
    *d2h_bytes += 2 * sizeof(int32_t);
    const int worst = h_meta[0];
    if (worst <= -2) {  // the caller words the image stage's capacity error
      *img_status = -2 - worst;
      return GPD_ERR_CAPACITY;
    }
    if (worst < 0) {
      set_error("label_view: the candidate records do not form the %d hand sets the plan counted", lists);
      return GPD_ERR_STATE;
    }
    if (worst <= cap) break;
    cap = search_next_capacity(gs, worst);
    if (!cap) {
      set_error("label_view: a ground-truth neighbourhood holds %d points, more than the list capacity %d", worst, kNnCapMax);
      return GPD_ERR_CAPACITY;
    }
  }
  *positives = h_meta[1];
  return GPD_OK;
}

int search_download(const gpd_params &p, SearchState &s, gpd_hand *hands, int *num_sets, hipStream_t stream) {
  const int slots = p.num_hand_axes * p.num_orientations;
  const int S = s.num_samples;
  std::vector<gpd_hand> tmp((size_t)S * slots);
  HIP_RET(hipMemcpyAsync(tmp.data(), s.d_hands, tmp.size() * sizeof(gpd_hand), hipMemcpyDeviceToHost, stream));
  HIP_RET(hipStreamSynchronize(stream));
  // drop samples without a frame neighbourhood before numbering sets (frame_estimator.cpp:24-29)
  s.h_set_sample.clear();
  s.h_samples.clear();
  int ns = 0;
  for (int i = 0; i < S; i++) {
    if (s.h_counts[8 * i + 2] == 0) continue;
    for (int j = 0; j < slots; j++) {
      gpd_hand h = tmp[(size_t)i * slots + j];
      h.set_index = ns;
      hands[(size_t)ns * slots + j] = h;
    }
    s.h_set_sample.push_back(i);
    for (int r = 0; r < 3; r++) s.h_samples.push_back(tmp[(size_t)i * slots].sample[r]);
    ns++;
  }
  *num_sets = ns;
  return GPD_OK;
}

}  // namespace gpd
