// Device helpers and LDS structs that the per-candidate bodies of images.hip (shadow_image_body, shadow_image_any_body,
// grasp_image_body) share: the candidate's box, the cell lookup, the block scans, the list of non-empty pixels, the plane
// finishing pass and the register sort networks.  They read `__constant__ ImgConsts c_img`, which a unit has to define
// BEFORE it includes this header — the build has no relocatable device code, so that unit is images.hip alone.
#pragma once
#include <cfloat>
#include <type_traits>

#include "gpd_internal.h"
#include "image_model.h"
#include "wave_ops.h"

namespace gpd {

static_assert(kImgCells == kImg, "image_model.h and gpd_internal.h disagree about the image size");
constexpr int IMG_THREADS = 512;   // 256 VGPRs per lane: no spills (1024 threads measured equally fast but spilled)
constexpr int IMG_WAVES = IMG_THREADS / 64;

struct Box {
  double F[9];
  double sample[3];
  double off[3];  // x_a = t_a - off[a]: bottom, center - half_od, -vol_height
  double lo[3], hi[3];
};

// points kernel: in-box points cached once, one projection's normals (3 planes) + depth at a time.
// BIG (the overflow fallback, up to PT_CAP_BIG in-box points): the point arrays live in a global
// scratch row instead of LDS.
struct PointArrays {
  double t[3][PT_CAP];  // hand-frame coordinates of the in-box points
  float4 an[PT_CAP];    // |normal| in the hand frame (x, y, z) and, as bits in w, the cell key
                        // cx | cy << 6 | cz << 12: one 16-byte read per visit
};
struct NoPointArrays {};
// Under 80 KB for the small instantiation, so that two workgroups — two grasp_image ones, or one of them next to a
// shadow_image one of another stream — share a CU (the kernels wait on LDS round trips and barriers most of their
// time; the second resident workgroup fills those gaps).  What made it 155 KB before: three normal planes + a depth
// plane held at once (57.6 KB) and 2048-point arrays.  Now the walks leave their four values per NON-EMPTY pixel
// (at most one per in-box point) and the planes are rebuilt one after the other in the storage of the segment
// counters, dilated straight into registers.
template <bool BIG>
struct __attribute__((aligned(16))) SmemPts {
  typename std::conditional<BIG, NoPointArrays, PointArrays>::type p;
  __attribute__((aligned(16))) uint32_t cells[kPix];   // (segment start << 16) | count of a pixel; after the walks: the index raster, then the staged bytes
  uint16_t place[BIG ? PT_CAP_BIG : PT_CAP];  // segment table: entry numbers (entries are numbered in neighbour order)
  float4 nzv[(BIG ? kPix : PT_CAP) + 1];      // slot 0: the empty pixel (zeros); slot q + 1: the three normal values and the
                                              // depth value of the q-th non-empty pixel
  uint16_t nzlist[BIG ? kPix : PT_CAP];       // the non-empty pixels, longest segment first
  double thr[3][kImg + 1];
  double recip[128];  // 1.0 / k
  float red_f[4 * IMG_WAVES];
  int red_i[IMG_WAVES];
  int counter;
  int flag;
  int nnz;  // non-empty pixels of the projection (scan_cells_hist)
};
typedef SmemPts<false> Smem;
// shadow kernel: kept under 80 KB (SHC = 6144) so that two workgroups share a CU
template <int SHC, bool WIDE>
struct __attribute__((aligned(16))) SmemShadow {
  __attribute__((aligned(16))) float raster0[kPix];
  __attribute__((aligned(16))) uint32_t cells[kPix];
  uint32_t lin[SHC];  // set bits inside the box, ascending: voxel position (iz | iy << 6 | ix << 12) | cell x << LB | cell y << (LB + 6)
  union {
    struct {                        // while the list is built: per row of the voxel window (a line along world z) ...
      uint16_t rowbase[Vox<WIDE>::VD * Vox<WIDE>::VD];  // ... where its in-box voxels start in `lin`
      uint8_t rowcnt[Vox<WIDE>::VD * Vox<WIDE>::VD];    // ... and how many they are
    } rows;
    uint16_t place[SHC];  // afterwards: segment table of the counting sort
  } bp;
  uint16_t nz[kPix];
  uint8_t cz[SHC];  // cell z of the list entries
  double thr[3][kImg + 1];
  double recip[128];
  float red_f[4 * IMG_WAVES];
  int red_i[IMG_WAVES];
  int vorg[3];
  int flag;
  int nnz;  // non-empty pixels of the projection (scan_cells_hist)
};

// hand-frame coordinates of a world point: t = F^T (w - sample)  (image_strategy.cpp:36-40)
__device__ inline void to_hand(const Box &B, double w0, double w1, double w2, double t[3]) {
  const double c0 = w0 - B.sample[0], c1 = w1 - B.sample[1], c2 = w2 - B.sample[2];
  t[0] = B.F[0] * c0 + B.F[3] * c1 + B.F[6] * c2;
  t[1] = B.F[1] * c0 + B.F[4] * c1 + B.F[7] * c2;
  t[2] = B.F[2] * c0 + B.F[5] * c1 + B.F[8] * c2;
}
// findPointsInUnitImage (image_strategy.cpp:53-70): strict box test
__device__ inline bool in_box(const Box &B, const double t[3]) {
  return (t[0] > B.lo[0]) && (t[0] < B.hi[0]) && (t[1] > B.lo[1]) && (t[1] < B.hi[1]) && (t[2] > B.lo[2]) && (t[2] < B.hi[2]);
}
// min(floor(((t - off)/len)/(1/60)), 59) by exact thresholds (see file header)
template <class SM>
__device__ inline int cell_coord(const SM &S, int axis, double x) {
  int k = (int)(x * c_img.inv_cell[axis]);
  k = k < 0 ? 0 : (k > kImg - 1 ? kImg - 1 : k);
  // both neighbours of the guess at once (one LDS round trip; the guess is off by one at most, the loops are for the proof)
  const double t0 = S.thr[axis][k], t1 = S.thr[axis][k + 1];
  if (k > 0 && x < t0) {
    k--;
    while (k > 0 && x < S.thr[axis][k]) k--;
  } else if (k < kImg - 1 && x >= t1) {
    k++;
    while (k < kImg - 1 && x >= S.thr[axis][k + 1]) k++;
  }
  return k;
}
template <class SM>
__device__ inline uint32_t cells_of(const SM &S, const Box &B, const double t[3]) {
  const int cx = cell_coord(S, 0, t[0] - B.off[0]);
  const int cy = cell_coord(S, 1, t[1] - B.off[1]);
  const int cz = cell_coord(S, 2, t[2] - B.off[2]);
  return (uint32_t)cx | ((uint32_t)cy << 6) | ((uint32_t)cz << 12);
}
// projections by cumulative row swaps 0<->2 then 1<->2: (x,y,z), (z,y,x), (z,x,y);
// cell = horizontal + 60 * vertical (image_strategy.cpp:92-102)
__device__ inline int cell_of_key(uint32_t key, int pr) {
  const int cx = key & 63, cy = (key >> 6) & 63, cz = (key >> 12) & 63;
  const int v = pr == 0 ? cx : cz;
  const int h = pr == 2 ? cx : cy;
  return h + v * kImg;
}
__device__ inline int depth_axis(int pr) { return pr == 0 ? 2 : (pr == 1 ? 0 : 1); }

// x / len[axis], correctly rounded, without a division: q = x*y, r = x - len*q (exact, FMA),
// q' = q + r*y with y = RN(1/len) (Markstein).  Bit-identical to the IEEE quotient for the
// image extents; image::axis_model() checks that on the host and falls back to a real division.
__device__ inline double div_len(double x, int axis) {
  const ImgConsts &K = c_img;
  if (K.true_div) return x / K.len[axis];
  const double y = K.inv_len[axis];
  const double q = x * y;
  const double r = __builtin_fma(-K.len[axis], q, x);
  return __builtin_fma(r, y, q);
}
// 1.0 / (double)count for the running means (image_strategy.cpp:170, 206)
template <int NTAB>
__device__ inline double recip_count(const double *tab, float fc) {
  const int k = (int)fc;
  return k < NTAB ? tab[k] : 1.0 / (double)fc;
}

__device__ inline uint32_t lcg_step(uint32_t &s) {  // HandSet::fastrand (hand_set.cpp:263-266)
  s = 214013u * s + 2531011u;
  return (uint32_t)(((int32_t)s >> 16) & 0x7FFF);
}
__device__ inline uint32_t lcg_jump(uint32_t s, unsigned long long n) {
  const image::LcgMap m = image::lcg_affine(n);
  return m.a * s + m.c;
}

// block-wide exclusive scan of one int per thread; returns the exclusive prefix, total in *total.
// ONE barrier.  (There was a second one in front of the red_i stores, against a reader of red_i that is still on its
// way.  No call site has one: each is entered through a barrier of its own — the row counts / the pixel counts that
// are summed here were written by other threads — and red_i is not read between that barrier and this call: its
// last readers, the previous scan's sums below (in the general shadow kernel also the `return S.red_i[0]` of
// list_nonempty_cells and the mask flags of its walk), lie several barriers back, for the persistent kernels the one
// at the loop head included.  A new call site has to keep that: a barrier between the last read of red_i and the call.)
template <class SM>
__device__ inline int block_excl_scan(SM &S, int v, int *total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int incl = wave_incl_scan_i32(v);
  if (lane == 63) S.red_i[wave] = incl;
  __syncthreads();
  int base = 0, tot = 0;
#pragma unroll
  for (int w = 0; w < IMG_WAVES; w++) {
    const int x = S.red_i[w];
    if (w < wave) base += x;
    tot += x;
  }
  *total = tot;
  return base + incl - v;
}

// exclusive scan of cells[].count into the start field; returns the total
template <class SM>
__device__ int scan_cells(SM &S) {
  const int tid = threadIdx.x;
  constexpr int PER = 8;  // consecutive cells per thread: two 16-byte LDS accesses each way (450 threads hold the 3600 cells)
  static_assert(kPix % PER == 0 && kPix / PER <= IMG_THREADS, "scan_cells: cells per thread");
  uint4 *c4 = reinterpret_cast<uint4 *>(S.cells);
  if (tid < 32) reinterpret_cast<int *>(S.red_f)[tid] = 0;  // the histogram of list_nonempty_cells (two barriers from here; its last readers, the scale factors of the final phase, are behind that phase's closing barrier)
  uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
  if (tid < kPix / PER) {
    a = c4[2 * tid];
    b = c4[2 * tid + 1];
  }
  const int c[PER] = {(int)(a.x & 0xffffu), (int)(a.y & 0xffffu), (int)(a.z & 0xffffu), (int)(a.w & 0xffffu),
                      (int)(b.x & 0xffffu), (int)(b.y & 0xffffu), (int)(b.z & 0xffffu), (int)(b.w & 0xffffu)};
  int sum = 0;
#pragma unroll
  for (int k = 0; k < PER; k++) sum += c[k];
  int total;
  int run = block_excl_scan(S, sum, &total);
  uint32_t o[PER];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    o[k] = (uint32_t)(run < 0xffff ? run : 0xffff) << 16;
    run += c[k];
  }
  if (tid < kPix / PER) {
    c4[2 * tid] = make_uint4(o[0], o[1], o[2], o[3]);
    c4[2 * tid + 1] = make_uint4(o[4], o[5], o[6], o[7]);
  }
  __syncthreads();
  return total;
}

// list of the non-empty cells, ordered by their point count, descending (counting sort into 32
// buckets; counts >= 31 share the first).  The walks give one pixel to one lane, so a wave runs as
// long as its longest pixel: with equal lengths side by side the waves execute ~40 % fewer
// (mostly idle) iterations than in cell order.  Pixels are independent, their order is free.
// Returns the number of non-empty cells.
template <class SM>
__device__ int list_nonempty_cells(SM &S, uint16_t *nz) {
  const int tid = threadIdx.x;
  constexpr int PER = (kPix + IMG_THREADS - 1) / IMG_THREADS;
  int *hist = reinterpret_cast<int *>(S.red_f);  // 32 counters, cleared by scan_cells; red_f is idle until the final phase
  static_assert(PER == 8, "two 16-byte reads per thread");
  uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
  if (tid < kPix / PER) {
    a = reinterpret_cast<const uint4 *>(S.cells)[2 * tid];
    b = reinterpret_cast<const uint4 *>(S.cells)[2 * tid + 1];
  }
  const uint32_t cw[PER] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  int bucket[PER];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int cn = (int)(cw[k] & 0xffffu);
    bucket[k] = cn ? 31 - (cn < 31 ? cn : 31) : -1;
    if (cn) atomicAdd(&hist[bucket[k]], 1);
  }
  __syncthreads();
  if (tid < 64) {
    const int v = tid < 32 ? hist[tid] : 0;
    const int incl = wave_incl_scan_i32(v);
    if (tid < 32) hist[tid] = incl - v;
    if (tid == 31) S.red_i[0] = incl;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < PER; k++)
    if (bucket[k] >= 0) nz[atomicAdd(&hist[bucket[k]], 1)] = (uint16_t)(tid * PER + k);
  __syncthreads();
  return S.red_i[0];
}

// scan_cells and list_nonempty_cells in the phases of ONE scan, for the per-candidate kernels: two barriers and a share of
// the caller's next phase where the pair above takes six.  A thread holds the counts of its eight pixels anyway, so
//   - scan_cells_hist: the histogram of the list is filled beside the wave scan (the caller has cleared S.red_f in the
//     phase of its count: the last readers of red_f are behind the closing barrier of the final phase) | barrier | the
//     segment starts go to `cells`, and the first wave turns the histogram into bucket offsets and leaves the number of
//     non-empty pixels in S.nnz | barrier.  The eight buckets stay with the thread, a byte each (0: empty pixel);
//   - scatter_nonempty: the list itself, in the phase in which the caller fills its segment table — both only read what
//     the second barrier published, the list is first read behind the barrier that ends that phase, and so is S.nnz.
// Same list as list_nonempty_cells up to the order inside a bucket, which is the order of LDS atomics there as here.
template <class SM>
__device__ inline void scan_cells_hist(SM &S, uint32_t (&pk)[2]) {
  const int tid = threadIdx.x;
  constexpr int PER = 8;
  static_assert(kPix % PER == 0 && kPix / PER <= IMG_THREADS, "scan_cells_hist: cells per thread");
  uint4 *c4 = reinterpret_cast<uint4 *>(S.cells);
  int *hist = reinterpret_cast<int *>(S.red_f);
  uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
  if (tid < kPix / PER) {
    a = c4[2 * tid];
    b = c4[2 * tid + 1];
  }
  const int c[PER] = {(int)(a.x & 0xffffu), (int)(a.y & 0xffffu), (int)(a.z & 0xffffu), (int)(a.w & 0xffffu),
                      (int)(b.x & 0xffffu), (int)(b.y & 0xffffu), (int)(b.z & 0xffffu), (int)(b.w & 0xffffu)};
  int sum = 0;
  pk[0] = pk[1] = 0u;
#pragma unroll
  for (int k = 0; k < PER; k++) {
    sum += c[k];
    if (c[k]) {
      const int bucket = 31 - (c[k] < 31 ? c[k] : 31);  // 0 .. 30: counter 31 stays zero
      atomicAdd(&hist[bucket], 1);
      pk[k >> 2] |= (uint32_t)(bucket + 1) << (8 * (k & 3));
    }
  }
  int total;
  int run = block_excl_scan(S, sum, &total);
  uint32_t o[PER];
#pragma unroll
  for (int k = 0; k < PER; k++) {
    o[k] = (uint32_t)(run < 0xffff ? run : 0xffff) << 16;
    run += c[k];
  }
  if (tid < kPix / PER) {
    c4[2 * tid] = make_uint4(o[0], o[1], o[2], o[3]);
    c4[2 * tid + 1] = make_uint4(o[4], o[5], o[6], o[7]);
  }
  if (tid < 64) {
    const int v = tid < 32 ? hist[tid] : 0;
    const int incl = wave_incl_scan_i32(v);
    if (tid < 32) hist[tid] = incl - v;
    if (tid == 31) S.nnz = incl;
  }
  __syncthreads();
}
template <class SM>
__device__ inline void scatter_nonempty(SM &S, uint16_t *nz, const uint32_t (&pk)[2]) {
  int *hist = reinterpret_cast<int *>(S.red_f);
  // (the pixel numbers are made here, from a value the optimiser cannot follow: hoisted out of the callers' projection
  // loops they were registers held through every phase of kernels that sit on their 128-register cap)
  int first = threadIdx.x * 8;
  asm volatile("" : "+v"(first));
#pragma unroll
  for (int k = 0; k < 8; k++) {
    const int b = (int)((pk[k >> 2] >> (8 * (k & 3))) & 0xffu);
    if (b) nz[atomicAdd(&hist[b - 1], 1)] = (uint16_t)(first + k);
  }
}

// 3x3 rect max-dilate (border ignored), NORM_MINMAX to [0,1], u8 = round-half-even(v*255)
// (image_strategy.cpp:144-153, 178-187, 221-230; cv::dilate / cv::normalize / convertTo).
// Planes are in cell-index order (cell row = 59 - image row; the 3x3 window is symmetric).
// NPL planes are finished in one pass; planes with the same norm group share min/max (the three
// normal channels are normalised jointly, depth/shadow on their own).  Each thread owns groups of
// 4 consecutive pixels: three 16-byte LDS reads + two edge reads per row (indices clamped to the
// image: a clamped duplicate cannot change a max), one dword store.
// planes 0..2 (or 0 alone) start at p012 and are kPix apart; plane 3, if present, is p3 and is
// normalised on its own; output channels are consecutive planes starting at out.
//
// finalize_planes_ex is the same pass with three hooks for a caller that folds neighbouring phases into it:
//   fold(x)   applied to every value as it is loaded (a pure function of the stored word: the dilation, the min / max
//             and the bytes see fold(x) wherever the plain pass sees x);
//   tail()    run by every thread in the last phase, behind the barrier that ends all reads of the planes — work that
//             only has to be done before the caller's next phase rides on the closing barrier;
//   OWN_RED   false (NPL == 1 only): the caller still reads red_f[4 * w + 2] and [4 * w + 3] when it enters, so the pass
//             writes just the two slots per wave that one norm group needs and does without the barrier in front of them
//             (nothing reads slots 4 * w + 0 / + 1 between the caller's previous barrier and this pass).
template <int NPL, bool OWN_RED, class SM, class FOLD, class TAIL>
__device__ __forceinline__ void finalize_planes_ex(SM &S, const float *p012, const float *p3, uint8_t *out, FOLD fold, TAIL tail) {
  static_assert(OWN_RED || NPL == 1, "the shared reduction slots hold one norm group");
  const int tid = threadIdx.x;
  constexpr int GROUPS = NPL * 900;
  constexpr int PER = (GROUPS + IMG_THREADS - 1) / IMG_THREADS;
  float d[PER][4];
  float mn[2] = {FLT_MAX, FLT_MAX}, mx[2] = {-FLT_MAX, -FLT_MAX};
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int g = tid + k * IMG_THREADS;
    if (g < GROUPS) {
      const int ch = g / 900, rem = g - ch * 900;
      const int r = rem / 15, c0 = (rem - r * 15) * 4;
      const float *pl = (ch < 3) ? p012 + ch * kPix : p3;
      const int rm = r > 0 ? r - 1 : 0, rp = r < kImg - 1 ? r + 1 : kImg - 1;
      const int cl = c0 > 0 ? c0 - 1 : 0, cr = c0 + 4 < kImg ? c0 + 4 : kImg - 1;
      const float4 a = *reinterpret_cast<const float4 *>(pl + rm * kImg + c0);
      const float4 b = *reinterpret_cast<const float4 *>(pl + r * kImg + c0);
      const float4 c = *reinterpret_cast<const float4 *>(pl + rp * kImg + c0);
      const float el = fmaxf(fmaxf(fold(pl[rm * kImg + cl]), fold(pl[r * kImg + cl])), fold(pl[rp * kImg + cl]));
      const float er = fmaxf(fmaxf(fold(pl[rm * kImg + cr]), fold(pl[r * kImg + cr])), fold(pl[rp * kImg + cr]));
      const float m0 = fmaxf(fmaxf(fold(a.x), fold(b.x)), fold(c.x)), m1 = fmaxf(fmaxf(fold(a.y), fold(b.y)), fold(c.y));
      const float m2 = fmaxf(fmaxf(fold(a.z), fold(b.z)), fold(c.z)), m3 = fmaxf(fmaxf(fold(a.w), fold(b.w)), fold(c.w));
      d[k][0] = fmaxf(fmaxf(el, m0), m1);
      d[k][1] = fmaxf(fmaxf(m0, m1), m2);
      d[k][2] = fmaxf(fmaxf(m1, m2), m3);
      d[k][3] = fmaxf(fmaxf(m2, m3), er);
      const float lo = fminf(fminf(d[k][0], d[k][1]), fminf(d[k][2], d[k][3]));
      const float hi = fmaxf(fmaxf(d[k][0], d[k][1]), fmaxf(d[k][2], d[k][3]));
      if (ch < 3) {
        mn[0] = fminf(mn[0], lo);
        mx[0] = fmaxf(mx[0], hi);
      } else {
        mn[1] = fminf(mn[1], lo);
        mx[1] = fmaxf(mx[1], hi);
      }
    }
  }
#pragma unroll
  for (int q = 0; q < 2; q++) {
    mn[q] = wave_min_f32(mn[q]);
    mx[q] = wave_max_f32(mx[q]);
  }
  if constexpr (OWN_RED) __syncthreads();
  if ((tid & 63) == 0) {
    S.red_f[4 * (tid >> 6) + 0] = mn[0];
    S.red_f[4 * (tid >> 6) + 1] = mx[0];
    if constexpr (OWN_RED) {
      S.red_f[4 * (tid >> 6) + 2] = mn[1];
      S.red_f[4 * (tid >> 6) + 3] = mx[1];
    }
  }
  __syncthreads();
  float fs[2] = {0.f, 0.f}, fb[2] = {0.f, 0.f};
#pragma unroll
  for (int q = 0; q < (OWN_RED ? 2 : 1); q++) {
    float a = S.red_f[2 * q], b = S.red_f[2 * q + 1];
#pragma unroll
    for (int w = 1; w < IMG_WAVES; w++) {
      a = fminf(a, S.red_f[4 * w + 2 * q]);
      b = fmaxf(b, S.red_f[4 * w + 2 * q + 1]);
    }
    const double smin = (double)a, smax = (double)b;
    const double scale = 1.0 * ((smax - smin) > DBL_EPSILON ? 1.0 / (smax - smin) : 0.0);
    const double shift = 0.0 - smin * scale;
    fs[q] = (float)scale;
    fb[q] = (float)shift;
  }
#pragma unroll
  for (int k = 0; k < PER; k++) {
    const int g = tid + k * IMG_THREADS;
    if (g < GROUPS) {
      const int ch = g / 900, rem = g - ch * 900;
      const int r = rem / 15, c0 = (rem - r * 15) * 4;
      const int q = ch < 3 ? 0 : 1;
      uint32_t packed = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float v = d[k][j] * fs[q] + fb[q];
        const float u = v * 255.0f + 0.0f;
        float t = rintf(u);
        t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
        packed |= (uint32_t)(int)t << (8 * j);
      }
      // image row = 59 - cell row (image_strategy.cpp:128-129)
      *reinterpret_cast<uint32_t *>(out + (size_t)ch * kPix + (kImg - 1 - r) * kImg + c0) = packed;
    }
  }
  tail();
  __syncthreads();
}
template <int NPL, class SM>
__device__ void finalize_planes(SM &S, const float *p012, const float *p3, uint8_t *out) {
  finalize_planes_ex<NPL, true>(S, p012, p3, out, [](float x) { return x; }, [] {});
}

// ---- one plane at a time (grasp_image_kernel): the same arithmetic as finalize_planes, with the dilated values
//      of a thread's pixel groups kept in registers across the planes that are normalised together
constexpr int GPT = (900 + IMG_THREADS - 1) / IMG_THREADS;  // groups of 4 pixels per thread and plane
__device__ inline void dilate_plane(const float *pl, float (&d)[GPT][4], float &mn, float &mx) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < GPT; k++) {
    const int g = tid + k * IMG_THREADS;
    if (g < 900) {
      const int r = g / 15, c0 = (g - r * 15) * 4;
      const int rm = r > 0 ? r - 1 : 0, rp = r < kImg - 1 ? r + 1 : kImg - 1;
      const int cl = c0 > 0 ? c0 - 1 : 0, cr = c0 + 4 < kImg ? c0 + 4 : kImg - 1;
      const float4 a = *reinterpret_cast<const float4 *>(pl + rm * kImg + c0);
      const float4 b = *reinterpret_cast<const float4 *>(pl + r * kImg + c0);
      const float4 c = *reinterpret_cast<const float4 *>(pl + rp * kImg + c0);
      const float el = fmaxf(fmaxf(pl[rm * kImg + cl], pl[r * kImg + cl]), pl[rp * kImg + cl]);
      const float er = fmaxf(fmaxf(pl[rm * kImg + cr], pl[r * kImg + cr]), pl[rp * kImg + cr]);
      const float m0 = fmaxf(fmaxf(a.x, b.x), c.x), m1 = fmaxf(fmaxf(a.y, b.y), c.y);
      const float m2 = fmaxf(fmaxf(a.z, b.z), c.z), m3 = fmaxf(fmaxf(a.w, b.w), c.w);
      d[k][0] = fmaxf(fmaxf(el, m0), m1);
      d[k][1] = fmaxf(fmaxf(m0, m1), m2);
      d[k][2] = fmaxf(fmaxf(m1, m2), m3);
      d[k][3] = fmaxf(fmaxf(m2, m3), er);
      mn = fminf(mn, fminf(fminf(d[k][0], d[k][1]), fminf(d[k][2], d[k][3])));
      mx = fmaxf(mx, fmaxf(fmaxf(d[k][0], d[k][1]), fmaxf(d[k][2], d[k][3])));
    }
  }
}
// block-wide min / max -> the scale and shift of cv::normalize(NORM_MINMAX) as floats (image_strategy.cpp:144-153)
template <class SM>
__device__ inline void minmax_scale(SM &S, float mn, float mx, float &fs, float &fb) {
  const int tid = threadIdx.x;
  mn = wave_min_f32(mn);
  mx = wave_max_f32(mx);
  __syncthreads();
  if ((tid & 63) == 0) {
    S.red_f[2 * (tid >> 6)] = mn;
    S.red_f[2 * (tid >> 6) + 1] = mx;
  }
  __syncthreads();
  float a = S.red_f[0], b = S.red_f[1];
#pragma unroll
  for (int w = 1; w < IMG_WAVES; w++) {
    a = fminf(a, S.red_f[2 * w]);
    b = fmaxf(b, S.red_f[2 * w + 1]);
  }
  const double smin = (double)a, smax = (double)b;
  const double scale = 1.0 * ((smax - smin) > DBL_EPSILON ? 1.0 / (smax - smin) : 0.0);
  const double shift = 0.0 - smin * scale;
  fs = (float)scale;
  fb = (float)shift;
}
__device__ inline void store_plane(const float (&d)[GPT][4], float fs, float fb, uint8_t *out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int k = 0; k < GPT; k++) {
    const int g = tid + k * IMG_THREADS;
    if (g < 900) {
      const int r = g / 15, c0 = (g - r * 15) * 4;
      uint32_t packed = 0;
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const float v = d[k][j] * fs + fb;
        const float u = v * 255.0f + 0.0f;
        float t = rintf(u);
        t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
        packed |= (uint32_t)(int)t << (8 * j);
      }
      // image row = 59 - cell row (image_strategy.cpp:128-129)
      *reinterpret_cast<uint32_t *>(out + (kImg - 1 - r) * kImg + c0) = packed;
    }
  }
}

template <int N>
__device__ inline void sort_u16_regs(uint16_t *p, int n);
__device__ inline void sort_u16(uint16_t *p, int n) {
  if (n <= 8) return sort_u16_regs<8>(p, n);
  if (n <= 16) return sort_u16_regs<16>(p, n);
  if (n <= 32) return sort_u16_regs<32>(p, n);
  for (int i = 1; i < n; i++) {
    const uint16_t v = p[i];
    int j = i - 1;
    while (j >= 0 && p[j] > v) {
      p[j + 1] = p[j];
      j--;
    }
    p[j + 1] = v;
  }
}
// The same with at most 16 keys in registers at a time (grasp_image_kernel is held to 128 VGPRs; the 32-key network
// alone costs it 21 spilled registers = 0.2 GB of scratch traffic per 5000 candidates).  17..32 keys: both halves
// through the 16-key network, the cross step of the bitonic merge element by element through LDS, then each half —
// a bitonic sequence now — through the 16-key merge network.  Same 240 compare-exchanges, five LDS round trips
// instead of one, and only for the few pixels that hold more than 16 points.
template <int N>
__device__ inline void merge_regs(uint32_t (&k)[N]) {  // bitonic -> ascending
#pragma unroll
  for (int stride = N >> 1; stride > 0; stride >>= 1) {
#pragma unroll
    for (int i = 0; i < N; i++) {
      const int j = i ^ stride;
      if (j > i) {
        const uint32_t lo = min(k[i], k[j]), hi = max(k[i], k[j]);
        k[i] = lo;
        k[j] = hi;
      }
    }
  }
}
template <int N>
__device__ inline void sort_regs(uint32_t (&k)[N]);
__device__ inline void sort_u16_lean(uint16_t *p, int n) {
  if (n <= 8) return sort_u16_regs<8>(p, n);
  if (n <= 16) return sort_u16_regs<16>(p, n);
  if (n > 32) return sort_u16(p, n);
  uint32_t k[16];
#pragma unroll
  for (int q = 0; q < 16; q++) k[q] = p[q];
  sort_regs<16>(k);
#pragma unroll
  for (int q = 0; q < 16; q++) p[q] = (uint16_t)k[q];
#pragma unroll
  for (int q = 0; q < 16; q++) k[q] = 16 + q < n ? (uint32_t)p[16 + q] : 0xffffffffu;
  sort_regs<16>(k);
#pragma unroll
  for (int q = 0; q < 16; q++)
    if (16 + q < n) p[16 + q] = (uint16_t)k[q];
  // cross step: element i against element 31 - i (missing ones are +inf and stay where they are)
#pragma unroll
  for (int i = 0; i < 16; i++) {
    if (31 - i < n) {
      const uint16_t a = p[i], b = p[31 - i];
      p[i] = a < b ? a : b;
      p[31 - i] = a < b ? b : a;
    }
  }
#pragma unroll
  for (int q = 0; q < 16; q++) k[q] = p[q];
  merge_regs<16>(k);
#pragma unroll
  for (int q = 0; q < 16; q++) p[q] = (uint16_t)k[q];
#pragma unroll
  for (int q = 0; q < 16; q++) k[q] = 16 + q < n ? (uint32_t)p[16 + q] : 0xffffffffu;
  merge_regs<16>(k);
#pragma unroll
  for (int q = 0; q < 16; q++)
    if (16 + q < n) p[16 + q] = (uint16_t)k[q];
}
// N keys in registers, ascending (bitonic network, fully unrolled: 24 / 80 / 240 compare-exchanges
// for N = 8 / 16 / 32).  The walks order their short per-pixel segments through registers: N
// independent LDS reads, the network, N writes — one LDS round trip instead of the dependent
// read-compare-write chain of an insertion sort (~300 cycles per step, O(n^2) steps).
template <int N>
__device__ inline void sort_regs(uint32_t (&k)[N]) {
#pragma unroll
  for (int size = 2; size <= N; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
#pragma unroll
      for (int i = 0; i < N; i++) {
        const int j = i ^ stride;
        if (j > i) {
          const uint32_t lo = min(k[i], k[j]), hi = max(k[i], k[j]);
          const bool up = (i & size) == 0;
          k[i] = up ? lo : hi;
          k[j] = up ? hi : lo;
        }
      }
    }
  }
}
template <int N>
__device__ inline void sort_u16_regs(uint16_t *p, int n) {
  uint32_t k[N];
#pragma unroll
  for (int q = 0; q < N; q++) k[q] = q < n ? (uint32_t)p[q] : 0xffffffffu;
  sort_regs<N>(k);
#pragma unroll
  for (int q = 0; q < N; q++)
    if (q < n) p[q] = (uint16_t)k[q];
}

// the candidate's box in scalar registers, bounds exactly as findPointsInUnitImage /
// transformPointsToUnitImage evaluate them (image_strategy.cpp:53-90)
__device__ inline void load_box(const gpd_hand &H, Box &B) {
  const ImgConsts &K = c_img;
#pragma unroll
  for (int i = 0; i < 9; i++) B.F[i] = uniform_f64(H.frame[i]);
#pragma unroll
  for (int i = 0; i < 3; i++) B.sample[i] = uniform_f64(H.sample[i]);
  const double hb = uniform_f64(H.bottom), hc = uniform_f64(H.center);
  B.off[0] = hb;
  B.off[1] = uniform_f64(hc - K.half_od);
  B.off[2] = uniform_f64(-K.vol_height);  // (t2 + height) == t2 - (-height)
  B.lo[0] = hb;
  B.hi[0] = uniform_f64(hb + K.vol_depth);
  B.lo[1] = B.off[1];
  B.hi[1] = uniform_f64(hc + K.half_od);
  B.lo[2] = uniform_f64(-1.0 * K.vol_height);
  B.hi[2] = uniform_f64(K.vol_height);
}

}  // namespace gpd
