// Grasp-image generation on gfx950: one workgroup per candidate, image tiles in LDS.
//
// Replaces ImageGenerator::createImages / createImageList (descriptor/image_generator.cpp:17-99),
// ImageStrategy::{transformToUnitImage, findPointsInUnitImage, transformPointsToUnitImage,
// findCellIndices, createNormalsImage, createDepthImage, createShadowImage}
// (descriptor/image_strategy.cpp:32-243), Image{15,12,3}ChannelsStrategy::{createImage,
// calculateImage, calculateChannels} (image_15_channels_strategy.cpp:27-105,
// image_12_channels_strategy.cpp:27-86, image_3_channels_strategy.cpp:27-42,
// image_1_channels_strategy.cpp:25-49) and
// HandSet::{calculateShadow, calculateShadowForCamera, shadowVoxelsToPoints, fastrand}
// (candidate/hand_set.cpp:118-283).
//
// The reference rasterises with per-pixel recurrences whose result depends on the order
// in which points hit a pixel (neighbour order; image_strategy.cpp:130-142, 166-174,
// 202-210).  Here every projection is a counting sort of the in-box points by pixel
// (LDS atomics, any order), after which the thread that owns a pixel orders its short
// segment by neighbour rank — through registers (bitonic network on 8/16/32 keys), the pixels
// handed out longest first — and runs the recurrence sequentially: same arithmetic, same order.  Shadow voxels (hand_set.cpp:202-233 hash set) become a bitset
// over the candidate's voxel AABB: set semantics for free, and walking the bits in index
// order is the lexicographic voxel order the oracle defines.
//
// The 33*N LCG draws of a hand set are generated once per set by shadow_set_kernel with
// jump-ahead (hand_set.cpp:263-266 is an affine map mod 2^32) into a bitset around the sample;
// each candidate extracts the voxels of its own box from it.
//
// Cell indices floor((x/len)/(1/60)) (image_strategy.cpp:92-102) are monotone in x, so
// they are looked up in a table of exact double thresholds computed on the host with the
// same IEEE divisions — bit-identical to dividing, without fp64 divisions in the kernel.
// Only the depth value that enters a pixel's running mean is actually divided.
//
// Device images are planar u8 [n][C][60][60]; the cv::Mat HWC layout of the reference
// interface is produced by planar_to_hwc_kernel when the caller asks for the pixels.
//
// This is the stage's ONE device unit: every image kernel reads c_img, so the kernels, the block's load and
// images_launch are here.  The caps, the voxel windows and the contents of the block are image_model.h (plain C++),
// the helpers and LDS structs the per-candidate bodies share image_device.h, and the host state around a launch —
// buffers, the window class, the block's values — image_state.hip.
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <mutex>

#include "const_block.h"
#include "gpd_internal.h"
#include "image_model.h"

namespace gpd {

__constant__ ImgConsts c_img;

struct ImgParams {
  const float *nn;
  int cap;
  const double *centers;
  const gpd_hand *hands;      // [S][slots] records of the search
  const int32_t *cand_hand;   // [n] record of a candidate (plan_kernel)
  const int32_t *meta;    // [n][4]: sample slot, N_images, first shadow bitset (< 0: no shadow), number of bitsets (cameras)
  const uint32_t *set_bits;  // [live sets][Vox::SETWORDS] shadow voxel bitsets (shadow_set_kernel)
  uint8_t *images;        // planar [n][C][3600]
  int32_t *status;
  int num_cand;              // candidates of the launch (the kernels that do not take a list)
  const int32_t *cand_list;  // large instantiations: the queued candidates (nullptr: all, in XCD-aware order) ...
  const int32_t *cand_count; // ... and how many there are (device side: nothing waits for the count)
  int32_t *overflow_list;    // shadow kernel: candidates whose box exceeds SHC voxels
  int32_t *overflow_count;
  unsigned long long *dbg;  // profiling aid (GPD_IMG_TIMING=1): per-phase cycle sums
  int32_t *pts_overflow_list;   // points kernel: candidates with more than PT_CAP in-box points
  int32_t *pts_overflow_count;
  char *pts_scratch;            // fallback instantiation: PTS_SCRATCH_BYTES per listed candidate
  int exit_after;               // read by the instrumented build only (profiles/img_exits.patch: leave the kernel after phase k)
  char *huge_scratch;           // shadow_image_any_kernel: HUGE_SCRATCH_BYTES per workgroup of its grid
};

}  // namespace gpd

#include "image_device.h"  // reads c_img: behind its definition

namespace gpd {

// The point of voxel (vx, vy, vz) that the box test, the cell lookup and the depth take is its lattice position or, in the
// JIT instantiations (gpd_hip_set_shadow_jitter), that moved by the voxel's own draw: voxel_shift, added to all three
// coordinates in the operand order of hand_set.cpp:197-199, unfused (jitter_model.h).  The draw is a hash of (seed, voxel),
// eight 64-bit multiplies, recomputed wherever a voxel's point is needed instead of kept per list entry (the lists fill the LDS).
__device__ __forceinline__ double voxel_shift(int vx, int vy, int vz) {
  return jitter::shift(jitter::draw(c_img.jitter_seed, vx, vy, vz), c_img.voxel);
}

#define TICK(k)                                                     \
  do {                                                              \
    if (P.dbg && tid == 0) {                                        \
      const unsigned long long now_ = __builtin_readcyclecounter(); \
      atomicAdd(&P.dbg[k], now_ - t_last);                          \
      t_last = now_;                                                \
    }                                                               \
  } while (0)

// ---------------------------------------------------------------------------
// shadow_image_kernel: the shadow channel of the three projections of one candidate
// (createShadowImage, image_strategy.cpp:192-233; 15 channels only).
// ---------------------------------------------------------------------------
// XCD-aware candidate order (workgroup L runs on XCD L % 8, one L2 per XCD): XCD x takes the x-th
// eighth of the candidate list, so the candidates of one hand set — which read the same neighbourhood
// rows / the same shadow bitset — meet in ONE L2 instead of being dealt out over all eight.
// Launch with 8 * ceil(n / 8) workgroups; returns -1 for the padding ones.
__device__ __forceinline__ int xcd_candidate(int n) {
  const int per = (n + 7) >> 3;
  const int L = blockIdx.x, slot = L >> 3;
  const int cand = (L & 7) * per + slot;
  return cand < n ? cand : -1;
}

template <int SHC, bool WIDE, bool JIT>
__device__ __forceinline__ void shadow_image_body(const ImgParams &P, SmemShadow<SHC, WIDE> &S, const int cand) {
  constexpr int VDIM = Vox<WIDE>::VD, SD = Vox<WIDE>::SD, SR = Vox<WIDE>::SR, LB = Vox<WIDE>::LB, SETWORDS = Vox<WIDE>::SETWORDS;
  unsigned long long t_last = __builtin_readcyclecounter();
  const ImgConsts &K = c_img;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int set_ord = P.meta[4 * cand + 2];
  const int set_nb = P.meta[4 * cand + 3];
  uint8_t *out = P.images + (size_t)cand * kPix * K.C;
  Box B;
  load_box(P.hands[P.cand_hand[cand]], B);
  for (int i = tid; i < 3 * (kImg + 1); i += IMG_THREADS) (&S.thr[0][0])[i] = (&K.thr[0][0])[i];
  for (int i = tid; i < 128; i += IMG_THREADS) S.recip[i] = i ? 1.0 / (double)i : 0.0;
  // the pixel counters of the first projection start from zero (nothing touches `cells` before the projections, and the
  // barriers of the list phases lie between this and the first count; projections 1 and 2 find them cleared by the last
  // phase of the projection before)
  for (int c = tid; c < kPix / 4; c += IMG_THREADS) reinterpret_cast<uint4 *>(S.cells)[c] = make_uint4(0u, 0u, 0u, 0u);
  if (tid == 0) {
    S.flag = 0;
    // voxel AABB of the image box: corners sample + F * (bx, by, bz)
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const double bx = (k & 1) ? B.hi[0] : B.lo[0];
      const double by = (k & 2) ? B.hi[1] : B.lo[1];
      const double bz = (k & 4) ? B.hi[2] : B.lo[2];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double w = B.sample[a] + B.F[3 * a] * bx + B.F[3 * a + 1] * by + B.F[3 * a + 2] * bz;
        lo[a] = fmin(lo[a], w);
        hi[a] = fmax(hi[a], w);
      }
    }
    if constexpr (JIT) {  // every voxel whose MOVED point can lie in the box: the AABB grows by the bound of the shift
#pragma unroll
      for (int a = 0; a < 3; a++) {
        lo[a] = lo[a] - jitter::kShiftBound;
        hi[a] = hi[a] + jitter::kShiftBound;
      }
    }
    // capacity: the box must fit the VDIM^3 voxel window of this kernel and the SD^3 region that
    // shadow_set_kernel voxelised around the sample; a larger image volume is reported
    // (GPD_ERR_CAPACITY, flag 1) instead of silently losing shadow voxels
    int bad = 0;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const int v0 = (int)floor(lo[a] * K.voxel_mult) - 1, v1 = (int)floor(hi[a] * K.voxel_mult) + 1;
      const int o = (int)floor(B.sample[a] * K.voxel_mult) - SR;
      S.vorg[a] = v0;
      // (the window's one-voxel margins may stick out of the region: they hold no voxel of the box)
      if (v1 - v0 >= VDIM || v0 + 1 < o || v1 - 1 >= o + SD) bad = 1;
    }
    S.flag = bad;
  }
  __syncthreads();
  const int x0 = S.vorg[0], y0 = S.vorg[1], z0 = S.vorg[2];
  // ---- the set's shadow voxels (shadow_set_kernel) restricted to this candidate's box:
  //      walk the AABB rows of the set bitset(s), exact f64 box test per set voxel.  A thread keeps the in-box voxels of
  //      its rows (row = tid + k * 512: neighbouring rows go to neighbouring lanes) as bit masks in registers — no
  //      candidate bitset in LDS, no atomics, nothing to zero or to count again.
  constexpr int NROWS = VDIM * VDIM, RPT = (NROWS + IMG_THREADS - 1) / IMG_THREADS;
  unsigned long long mask[RPT];
#pragma unroll
  for (int k = 0; k < RPT; k++) mask[k] = 0ull;
  if (set_ord >= 0) {
    // INVARIANT of the bitset rows: shadow_set_kernel<0> writes exactly the union of the windows floor(min) - 1 .. floor(max) + 1
    // that its candidates' boxes open (the same arithmetic as S.vorg above; min and max are those of the box's corners, with
    // the shadow jitter on moved outwards by the bound of the shift, on both sides alike); the fixed VDIM x VDIM walk below
    // can leave that union, and what it reads there is zero (images_reserve clears a new allocation) or voxels of an earlier
    // launch's set.  Neither can be kept: a bit survives only the exact f64 box test of its voxel's point, and no voxel outside
    // [floor(min), floor(max)] has its point in the box (the point lies within the bound of the voxel's lattice position).
    // A reader that counts or uses bits BEFORE that test must clamp to the union.
    const uint32_t *sb = P.set_bits + (size_t)set_ord * SETWORDS;
    const int ox = (int)floor(B.sample[0] * K.voxel_mult) - SR, oy = (int)floor(B.sample[1] * K.voxel_mult) - SR,
              oz = (int)floor(B.sample[2] * K.voxel_mult) - SR;
    const int zlo = z0 - oz;
    // t_a(z + 1) - t_a(z) = F[6 + a] * voxel, the same for every row
    double invBz[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      const double bz = B.F[6 + a] * K.voxel;
      invBz[a] = uniform_f64(fabs(bz) > 1e-9 ? 1.0 / bz : 0.0);
    }
    // 46 bits starting at rowbit + zlo, clipped to the row [0, SD): the same z range for every row
    const int za = zlo < 0 ? 0 : zlo, zb = (zlo + VDIM < SD) ? zlo + VDIM : SD;
    const int nbits = zb - za;
    // The row intervals below need the hand coordinates of a row's first voxel to ~1e-12 m only (EPS), so they come from
    // the affine form tb_a = T0_a + ix * Ax_a + iy * Ay_a and the slab faces in z-steps from one face + the slab's width
    // (24 f64 operations + two min / max per slab before); every number here is the same for the whole workgroup.
    double T0[3], Ax[3], Ay[3], Lf[3], Wd[3];
    {
      const double wx = (double)x0 * K.voxel - B.sample[0], wy = (double)y0 * K.voxel - B.sample[1],
                   wz = (double)(za - zlo + z0) * K.voxel - B.sample[2];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        T0[a] = uniform_f64(B.F[a] * wx + B.F[3 + a] * wy + B.F[6 + a] * wz);
        Ax[a] = uniform_f64(B.F[a] * K.voxel);
        Ay[a] = uniform_f64(B.F[3 + a] * K.voxel);
        Lf[a] = invBz[a] > 0.0 ? B.lo[a] : B.hi[a];                       // the face the row crosses first
        Wd[a] = uniform_f64(fabs((B.hi[a] - B.lo[a]) * invBz[a]));        // z-steps from that face to the other
      }
    }
    // Pass 1: the bit fields of all the thread's rows — straight-line loads at clamped addresses, 3 x RPT in flight
    // before the first use (inside the per-row loop below they were RPT dependent global round trips, one per row:
    // the bit loop of a row kept the next row's loads from being issued).
    unsigned long long fld[RPT];
#pragma unroll
    for (int k = 0; k < RPT; k++) fld[k] = 0ull;
    // several cameras: the shadow is the intersection of their voxel sets (hand_set.cpp:159-172)
    for (int cb = 0; cb < set_nb; cb++) {
      const uint32_t *sc = sb + (size_t)cb * SETWORDS;
      uint32_t wa[RPT], wb[RPT], wc[RPT];
#pragma unroll
      for (int k = 0; k < RPT; k++) {
        const int row = tid + k * IMG_THREADS;
        const int ix = row / VDIM, iy = row - ix * VDIM;
        const int sx = x0 + ix - ox, sy = y0 + iy - oy;
        const bool ok = row < NROWS && (unsigned)sx < (unsigned)SD && (unsigned)sy < (unsigned)SD && za < zb;
        const int w0 = ok ? ((sx * SD + sy) * SD + za) >> 5 : 0;
        wa[k] = sc[w0];
        wb[k] = sc[w0 + 1 < SETWORDS ? w0 + 1 : SETWORDS - 1];
        wc[k] = sc[w0 + 2 < SETWORDS ? w0 + 2 : SETWORDS - 1];
      }
#pragma unroll
      for (int k = 0; k < RPT; k++) {
        const int row = tid + k * IMG_THREADS;
        const int ix = row / VDIM, iy = row - ix * VDIM;
        const int sx = x0 + ix - ox, sy = y0 + iy - oy;
        const bool ok = row < NROWS && (unsigned)sx < (unsigned)SD && (unsigned)sy < (unsigned)SD && za < zb;
        const int b0 = ok ? (sx * SD + sy) * SD + za : 0;
        const int w0 = b0 >> 5, sh = b0 & 31;
        const unsigned long long lo64 = (unsigned long long)wa[k] | ((unsigned long long)(w0 + 1 < SETWORDS ? wb[k] : 0u) << 32);
        const unsigned long long hi = (w0 + 2 < SETWORDS) ? wc[k] : 0u;
        const unsigned long long f = (lo64 >> sh) | (sh ? (hi << (64 - sh)) : 0ull);
        fld[k] = !ok ? 0ull : (cb == 0 ? f : (fld[k] & f));
      }
    }
#pragma unroll
    for (int k = 0; k < RPT; k++) {
      const int row = tid + k * IMG_THREADS;
      if (row >= NROWS) continue;
      const int ix = row / VDIM, iy = row - ix * VDIM;
      unsigned long long field = fld[k];
      field &= (nbits >= 64) ? ~0ull : ((1ull << (nbits > 0 ? nbits : 0)) - 1ull);
      if (field) {
        // The row is a line along world z: its hand-frame coordinates are affine in z, t_a(z) = tb_a + z * bz_a, so per slab
        // lo_a < t_a < hi_a the voxels inside form an interval of z.  Voxels at least EPS steps inside all three intervals
        // are in the box (sure), voxels at least EPS outside one are not; only a voxel within EPS of a slab face goes
        // through the exact f64 test of the oracle below.  EPS = 1e-3 steps is >= 1e-12 m of hand coordinate (|bz| > 1e-9)
        // against ~1e-15 m of rounding in either evaluation, and ~1e-7 steps of error in the quotient.  (Every voxel of
        // the interval used to be tested exactly: ~35 VALU instructions per voxel and wave trip, a sixth of the kernel's
        // instructions — profiles/pmc_mix.sh: the kernel keeps the VALU pipe 56 % busy, it is instruction bound.)
        // With the shadow jitter on, the row's voxels are not on the line: a hand coordinate of a voxel's point is up to JB off
        // it (jitter_model.h), so both bands are that much wider — in z-steps, JB * |1 / bz_a| — and so are the micrometre
        // bands of the parallel branch.
        constexpr double EPS = 1e-3;
        constexpr double JB = JIT ? jitter::kHandShiftBound : 0.0;
        const double fx = (double)ix, fy = (double)iy;
        double dmin = 0.0, dmax = (double)(nbits - 1);  // may be inside
        double smin = 0.0, smax = (double)(nbits - 1);  // surely inside
#pragma unroll
        for (int a = 0; a < 3; a++) {
          const double tba = T0[a] + fx * Ax[a] + fy * Ay[a];
          if (invBz[a] != 0.0) {
            const double dl = (Lf[a] - tba) * invBz[a], dh = dl + Wd[a];
            double eps = EPS;
            if constexpr (JIT) eps = EPS + JB * fabs(invBz[a]);
            dmin = fmax(dmin, dl - eps);
            dmax = fmin(dmax, dh + eps);
            smin = fmax(smin, dl + eps);
            smax = fmin(smax, dh - eps);
          } else if (tba < B.lo[a] - (1e-6 + JB) || tba > B.hi[a] + (1e-6 + JB)) {
            dmax = -1.0;  // the row runs parallel to this slab (it moves < 1e-7 m over its 64 voxels), outside it
          } else if (!(tba > B.lo[a] + (1e-6 + JB) && tba < B.hi[a] - (1e-6 + JB))) {
            smax = -1.0;  // parallel and within a micrometre of a face: every voxel of the row is tested
          }
        }
        if (dmax < dmin) {
          field = 0ull;
        } else {
          const int t0 = (int)ceil(dmin), t1 = (int)floor(dmax);
          if (t0 > 0) field &= ~((1ull << t0) - 1ull);
          if (t1 < 63) field &= (2ull << t1) - 1ull;
          if (smax >= smin) {
            const int u0 = (int)ceil(smin), u1 = (int)floor(smax);
            if (u1 >= u0) {
              unsigned long long sure = field;
              if (u0 > 0) sure &= ~((1ull << u0) - 1ull);
              if (u1 < 63) sure &= (2ull << u1) - 1ull;
              mask[k] |= sure << (za - zlo);
              field &= ~sure;
            }
          }
        }
      }
      while (field) {
        const int t = __ffsll((long long)field) - 1;
        field &= field - 1;
        const int iz = za + t - zlo;
        double th[3];
        if constexpr (JIT) {
          const double sh = voxel_shift(ix + x0, iy + y0, iz + z0);
          to_hand(B, (double)(ix + x0) * K.voxel + sh, (double)(iy + y0) * K.voxel + sh, (double)(iz + z0) * K.voxel + sh, th);
        } else {
          to_hand(B, (double)(ix + x0) * K.voxel, (double)(iy + y0) * K.voxel, (double)(iz + z0) * K.voxel, th);
        }
        if (in_box(B, th)) mask[k] |= 1ull << iz;
      }
    }
  }
  // ---- ordered list of the in-box voxels (ascending voxel index = row, then z): row counts -> exclusive prefix over
  //      the rows in row order (a thread sums RPT consecutive rows) -> every thread writes its rows' voxels
#pragma unroll
  for (int k = 0; k < RPT; k++) {
    const int row = tid + k * IMG_THREADS;
    if (row < NROWS) S.bp.rows.rowcnt[row] = (uint8_t)__popcll(mask[k]);
  }
  __syncthreads();
  TICK(0);
  int cnt = 0;
#pragma unroll
  for (int k = 0; k < RPT; k++) {
    const int row = tid * RPT + k;
    if (row < NROWS) cnt += S.bp.rows.rowcnt[row];
  }
  int n_sh;
  int pos = block_excl_scan(S, cnt, &n_sh);
  if (n_sh > SHC) {  // this instantiation cannot list the box: queue the candidate for the large one
    if (tid == 0) {
      if (P.overflow_list) {
        const int slot = atomicAdd(P.overflow_count, 1);
        P.overflow_list[slot] = cand;
      } else {
        atomicOr(P.status, 4);
      }
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < RPT; k++) {
    const int row = tid * RPT + k;
    if (row < NROWS) {
      S.bp.rows.rowbase[row] = (uint16_t)pos;
      pos += S.bp.rows.rowcnt[row];
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < RPT; k++) {
    const int row = tid + k * IMG_THREADS;
    if (row >= NROWS) continue;
    unsigned long long m = mask[k];
    int at = S.bp.rows.rowbase[row];
    const int rx = row / VDIM, ry = row - rx * VDIM;
    const uint32_t rowpos = ((uint32_t)rx << 12) | ((uint32_t)ry << 6);  // shifts instead of divisions wherever it is read
    while (m) {
      const int iz = __ffsll((long long)m) - 1;
      m &= m - 1;
      S.lin[at++] = rowpos | (uint32_t)iz;
    }
  }
  __syncthreads();  // from here on bp.place may overwrite the row tables
  const int ns = n_sh < SHC ? n_sh : SHC;
  if (P.dbg && tid == 0) {
    atomicMax(&P.dbg[28], (unsigned long long)n_sh);
    atomicAdd(&P.dbg[29], (unsigned long long)n_sh);
  }
  // the three cell coordinates of every entry, once: voxel -> hand frame -> exact threshold lookup
  for (int k = tid; k < ns; k += IMG_THREADS) {
    const int lin = (int)S.lin[k];
    const int ix = lin >> 12, iy = (lin >> 6) & 63, iz = lin & 63;
    double th[3];
    if constexpr (JIT) {
      const double sh = voxel_shift(ix + x0, iy + y0, iz + z0);
      to_hand(B, (double)(ix + x0) * K.voxel + sh, (double)(iy + y0) * K.voxel + sh, (double)(iz + z0) * K.voxel + sh, th);
    } else {
      to_hand(B, (double)(ix + x0) * K.voxel, (double)(iy + y0) * K.voxel, (double)(iz + z0) * K.voxel, th);
    }
    const uint32_t c3 = cells_of(S, B, th);
    S.lin[k] = (uint32_t)lin | ((c3 & 0xfffu) << LB);
    S.cz[k] = (uint8_t)(c3 >> 12);
  }
  __syncthreads();
  TICK(1);
  auto cell_of_entry = [&](int k, int pr) {
    const uint32_t v = S.lin[k];
    return cell_of_key(((v >> LB) & 0xfffu) | ((uint32_t)S.cz[k] << 12), pr);
  };
  // A pixel of the raster that no voxel falls into holds EMPTY, a bit pattern no running mean takes (a NaN: the means are
  // sums and products of finite numbers — voxel indices, the box's frame, table reciprocals); the final phase reads it
  // as the 0 of the reference's zero-initialised image (the hook handed to finalize_planes_ex below).
  constexpr uint32_t EMPTY = 0xffffffffu;
  for (int pr = 0; pr < 3; pr++) {
    // Seven barriers per projection (sixteen before): count | scan (2) | place and list | walk | final (2).
    // (the pixel counters are zero: cleared at the kernel's entry, then by the last phase of the previous projection —
    // that was a pass and a barrier of its own at this place)
    if (tid < 32) reinterpret_cast<int *>(S.red_f)[tid] = 0;  // the histogram of scan_cells_hist
    for (int k = tid; k < ns; k += IMG_THREADS) atomicAdd(&S.cells[cell_of_entry(k, pr)], 1u);
    __syncthreads();
    uint32_t pk[2];
    scan_cells_hist(S, pk);
    scatter_nonempty(S, S.nz, pk);
    for (int k = tid; k < ns; k += IMG_THREADS) {
      const uint32_t old = atomicAdd(&S.cells[cell_of_entry(k, pr)], 1u);
      S.bp.place[(old >> 16) + (old & 0xffffu)] = (uint16_t)k;
    }
    const int da = depth_axis(pr);
    // column `da` of F and the matching offset, selected without indexing the register-resident box
    const double Fd0 = da == 0 ? B.F[0] : (da == 1 ? B.F[1] : B.F[2]);
    const double Fd1 = da == 0 ? B.F[3] : (da == 1 ? B.F[4] : B.F[5]);
    const double Fd2 = da == 0 ? B.F[6] : (da == 1 ? B.F[7] : B.F[8]);
    const double offd = da == 0 ? B.off[0] : (da == 1 ? B.off[1] : B.off[2]);
    float lmax = -FLT_MAX;
    int lany = 0;
    // The raster is reset in the phase of the segment table (it followed the list, with a barrier of its own): its last
    // readers, the dilation loads of the previous projection, are behind that projection's closing barrier, and the
    // walk that writes it next starts behind the barrier below.
    for (int c = tid; c < kPix / 4; c += IMG_THREADS) {
      const float e = __uint_as_float(EMPTY);
      reinterpret_cast<float4 *>(S.raster0)[c] = make_float4(e, e, e, e);
    }
    __syncthreads();
    TICK(2);
    const int n_nz = S.nnz;
    TICK(9);
    for (int qn = tid; qn < n_nz; qn += IMG_THREADS) {
      const int c = S.nz[qn];
      const uint32_t w = S.cells[c];
      const int cn = (int)(w & 0xffffu), start = (int)(w >> 16);
      float v = 0.f, fc = 0.f;
      auto visit = [&](int k) {  // one set voxel, in ascending voxel order (the std::set order of the oracle)
        const int lin = (int)(S.lin[k] & ((1u << LB) - 1u));
        const int ix = lin >> 12, iy = (lin >> 6) & 63, iz = lin & 63;
        double sh = 0.0;
        if constexpr (JIT) sh = voxel_shift(ix + x0, iy + y0, iz + z0);
        const double c0 = (JIT ? (double)(ix + x0) * K.voxel + sh : (double)(ix + x0) * K.voxel) - B.sample[0],
                     c1 = (JIT ? (double)(iy + y0) * K.voxel + sh : (double)(iy + y0) * K.voxel) - B.sample[1],
                     c2 = (JIT ? (double)(iz + z0) * K.voxel + sh : (double)(iz + z0) * K.voxel) - B.sample[2];
        const double td = Fd0 * c0 + Fd1 * c1 + Fd2 * c2;
        const double d = div_len(td - offd, da);
        fc = (float)((double)fc + 1.0);
        v = (float)((double)v + (d - (double)v) * recip_count<128>(S.recip, fc));
      };
      sort_u16(&S.bp.place[start], cn);
      for (int e = 0; e < cn; e++) visit((int)S.bp.place[start + e]);
      lmax = fmaxf(lmax, v);
      lany = 1;
      S.raster0[c] = v;
    }
    // The waves leave their maxima BEFORE the barrier that ends the walk (they had a barrier pair of their own behind
    // it), in slots 4 * w + 2 / + 3 of red_f.  Those 32 words were the histogram of the list until the barrier in front
    // of the walk; n_nz, read behind that barrier, is in S.nnz, which is not written here.  The final phase below writes slots
    // 4 * w + 0 / + 1 only, so it needs no barrier against the reads that follow, and the next writer of + 2 / + 3 is
    // the next projection's count phase (it clears the histogram), behind the two barriers of the final phase.
    lmax = wave_max_f32(lmax);
    lany = __ballot(lany != 0) != 0ull;
    if (lane == 0) {
      S.red_f[4 * (tid >> 6) + 2] = lmax;
      reinterpret_cast<int *>(S.red_f)[4 * (tid >> 6) + 3] = lany;
    }
    __syncthreads();
    TICK(10);
    float gmax = -FLT_MAX;
    int gany = 0;
#pragma unroll
    for (int w = 0; w < IMG_WAVES; w++) {
      gmax = fmaxf(gmax, S.red_f[4 * w + 2]);
      gany |= reinterpret_cast<const int *>(S.red_f)[4 * w + 3];
    }
    // minMaxLoc with mask -> max (0 if the mask is empty); image = max_img - image
    const double mxd = gany ? (double)gmax : 0.0;
    const float mxf = (float)mxd;
    TICK(3);
    // `max_img - image` is taken as the dilation loads the raster (it was a read-modify-write of all 3600 pixels and a
    // barrier): a pixel with voxels gives mxf - mean, an empty one 0 - 0, the same float operations on the same
    // operands.  The last phase clears the pixel counters for the next projection: the walk was their last reader.
    finalize_planes_ex<1, false>(
        S, &S.raster0[0], nullptr, out + (size_t)(pr * K.per + 4) * kPix,
        [mxf](float x) { return __float_as_uint(x) == EMPTY ? 0.0f - 0.0f : mxf - x; },
        [&S, tid] {
          int c0 = tid;  // (opaque, so that the store address is made here and not held in a register through the whole loop)
          asm volatile("" : "+v"(c0));
          for (int c = c0; c < kPix / 4; c += IMG_THREADS) reinterpret_cast<uint4 *>(S.cells)[c] = make_uint4(0u, 0u, 0u, 0u);
        });
    TICK(4);
  }
  if (tid == 0 && S.flag) atomicOr(P.status, S.flag);
}

template <int SHC, bool WIDE>
__global__ __launch_bounds__(IMG_THREADS, SHC <= SH_CAP ? 4 : 2) void shadow_image_kernel(ImgParams P) {
  __shared__ SmemShadow<SHC, WIDE> S;
  if constexpr (SHC > SH_CAP) {
    const int count = *P.cand_count;
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
      __syncthreads();  // the previous candidate's LDS is dead
      shadow_image_body<SHC, WIDE, false>(P, S, P.cand_list[q]);
    }
  } else {
    const int cand = xcd_candidate(P.num_cand);
    if (cand < 0) return;
    shadow_image_body<SHC, WIDE, false>(P, S, cand);
  }
}
// ... with the shadow jitter on (gpd_hip_set_shadow_jitter): kernels of their own, so that the ones above are the code —
// and keep the names — they had before the mode existed
template <int SHC, bool WIDE>
__global__ __launch_bounds__(IMG_THREADS, SHC <= SH_CAP ? 4 : 2) void shadow_image_jitter_kernel(ImgParams P) {
  __shared__ SmemShadow<SHC, WIDE> S;
  if constexpr (SHC > SH_CAP) {
    const int count = *P.cand_count;
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
      __syncthreads();  // the previous candidate's LDS is dead
      shadow_image_body<SHC, WIDE, true>(P, S, P.cand_list[q]);
    }
  } else {
    const int cand = xcd_candidate(P.num_cand);
    if (cand < 0) return;
    shadow_image_body<SHC, WIDE, true>(P, S, cand);
  }
}

// ---------------------------------------------------------------------------
// shadow_image_any_kernel: the shadow channels of a candidate whose box the tuned kernels above cannot take — an image
// volume beyond their voxel windows (the host then sends EVERY candidate here), or more in-box voxels than the large
// instantiation lists (queued by it).  The reference has no size limit (hand_set.cpp:138, image_strategy.cpp:192-233);
// this is its device counterpart without one that matters: window edges up to 256 voxels (0.77 m), 65535 voxels in
// the box, a set region of run-time size.  Same arithmetic and the same order as shadow_image_body — the voxel list in
// lexicographic order, per projection a counting sort by pixel and one lane per pixel running the mean in list order —
// with the list, its cell keys and the segment table in a scratch row in global memory and none of the register tricks.
// A persistent launch: workgroup b takes entries b, b + grid, ... of its list.
// ---------------------------------------------------------------------------
struct __attribute__((aligned(16))) SmemAny {
  __attribute__((aligned(16))) float raster0[kPix];
  __attribute__((aligned(16))) uint32_t cells[kPix];
  uint16_t nz[kPix];
  double thr[3][kImg + 1];
  double recip[128];
  float red_f[4 * IMG_WAVES];
  int red_i[IMG_WAVES];
  int vorg[3], wdim[3];
  int flag;
};

template <bool JIT>
__device__ void shadow_image_any_body(const ImgParams &P, SmemAny &S, const int cand, char *scratch) {
  const ImgConsts &K = c_img;
  const int SD = K.set_sd, SR = K.set_sr;
  const size_t SETWORDS = (size_t)(((long long)SD * SD * SD + 31) / 32);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int set_ord = P.meta[4 * cand + 2];
  const int set_nb = P.meta[4 * cand + 3];
  uint8_t *out = P.images + (size_t)cand * kPix * K.C;
  int32_t *rowtab = reinterpret_cast<int32_t *>(scratch);                              // [wx * wy]: count, then start of a window row
  uint32_t *lin = reinterpret_cast<uint32_t *>(rowtab + HUGE_WIN * HUGE_WIN);          // [n]: ix | iy << 8 | iz << 16, ascending = lexicographic
  uint32_t *ckey = lin + (HUGE_CAP + 1);                                               // [n]: cell x | y << 6 | z << 12
  uint16_t *place = reinterpret_cast<uint16_t *>(ckey + (HUGE_CAP + 1));               // [n]: segment table of the counting sort
  Box B;
  load_box(P.hands[P.cand_hand[cand]], B);
  for (int i = tid; i < 3 * (kImg + 1); i += IMG_THREADS) (&S.thr[0][0])[i] = (&K.thr[0][0])[i];
  for (int i = tid; i < 128; i += IMG_THREADS) S.recip[i] = i ? 1.0 / (double)i : 0.0;
  if (tid == 0) {
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    for (int k = 0; k < 8; k++) {
      const double bx = (k & 1) ? B.hi[0] : B.lo[0];
      const double by = (k & 2) ? B.hi[1] : B.lo[1];
      const double bz = (k & 4) ? B.hi[2] : B.lo[2];
      for (int a = 0; a < 3; a++) {
        const double w = B.sample[a] + B.F[3 * a] * bx + B.F[3 * a + 1] * by + B.F[3 * a + 2] * bz;
        lo[a] = fmin(lo[a], w);
        hi[a] = fmax(hi[a], w);
      }
    }
    if constexpr (JIT) {  // as in shadow_image_body: every voxel whose moved point can lie in the box
      for (int a = 0; a < 3; a++) {
        lo[a] = lo[a] - jitter::kShiftBound;
        hi[a] = hi[a] + jitter::kShiftBound;
      }
    }
    int bad = 0;
    for (int a = 0; a < 3; a++) {
      const int v0 = (int)floor(lo[a] * K.voxel_mult) - 1, v1 = (int)floor(hi[a] * K.voxel_mult) + 1;
      const int o = (int)floor(B.sample[a] * K.voxel_mult) - SR;
      S.vorg[a] = v0;
      S.wdim[a] = v1 - v0 + 1;
      // (the window's one-voxel margins may stick out of the region: they hold no voxel of the box)
      if (v1 - v0 + 1 > HUGE_WIN || v0 + 1 < o || v1 - 1 >= o + SD) bad = 1;
    }
    S.flag = bad;
  }
  __syncthreads();
  if (S.flag) {  // beyond even this kernel (GPD_ERR_CAPACITY, flag 1): reported, never truncated
    if (tid == 0) atomicOr(P.status, 1);
    return;
  }
  const int x0 = S.vorg[0], y0 = S.vorg[1], z0 = S.vorg[2];
  const int wx = S.wdim[0], wy = S.wdim[1], wz = S.wdim[2];
  const int nrows = wx * wy;
  const int ox = (int)floor(B.sample[0] * K.voxel_mult) - SR, oy = (int)floor(B.sample[1] * K.voxel_mult) - SR,
            oz = (int)floor(B.sample[2] * K.voxel_mult) - SR;
  // the set voxels of window row (ix, iy) that lie in the box, in ascending z: emit(iz) for each.  A row is a run of wz bits
  // of the set region(s) — several cameras: the intersection of their voxel sets (hand_set.cpp:159-172) — and every set bit
  // takes the oracle's exact f64 box test
  auto walk_row = [&](int row, auto emit) {
    const int ix = row / wy, iy = row - ix * wy;
    const int sx = x0 + ix - ox, sy = y0 + iy - oy;
    if (set_ord < 0 || (unsigned)sx >= (unsigned)SD || (unsigned)sy >= (unsigned)SD) return;
    const int zlo = z0 - oz;  // region z of window z 0
    const int za = zlo < 0 ? 0 : zlo, zb = zlo + wz < SD ? zlo + wz : SD;
    if (za >= zb) return;
    const long long rowbit = ((long long)sx * SD + sy) * SD;
    for (long long w = (rowbit + za) >> 5; w <= (rowbit + zb - 1) >> 5; w++) {
      uint32_t bits = ~0u;
      for (int cb = 0; cb < set_nb; cb++) bits &= P.set_bits[((size_t)set_ord + cb) * SETWORDS + (size_t)w];
      const long long first = w << 5;  // region bit of this word's bit 0
      if (first < rowbit + za) bits &= ~0u << (int)(rowbit + za - first);
      if (first + 32 > rowbit + zb) bits &= ~0u >> (int)(first + 32 - (rowbit + zb));
      while (bits) {
        const int t = __ffs((int)bits) - 1;
        bits &= bits - 1;
        const int iz = (int)(first + t - rowbit) - zlo;
        double th[3];
        if constexpr (JIT) {
          const double sh = voxel_shift(ix + x0, iy + y0, iz + z0);
          to_hand(B, (double)(ix + x0) * K.voxel + sh, (double)(iy + y0) * K.voxel + sh, (double)(iz + z0) * K.voxel + sh, th);
        } else {
          to_hand(B, (double)(ix + x0) * K.voxel, (double)(iy + y0) * K.voxel, (double)(iz + z0) * K.voxel, th);
        }
        if (in_box(B, th)) emit(iz);
      }
    }
  };
  for (int row = tid; row < nrows; row += IMG_THREADS) {
    int cnt = 0;
    walk_row(row, [&](int) { cnt++; });
    rowtab[row] = cnt;
  }
  __threadfence_block();
  __syncthreads();
  // exclusive prefix over the rows in row order: a thread sums a run of consecutive rows
  const int per = (nrows + IMG_THREADS - 1) / IMG_THREADS;
  int cnt = 0;
  for (int k = 0; k < per; k++) {
    const int row = tid * per + k;
    if (row < nrows) cnt += rowtab[row];
  }
  int n_sh;
  int pos = block_excl_scan(S, cnt, &n_sh);
  if (n_sh > HUGE_CAP) {
    if (tid == 0) atomicOr(P.status, 4);
    return;
  }
  for (int k = 0; k < per; k++) {
    const int row = tid * per + k;
    if (row < nrows) {
      const int c = rowtab[row];
      rowtab[row] = pos;
      pos += c;
    }
  }
  __threadfence_block();
  __syncthreads();
  for (int row = tid; row < nrows; row += IMG_THREADS) {
    int at = rowtab[row];
    const int ix = row / wy, iy = row - ix * wy;
    walk_row(row, [&](int iz) {
      double th[3];
      if constexpr (JIT) {
        const double sh = voxel_shift(ix + x0, iy + y0, iz + z0);
        to_hand(B, (double)(ix + x0) * K.voxel + sh, (double)(iy + y0) * K.voxel + sh, (double)(iz + z0) * K.voxel + sh, th);
      } else {
        to_hand(B, (double)(ix + x0) * K.voxel, (double)(iy + y0) * K.voxel, (double)(iz + z0) * K.voxel, th);
      }
      lin[at] = (uint32_t)ix | ((uint32_t)iy << 8) | ((uint32_t)iz << 16);
      ckey[at] = cells_of(S, B, th);
      at++;
    });
  }
  __threadfence_block();
  __syncthreads();
  const int ns = n_sh;
  for (int pr = 0; pr < 3; pr++) {
    for (int c = tid; c < kPix; c += IMG_THREADS) S.cells[c] = 0u;
    __syncthreads();
    for (int k = tid; k < ns; k += IMG_THREADS) atomicAdd(&S.cells[cell_of_key(ckey[k], pr)], 1u);
    __syncthreads();
    scan_cells(S);
    for (int k = tid; k < ns; k += IMG_THREADS) {
      const uint32_t old = atomicAdd(&S.cells[cell_of_key(ckey[k], pr)], 1u);
      place[(old >> 16) + (old & 0xffffu)] = (uint16_t)k;
    }
    __threadfence_block();
    __syncthreads();
    const int da = depth_axis(pr);
    const double Fd0 = da == 0 ? B.F[0] : (da == 1 ? B.F[1] : B.F[2]);
    const double Fd1 = da == 0 ? B.F[3] : (da == 1 ? B.F[4] : B.F[5]);
    const double Fd2 = da == 0 ? B.F[6] : (da == 1 ? B.F[7] : B.F[8]);
    const double offd = da == 0 ? B.off[0] : (da == 1 ? B.off[1] : B.off[2]);
    float lmax = -FLT_MAX;
    int lany = 0;
    const int n_nz = list_nonempty_cells(S, S.nz);
    for (int c = tid; c < kPix; c += IMG_THREADS) S.raster0[c] = 0.f;
    __syncthreads();
    for (int qn = tid; qn < n_nz; qn += IMG_THREADS) {
      const int c = S.nz[qn];
      const uint32_t w = S.cells[c];
      const int cn = (int)(w & 0xffffu), start = (int)(w >> 16);
      float v = 0.f, fc = 0.f;
      // the segment holds list positions in arrival order: ascending position = ascending voxel (the std::set order of the oracle)
      sort_u16(&place[start], cn);
      for (int e = 0; e < cn; e++) {
        const uint32_t lp = lin[place[start + e]];
        const int ix = lp & 255, iy = (lp >> 8) & 255, iz = lp >> 16;
        double sh = 0.0;
        if constexpr (JIT) sh = voxel_shift(ix + x0, iy + y0, iz + z0);
        const double c0 = (JIT ? (double)(ix + x0) * K.voxel + sh : (double)(ix + x0) * K.voxel) - B.sample[0],
                     c1 = (JIT ? (double)(iy + y0) * K.voxel + sh : (double)(iy + y0) * K.voxel) - B.sample[1],
                     c2 = (JIT ? (double)(iz + z0) * K.voxel + sh : (double)(iz + z0) * K.voxel) - B.sample[2];
        const double td = Fd0 * c0 + Fd1 * c1 + Fd2 * c2;
        const double d = div_len(td - offd, da);
        fc = (float)((double)fc + 1.0);
        v = (float)((double)v + (d - (double)v) * recip_count<128>(S.recip, fc));
      }
      lmax = fmaxf(lmax, v);
      lany = 1;
      S.raster0[c] = v;
    }
    __syncthreads();
    lmax = wave_max_f32(lmax);
    lany = __ballot(lany != 0) != 0ull;
    if (lane == 0) {
      S.red_f[tid >> 6] = lmax;
      S.red_i[tid >> 6] = lany;
    }
    __syncthreads();
    float gmax = -FLT_MAX;
    int gany = 0;
    for (int w = 0; w < IMG_WAVES; w++) {
      gmax = fmaxf(gmax, S.red_f[w]);
      gany |= S.red_i[w];
    }
    // minMaxLoc with mask -> max (0 if the mask is empty); image = max_img - image
    const double mxd = gany ? (double)gmax : 0.0;
    const float mxf = (float)mxd;
    __syncthreads();  // red_f is rewritten by finalize_planes
    for (int c = tid; c < kPix; c += IMG_THREADS) S.raster0[c] = ((S.cells[c] & 0xffffu) ? mxf : 0.0f) - S.raster0[c];
    __syncthreads();
    finalize_planes<1>(S, &S.raster0[0], nullptr, out + (size_t)(pr * K.per + 4) * kPix);
  }
}

__global__ __launch_bounds__(IMG_THREADS) void shadow_image_any_kernel(ImgParams P) {
  __shared__ SmemAny S;
  char *scratch = P.huge_scratch + (size_t)blockIdx.x * HUGE_SCRATCH_BYTES;
  const int count = P.cand_list ? *P.cand_count : P.num_cand;
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    __syncthreads();  // the previous candidate's LDS is dead
    shadow_image_any_body<false>(P, S, P.cand_list ? P.cand_list[q] : q, scratch);
  }
}
// ... with the shadow jitter on.  A template (JIT is always true) only so that the compiler emits it with the other
// instantiations, behind the kernels of the default path (kernel_order below).
template <bool JIT>
__global__ __launch_bounds__(IMG_THREADS) void shadow_image_any_jitter_kernel(ImgParams P) {
  static_assert(JIT, "the jitter-off kernel is shadow_image_any_kernel");
  __shared__ SmemAny S;
  char *scratch = P.huge_scratch + (size_t)blockIdx.x * HUGE_SCRATCH_BYTES;
  const int count = P.cand_list ? *P.cand_count : P.num_cand;
  for (int q = blockIdx.x; q < count; q += gridDim.x) {
    __syncthreads();  // the previous candidate's LDS is dead
    shadow_image_any_body<JIT>(P, S, P.cand_list ? P.cand_list[q] : q, scratch);
  }
}

// ---------------------------------------------------------------------------
// grasp_image_kernel: normals (3) and depth (1) channels per projection of one candidate
// (createNormalsImage / createDepthImage, image_strategy.cpp:124-190).
// ---------------------------------------------------------------------------
// The small instantiation runs every projection of its candidate.  The large one is entered once per (candidate,
// projection) item of the overflow queue: `item_pr` is the one projection it runs; the points are collected per item
// (the projections are independent behind that), and what happens once per CANDIDATE — the capacity report, the flag —
// is left to the item of projection 0.
template <bool BIG>
__device__ __forceinline__ void grasp_image_body(const ImgParams &P, SmemPts<BIG> &S, const int cand, const int item_pr = 0) {
  constexpr int CAP = BIG ? PT_CAP_BIG : PT_CAP;
  unsigned long long t_last = __builtin_readcyclecounter();
  const ImgConsts &K = c_img;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int slot_s = P.meta[4 * cand + 0];
  const int N = P.meta[4 * cand + 1];
  const float *nn = P.nn + (size_t)slot_s * 6 * P.cap;
  uint8_t *out = P.images + (size_t)cand * kPix * K.C;
  // the point arrays: LDS, or this workgroup's row of the global scratch
  double *gt = nullptr;
  float4 *gan = nullptr;
  uint32_t *gidx = nullptr;
  if constexpr (BIG) {
    char *row = P.pts_scratch + (size_t)blockIdx.x * PTS_SCRATCH_BYTES;
    gt = reinterpret_cast<double *>(row);
    gan = reinterpret_cast<float4 *>(row + (size_t)CAP * 3 * sizeof(double));
    gidx = reinterpret_cast<uint32_t *>(row + (size_t)CAP * (3 * sizeof(double) + sizeof(float4)));
  }
  auto IDX = [&](int e) -> int {
    if constexpr (BIG) return (int)gidx[e];
    else return (int)S.place[e];
  };
  auto T = [&](int a, int e) -> double & {
    if constexpr (BIG) return gt[(size_t)a * CAP + e];
    else return S.p.t[a][e];
  };
  auto AN = [&](int e) -> float4 & {
    if constexpr (BIG) return gan[e];
    else return S.p.an[e];
  };
  Box B;
  load_box(P.hands[P.cand_hand[cand]], B);
  for (int i = tid; i < 3 * (kImg + 1); i += IMG_THREADS) (&S.thr[0][0])[i] = (&K.thr[0][0])[i];
  for (int i = tid; i < 128; i += IMG_THREADS) S.recip[i] = i ? 1.0 / (double)i : 0.0;
  if (tid == 0) {
    S.flag = 0;  // (S.counter is reset in front of every walk)
    S.nzv[0] = make_float4(0.f, 0.f, 0.f, 0.f);  // the empty pixel of the index raster (the walks write slots >= 1)
  }
  // the cell counters of the first projection start from zero (the ballot counts of the compaction below used to borrow
  // their storage, so they were cleared behind it, with a barrier of their own; see `cnt`)
  for (int c = tid; c < kPix / 4; c += IMG_THREADS) reinterpret_cast<uint4 *>(S.cells)[c] = make_uint4(0u, 0u, 0u, 0u);
  __syncthreads();
  // The in-box points are numbered IN NEIGHBOUR ORDER (an ordered compaction: per 512 neighbours one ballot per wave
  // and a prefix over the eight wave counts), so that an entry's number is its rank among the in-box points: the
  // walks order a pixel's segment by entry number alone — no rank bits to carry, whatever the neighbourhood size.
  // Two passes over blocks of 16 rounds (8192 neighbours): first every thread tests its 16 points — straight-line
  // loads, all in flight together, no barrier — and the waves leave their 16 x 8 ballot counts in LDS; ONE barrier; then
  // every thread derives the entry numbers of its in-box points from those counts and writes them.  (One round per
  // barrier pair exposed the latency of its global loads six times per candidate: 28 of the kernel's 130 kcycles.)
  int n_before = 0;  // in-box points of the earlier blocks (the same in every thread)
  // [16][IMG_WAVES] ballot counts, in the storage of the list of non-empty pixels: the first projection writes that list
  // three barriers into its own phases, the counts are last read in front of the barrier that closes the last block
  static_assert(offsetof(SmemPts<BIG>, nzlist) % sizeof(int) == 0 && sizeof(S.nzlist) >= 16 * IMG_WAVES * sizeof(int), "ballot counts in nzlist");
  int *cnt = reinterpret_cast<int *>(S.nzlist);
  constexpr int RB = 16;
  const int wave = tid >> 6;
  for (int b0 = 0; b0 < N; b0 += RB * IMG_THREADS) {
    unsigned inmask = 0;
    const int left = N - b0, nr = left >= RB * IMG_THREADS ? RB : (left + IMG_THREADS - 1) / IMG_THREADS;  // rounds of this block
    for (int r0 = 0; r0 < nr; r0 += 4) {  // four rounds at a time: twelve loads in flight before the first use
      float px[4], py[4], pz[4];
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int i = b0 + (r0 + q) * IMG_THREADS + tid;
        const int ic = i < N ? i : N - 1;
        px[q] = nn[0 * P.cap + ic];
        py[q] = nn[1 * P.cap + ic];
        pz[q] = nn[2 * P.cap + ic];
      }
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int r = r0 + q;
        const int i = b0 + r * IMG_THREADS + tid;
        double t[3];
        to_hand(B, (double)px[q], (double)py[q], (double)pz[q], t);
        const bool in = i < N && in_box(B, t);
        const unsigned long long ballot = __ballot(in);
        if (lane == 0) cnt[r * IMG_WAVES + wave] = __popcll(ballot);  // (rounds past nr: zeros, never read)
        inmask |= (unsigned)in << r;
      }
    }
    __syncthreads();
    int run = n_before;
    for (int r = 0; r < nr; r++) {  // entry numbers of the thread's in-box points: their neighbour indices go to the list
      int base = run;
#pragma unroll
      for (int w = 0; w < IMG_WAVES; w++) {
        const int c = cnt[r * IMG_WAVES + w];
        if (w < wave) base += c;
        run += c;
      }
      const bool in = (inmask >> r) & 1u;
      const unsigned long long ballot = __ballot(in);
      if (in) {
        const int e = base + __popcll(ballot & ((1ull << lane) - 1ull));
        if (e < CAP) {
          if constexpr (BIG) gidx[e] = (uint32_t)(b0 + r * IMG_THREADS + tid);
          else S.place[e] = (uint16_t)(b0 + r * IMG_THREADS + tid);
        }
      }
    }
    n_before = run;
    // the counts are rewritten by the next block / the entries below read the index list: for the last block this barrier
    // is the one in front of the entry phase (there is no other)
    __syncthreads();
  }
  const int n_box_all = n_before;
  if (n_box_all > CAP || (!BIG && N > 65536)) {
    // more in-box points than this instantiation holds — or a neighbourhood of more than 65536 points, whose neighbour
    // indices do not fit the 16-bit segment table the small instantiation lists them in (the reference has no limit,
    // hand_search.cpp:178; the large one keeps them 32 bits wide): queue the candidate for the large one
    // (nothing has been written yet), or report it when this already is the large one
    if (tid == 0 && (!BIG || item_pr == 0)) {
      if (!BIG && P.pts_overflow_list)
        P.pts_overflow_list[atomicAdd(P.pts_overflow_count, 1)] = cand;
      else
        atomicOr(P.status, 2);
    }
    return;
  }
  // The entries themselves, densely: one in-box point per lane (hand-frame coordinates, |normal| in the hand frame, the
  // three cell coordinates: ~150 instructions) — inside the rounds above a wave paid them per round for the one lane
  // in seven that was in the box (a sixth of the kernel's instructions; it is instruction bound, profiles/pmc_mix.sh).
  for (int e0 = 0; e0 < n_box_all; e0 += 2 * IMG_THREADS) {
    float v[2][6];
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int e = e0 + q * IMG_THREADS + tid;
      const int i = e < n_box_all ? IDX(e) : 0;
#pragma unroll
      for (int a = 0; a < 6; a++) v[q][a] = nn[a * P.cap + i];
    }
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int e = e0 + q * IMG_THREADS + tid;
      if (e < n_box_all) {
        double t[3];
        to_hand(B, (double)v[q][0], (double)v[q][1], (double)v[q][2], t);
        const double n0 = (double)v[q][3], n1 = (double)v[q][4], n2 = (double)v[q][5];
        T(0, e) = t[0];
        T(1, e) = t[1];
        T(2, e) = t[2];
        AN(e) = make_float4((float)fabs(B.F[0] * n0 + B.F[3] * n1 + B.F[6] * n2),
                            (float)fabs(B.F[1] * n0 + B.F[4] * n1 + B.F[7] * n2),
                            (float)fabs(B.F[2] * n0 + B.F[5] * n1 + B.F[8] * n2), __uint_as_float(cells_of(S, B, t)));
      }
    }
  }
  // (the index list lives in the segment table; the first projection rewrites it two barriers from here)
  if constexpr (BIG) {
    __threadfence_block();  // the point arrays are global memory here: written above, read by other lanes below
    __syncthreads();
  }
  const int nb = n_box_all;
  if (P.dbg && tid == 0) {
    atomicMax(&P.dbg[30], (unsigned long long)n_box_all);
    atomicAdd(&P.dbg[31], (unsigned long long)n_box_all);
  }
  TICK(5);
  // No barrier between the entries and the first count (there was one, behind the clearing of the cell counters that has
  // moved to the kernel's entry): a thread counts and places exactly the entries it has written itself (e = tid + k *
  // IMG_THREADS in all three loops), and the index list in `place`, which other threads read above, is rewritten only
  // behind the barrier of the count.
  const int pr_first = BIG ? item_pr : 0, pr_end = BIG ? item_pr + 1 : K.nproj;
  for (int pr = pr_first; pr < pr_end; pr++) {
    // Nine barriers per projection (fifteen before): count | scan (2) | place and list | walk | listing of the live
    // groups | min / max | staging | copy-out.
    // (the cell counters are zero: cleared at the entry, then by the copy-out of the previous projection)
    if (tid < 32) reinterpret_cast<int *>(S.red_f)[tid] = 0;  // the histogram of scan_cells_hist
    for (int e = tid; e < nb; e += IMG_THREADS) atomicAdd(&S.cells[cell_of_key(__float_as_uint(AN(e).w), pr)], 1u);
    __syncthreads();
    uint32_t pk[2];
    scan_cells_hist(S, pk);
    uint16_t *nz = S.nzlist;
    scatter_nonempty(S, nz, pk);
    for (int e = tid; e < nb; e += IMG_THREADS) {
      const uint32_t key = __float_as_uint(AN(e).w);
      const uint32_t old = atomicAdd(&S.cells[cell_of_key(key, pr)], 1u);
      S.place[(old >> 16) + (old & 0xffffu)] = (uint16_t)e;
    }
    __syncthreads();
    TICK(6);
    // the pixel owner walks its segment in neighbour order
    const int da = depth_axis(pr);
    const double offd = da == 0 ? B.off[0] : (da == 1 ? B.off[1] : B.off[2]);
    const int n_nz = S.nnz;
    TICK(11);
    // the counter of the live-group list below is reset here, in front of the walk's barrier (it had a barrier of its
    // own behind it): its last reader, `n_live` of the previous projection, is three barriers back
    if (tid == 0) S.counter = 0;
    for (int qn = tid; qn < n_nz; qn += IMG_THREADS) {
      const int c = nz[qn];
      const uint32_t w = S.cells[c];
      const int cn = (int)(w & 0xffffu), start = (int)(w >> 16);
      float v0 = 0.f, v1 = 0.f, v2 = 0.f;
      float avg = 0.f, fc = 0.f;
      auto visit = [&](int e) {  // one in-box point, in neighbour order
        const float4 an = AN(e);
        const float a0 = an.x, a1 = an.y, a2 = an.z;
        if (v0 == 0.f && v1 == 0.f && v2 == 0.f) {
          v0 = a0;
          v1 = a1;
          v2 = a2;
        } else {
          const float sq = sqrtf(v0 * v0 + v1 * v1 + v2 * v2);
          const double inv = 1.0 / (double)sq;
          const float d0 = a0 - v0, d1 = a1 - v1, d2 = a2 - v2;
          v0 = v0 + (float)((double)d0 * inv);
          v1 = v1 + (float)((double)d1 * inv);
          v2 = v2 + (float)((double)d2 * inv);
        }
        const double d = div_len(T(da, e) - offd, da);
        fc = (float)((double)fc + 1.0);
        avg = (float)((double)avg + (d - (double)avg) * recip_count<128>(S.recip, fc));
      };
      sort_u16_lean(&S.place[start], cn);  // neighbour order = entry order
      for (int q = 0; q < cn; q++) visit((int)S.place[start + q]);
      S.nzv[qn + 1] = make_float4(v0, v1, v2, (float)(1.0 - (double)avg));
      S.cells[c] = 0x80000000u | (uint32_t)(qn + 1);  // the pixel's own word, read above: from here on the index raster
    }
    TICK(13);
    __syncthreads();
    TICK(7);
    // ---- the four planes of the projection at once.  `cells` is now an index raster: bit 31 set <-> the pixel holds
    //      points, low bits = its slot in nzv (float4: the three normal values and the depth value); every other word has
    //      bit 31 clear (segment starts are < 2^15) and stands for the empty pixel, slot 0 = zeros.  A group of four pixels
    //      is dilated for all four planes from one set of index reads + float4 gathers (a dense float raster per plane
    //      cost four scatter / dilate / barrier rounds); empty pixels take part with the value 0 exactly as in the
    //      reference's zero-initialised cv::Mat (the running normal "average" can go negative, so 0 matters).
    //      Five groups in six have no point in their 3 x 6 window: they are background in all four planes — the value 0
    //      enters the min / max and the normalised byte of 0 is stored, nothing to gather, dilate or round.  The others
    //      are LISTED first (one ballot + one LDS atomic per wave) and dealt out over the whole workgroup, one or two per
    //      thread.  (Measured: image stage 1.254 -> 1.242 ms; skipping the background groups in place, without the
    //      list, gave the same.)
    const bool with_normals = K.C != 1, with_depth = K.C == 1 || K.C >= 12;
    uint16_t *alist = S.place;  // the segment table is dead after the walks
    bool live[GPT];  // this thread's own groups tid + k * IMG_THREADS: does the window hold points?
    auto window = [&](int g, uint32_t(&ix)[3][6]) {
      const int r = g / 15, c0 = (g - r * 15) * 4;
      const int rows[3] = {r > 0 ? r - 1 : 0, r, r < kImg - 1 ? r + 1 : kImg - 1};
      const int cl = c0 > 0 ? c0 - 1 : 0, cr = c0 + 4 < kImg ? c0 + 4 : kImg - 1;
      uint32_t any = 0;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const uint4 m = *reinterpret_cast<const uint4 *>(&S.cells[rows[q] * kImg + c0]);
        ix[q][0] = S.cells[rows[q] * kImg + cl];
        ix[q][1] = m.x;
        ix[q][2] = m.y;
        ix[q][3] = m.z;
        ix[q][4] = m.w;
        ix[q][5] = S.cells[rows[q] * kImg + cr];
#pragma unroll
        for (int e = 0; e < 6; e++) any |= ix[q][e];
      }
      return (any >> 31) != 0u;
    };
    TICK(12);
#pragma unroll
    for (int k = 0; k < GPT; k++) {
      const int g = tid + k * IMG_THREADS;
      uint32_t ix[3][6];
      live[k] = g < 900 && window(g, ix);
      const unsigned long long ballot = __ballot(live[k]);
      if (ballot) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&S.counter, __popcll(ballot));
        base = __builtin_amdgcn_readfirstlane(base);
        if (live[k]) alist[base + __popcll(ballot & ((1ull << lane) - 1ull))] = (uint16_t)g;
      }
    }
    __syncthreads();
    const int n_live = S.counter;
    float d[GPT][4][4];  // the thread's live groups alist[tid + k * IMG_THREADS]: [plane][pixel]
    float mn0 = FLT_MAX, mx0 = -FLT_MAX, mn1 = FLT_MAX, mx1 = -FLT_MAX;
    if (n_live < 900) {  // some group is background
      mn0 = mn1 = 0.f;
      mx0 = mx1 = 0.f;
    }
#pragma unroll
    for (int k = 0; k < GPT; k++) {
      const int a = tid + k * IMG_THREADS;
      if (a < n_live) {
        uint32_t ix[3][6];
        window((int)alist[a], ix);
        float col[4][6];  // per plane: column maxima over the three rows
#pragma unroll
        for (int e = 0; e < 6; e++) {
          const float4 va = S.nzv[(ix[0][e] >> 31) ? (ix[0][e] & 0xffffu) : 0u];
          const float4 vb = S.nzv[(ix[1][e] >> 31) ? (ix[1][e] & 0xffffu) : 0u];
          const float4 vc = S.nzv[(ix[2][e] >> 31) ? (ix[2][e] & 0xffffu) : 0u];
          col[0][e] = fmaxf(fmaxf(va.x, vb.x), vc.x);
          col[1][e] = fmaxf(fmaxf(va.y, vb.y), vc.y);
          col[2][e] = fmaxf(fmaxf(va.z, vb.z), vc.z);
          col[3][e] = fmaxf(fmaxf(va.w, vb.w), vc.w);
        }
#pragma unroll
        for (int pl = 0; pl < 4; pl++) {
#pragma unroll
          for (int j = 0; j < 4; j++) d[k][pl][j] = fmaxf(fmaxf(col[pl][j], col[pl][j + 1]), col[pl][j + 2]);
          const float lo = fminf(fminf(d[k][pl][0], d[k][pl][1]), fminf(d[k][pl][2], d[k][pl][3]));
          const float hi = fmaxf(fmaxf(d[k][pl][0], d[k][pl][1]), fmaxf(d[k][pl][2], d[k][pl][3]));
          if (pl < 3) {
            mn0 = fminf(mn0, lo);
            mx0 = fmaxf(mx0, hi);
          } else {
            mn1 = fminf(mn1, lo);
            mx1 = fmaxf(mx1, hi);
          }
        }
      }
    }
    // createNormalsImage: the three planes are normalised as ONE 3-channel image; createDepthImage on its own
    // (image_strategy.cpp:144-153, 178-187; Image1ChannelsStrategy is the depth plane alone)
    if (64 * (tid >> 6) < n_live) {  // (a wave without a live group holds the initial values in every lane)
      mn0 = wave_min_f32(mn0);
      mx0 = wave_max_f32(mx0);
      mn1 = wave_min_f32(mn1);
      mx1 = wave_max_f32(mx1);
    }
    if (lane == 0) {
      S.red_f[4 * (tid >> 6) + 0] = mn0;
      S.red_f[4 * (tid >> 6) + 1] = mx0;
      S.red_f[4 * (tid >> 6) + 2] = mn1;
      S.red_f[4 * (tid >> 6) + 3] = mx1;
    }
    __syncthreads();
    float fs[2], fb[2];
    uint32_t bg[2];
    auto to_byte = [](float x, float s, float b) {  // cv::normalize + convertTo(CV_8U, 255.0)
      const float v = x * s + b;
      const float u = v * 255.0f + 0.0f;
      float t = rintf(u);
      t = t < 0.f ? 0.f : (t > 255.f ? 255.f : t);
      return (uint32_t)(int)t;
    };
#pragma unroll
    for (int q = 0; q < 2; q++) {
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
      bg[q] = to_byte(0.f, fs[q], fb[q]) * 0x01010101u;  // four background pixels: the value 0 through the same arithmetic
    }
    // The bytes are staged in LDS — the index raster is dead after the barrier above: 4 planes x 900 dwords in MEMORY order
    // (image row = 59 - cell row, image_strategy.cpp:128-129) — and leave as 16-byte stores, 15 per wave instead of 56
    // four-byte ones (the store phase was issue bound: 36 of the 158 us a projection costs, profiles/img_phases.sh).
    uint32_t *stage = S.cells;
    uint4 *stage4 = reinterpret_cast<uint4 *>(S.cells);
    // Every group is staged exactly once, so the staging is ONE phase ("fill everything with background, barrier, the
    // live groups over it" before): a thread stages the background of its OWN groups tid + k * IMG_THREADS that it found
    // without points when it listed the live ones ...
#pragma unroll
    for (int k = 0; k < GPT; k++) {
      const int g = tid + k * IMG_THREADS;
      if (g < 900 && !live[k]) {
        const int r = g / 15, cg = g - r * 15;
        const int m = (kImg - 1 - r) * 15 + cg;
#pragma unroll
        for (int pl = 0; pl < 4; pl++) stage[pl * 900 + m] = bg[pl < 3 ? 0 : 1];
      }
    }
#pragma unroll
    for (int k = 0; k < GPT; k++) {  // ... and the live groups of the list that it has dilated
      const int a = tid + k * IMG_THREADS;
      if (a < n_live) {
        const int g = (int)alist[a];
        const int r = g / 15, cg = g - r * 15;
        const int m = (kImg - 1 - r) * 15 + cg;
#pragma unroll
        for (int pl = 0; pl < 4; pl++) {
          const int q = pl < 3 ? 0 : 1;
          uint32_t packed = 0;
#pragma unroll
          for (int j = 0; j < 4; j++) packed |= to_byte(d[k][pl][j], fs[q], fb[q]) << (8 * j);
          stage[pl * 900 + m] = packed;
        }
      }
    }
    __syncthreads();
    for (int a = tid; a < 900; a += IMG_THREADS) {
      const int pl = a / 225, j = a - pl * 225;
      const uint4 v = stage4[a];
      stage4[a] = make_uint4(0u, 0u, 0u, 0u);  // the cell counters of the next projection start from zero
      if (pl < 3 ? !with_normals : !with_depth) continue;
      const int ch = K.C == 1 ? 0 : pr * K.per + pl;
      *reinterpret_cast<uint4 *>(out + (size_t)ch * kPix + 16 * j) = v;
    }
    __syncthreads();
    TICK(8);
  }
  if (tid == 0 && S.flag && (!BIG || item_pr == 0)) atomicOr(P.status, S.flag);
}

template <bool BIG>
__global__ __launch_bounds__(IMG_THREADS, BIG ? 2 : 4) void grasp_image_kernel(ImgParams P) {
  __shared__ SmemPts<BIG> S;
  if constexpr (BIG) {
    // the unit of the walk is one projection of one queued candidate: a queue of ten is thirty workgroups' work, not ten
    // workgroups' of three projections in a row (59 -> 30 us alone on the chip for the benchmark's ten; beside the shadow
    // kernel a workgroup waits for a CU with this much LDS free, whichever way the queue is cut: profiles/NOTES.md N)
    const int np = c_img.nproj;
    const int items = *P.cand_count * np;
    for (int it = blockIdx.x; it < items; it += gridDim.x) {
      __syncthreads();  // the previous item's LDS is dead
      const int q = it / np;
      grasp_image_body<true>(P, S, P.cand_list[q], it - q * np);
    }
  } else {
    const int cand = xcd_candidate(P.num_cand);
    if (cand < 0) return;
    grasp_image_body<false>(P, S, cand);
  }
}

// ---------------------------------------------------------------------------
// shadow_set_kernel: HandSet::calculateShadow / calculateShadowForCamera (hand_set.cpp:118-233)
// for one camera, once per hand set.  The 33 * N_i LCG draws of the set (stream offset given by
// the host, hand_set.cpp:263-266) are voxelised into a bitset over the cube of +-43 voxels around
// the sample, which contains every image box of the set; the candidates then cut their boxes
// out of it.
// ---------------------------------------------------------------------------
struct SetParams {
  const float *nn;
  int cap;
  const double *centers;
  const double *frames;     // [S][12], sample first
  const int32_t *set_meta;  // [bitsets][8]: sample slot, N_images, lcg offset lo, hi, camera, -
  uint32_t *set_bits;       // [sets][Vox::SETWORDS]
  const gpd_hand *hands;    // [S][slots] records of the search ...
  const int32_t *hand_cand; // ... and which of them are candidates (>= 0): the default mode writes only the part of a set's
  int slots;                //     region its candidates' boxes can touch
  unsigned long long lcg_base;  // draws consumed before this call's first hand set (gpd_hip_detect_sharded; else 0)
  double view_point[3 * kMaxCams];  // of the cloud (a kernel argument, not a device constant: clouds of a batch
                                    // with different cameras run side by side)
};

// MODE 0: the default region (86^3 bits, built in LDS, written out once); 1: WIDE (128^3 bits = 256 KB: straight into the
// set's global row, which the host has cleared); 2: a region of run-time size (c_img.set_sd), also straight into global memory —
// image volumes of any size the general shadow kernel below takes
// (MODE 0 is held to the 64 registers at which two workgroups — their bitsets fill the LDS between them — share a CU: eight waves per SIMD)
// JIT (gpd_hip_set_shadow_jitter): the bitsets hold the un-moved voxels all the same — the set semantics and the intersection
// over cameras are on voxels (hand_set.cpp:159-183) — but a candidate sees the voxels whose MOVED points lie in its box, so the
// windows MODE 0 cuts its work to are the widened ones, by the arithmetic of the reader: that is MODE 3, MODE 0 in everything
// else.  MODES 1 and 2 fill their whole region and serve both settings.
template <int MODE_>
__global__ __launch_bounds__(SET_THREADS, (MODE_ == 0 || MODE_ == 3) ? 8 : 1) void shadow_set_kernel(SetParams P) {
  constexpr bool JIT = MODE_ == 3;
  constexpr int MODE = JIT ? 0 : MODE_;
  constexpr bool WIDE = MODE != 0;
  const ImgConsts &K = c_img;
  const int SD = MODE == 2 ? K.set_sd : Vox<MODE == 1>::SD, SR = MODE == 2 ? K.set_sr : Vox<MODE == 1>::SR;
  const int SETWORDS = MODE == 2 ? (int)(((long long)SD * SD * SD + 31) / 32) : Vox<MODE == 1>::SETWORDS;
  __shared__ uint32_t lds_bits[WIDE ? 1 : Vox<false>::SETWORDS];
  __shared__ int s_bb[6];  // MODE 0: x0, x1, y0, y1, z0, z1 of the candidates' windows, in region voxels
  const int set = blockIdx.x;
  const int tid = threadIdx.x;
  const int slot_s = P.set_meta[8 * set + 0];
  const int N = P.set_meta[8 * set + 1];
  // position in the cloud's ONE stream of shadow draws (hand_set.cpp:268-283): the plan's offset among this call's hand sets
  // + the draws of the sample ranges before it, when the cloud's samples are sharded over several contexts
  const unsigned long long off =
      P.lcg_base + (((unsigned long long)(uint32_t)P.set_meta[8 * set + 3] << 32) | (uint32_t)P.set_meta[8 * set + 2]);
  const int cam = P.set_meta[8 * set + 4];
  const float *nn = P.nn + (size_t)slot_s * 6 * P.cap;
  uint32_t *out = P.set_bits + (size_t)set * SETWORDS;
  uint32_t *bits = WIDE ? out : lds_bits;
  if (!WIDE) {
    if (tid == 0) {
      s_bb[0] = s_bb[2] = s_bb[4] = SD;
      s_bb[1] = s_bb[3] = s_bb[5] = -1;
    }
    for (int w = tid; w < SETWORDS; w += SET_THREADS) lds_bits[w] = 0u;
    __syncthreads();
  }
  const double *smp = P.frames + 12 * (size_t)slot_s;
  const int org[3] = {(int)floor(smp[0] * K.voxel_mult) - SR, (int)floor(smp[1] * K.voxel_mult) - SR,
                      (int)floor(smp[2] * K.voxel_mult) - SR};
  if (!WIDE) {
    // The voxel bounding box of the windows shadow_image_kernel opens for the set's candidates, floor(min) - 1 ..
    // floor(max) + 1 per axis (the arithmetic of shadow_image_body's S.vorg / v1, the jitter's margin included), here relative to the region.  Nothing
    // outside it is ever read with effect: only its rows are written out below, and a bit survives a reader only through
    // the exact box test of its voxel.  So the rays are tested against it BEFORE they are drawn.
    if (tid < P.slots && P.hand_cand[(size_t)slot_s * P.slots + tid] >= 0) {
      const gpd_hand &H = P.hands[(size_t)slot_s * P.slots + tid];
      const double lo[3] = {H.bottom, H.center - K.half_od, -1.0 * K.vol_height};
      const double hi[3] = {H.bottom + K.vol_depth, H.center + K.half_od, K.vol_height};
      double wmin[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, wmax[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
      for (int k = 0; k < 8; k++) {
        const double bx = (k & 1) ? hi[0] : lo[0], by = (k & 2) ? hi[1] : lo[1], bz = (k & 4) ? hi[2] : lo[2];
        for (int a = 0; a < 3; a++) {
          const double w = H.sample[a] + H.frame[3 * a] * bx + H.frame[3 * a + 1] * by + H.frame[3 * a + 2] * bz;
          wmin[a] = fmin(wmin[a], w);
          wmax[a] = fmax(wmax[a], w);
        }
      }
      if constexpr (JIT) {  // shadow_image_body's AABB, grown by the bound of the shift
        for (int a = 0; a < 3; a++) {
          wmin[a] = wmin[a] - jitter::kShiftBound;
          wmax[a] = wmax[a] + jitter::kShiftBound;
        }
      }
      for (int a = 0; a < 3; a++) {
        atomicMin(&s_bb[2 * a], (int)floor(wmin[a] * K.voxel_mult) - 1 - org[a]);
        atomicMax(&s_bb[2 * a + 1], (int)floor(wmax[a] * K.voxel_mult) + 1 - org[a]);
      }
    }
    __syncthreads();
  }
  // shadow_vec = shadow_length * (center - view_point) / norm (hand_set.cpp:147-150)
  const double *cen = P.centers + 3 * (size_t)slot_s;
  double vec[3];
  for (int r = 0; r < 3; r++) vec[r] = cen[r] - P.view_point[3 * cam + r];
  const double nrm = sqrt(vec[0] * vec[0] + vec[1] * vec[1] + vec[2] * vec[2]);
  for (int r = 0; r < 3; r++) vec[r] = K.shadow_length * vec[r] / nrm;
  uint32_t state = lcg_jump(0u, off + (unsigned long long)tid * (unsigned)K.num_shadow);
  int ox = org[0], oy = org[1], oz = org[2];
  // opaque to the optimiser: it re-associated v - (floor - SR) into (v - floor) + SR, two operations per coordinate and draw
  asm volatile("" : "+v"(ox), "+v"(oy), "+v"(oz));
  // the num_shadow draws of one ray: point p, LCG state st at the ray's first draw
  auto draw_ray = [&](const double p0, const double p1, const double p2, uint32_t st) {
    for (int k = 0; k < K.num_shadow; k++) {
      const double t = (double)(int)lcg_step(st) * K.rand_inv;
      const int vx = (int)((p0 + t * vec[0]) * K.voxel_mult) - ox;
      const int vy = (int)((p1 + t * vec[1]) * K.voxel_mult) - oy;
      const int vz = (int)((p2 + t * vec[2]) * K.voxel_mult) - oz;
      if ((unsigned)vx < (unsigned)SD && (unsigned)vy < (unsigned)SD && (unsigned)vz < (unsigned)SD) {
        // 24-bit multiply-adds, spelled out: the compiler picks v_mad_u64_u32 for a 32-bit multiply-add
        unsigned bit;
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(bit) : "v"(vx), "s"(SD), "v"(vy));
        asm("v_mad_u32_u24 %0, %1, %2, %3" : "=v"(bit) : "v"(bit), "s"(SD), "v"(vz));
        atomicOr(&bits[bit >> 5], 1u << (bit & 31));
      }
    }
  };
  if constexpr (MODE == 0) {
    // ---- Rays that cannot reach the candidates' windows are dropped, the others packed 64 to a wave before they are drawn.
    // A draw sets voxel trunc(y_a) - org_a per axis, y_a = (p_a + t * vec_a) * voxel_mult, and is seen only if that index is
    // in [b0_a, b1_a] (s_bb clamped to the region), for which y_a must lie in (b0_a + org_a - 1, b1_a + org_a + 1) whichever
    // way the conversion truncates.  The test takes one voxel more on either side, W_a = [b0_a + org_a - 2, b1_a + org_a + 2],
    // against q_a + t * d_a with q = p * voxel_mult, d = vec * voxel_mult: that differs from y_a by rounding alone, ~1e-13
    // voxels for coordinates of metres, and so do the ends of the parameter interval (an error e in t moves the point by
    // e * d_a = ~1e-16 * |W_a - q_a|) — the spare voxel is 1e13 times that, no rounding question arises.
    // The parameter: lcg_step returns ((int32)s >> 16) & 0x7fff, an integer 0 .. 32767; rand_inv = RN(1 / 32767), so
    // t = (int)lcg_step(st) * rand_inv takes 32768 values from 0 to RN(32767 * RN(1 / 32767)), which is 1 to within an ulp:
    // the range tested is [0, 1], the ulp again ~1e-15 voxels.
    // An axis whose |d_a| < 1e-9 voxels (a ray parallel to the slab; d_a == 0 exactly when the view point lies on a coordinate
    // axis through the centre) is not divided by: the point moves < 1e-9 voxels along it, so it is in the slab W_a or not.
    double wlo[3], whi[3], dinv[3];
    bool par[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      // s_bb clamped to the region (no candidate: b0 > b1 + 4, every ray misses)
      const int b0 = max(s_bb[2 * a], 0), b1 = min(s_bb[2 * a + 1], SD - 1);
      wlo[a] = (double)(b0 + org[a] - 2);
      whi[a] = (double)(b1 + org[a] + 2);
      const double d = vec[a] * K.voxel_mult;
      par[a] = !(fabs(d) >= 1e-9);
      dinv[a] = par[a] ? 0.0 : 1.0 / d;
    }
    // The survivors of successive rounds gather in registers: `pend` of them wait in lanes 0 .. pend - 1 of the wave (pend
    // < 64, the same in every lane).  A round's lanes are permuted as a whole — its k survivors, in lane order, to lanes
    // pend, pend + 1, ... (mod 64), the others behind them — so that one ds_permute per register moves them (no LDS memory:
    // the two resident workgroups leave none).  When 64 have gathered they are drawn with every lane live; what is left
    // at the end is drawn once more.  The draws are OR-ed into the bitset, so their order is free, and a ray's LCG state
    // depends on its index alone: a dropped ray costs nothing else.
    const int lane = tid & 63;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0;  // the gathered rays
    uint32_t gs = 0u;
    int pend = 0;
    for (int base = 0; base < N; base += SET_THREADS) {
      const int i = base + tid, ic = i < N ? i : N - 1;
      const double p0 = (double)nn[0 * P.cap + ic], p1 = (double)nn[1 * P.cap + ic], p2 = (double)nn[2 * P.cap + ic];
      const double pp[3] = {p0, p1, p2};
      bool keep = i < N;
      double t0 = 0.0, t1 = 1.0;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const double q = pp[a] * K.voxel_mult;
        if (par[a]) {
          keep = keep && q >= wlo[a] && q <= whi[a];
        } else {
          const double ta = (wlo[a] - q) * dinv[a], tb = (whi[a] - q) * dinv[a];
          t0 = fmax(t0, fmin(ta, tb));
          t1 = fmin(t1, fmax(ta, tb));
        }
      }
      keep = keep && t0 <= t1;
      const unsigned long long ballot = __ballot(keep);
      const int k = __popcll(ballot);
      if (k) {  // (the same in every lane of the wave)
        const int below = __popcll(ballot & ((1ull << lane) - 1ull));
        const int dest = ((keep ? pend + below : pend + k + (lane - below)) & 63) << 2;
        auto move = [dest](const double x) {
          return __hiloint2double(__builtin_amdgcn_ds_permute(dest, __double2hiint(x)),
                                  __builtin_amdgcn_ds_permute(dest, __double2loint(x)));
        };
        const double a0 = move(p0), a1 = move(p1), a2 = move(p2);
        const uint32_t as = (uint32_t)__builtin_amdgcn_ds_permute(dest, (int)state);
        const bool arrived = ((lane - pend) & 63) < k;  // this lane received one of the round's survivors
        if (pend + k < 64) {
          if (arrived) g0 = a0, g1 = a1, g2 = a2, gs = as;
          pend += k;
        } else {
          if (lane >= pend) g0 = a0, g1 = a1, g2 = a2, gs = as;  // (all of them have: k >= 64 - pend)
          draw_ray(g0, g1, g2, gs);
          pend += k - 64;
          if (lane < pend) g0 = a0, g1 = a1, g2 = a2, gs = as;  // the survivors that wrapped round
        }
      }
      state = K.stride_a * state + K.stride_c;  // advance by SET_THREADS * num_shadow draws
    }
    if (lane < pend) draw_ray(g0, g1, g2, gs);
  } else {
    for (int i = tid; i < N; i += SET_THREADS) {
      draw_ray((double)nn[0 * P.cap + i], (double)nn[1 * P.cap + i], (double)nn[2 * P.cap + i], state);
      state = K.stride_a * state + K.stride_c;  // advance by SET_THREADS * num_shadow draws
    }
  }
  if (!WIDE) {
    // Written out: only the rows (lines along z) inside the x-y footprint of that bounding box — shadow_image_kernel reads
    // the rows of a candidate's window and keeps the bits its box test passes, and no bit outside a box passes it, so
    // whatever an earlier launch left in the rest of the row is never seen (129 MB of bitsets per 5000 candidates were
    // written in full before: half of the image stage's excess HBM traffic).
    __syncthreads();
    const int x0 = max(s_bb[0], 0), x1 = min(s_bb[1], SD - 1), y0 = max(s_bb[2], 0), y1 = min(s_bb[3], SD - 1);
    if (x1 >= x0 && y1 >= y0) {
      const int wpr = (((y1 - y0 + 1) * SD + 31) >> 5) + 1;  // words one x-slab's rows can span
      for (int idx = tid; idx < (x1 - x0 + 1) * wpr; idx += SET_THREADS) {
        const int x = x0 + idx / wpr, k = idx - (idx / wpr) * wpr;
        const int first = (x * SD + y0) * SD, last = (x * SD + y1 + 1) * SD - 1;  // the slab's bits
        const int w = (first >> 5) + k;
        if (w <= (last >> 5)) out[w] = lds_bits[w];
      }
    }
  }
}

// planar [n][C][3600] <-> HWC [n][3600][C] (cv::Mat CV_8UC(C), the reference's image layout)
__global__ void planar_to_hwc_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int C, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t per = (size_t)kPix * C;
  const size_t img = i / per, r = i - img * per;
  const int pix = (int)(r / C), c = (int)(r - (size_t)pix * C);
  dst[i] = src[img * per + (size_t)c * kPix + pix];
}
__global__ void hwc_to_planar_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, int C, size_t total) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const size_t per = (size_t)kPix * C;
  const size_t img = i / per, r = i - img * per;
  const int c = (int)(r / kPix), pix = (int)(r - (size_t)c * kPix);
  dst[i] = src[img * per + (size_t)pix * C + c];
}
hipError_t planar_to_hwc(const uint8_t *src, uint8_t *dst, int n, int C, hipStream_t stream) {
  const size_t total = (size_t)n * kPix * C;
  if (!total) return hipSuccess;
  planar_to_hwc_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(src, dst, C, total);
  return hipGetLastError();
}
hipError_t hwc_to_planar(const uint8_t *src, uint8_t *dst, int n, int C, hipStream_t stream) {
  const size_t total = (size_t)n * kPix * C;
  if (!total) return hipSuccess;
  hwc_to_planar_kernel<<<(unsigned)((total + 255) / 256), 256, 0, stream>>>(src, dst, C, total);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Host side: one enqueue per kernel, under the lock of c_img (const_block.h).
// ---------------------------------------------------------------------------
static ConstBlock g_img_block;

// Where a kernel lands in the code object is decided by the order in which this unit first uses the instantiations.  The
// three kernels of the default path run side by side and share the instruction caches, so the instantiations that existed
// before the shadow jitter keep the order they had, and with it their distances to one another: they are named here first
// (a function nobody calls), in the order images_launch used to reach them, and the kernels of the jitter behind them.
// (The image stage moves by about 1 % with where the same instructions lie: DESIGN.md §15, profiles/shadow_jitter_ab.json.)
[[maybe_unused]] static void kernel_order() {
  static const void *const order[] = {
      (const void *)grasp_image_kernel<false>,
      (const void *)grasp_image_kernel<true>,
      (const void *)shadow_set_kernel<2>,
      (const void *)shadow_set_kernel<1>,
      (const void *)shadow_set_kernel<0>,
      (const void *)shadow_image_kernel<SH_CAP, true>,
      (const void *)shadow_image_kernel<SH_CAP_BIG, true>,
      (const void *)shadow_image_kernel<SH_CAP, false>,
      (const void *)shadow_image_kernel<SH_CAP_BIG, false>,
      (const void *)shadow_set_kernel<3>,
      (const void *)shadow_image_any_jitter_kernel<true>,
      (const void *)shadow_image_jitter_kernel<SH_CAP, true>,
      (const void *)shadow_image_jitter_kernel<SH_CAP_BIG, true>,
      (const void *)shadow_image_jitter_kernel<SH_CAP, false>,
      (const void *)shadow_image_jitter_kernel<SH_CAP_BIG, false>,
  };
  (void)order;
}

// what every image kernel reads: the search's lists and records, the plan's candidate list, the images and the status
// word; the queues, overflow targets and scratch rows of one launch alone are off
static ImgParams img_params(const SearchState &s, const Plan &pl, const ImageState &im, unsigned long long *dbg) {
  ImgParams ip;
  std::memset(&ip, 0, sizeof(ip));
  ip.nn = s.d_nn;
  ip.cap = s.nn_cap;
  ip.centers = s.d_centers;
  ip.hands = s.d_hands;
  ip.cand_hand = pl.d_cand_hand;
  ip.meta = pl.d_cand_meta;
  ip.set_bits = im.d_set_bits;
  ip.images = im.d_images;
  ip.status = im.d_status;
  ip.num_cand = im.num_candidates;
  ip.dbg = dbg;
  ip.exit_after = prof_env("GPD_IMG_EXIT") ? atoi(prof_env("GPD_IMG_EXIT")) : 0;
  return ip;
}

// Launches the image kernels over the candidate list resident on the device.  Nothing here waits for the
// device: the large instantiations read the length of their queues on the device, capacity flags
// accumulate in im.d_status (read by the caller with its results).
int images_launch(const SearchState &s, const Plan &pl, ImageState &im, hipStream_t stream, bool counters_clean) {
  const int n = im.num_candidates;
  if (n <= 0) return GPD_OK;
  // the three overflow counters of the launch (the flags in d_status[0] accumulate over re-launches)
  if (!counters_clean) HIP_RET(hipMemsetAsync(im.d_status + 1, 0, 3 * sizeof(int32_t), stream));
  if (im.consts.size() != sizeof(ImgConsts)) return GPD_ERR_STATE;
  std::unique_lock<std::mutex> consts_lock;  // held until every kernel below is enqueued
  {
    const int rc = g_img_block.load(c_img, im.consts.data(), sizeof(ImgConsts), stream, consts_lock);
    if (rc) return rc;
  }
  static unsigned long long *d_dbg = nullptr;
  unsigned long long *dbg = nullptr;
  if (prof_env("GPD_IMG_TIMING")) {
    if (!d_dbg) HIP_RET(hipMalloc(&d_dbg, 32 * sizeof(unsigned long long)));
    HIP_RET(hipMemsetAsync(d_dbg, 0, 32 * sizeof(unsigned long long), stream));
    dbg = d_dbg;
  }
  const ImgParams base = img_params(s, pl, im, dbg);
  // the three queues of the stage: list and length (a counter of d_status), filled by one kernel and walked by the next
  int32_t *const pts_queue = im.d_pts_overflow, *const pts_queued = im.d_status + 3;  // more than PT_CAP in-box points
  int32_t *const sh_queue = im.d_overflow, *const sh_queued = im.d_status + 1;        // more than SH_CAP voxels in the box
  int32_t *const any_queue = im.d_overflow2, *const any_queued = im.d_status + 2;     // more than SH_CAP_BIG (wide windows only)
  const unsigned all = 8 * ((n + 7) / 8);  // grid of the kernels that take every candidate (xcd_candidate)
  // the shadow jitter of the block the list was built with: a compile-time parameter of the shadow kernels
  const bool jit = reinterpret_cast<const ImgConsts *>(im.consts.data())->jitter != 0;
  if (!im.aux) {
    HIP_RET(hipStreamCreate(&im.aux));
    HIP_RET(hipEventCreateWithFlags(&im.ev_fork, hipEventDisableTiming));
    HIP_RET(hipEventCreateWithFlags(&im.ev_join, hipEventDisableTiming));
  }
  static const bool serial = prof_env("GPD_IMG_SERIAL") != nullptr;  // profiling aid: each image kernel alone on the chip
  // profiling aid: unused dynamic LDS per workgroup of the two per-candidate kernels (8192: one workgroup per CU instead of two)
  static const size_t lds_pad = prof_env("GPD_IMG_LDS_PAD") ? (size_t)atoi(prof_env("GPD_IMG_LDS_PAD")) : 0;
  // normals + depth on the side stream (15 channels: beside the shadow kernels)
  hipStream_t pts_stream = (im.channels == 15 && !dbg && im.side_stream && !serial) ? im.aux : stream;
  if (pts_stream != stream) {
    HIP_RET(hipEventRecord(im.ev_fork, stream));
    HIP_RET(hipStreamWaitEvent(pts_stream, im.ev_fork, 0));
  }
  {  // every candidate.  Nearly every box holds fewer than PT_CAP points; the others are queued ...
    ImgParams ip = base;
    ip.pts_overflow_list = pts_queue;
    ip.pts_overflow_count = pts_queued;
    grasp_image_kernel<false><<<all, IMG_THREADS, lds_pad, pts_stream>>>(ip);
    HIP_RET(hipGetLastError());
  }
  {  // ... and redone by the instantiation that keeps its point arrays in a global scratch row
    ImgParams ip = base;
    ip.cand_list = pts_queue;
    ip.cand_count = pts_queued;
    ip.pts_scratch = im.d_pts_scratch;
    grasp_image_kernel<true><<<LGRID, IMG_THREADS, 0, pts_stream>>>(ip);
    HIP_RET(hipGetLastError());
  }
  if (im.num_shadow_sets > 0) {
    SetParams sp;
    sp.nn = s.d_nn;
    sp.cap = s.nn_cap;
    sp.centers = s.d_centers;
    sp.frames = s.d_frames;
    sp.set_meta = pl.d_set_meta;
    sp.set_bits = im.d_set_bits;
    sp.hands = s.d_hands;
    sp.hand_cand = pl.d_hand_cand;
    sp.slots = im.slots;
    sp.lcg_base = im.lcg_base;
    std::memcpy(sp.view_point, im.view_points, sizeof(sp.view_point));
    if (im.huge) {
      const size_t setwords = (size_t)(((long long)im.set_sd * im.set_sd * im.set_sd + 31) / 32);
      HIP_RET(hipMemsetAsync(im.d_set_bits, 0, (size_t)im.num_shadow_sets * setwords * sizeof(uint32_t), stream));
      shadow_set_kernel<2><<<im.num_shadow_sets, SET_THREADS, 0, stream>>>(sp);
    } else if (im.wide) {
      HIP_RET(hipMemsetAsync(im.d_set_bits, 0, (size_t)im.num_shadow_sets * Vox<true>::SETWORDS * sizeof(uint32_t), stream));
      shadow_set_kernel<1><<<im.num_shadow_sets, SET_THREADS, 0, stream>>>(sp);
    } else {
      if (jit)
        shadow_set_kernel<3><<<im.num_shadow_sets, SET_THREADS, 0, stream>>>(sp);
      else
        shadow_set_kernel<0><<<im.num_shadow_sets, SET_THREADS, 0, stream>>>(sp);
    }
    HIP_RET(hipGetLastError());
  }
  if (im.channels == 15 && im.huge) {
    // an image volume beyond the windows of the tuned kernels: every candidate through the general one
    ImgParams ip = base;
    ip.huge_scratch = im.d_huge_scratch;
    if (jit)
      shadow_image_any_jitter_kernel<true><<<LGRID, IMG_THREADS, 0, stream>>>(ip);
    else
      shadow_image_any_kernel<<<LGRID, IMG_THREADS, 0, stream>>>(ip);
    HIP_RET(hipGetLastError());
  } else if (im.channels == 15 && im.wide) {
    {  // every candidate; the boxes with more than SH_CAP voxels are queued ...
      ImgParams ip = base;
      ip.overflow_list = sh_queue;
      ip.overflow_count = sh_queued;
      if (jit)
        shadow_image_jitter_kernel<SH_CAP, true><<<all, IMG_THREADS, 0, stream>>>(ip);
      else
        shadow_image_kernel<SH_CAP, true><<<all, IMG_THREADS, 0, stream>>>(ip);
      HIP_RET(hipGetLastError());
    }
    {  // ... for the large instantiation; a wide box can hold more voxels than that one lists: it queues those ...
      ImgParams ip = base;
      ip.cand_list = sh_queue;
      ip.cand_count = sh_queued;
      ip.overflow_list = any_queue;
      ip.overflow_count = any_queued;
      if (jit)
        shadow_image_jitter_kernel<SH_CAP_BIG, true><<<LGRID, IMG_THREADS, 0, stream>>>(ip);
      else
        shadow_image_kernel<SH_CAP_BIG, true><<<LGRID, IMG_THREADS, 0, stream>>>(ip);
      HIP_RET(hipGetLastError());
    }
    {  // ... for the general kernel
      ImgParams ip = base;
      ip.cand_list = any_queue;
      ip.cand_count = any_queued;
      ip.huge_scratch = im.d_huge_scratch;
      if (jit)
        shadow_image_any_jitter_kernel<true><<<LGRID, IMG_THREADS, 0, stream>>>(ip);
      else
        shadow_image_any_kernel<<<LGRID, IMG_THREADS, 0, stream>>>(ip);
      HIP_RET(hipGetLastError());
    }
  } else if (im.channels == 15) {
    {  // every candidate.  Most boxes fit the two-per-CU instantiation; the few that do not are queued by it ...
      ImgParams ip = base;
      ip.overflow_list = sh_queue;
      ip.overflow_count = sh_queued;
      if (jit)
        shadow_image_jitter_kernel<SH_CAP, false><<<all, IMG_THREADS, lds_pad, stream>>>(ip);
      else
        shadow_image_kernel<SH_CAP, false><<<all, IMG_THREADS, lds_pad, stream>>>(ip);
      HIP_RET(hipGetLastError());
    }
    {  // ... and redone by the large one (the default box holds fewer voxel cells than it lists: no further queue)
      ImgParams ip = base;
      ip.cand_list = sh_queue;
      ip.cand_count = sh_queued;
      if (jit)
        shadow_image_jitter_kernel<SH_CAP_BIG, false><<<LGRID, IMG_THREADS, 0, stream>>>(ip);
      else
        shadow_image_kernel<SH_CAP_BIG, false><<<LGRID, IMG_THREADS, 0, stream>>>(ip);
      HIP_RET(hipGetLastError());
    }
  }
  HIP_RET(hipEventRecord(im.ev_join, pts_stream));
  if (pts_stream != stream) HIP_RET(hipStreamWaitEvent(stream, im.ev_join, 0));
  if (dbg) {
    unsigned long long h[32];
    HIP_RET(hipMemcpyAsync(h, d_dbg, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_RET(hipStreamSynchronize(stream));
    // sh_sort_list / pts_sort_list: count, scan, segment table AND the list of non-empty pixels (one run of phases since the
    // list is built inside the scan); sh_nnz_read / pts_nnz_read: the read of its length behind the barrier (slots 9 / 11
    // held the list's three phases); sh_max_read: the read of the walk's maxima; pts_setup: nothing but address
    // arithmetic (it held the barrier of the live-group counter)
    static const char *names[14] = {"sh_extract",  "sh_list",       "sh_sort_list",  "sh_max_read", "sh_final",
                                    "pts_collect", "pts_sort_list", "pts_walk_tail", "pts_final",   "sh_nnz_read",
                                    "sh_walk_loop", "pts_nnz_read", "pts_setup",     "pts_walk_loop"};
    unsigned long long tot = 0;
    for (int i = 0; i < 14; i++) tot += h[i];
    for (int i = 0; i < 14; i++)
      fprintf(stderr, "[img-timing] %-16s %10.1f kcycles/cand  %5.1f%%\n", names[i], (double)h[i] / n / 1e3,
              100.0 * h[i] / (double)tot);
    fprintf(stderr, "[img-timing] shadow voxels in box: max %llu mean %.0f; in-box points: max %llu mean %.0f\n", h[28],
            (double)h[29] / n, h[30], (double)h[31] / n);
  }
  return GPD_OK;
}

}  // namespace gpd
