// The host arithmetic of the image stage: the capacities and voxel windows of its kernels, which window class an image
// volume needs, and the constant block (ImgConsts) the kernels read — the exact cell thresholds, the self-check of the
// division by a constant, the LCG jump of the shadow draws.  Plain C++ with no HIP in it, compiled without FMA contraction:
// image_state.hip (images_reserve, images_run), the kernels of images.hip (the caps, Vox, ImgConsts, lcg_affine) and
// gpd_hip_image_model (host only, for the tests) are this code.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>

#include "../../include/gpd_hip.h"
#include "jitter_model.h"

namespace gpd {

constexpr int kImgCells = 60;  // cells per image edge (gpd_internal.h kImg; image_device.h holds the two together)

constexpr int SET_THREADS = 1024;  // shadow_set_kernel
constexpr int PT_CAP = 1024;  // in-box points per candidate on the two-per-CU instantiation (mean ~380 on the 3 mm benchmark clouds; entry
                              // indices are packed into 11 bits of the segment words); fuller boxes go to the large instantiation
constexpr int PT_CAP_BIG = 32768;  // fallback instantiation of the points kernel: storage in a global scratch row (its segment table, 64 KB, is what fills the CU's LDS)
constexpr int SH_CAP = 6144;      // in-box shadow voxels per candidate (two workgroups per CU)
constexpr int SH_CAP_BIG = 12288;  // fallback instantiation, one workgroup per CU
// Voxel windows of the shadow kernels.  Default geometry (image box diagonal 0.1233 m, every box of a hand set within
// 0.1233 m of the sample): a 46^3 window per candidate and an 86^3 region per set, the latter an LDS bitset.  WIDE — picked
// on the host for image volumes that do not fit those (image::window_class: up to ~0.18 m of box diagonal / 0.19 m of reach, e.g.
// volume_width 0.16): 64^3 / 128^3, the set region filled with global-memory atomics (256 KB per set and camera).  The
// reference has no such limits (hand_set.cpp:138); beyond WIDE the kernels still report GPD_ERR_CAPACITY.
template <bool WIDE>
struct Vox {
  static constexpr int VD = WIDE ? 64 : 46;   // candidate window edge (a window row = VD bits along world z, one 64-bit word)
  static constexpr int SD = WIDE ? 128 : 86;  // set region edge: offsets -SR .. SD - SR - 1 from the sample's voxel
  static constexpr int SR = WIDE ? 64 : 43;   // (default: 41.1 voxels of reach -> 42 whole ones, one more on the low side;
                                              //  86^3 bits = 79.5 KB: two shadow_set workgroups per CU)
  static constexpr int LB = 18;               // bits of a voxel position inside the window: iz | iy << 6 | ix << 12 (ascending = lexicographic)
  static constexpr int SETWORDS = (SD * SD * SD + 31) / 32;
};
// LGRID workgroups of the large instantiations walk the queue of the small one; the queue length is read
// on the device, so the host enqueues them without waiting for it (an empty queue costs an empty launch)
constexpr int LGRID = 256;
// scratch row of the points kernel's fallback instantiation: three doubles, a float4 and the 32-bit neighbour index per in-box point
constexpr size_t PTS_SCRATCH_BYTES = (size_t)PT_CAP_BIG * (3 * sizeof(double) + 4 * sizeof(float) + sizeof(uint32_t));
// the general shadow kernel (shadow_image_any_kernel)
constexpr int HUGE_CAP = 65535;       // in-box voxels (segment starts are 16 bits wide in the pixel table)
constexpr int HUGE_WIN = 256;         // window edge in voxels
constexpr size_t HUGE_SCRATCH_BYTES = (size_t)HUGE_WIN * HUGE_WIN * sizeof(int32_t) + (size_t)(HUGE_CAP + 1) * (2 * sizeof(uint32_t) + sizeof(uint16_t)) + 64;

struct ImgConsts {
  double vol_depth, vol_width, vol_height, half_od, dbl_h;
  int C, nproj, per;
  double shadow_length, voxel, voxel_mult, rand_inv;
  int num_shadow;
  uint32_t stride_a, stride_c;  // LCG jump by SET_THREADS * num_shadow draws
  double len[3];                // box extent per hand axis: vol_depth, vol_width, dbl_h
  double inv_cell[3];           // approximate cells per metre (first guess only)
  double thr[3][kImgCells + 1];  // thr[a][k] = smallest x with floor((x/len[a])/(1/60)) >= k
  double inv_len[3];            // RN(1/len[a]) for the division by a constant below
  int true_div;                 // 1: the host self-check of div_len failed for these extents, divide for real
  int set_sd, set_sr;           // edge / radius of the voxel region shadow_set_kernel fills around a sample: 86 / 43, 128 / 64 (WIDE) or,
                                // for image volumes beyond those windows, whatever the geometry needs (image::window_class)
  int jitter;                   // gpd_hip_set_shadow_jitter: 1 = the shadow points are moved off the lattice (jitter_model.h) ...
  unsigned long long jitter_seed;  // ... by the draws of this seed
};

namespace image {

// n steps of HandSet::fastrand's recurrence s -> 214013 s + 2531011 (mod 2^32; hand_set.cpp:263-266) as ONE affine map
// s -> a s + c, by squaring.  constexpr: plain C++ here, callable from device code as it stands (shadow_set_kernel's jump-ahead).
struct LcgMap {
  uint32_t a, c;
};
constexpr LcgMap lcg_affine(unsigned long long n) {
  uint32_t a = 214013u, c = 2531011u, A = 1u, Cc = 0u;
  while (n) {
    if (n & 1ull) {
      A = a * A;
      Cc = a * Cc + c;
    }
    c = (a + 1u) * c;
    a = a * a;
    n >>= 1;
  }
  return LcgMap{A, Cc};
}

// Which voxel windows the shadow kernels need (Vox<WIDE>): the window of a candidate must hold the diagonal of the
// image box (+ 3 voxels of margins), the region of a set every box of the set.  A box spans x in [bottom, bottom + depth]
// with init_bite - hand_depth <= bottom <= 0, y in center -+ width / 2 with |center| <= (outer_diameter - finger_width) / 2,
// |z| <= height (finger_hand.cpp:155-168, image_strategy.cpp:53-70).
// With the shadow jitter on, a voxel's point lies up to jitter::kShiftBound (under two voxels) from its lattice position: a
// candidate's window must hold every voxel whose MOVED point can lie in the box, a set's region likewise — two more voxels on
// each side of the window, two more of reach.  (The default window has one voxel to spare at the stock geometry: jitter
// there means the wide windows.)
struct Window {
  bool wide = false;           // the wide windows, or ...
  bool huge = false;           // ... beyond those: the general shadow kernel, a set region of the size this geometry needs
  int set_sd = 0, set_sr = 0;  // edge / radius (voxels) of the region shadow_set_kernel fills around a sample
  int cls() const { return huge ? 2 : (wide ? 1 : 0); }
};
// GPD_OK, or GPD_ERR_CAPACITY with its text in msg
inline int window_class(const gpd_params &p, int jitter, Window &w, char *msg, size_t msg_len) {
  const double vox = 0.003;
  const double diag = std::sqrt(p.volume_depth * p.volume_depth + p.volume_width * p.volume_width + 4.0 * p.volume_height * p.volume_height);
  const double rx = std::fmax(p.hand_depth - p.init_bite, p.volume_depth);
  const double ry = 0.5 * (p.hand_outer_diameter - p.finger_width) + 0.5 * p.volume_width;
  const double reach = std::sqrt(rx * rx + ry * ry + p.volume_height * p.volume_height);
  const double more = jitter ? (double)jitter::kShiftVoxels : 0.0;
  const double need_win = std::ceil(diag / vox) + 3.0 + 2.0 * more, need_reach = std::ceil(reach / vox) + 1.0 + more;
  w.wide = need_win > (double)Vox<false>::VD || need_reach > (double)(Vox<false>::SR - 1);
  // beyond the wide windows as well: the general shadow kernel with a set region of the size this geometry needs
  // (the reference has no limit, hand_set.cpp:138; what is left of ours: 256 voxels = 0.77 m of window edge, 65535 voxels in a box)
  w.huge = need_win > (double)Vox<true>::VD || need_reach > (double)(Vox<true>::SR - 1);
  if (w.huge) {
    if (need_reach + 2.0 > 640.0) {  // 1280^3 bits = 262 MB per hand set and camera: an image volume of metres is a mistake, not a gripper
      snprintf(msg, msg_len, "images: an image volume with %.2f m of reach is beyond the shadow region this library allocates", reach);
      return GPD_ERR_CAPACITY;
    }
    w.set_sr = (int)need_reach + 2;
    w.set_sd = 2 * w.set_sr;
  } else {
    w.set_sr = w.wide ? Vox<true>::SR : Vox<false>::SR;
    w.set_sd = w.wide ? Vox<true>::SD : Vox<false>::SD;
  }
  return GPD_OK;
}

// smallest positive double x with floor((x/len)/(1.0/60)) >= k — the exact image of the
// reference's cell formula (image_strategy.cpp:92-102 applied to transformPointsToUnitImage's
// quotient, :72-90), found by bisection on the bit pattern with the same IEEE operations.
inline double cell_threshold(double len, int k) {
  const double cellsize = 1.0 / (double)kImgCells;
  auto f = [&](double x) { return std::floor((x / len) / cellsize) >= (double)k; };
  uint64_t lo = 0, hi;  // f(bits lo) false, f(bits hi) true
  double top = len * 2.0;
  std::memcpy(&hi, &top, sizeof(hi));
  while (hi - lo > 1) {
    const uint64_t mid = lo + (hi - lo) / 2;
    double x;
    std::memcpy(&x, &mid, sizeof(x));
    if (f(x))
      hi = mid;
    else
      lo = mid;
  }
  double x;
  std::memcpy(&x, &hi, sizeof(x));
  return x;
}
inline void cell_thresholds(double len, double *out) {  // 61 doubles
  out[0] = 0.0;
  for (int k = 1; k < kImgCells; k++) out[k] = cell_threshold(len, k);
  out[kImgCells] = DBL_MAX;
}

// What the kernels need per box extent: the thresholds, RN(1/len) and whether div_len()'s FMA sequence (Markstein:
// q = x*y, r = x - len*q, q' = q + r*y) reproduces the IEEE quotient x / len.
struct Axis {
  double len = -1.0, thr[kImgCells + 1], inv_len = 0.0;
  int true_div = 0;
};
inline void axis_model(double len, Axis &ac) {
  ac.len = len;
  cell_thresholds(len, ac.thr);
  ac.inv_len = 1.0 / len;
  ac.true_div = 0;
  // self-check of div_len(): the FMA sequence must reproduce the IEEE quotient
  uint64_t rs = 88172645463325252ull;
  for (int i = 0; i < 200000 && !ac.true_div; i++) {
    rs ^= rs << 13;
    rs ^= rs >> 7;
    rs ^= rs << 17;
    double x = (double)(rs >> 11) * (1.0 / 9007199254740992.0) * len;
    if (i & 1) x = (double)(float)x;
    if (i < kImgCells) x = ac.thr[i];
    const double q = x * ac.inv_len;
    const double r = std::fma(-len, q, x);
    if (std::fma(r, ac.inv_len, q) != x / len) ac.true_div = 1;
  }
}

// The constant block of the geometry in p with the windows w (every byte defined: the block is compared bytewise).  The shadow
// jitter and its seed matter to 15 channels alone: without a shadow channel the block is the one of jitter off.
inline void fill_consts(const gpd_params &p, const Window &w, int jitter, unsigned long long jitter_seed, ImgConsts &k) {
  const int C = p.image_num_channels;
  std::memset(&k, 0, sizeof(k));
  k.vol_depth = p.volume_depth;
  k.vol_width = p.volume_width;
  k.vol_height = p.volume_height;
  k.half_od = p.volume_width / 2.0;
  k.dbl_h = 2.0 * p.volume_height;
  k.C = C;
  k.nproj = (C <= 3) ? 1 : 3;
  k.per = (C == 15) ? 5 : (C == 12 ? 4 : C);
  // shadow_length_ = max(volume_depth, volume_height/2, volume_width) (image_15_channels_strategy.h:70-75)
  k.shadow_length = std::fmax(std::fmax(p.volume_depth, p.volume_height / 2.0), p.volume_width);
  k.voxel = 0.003;
  k.voxel_mult = 1.0 / 0.003;
  k.rand_inv = 1.0 / 32767.0;
  k.num_shadow = (int)std::floor(k.shadow_length / k.voxel);  // plan_kernel places the sets in the LCG stream with the same count
  k.len[0] = k.vol_depth;
  k.len[1] = k.vol_width;
  k.len[2] = k.dbl_h;
  k.true_div = 0;
  k.set_sd = w.set_sd;
  k.set_sr = w.set_sr;
  k.jitter = (jitter && C == 15) ? 1 : 0;
  k.jitter_seed = k.jitter ? jitter_seed : 0ull;
  {
    // thresholds and the div_len() self-check depend on the box extents only: computed once per
    // geometry (the self-check alone is ~2 ms of host time)
    static Axis cache[3];
    static std::mutex cache_mutex;
    std::lock_guard<std::mutex> lock(cache_mutex);
    for (int a = 0; a < 3; a++) {
      Axis &ac = cache[a];
      if (ac.len != k.len[a]) axis_model(k.len[a], ac);
      k.inv_cell[a] = (double)kImgCells / k.len[a];
      std::memcpy(k.thr[a], ac.thr, sizeof(ac.thr));
      k.inv_len[a] = ac.inv_len;
      if (ac.true_div) k.true_div = 1;
    }
  }
  // shadow_set_kernel's threads advance by SET_THREADS * num_shadow draws
  const LcgMap stride = lcg_affine((unsigned long long)SET_THREADS * (unsigned)k.num_shadow);
  k.stride_a = stride.a;
  k.stride_c = stride.c;
}

}  // namespace image
}  // namespace gpd
