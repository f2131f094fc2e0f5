// Host state of the image stage: the buffers of an ImageState, the window class and the constant block of a geometry
// (image_model.h) and what the tests read back.  No kernel is defined or launched here: images_run ends in
// images_launch (images.hip, the stage's one device unit).
#include <cstdio>
#include <cstring>

#include <vector>

#include "gpd_internal.h"
#include "buffers.h"
#include "image_model.h"

namespace gpd {

void images_free(ImageState &im) {
  device_release(im.d_images, im.d_images_hwc, im.d_status, im.d_set_bits, im.d_overflow, im.d_overflow2, im.d_pts_overflow, im.d_pts_scratch, im.d_huge_scratch);
  if (im.ev_fork) (void)hipEventDestroy(im.ev_fork);
  if (im.ev_join) (void)hipEventDestroy(im.ev_join);
  if (im.aux) (void)hipStreamDestroy(im.aux);
  im = ImageState();
}

// Image buffers for up to n candidates and `shadow_sets` (live hand set, camera) voxel bitsets of the geometry in p
// (grow with 25 % slack, never shrink; a growth stalls the device).
int images_reserve(const gpd_params &p, ImageState &im, int n, int shadow_sets) {
  const int C = p.image_num_channels;
  if (!im.d_status) {
    HIP_RET(device_alloc(im.d_status, 4));  // [0] flags, [1..3] the counters of the three overflow lists: ONE memset per launch
    HIP_RET(hipMemset(im.d_status, 0, 4 * sizeof(int32_t)));
    HIP_RET(device_alloc(im.d_pts_scratch, (size_t)LGRID * PTS_SCRATCH_BYTES));
  }
  if (n > im.capacity) {
    note_alloc(__func__);
    device_release(im.d_images, im.d_images_hwc, im.d_overflow, im.d_overflow2, im.d_pts_overflow);
    im.capacity = 0;
    const int cap = slack_cap(n, 4);  // slack: the clouds of a batch differ a little
    HIP_RET(device_alloc(im.d_images, (size_t)cap * kPix * C));
    HIP_RET(device_alloc(im.d_overflow, (size_t)cap));  // list (its counter: d_status[1])
    HIP_RET(device_alloc(im.d_overflow2, (size_t)cap));  // ... of the large instantiation, for the general kernel
    HIP_RET(device_alloc(im.d_pts_overflow, (size_t)cap));
    im.capacity = cap;
  }
  {
    // which voxel windows the shadow kernels need
    image::Window w;
    char msg[160];
    // (the shadow jitter widens them; it is a setting of the shadow channel, so of 15 channels alone)
    const int rc = image::window_class(p, im.jitter && C == 15, w, msg, sizeof(msg));
    im.wide = w.wide;
    im.huge = w.huge;
    if (rc) {
      set_error("%s", msg);
      return rc;
    }
    im.set_sr = w.set_sr;
    im.set_sd = w.set_sd;
  }
  const size_t setwords = (size_t)(((long long)im.set_sd * im.set_sd * im.set_sd + 31) / 32);
  if (C == 15 && (shadow_sets > im.cap_shadow_sets || setwords > im.cap_setwords)) {
    note_alloc(__func__);
    device_release(im.d_set_bits);
    im.cap_shadow_sets = 0;
    const int want = shadow_sets > im.cap_shadow_sets ? shadow_sets : im.cap_shadow_sets;
    const int cap = slack_cap(want, 4);
    const size_t words = setwords > im.cap_setwords ? setwords : im.cap_setwords;
    HIP_RET(device_alloc(im.d_set_bits, (size_t)cap * words));
    // defined contents from the first launch on: shadow_set_kernel<0> writes only the rows its candidates' windows cover, and
    // the words around them keep what is there (zero, or an earlier launch's voxels — see the reader's note in shadow_image_kernel)
    HIP_RET(hipMemset(im.d_set_bits, 0, (size_t)cap * words * sizeof(uint32_t)));
    im.cap_shadow_sets = cap;
    im.cap_setwords = words;  // (a larger row also serves the smaller regions)
  }
  if (C == 15 && (im.wide || im.huge) && !im.d_huge_scratch) {
    // the general shadow kernel's list rows, one per workgroup of its persistent grid; the default geometry cannot reach it
    // (its box holds fewer voxel cells than the large instantiation lists)
    note_alloc(__func__);
    HIP_RET(device_alloc(im.d_huge_scratch, (size_t)LGRID * HUGE_SCRATCH_BYTES));
  }
  return GPD_OK;
}

// The buffers and the constant block of the list in `im` (num_candidates, num_shadow_sets) under the state's present settings:
// what images_run does ahead of its launch, and what a switch of the shadow jitter does to a resident list, so that a
// re-launch (gpd_hip_replay) never reads buffers or a block of the other setting.  The caller has waited for the lane.
int images_prepare(const gpd_params &p, ImageState &im) {
  {
    const int rc = images_reserve(p, im, im.num_candidates, im.num_shadow_sets);
    if (rc) return rc;
  }
  ImgConsts k;
  {
    image::Window w;
    w.wide = im.wide;
    w.huge = im.huge;
    w.set_sd = im.set_sd;
    w.set_sr = im.set_sr;
    image::fill_consts(p, w, im.jitter, im.jitter_seed, k);
  }
  const unsigned char *kb = reinterpret_cast<const unsigned char *>(&k);
  if (im.consts.size() != sizeof(k) || std::memcmp(im.consts.data(), kb, sizeof(k)) != 0) im.consts.assign(kb, kb + sizeof(k));
  return GPD_OK;
}

// The candidate list itself (which hands, in which order, where each hand set starts in the LCG stream) is
// built on the device by plan_kernel; its sizes are in pl.h_summary by now.  This sizes the image buffers,
// prepares the constant block of the image geometry and launches the kernels.
int images_run(const gpd_params &p, const Cloud &c, const SearchState &s, const Plan &pl, ImageState &im, hipStream_t stream) {
  const int C = p.image_num_channels;
  const PlanSummary &sm = *pl.h_summary;
  const int n = sm.num_candidates;
  im.num_candidates = n;
  im.channels = C;
  im.slots = p.num_hand_axes * p.num_orientations;
  im.stat_sets = sm.live_sets;
  im.stat_sum_set_ni = sm.sum_set_ni;
  im.stat_sum_cand_ni = sm.sum_cand_ni;
  im.num_shadow_sets = sm.num_shadow_sets;
  std::memcpy(im.view_points, c.view_points, sizeof(im.view_points));
  {
    const int rc = images_prepare(p, im);
    if (rc) return rc;
  }
  HIP_RET(hipMemsetAsync(im.d_status, 0, 4 * sizeof(int32_t), stream));  // the flags and the overflow counters of this launch
  if (n == 0) return GPD_OK;
  return images_launch(s, pl, im, stream, /*counters_clean=*/true);
}

// text of the capacity flags an image kernel left in d_status
void images_status_text(int status, char *buf, size_t len) {
  snprintf(buf, len, "images: kernel capacity exceeded (flags %d: 1 image box beyond %d voxels of window edge, 2 in-box points > %d, "
           "4 shadow voxels in a box > %d)", status, HUGE_WIN, PT_CAP_BIG, HUGE_CAP);
}

// The routes of the last launch from the three queues images_launch hands the kernels (d_overflow / d_status[1],
// d_overflow2 / [2], d_pts_overflow / [3]); the caller has waited for the lane's stream.
int images_routes(const ImageState &im, int32_t *route, long long info[8]) {
  const int n = im.num_candidates;
  info[0] = n;
  info[1] = im.huge ? 2 : (im.wide ? 1 : 0);
  info[2] = (n > 0 && im.num_shadow_sets > 0) ? (int)info[1] : -1;  // images_launch's condition for shadow_set_kernel
  info[3] = 0;
  info[4] = PT_CAP;
  info[5] = PT_CAP_BIG;
  info[6] = SH_CAP;
  info[7] = SH_CAP_BIG;
  if (n <= 0 || !im.d_status) return GPD_OK;
  std::memset(route, 0, (size_t)n * sizeof(int32_t));
  int32_t st[4];
  HIP_RET(hipMemcpy(st, im.d_status, sizeof(st), hipMemcpyDeviceToHost));
  info[3] = st[0];
  const int32_t *lists[3] = {im.d_overflow, im.d_overflow2, im.d_pts_overflow};
  const int bits[3] = {1, 2, 4};
  std::vector<int32_t> h;
  for (int l = 0; l < 3; l++) {
    const int cnt = st[1 + l];
    if (cnt == 0) continue;
    if (cnt < 0 || cnt > n || !lists[l]) {
      set_error("gpd_hip_last_image_routes: queue %d holds %d entries for %d candidates", l + 1, cnt, n);
      return GPD_ERR_STATE;
    }
    h.resize((size_t)cnt);
    HIP_RET(hipMemcpy(h.data(), lists[l], (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < cnt; i++) {
      if (h[i] < 0 || h[i] >= n || (route[h[i]] & bits[l])) {
        set_error("gpd_hip_last_image_routes: queue %d entry %d is %d (candidates: %d, or queued twice)", l + 1, i, h[i], n);
        return GPD_ERR_STATE;
      }
      route[h[i]] |= bits[l];
    }
  }
  return GPD_OK;
}

}  // namespace gpd

// The image model of a geometry, host only (include/gpd_hip.h)
static int image_model_of(const char *who, const gpd_params *params, int shadow_jitter, gpd_image_model *out) {
  using namespace gpd;
  if (!params || !out || (shadow_jitter != 0 && shadow_jitter != 1)) {
    set_error("%s: bad argument", who);
    return GPD_ERR_INVALID;
  }
  image::Window w;
  char msg[160];
  const int rc = image::window_class(*params, shadow_jitter, w, msg, sizeof(msg));
  if (rc) {
    set_error("%s", msg);
    return rc;
  }
  ImgConsts k;
  image::fill_consts(*params, w, shadow_jitter, 0ull, k);
  static_assert(sizeof(out->thr) == sizeof(k.thr), "gpd_image_model");
  out->window_class = w.cls();
  out->set_sd = k.set_sd;
  out->set_sr = k.set_sr;
  out->num_shadow = k.num_shadow;
  out->stride_a = k.stride_a;
  out->stride_c = k.stride_c;
  out->true_div = k.true_div;
  out->reserved_ = 0;
  std::memcpy(out->thr, k.thr, sizeof(k.thr));
  return GPD_OK;
}
extern "C" int gpd_hip_image_model(const gpd_params *params, gpd_image_model *out) {
  return image_model_of("gpd_hip_image_model", params, 0, out);
}
// ... with the windows of the given shadow-jitter setting (the geometry's own, whatever its channel count)
extern "C" int gpd_hip_image_model_jitter(const gpd_params *params, int shadow_jitter, gpd_image_model *out) {
  return image_model_of("gpd_hip_image_model_jitter", params, shadow_jitter, out);
}

// g of jitter_model.h for n voxels [n][3], host only
extern "C" int gpd_hip_shadow_jitter_model(uint64_t seed, const int32_t *voxels, int n, double *g) {
  using namespace gpd;
  if (!voxels || !g || n < 0) {
    set_error("gpd_hip_shadow_jitter_model: bad argument");
    return GPD_ERR_INVALID;
  }
  for (int i = 0; i < n; i++) g[i] = jitter::draw(seed, voxels[3 * (size_t)i], voxels[3 * (size_t)i + 1], voxels[3 * (size_t)i + 2]);
  return GPD_OK;
}
