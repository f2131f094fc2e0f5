// C-ABI of libgpd_hip.so (include/gpd_hip.h): the context and its lanes, the refusals and the lane stages every entry is built
// from, the LeNet setters, uploads and the single-stage entries.  The fused detect is detect.hip, the round-loop entries rounds.hip,
// the batch / multi-context / sharded entries batch.hip, bench.py's measurement hooks replay.hip; context.h is what they share.
//
// A context owns two LANES — each a HIP stream with its own cloud, search buffers, candidate plan,
// image buffers and LeNet scratch.  Every single-cloud entry point runs on lane 0.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "context.h"
#include "buffers.h"
#include "balance_model.h"
#include "outlier_model.h"
#include "sample_model.h"
#include "sis_model.h"

namespace gpd {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

const char *error_text() { return g_err; }
void error_text_set(const char *text) { snprintf(g_err, sizeof(g_err), "%s", text); }
void set_images_status_error(int status) { images_status_text(status, g_err, sizeof(g_err)); }

static thread_local int g_allocs = 0;
void note_alloc(const char *where) {
  g_allocs++;
  if (prof_env("GPD_ALLOC_TRACE")) fprintf(stderr, "[alloc] %s\n", where);  // (profiling build only)
}
int allocs_now() { return g_allocs; }

double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

void ctx_device_stream(gpd_hip_ctx *ctx, int *device, hipStream_t *stream) {
  *device = ctx->device;
  *stream = ctx->lane[0].stream;
}

int lane_init(Lane &L, hipStream_t shared) {
  if (L.stream) return GPD_OK;
  if (shared) {
    L.stream = shared;
  } else {
    HIP_RET(hipStreamCreate(&L.stream));
    L.owns_stream = true;
  }
  for (auto &e : L.ev) HIP_RET(hipEventCreate(&e));
  HIP_RET(hipEventCreate(&L.ev_plan));
  HIP_RET(hipEventCreate(&L.ev_done));
  for (auto &e : L.ev_chunk) HIP_RET(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  HIP_RET(pinned_alloc(L.h_flags, 1));
  std::memset(L.h_flags, 0, sizeof(HostFlags));
  return GPD_OK;
}

static void lane_free(Lane &L) {
  if (L.stream) (void)hipStreamSynchronize(L.stream);
  lenet_scratch_free(L.lenet_scratch);
  preprocess_free(L.pre);
  for (auto &e : L.pre.ev)
    if (e) (void)hipEventDestroy(e);
  if (L.pre.ev_keys) (void)hipEventDestroy(L.pre.ev_keys);
  cloud_free(L.cloud);
  search_free(L.search);
  plan_free(L.plan);
  images_free(L.images);
  plane_free(L.plane);
  refine_free(L.refine);
  outlier_free(L.outliers);
  pinned_release(L.h_pos);
  device_release(L.d_scores, L.d_out, L.d_sel, L.d_all, L.d_img_in, L.d_img_planar, L.d_pos);
  pinned_release(L.h_out, L.h_flags);
  for (auto &e : L.ev)
    if (e) (void)hipEventDestroy(e);
  if (L.ev_plan) (void)hipEventDestroy(L.ev_plan);
  if (L.ev_done) (void)hipEventDestroy(L.ev_done);
  for (auto &e : L.ev_chunk)
    if (e) (void)hipEventDestroy(e);
  if (L.stream && L.owns_stream) (void)hipStreamDestroy(L.stream);
  L = Lane();
}

int reserve_scores(Lane &L, int n) { return grow_device(L.d_scores, L.d_scores_cap, n, slack_cap(n, 4), __func__); }

int reserve_out(Lane &L, size_t records, size_t extra_bytes) {
  const int rc = grow_device(L.d_out, L.d_out_cap, records, slack_cap(records, 4), __func__);
  if (rc) return rc;
  const size_t bytes = L.d_out_cap * sizeof(gpd_hand) + extra_bytes;
  return grow_pinned(L.h_out, L.h_out_bytes, bytes, slack_cap(bytes, 8), __func__);
}

// the draw positions of up to n samples and the sample indices that come back
int reserve_draws(Lane &L, int n) {
  if (n <= L.draw_cap) return GPD_OK;
  note_alloc(__func__);
  device_release(L.d_pos);
  pinned_release(L.h_pos);
  L.draw_cap = 0;
  const int cap = slack_cap(n, 4);
  HIP_RET(device_alloc(L.d_pos, (size_t)cap));
  HIP_RET(pinned_alloc(L.h_pos, (size_t)cap * 3));
  L.draw_cap = cap;
  return GPD_OK;
}

// selections (num_selected > 0): the winners' ordinals + tie flag, and the job's own list of every scored candidate
int reserve_selection(Lane &L, int k, int n) {
  const int rc = grow_device(L.d_sel, L.d_sel_cap, k + 1, slack_cap(k, 4) + 1, __func__);  // (the slack is a quarter of k, not of k + 1)
  if (rc) return rc;
  return grow_device(L.d_all, L.d_all_cap, (size_t)n, slack_cap((size_t)n, 4), __func__);
}

// the most candidates `samples` samples can give (every slot a valid hand), cut to what `budget` bytes hold: per candidate
// its image, the LeNet scratch of both scoring modes (pool1, the f32 and the three-plane bf16 flatten, ip1 and its four K
// quarters), score and records; per (hand set, camera) a shadow voxel bitset of the 86^3-bit default window (wider image
// volumes take more: images_reserve grows them on demand).  With a network of the general route installed (`net`) a candidate
// costs that network's scratch (LeNetNet::scratch_per_image, of the mode in force: gpd_hip_set_lenet_net_mode) and its score instead of the stock scratch, which lane_reserve
// then sizes for one image.
int candidate_bound(const gpd_params &p, int samples, int cams, size_t budget, const LeNetNet *net) {
  const long long upper = (long long)samples * p.num_hand_axes * p.num_orientations;
  const size_t scratch = net && net->active ? (size_t)net->scratch_per_image + sizeof(float)
                                            : (20 * 784 + kFc1In + 5 * kFc1Out + 1) * sizeof(float) + 3 * (size_t)kLenetXld * 2;
  const size_t per = (size_t)kPix * p.image_num_channels + scratch + 2 * sizeof(gpd_hand);
  const size_t bitsets = p.image_num_channels == 15 ? (size_t)std::max(samples, 1) * std::max(cams, 1) * ((86 * 86 * 86 + 31) / 32 * 4) : 0;
  const long long fit = budget > bitsets ? (long long)((budget - bitsets) / per) : 0;
  return (int)std::max(1ll, std::min(upper, fit));
}

int lane_reserve(gpd_hip_ctx *ctx, Lane &L, int points, int cams, int samples, int candidates, int selected) {
  const gpd_params &p = ctx->params;
  const int slots = p.num_hand_axes * p.num_orientations;
  int rc = cloud_reserve(L.cloud, points, cams);
  if (!rc) rc = cloud_reserve_grid(L.cloud, 1 << 20);  // 2 cm cells of a scene up to ~8 m^3 (8 MB); a larger one grows the tables
  if (!rc && samples > 0) rc = search_reserve_samples(L.search, samples, slots);
  if (!rc && samples > 0) rc = plan_reserve(L.plan, L.search.capacity_samples, slots, cams, L.stream);
  if (rc || candidates <= 0) return rc;
  const long long sets = std::min((long long)samples, (long long)candidates) * cams;  // (live hand set, camera) voxel bitsets
  rc = images_reserve(p, L.images, candidates, p.image_num_channels == 15 ? (int)sets : 0);
  if (rc) return rc;
  const LeNetNet &net = ctx->lenet.net;
  if (net.active) {
    // the general route scores in its own scratch; of the stock one it needs the launch error word alone (lenet_net_forward).
    // The stock scratch first: when it grows it releases the general one with it (lenet_scratch_free)
    HIP_RET(lenet_scratch_reserve(L.lenet_scratch, 1));
    HIP_RET(lenet_net_scratch_reserve(net, L.lenet_scratch.net, std::min(candidates, net.chunk)));
  } else {
    HIP_RET(lenet_scratch_reserve(L.lenet_scratch, std::min(candidates, kLeNetChunk)));
  }
  rc = reserve_scores(L, candidates);
  if (rc) return rc;
  if (selected >= 0) {
    const int k = selected > 0 ? std::min(selected, candidates) : candidates;
    rc = reserve_out(L, (size_t)k, selected > 0 ? (size_t)candidates * sizeof(float) : 0);
    if (!rc && selected > 0) rc = reserve_selection(L, k, candidates);
  } else {
    rc = reserve_out(L, (size_t)samples * slots, 0);  // gpd_hip_detect: every slot of every set
  }
  return rc;
}

int check_samples(const char *who, const int32_t *sample_indices, const double *sample_xyz, int num_samples, int num_points) {
  if (sample_indices) {
    for (int i = 0; i < num_samples; i++)
      if (sample_indices[i] < 0 || sample_indices[i] >= num_points) {
        set_error("%s: sample index %d out of range", who, sample_indices[i]);
        return GPD_ERR_INVALID;
      }
  } else {
    for (int i = 0; i < 3 * num_samples; i++)
      if (!std::isfinite(sample_xyz[i])) {
        set_error("%s: sample %d is not finite", who, i / 3);
        return GPD_ERR_INVALID;
      }
  }
  return GPD_OK;
}

int refuse(const char *who, const gpd_hip_ctx *ctx, bool args_ok, std::initializer_list<Need> needs) {
  if (!ctx || !args_ok) {
    set_error("%s: bad argument", who);
    return GPD_ERR_INVALID;
  }
  for (Need need : needs) {
    if (need == Need::Cloud && !ctx->lane[0].cloud.num_points)
      set_error("%s: no cloud uploaded", who);
    else if (need == Need::LeNet && !ctx->lenet.channels)
      set_error("%s: LeNet weights not set", who);
    else if (need == Need::NoBatch && ctx->in_batch)
      set_error("%s: gpd_hip_detect_batch is driving the lanes", who);
    else
      continue;
    return GPD_ERR_STATE;
  }
  return GPD_OK;
}

int lane_images(gpd_hip_ctx *ctx, Lane &L, bool side_stream, unsigned long long lcg_base, const char *range, hipEvent_t ev_start,
                hipEvent_t ev_end) {
  if (ev_start) HIP_RET(hipEventRecord(ev_start, L.stream));
  L.images.side_stream = side_stream;
  L.images.lcg_base = lcg_base;
  {
    StageRange r(range);
    const int rc = images_run(ctx->params, L.cloud, L.search, L.plan, L.images, L.stream);
    if (rc) return rc;
  }
  HIP_RET(hipEventRecord(ev_end, L.stream));
  return GPD_OK;
}

int lane_lenet(gpd_hip_ctx *ctx, Lane &L, const uint8_t *d_images, int n, const char *range) {
  if (n <= 0) {
    L.h_flags->lenet = 0;
    return GPD_OK;
  }
  const int rc = reserve_scores(L, n);
  if (rc) return rc;
  {
    StageRange r(range);
    HIP_RET(lenet_forward(ctx->lenet, L.lenet_scratch, d_images, n, L.d_scores, L.stream));
  }
  // the word rides with the call's results: it is read (lane_check) after the wait the call makes for them anyway
  HIP_RET(hipMemcpyAsync(&L.h_flags->lenet, lenet_fault_word(L.lenet_scratch), sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
  return GPD_OK;
}

int lane_check(Lane &L, int32_t image_status, bool scored) {
  if (image_status) {
    set_images_status_error(image_status);
    return GPD_ERR_CAPACITY;
  }
  if (scored && L.h_flags->lenet) {
    const int rc = lenet_check(L.lenet_scratch);  // clears the device word, sets the error text
    return rc ? rc : GPD_ERR_HIP;
  }
  return GPD_OK;
}

int lane_download_images(const gpd_params &p, Lane &L, int n, uint8_t *images, int32_t *cand_index) {
  if (cand_index && n > 0)
    HIP_RET(hipMemcpyAsync(cand_index, L.plan.d_cand_out, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
  if (images && n > 0) {
    // the caller wants cv::Mat-layout pixels: planar -> HWC on the device, then one copy
    const size_t bytes = (size_t)L.images.capacity * kPix * p.image_num_channels;
    if (!L.images.d_images_hwc) HIP_RET(device_alloc(L.images.d_images_hwc, bytes));
    HIP_RET(planar_to_hwc(L.images.d_images, L.images.d_images_hwc, n, p.image_num_channels, L.stream));
    HIP_RET(hipMemcpyAsync(images, L.images.d_images_hwc, (size_t)n * kPix * p.image_num_channels, hipMemcpyDeviceToHost, L.stream));
  }
  return GPD_OK;
}

}  // namespace gpd

using namespace gpd;

extern "C" {

void gpd_hip_default_params(gpd_params *p) {
  std::memset(p, 0, sizeof(*p));
  p->finger_width = 0.01;
  p->hand_outer_diameter = 0.12;
  p->hand_depth = 0.06;
  p->hand_height = 0.02;
  p->init_bite = 0.01;
  p->volume_width = 0.10;
  p->volume_depth = 0.06;
  p->volume_height = 0.02;
  p->nn_radius_frames = 0.01;
  p->friction_coeff = 20.0;
  p->min_aperture = 0.0;
  p->max_aperture = 0.085;
  p->workspace_grasps[0] = -1;
  p->workspace_grasps[1] = 1;
  p->workspace_grasps[2] = -1;
  p->workspace_grasps[3] = 1;
  p->workspace_grasps[4] = -1;
  p->workspace_grasps[5] = 1;
  p->image_size = 60;
  p->image_num_channels = 15;
  p->num_orientations = 8;
  p->num_finger_placements = 10;
  p->num_hand_axes = 1;
  p->hand_axes[0] = 2;
  p->deepen_hand = 1;
  p->min_viable = 6;
  p->filter_approach_direction = 0;  // cfg/eigen_params.cfg:60-62
  p->direction[0] = 1.0;
  p->thresh_rad = 2.0;
}

const char *gpd_hip_last_error(void) { return g_err; }

int gpd_hip_create(int device, const gpd_params *params, gpd_hip_ctx **out) {
  if (!params || !out) {
    set_error("gpd_hip_create: null argument");
    return GPD_ERR_INVALID;
  }
  *out = nullptr;
  const int C = params->image_num_channels;
  if (params->image_size != kImg || (C != 1 && C != 3 && C != 12 && C != 15)) {
    set_error("gpd_hip_create: image_size must be 60 and image_num_channels one of 1/3/12/15");
    return GPD_ERR_INVALID;
  }
  const int slots = params->num_hand_axes * params->num_orientations;
  if (params->num_hand_axes < 1 || params->num_hand_axes > 3 || params->num_orientations < 1 || slots < 1 || slots > GPD_MAX_SLOTS ||
      params->num_finger_placements < 1 || params->num_finger_placements > 16) {
    set_error("gpd_hip_create: unsupported num_hand_axes/num_orientations/num_finger_placements");
    return GPD_ERR_INVALID;
  }
  for (int a = 0; a < params->num_hand_axes; a++)
    if (params->hand_axes[a] < 0 || params->hand_axes[a] > 2) {  // index into the unit axes (hand_set.cpp:52-53)
      set_error("gpd_hip_create: hand_axes[%d] = %d is not one of 0, 1, 2", a, params->hand_axes[a]);
      return GPD_ERR_INVALID;
    }
  {
    // lengths that end up as divisors, box extents and radii
    const double pos[] = {params->finger_width,  params->hand_outer_diameter, params->hand_depth,       params->hand_height,
                          params->init_bite,     params->volume_width,        params->volume_depth,     params->volume_height,
                          params->nn_radius_frames};
    static const char *names[] = {"finger_width", "hand_outer_diameter", "hand_depth",   "hand_height",     "init_bite",
                                  "volume_width", "volume_depth",        "volume_height", "nn_radius_frames"};
    for (size_t i = 0; i < sizeof(pos) / sizeof(pos[0]); i++)
      if (!(pos[i] > 0.0) || !std::isfinite(pos[i])) {
        set_error("gpd_hip_create: %s must be positive and finite", names[i]);
        return GPD_ERR_INVALID;
      }
    const double fin[] = {params->friction_coeff,      params->min_aperture,        params->max_aperture,
                          params->workspace_grasps[0], params->workspace_grasps[1], params->workspace_grasps[2],
                          params->workspace_grasps[3], params->workspace_grasps[4], params->workspace_grasps[5]};
    for (double v : fin)
      if (std::isnan(v)) {
        set_error("gpd_hip_create: NaN in friction_coeff / apertures / workspace_grasps");
        return GPD_ERR_INVALID;
      }
    if (params->filter_approach_direction)
      for (double v : {params->direction[0], params->direction[1], params->direction[2], params->thresh_rad})
        if (!std::isfinite(v)) {
          set_error("gpd_hip_create: direction / thresh_rad must be finite when filter_approach_direction is set");
          return GPD_ERR_INVALID;
        }
    if (!(params->hand_outer_diameter > params->finger_width)) {
      set_error("gpd_hip_create: hand_outer_diameter must exceed finger_width");
      return GPD_ERR_INVALID;
    }
    // deepenHand's steps (finger_hand.cpp:116-121) come from a 128-entry table (fingers up to init_bite + 0.64 m)
    int steps = 0;
    for (double d = params->init_bite + 0.005; d <= params->hand_depth && steps <= 128; d += 0.005) steps++;
    if (params->deepen_hand && steps > 128) {
      set_error("gpd_hip_create: hand_depth %.3f needs more than 128 deepening steps of 5 mm from init_bite %.3f", params->hand_depth,
                params->init_bite);
      return GPD_ERR_CAPACITY;
    }
  }
  int count = 0;
  HIP_RET(hipGetDeviceCount(&count));
  if (device < 0 || device >= count) {
    set_error("gpd_hip_create: device %d out of range (%d devices)", device, count);
    return GPD_ERR_INVALID;
  }
  HIP_RET(hipSetDevice(device));
  gpd_hip_ctx *ctx = new gpd_hip_ctx();
  ctx->device = device;
  ctx->params = *params;
  const int rc = lane_init(ctx->lane[0]);
  if (rc) {
    gpd_hip_destroy(ctx);
    return rc;
  }
  *out = ctx;
  return GPD_OK;
}

void gpd_hip_destroy(gpd_hip_ctx *ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  for (int l = kLanes - 1; l >= 0; l--) lane_free(ctx->lane[l]);
  preprocess_free(ctx->pre);
  cluster_free(ctx->cluster);
  plane_free(ctx->plane);
  refine_free(ctx->refine);
  outlier_free(ctx->outliers);
  label_free(ctx->label);
  sis_free(ctx->sis);
  for (auto &e : ctx->pre.ev)
    if (e) (void)hipEventDestroy(e);
  if (ctx->pre.ev_keys) (void)hipEventDestroy(ctx->pre.ev_keys);
  float **ws[] = {&ctx->lenet.c1w, &ctx->lenet.c1b, &ctx->lenet.c2w, &ctx->lenet.c2b,
                  &ctx->lenet.f1w, &ctx->lenet.f1b, &ctx->lenet.f2w, &ctx->lenet.f2b, &ctx->lenet.c1wp, &ctx->lenet.c2wt};
  for (float **p : ws) device_release(*p);
  lenet_fast_free(ctx->lenet.fast);
  lenet_net_free(ctx->lenet.net);
  for (auto &e : ctx->replay_events) (void)hipEventDestroy(e);
  if (ctx->pipe_stream) {
    (void)hipStreamSynchronize(ctx->pipe_stream);
    (void)hipStreamDestroy(ctx->pipe_stream);
    device_release(ctx->pipe_images[1]);
    for (int b = 0; b < 2; b++) {
      (void)hipEventDestroy(ctx->pipe_filled[b]);
      (void)hipEventDestroy(ctx->pipe_read[b]);
    }
  }
  delete ctx;
}

int gpd_hip_reserve(gpd_hip_ctx *ctx, int max_points, int max_cams, int max_samples, int max_candidates, int max_selected) {
  if (int rc = refuse("gpd_hip_reserve", ctx, max_points >= 1 && max_cams >= 1 && max_cams <= kMaxCams && max_samples >= 0 && max_candidates >= 0 &&
                                                   max_selected >= 0))
    return rc;
  HIP_RET(hipSetDevice(ctx->device));
  const int cand = max_candidates > 0 ? max_candidates : candidate_bound(ctx->params, max_samples, max_cams, kReserveBudget, &ctx->lenet.net);
  for (int l = 0; l < kLanes; l++) {
    int rc = lane_init(ctx->lane[l]);
    if (rc) return rc;
    Lane &L = ctx->lane[l];
    HIP_RET(hipStreamSynchronize(L.stream));
    // lane 0 also serves the single-cloud entries (all slots of all sets back); both serve the batch (candidates / winners)
    if (l == 0) {
      rc = lane_reserve(ctx, L, max_points, max_cams, max_samples, cand, -1);
      if (rc) return rc;
    }
    rc = lane_reserve(ctx, L, max_points, max_cams, max_samples, cand, 0);
    if (!rc && max_selected > 0) rc = lane_reserve(ctx, L, max_points, max_cams, max_samples, cand, max_selected);
    if (rc) return rc;
  }
  return outlier_reserve(ctx->outliers, max_points, max_cams);  // gpd_hip_remove_statistical_outliers on clouds within these sizes
}

int gpd_hip_set_lenet_weights(gpd_hip_ctx *ctx, int channels, const float *conv1_w, const float *conv1_b, const float *conv2_w,
                              const float *conv2_b, const float *ip1_w, const float *ip1_b, const float *ip2_w,
                              const float *ip2_b) {
  if (!ctx || !conv1_w || !conv1_b || !conv2_w || !conv2_b || !ip1_w || !ip1_b || !ip2_w || !ip2_b) {
    set_error("gpd_hip_set_lenet_weights: null argument");
    return GPD_ERR_INVALID;
  }
  if (channels != ctx->params.image_num_channels) {
    set_error("gpd_hip_set_lenet_weights: channels %d != image_num_channels %d", channels, ctx->params.image_num_channels);
    return GPD_ERR_INVALID;
  }
  HIP_RET(hipSetDevice(ctx->device));
  struct Item {
    float **dst;
    const float *src;
    size_t n;
  } items[] = {{&ctx->lenet.c1w, conv1_w, (size_t)20 * channels * 25}, {&ctx->lenet.c1b, conv1_b, 20},
               {&ctx->lenet.c2w, conv2_w, (size_t)50 * 500},          {&ctx->lenet.c2b, conv2_b, 50},
               {&ctx->lenet.f1w, ip1_w, (size_t)kFc1In * kFc1Out},    {&ctx->lenet.f1b, ip1_b, kFc1Out},
               {&ctx->lenet.f2w, ip2_w, (size_t)2 * kFc1Out},         {&ctx->lenet.f2b, ip2_b, 2}};
  // the f32 chain's conv1 drops input windows that are entirely zero; that is exact only for finite weights
  // (inf * 0 would be NaN in the reference's dense GEMM); the split path cuts conv1 / conv2 / ip1 weights into
  // fixed-point digits / bf16 pieces, which are defined for finite numbers
  {
    struct {
      const char *name;
      const float *w;
      size_t n;
    } fin[] = {{"conv1", conv1_w, (size_t)20 * channels * 25}, {"conv2", conv2_w, (size_t)50 * 500}, {"ip1", ip1_w, (size_t)kFc1In * kFc1Out}};
    for (auto &it : fin)
      for (size_t i = 0; i < it.n; i++)
        if (!std::isfinite(it.w[i])) {
          set_error("gpd_hip_set_lenet_weights: %s weight %zu is not finite", it.name, i);
          return GPD_ERR_INVALID;
        }
  }
  for (auto &L : ctx->lane)
    if (L.stream) HIP_RET(hipStreamSynchronize(L.stream));  // no kernel still reads the old weights
  // from here until every upload has succeeded the context holds NO weights: an update that fails half way (out of memory in
  // lenet_fast_prepare, say) leaves scoring calls refused with "LeNet weights not set" instead of launching on freed tables
  ctx->lenet.channels = 0;
  lenet_net_free(ctx->lenet.net);  // back to the stock route (gpd_hip_set_lenet_net)
  for (auto &it : items) {
    device_release(*it.dst);
    HIP_RET(device_alloc(*it.dst, it.n));
    HIP_RET(hipMemcpy(*it.dst, it.src, it.n * sizeof(float), hipMemcpyHostToDevice));
  }
  // device-side layouts of the conv weights (file layout is [filter][k], conv_layer.cpp:35-36):
  // conv1 rows padded from 25 to 28 taps per channel, conv2 k-major
  {
    const int K1 = channels * 25;
    std::vector<float> t1((size_t)20 * channels * 28, 0.f), t2((size_t)500 * 50);
    for (int f = 0; f < 20; f++)
      for (int c = 0; c < channels; c++)
        for (int t = 0; t < 25; t++) t1[((size_t)f * channels + c) * 28 + t] = conv1_w[(size_t)f * K1 + c * 25 + t];
    for (int f = 0; f < 50; f++)
      for (int k = 0; k < 500; k++) t2[(size_t)k * 50 + f] = conv2_w[(size_t)f * 500 + k];
    struct {
      float **dst;
      std::vector<float> *src;
    } tr[] = {{&ctx->lenet.c1wp, &t1}, {&ctx->lenet.c2wt, &t2}};
    for (auto &it : tr) {
      device_release(*it.dst);
      HIP_RET(device_alloc(*it.dst, it.src->size()));
      HIP_RET(hipMemcpy(*it.dst, it.src->data(), it.src->size() * sizeof(float), hipMemcpyHostToDevice));
    }
  }
  HIP_RET(lenet_fast_prepare(ctx->lenet.fast, channels, conv1_w, conv2_w, ip1_w));
  ctx->lenet.channels = channels;
  return GPD_OK;
}

int gpd_hip_set_lenet_mode(gpd_hip_ctx *ctx, int mode) {
  if (int rc = refuse("gpd_hip_set_lenet_mode", ctx, mode == GPD_LENET_SPLIT || mode == GPD_LENET_F32_CHAIN)) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  for (auto &L : ctx->lane)
    if (L.stream) HIP_RET(hipStreamSynchronize(L.stream));  // the two modes lay pool1 out differently: no launch in flight
  ctx->lenet.mode = mode;
  return GPD_OK;
}

// The ReLU after conv1 and conv2 of the reference's PyTorch network (pytorch/network.py: F.relu(conv), then the pool; the Eigen /
// Caffe / OpenVINO network has none).  Context state like the mode: every scoring entry goes through lenet_forward with
// ctx->lenet, which picks the kernels' RELU instantiations at enqueue time; gpd_hip_set_lenet_weights leaves it alone.
int gpd_hip_set_lenet_conv_relu(gpd_hip_ctx *ctx, int on) {
  if (int rc = refuse("gpd_hip_set_lenet_conv_relu", ctx, on == 0 || on == 1)) return rc;
  ctx->lenet.conv_relu = on != 0;
  return GPD_OK;
}

// The seeded per-voxel jitter of the shadow points (jitter_model.h; hand_set.cpp:187-204 draws it from an unseeded generator).
// Context state like the ReLU above: every entry that makes images goes through images_run / images_launch with the lane's
// ImageState, which holds the setting.  A switch can change the window class (image_model.h), so nothing may be in flight, and a
// resident candidate list gets the buffers and the constant block of the new setting here: gpd_hip_replay re-launches under it.
int gpd_hip_set_shadow_jitter(gpd_hip_ctx *ctx, int on, uint64_t seed) {
  if (int rc = refuse("gpd_hip_set_shadow_jitter", ctx, on == 0 || on == 1, {Need::NoBatch})) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  for (auto &L : ctx->lane)
    if (L.stream) HIP_RET(hipStreamSynchronize(L.stream));
  for (auto &L : ctx->lane) {
    ImageState &im = L.images;
    im.jitter = on;
    im.jitter_seed = on ? (unsigned long long)seed : 0ull;
    if (im.num_candidates > 0 && !im.consts.empty()) {
      const int rc = images_prepare(ctx->params, im);
      if (rc) {
        im.num_candidates = 0;  // no list this setting can re-launch
        return rc;
      }
    }
  }
  return GPD_OK;
}

// pytorch/network.py::Net's tensors -> the layouts gpd_hip_set_lenet_weights takes (host only).  conv2 and all biases need no
// conversion: [50][20][5][5] row-major is the reference's [50][500], and a bias is a bias.
//   conv1  [20][C][5][5] is the reference's row-major [20][C*25]; the input scale of the training data (hdf5_dataset.py:17:
//          image * 1/256) is folded in: w * scale, rounded once from double (exact for a power of two)
//   ip1    Net flattens pool2 channel-major (x.view(-1, 50*12*12): k = c * 144 + p) and nn.Linear stores [out][in]; the reference
//          flattens pixel-major (j = p * 50 + c) and stores [in][out] (column-major 500 x 7200)
//   ip2    [2][500] -> [500][2]
int gpd_hip_lenet_from_torch(int channels, double input_scale, const float *conv1_weight, const float *fc1_weight, const float *fc2_weight,
                             float *conv1_w_out, float *ip1_w_out, float *ip2_w_out) {
  if (!conv1_weight || !fc1_weight || !fc2_weight || !conv1_w_out || !ip1_w_out || !ip2_w_out) {
    set_error("gpd_hip_lenet_from_torch: null argument");
    return GPD_ERR_INVALID;
  }
  if (channels != 1 && channels != 3 && channels != 12 && channels != 15) {
    set_error("gpd_hip_lenet_from_torch: channels = %d (1, 3, 12 or 15)", channels);
    return GPD_ERR_INVALID;
  }
  if (!std::isfinite(input_scale) || !(input_scale > 0.0)) {
    set_error("gpd_hip_lenet_from_torch: input_scale must be finite and positive");
    return GPD_ERR_INVALID;
  }
  const size_t n1 = (size_t)20 * channels * 25;
  for (size_t i = 0; i < n1; i++) conv1_w_out[i] = (float)((double)conv1_weight[i] * input_scale);
  for (int p = 0; p < 144; p++)
    for (int c = 0; c < 50; c++) {
      float *dst = ip1_w_out + (size_t)(p * 50 + c) * kFc1Out;
      const float *src = fc1_weight + (size_t)c * 144 + p;
      for (int u = 0; u < kFc1Out; u++) dst[u] = src[(size_t)u * kFc1In];
    }
  for (int j = 0; j < kFc1Out; j++)
    for (int u = 0; u < 2; u++) ip2_w_out[j * 2 + u] = fc2_weight[(size_t)u * kFc1Out + j];
  return GPD_OK;
}

// test hook: the intermediate tensors of lane 0's last LeNet pass (which = 0: pool1 as f32 [n][15680], 1: the three bf16
// planes of the flattened pool2 [3][n][7200] (split path), 2: fc1 transposed f32 [500][n])
int gpd_hip_lenet_debug(gpd_hip_ctx *ctx, int which, int n, void *out) {
  if (int rc = refuse("gpd_hip_lenet_debug", ctx, out && n >= 1)) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  Lane &L = ctx->lane[0];
  LeNetScratch &s = L.lenet_scratch;
  if (n > s.capacity) {
    set_error("gpd_hip_lenet_debug: n = %d exceeds the scratch capacity %d", n, s.capacity);
    return GPD_ERR_STATE;
  }
  HIP_RET(hipStreamSynchronize(L.stream));
  if (which == 0) {
    HIP_RET(hipMemcpy(out, s.pool1, (size_t)n * 15680 * sizeof(float), hipMemcpyDeviceToHost));
  } else if (which == 1) {
    const size_t rows = ((size_t)n + 15) & ~(size_t)15;
    std::vector<unsigned short> blocked(3 * rows * kLenetXld);
    HIP_RET(hipMemcpy(blocked.data(), s.xs, blocked.size() * sizeof(unsigned short), hipMemcpyDeviceToHost));
    lenet_fast_unblock_x(blocked.data(), n, static_cast<unsigned short *>(out));
  } else if (which == 2 && ctx->lenet.mode == GPD_LENET_SPLIT) {
    // the split path keeps ip1's output as four partial sums (they meet inside ip2's kernel): added here as there, in order
    const size_t rows = ((size_t)n + 31) & ~(size_t)31;
    std::vector<float> part(rows * 4 * kFc1Out), b1(kFc1Out);
    HIP_RET(hipMemcpy(part.data(), s.fc1p, part.size() * sizeof(float), hipMemcpyDeviceToHost));
    HIP_RET(hipMemcpy(b1.data(), ctx->lenet.f1b, b1.size() * sizeof(float), hipMemcpyDeviceToHost));
    float *o = static_cast<float *>(out);
    for (int u = 0; u < kFc1Out; u++)
      for (int m = 0; m < n; m++) {
        const float v = ((part[fc1p_index(m, 0, u)] + part[fc1p_index(m, 1, u)]) + part[fc1p_index(m, 2, u)]) + part[fc1p_index(m, 3, u)] + b1[u];
        o[(size_t)u * n + m] = v > 0.f ? v : 0.f;
      }
  } else if (which == 2) {
    HIP_RET(hipMemcpy2D(out, (size_t)n * sizeof(float), s.fc1t, (size_t)s.capacity * sizeof(float), (size_t)n * sizeof(float), kFc1Out,
                        hipMemcpyDeviceToHost));
  } else {
    set_error("gpd_hip_lenet_debug: which = %d", which);
    return GPD_ERR_INVALID;
  }
  return GPD_OK;
}

int gpd_hip_score(gpd_hip_ctx *ctx, const uint8_t *images, int n, float *scores) {
  StageRange range_("gpd:score (classifyImages)");
  int rc = refuse("gpd_hip_score", ctx, scores && n >= 0, {Need::LeNet});
  if (rc || n == 0) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  Lane &L = ctx->lane[0];
  const size_t bytes = (size_t)n * kPix * ctx->lenet.channels;
  const uint8_t *d_img = nullptr;
  if (images) {
    if (bytes > L.d_img_in_bytes) {
      device_release(L.d_img_in);  // (never booked: note_alloc's comment in gpd_internal.h)
      device_release(L.d_img_planar);
      L.d_img_in_bytes = 0;
      HIP_RET(device_alloc(L.d_img_in, bytes));
      HIP_RET(device_alloc(L.d_img_planar, bytes));
      L.d_img_in_bytes = bytes;
    }
    HIP_RET(hipMemcpyAsync(L.d_img_in, images, bytes, hipMemcpyHostToDevice, L.stream));
    HIP_RET(hwc_to_planar(L.d_img_in, L.d_img_planar, n, ctx->lenet.channels, L.stream));
    d_img = L.d_img_planar;
  } else {
    if (n != L.images.num_candidates || !L.images.d_images) {
      set_error("gpd_hip_score: no device images for n=%d (gpd_hip_images produced %d)", n, L.images.num_candidates);
      return GPD_ERR_STATE;
    }
    d_img = L.images.d_images;
  }
  HIP_RET(hipEventRecord(L.ev[2], L.stream));
  rc = lane_lenet(ctx, L, d_img, n, "gpd:lenet (gpd_hip_score)");
  if (rc) return rc;
  HIP_RET(hipEventRecord(L.ev[3], L.stream));
  HIP_RET(hipMemcpyAsync(scores, L.d_scores, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, L.stream));
  HIP_RET(hipStreamSynchronize(L.stream));
  HIP_RET(hipEventElapsedTime(&L.stage_ms[2], L.ev[2], L.ev[3]));
  return lane_check(L, 0, /*scored=*/true);
}

int gpd_hip_upload_cloud(gpd_hip_ctx *ctx, const float *xyz, const float *normals, int num_points, const int32_t *cam_source,
                         int num_cams, const double *view_points) {
  StageRange range_("gpd:upload_cloud (+ uniform grid)");
  if (int rc = refuse("gpd_hip_upload_cloud", ctx, xyz && normals && num_points > 0 && cam_source && num_cams >= 1 && view_points)) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  Lane &L = ctx->lane[0];
  return cloud_upload(L.cloud, xyz, normals, num_points, cam_source, num_cams, view_points, L.stream, /*sync=*/true);
}

int gpd_hip_upload_ground_truth(gpd_hip_ctx *ctx, const float *xyz, const float *normals, int num_points) {
  StageRange range_("gpd:upload_ground_truth (+ uniform grid)");
  if (int rc = refuse("gpd_hip_upload_ground_truth", ctx, num_points >= 0 && (num_points == 0 || (xyz && normals)))) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  Lane &L = ctx->lane[0];
  LabelState &ls = ctx->label;
  if (num_points == 0) {  // cleared: the buffers stay, the next gpd_hip_label_view is refused
    HIP_RET(hipStreamSynchronize(L.stream));
    ls.gt.num_points = 0;
    ls.gt.generation++;
    return GPD_OK;
  }
  const std::vector<int32_t> cam((size_t)num_points, 1);  // reevaluateHypotheses reads no camera: one that sees every point
  const double view_point[3] = {0.0, 0.0, 0.0};
  const int rc = cloud_upload(ls.gt, xyz, normals, num_points, cam.data(), 1, view_point, L.stream, /*sync=*/true);
  if (rc) ls.gt.num_points = 0;
  return rc;
}

int gpd_hip_sizeof_label_view_job(void) { return (int)sizeof(gpd_label_view_job); }

int gpd_hip_balance_view(const uint8_t *labels, int n, int max_grasps_per_view, int32_t *out_index, int *num_out, int *num_positives_out) {
  if (n < 0 || (n > 0 && !labels) || !num_out || !num_positives_out) {
    set_error("gpd_hip_balance_view: bad argument");
    return GPD_ERR_INVALID;
  }
  std::vector<int32_t> keep;
  const int end = balance::view(labels, n, max_grasps_per_view, keep);
  if (end > 0 && !out_index) {
    set_error("gpd_hip_balance_view: bad argument");
    return GPD_ERR_INVALID;
  }
  if (end > 0) std::memcpy(out_index, keep.data(), keep.size() * sizeof(int32_t));
  *num_out = 2 * end;
  *num_positives_out = end;
  return GPD_OK;
}

int gpd_hip_sizeof_sis_job(void) { return (int)sizeof(gpd_sis_job); }

int gpd_hip_sis_proposals(uint32_t seed, int round, int kind, long long first, int count, double sigma, void *out) {
  if (round < 0 || first < 0 || count < 0 || (count > 0 && !out) || (kind != 0 && kind != 1) || (kind == 0 && !(sigma > 0.0))) {
    set_error("gpd_hip_sis_proposals: bad argument");
    return GPD_ERR_INVALID;
  }
  sample::Stream st(sis::stream_seed(seed, round, kind));
  sis::skip(st, (unsigned long long)first * (kind == 0 ? sis::kGaussDraws : 1));
  if (kind == 0) {
    static_assert(sizeof(gpd_sis_proposal) == sizeof(sis::Proposal), "gpd_sis_proposal");
    sis::Proposal *o = static_cast<sis::Proposal *>(out);
    for (int i = 0; i < count; i++) o[i] = sis::next_gauss(st, sigma);
  } else {
    uint64_t *o = static_cast<uint64_t *>(out);
    for (int i = 0; i < count; i++) o[i] = st.next();
  }
  return GPD_OK;
}

int gpd_hip_sis_select(const double *centres, int num_centres, const gpd_sis_proposal *gauss, int num_gauss_proposals,
                       const uint64_t *uniform, int num_uniform_proposals, const int32_t *uniform_list, int num_uniform_list,
                       const float *cloud_xyz, int num_points, const double *workspace, int sampling_method, int num_gauss, int num_rand,
                       double *samples, int32_t *accepted, int32_t *consumed, int *shortfall) {
  if (num_centres < 0 || num_gauss_proposals < 0 || num_uniform_proposals < 0 || num_uniform_list < 0 || num_points < 0 || num_gauss < 0 ||
      num_rand < 0 || !accepted || !consumed || !shortfall || (sampling_method != 0 && sampling_method != 1) ||
      (num_gauss + num_rand > 0 && !samples) || (num_gauss > 0 && (num_centres < 1 || !centres)) || (num_gauss_proposals > 0 && !gauss) ||
      (num_uniform_proposals > 0 && !uniform) || (num_uniform_list > 0 && !uniform_list) ||
      (num_rand > 0 && (!cloud_xyz || !workspace || (num_uniform_list == 0 && num_points < 1)))) {
    set_error("gpd_hip_sis_select: bad argument");
    return GPD_ERR_INVALID;
  }
  for (int i = 0; i < num_uniform_list; i++)
    if (uniform_list[i] < 0 || uniform_list[i] >= num_points) {
      set_error("gpd_hip_sis_select: uniform_list index %d out of range", uniform_list[i]);
      return GPD_ERR_INVALID;
    }
  if (accepted[0] < 0 || accepted[0] > num_gauss || accepted[1] < 0 || accepted[1] > num_rand || consumed[0] < 0 || consumed[1] < 0) {
    set_error("gpd_hip_sis_select: counts that no earlier block left");
    return GPD_ERR_INVALID;
  }
  sis::Counts g = {accepted[0], consumed[0]}, u = {accepted[1], consumed[1]};
  const double none[6] = {0, 0, 0, 0, 0, 0};
  *shortfall = sis::select(centres, num_centres, reinterpret_cast<const sis::Proposal *>(gauss), num_gauss_proposals, uniform,
                           num_uniform_proposals, num_uniform_list > 0 ? uniform_list : nullptr, num_uniform_list, cloud_xyz, num_points,
                           workspace ? workspace : none, sampling_method, num_gauss, num_rand, samples, g, u);
  accepted[0] = g.accepted;
  consumed[0] = g.consumed;
  accepted[1] = u.accepted;
  consumed[1] = u.consumed;
  return GPD_OK;
}

int gpd_hip_shuffle_orders(uint32_t seed, const int32_t *sizes, int num_sets, int32_t *out) {
  if (num_sets < 0 || (num_sets > 0 && !sizes)) {
    set_error("gpd_hip_shuffle_orders: bad argument");
    return GPD_ERR_INVALID;
  }
  for (int s = 0; s < num_sets; s++)
    if (sizes[s] < 0 || (sizes[s] > 0 && !out)) {
      set_error("gpd_hip_shuffle_orders: bad argument");
      return GPD_ERR_INVALID;
    }
  sample::Stream st(seed);
  std::vector<int32_t> order;
  size_t at = 0;
  for (int s = 0; s < num_sets; s++) {
    balance::shuffle_order(sizes[s], st, order);
    if (!order.empty()) std::memcpy(out + at, order.data(), order.size() * sizeof(int32_t));
    at += order.size();
  }
  return GPD_OK;
}

int gpd_hip_find_clusters(gpd_hip_ctx *ctx, const gpd_hand *hands, const double *scores, int n, int min_inliers, int remove_inliers,
                          gpd_hand *out, double *out_scores, int32_t *out_src, int *num_out) {
  StageRange range_("gpd:find_clusters");
  if (int rc = refuse("gpd_hip_find_clusters", ctx, num_out && n >= 0 && (n == 0 || (hands && scores && out && out_scores && out_src)))) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  return cluster_run(ctx->cluster, hands, scores, n, min_inliers, remove_inliers, out, out_scores, out_src, num_out, ctx->lane[0].stream);
}

int gpd_hip_preprocess_cloud(gpd_hip_ctx *ctx, const float *xyz, const int32_t *cam_source, int num_points, int num_cams,
                             const double *workspace, float voxel_size, float *xyz_out, int32_t *cam_out, int32_t *src_out,
                             int *num_out, float *kernel_ms) {
  StageRange range_("gpd:preprocess_cloud (workspace cut, voxeliser)");
  const bool bad = !num_out || num_points < 0 || num_cams < 0 || (num_points > 0 && (!xyz || !xyz_out)) ||
                   (num_points > 0 && num_cams > 0 && (!cam_source || !cam_out)) || !(voxel_size == voxel_size);
  if (int rc = refuse("gpd_hip_preprocess_cloud", ctx, !bad)) return rc;
  if (workspace)
    for (int a = 0; a < 6; a++)
      if (workspace[a] != workspace[a]) {
        set_error("gpd_hip_preprocess_cloud: the workspace holds a NaN");
        return GPD_ERR_INVALID;
      }
  HIP_RET(hipSetDevice(ctx->device));
  return preprocess_run(ctx->pre, xyz, cam_source, num_points, num_cams, workspace, voxel_size, xyz_out, cam_out, src_out, num_out,
                        kernel_ms, ctx->lane[0].stream);
}

int gpd_hip_estimate_normals(gpd_hip_ctx *ctx, double radius, float *normals) {
  StageRange range_("gpd:estimate_normals");
  if (int rc = refuse("gpd_hip_estimate_normals", ctx, normals && radius > 0.0, {Need::Cloud})) return rc;
  Lane &L = ctx->lane[0];
  HIP_RET(hipSetDevice(ctx->device));
  return normals_run(L.cloud, radius, normals, L.stream);
}

int gpd_hip_sample_above_plane(gpd_hip_ctx *ctx, double threshold, int max_iterations, double probability, int optimize,
                                int32_t *indices_out, int *num_out, float coeffs[4], int *num_inliers, int *iterations) {
  if (int rc = refuse("gpd_hip_sample_above_plane", ctx, indices_out && num_out && coeffs && num_inliers && iterations && max_iterations >= 0))
    return rc;
  if (max_iterations >= kPlaneMaxHyp) {
    set_error("gpd_hip_sample_above_plane: max_iterations = %d, the capacity is %d", max_iterations, kPlaneMaxHyp - 1);
    return GPD_ERR_CAPACITY;
  }
  if (int rc = refuse("gpd_hip_sample_above_plane", ctx, true, {Need::Cloud})) return rc;
  Lane &L = ctx->lane[0];
  HIP_RET(hipSetDevice(ctx->device));
  return plane_fit_run(ctx->plane, L.cloud, threshold, max_iterations, probability, optimize, indices_out, num_out, coeffs, num_inliers,
                       iterations, L.stream);
}

int gpd_hip_sample_positions(int n, int num_draws, uint32_t seed, int with_repetition, int32_t *out, int *num_out) {
  if (n < 0 || !num_out || (!out && n > 0 && num_draws > 0)) {
    set_error("gpd_hip_sample_positions: bad argument");
    return GPD_ERR_INVALID;
  }
  std::vector<int32_t> pos;
  if (with_repetition)
    sample::with_repetition(n, num_draws, seed, pos);
  else
    sample::distinct(n, num_draws, seed, pos);
  if (!pos.empty()) std::memcpy(out, pos.data(), pos.size() * sizeof(int32_t));
  *num_out = (int)pos.size();
  return GPD_OK;
}

int gpd_hip_refine_normals(gpd_hip_ctx *ctx, int k, int max_iterations, float convergence_threshold, float *normals_out, int *iterations_out,
                           float *ddot_out, int *num_nan_out, float kernel_ms[3]) {
  if (int rc = refuse("gpd_hip_refine_normals", ctx, normals_out && iterations_out && num_nan_out && k >= 1 && max_iterations >= 0 &&
                                                          std::isfinite(convergence_threshold) && convergence_threshold >= 0.f))
    return rc;
  if (k > kRefineKCap) {
    set_error("gpd_hip_refine_normals: k = %d, the capacity is %d", k, kRefineKCap);
    return GPD_ERR_CAPACITY;
  }
  Lane &L = ctx->lane[0];
  if (!L.cloud.num_points) {
    set_error("gpd_hip_refine_normals: bad argument: no cloud uploaded");
    return GPD_ERR_INVALID;
  }
  HIP_RET(hipSetDevice(ctx->device));
  return refine_run(ctx->refine, L.cloud, k, max_iterations, convergence_threshold, normals_out, iterations_out, ddot_out, num_nan_out, kernel_ms,
                    L.stream);
}

int gpd_hip_remove_statistical_outliers(gpd_hip_ctx *ctx, int mean_k, double stddev_mult, int32_t *kept_out, int *num_kept, double stats[3],
                                        float *dist_out, float kernel_ms[3]) {
  if (int rc = refuse("gpd_hip_remove_statistical_outliers", ctx, kept_out && num_kept && stats && mean_k >= 1 && std::isfinite(stddev_mult)))
    return rc;
  if (mean_k > outlier::kMeanKCap) {
    set_error("gpd_hip_remove_statistical_outliers: mean_k = %d, the capacity is %d", mean_k, outlier::kMeanKCap);
    return GPD_ERR_CAPACITY;
  }
  Lane &L = ctx->lane[0];
  if (!L.cloud.num_points) {
    set_error("gpd_hip_remove_statistical_outliers: bad argument: no cloud uploaded");
    return GPD_ERR_INVALID;
  }
  if (L.cloud.num_points < mean_k + 1) {
    set_error("gpd_hip_remove_statistical_outliers: bad argument: mean_k = %d needs %d points, the cloud has %d", mean_k, mean_k + 1,
              L.cloud.num_points);
    return GPD_ERR_INVALID;
  }
  HIP_RET(hipSetDevice(ctx->device));
  return outlier_run(ctx->outliers, L.cloud, mean_k, stddev_mult, /*carry_normals=*/true, kept_out, num_kept, stats, dist_out, kernel_ms, L.stream);
}

// samples by index (sample_xyz == nullptr) or by coordinates (sample_indices == nullptr)
static int search_any(gpd_hip_ctx *ctx, const char *who, const int32_t *sample_indices, const double *sample_xyz, int num_samples,
                      gpd_hand *hands, int *num_sets) {
  int rc = refuse(who, ctx, (sample_indices || sample_xyz) && num_samples >= 0 && hands && num_sets, {Need::Cloud});
  if (rc) return rc;
  Lane &L = ctx->lane[0];
  *num_sets = 0;
  if (num_samples == 0) return GPD_OK;
  rc = check_samples(who, sample_indices, sample_xyz, num_samples, L.cloud.num_points);
  if (rc) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  HIP_RET(hipEventRecord(L.ev[0], L.stream));
  rc = search_run(ctx->params, L.cloud, L.search, sample_indices, sample_xyz, num_samples, L.stream);
  if (rc) return rc;
  HIP_RET(hipEventRecord(L.ev[1], L.stream));
  rc = search_download(ctx->params, L.search, hands, num_sets, L.stream);
  if (rc) return rc;
  HIP_RET(hipEventElapsedTime(&L.stage_ms[0], L.ev[0], L.ev[1]));
  return GPD_OK;
}

int gpd_hip_search(gpd_hip_ctx *ctx, const int32_t *sample_indices, int num_samples, gpd_hand *hands, int *num_sets) {
  StageRange range_("gpd:search (unfused entry)");
  if (int rc = refuse("gpd_hip_search", ctx, sample_indices)) return rc;
  return search_any(ctx, "gpd_hip_search", sample_indices, nullptr, num_samples, hands, num_sets);
}

int gpd_hip_search_samples(gpd_hip_ctx *ctx, const double *samples_xyz, int num_samples, gpd_hand *hands, int *num_sets) {
  if (int rc = refuse("gpd_hip_search_samples", ctx, samples_xyz)) return rc;
  return search_any(ctx, "gpd_hip_search_samples", nullptr, samples_xyz, num_samples, hands, num_sets);
}

int gpd_hip_reevaluate(gpd_hip_ctx *ctx, gpd_hand *hands, int num_hands, int32_t *labels) {
  StageRange range_("gpd:reevaluate");
  int rc = refuse("gpd_hip_reevaluate", ctx, num_hands >= 0 && (num_hands == 0 || (hands && labels)), {Need::Cloud});
  if (rc || num_hands == 0) return rc;
  Lane &L = ctx->lane[0];
  for (int i = 0; i < num_hands; i++)
    for (int r = 0; r < 3; r++)
      if (!std::isfinite(hands[i].sample[r])) {
        set_error("gpd_hip_reevaluate: hand %d has a non-finite sample", i);
        return GPD_ERR_INVALID;
      }
  HIP_RET(hipSetDevice(ctx->device));
  L.images.num_candidates = 0;  // the search buffers the resident candidate list points into are reused
  return reevaluate_run(ctx->params, L.cloud, L.search, hands, num_hands, labels, L.stream);
}

int gpd_hip_images(gpd_hip_ctx *ctx, const gpd_hand *hands, int num_sets, uint8_t *images, int32_t *cand_index,
                   int *num_candidates) {
  StageRange range_("gpd:images (unfused entry)");
  int rc = refuse("gpd_hip_images", ctx, hands && num_sets >= 0 && num_candidates, {Need::Cloud});
  if (rc) return rc;
  Lane &L = ctx->lane[0];
  HIP_RET(hipSetDevice(ctx->device));
  SearchState &s = L.search;
  const int slots = ctx->params.num_hand_axes * ctx->params.num_orientations;
  *num_candidates = 0;
  if (s.cloud_generation != L.cloud.generation || s.num_samples == 0) {
    set_error("images: hands must come from gpd_hip_search / gpd_hip_detect on this context and cloud");
    return GPD_ERR_STATE;
  }
  if (num_sets > s.num_samples) {
    set_error("images: %d sets passed, the search had %d samples", num_sets, s.num_samples);
    return GPD_ERR_INVALID;
  }
  // the caller's validity flags (the host filters between the stages clear them: grasp_detector.cpp:238-255)
  // replace the ones the search left on the device; everything else about the hands is already there.  The
  // sets' samples travel along: plan_kernel checks them against the search's (a moved hand set is refused).
  std::vector<uint8_t> fv((size_t)num_sets * slots + 1, 0);
  std::vector<double> smp((size_t)num_sets * 3 + 1, 0.0);
  for (int si = 0; si < num_sets; si++) {
    for (int j = 0; j < slots; j++) fv[(size_t)si * slots + j] = hands[(size_t)si * slots + j].valid ? 1 : 0;
    for (int r = 0; r < 3; r++) smp[3 * (size_t)si + r] = hands[(size_t)si * slots].sample[r];
  }
  HIP_RET(hipEventRecord(L.ev[0], L.stream));
  rc = plan_build(ctx->params, L.cloud, s, L.plan, L.stream, fv.data(), smp.data(), num_sets);
  if (rc) return rc;
  HIP_RET(hipStreamSynchronize(L.stream));  // fv / smp are pageable: their copies have left them by now as well
  if (L.plan.h_summary->mismatch_set >= 0) {
    set_error("images: set %d does not match the last search (sample moved, or more sets than the search produced)",
              L.plan.h_summary->mismatch_set);
    return GPD_ERR_STATE;
  }
  // the cloud's stream of shadow draws from its start; ev[0] stands ahead of the plan: stage_ms[1] is plan + images
  rc = lane_images(ctx, L, /*side_stream=*/true, 0, "gpd:images (gpd_hip_images)", nullptr, L.ev[1]);
  if (rc) return rc;
  const int n = L.images.num_candidates;
  *num_candidates = n;
  rc = lane_download_images(ctx->params, L, n, images, cand_index);
  if (rc) return rc;
  HIP_RET(hipMemcpyAsync(&L.h_flags->status, L.images.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
  HIP_RET(hipStreamSynchronize(L.stream));
  HIP_RET(hipEventElapsedTime(&L.stage_ms[1], L.ev[0], L.ev[1]));
  return lane_check(L, L.h_flags->status, /*scored=*/false);
}

}  // extern "C"
