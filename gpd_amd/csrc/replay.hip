// C-ABI of libgpd_hip.so (include/gpd_hip.h): measurement only — the replays bench.py times on the resident candidate
// list, and what the last call left behind (stage times, image statistics, slow paths taken).
#include <cstdlib>
#include <vector>

#include "context.h"
#include "buffers.h"

using namespace gpd;

extern "C" {

int gpd_hip_replay(gpd_hip_ctx *ctx, int stages) {
  StageRange range_("gpd:replay (images + lenet on the resident list)");
  if (!ctx || !(stages & 3) || (stages & ~3)) {
    set_error("gpd_hip_replay: bad argument");
    return GPD_ERR_INVALID;
  }
  Lane &L = ctx->lane[0];
  if (L.images.num_candidates <= 0 || !L.images.d_images || L.search.num_samples == 0) {
    set_error("gpd_hip_replay: no candidate list on the device (call gpd_hip_images / gpd_hip_detect first)");
    return GPD_ERR_STATE;
  }
  if ((stages & 2) && !ctx->lenet.channels) {
    set_error("gpd_hip_replay: LeNet weights not set");
    return GPD_ERR_STATE;
  }
  HIP_RET(hipSetDevice(ctx->device));
  const int n = L.images.num_candidates;
  int rc = reserve_scores(L, n);
  if (rc) return rc;
  while (ctx->replay_events.size() < ctx->replay_used + 6) {
    hipEvent_t e;
    HIP_RET(hipEventCreate(&e));
    ctx->replay_events.push_back(e);
  }
  hipEvent_t *ev = &ctx->replay_events[ctx->replay_used];
  ctx->replay_used += 6;
  static const bool pipe = prof_env("GPD_REPLAY_PIPE") && atoi(prof_env("GPD_REPLAY_PIPE")) > 0;
  if (pipe && stages == 3) {
    const size_t bytes = (size_t)L.images.capacity * L.images.channels * 3600;
    if (!ctx->pipe_stream) {
      HIP_RET(hipStreamCreate(&ctx->pipe_stream));
      for (int b = 0; b < 2; b++) {
        HIP_RET(hipEventCreateWithFlags(&ctx->pipe_filled[b], hipEventDisableTiming));
        HIP_RET(hipEventCreateWithFlags(&ctx->pipe_read[b], hipEventDisableTiming));
      }
    }
    if (ctx->pipe_bytes != bytes || ctx->pipe_images[0] != L.images.d_images) {
      // (re)start: the list was rebuilt since; lane 0's buffer is [0], a second one of the same size is [1]
      HIP_RET(hipStreamSynchronize(ctx->pipe_stream));
      device_release(ctx->pipe_images[1]);
      HIP_RET(device_alloc(ctx->pipe_images[1], bytes));
      ctx->pipe_images[0] = L.images.d_images;
      ctx->pipe_bytes = bytes;
      ctx->pipe_read_valid[0] = ctx->pipe_read_valid[1] = false;
      ctx->pipe_k = 0;
    }
    const int b = (int)(ctx->pipe_k++ & 1);
    if (ctx->pipe_read_valid[b]) HIP_RET(hipStreamWaitEvent(L.stream, ctx->pipe_read[b], 0));  // LeNet of replay k - 2 has read it
    HIP_RET(hipEventRecord(ev[0], L.stream));
    uint8_t *own = L.images.d_images;
    L.images.d_images = ctx->pipe_images[b];
    rc = images_launch(L.search, L.plan, L.images, L.stream);
    L.images.d_images = own;
    if (rc) return rc;
    HIP_RET(hipEventRecord(ev[1], L.stream));
    HIP_RET(hipEventRecord(ctx->pipe_filled[b], L.stream));
    HIP_RET(hipStreamWaitEvent(ctx->pipe_stream, ctx->pipe_filled[b], 0));
    HIP_RET(lenet_forward(ctx->lenet, L.lenet_scratch, ctx->pipe_images[b], n, L.d_scores, ctx->pipe_stream, ev + 2));
    HIP_RET(hipEventRecord(ev[5], ctx->pipe_stream));
    HIP_RET(hipEventRecord(ctx->pipe_read[b], ctx->pipe_stream));
    ctx->pipe_read_valid[b] = true;
    return GPD_OK;
  }
  HIP_RET(hipEventRecord(ev[0], L.stream));
  if (stages & 1) {
    rc = images_launch(L.search, L.plan, L.images, L.stream);
    if (rc) return rc;
  }
  HIP_RET(hipEventRecord(ev[1], L.stream));
  if (stages & 2) {
    HIP_RET(lenet_forward(ctx->lenet, L.lenet_scratch, L.images.d_images, n, L.d_scores, L.stream, ev + 2));
  } else {
    for (int i = 2; i < 5; i++) HIP_RET(hipEventRecord(ev[i], L.stream));
  }
  HIP_RET(hipEventRecord(ev[5], L.stream));
  return GPD_OK;
}

int gpd_hip_replay_times(gpd_hip_ctx *ctx, float ms[2], int *launches, float *scores) {
  if (!ctx || !ms) return GPD_ERR_INVALID;
  HIP_RET(hipSetDevice(ctx->device));
  Lane &L = ctx->lane[0];
  HIP_RET(hipStreamSynchronize(L.stream));
  if (ctx->pipe_stream) HIP_RET(hipStreamSynchronize(ctx->pipe_stream));
  ms[0] = ms[1] = 0.f;
  for (int k = 0; k < 4; k++) ctx->replay_kernel_ms[k] = 0.f;
  for (size_t i = 0; i + 5 < ctx->replay_used; i += 6) {
    float a = 0.f, b = 0.f;
    HIP_RET(hipEventElapsedTime(&a, ctx->replay_events[i], ctx->replay_events[i + 1]));
    HIP_RET(hipEventElapsedTime(&b, ctx->replay_events[i + 1], ctx->replay_events[i + 5]));
    ms[0] += a;
    ms[1] += b;
    for (int k = 0; k < 4; k++) {
      float t = 0.f;
      HIP_RET(hipEventElapsedTime(&t, ctx->replay_events[i + 1 + k], ctx->replay_events[i + 2 + k]));
      ctx->replay_kernel_ms[k] += t;
    }
  }
  if (launches) *launches = (int)(ctx->replay_used / 6);
  ctx->replay_used = 0;
  if (scores && L.images.num_candidates > 0 && L.d_scores)
    HIP_RET(hipMemcpy(scores, L.d_scores, (size_t)L.images.num_candidates * sizeof(float), hipMemcpyDeviceToHost));
  int32_t status = 0;
  if (L.images.d_status) HIP_RET(hipMemcpy(&status, L.images.d_status, sizeof(int32_t), hipMemcpyDeviceToHost));
  if (status) {
    set_images_status_error(status);
    return GPD_ERR_CAPACITY;
  }
  return lenet_check(L.lenet_scratch);
}

int gpd_hip_conv1_stats(gpd_hip_ctx *ctx, unsigned long long pairs[2], int reset) {
  if (!ctx || !pairs) {
    set_error("gpd_hip_conv1_stats: bad argument");
    return GPD_ERR_INVALID;
  }
  HIP_RET(hipSetDevice(ctx->device));
  LeNetScratch &s = ctx->lane[0].lenet_scratch;
  pairs[0] = pairs[1] = 0;
  if (!s.c1_stats) return GPD_OK;
  HIP_RET(hipStreamSynchronize(ctx->lane[0].stream));
  HIP_RET(hipMemcpy(pairs, s.c1_stats, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  if (reset) HIP_RET(hipMemset(s.c1_stats, 0, 2 * sizeof(unsigned long long)));
  return GPD_OK;
}

int gpd_hip_replay_kernel_ms(gpd_hip_ctx *ctx, float ms[4]) {
  if (!ctx || !ms) return GPD_ERR_INVALID;
  for (int k = 0; k < 4; k++) ms[k] = ctx->replay_kernel_ms[k];
  return GPD_OK;
}

int gpd_hip_last_images_stats(gpd_hip_ctx *ctx, long long out[4]) {
  if (!ctx || !out) return GPD_ERR_INVALID;
  const Lane &L = ctx->lane[0];
  out[0] = L.images.num_candidates;
  out[1] = L.images.stat_sets;
  out[2] = L.images.stat_sum_set_ni;
  out[3] = L.images.stat_sum_cand_ni;
  return GPD_OK;
}

int gpd_hip_last_fallbacks(gpd_hip_ctx *ctx, long long out[4]) {
  if (!ctx || !out) return GPD_ERR_INVALID;
  HIP_RET(hipSetDevice(ctx->device));
  Lane &L = ctx->lane[0];
  HIP_RET(hipStreamSynchronize(L.stream));
  out[0] = L.search.nn_cap;
  out[1] = out[2] = 0;
  const ImageState &im = L.images;
  int32_t v = 0;
  if (im.d_overflow && im.channels == 15 && im.num_candidates > 0) {
    HIP_RET(hipMemcpy(&v, im.d_status + 1, sizeof(int32_t), hipMemcpyDeviceToHost));
    out[1] = v;
  }
  if (im.d_pts_overflow && im.num_candidates > 0) {
    HIP_RET(hipMemcpy(&v, im.d_status + 3, sizeof(int32_t), hipMemcpyDeviceToHost));
    out[2] = v;
  }
  out[3] = im.num_candidates > 0 ? (im.num_candidates + 65535) / 65536 : 0;
  return GPD_OK;
}

int gpd_hip_last_image_routes(gpd_hip_ctx *ctx, int32_t *route, int n, long long info[8]) {
  if (!ctx || !route || !info || n < 0) {
    set_error("gpd_hip_last_image_routes: bad argument");
    return GPD_ERR_INVALID;
  }
  Lane &L = ctx->lane[0];
  if (n < L.images.num_candidates) {
    set_error("gpd_hip_last_image_routes: room for %d candidates, the last launch had %d", n, L.images.num_candidates);
    return GPD_ERR_INVALID;
  }
  HIP_RET(hipSetDevice(ctx->device));
  HIP_RET(hipStreamSynchronize(L.stream));
  return images_routes(L.images, route, info);
}

int gpd_hip_last_normals_routes(gpd_hip_ctx *ctx, int32_t *count, int n, long long info[8]) {
  if (!ctx || !count || !info || n < 0) {
    set_error("gpd_hip_last_normals_routes: bad argument");
    return GPD_ERR_INVALID;
  }
  Lane &L = ctx->lane[0];
  HIP_RET(hipSetDevice(ctx->device));
  HIP_RET(hipStreamSynchronize(L.stream));
  return normals_routes(L.cloud, count, n, info);
}

int gpd_hip_last_centre_chains(gpd_hip_ctx *ctx, long long *out) {
  if (!ctx || !out) return GPD_ERR_INVALID;
  HIP_RET(hipSetDevice(ctx->device));
  Lane &L = ctx->lane[0];
  HIP_RET(hipStreamSynchronize(L.stream));
  *out = 0;
  const int S = L.search.num_samples;
  if (S <= 0 || !L.search.d_counts) return GPD_OK;
  std::vector<int32_t> h((size_t)S * 8);
  HIP_RET(hipMemcpy(h.data(), L.search.d_counts, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
  long long n = 0;
  for (int i = 0; i < S; i++) n += __builtin_popcount((unsigned)h[(size_t)8 * i + 5] & 7u);
  *out = n;
  return GPD_OK;
}

int gpd_hip_last_stage_ms(gpd_hip_ctx *ctx, float ms[3]) {
  if (!ctx || !ms) return GPD_ERR_INVALID;
  for (int i = 0; i < 3; i++) ms[i] = ctx->lane[0].stage_ms[i];
  return GPD_OK;
}

}  // extern "C"
