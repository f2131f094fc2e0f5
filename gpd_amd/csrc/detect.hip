// C-ABI of libgpd_hip.so (include/gpd_hip.h): the fused detect — its three steps and the single-cloud entries built on
// them.  (The entries that accumulate rounds of the first step and a half, gpd_hip_label_view and gpd_hip_detect_sis: rounds.hip.)
//
// A context owns two LANES — each a HIP stream with its own cloud, search buffers, candidate plan,
// image buffers and LeNet scratch.  Every single-cloud entry point runs on lane 0.
// gpd_hip_detect_batch alternates the lanes: while the image + LeNet kernels of cloud i run on one
// lane, the upload + grid + search of cloud i+1 is already enqueued on the other, so host hops and
// the host-device copies of one cloud hide behind the kernels of its neighbour, and the
// tail of one cloud's kernel is filled by the other's.  (Measured against ONE stream carrying
// search(i+1) ahead of images+LeNet(i), i.e. the same pipelining with strictly sequential kernels: two streams
// 796 k candidates/s, one stream 735 k, same box, same 48 clouds.)
//
// A fused detect is three steps per cloud:
//   begin   enqueue sample upload, neighbourhood / centre / hand_eval kernels (incl. the workspace filter)
//           and plan_kernel (candidate list, shadow LCG offsets) + the 48-byte summary copy — no waiting
//   middle  wait for the summary (the only mid-pipeline wait: the launch sizes), enqueue image kernels,
//           LeNet, the record gather (all sets / candidates / the num_selected best) and ONE device-to-host
//           copy into pinned memory
//   end     wait, hand the records to the caller
// Between the stages nothing crosses PCIe but that summary.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "context.h"
#include "buffers.h"

using namespace gpd;

namespace gpd {

// ---- the three steps of a fused detect -------------------------------------------------------
int job_begin(gpd_hip_ctx *ctx, Lane &L, Job &J) {
  J.live = false;
  J.num_sets = J.num_candidates = J.num_hands = 0;
  if (J.S == 0) return GPD_OK;
  HIP_RET(hipEventRecord(L.ev[0], L.stream));
  int rc;
  {
    StageRange r("gpd:search (neighbourhoods, frames, hand evaluation, workspace filter)");
    rc = search_run(ctx->params, L.cloud, L.search, J.sample_idx, J.sample_xyz, J.S, L.stream, /*sync_counts=*/false,
                    J.resident ? &J.gather : nullptr);
  }
  if (rc) return rc;
  HIP_RET(hipEventRecord(L.ev[1], L.stream));
  {
    StageRange r("gpd:plan (hand sets, candidate list, shadow LCG offsets)");
    rc = plan_build(ctx->params, L.cloud, L.search, L.plan, L.stream);
  }
  if (rc) return rc;
  HIP_RET(hipEventRecord(L.ev_plan, L.stream));
  J.live = true;
  return GPD_OK;
}

// the middle step in two halves: wait for the plan summary (the only mid-pipeline wait; a list-capacity retry happens here), then
// enqueue images + LeNet + gather.  gpd_hip_detect_sharded puts the host-side scan of the shards' draw totals between the two.
int job_wait_plan(gpd_hip_ctx *ctx, Lane &L, Job &J) {
  if (!J.live) return GPD_OK;
  J.live = false;  // set again once everything is enqueued
  HIP_RET(hipEventSynchronize(L.ev_plan));  // not the stream: in a batch the next cloud's search is already queued behind
  J.t_plan_ms = now_ms();
  if (L.plan.h_summary->worst_found > L.search.nn_cap) {
    // a neighbourhood overflowed the list capacity of the search kernel: once more with the large lists
    const int cap = search_next_capacity(L.search, L.plan.h_summary->worst_found);
    if (!cap) {
      set_error("search: a neighbourhood holds %d points, more than the list capacity %d", L.plan.h_summary->worst_found, kNnCapMax);
      return GPD_ERR_CAPACITY;
    }
    // the side stream's centre_kernel of the first run is ordered before the plan, so it is done; the main stream still waits for
    // it explicitly before neighbourhood_kernel rebuilds the lists
    int rc = search_join(L.search, L.stream);
    if (rc) return rc;
    rc = search_force_capacity(L.search, cap);
    if (rc) return rc;
    rc = job_begin(ctx, L, J);
    if (rc) return rc;
    J.live = false;
    HIP_RET(hipStreamSynchronize(L.stream));
  }
  J.lcg_draws = L.plan.h_summary->total_draws;
  J.live = true;
  return GPD_OK;
}

int job_enqueue(gpd_hip_ctx *ctx, Lane &L, Job &J) {
  if (!J.live) return GPD_OK;
  J.live = false;
  const PlanSummary sm = *L.plan.h_summary;
  static const bool plan_timing = prof_env("GPD_PLAN_TIMING") != nullptr;
  if (plan_timing)
    fprintf(stderr, "[plan-timing] own sums %.2f us, look-back %.2f, tables + summary %.2f (last workgroup's thread 0, 100 MHz clock)\n",
            (sm.pad_[0] & 0xffff) * 0.01, ((unsigned)sm.pad_[0] >> 16) * 0.01, (sm.pad_[1] & 0xffff) * 0.01);
  const int slots = ctx->params.num_hand_axes * ctx->params.num_orientations;
  J.num_sets = sm.num_sets;
  J.num_candidates = sm.num_candidates;
  const int n = sm.num_candidates;
  int k = 0;
  if (J.mode == 0)
    J.out_records = sm.num_sets * slots;
  else if (J.num_selected > 0)
    J.out_records = k = std::min(J.num_selected, n);
  else
    J.out_records = n;
  J.num_hands = J.out_records;
  if ((long long)J.out_records > J.capacity) {
    set_error("detect: %d hand records to return, the caller's buffer holds %lld", J.out_records, J.capacity);
    return GPD_ERR_INVALID;
  }
  (void)hipEventElapsedTime(&L.stage_ms[0], L.ev[0], L.ev[1]);  // here: the next job on this lane records them again
  // (inside gpd_hip_detect_batch no side stream: the other cloud's kernels already fill the gaps)
  int rc = lane_images(ctx, L, !ctx->in_batch, J.lcg_base, "gpd:images (shadow sets, shadow channels, normals + depth channels)", L.ev[4],
                       L.ev[2]);
  if (rc) return rc;
  rc = lane_lenet(ctx, L, L.images.d_images, n, "gpd:lenet (conv1, conv2, ip1, ip2)");
  if (rc) return rc;
  HIP_RET(hipEventRecord(L.ev[3], L.stream));
  rc = reserve_out(L, (size_t)J.out_records, k ? (size_t)n * sizeof(float) : 0);
  if (rc) return rc;
  L.h_flags->tie = 0;
  if (J.mode == 0) {
    rc = plan_emit_hands(ctx->params, L.search, L.plan, n > 0 ? L.d_scores : nullptr, L.d_out, false, L.stream);
  } else if (k > 0) {
    rc = reserve_selection(L, k, n);
    if (rc) return rc;
    // every candidate record, scored, in a list of this job's own: the selection gathers from it, and so does the
    // std::partial_sort rerun of job_end — by then, in a batch, the lane's search / plan buffers already hold the
    // cloud after next (begin(i + 1) is enqueued before end(i - 1))
    rc = plan_emit_hands(ctx->params, L.search, L.plan, L.d_scores, L.d_all, true, L.stream);
    if (rc) return rc;
    if (k <= select_topk_capacity()) {
      rc = select_topk(L.d_scores, n, k, L.d_sel, L.d_sel + k, L.stream);
      if (rc) return rc;
      rc = gather_records(L.d_all, L.d_sel, k, L.d_out, L.stream);
      if (rc) return rc;
      HIP_RET(hipMemcpyAsync(&L.h_flags->tie, L.d_sel + k, sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
    } else {
      L.h_flags->tie = 2;  // more winners than the device selection sorts: std::partial_sort on the host (job_end), no limit
    }
    // the scores (4 bytes per candidate) ride along: equal scores are settled with std::partial_sort on the host
    HIP_RET(hipMemcpyAsync(L.h_out + L.d_out_cap * sizeof(gpd_hand), L.d_scores, (size_t)n * sizeof(float), hipMemcpyDeviceToHost,
                           L.stream));
  } else {
    rc = plan_emit_hands(ctx->params, L.search, L.plan, L.d_scores, L.d_out, true, L.stream);
  }
  if (rc) return rc;
  // A megabyte or more of records (all hand sets of a cloud: 3.6 MB) leaves in four copies with an event behind each, so that
  // job_end hands chunk c to the caller while chunk c + 1 is still on the bus: the pinned-to-caller memcpy (0.2 ms for 3.6 MB)
  // used to start only after the last byte had arrived.  Not for selections: their records may be gathered again (ties).
  J.chunks = ((size_t)J.out_records * sizeof(gpd_hand) >= (1u << 20) && !(J.mode == 1 && J.num_selected > 0)) ? 4 : 0;
  if (J.chunks) {
    const size_t per = ((size_t)J.out_records + J.chunks - 1) / J.chunks;
    for (int c = 0; c < J.chunks; c++) {
      const size_t r0 = std::min((size_t)c * per, (size_t)J.out_records), r1 = std::min(r0 + per, (size_t)J.out_records);
      if (r1 > r0)
        HIP_RET(hipMemcpyAsync(L.h_out + r0 * sizeof(gpd_hand), L.d_out + r0, (r1 - r0) * sizeof(gpd_hand), hipMemcpyDeviceToHost, L.stream));
      HIP_RET(hipEventRecord(L.ev_chunk[c], L.stream));
    }
  } else if (J.out_records > 0) {
    HIP_RET(hipMemcpyAsync(L.h_out, L.d_out, (size_t)J.out_records * sizeof(gpd_hand), hipMemcpyDeviceToHost, L.stream));
  }
  HIP_RET(hipMemcpyAsync(&L.h_flags->status, L.images.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
  HIP_RET(hipEventRecord(L.ev_done, L.stream));
  J.live = true;
  return GPD_OK;
}

int job_middle(gpd_hip_ctx *ctx, Lane &L, Job &J) {
  const int rc = job_wait_plan(ctx, L, J);
  return rc ? rc : job_enqueue(ctx, L, J);
}

static bool score_greater(const std::pair<float, int32_t> &a, const std::pair<float, int32_t> &b) { return a.first > b.first; }

int job_end(gpd_hip_ctx *ctx, Lane &L, Job &J) {
  if (!J.live) return GPD_OK;
  J.live = false;
  double early_copy_ms = 0.0;
  if (J.chunks) {
    // (should a flag below turn out set, the caller's buffer holds records of a failed call: its content is unspecified then)
    const size_t per = ((size_t)J.out_records + J.chunks - 1) / J.chunks;
    for (int c = 0; c < J.chunks; c++) {
      HIP_RET(hipEventSynchronize(L.ev_chunk[c]));
      const auto t0 = std::chrono::steady_clock::now();
      const size_t r0 = std::min((size_t)c * per, (size_t)J.out_records), r1 = std::min(r0 + per, (size_t)J.out_records);
      if (r1 > r0) std::memcpy(J.hands + r0, L.h_out + r0 * sizeof(gpd_hand), (r1 - r0) * sizeof(gpd_hand));
      early_copy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
  }
  HIP_RET(hipEventSynchronize(L.ev_done));
  const auto t_done = std::chrono::steady_clock::now();
  (void)hipEventElapsedTime(&L.stage_ms[1], L.ev[4], L.ev[2]);
  (void)hipEventElapsedTime(&L.stage_ms[2], L.ev[2], L.ev[3]);
  if (int rc = lane_check(L, L.h_flags->status, /*scored=*/true)) return rc;
  const int n = J.num_candidates;
  if (J.mode == 1 && J.num_selected > 0 && J.out_records > 0 && L.h_flags->tie) {
    // equal scores among the winners: the reference's result is whatever std::partial_sort leaves
    // (grasp_detector.cpp:409), which depends on the history of its heap — so run exactly that, on
    // (score, candidate) pairs in candidate order, and gather the winners again
    const float *sc = reinterpret_cast<const float *>(L.h_out + L.d_out_cap * sizeof(gpd_hand));
    std::vector<std::pair<float, int32_t>> v((size_t)n);
    for (int i = 0; i < n; i++) v[i] = {sc[i], i};
    const int k = J.out_records;
    std::partial_sort(v.begin(), v.begin() + k, v.end(), score_greater);
    std::vector<int32_t> sel((size_t)k);
    for (int i = 0; i < k; i++) sel[i] = v[i].second;
    HIP_RET(hipMemcpyAsync(L.d_sel, sel.data(), (size_t)k * sizeof(int32_t), hipMemcpyHostToDevice, L.stream));
    int rc = gather_records(L.d_all, L.d_sel, k, L.d_out, L.stream);  // not from L.search / L.plan: see job_middle
    if (rc) return rc;
    HIP_RET(hipMemcpyAsync(L.h_out, L.d_out, (size_t)k * sizeof(gpd_hand), hipMemcpyDeviceToHost, L.stream));
    HIP_RET(hipStreamSynchronize(L.stream));
  }
  if (J.out_records > 0 && !J.chunks) std::memcpy(J.hands, L.h_out, (size_t)J.out_records * sizeof(gpd_hand));
  J.copy_ms = early_copy_ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_done).count();
  return GPD_OK;
}

}  // namespace gpd

extern "C" {

static int detect_any(gpd_hip_ctx *ctx, const char *who, const int32_t *sample_indices, const double *sample_xyz, int num_samples,
                      int mode, int num_selected, gpd_hand *hands, long long capacity, int *num_sets, int *num_candidates,
                      int *num_hands) {
  int rc = refuse(who, ctx, hands && num_sets && num_candidates && (sample_indices || sample_xyz) && num_samples >= 0 && num_selected >= 0,
                  {Need::LeNet, Need::Cloud});
  if (rc) return rc;
  Lane &L = ctx->lane[0];
  *num_sets = 0;
  *num_candidates = 0;
  if (num_hands) *num_hands = 0;
  rc = check_samples(who, sample_indices, sample_xyz, num_samples, L.cloud.num_points);
  if (rc) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  // GPD_DETECT_TIMING=1: wall time of the three steps, to stderr
  const bool timing = prof_env("GPD_DETECT_TIMING") != nullptr;
  const double t0 = now_ms();
  Job J;
  J.sample_idx = sample_indices;
  J.sample_xyz = sample_xyz;
  J.S = num_samples;
  J.mode = mode;
  J.num_selected = num_selected;
  J.hands = hands;
  J.capacity = capacity;
  rc = job_begin(ctx, L, J);
  if (rc) return rc;
  const double t1 = now_ms();
  rc = job_middle(ctx, L, J);
  if (rc) return rc;
  const double t2 = now_ms();
  rc = job_end(ctx, L, J);
  if (rc) return rc;
  *num_sets = J.num_sets;
  *num_candidates = J.num_candidates;
  if (num_hands) *num_hands = J.num_hands;
  if (timing)
    fprintf(stderr, "[detect-timing] enqueue search+plan %.3f ms, wait+enqueue images/LeNet/gather %.3f, wait+copy out %.3f; kernels: search %.3f images %.3f LeNet %.3f\n",
            t1 - t0, t2 - t1, now_ms() - t2, L.stage_ms[0], L.stage_ms[1], L.stage_ms[2]);
  return GPD_OK;
}

int gpd_hip_detect(gpd_hip_ctx *ctx, const int32_t *sample_indices, int num_samples, gpd_hand *hands, int *num_sets,
                   int *num_candidates) {
  if (int rc = refuse("gpd_hip_detect", ctx, sample_indices)) return rc;
  const long long cap = (long long)num_samples * ctx->params.num_hand_axes * ctx->params.num_orientations;
  return detect_any(ctx, "gpd_hip_detect", sample_indices, nullptr, num_samples, 0, 0, hands, cap, num_sets, num_candidates, nullptr);
}

int gpd_hip_detect_samples(gpd_hip_ctx *ctx, const double *samples_xyz, int num_samples, gpd_hand *hands, int *num_sets,
                           int *num_candidates) {
  if (int rc = refuse("gpd_hip_detect_samples", ctx, samples_xyz)) return rc;
  const long long cap = (long long)num_samples * ctx->params.num_hand_axes * ctx->params.num_orientations;
  return detect_any(ctx, "gpd_hip_detect_samples", nullptr, samples_xyz, num_samples, 0, 0, hands, cap, num_sets, num_candidates,
                    nullptr);
}

int gpd_hip_detect_select(gpd_hip_ctx *ctx, const int32_t *sample_indices, int num_samples, int num_selected, gpd_hand *hands,
                          int hands_capacity, int *num_sets, int *num_candidates, int *num_hands) {
  if (int rc = refuse("gpd_hip_detect_select", ctx, sample_indices && num_hands && hands_capacity >= 0)) return rc;
  return detect_any(ctx, "gpd_hip_detect_select", sample_indices, nullptr, num_samples, 1, num_selected, hands, hands_capacity, num_sets,
                    num_candidates, num_hands);
}

}  // extern "C"
