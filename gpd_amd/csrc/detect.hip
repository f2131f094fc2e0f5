// C-ABI of libgpd_hip.so (include/gpd_hip.h): the fused detect — its three steps, the single-cloud entries built on
// them, gpd_hip_label_view, whose round loop is the first step and a half with a tail of its own, and gpd_hip_detect_sis, whose
// rounds are that step and a half behind a draw on the device (sis.hip), with one LeNet pass over everything at the end.
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
#include "balance_model.h"
#include "sis_model.h"

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
  HIP_RET(hipEventRecord(L.ev[4], L.stream));
  L.images.side_stream = !ctx->in_batch;
  L.images.lcg_base = J.lcg_base;
  int rc;
  {
    StageRange r("gpd:images (shadow sets, shadow channels, normals + depth channels)");
    rc = images_run(ctx->params, L.cloud, L.search, L.plan, L.images, L.stream);
  }
  if (rc) return rc;
  HIP_RET(hipEventRecord(L.ev[2], L.stream));
  if (n > 0) {
    rc = reserve_scores(L, n);
    if (rc) return rc;
    {
      StageRange r("gpd:lenet (conv1, conv2, ip1, ip2)");
      HIP_RET(lenet_forward(ctx->lenet, L.lenet_scratch, L.images.d_images, n, L.d_scores, L.stream));
    }
    HIP_RET(hipMemcpyAsync(&L.h_flags->lenet, L.lenet_scratch.c1_stats + 2, sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
  } else {
    L.h_flags->lenet = 0;
  }
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
  if (L.h_flags->status) {
    set_images_status_error(L.h_flags->status);
    return GPD_ERR_CAPACITY;
  }
  if (L.h_flags->lenet) {
    const int rc = lenet_check(L.lenet_scratch);  // clears the device word, sets the error text
    return rc ? rc : GPD_ERR_HIP;
  }
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

// gpd_hip_label_view, and gpd_hip_train_append_view through a sink (train.hip): the rounds and the selection are one code
int label_view_run(gpd_hip_ctx *ctx, gpd_label_view_job *job, const char *who, const LabelSink *sink) {
  StageRange range_("gpd:label_view");
  if (!ctx || !job) {
    set_error("%s: bad argument", who);
    return GPD_ERR_INVALID;
  }
  gpd_label_view_job &j = *job;
  j.rounds_run = j.num_candidates = j.num_positives = j.num_out = j.num_positives_out = j.gt_neighbourhoods = 0;
  j.d2h_bytes = 0;
  for (float &m : j.stage_ms) m = 0.f;
  const int half = j.max_grasps_per_view > 0 ? j.max_grasps_per_view / 2 : 0;
  const long long total_samples = (long long)j.samples_per_round * j.max_rounds;
  if (j.samples_per_round < 0 || j.max_rounds < 0 || (total_samples > 0 && !j.sample_indices) || total_samples > 0x7fffffffll ||
      (!sink && (j.capacity < 0 || (j.capacity > 0 && (!j.images || !j.labels)))) || (j.all_labels && j.all_labels_capacity < 0)) {
    set_error("%s: bad argument", who);
    return GPD_ERR_INVALID;
  }
  if (!sink && (long long)j.capacity < 2ll * half) {
    set_error("%s: capacity %d, up to %d instances are kept at max_grasps_per_view = %d", who, j.capacity, 2 * half,
              j.max_grasps_per_view);
    return GPD_ERR_INVALID;
  }
  Lane &L = ctx->lane[0];
  LabelState &ls = ctx->label;
  if (!L.cloud.num_points) {
    set_error("%s: no cloud uploaded", who);
    return GPD_ERR_STATE;
  }
  if (!ls.gt.num_points) {
    set_error("%s: no ground truth uploaded (gpd_hip_upload_ground_truth)", who);
    return GPD_ERR_STATE;
  }
  int rc = check_samples(who, j.sample_indices, nullptr, (int)total_samples, L.cloud.num_points);
  if (rc) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  rc = label_init(ls);
  if (rc) return rc;
  if (j.round_counts) std::memset(j.round_counts, 0, (size_t)j.max_rounds * 2 * sizeof(int32_t));
  const gpd_params &p = ctx->params;
  const int C = p.image_num_channels;
  const size_t image_bytes = (size_t)kPix * C;
  ls.grows = 0;
  long long d2h = 0;
  size_t acc = 0;  // candidates accumulated
  int positives = 0, lists = 0, r = 0;
  for (; r < j.max_rounds && positives < j.min_positives; r++) {
    // createGraspImages (grasp_detector.cpp:458-521): what a fused detect builds before the LeNet
    Job J;
    J.sample_idx = j.sample_indices + (size_t)r * j.samples_per_round;
    J.S = j.samples_per_round;
    J.mode = 1;
    rc = job_begin(ctx, L, J);
    if (rc) return rc;
    if (!J.live) continue;  // a round without samples
    const int cap_before = L.search.nn_cap;
    rc = job_wait_plan(ctx, L, J);
    if (rc) return rc;
    d2h += (long long)sizeof(PlanSummary) * (L.search.nn_cap != cap_before ? 2 : 1);
    const PlanSummary sm = *L.plan.h_summary;
    const int n = sm.num_candidates;
    float ms = 0.f;
    (void)hipEventElapsedTime(&ms, L.ev[0], L.ev[1]);
    j.stage_ms[0] += ms;
    int round_pos = 0;
    if (n > 0) {
      HIP_RET(hipEventRecord(L.ev[4], L.stream));
      L.images.side_stream = true;
      L.images.lcg_base = 0;  // every round is an ordinary call: its shadow stream starts at 0
      {
        StageRange r_("gpd:images (label_view round)");
        rc = images_run(p, L.cloud, L.search, L.plan, L.images, L.stream);
      }
      if (rc) return rc;
      HIP_RET(hipEventRecord(L.ev[2], L.stream));
      // the round joins the view's accumulator: images in the caller's layout, records as detect_select(0) returns them
      HIP_RET(hipEventRecord(ls.ev[0], L.stream));
      rc = label_reserve(ls, acc + (size_t)n, acc, image_bytes, (size_t)n, L.stream);
      if (rc) return rc;
      HIP_RET(planar_to_hwc(L.images.d_images, ls.d_images + acc * image_bytes, n, C, L.stream));
      rc = plan_emit_hands(p, L.search, L.plan, nullptr, ls.d_hands + acc, true, L.stream);
      if (rc) return rc;
      // evalGroundTruth (grasp_detector.cpp:522-526) on the records where they are
      int img_status = 0;
      {
        StageRange r_("gpd:labels (ground-truth neighbourhoods per hand set, reevaluateHypotheses)");
        rc = label_round(p, ls.gt, ls.gt_search, ls.d_hands + acc, ls.d_labels + acc, n, sm.live_sets, ls.d_cand_list, ls.d_meta, ls.h_meta,
                         L.images.d_status, &img_status, &round_pos, &d2h, L.stream);
      }
      if (img_status) set_images_status_error(img_status);
      if (rc) return rc;
      HIP_RET(hipEventRecord(ls.ev[1], L.stream));
      HIP_RET(hipEventSynchronize(ls.ev[1]));
      (void)hipEventElapsedTime(&ms, L.ev[4], L.ev[2]);
      j.stage_ms[1] += ms;
      (void)hipEventElapsedTime(&ms, ls.ev[0], ls.ev[1]);
      j.stage_ms[2] += ms;
      lists += sm.live_sets;
    } else {
      L.images.num_candidates = 0;  // no candidate list of this round is resident
    }
    if (j.round_counts) {
      j.round_counts[2 * r] = n;
      j.round_counts[2 * r + 1] = round_pos;
    }
    acc += (size_t)n;
    positives += round_pos;
    if (acc > 0x7fffffffull) {
      set_error("%s: more than 2^31 accumulated candidates", who);
      return GPD_ERR_CAPACITY;
    }
  }
  j.rounds_run = r;
  j.num_candidates = (int)acc;
  j.num_positives = positives;
  j.gt_neighbourhoods = lists;
  // balanceInstances (data_generator.cpp:406-430): P and N are known here, the indices are the device's business
  const int end = balance::kept_per_class(positives, (long long)acc - positives, j.max_grasps_per_view);
  const size_t k = (size_t)2 * end;
  const size_t all = j.all_labels ? std::min(acc, (size_t)j.all_labels_capacity) : 0;
  size_t off[4];
  const size_t out_bytes = sink ? 0 : label_out_layout(k, image_bytes, off);  // what the kept set takes in the pinned block
  if (k + all > 0) {
    rc = grow_pinned(ls.h_out, ls.h_out_bytes, out_bytes + all, slack_cap(out_bytes + all, 8), __func__);
    if (rc) return rc;
    HIP_RET(hipEventRecord(ls.ev[2], L.stream));
    if (sink && k > 0) {  // the kept set stays on the device: straight behind what the sink holds
      uint8_t *to_images = nullptr, *to_labels = nullptr;
      rc = sink->place(sink->self, k, &to_images, &to_labels);
      if (rc) return rc;
      HIP_RET(hipSetDevice(ctx->device));
      rc = label_select_gather(ls, (int)acc, end, L.stream, to_images, to_labels);
    } else {
      rc = label_select_gather(ls, (int)acc, end, L.stream);
    }
    if (rc) return rc;
    if (k > 0 && !sink) HIP_RET(hipMemcpyAsync(ls.h_out, ls.d_out, out_bytes, hipMemcpyDeviceToHost, L.stream));  // the kept set: one copy
    if (all > 0) HIP_RET(hipMemcpyAsync(ls.h_out + out_bytes, ls.d_labels, all, hipMemcpyDeviceToHost, L.stream));
    HIP_RET(hipEventRecord(ls.ev[3], L.stream));
    HIP_RET(hipEventSynchronize(ls.ev[3]));
    (void)hipEventElapsedTime(&j.stage_ms[3], ls.ev[2], ls.ev[3]);
    d2h += (long long)(k > 0 ? out_bytes : 0) + (long long)all;
    if (k > 0 && !sink) {
      std::memcpy(j.images, ls.h_out + off[0], k * image_bytes);
      if (j.hands) std::memcpy(j.hands, ls.h_out + off[1], k * sizeof(gpd_hand));
      if (j.src_index) std::memcpy(j.src_index, ls.h_out + off[2], k * sizeof(int32_t));
      std::memcpy(j.labels, ls.h_out + off[3], k);
    }
    if (all > 0) std::memcpy(j.all_labels, ls.h_out + out_bytes, all);
  }
  j.num_out = (int)k;
  j.num_positives_out = end;
  j.d2h_bytes = d2h;
  return GPD_OK;
}

}  // namespace gpd

extern "C" {

static int detect_any(gpd_hip_ctx *ctx, const char *who, const int32_t *sample_indices, const double *sample_xyz, int num_samples,
                      int mode, int num_selected, gpd_hand *hands, long long capacity, int *num_sets, int *num_candidates,
                      int *num_hands) {
  if (!ctx || !hands || !num_sets || !num_candidates || (!sample_indices && !sample_xyz) || num_samples < 0 || num_selected < 0) {
    set_error("%s: bad argument", who);
    return GPD_ERR_INVALID;
  }
  if (!ctx->lenet.channels) {
    set_error("%s: LeNet weights not set", who);
    return GPD_ERR_STATE;
  }
  Lane &L = ctx->lane[0];
  if (!L.cloud.num_points) {
    set_error("%s: no cloud uploaded", who);
    return GPD_ERR_STATE;
  }
  *num_sets = 0;
  *num_candidates = 0;
  if (num_hands) *num_hands = 0;
  int rc = check_samples(who, sample_indices, sample_xyz, num_samples, L.cloud.num_points);
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
  if (!sample_indices) {
    set_error("gpd_hip_detect: bad argument");
    return GPD_ERR_INVALID;
  }
  const long long cap = ctx ? (long long)num_samples * ctx->params.num_hand_axes * ctx->params.num_orientations : 0;
  return detect_any(ctx, "gpd_hip_detect", sample_indices, nullptr, num_samples, 0, 0, hands, cap, num_sets, num_candidates, nullptr);
}

int gpd_hip_detect_samples(gpd_hip_ctx *ctx, const double *samples_xyz, int num_samples, gpd_hand *hands, int *num_sets,
                           int *num_candidates) {
  if (!samples_xyz) {
    set_error("gpd_hip_detect_samples: bad argument");
    return GPD_ERR_INVALID;
  }
  const long long cap = ctx ? (long long)num_samples * ctx->params.num_hand_axes * ctx->params.num_orientations : 0;
  return detect_any(ctx, "gpd_hip_detect_samples", nullptr, samples_xyz, num_samples, 0, 0, hands, cap, num_sets, num_candidates,
                    nullptr);
}

int gpd_hip_detect_select(gpd_hip_ctx *ctx, const int32_t *sample_indices, int num_samples, int num_selected, gpd_hand *hands,
                          int hands_capacity, int *num_sets, int *num_candidates, int *num_hands) {
  if (!sample_indices || !num_hands || hands_capacity < 0) {
    set_error("gpd_hip_detect_select: bad argument");
    return GPD_ERR_INVALID;
  }
  return detect_any(ctx, "gpd_hip_detect_select", sample_indices, nullptr, num_samples, 1, num_selected, hands, hands_capacity, num_sets,
                    num_candidates, num_hands);
}

int gpd_hip_label_view(gpd_hip_ctx *ctx, gpd_label_view_job *job) { return label_view_run(ctx, job, "gpd_hip_label_view", nullptr); }

int gpd_hip_detect_sis(gpd_hip_ctx *ctx, gpd_sis_job *job) {
  StageRange range_("gpd:detect_sis");
  if (!ctx || !job) {
    set_error("gpd_hip_detect_sis: bad argument");
    return GPD_ERR_INVALID;
  }
  gpd_sis_job &j = *job;
  j.num_hands = j.rounds_run = j.num_sets = j.num_candidates = 0;
  j.d2h_bytes = 0;
  for (float &m : j.stage_ms) m = 0.f;
  const long long all_samples = (long long)j.num_iterations * j.num_samples;
  bool ws_ok = true;
  for (double w : j.workspace) ws_ok = ws_ok && w == w;
  if (j.num_init_samples < 0 || j.num_iterations < 0 || j.capacity < 0 || j.centres_capacity < 0 || j.proposal_block < 0 ||
      (j.num_init_samples > 0 && !j.sample_indices) || (j.num_iterations > 0 && j.num_samples < 1) ||
      !(j.prob_rand_samples >= 0.0 && j.prob_rand_samples <= 1.0) || !(j.sigma > 0.0) || (j.sampling_method != 0 && j.sampling_method != 1) ||
      (j.capacity > 0 && !j.hands) || !ws_ok || !(j.min_score == j.min_score) || j.num_iterations >= (1 << 24) ||
      (j.num_iterations > 0 && (all_samples > 0x7fffffffll / 3 || j.num_samples > (1 << 28)))) {
    set_error("gpd_hip_detect_sis: bad argument");
    return GPD_ERR_INVALID;
  }
  if (ctx->in_batch) {
    set_error("gpd_hip_detect_sis: gpd_hip_detect_batch is driving the lanes");
    return GPD_ERR_STATE;
  }
  if (!ctx->lenet.channels) {
    set_error("gpd_hip_detect_sis: LeNet weights not set");
    return GPD_ERR_STATE;
  }
  Lane &L = ctx->lane[0];
  SisState &ss = ctx->sis;
  if (!L.cloud.num_points) {
    set_error("gpd_hip_detect_sis: no cloud uploaded");
    return GPD_ERR_STATE;
  }
  int rc = check_samples("gpd_hip_detect_sis", j.sample_indices, nullptr, j.num_init_samples, L.cloud.num_points);
  if (rc) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  rc = sis_init(ss);
  if (rc) return rc;
  const gpd_params &p = ctx->params;
  const size_t image_bytes = (size_t)kPix * p.image_num_channels;
  const bool rounds = j.num_iterations > 0;
  const int num_rand = rounds ? sis::num_rand_samples(j.prob_rand_samples, j.num_samples) : 0;
  const int num_gauss = rounds ? j.num_samples - num_rand : 0;
  // proposals per stream and block.  With proposal_block = 0 a block is sized to fill what is missing at the acceptance rate seen so
  // far (a round's first block: the last round's), with a margin: a block that falls short costs the round a second search.  The
  // result does not depend on the block sizes.
  const int block_max = 1 << 22;
  int block = j.proposal_block > 0 ? j.proposal_block : (int)std::min<long long>(2ll * j.num_samples + 64, block_max);
  double rate_g = 1.0, rate_u = 1.0;
  auto sized = [&](int missing, double rate) {
    if (j.proposal_block > 0) return j.proposal_block;
    return (int)std::min<double>((double)missing / std::max(rate, 1.0 / 256) * 1.25 + 64.0, (double)block_max);
  };
  constexpr int kMaxProposals = 1 << 20;  // of one stream in one round: a draw that has not filled its list by then never will
  rc = sis_reserve_round(ss, rounds ? (size_t)j.num_samples : 0, j.samples_out ? (size_t)all_samples : 0, (size_t)j.num_init_samples,
                         rounds ? (size_t)block : 0);
  if (rc) return rc;
  if (rounds && j.num_init_samples > 0)
    HIP_RET(hipMemcpyAsync(ss.d_uniform, j.sample_indices, (size_t)j.num_init_samples * sizeof(int32_t), hipMemcpyHostToDevice, L.stream));
  HIP_RET(hipMemsetAsync(ss.d_meta, 0, sizeof(SisMeta), L.stream));
  *ss.h_meta = SisMeta();
  if (j.round_counts) std::memset(j.round_counts, 0, (size_t)(1 + j.num_iterations) * 4 * sizeof(int32_t));
  ss.grows = 0;
  long long d2h = 0;
  size_t acc = 0;               // candidates accumulated
  int centres = 0;              // live hand sets accumulated
  unsigned long long lcg = 0;   // shadow draws of the rounds so far: the collected list sits in ONE stream (:167)
  bool img_pending = false;     // the image events of the last round have not been read yet
  auto book_images = [&]() {
    float ms = 0.f;
    if (img_pending && hipEventElapsedTime(&ms, L.ev[4], ss.ev[2]) == hipSuccess) j.stage_ms[2] += ms;
    img_pending = false;
  };
  int pass = 0;
  for (; pass <= j.num_iterations; pass++) {
    if (pass > 0 && centres == 0) break;  // the reference returns nothing after an initial pass without hand sets (:79-82)
    const int r = pass - 1;
    Job J;
    J.mode = 1;
    J.lcg_base = lcg;
    if (pass == 0) {
      J.sample_idx = j.sample_indices;
      J.S = j.num_init_samples;
    } else {
      J.S = j.num_samples;
      J.resident = true;
      J.gather.d_xyz = ss.d_round_xyz;
    }
    sample::Stream sg(sis::stream_seed(j.seed, r < 0 ? 0 : r, 0)), su(sis::stream_seed(j.seed, r < 0 ? 0 : r, 1));
    for (bool first = true;; first = false) {  // the draw and the search; redone from the draw when the proposal blocks fell short
      if (pass > 0) {
        if (first) HIP_RET(hipMemsetAsync(ss.d_meta, 0, 4 * sizeof(int32_t), L.stream));  // the round's draw counts
        const SisMeta left = first ? SisMeta() : *ss.h_meta;
        if (!first) {
          if (left.used_g > 0) rate_g = (double)left.acc_g / left.used_g;
          if (left.used_u > 0) rate_u = (double)left.acc_u / left.used_u;
        }
        const int n_g = left.acc_g < num_gauss ? sized(num_gauss - left.acc_g, rate_g) : 0;
        const int n_u = left.acc_u < num_rand ? sized(num_rand - left.acc_u, rate_u) : 0;
        if (std::max(n_g, n_u) > block) {  // (nothing of the call is in flight on the buffers: the last wait is behind us)
          block = std::max(n_g, n_u);
          rc = sis_reserve_round(ss, (size_t)j.num_samples, j.samples_out ? (size_t)all_samples : 0, (size_t)j.num_init_samples, (size_t)block);
          if (rc) return rc;
        }
        if ((n_g && left.used_g > kMaxProposals) || (n_u && left.used_u > kMaxProposals)) {
          set_error("gpd_hip_detect_sis: round %d: %d Gaussian and %d uniform proposals gave %d of %d and %d of %d samples", r, left.used_g,
                    left.used_u, left.acc_g, num_gauss, left.acc_u, num_rand);
          return GPD_ERR_CAPACITY;
        }
        sis::Proposal *hg = reinterpret_cast<sis::Proposal *>(ss.h_block);
        uint64_t *hu = reinterpret_cast<uint64_t *>(ss.h_block + ss.cap_block * sizeof(sis::Proposal));
        for (int i = 0; i < n_g; i++) hg[i] = sis::next_gauss(sg, j.sigma);
        for (int i = 0; i < n_u; i++) hu[i] = su.next();
        HIP_RET(hipEventRecord(ss.ev[0], L.stream));
        rc = sis_draw(ss, L.cloud, centres, n_g, n_u, j.num_init_samples, j.workspace, j.sampling_method, num_gauss, num_rand, L.stream);
        if (rc) return rc;
        HIP_RET(hipEventRecord(ss.ev[1], L.stream));
      }
      rc = job_begin(ctx, L, J);
      if (rc) return rc;
      if (!J.live) break;  // an initial pass without samples
      const int cap_before = L.search.nn_cap;
      rc = job_wait_plan(ctx, L, J);  // the round's one wait: plan summary, draw counts, capacity flags
      if (rc) return rc;
      d2h += (long long)sizeof(PlanSummary) * (L.search.nn_cap != cap_before ? 2 : 1) + (pass > 0 ? (long long)sizeof(SisMeta) : 0);
      book_images();
      float ms = 0.f;
      (void)hipEventElapsedTime(&ms, L.ev[0], L.ev[1]);
      j.stage_ms[1] += ms;
      if (pass > 0) {
        (void)hipEventElapsedTime(&ms, ss.ev[0], ss.ev[1]);
        j.stage_ms[0] += ms;
      }
      if (ss.h_meta->img_status) {
        set_images_status_error(ss.h_meta->img_status);
        return GPD_ERR_CAPACITY;
      }
      if (pass == 0) break;
      if (ss.h_meta->acc_g >= num_gauss && ss.h_meta->acc_u >= num_rand) {
        if (ss.h_meta->used_g > 0) rate_g = (double)num_gauss / ss.h_meta->used_g;
        if (ss.h_meta->used_u > 0) rate_u = (double)num_rand / ss.h_meta->used_u;
        break;
      }
    }
    if (!J.live) continue;
    const PlanSummary sm = *L.plan.h_summary;
    const int n = sm.num_candidates;
    if (n > 0) {
      HIP_RET(hipEventRecord(L.ev[4], L.stream));
      L.images.side_stream = true;
      L.images.lcg_base = lcg;
      {
        StageRange r_("gpd:images (detect_sis round)");
        rc = images_run(p, L.cloud, L.search, L.plan, L.images, L.stream);
      }
      if (rc) return rc;
      HIP_RET(hipEventRecord(L.ev[2], L.stream));
      // the round joins the accumulators: images as the LeNet reads them, records as detect_select(0) returns them
      rc = sis_reserve(ss, acc + (size_t)n, acc, (size_t)centres + (size_t)sm.live_sets, (size_t)centres, image_bytes, L.stream);
      if (rc) return rc;
      HIP_RET(hipMemcpyAsync(ss.d_images + acc * image_bytes, L.images.d_images, (size_t)n * image_bytes, hipMemcpyDeviceToDevice, L.stream));
      rc = plan_emit_hands(p, L.search, L.plan, nullptr, ss.d_hands + acc, true, L.stream);
      if (rc) return rc;
      rc = sis_accumulate(ss, acc, n, centres, L.images.d_status, L.stream);
      if (rc) return rc;
      HIP_RET(hipEventRecord(ss.ev[2], L.stream));
      img_pending = true;
    } else {
      L.images.num_candidates = 0;  // no candidate list of this round is resident
    }
    if (pass > 0 && j.samples_out)
      HIP_RET(hipMemcpyAsync(ss.d_samples + (size_t)r * j.num_samples * 3, ss.d_round_xyz, (size_t)j.num_samples * 3 * sizeof(double),
                             hipMemcpyDeviceToDevice, L.stream));
    if (j.round_counts) {
      int32_t *rcnt = j.round_counts + 4 * (size_t)pass;
      rcnt[0] = sm.live_sets;
      rcnt[1] = n;
      rcnt[2] = pass > 0 ? ss.h_meta->used_g : 0;
      rcnt[3] = pass > 0 ? ss.h_meta->used_u : 0;
    }
    lcg += J.lcg_draws;
    centres += sm.live_sets;
    acc += (size_t)n;
    if (acc > 0x7fffffffull) {
      set_error("gpd_hip_detect_sis: more than 2^31 accumulated candidates");
      return GPD_ERR_CAPACITY;
    }
  }
  const int rounds_run = pass > 0 ? pass - 1 : 0;
  const int N = (int)acc;
  // classify everything at once (:164-167), cut at min_score, cluster (:175-181)
  HIP_RET(hipEventRecord(ss.ev[3], L.stream));
  L.h_flags->lenet = 0;
  if (N > 0) {
    rc = reserve_scores(L, N);
    if (rc) return rc;
    {
      StageRange r_("gpd:lenet (detect_sis: every accumulated image)");
      HIP_RET(lenet_forward(ctx->lenet, L.lenet_scratch, ss.d_images, N, L.d_scores, L.stream));
    }
    HIP_RET(hipMemcpyAsync(&L.h_flags->lenet, L.lenet_scratch.c1_stats + 2, sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
    rc = sis_select(ss, L.d_scores, N, j.min_score, L.stream);
    if (rc) return rc;
  }
  HIP_RET(hipMemcpyAsync(ss.h_meta, ss.d_meta, sizeof(SisMeta), hipMemcpyDeviceToHost, L.stream));
  HIP_RET(hipEventRecord(ss.ev[5], L.stream));
  HIP_RET(hipEventSynchronize(ss.ev[5]));
  d2h += (long long)sizeof(SisMeta) + (N > 0 ? 4 : 0);
  book_images();
  if (ss.h_meta->img_status) {
    set_images_status_error(ss.h_meta->img_status);
    return GPD_ERR_CAPACITY;
  }
  if (L.h_flags->lenet) {
    rc = lenet_check(L.lenet_scratch);  // clears the device word, sets the error text
    return rc ? rc : GPD_ERR_HIP;
  }
  if (ss.h_meta->centres != centres || ss.h_meta->candidates != N) {
    set_error("gpd_hip_detect_sis: the accumulated records form %d hand sets of %d candidates, the plans counted %d of %d", ss.h_meta->centres,
              ss.h_meta->candidates, centres, N);
    return GPD_ERR_STATE;
  }
  int k = N > 0 ? ss.h_meta->kept : 0;
  const gpd_hand *d_res = ss.d_keep;
  if (j.min_inliers > 0 && k > 0) {
    StageRange r_("gpd:find_clusters (detect_sis)");
    rc = cluster_run_resident(ctx->cluster, ss.d_keep, k, j.min_inliers, j.remove_inliers, L.stream);
    if (rc) return rc;
    HIP_RET(hipMemcpyAsync(&ss.h_meta->kept, ctx->cluster.d_num, sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
    HIP_RET(hipStreamSynchronize(L.stream));
    d2h += 4;
    k = ss.h_meta->kept;
    d_res = ctx->cluster.d_out;
  }
  j.num_hands = k;
  j.rounds_run = rounds_run;
  j.num_sets = centres;
  j.num_candidates = N;
  if (k > j.capacity) {
    set_error("gpd_hip_detect_sis: %d hand records to return, the caller's buffer holds %d", k, j.capacity);
    return GPD_ERR_CAPACITY;
  }
  if (j.centres_out && centres > j.centres_capacity) {
    set_error("gpd_hip_detect_sis: %d live centres, centres_out holds %d", centres, j.centres_capacity);
    return GPD_ERR_CAPACITY;
  }
  const size_t b_rec = (size_t)k * sizeof(gpd_hand);
  const size_t b_smp = j.samples_out ? (size_t)rounds_run * j.num_samples * 3 * sizeof(double) : 0;
  const size_t b_cen = j.centres_out ? (size_t)centres * 3 * sizeof(double) : 0;
  if (b_rec + b_smp + b_cen > 0) {
    rc = grow_pinned(ss.h_out, ss.h_out_bytes, b_rec + b_smp + b_cen, slack_cap(b_rec + b_smp + b_cen, 8), __func__);
    if (rc) return rc;
    if (b_rec) HIP_RET(hipMemcpyAsync(ss.h_out, d_res, b_rec, hipMemcpyDeviceToHost, L.stream));  // the result: one copy
    if (b_smp) HIP_RET(hipMemcpyAsync(ss.h_out + b_rec, ss.d_samples, b_smp, hipMemcpyDeviceToHost, L.stream));
    if (b_cen) HIP_RET(hipMemcpyAsync(ss.h_out + b_rec + b_smp, ss.d_centres, b_cen, hipMemcpyDeviceToHost, L.stream));
  }
  HIP_RET(hipEventRecord(ss.ev[4], L.stream));
  HIP_RET(hipEventSynchronize(ss.ev[4]));
  (void)hipEventElapsedTime(&j.stage_ms[3], ss.ev[3], ss.ev[4]);
  d2h += (long long)(b_rec + b_smp + b_cen);
  if (b_rec) std::memcpy(j.hands, ss.h_out, b_rec);
  if (b_smp) std::memcpy(j.samples_out, ss.h_out + b_rec, b_smp);
  if (b_cen) std::memcpy(j.centres_out, ss.h_out + b_rec + b_smp, b_cen);
  j.d2h_bytes = d2h;
  return GPD_OK;
}

}  // extern "C"
