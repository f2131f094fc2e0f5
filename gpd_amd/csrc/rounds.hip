// C-ABI of libgpd_hip.so (include/gpd_hip.h): the entries that accumulate ROUNDS of a fused detect's first step and a half
// (detect.hip: job_begin, job_wait_plan, then the image stage) — gpd_hip_label_view, whose rounds end in the ground-truth labels of
// their candidates and whose tail is the balanced selection (label.hip), and gpd_hip_detect_sis, whose rounds sit behind a draw on
// the device (sis.hip), with one LeNet pass over everything at the end.  Both run on lane 0.
#include <algorithm>
#include <cstring>

#include "context.h"
#include "buffers.h"
#include "balance_model.h"
#include "sis_model.h"

using namespace gpd;

namespace gpd {

// What a round of either entry is up to its candidate count: the search and the plan of J, the wait for the plan summary (a
// list-capacity retry brings a second one), and the books — the summaries into d2h, the search kernels' time into search_ms.
// J.live is false afterwards when the round has no samples: nothing was enqueued, and sm is not written.
static int round_plan(gpd_hip_ctx *ctx, Lane &L, Job &J, PlanSummary &sm, long long &d2h, float &search_ms) {
  int rc = job_begin(ctx, L, J);
  if (rc || !J.live) return rc;
  const int cap_before = L.search.nn_cap;
  rc = job_wait_plan(ctx, L, J);
  if (rc) return rc;
  d2h += (long long)sizeof(PlanSummary) * (L.search.nn_cap != cap_before ? 2 : 1);
  float ms = 0.f;
  (void)hipEventElapsedTime(&ms, L.ev[0], L.ev[1]);
  search_ms += ms;
  sm = *L.plan.h_summary;
  return GPD_OK;
}

// gpd_hip_label_view, and gpd_hip_train_append_view through a sink (train_sets.hip): the rounds and the selection are one code
int label_view_run(gpd_hip_ctx *ctx, gpd_label_view_job *job, const char *who, const LabelSink *sink) {
  StageRange range_("gpd:label_view");
  int rc = refuse(who, ctx, job);
  if (rc) return rc;
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
  rc = refuse(who, ctx, true, {Need::Cloud});
  if (rc) return rc;
  Lane &L = ctx->lane[0];
  LabelState &ls = ctx->label;
  if (!ls.gt.num_points) {
    set_error("%s: no ground truth uploaded (gpd_hip_upload_ground_truth)", who);
    return GPD_ERR_STATE;
  }
  rc = check_samples(who, j.sample_indices, nullptr, (int)total_samples, L.cloud.num_points);
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
    PlanSummary sm;
    rc = round_plan(ctx, L, J, sm, d2h, j.stage_ms[0]);
    if (rc) return rc;
    if (!J.live) continue;  // a round without samples
    const int n = sm.num_candidates;
    int round_pos = 0;
    if (n > 0) {
      // every round is an ordinary call: its shadow stream starts at 0
      rc = lane_images(ctx, L, /*side_stream=*/true, /*lcg_base=*/0, "gpd:images (label_view round)", L.ev[4], L.ev[2]);
      if (rc) return rc;
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
      float ms = 0.f;
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

int gpd_hip_label_view(gpd_hip_ctx *ctx, gpd_label_view_job *job) { return label_view_run(ctx, job, "gpd_hip_label_view", nullptr); }

int gpd_hip_detect_sis(gpd_hip_ctx *ctx, gpd_sis_job *job) {
  StageRange range_("gpd:detect_sis");
  int rc = refuse("gpd_hip_detect_sis", ctx, job);
  if (rc) return rc;
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
  rc = refuse("gpd_hip_detect_sis", ctx, true, {Need::NoBatch, Need::LeNet, Need::Cloud});
  if (rc) return rc;
  Lane &L = ctx->lane[0];
  SisState &ss = ctx->sis;
  rc = check_samples("gpd_hip_detect_sis", j.sample_indices, nullptr, j.num_init_samples, L.cloud.num_points);
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
    PlanSummary sm;
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
      rc = round_plan(ctx, L, J, sm, d2h, j.stage_ms[1]);  // the round's one wait: plan summary, draw counts, capacity flags
      if (rc) return rc;
      if (!J.live) break;  // an initial pass without samples
      book_images();
      if (pass > 0) {
        d2h += (long long)sizeof(SisMeta);
        float ms = 0.f;
        (void)hipEventElapsedTime(&ms, ss.ev[0], ss.ev[1]);
        j.stage_ms[0] += ms;
      }
      rc = lane_check(L, ss.h_meta->img_status, /*scored=*/false);
      if (rc) return rc;
      if (pass == 0) break;
      if (ss.h_meta->acc_g >= num_gauss && ss.h_meta->acc_u >= num_rand) {
        if (ss.h_meta->used_g > 0) rate_g = (double)num_gauss / ss.h_meta->used_g;
        if (ss.h_meta->used_u > 0) rate_u = (double)num_rand / ss.h_meta->used_u;
        break;
      }
    }
    if (!J.live) continue;
    const int n = sm.num_candidates;
    if (n > 0) {
      rc = lane_images(ctx, L, /*side_stream=*/true, lcg, "gpd:images (detect_sis round)", L.ev[4], L.ev[2]);
      if (rc) return rc;
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
  rc = lane_lenet(ctx, L, ss.d_images, N, "gpd:lenet (detect_sis: every accumulated image)");
  if (rc) return rc;
  if (N > 0) {
    rc = sis_select(ss, L.d_scores, N, j.min_score, L.stream);
    if (rc) return rc;
  }
  HIP_RET(hipMemcpyAsync(ss.h_meta, ss.d_meta, sizeof(SisMeta), hipMemcpyDeviceToHost, L.stream));
  HIP_RET(hipEventRecord(ss.ev[5], L.stream));
  HIP_RET(hipEventSynchronize(ss.ev[5]));
  d2h += (long long)sizeof(SisMeta) + (N > 0 ? 4 : 0);
  book_images();
  rc = lane_check(L, ss.h_meta->img_status, /*scored=*/true);
  if (rc) return rc;
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
