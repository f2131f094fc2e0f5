// gpd_hip_images_given / gpd_hip_score_given: images and scores of hand sets the CALLER supplies
// (ImageGenerator::createImages(cloud, hand_set_list), image_generator.cpp:17-99, images whatever it is handed), and
// gpd_hip_given_check, the definition of what may be supplied (given_model.h).
//
// The route: neighbourhood lists around the sets' samples (given_lists_run, search.hip — the search's own kernel and capacity
// retry; no frame is used and no hand evaluated), the caller's records copied to where the image kernels read a candidate's
// record (SearchState::d_hands, [set][slot]: cand_hand = s * slots + j), given_ingest_kernel, and from there the stages of
// gpd_hip_images as they are: plan_kernel, the image kernels, the LeNet.
#include <cstring>
#include <vector>

#include "context.h"
#include "buffers.h"
#include "given_model.h"

namespace gpd {

// The records are in d_hands already.  What plan_kernel reads beside them: the validity flags, [set][slot] bytes, and whether a
// sample is a hand set at all — k_frames > 0 in the counts word, which for the search means "has a frame"; here every listed
// sample is a set (createImages estimates no frame), so the word is set.  The set's sample, which shadow_set_kernel takes from
// d_frames, is written as well: it is slot 0's, whatever the neighbourhood kernel did for a sample without a frame.
// (centre_kernel reads other words of d_counts, and given_lists_run has joined it.)
__global__ __launch_bounds__(256) void given_ingest_kernel(const gpd_hand *__restrict__ hands, int S, int slots, uint8_t *__restrict__ fvalid,
                                                           int32_t *__restrict__ counts, double *__restrict__ frames) {
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= S * slots) return;
  fvalid[h] = hands[h].valid ? 1 : 0;
  const int s = h / slots;
  if (h == s * slots) {
    counts[8 * (size_t)s + 2] = 1;
    for (int r = 0; r < 3; r++) frames[12 * (size_t)s + r] = hands[h].sample[r];
  }
}

int given_ingest(SearchState &s, const gpd_hand *hands, int S, int slots, hipStream_t stream) {
  if (S > s.capacity_samples) {
    set_error("given hands: %d sets, the lists hold %d", S, s.capacity_samples);
    return GPD_ERR_STATE;
  }
  const size_t n = (size_t)S * slots;
  HIP_RET(hipMemcpyAsync(s.d_hands, hands, n * sizeof(gpd_hand), hipMemcpyHostToDevice, stream));
  given_ingest_kernel<<<(unsigned)((n + 255) / 256), 256, 0, stream>>>(s.d_hands, S, slots, s.d_fvalid, s.d_counts, s.d_frames);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

// the body of both entries; with_scores: the LeNet pass behind the images, scores [n] and cand [n] on the host
static int given_run(gpd_hip_ctx *ctx, const char *who, const gpd_hand *hands, int num_sets, uint64_t lcg_base, uint8_t *images,
                     int32_t *cand_index, int *num_candidates, uint64_t *lcg_draws, float *scores) {
  const bool args_ok = num_sets >= 0 && (num_sets == 0 || hands) && num_candidates;
  int rc = scores ? refuse(who, ctx, args_ok, {Need::Cloud, Need::LeNet}) : refuse(who, ctx, args_ok, {Need::Cloud});
  if (rc) return rc;
  Lane &L = ctx->lane[0];
  {
    int bad_set = -1, bad_slot = -1;
    char msg[256];
    if (given::check(ctx->params, hands, num_sets, &bad_set, &bad_slot, msg, sizeof(msg))) {
      set_error("%s: %s", who, msg);
      return GPD_ERR_INVALID;
    }
  }
  *num_candidates = 0;
  if (lcg_draws) *lcg_draws = 0;
  HIP_RET(hipSetDevice(ctx->device));
  SearchState &s = L.search;
  const gpd_params &p = ctx->params;
  const int slots = p.num_hand_axes * p.num_orientations;
  L.images.num_candidates = 0;  // the search buffers the resident candidate list points into are reused
  s.num_samples = 0;
  if (num_sets == 0) return GPD_OK;
  std::vector<double> xyz((size_t)num_sets * 3);
  for (int i = 0; i < num_sets; i++)
    for (int r = 0; r < 3; r++) xyz[3 * (size_t)i + r] = hands[(size_t)i * slots].sample[r];
  HIP_RET(hipEventRecord(L.ev[0], L.stream));
  rc = given_lists_run(p, L.cloud, s, xyz.data(), num_sets, L.stream);
  if (rc) return rc;
  rc = given_ingest(s, hands, num_sets, slots, L.stream);
  if (rc) return rc;
  s.num_samples = num_sets;  // for the plan alone ...
  rc = plan_build(p, L.cloud, s, L.plan, L.stream);
  s.num_samples = 0;         // ... these lists have no search behind them (gpd_hip_images, gpd_hip_replay refuse)
  if (rc) return rc;
  HIP_RET(hipStreamSynchronize(L.stream));  // `hands` is pageable: its copy has left it by now as well
  // ev[0] stands ahead of the lists: stage_ms[1] is lists + plan + images
  rc = lane_images(ctx, L, /*side_stream=*/true, lcg_base, "gpd:images (given hand sets)", nullptr, L.ev[1]);
  if (rc) return rc;
  const int n = L.images.num_candidates;
  rc = lane_download_images(p, L, n, images, cand_index);
  if (rc) return rc;
  const bool scored = scores && n > 0;
  if (scored) {
    HIP_RET(hipEventRecord(L.ev[2], L.stream));
    rc = lane_lenet(ctx, L, L.images.d_images, n, "gpd:lenet (given hand sets)");
    if (rc) return rc;
    HIP_RET(hipEventRecord(L.ev[3], L.stream));
    HIP_RET(hipMemcpyAsync(scores, L.d_scores, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, L.stream));
  }
  HIP_RET(hipMemcpyAsync(&L.h_flags->status, L.images.d_status, sizeof(int32_t), hipMemcpyDeviceToHost, L.stream));
  HIP_RET(hipStreamSynchronize(L.stream));
  HIP_RET(hipEventElapsedTime(&L.stage_ms[1], L.ev[0], L.ev[1]));
  if (scored) HIP_RET(hipEventElapsedTime(&L.stage_ms[2], L.ev[2], L.ev[3]));
  rc = lane_check(L, L.h_flags->status, scored);
  if (rc) return rc;
  *num_candidates = n;
  if (lcg_draws) *lcg_draws = L.plan.h_summary->total_draws;
  return GPD_OK;
}

}  // namespace gpd

using namespace gpd;

extern "C" {

int gpd_hip_given_check(const gpd_params *params, const gpd_hand *hands, int num_sets, int *bad_set, int *bad_slot) {
  int bs = -1, bj = -1;
  if (bad_set) *bad_set = -1;
  if (bad_slot) *bad_slot = -1;
  if (!params || num_sets < 0 || (num_sets > 0 && !hands)) {
    set_error("gpd_hip_given_check: bad argument");
    return GPD_ERR_INVALID;
  }
  char msg[256];
  const int rc = given::check(*params, hands, num_sets, &bs, &bj, msg, sizeof(msg));
  if (bad_set) *bad_set = bs;
  if (bad_slot) *bad_slot = bj;
  if (rc) set_error("gpd_hip_given_check: %s", msg);
  return rc;
}

int gpd_hip_images_given(gpd_hip_ctx *ctx, const gpd_hand *hands, int num_sets, uint64_t lcg_base, uint8_t *images,
                         int32_t *cand_index, int *num_candidates, uint64_t *lcg_draws) {
  StageRange range_("gpd:images_given");
  return given_run(ctx, "gpd_hip_images_given", hands, num_sets, lcg_base, images, cand_index, num_candidates, lcg_draws, nullptr);
}

int gpd_hip_score_given(gpd_hip_ctx *ctx, gpd_hand *hands, int num_sets, uint64_t lcg_base, float *scores, int32_t *cand_index,
                        int *num_candidates, uint64_t *lcg_draws) {
  StageRange range_("gpd:score_given");
  if (int rc = refuse("gpd_hip_score_given", ctx, num_sets >= 0 && num_candidates)) return rc;
  // one score and one index per candidate come back (the caller holds the records): room for every valid hand
  const int slots = ctx->params.num_hand_axes * ctx->params.num_orientations;
  size_t nv = 0;
  if (hands)
    for (size_t h = 0; h < (size_t)num_sets * slots; h++) nv += hands[h].valid ? 1 : 0;
  std::vector<float> sc(nv + 1);
  std::vector<int32_t> ci(nv + 1);
  const int rc = given_run(ctx, "gpd_hip_score_given", hands, num_sets, lcg_base, nullptr, ci.data(), num_candidates, lcg_draws, sc.data());
  if (rc) return rc;
  const int n = *num_candidates;
  for (int i = 0; i < n; i++) hands[ci[(size_t)i]].score = sc[(size_t)i];
  if (scores && n > 0) std::memcpy(scores, sc.data(), (size_t)n * sizeof(float));
  if (cand_index && n > 0) std::memcpy(cand_index, ci.data(), (size_t)n * sizeof(int32_t));
  return GPD_OK;
}

}  // extern "C"
