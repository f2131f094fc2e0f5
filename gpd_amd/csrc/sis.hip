// gpd_hip_detect_sis's own device state (SequentialImportanceSampling::detectGrasps, sequential_importance_sampling.cpp:54-187, keeps
// hand_set_list on the host and draws on one core): the draw of a round's samples from proposal blocks of the host
// (sis_draw_kernel; the definition of the rule is sis_model.h), the accumulators of the rounds' live centres, candidate records
// and images (sis_accumulate_kernel), and the cut at min_score over the accumulated records (sis_select_kernel).  The round loop
// itself is gpd_hip_detect_sis in detect.hip.
#include "gpd_internal.h"
#include "buffers.h"

#include <algorithm>

#include "sis_model.h"

namespace gpd {

namespace {

constexpr int DRAW_T = kSisDrawThreads;
constexpr int TILE = kSisCentreTile;
constexpr size_t kSisAccBudget = 16ull << 30;

struct DrawParams {
  const double *centres;  // [L][3]
  int L;
  const sis::Proposal *gauss;  // the block in flight
  int n_gauss;
  const unsigned long long *unif;
  int n_unif;
  const int32_t *list;  // uniform source (null: every point)
  int n_list;
  const float *px, *py, *pz;
  int num_points;
  double ws[6];
  int method, num_gauss, num_rand;
  double *out;  // [num_gauss + num_rand][3]: where the search reads the round's samples
  SisMeta *meta;
};

// ranks of the lanes with `ok` among the workgroup's, in thread order; *total: how many there are.  Two barriers.
__device__ inline int block_rank(bool ok, int *s_cnt, int *total) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long mask = __ballot(ok);
  if (lane == 0) s_cnt[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, t = 0;
  for (int w = 0; w < DRAW_T / 64; w++) {
    before += w < wave ? s_cnt[w] : 0;
    t += s_cnt[w];
  }
  __syncthreads();
  *total = t;
  return before + __popcll(mask & ((1ull << lane) - 1ull));
}

// The selection rule of sis_model.h over one block of each stream, continuing from the counts in meta.  One workgroup: a lane
// takes one proposal of a step of DRAW_T; under method 1 the centres pass through LDS in tiles of TILE (every lane reads the
// same centre: a broadcast), the accepted proposals of a step are ranked by ballot + popcount and written in proposal order.
// The loops stop where the sequential loops of the reference stop: behind the proposal that fills the list.
__global__ __launch_bounds__(DRAW_T) void sis_draw_kernel(DrawParams P) {
  __shared__ double s_c[3 * TILE];
  __shared__ int s_cnt[DRAW_T / 64];
  __shared__ int s_fill;
  const int tid = threadIdx.x;
  int acc = P.meta->acc_g, used = P.meta->used_g;
  for (int base = 0; base < P.n_gauss && acc < P.num_gauss; base += DRAW_T) {
    const int i = base + tid;
    const bool in = i < P.n_gauss;
    double x[3] = {0.0, 0.0, 0.0}, own = 0.0;
    if (in) {
      const int idx = sis::gauss_point(P.centres, P.L, P.gauss[i], x);
      own = sis::d2(x, P.centres + 3 * (size_t)idx);
    }
    bool ok = in;
    if (P.method == 1) {
      for (int t0 = 0; t0 < P.L; t0 += TILE) {
        const int m = min(TILE, P.L - t0);
        __syncthreads();
        for (int k = tid; k < 3 * m; k += DRAW_T) s_c[k] = P.centres[3 * (size_t)t0 + k];
        __syncthreads();
        if (ok)
          for (int k = 0; k < m; k++) ok = ok && !(sis::d2(x, s_c + 3 * k) < own);
      }
    }
    if (tid == 0) s_fill = 0;
    int total;
    const int rank = acc + block_rank(ok, s_cnt, &total);
    if (ok && rank < P.num_gauss) {
      for (int r = 0; r < 3; r++) P.out[3 * (size_t)rank + r] = x[r];
      if (rank == P.num_gauss - 1) s_fill = i - base + 1;
    }
    __syncthreads();
    if (acc + total >= P.num_gauss) {
      used += s_fill;
      acc = P.num_gauss;
    } else {
      used += min(DRAW_T, P.n_gauss - base);
      acc += total;
    }
    __syncthreads();
  }
  int acc_u = P.meta->acc_u, used_u = P.meta->used_u;
  for (int base = 0; base < P.n_unif && acc_u < P.num_rand; base += DRAW_T) {
    const int i = base + tid;
    bool ok = false;
    double s[3] = {0.0, 0.0, 0.0};
    if (i < P.n_unif) {
      const int pt = sis::uniform_point(P.unif[i], P.list, P.n_list, P.num_points);
      s[0] = (double)P.px[pt];
      s[1] = (double)P.py[pt];
      s[2] = (double)P.pz[pt];
      ok = sis::inside(s, P.ws);
    }
    if (tid == 0) s_fill = 0;
    int total;
    const int rank = acc_u + block_rank(ok, s_cnt, &total);
    if (ok && rank < P.num_rand) {
      for (int r = 0; r < 3; r++) P.out[3 * (size_t)(P.num_gauss + rank) + r] = s[r];
      if (rank == P.num_rand - 1) s_fill = i - base + 1;
    }
    __syncthreads();
    if (acc_u + total >= P.num_rand) {
      used_u += s_fill;
      acc_u = P.num_rand;
    } else {
      used_u += min(DRAW_T, P.n_unif - base);
      acc_u += total;
    }
    __syncthreads();
  }
  if (tid == 0) {
    P.meta->acc_g = acc;
    P.meta->used_g = used;
    P.meta->acc_u = acc_u;
    P.meta->used_u = used_u;
  }
}

// A round's n candidate records (set-major, set_index = the set's ordinal in the round's search): the sample of every set with
// a candidate joins the centre list behind the `centres_before` it holds, and set_index becomes the index in that list — what
// pruneGraspCandidates numbers the collected hand sets with.  One workgroup; ranks by ballot + popcount as label_sets_kernel.
__global__ __launch_bounds__(1024) void sis_accumulate_kernel(gpd_hand *__restrict__ recs, int n, int centres_before, double *__restrict__ centres,
                                                              const int32_t *__restrict__ img_status, SisMeta *__restrict__ meta) {
  __shared__ int s_w[16];
  __shared__ int s_last;  // set_index (as the search numbered it) of the record before this step's first
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int running = 0;
  if (tid == 0) s_last = -1;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const int own = i < n ? recs[i].set_index : -1;
    const int prev = i < n ? (tid == 0 ? s_last : recs[i - 1].set_index) : -1;
    const bool head = i < n && (i == 0 || own != prev);
    const unsigned long long mask = __ballot(head);
    if (lane == 0) s_w[wave] = __popcll(mask);
    __syncthreads();  // every set_index of the step has been read
    int before = running, total = 0;
    for (int w = 0; w < 16; w++) {
      before += w < wave ? s_w[w] : 0;
      total += s_w[w];
    }
    const int ord = before + __popcll(mask & ((1ull << lane) - 1ull)) + (head ? 1 : 0) - 1;
    if (i < n) recs[i].set_index = centres_before + ord;
    if (head)
      for (int r = 0; r < 3; r++) centres[3 * (size_t)(centres_before + ord) + r] = recs[i].sample[r];
    if (tid == 1023) s_last = own;
    running += total;
    __syncthreads();
  }
  if (tid == 0) {
    meta->centres = centres_before + running;
    meta->candidates += n;
    meta->img_status |= img_status[0];
  }
}

static_assert(sizeof(gpd_hand) == 176 && offsetof(gpd_hand, score) == 152, "sis_select_kernel moves records as 11 x 16 bytes");

// classify everything at once (:164-167), then the cut of pruneGraspCandidates: the score of every accumulated record is written
// back, the records with score > min_score are kept in order
__global__ __launch_bounds__(1024) void sis_select_kernel(gpd_hand *__restrict__ recs, const float *__restrict__ scores, int n, double min_score,
                                                          gpd_hand *__restrict__ keep, SisMeta *__restrict__ meta) {
  __shared__ int s_w[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int running = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    float sc = 0.f;
    bool ok = false;
    if (i < n) {
      sc = scores[i];
      recs[i].score = sc;
      ok = (double)sc > min_score;
    }
    const unsigned long long mask = __ballot(ok);
    if (lane == 0) s_w[wave] = __popcll(mask);
    __syncthreads();
    int before = running, total = 0;
    for (int w = 0; w < 16; w++) {
      before += w < wave ? s_w[w] : 0;
      total += s_w[w];
    }
    if (ok) {
      const int k = before + __popcll(mask & ((1ull << lane) - 1ull));
      const uint4 *src = reinterpret_cast<const uint4 *>(recs + i);
      uint4 *dst = reinterpret_cast<uint4 *>(keep + k);
#pragma unroll
      for (int piece = 0; piece < 11; piece++) {
        uint4 v = src[piece];
        if (piece == 9) v.z = __float_as_uint(sc);  // bytes 144..159: grasp_width, score, finger_placement_index
        dst[piece] = v;
      }
    }
    running += total;
    __syncthreads();
  }
  if (tid == 0) meta->kept = running;
}

// the draw's buffers and the accumulators grow by half, to 64 elements at the least
size_t half_more(size_t need) { return std::max(slack_cap(need, 2), (size_t)64); }

}  // namespace

void sis_free(SisState &ss) {
  device_release(ss.d_images, ss.d_hands, ss.d_keep, ss.d_centres, ss.d_round_xyz, ss.d_samples, ss.d_uniform, ss.d_gauss, ss.d_unif,
                 ss.d_meta);
  pinned_release(ss.h_block, ss.h_meta, ss.h_out);
  for (auto &e : ss.ev)
    if (e) (void)hipEventDestroy(e);
  ss = SisState();
}

int sis_init(SisState &ss) {
  if (ss.d_meta) return GPD_OK;
  HIP_RET(device_alloc(ss.d_meta, 1));
  HIP_RET(pinned_alloc(ss.h_meta, 1));
  for (auto &e : ss.ev) HIP_RET(hipEventCreate(&e));
  return GPD_OK;
}

int sis_reserve(SisState &ss, size_t need, size_t used, size_t centres, size_t used_centres, size_t image_bytes, hipStream_t stream) {
  int rc = grow_device_keep(ss.d_centres, ss.cap_centres, centres * 3, half_more(centres * 3), used_centres * 3, stream, __func__);
  if (rc) return rc;
  if (image_bytes != ss.image_bytes) {  // (a context has one channel count: only the first call comes here)
    used = 0;
    ss.cap = 0;
  }
  if (need <= ss.cap) return GPD_OK;
  const size_t per = image_bytes + 2 * sizeof(gpd_hand);
  if (need > kSisAccBudget / per) {
    set_error("detect_sis: %zu accumulated candidates of %zu bytes each exceed the accumulators' %zu GB", need, per, kSisAccBudget >> 30);
    return GPD_ERR_CAPACITY;
  }
  note_alloc(__func__);
  const size_t cap = std::min(half_more(need), kSisAccBudget / per);
  // the rounds so far move over (d_keep is rewritten by every selection)
  rc = grow_group_keep({group_buffer(ss.d_images, image_bytes, true), group_buffer(ss.d_hands, sizeof(gpd_hand), true),
                        group_buffer(ss.d_keep, sizeof(gpd_hand), false)},
                       cap, used, stream);
  if (rc) return rc;
  ss.cap = cap;
  ss.image_bytes = image_bytes;
  ss.grows++;
  return GPD_OK;
}

int sis_reserve_round(SisState &ss, size_t round_samples, size_t all_samples, size_t uniform, size_t block) {
  const size_t had_round = ss.cap_round;
  int rc = grow_device_keep(ss.d_round_xyz, ss.cap_round, round_samples * 3, half_more(round_samples * 3), 0, nullptr, __func__);
  if (rc) return rc;
  // a round whose draw falls short is searched as far as it is filled and then redone: the rest must be finite coordinates
  if (ss.cap_round != had_round) {
    HIP_RET(hipMemset(ss.d_round_xyz, 0, ss.cap_round * sizeof(double)));
    HIP_RET(hipDeviceSynchronize());  // (a growth: as rare as the hipMalloc before it)
  }
  rc = grow_device_keep(ss.d_samples, ss.cap_samples, all_samples * 3, half_more(all_samples * 3), 0, nullptr, __func__);
  if (rc) return rc;
  rc = grow_device_keep(ss.d_uniform, ss.cap_uniform, uniform, half_more(uniform), 0, nullptr, __func__);
  if (rc) return rc;
  if (block > ss.cap_block) {
    note_alloc(__func__);
    device_release(ss.d_gauss, ss.d_unif);
    pinned_release(ss.h_block);
    ss.cap_block = 0;
    HIP_RET(device_alloc(ss.d_gauss, block * sizeof(sis::Proposal)));
    HIP_RET(device_alloc(ss.d_unif, block));
    HIP_RET(pinned_alloc(ss.h_block, block * (sizeof(sis::Proposal) + sizeof(unsigned long long))));
    ss.cap_block = block;
  }
  return GPD_OK;
}

int sis_draw(SisState &ss, const Cloud &c, int L, int n_gauss, int n_unif, int n_uniform_list, const double ws[6], int method, int num_gauss,
             int num_rand, hipStream_t stream) {
  if ((size_t)std::max(n_gauss, n_unif) > ss.cap_block || (size_t)(num_gauss + num_rand) * 3 > ss.cap_round || (num_gauss > 0 && L < 1) ||
      (size_t)L * 3 > ss.cap_centres || (size_t)n_uniform_list > ss.cap_uniform) {
    set_error("detect_sis: a draw beyond the buffers reserved for it");
    return GPD_ERR_STATE;
  }
  const sis::Proposal *hg = reinterpret_cast<const sis::Proposal *>(ss.h_block);
  const unsigned long long *hu = reinterpret_cast<const unsigned long long *>(ss.h_block + ss.cap_block * sizeof(sis::Proposal));
  if (n_gauss > 0) HIP_RET(hipMemcpyAsync(ss.d_gauss, hg, (size_t)n_gauss * sizeof(sis::Proposal), hipMemcpyHostToDevice, stream));
  if (n_unif > 0) HIP_RET(hipMemcpyAsync(ss.d_unif, hu, (size_t)n_unif * sizeof(unsigned long long), hipMemcpyHostToDevice, stream));
  DrawParams P;
  P.centres = ss.d_centres;
  P.L = L;
  P.gauss = static_cast<const sis::Proposal *>(ss.d_gauss);
  P.n_gauss = n_gauss;
  P.unif = ss.d_unif;
  P.n_unif = n_unif;
  P.list = n_uniform_list > 0 ? ss.d_uniform : nullptr;
  P.n_list = n_uniform_list;
  P.px = c.px;
  P.py = c.py;
  P.pz = c.pz;
  P.num_points = c.num_points;
  for (int a = 0; a < 6; a++) P.ws[a] = ws[a];
  P.method = method;
  P.num_gauss = num_gauss;
  P.num_rand = num_rand;
  P.out = ss.d_round_xyz;
  P.meta = ss.d_meta;
  sis_draw_kernel<<<1, DRAW_T, 0, stream>>>(P);
  HIP_RET(hipGetLastError());
  HIP_RET(hipMemcpyAsync(ss.h_meta, ss.d_meta, sizeof(SisMeta), hipMemcpyDeviceToHost, stream));
  return GPD_OK;
}

int sis_accumulate(SisState &ss, size_t acc, int n, int centres_before, const int32_t *d_img_status, hipStream_t stream) {
  if (n <= 0) return GPD_OK;
  sis_accumulate_kernel<<<1, 1024, 0, stream>>>(ss.d_hands + acc, n, centres_before, ss.d_centres, d_img_status, ss.d_meta);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

int sis_select(SisState &ss, const float *d_scores, int n, double min_score, hipStream_t stream) {
  sis_select_kernel<<<1, 1024, 0, stream>>>(ss.d_hands, d_scores, n, min_score, ss.d_keep, ss.d_meta);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

}  // namespace gpd
