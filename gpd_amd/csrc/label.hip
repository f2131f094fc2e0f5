// gpd_hip_label_view's own device state: the accumulator of a view's labelled candidates (DataGenerator::generateData keeps
// images_view / labeled_grasps_view on the host, data_generator.cpp:121-192), DataGenerator::balanceInstances (:406-430) as a scan
// over the accumulated labels, and the gather of the kept instances into ONE contiguous block, so that what crosses PCIe at the
// end of a view is the kept set in one copy.  The ground-truth check itself (reevaluateHypotheses per hand set) is search.hip's
// label_round; the definition of the selection is balance_model.h.
#include "gpd_internal.h"
#include "buffers.h"

#include <algorithm>

namespace gpd {

namespace {

constexpr int SEL_T = 1024;

// sel[0 .. end) = the first `end` candidates with a label, sel[end .. 2 end) = the first `end` without, both ascending
// (balance::view).  One workgroup walks the labels 1024 at a time — ranks by ballot + popcount — and stops once both
// classes are full: the kept instances sit at the front of the list unless a class is rare.
__global__ __launch_bounds__(SEL_T) void balance_select_kernel(const uint8_t *__restrict__ labels, int n, int end, int32_t *__restrict__ sel) {
  __shared__ int s_p[SEL_T / 64], s_n[SEL_T / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int run_p = 0, run_n = 0;
  for (int base = 0; base < n && (run_p < end || run_n < end); base += SEL_T) {
    const int i = base + tid;
    const bool in = i < n;
    const bool pos = in && labels[i] != 0, neg = in && !pos;
    const unsigned long long mp = __ballot(pos), mn = __ballot(neg);
    if (lane == 0) {
      s_p[wave] = __popcll(mp);
      s_n[wave] = __popcll(mn);
    }
    __syncthreads();
    int bp = run_p, bn = run_n, tp = 0, tn = 0;
    for (int w = 0; w < SEL_T / 64; w++) {
      bp += w < wave ? s_p[w] : 0;
      bn += w < wave ? s_n[w] : 0;
      tp += s_p[w];
      tn += s_n[w];
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const int rp = bp + __popcll(mp & below), rn = bn + __popcll(mn & below);
    if (pos && rp < end) sel[rp] = i;
    if (neg && rn < end) sel[end + rn] = i;
    run_p += tp;
    run_n += tn;
    __syncthreads();
  }
}

struct GatherParams {
  const uint4 *images;   // accumulator, units of 16 bytes
  const uint4 *hands;
  const uint8_t *labels;
  const int32_t *sel;
  uint4 *out_images, *out_hands;
  int32_t *out_src;
  uint8_t *out_labels;
  int k;
  unsigned img_units;    // 16-byte units per image (3600 * C / 16)
  unsigned blocks_per;   // workgroups per instance
};
constexpr unsigned kHandUnits = sizeof(gpd_hand) / 16;
static_assert(sizeof(gpd_hand) % 16 == 0, "the gather copies records in 16-byte units");

// kept instance j = accumulator entry sel[j]: its image and its record move in 16-byte units (one per lane: dwordx4 loads and
// stores, whole lines), its label and index ride along on the first lane
__global__ __launch_bounds__(256) void label_gather_kernel(GatherParams P) {
  const unsigned j = blockIdx.x / P.blocks_per, b = blockIdx.x - j * P.blocks_per;
  const unsigned u = b * 256 + threadIdx.x;
  const size_t src = (size_t)P.sel[j];
  if (u < P.img_units) {
    P.out_images[(size_t)j * P.img_units + u] = P.images[src * P.img_units + u];
  } else if (u < P.img_units + kHandUnits) {
    const unsigned piece = u - P.img_units;
    P.out_hands[(size_t)j * kHandUnits + piece] = P.hands[src * kHandUnits + piece];
  }
  if (u == 0) {
    P.out_src[j] = (int32_t)src;
    P.out_labels[j] = P.labels[src];
  }
}

// the same into a caller's pool: images and labels only, destination offsets in 64 bits
__global__ __launch_bounds__(256) void label_gather_sink_kernel(const uint4 *__restrict__ images, const uint8_t *__restrict__ labels,
                                                                const int32_t *__restrict__ sel, uint4 *__restrict__ out_images,
                                                                uint8_t *__restrict__ out_labels, unsigned img_units, unsigned blocks_per) {
  const unsigned j = blockIdx.x / blocks_per, b = blockIdx.x - j * blocks_per;
  const unsigned u = b * 256 + threadIdx.x;
  const size_t src = (size_t)sel[j];
  if (u < img_units) out_images[(size_t)j * img_units + u] = images[src * img_units + u];
  if (u == 0) out_labels[j] = labels[src];
}

}  // namespace

void label_free(LabelState &ls) {
  cloud_free(ls.gt);
  search_free(ls.gt_search);
  device_release(ls.d_images, ls.d_hands, ls.d_labels, ls.d_cand_list, ls.d_meta, ls.d_sel, ls.d_out);
  pinned_release(ls.h_meta, ls.h_out);
  for (auto &e : ls.ev)
    if (e) (void)hipEventDestroy(e);
  ls = LabelState();
}

int label_init(LabelState &ls) {
  if (ls.d_meta) return GPD_OK;
  HIP_RET(device_alloc(ls.d_meta, 4));
  HIP_RET(pinned_alloc(ls.h_meta, 4));
  for (auto &e : ls.ev) HIP_RET(hipEventCreate(&e));
  return GPD_OK;
}

int label_reserve(LabelState &ls, size_t need, size_t used, size_t image_bytes, size_t round_candidates, hipStream_t stream) {
  int rc = grow_device(ls.d_cand_list, ls.cap_round, round_candidates, slack_cap(round_candidates, 4), __func__);
  if (rc) return rc;
  if (image_bytes != ls.image_bytes) {  // (a context has one channel count: only the first call comes here)
    used = 0;
    ls.cap = 0;
  }
  if (need <= ls.cap) return GPD_OK;
  const size_t per = image_bytes + sizeof(gpd_hand) + 1;
  if (need > kLabelAccBudget / per) {
    set_error("label_view: %zu accumulated candidates of %zu bytes each exceed the accumulator's %zu GB", need, per, kLabelAccBudget >> 30);
    return GPD_ERR_CAPACITY;
  }
  note_alloc(__func__);
  const size_t cap = std::min(std::max(slack_cap(need, 2), (size_t)64), kLabelAccBudget / per);
  // the rounds so far move over
  rc = grow_group_keep({group_buffer(ls.d_images, image_bytes, true), group_buffer(ls.d_hands, sizeof(gpd_hand), true),
                        group_buffer(ls.d_labels, 1, true)},
                       cap, used, stream);
  if (rc) return rc;
  ls.cap = cap;
  ls.image_bytes = image_bytes;
  ls.grows++;
  return GPD_OK;
}

size_t label_out_layout(size_t k, size_t image_bytes, size_t off[4]) {
  auto up16 = [](size_t v) { return (v + 15) / 16 * 16; };
  off[0] = 0;
  off[1] = k * image_bytes;  // 3600 * C: a multiple of 16
  off[2] = off[1] + k * sizeof(gpd_hand);
  off[3] = off[2] + up16(k * sizeof(int32_t));
  return off[3] + up16(k);
}

int label_select_gather(LabelState &ls, int n, int end, hipStream_t stream, uint8_t *sink_images, uint8_t *sink_labels) {
  const size_t k = (size_t)2 * end;
  if (k == 0) return GPD_OK;
  int rc = grow_device(ls.d_sel, ls.cap_sel, k, slack_cap(k, 4), __func__);
  if (rc) return rc;
  size_t off[4];
  const size_t bytes = label_out_layout(k, ls.image_bytes, off);
  if (!sink_images) {
    rc = grow_device(ls.d_out, ls.d_out_bytes, bytes, slack_cap(bytes, 4), __func__);
    if (rc) return rc;
  }
  balance_select_kernel<<<1, SEL_T, 0, stream>>>(ls.d_labels, n, end, ls.d_sel);
  HIP_RET(hipGetLastError());
  if (sink_images) {
    const unsigned units = (unsigned)(ls.image_bytes / 16), per = (units + 255) / 256;
    if (k * per > 0x7fffffffull) {
      set_error("label_view: %zu kept instances are more than one gather launch takes", k);
      return GPD_ERR_CAPACITY;
    }
    label_gather_sink_kernel<<<(unsigned)(k * per), 256, 0, stream>>>(reinterpret_cast<const uint4 *>(ls.d_images), ls.d_labels, ls.d_sel,
                                                                      reinterpret_cast<uint4 *>(sink_images), sink_labels, units, per);
    HIP_RET(hipGetLastError());
    return GPD_OK;
  }
  GatherParams gp;
  gp.images = reinterpret_cast<const uint4 *>(ls.d_images);
  gp.hands = reinterpret_cast<const uint4 *>(ls.d_hands);
  gp.labels = ls.d_labels;
  gp.sel = ls.d_sel;
  gp.out_images = reinterpret_cast<uint4 *>(ls.d_out + off[0]);
  gp.out_hands = reinterpret_cast<uint4 *>(ls.d_out + off[1]);
  gp.out_src = reinterpret_cast<int32_t *>(ls.d_out + off[2]);
  gp.out_labels = reinterpret_cast<uint8_t *>(ls.d_out + off[3]);
  gp.k = (int)k;
  gp.img_units = (unsigned)(ls.image_bytes / 16);
  gp.blocks_per = (gp.img_units + kHandUnits + 255) / 256;
  const size_t grid = k * gp.blocks_per;
  if (grid > 0x7fffffffull) {
    set_error("label_view: %zu kept instances are more than one gather launch takes", k);
    return GPD_ERR_CAPACITY;
  }
  label_gather_kernel<<<(unsigned)grid, 256, 0, stream>>>(gp);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

}  // namespace gpd
