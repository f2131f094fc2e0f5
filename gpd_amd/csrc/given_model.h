// What a caller may hand to gpd_hip_images_given / gpd_hip_score_given: hand sets that did not come from the last search.
// Plain C++ with no HIP in it: gpd_hip_given_check, the two entries (which make the check before anything is enqueued) and the
// host mirror read the same code.
//
// The image kernels take `sample`, `frame`, `bottom` and `center` of a candidate from its record (load_box, image_device.h) and
// the neighbourhood list and the shadow voxels from its SET, so the hands of a set must share the set's sample exactly — the
// reference's HandSet has one sample (hand_set.h) — and their boxes must stay inside the voxel windows the kernels were sized
// for (image_model.h, window_class): init_bite - hand_depth <= bottom <= 0, |center| <= (outer_diameter - finger_width) / 2,
// what FingerHand leaves (finger_hand.cpp:155-168), and a frame that is a rotation.  Hands outside that domain are refused.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include "../../include/gpd_hip.h"

namespace gpd {
namespace given {

constexpr double kRotTol = 1e-6;      // every entry of F^T F - I
constexpr double kRangeSlack = 1e-9;  // on each end of the ranges of bottom and center: a third of a millionth of a voxel, and it
                                      // admits the search's own records (it returns bottom = -6.9e-18)

inline bool finite_n(const double *v, int n) {
  for (int i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// GPD_OK, or GPD_ERR_INVALID with the first offending set / slot and the reason in msg
inline int check(const gpd_params &p, const gpd_hand *hands, int num_sets, int *bad_set, int *bad_slot, char *msg, size_t msg_len) {
  const int slots = p.num_hand_axes * p.num_orientations;
  const double bottom_lo = p.init_bite - p.hand_depth, center_max = 0.5 * (p.hand_outer_diameter - p.finger_width);
  auto refuse = [&](int s, int j, const char *why) {
    *bad_set = s;
    *bad_slot = j;
    snprintf(msg, msg_len, "given hands: set %d, slot %d: %s", s, j, why);
    return GPD_ERR_INVALID;
  };
  *bad_set = -1;
  *bad_slot = -1;
  for (int s = 0; s < num_sets; s++) {
    const gpd_hand *set = hands + (size_t)s * slots;
    if (!finite_n(set[0].sample, 3)) return refuse(s, 0, "the set's sample (slot 0's) is not finite");
    for (int j = 0; j < slots; j++) {
      const gpd_hand &h = set[j];
      if (!h.valid) continue;  // a husk: nothing else is read from it
      if (std::memcmp(h.sample, set[0].sample, sizeof(h.sample)) != 0)
        return refuse(s, j, "the sample differs from the set's (slot 0's): the hands of a set share one sample, bit for bit");
      if (!finite_n(h.frame, 9) || !std::isfinite(h.bottom) || !std::isfinite(h.center))
        return refuse(s, j, "frame, bottom or center is not finite");
      for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++) {
          double g = a == b ? -1.0 : 0.0;
          for (int r = 0; r < 3; r++) g += h.frame[3 * r + a] * h.frame[3 * r + b];
          if (!(std::fabs(g) <= kRotTol)) return refuse(s, j, "the frame is not a rotation (an entry of F^T F - I beyond 1e-6)");
        }
      if (!(h.bottom >= bottom_lo - kRangeSlack && h.bottom <= kRangeSlack))
        return refuse(s, j, "bottom outside [init_bite - hand_depth, 0]");
      if (!(std::fabs(h.center) <= center_max + kRangeSlack))
        return refuse(s, j, "|center| beyond (hand_outer_diameter - finger_width) / 2");
    }
  }
  return GPD_OK;
}

}  // namespace given
}  // namespace gpd
