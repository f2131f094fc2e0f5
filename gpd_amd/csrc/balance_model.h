// DataGenerator::balanceInstances (data_generator.cpp:406-430) followed by the order DataGenerator::addInstances writes
// (:432-458), over the labels of a view's accumulated candidates.  Plain C++ with no HIP in it: gpd_hip_balance_view, the host
// mirror and the tests of the device selection (label.hip balance_select_kernel) read the same code.  The reference keeps the
// first `end` of each class in accumulated order (its positives / negatives lists are filled ascending) and writes the
// positives before the negatives.
#pragma once
#include <cstdint>
#include <vector>

#include "sample_model.h"

namespace gpd {
namespace balance {

// The shuffle of a set of instances before it is stored (data_generator.cpp:219-220: std::random_shuffle, whose generator is
// the C library's rand() — unseeded and implementation-defined, so the project's seeded stream is the definition): a
// Fisher-Yates from the back, entry i with entry next() % (i + 1), on a stream that runs on from one set to the next.
// order[k] = the instance that ends up at position k.
inline void shuffle_order(int n, sample::Stream &st, std::vector<int32_t> &order) {
  order.resize((size_t)(n > 0 ? n : 0));
  for (int i = 0; i < n; i++) order[(size_t)i] = i;
  for (int i = n - 1; i > 0; i--) {
    const int j = (int)(st.next() % (uint64_t)(i + 1));
    const int32_t t = order[(size_t)i];
    order[(size_t)i] = order[(size_t)j];
    order[(size_t)j] = t;
  }
}

// end of balanceInstances: max_grasps_per_view is halved the way the reference's int(0.5 * max) does it
inline int kept_per_class(long long positives, long long negatives, int max_grasps_per_view) {
  const long long half = max_grasps_per_view > 0 ? max_grasps_per_view / 2 : 0;
  long long end = positives < negatives ? positives : negatives;
  if (half < end) end = half;
  return (int)end;
}

// indices of the kept candidates, positives first; returns `end`
inline int view(const uint8_t *labels, int n, int max_grasps_per_view, std::vector<int32_t> &out) {
  long long pos = 0;
  for (int i = 0; i < n; i++) pos += labels[i] != 0;
  const int end = kept_per_class(pos, (long long)n - pos, max_grasps_per_view);
  out.assign((size_t)2 * end, 0);
  int np = 0, nn = 0;
  for (int i = 0; i < n && (np < end || nn < end); i++) {
    if (labels[i] != 0) {
      if (np < end) out[(size_t)np++] = i;
    } else if (nn < end) {
      out[(size_t)end + nn++] = i;
    }
  }
  return end;
}

}  // namespace balance
}  // namespace gpd
