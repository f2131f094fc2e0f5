// Cloud::removeStatisticalOutliers (util/cloud.cpp:166-174): PCL 1.9's StatisticalOutlierRemoval::applyFilterIndices with
// setMeanK(mean_k) and setStddevMulThresh(mult), negative = false, on finite coordinates — restated in DESIGN §7
// ("removeStatisticalOutliers").  Plain C++ with no HIP in it: the host mirror's single-core model
// (util::Cloud::removeStatisticalOutliers) runs filter() below, the device path (outliers.hip) runs threshold() between its
// two kernels and equals filter() bit for bit.  Every expression is written in the operation order the definition gives and
// must be compiled without FMA contraction.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "refine_model.h"

namespace gpd {
namespace outlier {

constexpr int kMeanKCap = 255;  // the kNN rows hold 256 keys: the point itself and mean_k neighbours

// 0: inside the domain; 1: refused as invalid (mean_k < 1, a non-finite mult, fewer than mean_k + 1 points — PCL reads past
// the lists its search returned there); 2: beyond the capacity (mean_k > 255)
inline int refusal(int n, int mean_k, double mult) {
  if (mean_k < 1 || !std::isfinite(mult)) return 1;
  if (mean_k > kMeanKCap) return 2;
  if (n < mean_k + 1) return 1;
  return 0;
}

// item 2 for one point: d2 holds the sorted float d2 of ranks 0 .. mean_k; rank 0 is skipped whatever point it is.  The
// float sqrt is the correctly rounded one; the adds are sequential doubles in rank order.
inline float mean_distance(const float *d2, int mean_k) {
  double dist_sum = 0.0;
  for (int r = 1; r <= mean_k; r++) dist_sum += (double)std::sqrt(d2[r]);
  return (float)(dist_sum / (double)mean_k);
}

struct Stats {
  double mean = 0.0, stddev = 0.0, threshold = 0.0;
};

// items 3-4: the two sequential double sums over i = 0 .. n-1 (the square is a float product, rounded, then widened) and
// the threshold.  A variance that rounding made negative gives a NaN stddev and threshold: nothing is removed then.
inline Stats threshold(const float *dist, int n, double mult) {
  double sum = 0.0, sq_sum = 0.0;
  for (int i = 0; i < n; i++) {
    sum += (double)dist[i];
    const float sq = dist[i] * dist[i];
    sq_sum += (double)sq;
  }
  Stats s;
  s.mean = sum / (double)n;
  const double sum2 = sum * sum;
  const double variance = (sq_sum - sum2 / (double)n) / ((double)n - 1.0);
  s.stddev = std::sqrt(variance);
  const double spread = mult * s.stddev;
  s.threshold = s.mean + spread;
  return s;
}

// item 5: point i is removed iff this is true (false for a NaN threshold)
inline bool removed(float dist, double threshold) { return (double)dist > threshold; }

struct Result {
  std::vector<float> dist;    // [n] the mean distance of every point to its mean_k nearest neighbours
  std::vector<int32_t> kept;  // the kept input indices, ascending
  Stats stats;
};

// the whole filter on xyz [n][3]; the caller has checked refusal()
inline Result filter(const float *xyz, int n, int mean_k, double mult) {
  Result r;
  std::vector<int32_t> lists;
  const int k = refine::knn(xyz, n, mean_k + 1, lists);  // ascending by (d2, index): the d2 sequence is the sorted one
  r.dist.resize((size_t)n);
  std::vector<float> d2((size_t)k);
  for (int i = 0; i < n; i++) {
    for (int t = 0; t < k; t++) d2[t] = refine::dist2(xyz + 3 * (size_t)i, xyz + 3 * (size_t)lists[(size_t)i * k + t]);
    r.dist[i] = mean_distance(d2.data(), mean_k);
  }
  r.stats = threshold(r.dist.data(), n, mult);
  for (int i = 0; i < n; i++)
    if (!removed(r.dist[i], r.stats.threshold)) r.kept.push_back(i);
  return r;
}

}  // namespace outlier
}  // namespace gpd
