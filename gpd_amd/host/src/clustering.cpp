// gpd::Clustering — see include/gpd/clustering.h.  Clustering::findClusters (clustering.cpp:5-105) runs on the device
// (gpd_hip_find_clusters); the per-cluster lines the reference prints (:88-91) are printed from the results.
#include "gpd/clustering.h"

#include <cmath>
#include <cstdio>

namespace gpd {

Clustering::~Clustering() {
  if (own_ctx_) gpd_hip_destroy(own_ctx_);
}

std::vector<std::unique_ptr<candidate::Hand>> Clustering::findClusters(const std::vector<std::unique_ptr<candidate::Hand>> &hand_list,
                                                                        bool remove_inliers) {
  std::vector<std::unique_ptr<candidate::Hand>> hands_out;
  failed_ = false;
  const int n = (int)hand_list.size();
  if (n == 0) return hands_out;
  if (!ctx_) {
    gpd_params p;
    gpd_hip_default_params(&p);
    if (gpd_hip_create(0, &p, &own_ctx_) != GPD_OK) {
      printf("ERROR: Clustering::findClusters: %s\n", gpd_hip_last_error());
      failed_ = true;
      return hands_out;
    }
    ctx_ = own_ctx_;
  }
  std::vector<gpd_hand> in(n), out(n);
  std::vector<double> scores(n), out_scores(n);
  std::vector<int32_t> src(n);
  for (int i = 0; i < n; i++) {
    in[i] = hand_list[i]->record();
    scores[i] = hand_list[i]->getScore();
  }
  int k = 0;
  if (gpd_hip_find_clusters(ctx_, in.data(), scores.data(), n, min_inliers_, remove_inliers ? 1 : 0, out.data(), out_scores.data(), src.data(),
                            &k) != GPD_OK) {
    printf("ERROR: Clustering::findClusters: %s\n", gpd_hip_last_error());
    failed_ = true;
    return hands_out;
  }
  for (int c = 0; c < k; c++) {
    const gpd_hand &seed = in[src[c]];
    const double d[3] = {out[c].position[0] - seed.position[0], out[c].position[1] - seed.position[1], out[c].position[2] - seed.position[2]};
    printf("grasp %d, ||position_delta||: %3.4f, conf_lb: %3.4f\n", (int)src[c], sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), out_scores[c]);
    auto hand = std::make_unique<candidate::Hand>(out[c]);
    hand->setScore(out_scores[c]);
    hands_out.push_back(std::move(hand));
  }
  return hands_out;
}

}  // namespace gpd
