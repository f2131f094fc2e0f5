// gpd::SequentialImportanceSampling — see include/gpd/sequential_importance_sampling.h (reference:
// sequential_importance_sampling.cpp:11-272).
#include "gpd/sequential_importance_sampling.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <iostream>

#include "gpd/util/config_file.h"
#include "host_internal.h"

namespace gpd {

static const int SUM_OF_GAUSSIANS = 0, MAX_OF_GAUSSIANS = 1;

// GPD_SIS_DUMP=<file>: the initial sample indices, then the samples of every round (tests replay them through the oracle)
static FILE *sis_dump_open() {
  const char *path = getenv("GPD_SIS_DUMP");
  return path ? fopen(path, "w") : nullptr;
}
static void sis_dump_init(FILE *dump, const std::vector<int> &indices) {
  if (!dump) return;
  fprintf(dump, "INIT %zu\n", indices.size());
  for (int i : indices) fprintf(dump, "%d\n", i);
}
static void sis_dump_round(FILE *dump, int round, const double *samples, int num_samples) {
  if (!dump) return;
  fprintf(dump, "ROUND %d %d\n", round, num_samples);
  for (int k = 0; k < num_samples; k++) fprintf(dump, "%.17g %.17g %.17g\n", samples[3 * k], samples[3 * k + 1], samples[3 * k + 2]);
}

SequentialImportanceSampling::SequentialImportanceSampling(const std::string &config_filename) {
  util::ConfigFile config_file(config_filename);
  config_file.ExtractKeys();
  num_init_samples_ = config_file.getValueOfKey<int>("num_init_samples", 50);
  num_iterations_ = config_file.getValueOfKey<int>("num_iterations", 5);
  num_samples_ = config_file.getValueOfKey<int>("num_samples_per_iteration", 50);
  prob_rand_samples_ = config_file.getValueOfKey<double>("prob_rand_samples", 0.3);
  radius_ = config_file.getValueOfKey<double>("standard_deviation", 0.02);
  sampling_method_ = config_file.getValueOfKey<int>("sampling_method", SUM_OF_GAUSSIANS);
  min_score_ = config_file.getValueOfKey<double>("min_score", 0);
  workspace_ = config_file.getValueOfKeyAsStdVectorDouble("workspace", "-1 1 -1 1 -1 1");
  workspace_.resize(6, 0.0);
  workspace_grasps_ = config_file.getValueOfKeyAsStdVectorDouble("workspace_grasps", "-1 1 -1 1 -1 1");
  workspace_grasps_.resize(6, 0.0);
  filter_approach_direction_ = config_file.getValueOfKey<bool>("filter_approach_direction", false);
  std::vector<double> approach = config_file.getValueOfKeyAsStdVectorDouble("direction", "1 0 0");
  approach.resize(3, 0.0);
  direction_ = {approach[0], approach[1], approach[2]};
  thresh_rad_ = config_file.getValueOfKey<double>("thresh_rad", 2.3);
  rng_state_ = 0x9E3779B97F4A7C15ull ^ (unsigned long long)config_file.getValueOfKey<int>("random_seed", 0);
  seed_ = (unsigned)config_file.getValueOfKey<int>("random_seed", 0);
  resident_ = config_file.getValueOfKey<int>("hip_sis_resident", 0) != 0;
  grasp_detector_ = std::make_unique<GraspDetector>(config_filename);
  clustering_ = std::make_unique<Clustering>(config_file.getValueOfKey<int>("min_inliers", 1));
  if (grasp_detector_->context()) clustering_->setContext(grasp_detector_->context());
}

unsigned long long SequentialImportanceSampling::nextRandom() {
  rng_state_ ^= rng_state_ << 13;
  rng_state_ ^= rng_state_ >> 7;
  rng_state_ ^= rng_state_ << 17;
  return rng_state_;
}

double SequentialImportanceSampling::randNormal(double sigma) {  // Box-Muller on two 53-bit uniforms
  const double u1 = ((double)(nextRandom() >> 11) + 1.0) * (1.0 / 9007199254740993.0);
  const double u2 = (double)(nextRandom() >> 11) * (1.0 / 9007199254740992.0);
  return sigma * sqrt(-2.0 * log(u1)) * cos(2.0 * M_PI * u2);
}

// :189-201
void SequentialImportanceSampling::drawSamplesFromSumOfGaussians(const std::vector<std::unique_ptr<candidate::HandSet>> &hand_sets,
                                                                 double sigma, int num_gauss_samples, std::vector<double> &samples_out) {
  for (int j = 0; j < num_gauss_samples; j++) {
    const int idx = randInt((int)hand_sets.size());
    const auto s = hand_sets[idx]->getSample();
    for (int r = 0; r < 3; r++) samples_out[3 * (size_t)j + r] = s[r] + randNormal(sigma);
  }
}

// :203-237, rejection sampling
void SequentialImportanceSampling::drawSamplesFromMaxOfGaussians(const std::vector<std::unique_ptr<candidate::HandSet>> &hand_sets,
                                                                 double sigma, int num_gauss_samples, std::vector<double> &samples_out,
                                                                 double term) {
  int j = 0;
  while (j < num_gauss_samples) {
    const int idx = randInt((int)hand_sets.size());
    const auto s = hand_sets[idx]->getSample();
    double x[3];
    for (int r = 0; r < 3; r++) x[r] = s[r] + randNormal(sigma);
    auto density = [&](const std::array<double, 3> &c) {
      double p = 0.0;
      for (int r = 0; r < 3; r++) p += (x[r] - c[r]) * (x[r] - c[r]);
      return term * exp((-1.0 / (2.0 * sigma)) * p);
    };
    double maxp = 0;
    for (size_t k = 0; k < hand_sets.size(); k++) {
      const double p = density(hand_sets[k]->getSample());
      if (p > maxp) maxp = p;
    }
    if (density(s) >= maxp) {
      for (int r = 0; r < 3; r++) samples_out[3 * (size_t)j + r] = x[r];
      j++;
    }
  }
}

// :239-270: uniform over the cloud's sample indices (or samples, or all points), inside the workspace
void SequentialImportanceSampling::drawUniformSamples(const util::Cloud &cloud, int num_samples, int start_idx, std::vector<double> &samples) {
  const std::vector<float> &xyz = cloud.getCloudProcessed();
  int i = 0, guard = 0;
  while (i < num_samples && guard++ < 1000000) {
    double sample[3];
    if (!cloud.getSampleIndices().empty()) {
      const int idx = cloud.getSampleIndices()[randInt((int)cloud.getSampleIndices().size())];
      for (int r = 0; r < 3; r++) sample[r] = (double)xyz[3 * (size_t)idx + r];
    } else if (cloud.getSamples().size() >= 3) {
      const int idx = randInt((int)(cloud.getSamples().size() / 3));
      for (int r = 0; r < 3; r++) sample[r] = cloud.getSamples()[3 * (size_t)idx + r];
    } else {
      const int idx = randInt((int)cloud.size());
      for (int r = 0; r < 3; r++) sample[r] = (double)xyz[3 * (size_t)idx + r];
    }
    if (sample[0] >= workspace_[0] && sample[0] <= workspace_[1] && sample[1] >= workspace_[2] && sample[1] <= workspace_[3] &&
        sample[2] >= workspace_[4] && sample[2] <= workspace_[5]) {
      for (int r = 0; r < 3; r++) samples[3 * (size_t)(start_idx + i) + r] = sample[r];
      i++;
    }
  }
}

// :54-187
std::vector<std::unique_ptr<candidate::Hand>> SequentialImportanceSampling::detectGrasps(util::Cloud &cloud) {
  std::vector<std::unique_ptr<candidate::Hand>> none;
  if (cloud.size() == 0) {
    printf("Error: Point cloud is empty!");
    return none;
  }
  if (resident_) return detectGraspsResident(cloud);
  const double t0 = now_s();
  FILE *dump = sis_dump_open();
  // 1. initial grasp hypotheses
  cloud.setSamples({});
  cloud.subsample(num_init_samples_);
  sis_dump_init(dump, cloud.getSampleIndices());
  std::vector<std::unique_ptr<candidate::HandSet>> hand_set_list = grasp_detector_->generateGraspCandidates(cloud);
  printf("Initially detected grasp candidates: %zu\n", hand_set_list.size());
  if (hand_set_list.empty()) {
    if (dump) fclose(dump);
    return none;
  }
  hand_set_list = grasp_detector_->filterGraspsWorkspace(hand_set_list, workspace_grasps_);
  printf("Grasps within workspace: %zu", hand_set_list.size());
  if (filter_approach_direction_) hand_set_list = grasp_detector_->filterGraspsDirection(hand_set_list, direction_, thresh_rad_);
  const int num_rand_samples = (int)(prob_rand_samples_ * num_samples_);
  const int num_gauss_samples = num_samples_ - num_rand_samples;
  const double sigma = radius_;
  const double term = 1.0 / sqrt(pow(2.0 * M_PI, 3.0) * pow(sigma, 3.0));
  std::vector<double> samples((size_t)3 * num_samples_, 0.0);
  // 2. importance sampling rounds
  for (int i = 0; i < num_iterations_ && !hand_set_list.empty(); i++) {
    std::cout << i << " " << num_gauss_samples << std::endl;
    if (sampling_method_ == SUM_OF_GAUSSIANS)
      drawSamplesFromSumOfGaussians(hand_set_list, sigma, num_gauss_samples, samples);
    else if (sampling_method_ == MAX_OF_GAUSSIANS)
      drawSamplesFromMaxOfGaussians(hand_set_list, sigma, num_gauss_samples, samples, term);
    drawUniformSamples(cloud, num_rand_samples, num_samples_ - num_rand_samples, samples);
    sis_dump_round(dump, i, samples.data(), num_samples_);
    cloud.setSamples(samples);
    std::vector<std::unique_ptr<candidate::HandSet>> hand_set_list_new = grasp_detector_->generateGraspCandidates(cloud);
    hand_set_list_new = grasp_detector_->filterGraspsWorkspace(hand_set_list_new, workspace_grasps_);
    if (filter_approach_direction_) hand_set_list_new = grasp_detector_->filterGraspsDirection(hand_set_list_new, direction_, thresh_rad_);
    const size_t added = hand_set_list_new.size();
    hand_set_list.insert(hand_set_list.end(), std::make_move_iterator(hand_set_list_new.begin()),
                         std::make_move_iterator(hand_set_list_new.end()));
    printf("Added %zu grasp candidates in round %d. Total: %zu.\n", added, i, hand_set_list.size());
  }
  if (dump) fclose(dump);
  // 3. classify everything at once
  std::vector<std::unique_ptr<candidate::Hand>> valid_grasps = grasp_detector_->pruneGraspCandidates(cloud, hand_set_list, min_score_);
  printf("Valid grasps: %zu\n", valid_grasps.size());
  // 4. cluster
  if (clustering_->getMinInliers() > 0) {
    valid_grasps = clustering_->findClusters(valid_grasps);
    if (clustering_->failed()) printf("ERROR: the clustering step failed; no grasps returned.\n");
  }
  printf("Final result: found %zu grasps.\n", valid_grasps.size());
  printf("Total runtime: %3.4fs\n.\n", now_s() - t0);
  return valid_grasps;
}

// :54-187 as ONE gpd_hip_detect_sis call (cfg hip_sis_resident = 1): the initial samples are drawn here, everything after them
// happens on the device; the lines of the rounds are printed from round_counts, GPD_SIS_DUMP is written from samples_out
std::vector<std::unique_ptr<candidate::Hand>> SequentialImportanceSampling::detectGraspsResident(util::Cloud &cloud) {
  std::vector<std::unique_ptr<candidate::Hand>> none;
  const double t0 = now_s();
  cloud.setSamples({});
  cloud.subsample(num_init_samples_);
  if (!grasp_detector_->upload(cloud)) return none;
  const std::vector<int> &idx = cloud.getSampleIndices();
  const std::vector<int32_t> init(idx.begin(), idx.end());
  const size_t slots = (size_t)num_slots(grasp_detector_->getParams());
  const size_t iters = (size_t)std::max(num_iterations_, 0), per = (size_t)std::max(num_samples_, 0);
  std::vector<gpd_hand> recs(std::max((init.size() + iters * per) * slots, (size_t)1));
  std::vector<double> samples(std::max(iters * per * 3, (size_t)1));
  std::vector<int32_t> counts((1 + iters) * 4, 0);
  gpd_sis_job job;
  std::memset(&job, 0, sizeof(job));
  job.sample_indices = init.data();
  job.num_init_samples = (int)init.size();
  job.num_iterations = num_iterations_;
  job.num_samples = num_samples_;
  job.sampling_method = sampling_method_;
  job.prob_rand_samples = prob_rand_samples_;
  job.sigma = radius_;
  job.min_score = min_score_;
  for (int a = 0; a < 6; a++) job.workspace[a] = workspace_[a];
  job.min_inliers = clustering_->getMinInliers();
  job.seed = seed_;
  job.hands = recs.data();
  job.capacity = (int)std::min(recs.size(), (size_t)0x7fffffff);
  job.samples_out = samples.data();
  job.round_counts = counts.data();
  if (hip_failed(gpd_hip_detect_sis(grasp_detector_->context(), &job))) return none;
  if (FILE *dump = sis_dump_open()) {
    sis_dump_init(dump, init);
    for (int r = 0; r < job.rounds_run; r++) sis_dump_round(dump, r, samples.data() + (size_t)r * per * 3, num_samples_);
    fclose(dump);
  }
  printf("Grasps within workspace: %d\n", counts[0]);
  const int num_gauss_samples = num_samples_ - (int)(prob_rand_samples_ * num_samples_);
  int total = counts[0];
  for (int r = 0; r < job.rounds_run; r++) {
    std::cout << r << " " << num_gauss_samples << std::endl;
    total += counts[4 * (r + 1)];
    printf("Added %d grasp candidates in round %d. Total: %d.\n", counts[4 * (r + 1)], r, total);
  }
  std::vector<std::unique_ptr<candidate::Hand>> valid_grasps;
  for (int k = 0; k < job.num_hands; k++) {
    auto h = std::make_unique<candidate::Hand>(recs[k]);
    h->setScore(recs[k].score);
    valid_grasps.push_back(std::move(h));
  }
  if (job.min_inliers <= 0) printf("Valid grasps: %zu\n", valid_grasps.size());
  printf("Final result: found %zu grasps.\n", valid_grasps.size());
  printf("Total runtime: %3.4fs\n.\n", now_s() - t0);
  return valid_grasps;
}

}  // namespace gpd
