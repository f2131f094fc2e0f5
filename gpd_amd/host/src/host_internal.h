// Private to src/: the steps the classes of the mirror share, each written once.  Not installed.  Everything here has
// internal linkage (an anonymous namespace): the library is built without visibility flags, so anything else would be a
// new exported symbol.  config_file.cpp and cloud.cpp do not include it: they call nothing of libgpd_hip.so.
#pragma once
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "gpd/grasp_detector.h"

namespace gpd {
namespace {

inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Error convention of the reference: print + empty result (grasp_detector.cpp:201-205, 227-229).  True when the
// gpd_hip_* call failed, its reason printed.
inline bool hip_failed(int rc) {
  if (rc == GPD_OK) return false;
  printf("ERROR: %s\n", gpd_hip_last_error());
  return true;
}

// gpd_hip_upload_cloud of a util::Cloud; zeros travel as normals when the cloud has none, or when the caller is about
// to compute them (zero_normals)
inline int upload_cloud(gpd_hip_ctx *ctx, const util::Cloud &cloud, bool zero_normals = false) {
  const bool zeros = zero_normals || !cloud.hasNormals();
  const std::vector<float> none(zeros ? cloud.size() * 3 : 0, 0.f);
  return gpd_hip_upload_cloud(ctx, cloud.getCloudProcessed().data(), zeros ? none.data() : cloud.getNormals().data(), (int)cloud.size(),
                              cloud.getCameraSource().data(), cloud.numCameras(), cloud.getViewPoints().data());
}

inline int num_slots(const gpd_params &p) { return p.num_hand_axes * p.num_orientations; }

inline size_t count_valid(const std::vector<gpd_hand> &recs, size_t n) {
  size_t nv = 0;
  for (size_t i = 0; i < n; i++) nv += recs[i].valid;
  return nv;
}

// what the image entries return -> the reference's lists: image k and Hand(recs[cand[k]]), in candidate order (set-major,
// slot-minor, valid only: image_generator.cpp:91-98)
inline void emit_images(const std::vector<uint8_t> &pix, const std::vector<int32_t> &cand, int n_cand, const std::vector<gpd_hand> &recs,
                        int channels, std::vector<std::unique_ptr<net::Image>> &images_out,
                        std::vector<std::unique_ptr<candidate::Hand>> &hands_out) {
  const size_t bytes = (size_t)60 * 60 * channels;
  for (int k = 0; k < n_cand; k++) {
    auto im = std::make_unique<net::Image>(60, 60, channels);
    std::memcpy(im->data.data(), pix.data() + (size_t)k * bytes, bytes);
    images_out.push_back(std::move(im));
    hands_out.push_back(std::make_unique<candidate::Hand>(recs[cand[k]]));
  }
}

// GraspDetector::getHandSearchParameters (grasp_detector.h:176-186) of a parameter block
inline candidate::HandSearch::Parameters hand_search_parameters(const gpd_params &params, int num_samples) {
  candidate::HandSearch::Parameters p;
  p.nn_radius_frames_ = params.nn_radius_frames;
  p.num_threads_ = 1;
  p.num_samples_ = num_samples;
  p.num_orientations_ = params.num_orientations;
  p.num_finger_placements_ = params.num_finger_placements;
  p.hand_axes_.assign(params.hand_axes, params.hand_axes + params.num_hand_axes);
  p.deepen_hand_ = params.deepen_hand != 0;
  p.friction_coeff_ = params.friction_coeff;
  p.min_viable_ = params.min_viable;
  p.hand_geometry_ = {params.finger_width, params.hand_outer_diameter, params.hand_depth, params.hand_height, params.init_bite};
  return p;
}

inline std::vector<std::unique_ptr<candidate::HandSet>> to_sets(const std::vector<gpd_hand> &recs, int n_sets, int slots) {
  std::vector<std::unique_ptr<candidate::HandSet>> sets(n_sets);
  for (int s = 0; s < n_sets; s++) {
    sets[s] = std::make_unique<candidate::HandSet>();
    sets[s]->is_valid_.resize(slots);
    for (int j = 0; j < slots; j++) {
      const gpd_hand &r = recs[(size_t)s * slots + j];
      sets[s]->hands_.push_back(std::make_unique<candidate::Hand>(r));
      sets[s]->is_valid_[j] = r.valid != 0;
    }
    sets[s]->sample_ = {recs[(size_t)s * slots].sample[0], recs[(size_t)s * slots].sample[1], recs[(size_t)s * slots].sample[2]};
  }
  return sets;
}

// the flat record array gpd_hip_images_given / gpd_hip_score_given read: the listed hand sets in the order listed (empty ones
// left out), one row of slots each, set_index as listed; slots a set does not have stay invalid
inline std::vector<gpd_hand> given_records(const std::vector<std::unique_ptr<candidate::HandSet>> &sets, int slots) {
  std::vector<gpd_hand> recs;
  int n = 0;
  for (const auto &hs : sets) {
    if (!hs || hs->getHands().empty()) continue;
    recs.resize((size_t)(n + 1) * slots, gpd_hand());
    for (int j = 0; j < slots && j < (int)hs->getHands().size(); j++) {
      gpd_hand r = hs->getHands()[j]->record();
      r.set_index = n;
      r.valid = hs->getIsValid()[j] ? 1 : 0;
      recs[(size_t)n * slots + j] = r;
    }
    n++;
  }
  return recs;
}

}  // namespace
}  // namespace gpd
