// gpd::GraspDetector — see include/gpd/grasp_detector.h (reference: grasp_detector.cpp), re-hosted on libgpd_hip.so
// (include/gpd_hip.h).
#include <algorithm>
#include <cmath>
#include <fstream>
#include <iostream>

#include "gpd/util/config_file.h"
#include "host_internal.h"

namespace gpd {

static std::string dir_of(const std::string &path) {
  size_t s = path.find_last_of('/');
  return s == std::string::npos ? std::string("./") : path.substr(0, s + 1);
}
// cfg paths are relative to the working directory in the reference; also try the cfg file's own directory
static std::string resolve(const std::string &p, const std::string &cfg_dir) {
  if (p.empty() || p[0] == '/') return p;
  std::ifstream a(p.c_str());
  if (a.good()) return p;
  return cfg_dir + p;
}

GraspDetector::GraspDetector(const std::string &config_filename) {
  util::ConfigFile config_file(config_filename);
  if (!config_file.ExtractKeys()) return;
  const std::string cfg_dir = dir_of(config_filename);
  gpd_hip_default_params(&params_);
  // hand geometry (grasp_detector.cpp:13-19, hand_geometry.cpp:22-30)
  std::string hg = config_file.getValueOfKeyAsString("hand_geometry_filename", "");
  util::ConfigFile hand_cfg(hg == "0" || hg.empty() ? config_filename : resolve(hg, cfg_dir));
  hand_cfg.ExtractKeys();
  params_.finger_width = hand_cfg.getValueOfKey<double>("finger_width", 0.01);
  params_.hand_outer_diameter = hand_cfg.getValueOfKey<double>("hand_outer_diameter", 0.12);
  params_.hand_depth = hand_cfg.getValueOfKey<double>("hand_depth", 0.06);
  params_.hand_height = hand_cfg.getValueOfKey<double>("hand_height", 0.02);
  params_.init_bite = hand_cfg.getValueOfKey<double>("init_bite", 0.01);
  // candidate generation (grasp_detector.cpp:47-88)
  num_samples_ = config_file.getValueOfKey<int>("num_samples", 1000);
  workspace_ = config_file.getValueOfKeyAsStdVectorDouble("workspace", "-1 1 -1 1 -1 1");
  workspace_.resize(6, 0.0);
  voxelize_ = config_file.getValueOfKey<bool>("voxelize", true);
  voxel_size_ = config_file.getValueOfKey<double>("voxel_size", 0.003);
  normals_radius_ = config_file.getValueOfKey<double>("normals_radius", 0.03);
  params_.nn_radius_frames = config_file.getValueOfKey<double>("nn_radius", 0.01);
  params_.num_orientations = config_file.getValueOfKey<int>("num_orientations", 8);
  params_.num_finger_placements = config_file.getValueOfKey<int>("num_finger_placements", 10);
  params_.deepen_hand = config_file.getValueOfKey<bool>("deepen_hand", true) ? 1 : 0;
  std::vector<int> axes = config_file.getValueOfKeyAsStdVectorInt("hand_axes", "2");
  params_.num_hand_axes = (int)std::min<size_t>(axes.size(), 3);
  for (int i = 0; i < params_.num_hand_axes; i++) params_.hand_axes[i] = axes[i];
  params_.friction_coeff = config_file.getValueOfKey<double>("friction_coeff", 20.0);
  params_.min_viable = config_file.getValueOfKey<int>("min_viable", 6);
  // image geometry (grasp_detector.cpp:120-127, image_geometry.cpp:21-29)
  std::string ig = config_file.getValueOfKeyAsString("image_geometry_filename", "");
  util::ConfigFile img_cfg(ig == "0" || ig.empty() ? config_filename : resolve(ig, cfg_dir));
  img_cfg.ExtractKeys();
  params_.volume_width = img_cfg.getValueOfKey<double>("volume_width", 0.10);
  params_.volume_depth = img_cfg.getValueOfKey<double>("volume_depth", 0.06);
  params_.volume_height = img_cfg.getValueOfKey<double>("volume_height", 0.02);
  params_.image_size = img_cfg.getValueOfKey<int>("image_size", 60);
  params_.image_num_channels = img_cfg.getValueOfKey<int>("image_num_channels", 15);
  // filtering and selection (grasp_detector.cpp:157-185)
  workspace_grasps_ = config_file.getValueOfKeyAsStdVectorDouble("workspace_grasps", "-1 1 -1 1 -1 1");
  workspace_grasps_.resize(6, 0.0);
  for (int i = 0; i < 6; i++) params_.workspace_grasps[i] = workspace_grasps_[i];
  params_.min_aperture = config_file.getValueOfKey<double>("min_aperture", 0.0);
  params_.max_aperture = config_file.getValueOfKey<double>("max_aperture", 0.085);
  // approach-direction filter, clustering, selection (grasp_detector.cpp:168-185)
  filter_approach_direction_ = config_file.getValueOfKey<bool>("filter_approach_direction", false);
  std::vector<double> approach = config_file.getValueOfKeyAsStdVectorDouble("direction", "1 0 0");
  approach.resize(3, 0.0);
  direction_ = {approach[0], approach[1], approach[2]};
  thresh_rad_ = config_file.getValueOfKey<double>("thresh_rad", 2.3);
  // the fused device entries apply the direction filter themselves, right after the workspace filter (gpd_params)
  params_.filter_approach_direction = filter_approach_direction_ ? 1 : 0;
  for (int i = 0; i < 3; i++) params_.direction[i] = direction_[i];
  params_.thresh_rad = thresh_rad_;
  const int min_inliers = config_file.getValueOfKey<int>("min_inliers", 1);
  clustering_ = std::make_unique<Clustering>(min_inliers);  // runs on ctx_ once that exists (below)
  cluster_grasps_ = min_inliers > 0;
  num_selected_ = config_file.getValueOfKey<int>("num_selected", 100);
  use_file_normals_ = config_file.getValueOfKey<int>("use_file_normals", 0) != 0;
  // Preprocessing steps of CandidatesGenerator::preprocessPointCloud that are PCL algorithms of their own and are not
  // restated here (candidates_generator.cpp:28-34, grasp_detector.cpp:52-63): a cloud that needs them has to go through
  // them before it gets here.  Refused, not skipped: a silently different cloud would give silently different grasps.
  // Not all off in the shipped cfg files: ur5.cfg and cem_vino_params.cfg set sample_above_plane = 1; the fit itself is
  // GraspDetector::sampleAbovePlane (call it between preprocessPointCloud with num_samples = 0 and subsample).
  const struct {
    const char *key, *what;
  } unsupported[] = {{"remove_outliers",
                      "pcl::StatisticalOutlierRemoval (cloud.cpp:166-174; the reference reads the key and never runs the filter — here it is "
                      "GraspDetector::removeStatisticalOutliers, called between preprocessPointCloud and subsample)"},
                     {"sample_above_plane", "a RANSAC plane fit, pcl::SACSegmentation (cloud.cpp:407-436)"},
                     {"refine_normals_k", "pcl::NormalRefinement (cloud.cpp:176-204)"},
                     {"remove_plane_before_image_calculation",
                      "ImageGenerator::removePlane, pcl::SACSegmentation (image_generator.cpp:32, 101-125): it changes the point list behind every grasp image"}};
  for (const auto &u : unsupported)
    if (config_file.getValueOfKey<int>(u.key, 0) != 0) {
      printf("ERROR: %s = %d asks for %s, which this build does not have; unset it or preprocess the cloud beforehand\n", u.key,
             config_file.getValueOfKey<int>(u.key, 0), u.what);
      return;  // ok() stays false
    }
  printf("============ CANDIDATE GENERATION ============\n");
  printf("num_samples: %d\nnn_radius: %3.2f\nnum_orientations: %d\nnum_finger_placements: %d\ndeepen_hand: %s\n", num_samples_,
         params_.nn_radius_frames, params_.num_orientations, params_.num_finger_placements, params_.deepen_hand ? "true" : "false");
  printf("==============================================\n");
  if (hip_failed(gpd_hip_create(config_file.getValueOfKey<int>("hip_device", 0), &params_, &ctx_))) {
    ctx_ = nullptr;
    return;
  }
  if (ctx_) clustering_->setContext(ctx_);
  // hip_shadow_jitter / hip_shadow_jitter_seed (not reference keys): 1 = the shadow points of the 15-channel images leave the
  // 3 mm lattice by a seeded per-voxel draw of the reference's magnitude and arithmetic (gpd_hip_set_shadow_jitter; the
  // reference's own draw is unseeded, hand_set.cpp:187-204).  Default 0: the lattice.  Context state: detectGrasps, the
  // importance sampler and the data generator on this detector's context all image with it.
  shadow_jitter_ = config_file.getValueOfKey<int>("hip_shadow_jitter", 0);
  shadow_jitter_seed_ = config_file.getValueOfKey<unsigned long long>("hip_shadow_jitter_seed", 0ull);
  if (shadow_jitter_ != 0) {  // (printed like hip_lenet_mode: only when it is not the default)
    if (gpd_hip_set_shadow_jitter(ctx_, shadow_jitter_, shadow_jitter_seed_) != GPD_OK) {
      printf("ERROR: hip_shadow_jitter = %d: %s\n", shadow_jitter_, gpd_hip_last_error());
      gpd_hip_destroy(ctx_);
      ctx_ = nullptr;  // ok() is false: a detector that images differently from its cfg file is not handed out
      return;
    }
    printf("============ IMAGES ==========================\n");
    printf("volume_width: %.3f\nvolume_depth: %.3f\nvolume_height: %.3f\nimage_num_channels: %d\nhip_shadow_jitter: %d\nhip_shadow_jitter_seed: %llu\n",
           params_.volume_width, params_.volume_depth, params_.volume_height, params_.image_num_channels, shadow_jitter_, shadow_jitter_seed_);
    printf("==============================================\n");
  }
  // classifier (grasp_detector.cpp:129-145): created through the plugin factory, as the reference does.  For the
  // Eigen-layout parameters weights_file is the parameter directory.
  std::string model_file = config_file.getValueOfKeyAsString("model_file", "");
  std::string weights_file = config_file.getValueOfKeyAsString("weights_file", "");
  if (!model_file.empty() || !weights_file.empty()) {
    const int device = config_file.getValueOfKey<int>("device", 0);
    const int batch_size = config_file.getValueOfKey<int>("batch_size", 1);
    const std::string dir = resolve(weights_file, cfg_dir);
    classifier_ = net::Classifier::create(model_file, dir, static_cast<net::Classifier::Device>(device), batch_size);
    printf("============ CLASSIFIER ======================\nmodel_file: %s\nweights_file: %s\nbatch_size: %d\n"
           "==============================================\n",
           model_file.c_str(), dir.c_str(), batch_size);
    // detectGrasps normally runs search -> images -> scores fused on the device, in ctx_: the HIP back-end's
    // parameters are loaded there as well.  Any other Classifier (or cfg classifier_plugin_route = 1) is driven
    // through classifyImages, the reference's own sequence (grasp_detector.cpp:261-273).
    auto *hc = dynamic_cast<net::HipClassifier *>(classifier_.get());
    if (!classifier_) {
      printf("ERROR: could not create the classifier from %s\n", dir.c_str());
    } else if (!hc) {
      has_classifier_ = true;  // a foreign back-end: plugin route only
    } else if (hc->channels() != params_.image_num_channels) {
      printf("ERROR: the classifier's %d channels do not match image_num_channels = %d\n", hc->channels(), params_.image_num_channels);
      classifier_.reset();
    } else if (hip_failed(hc->installOn(ctx_))) {  // the weights (either route) and the conv ReLU flag of the directory's network.cfg, if any
      classifier_.reset();
    } else {
      has_classifier_ = true;
      fused_classifier_ = true;
    }
    // a mode key of the fused classifier (not a reference key; printed only when it is not the default): both the fused
    // path's context and the plugin's own take the value; a refusal by either leaves the detector without a classifier
    auto mode_key = [&](const char *key, int (*set_context)(gpd_hip_ctx *, int), bool (net::HipClassifier::*set_classifier)(int)) {
      const int mode = config_file.getValueOfKey<int>(key, 0);
      if (!fused_classifier_ || mode == 0) return;
      bool set = set_context(ctx_, mode) == GPD_OK;
      if (!set) printf("ERROR: %s = %d: %s\n", key, mode, gpd_hip_last_error());
      set = set && (hc->*set_classifier)(mode);
      if (!set) {
        has_classifier_ = fused_classifier_ = false;
        classifier_.reset();
      } else {
        printf("%s: %d\n", key, mode);
      }
    };
    // hip_lenet_mode: 0 = split operands on the int8 / bf16 matrix pipes (default), 1 = the f32 chain in EigenClassifier's
    // operation order
    mode_key("hip_lenet_mode", gpd_hip_set_lenet_mode, &net::HipClassifier::setScoringMode);
    // hip_lenet_net_mode: the arithmetic of the shape-general route (gpd_hip_set_lenet_net_mode), 0 = the f32 chains (default),
    // 1 = split operands on the bf16 matrix pipe; context state, so it is legal whichever route the directory's network takes
    mode_key("hip_lenet_net_mode", gpd_hip_set_lenet_net_mode, &net::HipClassifier::setNetMode);
    plugin_route_ = config_file.getValueOfKey<int>("classifier_plugin_route", 0) != 0;
  }
}

GraspDetector::GraspDetector(const candidate::HandSearch::Parameters &hs, const descriptor::ImageGeometry &ig, int hip_device) {
  gpd_hip_default_params(&params_);
  params_.finger_width = hs.hand_geometry_.finger_width_;
  params_.hand_outer_diameter = hs.hand_geometry_.outer_diameter_;
  params_.hand_depth = hs.hand_geometry_.depth_;
  params_.hand_height = hs.hand_geometry_.height_;
  params_.init_bite = hs.hand_geometry_.init_bite_;
  params_.nn_radius_frames = hs.nn_radius_frames_;
  params_.num_orientations = hs.num_orientations_;
  params_.num_finger_placements = hs.num_finger_placements_;
  params_.deepen_hand = hs.deepen_hand_ ? 1 : 0;
  params_.num_hand_axes = (int)std::min<size_t>(hs.hand_axes_.size(), 3);
  for (int i = 0; i < params_.num_hand_axes; i++) params_.hand_axes[i] = hs.hand_axes_[i];
  params_.friction_coeff = hs.friction_coeff_;
  params_.min_viable = hs.min_viable_;
  params_.volume_width = ig.outer_diameter_;
  params_.volume_depth = ig.depth_;
  params_.volume_height = ig.height_;
  params_.image_size = ig.size_;
  params_.image_num_channels = ig.num_channels_;
  num_samples_ = hs.num_samples_;
  voxelize_ = false;
  workspace_ = {-1.0, 1.0, -1.0, 1.0, -1.0, 1.0};
  workspace_grasps_ = workspace_;
  for (int i = 0; i < 6; i++) params_.workspace_grasps[i] = workspace_grasps_[i];
  clustering_ = std::make_unique<Clustering>(0);
  if (hip_failed(gpd_hip_create(hip_device, &params_, &ctx_))) ctx_ = nullptr;
  if (ctx_) clustering_->setContext(ctx_);
}

candidate::HandSearch::Parameters GraspDetector::getHandSearchParameters() const {
  return hand_search_parameters(params_, num_samples_);
}

GraspDetector::~GraspDetector() {
  if (ctx_) gpd_hip_destroy(ctx_);
}

bool GraspDetector::calculateNormals(util::Cloud &cloud, double radius) {
  if (!ctx_ || cloud.size() == 0) return false;
  std::vector<float> normals(cloud.size() * 3, 0.f);
  printf("Calculating surface normals ...\n");
  if (hip_failed(upload_cloud(ctx_, cloud, true)) || hip_failed(gpd_hip_estimate_normals(ctx_, radius, normals.data()))) return false;
  last_num_sets_ = 0;
  cloud.setNormals(normals);
  return true;
}

// CandidatesGenerator::preprocessPointCloud (candidates_generator.cpp:14-37): workspace cut, voxelise when enabled,
// normals ALWAYS recomputed, subsample.  The reference never reads normals from a PCD; normals that came with the
// file are used only when the cfg says so (use_file_normals = 1: no voxelisation then either, the normals belong to
// the points as loaded) — the synthetic benchmark clouds ship their analytic normals this way.
// The workspace cut and the voxeliser run on the device (gpd_hip_preprocess_cloud); util::Cloud's own
// filterWorkspace / voxelizeCloud are the host-side API mirror for callers that hold a Cloud and no detector.
void GraspDetector::preprocessPointCloud(util::Cloud &cloud) {
  printf("Processing cloud with %zu points.\n", cloud.size());
  const bool keep_normals = use_file_normals_ && cloud.hasNormals();
  if (!ctx_) {
    printf("ERROR: no device context\n");
    return;
  }
  cloud.filterWorkspaceSamples(workspace_);  // candidates_generator.cpp:19 (NaN rows are dropped at load time)
  const int n = (int)cloud.size(), cams = cloud.numCameras();
  if (n > 0) {
    std::vector<float> xyz((size_t)n * 3);
    std::vector<int> cam((size_t)n * cams), src(n);
    int m = 0;
    const bool voxelise = voxelize_ && !keep_normals;
    if (hip_failed(gpd_hip_preprocess_cloud(ctx_, cloud.getCloudProcessed().data(), cloud.getCameraSource().data(), n, cams,
                                        workspace_.size() >= 6 ? workspace_.data() : nullptr, voxelise ? (float)voxel_size_ : 0.f,
                                        xyz.data(), cam.data(), src.data(), &m, nullptr)))
      return;
    xyz.resize((size_t)m * 3);
    cam.resize((size_t)m * cams);
    std::vector<float> normals;
    if (keep_normals) {
      normals.resize((size_t)m * 3);
      for (int k = 0; k < m; k++)
        for (int r = 0; r < 3; r++) normals[3 * (size_t)k + r] = cloud.getNormals()[3 * (size_t)src[k] + r];
    }
    cloud.setProcessed(xyz, cam, normals);
    if (voxelise) printf("Voxelized cloud: %zu\n", cloud.size());
  }
  if (!keep_normals && cloud.size() > 0 && !calculateNormals(cloud, normals_radius_)) return;
  cloud.subsample(num_samples_);
}

bool GraspDetector::sampleAbovePlane(util::Cloud &cloud, double threshold, int max_iterations, double probability, bool optimize) {
  const auto t0 = std::chrono::steady_clock::now();
  printf("Sampling above plane ...\n");
  if (!ctx_ || cloud.size() == 0) return false;
  util::Cloud::PlaneFit fit;
  fit.above.resize(cloud.size());
  int num = 0;
  if (hip_failed(upload_cloud(ctx_, cloud)) ||
      hip_failed(gpd_hip_sample_above_plane(ctx_, threshold, max_iterations, probability, optimize ? 1 : 0, fit.above.data(), &num, fit.coeffs,
                                        &fit.num_inliers, &fit.iterations)))
    return false;
  last_num_sets_ = 0;
  fit.above.resize(num);
  cloud.applyPlaneFit(fit, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return true;
}

bool GraspDetector::refineNormals(util::Cloud &cloud, int k, int max_iterations, float convergence_threshold) {
  if (!ctx_ || cloud.size() == 0 || !cloud.hasNormals()) return false;
  std::vector<float> refined(cloud.size() * 3, 0.f);
  int iterations = 0, num_nan = 0;
  if (hip_failed(upload_cloud(ctx_, cloud)) ||
      hip_failed(gpd_hip_refine_normals(ctx_, k, max_iterations, convergence_threshold, refined.data(), &iterations, nullptr, &num_nan, nullptr)))
    return false;
  last_num_sets_ = 0;
  cloud.applyRefinedNormals(refined);
  return true;
}

bool GraspDetector::removeStatisticalOutliers(util::Cloud &cloud, int mean_k, double stddev_mult) {
  if (!ctx_ || cloud.size() == 0) return false;
  std::vector<int> kept(cloud.size());
  int num = 0;
  double stats[3];
  if (hip_failed(upload_cloud(ctx_, cloud)) ||
      hip_failed(gpd_hip_remove_statistical_outliers(ctx_, mean_k, stddev_mult, kept.data(), &num, stats, nullptr, nullptr)))
    return false;
  last_num_sets_ = 0;
  kept.resize(num);
  cloud.applyOutlierRemoval(kept);
  return true;
}

bool GraspDetector::upload(const util::Cloud &cloud) {
  if (!ctx_) return false;
  if (cloud.size() == 0) {
    printf("ERROR: Point cloud is empty!");
    return false;
  }
  if (!cloud.hasNormals()) {
    printf("ERROR: the cloud has no normals (call preprocessPointCloud first)\n");
    return false;
  }
  return !hip_failed(upload_cloud(ctx_, cloud));
}

bool GraspDetector::searchDevice(const util::Cloud &cloud, bool fused, std::vector<gpd_hand> &recs, int &n_sets, int &n_cand) {
  const std::vector<double> &samples = cloud.getSamples();
  const std::vector<int> &idx = cloud.getSampleIndices();
  const int slots = num_slots(params_);
  n_sets = n_cand = 0;
  int rc;
  if (samples.size() >= 3) {  // use samples (hand_search.cpp:37-39)
    const int S = (int)(samples.size() / 3);
    recs.assign((size_t)S * slots, gpd_hand());
    rc = fused ? gpd_hip_detect_samples(ctx_, samples.data(), S, recs.data(), &n_sets, &n_cand)
               : gpd_hip_search_samples(ctx_, samples.data(), S, recs.data(), &n_sets);
  } else if (!idx.empty()) {  // use indices (:40-43)
    recs.assign(idx.size() * slots, gpd_hand());
    rc = fused ? gpd_hip_detect(ctx_, idx.data(), (int)idx.size(), recs.data(), &n_sets, &n_cand)
               : gpd_hip_search(ctx_, idx.data(), (int)idx.size(), recs.data(), &n_sets);
  } else {
    std::cout << "Error: No samples or no indices!\n";  // hand_search.cpp:44-48
    return false;
  }
  if (hip_failed(rc)) return false;
  last_num_sets_ = n_sets;
  last_samples_.resize((size_t)n_sets * 3);
  for (int s = 0; s < n_sets; s++)
    for (int r = 0; r < 3; r++) last_samples_[3 * (size_t)s + r] = recs[(size_t)s * slots].sample[r];
  return true;
}

// grasp_detector.cpp:522-526
std::vector<int> GraspDetector::evalGroundTruth(const util::Cloud &cloud_gt, std::vector<std::unique_ptr<candidate::Hand>> &hands) {
  std::vector<int> labels(hands.size(), 0);
  if (hands.empty() || !upload(cloud_gt)) return labels;
  last_num_sets_ = 0;  // the device search buffers now belong to cloud_gt
  std::vector<gpd_hand> recs(hands.size());
  for (size_t i = 0; i < hands.size(); i++) recs[i] = hands[i]->record();
  std::vector<int32_t> l(hands.size(), 0);
  if (hip_failed(gpd_hip_reevaluate(ctx_, recs.data(), (int)recs.size(), l.data()))) return labels;
  for (size_t i = 0; i < hands.size(); i++) {
    labels[i] = l[i];
    hands[i]->setHalfAntipodal(recs[i].half_antipodal != 0);
    hands[i]->setFullAntipodal(recs[i].full_antipodal != 0);
  }
  return labels;
}

std::vector<std::unique_ptr<candidate::HandSet>> GraspDetector::generateGraspCandidates(const util::Cloud &cloud) {
  std::vector<std::unique_ptr<candidate::HandSet>> none;
  if (!upload(cloud)) return none;
  std::vector<gpd_hand> recs;
  int n_sets = 0, n_cand = 0;
  if (!searchDevice(cloud, false, recs, n_sets, n_cand)) return none;
  return to_sets(recs, n_sets, num_slots(params_));
}

// grasp_detector.cpp:334-398 (the right_top typo at :360-363 is kept)
std::vector<std::unique_ptr<candidate::HandSet>> GraspDetector::filterGraspsWorkspace(
    std::vector<std::unique_ptr<candidate::HandSet>> &hand_set_list, const std::vector<double> &workspace) const {
  int remaining = 0;
  std::vector<std::unique_ptr<candidate::HandSet>> out;
  printf("Filtering grasps outside of workspace ...\n");
  for (size_t i = 0; i < hand_set_list.size(); i++) {
    const auto &hands = hand_set_list[i]->getHands();
    std::vector<bool> is_valid = hand_set_list[i]->getIsValid();
    bool any = false;
    for (size_t j = 0; j < hands.size(); j++) {
      if (!is_valid[j]) continue;
      const double half_width = 0.5 * params_.hand_outer_diameter;
      auto pos = hands[j]->getPosition(), bin = hands[j]->getBinormal(), app = hands[j]->getApproach();
      bool ok = hands[j]->getGraspWidth() >= params_.min_aperture && hands[j]->getGraspWidth() <= params_.max_aperture;
      for (int r = 0; r < 3 && ok; r++) {
        const double lb = pos[r] + half_width * bin[r], rb = pos[r] - half_width * bin[r];
        const double lt = lb + params_.hand_depth * app[r], rt = lb + params_.hand_depth * app[r];
        const double ap = pos[r] - 0.05 * app[r];
        const double mn = std::min({lb, rb, lt, rt, ap}), mx = std::max({lb, rb, lt, rt, ap});
        ok = mn >= workspace[2 * r] && mx <= workspace[2 * r + 1];
      }
      is_valid[j] = ok;
      if (ok) {
        remaining++;
        any = true;
      }
    }
    if (any) {
      hand_set_list[i]->setIsValid(is_valid);
      out.push_back(std::move(hand_set_list[i]));
    }
  }
  printf("Number of grasp candidates within workspace and gripper width: %d\n", remaining);
  return out;
}

// grasp_detector.cpp:422-453
std::vector<std::unique_ptr<candidate::HandSet>> GraspDetector::filterGraspsDirection(
    std::vector<std::unique_ptr<candidate::HandSet>> &hand_set_list, const std::array<double, 3> &direction, double thresh_rad) {
  std::vector<std::unique_ptr<candidate::HandSet>> out;
  int remaining = 0;
  for (size_t i = 0; i < hand_set_list.size(); i++) {
    const auto &hands = hand_set_list[i]->getHands();
    std::vector<bool> is_valid = hand_set_list[i]->getIsValid();
    bool any = false;
    for (size_t j = 0; j < hands.size(); j++) {
      if (!is_valid[j]) continue;
      const auto app = hands[j]->getApproach();
      const double angle = acos(direction[0] * app[0] + direction[1] * app[1] + direction[2] * app[2]);
      if (angle > thresh_rad) {
        is_valid[j] = false;
      } else {
        remaining++;
        any = true;
      }
    }
    if (any) {
      hand_set_list[i]->setIsValid(is_valid);
      out.push_back(std::move(hand_set_list[i]));
    }
  }
  printf("Number of grasp candidates with correct approach direction: %d\n", remaining);
  return out;
}

// the flat record array gpd_hip_images reads: one row of slots per set of the last search, rows of
// sets that are not in `sets` stay invalid
std::vector<gpd_hand> GraspDetector::flatten(const std::vector<std::unique_ptr<candidate::HandSet>> &sets) const {
  const int slots = num_slots(params_);
  std::vector<gpd_hand> recs((size_t)last_num_sets_ * slots, gpd_hand());
  for (const auto &hs : sets) {
    if (!hs || hs->getHands().empty()) continue;
    const int si = hs->getHands()[0]->record().set_index;
    if (si < 0 || si >= last_num_sets_) continue;
    for (int j = 0; j < slots && j < (int)hs->getHands().size(); j++) {
      recs[(size_t)si * slots + j] = hs->getHands()[j]->record();
      recs[(size_t)si * slots + j].valid = hs->getIsValid()[j] ? 1 : 0;
    }
  }
  return recs;
}

// Are these hand sets still the ones on the device: the numbering and the samples of the last search (last_num_sets of
// them, last_samples [set][3])?  Two rules over one test of a set's first record:
//   kTheWholeSearch  createImages: the list IS the last search, every set present and at its own position;
//   kAmongTheSearch  pruneGraspCandidates: any selection of it, in any order, empty sets passed over.
enum class Resident { kTheWholeSearch, kAmongTheSearch };
static bool sets_resident(const std::vector<std::unique_ptr<candidate::HandSet>> &sets, int last_num_sets,
                          const std::vector<double> &last_samples, Resident rule) {
  const bool whole = rule == Resident::kTheWholeSearch;
  if (whole ? (int)sets.size() != last_num_sets : last_num_sets <= 0) return false;
  for (size_t s = 0; s < sets.size(); s++) {
    if (!sets[s] || sets[s]->getHands().empty()) {
      if (whole) return false;
      continue;
    }
    const gpd_hand &r0 = sets[s]->getHands()[0]->record();
    if (whole ? r0.set_index != (int)s : (r0.set_index < 0 || r0.set_index >= last_num_sets)) return false;
    for (int r = 0; r < 3; r++)
      if (!(last_samples[3 * (size_t)r0.set_index + r] == r0.sample[r])) return false;
  }
  return true;
}

// grasp_detector.cpp:528-551
std::vector<std::unique_ptr<candidate::Hand>> GraspDetector::pruneGraspCandidates(
    const util::Cloud &cloud, const std::vector<std::unique_ptr<candidate::HandSet>> &hand_set_list, double min_score) {
  std::vector<std::unique_ptr<candidate::Hand>> hands_out;
  if (!ctx_ || !has_classifier_ || hand_set_list.empty()) return hands_out;
  std::vector<gpd_hand> recs;
  std::vector<int32_t> cand;
  std::vector<float> scores;
  int n_cand = 0;
  if (sets_resident(hand_set_list, last_num_sets_, last_samples_, Resident::kAmongTheSearch)) {
    recs = flatten(hand_set_list);
    const size_t nv = count_valid(recs, recs.size());
    cand.resize(nv);
    scores.resize(nv);
    if (hip_failed(gpd_hip_images(ctx_, recs.data(), last_num_sets_, nullptr, cand.data(), &n_cand)) ||
        (n_cand > 0 && hip_failed(gpd_hip_score(ctx_, nullptr, n_cand, scores.data()))))
      return hands_out;
  } else {
    // a list gathered over several searches, or hands of another cloud: the records themselves go to the device
    // (gpd_hip_score_given), sets numbered as listed; no second search
    if (!upload(cloud)) return hands_out;
    const int slots = num_slots(params_);
    recs = given_records(hand_set_list, slots);
    if (recs.empty()) return hands_out;
    const size_t nv = count_valid(recs, recs.size());
    cand.resize(nv + 1);  // + 1: never an empty buffer, whose data() may be null
    scores.resize(nv + 1);
    last_num_sets_ = 0;  // the device search buffers are reused
    last_samples_.clear();
    if (hip_failed(gpd_hip_score_given(ctx_, recs.data(), (int)(recs.size() / slots), 0, scores.data(), cand.data(), &n_cand, nullptr)))
      return hands_out;
  }
  for (int k = 0; k < n_cand; k++) {
    if (scores[k] > min_score) {
      auto h = std::make_unique<candidate::Hand>(recs[cand[k]]);
      h->setScore(scores[k]);
      hands_out.push_back(std::move(h));
    }
  }
  return hands_out;
}

bool GraspDetector::createImages(const util::Cloud &cloud, const std::vector<std::unique_ptr<candidate::HandSet>> &hand_set_list,
                                 std::vector<std::unique_ptr<net::Image>> &images_out,
                                 std::vector<std::unique_ptr<candidate::Hand>> &hands_out) {
  images_out.clear();
  hands_out.clear();
  if (!ctx_) return false;
  if (hand_set_list.empty()) return true;
  const size_t bytes = (size_t)60 * 60 * params_.image_num_channels;
  std::vector<gpd_hand> recs;
  std::vector<uint8_t> pix;
  std::vector<int32_t> cand;
  int n_cand = 0;
  // the hand sets of the last generateGraspCandidates call are on the device already; any others travel there
  if (sets_resident(hand_set_list, last_num_sets_, last_samples_, Resident::kTheWholeSearch)) {
    recs = flatten(hand_set_list);
    const size_t nv = count_valid(recs, recs.size());
    pix.resize(nv * bytes);
    cand.resize(nv);
    if (hip_failed(gpd_hip_images(ctx_, recs.data(), last_num_sets_, pix.data(), cand.data(), &n_cand))) return false;
  } else {
    // ImageGenerator::createImages(cloud, hand_set_list) images whatever it is handed (image_generator.cpp:17-99)
    if (!upload(cloud)) return false;
    const int slots = num_slots(params_);
    recs = given_records(hand_set_list, slots);
    if (recs.empty()) return true;
    const size_t nv = count_valid(recs, recs.size());
    pix.resize(nv * bytes + 1);  // + 1, as in pruneGraspCandidates
    cand.resize(nv + 1);
    last_num_sets_ = 0;  // the device search buffers are reused
    last_samples_.clear();
    if (hip_failed(gpd_hip_images_given(ctx_, recs.data(), (int)(recs.size() / slots), 0, pix.data(), cand.data(), &n_cand, nullptr))) return false;
  }
  emit_images(pix, cand, n_cand, recs, params_.image_num_channels, images_out, hands_out);
  return true;
}

bool GraspDetector::createGraspImages(util::Cloud &cloud, std::vector<std::unique_ptr<candidate::Hand>> &hands_out,
                                      std::vector<std::unique_ptr<net::Image>> &images_out) {
  hands_out.clear();
  images_out.clear();
  if (!upload(cloud)) return false;
  const int slots = num_slots(params_);
  std::vector<gpd_hand> recs;
  int n_sets = 0, n_cand = 0;
  if (!searchDevice(cloud, false, recs, n_sets, n_cand)) return false;
  printf("Generated %d hand sets.\n", n_sets);
  // workspace / aperture filter on the flat records (same predicate as filterGraspsWorkspace)
  {
    auto sets = to_sets(recs, n_sets, slots);
    std::vector<std::vector<bool>> keep(n_sets, std::vector<bool>(slots, false));
    for (int s = 0; s < n_sets; s++) sets[s]->sample_[0] = s;  // remember the set number through the move
    auto filtered = filterGraspsWorkspace(sets, workspace_grasps_);
    if (filter_approach_direction_)  // grasp_detector.cpp:505-512
      filtered = filterGraspsDirection(filtered, direction_, thresh_rad_);
    for (auto &hs : filtered) keep[(int)hs->sample_[0]] = hs->getIsValid();
    for (int s = 0; s < n_sets; s++)
      for (int j = 0; j < slots; j++) recs[(size_t)s * slots + j].valid = keep[s][j] ? 1 : 0;
  }
  const size_t nv = count_valid(recs, (size_t)n_sets * slots);
  std::vector<uint8_t> pix(nv * (size_t)60 * 60 * params_.image_num_channels);
  std::vector<int32_t> cand(nv);
  if (hip_failed(gpd_hip_images(ctx_, recs.data(), n_sets, pix.data(), cand.data(), &n_cand))) return false;
  emit_images(pix, cand, n_cand, recs, params_.image_num_channels, images_out, hands_out);
  return true;
}

std::vector<std::unique_ptr<candidate::Hand>> GraspDetector::selectGrasps(std::vector<std::unique_ptr<candidate::Hand>> &hands) const {
  printf("Selecting the %d highest scoring grasps ...\n", num_selected_);  // grasp_detector.cpp:405-420
  int middle = std::min((int)hands.size(), num_selected_);
  std::partial_sort(hands.begin(), hands.begin() + middle, hands.end(), isScoreGreater);
  std::vector<std::unique_ptr<candidate::Hand>> out;
  for (int i = 0; i < middle; i++) {
    out.push_back(std::move(hands[i]));
    printf(" grasp #%d, score: %3.4f\n", i, out[i]->getScore());
  }
  return out;
}

std::vector<std::unique_ptr<candidate::Hand>> GraspDetector::detectGrasps(const util::Cloud &cloud) {
  const double t0 = now_s();
  std::vector<std::unique_ptr<candidate::Hand>> hands_out;
  if (!upload(cloud)) return hands_out;
  if (!has_classifier_) {
    printf("ERROR: no classifier weights loaded (cfg key weights_file)\n");
    return hands_out;
  }
  const int slots = num_slots(params_);
  std::vector<gpd_hand> recs;
  int n_sets = 0, n_cand = 0;
  std::vector<std::unique_ptr<candidate::Hand>> hands;
  float ms[3] = {0, 0, 0};
  if (plugin_route_ || !fused_classifier_) {
    // the reference's own sequence through the plugin interface (grasp_detector.cpp:222-273): candidates ->
    // filterGraspsWorkspace [-> filterGraspsDirection] -> ImageGenerator::createImages -> classifier_->classifyImages
    // -> hands[i]->setScore
    util::Cloud work = cloud;
    std::vector<std::unique_ptr<net::Image>> images;
    if (!createGraspImages(work, hands, images)) return hands_out;
    float t[3];
    gpd_hip_last_stage_ms(ctx_, t);
    ms[0] = t[0];
    ms[1] = t[1];
    const double tc = now_s();
    const std::vector<float> scores = classifier_->classifyImages(images);
    ms[2] = (float)((now_s() - tc) * 1e3);
    for (size_t i = 0; i < hands.size(); i++) hands[i]->setScore(scores[i]);
  } else {
    // steps 1-4 fused on the device (grasp_detector.cpp:222-273), filterGraspsWorkspace and — when the cfg asks for it —
    // filterGraspsDirection (:247-250) included: both run at the end of the hand kernel, before the candidate list is built
    if (!searchDevice(cloud, true, recs, n_sets, n_cand)) return hands_out;
    printf("Generated %d hand sets.\n", n_sets);
    if (filter_approach_direction_) printf("Number of grasp candidates with correct approach direction: %d\n", n_cand);
    gpd_hip_last_stage_ms(ctx_, ms);
    for (size_t i = 0; i < (size_t)n_sets * slots; i++)
      if (recs[i].valid) hands.push_back(std::make_unique<candidate::Hand>(recs[i]));
  }
  // 5. select the highest scoring grasps
  hands = selectGrasps(hands);
  // 6. cluster the grasps (grasp_detector.cpp:283-303)
  std::vector<std::unique_ptr<candidate::Hand>> clusters;
  if (cluster_grasps_) {
    clusters = clustering_->findClusters(hands);
    if (clustering_->failed()) {  // a device error is not "fewer than four clusters": print-and-return-empty, as for every failure
      printf("ERROR: the clustering step failed; no grasps returned.\n");
      return std::vector<std::unique_ptr<candidate::Hand>>();
    }
    printf("Found %d clusters.\n", (int)clusters.size());
    if (clusters.size() <= 3) {
      printf("Not enough clusters found! Adding all grasps from previous step.");
      for (size_t i = 0; i < hands.size(); i++) clusters.push_back(std::move(hands[i]));
    }
  } else {
    clusters = std::move(hands);
  }
  // 7. sort by score
  std::sort(clusters.begin(), clusters.end(), isScoreGreater);
  printf("======== Selected grasps ========\n");
  for (size_t i = 0; i < clusters.size(); i++) std::cout << "Grasp " << i << ": " << clusters[i]->getScore() << "\n";
  printf("Selected the %d best grasps.\n", (int)clusters.size());
  runtimes_[0] = ms[0] / 1e3;
  runtimes_[1] = ms[1] / 1e3;
  runtimes_[2] = ms[2] / 1e3;
  runtimes_[3] = now_s() - t0;
  printf("======== RUNTIMES ========\n 1. Candidate generation: %3.4fs\n 2. Descriptor extraction: %3.4fs\n 3. Classification: %3.4fs\n"
         "==========\n TOTAL: %3.4fs\n",
         runtimes_[0], runtimes_[1], runtimes_[2], runtimes_[3]);
  return clusters;
}

}  // namespace gpd
