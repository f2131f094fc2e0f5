// gpd::DataGenerator over libgpd_hip.so — see include/gpd/data_generator.h.
#include "gpd/data_generator.h"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

#include "gpd/util/config_file.h"
#include "host_internal.h"
#include "../../csrc/balance_model.h"

namespace gpd {

namespace {
constexpr int kImageSize = 60;
constexpr size_t kNpyHeaderBytes = 128;  // magic, version, length and the dictionary, padded: a multiple of 64 as the format asks
}  // namespace

DataGenerator::DataGenerator(const std::string &config_filename) {
  detector_ = std::make_unique<GraspDetector>(config_filename);
  util::ConfigFile config_file(config_filename);
  config_file.ExtractKeys();
  data_root_ = config_file.getValueOfKeyAsString("data_root", "");
  objects_file_location_ = config_file.getValueOfKeyAsString("objects_file_location", "");
  output_root_ = config_file.getValueOfKeyAsString("output_root", "");
  num_views_per_object_ = config_file.getValueOfKey<int>("num_views_per_object", 1);
  min_grasps_per_view_ = config_file.getValueOfKey<int>("min_grasps_per_view", 100);
  max_grasps_per_view_ = config_file.getValueOfKey<int>("max_grasps_per_view", 500);
  test_views_ = config_file.getValueOfKeyAsStdVectorInt("test_views", "3 7 11 15 19");
  num_samples_ = config_file.getValueOfKey<int>("num_samples", 500);
  remove_nans_ = config_file.getValueOfKey<bool>("remove_nans", true);
  voxel_size_views_ = config_file.getValueOfKey<double>("voxel_size_views", 0.003);
  normals_radius_ = config_file.getValueOfKey<double>("normals_radius", 0.03);
  reverse_mesh_normals_ = config_file.getValueOfKey<bool>("reverse_mesh_normals", true);
  reverse_view_normals_ = config_file.getValueOfKey<bool>("reverse_view_normals", true);
  sample_seed_ = config_file.getValueOfKey<uint32_t>("sample_seed", 0u);
  shuffle_seed_ = config_file.getValueOfKey<uint32_t>("shuffle_seed", 0u);
  max_rounds_per_view_ = config_file.getValueOfKey<int>("max_rounds_per_view", 20);

  printf("============ DATA GENERATION =================\n");
  std::cout << "data_root: " << data_root_ << "\n";
  std::cout << "objects_file_location: " << objects_file_location_ << "\n";
  std::cout << "output_root: " << output_root_ << "\n";
  std::cout << "num_views_per_object: " << num_views_per_object_ << "\n";
  std::cout << "min_grasps_per_view: " << min_grasps_per_view_ << "\n";
  std::cout << "max_grasps_per_view: " << max_grasps_per_view_ << "\n";
  std::cout << "test_views: ";
  for (int v : test_views_) std::cout << v << " ";
  std::cout << "\n";
  printf("max_rounds_per_view: %d\nsample_seed: %u\nshuffle_seed: %u\n", max_rounds_per_view_, sample_seed_, shuffle_seed_);
  printf("==============================================\n");
  printf("============ CLOUD PREPROCESSING =============\n");
  printf("remove_nans: %d\n", remove_nans_);
  printf("voxel_size_views: %.3f\n", voxel_size_views_);
  printf("normals_radius_: %.3f\n", normals_radius_);
  printf("reverse_mesh_normals: %d\n", reverse_mesh_normals_);
  printf("reverse_view_normals: %d\n", reverse_view_normals_);
  printf("==============================================\n");
  printf("============ CANDIDATE GENERATION ============\n");
  printf("num_samples: %d\n", num_samples_);
  printf("==============================================\n");
  // the PCD reader of util::Cloud drops NaN rows as it loads (the device takes finite coordinates only)
  if (!remove_nans_) printf("remove_nans = 0: rows with a NaN coordinate are dropped at load time all the same\n");
}

DataGenerator::~DataGenerator() {
  closeSet(train_);
  closeSet(test_);
}

std::vector<std::string> DataGenerator::loadObjectNames(const std::string &objects_file_location) {
  std::ifstream in(objects_file_location.c_str());
  std::string line;
  std::vector<std::string> objects;
  while (std::getline(in, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    if (line.empty()) continue;
    std::cout << line << "\n";
    objects.push_back(line);
  }
  return objects;
}

bool DataGenerator::writeHeader(FILE *f, int rows, bool images) const {
  char dict[kNpyHeaderBytes];
  int n;
  if (images)
    n = snprintf(dict, sizeof(dict), "{'descr': '|u1', 'fortran_order': False, 'shape': (%d, %d, %d, %d), }", rows, kImageSize, kImageSize,
                 detector_->getParams().image_num_channels);
  else
    n = snprintf(dict, sizeof(dict), "{'descr': '|u1', 'fortran_order': False, 'shape': (%d, 1), }", rows);
  unsigned char head[kNpyHeaderBytes];
  std::memset(head, ' ', sizeof(head));
  std::memcpy(head, "\x93NUMPY\x01\x00", 8);
  const unsigned len = (unsigned)(kNpyHeaderBytes - 10);
  head[8] = (unsigned char)(len & 0xff);
  head[9] = (unsigned char)(len >> 8);
  if (n < 0 || (size_t)n > kNpyHeaderBytes - 11) return false;
  std::memcpy(head + 10, dict, (size_t)n);
  head[kNpyHeaderBytes - 1] = '\n';
  return fseek(f, 0, SEEK_SET) == 0 && fwrite(head, 1, sizeof(head), f) == sizeof(head) && fseek(f, 0, SEEK_END) == 0;
}

bool DataGenerator::openSet(NpySet &set, const std::string &name) {
  const std::string img = output_root_ + name + "_images.npy", lab = output_root_ + name + "_labels.npy";
  set.images = fopen(img.c_str(), "wb");
  set.labels = fopen(lab.c_str(), "wb");
  set.count = 0;
  if (!set.images || !set.labels) {
    printf("ERROR: cannot write %s / %s\n", img.c_str(), lab.c_str());
    return false;
  }
  printf("Writing %s and %s\n", img.c_str(), lab.c_str());
  return writeHeader(set.images, 0, true) && writeHeader(set.labels, 0, false);
}

bool DataGenerator::appendSet(NpySet &set, const SetData &data, const std::vector<int32_t> &order) {
  const size_t bytes = (size_t)kImageSize * kImageSize * detector_->getParams().image_num_channels;
  for (int32_t i : order) {
    if (fwrite(data.images.data() + (size_t)i * bytes, 1, bytes, set.images) != bytes || fwrite(data.labels.data() + i, 1, 1, set.labels) != 1) {
      printf("ERROR: short write to the data set files\n");
      return false;
    }
  }
  set.count += (int)order.size();
  return true;
}

bool DataGenerator::closeSet(NpySet &set) {
  bool good = true;
  if (set.images) good = writeHeader(set.images, set.count, true) && fclose(set.images) == 0 && good;
  if (set.labels) good = writeHeader(set.labels, set.count, false) && fclose(set.labels) == 0 && good;
  set.images = set.labels = nullptr;
  return good;
}

bool DataGenerator::estimateNormals(util::Cloud &cloud, bool reverse) {
  if (!detector_->calculateNormals(cloud, normals_radius_)) return false;
  if (reverse) {
    std::vector<float> n = cloud.getNormals();
    for (float &v : n) v = -v;
    cloud.setNormals(n);
  }
  return true;
}

// steps 1-5 of a view (data_generator.cpp:126-201): preprocess, then ONE gpd_hip_label_view call
bool DataGenerator::labelView(int object, int view, util::Cloud &cloud, SetData &into, gpd_hip_trainer *sink, int which) {
  gpd_hip_ctx *ctx = detector_->context();
  const int n = (int)cloud.size(), cams = cloud.numCameras();
  std::vector<float> xyz((size_t)n * 3);
  std::vector<int> cam((size_t)n * cams), src(n);
  int m = 0;
  if (hip_failed(gpd_hip_preprocess_cloud(ctx, cloud.getCloudProcessed().data(), cloud.getCameraSource().data(), n, cams, nullptr,
                                          (float)voxel_size_views_, xyz.data(), cam.data(), src.data(), &m, nullptr)))
    return false;
  xyz.resize((size_t)m * 3);
  cam.resize((size_t)m * cams);
  cloud.setProcessed(xyz, cam, std::vector<float>());
  printf("Voxelized cloud: %zu\n", cloud.size());
  if (!estimateNormals(cloud, reverse_view_normals_)) return false;
  if (hip_failed(upload_cloud(ctx, cloud))) return false;
  // hip_shadow_jitter (the detector read it): every view its own pattern, seed + the view's ordinal in the data set — with one
  // seed all views would move the voxel at a given lattice position alike
  if (detector_->shadowJitter() != 0 &&
      hip_failed(gpd_hip_set_shadow_jitter(ctx, 1, detector_->shadowJitterSeed() + (unsigned long long)(object * num_views_per_object_ + view))))
    return false;
  // the draws of every round that may run (Cloud::subsampleUniformly is time-seeded in the reference; these are seeded)
  const int per = std::max(std::min(num_samples_, m), 0), rounds = std::max(max_rounds_per_view_, 0);
  std::vector<int32_t> samples((size_t)per * rounds + 1);
  const uint32_t view_seed = sample_seed_ + 1000003u * (uint32_t)(object * num_views_per_object_ + view);
  for (int r = 0; r < rounds; r++) {
    int k = 0;
    if (gpd_hip_sample_positions(m, num_samples_, view_seed + (uint32_t)r, 0, samples.data() + (size_t)r * per, &k) != GPD_OK || k != per) {
      printf("ERROR: sample draw of round %d failed: %s\n", r, gpd_hip_last_error());
      return false;
    }
  }
  const size_t bytes = (size_t)kImageSize * kImageSize * detector_->getParams().image_num_channels;
  const int capacity = 2 * (std::max(max_grasps_per_view_, 0) / 2);
  std::vector<uint8_t> images(sink ? 1 : (size_t)capacity * bytes + 1), labels(sink ? 1 : (size_t)capacity + 1);
  gpd_label_view_job job;
  std::memset(&job, 0, sizeof(job));
  job.sample_indices = samples.data();
  job.samples_per_round = per;
  job.max_rounds = rounds;
  job.min_positives = min_grasps_per_view_;
  job.max_grasps_per_view = max_grasps_per_view_;
  if (!sink) {
    job.images = images.data();
    job.labels = labels.data();
    job.capacity = capacity;
  }
  if (hip_failed(sink ? gpd_hip_train_append_view(sink, which, ctx, &job) : gpd_hip_label_view(ctx, &job))) return false;
  printf("rounds: %d, #grasps: %d\n", job.rounds_run, job.num_candidates);
  printf("positives, negatives found for this view: %d, %d\n", job.num_positives, job.num_candidates - job.num_positives);
  printf("#positives: %d, #negatives: %d\n", job.num_positives_out, job.num_out - job.num_positives_out);
  into.count += job.num_out;
  if (sink) return true;
  into.images.insert(into.images.end(), images.begin(), images.begin() + (size_t)job.num_out * bytes);
  into.labels.insert(into.labels.end(), labels.begin(), labels.begin() + job.num_out);
  return true;
}

bool DataGenerator::generateData(gpd_hip_trainer *sink) {
  if (!ok()) return false;
  gpd_hip_ctx *ctx = detector_->context();
  const std::vector<std::string> objects = loadObjectNames(objects_file_location_);
  const int num_objects = (int)objects.size();
  if (sink)
    train_.count = test_.count = 0;
  else if (!openSet(train_, "train") || !openSet(test_, "test"))
    return false;
  sample::Stream shuffle(shuffle_seed_);  // one stream through every stored set
  double total_time = 0.0;
  for (int i = 0; i < num_objects; i++) {
    printf("===> Generating images for object %d/%d: %s\n", i + 1, num_objects, objects[i].c_str());
    const auto t0 = std::chrono::steady_clock::now();
    // the mesh: the ground truth of every view of the object, uploaded once (its _gt_normals.csv is not read: the reference
    // overwrites those normals at data_generator.cpp:113)
    const std::string prefix = data_root_ + objects[i];
    std::cout << " mesh_file_path: " << prefix + "_gt.pcd" << '\n';
    util::Cloud mesh(prefix + "_gt.pcd", {0.0, 0.0, 0.0});
    if (mesh.size() == 0) {
      printf("ERROR: the mesh %s_gt.pcd is empty or does not exist\n", prefix.c_str());
      return false;
    }
    printf("Loaded mesh with %d points.\n", (int)mesh.size());
    if (!estimateNormals(mesh, reverse_mesh_normals_)) return false;
    if (hip_failed(gpd_hip_upload_ground_truth(ctx, mesh.getCloudProcessed().data(), mesh.getNormals().data(), (int)mesh.size()))) return false;
    SetData train_data, test_data;
    int first[2] = {0, 0};  // under a sink: where this object's range of each resident set begins
    if (sink && (hip_failed(gpd_hip_train_count(sink, 0, &first[0], nullptr)) || hip_failed(gpd_hip_train_count(sink, 1, &first[1], nullptr))))
      return false;
    for (int j = 0; j < num_views_per_object_; j++) {
      printf("===> Processing view %d/%d\n", j + 1, num_views_per_object_);
      util::Cloud cloud(prefix + "_" + std::to_string(j + 1) + ".pcd", {0.0, 0.0, 0.0});
      if (cloud.size() == 0) {
        printf("ERROR: the view %s_%d.pcd is empty or does not exist\n", prefix.c_str(), j + 1);
        return false;
      }
      // 6. the view's instances go to the training or the test data (data_generator.cpp:204-212)
      const bool is_test = std::find(test_views_.begin(), test_views_.end(), j) != test_views_.end();
      SetData &into = is_test ? test_data : train_data;
      if (!labelView(i, j, cloud, into, sink, is_test ? 1 : 0)) return false;
      std::cout << (is_test ? "test view, # test data: " : "train view, # train data: ") << into.count << "\n";
      printf("------------------------------------\n");
    }
    // store_step is 1: shuffle and store after every object (:217-228)
    std::vector<int32_t> order;
    SetData *const data[2] = {&train_data, &test_data};
    NpySet *const sets[2] = {&train_, &test_};
    for (int w = 0; w < 2; w++) {  // one stream: the training set's order, then the test set's
      balance::shuffle_order(data[w]->count, shuffle, order);
      if (!sink) {
        if (!appendSet(*sets[w], *data[w], order)) return false;
      } else if (hip_failed(gpd_hip_train_reorder(sink, w, first[w], data[w]->count, order.data()))) {
        return false;
      } else {
        sets[w]->count += data[w]->count;
      }
    }
    printf("train_offset: %d, test_offset: %d\n", train_.count, test_.count);
    const double ti = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    total_time += ti;
    printf("Number of objects left: %3.4f\n", (double)(num_objects - i));
    printf("Time for this object: %4.2fs. Total time: %3.2fs.\n", ti, total_time);
    printf("======================================\n\n");
  }
  const int n_train = train_.count, n_test = test_.count;
  const bool closed_train = closeSet(train_), closed_test = closeSet(test_);
  if (!closed_train || !closed_test) {
    printf("ERROR: could not finish the data set files\n");
    return false;
  }
  train_.count = n_train;
  test_.count = n_test;
  printf("Generated %d training and test %d instances\n", n_train, n_test);
  printf(sink ? "Left the data in the trainer's resident sets\n" : "Wrote data to training and test databases\n");
  return true;
}

}  // namespace gpd
