// gpd::DataGenerator — the reference's training-set generator (include/gpd/data_generator.h, src/gpd/data_generator.cpp)
// over the HIP path: for every object its mesh becomes the context's resident ground truth, every view is one
// gpd_hip_label_view call (rounds of createGraspImages + evalGroundTruth on the device, balanceInstances, one copy of the
// kept instances), and the balanced (image, label) sets are written for pytorch/train_net3.py.
// Departures from the reference (DESIGN "generate_data"): every round's indices are shifted by the accumulated count; the
// rounds of a view are bounded (cfg max_rounds_per_view); the sample draws and the shuffle are seeded (cfg sample_seed,
// shuffle_seed); the output is NumPy .npy instead of HDF5.
#pragma once
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "gpd/grasp_detector.h"

namespace gpd {

class DataGenerator {
 public:
  // cfg keys of data_generator.cpp:10-39 (data_root, objects_file_location, output_root, num_views_per_object,
  // min_grasps_per_view, max_grasps_per_view, test_views, num_samples, remove_nans, voxel_size_views, normals_radius,
  // reverse_mesh_normals, reverse_view_normals; chunk_size, max_in_memory and num_threads are read and not needed) plus
  // sample_seed (0), shuffle_seed (0), max_rounds_per_view (20); the detector's keys as GraspDetector reads them
  explicit DataGenerator(const std::string &config_filename);
  ~DataGenerator();
  bool ok() const { return detector_ && detector_->ok(); }
  // writes output_root + {train,test}_{images,labels}.npy; false when a file or a device call fails.
  // sink != nullptr: no file is opened; every view is one gpd_hip_train_append_view into the trainer's resident sets (train
  // views: set 0, test views: set 1) and after each object its range of each set is put into the stored order on the device
  // (gpd_hip_train_reorder, the same shuffle stream consumed in the same sequence): the sets end up holding the bytes the
  // four files would hold, and no image crosses to the host
  bool generateData(gpd_hip_trainer *sink = nullptr);
  int numTrain() const { return train_.count; }
  int numTest() const { return test_.count; }

 private:
  // the kept instances of an object's views, in view order: images back to back (60 * 60 * C bytes each), one label each
  struct SetData {
    std::vector<uint8_t> images, labels;  // stay empty under a sink
    int count = 0;
  };
  // one growing pair of NumPy 1.0 files: a fixed-size header, rewritten with the final row count on close
  struct NpySet {
    FILE *images = nullptr, *labels = nullptr;
    int count = 0;
  };
  static std::vector<std::string> loadObjectNames(const std::string &objects_file_location);
  bool openSet(NpySet &set, const std::string &name);
  bool appendSet(NpySet &set, const SetData &data, const std::vector<int32_t> &order);
  bool closeSet(NpySet &set);
  bool writeHeader(FILE *f, int rows, bool images) const;
  // Cloud::calculateNormals on the device at normals_radius, negated when `reverse`
  bool estimateNormals(util::Cloud &cloud, bool reverse);
  // sink != nullptr: the kept instances go behind the last image of the trainer's set `which` instead of `into`'s vectors
  bool labelView(int object, int view, util::Cloud &cloud, SetData &into, gpd_hip_trainer *sink, int which);

  std::unique_ptr<GraspDetector> detector_;
  std::string data_root_, objects_file_location_, output_root_;
  int num_views_per_object_, min_grasps_per_view_, max_grasps_per_view_, num_samples_, max_rounds_per_view_;
  std::vector<int> test_views_;
  bool remove_nans_, reverse_mesh_normals_, reverse_view_normals_;
  double voxel_size_views_, normals_radius_;
  uint32_t sample_seed_, shuffle_seed_;
  NpySet train_, test_;
};

}  // namespace gpd
