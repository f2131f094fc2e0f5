// util::Cloud — the part of the reference's PCL wrapper that the hot path reads
// (util/cloud.h: getCloudProcessed, getNormals, getCameraSource, getViewPoints,
// getSampleIndices/setSampleIndices, getSamples/setSamples, subsample, voxelizeCloud).  Normal
// estimation runs on the device (gpd_hip_estimate_normals) from GraspDetector::preprocessPointCloud.
#pragma once
#include <string>
#include <vector>

namespace gpd {
namespace util {

class Cloud {
 public:
  Cloud() {}
  // xyz / normals: 3 floats per point; camera_source: n_cams x P (0/1); view_points: 3 doubles per camera
  Cloud(const std::vector<float> &xyz, const std::vector<float> &normals, const std::vector<int> &camera_source,
        const std::vector<double> &view_points);
  // ASCII PCD with FIELDS x y z [normal_x normal_y normal_z ...] (pcl::io::loadPCDFile, cloud.cpp:643-660)
  Cloud(const std::string &filename, const std::vector<double> &view_points);

  size_t size() const { return xyz_.size() / 3; }
  bool hasNormals() const { return normals_.size() == xyz_.size() && !xyz_.empty(); }
  const std::vector<float> &getCloudProcessed() const { return xyz_; }
  const std::vector<float> &getNormals() const { return normals_; }
  const std::vector<int> &getCameraSource() const { return camera_source_; }
  const std::vector<double> &getViewPoints() const { return view_points_; }
  int numCameras() const { return (int)(view_points_.size() / 3); }
  const std::vector<int> &getSampleIndices() const { return sample_indices_; }
  void setSampleIndices(const std::vector<int> &idx) { sample_indices_ = idx; }
  // Cloud::getSamples / setSamples (cloud.h:248-262): samples by coordinates, 3 doubles each; when
  // present they take precedence over the indices (hand_search.cpp:37-44)
  const std::vector<double> &getSamples() const { return samples_; }
  void setSamples(const std::vector<double> &samples) { samples_ = samples; }
  void setNormals(const std::vector<float> &normals) { normals_ = normals; }
  // Cloud::setNormalsFromFile (cloud.cpp:622-641): a CSV of three rows (x, y, z components) with one
  // column per point.  The device boundary carries float32 normals (the reference keeps these doubles).
  void setNormalsFromFile(const std::string &filename);
  // Cloud::filterWorkspace (cloud.cpp:206-267): keeps the points (normals, camera columns) strictly inside
  // the box [x0 x1 y0 y1 z0 z1]; samples by coordinate likewise.  As in the reference the sample
  // INDICES are replaced by the positions of the surviving entries (:215) and not remapped to the
  // filtered cloud — call it before sampling, as preprocessPointCloud does.
  void filterWorkspace(const std::vector<double> &workspace);
  // its first two blocks alone (cloud.cpp:208-241): sample indices and samples by coordinate; the detector runs the
  // third one — the points — on the device (gpd_hip_preprocess_cloud) and hands the result back through setProcessed
  void filterWorkspaceSamples(const std::vector<double> &workspace);
  // replaces points and camera source (rows of xyz.size() / 3); normals may be empty; sample indices are kept
  void setProcessed(const std::vector<float> &xyz, const std::vector<int> &camera_source, const std::vector<float> &normals);
  // Cloud::voxelizeCloud (cloud.cpp:286-348), including what its std::set comparator (cloud.h:105-122,
  // not an ordering) keeps under libstdc++; drops normals like the reference's preprocessing order does.
  void voxelizeCloud(float cell_size);
  // Cloud::subsample (cloud.cpp:350-405) draws with pcl::RandomSample (time-seeded); here a
  // seeded Fisher-Yates permutation so runs are reproducible.
  void subsample(int num_samples, unsigned seed = 0);
  // Cloud::sampleAbovePlane (cloud.cpp:407-436): PCL 1.9's RANSAC plane fit (SACMODEL_PLANE, distance threshold,
  // refined when `optimize`) and the sample indices set to the points off the plane, ascending — the definition is
  // DESIGN §7.  When no plane is found or no point lies off it ("plane fit failed") the sample indices stay as they
  // are.  This is the single-core host model; GraspDetector::sampleAbovePlane runs the same fit on the device.
  struct PlaneFit {
    std::vector<int> above;  // the points off the plane (empty: the fit failed)
    float coeffs[4] = {0, 0, 0, 0};
    int num_inliers = 0, iterations = 0;
  };
  PlaneFit sampleAbovePlane(double threshold = 0.01, int max_iterations = 50, double probability = 0.99, bool optimize = true);
  // what sampleAbovePlane does with a fit: the reference's messages, the sample indices replaced when it succeeded
  void applyPlaneFit(const PlaneFit &fit, double seconds);
  // Cloud::refineNormals (cloud.cpp:176-204): the k nearest neighbours of every point (pcl::search::KdTree, sorted by
  // (d2, index), k clamped to the cloud's size), then pcl::NormalRefinement with max_iterations passes and the
  // convergence threshold (the reference's defaults 15 and 1e-5) — the definition is DESIGN §7.  The normals become the
  // refined ones (NaN where the refinement met a singularity).  This is the single-core host model;
  // GraspDetector::refineNormals runs the same refinement on the device.  A cloud without normals is left as it is.
  struct NormalRefinement {
    int iterations = 0;        // passes run
    std::vector<float> ddots;  // the stop rule's mean dot product of every pass
    int num_nan = 0;           // refined normals with a non-finite component
  };
  NormalRefinement refineNormals(int k, int max_iterations = 15, float convergence_threshold = 1e-5f);
  // what refineNormals does with refined normals: the reference's messages, then the normals replaced
  void applyRefinedNormals(const std::vector<float> &refined);
  // Cloud::removeStatisticalOutliers (cloud.cpp:166-174): pcl::StatisticalOutlierRemoval with setMeanK(mean_k) and
  // setStddevMulThresh(stddev_mult) — the definition is DESIGN §7.  Unlike the reference's sor.filter(*cloud_processed_),
  // which leaves camera_source_, normals_ and the sample indices misaligned, the camera-source columns and the normals
  // follow their points, and the sample indices are remapped to the kept cloud (those of removed points are dropped, the
  // order stays).  This is the single-core host model; GraspDetector::removeStatisticalOutliers runs the same filter on
  // the device.  Outside the domain (mean_k < 1 or > 255, a non-finite multiplier, fewer than mean_k + 1 points) the cloud
  // is left as it is and `ok` is false.
  struct OutlierRemoval {
    bool ok = false;
    std::vector<int> kept;                  // the kept input indices, ascending
    double mean = 0, stddev = 0, threshold = 0;
    std::vector<float> dist;                // the mean neighbour distance of every input point
  };
  OutlierRemoval removeStatisticalOutliers(int mean_k = 50, double stddev_mult = 1.0);
  // what removeStatisticalOutliers does with the kept indices (ascending): points, normals, camera columns gathered, the
  // sample indices remapped, then the reference's message
  void applyOutlierRemoval(const std::vector<int> &kept);

 private:
  std::vector<float> xyz_, normals_;
  std::vector<int> camera_source_;
  std::vector<double> view_points_;
  std::vector<int> sample_indices_;
  std::vector<double> samples_;
};

}  // namespace util
}  // namespace gpd
