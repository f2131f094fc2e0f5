// The extern "C" gpd_host_* entries of libgpd_host.so: flat hooks into the classes for callers without them (tests, ctypes:
// gpd_amd/hostlib.py).
#include <algorithm>
#include <cstring>

#include "gpd/data_generator.h"
#include "host_internal.h"
#include "../../csrc/outlier_model.h"
#include "../../csrc/plane_model.h"
#include "../../csrc/refine_model.h"

// the detector of the two detector hooks: the reference's default geometry (gpd_hip_default_params), no samples, device 0
static gpd::GraspDetector default_detector() {
  gpd_params p;
  gpd_hip_default_params(&p);
  return gpd::GraspDetector(gpd::hand_search_parameters(p, 0),
                            {p.volume_width, p.volume_depth, p.volume_height, p.image_size, p.image_num_channels}, 0);
}

// Flat entry for callers without the C++ classes (tests, ctypes): cluster n records with double
// scores; out / out_scores / out_src (the index of the seeding hand) hold up to n results.
extern "C" int gpd_host_find_clusters(const gpd_hand *hands, const double *scores, int n, int min_inliers, int remove_inliers,
                                      gpd_hand *out, double *out_scores, int *out_src) {
  std::vector<std::unique_ptr<gpd::candidate::Hand>> list;
  for (int i = 0; i < n; i++) {
    gpd_hand r = hands[i];
    r.slot = i;  // carries the source index through the copy
    list.push_back(std::make_unique<gpd::candidate::Hand>(r));
    list.back()->setScore(scores[i]);
  }
  gpd::Clustering c(min_inliers);
  auto res = c.findClusters(list, remove_inliers != 0);
  for (size_t k = 0; k < res.size(); k++) {
    out[k] = res[k]->record();
    out_src[k] = out[k].slot;
    out[k].slot = hands[out_src[k]].slot;
    out_scores[k] = res[k]->getScore();
  }
  return (int)res.size();
}

// Flat entry for tests / ctypes: util::Cloud::sampleAbovePlane's fit on xyz [n][3]; above holds n entries.  Returns the
// number of points off the plane (0: the fit failed).
extern "C" int gpd_host_sample_above_plane(const float *xyz, int n, double threshold, int max_iterations, double probability, int optimize,
                                           int *above, float *coeffs, int *num_inliers, int *iterations) {
  const gpd::plane::Result r = gpd::plane::fit(xyz, n, threshold, max_iterations, probability, optimize != 0);
  std::copy(r.above.begin(), r.above.end(), above);
  for (int a = 0; a < 4; a++) coeffs[a] = r.coeffs[a];
  *num_inliers = r.num_inliers;
  *iterations = r.iterations;
  return (int)r.above.size();
}

// Flat entry for tests / ctypes: util::Cloud::refineNormals on xyz / normals [n][3] (the host model); normals_out [n][3],
// ddots holds max_iterations floats.  Returns the passes run; *num_nan: refined normals with a non-finite component.
extern "C" int gpd_host_refine_normals(const float *xyz, const float *normals, int n, int k, int max_iterations, float convergence_threshold,
                                       float *normals_out, float *ddots, int *num_nan) {
  std::vector<int32_t> lists;
  const int kk = gpd::refine::knn(xyz, n, k, lists);
  const gpd::refine::Result r = gpd::refine::refine(normals, n, lists.data(), kk, max_iterations, convergence_threshold);
  std::copy(r.normals.begin(), r.normals.end(), normals_out);
  std::copy(r.ddots.begin(), r.ddots.end(), ddots);
  *num_nan = r.num_nan;
  return r.iterations;
}

// Flat entry for tests / ctypes: the host model of removeStatisticalOutliers on xyz [n][3]; kept and dist hold n entries,
// stats 3.  Returns the number of kept points, -1 outside the domain (invalid), -2 beyond the capacity.
extern "C" int gpd_host_remove_statistical_outliers(const float *xyz, int n, int mean_k, double stddev_mult, int32_t *kept, double *stats,
                                                    float *dist) {
  if (const int why = gpd::outlier::refusal(n, mean_k, stddev_mult)) return -why;
  const gpd::outlier::Result r = gpd::outlier::filter(xyz, n, mean_k, stddev_mult);
  std::copy(r.kept.begin(), r.kept.end(), kept);
  std::copy(r.dist.begin(), r.dist.end(), dist);
  stats[0] = r.stats.mean;
  stats[1] = r.stats.stddev;
  stats[2] = r.stats.threshold;
  return (int)r.kept.size();
}

// Flat entry for tests / ctypes: util::Cloud::removeStatisticalOutliers on a cloud of `cams` cameras that carries normals
// (may be null), camera-source rows [cams][n] and sample indices: what the cloud holds afterwards.  xyz_out / normals_out
// [n][3], cam_out [cams][kept], samples_out [num_samples].  Returns the kept points (-1: refused), *num_samples_out the
// sample indices left.
extern "C" int gpd_host_cloud_remove_statistical_outliers(const float *xyz, const float *normals, const int *cam, int n, int cams,
                                                          const int *samples, int num_samples, int mean_k, double stddev_mult, float *xyz_out,
                                                          float *normals_out, int *cam_out, int *samples_out, int *num_samples_out) {
  gpd::util::Cloud cloud(std::vector<float>(xyz, xyz + 3 * (size_t)n),
                         normals ? std::vector<float>(normals, normals + 3 * (size_t)n) : std::vector<float>(),
                         std::vector<int>(cam, cam + (size_t)cams * n), std::vector<double>(3 * (size_t)cams, 0.0));
  cloud.setSampleIndices(std::vector<int>(samples, samples + num_samples));
  if (!cloud.removeStatisticalOutliers(mean_k, stddev_mult).ok) return -1;
  fflush(stdout);
  std::copy(cloud.getCloudProcessed().begin(), cloud.getCloudProcessed().end(), xyz_out);
  if (normals) std::copy(cloud.getNormals().begin(), cloud.getNormals().end(), normals_out);
  std::copy(cloud.getCameraSource().begin(), cloud.getCameraSource().end(), cam_out);
  std::copy(cloud.getSampleIndices().begin(), cloud.getSampleIndices().end(), samples_out);
  *num_samples_out = (int)cloud.getSampleIndices().size();
  return (int)cloud.size();
}

// Flat entry for tests / ctypes: util::Cloud::subsample on a cloud of num_points points that carries the sample indices
// `list` (num_list of them; 0: none).  out holds max(num_list, num_samples, 0) entries; returns how many sample indices
// the cloud carries afterwards.
extern "C" int gpd_host_subsample_indices(int num_points, const int *list, int num_list, int num_samples, unsigned seed, int *out) {
  const std::vector<float> xyz((size_t)(num_points > 0 ? num_points : 0) * 3, 0.f);
  gpd::util::Cloud cloud(xyz, std::vector<float>(), std::vector<int>(xyz.size() / 3, 1), {0.0, 0.0, 0.0});
  if (num_list > 0) cloud.setSampleIndices(std::vector<int>(list, list + num_list));
  cloud.subsample(num_samples, seed);
  const std::vector<int> &idx = cloud.getSampleIndices();
  std::copy(idx.begin(), idx.end(), out);
  return (int)idx.size();
}

// Flat entry for tests / ctypes: the host model's kNN lists [n][min(k, n)] (the (d2, index) order); returns min(k, n)
extern "C" int gpd_host_knn(const float *xyz, int n, int k, int32_t *lists) {
  std::vector<int32_t> out;
  const int kk = gpd::refine::knn(xyz, n, k, out);
  std::copy(out.begin(), out.end(), lists);
  return kk;
}

// Flat entry for tests / ctypes: GraspDetector::refineNormals on a cloud of one camera at the origin, through a detector
// of the reference's default geometry on device 0.  normals_out [n][3]; returns 0, or -1 when the device call failed.
extern "C" int gpd_host_detector_refine_normals(const float *xyz, const float *normals, int n, int k, float *normals_out) {
  gpd::GraspDetector detector = default_detector();
  gpd::util::Cloud cloud(std::vector<float>(xyz, xyz + 3 * (size_t)n), std::vector<float>(normals, normals + 3 * (size_t)n),
                         std::vector<int>((size_t)n, 1), std::vector<double>(3, 0.0));
  if (!detector.refineNormals(cloud, k)) return -1;
  std::copy(cloud.getNormals().begin(), cloud.getNormals().end(), normals_out);
  return 0;
}

// Flat entry for tests / ctypes: GraspDetector::removeStatisticalOutliers on a cloud of one camera at the origin that carries
// normals and sample indices, through a detector as above.  xyz_out / normals_out [n][3], samples_out [num_samples]; returns
// the kept points (-1: the device call failed), *num_samples_out the sample indices left.
extern "C" int gpd_host_detector_remove_statistical_outliers(const float *xyz, const float *normals, int n, const int *samples, int num_samples,
                                                             int mean_k, double stddev_mult, float *xyz_out, float *normals_out,
                                                             int *samples_out, int *num_samples_out) {
  gpd::GraspDetector detector = default_detector();
  gpd::util::Cloud cloud(std::vector<float>(xyz, xyz + 3 * (size_t)n), std::vector<float>(normals, normals + 3 * (size_t)n),
                         std::vector<int>((size_t)n, 1), std::vector<double>(3, 0.0));
  cloud.setSampleIndices(std::vector<int>(samples, samples + num_samples));
  if (!detector.removeStatisticalOutliers(cloud, mean_k, stddev_mult)) return -1;
  fflush(stdout);
  std::copy(cloud.getCloudProcessed().begin(), cloud.getCloudProcessed().end(), xyz_out);
  std::copy(cloud.getNormals().begin(), cloud.getNormals().end(), normals_out);
  std::copy(cloud.getSampleIndices().begin(), cloud.getSampleIndices().end(), samples_out);
  *num_samples_out = (int)cloud.getSampleIndices().size();
  return (int)cloud.size();
}

// Flat entry for tests / ctypes: loads a PCD like util::Cloud does; returns the number of points
// (at most cap are copied), *has_normals tells whether normal_x/y/z fields were present.
extern "C" int gpd_host_load_pcd(const char *path, float *xyz, float *normals, int cap, int *has_normals) {
  gpd::util::Cloud cloud(path, {0.0, 0.0, 0.0});
  const int n = (int)cloud.size();
  if (has_normals) *has_normals = cloud.hasNormals() ? 1 : 0;
  const int m = n < cap ? n : cap;
  if (xyz && m > 0) std::memcpy(xyz, cloud.getCloudProcessed().data(), (size_t)m * 3 * sizeof(float));
  if (normals && cloud.hasNormals() && m > 0) std::memcpy(normals, cloud.getNormals().data(), (size_t)m * 3 * sizeof(float));
  return n;
}

extern "C" int gpd_host_load_normals_csv(const char *pcd_path, const char *csv_path, float *normals, int cap) {
  gpd::util::Cloud cloud(pcd_path, {0.0, 0.0, 0.0});
  cloud.setNormalsFromFile(csv_path);
  if (!cloud.hasNormals()) return -1;
  const int n = (int)cloud.size(), m = n < cap ? n : cap;
  std::memcpy(normals, cloud.getNormals().data(), (size_t)m * 3 * sizeof(float));
  return n;
}

// DataGenerator::generateData into the resident sets of a trainer (gpd_hip_trainer *) instead of .npy files: 0 and the
// generated counts, or -1
extern "C" int gpd_host_generate_data(const char *config, void *trainer, int *n_train, int *n_test) {
  if (!config || !trainer) return -1;
  gpd::DataGenerator generator(config);
  if (!generator.ok() || !generator.generateData(static_cast<gpd_hip_trainer *>(trainer))) return -1;
  if (n_train) *n_train = generator.numTrain();
  if (n_test) *n_test = generator.numTest();
  fflush(stdout);
  return 0;
}
