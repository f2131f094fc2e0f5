// util::Cloud — see include/gpd/util/cloud.h (reference: util/cloud.cpp): the PCD reader with its LZF decompressor, the
// host-side cloud operations and the single-core host models.  Plain C++: nothing of libgpd_hip.so is called here, the
// models come from the *_model.h headers that libgpd_hip.so shares.
#include "gpd/util/cloud.h"

#include <algorithm>
#include <array>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <limits>
#include <set>
#include <sstream>

#include "../../csrc/outlier_model.h"
#include "../../csrc/plane_model.h"
#include "../../csrc/refine_model.h"
#include "../../csrc/sample_model.h"

namespace gpd {
namespace util {

Cloud::Cloud(const std::vector<float> &xyz, const std::vector<float> &normals, const std::vector<int> &camera_source,
             const std::vector<double> &view_points)
    : xyz_(xyz), normals_(normals), camera_source_(camera_source), view_points_(view_points) {
  if (camera_source_.empty()) camera_source_.assign(size() * std::max(1, numCameras()), 1);
}

namespace {
// LZF (liblzf's stream format, what pcl::lzfDecompress reads): a control byte below 32 starts a run of ctrl + 1 literal
// bytes; otherwise it is a back reference of length (ctrl >> 5) + 2 (length field 7: one more byte is added to it) at
// distance ((ctrl & 31) << 8 | next byte) + 1.  Returns false unless exactly out_len bytes come out of a well-formed stream.
bool lzfDecompress(const unsigned char *in, size_t in_len, unsigned char *out, size_t out_len) {
  size_t ip = 0, op = 0;
  while (ip < in_len) {
    unsigned ctrl = in[ip++];
    if (ctrl < 32) {
      const size_t run = ctrl + 1;
      if (ip + run > in_len || op + run > out_len) return false;
      std::memcpy(out + op, in + ip, run);
      ip += run;
      op += run;
    } else {
      size_t len = ctrl >> 5;
      if (len == 7) {
        if (ip >= in_len) return false;
        len += in[ip++];
      }
      if (ip >= in_len) return false;
      const size_t dist = (((size_t)ctrl & 31) << 8 | in[ip++]) + 1;
      len += 2;
      if (dist > op || op + len > out_len) return false;
      for (size_t k = 0; k < len; k++, op++) out[op] = out[op - dist];  // overlapping copies repeat the pattern
    }
  }
  return op == out_len;
}
}  // namespace

Cloud::Cloud(const std::string &filename, const std::vector<double> &view_points) : view_points_(view_points) {
  // pcl::io::loadPCDFile (cloud.cpp:643-660): the ASCII, the binary and the binary_compressed (LZF, fields-major) layout
  std::ifstream f(filename.c_str(), std::ios::binary);
  if (!f) {
    printf("Couldn't read .pcd file: %s\n", filename.c_str());
    return;
  }
  std::string line;
  std::vector<std::string> fields, types;
  std::vector<int> sizes, counts;
  std::string kind;
  size_t points = 0;
  while (std::getline(f, line)) {
    if (!line.empty() && line.back() == '\r') line.pop_back();
    std::stringstream ss(line);
    std::string tag;
    ss >> tag;
    if (tag == "FIELDS") {
      std::string x;
      while (ss >> x) fields.push_back(x);
    } else if (tag == "SIZE") {
      int x;
      while (ss >> x) sizes.push_back(x);
    } else if (tag == "TYPE") {
      std::string x;
      while (ss >> x) types.push_back(x);
    } else if (tag == "COUNT") {
      int x;
      while (ss >> x) counts.push_back(x);
    } else if (tag == "POINTS") {
      ss >> points;
    } else if (tag == "DATA") {
      ss >> kind;
      break;
    }
  }
  if (kind != "ascii" && kind != "binary" && kind != "binary_compressed") {
    printf("Unknown .pcd data layout (DATA %s): %s\n", kind.c_str(), filename.c_str());
    return;
  }
  // an untrusted header: field counts must agree, sizes are 1 / 2 / 4 / 8 bytes, counts at least 1 and small
  counts.resize(fields.size(), 1);
  bool header_ok = !fields.empty() && fields.size() <= 64 && (sizes.empty() || sizes.size() == fields.size()) &&
                   (types.empty() || types.size() == fields.size()) && points <= ((size_t)1 << 31);
  for (int v : sizes) header_ok = header_ok && (v == 1 || v == 2 || v == 4 || v == 8);
  for (int v : counts) header_ok = header_ok && v >= 1 && v <= 1024;
  if (!header_ok) {
    printf("PCD header is malformed (FIELDS / SIZE / TYPE / COUNT / POINTS): %s\n", filename.c_str());
    return;
  }
  int ix = -1, iy = -1, iz = -1, inx = -1, iny = -1, inz = -1;
  for (int i = 0; i < (int)fields.size(); i++) {
    if (fields[i] == "x") ix = i;
    if (fields[i] == "y") iy = i;
    if (fields[i] == "z") iz = i;
    if (fields[i] == "normal_x") inx = i;
    if (fields[i] == "normal_y") iny = i;
    if (fields[i] == "normal_z") inz = i;
  }
  if (ix < 0 || iy < 0 || iz < 0) {
    printf("PCD file has no x y z fields: %s\n", filename.c_str());
    return;
  }
  const bool with_normals = inx >= 0 && iny >= 0 && inz >= 0;
  auto keep = [&](const double *row) {
    if (row[ix] != row[ix] || row[iy] != row[iy] || row[iz] != row[iz]) return;  // removeNans
    xyz_.push_back((float)row[ix]);
    xyz_.push_back((float)row[iy]);
    xyz_.push_back((float)row[iz]);
    if (with_normals) {
      normals_.push_back((float)row[inx]);
      normals_.push_back((float)row[iny]);
      normals_.push_back((float)row[inz]);
    }
  };
  std::vector<double> row(fields.size());
  if (kind == "ascii") {
    while (std::getline(f, line)) {
      std::stringstream ss(line);
      bool good = true;
      for (size_t i = 0; i < fields.size() && good; i++)
        for (int c = 0; c < counts[i] && good; c++) {  // a field of COUNT n takes n columns; its first value is kept
          double v;
          if (!(ss >> v)) good = false;
          if (c == 0) row[i] = v;
        }
      if (good) keep(row.data());
    }
  } else {
    // one record per point: the fields back to back, SIZE bytes each (x COUNT), little endian
    if (sizes.size() != fields.size() || types.size() != fields.size()) {
      printf("PCD header is incomplete (SIZE / TYPE): %s\n", filename.c_str());
      return;
    }
    std::vector<size_t> offset(fields.size());
    size_t stride = 0;
    for (size_t i = 0; i < fields.size(); i++) {
      offset[i] = stride;
      stride += (size_t)sizes[i] * (size_t)counts[i];
    }
    auto value = [&](size_t i, const char *p) {
      double v = 0.0;
      if (types[i] == "F" && sizes[i] == 4) {
        float x;
        std::memcpy(&x, p, 4);
        v = x;
      } else if (types[i] == "F" && sizes[i] == 8) {
        std::memcpy(&v, p, 8);
      } else if (sizes[i] == 4) {
        int32_t x;
        std::memcpy(&x, p, 4);
        v = types[i] == "U" ? (double)(uint32_t)x : (double)x;
      } else if (sizes[i] == 2) {
        int16_t x;
        std::memcpy(&x, p, 2);
        v = types[i] == "U" ? (double)(uint16_t)x : (double)x;
      } else if (sizes[i] == 1) {
        v = types[i] == "U" ? (double)(uint8_t)p[0] : (double)(int8_t)p[0];
      }
      return v;
    };
    if (kind == "binary") {
      std::vector<char> rec(stride);
      for (size_t n = 0; n < points && f.read(rec.data(), (std::streamsize)stride); n++) {
        for (size_t i = 0; i < fields.size(); i++) row[i] = value(i, rec.data() + offset[i]);
        keep(row.data());
      }
    } else {
      // binary_compressed (PCDWriter::writeBinaryCompressed): two little-endian uint32 (compressed, uncompressed byte
      // count), then one LZF stream of the cloud stored fields-major (all x, all y, ...; a field of COUNT n keeps its n
      // values of a point together)
      uint32_t head[2];
      if (!f.read(reinterpret_cast<char *>(head), 8)) {
        printf("PCD file ends inside the compression header: %s\n", filename.c_str());
        return;
      }
      const size_t comp = head[0], raw = head[1];
      if (raw != stride * points) {
        printf("PCD compressed block does not match the header (%zu bytes for %zu points of %zu): %s\n", raw, points, stride,
               filename.c_str());
        return;
      }
      // the 8-byte block header is not trusted: the compressed size cannot exceed what is left of the file (a crafted
      // header would otherwise ask for up to 4 GiB before a single byte is read)
      const std::streampos here = f.tellg();
      f.seekg(0, std::ios::end);
      const std::streampos end = f.tellg();
      f.seekg(here);
      if (here < 0 || end < here || comp > (size_t)(end - here)) {
        printf("PCD file ends inside the compressed block: %s\n", filename.c_str());
        return;
      }
      std::vector<unsigned char> in;
      std::vector<char> out;
      try {
        in.resize(comp);
        out.resize(raw);
      } catch (const std::bad_alloc &) {
        printf("PCD compressed block is corrupt (%zu / %zu bytes cannot be held): %s\n", comp, raw, filename.c_str());
        return;
      }
      if (comp && !f.read(reinterpret_cast<char *>(in.data()), (std::streamsize)comp)) {
        printf("PCD file ends inside the compressed block: %s\n", filename.c_str());
        return;
      }
      if (!lzfDecompress(in.data(), comp, reinterpret_cast<unsigned char *>(out.data()), raw)) {
        printf("PCD compressed block is corrupt: %s\n", filename.c_str());
        return;
      }
      std::vector<size_t> base(fields.size());
      for (size_t i = 0; i < fields.size(); i++) base[i] = offset[i] * points;
      for (size_t n = 0; n < points; n++) {
        for (size_t i = 0; i < fields.size(); i++) row[i] = value(i, out.data() + base[i] + n * (size_t)sizes[i] * (size_t)counts[i]);
        keep(row.data());
      }
    }
  }
  if (view_points_.empty()) view_points_.assign(3, 0.0);
  camera_source_.assign(size() * numCameras(), 1);
}

namespace {
struct VoxelDiffers {  // UniqueVector4First3Comparator (cloud.h:105-122)
  bool operator()(const std::array<int, 4> &a, const std::array<int, 4> &b) const {
    return a[0] != b[0] || a[1] != b[1] || a[2] != b[2];
  }
};
}  // namespace

void Cloud::setProcessed(const std::vector<float> &xyz, const std::vector<int> &camera_source, const std::vector<float> &normals) {
  xyz_ = xyz;
  camera_source_ = camera_source;
  normals_ = normals;
}

void Cloud::filterWorkspaceSamples(const std::vector<double> &ws) {
  if (ws.size() < 6) return;
  auto inside = [&](double x, double y, double z) { return x > ws[0] && x < ws[1] && y > ws[2] && y < ws[3] && z > ws[4] && z < ws[5]; };
  if (!sample_indices_.empty()) {
    std::vector<int> keep;
    for (int i = 0; i < (int)sample_indices_.size(); i++) {
      const float *p = &xyz_[3 * (size_t)sample_indices_[i]];
      if (inside(p[0], p[1], p[2])) keep.push_back(i);  // the position, as cloud.cpp:215 stores it
    }
    sample_indices_ = keep;
    std::cout << sample_indices_.size() << " sample indices left after workspace filtering \n";
  }
  if (samples_.size() >= 3) {
    std::vector<double> keep;
    for (size_t i = 0; i + 2 < samples_.size(); i += 3)
      if (inside(samples_[i], samples_[i + 1], samples_[i + 2])) keep.insert(keep.end(), samples_.begin() + i, samples_.begin() + i + 3);
    samples_ = keep;
    std::cout << samples_.size() / 3 << " samples left after workspace filtering \n";
  }
}

void Cloud::filterWorkspace(const std::vector<double> &ws) {
  if (ws.size() < 6) return;
  auto inside = [&](double x, double y, double z) { return x > ws[0] && x < ws[1] && y > ws[2] && y < ws[3] && z > ws[4] && z < ws[5]; };
  filterWorkspaceSamples(ws);
  const size_t n = size();
  const int cams = numCameras();
  const bool with_normals = hasNormals();
  std::vector<size_t> idx;
  for (size_t i = 0; i < n; i++)
    if (inside(xyz_[3 * i], xyz_[3 * i + 1], xyz_[3 * i + 2])) idx.push_back(i);
  std::vector<float> xyz(idx.size() * 3), normals(with_normals ? idx.size() * 3 : 0);
  std::vector<int> cam((size_t)cams * idx.size());
  for (size_t k = 0; k < idx.size(); k++) {
    for (int r = 0; r < 3; r++) {
      xyz[3 * k + r] = xyz_[3 * idx[k] + r];
      if (with_normals) normals[3 * k + r] = normals_[3 * idx[k] + r];
    }
    for (int c = 0; c < cams; c++) cam[(size_t)c * idx.size() + k] = camera_source_[(size_t)c * n + idx[k]];
  }
  xyz_ = xyz;
  normals_ = normals;
  camera_source_ = cam;
}

void Cloud::setNormalsFromFile(const std::string &filename) {
  std::ifstream in(filename.c_str());
  std::string line;
  std::vector<float> normals(xyz_.size(), 0.f);
  size_t i = 0;
  while (i < 3 && std::getline(in, line)) {
    std::stringstream ls(line);
    std::string cell;
    size_t j = 0;
    while (std::getline(ls, cell, ',')) {
      if (j < size()) {
        char *end = nullptr;
        const double v = std::strtod(cell.c_str(), &end);
        if (end == cell.c_str()) {  // not a number: the file is refused as a whole (std::stod would throw)
          printf("ERROR: cannot parse the normals file %s\n", filename.c_str());
          return;
        }
        normals[3 * j + i] = (float)v;
      }
      j++;
    }
    i++;
  }
  if (i == 3) normals_ = normals;
}

void Cloud::voxelizeCloud(float cell_size) {
  const int n = (int)size();
  if (n == 0) return;
  float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
  for (int i = 0; i < n; i++)
    for (int c = 0; c < 3; c++) mn[c] = std::min(mn[c], xyz_[3 * i + c]);
  std::set<std::array<int, 4>, VoxelDiffers> bins;
  for (int i = 0; i < n; i++) {
    std::array<int, 4> v;
    for (int c = 0; c < 3; c++) v[c] = (int)std::floor((xyz_[3 * i + c] - mn[c]) / cell_size);
    v[3] = i;
    bins.insert(v);
  }
  const int cams = numCameras();
  std::vector<float> out;
  std::vector<int> cam((size_t)cams * bins.size());
  size_t k = 0;
  for (const auto &v : bins) {
    for (int c = 0; c < 3; c++) out.push_back(mn[c] + cell_size * (float)v[c]);
    for (int j = 0; j < cams; j++) cam[(size_t)j * bins.size() + k] = camera_source_[(size_t)j * n + v[3]] == 1 ? 1 : 0;
    k++;
  }
  xyz_ = out;
  camera_source_ = cam;
  normals_.clear();
  sample_indices_.clear();
  printf("Voxelized cloud: %zu\n", size());
}

Cloud::PlaneFit Cloud::sampleAbovePlane(double threshold, int max_iterations, double probability, bool optimize) {
  const auto t0 = std::chrono::steady_clock::now();
  printf("Sampling above plane ...\n");
  const plane::Result r = plane::fit(xyz_.data(), (int)size(), threshold, max_iterations, probability, optimize);
  PlaneFit fit;
  fit.above = r.above;
  for (int a = 0; a < 4; a++) fit.coeffs[a] = r.coeffs[a];
  fit.num_inliers = r.num_inliers;
  fit.iterations = r.iterations;
  applyPlaneFit(fit, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  return fit;
}

void Cloud::applyPlaneFit(const PlaneFit &fit, double seconds) {
  if (!fit.above.empty()) {
    sample_indices_ = fit.above;
    printf(" Plane fit succeeded. %zu samples above plane.\n", sample_indices_.size());
  } else {
    printf(" Plane fit failed. Using entire point cloud ...\n");
  }
  std::cout << " runtime (plane fit): " << seconds << "\n";
}

Cloud::NormalRefinement Cloud::refineNormals(int k, int max_iterations, float convergence_threshold) {
  NormalRefinement out;
  if (!hasNormals() || k < 1) return out;
  std::vector<int32_t> lists;
  const int kk = refine::knn(xyz_.data(), (int)size(), k, lists);
  refine::Result r = refine::refine(normals_.data(), (int)size(), lists.data(), kk, max_iterations, convergence_threshold);
  out.iterations = r.iterations;
  out.ddots = r.ddots;
  out.num_nan = r.num_nan;
  applyRefinedNormals(r.normals);
  return out;
}

// The reference prints the statistics of (refined - input) over pcl::Normal's 8-float map, whose padding and curvature rows
// are zero in both (the four extra rows add nothing to the sum and max, and dilute the mean by 8 / 3); here they are taken
// over the three normal rows alone.
void Cloud::applyRefinedNormals(const std::vector<float> &refined) {
  float mx = -std::numeric_limits<float>::infinity(), sum = 0.f;
  for (size_t i = 0; i < refined.size(); i++) {
    const float d = refined[i] - normals_[i];
    sum += d;
    mx = std::isnan(d) || d > mx ? d : mx;
  }
  const float mean = sum / (float)refined.size();
  printf("Refining surface normals ...\n");
  printf(" mean: %.3f, max: %.3f, sum: %.3f\n", mean, mx, sum);
  normals_ = refined;
}

Cloud::OutlierRemoval Cloud::removeStatisticalOutliers(int mean_k, double stddev_mult) {
  OutlierRemoval out;
  if (outlier::refusal((int)size(), mean_k, stddev_mult)) return out;
  const outlier::Result r = outlier::filter(xyz_.data(), (int)size(), mean_k, stddev_mult);
  out.ok = true;
  out.kept.assign(r.kept.begin(), r.kept.end());
  out.mean = r.stats.mean;
  out.stddev = r.stats.stddev;
  out.threshold = r.stats.threshold;
  out.dist = r.dist;
  applyOutlierRemoval(out.kept);
  return out;
}

void Cloud::applyOutlierRemoval(const std::vector<int> &kept) {
  const size_t n = size(), m = kept.size();
  const int cams = numCameras();
  const bool with_normals = hasNormals();
  std::vector<float> xyz(m * 3), normals(with_normals ? m * 3 : 0);
  std::vector<int> cam((size_t)cams * m), new_index(n, -1);
  for (size_t k = 0; k < m; k++) {
    new_index[kept[k]] = (int)k;
    for (int r = 0; r < 3; r++) {
      xyz[3 * k + r] = xyz_[3 * (size_t)kept[k] + r];
      if (with_normals) normals[3 * k + r] = normals_[3 * (size_t)kept[k] + r];
    }
    for (int c = 0; c < cams; c++) cam[(size_t)c * m + k] = camera_source_[(size_t)c * n + kept[k]];
  }
  std::vector<int> samples;
  for (int i : sample_indices_)
    if (i >= 0 && (size_t)i < n && new_index[i] >= 0) samples.push_back(new_index[i]);
  setProcessed(xyz, cam, normals);
  sample_indices_ = samples;
  printf("Cloud after removing statistical outliers: %zu\n", size());
}

// Cloud::subsample (cloud.cpp:350-405): samples given by coordinates are thinned to num_samples of them without
// repetition (subsampleSamples), sample indices are redrawn num_samples times WITH repetition
// (subsampleSampleIndices: sample_indices_[rand() % size]), otherwise num_samples points are drawn uniformly
// (subsampleUniformly).  The reference's generators are time-seeded; here one seeded xorshift.
void Cloud::subsample(int num_samples, unsigned seed) {
  if (num_samples <= 0) return;
  std::vector<int32_t> pos;  // the draws: ../../csrc/sample_model.h, shared with libgpd_hip.so
  if (samples_.size() >= 3) {
    const int have = (int)(samples_.size() / 3);
    if (num_samples >= have) return;
    printf("Using %d out of %d available samples.\n", num_samples, have);
    gpd::sample::distinct(have, num_samples, seed, pos);
    std::vector<double> sub((size_t)num_samples * 3);
    for (int i = 0; i < num_samples; i++)
      for (int r = 0; r < 3; r++) sub[3 * (size_t)i + r] = samples_[3 * (size_t)pos[(size_t)i] + r];
    samples_ = sub;
    return;
  }
  if (!sample_indices_.empty()) {
    if (num_samples >= (int)sample_indices_.size()) return;
    gpd::sample::with_repetition((int)sample_indices_.size(), num_samples, seed, pos);
    std::vector<int> indices(num_samples);
    for (int i = 0; i < num_samples; i++) indices[i] = sample_indices_[(size_t)pos[(size_t)i]];
    sample_indices_ = indices;
    return;
  }
  const int n = (int)size();
  if (n == 0) return;
  gpd::sample::distinct(n, num_samples, seed, pos);
  sample_indices_.assign(pos.begin(), pos.end());
}

}  // namespace util
}  // namespace gpd
