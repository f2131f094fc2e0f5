// Cloud::refineNormals(k) (util/cloud.cpp:176-204): pcl::search::KdTree<PointXYZRGBA>::nearestKSearch over every point of
// the cloud, then pcl::NormalRefinement<pcl::Normal> with its default settings — PCL 1.9 restated in DESIGN §7
// ("refineNormals").  Plain C++ with no HIP in it: the host mirror's single-core model (util::Cloud::refineNormals) runs
// knn() and refine() below, the device path (refine.hip) uses the same stop rule (StopRule) between its pass launches.
// Every float expression is written in the operation order the definition gives and must be compiled without FMA contraction.
#pragma once
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

namespace gpd {
namespace refine {

constexpr int kMaxIterations = 15;              // NormalRefinement's default max_iterations_
constexpr float kConvergenceThreshold = 1e-5f;  // ... and convergence_threshold_

inline bool finite3(float x, float y, float z) { return std::isfinite(x) && std::isfinite(y) && std::isfinite(z); }

// (d2 bits, index): FLANN's result order, ties at equal d2 by ascending index; d2 >= 0 orders as its bits
inline uint64_t key(float d2, int i) {
  uint32_t b;
  std::memcpy(&b, &d2, 4);
  return ((uint64_t)b << 32) | (uint32_t)i;
}
// FLANN L2_Simple<float>: the squared differences accumulated over x, y, z, unfused
inline float dist2(const float *q, const float *p) {
  float d2 = 0.f, d = q[0] - p[0];
  d2 += d * d;
  d = q[1] - p[1];
  d2 += d * d;
  d = q[2] - p[2];
  d2 += d * d;
  return d2;
}

// Lower bound of the float d2 from a query to any point at least R cells away from the query's cell along some axis of a grid
// of cells `cell` wide (R >= 1): the real distance along that axis is at least R cells minus what the float cell coordinates
// of the two points may be off (a few 1e-5 cells on grids of at most 256 cells per axis: 1e-3 is ample), and the float d2
// loses less than 1e-6 of itself to rounding.  R = 0 certifies nothing.
inline float ring_bound(int R, float cell) {
  if (R < 1) return 0.f;
  const double m = ((double)R - 1e-3) * (double)cell;
  return (float)(m * m * (1.0 - 1e-5));
}

// kNN of every point of xyz [n][3] by (d2, index), k clamped to n: out [n][min(k, n)].  A uniform grid (2 cm cells, doubled
// until at most 256 per axis, as the device cloud's) visited in square shells around the query's cell until the k-th key is
// closer than ring_bound, or the shell has covered the grid.
inline int knn(const float *xyz, int n, int k, std::vector<int32_t> &out) {
  out.clear();
  if (n <= 0 || k <= 0) return 0;
  const int kk = std::min(k, n);
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) {
      lo[a] = std::min(lo[a], xyz[3 * (size_t)i + a]);
      hi[a] = std::max(hi[a], xyz[3 * (size_t)i + a]);
    }
  float cell = 0.02f;
  int dim[3];
  for (;;) {
    bool ok = true;
    for (int a = 0; a < 3; a++) {
      dim[a] = (int)std::floor((hi[a] - lo[a]) / cell) + 1;
      if (dim[a] > 256 || dim[a] < 1) ok = false;
    }
    if (ok) break;
    cell *= 2.f;
  }
  auto coord = [&](int a, float v) {
    const int c = (int)std::floor((v - lo[a]) / cell);
    return c < 0 ? 0 : (c > dim[a] - 1 ? dim[a] - 1 : c);
  };
  const size_t cells = (size_t)dim[0] * dim[1] * dim[2];
  std::vector<int32_t> start(cells + 1, 0), order((size_t)n), cid((size_t)n);
  for (int i = 0; i < n; i++) {
    const float *p = xyz + 3 * (size_t)i;
    cid[i] = (coord(0, p[0]) * dim[1] + coord(1, p[1])) * dim[2] + coord(2, p[2]);
    start[cid[i] + 1]++;
  }
  for (size_t c = 0; c < cells; c++) start[c + 1] += start[c];
  {
    std::vector<int32_t> cur(start.begin(), start.end() - 1);
    for (int i = 0; i < n; i++) order[cur[cid[i]]++] = i;
  }
  out.resize((size_t)n * kk);
  std::vector<uint64_t> cand;
  for (int q = 0; q < n; q++) {
    const float *qp = xyz + 3 * (size_t)q;
    const int c[3] = {coord(0, qp[0]), coord(1, qp[1]), coord(2, qp[2])};
    cand.clear();
    uint64_t kth = ~0ull;  // the k-th key once k are known: a candidate must beat it
    auto visit_cells = [&](int x, int y, int z0, int z1) {
      const size_t base = ((size_t)x * dim[1] + y) * dim[2];
      for (int t = start[base + z0]; t < start[base + z1 + 1]; t++) {
        const int i = order[t];
        const uint64_t kv = key(dist2(qp, xyz + 3 * (size_t)i), i);
        if (kv < kth) cand.push_back(kv);
      }
    };
    for (int R = 0;; R++) {
      const int x0 = std::max(0, c[0] - R), x1 = std::min(dim[0] - 1, c[0] + R);
      const int y0 = std::max(0, c[1] - R), y1 = std::min(dim[1] - 1, c[1] + R);
      for (int x = x0; x <= x1; x++)
        for (int y = y0; y <= y1; y++) {
          if (std::abs(x - c[0]) == R || std::abs(y - c[1]) == R) {
            visit_cells(x, y, std::max(0, c[2] - R), std::min(dim[2] - 1, c[2] + R));
          } else {  // an inner column of the shell: its bottom and top cells
            if (c[2] - R >= 0) visit_cells(x, y, c[2] - R, c[2] - R);
            if (c[2] + R <= dim[2] - 1) visit_cells(x, y, c[2] + R, c[2] + R);
          }
        }
      if ((int)cand.size() > kk) {
        std::nth_element(cand.begin(), cand.begin() + (kk - 1), cand.end());
        cand.resize(kk);
      }
      if ((int)cand.size() == kk) kth = *std::max_element(cand.begin(), cand.end());
      bool all = true;
      for (int a = 0; a < 3; a++) all = all && c[a] - R <= 0 && c[a] + R >= dim[a] - 1;
      float kd2;
      const uint32_t kb = (uint32_t)(kth >> 32);
      std::memcpy(&kd2, &kb, 4);
      if (all || ((int)cand.size() == kk && kd2 < ring_bound(R, cell))) break;
    }
    std::sort(cand.begin(), cand.end());
    for (int r = 0; r < kk; r++) out[(size_t)q * kk + r] = (int32_t)(uint32_t)cand[r];
  }
  return kk;
}

// One Jacobi pass for point j: the uniform-weight sum of the finite normals of its list, in list order, normalised; NaN
// (a singularity) when no neighbour counts or the norm is not finite or not above FLT_EPSILON.
inline void refine_point(const float *nrm, const int32_t *list, int k, float out[3]) {
  float nx = 0.f, ny = 0.f, nz = 0.f;
  for (int r = 0; r < k; r++) {
    const float *v = nrm + 3 * (size_t)list[r];
    if (!finite3(v[0], v[1], v[2])) continue;
    nx += 1.0f * v[0];
    ny += 1.0f * v[1];
    nz += 1.0f * v[2];
  }
  const float norm = std::sqrt(nx * nx + ny * ny + nz * nz);
  if (std::isfinite(norm) && norm > FLT_EPSILON) {
    out[0] = nx / norm;
    out[1] = ny / norm;
    out[2] = nz / norm;
  } else {
    out[0] = out[1] = out[2] = std::numeric_limits<float>::quiet_NaN();
  }
}

// the dot product a pass contributes for point j (new normal t, old normal o): NaN when it does not count
inline float pass_dot(const float *t, const float *o) {
  if (!finite3(t[0], t[1], t[2])) return std::numeric_limits<float>::quiet_NaN();
  return t[0] * o[0] + t[1] * o[1] + t[2] * o[2];
}

// NormalRefinement's convergence check of one pass: the finite dots summed in float, SEQUENTIALLY in ascending point index,
// divided by their number; stop when 1 - mean < threshold (never with no valid dot: the mean is NaN).  The mean is taken
// whatever the threshold (the caller reports it); the stop rule only with threshold > 0.
struct StopRule {
  float ddot = 0.f;
  unsigned num_valids = 0;
  void add(const float *dots, int n) {
    for (int j = 0; j < n; j++)
      if (std::isfinite(dots[j])) {
        ddot += dots[j];
        num_valids++;
      }
  }
  float mean() const { return ddot / (float)num_valids; }
  static bool stop(float mean, float threshold) { return threshold > 0.f && 1.0f - mean < threshold; }
};

struct Result {
  std::vector<float> normals;  // [n][3]
  int iterations = 0;          // passes run (the last one's output is the result)
  std::vector<float> ddots;    // [iterations] the means of the stop rule
  int num_nan = 0;             // normals with a non-finite component
};

// NormalRefinement on normals [n][3] with the lists [n][k] of knn()
inline Result refine(const float *normals, int n, const int32_t *lists, int k, int max_iterations, float threshold) {
  Result r;
  r.normals.assign(normals, normals + 3 * (size_t)n);
  std::vector<float> tmp((size_t)n * 3), dots((size_t)n);
  for (int it = 0; it < max_iterations; it++) {
    for (int j = 0; j < n; j++) {
      refine_point(r.normals.data(), lists + (size_t)j * k, k, &tmp[3 * (size_t)j]);
      dots[j] = pass_dot(&tmp[3 * (size_t)j], &r.normals[3 * (size_t)j]);
    }
    StopRule s;
    s.add(dots.data(), n);
    r.normals.swap(tmp);
    r.iterations = it + 1;
    r.ddots.push_back(s.mean());
    if (StopRule::stop(s.mean(), threshold)) break;
  }
  for (int j = 0; j < n; j++) r.num_nan += !finite3(r.normals[3 * (size_t)j], r.normals[3 * (size_t)j + 1], r.normals[3 * (size_t)j + 2]);
  return r;
}

}  // namespace refine
}  // namespace gpd
