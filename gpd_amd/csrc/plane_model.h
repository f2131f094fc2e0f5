// The support-plane fit of Cloud::sampleAbovePlane (util/cloud.cpp:407-436): pcl::SACSegmentation<PointXYZRGBA> with
// SACMODEL_PLANE, SAC_RANSAC and setOptimizeCoefficients(true), then ExtractIndices(negative) — PCL 1.9 with Eigen 3.3's
// x86-64 SSE2 reductions, restated step by step in DESIGN §7 ("sampleAbovePlane").  Plain C++ with no HIP in it: the host
// mirror's single-core model (util::Cloud::sampleAbovePlane) runs fit() below, the device path (plane.hip) uses the same
// random stream, stop rule and refinement between its kernel launches.  Every float expression is written in the
// operation order PCL / Eigen evaluate it and must be compiled without FMA contraction.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <limits>
#include <utility>
#include <vector>

namespace gpd {
namespace plane {

constexpr uint32_t kSeed = 12345u;         // SampleConsensusModel's non-random constructor (boost::mt19937(12345u))
constexpr int kMaxSampleChecks = 1000;     // SampleConsensusModel::max_sample_checks_

// boost::mt19937; rnd() = boost::uniform_int<>(0, INT_MAX) on it, which is the engine's output shifted right by one
struct Mt19937 {
  uint32_t s[624];
  int i;
  explicit Mt19937(uint32_t seed = 5489u) {
    s[0] = seed;
    for (int k = 1; k < 624; k++) s[k] = 1812433253u * (s[k - 1] ^ (s[k - 1] >> 30)) + (uint32_t)k;
    i = 624;
  }
  uint32_t operator()() {
    if (i == 624) {
      for (int k = 0; k < 624; k++) {
        const uint32_t y = (s[k] & 0x80000000u) | (s[(k + 1) % 624] & 0x7fffffffu);
        s[k] = s[(k + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
      }
      i = 0;
    }
    uint32_t y = s[i++];
    y ^= y >> 11;
    y ^= (y << 7) & 0x9d2c5680u;
    y ^= (y << 15) & 0xefc60000u;
    y ^= y >> 18;
    return y;
  }
  uint32_t rnd() { return (*this)() >> 1; }
};

// SampleConsensusModelPlane::isSampleGood (PCL 1.9): (p1 - p0) / (p2 - p0) per component; NaN counts as "different"
inline bool sample_good(const float *p0, const float *p1, const float *p2) {
  const float d0 = (p1[0] - p0[0]) / (p2[0] - p0[0]);
  const float d1 = (p1[1] - p0[1]) / (p2[1] - p0[1]);
  const float d2 = (p1[2] - p0[2]) / (p2[2] - p0[2]);
  return d0 != d1 || d2 != d1;
}

// computeModelCoefficients: the cross product of the two edges, normalised (a zero normal stays zero), d through p0
inline void plane_from3(const float *p0, const float *p1, const float *p2, float c[4]) {
  const float u0 = p1[0] - p0[0], u1 = p1[1] - p0[1], u2 = p1[2] - p0[2];
  const float v0 = p2[0] - p0[0], v1 = p2[1] - p0[1], v2 = p2[2] - p0[2];
  float n0 = u1 * v2 - u2 * v1, n1 = u2 * v0 - u0 * v2, n2 = u0 * v1 - u1 * v0;
  const float z = (n0 * n0 + n2 * n2) + (n1 * n1 + 0.0f);  // Vector4f::squaredNorm, SSE2 horizontal sum
  if (z > 0.0f) {
    const float r = std::sqrt(z);
    n0 = n0 / r;
    n1 = n1 / r;
    n2 = n2 / r;
  }
  c[0] = n0;
  c[1] = n1;
  c[2] = n2;
  c[3] = -((n0 * p0[0] + n2 * p0[2]) + (n1 * p0[1] + 0.0f * 1.0f));
}

// pointToPlaneDistance as countWithinDistance / selectWithinDistance evaluate it: |(a x + c z) + (b y + d)|
inline float plane_dist(const float c[4], float x, float y, float z) { return std::fabs((c[0] * x + c[2] * z) + (c[1] * y + c[3] * 1.0f)); }
inline bool inlier(const float c[4], const float *p, double threshold) { return (double)plane_dist(c, p[0], p[1], p[2]) < threshold; }

// The float compare that decides `(double)fabsf(dist) < threshold` for every float: dist <= largest float below threshold
// (a NaN threshold gives NaN: nothing is an inlier, as in the double compare)
inline float threshold_f32(double threshold) {
  float f = (float)threshold;
  if ((double)f >= threshold) f = std::nextafter(f, -std::numeric_limits<float>::infinity());
  return f;
}

// RandomSampleConsensus::computeModel's stop rule after a new best count: k = log(1 - probability) / log(p_no_outliers)
inline double stop_bound(int count, int n, double probability) {
  const double eps = std::numeric_limits<double>::epsilon();
  const double w = (double)count * (1.0 / (double)n);
  double p = 1.0 - std::pow(w, 3.0);
  p = std::max(eps, p);
  p = std::min(1.0 - eps, p);
  return std::log(1.0 - probability) / std::log(p);
}

// pcl::computeRoots2 — its discriminant is a double expression (4.0 is a double)
inline void roots2(float b, float c, float r[3]) {
  r[0] = 0.0f;
  float d = (float)(b * b - 4.0 * c);
  if (d < 0.0f) d = 0.0f;
  const float sd = std::sqrt(d);
  r[2] = 0.5f * (b + sd);
  r[1] = 0.5f * (b - sd);
}

// pcl::computeRoots (common/impl/eigen.hpp, PCL 1.9): closed form, ascending, with the quadratic fallback
inline void roots3(const float m[9], float r[3]) {
  const float m00 = m[0], m01 = m[1], m02 = m[2], m11 = m[4], m12 = m[5], m22 = m[8];
  const float c0 = m00 * m11 * m22 + 2.0f * m01 * m02 * m12 - m00 * m12 * m12 - m11 * m02 * m02 - m22 * m01 * m01;
  const float c1 = m00 * m11 - m01 * m01 + m00 * m22 - m02 * m02 + m11 * m22 - m12 * m12;
  const float c2 = m00 + m11 + m22;
  if (std::fabs(c0) < FLT_EPSILON) {
    roots2(c2, c1, r);
    return;
  }
  const float s_inv3 = (float)(1.0 / 3.0);
  const float s_sqrt3 = std::sqrt(3.0f);
  const float c2_over_3 = c2 * s_inv3;
  float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
  if (a_over_3 > 0.0f) a_over_3 = 0.0f;
  const float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
  float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
  if (q > 0.0f) q = 0.0f;
  const float rho = std::sqrt(-a_over_3);
  const float theta = atan2f(std::sqrt(-q), half_b) * s_inv3;
  const float cos_theta = cosf(theta), sin_theta = sinf(theta);
  r[0] = c2_over_3 + 2.0f * rho * cos_theta;
  r[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  r[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  if (r[0] >= r[1]) std::swap(r[0], r[1]);
  if (r[1] >= r[2]) {
    std::swap(r[1], r[2]);
    if (r[0] >= r[1]) std::swap(r[0], r[1]);
  }
  if (r[0] <= 0.0f) roots2(c2, c1, r);
}

// pcl::eigen33(mat, eigenvalue, eigenvector): the eigenvector of the smallest eigenvalue of a symmetric 3x3 (row major)
inline void eigen33(const float mat[9], float e[3]) {
  float scale = 0.0f;
  for (int k = 0; k < 9; k++) scale = std::max(scale, std::fabs(mat[k]));
  if (scale <= std::numeric_limits<float>::min()) scale = 1.0f;
  float s[9];
  for (int k = 0; k < 9; k++) s[k] = mat[k] / scale;
  float r[3];
  roots3(s, r);
  s[0] -= r[0];
  s[4] -= r[0];
  s[8] -= r[0];
  auto cross = [](const float *a, const float *b, float *o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
  };
  float v[3][3];
  cross(s + 0, s + 3, v[0]);
  cross(s + 0, s + 6, v[1]);
  cross(s + 3, s + 6, v[2]);
  float len[3];
  for (int k = 0; k < 3; k++) len[k] = v[k][0] * v[k][0] + (v[k][1] * v[k][1] + v[k][2] * v[k][2]);  // Vector3f::squaredNorm
  const int pick = (len[0] >= len[1] && len[0] >= len[2]) ? 0 : (len[1] >= len[0] && len[1] >= len[2]) ? 1 : 2;
  const float l = std::sqrt(len[pick]);
  for (int k = 0; k < 3; k++) e[k] = v[pick][k] / l;
}

// computeMeanAndCovarianceMatrix's nine float accumulators, summed in inlier order
struct Accu {
  float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  void add(float x, float y, float z) {
    a[0] += x * x;
    a[1] += x * y;
    a[2] += x * z;
    a[3] += y * y;
    a[4] += y * z;
    a[5] += z * z;
    a[6] += x;
    a[7] += y;
    a[8] += z;
  }
};

// optimizeModelCoefficients from the accumulated sums of `count` (> 3) inliers: covariance, eigen33, the plane through the centroid
inline void refine_from_accu(const float accu_in[9], int count, float c[4]) {
  float accu[9];
  for (int k = 0; k < 9; k++) accu[k] = accu_in[k] / (float)count;
  float cov[9];
  cov[0] = accu[0] - accu[6] * accu[6];
  cov[1] = accu[1] - accu[6] * accu[7];
  cov[2] = accu[2] - accu[6] * accu[8];
  cov[4] = accu[3] - accu[7] * accu[7];
  cov[5] = accu[4] - accu[7] * accu[8];
  cov[8] = accu[5] - accu[8] * accu[8];
  cov[3] = cov[1];
  cov[6] = cov[2];
  cov[7] = cov[5];
  float e[3];
  eigen33(cov, e);
  c[0] = e[0];
  c[1] = e[1];
  c[2] = e[2];
  c[3] = -((e[0] * accu[6] + e[2] * accu[8]) + (e[1] * accu[7] + 0.0f * 1.0f));
}

// the draws of SampleConsensusModel::getSamples over a persistent shuffled_indices; false: no good sample (empty draw)
struct Drawer {
  Mt19937 mt{kSeed};
  std::vector<int> sh;
  explicit Drawer(int n) : sh((size_t)n) {
    for (int k = 0; k < n; k++) sh[k] = k;
  }
  bool draw(const float *xyz, int out[3]) {
    const int n = (int)sh.size();
    if (n < 3) return false;
    for (int t = 0; t < kMaxSampleChecks; t++) {
      for (int i = 0; i < 3; i++) std::swap(sh[i], sh[i + (int)(mt.rnd() % (uint32_t)(n - i))]);
      if (sample_good(xyz + 3 * (size_t)sh[0], xyz + 3 * (size_t)sh[1], xyz + 3 * (size_t)sh[2])) {
        for (int i = 0; i < 3; i++) out[i] = sh[i];
        return true;
      }
    }
    return false;
  }
};

struct Result {
  std::vector<int> above;  // ascending indices off the plane (empty: the fit failed)
  float coeffs[4] = {0, 0, 0, 0};
  int num_inliers = 0;     // points within the threshold of the final plane
  int iterations = 0;      // hypotheses RANSAC evaluated
  bool model = false;      // RANSAC found a model
};

// The whole definition on one core: xyz [n][3]
inline Result fit(const float *xyz, int n, double threshold, int max_iterations, double probability, bool optimize) {
  Result res;
  Drawer dr(n);
  int best = 0, it = 0;
  double k = std::numeric_limits<double>::max();
  float model[4] = {0, 0, 0, 0};
  while (it < k) {
    int smp[3];
    if (!dr.draw(xyz, smp)) break;
    float c[4];
    plane_from3(xyz + 3 * (size_t)smp[0], xyz + 3 * (size_t)smp[1], xyz + 3 * (size_t)smp[2], c);
    int count = 0;
    for (int i = 0; i < n; i++) count += inlier(c, xyz + 3 * (size_t)i, threshold);
    if (count > best) {
      best = count;
      for (int a = 0; a < 4; a++) model[a] = c[a];
      k = stop_bound(count, n, probability);
    }
    ++it;
    if (it > max_iterations) break;
  }
  res.iterations = it;
  if (best == 0) return res;
  res.model = true;
  if (optimize && best > 3) {
    Accu acc;
    for (int i = 0; i < n; i++)
      if (inlier(model, xyz + 3 * (size_t)i, threshold)) acc.add(xyz[3 * (size_t)i], xyz[3 * (size_t)i + 1], xyz[3 * (size_t)i + 2]);
    refine_from_accu(acc.a, best, model);
  }
  for (int a = 0; a < 4; a++) res.coeffs[a] = model[a];
  for (int i = 0; i < n; i++) {
    if (inlier(model, xyz + 3 * (size_t)i, threshold))
      res.num_inliers++;
    else
      res.above.push_back(i);
  }
  return res;
}

}  // namespace plane
}  // namespace gpd
