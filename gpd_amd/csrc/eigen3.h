// The 3x3 symmetric eigensolver the local frames (search.hip) and the normals (normals.hip) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>

namespace gpd {

// ---------------------------------------------------------------------------
// 3x3 symmetric eigensolver, fp64: scale, closed-form tridiagonalisation, implicit
// QR with Wilkinson shift, ascending sort — the algorithm of Eigen's
// SelfAdjointEigenSolver<Matrix3d>::compute (used at local_frame.cpp:17-21).
// Q is row-major, columns are eigenvectors.
// ---------------------------------------------------------------------------
__device__ inline void givens(double p, double q, double &c, double &s) {
  if (q == 0.0) {
    c = p < 0 ? -1.0 : 1.0;
    s = 0.0;
  } else if (p == 0.0) {
    c = 0.0;
    s = q < 0 ? 1.0 : -1.0;
  } else if (fabs(p) > fabs(q)) {
    double t = q / p;
    double u = sqrt(1.0 + t * t);
    if (p < 0) u = -u;
    c = 1.0 / u;
    s = -t * c;
  } else {
    double t = p / q;
    double u = sqrt(1.0 + t * t);
    if (q < 0) u = -u;
    s = -1.0 / u;
    c = -t * s;
  }
}

__device__ inline double hypot_pos(double x, double y) {
  x = fabs(x);
  y = fabs(y);
  double p = fmax(x, y);
  if (p == 0.0) return 0.0;
  double qp = fmin(y, x) / p;
  return p * sqrt(1.0 + qp * qp);
}

__device__ inline void eigen3(double m00, double m10, double m11, double m20, double m21, double m22, double *eval, double *Q) {
  double scale = fmax(fmax(fmax(fabs(m00), fabs(m10)), fmax(fabs(m11), fabs(m20))), fmax(fabs(m21), fabs(m22)));
  if (scale == 0.0) scale = 1.0;
  m00 /= scale;
  m10 /= scale;
  m11 /= scale;
  m20 /= scale;
  m21 /= scale;
  m22 /= scale;
  double diag[3], sub[2];
  diag[0] = m00;
  const double v1norm2 = m20 * m20;
  if (v1norm2 <= DBL_MIN) {
    diag[1] = m11;
    diag[2] = m22;
    sub[0] = m10;
    sub[1] = m21;
    Q[0] = 1; Q[1] = 0; Q[2] = 0; Q[3] = 0; Q[4] = 1; Q[5] = 0; Q[6] = 0; Q[7] = 0; Q[8] = 1;
  } else {
    const double beta = sqrt(m10 * m10 + v1norm2);
    const double invBeta = 1.0 / beta;
    const double m01 = m10 * invBeta;
    const double m02 = m20 * invBeta;
    const double q = 2.0 * m01 * m21 + m02 * (m22 - m11);
    diag[1] = m11 + m02 * q;
    diag[2] = m22 - m02 * q;
    sub[0] = beta;
    sub[1] = m21 - m01 * q;
    Q[0] = 1; Q[1] = 0; Q[2] = 0; Q[3] = 0; Q[4] = m01; Q[5] = m02; Q[6] = 0; Q[7] = m02; Q[8] = -m01;
  }
  int end = 2, start = 0, iter = 0;
  const double precision_inv = 1.0 / DBL_EPSILON;
  while (end > 0) {
    for (int i = start; i < end; i++) {
      if (fabs(sub[i]) < DBL_MIN) {
        sub[i] = 0.0;
      } else {
        const double ss = precision_inv * sub[i];
        if (ss * ss <= (fabs(diag[i]) + fabs(diag[i + 1]))) sub[i] = 0.0;
      }
    }
    while (end > 0 && sub[end - 1] == 0.0) end--;
    if (end <= 0) break;
    iter++;
    if (iter > 90) break;
    start = end - 1;
    while (start > 0 && sub[start - 1] != 0.0) start--;
    const double td = (diag[end - 1] - diag[end]) * 0.5;
    const double e = sub[end - 1];
    double mu = diag[end];
    if (td == 0.0) {
      mu -= fabs(e);
    } else if (e != 0.0) {
      const double e2 = e * e;
      const double h = hypot_pos(td, e);
      if (e2 == 0.0)
        mu -= e / ((td + (td > 0.0 ? h : -h)) / e);
      else
        mu -= e2 / (td + (td > 0.0 ? h : -h));
    }
    double x = diag[start] - mu;
    double z = sub[start];
    for (int k = start; k < end && z != 0.0; k++) {
      double c, s;
      givens(x, z, c, s);
      const double sdk = s * diag[k] + c * sub[k];
      const double dkp1 = s * sub[k] + c * diag[k + 1];
      diag[k] = c * (c * diag[k] - s * sub[k]) - s * (c * sub[k] - s * diag[k + 1]);
      diag[k + 1] = s * sdk + c * dkp1;
      sub[k] = c * sdk - s * dkp1;
      if (k > start) sub[k - 1] = c * sub[k - 1] - s * z;
      x = sub[k];
      if (k < end - 1) {
        z = -s * sub[k + 1];
        sub[k + 1] = c * sub[k + 1];
      }
      for (int i = 0; i < 3; i++) {
        const double xi = Q[3 * i + k], yi = Q[3 * i + k + 1];
        Q[3 * i + k] = c * xi - s * yi;
        Q[3 * i + k + 1] = s * xi + c * yi;
      }
    }
  }
  for (int i = 0; i < 2; i++) {
    int k = 0;
    for (int j = 1; j < 3 - i; j++)
      if (diag[i + j] < diag[i + k]) k = j;
    if (k > 0) {
      double t = diag[i];
      diag[i] = diag[k + i];
      diag[k + i] = t;
      for (int r = 0; r < 3; r++) {
        t = Q[3 * r + i];
        Q[3 * r + i] = Q[3 * r + k + i];
        Q[3 * r + k + i] = t;
      }
    }
  }
  for (int i = 0; i < 3; i++) eval[i] = diag[i] * scale;
}

}  // namespace gpd
