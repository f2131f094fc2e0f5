// The draws of SequentialImportanceSampling::detectGrasps (sequential_importance_sampling.cpp:54-270).  The reference's generators
// are std::random_device, time-seeded rand() and static std::normal_distributions, so there is nothing to be bit-faithful to: as
// with Cloud::subsample (sample_model.h) the project's seeded stream is the definition.  Plain C++ with no HIP in it, compiled
// without FMA contraction: gpd_hip_sis_proposals / gpd_hip_sis_select (host only), the host side of gpd_hip_detect_sis (the
// proposals) and sis_draw_kernel (the selection rule, sis.hip) are this code.
//
// Round r (0-based, the rounds after the initial pass) has two independent sample::Stream's, seeds in uint32 arithmetic:
//   Gaussian   Stream(seed + 1000003u * (2r))      7 draws per proposal: idx_raw, then three Box-Muller offsets of two draws each
//   uniform    Stream(seed + 1000003u * (2r + 1))  1 draw per proposal: pos_raw
// so that the host generates either stream without knowing how many proposals of the other the device rejected.  Proposals are
// generated on the HOST only (log, sqrt, cos of its libm); the device never evaluates a transcendental.
//
// The selection rule over L live centres c[0 .. L):
//   Gaussian   idx = idx_raw % L, x = c[idx] + off (one double addition per component)
//              method 0 (SUM_OF_GAUSSIANS, :189-201): accepted
//              method 1 (MAX_OF_GAUSSIANS, :203-237): accepted iff d2(x, c[idx]) <= min_k d2(x, c[k]), d2 = (dx*dx + dy*dy) + dz*dz.
//              The reference compares term * exp(-d2 / (2 sigma)) with >=; exp is monotone, so what is accepted here is accepted
//              there, and the reverse fails only where two different distances round to one density.
//   uniform    i = list[pos_raw % n] (no list: the point pos_raw % P), the sample is the point's float coordinates cast to double,
//              accepted iff inside the workspace, bounds inclusive (:263-265)
// A round's samples: the first num_gauss accepted Gaussian proposals in proposal order, then the first num_rand accepted uniform
// ones.  Every proposal consumes a fixed number of draws, so the reference's sequential rejection loops equal "filter in
// parallel, keep the first n in order".
#pragma once
#include <cmath>
#include <cstdint>

#include "sample_model.h"

namespace gpd {
namespace sis {

struct Proposal {  // a Gaussian proposal as it travels to the device: 32 bytes
  uint64_t idx_raw;
  double off[3];
};
static_assert(sizeof(Proposal) == 32, "Proposal");

constexpr int kGaussDraws = 7;  // draws of the stream per Gaussian proposal

inline uint32_t stream_seed(uint32_t seed, int round, int kind /* 0: Gaussian, 1: uniform */) {
  return seed + 1000003u * (uint32_t)(2 * round + kind);
}

// Box-Muller on two 53-bit uniforms, as the host mirror's randNormal
inline double rand_normal(sample::Stream &st, double sigma) {
  const double u1 = ((double)(st.next() >> 11) + 1.0) * (1.0 / 9007199254740993.0);
  const double u2 = (double)(st.next() >> 11) * (1.0 / 9007199254740992.0);
  return sigma * std::sqrt(-2.0 * std::log(u1)) * std::cos(2.0 * M_PI * u2);
}

inline Proposal next_gauss(sample::Stream &st, double sigma) {
  Proposal p;
  p.idx_raw = st.next();
  for (int r = 0; r < 3; r++) p.off[r] = rand_normal(st, sigma);
  return p;
}

inline void skip(sample::Stream &st, unsigned long long draws) {
  for (unsigned long long i = 0; i < draws; i++) (void)st.next();
}

// The pieces of the rule that sis_draw_kernel shares are constexpr: plain C++ here, callable from device code as they stand.
constexpr double d2(const double x[3], const double c[3]) {
  const double dx = x[0] - c[0], dy = x[1] - c[1], dz = x[2] - c[2];
  return (dx * dx + dy * dy) + dz * dz;
}

// the point a Gaussian proposal stands for; returns the centre it was drawn around
constexpr int gauss_point(const double *centres, int L, const Proposal &p, double x[3]) {
  const int idx = (int)(p.idx_raw % (uint64_t)L);
  for (int r = 0; r < 3; r++) x[r] = centres[3 * (size_t)idx + r] + p.off[r];
  return idx;
}

// the cloud point a uniform proposal stands for
constexpr int uniform_point(uint64_t pos_raw, const int32_t *list, int n_list, int num_points) {
  return list ? list[pos_raw % (uint64_t)n_list] : (int)(pos_raw % (uint64_t)num_points);
}

constexpr bool inside(const double s[3], const double ws[6]) {
  return s[0] >= ws[0] && s[0] <= ws[1] && s[1] >= ws[2] && s[1] <= ws[3] && s[2] >= ws[4] && s[2] <= ws[5];
}

struct Counts {        // of one stream of one round
  int32_t accepted;    // samples written so far (in: by earlier blocks)
  int32_t consumed;    // proposals of the stream used so far: past the one that filled the list, or every one given
};

// The selection over one block of each stream, continuing from the counts earlier blocks of the round left.  samples holds
// (num_gauss + num_rand) x 3 doubles.  Returns the samples still missing (Gaussian + uniform): > 0 asks for the next blocks.
inline int select(const double *centres, int L, const Proposal *gauss, int n_gauss, const uint64_t *uniform, int n_uniform,
                  const int32_t *list, int n_list, const float *cloud_xyz, int num_points, const double ws[6], int method, int num_gauss,
                  int num_rand, double *samples, Counts &g, Counts &u) {
  for (int i = 0; i < n_gauss && g.accepted < num_gauss; i++) {
    double x[3];
    const int idx = gauss_point(centres, L, gauss[i], x);
    bool ok = true;
    if (method == 1) {
      const double own = d2(x, centres + 3 * (size_t)idx);
      for (int k = 0; k < L && ok; k++) ok = !(d2(x, centres + 3 * (size_t)k) < own);
    }
    if (ok) {
      for (int r = 0; r < 3; r++) samples[3 * (size_t)g.accepted + r] = x[r];
      g.accepted++;
    }
    g.consumed++;
  }
  for (int i = 0; i < n_uniform && u.accepted < num_rand; i++) {
    const int pt = uniform_point(uniform[i], list, n_list, num_points);
    const double s[3] = {(double)cloud_xyz[3 * (size_t)pt], (double)cloud_xyz[3 * (size_t)pt + 1], (double)cloud_xyz[3 * (size_t)pt + 2]};
    if (inside(s, ws)) {
      for (int r = 0; r < 3; r++) samples[3 * (size_t)(num_gauss + u.accepted) + r] = s[r];
      u.accepted++;
    }
    u.consumed++;
  }
  return (num_gauss - g.accepted) + (num_rand - u.accepted);
}

inline int num_rand_samples(double prob_rand_samples, int num_samples) { return (int)(prob_rand_samples * num_samples); }

}  // namespace sis
}  // namespace gpd
