// The opt-in jitter of the shadow points (gpd_hip_set_shadow_jitter): one N(0,1)-like draw g per voxel, a pure function of
// (seed, voxel), and the point p_a = v_a * 0.003 + (g * 0.003) * 0.3 with the operand order of HandSet::shadowVoxelsToPoints
// (hand_set.cpp:197-199; the same draw on all three coordinates).  The reference seeds its generator from
// std::random_device, so its own stream cannot be reproduced; this has its magnitude and its arithmetic.
// Plain C++ with no HIP in it, constexpr like image::lcg_affine: the host model (gpd_hip_shadow_jitter_model) and the
// shadow kernels of images.hip are this code.  Integer arithmetic and exact double operations only.
#pragma once
#include <cstdint>

namespace gpd {
namespace jitter {

constexpr uint64_t mix(uint64_t z) {  // the splitmix64 step
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
constexpr uint32_t fields16(uint64_t k) {  // sum of the four 16-bit fields of a word
  return (uint32_t)(k & 0xffffu) + (uint32_t)((k >> 16) & 0xffffu) + (uint32_t)((k >> 32) & 0xffffu) + (uint32_t)(k >> 48);
}
// Irwin-Hall with twelve terms: mean 0, variance 1 - 2^-32, |g| < 6; every step exact
constexpr double draw(uint64_t seed, int32_t x, int32_t y, int32_t z) {
  const uint64_t k0 = mix(seed ^ ((uint64_t)(uint32_t)x | ((uint64_t)(uint32_t)y << 32)));
  const uint64_t k1 = mix(k0 ^ (uint64_t)(uint32_t)z);
  const uint64_t k2 = mix(k1);
  const uint64_t k3 = mix(k2);
  const int32_t S = (int32_t)(fields16(k1) + fields16(k2) + fields16(k3));
  return (double)(S - 393210) * (1.0 / 65536.0);
}
// the shift of a voxel's point along every world axis; g * voxel, then * 0.3 (the reference's order, unfused)
constexpr double shift(double g, double voxel) { return (g * voxel) * 0.3; }

// |shift| < 6 * 0.003 * 0.3 per world axis: under two voxels.  A hand coordinate moves by the shift times the sum of a
// frame column, |sum| <= sqrt(3).
constexpr double kShiftBound = 0.0054;
constexpr double kHandShiftBound = 0.0094;
constexpr int kShiftVoxels = 2;  // whole voxels the bound adds on each side of a window / to the reach

}  // namespace jitter
}  // namespace gpd
