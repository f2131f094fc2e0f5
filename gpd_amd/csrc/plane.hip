// Cloud::sampleAbovePlane on the device (util/cloud.cpp:407-436): PCL 1.9's RANSAC plane fit with refinement, then the
// complement of the inliers — the definition is DESIGN §7 ("sampleAbovePlane") and plane_model.h, the host model this
// path equals bit for bit.  On the cloud uploaded last (Cloud::px/py/pz, pxyz), which never leaves the device:
//   1. hypothesis_kernel, one wave: boost::mt19937 in the LDS (the 64 lanes twist it), PCL's swap draws over
//      shuffled_indices — kept as a sparse table of the positions the swaps have touched (every other position still holds
//      its own index), the good-sample test on the three points and the plane through them, for all max_iterations + 1
//      hypotheses.  The draws do not depend on the counts, so they are all made up front.
//   2. count_kernel: every thread loads its points once and tests every plane; per plane a wave ballot + popcount, one
//      LDS atomic per wave and one global atomic per workgroup — integer counts, exact in any order.
//   3. on the host, between launches: RANSAC's stop rule over the counts in hypothesis order (log / pow of glibc).
//   4. the best model's inliers, compacted in index order (flag / scan / write), their xyz to the host, where the
//      refinement's sequential float sums and eigen33 (atan2f, cosf, sinf of glibc) run — DESIGN §7 has the measurement
//      against one wave summing on the device (the profiling build's GPD_PLANE_REFINE=device).
//   5. the complement of the refined plane's inliers, compacted in index order: the sample indices.
// The distance test `(double)fabsf(dist) < threshold` runs as `fabsf(dist) <= threshold_f32(threshold)`, the same
// decision for every float (plane_model.h).  -ffp-contract=off (Makefile): every expression is evaluated unfused.
#include "gpd_internal.h"
#include "buffers.h"
#include "plane_model.h"
#include "wave_ops.h"

#include <cstdio>
#include <cstring>
#include <vector>

namespace gpd {

namespace {

constexpr int kPtsPerThread = 4;   // count_kernel: points per thread
constexpr int kCountThreads = 256;
constexpr int kFlagThreads = 256;  // compaction: one point per thread

struct PlaneMeta {
  int32_t hyps;      // hypotheses drawn (fewer than asked: a draw found no good sample in 1000 tries)
  int32_t overflow;  // the swap table ran out of room
  int32_t total;     // points the last compaction wrote
  int32_t pad_;
};

__device__ inline uint32_t mt_temper(uint32_t y) {
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

__device__ inline float plane_dist(float4 c, float x, float y, float z) { return fabsf((c.x * x + c.z * z) + (c.y * y + c.w * 1.0f)); }

// one wave: every lane holds the same stream position, swap slots and counters (wave-uniform values)
__global__ __launch_bounds__(64) void hypothesis_kernel(const float4 *__restrict__ pxyz, int n, int H, float4 *__restrict__ coef, PlaneMeta *meta) {
  __shared__ uint32_t mt[624];
  __shared__ int32_t keys[kPlaneSwapCap], vals[kPlaneSwapCap];
  const int lane = threadIdx.x;
  // seed (12345u): a serial recurrence, 624 steps on lane 0
  if (lane == 0) {
    uint32_t s = plane::kSeed;
    mt[0] = s;
    for (int k = 1; k < 624; k++) {
      s = 1812433253u * (s ^ (s >> 30)) + (uint32_t)k;
      mt[k] = s;
    }
  }
  __syncthreads();
  int mti = 624, entries = 0, h = 0, overflow = 0;
  int s0 = 0, s1 = 1, s2 = 2;  // shuffled_indices[0..2]
  auto rnd = [&]() -> uint32_t {
    if (mti == 624) {
      // the twist in chunks of 64: element i reads i + 1 (old, or new element 0 for i = 623) and i + 397 mod 624, which
      // for i >= 227 is i - 227, written at least one chunk earlier
      for (int c = 0; c < 624; c += 64) {
        const int i = c + lane;
        uint32_t a = 0, b = 0, m = 0;
        if (i < 624) {
          a = mt[i];
          b = mt[i == 623 ? 0 : i + 1];
          m = mt[i < 227 ? i + 397 : i - 227];
        }
        __syncthreads();
        if (i < 624) {
          const uint32_t y = (a & 0x80000000u) | (b & 0x7fffffffu);
          mt[i] = m ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
        }
        __syncthreads();
      }
      mti = 0;
    }
    return mt_temper(mt[mti++]) >> 1;
  };
  // value at position j >= 3 of shuffled_indices; sets *slot to its table entry or -1
  auto lookup = [&](int j, int *slot) -> int {
    for (int base = 0; base < entries; base += 64) {
      const int k = base + lane;
      const unsigned long long hit = __builtin_amdgcn_ballot_w64(k < entries && keys[k] == j);
      if (hit) {
        *slot = base + (int)__builtin_ctzll(hit);
        return vals[*slot];
      }
    }
    *slot = -1;
    return j;
  };
  int tries = 0;
  while (h < H && n >= 3) {
    for (int i = 0; i < 3; i++) {
      const int j = i + (int)(rnd() % (uint32_t)(n - i));
      int si = i == 0 ? s0 : i == 1 ? s1 : s2;
      int v;
      if (j < 3) {
        v = j == 0 ? s0 : j == 1 ? s1 : s2;
        if (j == 0) s0 = si;
        if (j == 1) s1 = si;
        if (j == 2) s2 = si;
      } else {
        int slot;
        v = lookup(j, &slot);
        if (slot < 0) {
          if (entries == kPlaneSwapCap) {
            overflow = 1;
            break;
          }
          slot = entries++;
          if (lane == 0) keys[slot] = j;
        }
        if (lane == 0) vals[slot] = si;
        __syncthreads();
      }
      if (i == 0) s0 = v;
      if (i == 1) s1 = v;
      if (i == 2) s2 = v;
    }
    if (overflow) break;
    // lanes 0..2 load the three points
    const int mine = lane == 0 ? s0 : lane == 1 ? s1 : s2;
    float4 p = make_float4(0.f, 0.f, 0.f, 0.f);
    if (lane < 3) p = pxyz[mine];
    const float p0[3] = {__shfl(p.x, 0), __shfl(p.y, 0), __shfl(p.z, 0)};
    const float p1[3] = {__shfl(p.x, 1), __shfl(p.y, 1), __shfl(p.z, 1)};
    const float p2[3] = {__shfl(p.x, 2), __shfl(p.y, 2), __shfl(p.z, 2)};
    const float d0 = __fdiv_rn(p1[0] - p0[0], p2[0] - p0[0]);
    const float d1 = __fdiv_rn(p1[1] - p0[1], p2[1] - p0[1]);
    const float d2 = __fdiv_rn(p1[2] - p0[2], p2[2] - p0[2]);
    if (d0 != d1 || d2 != d1) {
      const float u0 = p1[0] - p0[0], u1 = p1[1] - p0[1], u2 = p1[2] - p0[2];
      const float v0 = p2[0] - p0[0], v1 = p2[1] - p0[1], v2 = p2[2] - p0[2];
      float n0 = u1 * v2 - u2 * v1, n1 = u2 * v0 - u0 * v2, n2 = u0 * v1 - u1 * v0;
      const float z = (n0 * n0 + n2 * n2) + (n1 * n1 + 0.0f);
      if (z > 0.0f) {
        const float r = sqrtf(z);  // correctly rounded (__fsqrt_rn is the bare v_sqrt_f32 here, 1 ulp)
        n0 = __fdiv_rn(n0, r);
        n1 = __fdiv_rn(n1, r);
        n2 = __fdiv_rn(n2, r);
      }
      const float d = -((n0 * p0[0] + n2 * p0[2]) + (n1 * p0[1] + 0.0f * 1.0f));
      if (lane == 0) coef[h] = make_float4(n0, n1, n2, d);
      h++;
      tries = 0;
    } else if (++tries == plane::kMaxSampleChecks) {
      break;  // an empty draw: RANSAC stops here
    }
  }
  if (lane == 0) {
    meta->hyps = h;
    meta->overflow = overflow;
  }
}

__global__ __launch_bounds__(kCountThreads) void count_kernel(const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pz,
                                                              int n, const float4 *__restrict__ coef, const PlaneMeta *__restrict__ meta, float thr,
                                                              int32_t *__restrict__ counts) {
  __shared__ float4 s_coef[kPlaneMaxHyp];
  __shared__ int s_cnt[kPlaneMaxHyp];
  const int H = meta->hyps;
  for (int h = threadIdx.x; h < H; h += kCountThreads) {
    s_coef[h] = coef[h];
    s_cnt[h] = 0;
  }
  float x[kPtsPerThread], y[kPtsPerThread], z[kPtsPerThread];
  bool ok[kPtsPerThread];
#pragma unroll
  for (int k = 0; k < kPtsPerThread; k++) {
    const int i = (blockIdx.x * kPtsPerThread + k) * kCountThreads + threadIdx.x;
    ok[k] = i < n;
    x[k] = ok[k] ? px[i] : 0.f;
    y[k] = ok[k] ? py[i] : 0.f;
    z[k] = ok[k] ? pz[i] : 0.f;
  }
  __syncthreads();
  for (int h = 0; h < H; h++) {
    const float4 c = s_coef[h];
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < kPtsPerThread; k++) cnt += __popcll(__builtin_amdgcn_ballot_w64(ok[k] && plane_dist(c, x[k], y[k], z[k]) <= thr));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(&s_cnt[h], cnt);
  }
  __syncthreads();
  for (int h = threadIdx.x; h < H; h += kCountThreads)
    if (s_cnt[h]) atomicAdd(&counts[h], s_cnt[h]);
}

// ordered compaction of the points whose test against `c` equals `want`: per-block counts, one-workgroup scan, write
__global__ __launch_bounds__(kFlagThreads) void flag_count_kernel(const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pz,
                                                                  int n, float4 c, float thr, int want, int32_t *__restrict__ block_count) {
  __shared__ int s_cnt[kFlagThreads / 64];
  const int i = blockIdx.x * kFlagThreads + threadIdx.x;
  const bool f = i < n && (plane_dist(c, px[i], py[i], pz[i]) <= thr) == (want != 0);
  const unsigned long long b = __builtin_amdgcn_ballot_w64(f);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kFlagThreads / 64; w++) t += s_cnt[w];
    block_count[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(1024) void scan_kernel(const int32_t *__restrict__ block_count, int nblocks, int32_t *__restrict__ block_off, PlaneMeta *meta) {
  __shared__ int s_part[16];
  __shared__ int s_carry;
  const int tid = threadIdx.x;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < nblocks; base += 1024) {
    const int i = base + tid;
    const int before = block_scan_step(i < nblocks ? block_count[i] : 0, s_part, s_carry);
    if (i < nblocks) block_off[i] = before;
  }
  if (tid == 0) meta->total = s_carry;
}

// writes the selected points in index order: their xyz (xyz_out) or their indices (idx_out)
__global__ __launch_bounds__(kFlagThreads) void flag_write_kernel(const float *__restrict__ px, const float *__restrict__ py, const float *__restrict__ pz,
                                                                  int n, float4 c, float thr, int want, const int32_t *__restrict__ block_off,
                                                                  float *__restrict__ xyz_out, int32_t *__restrict__ idx_out) {
  __shared__ int s_cnt[kFlagThreads / 64];
  const int i = blockIdx.x * kFlagThreads + threadIdx.x;
  float x = 0.f, y = 0.f, z = 0.f;
  bool f = false;
  if (i < n) {
    x = px[i];
    y = py[i];
    z = pz[i];
    f = (plane_dist(c, x, y, z) <= thr) == (want != 0);
  }
  const unsigned long long b = __builtin_amdgcn_ballot_w64(f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_cnt[wave] = __popcll(b);
  __syncthreads();
  if (!f) return;
  int off = block_off[blockIdx.x];
  for (int w = 0; w < wave; w++) off += s_cnt[w];
  off += __popcll(b & ((1ull << lane) - 1ull));
  if (xyz_out) {
    xyz_out[3 * (size_t)off] = x;
    xyz_out[3 * (size_t)off + 1] = y;
    xyz_out[3 * (size_t)off + 2] = z;
  }
  if (idx_out) idx_out[off] = i;
}

// the refinement's nine sums on one wave (the profiling build's comparison): the 64 lanes load 64 points, every
// lane adds them in order, so every lane holds the same sequential sums
__global__ __launch_bounds__(64) void accu_kernel(const float *__restrict__ xyz, int m, float *__restrict__ out) {
  const int lane = threadIdx.x;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f, a8 = 0.f;
  for (int base = 0; base < m; base += 64) {
    const int i = base + lane;
    const float x = i < m ? xyz[3 * (size_t)i] : 0.f, y = i < m ? xyz[3 * (size_t)i + 1] : 0.f, z = i < m ? xyz[3 * (size_t)i + 2] : 0.f;
    const int cnt = min(64, m - base);
    for (int j = 0; j < cnt; j++) {
      const float xj = __shfl(x, j), yj = __shfl(y, j), zj = __shfl(z, j);
      a0 += xj * xj;
      a1 += xj * yj;
      a2 += xj * zj;
      a3 += yj * yj;
      a4 += yj * zj;
      a5 += zj * zj;
      a6 += xj;
      a7 += yj;
      a8 += zj;
    }
  }
  if (lane == 0) {
    out[0] = a0;
    out[1] = a1;
    out[2] = a2;
    out[3] = a3;
    out[4] = a4;
    out[5] = a5;
    out[6] = a6;
    out[7] = a7;
    out[8] = a8;
  }
}

// flag / scan / write over the cloud for the points whose test against c equals `want`
hipError_t compact(PlaneState &s, const Cloud &c, float4 plane, float thr, int want, float *xyz_out, int32_t *idx_out, hipStream_t stream) {
  const int n = c.num_points, nb = (n + kFlagThreads - 1) / kFlagThreads;
  flag_count_kernel<<<nb, kFlagThreads, 0, stream>>>(c.px, c.py, c.pz, n, plane, thr, want, s.d_block_count);
  scan_kernel<<<1, 1024, 0, stream>>>(s.d_block_count, nb, s.d_block_off, reinterpret_cast<PlaneMeta *>(s.d_meta));
  flag_write_kernel<<<nb, kFlagThreads, 0, stream>>>(c.px, c.py, c.pz, n, plane, thr, want, s.d_block_off, xyz_out, idx_out);
  return hipGetLastError();
}

}  // namespace

int plane_reserve(PlaneState &s, int n) {
  if (!s.d_meta) {
    HIP_RET(device_alloc(s.d_meta, sizeof(PlaneMeta)));
    HIP_RET(device_alloc(s.d_coef, kPlaneMaxHyp));
    HIP_RET(device_alloc(s.d_counts, kPlaneMaxHyp));
    HIP_RET(device_alloc(s.d_accu, 9));
    HIP_RET(pinned_alloc(s.h_pin, sizeof(PlaneMeta) + kPlaneMaxHyp * (sizeof(float4) + sizeof(int32_t)) + 16 * sizeof(float)));
    note_alloc("plane: fixed buffers");
  }
  if (n > s.capacity) {
    const int cap = slack_cap(n, 4) + 1024;
    const int nb = (cap + kFlagThreads - 1) / kFlagThreads;
    device_release(s.d_block_count, s.d_block_off, s.d_xyz, s.d_idx);
    s.capacity = 0;
    HIP_RET(device_alloc(s.d_block_count, (size_t)nb));
    HIP_RET(device_alloc(s.d_block_off, (size_t)nb));
    HIP_RET(device_alloc(s.d_xyz, (size_t)cap * 3));
    HIP_RET(device_alloc(s.d_idx, (size_t)cap));
    note_alloc("plane: compaction buffers");
    s.capacity = cap;
  }
  return GPD_OK;
}

void plane_free(PlaneState &s) {
  device_release(s.d_meta, s.d_coef, s.d_counts, s.d_accu, s.d_block_count, s.d_block_off, s.d_xyz, s.d_idx);
  pinned_release(s.h_pin);
  s = PlaneState();
}

int plane_fit_run(PlaneState &s, const Cloud &c, double threshold, int max_iterations, double probability, int optimize, int32_t *indices_out,
                  int *num_out, float coeffs[4], int *num_inliers, int *iterations, hipStream_t stream) {
  StageRange range_("gpd:sample_above_plane");
  const int n = c.num_points;
  *num_out = 0;
  *num_inliers = 0;
  *iterations = 0;
  for (int a = 0; a < 4; a++) coeffs[a] = 0.f;
  if (n < 3) return GPD_OK;  // no sample can be drawn: no model
  int rc = plane_reserve(s, n);
  if (rc) return rc;
  const int H = max_iterations + 1;
  const float thr = plane::threshold_f32(threshold);
  PlaneMeta *d_meta = reinterpret_cast<PlaneMeta *>(s.d_meta);
  PlaneMeta *h_meta = reinterpret_cast<PlaneMeta *>(s.h_pin);
  float4 *h_coef = reinterpret_cast<float4 *>(s.h_pin + sizeof(PlaneMeta));
  int32_t *h_counts = reinterpret_cast<int32_t *>(h_coef + kPlaneMaxHyp);
  float *h_accu = reinterpret_cast<float *>(h_counts + kPlaneMaxHyp);

  // 1-2: the hypotheses and their inlier counts, back in one copy
  HIP_RET(hipMemsetAsync(s.d_counts, 0, (size_t)H * sizeof(int32_t), stream));
  hypothesis_kernel<<<1, 64, 0, stream>>>(c.pxyz, n, H, s.d_coef, d_meta);
  count_kernel<<<(n + kCountThreads * kPtsPerThread - 1) / (kCountThreads * kPtsPerThread), kCountThreads, 0, stream>>>(c.px, c.py, c.pz, n, s.d_coef,
                                                                                                                    d_meta, thr, s.d_counts);
  HIP_RET(hipGetLastError());
  HIP_RET(hipMemcpyAsync(h_meta, d_meta, sizeof(PlaneMeta), hipMemcpyDeviceToHost, stream));
  HIP_RET(hipMemcpyAsync(h_coef, s.d_coef, (size_t)H * sizeof(float4), hipMemcpyDeviceToHost, stream));
  HIP_RET(hipMemcpyAsync(h_counts, s.d_counts, (size_t)H * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_RET(hipStreamSynchronize(stream));
  if (h_meta->overflow) {
    set_error("gpd_hip_sample_above_plane: the draws touched more than %d positions of the shuffled index list (capacity)", kPlaneSwapCap);
    return GPD_ERR_CAPACITY;
  }

  // 3: RANSAC's loop over the hypotheses in order
  int best = 0, best_h = -1, it = 0;
  double k = std::numeric_limits<double>::max();
  while (it < k) {
    if (it >= h_meta->hyps) break;  // the draw was empty
    if (h_counts[it] > best) {
      best = h_counts[it];
      best_h = it;
      k = plane::stop_bound(best, n, probability);
    }
    ++it;
    if (it > max_iterations) break;
  }
  *iterations = it;
  if (best_h < 0) return GPD_OK;
  float model[4] = {h_coef[best_h].x, h_coef[best_h].y, h_coef[best_h].z, h_coef[best_h].w};

  // 4: refinement from the best model's inliers, in index order
  if (optimize && best > 3) {
    HIP_RET(compact(s, c, make_float4(model[0], model[1], model[2], model[3]), thr, 1, s.d_xyz, nullptr, stream));
    const char *where = prof_env("GPD_PLANE_REFINE");
    if (where && !strcmp(where, "device")) {
      accu_kernel<<<1, 64, 0, stream>>>(s.d_xyz, best, s.d_accu);
      HIP_RET(hipGetLastError());
      HIP_RET(hipMemcpyAsync(h_accu, s.d_accu, 9 * sizeof(float), hipMemcpyDeviceToHost, stream));
      HIP_RET(hipStreamSynchronize(stream));
      plane::refine_from_accu(h_accu, best, model);
    } else {
      s.h_xyz.resize((size_t)best * 3);
      HIP_RET(hipMemcpyAsync(s.h_xyz.data(), s.d_xyz, (size_t)best * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
      HIP_RET(hipStreamSynchronize(stream));
      plane::Accu acc;
      for (int i = 0; i < best; i++) acc.add(s.h_xyz[3 * (size_t)i], s.h_xyz[3 * (size_t)i + 1], s.h_xyz[3 * (size_t)i + 2]);
      plane::refine_from_accu(acc.a, best, model);
    }
  }
  for (int a = 0; a < 4; a++) coeffs[a] = model[a];

  // 5: the points off the final plane, ascending
  HIP_RET(compact(s, c, make_float4(model[0], model[1], model[2], model[3]), thr, 0, nullptr, s.d_idx, stream));
  HIP_RET(hipMemcpyAsync(h_meta, d_meta, sizeof(PlaneMeta), hipMemcpyDeviceToHost, stream));
  HIP_RET(hipStreamSynchronize(stream));
  const int m = h_meta->total;
  if (m < 0 || m > n) {
    set_error("gpd_hip_sample_above_plane: compaction wrote %d of %d points", m, n);
    return GPD_ERR_HIP;
  }
  if (m > 0 && indices_out) {
    HIP_RET(hipMemcpyAsync(indices_out, s.d_idx, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_RET(hipStreamSynchronize(stream));
  }
  *num_inliers = n - m;
  *num_out = m;
  return GPD_OK;
}

}  // namespace gpd
