// Cloud::removeStatisticalOutliers on the device (util/cloud.cpp:166-174): PCL 1.9's StatisticalOutlierRemoval — the
// definition is DESIGN §7 ("removeStatisticalOutliers") and outlier_model.h, the host model this path equals bit for bit.
// On the cloud uploaded last, which never leaves the device:
//   1. outlier_dist_kernel, a WAVE per point in cell order: the shell search of knn_device.h (the one knn_kernel of refine.hip
//      runs) for the mean_k + 1 nearest keys, then the epilogue — the lanes take the correctly rounded sqrtf of their ranks'
//      d2, and the wave adds them as doubles in rank order 1 .. mean_k (a wave-uniform chain: every lane holds the same sum).
//      One float per point leaves, by original index; no neighbour list goes to memory.
//   2. on the host, between the kernels: the two sequential double sums over the points in index order and the threshold
//      (outlier::threshold), over the pinned copy of those floats — 4 N bytes down, 8 bytes up as a kernel argument.
//   3. the keep mask `!((double)dist > threshold)`, compacted in index order (flag / scan / write, integer scans only): the
//      kept indices, their xyz, normals and camera-source rows.
//   4. cloud_from_device makes the kept points the cloud (grid rebuilt, generation bumped), cloud_set_normals carries the
//      normals over.
// -ffp-contract=off (Makefile): every expression is evaluated unfused.
#include "gpd_internal.h"
#include "buffers.h"
#include "knn_device.h"
#include "outlier_model.h"
#include "wave_ops.h"

#include <chrono>
#include <cstring>

namespace gpd {

namespace {

constexpr int kFlagThreads = 256;  // compaction: one point per thread

struct DistParams {
  KnnSearch search;  // k = mean_k + 1 <= num_points
  float *dist;       // [P] by original index
};

__global__ __launch_bounds__(64 * KN_WAVES) void outlier_dist_kernel(DistParams P) {
  __shared__ KnnLds s;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int w = blockIdx.x * KN_WAVES + wv;
  if (w >= P.search.num_points) return;
  const int n = knn_search_row(P.search, w, lane, s.keys[wv], s.beg[wv], s.off[wv]);
  const unsigned long long *keys = s.keys[wv];
  const int mean_k = P.search.k - 1;
  // rank r = 64 j + lane: its sqrtf; the row holds n <= kRefineKCap = 4 * 64 sorted keys
  float root[4];
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int r = 64 * j + lane;
    root[j] = r < n ? sqrtf(__uint_as_float((unsigned)(keys[r] >> 32))) : 0.f;
  }
  const int last = mean_k < n - 1 ? mean_k : n - 1;  // (n == mean_k + 1: the caller refuses clouds smaller than that)
  double dist_sum = 0.0;
#pragma unroll
  for (int j = 0; j < 4; j++)
    for (int l = j == 0 ? 1 : 0; l < 64 && 64 * j + l <= last; l++)  // wave-uniform bounds: rank 0 is skipped whatever point it is
      dist_sum += (double)__int_as_float(__builtin_amdgcn_readlane(__float_as_int(root[j]), l));
  if (lane == 0) P.dist[__float_as_int(P.search.grid.p[w].w)] = (float)(dist_sum / (double)mean_k);
}

__device__ __forceinline__ bool keeps(float dist, double threshold) { return !((double)dist > threshold); }

// ordered compaction of the kept points: per-block counts, one-workgroup scan, write
__global__ __launch_bounds__(kFlagThreads) void keep_count_kernel(const float *__restrict__ dist, int n, double threshold,
                                                                  int32_t *__restrict__ block_count) {
  __shared__ int s_cnt[kFlagThreads / 64];
  const int i = blockIdx.x * kFlagThreads + threadIdx.x;
  const bool f = i < n && keeps(dist[i], threshold);
  const unsigned long long b = __builtin_amdgcn_ballot_w64(f);
  if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = __popcll(b);
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kFlagThreads / 64; w++) t += s_cnt[w];
    block_count[blockIdx.x] = t;
  }
}

__global__ __launch_bounds__(1024) void keep_scan_kernel(const int32_t *__restrict__ block_count, int nblocks, int32_t *__restrict__ block_off,
                                                         int32_t *__restrict__ total) {
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
  if (tid == 0) *total = s_carry;
}

struct KeepSource {
  const float *px, *py, *pz, *nx, *ny, *nz;  // nx == nullptr: the normals are zeros
  const int32_t *cam;                        // [cams][n]
  int n, cams;
};

// the kept points in index order: their indices, xyz, normals and camera-source rows ([cams][*total])
__global__ __launch_bounds__(kFlagThreads) void keep_write_kernel(KeepSource src, const float *__restrict__ dist, double threshold,
                                                                  const int32_t *__restrict__ block_off, const int32_t *__restrict__ total,
                                                                  int32_t *__restrict__ kept, float *__restrict__ xyz, float *__restrict__ nrm,
                                                                  int32_t *__restrict__ cam) {
  __shared__ int s_cnt[kFlagThreads / 64];
  const int i = blockIdx.x * kFlagThreads + threadIdx.x;
  const bool f = i < src.n && keeps(dist[i], threshold);
  const unsigned long long b = __builtin_amdgcn_ballot_w64(f);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) s_cnt[wave] = __popcll(b);
  __syncthreads();
  if (!f) return;
  int off = block_off[blockIdx.x];
  for (int w = 0; w < wave; w++) off += s_cnt[w];
  off += __popcll(b & ((1ull << lane) - 1ull));
  const int m = *total;  // off < m <= n
  kept[off] = i;
  xyz[3 * (size_t)off] = src.px[i];
  xyz[3 * (size_t)off + 1] = src.py[i];
  xyz[3 * (size_t)off + 2] = src.pz[i];
  nrm[3 * (size_t)off] = src.nx ? src.nx[i] : 0.f;
  nrm[3 * (size_t)off + 1] = src.nx ? src.ny[i] : 0.f;
  nrm[3 * (size_t)off + 2] = src.nx ? src.nz[i] : 0.f;
  for (int c = 0; c < src.cams; c++) cam[(size_t)c * m + off] = src.cam[(size_t)c * src.n + i];
}

}  // namespace

int outlier_reserve(OutlierState &s, int n, int num_cams) {
  if (n > s.cap_points || num_cams > s.cap_cams) {
    note_alloc(__func__);
    device_release(s.d_dist, s.d_block_count, s.d_block_off, s.d_kept, s.d_xyz, s.d_nrm, s.d_cam);
    pinned_release(s.h_dist);
    const int cap = n > s.cap_points ? slack_cap(n, 4) : s.cap_points;
    const int cams = num_cams > s.cap_cams ? num_cams : s.cap_cams;
    s.cap_points = s.cap_cams = 0;
    const size_t blocks = ((size_t)cap + kFlagThreads - 1) / kFlagThreads + 1;
    HIP_RET(device_alloc(s.d_dist, (size_t)cap));
    HIP_RET(pinned_alloc(s.h_dist, (size_t)cap));
    HIP_RET(device_alloc(s.d_block_count, blocks));
    HIP_RET(device_alloc(s.d_block_off, blocks));
    HIP_RET(device_alloc(s.d_kept, (size_t)cap));
    HIP_RET(device_alloc(s.d_xyz, (size_t)cap * 3));
    HIP_RET(device_alloc(s.d_nrm, (size_t)cap * 3));
    HIP_RET(device_alloc(s.d_cam, (size_t)cap * cams));
    s.cap_points = cap;
    s.cap_cams = cams;
  }
  if (!s.d_total) {
    HIP_RET(device_alloc(s.d_total, 1));
    HIP_RET(pinned_alloc(s.h_total, 1));
  }
  if (!s.ev[0])
    for (hipEvent_t &e : s.ev) HIP_RET(hipEventCreate(&e));
  return GPD_OK;
}

void outlier_free(OutlierState &s) {
  device_release(s.d_dist, s.d_block_count, s.d_block_off, s.d_kept, s.d_xyz, s.d_nrm, s.d_cam, s.d_total);
  pinned_release(s.h_dist);
  pinned_release(s.h_total);
  for (hipEvent_t e : s.ev)
    if (e) (void)hipEventDestroy(e);
  s = OutlierState();
}

int outlier_run(OutlierState &s, Cloud &c, int mean_k, double mult, bool carry_normals, int32_t *kept_out, int *num_kept, double stats[3],
                float *dist_out, float *kernel_ms, hipStream_t stream) {
  StageRange range_("gpd:remove_statistical_outliers");
  const auto t_start = std::chrono::steady_clock::now();
  const int n = c.num_points, cams = c.num_cams;
  if (outlier::refusal(n, mean_k, mult)) {  // the callers refuse with their own texts; no kernel runs outside the domain
    set_error("remove_statistical_outliers: mean_k = %d on %d points is outside the domain", mean_k, n);
    return GPD_ERR_INVALID;
  }
  int rc = outlier_reserve(s, n, cams);
  if (rc) return rc;

  // 1: the mean distances
  DistParams dp;
  knn_search_fill(dp.search, c, mean_k + 1);
  dp.dist = s.d_dist;
  HIP_RET(hipEventRecord(s.ev[0], stream));
  outlier_dist_kernel<<<(n + KN_WAVES - 1) / KN_WAVES, 64 * KN_WAVES, 0, stream>>>(dp);
  HIP_RET(hipGetLastError());
  HIP_RET(hipEventRecord(s.ev[1], stream));
  HIP_RET(hipMemcpyAsync(s.h_dist, s.d_dist, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, stream));
  HIP_RET(hipStreamSynchronize(stream));

  // 2: the threshold
  const outlier::Stats st = outlier::threshold(s.h_dist, n, mult);
  stats[0] = st.mean;
  stats[1] = st.stddev;
  stats[2] = st.threshold;
  if (dist_out) std::memcpy(dist_out, s.h_dist, (size_t)n * sizeof(float));

  // 3: the kept points
  const int nblocks = (n + kFlagThreads - 1) / kFlagThreads;
  KeepSource src;
  src.px = c.px;
  src.py = c.py;
  src.pz = c.pz;
  src.nx = carry_normals ? c.nx : nullptr;
  src.ny = c.ny;
  src.nz = c.nz;
  src.cam = c.cam_source;
  src.n = n;
  src.cams = cams;
  HIP_RET(hipEventRecord(s.ev[2], stream));
  keep_count_kernel<<<nblocks, kFlagThreads, 0, stream>>>(s.d_dist, n, st.threshold, s.d_block_count);
  keep_scan_kernel<<<1, 1024, 0, stream>>>(s.d_block_count, nblocks, s.d_block_off, s.d_total);
  keep_write_kernel<<<nblocks, kFlagThreads, 0, stream>>>(src, s.d_dist, st.threshold, s.d_block_off, s.d_total, s.d_kept, s.d_xyz, s.d_nrm,
                                                           s.d_cam);
  HIP_RET(hipGetLastError());
  HIP_RET(hipEventRecord(s.ev[3], stream));
  HIP_RET(hipMemcpyAsync(s.h_total, s.d_total, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
  HIP_RET(hipStreamSynchronize(stream));
  const int m = *s.h_total;
  if (m < 1 || m > n) {
    set_error("remove_statistical_outliers: no point is left (threshold %g)", st.threshold);
    return GPD_ERR_INVALID;
  }
  if (kept_out) {
    HIP_RET(hipMemcpyAsync(kept_out, s.d_kept, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_RET(hipStreamSynchronize(stream));
  }
  *num_kept = m;

  // 4: the kept points become the cloud
  double view_points[3 * kMaxCams];
  std::memcpy(view_points, c.view_points, sizeof(view_points));
  rc = cloud_from_device(c, s.d_xyz, s.d_cam, m, cams, view_points, stream);
  if (!rc && carry_normals) rc = cloud_set_normals(c, s.d_nrm, stream);
  if (rc) return rc;
  if (kernel_ms) {
    HIP_RET(hipStreamSynchronize(stream));
    HIP_RET(hipEventElapsedTime(&kernel_ms[0], s.ev[0], s.ev[1]));
    HIP_RET(hipEventElapsedTime(&kernel_ms[1], s.ev[2], s.ev[3]));
    kernel_ms[2] = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
  }
  return GPD_OK;
}

}  // namespace gpd
