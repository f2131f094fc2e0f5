// Cloud::refineNormals(k) on the device (util/cloud.cpp:176-204): the k nearest neighbours of every point, then
// pcl::NormalRefinement's Jacobi passes — the definition is DESIGN §7 ("refineNormals") and refine_model.h, the host model
// this path equals bit for bit.  On the cloud uploaded last (Cloud::g_p, pnrm), which never leaves the device:
//   1. knn_kernel, a WAVE per point in cell order (neighbouring waves share grid cells in L1): the shell search of the cloud's
//      uniform grid that knn_device.h holds (outliers.hip runs it too), which leaves the k nearest (d2 bits, index) keys sorted
//      in the wave's LDS row.  The sorted indices leave as [P / 64][k][64]: lane p of a block reads one contiguous row per rank.
//   2. refine_pass_kernel, a LANE per point: the k normals of its list gathered, the finite ones summed in list order (k
//      sequential float adds), sqrtf and three divisions — the correctly rounded sequences (-ffp-contract=off, Makefile;
//      hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt) — and the dot product with the point's old normal.
//   3. on the host, between passes: the stop rule's sequential float sum of the dots in ascending index order
//      (refine::StopRule).  It overlaps the next pass, launched speculatively on the other buffer of a ping-pong pair: a
//      stop discards it.
//   4. the result replaces the cloud's normals (planes nx, ny, nz and pnrm); the cloud's generation moves on.
#include "gpd_internal.h"
#include "buffers.h"
#include "knn_device.h"

#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

namespace gpd {

namespace {

struct KnnParams {
  KnnSearch search;
  int32_t *lists;           // [ceil(P / 64)][k][64] by cell-order position
};

// the search (knn_device.h), then the sorted indices of the row out to the lists
__global__ __launch_bounds__(64 * KN_WAVES) void knn_kernel(KnnParams P) {
  __shared__ KnnLds s;
  const int lane = threadIdx.x & 63;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int w = blockIdx.x * KN_WAVES + wv;
  if (w >= P.search.num_points) return;
  const unsigned long long *keys = s.keys[wv];
  const int k = P.search.k;
  const int n = knn_search_row(P.search, w, lane, s.keys[wv], s.beg[wv], s.off[wv]);
  int32_t *row = P.lists + (size_t)(w >> 6) * k * 64 + (w & 63);
  for (int r = lane; r < n; r += 64) row[(size_t)r * 64] = (int32_t)(unsigned)keys[r];
}

__device__ __forceinline__ bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// one Jacobi pass: in / out by original index, a lane per cell-order position w (its list is a contiguous row per rank)
__global__ __launch_bounds__(256) void refine_pass_kernel(const float4 *__restrict__ gp, const int32_t *__restrict__ lists, int num_points, int k,
                                                          const float4 *__restrict__ in, float4 *__restrict__ out, float *__restrict__ dots) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= num_points) return;
  const int j = __float_as_int(gp[w].w);
  const int32_t *row = lists + (size_t)(w >> 6) * k * 64 + (w & 63);
  float nx = 0.f, ny = 0.f, nz = 0.f;
#pragma unroll 8
  for (int r = 0; r < k; r++) {
    const float4 v = in[row[(size_t)r * 64]];
    if (finite3(v.x, v.y, v.z)) {
      nx += 1.0f * v.x;
      ny += 1.0f * v.y;
      nz += 1.0f * v.z;
    }
  }
  const float norm = sqrtf(nx * nx + ny * ny + nz * nz);
  const float nan = __int_as_float(0x7fc00000);
  float4 t = make_float4(nan, nan, nan, 0.f);
  if (isfinite(norm) && norm > FLT_EPSILON) t = make_float4(nx / norm, ny / norm, nz / norm, 0.f);
  out[j] = t;
  const float4 o = in[j];
  dots[j] = finite3(t.x, t.y, t.z) ? t.x * o.x + t.y * o.y + t.z * o.z : nan;
}

// the result into the cloud's normal planes and an AoS copy for the caller
__global__ void refine_store_kernel(const float4 *__restrict__ res, int num_points, float *nx, float *ny, float *nz, float4 *pnrm, float *aos) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num_points) return;
  const float4 v = res[i];
  nx[i] = v.x;
  ny[i] = v.y;
  nz[i] = v.z;
  pnrm[i] = make_float4(v.x, v.y, v.z, 0.f);
  aos[3 * (size_t)i] = v.x;
  aos[3 * (size_t)i + 1] = v.y;
  aos[3 * (size_t)i + 2] = v.z;
}

// the resident form's only scalar: normals with a non-finite component (a ballot per wave, one atomic per wave that has any)
__global__ __launch_bounds__(256) void refine_count_nan_kernel(const float4 *__restrict__ res, int num_points, int32_t *count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  bool bad = false;
  if (i < num_points) {
    const float4 v = res[i];
    bad = !finite3(v.x, v.y, v.z);
  }
  const unsigned long long m = __ballot(bad);
  if (m && (threadIdx.x & 63) == 0) atomicAdd(count, (int32_t)__popcll(m));
}

}  // namespace

int refine_reserve(RefineState &s, int n, int k) {
  const size_t lists = ((size_t)n + 63) / 64 * 64 * (size_t)k;
  if (n > s.cap_points) {
    note_alloc(__func__);
    for (float4 *&b : s.d_buf) device_release(b);
    device_release(s.d_dots, s.d_aos);
    pinned_release(s.h_dots);
    s.cap_points = 0;
    const int cap = slack_cap(n, 4);
    for (float4 *&b : s.d_buf) HIP_RET(device_alloc(b, (size_t)cap));
    HIP_RET(device_alloc(s.d_dots, (size_t)cap));
    HIP_RET(device_alloc(s.d_aos, (size_t)cap * 3));
    HIP_RET(pinned_alloc(s.h_dots, (size_t)cap * 2));
    s.cap_points = cap;
  }
  const int rc = grow_device(s.d_lists, s.cap_lists, lists, slack_cap(lists, 4), __func__);
  if (rc) return rc;
  if (!s.ev_dots[0])
    for (hipEvent_t &e : s.ev_dots) HIP_RET(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  if (!s.d_nan) {
    HIP_RET(device_alloc(s.d_nan, 1));
    HIP_RET(pinned_alloc(s.h_nan, 1));
  }
  return GPD_OK;
}

void refine_free(RefineState &s) {
  device_release(s.d_lists);
  for (float4 *&b : s.d_buf) device_release(b);
  device_release(s.d_dots, s.d_aos);
  pinned_release(s.h_dots);
  device_release(s.d_nan);
  pinned_release(s.h_nan);
  for (hipEvent_t e : s.ev_dots)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : s.ev)
    if (e) (void)hipEventDestroy(e);
  s = RefineState();
}

int refine_run(RefineState &s, Cloud &c, int k, int max_iterations, float threshold, float *normals_out, int *iterations_out, float *ddot_out,
               int *num_nan_out, float *kernel_ms, hipStream_t stream) {
  StageRange range_("gpd:refine_normals");
  const auto t_start = std::chrono::steady_clock::now();
  const int n = c.num_points;
  const int kk = k < n ? k : n;  // KdTreeFLANN::nearestKSearch clamps k to the cloud's size
  int rc = refine_reserve(s, n, kk);
  if (rc) return rc;
  const size_t need_ev = 2 + 2 * (size_t)max_iterations;
  while (s.ev.size() < need_ev) {
    hipEvent_t e;
    HIP_RET(hipEventCreate(&e));
    s.ev.push_back(e);
  }

  // 1: the lists
  KnnParams kp;
  knn_search_fill(kp.search, c, kk);
  kp.lists = s.d_lists;
  HIP_RET(hipEventRecord(s.ev[0], stream));
  knn_kernel<<<(n + KN_WAVES - 1) / KN_WAVES, 64 * KN_WAVES, 0, stream>>>(kp);
  HIP_RET(hipGetLastError());
  HIP_RET(hipEventRecord(s.ev[1], stream));

  // 2-3: the passes, ping-pong between d_buf[0] (a copy of the cloud's normals: an error leaves those as they were) and d_buf[1]
  HIP_RET(hipMemcpyAsync(s.d_buf[0], c.pnrm, (size_t)n * sizeof(float4), hipMemcpyDeviceToDevice, stream));
  const bool need_dots = threshold > 0.f || ddot_out;
  int launched = 0;
  auto launch = [&](int t) -> int {
    HIP_RET(hipEventRecord(s.ev[2 + 2 * (size_t)t], stream));
    refine_pass_kernel<<<(n + 255) / 256, 256, 0, stream>>>(c.g_p, s.d_lists, n, kk, s.d_buf[t & 1], s.d_buf[(t + 1) & 1], s.d_dots);
    HIP_RET(hipGetLastError());
    HIP_RET(hipEventRecord(s.ev[3 + 2 * (size_t)t], stream));
    if (need_dots) {
      HIP_RET(hipMemcpyAsync(s.h_dots + (size_t)(t & 1) * s.cap_points, s.d_dots, (size_t)n * sizeof(float), hipMemcpyDeviceToHost, stream));
      HIP_RET(hipEventRecord(s.ev_dots[t & 1], stream));
    }
    launched = t + 1;
    return GPD_OK;
  };
  int done = 0;
  if (max_iterations > 0 && (rc = launch(0))) return rc;
  for (int t = 0; t < max_iterations; t++) {
    if (t + 1 < max_iterations && (rc = launch(t + 1))) return rc;  // speculative: runs while the host sums pass t
    done = t + 1;
    if (need_dots) {
      HIP_RET(hipEventSynchronize(s.ev_dots[t & 1]));
      refine::StopRule st;
      st.add(s.h_dots + (size_t)(t & 1) * s.cap_points, n);
      const float mean = st.mean();
      if (ddot_out) ddot_out[t] = mean;
      if (refine::StopRule::stop(mean, threshold)) break;
    }
  }

  // 4: pass `done` wrote d_buf[done & 1]
  refine_store_kernel<<<(n + 255) / 256, 256, 0, stream>>>(s.d_buf[done & 1], n, c.nx, c.ny, c.nz, c.pnrm, s.d_aos);
  HIP_RET(hipGetLastError());
  int nan = 0;
  if (normals_out) {
    HIP_RET(hipMemcpyAsync(normals_out, s.d_aos, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIP_RET(hipStreamSynchronize(stream));
    for (int i = 0; i < n; i++) nan += !refine::finite3(normals_out[3 * (size_t)i], normals_out[3 * (size_t)i + 1], normals_out[3 * (size_t)i + 2]);
  } else {
    HIP_RET(hipMemsetAsync(s.d_nan, 0, sizeof(int32_t), stream));
    refine_count_nan_kernel<<<(n + 255) / 256, 256, 0, stream>>>(s.d_buf[done & 1], n, s.d_nan);
    HIP_RET(hipGetLastError());
    HIP_RET(hipMemcpyAsync(s.h_nan, s.d_nan, sizeof(int32_t), hipMemcpyDeviceToHost, stream));
    HIP_RET(hipStreamSynchronize(stream));
    nan = *s.h_nan;
  }
  c.generation++;
  *iterations_out = done;
  *num_nan_out = nan;
  if (kernel_ms) {
    float ms = 0.f, passes = 0.f;
    HIP_RET(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
    for (int t = 0; t < launched; t++) {
      float m = 0.f;
      HIP_RET(hipEventElapsedTime(&m, s.ev[2 + 2 * (size_t)t], s.ev[3 + 2 * (size_t)t]));
      passes += m;
    }
    kernel_ms[0] = ms;
    kernel_ms[1] = passes;
    kernel_ms[2] = (float)(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count());
  }
  return GPD_OK;
}

}  // namespace gpd
