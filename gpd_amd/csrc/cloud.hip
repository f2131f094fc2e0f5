// The device copy of a point cloud on gfx950: the caller's AoS arrays split into SoA planes, and the uniform 2 cm
// grid (counting sort by cell) that the radius searches (search.hip, normals.hip) and the k-nearest-neighbour search
// (refine.hip) visit instead of walking PCL's k-d tree.
#include <cfloat>
#include <cmath>
#include <cstring>

#include "gpd_internal.h"
#include "buffers.h"
#include "grid_sort.h"
#include "wave_ops.h"

namespace gpd {

// ---------------------------------------------------------------------------
// Cloud upload: AoS (caller layout) -> SoA planes.
// ---------------------------------------------------------------------------
// pxyz.w carries the first camera's flag of the point (bits of the int): the gather of neighbourhood_kernel then needs no
// third random access per neighbour (that phase is bound by the address unit: one lane per cycle and load)
__global__ void split_soa_kernel(const float *__restrict__ xyz, const float *__restrict__ nrm, const int32_t *__restrict__ cam0, int n,
                                 float *px, float *py, float *pz, float *nx, float *ny, float *nz, float4 *pxyz, float4 *pnrm) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
  const float a = nrm[3 * i], b = nrm[3 * i + 1], c = nrm[3 * i + 2];
  px[i] = x;
  py[i] = y;
  pz[i] = z;
  nx[i] = a;
  ny[i] = b;
  nz[i] = c;
  pxyz[i] = make_float4(x, y, z, __int_as_float(cam0[i]));
  pnrm[i] = make_float4(a, b, c, 0.f);
}
// the planes of c again, with the normals d_nrm [num_points][3] (normals_run's result) beside its staged coordinates
int cloud_set_normals(Cloud &c, const float *d_nrm, hipStream_t stream) {
  const int n = c.num_points;
  split_soa_kernel<<<(n + 255) / 256, 256, 0, stream>>>(c.staging, d_nrm, c.cam_source, n, c.px, c.py, c.pz, c.nx, c.ny, c.nz, c.pxyz, c.pnrm);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

// ---- uniform grid ----------------------------------------------------------------------
__global__ void grid_count_kernel(GridView g, const float *px, const float *py, const float *pz, int n, int32_t *counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (grid_coord(g, 0, px[i]) * g.dim[1] + grid_coord(g, 1, py[i])) * g.dim[2] + grid_coord(g, 2, pz[i]);
  atomicAdd(&counts[c], 1);
}
// exclusive scan of counts[0..n) into start[0..n], single workgroup with a running carry
__global__ __launch_bounds__(1024) void grid_scan_kernel(const int32_t *counts, int32_t *start, int32_t *cursor, int n) {
  __shared__ int s_part[16];
  __shared__ int s_carry;
  const int tid = threadIdx.x;
  if (tid == 0) s_carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const int off = block_scan_step(i < n ? counts[i] : 0, s_part, s_carry);
    if (i < n) {
      start[i] = off;
      cursor[i] = off;
    }
  }
  if (tid == 0) start[n] = s_carry;
}
__global__ void grid_scatter_kernel(GridView g, const float *px, const float *py, const float *pz, int n, int32_t *cursor,
                                    float4 *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int c = (grid_coord(g, 0, px[i]) * g.dim[1] + grid_coord(g, 1, py[i])) * g.dim[2] + grid_coord(g, 2, pz[i]);
  const int pos = atomicAdd(&cursor[c], 1);
  out[pos] = make_float4(px[i], py[i], pz[i], __int_as_float(i));
}

void cloud_free(Cloud &c) {
  normals_free(c.normals);
  device_release(c.px, c.py, c.pz, c.nx, c.ny, c.nz, c.cam_source, c.staging, c.g_start, c.g_cursor, c.g_p, c.pxyz, c.pnrm);
  pinned_release(c.h_pin);
  c = Cloud();
}

// Device + pinned staging buffers for clouds of up to n points / num_cams cameras (grows with 25 % slack, never
// shrinks).  A growth is hipFree + hipMalloc, i.e. a device stall: gpd_hip_reserve / gpd_hip_detect_batch size the lanes
// once, ahead of the first cloud.
int cloud_reserve(Cloud &c, int n, int num_cams) {
  if (n <= c.capacity && num_cams <= c.cap_cams) return GPD_OK;
  note_alloc(__func__);
  const uint64_t gen = c.generation;
  const int cap = n > c.capacity ? slack_cap(n, 4) : c.capacity;  // slack: clouds of a batch differ by a few points
  const int cams = num_cams > c.cap_cams ? num_cams : c.cap_cams;
  const int cells_cap = c.g_cells_cap;
  cloud_free(c);  // hipFree waits for the device: kernels of an earlier cloud on this stream are done
  c.generation = gen;
  float **planes[] = {&c.px, &c.py, &c.pz, &c.nx, &c.ny, &c.nz};
  for (float **p : planes) HIP_RET(device_alloc(*p, (size_t)cap));
  float4 **quads[] = {&c.g_p, &c.pxyz, &c.pnrm};
  for (float4 **p : quads) HIP_RET(device_alloc(*p, (size_t)cap));
  HIP_RET(device_alloc(c.cam_source, (size_t)cap * cams));
  HIP_RET(device_alloc(c.staging, (size_t)cap * 6 + 8));  // + 8: the bounds of a cloud handed over on the device
  HIP_RET(pinned_alloc(c.h_pin, (size_t)cap * (6 * sizeof(float) + cams * sizeof(int32_t)) + 32));
  c.capacity = cap;
  c.cap_cams = cams;
  if (cells_cap > 0) {  // the grid tables keep their size across a growth of the point buffers
    HIP_RET(device_alloc(c.g_start, (size_t)cells_cap + 1));
    HIP_RET(device_alloc(c.g_cursor, (size_t)cells_cap));
    c.g_cells_cap = cells_cap;
  }
  return GPD_OK;
}

// The uniform grid's tables for scenes of up to `cells` cells of 2 cm (a 2 x 2 x 1 m scene has 500 000); a larger scene grows them.
int cloud_reserve_grid(Cloud &c, int cells) {
  if (cells <= c.g_cells_cap) return GPD_OK;
  note_alloc(__func__);
  device_release(c.g_start, c.g_cursor);
  c.g_cells_cap = 0;
  HIP_RET(device_alloc(c.g_start, (size_t)cells + 1));
  HIP_RET(device_alloc(c.g_cursor, (size_t)cells));
  c.g_cells_cap = cells;
  return GPD_OK;
}

// The caller's arrays are copied into a pinned staging buffer (one pass that also takes the bounds of the
// uniform grid and rejects non-finite coordinates), so the three host-to-device copies are truly
// asynchronous: with sync == false nothing here waits for the device and the upload of the next cloud
// overlaps the kernels of the current one (gpd_hip_detect_batch).
int cloud_upload(Cloud &c, const float *xyz, const float *normals, int n, const int32_t *cam_source, int num_cams,
                 const double *view_points, hipStream_t stream, bool sync) {
  if (num_cams > kMaxCams) {
    set_error("upload_cloud: at most %d cameras are supported", kMaxCams);
    return GPD_ERR_INVALID;
  }
  {
    const int rc = cloud_reserve(c, n, num_cams);
    if (rc) return rc;
  }
  float *hx = reinterpret_cast<float *>(c.h_pin), *hn = hx + (size_t)3 * n;
  int32_t *hc = reinterpret_cast<int32_t *>(hx + (size_t)6 * n);
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  bool finite = true;
  for (int i = 0; i < n; i++)
    for (int a = 0; a < 3; a++) {
      const float v = xyz[3 * (size_t)i + a];
      hx[3 * (size_t)i + a] = v;
      finite &= std::isfinite(v);
      lo[a] = v < lo[a] ? v : lo[a];
      hi[a] = v > hi[a] ? v : hi[a];
    }
  if (!finite) {  // pcl::removeNaNFromPointCloud runs before the path (candidates_generator.cpp:17); an Inf would
                  // make the grid dimensions undefined
    set_error("upload_cloud: the cloud holds non-finite coordinates (remove NaN/Inf points first)");
    return GPD_ERR_INVALID;
  }
  std::memcpy(hn, normals, (size_t)n * 3 * sizeof(float));
  std::memcpy(hc, cam_source, (size_t)n * num_cams * sizeof(int32_t));
  c.num_points = n;
  c.num_cams = num_cams;
  c.generation++;
  std::memcpy(c.view_points, view_points, sizeof(double) * 3 * num_cams);
  HIP_RET(hipMemcpyAsync(c.staging, hx, (size_t)n * 6 * sizeof(float), hipMemcpyHostToDevice, stream));
  HIP_RET(hipMemcpyAsync(c.cam_source, hc, (size_t)n * num_cams * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  split_soa_kernel<<<(n + 255) / 256, 256, 0, stream>>>(c.staging, c.staging + (size_t)n * 3, c.cam_source, n, c.px, c.py, c.pz, c.nx,
                                                         c.ny, c.nz, c.pxyz, c.pnrm);
  HIP_RET(hipGetLastError());
  // uniform grid: bounds from the pass above, counting sort on the device
  c.g_cell = 0.02f;
  for (;;) {  // at most 256 cells per axis
    bool ok = true;
    for (int a = 0; a < 3; a++) {
      c.g_lo[a] = lo[a];
      c.g_dim[a] = (int)std::floor((hi[a] - lo[a]) / c.g_cell) + 1;
      if (c.g_dim[a] > 256 || c.g_dim[a] < 1) ok = false;
    }
    if (ok) break;
    c.g_cell *= 2.f;
  }
  const int cells = c.g_dim[0] * c.g_dim[1] * c.g_dim[2];
  if (cells > c.g_cells_cap) {
    const int rc = cloud_reserve_grid(c, cells + cells / 2);
    if (rc) return rc;
  }
  GridView g = grid_view(c);
  HIP_RET(hipMemsetAsync(c.g_cursor, 0, (size_t)cells * sizeof(int32_t), stream));
  grid_count_kernel<<<(n + 255) / 256, 256, 0, stream>>>(g, c.px, c.py, c.pz, n, c.g_cursor);
  grid_scan_kernel<<<1, 1024, 0, stream>>>(c.g_cursor, c.g_start, c.g_cursor, cells);
  grid_scatter_kernel<<<(n + 255) / 256, 256, 0, stream>>>(g, c.px, c.py, c.pz, n, c.g_cursor, c.g_p);
  HIP_RET(hipGetLastError());
  if (sync) HIP_RET(hipStreamSynchronize(stream));
  return GPD_OK;
}

// min / max of n points [n][3] on the device -> out[6] (one workgroup: the clouds handed over on the device are the voxelised ones)
__global__ __launch_bounds__(1024) void bounds_kernel(const float *__restrict__ xyz, int n, float *__restrict__ out) {
  __shared__ float s_lo[16][3], s_hi[16][3];
  float lo[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, hi[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
  for (int i = threadIdx.x; i < n; i += 1024)
    for (int a = 0; a < 3; a++) {
      const float v = xyz[3 * (size_t)i + a];
      lo[a] = fminf(lo[a], v);
      hi[a] = fmaxf(hi[a], v);
    }
  for (int a = 0; a < 3; a++)
    for (int o = 32; o > 0; o >>= 1) {
      lo[a] = fminf(lo[a], __shfl_xor(lo[a], o));
      hi[a] = fmaxf(hi[a], __shfl_xor(hi[a], o));
    }
  if ((threadIdx.x & 63) == 0)
    for (int a = 0; a < 3; a++) {
      s_lo[threadIdx.x >> 6][a] = lo[a];
      s_hi[threadIdx.x >> 6][a] = hi[a];
    }
  __syncthreads();
  if (threadIdx.x < 3) {
    float l = FLT_MAX, h = -FLT_MAX;
    for (int w = 0; w < 16; w++) {
      l = fminf(l, s_lo[w][threadIdx.x]);
      h = fmaxf(h, s_hi[w][threadIdx.x]);
    }
    out[threadIdx.x] = l;
    out[3 + threadIdx.x] = h;
  }
}

// The cloud from arrays that are ALREADY on the device (the output of the preprocessing kernels: finite by construction):
// d_xyz [n][3], d_cam [cams][n]; normals zero until normals_run fills them.  One small wait: the bounds of the grid.
int cloud_from_device(Cloud &c, const float *d_xyz, const int32_t *d_cam, int n, int num_cams, const double *view_points, hipStream_t stream) {
  if (num_cams > kMaxCams || num_cams < 1 || n < 1) {
    set_error("cloud_from_device: bad argument");
    return GPD_ERR_INVALID;
  }
  {
    const int rc = cloud_reserve(c, n, num_cams);
    if (rc) return rc;
  }
  c.num_points = n;
  c.num_cams = num_cams;
  c.generation++;
  std::memcpy(c.view_points, view_points, sizeof(double) * 3 * num_cams);
  HIP_RET(hipMemcpyAsync(c.staging, d_xyz, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, stream));
  HIP_RET(hipMemsetAsync(c.staging + (size_t)n * 3, 0, (size_t)n * 3 * sizeof(float), stream));
  HIP_RET(hipMemcpyAsync(c.cam_source, d_cam, (size_t)n * num_cams * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
  float *hb = reinterpret_cast<float *>(c.h_pin);  // the pinned staging is free: nothing of this cloud came through it
  bounds_kernel<<<1, 1024, 0, stream>>>(c.staging, n, c.staging + (size_t)c.capacity * 6);
  HIP_RET(hipMemcpyAsync(hb, c.staging + (size_t)c.capacity * 6, 6 * sizeof(float), hipMemcpyDeviceToHost, stream));
  split_soa_kernel<<<(n + 255) / 256, 256, 0, stream>>>(c.staging, c.staging + (size_t)n * 3, c.cam_source, n, c.px, c.py, c.pz, c.nx,
                                                         c.ny, c.nz, c.pxyz, c.pnrm);
  HIP_RET(hipGetLastError());
  HIP_RET(hipStreamSynchronize(stream));
  const float *lo = hb, *hi = hb + 3;
  c.g_cell = 0.02f;
  for (;;) {  // at most 256 cells per axis
    bool ok = true;
    for (int a = 0; a < 3; a++) {
      c.g_lo[a] = lo[a];
      c.g_dim[a] = (int)std::floor((hi[a] - lo[a]) / c.g_cell) + 1;
      if (c.g_dim[a] > 256 || c.g_dim[a] < 1) ok = false;
    }
    if (ok) break;
    c.g_cell *= 2.f;
  }
  const int cells = c.g_dim[0] * c.g_dim[1] * c.g_dim[2];
  if (cells > c.g_cells_cap) {
    const int rc = cloud_reserve_grid(c, cells + cells / 2);
    if (rc) return rc;
  }
  GridView g = grid_view(c);
  HIP_RET(hipMemsetAsync(c.g_cursor, 0, (size_t)cells * sizeof(int32_t), stream));
  grid_count_kernel<<<(n + 255) / 256, 256, 0, stream>>>(g, c.px, c.py, c.pz, n, c.g_cursor);
  grid_scan_kernel<<<1, 1024, 0, stream>>>(c.g_cursor, c.g_start, c.g_cursor, cells);
  grid_scatter_kernel<<<(n + 255) / 256, 256, 0, stream>>>(g, c.px, c.py, c.pz, n, c.g_cursor, c.g_p);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

}  // namespace gpd
