// C-ABI of libgpd_hip.so (include/gpd_hip.h): many clouds per call — gpd_hip_detect_batch (two clouds in flight on the
// context's two lanes), its fan-out over several contexts, and one cloud sharded by sample range over several contexts.
// Why the lanes alternate, and the three steps of a fused detect that the schedule interleaves: detect.hip.
#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>

#include "context.h"
#include "outlier_model.h"
#include "sample_model.h"

using namespace gpd;

namespace {

// what a batch job asks of its fused detect (the samples are the caller's business: indices, coordinates or draws)
void fill_job(Job &J, const gpd_detect_job &j) {
  J.mode = 1;
  J.num_selected = j.num_selected;
  J.hands = j.hands;
  J.capacity = j.hands_capacity;
  J.lcg_base = j.lcg_base;
}

// One call of gpd_hip_detect_batch: job i runs on lane i mod kLanes.  run() is the schedule; everything else is a step of it.
struct BatchRun {
  gpd_hip_ctx *ctx;
  gpd_detect_job *jobs;
  int n;
  double t_entry = 0.0;  // host_ms of every job counts from here
  std::vector<Job> J;
  std::vector<char> raw_pending;  // a raw scan between begin_raw and begin_raw_finish
  // a raw scan's samples after Cloud::filterWorkspace (cloud.cpp:225-237): the reference cuts `samples_` with the cloud
  std::vector<std::vector<double>> raw_samples;
  int first_error = GPD_OK;
  std::string first_text;

  BatchRun(gpd_hip_ctx *ctx_, gpd_detect_job *jobs_, int n_)
      : ctx(ctx_), jobs(jobs_), n(n_), J((size_t)n_), raw_pending((size_t)n_, 0), raw_samples((size_t)n_) {}

  Lane &lane(int i) { return ctx->lane[i % kLanes]; }

  int validate() {
    for (int i = 0; i < n; i++) {
      gpd_detect_job &j = jobs[i];
      j.status = GPD_OK;
      j.num_sets = j.num_candidates = j.num_hands = 0;
      j.stage_ms[0] = j.stage_ms[1] = j.stage_ms[2] = 0.f;
      j.allocs = 0;
      for (float &t : j.host_ms) t = 0.f;
      const bool samples_ok = j.raw ? (j.sample_xyz != nullptr || j.num_samples == 0) : j.sample_indices != nullptr;
      if (!j.xyz || (!j.raw && !j.normals) || j.num_points <= 0 || !j.cam_source || j.num_cams < 1 || !j.view_points || !samples_ok ||
          j.num_samples < 0 || !j.hands || j.hands_capacity < 0 || j.num_selected < 0 ||
          (j.raw && !(j.normals_radius > 0.0 && std::isfinite(j.normals_radius) && std::isfinite(j.voxel_size)))) {
        set_error("gpd_hip_detect_batch: job %d has a bad argument", i);
        return GPD_ERR_INVALID;
      }
    }
    return GPD_OK;
  }

  // Both lanes sized once for the largest cloud of the batch before anything is enqueued: a buffer that grows in the
  // middle of the batch is a hipFree + hipMalloc, which waits for the whole device (both lanes).  Points, cameras and
  // samples are known; the candidate-sized buffers (images, LeNet scratch, records) take the upper bound
  // samples x slots, cut to kReserveBudget per lane — a cloud beyond that still grows its lane, and says so in `allocs`.
  int presize() {
    int maxP = 0, maxC = 0, maxS = 0, maxSel = 0, maxDraws = 0;
    int planeP = 0, refineP = 0, refineK = 0;  // raw jobs that carry on past the normals: their largest cloud (before the cut) and k
    int outlierP = 0;                          // raw jobs that remove outliers ahead of the normals
    bool all_selected = n > 0;
    for (int i = 0; i < n; i++) {
      maxP = std::max(maxP, jobs[i].num_points);
      maxC = std::max(maxC, jobs[i].num_cams);
      maxS = std::max(maxS, jobs[i].num_samples);
      // the index route of a raw scan searches at most num_draws samples, and no more than the cloud has points
      if (jobs[i].raw && !jobs[i].sample_xyz && jobs[i].num_draws > 0) {
        maxS = std::max(maxS, std::min(jobs[i].num_draws, jobs[i].num_points));
        maxDraws = std::max(maxDraws, std::min(jobs[i].num_draws, jobs[i].num_points));
        if (jobs[i].sample_above_plane) planeP = std::max(planeP, jobs[i].num_points);
      }
      if (jobs[i].raw && jobs[i].refine_normals_k > 0 && jobs[i].refine_normals_k <= kRefineKCap) {
        refineP = std::max(refineP, jobs[i].num_points);
        refineK = std::max(refineK, jobs[i].refine_normals_k);
      }
      if (jobs[i].raw && jobs[i].outlier_mean_k > 0) outlierP = std::max(outlierP, jobs[i].num_points);
      maxSel = std::max(maxSel, jobs[i].num_selected);
      all_selected = all_selected && jobs[i].num_selected > 0;
    }
    if (maxC > kMaxCams) {
      set_error("gpd_hip_detect_batch: at most %d cameras are supported", kMaxCams);
      return GPD_ERR_INVALID;
    }
    const int before = allocs_now();
    // Best effort: the bound samples x slots is an UPPER bound — sized against what the device has free right now
    // (half of it over the lanes in use, the set bitsets counted), and when the allocation still fails (several contexts
    // on one GPU, a fragmented heap) the batch goes on: the buffers then grow on demand to the real candidate counts, as
    // before round 4 — a failed pre-size is a slower first pass, not a failed batch.
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) {
      (void)hipGetLastError();
      free_b = 2 * kReserveBudget;
    }
    const int lanes_used = std::min(kLanes, n);
    // the draw buffers first and for every lane, not best effort: a few KB, and they must not grow inside the batch — a
    // lane's previous job still has its sample indices in them when the next one draws
    for (int l = 0; l < lanes_used && maxDraws > 0; l++) {
      const int rc = reserve_draws(ctx->lane[l], maxDraws);
      if (rc) return rc;
    }
    const size_t budget = std::min(kReserveBudget, free_b / 2 / (size_t)std::max(lanes_used, 1));
    for (int l = 0; l < lanes_used; l++) {
      Lane &L = ctx->lane[l];
      if (L.search.nn_cap > 16384) {  // lists beyond the LDS sizes, left by a dense cloud of an earlier call: not pre-sized for a whole batch
        const int rcf = search_force_capacity(L.search, 8192);
        if (rcf) return rcf;
      }
      const int cand = candidate_bound(ctx->params, maxS, maxC, budget, &ctx->lenet.net);
      int rc = GPD_OK;
      if (!all_selected) rc = lane_reserve(ctx, L, maxP, maxC, maxS, cand, 0);
      if (!rc && maxSel > 0) rc = lane_reserve(ctx, L, maxP, maxC, maxS, cand, maxSel);
      // the lane's fit / refinement states for the raw scans as they come in (the voxeliser only makes them smaller)
      if (!rc && planeP > 0) rc = plane_reserve(L.plane, planeP);
      if (!rc && refineP > 0) rc = refine_reserve(L.refine, refineP, std::min(refineK, refineP));
      if (!rc && outlierP > 0) rc = outlier_reserve(L.outliers, outlierP, maxC);
      if (rc == GPD_ERR_HIP) {
        (void)hipGetLastError();  // out of memory: clear it, the jobs size their buffers themselves
        break;
      }
      if (rc) return rc;
    }
    if (n > 0) jobs[0].allocs = allocs_now() - before;  // the pre-sizing is booked on the first cloud
    return GPD_OK;
  }

  void fail(int i, int rc) {
    jobs[i].status = rc;
    J[i].live = false;
    // a job that fails after its uploads were enqueued leaves async copies out of the lane's pinned staging in flight;
    // the next job of the lane rewrites (or frees) that staging, so they have to land first
    (void)hipStreamSynchronize(lane(i).stream);
    if (!first_error) {
      first_error = rc;
      first_text = error_text();
    }
  }

  void begin(int i) {
    gpd_detect_job &j = jobs[i];
    if (j.raw) return begin_raw(i);
    Lane &L = lane(i);
    const int allocs0 = allocs_now();
    int rc = check_samples("gpd_hip_detect_batch", j.sample_indices, nullptr, j.num_samples, j.num_points);
    if (!rc) rc = cloud_upload(L.cloud, j.xyz, j.normals, j.num_points, j.cam_source, j.num_cams, j.view_points, L.stream, /*sync=*/false);
    if (rc) return fail(i, rc);
    J[i].sample_idx = j.sample_indices;
    J[i].S = j.num_samples;
    fill_job(J[i], j);
    rc = job_begin(ctx, L, J[i]);
    j.allocs += allocs_now() - allocs0;
    j.host_ms[0] = (float)(now_ms() - t_entry);
    if (rc) fail(i, rc);
  }

  // a RAW scan's first half: upload, workspace cut, voxel keys, the keys on their way to the host — nothing waits
  void begin_raw(int i) {
    gpd_detect_job &j = jobs[i];
    Lane &L = lane(i);
    const int allocs0 = allocs_now();
    j.num_points_processed = 0;
    j.num_samples_processed = 0;
    j.refine_passes = j.refine_num_nan = j.plane_num_above = j.plane_iterations = 0;
    for (float &t : j.preprocess_ms) t = 0.f;
    j.num_outliers = 0;
    j.outlier_ms = 0.f;
    const double t_begin = now_ms();
    int rc = check_samples("gpd_hip_detect_batch", nullptr, j.sample_xyz, j.num_samples, j.num_points);
    if (!rc && (j.refine_normals_k < 0 || j.num_draws < 0 || (j.num_draws != 0 && j.sample_xyz))) {
      set_error("gpd_hip_detect_batch: cloud %d: %s", i,
                j.refine_normals_k < 0 ? "refine_normals_k is negative"
                : j.num_draws < 0     ? "num_draws is negative"
                                      : "num_draws and sample_xyz are both given (draw sample indices or pass coordinates)");
      rc = GPD_ERR_INVALID;
    }
    if (!rc && j.refine_normals_k > kRefineKCap) {
      set_error("gpd_hip_detect_batch: cloud %d: refine_normals_k = %d, the capacity is %d", i, j.refine_normals_k, kRefineKCap);
      rc = GPD_ERR_CAPACITY;
    }
    if (!rc && j.outlier_mean_k != 0) {
      const int why = outlier::refusal(j.outlier_mean_k + 1, j.outlier_mean_k, j.outlier_stddev_mult);  // (the cloud's size: once it is voxelised)
      if (why) {
        set_error("gpd_hip_detect_batch: cloud %d: outlier_mean_k = %d, outlier_stddev_mult = %g: %s", i, j.outlier_mean_k, j.outlier_stddev_mult,
                  why == 2 ? "the capacity is 255" : "mean_k must be positive and the multiplier finite");
        rc = why == 2 ? GPD_ERR_CAPACITY : GPD_ERR_INVALID;
      }
    }
    if (!rc && j.workspace) {
      // strict double comparisons on both sides, sample by sample, order kept (cloud.cpp:229-233): a sample outside the cut would
      // still find neighbours, produce hand sets and shift every later set's shadow LCG offset away from the reference's
      const double *w = j.workspace;
      std::vector<double> &keep = raw_samples[(size_t)i];
      keep.reserve((size_t)j.num_samples * 3);
      for (int k = 0; k < j.num_samples; k++) {
        const double *q = j.sample_xyz + 3 * (size_t)k;
        if (q[0] > w[0] && q[0] < w[1] && q[1] > w[2] && q[1] < w[3] && q[2] > w[4] && q[2] < w[5]) keep.insert(keep.end(), q, q + 3);
      }
    }
    // Cloud::removeNans (candidates_generator.cpp:17) is part of preprocessPointCloud: non-finite points are dropped here
    if (!rc) rc = preprocess_begin(L.pre, j.xyz, j.cam_source, j.num_points, j.num_cams, j.workspace, j.voxel_size, L.stream, /*drop_nonfinite=*/true);
    j.allocs += allocs_now() - allocs0;
    j.preprocess_ms[0] = (float)(now_ms() - t_begin);
    if (rc) return fail(i, rc);
    raw_pending[(size_t)i] = 1;
  }

  // ... and its second half, called once the previous cloud's image / LeNet kernels are in the queue: the voxeliser's sequential
  // chain on this host core (beside those kernels), the gather, the cloud built from the device arrays, the normals, the search
  void begin_raw_finish(int i) {
    if (!raw_pending[(size_t)i]) return;
    raw_pending[(size_t)i] = 0;
    gpd_detect_job &j = jobs[i];
    Lane &L = lane(i);
    const int allocs0 = allocs_now();
    double t0 = now_ms();
    int rc = preprocess_finish(L.pre, L.stream);
    if (!rc && L.pre.M < 1) {
      set_error("gpd_hip_detect_batch: cloud %d: no point is left after the workspace cut", i);
      rc = GPD_ERR_INVALID;
    }
    if (!rc) rc = cloud_from_device(L.cloud, L.pre.d_out_xyz, L.pre.d_out_cam, L.pre.M, j.num_cams, j.view_points, L.stream);
    j.preprocess_ms[0] += (float)(now_ms() - t0);
    // removeStatisticalOutliers, where the cloud has a grid and nothing has read it yet: the kept points replace the lane's cloud
    if (!rc && j.outlier_mean_k > 0) {
      t0 = now_ms();
      if (L.cloud.num_points < j.outlier_mean_k + 1) {
        set_error("gpd_hip_detect_batch: cloud %d: outlier_mean_k = %d needs %d points, %d are left after the voxeliser", i, j.outlier_mean_k,
                  j.outlier_mean_k + 1, L.cloud.num_points);
        rc = GPD_ERR_INVALID;
      } else {
        int kept = 0;
        double stats[3];
        rc = outlier_run(L.outliers, L.cloud, j.outlier_mean_k, j.outlier_stddev_mult, /*carry_normals=*/false, nullptr, &kept, stats, nullptr,
                         nullptr, L.stream);
        if (!rc) j.num_outliers = L.pre.M - kept;
      }
      j.outlier_ms = (float)(now_ms() - t0);
    }
    t0 = now_ms();
    if (!rc) rc = normals_run(L.cloud, j.normals_radius, nullptr, L.stream);
    j.preprocess_ms[1] = (float)(now_ms() - t0);
    // the rest of preprocessPointCloud (candidates_generator.cpp:28-36), resident: nothing cloud-sized comes back.
    // refineNormals replaces the lane cloud's normals and bumps its generation before the search below takes it
    if (!rc && j.refine_normals_k > 0) {
      t0 = now_ms();
      rc = refine_run(L.refine, L.cloud, j.refine_normals_k, 15, 1e-5f, nullptr, &j.refine_passes, nullptr, &j.refine_num_nan, nullptr, L.stream);
      j.preprocess_ms[2] = (float)(now_ms() - t0);
    }
    const bool index_route = !j.sample_xyz && j.num_draws > 0;
    if (!rc && index_route) {
      rc = draw_samples(i);
    } else {
      J[i].sample_xyz = j.workspace ? raw_samples[(size_t)i].data() : j.sample_xyz;
      J[i].S = j.workspace ? (int)(raw_samples[(size_t)i].size() / 3) : j.num_samples;
    }
    if (rc) {
      j.allocs += allocs_now() - allocs0;
      return fail(i, rc);
    }
    j.num_points_processed = L.cloud.num_points;
    J[i].sample_idx = nullptr;
    j.num_samples_processed = J[i].S;
    fill_job(J[i], j);
    rc = job_begin(ctx, L, J[i]);
    if (!rc && J[i].resident && j.samples_out && J[i].S > 0) {
      // the sample indices searched, behind the search in stream order; end(i) hands them over.  A half of the pinned
      // buffer per job of the lane in flight: this lane's previous job is collected only after this point
      const hipError_t e = hipMemcpyAsync(samples_back(i), L.search.d_sample_idx, (size_t)J[i].S * sizeof(int32_t), hipMemcpyDeviceToHost, L.stream);
      if (e != hipSuccess) {
        set_error("gpd_hip_detect_batch: cloud %d: the sample indices could not be copied back: %s", i, hipGetErrorString(e));
        rc = GPD_ERR_HIP;
      }
    }
    j.allocs += allocs_now() - allocs0;
    j.host_ms[0] = (float)(now_ms() - t_entry);
    if (rc) fail(i, rc);
  }

  // the index route of a raw scan (begin_raw_finish): sampleAbovePlane when asked for, then Cloud::subsample's draw positions
  // on the host and their upload; the search gathers its sample indices from them on the device
  int draw_samples(int i) {
    gpd_detect_job &j = jobs[i];
    Lane &L = lane(i);
    int rc = GPD_OK;
    const int M = L.cloud.num_points;  // (the voxelised cloud, less the outliers when they were removed)
    int above = 0;
    if (j.sample_above_plane) {
      const double t0 = now_ms();
      float coeffs[4];
      int inliers = 0;
      rc = plane_fit_run(L.plane, L.cloud, 0.01, 50, 0.99, 1, nullptr, &above, coeffs, &inliers, &j.plane_iterations, L.stream);
      j.preprocess_ms[3] = (float)(now_ms() - t0);
      if (rc) above = 0;
      j.plane_num_above = above;
    }
    // Cloud::subsample: the positions come from a count alone (the list's, or the cloud's when there is none — no fit
    // asked for, or "plane fit failed": the reference then uses the entire point cloud), the indices never leave the device
    std::vector<int32_t> pos;
    if (!rc) {
      if (above > 0)
        sample::with_repetition(above, j.num_draws, j.sample_seed, pos);
      else
        sample::distinct(M, j.num_draws, j.sample_seed, pos);
      if ((int)pos.size() > L.draw_cap) {  // cannot happen: pos.size() <= min(num_draws, num_points), which sized the lanes
        set_error("gpd_hip_detect_batch: cloud %d: %d draws, the lane holds %d", i, (int)pos.size(), L.draw_cap);
        rc = GPD_ERR_STATE;
      }
    }
    if (!rc) {
      std::memcpy(L.h_pos, pos.data(), pos.size() * sizeof(int32_t));
      const hipError_t e = hipMemcpyAsync(L.d_pos, L.h_pos, pos.size() * sizeof(int32_t), hipMemcpyHostToDevice, L.stream);
      if (e != hipSuccess) {
        set_error("gpd_hip_detect_batch: cloud %d: the draw positions could not be uploaded: %s", i, hipGetErrorString(e));
        rc = GPD_ERR_HIP;
      }
    }
    J[i].resident = true;
    J[i].gather.d_list = above > 0 ? L.plane.d_idx : nullptr;
    J[i].gather.list_size = above;
    J[i].gather.d_pos = L.d_pos;
    J[i].sample_xyz = nullptr;
    J[i].S = (int)pos.size();
    return rc;
  }

  // where job i's searched sample indices land (samples_out): the pinned draw buffer's second and third part, one per job
  // of the lane in flight
  int32_t *samples_back(int i) { return lane(i).h_pos + (size_t)lane(i).draw_cap * (1 + ((i / kLanes) & 1)); }

  void middle(int i) {
    if (jobs[i].status != GPD_OK) return;
    const int allocs0 = allocs_now();
    const int rc = job_middle(ctx, lane(i), J[i]);
    jobs[i].allocs += allocs_now() - allocs0;
    jobs[i].host_ms[1] = (float)(J[i].t_plan_ms - t_entry);
    jobs[i].host_ms[2] = (float)(now_ms() - t_entry);
    if (rc) fail(i, rc);
  }

  void end(int i) {
    Lane &L = lane(i);
    const int rc = job_end(ctx, L, J[i]);
    jobs[i].host_ms[4] = (float)(now_ms() - t_entry);
    jobs[i].host_ms[3] = jobs[i].host_ms[4] - (float)J[i].copy_ms;
    if (rc) return fail(i, rc);
    jobs[i].num_sets = J[i].num_sets;
    jobs[i].num_candidates = J[i].num_candidates;
    jobs[i].num_hands = J[i].num_hands;
    jobs[i].lcg_draws = J[i].lcg_draws;
    if (jobs[i].status == GPD_OK && J[i].resident && jobs[i].samples_out && J[i].S > 0)
      std::memcpy(jobs[i].samples_out, samples_back(i), (size_t)J[i].S * sizeof(int32_t));
    for (int k = 0; k < 3; k++) jobs[i].stage_ms[k] = L.stage_ms[k];
  }

  // cloud i+1's upload + search are enqueued (other lane's buffers) before the host waits for cloud i's plan;
  // cloud i-1's results are collected after cloud i's image / LeNet kernels are in the queue
  // (stream order keeps cloud i+1's search behind the image / LeNet kernels of cloud i-1, whose buffers it reuses; of
  //  the pinned host buffers, begin touches the cloud / summary staging only, which job i-1 is done with since its
  //  own middle step)
  void run() {
    if (n > 0) {
      begin(0);
      begin_raw_finish(0);
    }
    for (int i = 0; i < n; i++) {
      if (i + 1 < n) begin(i + 1);
      middle(i);
      if (i + 1 < n) begin_raw_finish(i + 1);  // (a raw scan: its host-side chain runs beside cloud i's image / LeNet kernels)
      if (i >= 1) end(i - 1);
    }
    if (n > 0) end(n - 1);
  }
};

}  // namespace

extern "C" {

int gpd_hip_detect_batch(gpd_hip_ctx *ctx, gpd_detect_job *jobs, int num_jobs) {
  StageRange range_("gpd:detect_batch");
  int rc = refuse("gpd_hip_detect_batch", ctx, num_jobs >= 0 && (num_jobs == 0 || jobs), {Need::LeNet});
  if (rc) return rc;
  HIP_RET(hipSetDevice(ctx->device));
  BatchRun b(ctx, jobs, num_jobs);
  rc = b.validate();
  if (rc) return rc;
  for (int l = 1; l < kLanes; l++) {
    rc = lane_init(ctx->lane[l]);
    if (rc) return rc;
  }
  b.t_entry = now_ms();
  rc = b.presize();
  if (rc) return rc;
  ctx->in_batch = true;
  b.run();
  ctx->in_batch = false;
  for (int l = 0; l < kLanes; l++) ctx->lane[l].images.side_stream = true;
  if (b.first_error) error_text_set(b.first_text.c_str());
  return b.first_error;
}

// The CPUs of the NUMA node a device hangs off (sysfs: the PCI function's numa_node, the node's cpulist).  Eight
// processes / threads feeding eight GPUs from a two-socket host is SURVEY 8e's expected limiter: a feeding thread that
// runs on the far socket pays the inter-socket hop on every staging copy and every doorbell.
static int device_numa_cpus(int device, cpu_set_t *set) {
  char bdf[64] = "";
  if (hipDeviceGetPCIBusId(bdf, sizeof(bdf), device) != hipSuccess) return -1;
  for (char *c = bdf; *c; c++) *c = (char)std::tolower((unsigned char)*c);
  char path[160];
  snprintf(path, sizeof(path), "/sys/bus/pci/devices/%s/numa_node", bdf);
  FILE *f = fopen(path, "r");
  if (!f) return -1;
  int node = -1;
  if (fscanf(f, "%d", &node) != 1) node = -1;
  fclose(f);
  if (node < 0) return -1;  // a single-node host (or a VM that hides the topology): nothing to bind to
  snprintf(path, sizeof(path), "/sys/devices/system/node/node%d/cpulist", node);
  f = fopen(path, "r");
  if (!f) return -1;
  CPU_ZERO(set);
  int a = 0, b = 0, n = 0;
  for (;;) {  // "0-63,128-191"
    if (fscanf(f, "%d", &a) != 1) break;
    b = a;
    int c = fgetc(f);
    if (c == '-') {
      if (fscanf(f, "%d", &b) != 1) break;
      c = fgetc(f);
    }
    for (int k = a; k <= b && k < CPU_SETSIZE; k++) {
      CPU_SET(k, set);
      n++;
    }
    if (c != ',') break;
  }
  fclose(f);
  return n > 0 ? node : -1;
}

int gpd_hip_bind_host_thread(int device, int *num_cpus) {
  if (num_cpus) *num_cpus = 0;
  cpu_set_t set;
  const int node = device_numa_cpus(device, &set);
  if (node < 0) return -1;
  // only within what the process is allowed to use (a container's cpuset)
  cpu_set_t allowed, both;
  if (pthread_getaffinity_np(pthread_self(), sizeof(allowed), &allowed) != 0) return -1;
  CPU_AND(&both, &set, &allowed);
  if (CPU_COUNT(&both) == 0) return -1;
  if (pthread_setaffinity_np(pthread_self(), sizeof(both), &both) != 0) return -1;
  if (num_cpus) *num_cpus = CPU_COUNT(&both);
  return node;
}

}  // extern "C"

// entry c of a context list: there, and not listed before
static int check_context(const char *who, gpd_hip_ctx *const *ctxs, int c) {
  if (!ctxs[c]) {
    set_error("%s: context %d is null", who, c);
    return GPD_ERR_INVALID;
  }
  for (int d = 0; d < c; d++)
    if (ctxs[d] == ctxs[c]) {
      set_error("%s: context %d is listed twice (a context serves one thread)", who, c);
      return GPD_ERR_INVALID;
    }
  return GPD_OK;
}

// One host thread per context that has not failed yet, bound to its device's NUMA node (the worker feeds ONE device: it
// stays on that device's socket): body(c) -> rc.  A failure is left in rcs[c] with its text: the error text is per thread.
template <typename Body>
static void for_each_context(gpd_hip_ctx *const *ctxs, int n, std::vector<int> &rcs, std::vector<std::string> &texts, Body body) {
  std::vector<std::thread> threads;
  for (int c = 0; c < n; c++)
    threads.emplace_back([&, c]() {
      if (rcs[(size_t)c]) return;
      (void)gpd_hip_bind_host_thread(ctxs[c]->device, nullptr);
      const int rc = body(c);
      if (rc) {
        rcs[(size_t)c] = rc;
        texts[(size_t)c] = error_text();
      }
    });
  for (auto &t : threads) t.join();
}

extern "C" {

// One host thread per context (one context per GPU; more than one on a device is allowed), job i -> context i mod
// num_ctx: the in-process form of "independent clouds shard over the GPUs of a node" (the reference's unit
// of work is one detect_grasps run per cloud, src/detect_grasps.cpp:20-86).  No device talks to another.
int gpd_hip_detect_batch_multi(gpd_hip_ctx *const *ctxs, int num_ctx, gpd_detect_job *jobs, int num_jobs) {
  if (!ctxs || num_ctx < 1 || num_jobs < 0 || (num_jobs > 0 && !jobs)) {
    set_error("gpd_hip_detect_batch_multi: bad argument");
    return GPD_ERR_INVALID;
  }
  for (int c = 0; c < num_ctx; c++) {
    const int rc = check_context("gpd_hip_detect_batch_multi", ctxs, c);
    if (rc) return rc;
  }
  std::vector<std::vector<gpd_detect_job>> mine((size_t)num_ctx);
  for (int i = 0; i < num_jobs; i++) mine[(size_t)(i % num_ctx)].push_back(jobs[i]);
  std::vector<int> rcs((size_t)num_ctx, GPD_OK);
  std::vector<std::string> texts((size_t)num_ctx);
  for_each_context(ctxs, num_ctx, rcs, texts,
                   [&](int c) { return gpd_hip_detect_batch(ctxs[c], mine[(size_t)c].data(), (int)mine[(size_t)c].size()); });
  for (int i = 0; i < num_jobs; i++) jobs[i] = mine[(size_t)(i % num_ctx)][(size_t)(i / num_ctx)];
  for (int c = 0; c < num_ctx; c++)
    if (rcs[(size_t)c]) {
      set_error("context %d: %s", c, texts[(size_t)c].c_str());
      return rcs[(size_t)c];
    }
  return GPD_OK;
}

// ONE cloud, its samples cut into contiguous ranges, one range per context (sample-range sharding with the cloud
// replicated; BASELINE configs[3] across GPUs).  The reference draws every shadow point of a cloud from ONE LCG stream
// (hand_set.cpp:268-283), hand set after hand set, so range g has to start where the ranges before it stopped:
//   phase 1  every context uploads the cloud and searches + plans its range; the plan summary carries the range's draw total
//   host     exclusive scan of the G totals (G numbers: still no collective)
//   phase 2  images + LeNet + records with lcg_base = the draws before the range
// The concatenated results are byte for byte those of one gpd_hip_detect_select over all samples (tests/test_gpu_resident.py).
int gpd_hip_detect_sharded(gpd_hip_ctx *const *ctxs, int num_ctx, gpd_detect_job *shards) {
  if (!ctxs || num_ctx < 1 || !shards) {
    set_error("gpd_hip_detect_sharded: bad argument");
    return GPD_ERR_INVALID;
  }
  for (int c = 0; c < num_ctx; c++) {
    const int rc = check_context("gpd_hip_detect_sharded", ctxs, c);
    if (rc) return rc;
    const gpd_detect_job &j = shards[c];
    if (!j.xyz || !j.normals || !j.cam_source || !j.view_points || (j.num_samples > 0 && (!j.sample_indices || !j.hands)) || j.num_points < 1 ||
        j.num_cams < 1 || j.num_samples < 0 || j.hands_capacity < 0 || j.num_selected != 0) {
      set_error("gpd_hip_detect_sharded: shard %d: bad argument (selectGrasps over a sharded cloud is the caller's: num_selected must be 0)", c);
      return GPD_ERR_INVALID;
    }
    if (!ctxs[c]->lenet.channels) {
      set_error("gpd_hip_detect_sharded: context %d: LeNet weights not set", c);
      return GPD_ERR_STATE;
    }
  }
  std::vector<Job> J((size_t)num_ctx);
  std::vector<int> rcs((size_t)num_ctx, GPD_OK);
  std::vector<std::string> texts((size_t)num_ctx);
  // a phase on every context that is still good, on its device; a context that fails is drained (lane 0)
  auto phase = [&](auto &&body) {
    for_each_context(ctxs, num_ctx, rcs, texts, [&](int c) {
      int rc = hipSetDevice(ctxs[c]->device) == hipSuccess ? GPD_OK : GPD_ERR_HIP;
      if (!rc) rc = body(c);
      if (rc) (void)hipStreamSynchronize(ctxs[c]->lane[0].stream);
      return rc;
    });
  };
  phase([&](int c) -> int {
    gpd_hip_ctx *ctx = ctxs[c];
    gpd_detect_job &j = shards[c];
    j.status = GPD_OK;
    j.num_sets = j.num_candidates = j.num_hands = 0;
    int rc = lane_init(ctx->lane[0]);
    if (rc) return rc;
    Lane &L = ctx->lane[0];
    rc = check_samples("gpd_hip_detect_sharded", j.sample_indices, nullptr, j.num_samples, j.num_points);
    if (!rc) rc = cloud_upload(L.cloud, j.xyz, j.normals, j.num_points, j.cam_source, j.num_cams, j.view_points, L.stream, /*sync=*/false);
    if (rc) return rc;
    Job &jb = J[(size_t)c];
    jb.sample_idx = j.sample_indices;
    jb.S = j.num_samples;
    fill_job(jb, j);
    jb.num_selected = 0;
    jb.lcg_base = 0;  // the scan below sets it
    rc = job_begin(ctx, L, jb);
    if (!rc) rc = job_wait_plan(ctx, L, jb);
    return rc;
  });
  unsigned long long base = 0;
  for (int c = 0; c < num_ctx; c++) {
    J[(size_t)c].lcg_base = shards[c].lcg_base = base;
    shards[c].lcg_draws = J[(size_t)c].lcg_draws;
    base += J[(size_t)c].lcg_draws;
  }
  phase([&](int c) -> int {
    gpd_hip_ctx *ctx = ctxs[c];
    Lane &L = ctx->lane[0];
    Job &jb = J[(size_t)c];
    int rc = job_enqueue(ctx, L, jb);
    if (!rc) rc = job_end(ctx, L, jb);
    if (rc) return rc;
    shards[c].num_sets = jb.num_sets;
    shards[c].num_candidates = jb.num_candidates;
    shards[c].num_hands = jb.num_hands;
    for (int k = 0; k < 3; k++) shards[c].stage_ms[k] = L.stage_ms[k];
    return GPD_OK;
  });
  for (int c = 0; c < num_ctx; c++)
    if (rcs[(size_t)c]) {
      shards[c].status = rcs[(size_t)c];
      set_error("context %d: %s", c, texts[(size_t)c].c_str());
      return rcs[(size_t)c];
    }
  // a record's set_index counts the hand sets of the whole cloud: the sets of the ranges before are added
  int sets_before = 0;
  for (int c = 0; c < num_ctx; c++) {
    if (sets_before)
      for (int i = 0; i < shards[c].num_hands; i++) shards[c].hands[i].set_index += sets_before;
    sets_before += shards[c].num_sets;
  }
  return GPD_OK;
}

}  // extern "C"
