// Internal declarations shared by the HIP translation units of libgpd_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>

#include <vector>

#ifdef GPD_PROFILING
#include <cstdlib>
#include <rocprofiler-sdk-roctx/roctx.h>
#endif

#include "../../include/gpd_hip.h"

namespace gpd {

constexpr int kImg = 60;            // image_size (eigen_classifier.cpp:12)
constexpr int kPix = kImg * kImg;   // 3600
constexpr int kFc1In = 7200;        // 50 * 12 * 12
constexpr int kFc1Out = 500;
// split path: where ip1 leaves the partial sum of (image m, K quarter kq, unit u) for ip2's kernel (floats)
__host__ __device__ inline size_t fc1p_index(int m, int kq, int u) { return (((size_t)(m >> 5) * 4 + kq) * kFc1Out + u) * 32 + (m & 31); }
constexpr int kLenetXld = 7296;     // row length of the split path's flat bf16 planes: 7200 + 96 zeros = 4 K quarters x 57 steps of 32 (lenet_fast.hip)

// ---- LeNet (lenet.hip) ----------------------------------------------------
// operand tables of the split path (lenet_fast.hip): conv1 as four int8 digit planes of 32-bit fixed-point weights, conv2 / ip1
// as three bf16 pieces per weight, all in the kernels' MFMA fragment layouts
struct LeNetFast {
  uint4 *c1a = nullptr;            // conv1 A fragments [7 k-steps][5 row tiles][64 lanes] x 16 int8
  double *c1corr = nullptr;        // [20] 128 * sum of the filter's fixed-point weights (the x - 128 shift of the inputs)
  int *c1shift = nullptr;          // [20] fixed-point position s of the filter: value = integer * 2^-s
  uint4 *c2b = nullptr;            // conv2 fragments [4 slots][3 pieces][16 k-steps][64 lanes] x 8 bf16 (slot 3: the A fragments of filters 48, 49)
  unsigned short *f1wt = nullptr;  // ip1's weights as bf16 pieces, blocked [32 unit blocks][228 k steps][3 pieces][16 units][32 k] (lenet_fast.hip f3_blocked)
};
void lenet_fast_free(LeNetFast &f);
void lenet_fast_unblock_x(const unsigned short *blocked, int n, unsigned short *planes);  // test hook: [3][n][7200] from the blocked X
hipError_t lenet_fast_prepare(LeNetFast &f, int channels, const float *c1w, const float *c2w, const float *f1w);

// ---- the shape-general route (lenet_net.hip): any gpd_lenet_shape within the limits of gpd_hip_lenet_shape_check ----
// A network installed by gpd_hip_set_lenet_net, in the kernels' layouts: conv weights k-major with the filters padded to
// whole tiles of 32 and the k padded to an even count ([K + K % 2][Fpad], zeros in the padding: the tail of a chain);
// dense weights k-major with the k padded to whole steps of 32 and the units to whole tiles of 128.
struct LeNetNet {
  bool active = false;  // every scoring call of the context takes this route (lenet_forward's first branch)
  gpd_lenet_shape shape = {0, 0, 0, 0, 0};
  float *c1wt = nullptr, *c1b = nullptr, *c2wt = nullptr, *c2b = nullptr;
  float *f1w = nullptr, *f1b = nullptr, *f2w = nullptr, *f2b = nullptr;  // f2*: null when shape.fc2_out == 0
  float *lw = nullptr, *lb = nullptr;                                    // the 2-logit layer [H][2], [2]
  int f1pad = 0, f2pad = 0;          // conv filters in whole tiles of 32
  int u1pad = 0, u2pad = 0;          // dense units in whole tiles of 128
  int cb1 = 0, cb2 = 0;              // input channels a workgroup stages at a time (at most 8; even when there are several chunks)
  int aoff1 = 0, aoff2 = 0;          // where the weight tile starts in a conv launch's dynamic LDS (behind the input rows)
  int lds1 = 0, lds2 = 0, lds_max = 0;  // dynamic LDS of the two conv launches; the largest LDS of any kernel of the route
  long long scratch_per_image = 0;   // bytes
  long long macs_per_image = 0;
  int chunk = 0;                     // images per pass
  // GPD_LENET_NET_SPLIT (lenet_net_split.hip).  `mode` is the arithmetic in force: scratch_per_image, chunk and lds_max above are
  // its values (lenet_net_apply_mode); the chain's tables stay as they are, the pieces below exist in split mode only.
  int mode = 0;
  uint4 *s_c1 = nullptr, *s_c2 = nullptr;  // conv weights as B fragments [chunk of 8 channels][filter tile of 16][7 k-steps][3 pieces][64 lanes] x 8 bf16
  uint4 *s_f1 = nullptr, *s_f2 = nullptr;  // dense weights as B fragments [unit tile of 16][k-steps][3 pieces][64 lanes] x 8 bf16
  int s_ft1 = 0, s_ft2 = 0;                // filter tiles the conv tables hold per chunk (an even count)
  int s_k1 = 0, s_k2 = 0;                  // fc1's and fc2's K, padded to whole k-steps of 32 (row length of the bf16 planes)
};
struct LeNetNetScratch {
  int capacity = 0;  // images
  bool ran = false;  // the lane's last scoring call took the general route (gpd_hip_lenet_net_debug)
  float *pool1 = nullptr;  // [cap][F1][28][28]
  float *pool2 = nullptr;  // [cap][144][F2]: pixel-major, fc1's k order
  float *h1 = nullptr, *h2 = nullptr;  // [cap][ld]: ld = the units rounded up to a multiple of 4 (16-byte row reads)
  float *logits = nullptr;             // [cap][2]
  // GPD_LENET_NET_SPLIT: activations as three bf16 planes, in the layout the consuming loader takes (lenet_net_split.hip).
  // h1 / h2 above hold the LAST hidden layer as f32 for the logit chains; pool1 and pool2 stay null.
  int mode = 0;                        // the mode the buffers were sized for
  unsigned short *p1s = nullptr;       // [cap][F1 / 8 chunks][3][784][8]
  unsigned short *xs = nullptr;        // [cap][3][K1pad], k = pixel * round_up(F2, 8) + channel
  unsigned short *h1s = nullptr;       // [cap][3][K2pad] (networks with fc2; the padding zeroed at allocation)
};
void lenet_net_free(LeNetNet &net);
void lenet_net_scratch_free(LeNetNetScratch &s);
// the scratch of `net` for passes of up to n images (cut to net.chunk, a quarter of slack); a growth is booked (note_alloc).
// lenet_net_forward calls it per pass, lane_reserve ahead of the first cloud.  gpd_hip_set_lenet_net frees the scratch of every
// lane when it installs a network: a reservation made before the install does not outlive it.
hipError_t lenet_net_scratch_reserve(const LeNetNet &net, LeNetNetScratch &s, int n);
// gpd_hip_set_lenet_net_mode met gpd_hip_set_lenet_net (whichever came second): builds or frees the weight piece tables and sets
// net.mode, scratch_per_image, chunk and lds_max to the values of `mode`.  The caller has freed the lanes' general-route scratch.
int lenet_net_apply_mode(LeNetNet &net, int mode);
// lenet_net_split.hip
struct LeNetWeights;
struct LeNetScratch;
void lenet_net_split_free(LeNetNet &net);
int lenet_net_split_prepare(LeNetNet &net);  // the piece tables from the chain's device tables
long long lenet_net_split_scratch_per_image(const gpd_lenet_shape &sh);
int lenet_net_split_lds();
hipError_t lenet_net_split_scratch_alloc(const LeNetNet &net, LeNetNetScratch &s, size_t cap);
hipError_t lenet_net_split_forward(const LeNetWeights &w, LeNetNetScratch &t, const uint8_t *img, int m, float *d_scores, hipStream_t stream,
                                   hipEvent_t *kernel_events);
int lenet_net_split_debug(const LeNetNet &net, const LeNetNetScratch &t, int which, int n, float *out);  // the stream is idle
// the two logits and the score of m images from the last hidden layer (lenet_net.hip: one kernel for both modes)
void lenet_net_logits(const LeNetNet &net, const float *hid, int ldh, int K, float *logits, float *d_scores, int m, hipStream_t stream);

struct LeNetWeights {
  int channels = 0;
  int mode = GPD_LENET_SPLIT;  // gpd_hip_set_lenet_mode
  bool conv_relu = false;      // gpd_hip_set_lenet_conv_relu: ReLU on pool1 and pool2 (the network of the reference's PyTorch scripts)
  int net_mode = GPD_LENET_NET_CHAIN;  // gpd_hip_set_lenet_net_mode: outlives installs and gpd_hip_set_lenet_weights (net.mode: what is in force)
  LeNetNet net;                // gpd_hip_set_lenet_net
  LeNetFast fast;
  float *c1w = nullptr, *c1b = nullptr, *c2w = nullptr, *c2b = nullptr;
  float *c1wp = nullptr;  // conv1 weights padded to [20][C][28] (25 taps + 3 zeros): 16-byte rows for the LDS table
  float *c2wt = nullptr;  // conv2 weights k-major [K][F] for the implicit-GEMM A operand
  float *f1w = nullptr, *f1b = nullptr, *f2w = nullptr, *f2b = nullptr;
};

struct LeNetScratch {
  int capacity = 0;        // images per chunk
  float *pool1 = nullptr;  // f32 chain: [cap][20][784], planes in conv1's chunk order (whole-line stores, lenet.hip P1_PLANE);
                           // split path: [cap][784][20], pixel-major
  float *flat = nullptr;   // [cap][7200]  (pixel-major, channel-minor)
  unsigned short *xs = nullptr;  // split path: flat as three bf16 pieces, blocked like ip1's weights [cap / 16][228][3][16][32] (k >= 7200: zeros, written once at allocation)
  float *fc1t = nullptr;   // [500][cap]   (transposed, ReLU applied)
  float *fc1p = nullptr;   // split path: ip1's partial sums over the four K quarters, blocked [cap / 32][4][500][32] (fc1p_index)
  int num_cus = 0;         // compute units of the context's device (grid of the persistent conv2)
  unsigned long long *c1_stats = nullptr;  // device: [0] (chunk, channel) pairs conv1 executed, [1] pairs it looked at — summed
                                           // over its launches since the last gpd_hip_conv1_stats(reset); [2] != 0: a launch gave up
                                           // waiting for an image slot (its scores are invalid: lenet_check)
  LeNetNetScratch net;     // the general route's own buffers (lenet_net.hip)
};
// lenet_forward's branch for a context whose network came through gpd_hip_set_lenet_net
hipError_t lenet_net_forward(const LeNetWeights &w, LeNetScratch &s, const uint8_t *d_images, int n, float *d_scores,
                             hipStream_t stream, hipEvent_t *kernel_events);

// Scores n images (device pointer, planar u8 [n][C][3600]) into d_scores (device). Async on stream.
hipError_t lenet_forward(const LeNetWeights &w, LeNetScratch &s, const uint8_t *d_images, int n, float *d_scores,
                         hipStream_t stream, hipEvent_t *kernel_events = nullptr);
// the split path's three matrix kernels (lenet_fast.hip); `queue`: two zeroed image counters (conv1's, conv2's)
hipError_t lenet_forward_fast(const LeNetWeights &w, LeNetScratch &s, const uint8_t *img, int m, float *d_scores, hipStream_t stream,
                              hipEvent_t *kernel_events, int *queue);
hipError_t lenet_scratch_reserve(LeNetScratch &s, int n);
// after the stream was synchronised: GPD_ERR_HIP (and the error word cleared) when a conv1 launch gave up on its slot protocol
int lenet_check(LeNetScratch &s);
// the launch error word lenet_check reads, for a caller that copies its low four bytes out behind a pass (non-zero: call lenet_check)
inline const void *lenet_fault_word(const LeNetScratch &s) { return s.c1_stats + 2; }
void lenet_scratch_free(LeNetScratch &s);

void set_error(const char *fmt, ...);
#define HIP_RET(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) {                                                                 \
      set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return GPD_ERR_HIP;                                                                   \
    }                                                                                       \
  } while (0)
// the device and the first lane's stream of a context (context.hip): what a trainer (train.hip) runs on
void ctx_device_stream(gpd_hip_ctx *ctx, int *device, hipStream_t *stream);
// Growths of device / pinned buffers (hipFree + hipMalloc: a device stall) are counted per host thread; the batch entry
// reports the count per cloud (gpd_detect_job::allocs) so that a pass that was supposed to run on pre-sized lanes can be
// seen to have done so.  The rule of a growth has one text, buffers.h; its helpers book on the `who` they are handed, and
// a group site books once itself.  BOOKED: everything a lane, a cloud, a search, a plan, the image and LeNet buffers, the
// normals, plane, refine, outlier, label and SIS states grow by size.  NOT booked (as found; the helpers take a null `who`, these
// sites use the typed allocate / release alone): gpd_hip_score's staging pair (d_img_in, d_img_planar), the HWC copy of a
// download (d_images_hwc), plan_build's given-set tables, cluster_reserve, the LeNet weight tables, everything of a
// trainer and a trainer group (their pools included), the replay pipe's second buffer, and the fixed-size words a state
// allocates once (h_flags, d_status / d_pts_scratch, the d_meta / h_meta pairs, d_nan / h_nan).  DESIGN §3 has the list.
void note_alloc(const char *where);

// roctx range around a stage of the path (host side: what the stage enqueues); `rocprofv3 --marker-trace --kernel-trace`
// shows them over the kernel timeline (the reference times its stages with omp_get_wtime, grasp_detector.cpp:223-273)
// — in the profiling build only (make prof -> libgpd_hip_prof.so, -DGPD_PROFILING).  The release library links no
// profiler and reads no environment variable: the measurement switches (GPD_*_TIMING, GPD_IMG_SERIAL, GPD_IMG_EXIT,
// GPD_IMG_LDS_PAD, GPD_REPLAY_PIPE, GPD_DETECT_TIMING, GPD_PLAN_TIMING) and the watchdog's fault injector
// (GPD_C1_FAULT) go through prof_env(), which is a constant nullptr there.
#ifdef GPD_PROFILING
struct StageRange {
  explicit StageRange(const char *name) { roctxRangePushA(name); }
  ~StageRange() { roctxRangePop(); }
  StageRange(const StageRange &) = delete;
  StageRange &operator=(const StageRange &) = delete;
};
inline const char *prof_env(const char *name) { return getenv(name); }
#else
struct StageRange {
  explicit StageRange(const char *) {}
  StageRange(const StageRange &) = delete;
  StageRange &operator=(const StageRange &) = delete;
};
inline const char *prof_env(const char *) { return nullptr; }
#endif

// ---- point-cloud preparation (preprocess.hip): workspace cut + the reference's voxeliser ------------------------
struct PreState {
  int capacity = 0, cap_cams = 0;
  float *d_xyz = nullptr, *d_block_lo = nullptr, *d_out_xyz = nullptr;
  int32_t *d_cam = nullptr, *d_block_count = nullptr, *d_block_off = nullptr, *d_src = nullptr, *d_rank = nullptr, *d_out_cam = nullptr,
          *d_out_src = nullptr;
  int4 *d_keys = nullptr;
  void *d_meta = nullptr;
  char *h_pin = nullptr;        // pinned host side of the voxeliser's chain: the voxel keys of every point (16 B), what the walk
                                // decided (rank among the kept points, -1: dropped; 4 B), the counters
  hipEvent_t ev[2] = {nullptr, nullptr};
  hipEvent_t ev_keys = nullptr; // the keys and counters have arrived in h_pin
  int n = 0, num_cams = 0, M = 0;  // the call in flight between preprocess_begin and preprocess_finish; M: points it left on the device
  float cell = 0.f;
};
void preprocess_free(PreState &s);
// the two halves of preprocess_run (gpd_hip_detect_batch on raw scans puts other clouds' work between them): begin enqueues the
// upload, the workspace cut, the voxel keys and their way back to pinned memory; finish waits for them, walks the voxeliser's
// chain on the host and gathers the kept points: s.M of them in s.d_out_xyz [M][3] / s.d_out_cam [cams][M] on the device.
// drop_nonfinite: Cloud::removeNans first (cloud.cpp:154-164: a NaN / Inf point is dropped); without it such a cloud is refused
int preprocess_begin(PreState &s, const float *xyz, const int32_t *cam_source, int n, int num_cams, const double *workspace, float cell,
                     hipStream_t stream, bool drop_nonfinite);
int preprocess_finish(PreState &s, hipStream_t stream);
// workspace: 6 doubles or nullptr; cell <= 0: no voxeliser.  src_out (may be nullptr): input index of every output point.
// ms (may be nullptr): device time of the kernels.
int preprocess_run(PreState &s, const float *xyz, const int32_t *cam_source, int n, int num_cams, const double *workspace, float cell,
                   float *xyz_out, int32_t *cam_out, int32_t *src_out, int *num_out, float *ms, hipStream_t stream);

// ---- Clustering::findClusters on the device (cluster.hip) ---------------------------------------------------------
struct ClusterState {
  int capacity = 0;
  gpd_hand *d_hands = nullptr, *d_out = nullptr;
  double *d_scores = nullptr, *d_res = nullptr, *d_out_scores = nullptr;
  uint8_t *d_used = nullptr;
  int32_t *d_keep = nullptr, *d_out_src = nullptr, *d_num = nullptr;
};
void cluster_free(ClusterState &s);
int cluster_run(ClusterState &s, const gpd_hand *hands, const double *scores, int n, int min_inliers, int remove_inliers, gpd_hand *out,
                double *out_scores, int32_t *out_src, int *num_out, hipStream_t stream);
// the same on n records that are on the device already (gpd_hip_detect_sis), scores = (double)record.score: the clusters are left
// in s.d_out, their number in s.d_num; nothing waits for the device
int cluster_run_resident(ClusterState &s, const gpd_hand *d_hands, int n, int min_inliers, int remove_inliers, hipStream_t stream);

// ---- Cloud (cloud.hip) ------------------------------------------------------
// Device copy of what the path reads from util::Cloud, as SoA for coalesced streaming.
// cameras of a cloud: the kernels carry "which cameras see this neighbourhood" as a 32-bit mask and the view points
// as a kernel argument (768 bytes)
constexpr int kMaxCams = 32;
// largest neighbourhood the search lists per sample (the reference has no limit, hand_search.cpp:178; ours is a matter of
// memory: 44 bytes per list entry and sample).  Beyond 65535 entries hand_eval_kernel walks the full list instead of its
// LDS table, whose neighbour ranks are 16 bits wide.
constexpr int kNnCapMax = (1 << 20) - 1;
// scratch of Cloud::calculateNormals on the device (normals.hip normals_run): per-point neighbour lists in one array
struct NormalsScratch {
  int cap_points = 0;
  long long arena_cap = 0;         // 8-byte units
  int32_t *d_count = nullptr, *d_big = nullptr;
  float4 *d_lists = nullptr;        // [P / 64][1024][64] transposed neighbour lists
  long long *d_big_off = nullptr;
  unsigned long long *d_arena = nullptr, *d_ctl = nullptr;
  float *d_out = nullptr;
  double *d_cent = nullptr;         // [P][3] centroids certified by the list kernel (NaN: walk the chain)
  int last_queued = 0;             // of the last run: points that went through the large-neighbourhood kernel
  int last_points = 0, last_tiles = 0, last_attempts = 0;  // of the last run, for normals_routes: its cloud size, its tiles, 2 when the arena grew
  uint64_t last_generation = 0;    // the cloud's generation the last run left: normals_routes reads the grid of THAT cloud
};
void normals_free(NormalsScratch &s);
struct Cloud {
  int num_points = 0, num_cams = 0, capacity = 0, cap_cams = 0;
  char *h_pin = nullptr;              // pinned staging of the caller's arrays (xyz, normals, cam_source)
  uint64_t generation = 0;            // bumped by every upload
  float *px = nullptr, *py = nullptr, *pz = nullptr;
  float *nx = nullptr, *ny = nullptr, *nz = nullptr;
  int32_t *cam_source = nullptr;      // [num_cams][num_points]
  float *staging = nullptr;           // AoS upload buffer, 6 floats per point
  double view_points[3 * kMaxCams] = {0};
  // uniform grid over the cloud (cells of 2 cm, z fastest): the radius searches visit the cells
  // that overlap the query sphere instead of streaming all P points (replaces the k-d tree of
  // hand_search.cpp:29-31 / image_generator.cpp:37-38; only a candidate filter — the distance
  // test and the (d2, index) order are unchanged)
  float g_lo[3] = {0, 0, 0};
  float g_cell = 0.02f;
  int g_dim[3] = {1, 1, 1};
  int g_cells_cap = 0;
  int32_t *g_start = nullptr;         // [cells + 1]
  int32_t *g_cursor = nullptr;        // [cells] scatter cursors
  float4 *g_p = nullptr;              // [P] the points in cell order: x, y, z and, as bits in w, the original index (one
                                      // 16-byte load per visited point instead of four dword loads)
  float4 *pxyz = nullptr, *pnrm = nullptr;  // [P] AoS copies (x, y, z, 0) / (nx, ny, nz, 0): one load per random access
  NormalsScratch normals;
};
struct GridView {
  float lo[3];
  float cell;
  int dim[3];
  const int32_t *start;
  const float4 *p;  // x, y, z, index bits
};
inline GridView grid_view(const Cloud &c) {
  GridView g;
  for (int i = 0; i < 3; i++) {
    g.lo[i] = c.g_lo[i];
    g.dim[i] = c.g_dim[i];
  }
  g.cell = c.g_cell;
  g.start = c.g_start;
  g.p = c.g_p;
  return g;
}
int cloud_upload(Cloud &c, const float *xyz, const float *normals, int n, const int32_t *cam_source, int num_cams,
                 const double *view_points, hipStream_t stream, bool sync);
int cloud_reserve(Cloud &c, int n, int num_cams);
// the cloud from device arrays (the preprocessing kernels' output): d_xyz [n][3], d_cam [cams][n]; normals zero until normals_run
int cloud_from_device(Cloud &c, const float *d_xyz, const int32_t *d_cam, int n, int num_cams, const double *view_points, hipStream_t stream);
int cloud_reserve_grid(Cloud &c, int cells);
void cloud_free(Cloud &c);
int normals_run(Cloud &c, double radius, float *normals_out, hipStream_t stream);  // normals.hip
// gpd_hip_last_normals_routes on a cloud whose stream has been waited for (count: room for n_room entries, by original index)
int normals_routes(const Cloud &c, int32_t *count, int n_room, long long info[8]);

// ---- Candidate search (search.hip) -----------------------------------------------
struct SearchState {
  int num_samples = 0, capacity_samples = 0;
  int min_samples = 0;                // sample capacity to keep across a change of the list capacity (search_force_capacity)
  uint64_t seen_generation = 0;       // Cloud::generation of the last run: lists beyond the LDS capacities shrink back on a new cloud
  int nn_cap = 0;                     // entries per neighbourhood list: 8192 / 16384 (LDS sorts) or up to kNnCapMax (global-memory sort)
  uint64_t cloud_generation = 0;
  int32_t *d_sample_idx = nullptr;    // [S]
  double *d_sample_xyz = nullptr;     // [S][3] samples given by coordinates (used instead of the indices)
  int32_t *d_counts = nullptr;        // [S][8]: N_hands, N_images, k_frames, total found, seen by camera 0
  int32_t *d_nn_idx = nullptr;        // [S][nn_cap] scratch of the global-memory lists (neighbourhoods beyond the LDS capacities)
  float *d_nn = nullptr;              // [S][6][nn_cap] gathered px,py,pz,nx,ny,nz in that order
  double *d_frames = nullptr;         // [S][12] sample, normal, binormal, curvature
  double *d_centers = nullptr;        // [S][3] mean of the image neighbourhood
  gpd_hand *d_hands = nullptr;        // [S][slots]
  float4 *d_hl = nullptr;             // [S][cap] points that can be in-height for some orientation: x, y, z, rank bits (height_list_kernel)
  uint8_t *d_fvalid = nullptr;        // [S][slots] is_valid after filterGraspsWorkspace (hand_eval_kernel writes it; the
                                      // unfused gpd_hip_images overwrites it with the caller's flags)
  int32_t *d_labels = nullptr;        // [S] reeval_kernel's labels (one hand per sample slot)
  // centre_kernel (serial fp64 chains: a hundred-odd waves, latency-bound) runs on a side stream beside
  // hand_eval_kernel and is joined before anything reads d_centers
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  std::vector<int32_t> h_counts;      // host copy of d_counts (unfused entry points only)
  std::vector<int32_t> h_set_sample;  // set -> sample slot
  std::vector<double> h_samples;      // [S][3] sample coordinates (to validate hands passed to images)
};
// samples by index (sample_xyz == nullptr) or by coordinates (sample_idx == nullptr).  sync_counts: download the
// neighbourhood sizes and grow the list capacity when one overflows (the unfused entry points); without it nothing
// waits for the device and the caller checks `worst found` in the plan summary (search_retry_needed).
// resident (may be null; then neither host pointer is read): the sample indices are gathered on the device,
// d_sample_idx[i] = d_list ? d_list[d_pos[i]] : d_pos[i].  Both arrays must stay as they are until the job's plan summary has
// arrived: a list-capacity retry gathers again.
struct SampleGather {
  const int32_t *d_list = nullptr;  // nullptr: the positions are the indices
  int list_size = 0;
  const int32_t *d_pos = nullptr;   // [S]
  // non-null: the samples are these device-resident coordinates [S][3] instead (gpd_hip_detect_sis: sis_draw_kernel wrote
  // them); the search reads them in place, with gpd_hip_search_samples' semantics — the queries use their float cast, the
  // frames keep the doubles.  d_list / d_pos are not read then.
  const double *d_xyz = nullptr;
};
int search_run(const gpd_params &p, const Cloud &c, SearchState &s, const int32_t *sample_idx, const double *sample_xyz, int S,
               hipStream_t stream, bool sync_counts = true, const SampleGather *resident = nullptr);
// list capacity the next search_run would use after a neighbourhood of `worst` entries; 0: beyond every capacity
int search_reserve_samples(SearchState &s, int S, int slots);  // buffers for S samples at the current list capacity
int search_next_capacity(const SearchState &s, int worst);
// the main stream waits for the centre sums (side stream) of the last run_neighbourhoods
int search_join(SearchState &s, hipStream_t stream);
int search_force_capacity(SearchState &s, int cap);
// HandSearch::reevaluateHypotheses on the uploaded cloud; invalidates the search state
int reevaluate_run(const gpd_params &p, const Cloud &c, SearchState &s, gpd_hand *hands, int n, int32_t *labels, hipStream_t stream);
// gpd_hip_images_given: the neighbourhood lists of S samples given by coordinates and nothing else (no hand is evaluated);
// invalidates the search state, the side stream is joined on return
int given_lists_run(const gpd_params &p, const Cloud &c, SearchState &s, const double *sample_xyz, int S, hipStream_t stream);
// ... and the caller's records [S][slots] (host) as the lists' hand sets: into d_hands, their flags into d_fvalid, every
// sample a hand set for plan_kernel (given.hip)
int given_ingest(SearchState &s, const gpd_hand *hands, int S, int slots, hipStream_t stream);
int search_download(const gpd_params &p, SearchState &s, gpd_hand *hands, int *num_sets, hipStream_t stream);
void search_free(SearchState &s);
// gpd_hip_label_view, one round: reevaluateHypotheses of n candidate records on the device (set-major, `lists` hand sets among
// them) against the ground-truth cloud gt, one neighbourhood list per hand set (search.hip)
int label_round(const gpd_params &p, const Cloud &gt, SearchState &gs, gpd_hand *d_recs, uint8_t *d_labels8, int n, int lists,
                int32_t *d_cand_list, int32_t *d_meta, int32_t *h_meta, const int32_t *d_img_status, int *img_status, int *positives,
                long long *d2h_bytes, hipStream_t stream);

// ---- gpd_hip_label_view: the ground-truth slot, a view's accumulator, selection and gather (label.hip) --------------------
struct LabelState {
  Cloud gt;                        // the ground-truth cloud (gpd_hip_upload_ground_truth) ...
  SearchState gt_search;           // ... and its neighbourhood lists, one per hand set with a candidate
  size_t cap = 0;                  // candidates the accumulator holds
  size_t image_bytes = 0;          // 3600 * C of the accumulator's images
  uint8_t *d_images = nullptr;     // [cap][60][60][C] HWC
  gpd_hand *d_hands = nullptr;     // [cap] candidate records, flags rewritten by the ground-truth check
  uint8_t *d_labels = nullptr;     // [cap]
  int32_t *d_cand_list = nullptr;  // [cap_round] candidate of the round in flight -> neighbourhood list of its hand set
  size_t cap_round = 0;
  int32_t *d_meta = nullptr;       // [4] largest ground-truth neighbourhood, positives of the round, lists built
  int32_t *h_meta = nullptr;       // pinned
  int32_t *d_sel = nullptr;        // [cap_sel] accumulator indices of the kept instances, positives first
  size_t cap_sel = 0;
  char *d_out = nullptr;           // the kept instances, contiguous: images | records | src_index | labels (16-byte aligned parts)
  char *h_out = nullptr;           // pinned: the same, then the labels of every candidate when asked for
  size_t d_out_bytes = 0, h_out_bytes = 0;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // labels start / end, select + gather start / end
  int grows = 0;                   // accumulator growths of the last call
};
constexpr size_t kLabelAccBudget = 16ull << 30;
void label_free(LabelState &ls);
int label_init(LabelState &ls);
// room for `need` accumulated candidates of image_bytes each, the first `used` kept across a growth; GPD_ERR_CAPACITY beyond 16 GB
int label_reserve(LabelState &ls, size_t need, size_t used, size_t image_bytes, size_t round_candidates, hipStream_t stream);
// offsets of the four parts of the contiguous output for k kept instances; returns the total
size_t label_out_layout(size_t k, size_t image_bytes, size_t off[4]);
// balanceInstances over the n accumulated labels on the device (balance_model.h is the definition) and the gather of the `end`
// kept positives and negatives into ls.d_out; nothing waits for the device.  sink_images != null: the images [2 end][image_bytes]
// and the labels [2 end] go there instead (device memory of the caller's, 16-byte aligned), and ls.d_out is not touched
int label_select_gather(LabelState &ls, int n, int end, hipStream_t stream, uint8_t *sink_images = nullptr, uint8_t *sink_labels = nullptr);
// gpd_hip_train_append_view: where a view's kept instances go instead of the host.  place() is called once, when their number k
// (> 0) is known and before the gather is enqueued; it returns device room for k images and k labels that stays put until the
// call returns
struct LabelSink {
  void *self;
  int (*place)(void *self, size_t k, uint8_t **images, uint8_t **labels);
};
// the body of gpd_hip_label_view (rounds.hip); sink != null: the kept images and labels go to the sink, and job->images, labels,
// hands, src_index and capacity are not read
int label_view_run(gpd_hip_ctx *ctx, gpd_label_view_job *job, const char *who, const LabelSink *sink);

// ---- gpd_hip_detect_sis: the draw, the accumulators of the rounds, the final selection (sis.hip; the definition: sis_model.h) --
constexpr int kSisDrawThreads = 512;  // sis_draw_kernel: proposals per step of its one workgroup
constexpr int kSisCentreTile = 512;   // ... and centres per LDS tile of the nearest-centre test
struct SisMeta {  // device words of a call; a copy travels to pinned memory behind every draw and at the end
  int32_t acc_g, used_g, acc_u, used_u;  // the round's draw: samples accepted / proposals consumed per stream
  int32_t centres;                       // live centres accumulated
  int32_t candidates;                    // candidate records accumulated
  int32_t kept;                          // records with score > min_score
  int32_t img_status;                    // capacity flags of the image kernels of the rounds so far
};
struct SisState {
  size_t cap = 0;                  // candidates the accumulators hold
  size_t image_bytes = 0;          // 3600 * C
  uint8_t *d_images = nullptr;     // [cap][C][60][60] planar, as the LeNet reads them
  gpd_hand *d_hands = nullptr;     // [cap] candidate records, set_index = index in the accumulated live list
  gpd_hand *d_keep = nullptr;      // [cap] the records with score > min_score, in order
  double *d_centres = nullptr;     // [cap_centres][3] samples of the live hand sets, in accumulated order
  size_t cap_centres = 0;
  double *d_round_xyz = nullptr;   // [cap_round][3] the samples of the round in flight: sis_draw_kernel writes, the search reads
  double *d_samples = nullptr;     // [cap_samples][3] the samples of every round, for samples_out
  size_t cap_round = 0, cap_samples = 0;
  int32_t *d_uniform = nullptr;    // [cap_uniform] the uniform source list
  size_t cap_uniform = 0;
  void *d_gauss = nullptr;         // [cap_block] sis::Proposal, the block in flight
  unsigned long long *d_unif = nullptr;  // [cap_block] pos_raw
  char *h_block = nullptr;         // pinned: [cap_block] Proposal, then [cap_block] pos_raw
  size_t cap_block = 0;
  SisMeta *d_meta = nullptr;
  SisMeta *h_meta = nullptr;       // pinned
  char *h_out = nullptr;           // pinned: records | samples | centres
  size_t h_out_bytes = 0;
  hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // draw start / end, accumulate end, tail start / end, words
  int grows = 0;
};
void sis_free(SisState &ss);
int sis_init(SisState &ss);
// room for `need` accumulated candidates and `centres` live centres, the first `used` / `used_centres` kept across a growth
// (by half, device to device); GPD_ERR_CAPACITY beyond 16 GB
int sis_reserve(SisState &ss, size_t need, size_t used, size_t centres, size_t used_centres, size_t image_bytes, hipStream_t stream);
int sis_reserve_round(SisState &ss, size_t round_samples, size_t all_samples, size_t uniform, size_t block);
// one block of each stream through the selection rule; continues from the counts in ss.d_meta.  Nothing waits for the device.
int sis_draw(SisState &ss, const Cloud &c, int L, int n_gauss, int n_unif, int n_uniform_list, const double ws[6], int method, int num_gauss,
             int num_rand, hipStream_t stream);
// the round's n candidate records at ss.d_hands + acc (set-major, as plan_emit_hands left them): their live sets' samples join
// the centre list behind the centres_before it holds, set_index becomes the index in the accumulated live list; the image kernels'
// capacity flags (d_img_status) are folded into the call's
int sis_accumulate(SisState &ss, size_t acc, int n, int centres_before, const int32_t *d_img_status, hipStream_t stream);
// scores into the n accumulated records; those with score > min_score, in order, into ss.d_keep, their number into d_meta->kept
int sis_select(SisState &ss, const float *d_scores, int n, double min_score, hipStream_t stream);

// GraspDetector::filterGraspsWorkspace (grasp_detector.cpp:334-398) [+ filterGraspsDirection, :423-456] for one valid
// hand: aperture and the workspace box around the hand's outline [, then the approach direction].  The reference computes right_top from left_bottom
// (:360-363); kept.  Evaluated with the same unfused fp64 operations on the host and on the device.
struct FilterConsts {
  double min_aperture, max_aperture, half_width, hand_depth;
  double workspace[6];
  // filterGraspsDirection (grasp_detector.cpp:423-456): a hand is dropped when acos(direction . approach) > thresh_rad.
  // The device has no glibc acos, and a one-ulp difference between two acos implementations would be a different
  // candidate list; so the HOST turns the test into one on the dot product itself: dot_drop_max = the largest double x
  // in [-1, 1] with acos(x) > thresh_rad by the host's libm (bisection over the doubles; acos is monotone), and a hand is
  // dropped iff -1 <= dot <= dot_drop_max.  A dot product outside [-1, 1] (acos = NaN) keeps the hand, as the reference does.
  int dir_on;
  double dir[3];
  double dot_drop_max;
};
FilterConsts filter_consts(const gpd_params &p);  // host_math.cpp
__host__ __device__ inline bool workspace_ok(const FilterConsts &f, const gpd_hand &h) {
  bool ok = h.grasp_width >= f.min_aperture && h.grasp_width <= f.max_aperture;
  for (int r = 0; r < 3 && ok; r++) {
    const double bin = h.frame[3 * r + 1], app = h.frame[3 * r + 0];
    const double lb = h.position[r] + f.half_width * bin;
    const double rb = h.position[r] - f.half_width * bin;
    const double lt = lb + f.hand_depth * app;
    const double rt = lb + f.hand_depth * app;
    const double ap = h.position[r] - 0.05 * app;
    const double mn = fmin(fmin(fmin(lb, rb), fmin(lt, rt)), ap);
    const double mx = fmax(fmax(fmax(lb, rb), fmax(lt, rt)), ap);
    ok = mn >= f.workspace[2 * r] && mx <= f.workspace[2 * r + 1];
  }
  if (ok && f.dir_on) {
    const double dot = f.dir[0] * h.frame[0] + f.dir[1] * h.frame[3] + f.dir[2] * h.frame[6];  // direction^T * approach, unfused
    ok = !(dot >= -1.0 && dot <= f.dot_drop_max);
  }
  return ok;
}
void filter_workspace_host(const gpd_params &p, gpd_hand *hands, int num_sets);

// ---- Candidate plan (plan.hip) -----------------------------------------------------
// What GraspDetector::detectGrasps does between its stages on the host — filterGraspsWorkspace
// dropping hand sets (grasp_detector.cpp:238, 334-398), createImageList's set-major / slot-minor
// gather of the valid hands (image_generator.cpp:91-98), the per-set shadow LCG offsets
// (hand_set.cpp:263-266 is one global stream) and the score write-back (:269-273) — as device
// tables, built by one plan_kernel launch from the search results.
struct PlanSummary {  // copied to the host once per call (pinned)
  int32_t num_sets;          // samples with a frame neighbourhood (frame_estimator.cpp:24-29)
  int32_t num_candidates;    // valid hands after the filter
  int32_t num_shadow_sets;   // (live set, camera) voxel bitsets
  int32_t worst_found;       // largest neighbourhood found by the search (list capacity check)
  int32_t live_sets;         // sets with at least one candidate
  int32_t mismatch_set;      // gpd_hip_images: first set whose sample differs from the search's (or that the search does
                             // not have), -1: none
  int32_t pad_[2];
  long long sum_set_ni, sum_cand_ni;  // for the algorithmic byte count of SURVEY §8d
  unsigned long long total_draws;     // shadow LCG draws of all hand sets of the call (the next sample range's lcg_base)
};
struct PlanPart {  // what one workgroup of plan_kernel publishes for the workgroups after it (64 bytes)
  int32_t sum[3];   // hand sets, candidates, shadow bitsets of its samples
  int32_t worst;
  unsigned long long draws;  // LCG draws of its samples
  long long sum_set_ni, sum_cand_ni;
  int32_t live, mismatch;
  int32_t sets;          // caller flags: hand sets of its samples, published first
  unsigned ready_sets;   // stamps: the launch number once `sets` / the rest is complete
  unsigned ready;
  unsigned pad_;
};
static_assert(sizeof(PlanPart) == 64, "PlanPart");
struct Plan {
  int cap_samples = 0, cap_slots = 0, cap_cams = 0;
  PlanPart *d_parts = nullptr;   // [cap_samples / 256 + 1]
  unsigned *d_ticket = nullptr;  // arrival counter of plan_kernel's workgroups (0 between launches: the kernel resets it)
  unsigned epoch = 0;
  int32_t *d_sample_of_set = nullptr;  // [S]
  int32_t *d_hand_cand = nullptr;      // [S][slots] candidate ordinal of a hand, -1: none
  int32_t *d_cand_hand = nullptr;      // [S*slots] hand (sample slot * slots + slot) of a candidate
  int32_t *d_cand_out = nullptr;       // [S*slots] index of the candidate in the set-major hand array handed to the caller
  int32_t *d_cand_meta = nullptr;      // [S*slots][4]: sample slot, N_images, first shadow bitset (< 0: none), number of bitsets
  int32_t *d_set_meta = nullptr;       // [S*cams][8]: sample slot, N_images, lcg offset lo, hi, camera
  PlanSummary *d_summary = nullptr;
  PlanSummary *h_summary = nullptr;    // pinned
  uint8_t *d_set_flags = nullptr;      // gpd_hip_images: the caller's is_valid flags, [sets][slots] ...
  double *d_set_samples = nullptr;     // ... and the samples of its hand sets, [sets][3]
  int cap_set_flags = 0;
};
void plan_free(Plan &pl);
int plan_reserve(Plan &pl, int want_samples, int slots, int cams, hipStream_t stream);
// Enqueues plan_kernel + the summary copy on `stream`; the caller waits for the stream before reading pl.h_summary.
// set_flags == nullptr: the validity flags are the ones hand_eval_kernel left (search + workspace filter).
// Otherwise (gpd_hip_images) the caller's flags, set-major [num_sets_given][slots], and the samples of its sets
// [num_sets_given][3] (host pointers, copied asynchronously: keep them alive until the stream has been waited for).
int plan_build(const gpd_params &p, const Cloud &c, const SearchState &s, Plan &pl, hipStream_t stream,
               const uint8_t *set_flags = nullptr, const double *set_samples = nullptr, int num_sets_given = 0);
// set-major hand records of the last search with `valid` = the filtered flag and the scores written back
// (out: [num_sets][slots], device); candidates_only: the scored valid hands in candidate order instead.
int plan_emit_hands(const gpd_params &p, const SearchState &s, const Plan &pl, const float *d_scores, gpd_hand *d_out,
                    bool candidates_only, hipStream_t stream);
// GraspDetector::selectGrasps (grasp_detector.cpp:405-420) over the device score array: the k best candidates,
// score descending; *tie: equal scores among them or at the cut (the caller then falls back to std::partial_sort)
int select_topk(const float *d_scores, int n, int k, int32_t *d_sel /* [k] candidate ordinals */, int32_t *d_tie,
                hipStream_t stream);
int gather_hands(const gpd_params &p, const SearchState &s, const Plan &pl, const float *d_scores, const int32_t *d_sel, int k,
                 gpd_hand *d_out, hipStream_t stream);
// records sel[0..k) of a flat candidate list emitted earlier (plan_emit_hands, candidates only)
int gather_records(const gpd_hand *d_all, const int32_t *d_sel, int k, gpd_hand *d_out, hipStream_t stream);
// the largest k select_topk takes; beyond it the fused entries select with std::partial_sort on the downloaded scores
int select_topk_capacity();

// ---- Grasp images (image_state.hip; images.hip: images_launch and the layout converters) ------------
struct ImageState {
  unsigned long long lcg_base = 0;    // shadow draws consumed before this list's first hand set (a sample range of a sharded cloud)
  int num_candidates = 0;
  int capacity = 0;                   // images
  uint8_t *d_images = nullptr;        // planar [n][C][60][60]
  uint8_t *d_images_hwc = nullptr;    // [n][60][60][C], only when the caller downloads pixels
  uint32_t *d_set_bits = nullptr;     // [sets][SETWORDS] shadow voxel bitsets
  int num_shadow_sets = 0, cap_shadow_sets = 0;
  bool wide = false;                  // the shadow kernels' wide voxel windows (image_model.h Vox<WIDE>), picked from the image volume
  bool huge = false;                  // ... or beyond those: the general shadow kernel, a set region of run-time size
  int set_sd = 0, set_sr = 0;         // edge / radius (voxels) of the region shadow_set_kernel fills around a sample
  size_t cap_setwords = 0;            // words per row of d_set_bits
  int jitter = 0;                     // gpd_hip_set_shadow_jitter (15 channels): the windows above and the constant block follow it,
  unsigned long long jitter_seed = 0; // so a switch is a new geometry to this state
  int32_t *d_overflow2 = nullptr;     // [capacity]: candidates the large shadow instantiation could not list (count: d_status[2])
  char *d_huge_scratch = nullptr;     // list rows of the general shadow kernel
  int channels = 0;
  int slots = 0;                      // hand slots per set of the list (num_hand_axes * num_orientations)
  int32_t *d_overflow = nullptr;      // [capacity]: candidates for the large shadow instantiation (count: d_status[1])
  int32_t *d_pts_overflow = nullptr;  // [capacity]: candidates for the large points instantiation (count: d_status[3])
  char *d_pts_scratch = nullptr;      // point arrays of the large instantiation, one row per workgroup of its grid
  int32_t *d_status = nullptr;        // [4]: error flags from the kernels, then the counters of the three overflow lists
  long long stat_sets = 0, stat_sum_set_ni = 0, stat_sum_cand_ni = 0;  // for the algorithmic byte count
  std::vector<unsigned char> consts;  // the constant block (image geometry) the candidate list was built with
  double view_points[3 * kMaxCams] = {0};  // of the cloud the list was built on (shadow_set_kernel argument)
  // the normals + depth kernel does not depend on the shadow kernels: it runs on a side stream beside them (both kinds
  // of workgroup fit a CU together) and is joined at the end of the stage
  hipStream_t aux = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  bool side_stream = true;  // off inside gpd_hip_detect_batch: the other cloud's kernels already fill the gaps (measured)
};
int images_reserve(const gpd_params &p, ImageState &im, int n, int shadow_sets);
// images_reserve for the state's own list and its constant block, under the state's present settings (the lane is idle)
int images_prepare(const gpd_params &p, ImageState &im);
// Sizes the image buffers for the plan's candidate list (summary already on the host) and launches the image kernels.
int images_run(const gpd_params &p, const Cloud &c, const SearchState &s, const Plan &pl, ImageState &im, hipStream_t stream);
// Re-launches them on the resident list.  Nothing waits for the device: capacity flags accumulate in im.d_status.
int images_launch(const SearchState &s, const Plan &pl, ImageState &im, hipStream_t stream, bool counters_clean = false);
void images_status_text(int status, char *buf, size_t len);
// gpd_hip_last_image_routes on a lane whose stream has been waited for (route: im.num_candidates entries)
int images_routes(const ImageState &im, int32_t *route, long long info[8]);
hipError_t planar_to_hwc(const uint8_t *src, uint8_t *dst, int n, int C, hipStream_t stream);
hipError_t hwc_to_planar(const uint8_t *src, uint8_t *dst, int n, int C, hipStream_t stream);
void images_free(ImageState &im);

// Host-side constants of the path (host_math.cpp), computed with libm exactly as the
// reference computes them on the host.
struct HostConsts {
  double rot[GPD_MAX_SLOTS][9];  // Ry(pi) * R_axis(angle) factors: see host_math.cpp
  double rot_binormal[9];        // AngleAxisd(pi, UnitY)
  double finger_spacing[32];     // 2 * num_finger_placements
  double deepen_depths[128];
  int num_deepen;
  double cos_friction;
  double nn_radius_hands, nn_radius_images;
};
void host_consts(const gpd_params &p, HostConsts &h);

// ---- Launchers for other units (a kernel is launched from the unit that defines it).  Hand kernels (hands.hip): what the
// drivers of search.hip enqueue on the lists of a SearchState ------------------------------------------------------------
// Each takes the lock of the device's constant block (uploading p / hc when they differ from the loaded ones), launches and
// drops the lock.  cap: the list capacity the neighbourhoods were built with.
#pragma GCC visibility push(hidden)  // calls between two units of the library: not part of its dynamic symbol table
// hand_eval_kernel over S samples: s.d_hands, s.d_fvalid
int hands_enqueue_eval(const gpd_params &p, const HostConsts &hc, SearchState &s, int cap, int S, hipStream_t stream);
// reeval_kernel over the n records in s.d_hands (one per sample slot): their flags, s.d_labels
int hands_enqueue_reeval(const gpd_params &p, const HostConsts &hc, SearchState &s, int cap, int n, hipStream_t stream);
// label_kernel over the n records d_recs, candidate c on list d_cand_list[c] of the `lists` in gs: their flags, d_labels8
int hands_enqueue_label(const gpd_params &p, const HostConsts &hc, SearchState &gs, int cap, int lists, gpd_hand *d_recs, int n,
                        const int32_t *d_cand_list, uint8_t *d_labels8, hipStream_t stream);
// label_sets_kernel / label_meta_kernel (one workgroup each) around it
int hands_enqueue_label_sets(const gpd_hand *d_recs, int n, int32_t *d_cand_list, double *d_sample_xyz, int32_t *d_meta, hipStream_t stream);
int hands_enqueue_label_meta(const int32_t *d_counts, int lists, const uint8_t *d_labels8, int n, const int32_t *d_img_status, int32_t *d_meta,
                             hipStream_t stream);
// (cloud.hip, for normals.hip) the planes of c again, its coordinates as staged and the normals d_nrm [num_points][3]
int cloud_set_normals(Cloud &c, const float *d_nrm, hipStream_t stream);
#pragma GCC visibility pop

// ---- Cloud::sampleAbovePlane on the device (plane.hip; the definition: plane_model.h) ------------------------
constexpr int kPlaneMaxHyp = 1024;   // hypotheses per call: max_iterations <= 1023
constexpr int kPlaneSwapCap = 7680;  // positions >= 3 of shuffled_indices the draws of one call may touch (LDS table)
struct PlaneState {
  int capacity = 0;                  // points of the compaction buffers
  void *d_meta = nullptr;            // hypotheses drawn, swap-table overflow, points the last compaction wrote
  float4 *d_coef = nullptr;          // [kPlaneMaxHyp] plane of every hypothesis
  int32_t *d_counts = nullptr;       // [kPlaneMaxHyp] its inliers
  float *d_accu = nullptr;           // [9] the refinement's sums (one-wave variant)
  int32_t *d_block_count = nullptr, *d_block_off = nullptr;
  float *d_xyz = nullptr;            // [capacity][3] the best model's inliers in index order
  int32_t *d_idx = nullptr;          // [capacity] the points off the final plane, ascending
  char *h_pin = nullptr;             // pinned: meta, planes, counts, sums
  std::vector<float> h_xyz;          // the inliers' xyz for the host's refinement
};
void plane_free(PlaneState &s);
int plane_reserve(PlaneState &s, int n);  // the buffers for clouds of up to n points (gpd_hip_detect_batch sizes its lanes ahead)
// on the uploaded cloud c; indices_out holds c.num_points entries.  *num_out = 0: no plane, or no point off it.
// indices_out == nullptr (the resident form, raw scans of gpd_hip_detect_batch): the list stays in s.d_idx, *num_out of them;
// only the hypotheses' counts, the refinement's inliers and the 4-byte total cross PCIe
int plane_fit_run(PlaneState &s, const Cloud &c, double threshold, int max_iterations, double probability, int optimize, int32_t *indices_out,
                  int *num_out, float coeffs[4], int *num_inliers, int *iterations, hipStream_t stream);

// ---- Cloud::refineNormals on the device (refine.hip; the definition: refine_model.h) --------------------------
constexpr int kRefineKCap = 256;     // neighbours per point: k <= 256
struct RefineState {
  int cap_points = 0;
  size_t cap_lists = 0;              // int32 entries of d_lists
  int32_t *d_lists = nullptr;        // [ceil(P / 64)][k][64] the sorted neighbour indices by cell-order position
  float4 *d_buf[2] = {nullptr, nullptr};  // [P] the normals between passes (ping-pong), by original index
  float *d_dots = nullptr;           // [P] the stop rule's dot of every point (NaN: not counted)
  float *d_aos = nullptr;            // [P][3] the result for the caller
  float *h_dots = nullptr;           // pinned [2][cap_points]
  hipEvent_t ev_dots[2] = {nullptr, nullptr};  // a pass's dots are on the host
  std::vector<hipEvent_t> ev;        // kNN start / end, then start / end of every pass
  int32_t *d_nan = nullptr;          // the resident form's count of non-finite normals ...
  int32_t *h_nan = nullptr;          // ... and its pinned host side
};
void refine_free(RefineState &s);
int refine_reserve(RefineState &s, int n, int k);  // the buffers for clouds of up to n points with k neighbours each
// on the uploaded cloud c, k <= kRefineKCap (clamped to the cloud's size); replaces c's normals and bumps its generation.
// ddot_out (may be null) receives one mean per pass; kernel_ms (may be null): kNN, the passes launched, the whole call.
// normals_out == nullptr (the resident form, raw scans of gpd_hip_detect_batch): the normals are not downloaded, the
// non-finite ones are counted on the device; only the per-pass dots of the stop rule and that count cross PCIe
int refine_run(RefineState &s, Cloud &c, int k, int max_iterations, float threshold, float *normals_out, int *iterations_out, float *ddot_out,
               int *num_nan_out, float *kernel_ms, hipStream_t stream);

// ---- Cloud::removeStatisticalOutliers on the device (outliers.hip; the definition: outlier_model.h) ----------
struct OutlierState {
  int cap_points = 0, cap_cams = 0;
  float *d_dist = nullptr;           // [P] the mean neighbour distance of every point, by original index
  float *h_dist = nullptr;           // pinned: its way down for the two sequential sums of the threshold
  int32_t *d_block_count = nullptr, *d_block_off = nullptr;  // the compaction's per-workgroup counts and their scan
  int32_t *d_kept = nullptr;         // [P] the kept input indices, ascending
  float *d_xyz = nullptr, *d_nrm = nullptr;  // [P][3] the kept points and their normals
  int32_t *d_cam = nullptr;          // [cams][kept] their camera-source rows
  int32_t *d_total = nullptr;        // the number of kept points ...
  int32_t *h_total = nullptr;        // ... and its pinned host side
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // distance kernel start / end, compaction start / end
};
void outlier_free(OutlierState &s);
int outlier_reserve(OutlierState &s, int n, int num_cams);  // the buffers for clouds of up to n points / num_cams cameras
// On the uploaded cloud c, inside the domain of outlier::refusal (the caller has checked it): the kept points, with their
// normals (carry_normals; zeros otherwise) and camera-source rows, become c — grid rebuilt, generation bumped.
// kept_out (may be null, else room for the old num_points): the kept input indices, ascending; *num_kept their number;
// stats: mean, stddev, threshold; dist_out (may be null): the old num_points mean distances; kernel_ms (may be null):
// distance kernel, compaction, the whole call.  GPD_ERR_INVALID and c untouched when no point would be kept.
int outlier_run(OutlierState &s, Cloud &c, int mean_k, double mult, bool carry_normals, int32_t *kept_out, int *num_kept, double stats[3],
                float *dist_out, float *kernel_ms, hipStream_t stream);

}  // namespace gpd
