// What the host-side translation units of the C-ABI share (context.hip, detect.hip, rounds.hip, given.hip, batch.hip, replay.hip; no kernel
// includes this): the context and its lanes, one fused detect in flight, the error text and the allocation counter.
#pragma once

#include <initializer_list>
#include <vector>

#include "gpd_internal.h"

namespace gpd {

constexpr int kLanes = 2;
constexpr int kLeNetChunk = 65536;                // lenet_forward's images per pass (lenet.hip)
constexpr size_t kReserveBudget = 16ull << 30;   // candidate-sized buffers of a lane when the caller names no bound

struct HostFlags {  // pinned; written by the last copies of a job
  int32_t status;   // capacity flags of the image kernels
  int32_t tie;      // select_topk: equal scores among the winners or at the cut
  int32_t lenet;    // != 0: a conv1 launch of this job gave up on its slot protocol (lenet.hip)
  int32_t pad_;
};

struct Lane {
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // search start / end, images end, LeNet end, images start
  hipEvent_t ev_plan = nullptr, ev_done = nullptr;  // the plan summary / the results of the job in flight are on the host
  hipEvent_t ev_chunk[4] = {nullptr, nullptr, nullptr, nullptr};  // a large record list leaves in four copies: the host copies one on while the next travels
  float stage_ms[3] = {0.f, 0.f, 0.f};
  Cloud cloud;
  PreState pre;      // raw scans of gpd_hip_detect_batch: workspace cut + voxeliser of the cloud this lane works on
  SearchState search;
  Plan plan;
  ImageState images;
  LeNetScratch lenet_scratch;
  float *d_scores = nullptr;
  int d_scores_cap = 0;
  gpd_hand *d_out = nullptr;  // hand records gathered for the caller
  size_t d_out_cap = 0;       // records
  char *h_out = nullptr;      // pinned: records, then scores
  size_t h_out_bytes = 0;
  HostFlags *h_flags = nullptr;  // pinned
  int32_t *d_sel = nullptr;      // [SEL capacity] candidate ordinals of the selection, then the tie flag
  int d_sel_cap = 0;
  gpd_hand *d_all = nullptr;     // selections (num_selected > 0): every candidate record of the job, scored — what a selection
  size_t d_all_cap = 0;          // gathers from, also after the lane's search / plan buffers belong to the next cloud
  // staging for gpd_hip_score with host images
  uint8_t *d_img_in = nullptr;      // HWC images handed to gpd_hip_score
  uint8_t *d_img_planar = nullptr;  // their planar copy
  size_t d_img_in_bytes = 0;
  // raw scans of gpd_hip_detect_batch that carry on past the normals: a state per LANE — the next cloud's fit runs on the other
  // lane's stream while this lane's search still gathers from plane.d_idx
  PlaneState plane;
  RefineState refine;
  OutlierState outliers;
  int32_t *d_pos = nullptr;  // [draw_cap] the draw positions of Cloud::subsample (sample_model.h), computed on the host
  int32_t *h_pos = nullptr;  // pinned: [draw_cap] their way up, then [2][draw_cap] the sample indices searched on their way
  int draw_cap = 0;          //   down (samples_out), one half per job of the lane in flight
};

// one fused detect in flight on a lane
struct Job {
  const int32_t *sample_idx = nullptr;
  const double *sample_xyz = nullptr;
  int S = 0;
  int mode = 0;          // 0: all hand sets [num_sets][slots]; 1: candidates only (num_selected > 0: the best ones)
  int num_selected = 0;
  gpd_hand *hands = nullptr;
  long long capacity = 0;  // records `hands` can take
  int num_sets = 0, num_candidates = 0, num_hands = 0;
  bool live = false;       // device work enqueued, end() still has to collect it
  int out_records = 0;
  double t_plan_ms = 0.0;  // host clock when the plan summary had arrived (job_middle past its wait)
  double copy_ms = 0.0;    // job_end: handing the records over (after the wait)
  int chunks = 0;          // > 0: the records leave the device in this many copies, an event behind each
  unsigned long long lcg_base = 0;   // in: shadow draws of the cloud's sample ranges before this one (gpd_hip_detect_sharded)
  unsigned long long lcg_draws = 0;  // out: shadow draws of this job's hand sets
  bool resident = false;             // the sample indices are gathered on the device from `gather` (neither host pointer is read)
  SampleGather gather;
};

}  // namespace gpd

struct gpd_hip_ctx {
  int device = 0;
  bool in_batch = false;  // gpd_hip_detect_batch is driving the lanes
  gpd_params params;
  gpd::LeNetWeights lenet;
  gpd::Lane lane[gpd::kLanes];
  gpd::PreState pre;
  gpd::ClusterState cluster;
  gpd::PlaneState plane;  // gpd_hip_sample_above_plane
  gpd::RefineState refine;  // gpd_hip_refine_normals
  gpd::OutlierState outliers;  // gpd_hip_remove_statistical_outliers
  gpd::LabelState label;    // gpd_hip_upload_ground_truth / gpd_hip_label_view: the ground-truth slot and a view's accumulator
  gpd::SisState sis;        // gpd_hip_detect_sis: the draw's buffers and the accumulators of the rounds
  std::vector<hipEvent_t> replay_events;  // 6 per gpd_hip_replay call: start, images done, conv1, conv2, fc1, end
  float replay_kernel_ms[4] = {0, 0, 0, 0};  // conv1, conv2, fc1, fc2 sums of the replays of the last gpd_hip_replay_times
  size_t replay_used = 0;
  // GPD_REPLAY_PIPE=1 (experiment): the image stage of replay k + 1 beside the LeNet stage of replay k —
  // images on lane 0's stream into one of two image buffers, LeNet on `pipe_stream` behind the buffer's event
  hipStream_t pipe_stream = nullptr;
  uint8_t *pipe_images[2] = {nullptr, nullptr};  // [0] is lane 0's own buffer while the mode is on
  size_t pipe_bytes = 0;
  hipEvent_t pipe_filled[2] = {nullptr, nullptr}, pipe_read[2] = {nullptr, nullptr};
  bool pipe_read_valid[2] = {false, false};
  unsigned pipe_k = 0;
};

namespace gpd {

// ---- context.hip ----
const char *error_text();               // this thread's error text (what gpd_hip_last_error returns)
void error_text_set(const char *text);  // ... put back, or taken over from another thread
void set_images_status_error(int status);  // images_status_text as the error text
int allocs_now();                       // buffer growths of this thread so far (note_alloc); callers book differences
double now_ms();                        // the steady clock, for host timelines

int lane_init(Lane &L, hipStream_t shared = nullptr);
// Every buffer of a lane for clouds of up to `points` points / `cams` cameras, `samples` samples and `candidates`
// scored hands (selections of up to `selected` winners; -1: none), so that no call within those sizes allocates:
// growing a buffer is hipFree + hipMalloc, which waits for the whole device — in a batch that is a hole in BOTH
// lanes' queues.  gpd_hip_reserve and gpd_hip_detect_batch call this ahead of the first cloud.
int lane_reserve(gpd_hip_ctx *ctx, Lane &L, int points, int cams, int samples, int candidates, int selected);
int candidate_bound(const gpd_params &p, int samples, int cams = 1, size_t budget = kReserveBudget, const LeNetNet *net = nullptr);
int reserve_scores(Lane &L, int n);
int reserve_out(Lane &L, size_t records, size_t extra_bytes);
int reserve_draws(Lane &L, int n);
int reserve_selection(Lane &L, int k, int n);
int check_samples(const char *who, const int32_t *sample_indices, const double *sample_xyz, int num_samples, int num_points);

// The refusals an entry opens with, in the order it names them: "<who>: bad argument" (GPD_ERR_INVALID) without a context or
// with args_ok false, then per need the text and GPD_ERR_STATE.  GPD_OK: the entry may go on.
enum class Need { Cloud, LeNet, NoBatch };  // lane 0 holds a cloud; LeNet weights are set; gpd_hip_detect_batch is not driving the lanes
int refuse(const char *who, const gpd_hip_ctx *ctx, bool args_ok, std::initializer_list<Need> needs = {});

// ---- one stage on a lane (context.hip); the callers record the events that time a stage around these ----
// The image kernels over the lane's plan (its summary is on the host), under a StageRange `range`, between ev_start and ev_end;
// ev_start null: the caller recorded it ahead of the lists and the plan it times with the images.
int lane_images(gpd_hip_ctx *ctx, Lane &L, bool side_stream, unsigned long long lcg_base, const char *range, hipEvent_t ev_start,
                hipEvent_t ev_end);
// A LeNet pass over n planar images into L.d_scores, and the pass's launch error word on its way to h_flags->lenet; n == 0
// enqueues nothing and clears the flag on the host.
int lane_lenet(gpd_hip_ctx *ctx, Lane &L, const uint8_t *d_images, int n, const char *range);
// After the wait: the capacity flags of the image kernels (GPD_ERR_CAPACITY), then, for a call that scored, h_flags->lenet.
int lane_check(Lane &L, int32_t image_status, bool scored);
// The lane's n images in the caller's layout (HWC) and their candidates' indices, enqueued towards the caller's memory.
int lane_download_images(const gpd_params &p, Lane &L, int n, uint8_t *images, int32_t *cand_index);

// ---- detect.hip: the three steps of a fused detect ----
int job_begin(gpd_hip_ctx *ctx, Lane &L, Job &J);
int job_wait_plan(gpd_hip_ctx *ctx, Lane &L, Job &J);  // the middle step in two halves, for gpd_hip_detect_sharded
int job_enqueue(gpd_hip_ctx *ctx, Lane &L, Job &J);
int job_middle(gpd_hip_ctx *ctx, Lane &L, Job &J);
int job_end(gpd_hip_ctx *ctx, Lane &L, Job &J);

}  // namespace gpd
