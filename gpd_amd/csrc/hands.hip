// Hand evaluation on gfx950, over the neighbourhood lists that search.hip builds.
//
// Replaces HandSearch::evalHands (candidate/hand_search.cpp:144-188),
// HandSet::evalHandSet/evalHands (candidate/hand_set.cpp:31-116), FingerHand
// (candidate/finger_hand.cpp:6-184), Hand::construct (candidate/hand.cpp:24-45),
// HandSet::modifyCandidate/labelHypothesis (hand_set.cpp:235-261) and
// Antipodal::evaluateGrasp (candidate/antipodal.cpp:10-96).
//
// hand_eval_kernel       one workgroup per (sample, orientation): one transform pass compacts
//     the in-height points into LDS, then order-free reductions over them (finger
//     collision masks, deepen masks, closing region, antipodal extremes, antipodal
//     counts).  The reference's cropByHandHeight quirk (point_list.cpp:44-55 pads with
//     copies of column 0) is reproduced by a ghost point with multiplicity N-k.
// reeval_kernel          HandSearch::reevaluateHypotheses (hand_search.cpp:66-134, 190-228).
// label_*_kernel         the same check for a round of gpd_hip_label_view, and its bookkeeping.
//
// All fp64 expressions are evaluated unfused, left to right (-ffp-contract=off),
// exactly as oracle/gpd_oracle.cpp defines them.
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstring>

#include <mutex>

#include "const_block.h"
#include "gpd_internal.h"
#include "wave_ops.h"

namespace gpd {

// ---------------------------------------------------------------------------
// hand_eval_kernel
// ---------------------------------------------------------------------------
struct HandConsts {
  double rot[GPD_MAX_SLOTS][9];
  double rot_binormal[9];
  double spacing[32];
  double spfw[32];  // spacing[i] + finger width, as isGapFree adds them (finger_hand.cpp:173-184)
  // finger slots a lateral coordinate can fall into: cell q = (t1 - lut_base) * lut_inv of 256 cells over the slots'
  // extent (the outer cells reach to infinity) -> bit mask of the slots whose open interval touches the cell widened
  // by 1 % — a superset; the exact comparisons decide
  uint32_t slot_lut[256];
  double lut_base, lut_inv;
  double depths[128];  // deepenHand's steps (finger_hand.cpp:116-121), evaluated 32 at a time
  int num_deepen;
  int nfp;  // num_finger_placements
  int slots;
  int deepen;
  int min_viable;
  double cos_friction;
  double fw, hand_depth, hand_height, init_bite;
  FilterConsts filter;  // filterGraspsWorkspace (grasp_detector.cpp:334-398), applied to the valid hands
};

struct HandParams {
  const int32_t *counts;
  const float *nn;
  const double *frames;
  int cap;
  gpd_hand *hands;
  uint8_t *fvalid;  // hand_eval_kernel: [S][slots] is_valid after filterGraspsWorkspace
  float4 *hl;       // [S][cap] neighbourhood_kernel's gather -> hand_eval_kernel; its length per sample in counts[8 s + 6]
  double radius;    // of the hand-search neighbourhood (bounds |p - sample|)
  int num_samples;
  int32_t *labels;  // reeval_kernel only: [n] labels (SearchState::d_labels; counts[8 s + 5] is centre_kernel's, on the side stream)
  unsigned long long *dbg;  // profiling aid (GPD_HE_TIMING=1): per-phase cycle sums of thread 0, [8] = sum of N, [9] = sum of k
};

__device__ inline void mat3mul(const double *a, const double *b, double *c) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) c[3 * i + j] = a[3 * i + 0] * b[0 + j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}

// The list FingerHand sees: in-height points (z in (-h, h)) followed by the ghost
// (column 0) with multiplicity N-k.  Iterates entries e in [0, N]; e == N is the
// ghost.  Returns false when the entry is not part of the list.
struct ListCtx {
  const float *nn;
  int cap, N;
  double FR[9];
  double sample[3];
  double hand_height;
  int ghost_mult;  // N - k (valid after pass 0)
  // hand_eval_kernel: the in-height entries compacted into LDS by pass 0 — forward / lateral
  // coordinate and neighbour rank of each (ct0 == nullptr: not compacted, every pass transforms
  // all N points again)
  const double *ct0, *ct1;
  const unsigned short *ce;
  int kc;
};
__device__ inline bool list_entry(const ListCtx &L, int e, double t[3], double tn[3], int &mult) {
  const int i = (e == L.N) ? 0 : e;
  const double c0 = (double)L.nn[0 * L.cap + i] - L.sample[0];
  const double c1 = (double)L.nn[1 * L.cap + i] - L.sample[1];
  const double c2 = (double)L.nn[2 * L.cap + i] - L.sample[2];
  const double n0 = (double)L.nn[3 * L.cap + i], n1 = (double)L.nn[4 * L.cap + i], n2 = (double)L.nn[5 * L.cap + i];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    t[r] = L.FR[0 + r] * c0 + L.FR[3 + r] * c1 + L.FR[6 + r] * c2;
    tn[r] = L.FR[0 + r] * n0 + L.FR[3 + r] * n1 + L.FR[6 + r] * n2;
  }
  if (e == L.N) {
    mult = L.ghost_mult;
    return L.ghost_mult > 0;
  }
  mult = 1;
  return t[2] > -1.0 * L.hand_height && t[2] < L.hand_height;
}

// f(t0, t1, mult, rank) for every entry of the list FingerHand sees (in-height points, then the
// ghost with rank N); the passes are order-free reductions, so the compacted order is as good
template <class F>
__device__ inline void for_each_entry(const ListCtx &L, F f) {
  if (L.ct0) {
    for (int c = threadIdx.x; c < L.kc; c += 256) f(L.ct0[c], L.ct1[c], 1, (int)L.ce[c]);
    if (threadIdx.x == 255 && L.ghost_mult > 0) {
      double t[3], tn[3];
      int mult;
      list_entry(L, L.N, t, tn, mult);
      f(t[0], t[1], mult, L.N);
    }
  } else {
    for (int e = threadIdx.x; e <= L.N; e += 256) {
      double t[3], tn[3];
      int mult;
      if (list_entry(L, e, t, tn, mult)) f(t[0], t[1], mult, e);
    }
  }
}

__constant__ HandConsts c_hand;
constexpr int HE_COMPACT = 2048;  // in-height entries kept in LDS by hand_eval_kernel (36 KB: four workgroups per CU; 1664 entries = five per CU
                                  // measured slower, 0.566 vs 0.557 ms of search: more samples fall back to walking their full list)

// computePointsInClosingRegion (finger_hand.cpp:141-171) + grasp width (hand_set.cpp:235-245) +
// Antipodal::evaluateGrasp (antipodal.cpp:10-96; lateral 1, forward 0, vertical 2) over the list of
// L.  Returns false when the closing region is empty; label 0 none, 1 half, 2 full.
__device__ bool closing_region_label(const ListCtx &L, int N, double top, double bottom, double left, double right, const HandConsts &K,
                                     double &width, int &label, unsigned *s_u, double *s_d, long long *s_l) {
  double ymin = DBL_MAX, ymax = -DBL_MAX;
  unsigned any_c = 0;
  for_each_entry(L, [&](double t0, double t1, int, int) {
    if (t0 > bottom && t0 < top && t1 > left && t1 < right) {
      any_c = 1;
      ymin = fmin(ymin, t1);
      ymax = fmax(ymax, t1);
    }
  });
  any_c = block_or(any_c, s_u);
  label = 0;
  width = 0.0;
  if (!any_c) return false;
  ymin = block_min(ymin, s_d);
  ymax = block_max(ymax, s_d);
  width = ymax - ymin;
  const double min_x = ymin + 0.003, max_x = ymax - 0.003;
  double lx0 = DBL_MAX, lx1 = -DBL_MAX, lz0 = DBL_MAX, lz1 = -DBL_MAX;
  double rx0 = DBL_MAX, rx1 = -DBL_MAX, rz0 = DBL_MAX, rz1 = -DBL_MAX;
  unsigned lr = 0;
  for_each_entry(L, [&](double t0, double t1, int, int e) {
    if (!(t0 > bottom && t0 < top && t1 > left && t1 < right)) return;
    double t[3], tn[3];  // the vertical coordinate and the normal only of the few points between the fingers
    int mult;
    list_entry(L, e, t, tn, mult);
    const double ln = 0.0 * tn[0] + -1.0 * tn[1] + 0.0 * tn[2];
    const double rn = 0.0 * tn[0] + 1.0 * tn[1] + 0.0 * tn[2];
    if (ln > K.cos_friction && t[1] < min_x) {
      lr |= 1u;
      lx0 = fmin(lx0, t[0]);
      lx1 = fmax(lx1, t[0]);
      lz0 = fmin(lz0, t[2]);
      lz1 = fmax(lz1, t[2]);
    }
    if (rn > K.cos_friction && t[1] > max_x) {
      lr |= 2u;
      rx0 = fmin(rx0, t[0]);
      rx1 = fmax(rx1, t[0]);
      rz0 = fmin(rz0, t[2]);
      rz1 = fmax(rz1, t[2]);
    }
  });
  lr = block_or(lr, s_u);
  if (lr) label = 1;
  if (lr == 3u) {
    lx0 = block_min(lx0, s_d);
    lx1 = block_max(lx1, s_d);
    lz0 = block_min(lz0, s_d);
    lz1 = block_max(lz1, s_d);
    rx0 = block_min(rx0, s_d);
    rx1 = block_max(rx1, s_d);
    rz0 = block_min(rz0, s_d);
    rz1 = block_max(rz1, s_d);
    const double top_y = fmin(lx1, rx1), bot_y = fmax(lx0, rx0);
    const double top_z = fmin(lz1, rz1), bot_z = fmax(lz0, rz0);
    long long nl = 0, nr = 0;
    for_each_entry(L, [&](double t0, double t1, int mult, int e) {
      if (!(t0 > bottom && t0 < top && t1 > left && t1 < right)) return;
      double t[3], tn[3];
      int m1;
      list_entry(L, e, t, tn, m1);
      const double ln = 0.0 * tn[0] + -1.0 * tn[1] + 0.0 * tn[2];
      const double rn = 0.0 * tn[0] + 1.0 * tn[1] + 0.0 * tn[2];
      const bool inb = t[0] >= bot_y && t[0] <= top_y && t[2] >= bot_z && t[2] <= top_z;
      if (ln > K.cos_friction && t[1] < min_x && inb) nl += mult;
      if (rn > K.cos_friction && t[1] > max_x && inb) nr += mult;
    });
    nl = block_sum(nl, s_l);
    nr = block_sum(nr, s_l);
    if (nl >= K.min_viable && nr >= K.min_viable) label = 2;
  }
  return true;
}

// HandSearch::reevaluateHypotheses (hand_search.cpp:66-134, 190-228): one
// workgroup per hand checks it again against the uploaded (ground-truth) cloud with the hand's own
// frame, depth and finger placement: evaluateFingers(points, top, idx), evaluateHand(idx), closing
// region, antipodal label.  labels[i] receives the label (1 = full antipodal grasp): a buffer of its
// own, since centre_kernel may still be reading counts[8 s + 5] on the side stream.
// the check of hand H against neighbourhood list s of P (the whole workgroup calls it) -> 0 none, 1 half, 2 full antipodal
__device__ inline int reeval_hand(const HandParams &P, int s, const gpd_hand *H, unsigned *s_u, double *s_d, long long *s_l) {
  const HandConsts &K = c_hand;
  const int tid = threadIdx.x;
  const int N = P.counts[8 * s + 0];
  const int idx = H->finger_placement_index;
  int label = 0;
  if (N > 0 && idx >= 0 && idx < K.nfp) {
    ListCtx L;
    L.nn = P.nn + (size_t)s * 6 * P.cap;
    L.cap = P.cap;
    L.N = N;
    L.hand_height = K.hand_height;
#pragma unroll
    for (int r = 0; r < 3; r++) L.sample[r] = H->sample[r];
#pragma unroll
    for (int i = 0; i < 9; i++) L.FR[i] = H->frame[i];
    L.ghost_mult = 0;
    L.ct0 = nullptr;
    L.ct1 = nullptr;
    L.ce = nullptr;
    L.kc = 0;
    long long kin = 0;
    for (int e = tid; e < N; e += 256) {
      double t[3], tn[3];
      int mult;
      if (list_entry(L, e, t, tn, mult)) kin++;
    }
    L.ghost_mult = N - (int)block_sum(kin, s_l);
    const double top = H->top, bottom = top - K.hand_depth;
    const double sl = K.spacing[idx], sr = K.spacing[K.nfp + idx];
    unsigned flags = 0;  // bit0 some x<top, bit1 some x<bottom, bit2 a finger of the pair is blocked
    for (int e = tid; e <= N; e += 256) {
      double t[3], tn[3];
      int mult;
      if (!list_entry(L, e, t, tn, mult)) continue;
      if (t[0] < top) {
        flags |= 1u;
        if (t[0] < bottom) flags |= 2u;
        if ((t[1] > sl && t[1] < sl + K.fw) || (t[1] > sr && t[1] < sr + K.fw)) flags |= 4u;
      }
    }
    flags = block_or(flags, s_u);
    if (flags == 1u) {
      double width;
      closing_region_label(L, N, top, bottom, sl + K.fw, sr, K, width, label, s_u, s_d, s_l);
    }
  }
  return label;
}

__global__ __launch_bounds__(256) void reeval_kernel(HandParams P) {
  __shared__ unsigned s_u[4];
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  const int s = blockIdx.x;
  gpd_hand *H = P.hands + s;
  const int label = reeval_hand(P, s, H, s_u, s_d, s_l);
  if (threadIdx.x == 0) {
    H->half_antipodal = label == 1;
    H->full_antipodal = label == 2;
    P.labels[s] = label == 2 ? 1 : 0;
  }
}

// gpd_hip_label_view: the same check for the candidates of a round, whose records are on the device already and whose
// neighbourhood lists exist once per hand SET (the hands of a set share their sample): candidate c reads list cand_list[c].
// labels8[c] = 1 for a full antipodal grasp, one byte per accumulated candidate.
__global__ __launch_bounds__(256) void label_kernel(HandParams P, const int32_t *__restrict__ cand_list, uint8_t *__restrict__ labels8) {
  __shared__ unsigned s_u[4];
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  const int c = blockIdx.x;
  gpd_hand *H = P.hands + c;
  const int label = reeval_hand(P, cand_list[c], H, s_u, s_d, s_l);
  if (threadIdx.x == 0) {
    H->half_antipodal = label == 1;
    H->full_antipodal = label == 2;
    labels8[c] = label == 2 ? 1 : 0;
  }
}

// The hand sets of a round's candidate records (set-major: the candidates of a set are neighbours): candidate c -> the ordinal of
// its set among the sets that have a candidate (cand_list), that set's sample -> sample_xyz[ordinal] (the query of its ground-truth
// neighbourhood), the number of such sets -> meta[2].  One workgroup: a round has a few thousand candidates.
__global__ __launch_bounds__(1024) void label_sets_kernel(const gpd_hand *__restrict__ recs, int n, int32_t *__restrict__ cand_list,
                                                          double *__restrict__ sample_xyz, int32_t *__restrict__ meta) {
  __shared__ int s_w[16];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int running = 0;
  for (int base = 0; base < n; base += 1024) {
    const int i = base + tid;
    const bool head = i < n && (i == 0 || recs[i].set_index != recs[i - 1].set_index);
    const unsigned long long mask = __ballot(head);
    if (lane == 0) s_w[wave] = __popcll(mask);
    __syncthreads();
    int before = running, total = 0;
    for (int w = 0; w < 16; w++) {
      before += w < wave ? s_w[w] : 0;
      total += s_w[w];
    }
    const int ord = before + __popcll(mask & ((1ull << lane) - 1ull)) + (head ? 1 : 0) - 1;  // the set of candidate 0 is a head
    if (i < n) cand_list[i] = ord;
    if (head)
      for (int r = 0; r < 3; r++) sample_xyz[3 * (size_t)ord + r] = recs[i].sample[r];
    running += total;
    __syncthreads();
  }
  if (tid == 0) meta[2] = running;
}

// what the host needs of a round: meta[0] = the largest ground-truth neighbourhood found (list capacity check), or -1: the lists
// are not the `lists` the plan counted, or -2 - f: the round's image kernels left the capacity flags f; meta[1] = positives among
// the round's n labels
__global__ __launch_bounds__(256) void label_meta_kernel(const int32_t *__restrict__ counts, int lists, const uint8_t *__restrict__ labels8, int n,
                                                         const int32_t *__restrict__ img_status, int32_t *__restrict__ meta) {
  __shared__ int s_worst, s_pos;
  if (threadIdx.x == 0) s_worst = s_pos = 0;
  __syncthreads();
  int worst = 0, pos = 0;
  for (int i = threadIdx.x; i < lists; i += 256) worst = max(worst, counts[8 * i + 3]);
  for (int i = threadIdx.x; i < n; i += 256) pos += labels8[i] != 0;
  atomicMax(&s_worst, worst);
  atomicAdd(&s_pos, pos);
  __syncthreads();
  if (threadIdx.x == 0) {
    const int flags = img_status[0];
    meta[0] = flags ? -2 - flags : meta[2] == lists ? s_worst : -1;
    meta[1] = s_pos;
  }
}

__global__ __launch_bounds__(256) void hand_eval_kernel(HandParams P) {
  __shared__ unsigned s_u[4];
  __shared__ double s_d[4];
  __shared__ long long s_l[4];
  const HandConsts &K = c_hand;
  // XCD-aware order (workgroup L runs on XCD L % 8, one L2 per XCD): all orientations of a sample
  // run on the same XCD, so its neighbourhood is fetched from HBM once, not once per XCD
  // (1.87 GB per launch before, 9x the algorithmic bytes).  L = 8 * (slots * g + slot) + xcd.
  const int xcd = blockIdx.x & 7, idx = blockIdx.x >> 3;
  const int s = (idx / K.slots) * 8 + xcd;
  const int slot = idx % K.slots;
  if (s >= P.num_samples) return;
  const int tid = threadIdx.x;
  const int N = P.counts[8 * s + 0];
  const int kf = P.counts[8 * s + 2];
  gpd_hand *H = P.hands + (size_t)s * K.slots + slot;
  const double *fr = P.frames + 12 * (size_t)s;
  // The 184-byte record is put together in LDS and stored by 46 lanes, one dword each: a gpd_hand on thread 0's
  // stack lives in scratch memory (184 B/lane), and writing it there and copying it out was a tenth of the kernel.
  constexpr int REC_DW = (int)(sizeof(gpd_hand) / 4);
  static_assert(sizeof(gpd_hand) % 4 == 0 && REC_DW <= 64, "record store");
  __shared__ gpd_hand s_rec;
  if (kf == 0 || N == 0) {  // no frame: the sample is dropped on the host
    if (tid < REC_DW) {
      uint32_t v = 0u;
      if (tid == (int)(offsetof(gpd_hand, finger_placement_index) / 4)) v = 0xffffffffu;  // -1
      if (tid == (int)(offsetof(gpd_hand, slot) / 4)) v = (uint32_t)slot;
      reinterpret_cast<uint32_t *>(H)[tid] = v;
    }
    if (tid == 0) P.fvalid[(size_t)s * K.slots + slot] = 0;
    return;
  }
  if (tid < REC_DW) reinterpret_cast<uint32_t *>(&s_rec)[tid] = 0u;  // ordered before thread 0's fields by the barriers below
  long long t_last = P.dbg ? clock64() : 0;
#define HTICK(k)                                  \
  if (P.dbg && tid == 0) {                        \
    const long long now_ = clock64();             \
    atomicAdd(&P.dbg[k], (unsigned long long)(now_ - t_last)); \
    t_last = now_;                                \
  }
  ListCtx L;
  L.nn = P.nn + (size_t)s * 6 * P.cap;
  L.cap = P.cap;
  L.N = N;
  L.hand_height = K.hand_height;
  // frame_ << normal, binormal, curvature (hand_set.cpp:39-40); frame_rot = frame_ * RB * R (:72)
  double F[9], FRB[9];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    L.sample[r] = fr[r];
    F[3 * r + 0] = fr[3 + r];
    F[3 * r + 1] = fr[6 + r];
    F[3 * r + 2] = fr[9 + r];
  }
  mat3mul(F, K.rot_binormal, FRB);
  mat3mul(FRB, K.rot[slot], L.FR);
  L.ghost_mult = 0;

  const int nfp = K.nfp;
  const double bite = K.init_bite;
  const double bottom0 = bite - K.hand_depth;
  // ---- pass 0: the one transform of all N points (PointList::transformToHandFrame +
  //      cropByHandHeight, point_list.cpp:22-55): in-height entries are compacted into LDS
  //      (forward / lateral coordinate, rank), every later pass reads those k entries instead of
  //      transforming the N points again (the kernel is fp64-VALU bound: k is ~0.3 N).
  __shared__ double s_t0[HE_COMPACT], s_t1[HE_COMPACT];
  __shared__ unsigned short s_e[HE_COMPACT];
  __shared__ int s_kc;
  __shared__ uint32_t s_lut[256];
  __shared__ double s_sp[32], s_spfw[32];
  if (tid == 0) s_kc = 0;
  s_lut[tid] = K.slot_lut[tid];
  if (tid < 32) {
    s_sp[tid] = K.spacing[tid];
    s_spfw[tid] = K.spfw[tid];
  }
  __syncthreads();
  L.ct0 = nullptr;
  L.ct1 = nullptr;
  L.ce = nullptr;
  L.kc = 0;
  // The points come from the sample's height list (written by neighbourhood_kernel's gather: the superset of every orientation's crop, one
  // 16-byte record per point); two rounds are in flight per thread.
  const float4 *hl = P.hl + (size_t)s * P.cap;
  const int NL = P.counts[8 * s + 6];
  constexpr int HE_R = 2;
  float4 cx[2][HE_R];
  auto request = [&](int i0, float4(&c)[HE_R]) {
#pragma unroll
    for (int q = 0; q < HE_R; q++) c[q] = hl[min(i0 + 256 * q + tid, NL - 1)];
  };
  auto consume = [&](int i0, const float4(&c)[HE_R]) {
#pragma unroll
    for (int q = 0; q < HE_R; q++) {
      const int i = i0 + 256 * q + tid;
      if (i0 + 256 * q >= NL) break;  // uniform
      double t[3] = {0, 0, 0};
      bool in = false;
      if (i < NL) {  // list_entry() on the listed coordinates: transformToHandFrame + the height test
        const double c0 = (double)c[q].x - L.sample[0], c1 = (double)c[q].y - L.sample[1], c2 = (double)c[q].z - L.sample[2];
#pragma unroll
        for (int r = 0; r < 3; r++) t[r] = L.FR[0 + r] * c0 + L.FR[3 + r] * c1 + L.FR[6 + r] * c2;
        in = t[2] > -1.0 * L.hand_height && t[2] < L.hand_height;
      }
      const unsigned long long ballot = __ballot(in);
      if (ballot) {
        int base = 0;
        if ((tid & 63) == 0) base = atomicAdd(&s_kc, __popcll(ballot));
        base = __builtin_amdgcn_readfirstlane(base);  // every lane is active here and lane 0 holds it
        if (in) {
          const int cpos = base + __popcll(ballot & ((1ull << (tid & 63)) - 1ull));
          if (cpos < HE_COMPACT) {
            s_t0[cpos] = t[0];
            s_t1[cpos] = t[1];
            s_e[cpos] = (unsigned short)__float_as_int(c[q].w);
          }
        }
      }
    }
  };
  if (NL > 0) {
    request(0, cx[0]);
    for (int i0 = 0; i0 < NL; i0 += 2 * 256 * HE_R) {
      if (i0 + 256 * HE_R < NL) request(i0 + 256 * HE_R, cx[1]);
      consume(i0, cx[0]);
      if (i0 + 256 * HE_R >= NL) break;
      if (i0 + 2 * 256 * HE_R < NL) request(i0 + 2 * 256 * HE_R, cx[0]);
      consume(i0 + 256 * HE_R, cx[1]);
    }
  }
  __syncthreads();
  HTICK(0);
  const int k = s_kc;
  L.ghost_mult = N - k;
  if (P.dbg && tid == 0) {
    atomicAdd(&P.dbg[8], (unsigned long long)N);
    atomicAdd(&P.dbg[9], (unsigned long long)k);
  }
  if (k <= HE_COMPACT && N <= 65535) {  // (the table's neighbour ranks are 16 bits wide: a longer list is walked in full)
    L.ct0 = s_t0;
    L.ct1 = s_t1;
    L.ce = s_e;
    L.kc = k;
  }
  // ---- pass 1: finger collision masks at init_bite (finger_hand.cpp:26-73)
  unsigned blocked = 0, flags = 0;  // flags bit0: some x<bite, bit1: some x<bottom
  // isGapFree for all 2 nfp slots: the slots an entry can block come from the lookup table (none, one, rarely
  // two), the reference's own comparisons decide — twenty pairs of comparisons per entry were 31 of the kernel's
  // 85 kcycles per workgroup
  for_each_entry(L, [&](double t0, double t1, int, int) {
    if (t0 < bite) {
      flags |= 1u;
      if (t0 < bottom0) flags |= 2u;
      const double u = (t1 - K.lut_base) * K.lut_inv;
      const int q = u < 0.0 ? 0 : (u >= 255.0 ? 255 : (int)u);
      unsigned m = s_lut[q] & ~blocked;
      while (m) {
        const int i = __ffs(m) - 1;
        m &= m - 1u;
        if (t1 > s_sp[i] && t1 < s_spfw[i]) blocked |= 1u << i;
      }
    }
  });
  blocked = block_or(blocked, s_u);
  flags = block_or(flags, s_u);
  HTICK(1);
  unsigned fingers = 0;
  if ((flags & 1u) && !(flags & 2u)) fingers = ~blocked & ((1u << (2 * nfp)) - 1u);
  unsigned hand = fingers & (fingers >> nfp) & ((1u << nfp) - 1u);

  double top = bite, bottom = bottom0, center = 0.0;
  int fidx = hand ? (__ffs(hand) - 1) : -1;
  bool valid = false;
  double width = 0.0;
  int label = 0;
  if (hand) {
    // chooseMiddleHand (finger_hand.cpp:89-105): idx[ceil(m/2) - 1]
    const int mcount = __popc(hand);
    const int want = (mcount + 1) / 2 - 1;
    int mid = -1, seen = 0;
    for (int i = 0; i < nfp; i++)
      if (hand & (1u << i)) {
        if (seen == want) {
          mid = i;
          break;
        }
        seen++;
      }
    if (K.deepen) {
      // ---- pass 2: deepenHand (finger_hand.cpp:107-139), 32 depths at once (the shipped geometry has ten; a longer
      //      finger simply takes another round of the loop — the reference has no bound on hand_depth)
      const double sl = K.spacing[mid], sr = K.spacing[nfp + mid];
      bool deeper = true;
      for (int j0 = 0; j0 < K.num_deepen && deeper; j0 += 32) {
        const int nj = min(32, K.num_deepen - j0);
        unsigned m_any = 0, m_back = 0, m_blk = 0;
        for_each_entry(L, [&](double t0, double t1, int, int) {
          const bool blk = (t1 > sl && t1 < sl + K.fw) || (t1 > sr && t1 < sr + K.fw);
          for (int j = 0; j < nj; j++) {
            const double d = K.depths[j0 + j];
            if (t0 < d) {
              m_any |= 1u << j;
              if (t0 < d - K.hand_depth) m_back |= 1u << j;
              if (blk) m_blk |= 1u << j;
            }
          }
        });
        m_any = block_or(m_any, s_u);
        m_back = block_or(m_back, s_u);
        m_blk = block_or(m_blk, s_u);
        for (int j = 0; j < nj; j++) {
          const bool ok = (m_any >> j & 1u) && !(m_back >> j & 1u) && !(m_blk >> j & 1u);
          if (!ok) {
            deeper = false;
            break;
          }
          top = K.depths[j0 + j];
          bottom = K.depths[j0 + j] - K.hand_depth;
        }
      }
      HTICK(2);
      hand = 1u << mid;
    }
    // ---- pass 3-5: closing region, width, antipodal label
    const double left = K.spacing[mid] + K.fw;
    const double right = K.spacing[nfp + mid];
    const double center_c = 0.5 * (left + right);
    if (closing_region_label(L, N, top, bottom, left, right, K, width, label, s_u, s_d, s_l)) {
      valid = true;
      center = center_c;
      fidx = __ffs(hand) - 1;
    } else {
      // closing region empty: the hand keeps what Hand() saw before deepening (hand_set.cpp:89-109)
      top = bite;
      bottom = bottom0;
      center = 0.0;
      fidx = __ffs(fingers & (fingers >> nfp) & ((1u << nfp) - 1u)) - 1;
    }
    HTICK(3);
  }
  if (tid == 0) {
    gpd_hand &h = s_rec;
#pragma unroll
    for (int r = 0; r < 3; r++) h.sample[r] = L.sample[r];
#pragma unroll
    for (int i = 0; i < 9; i++) h.frame[i] = L.FR[i];
    h.top = top;
    h.bottom = bottom;
    h.center = center;
    // Hand::calculateGraspPositions (hand.cpp:41-45)
#pragma unroll
    for (int r = 0; r < 3; r++) h.position[r] = (L.FR[3 * r + 0] * bottom + L.FR[3 * r + 1] * center + L.FR[3 * r + 2] * 0.0) + L.sample[r];
    h.grasp_width = width;
    h.finger_placement_index = fidx;
    h.set_index = s;
    h.slot = slot;
    h.valid = valid ? 1 : 0;
    h.half_antipodal = label >= 1;
    h.full_antipodal = label == 2;
    // detectGrasps step 2 (grasp_detector.cpp:238): the workspace / aperture filter only clears is_valid, the
    // record itself stays as the search produced it
    P.fvalid[(size_t)s * K.slots + slot] = (valid && workspace_ok(K.filter, h)) ? 1 : 0;
  }
  __syncthreads();
  if (tid < REC_DW) reinterpret_cast<uint32_t *>(H)[tid] = reinterpret_cast<const uint32_t *>(&s_rec)[tid];
  HTICK(4);
#undef HTICK
}

static ConstBlock g_hand_block;  // c_hand on every device (const_block.h)

static int upload_hand_consts(const gpd_params &p, const HostConsts &hc, int slots, hipStream_t stream,
                              std::unique_lock<std::mutex> &lock) {
  HandConsts hk;
  std::memset(&hk, 0, sizeof(hk));
  std::memcpy(hk.rot, hc.rot, sizeof(hk.rot));
  std::memcpy(hk.rot_binormal, hc.rot_binormal, sizeof(hk.rot_binormal));
  std::memcpy(hk.spacing, hc.finger_spacing, sizeof(hk.spacing));
  std::memcpy(hk.depths, hc.deepen_depths, sizeof(hk.depths));
  {
    const int nslots = 2 * p.num_finger_placements;
    double lo = DBL_MAX, hi = -DBL_MAX;
    for (int i = 0; i < nslots; i++) {
      hk.spfw[i] = hk.spacing[i] + p.finger_width;
      lo = std::fmin(lo, hk.spacing[i]);
      hi = std::fmax(hi, hk.spfw[i]);
    }
    const double w = (hi - lo) / 256.0;
    hk.lut_base = lo;
    hk.lut_inv = w > 0.0 ? 1.0 / w : 0.0;
    for (int c = 0; c < 256; c++) {
      const double c_lo = c == 0 ? -DBL_MAX : lo + (c - 0.01) * w - 1e-12;
      const double c_hi = c == 255 ? DBL_MAX : lo + (c + 1.01) * w + 1e-12;
      uint32_t m = 0;
      for (int i = 0; i < nslots; i++)
        if (hk.spacing[i] < c_hi && hk.spfw[i] > c_lo) m |= 1u << i;
      hk.slot_lut[c] = w > 0.0 ? m : (nslots >= 32 ? 0xffffffffu : (1u << nslots) - 1u);
    }
  }
  hk.num_deepen = hc.num_deepen;
  hk.nfp = p.num_finger_placements;
  hk.slots = slots;
  hk.deepen = p.deepen_hand;
  hk.min_viable = p.min_viable;
  hk.cos_friction = hc.cos_friction;
  hk.fw = p.finger_width;
  hk.hand_depth = p.hand_depth;
  hk.hand_height = p.hand_height;
  hk.init_bite = p.init_bite;
  hk.filter = filter_consts(p);
  return g_hand_block.load(c_hand, &hk, sizeof(hk), stream, lock);
}

// ---------------------------------------------------------------------------
// Host side: one enqueue per kernel.  A kernel that reads c_hand is launched under the lock of the block.
// ---------------------------------------------------------------------------
// what every hand kernel reads: the lists of s at capacity cap and the records; the fields of one kernel alone are off
static HandParams hand_params(const SearchState &s, int cap, int num_samples, gpd_hand *hands) {
  HandParams hp;
  hp.counts = s.d_counts;
  hp.nn = s.d_nn;
  hp.frames = s.d_frames;
  hp.cap = cap;
  hp.hands = hands;
  hp.fvalid = nullptr;
  hp.hl = nullptr;
  hp.radius = 0.0;
  hp.num_samples = num_samples;
  hp.labels = nullptr;
  hp.dbg = nullptr;
  return hp;
}

int hands_enqueue_eval(const gpd_params &p, const HostConsts &hc, SearchState &s, int cap, int S, hipStream_t stream) {
  const int slots = p.num_hand_axes * p.num_orientations;
  std::unique_lock<std::mutex> consts_lock;  // held until the kernel that reads c_hand is enqueued
  const int rc = upload_hand_consts(p, hc, slots, stream, consts_lock);
  if (rc) return rc;
  HandParams hp = hand_params(s, cap, S, s.d_hands);
  hp.fvalid = s.d_fvalid;
  hp.hl = s.d_hl;
  hp.radius = hc.nn_radius_hands * 1.001 + 1e-6;
  static unsigned long long *d_hedbg = nullptr;
  if (prof_env("GPD_HE_TIMING")) {
    if (!d_hedbg) HIP_RET(hipMalloc(&d_hedbg, 16 * sizeof(unsigned long long)));
    HIP_RET(hipMemsetAsync(d_hedbg, 0, 16 * sizeof(unsigned long long), stream));
    hp.dbg = d_hedbg;
  }
  hand_eval_kernel<<<((S + 7) / 8) * 8 * slots, 256, 0, stream>>>(hp);
  HIP_RET(hipGetLastError());
  if (hp.dbg) {
    unsigned long long h[16];
    HIP_RET(hipMemcpyAsync(h, d_hedbg, sizeof(h), hipMemcpyDeviceToHost, stream));
    HIP_RET(hipStreamSynchronize(stream));
    static const char *names[5] = {"transform+compact", "finger masks", "deepen", "closing region", "record"};
    const double wg = (double)S * slots;
    for (int i = 0; i < 5; i++) fprintf(stderr, "[he-timing] %-18s %8.2f kcycles/workgroup\n", names[i], (double)h[i] / wg / 1e3);
    fprintf(stderr, "[he-timing] mean N %.0f, mean in-height k %.0f\n", (double)h[8] / wg, (double)h[9] / wg);
  }
  return GPD_OK;
}

int hands_enqueue_reeval(const gpd_params &p, const HostConsts &hc, SearchState &s, int cap, int n, hipStream_t stream) {
  std::unique_lock<std::mutex> consts_lock;
  const int rc = upload_hand_consts(p, hc, p.num_hand_axes * p.num_orientations, stream, consts_lock);
  if (rc) return rc;
  HandParams hp = hand_params(s, cap, n, s.d_hands);
  hp.labels = s.d_labels;
  reeval_kernel<<<n, 256, 0, stream>>>(hp);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

int hands_enqueue_label(const gpd_params &p, const HostConsts &hc, SearchState &gs, int cap, int lists, gpd_hand *d_recs, int n,
                        const int32_t *d_cand_list, uint8_t *d_labels8, hipStream_t stream) {
  std::unique_lock<std::mutex> consts_lock;
  const int rc = upload_hand_consts(p, hc, p.num_hand_axes * p.num_orientations, stream, consts_lock);
  if (rc) return rc;
  label_kernel<<<n, 256, 0, stream>>>(hand_params(gs, cap, lists, d_recs), d_cand_list, d_labels8);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

int hands_enqueue_label_sets(const gpd_hand *d_recs, int n, int32_t *d_cand_list, double *d_sample_xyz, int32_t *d_meta, hipStream_t stream) {
  label_sets_kernel<<<1, 1024, 0, stream>>>(d_recs, n, d_cand_list, d_sample_xyz, d_meta);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

int hands_enqueue_label_meta(const int32_t *d_counts, int lists, const uint8_t *d_labels8, int n, const int32_t *d_img_status, int32_t *d_meta,
                             hipStream_t stream) {
  label_meta_kernel<<<1, 256, 0, stream>>>(d_counts, lists, d_labels8, n, d_img_status, d_meta);
  HIP_RET(hipGetLastError());
  return GPD_OK;
}

}  // namespace gpd
