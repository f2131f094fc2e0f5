// Training on several replicas (train_group.hip): the definition.  Plain C++ with no HIP in it, compiled without FMA
// contraction: gpd_hip_train_group_mean / _slices / _schedule (host only) are this code, gpd_hip_train_group_steps executes the
// schedule's list as it stands and group_sum_kernel is mean()'s expression over one slice.
//
// The gradient every replica's solver applies is the mean of the G replicas' gradients in RANK order,
//     s = g_0;  s = s + g_r  (r = 1 .. G - 1);  out = s * (float)(1.0 / G)
// every operation a rounded f32 operation — what averaging gpd_hip_train_gradients over the replicas on the host and handing
// the mean to gpd_hip_train_apply computes.  The step's loss is the same expression over the replicas' losses.
//
// The device entry computes it as a reduce-scatter and an all-gather.  The parameter-sized buffer [0, n) is cut into G
// contiguous slices; replica o ("owner") sums slice o.  Per step, with three events per replica (grad, sum, gathered):
//   (a) replica r: forward and backward into its gradient buffer, record grad[r]
//   (b) owner o:   wait grad[r] (r != o); copy slice o of every peer's gradient buffer into its gather rows; sum its own slice
//                  with the rows in rank order, in place; record sum[o]
//   (c) replica r: wait sum[o] (o != r); copy slice o of owner o's buffer into its own; record gathered[r]
//   (d) replica r: the solver's update from its now complete buffer
//   (e) next step: replica r waits gathered[o] (o != r) before its backward pass writes the buffer its peers read in (b), (c)
// A stream's wait on an event binds to the record that has been ENQUEUED last: a wait enqueued ahead of its record passes at
// once.  The order of the list is therefore part of its correctness, and one host thread enqueues it in list order.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gpd {
namespace group {

constexpr int kMaxReplicas = 16;

inline float mean_weight(int G) { return (float)(1.0 / (double)G); }

inline void mean(const float *const *g, int G, size_t n, float *out) {
  const float w = mean_weight(G);
  for (size_t i = 0; i < n; i++) {
    float s = g[0][i];
    for (int r = 1; r < G; r++) s = s + g[r][i];
    out[i] = G > 1 ? s * w : s;  // G = 1: the input's bits (w is 1)
  }
}

// first[o] .. first[o + 1]: slice o.  The ceil(n / 4) quads (16 bytes: a dwordx4 lane) are dealt out evenly, the larger shares
// to the last owners, so that the slice with the short last quad is never the smallest by more than a quad.
inline void slices(size_t n, int G, long long *first) {
  const size_t quads = (n + 3) / 4, base = quads / (size_t)G, rem = quads % (size_t)G;
  size_t q = 0;
  for (int o = 0; o < G; o++) {
    first[o] = (long long)(4 * q);
    q += base + ((size_t)o >= (size_t)G - rem ? 1 : 0);
  }
  first[G] = (long long)n;
}

enum Kind : int32_t { kBackward = 0, kWait = 1, kRecord = 2, kCopy = 3, kSum = 4, kUpdate = 5 };

// One operation on replica `stream`'s stream.  peer, slice, event: -1 where the kind has none.
//   kBackward  forward and backward of the replica's next batch (the n-th kBackward of a stream is step n)
//   kWait      on `event`
//   kRecord    of `event`
//   kCopy      slice `slice` of replica `peer`'s gradient buffer: slice == stream (the replica's own slice) into the gather row
//              of `peer`, any other slice (the peer's, summed) to the same place of the replica's own buffer
//   kSum       the replica's own slice: its buffer and the gather rows in rank order, times 1 / G, in place
//   kUpdate    the solver's update
struct Op {
  int32_t kind, stream, peer, slice, event;
};
static_assert(sizeof(Op) == 20, "Op");

inline int event_grad(int, int r) { return r; }
inline int event_sum(int G, int o) { return G + o; }
inline int event_gathered(int G, int r) { return 2 * G + r; }
inline int num_events(int G) { return 3 * G; }

// ops == nullptr or capacity too small: only the count
inline int schedule(int G, int num_steps, Op *ops, int capacity) {
  int k = 0;
  auto put = [&](int kind, int stream, int peer, int slice, int event) {
    if (ops && k < capacity) ops[k] = Op{kind, stream, peer, slice, event};
    k++;
  };
  for (int s = 0; s < num_steps; s++) {
    for (int r = 0; r < G; r++) {  // (e), (a)
      if (s > 0)
        for (int o = 0; o < G; o++)
          if (o != r) put(kWait, r, -1, -1, event_gathered(G, o));
      put(kBackward, r, -1, -1, -1);
      if (G > 1) put(kRecord, r, -1, -1, event_grad(G, r));
    }
    for (int o = 0; o < G && G > 1; o++) {  // (b)
      for (int r = 0; r < G; r++)
        if (r != o) {
          put(kWait, o, -1, -1, event_grad(G, r));
          put(kCopy, o, r, o, -1);
        }
      put(kSum, o, -1, o, -1);
      put(kRecord, o, -1, -1, event_sum(G, o));
    }
    for (int r = 0; r < G && G > 1; r++) {  // (c)
      for (int o = 0; o < G; o++)
        if (o != r) {
          put(kWait, r, -1, -1, event_sum(G, o));
          put(kCopy, r, o, o, -1);
        }
      put(kRecord, r, -1, -1, event_gathered(G, r));
    }
    for (int r = 0; r < G; r++) put(kUpdate, r, -1, -1, -1);  // (d)
  }
  return k;
}

// the gather row of replica r in owner o's block of G - 1 rows (constexpr: group_sum_kernel calls it as it stands)
constexpr int gather_row(int o, int r) { return r < o ? r : r - 1; }

}  // namespace group
}  // namespace gpd
