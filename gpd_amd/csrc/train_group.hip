// Training on several replicas: G trainers, each on a context of its own — on G devices, or several on one —
// step together, and the gradient every replica's solver applies is group::mean (group_model.h) of the G gradients.  The data
// stay on the devices: a reduce-scatter and an all-gather per step, each replica moving 2 (G - 1) / G of a buffer.
//
// gpd_hip_train_group_steps executes group::schedule's list, in list order, from the calling thread alone: a stream's wait on
// an event binds to the record enqueued last, so a wait enqueued ahead of its record would pass at once and the race would be
// silent.  Kernels read and write only memory of their own device; data crosses between replicas by hipMemcpyPeerAsync on
// the destination's stream, which works with or without peer access (never enabled here) and is an ordinary device-to-device
// copy when both replicas share a device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <vector>

#include "context.h"
#include "buffers.h"
#include "group_model.h"
#include "train.h"

using namespace gpd;

namespace {

// the owner's slice: own[0 .. n) and the G - 1 gather rows (row stride `row` floats, a multiple of 4) added in rank order — the
// owner's own values at rank o — then the one multiply; in place.  A dwordx4 lane per 4 floats, the n % 4 floats behind the
// last quad by a lane each.  Memory-bound: G reads and one write per float.
__global__ void __launch_bounds__(256) group_sum_kernel(float *__restrict__ own, const float *__restrict__ gather, size_t row, int G, int o,
                                                        size_t n, float w) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, nq = n / 4;
  if (i < nq) {
    float4 *own4 = reinterpret_cast<float4 *>(own);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int r = 0; r < G; r++) {
      const float4 v = r == o ? own4[i] : reinterpret_cast<const float4 *>(gather + (size_t)group::gather_row(o, r) * row)[i];
      if (r == 0) {
        s = v;
      } else {
        s.x = s.x + v.x;
        s.y = s.y + v.y;
        s.z = s.z + v.z;
        s.w = s.w + v.w;
      }
    }
    own4[i] = make_float4(s.x * w, s.y * w, s.z * w, s.w * w);
  } else if (i - nq < n - 4 * nq) {
    const size_t e = 4 * nq + (i - nq);
    float s = 0.f;
    for (int r = 0; r < G; r++) {
      const float v = r == o ? own[e] : gather[(size_t)group::gather_row(o, r) * row + e];
      s = r == 0 ? v : s + v;
    }
    own[e] = s * w;
  }
}

// *count += the 32-bit words of a[0 .. n) that differ from b's: a ballot and a popcount per word of the lane's quad (the
// n % 4 words behind the last quad by a lane each), one atomic per wave
__global__ void __launch_bounds__(256) group_diff_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b, size_t n,
                                                         unsigned long long *count) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x, nq = n / 4;
  bool d[4] = {false, false, false, false};
  if (i < nq) {
    const uint4 x = reinterpret_cast<const uint4 *>(a)[i], y = reinterpret_cast<const uint4 *>(b)[i];
    d[0] = x.x != y.x, d[1] = x.y != y.y, d[2] = x.z != y.z, d[3] = x.w != y.w;
  } else if (i - nq < n - 4 * nq) {
    const size_t e = 4 * nq + (i - nq);
    d[0] = a[e] != b[e];
  }
  unsigned long long c = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) c += (unsigned long long)__popcll(__ballot(d[j]));
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

unsigned blocks_for(size_t n) { return (unsigned)((n / 4 + 3 + 255) / 256); }

bool same_params(const gpd_train_params &a, const gpd_train_params &b) {
  return a.channels == b.channels && a.lr == b.lr && a.beta1 == b.beta1 && a.beta2 == b.beta2 && a.eps == b.eps &&
         a.weight_decay == b.weight_decay && a.input_scale == b.input_scale;
}

bool same_recipe(const gpd_train_recipe &a, const gpd_train_recipe &b) {
  if (a.network != b.network || a.solver != b.solver || a.momentum != b.momentum || a.lr_policy != b.lr_policy || a.stepsize != b.stepsize ||
      a.gamma != b.gamma || a.power != b.power)
    return false;
  for (int i = 0; i < 8; i++)
    if (a.lr_mult[i] != b.lr_mult[i] || a.decay_mult[i] != b.decay_mult[i]) return false;
  return true;
}

}  // namespace

struct gpd_hip_train_group {
  int G = 0;
  std::vector<gpd_hip_trainer *> t;
  size_t n = 0;                                 // floats of a parameter-sized buffer
  long long first[group::kMaxReplicas + 1] = {0};
  size_t row = 0;                               // floats of a gather row: the largest slice, rounded up to a quad
  std::vector<float *> gather;                  // per replica, on its device: [G - 1][row]
  std::vector<unsigned long long *> d_count;    // per replica: group_diff_kernel's counter
  std::vector<hipEvent_t> ev;                   // group::num_events(G): event e on the device of replica e % G
  std::vector<group::Op> ops;
  std::vector<float> h_loss;                    // [G][steps of an enqueue]
  long long bytes[2] = {0, 0};                  // of the last call: between replicas, host <-> device
  int current = -1;                             // the device made current last
};

namespace {

hipError_t use_device(gpd_hip_train_group *g, int r) {
  const int dev = g->t[(size_t)r]->device;
  if (dev == g->current) return hipSuccess;
  g->current = dev;
  return hipSetDevice(dev);
}

size_t slice_size(const gpd_hip_train_group *g, int o) { return (size_t)(g->first[o + 1] - g->first[o]); }

// every stream of the group has run dry: the first error, the others' waited for all the same
hipError_t sync_all(gpd_hip_train_group *g) {
  hipError_t first = hipSuccess;
  for (int r = 0; r < g->G; r++) {
    hipError_t e = use_device(g, r);
    if (e == hipSuccess) e = hipStreamSynchronize(g->t[(size_t)r]->stream);
    if (first == hipSuccess) first = e;
  }
  return first;
}

hipError_t copy_between(gpd_hip_train_group *g, int dst_r, void *dst, int src_r, const void *src, size_t bytes) {
  if (!bytes) return hipSuccess;
  g->bytes[0] += (long long)bytes;
  return hipMemcpyPeerAsync(dst, g->t[(size_t)dst_r]->device, src, g->t[(size_t)src_r]->device, bytes, g->t[(size_t)dst_r]->stream);
}

// one operation of the schedule; step[r]: the batches replica r has run in this enqueue
hipError_t enqueue_op(gpd_hip_train_group *g, const group::Op &op, int batch, std::vector<int> &step) {
  const int r = op.stream;
  gpd_hip_trainer *t = g->t[(size_t)r];
  hipError_t e = use_device(g, r);
  if (e != hipSuccess) return e;
  int k = 0;
  switch (op.kind) {
    case group::kBackward: {
      const int s = step[(size_t)r]++;
      enqueue_gradients(t, t->d_idx + (size_t)s * batch, batch, t->d_loss + s, false, k);
      return hipGetLastError();
    }
    case group::kWait: return hipStreamWaitEvent(t->stream, g->ev[(size_t)op.event], 0);
    case group::kRecord: return hipEventRecord(g->ev[(size_t)op.event], t->stream);
    case group::kCopy: {
      const size_t at = (size_t)g->first[op.slice], cnt = slice_size(g, op.slice);
      float *dst = op.slice == r ? g->gather[(size_t)r] + (size_t)group::gather_row(r, op.peer) * g->row : t->d_g + at;
      return copy_between(g, r, dst, op.peer, g->t[(size_t)op.peer]->d_g + at, cnt * sizeof(float));
    }
    case group::kSum: {
      const size_t cnt = slice_size(g, op.slice);
      if (!cnt) return hipSuccess;
      hipLaunchKernelGGL(group_sum_kernel, dim3(blocks_for(cnt)), dim3(256), 0, t->stream, t->d_g + g->first[op.slice], g->gather[(size_t)r], g->row,
                         g->G, r, cnt, group::mean_weight(g->G));
      return hipGetLastError();
    }
    case group::kUpdate:
      enqueue_update(t, false, k);
      return hipGetLastError();
    default: return hipErrorInvalidValue;
  }
}

int fail_hip(gpd_hip_train_group *g, const char *who, hipError_t e) {
  (void)sync_all(g);  // nothing of the group is left running
  (void)hipGetLastError();
  set_error("%s: %s", who, hipGetErrorString(e));
  return GPD_ERR_HIP;
}

}  // namespace

extern "C" {

int gpd_hip_train_group_mean(const float *const *g, int G, size_t n, float *out) {
  if (!g || G < 1 || G > group::kMaxReplicas || (n > 0 && !out)) {
    set_error("gpd_hip_train_group_mean: a null argument, or %d gradients (1 .. %d)", G, group::kMaxReplicas);
    return GPD_ERR_INVALID;
  }
  for (int r = 0; r < G; r++)
    if (n > 0 && !g[r]) {
      set_error("gpd_hip_train_group_mean: gradient %d is null", r);
      return GPD_ERR_INVALID;
    }
  group::mean(g, G, n, out);
  return GPD_OK;
}

int gpd_hip_train_group_slices(size_t n, int G, long long *first) {
  if (!first || G < 1 || G > group::kMaxReplicas) {
    set_error("gpd_hip_train_group_slices: a null argument, or %d replicas (1 .. %d)", G, group::kMaxReplicas);
    return GPD_ERR_INVALID;
  }
  group::slices(n, G, first);
  return GPD_OK;
}

int gpd_hip_train_group_schedule(int G, int num_steps, void *ops, int capacity, int *num) {
  if (!num || G < 1 || G > group::kMaxReplicas || num_steps < 0 || capacity < 0) {
    set_error("gpd_hip_train_group_schedule: a null argument, %d replicas (1 .. %d) or a negative count", G, group::kMaxReplicas);
    return GPD_ERR_INVALID;
  }
  const long long per = group::schedule(G, 1, nullptr, 0) + (long long)G * (G - 1);  // a later step has the waits of (e) too
  if (per * num_steps > 0x7fffffffll) {
    set_error("gpd_hip_train_group_schedule: %d steps of %d replicas are more operations than an int counts", num_steps, G);
    return GPD_ERR_CAPACITY;
  }
  *num = group::schedule(G, num_steps, static_cast<group::Op *>(ops), ops ? capacity : 0);
  if (ops && *num > capacity) {
    set_error("gpd_hip_train_group_schedule: %d operations, room for %d", *num, capacity);
    return GPD_ERR_CAPACITY;
  }
  return GPD_OK;
}

int gpd_hip_train_group_create(gpd_hip_trainer *const *trainers, int num, gpd_hip_train_group **out) {
  if (!trainers || !out || num < 1 || num > group::kMaxReplicas) {
    set_error("gpd_hip_train_group_create: a null argument, or %d trainers (1 .. %d)", num, group::kMaxReplicas);
    return GPD_ERR_INVALID;
  }
  for (int r = 0; r < num; r++) {
    if (!trainers[r]) {
      set_error("gpd_hip_train_group_create: trainer %d is null", r);
      return GPD_ERR_INVALID;
    }
    for (int q = 0; q < r; q++) {
      if (trainers[q] == trainers[r]) {
        set_error("gpd_hip_train_group_create: trainer %d is trainer %d again", r, q);
        return GPD_ERR_INVALID;
      }
      if (trainers[q]->stream == trainers[r]->stream) {
        set_error("gpd_hip_train_group_create: trainers %d and %d share a context; every replica needs one of its own", q, r);
        return GPD_ERR_INVALID;
      }
    }
    if (trainers[r]->p.channels != trainers[0]->p.channels) {
      set_error("gpd_hip_train_group_create: trainer %d has %d channels, trainer 0 has %d", r, trainers[r]->p.channels, trainers[0]->p.channels);
      return GPD_ERR_INVALID;
    }
    const gpd_lenet_shape &sr = trainers[r]->shape, &s0 = trainers[0]->shape;
    if (sr.conv1_out != s0.conv1_out || sr.conv2_out != s0.conv2_out || sr.fc1_out != s0.fc1_out || sr.fc2_out != s0.fc2_out) {
      set_error("gpd_hip_train_group_create: trainer %d trains a network of widths %d, %d, %d, %d, trainer 0 one of %d, %d, %d, %d", r, sr.conv1_out,
                sr.conv2_out, sr.fc1_out, sr.fc2_out, s0.conv1_out, s0.conv2_out, s0.fc1_out, s0.fc2_out);
      return GPD_ERR_INVALID;
    }
    if (!same_params(trainers[r]->p, trainers[0]->p)) {
      set_error("gpd_hip_train_group_create: the gpd_train_params of trainer %d differ from trainer 0's in more than max_batch", r);
      return GPD_ERR_INVALID;
    }
    if (!same_recipe(trainers[r]->r, trainers[0]->r)) {
      set_error("gpd_hip_train_group_create: the recipe of trainer %d differs from trainer 0's", r);
      return GPD_ERR_INVALID;
    }
  }
  gpd_hip_train_group *g = new gpd_hip_train_group();
  g->G = num;
  g->t.assign(trainers, trainers + num);
  g->n = trainers[0]->total;
  group::slices(g->n, num, g->first);
  for (int o = 0; o < num; o++) g->row = std::max(g->row, (slice_size(g, o) + 3) / 4 * 4);
  g->gather.assign((size_t)num, nullptr);
  g->d_count.assign((size_t)num, nullptr);
  g->ev.assign((size_t)group::num_events(num), nullptr);
  hipError_t e = hipSuccess;
  for (int r = 0; r < num && e == hipSuccess; r++) {
    e = use_device(g, r);
    if (e == hipSuccess) e = device_alloc(g->gather[(size_t)r], std::max<size_t>((size_t)(num - 1) * g->row, 4));
    if (e == hipSuccess) e = device_alloc(g->d_count[(size_t)r], 1);
    for (int j = 0; j < 3 && e == hipSuccess; j++) e = hipEventCreateWithFlags(&g->ev[(size_t)(j * num + r)], hipEventDisableTiming);
  }
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("gpd_hip_train_group_create: %s", hipGetErrorString(e));
    gpd_hip_train_group_destroy(g);
    return GPD_ERR_HIP;
  }
  *out = g;
  return GPD_OK;
}

void gpd_hip_train_group_destroy(gpd_hip_train_group *g) {
  if (!g) return;
  g->current = -1;
  (void)sync_all(g);
  for (int r = 0; r < g->G; r++) {
    (void)use_device(g, r);
    device_release(g->gather[(size_t)r], g->d_count[(size_t)r]);
    for (int j = 0; j < 3; j++)
      if (g->ev[(size_t)(j * g->G + r)]) (void)hipEventDestroy(g->ev[(size_t)(j * g->G + r)]);
  }
  delete g;
}

int gpd_hip_train_group_broadcast(gpd_hip_train_group *g, int src) {
  if (!g || src < 0 || src >= g->G) {
    set_error("gpd_hip_train_group_broadcast: a null group, or source %d of %d replicas", src, g ? g->G : 0);
    return GPD_ERR_INVALID;
  }
  g->current = -1;
  g->bytes[0] = g->bytes[1] = 0;
  hipError_t e = sync_all(g);
  gpd_hip_trainer *s = g->t[(size_t)src];
  const size_t bytes = g->n * sizeof(float);
  for (int r = 0; r < g->G && e == hipSuccess; r++) {
    if (r == src) continue;
    gpd_hip_trainer *t = g->t[(size_t)r];
    e = use_device(g, r);
    if (e == hipSuccess) e = copy_between(g, r, t->d_p, src, s->d_p, bytes);
    if (e == hipSuccess) e = copy_between(g, r, t->d_m, src, s->d_m, bytes);
    if (e == hipSuccess && s->d_v) e = copy_between(g, r, t->d_v, src, s->d_v, bytes);
  }
  if (e == hipSuccess) e = sync_all(g);
  if (e != hipSuccess) return fail_hip(g, "gpd_hip_train_group_broadcast", e);
  for (int r = 0; r < g->G; r++) g->t[(size_t)r]->step = s->step;
  return GPD_OK;
}

int gpd_hip_train_group_steps(gpd_hip_train_group *g, const int32_t *const *indices, int num_steps, int batch, float *losses,
                              float *replica_losses) {
  if (!g || !indices || num_steps < 0 || (num_steps > 0 && !losses)) {
    set_error("gpd_hip_train_group_steps: bad argument");
    return GPD_ERR_INVALID;
  }
  const int G = g->G;
  for (int r = 0; r < G; r++) {
    const gpd_hip_trainer *t = g->t[(size_t)r];
    if (!indices[r]) {
      set_error("gpd_hip_train_group_steps: replica %d has no index list", r);
      return GPD_ERR_INVALID;
    }
    if (batch < 1 || batch > t->p.max_batch) {
      set_error("gpd_hip_train_group_steps: batch %d is outside 1 .. max_batch = %d of replica %d", batch, t->p.max_batch, r);
      return GPD_ERR_INVALID;
    }
    if (t->n[0] < 1) {
      set_error("gpd_hip_train_group_steps: replica %d has no training set (gpd_hip_train_set_data)", r);
      return GPD_ERR_STATE;
    }
  }
  for (int r = 0; r < G; r++) {
    const int n = g->t[(size_t)r]->n[0];
    const long long count = (long long)num_steps * batch;
    for (long long i = 0; i < count; i++)
      if (indices[r][i] < 0 || indices[r][i] >= n) {
        set_error("gpd_hip_train_group_steps: replica %d: index %d at position %lld is outside the resident set of %d images", r, indices[r][i], i, n);
        return GPD_ERR_INVALID;
      }
  }
  g->current = -1;
  g->bytes[0] = g->bytes[1] = 0;
  const char *who = "gpd_hip_train_group_steps";
  const float w = group::mean_weight(G);
  const int per = kIdxCap / batch;
  std::vector<int> step((size_t)G);
  for (int s0 = 0; s0 < num_steps; s0 += per) {
    const int ns = std::min(per, num_steps - s0);
    hipError_t e = hipSuccess;
    for (int r = 0; r < G && e == hipSuccess; r++) {
      gpd_hip_trainer *t = g->t[(size_t)r];
      const size_t bytes = (size_t)ns * batch * sizeof(int32_t);
      e = use_device(g, r);
      if (e == hipSuccess) e = hipMemcpyAsync(t->d_idx, indices[r] + (size_t)s0 * batch, bytes, hipMemcpyHostToDevice, t->stream);
      g->bytes[1] += (long long)bytes;
    }
    if (e != hipSuccess) return fail_hip(g, who, e);
    const int num_ops = group::schedule(G, ns, nullptr, 0);
    g->ops.resize((size_t)num_ops);
    (void)group::schedule(G, ns, g->ops.data(), num_ops);
    std::fill(step.begin(), step.end(), 0);
    for (int i = 0; i < num_ops && e == hipSuccess; i++) e = enqueue_op(g, g->ops[(size_t)i], batch, step);
    if (e != hipSuccess) return fail_hip(g, who, e);
    g->h_loss.resize((size_t)G * ns);
    for (int r = 0; r < G && e == hipSuccess; r++) {
      gpd_hip_trainer *t = g->t[(size_t)r];
      e = use_device(g, r);
      if (e == hipSuccess) e = hipMemcpyAsync(g->h_loss.data() + (size_t)r * ns, t->d_loss, (size_t)ns * sizeof(float), hipMemcpyDeviceToHost, t->stream);
      g->bytes[1] += (long long)((size_t)ns * sizeof(float));
    }
    if (e == hipSuccess) e = sync_all(g);
    if (e != hipSuccess) return fail_hip(g, who, e);
    for (int s = 0; s < ns; s++) {
      float sum = g->h_loss[(size_t)s];
      for (int r = 1; r < G; r++) sum = sum + g->h_loss[(size_t)r * ns + s];
      losses[s0 + s] = G > 1 ? sum * w : sum;
      if (replica_losses)
        for (int r = 0; r < G; r++) replica_losses[(size_t)r * num_steps + s0 + s] = g->h_loss[(size_t)r * ns + s];
    }
  }
  return GPD_OK;
}

int gpd_hip_train_group_verify(gpd_hip_train_group *g, long long *num_different) {
  if (!g || !num_different) {
    set_error("gpd_hip_train_group_verify: null argument");
    return GPD_ERR_INVALID;
  }
  const char *who = "gpd_hip_train_group_verify";
  g->current = -1;
  g->bytes[0] = g->bytes[1] = 0;
  hipError_t e = sync_all(g);
  if (e != hipSuccess) return fail_hip(g, who, e);
  const gpd_hip_trainer *t0 = g->t[0];
  std::vector<unsigned long long> h_count((size_t)g->G, 0);
  for (int r = 1; r < g->G && e == hipSuccess; r++) {
    gpd_hip_trainer *t = g->t[(size_t)r];
    e = use_device(g, r);
    if (e == hipSuccess) e = hipMemsetAsync(g->d_count[(size_t)r], 0, sizeof(unsigned long long), t->stream);
    const float *mine[3] = {t->d_p, t->d_m, t->d_v}, *theirs[3] = {t0->d_p, t0->d_m, t0->d_v};
    for (int b = 0; b < 3 && e == hipSuccess; b++) {
      if (!mine[b] || !theirs[b]) continue;
      // replica 0's buffer comes over slice by slice, through the first gather row (no slice is longer than a row)
      for (int o = 0; o < g->G && e == hipSuccess; o++) {
        const size_t at = (size_t)g->first[o], cnt = slice_size(g, o);
        if (!cnt) continue;
        e = copy_between(g, r, g->gather[(size_t)r], 0, theirs[b] + at, cnt * sizeof(float));
        if (e != hipSuccess) break;
        hipLaunchKernelGGL(group_diff_kernel, dim3(blocks_for(cnt)), dim3(256), 0, t->stream, reinterpret_cast<const uint32_t *>(mine[b] + at),
                           reinterpret_cast<const uint32_t *>(g->gather[(size_t)r]), cnt, g->d_count[(size_t)r]);
        e = hipGetLastError();
      }
    }
    if (e == hipSuccess) e = hipMemcpyAsync(&h_count[(size_t)r], g->d_count[(size_t)r], sizeof(unsigned long long), hipMemcpyDeviceToHost, t->stream);
    g->bytes[1] += (long long)sizeof(unsigned long long);
  }
  if (e == hipSuccess) e = sync_all(g);
  if (e != hipSuccess) return fail_hip(g, who, e);
  long long total = 0;
  for (int r = 1; r < g->G; r++) total += (long long)h_count[(size_t)r] + (g->t[(size_t)r]->step != t0->step ? 1 : 0);
  *num_different = total;
  return GPD_OK;
}

int gpd_hip_train_group_last_bytes(gpd_hip_train_group *g, long long out[2]) {
  if (!g || !out) {
    set_error("gpd_hip_train_group_last_bytes: null argument");
    return GPD_ERR_INVALID;
  }
  out[0] = g->bytes[0];
  out[1] = g->bytes[1];
  return GPD_OK;
}

}  // extern "C"
