// The trainer's entries (gpd_hip_train_*) but those of its resident sets: recipes and learning rates, the state's
// tensor tables and their initialisers, creation, and the calls that step, differentiate, apply and evaluate.  What runs on the
// device and what enqueues it is train_passes.hip, the resident sets are train_sets.hip, several replicas train_group.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "context.h"
#include "buffers.h"
#include "sample_model.h"
#include "train.h"

using namespace gpd;

namespace {

constexpr int kF1 = 20, kF2 = 50;  // kF1, kF2, kFc1Out: the stock widths, what the entries without a shape create
constexpr int kMaxBatch = 1024;

int check_recipe(const char *who, const gpd_train_recipe &r) {
  const char *bad = nullptr;
  if (r.network != GPD_TRAIN_NET_TORCH && r.network != GPD_TRAIN_NET_CAFFE)
    bad = "unknown network";
  else if (r.solver != GPD_TRAIN_SOLVER_ADAM && r.solver != GPD_TRAIN_SOLVER_SGD)
    bad = "unknown solver";
  else if (r.lr_policy < GPD_LR_FIXED || r.lr_policy > GPD_LR_INV)
    bad = "unknown lr_policy";
  else if (!(r.momentum >= 0 && r.momentum < 1))
    bad = "momentum is outside [0, 1)";
  else if (r.lr_policy == GPD_LR_STEP && r.stepsize < 1)
    bad = "stepsize < 1 under the step policy";
  else if (!std::isfinite(r.gamma) || !std::isfinite(r.power))
    bad = "gamma or power is not finite";
  else if (r.lr_policy == GPD_LR_INV && r.gamma < 0)
    bad = "a negative gamma under the inv policy";
  for (int i = 0; i < 8 && !bad; i++) {
    if (!(r.lr_mult[i] >= 0 && std::isfinite(r.lr_mult[i])) || !(r.decay_mult[i] >= 0 && std::isfinite(r.decay_mult[i])))
      bad = "a multiplier is negative or not finite";
    else if (r.solver == GPD_TRAIN_SOLVER_ADAM && (r.lr_mult[i] != 1.0 || r.decay_mult[i] != 1.0))
      bad = "multipliers other than 1 belong to the SGD solver";
  }
  if (!bad) return GPD_OK;
  set_error("%s: recipe: %s", who, bad);
  return GPD_ERR_INVALID;
}

bool channels_ok(int c) { return c == 1 || c == 3 || c == 12 || c == 15; }

gpd_lenet_shape stock_shape(int C) { return {C, kF1, kF2, kFc1Out, 0}; }

int num_tensors(const gpd_lenet_shape &s) { return s.fc2_out > 0 ? 10 : 8; }

// element counts of the state's tensors in state order: eight, or ten with a third dense layer (n[8] = n[9] = 0 without)
void tensor_sizes(const gpd_lenet_shape &s, size_t n[10]) {
  const size_t F1 = (size_t)s.conv1_out, F2 = (size_t)s.conv2_out, H1 = (size_t)s.fc1_out, H2 = (size_t)s.fc2_out, N = H2 ? H2 : 2;
  n[0] = F1 * (size_t)s.channels * kTaps, n[1] = F1, n[2] = F2 * F1 * kTaps, n[3] = F2;
  n[4] = H1 * F2 * kP2, n[5] = H1, n[6] = N * H1, n[7] = N;
  n[8] = H2 ? 2 * H2 : 0, n[9] = H2 ? 2 : 0;
}

// fan_in of layer l = tensor / 2
void fan_ins(const gpd_lenet_shape &s, int f[5]) {
  f[0] = s.channels * kTaps, f[1] = s.conv1_out * kTaps, f[2] = s.conv2_out * kP2, f[3] = s.fc1_out, f[4] = s.fc2_out;
}

const char *const kTensorNames[10] = {"conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias", "fc1.weight",
                                      "fc1.bias",     "fc2.weight", "fc2.bias",   "fc3.weight", "fc3.bias"};

int check_indices(const char *who, const int32_t *indices, long long count, int n) {
  for (long long i = 0; i < count; i++)
    if (indices[i] < 0 || indices[i] >= n)
      return invalid("%s: index %d at position %lld is outside the resident set of %d images", who, indices[i], i, n);
  return GPD_OK;
}

int check_batch(const char *who, gpd_hip_trainer *t, const void *indices, int batch) {
  if (!t || !indices) return invalid("%s: null argument", who);
  if (batch < 1 || batch > t->p.max_batch) return invalid("%s: batch %d is outside 1 .. max_batch = %d", who, batch, t->p.max_batch);
  if (t->n[0] < 1) {
    set_error("%s: no training set (gpd_hip_train_set_data)", who);
    return GPD_ERR_STATE;
  }
  return GPD_OK;
}

bool all_finite(const float *v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

// a table of 8 on a trainer of ten tensors: refused, nothing changed (a null trainer is the callee's to refuse)
int eight_only(const char *who, const gpd_hip_trainer *t) {
  if (!t || t->nt == 8) return GPD_OK;
  set_error("%s: the trainer's network has a third dense layer and ten tensors; use the gpd_hip_train_net_ entry", who);
  return GPD_ERR_STATE;
}

size_t tensor_size(const gpd_hip_trainer *t, int i) { return t->off[i + 1] - t->off[i]; }

// U(-bound, bound) per tensor from one xorshift64 stream, the tensors in order.  xavier: Caffe's filler, bound sqrt(3 / fan_in),
// biases 0 without a draw, no weight outside its bound; otherwise torch's default, bound 1 / sqrt(fan_in), biases drawn too
int init_tensors(const char *who, const gpd_lenet_shape *shape, uint32_t seed, float *const tensors[10], bool xavier) {
  if (!shape || !tensors) return invalid("%s: null argument", who);
  if (gpd_hip_lenet_shape_check(shape) != GPD_OK) return GPD_ERR_INVALID;
  size_t sz[10];
  tensor_sizes(*shape, sz);
  const int nt = num_tensors(*shape);
  for (int i = 0; i < nt; i++)
    if (!tensors[i]) return invalid("%s: tensor %d is null", who, i);
  int fan_in[5];
  fan_ins(*shape, fan_in);
  sample::Stream st(seed);
  for (int i = 0; i < nt; i++) {
    if (xavier && (i & 1)) {  // a bias: constant filler 0, no draw
      std::fill(tensors[i], tensors[i] + sz[i], 0.f);
      continue;
    }
    const double bound = xavier ? std::sqrt(3.0 / (double)fan_in[i / 2]) : (double)(float)(1.0 / std::sqrt((double)fan_in[i / 2]));
    // 24 bits of the draw -> the centres of 2^24 equal cells of (-bound, bound); xavier: the rounding to float never leaves the bound
    for (size_t j = 0; j < sz[i]; j++) {
      float w = (float)((2.0 * ((double)(st.next() >> 40) + 0.5) / 16777216.0 - 1.0) * bound);
      if (xavier && std::fabs((double)w) > bound) w = std::nextafterf(w, 0.f);
      tensors[i][j] = w;
    }
  }
  return GPD_OK;
}

// the entries with a channel count for a shape: the stock widths
int init_stock(const char *who, int channels, uint32_t seed, float *const tensors[8], bool xavier) {
  if (!channels_ok(channels) || !tensors) return invalid("%s: %d channels (1, 3, 12 or 15) or a null argument", who, channels);
  const gpd_lenet_shape stock = stock_shape(channels);
  return init_tensors(who, &stock, seed, tensors, xavier);
}

// ---- a tensor table: the caller's nt pointers, one per tensor, against one parameter-sized device buffer.  An entry refuses
// every table it is handed, in its own words, before it copies anything or makes the device current ----

// the first slot that is null or (finite) holds a value that is not finite; -1: none
int bad_slot(const gpd_hip_trainer *t, const float *const *tensors, bool finite) {
  for (int i = 0; i < t->nt; i++)
    if (!tensors[i] || (finite && !all_finite(tensors[i], tensor_size(t, i)))) return i;
  return -1;
}

// the table's tensors into the device buffer d through h_all: enqueued; h_all is the caller's again once the stream has been waited for
hipError_t upload_table(gpd_hip_trainer *t, const float *const *tensors, float *d) {
  for (int i = 0; i < t->nt; i++) std::memcpy(t->h_all.data() + t->off[i], tensors[i], tensor_size(t, i) * sizeof(float));
  return hipMemcpyAsync(d, t->h_all.data(), t->total * sizeof(float), hipMemcpyHostToDevice, t->stream);
}

// the device buffer d, as the stream's work so far leaves it, into the table's tensors through h_all: waited for
hipError_t download_table(gpd_hip_trainer *t, const float *d, float *const *tensors) {
  hipError_t e = hipMemcpyAsync(t->h_all.data(), d, t->total * sizeof(float), hipMemcpyDeviceToHost, t->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if (e != hipSuccess) return e;
  for (int i = 0; i < t->nt; i++) std::memcpy(tensors[i], t->h_all.data() + t->off[i], tensor_size(t, i) * sizeof(float));
  return hipSuccess;
}

int set_state(const char *who, gpd_hip_trainer *t, const float *const *tensors) {
  if (!t || !tensors) return invalid("%s: null argument", who);
  const int bad = bad_slot(t, tensors, true);
  if (bad >= 0) return invalid("%s: %s is null or holds a non-finite value", who, kTensorNames[bad]);
  HIP_RET(hipSetDevice(t->device));
  const size_t bytes = t->total * sizeof(float);
  HIP_RET(upload_table(t, tensors, t->d_p));
  HIP_RET(hipMemsetAsync(t->d_m, 0, bytes, t->stream));
  if (t->d_v) HIP_RET(hipMemsetAsync(t->d_v, 0, bytes, t->stream));
  HIP_RET(hipStreamSynchronize(t->stream));
  t->step = 0;
  return GPD_OK;
}

int get_state(const char *who, gpd_hip_trainer *t, float *const *tensors) {
  if (!t || !tensors) return invalid("%s: null argument", who);
  const int bad = bad_slot(t, tensors, false);
  if (bad >= 0) return invalid("%s: tensor %d is null", who, bad);
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(download_table(t, t->d_p, tensors));
  return GPD_OK;
}

int get_solver_state(const char *who, gpd_hip_trainer *t, float *const *m, float *const *v, long long *count) {
  if (!t || !m || !count || (t->d_v && !v)) return invalid("%s: null argument", who);
  int bad = bad_slot(t, m, false);
  const int bad_v = t->d_v ? bad_slot(t, v, false) : -1;
  if (bad_v >= 0 && (bad < 0 || bad_v < bad)) bad = bad_v;  // the lower slot of the two tables
  if (bad >= 0) return invalid("%s: tensor %d is null", who, bad);
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(download_table(t, t->d_m, m));
  if (t->d_v) HIP_RET(download_table(t, t->d_v, v));
  *count = t->step;
  return GPD_OK;
}

int set_solver_state(const char *who, gpd_hip_trainer *t, const float *const *m, const float *const *v, long long count) {
  if (!t || !m || (t->d_v && !v) || count < 0) return invalid("%s: null argument or a negative count", who);
  const float *const *src[2] = {m, t->d_v ? v : nullptr};
  float *dst[2] = {t->d_m, t->d_v};
  for (int b = 0; b < 2 && src[b]; b++) {
    const int bad = bad_slot(t, src[b], true);
    if (bad >= 0) return invalid("%s: buffer %d, tensor %d is null or holds a non-finite value", who, b, bad);
  }
  HIP_RET(hipSetDevice(t->device));
  for (int b = 0; b < 2 && src[b]; b++) {
    HIP_RET(upload_table(t, src[b], dst[b]));
    HIP_RET(hipStreamSynchronize(t->stream));
  }
  t->step = count;
  return GPD_OK;
}

int gradients(const char *who, gpd_hip_trainer *t, const int32_t *indices, int batch, float *const *grads, float *loss) {
  int rc = check_batch(who, t, indices, batch);
  if (rc) return rc;
  if (!grads || !loss) return invalid("%s: null argument", who);
  const int bad = bad_slot(t, grads, false);
  if (bad >= 0) return invalid("%s: tensor %d is null", who, bad);
  rc = check_indices(who, indices, batch, t->n[0]);
  if (rc) return rc;
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipMemcpyAsync(t->d_idx, indices, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice, t->stream));
  int k = 0;
  enqueue_gradients(t, t->d_idx, batch, t->d_loss, false, k);
  HIP_RET(hipGetLastError());
  HIP_RET(hipMemcpyAsync(loss, t->d_loss, sizeof(float), hipMemcpyDeviceToHost, t->stream));
  HIP_RET(download_table(t, t->d_g, grads));
  return GPD_OK;
}

int apply(const char *who, gpd_hip_trainer *t, const float *const *grads) {
  if (!t || !grads) return invalid("%s: null argument", who);
  const int bad = bad_slot(t, grads, true);
  if (bad >= 0) return invalid("%s: tensor %d is null or holds a non-finite value", who, bad);
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(upload_table(t, grads, t->d_g));
  int k = 0;
  enqueue_update(t, false, k);
  HIP_RET(hipGetLastError());
  HIP_RET(hipStreamSynchronize(t->stream));
  return GPD_OK;
}

// every creation entry; shape == null: the stock widths at the parameters' channel count.  Everything is checked before anything is allocated
int create_trainer(gpd_hip_ctx *ctx, const gpd_train_params *params, const gpd_train_recipe *recipe, const gpd_lenet_shape *shape,
                   gpd_hip_trainer **out) {
  if (!ctx || !params || !out) return invalid("gpd_hip_train_create: null argument");
  gpd_train_recipe r;
  (void)gpd_hip_train_default_recipe(&r, 0);
  if (recipe) {
    r = *recipe;
    const int rc = check_recipe("gpd_hip_train_create_recipe", r);
    if (rc) return rc;
  }
  const gpd_train_params &q = *params;
  if (shape) {
    if (gpd_hip_lenet_shape_check(shape) != GPD_OK) return GPD_ERR_INVALID;
    if (shape->channels != q.channels)
      return invalid("gpd_hip_train_create_net: the shape has %d channels, the parameters %d", shape->channels, q.channels);
    for (int i = 0; i < 8 && shape->fc2_out > 0; i++)
      if (r.lr_mult[i] != 1.0 || r.decay_mult[i] != 1.0)
        return invalid("gpd_hip_train_create_net: a network with a third dense layer has ten tensors, the recipe eight multiplier slots: every multiplier must be 1");
  }
  if (!channels_ok(q.channels)) return invalid("gpd_hip_train_create: %d channels (1, 3, 12 or 15)", q.channels);
  if (q.max_batch < 1 || q.max_batch > kMaxBatch)
    return invalid("gpd_hip_train_create: max_batch %d is outside 1 .. %d", q.max_batch, kMaxBatch);
  if (!(q.lr >= 0 && std::isfinite(q.lr)) || !(q.beta1 >= 0 && q.beta1 < 1) || !(q.beta2 >= 0 && q.beta2 < 1) ||
      !(q.eps >= 0 && std::isfinite(q.eps)) || !(q.weight_decay >= 0 && std::isfinite(q.weight_decay)) ||
      !(q.input_scale > 0 && std::isfinite(q.input_scale)))
    return invalid("gpd_hip_train_create: a hyper-parameter is out of range");
  gpd_hip_trainer *t = new gpd_hip_trainer();
  ctx_device_stream(ctx, &t->device, &t->stream);
  t->p = q;
  t->r = r;
  t->shape = shape ? *shape : stock_shape(q.channels);
  t->nt = num_tensors(t->shape);
  t->names = step_names(t->shape.fc2_out > 0, r.solver == GPD_TRAIN_SOLVER_SGD);
  size_t sz[10];
  tensor_sizes(t->shape, sz);
  for (int i = 0; i < t->nt; i++) t->off[i + 1] = t->off[i] + sz[i];
  t->total = t->off[t->nt];
  // every count below in size_t: at the limits (64, 128, 1024, 1024; batch 1024) conv2's partials alone are 0.8 GB
  const size_t total = t->total, B = (size_t)q.max_batch, C = (size_t)q.channels;
  const size_t F1 = (size_t)t->shape.conv1_out, F2 = (size_t)t->shape.conv2_out, H1 = (size_t)t->shape.fc1_out, H2 = (size_t)t->shape.fc2_out;
  const size_t fc1_in = F2 * kP2;
  // d_part: fc1's forward partials, conv2's dW partials (one per image), conv1's dW partials (four per image)
  const size_t part = B * std::max(std::max(F2 * F1 * kTaps, 4 * F1 * kTaps * C), kFc1Splits * H1);
  hipError_t e = hipSetDevice(t->device);
  if (e == hipSuccess) e = device_alloc(t->d_p, total);
  if (e == hipSuccess) e = device_alloc(t->d_g, total);
  if (e == hipSuccess) e = device_alloc(t->d_m, total);
  if (e == hipSuccess && r.solver == GPD_TRAIN_SOLVER_ADAM) e = device_alloc(t->d_v, total);
  if (e == hipSuccess) e = device_alloc(t->d_idx, (size_t)kIdxCap);
  if (e == hipSuccess) e = device_alloc(t->d_loss, (size_t)kIdxCap);
  if (e == hipSuccess) e = device_alloc(t->d_pool1, B * F1 * kP1);
  if (e == hipSuccess) e = device_alloc(t->d_dpool1, B * F1 * kP1);
  if (e == hipSuccess) e = device_alloc(t->d_arg1, B * F1 * kP1);
  if (e == hipSuccess) e = device_alloc(t->d_pool2, B * fc1_in);
  if (e == hipSuccess) e = device_alloc(t->d_dpool2, B * fc1_in);
  if (e == hipSuccess) e = device_alloc(t->d_arg2, B * fc1_in);
  if (e == hipSuccess) e = device_alloc(t->d_a1, B * H1);
  if (e == hipSuccess) e = device_alloc(t->d_dz1, B * H1);
  if (e == hipSuccess && H2) e = device_alloc(t->d_a2, B * H2);
  if (e == hipSuccess && H2) e = device_alloc(t->d_dz2, B * H2);
  if (e == hipSuccess) e = device_alloc(t->d_logits, B * 2);
  if (e == hipSuccess) e = device_alloc(t->d_dl, B * 2);
  if (e == hipSuccess) e = device_alloc(t->d_loss_b, B);
  if (e == hipSuccess) e = device_alloc(t->d_part, part);
  for (int i = 0; i < kMaxKernels && e == hipSuccess; i++) e = hipEventCreate(&t->ev[i]);
  if (e == hipSuccess) e = hipMemsetAsync(t->d_p, 0, total * sizeof(float), t->stream);
  if (e == hipSuccess) e = hipMemsetAsync(t->d_m, 0, total * sizeof(float), t->stream);
  if (e == hipSuccess && t->d_v) e = hipMemsetAsync(t->d_v, 0, total * sizeof(float), t->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(t->stream);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    set_error("gpd_hip_train_create: %s", hipGetErrorString(e));
    gpd_hip_train_destroy(t);
    return GPD_ERR_HIP;
  }
  t->h_all.resize(total);
  *out = t;
  return GPD_OK;
}

}  // namespace

extern "C" {

void gpd_hip_train_default_params(gpd_train_params *p) {
  if (!p) return;
  p->channels = 15;
  p->max_batch = 64;
  p->lr = 1e-3, p->beta1 = 0.9, p->beta2 = 0.999, p->eps = 1e-8, p->weight_decay = 5e-4;
  p->input_scale = 1.0 / 256;
}

int gpd_hip_sizeof_train_recipe(void) { return (int)sizeof(gpd_train_recipe); }

int gpd_hip_train_default_recipe(gpd_train_recipe *r, int which) {
  if (!r || which < 0 || which > 1) return invalid("gpd_hip_train_default_recipe: a null recipe or which = %d (0 or 1)", which);
  std::memset(r, 0, sizeof(*r));
  r->network = which ? GPD_TRAIN_NET_CAFFE : GPD_TRAIN_NET_TORCH;
  r->solver = which ? GPD_TRAIN_SOLVER_SGD : GPD_TRAIN_SOLVER_ADAM;
  r->momentum = which ? 0.9 : 0.0;
  r->lr_policy = which ? GPD_LR_INV : GPD_LR_FIXED;
  r->stepsize = 1;
  r->gamma = which ? 0.0001 : 1.0;
  r->power = which ? 0.75 : 0.0;
  for (int i = 0; i < 8; i++) r->lr_mult[i] = r->decay_mult[i] = 1.0;
  return GPD_OK;
}

int gpd_hip_train_learning_rate(const gpd_train_recipe *recipe, double base_lr, long long it, float *lr) {
  if (!recipe || !lr || it < 0 || !(base_lr >= 0 && std::isfinite(base_lr)))
    return invalid("gpd_hip_train_learning_rate: a null argument, a negative count or a base_lr that is negative or not finite");
  const int rc = check_recipe("gpd_hip_train_learning_rate", *recipe);
  if (rc) return rc;
  *lr = (float)learning_rate(*recipe, base_lr, it);
  return GPD_OK;
}

int gpd_hip_train_create(gpd_hip_ctx *ctx, const gpd_train_params *params, gpd_hip_trainer **out) {
  return gpd_hip_train_create_recipe(ctx, params, nullptr, out);
}

int gpd_hip_train_create_recipe(gpd_hip_ctx *ctx, const gpd_train_params *params, const gpd_train_recipe *recipe, gpd_hip_trainer **out) {
  return create_trainer(ctx, params, recipe, nullptr, out);
}

int gpd_hip_train_create_net(gpd_hip_ctx *ctx, const gpd_train_params *params, const gpd_train_recipe *recipe, const gpd_lenet_shape *shape,
                             gpd_hip_trainer **out) {
  if (!shape) return invalid("gpd_hip_train_create_net: null argument");
  return create_trainer(ctx, params, recipe, shape, out);
}

int gpd_hip_train_shape(const gpd_hip_trainer *t, gpd_lenet_shape *out) {
  if (!t || !out) return invalid("gpd_hip_train_shape: null argument");
  *out = t->shape;
  return GPD_OK;
}

void gpd_hip_train_destroy(gpd_hip_trainer *t) {
  if (!t) return;
  (void)hipSetDevice(t->device);
  if (t->stream) (void)hipStreamSynchronize(t->stream);
  device_release(t->d_p, t->d_g, t->d_m, t->d_v, t->d_img[0], t->d_img[1], t->d_lab[0], t->d_lab[1], t->d_idx, t->d_loss, t->d_pool1,
                 t->d_pool2, t->d_dpool1, t->d_dpool2, t->d_arg1, t->d_arg2, t->d_a1, t->d_dz1, t->d_a2, t->d_dz2, t->d_logits, t->d_dl,
                 t->d_loss_b, t->d_part);
  for (hipEvent_t e : t->ev)
    if (e) (void)hipEventDestroy(e);
  delete t;
}

int gpd_hip_train_net_sizes(const gpd_lenet_shape *shape, size_t n[10]) {
  if (!shape || !n) return invalid("gpd_hip_train_net_sizes: null argument");
  if (gpd_hip_lenet_shape_check(shape) != GPD_OK) return GPD_ERR_INVALID;
  tensor_sizes(*shape, n);
  return GPD_OK;
}

int gpd_hip_train_net_init_state(const gpd_lenet_shape *shape, uint32_t seed, float *const tensors[10]) {
  return init_tensors("gpd_hip_train_net_init_state", shape, seed, tensors, false);
}

int gpd_hip_train_net_init_xavier(const gpd_lenet_shape *shape, uint32_t seed, float *const tensors[10]) {
  return init_tensors("gpd_hip_train_net_init_xavier", shape, seed, tensors, true);
}

int gpd_hip_train_init_state(int channels, uint32_t seed, float *const tensors[8]) {
  return init_stock("gpd_hip_train_init_state", channels, seed, tensors, false);
}

int gpd_hip_train_init_xavier(int channels, uint32_t seed, float *const tensors[8]) {
  return init_stock("gpd_hip_train_init_xavier", channels, seed, tensors, true);
}

// The entries with tables of 8 serve every trainer without a third dense layer; the _net_ entries, with tables of 10 whose
// slots [8] and [9] are not read for such a trainer, serve every trainer.
int gpd_hip_train_set_state(gpd_hip_trainer *t, const float *const tensors[8]) {
  const int rc = eight_only("gpd_hip_train_set_state", t);
  return rc ? rc : set_state("gpd_hip_train_set_state", t, tensors);
}
int gpd_hip_train_net_set_state(gpd_hip_trainer *t, const float *const tensors[10]) { return set_state("gpd_hip_train_net_set_state", t, tensors); }

int gpd_hip_train_get_state(gpd_hip_trainer *t, float *const tensors[8]) {
  const int rc = eight_only("gpd_hip_train_get_state", t);
  return rc ? rc : get_state("gpd_hip_train_get_state", t, tensors);
}
int gpd_hip_train_net_get_state(gpd_hip_trainer *t, float *const tensors[10]) { return get_state("gpd_hip_train_net_get_state", t, tensors); }

int gpd_hip_train_get_solver_state(gpd_hip_trainer *t, float *const m[8], float *const v[8], long long *count) {
  const int rc = eight_only("gpd_hip_train_get_solver_state", t);
  return rc ? rc : get_solver_state("gpd_hip_train_get_solver_state", t, m, v, count);
}
int gpd_hip_train_net_get_solver_state(gpd_hip_trainer *t, float *const m[10], float *const v[10], long long *count) {
  return get_solver_state("gpd_hip_train_net_get_solver_state", t, m, v, count);
}

int gpd_hip_train_set_solver_state(gpd_hip_trainer *t, const float *const m[8], const float *const v[8], long long count) {
  const int rc = eight_only("gpd_hip_train_set_solver_state", t);
  return rc ? rc : set_solver_state("gpd_hip_train_set_solver_state", t, m, v, count);
}
int gpd_hip_train_net_set_solver_state(gpd_hip_trainer *t, const float *const m[10], const float *const v[10], long long count) {
  return set_solver_state("gpd_hip_train_net_set_solver_state", t, m, v, count);
}

int gpd_hip_train_steps(gpd_hip_trainer *t, const int32_t *indices, int num_steps, int batch, float *losses) {
  int rc = check_batch("gpd_hip_train_steps", t, indices, batch);
  if (rc) return rc;
  if (num_steps < 0 || (num_steps > 0 && !losses)) return invalid("gpd_hip_train_steps: bad argument");
  rc = check_indices("gpd_hip_train_steps", indices, (long long)num_steps * batch, t->n[0]);
  if (rc) return rc;
  HIP_RET(hipSetDevice(t->device));
  const int per = kIdxCap / batch;
  for (int s0 = 0; s0 < num_steps; s0 += per) {
    const int ns = std::min(per, num_steps - s0);
    HIP_RET(hipMemcpyAsync(t->d_idx, indices + (size_t)s0 * batch, (size_t)ns * batch * sizeof(int32_t), hipMemcpyHostToDevice, t->stream));
    for (int s = 0; s < ns; s++) {
      int k = 0;
      enqueue_gradients(t, t->d_idx + (size_t)s * batch, batch, t->d_loss + s, false, k);
      enqueue_update(t, false, k);
    }
    HIP_RET(hipGetLastError());
    HIP_RET(hipMemcpyAsync(losses + s0, t->d_loss, (size_t)ns * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    HIP_RET(hipStreamSynchronize(t->stream));
  }
  return GPD_OK;
}

int gpd_hip_train_gradients(gpd_hip_trainer *t, const int32_t *indices, int batch, float *const grads[8], float *loss) {
  const int rc = eight_only("gpd_hip_train_gradients", t);
  return rc ? rc : gradients("gpd_hip_train_gradients", t, indices, batch, grads, loss);
}
int gpd_hip_train_net_gradients(gpd_hip_trainer *t, const int32_t *indices, int batch, float *const grads[10], float *loss) {
  return gradients("gpd_hip_train_net_gradients", t, indices, batch, grads, loss);
}

int gpd_hip_train_apply(gpd_hip_trainer *t, const float *const grads[8]) {
  const int rc = eight_only("gpd_hip_train_apply", t);
  return rc ? rc : apply("gpd_hip_train_apply", t, grads);
}
int gpd_hip_train_net_apply(gpd_hip_trainer *t, const float *const grads[10]) { return apply("gpd_hip_train_net_apply", t, grads); }

int gpd_hip_train_eval(gpd_hip_trainer *t, int which, const int32_t *indices, int n, float *logits, int *num_correct) {
  if (!set_ok(t, which) || n < 0 || (n > 0 && !logits) || !num_correct) return invalid("gpd_hip_train_eval: bad argument");
  if (n > 0 && t->n[which] < 1) {
    set_error("gpd_hip_train_eval: set %d is empty (gpd_hip_train_set_data)", which);
    return GPD_ERR_STATE;
  }
  if (indices) {
    const int rc = check_indices("gpd_hip_train_eval", indices, n, t->n[which]);
    if (rc) return rc;
  } else if (n > t->n[which]) {
    return invalid("gpd_hip_train_eval: %d images asked for, set %d holds %d", n, which, t->n[which]);
  }
  HIP_RET(hipSetDevice(t->device));
  std::vector<int32_t> idx((size_t)n);
  std::vector<uint8_t> lab((size_t)n);
  for (int i = 0; i < n; i++) idx[(size_t)i] = indices ? indices[i] : i;
  const int maxb = t->p.max_batch;
  for (int i0 = 0; i0 < n; i0 += maxb) {
    const int B = std::min(maxb, n - i0);
    HIP_RET(hipMemcpyAsync(t->d_idx, idx.data() + i0, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice, t->stream));
    int k = 0;
    enqueue_forward(t, which, t->d_idx, B, false, nullptr, false, k);
    HIP_RET(hipGetLastError());
    HIP_RET(hipMemcpyAsync(logits + 2 * (size_t)i0, t->d_logits, (size_t)B * 2 * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    HIP_RET(hipStreamSynchronize(t->stream));
  }
  // the labels of the set come back once; argmax as torch.max: the first maximum
  std::vector<uint8_t> all((size_t)std::max(t->n[which], 1));
  if (n > 0) HIP_RET(hipMemcpy(all.data(), t->d_lab[which], (size_t)t->n[which], hipMemcpyDeviceToHost));
  int correct = 0;
  for (int i = 0; i < n; i++) correct += (logits[2 * i + 1] > logits[2 * i] ? 1 : 0) == all[(size_t)idx[(size_t)i]];
  *num_correct = correct;
  return GPD_OK;
}

int gpd_hip_train_step_timed(gpd_hip_trainer *t, const int32_t *indices, int batch, float *ms, int capacity, int *num) {
  int rc = check_batch("gpd_hip_train_step_timed", t, indices, batch);
  if (rc) return rc;
  const int launches = (int)t->names.size();
  if (!ms || !num || capacity < launches) return invalid("gpd_hip_train_step_timed: ms must hold %d values", launches);
  rc = check_indices("gpd_hip_train_step_timed", indices, batch, t->n[0]);
  if (rc) return rc;
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipMemcpyAsync(t->d_idx, indices, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice, t->stream));
  (void)hipEventRecord(t->ev[0], t->stream);  // in front of the first launch; the enqueues record one behind each
  int k = 1;
  enqueue_gradients(t, t->d_idx, batch, t->d_loss, true, k);
  enqueue_update(t, true, k);
  HIP_RET(hipGetLastError());
  HIP_RET(hipStreamSynchronize(t->stream));
  for (int i = 0; i + 1 < k; i++) HIP_RET(hipEventElapsedTime(&ms[i], t->ev[i], t->ev[i + 1]));
  *num = k - 1;
  return GPD_OK;
}

// the launches of a stock Adam trainer: what gpd_hip_train_kernel_name_of answers for one
const char *gpd_hip_train_kernel_name(int i) {
  static const std::vector<const char *> stock = step_names(false, false);
  return i >= 0 && i < (int)stock.size() ? stock[(size_t)i] : "";
}

const char *gpd_hip_train_kernel_name_of(const gpd_hip_trainer *t, int i) {
  if (!t) return gpd_hip_train_kernel_name(i);
  return i >= 0 && i < (int)t->names.size() ? t->names[(size_t)i] : "";
}

}  // extern "C"
