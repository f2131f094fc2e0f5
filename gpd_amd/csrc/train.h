// What the trainer's translation units share (train.hip, train_passes.hip, train_sets.hip, train_group.hip): the
// trainer, the sizes its buffers and its passes agree on, and what a training step is enqueued with.
#pragma once

#include <vector>

#include "gpd_internal.h"

namespace gpd {

constexpr int kIdxCap = 1 << 20;  // indices of one enqueue
constexpr int kMaxKernels = 24;
constexpr int kTaps = 25;         // of a 5 x 5 filter
constexpr int kP1 = 784;          // pool1: 28 x 28 positions
constexpr int kP2 = 144;          // pool2: 12 x 12 positions
constexpr int kFc1Splits = 16;    // fc1 forward: K = 144 F2 in 16 ranges of 9 F2 (7200 in ranges of 450 at F2 = 50)

}  // namespace gpd

struct gpd_hip_trainer {
  int device = 0;
  hipStream_t stream = nullptr;
  gpd_train_params p;                                                 // p.channels == shape.channels
  gpd_train_recipe r;
  gpd_lenet_shape shape = {0, 0, 0, 0, 0};                            // the widths are the trainer's: F1 -> F2 -> H1 [-> H2] -> 2
  int nt = 8;                                                         // tensors of the state: 8, or 10 with a third dense layer (H2 > 0)
  size_t off[11] = {0};                                               // the tensors inside the four parameter-sized buffers
  size_t total = 0;                                                   // off[nt]: floats of a parameter-sized buffer
  float *d_p = nullptr, *d_g = nullptr, *d_m = nullptr, *d_v = nullptr;  // SGD: d_m is the history, d_v stays null
  long long step = 0;                                                 // updates since the last set_state
  uint8_t *d_img[2] = {nullptr, nullptr}, *d_lab[2] = {nullptr, nullptr};
  int n[2] = {0, 0};
  int cap[2] = {0, 0};         // images the pools hold: n <= cap
  int *d_idx = nullptr;        // [kIdxCap]
  float *d_loss = nullptr;     // [kIdxCap] one per step of an enqueue
  float *d_pool1 = nullptr, *d_pool2 = nullptr, *d_dpool1 = nullptr, *d_dpool2 = nullptr;  // [max_batch][F1][784], [max_batch][F2 * 144]
  uint8_t *d_arg1 = nullptr, *d_arg2 = nullptr;
  float *d_a1 = nullptr, *d_dz1 = nullptr;  // [max_batch][H1]
  float *d_a2 = nullptr, *d_dz2 = nullptr;  // [max_batch][H2], H2 > 0 only
  float *d_logits = nullptr, *d_dl = nullptr, *d_loss_b = nullptr;
  float *d_part = nullptr;     // split-K partials of fc1 forward, conv2 dW, conv1 dW: room for the largest of the three
  hipEvent_t ev[gpd::kMaxKernels] = {nullptr};
  std::vector<float> h_all;    // host staging of a parameter-sized buffer
  std::vector<const char *> names;  // of the launches of one timed step, in launch order
};

namespace gpd {

// a trainer and one of its two resident sets (0: training, 1: test)
inline bool set_ok(const gpd_hip_trainer *t, int which) { return t && which >= 0 && which <= 1; }

// a refusal in one statement: set_error's arguments, GPD_ERR_INVALID to return
template <class... A>
int invalid(const char *fmt, A... a) {
  set_error(fmt, a...);
  return GPD_ERR_INVALID;
}

// ---- train_passes.hip: launches on the trainer's stream, the caller has made its device current.  timed: an event of t->ev
// behind every kernel; k counts the kernels ----
// forward over batch B of set `which` on the indices at d_idx; train: the loss of the batch into *d_loss_out and dlogits
void enqueue_forward(gpd_hip_trainer *t, int which, const int *d_idx, int B, bool train, float *d_loss_out, bool timed, int &k);
// forward (train) over batch B of the training set and backward: the gradients of all nt tensors into t->d_g (every element is written)
void enqueue_gradients(gpd_hip_trainer *t, const int *d_idx, int B, float *d_loss_out, bool timed, int &k);
// the recipe's solver from t->d_g; counts the update (t->step)
void enqueue_update(gpd_hip_trainer *t, bool timed, int &k);
// the learning rate of update `it` in double; the recipe has been checked
double learning_rate(const gpd_train_recipe &r, double base_lr, long long it);
// the launches of one step of a trainer with (third) or without a third dense layer, in launch order, the solver's last
std::vector<const char *> step_names(bool third, bool sgd);

}  // namespace gpd
