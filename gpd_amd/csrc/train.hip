// Training of pytorch/network.py::Net and of the Caffe LeNet (the same network without the ReLUs behind the convolutions) on
// the device: forward with pooling argmax, backward, Adam or Caffe's SGD.  The layer widths are the trainer's
// (gpd_hip_train_create_net: any gpd_lenet_shape, NetCCFFF's third dense layer included); the spatial sizes are constants.
//
// Every GEMM-shaped pass is one instantiation of gemm32: a wave owns a 32 x 32 tile of the result and walks its K range with
// v_mfma_f32_32x32x2_f32, whose result is a k-ascending f32 fmaf chain.  The operands are never materialised: an operand type
// turns (row or column, k) into an address — a convolution patch, a transposed-convolution patch, the pooled gradient expanded
// to the one window position its argmax names, or a plain strided matrix — and an epilogue type turns the accumulators into
// what the pass leaves behind (pooled value + argmax byte, a raw partial, a masked gradient).  Long K ranges are split over
// grid.y into partials that sum_partials adds in a fixed tree: no floating-point atomics anywhere, so a step is a pure
// function of state, data and index list.
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

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kF1 = 20, kF2 = 50, kTaps = 25;  // kF1, kF2, kFc1Out: the stock widths, what the entries without a shape create
constexpr int kP1 = 784, kP1W = 28;    // pool1: 28 x 28
constexpr int kP2 = 144, kP2W = 12;    // pool2: 12 x 12
constexpr int kO1 = 3136, kO1W = 56;   // conv1 output: 56 x 56
constexpr int kO2 = 576, kO2W = 24;    // conv2 output: 24 x 24
constexpr int kMasked = 4;             // argmax byte of a pooled value the ReLU clamped (value <= 0)
constexpr int kFc1Splits = 16;         // fc1 forward: K = 144 F2 in 16 ranges of 9 F2 (7200 in ranges of 450 at F2 = 50)
constexpr int kMaxBatch = 1024;

// ---- operands: ctx(i) once per lane, at(ctx, k) once per k step --------------------------------------------------------------

// a [batch][channel][y][x] tensor with arbitrary strides; idx != null: image b is idx[b] of a resident set
template <class T>
struct Input {
  const T *p;
  const int *idx;
  long long sb;
  int sc, sy, sx;
  float scale;
  __device__ long long image(int b) const { return (long long)(idx ? idx[b] : b) * sb; }
  __device__ float load(long long off) const { return (float)p[off] * scale; }
};

// element (i, k) = p[i * si + k * sk], i < n
struct Plain {
  const float *p;
  long long si, sk;
  int n;
  struct Ctx {
    const float *q;
  };
  __device__ Ctx ctx(int i) const { return {i < n ? p + (long long)i * si : nullptr}; }
  __device__ float at(const Ctx &c, int k) const { return c.q ? c.q[(long long)k * sk] : 0.f; }
};

// forward A: i = (pooled position of the batch) * 4 + window position, k = (channel, ky, kx)
template <class T>
struct PatchByPos {
  Input<T> in;
  int pw, pp, m;  // pooled width, pooled positions per image, rows
  struct Ctx {
    long long off;
  };
  __device__ Ctx ctx(int i) const {
    if (i >= m) return {-1};
    const int pm = i >> 2, w = i & 3, b = pm / pp, q = pm % pp;
    const int y = 2 * (q / pw) + (w >> 1), x = 2 * (q % pw) + (w & 1);
    return {in.image(b) + (long long)y * in.sy + (long long)x * in.sx};
  }
  __device__ float at(const Ctx &c, int k) const {
    if (c.off < 0) return 0.f;
    const int ch = k / kTaps, t = k % kTaps;
    return in.load(c.off + (long long)ch * in.sc + (t / 5) * in.sy + (t % 5) * in.sx);
  }
};

// weight-gradient B: i = (channel, ky, kx), k = (image, y, x) over the convolution's output positions
template <class T, int OW, int OP>  // output width, output positions per image: constants, so that the k decode is multiplies
struct PatchByTap {
  Input<T> in;
  int n;  // taps
  struct Ctx {
    long long off;
  };
  __device__ Ctx ctx(int i) const {
    if (i >= n) return {-1};
    const int ch = i / kTaps, t = i % kTaps;
    return {(long long)ch * in.sc + (t / 5) * in.sy + (t % 5) * in.sx};
  }
  __device__ float at(const Ctx &c, int k) const {
    if (c.off < 0) return 0.f;
    const int b = k / OP, q = k % OP;
    return in.load(in.image(b) + c.off + (long long)(q / OW) * in.sy + (long long)(q % OW) * in.sx);
  }
};

// the gradient in front of a 2 x 2 max-pool, never stored: the pooled gradient sits at the window position its argmax byte names
struct PoolGrad {
  const float *g;        // [batch][F][pp]
  const uint8_t *arg;    // 0 .. 3: row-major window position of the first maximum; kMasked: clamped by the ReLU
  int F, pw, pp;
  __device__ float at(int b, int f, int y, int x) const {
    const long long o = ((long long)b * F + f) * pp + (y >> 1) * pw + (x >> 1);
    return arg[o] == ((y & 1) * 2 + (x & 1)) ? g[o] : 0.f;
  }
};

// weight-gradient A: i = filter, k = (image, y, x)
template <int OW, int OP>
struct GradByFilter {
  PoolGrad pg;
  struct Ctx {
    int f;
  };
  __device__ Ctx ctx(int i) const { return {i < pg.F ? i : -1}; }
  __device__ float at(const Ctx &c, int k) const {
    if (c.f < 0) return 0.f;
    const int b = k / OP, q = k % OP;
    return pg.at(b, c.f, q / OW, q % OW);
  }
};

// input-gradient A (transposed convolution): i = (image, y, x) of the layer's input, k = (filter, ky, kx)
struct GradByPos {
  PoolGrad pg;
  int iw, ip, ow, m;  // input width, input positions per image, output width, rows
  struct Ctx {
    int b, y, x;
  };
  __device__ Ctx ctx(int i) const {
    if (i >= m) return {-1, 0, 0};
    const int q = i % ip;
    return {i / ip, q / iw, q % iw};
  }
  __device__ float at(const Ctx &c, int k) const {
    if (c.b < 0) return 0.f;
    const int f = k / kTaps, t = k % kTaps;
    const int y = c.y - t / 5, x = c.x - t % 5;
    if (y < 0 || y >= ow || x < 0 || x >= ow) return 0.f;
    return pg.at(c.b, f, y, x);
  }
};

// input-gradient B: weights [F][cin][25] read as (k = (filter, tap), i = input channel)
struct WeightByChannel {
  const float *w;
  int cin;
  struct Ctx {
    int c;
  };
  __device__ Ctx ctx(int i) const { return {i < cin ? i : -1}; }
  __device__ float at(const Ctx &c, int k) const {
    if (c.c < 0) return 0.f;
    return w[((long long)(k / kTaps) * cin + c.c) * kTaps + k % kTaps];
  }
};

// ---- epilogues: lane (r = lane & 31, h = lane >> 5) holds column n0 + r, rows m0 + 8 (reg >> 2) + 4 h + (reg & 3) -----------

// bias, 2 x 2 max-pool over the four consecutive rows of a register quad (first maximum in row-major window order); RELU: the
// pooled value clamped at zero and kMasked for a clamped one, otherwise (the Caffe network) the value as it is and its position
template <bool RELU>
struct PoolStore {
  const float *bias;
  float *out;
  uint8_t *arg;
  int F, pp, mp;  // filters, pooled positions per image, pooled rows
  __device__ void store(const f32x16 &acc, int m0, int n0, int lane, int) const {
    const int f = n0 + (lane & 31);
    if (f >= F) return;
    const float bv = bias[f];
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const int pm = (m0 >> 2) + 2 * g + (lane >> 5);
      if (pm >= mp) continue;
      float best = acc[4 * g] + bv;
      int w = 0;
#pragma unroll
      for (int j = 1; j < 4; j++) {
        const float v = acc[4 * g + j] + bv;
        if (v > best) best = v, w = j;
      }
      const long long o = ((long long)(pm / pp) * F + f) * pp + pm % pp;
      if constexpr (RELU) {
        out[o] = best > 0.f ? best : 0.f;
        arg[o] = (uint8_t)(best > 0.f ? w : kMasked);
      } else {
        out[o] = best;
        arg[o] = (uint8_t)w;
      }
    }
  }
};

// out[(split * M + m) * N + n]
struct RawStore {
  float *out;
  int M, N;
  __device__ void store(const f32x16 &acc, int m0, int n0, int lane, int split) const {
    const int n = n0 + (lane & 31);
    if (n >= N) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int m = m0 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
      if (m < M) out[((long long)split * M + m) * N + n] = acc[r];
    }
  }
};

// the gradient of a pooled tensor [m / ip][N][ip]; RELU: zero where the ReLU clamped (no ReLU: arg is not read)
template <bool RELU>
struct MaskStore {
  float *out;
  const uint8_t *arg;
  int M, N, ip;
  __device__ void store(const f32x16 &acc, int m0, int n0, int lane, int) const {
    const int n = n0 + (lane & 31);
    if (n >= N) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int m = m0 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
      if (m >= M) continue;
      const long long o = ((long long)(m / ip) * N + n) * ip + m % ip;
      if constexpr (RELU)
        out[o] = arg[o] != kMasked ? acc[r] : 0.f;
      else
        out[o] = acc[r];
    }
  }
};

// a dense layer whose K fits one range: out[m][n] = relu(acc + bias[n]), row-major [M][N]
struct BiasReluStore {
  const float *bias;
  float *out;
  int M, N;
  __device__ void store(const f32x16 &acc, int m0, int n0, int lane, int) const {
    const int n = n0 + (lane & 31);
    if (n >= N) return;
    const float bv = bias[n];
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int m = m0 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
      if (m >= M) continue;
      const float v = acc[r] + bv;
      out[(long long)m * N + n] = v > 0.f ? v : 0.f;
    }
  }
};

// the gradient in front of a dense layer's ReLU, row-major [M][N]: zero where the activation act[m][n] was clamped
struct ActMaskStore {
  float *out;
  const float *act;
  int M, N;
  __device__ void store(const f32x16 &acc, int m0, int n0, int lane, int) const {
    const int n = n0 + (lane & 31);
    if (n >= N) return;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int m = m0 + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
      if (m >= M) continue;
      const long long o = (long long)m * N + n;
      out[o] = act[o] > 0.f ? acc[r] : 0.f;
    }
  }
};

template <class A, class B, class E>
__global__ void __launch_bounds__(256) gemm32(A a, B b, E e, int tiles_m, int tiles_n, int K, int k_chunk) {
  const int lane = threadIdx.x & 63;
  const int tile = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (tile >= tiles_m * tiles_n) return;
  const int m0 = (tile / tiles_n) * 32, n0 = (tile % tiles_n) * 32;
  const int k0 = blockIdx.y * k_chunk;
  const int k1 = min(K, k0 + k_chunk);
  const auto ca = a.ctx(m0 + (lane & 31));
  const auto cb = b.ctx(n0 + (lane & 31));
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = 0.f;
  for (int k = k0; k < k1; k += 2) {
    const int kk = k + (lane >> 5);
    const float av = kk < k1 ? a.at(ca, kk) : 0.f;
    const float bv = kk < k1 ? b.at(cb, kk) : 0.f;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
  }
  e.store(acc, m0, n0, lane, blockIdx.y);
}

template <class A, class B, class E>
void launch_gemm(hipStream_t st, const A &a, const B &b, const E &e, int M, int N, int K, int k_chunk) {
  const int tm = (M + 31) / 32, tn = (N + 31) / 32;
  hipLaunchKernelGGL((gemm32<A, B, E>), dim3((tm * tn + 3) / 4, (K + k_chunk - 1) / k_chunk), dim3(256), 0, st, a, b, e, tm, tn, K,
                     k_chunk);
}

// ---- the small kernels -----------------------------------------------------------------------------------------------------

// out[e] = sum over s of part[s][e], the partials in eight interleaved chains (s mod 8) joined pairwise; RELU: + bias[e % nb], clamped
template <bool RELU>
__global__ void sum_partials(const float *part, int S, int E, const float *bias, int nb, float *out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= E) return;
  float c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int s = 0; s < S; s++) c[s & 7] += part[(size_t)s * E + e];
  float v = ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7]));
  if (RELU) {
    v += bias[e % nb];
    v = v > 0.f ? v : 0.f;
  }
  out[e] = v;
}

// eight interleaved chains joined pairwise (sum_partials' shape): a 500-term or a batch-long sum as ONE chain rounds some
// sqrt(8) times more than torch's blocked float32 sums do, and it showed in the loss and in fc2.bias at B = 257 (NOTES §L)
__device__ inline float join8(const float c[8]) { return ((c[0] + c[1]) + (c[2] + c[3])) + ((c[4] + c[5]) + (c[6] + c[7])); }

// the last dense layer (W inputs: H1, or H2 behind a third dense layer), softmax cross-entropy and its gradient, one image per
// thread.  WC: the width as a constant (the stock 500: the loop's trip count is then known, which is worth 0.015 ms of a step at
// batch 64), 0: the argument
template <int WC>
__global__ void head_kernel(const float *a1, const float *w, const float *bias, const uint8_t *labels, const int *idx, int B, int W_arg,
                            float *logits, float *loss_b, float *dl) {
  const int W = WC ? WC : W_arg;
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  float c0[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, c1[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int u0 = 0; u0 < W; u0 += 8) {
#pragma unroll
    for (int j = 0; j < 8; j++) {
      if (u0 + j < W) {
        const float a = a1[(size_t)b * W + u0 + j];
        c0[j] = fmaf(a, w[u0 + j], c0[j]);
        c1[j] = fmaf(a, w[W + u0 + j], c1[j]);
      }
    }
  }
  const float z0 = join8(c0) + bias[0], z1 = join8(c1) + bias[1];
  logits[2 * b] = z0;
  logits[2 * b + 1] = z1;
  if (!dl) return;
  const int lab = labels[idx[b]];
  // two classes: everything hangs on d = z1 - z0.  loss = softplus(-+d); p1 = 1 / (1 + e^-d) as 1/2 + tanh(d / 2) / 2 near
  // d = 0 (one rounding of a value near 1/2) and as e^-|d| / (1 + e^-|d|) beyond (the small probability keeps its relative
  // precision); the wrong class gets p_false / B, the true class (p_true - 1) / B = -p_false / B
  const float d = z1 - z0, s = lab ? d : -d;  // s: the margin of the true class
  const float e = expf(-fabsf(d));
  loss_b[b] = fmaxf(-s, 0.f) + log1pf(e);
  float p_false;  // the probability of the wrong class
  if (fabsf(d) < 1.f)
    p_false = fmaf(-0.5f, tanhf(0.5f * s), 0.5f);
  else
    p_false = (s > 0.f ? e : 1.f) / (1.f + e);
  const float g_false = p_false / (float)B;
  dl[2 * b] = lab ? g_false : -g_false;
  dl[2 * b + 1] = lab ? -g_false : g_false;
}

// a block's sum of v[0 .. n): 256 strided chains, then a tree
__device__ float block_sum(const float *v, long long n) {
  __shared__ float sh[256];
  float s = 0.f;
  for (long long i = threadIdx.x; i < n; i += 256) s += v[i];
  sh[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
    __syncthreads();
  }
  return sh[0];
}

__global__ void __launch_bounds__(256) loss_kernel(const float *loss_b, int B, float *out) {
  const float s = block_sum(loss_b, B);
  if (threadIdx.x == 0) *out = s / (float)B;
}

// dZ = (dlogits W_last) where the ReLU of the layer in front of the logits (W wide) passed
__global__ void fc2_back_kernel(const float *dl, const float *w, const float *a1, int B, int W, float *dz1) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * W) return;
  const int b = e / W, u = e % W;
  dz1[e] = a1[e] > 0.f ? fmaf(dl[2 * b + 1], w[W + u], dl[2 * b] * w[u]) : 0.f;
}

// the last layer's weight [2][W] and bias [2], and the bias [W] of the layer in front of it: sums over the batch, image b on
// chain b mod 8
__global__ void head_grads_kernel(const float *dl, const float *a1, const float *dz1, int B, int W, float *g_f2w, float *g_f2b, float *g_f1b) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 3 * W + 2) return;
  const int kind = t < 2 * W ? 0 : t < 2 * W + 2 ? 1 : 2;
  const int j = kind == 0 ? t / W : t - 2 * W, u = kind == 0 ? t % W : t - 2 * W - 2;
  float c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < B; b0 += 8) {
#pragma unroll
    for (int i = 0; i < 8; i++) {
      const int b = b0 + i;
      if (b >= B) continue;
      if (kind == 0)
        c[i] = fmaf(dl[2 * b + j], a1[(size_t)b * W + u], c[i]);
      else if (kind == 1)
        c[i] += dl[2 * b + j];
      else
        c[i] += dz1[(size_t)b * W + u];
    }
  }
  const float s = join8(c);
  if (kind == 0)
    g_f2w[t] = s;
  else if (kind == 1)
    g_f2b[j] = s;
  else
    g_f1b[u] = s;
}

// out[u] = the sum over the batch of dz[b][u], image b on chain b mod 8 as in head_grads_kernel: fc1.bias behind a third dense layer
__global__ void batch_sum_kernel(const float *dz, int B, int W, float *out) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= W) return;
  float c[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int b0 = 0; b0 < B; b0 += 8) {
#pragma unroll
    for (int i = 0; i < 8; i++)
      if (b0 + i < B) c[i] += dz[(size_t)(b0 + i) * W + u];
  }
  out[u] = join8(c);
}

// a convolution's bias gradient: block f sums g[b][f][0 .. pp) image by image, the images' sums joined in image order
__global__ void __launch_bounds__(256) bias_grad_kernel(const float *g, int B, int F, int pp, float *out) {
  const int f = blockIdx.x;
  float total = 0.f;
  for (int b = 0; b < B; b++) {
    const float s = block_sum(g + ((size_t)b * F + f) * pp, pp);
    __syncthreads();
    total += s;
  }
  if (threadIdx.x == 0) out[f] = total;
}

// torch.optim.Adam (single-tensor form, weight_decay as L2) over the eight tensors, which are one buffer
__global__ void adam_kernel(float *p, const float *g, float *m, float *v, int n, float wd, float b1, float w1, float b2, float w2,
                            float step_size, float bc2_sqrt, float eps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float pi = p[i];
  const float gi = fmaf(wd, pi, g[i]);
  // exp_avg.lerp_(grad, 1 - beta1), both forms of torch's lerp: from the start for a weight below 1/2, from the end otherwise —
  // at beta1 = 0 the first form is (g - m) + m, which is not g (a gradient of 1e-12 behind a moment of 0.05 came out as 0)
  const float mi = w1 < 0.5f ? fmaf(w1, gi - m[i], m[i]) : fmaf(-b1, gi - m[i], gi);
  const float vi = fmaf(w2 * gi, gi, v[i] * b2);        // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
  m[i] = mi;
  v[i] = vi;
  const float denom = sqrtf(vi) / bc2_sqrt + eps;
  p[i] = pi - step_size * (mi / denom);
}

// Caffe's SGDSolver over the same buffer: tensor t of eight (its end at off[t + 1]) has its own rate lr_s * lr_mult[t] and decay
// weight_decay * decay_mult[t], both products made on the host
struct SgdTensors {
  int end[8];
  float rate[8], decay[8];
};

__global__ void sgd_kernel(float *p, const float *g, float *h, int n, SgdTensors ts, float momentum) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int t = 0;
#pragma unroll
  for (int j = 0; j < 7; j++) t += i >= ts.end[j];
  float rate = ts.rate[0], decay = ts.decay[0];
#pragma unroll
  for (int j = 1; j < 8; j++)
    if (t == j) rate = ts.rate[j], decay = ts.decay[j];
  const float pi = p[i];
  const float d = fmaf(decay, pi, g[i]);
  const float hi = fmaf(momentum, h[i], rate * d);
  h[i] = hi;
  p[i] = pi - hi;
}

// gpd_hip_train_reorder: image k of the range = image order[k] of its copy in the scratch block, in 16-byte units (one per
// lane: dwordx4 loads and stores) as label.hip's gather moves them; the label rides along on the first lane
__global__ void __launch_bounds__(256) pool_reorder_kernel(const uint4 *__restrict__ src, const uint8_t *__restrict__ src_labels,
                                                           const int32_t *__restrict__ order, uint4 *__restrict__ dst,
                                                           uint8_t *__restrict__ dst_labels, unsigned img_units, unsigned blocks_per) {
  const unsigned k = blockIdx.x / blocks_per, b = blockIdx.x - k * blocks_per;
  const unsigned u = b * 256 + threadIdx.x;
  const size_t from = (size_t)order[k];
  if (u < img_units) dst[(size_t)k * img_units + u] = src[from * img_units + u];
  if (u == 0) dst_labels[k] = src_labels[from];
}

const char *const kKernelNames[] = {"conv1_forward", "conv2_forward", "fc1_forward", "fc1_sum_relu", "head", "loss", "fc2_backward",
                                    "head_grads", "fc1_dw", "fc1_dx", "conv2_db", "conv2_dw", "conv2_dw_sum", "conv2_dx", "conv1_db",
                                    "conv1_dw", "conv1_dw_sum", "adam", "sgd"};
constexpr int kNumKernels = sizeof(kKernelNames) / sizeof(kKernelNames[0]) - 1;  // of one step: it ends in adam or in sgd
static_assert(kNumKernels + 1 <= kMaxKernels, "events");

// the launches of one timed step of a trainer with (third) or without a third dense layer, in launch order
std::vector<const char *> step_names(bool third, bool sgd) {
  std::vector<const char *> n = {"conv1_forward", "conv2_forward", "fc1_forward", "fc1_sum_relu"};
  if (third) n.push_back("fc2_forward");
  n.insert(n.end(), {"head", "loss", third ? "fc3_backward" : "fc2_backward", "head_grads"});
  if (third) n.insert(n.end(), {"fc2_dw", "fc2_dx", "fc1_db"});
  n.insert(n.end(), {"fc1_dw", "fc1_dx", "conv2_db", "conv2_dw", "conv2_dw_sum", "conv2_dx", "conv1_db", "conv1_dw", "conv1_dw_sum", sgd ? "sgd" : "adam"});
  return n;
}
constexpr int kNumKernelsThird = kNumKernels + 4;
static_assert(kNumKernelsThird + 1 <= kMaxKernels, "events");

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

}  // namespace

namespace {

void mark(gpd_hip_trainer *t, bool timed, int &k) {
  if (timed) (void)hipEventRecord(t->ev[k], t->stream);
  k++;
}

// forward over batch B of set `which` on the indices at d_idx; train: the loss of the batch into *d_loss_out and dlogits
template <bool RELU>
void forward_passes(gpd_hip_trainer *t, int which, const int *d_idx, int B, bool train, float *d_loss_out, bool timed, int &k) {
  hipStream_t st = t->stream;
  const int C = t->C, F1 = t->F1, F2 = t->F2, H1 = t->H1, H2 = t->H2, fc1_in = F2 * kP2;
  const float *p = t->d_p;
  const Input<uint8_t> img{t->d_img[which], d_idx, (long long)kPix * C, 1, kImg * C, C, (float)t->p.input_scale};
  launch_gemm(st, PatchByPos<uint8_t>{img, kP1W, kP1, B * kO1}, Plain{p + t->off[0], (long long)C * kTaps, 1, F1},
              PoolStore<RELU>{p + t->off[1], t->d_pool1, t->d_arg1, F1, kP1, B * kP1}, B * kO1, F1, C * kTaps, (C * kTaps + 1) & ~1);
  mark(t, timed, k);
  const Input<float> p1{t->d_pool1, nullptr, (long long)F1 * kP1, kP1, kP1W, 1, 1.f};
  launch_gemm(st, PatchByPos<float>{p1, kP2W, kP2, B * kO2}, Plain{p + t->off[2], (long long)F1 * kTaps, 1, F2},
              PoolStore<RELU>{p + t->off[3], t->d_pool2, t->d_arg2, F2, kP2, B * kP2}, B * kO2, F2, F1 * kTaps, F1 * kTaps);
  mark(t, timed, k);
  // K = 144 F2 in kFc1Splits ranges of 9 F2 (an odd range is legal: the k loop pads its last pair)
  launch_gemm(st, Plain{t->d_pool2, fc1_in, 1, B}, Plain{p + t->off[4], fc1_in, 1, H1}, RawStore{t->d_part, B, H1}, B, H1, fc1_in,
              fc1_in / kFc1Splits);
  mark(t, timed, k);
  hipLaunchKernelGGL(sum_partials<true>, dim3((B * H1 + 255) / 256), dim3(256), 0, st, t->d_part, kFc1Splits, B * H1, p + t->off[5], H1,
                     t->d_a1);
  mark(t, timed, k);
  if (H2 > 0) {
    // A2 [B][H2] = relu(A1 W2^T + b2), K = H1: one chain per output, no split
    launch_gemm(st, Plain{t->d_a1, H1, 1, B}, Plain{p + t->off[6], H1, 1, H2}, BiasReluStore{p + t->off[7], t->d_a2, B, H2}, B, H2, H1, H1);
    mark(t, timed, k);
  }
  const int last = H2 > 0 ? 8 : 6;  // the tensor of the layer that makes the logits
  const int W = H2 > 0 ? H2 : H1;
  hipLaunchKernelGGL(W == kFc1Out ? head_kernel<kFc1Out> : head_kernel<0>, dim3((B + 63) / 64), dim3(64), 0, st, H2 > 0 ? t->d_a2 : t->d_a1,
                     p + t->off[last], p + t->off[last + 1], t->d_lab[which], d_idx, B, W, t->d_logits, t->d_loss_b, train ? t->d_dl : nullptr);
  mark(t, timed, k);
  if (!train) return;
  hipLaunchKernelGGL(loss_kernel, dim3(1), dim3(256), 0, st, t->d_loss_b, B, d_loss_out);
  mark(t, timed, k);
}

template <bool RELU>
void backward_passes(gpd_hip_trainer *t, const int *d_idx, int B, bool timed, int &k) {
  hipStream_t st = t->stream;
  const int C = t->C, F1 = t->F1, F2 = t->F2, H1 = t->H1, H2 = t->H2, fc1_in = F2 * kP2;
  const float *p = t->d_p;
  float *g = t->d_g;
  if (H2 > 0) {
    hipLaunchKernelGGL(fc2_back_kernel, dim3((B * H2 + 255) / 256), dim3(256), 0, st, t->d_dl, p + t->off[8], t->d_a2, B, H2, t->d_dz2);
    mark(t, timed, k);
    hipLaunchKernelGGL(head_grads_kernel, dim3((3 * H2 + 2 + 255) / 256), dim3(256), 0, st, t->d_dl, t->d_a2, t->d_dz2, B, H2, g + t->off[8],
                       g + t->off[9], g + t->off[7]);
    mark(t, timed, k);
    // fc2.weight [H2][H1] = dZ2^T A1, K = B
    launch_gemm(st, Plain{t->d_dz2, 1, H2, H2}, Plain{t->d_a1, 1, H1, H1}, RawStore{g + t->off[6], H2, H1}, H2, H1, B, (B + 1) & ~1);
    mark(t, timed, k);
    // dZ1 [B][H1] = dZ2 W2, K = H2, zero where fc1's ReLU clamped
    launch_gemm(st, Plain{t->d_dz2, H2, 1, B}, Plain{p + t->off[6], 1, H1, H1}, ActMaskStore{t->d_dz1, t->d_a1, B, H1}, B, H1, H2, H2);
    mark(t, timed, k);
    hipLaunchKernelGGL(batch_sum_kernel, dim3((H1 + 255) / 256), dim3(256), 0, st, t->d_dz1, B, H1, g + t->off[5]);
    mark(t, timed, k);
  } else {
    hipLaunchKernelGGL(fc2_back_kernel, dim3((B * H1 + 255) / 256), dim3(256), 0, st, t->d_dl, p + t->off[6], t->d_a1, B, H1, t->d_dz1);
    mark(t, timed, k);
    hipLaunchKernelGGL(head_grads_kernel, dim3((3 * H1 + 2 + 255) / 256), dim3(256), 0, st, t->d_dl, t->d_a1, t->d_dz1, B, H1, g + t->off[6],
                       g + t->off[7], g + t->off[5]);
    mark(t, timed, k);
  }
  // fc1.weight [H1][144 F2] = dZ1^T P2, K = B
  launch_gemm(st, Plain{t->d_dz1, 1, H1, H1}, Plain{t->d_pool2, 1, fc1_in, fc1_in}, RawStore{g + t->off[4], H1, fc1_in}, H1, fc1_in, B,
              (B + 1) & ~1);
  mark(t, timed, k);
  // dPool2 [B][144 F2] = dZ1 W1, K = H1, zero where conv2's ReLU (Net) clamped
  launch_gemm(st, Plain{t->d_dz1, H1, 1, B}, Plain{p + t->off[4], 1, fc1_in, fc1_in}, MaskStore<RELU>{t->d_dpool2, t->d_arg2, B, fc1_in, 1}, B,
              fc1_in, H1, H1);
  mark(t, timed, k);
  hipLaunchKernelGGL(bias_grad_kernel, dim3(F2), dim3(256), 0, st, t->d_dpool2, B, F2, kP2, g + t->off[3]);
  mark(t, timed, k);
  // conv2.weight [F2][25 F1], K = B * 576: one partial per image
  const PoolGrad pg2{t->d_dpool2, t->d_arg2, F2, kP2W, kP2};
  const Input<float> p1{t->d_pool1, nullptr, (long long)F1 * kP1, kP1, kP1W, 1, 1.f};
  launch_gemm(st, GradByFilter<kO2W, kO2>{pg2}, PatchByTap<float, kO2W, kO2>{p1, F1 * kTaps}, RawStore{t->d_part, F2, F1 * kTaps}, F2,
              F1 * kTaps, B * kO2, kO2);
  mark(t, timed, k);
  hipLaunchKernelGGL(sum_partials<false>, dim3((F2 * F1 * kTaps + 255) / 256), dim3(256), 0, st, t->d_part, B, F2 * F1 * kTaps, nullptr, 1,
                     g + t->off[2]);
  mark(t, timed, k);
  // dPool1 [B][F1][784] = transposed convolution of the expanded dPool2, K = 25 F2, zero where conv1's ReLU (Net) clamped
  launch_gemm(st, GradByPos{pg2, kP1W, kP1, kO2W, B * kP1}, WeightByChannel{p + t->off[2], F1}, MaskStore<RELU>{t->d_dpool1, t->d_arg1, B * kP1, F1, kP1},
              B * kP1, F1, F2 * kTaps, F2 * kTaps);
  mark(t, timed, k);
  hipLaunchKernelGGL(bias_grad_kernel, dim3(F1), dim3(256), 0, st, t->d_dpool1, B, F1, kP1, g + t->off[1]);
  mark(t, timed, k);
  // conv1.weight [F1][25 C], K = B * 3136: four partials per image
  const PoolGrad pg1{t->d_dpool1, t->d_arg1, F1, kP1W, kP1};
  const Input<uint8_t> img{t->d_img[0], d_idx, (long long)kPix * C, 1, kImg * C, C, (float)t->p.input_scale};
  launch_gemm(st, GradByFilter<kO1W, kO1>{pg1}, PatchByTap<uint8_t, kO1W, kO1>{img, C * kTaps}, RawStore{t->d_part, F1, C * kTaps}, F1,
              C * kTaps, B * kO1, kO1 / 4);
  mark(t, timed, k);
  hipLaunchKernelGGL(sum_partials<false>, dim3((F1 * C * kTaps + 255) / 256), dim3(256), 0, st, t->d_part, 4 * B, F1 * C * kTaps, nullptr, 1,
                     g + t->off[0]);
  mark(t, timed, k);
}

}  // namespace

// the network is chosen where the kernels are instantiated: no pass tests a flag per element
void gpd::enqueue_forward(gpd_hip_trainer *t, int which, const int *d_idx, int B, bool train, float *d_loss_out, bool timed, int &k) {
  if (t->r.network == GPD_TRAIN_NET_TORCH)
    forward_passes<true>(t, which, d_idx, B, train, d_loss_out, timed, k);
  else
    forward_passes<false>(t, which, d_idx, B, train, d_loss_out, timed, k);
}

void gpd::enqueue_backward(gpd_hip_trainer *t, const int *d_idx, int B, bool timed, int &k) {
  if (t->r.network == GPD_TRAIN_NET_TORCH)
    backward_passes<true>(t, d_idx, B, timed, k);
  else
    backward_passes<false>(t, d_idx, B, timed, k);
}

namespace {

// the learning rate of update `it` in double; the recipe has been checked
double learning_rate(const gpd_train_recipe &r, double base_lr, long long it) {
  switch (r.lr_policy) {
    case GPD_LR_STEP: return base_lr * std::pow(r.gamma, (double)(it / r.stepsize));
    case GPD_LR_EXP: return base_lr * std::pow(r.gamma, (double)it);
    case GPD_LR_INV: return base_lr * std::pow(1.0 + r.gamma * (double)it, -r.power);
    default: return base_lr;
  }
}

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

void enqueue_sgd(gpd_hip_trainer *t, bool timed, int &k) {
  const float lr = (float)learning_rate(t->r, t->p.lr, t->step);
  t->step++;
  // ten tensors (a third dense layer): every multiplier is 1 (checked at creation), so the eight slots serve: whichever slot an
  // element of the last two tensors lands in holds their rate and decay
  SgdTensors ts;
  for (int i = 0; i < 8; i++) {
    ts.end[i] = (int)t->off[i + 1];
    ts.rate[i] = lr * (float)t->r.lr_mult[i];
    ts.decay[i] = (float)t->p.weight_decay * (float)t->r.decay_mult[i];
  }
  const int n = (int)t->total;
  hipLaunchKernelGGL(sgd_kernel, dim3((n + 255) / 256), dim3(256), 0, t->stream, t->d_p, t->d_g, t->d_m, n, ts, (float)t->r.momentum);
  mark(t, timed, k);
}

void enqueue_adam(gpd_hip_trainer *t, bool timed, int &k) {
  const double lr = learning_rate(t->r, t->p.lr, t->step);  // fixed: p.lr itself
  t->step++;
  const gpd_train_params &q = t->p;
  const double bc1 = 1.0 - std::pow(q.beta1, (double)t->step), bc2 = 1.0 - std::pow(q.beta2, (double)t->step);
  const int n = (int)t->total;
  hipLaunchKernelGGL(adam_kernel, dim3((n + 255) / 256), dim3(256), 0, t->stream, t->d_p, t->d_g, t->d_m, t->d_v, n, (float)q.weight_decay,
                     (float)q.beta1, (float)(1.0 - q.beta1), (float)q.beta2, (float)(1.0 - q.beta2), (float)(lr / bc1), (float)std::sqrt(bc2), (float)q.eps);
  mark(t, timed, k);
}

}  // namespace

void gpd::enqueue_update(gpd_hip_trainer *t, bool timed, int &k) {
  if (t->r.solver == GPD_TRAIN_SOLVER_SGD)
    enqueue_sgd(t, timed, k);
  else
    enqueue_adam(t, timed, k);
}

namespace {

int check_indices(const char *who, const int32_t *indices, long long count, int n) {
  for (long long i = 0; i < count; i++)
    if (indices[i] < 0 || indices[i] >= n) {
      set_error("%s: index %d at position %lld is outside the resident set of %d images", who, indices[i], i, n);
      return GPD_ERR_INVALID;
    }
  return GPD_OK;
}

int check_batch(const char *who, gpd_hip_trainer *t, const void *indices, int batch) {
  if (!t || !indices) {
    set_error("%s: null argument", who);
    return GPD_ERR_INVALID;
  }
  if (batch < 1 || batch > t->maxb) {
    set_error("%s: batch %d is outside 1 .. max_batch = %d", who, batch, t->maxb);
    return GPD_ERR_INVALID;
  }
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

size_t image_bytes(const gpd_hip_trainer *t) { return (size_t)kPix * t->C; }

// pool `which` holds exactly `capacity` (>= n) images afterwards, its first n kept.  The stream is synchronised before a pool is
// moved or freed; a failed allocation is GPD_ERR_CAPACITY and leaves the pool as it was
int pool_resize(const char *who, gpd_hip_trainer *t, int which, int capacity) {
  if (capacity == t->cap[which]) return GPD_OK;
  const size_t ib = image_bytes(t);
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipStreamSynchronize(t->stream));
  uint8_t *img = nullptr, *lab = nullptr;
  if (capacity > 0) {
    hipError_t e = device_alloc(img, (size_t)capacity * ib);
    if (e == hipSuccess) e = device_alloc(lab, (size_t)capacity);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      device_release(img);
      set_error("%s: no room for %d images of %d channels (%zu bytes): %s", who, capacity, t->C, (size_t)capacity * (ib + 1), hipGetErrorString(e));
      return GPD_ERR_CAPACITY;
    }
    if (t->n[which] > 0) {
      hipError_t c = hipMemcpyAsync(img, t->d_img[which], (size_t)t->n[which] * ib, hipMemcpyDeviceToDevice, t->stream);
      if (c == hipSuccess) c = hipMemcpyAsync(lab, t->d_lab[which], (size_t)t->n[which], hipMemcpyDeviceToDevice, t->stream);
      if (c == hipSuccess) c = hipStreamSynchronize(t->stream);
      if (c != hipSuccess) {
        device_release(img, lab);
        set_error("%s: moving the pool failed: %s", who, hipGetErrorString(c));
        return GPD_ERR_HIP;
      }
    }
  }
  device_release(t->d_img[which], t->d_lab[which]);
  t->d_img[which] = img;
  t->d_lab[which] = lab;
  t->cap[which] = capacity;
  return GPD_OK;
}

// room for `more` images behind n: geometric growth, at least x 1.5 and never less than the need
int pool_grow(const char *who, gpd_hip_trainer *t, int which, long long more) {
  const long long need = (long long)t->n[which] + more;
  if (need > 0x7fffffffll) {
    set_error("%s: %lld images, a resident set counts them in an int", who, need);
    return GPD_ERR_CAPACITY;
  }
  if (need <= t->cap[which]) return GPD_OK;
  const long long grown = (long long)t->cap[which] + t->cap[which] / 2 + 1;
  return pool_resize(who, t, which, (int)std::min(std::max(need, grown), 0x7fffffffll));
}

int check_labels(const char *who, const uint8_t *labels, int n) {
  for (int i = 0; i < n; i++)
    if (labels[i] > 1) {
      set_error("%s: label %d of image %d (0 or 1)", who, (int)labels[i], i);
      return GPD_ERR_INVALID;
    }
  return GPD_OK;
}

// gpd_hip_train_append_view's sink: the pool grows when the view's kept count is known, the gather writes behind n
struct ViewSink {
  gpd_hip_trainer *t;
  int which;
  static int place(void *self, size_t k, uint8_t **images, uint8_t **labels) {
    ViewSink *s = static_cast<ViewSink *>(self);
    const int rc = pool_grow("gpd_hip_train_append_view", s->t, s->which, (long long)k);
    if (rc) return rc;
    *images = s->t->d_img[s->which] + (size_t)s->t->n[s->which] * image_bytes(s->t);
    *labels = s->t->d_lab[s->which] + (size_t)s->t->n[s->which];
    return GPD_OK;
  }
};

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
  if (!shape || !tensors) {
    set_error("%s: null argument", who);
    return GPD_ERR_INVALID;
  }
  if (gpd_hip_lenet_shape_check(shape) != GPD_OK) return GPD_ERR_INVALID;
  size_t sz[10];
  tensor_sizes(*shape, sz);
  const int nt = num_tensors(*shape);
  for (int i = 0; i < nt; i++)
    if (!tensors[i]) {
      set_error("%s: tensor %d is null", who, i);
      return GPD_ERR_INVALID;
    }
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

int set_state(const char *who, gpd_hip_trainer *t, const float *const *tensors) {
  if (!t || !tensors) {
    set_error("%s: null argument", who);
    return GPD_ERR_INVALID;
  }
  for (int i = 0; i < t->nt; i++)
    if (!tensors[i] || !all_finite(tensors[i], tensor_size(t, i))) {
      set_error("%s: %s is null or holds a non-finite value", who, kTensorNames[i]);
      return GPD_ERR_INVALID;
    }
  for (int i = 0; i < t->nt; i++) std::memcpy(t->h_all.data() + t->off[i], tensors[i], tensor_size(t, i) * sizeof(float));
  HIP_RET(hipSetDevice(t->device));
  const size_t bytes = t->total * sizeof(float);
  HIP_RET(hipMemcpyAsync(t->d_p, t->h_all.data(), bytes, hipMemcpyHostToDevice, t->stream));
  HIP_RET(hipMemsetAsync(t->d_m, 0, bytes, t->stream));
  if (t->d_v) HIP_RET(hipMemsetAsync(t->d_v, 0, bytes, t->stream));
  HIP_RET(hipStreamSynchronize(t->stream));
  t->step = 0;
  return GPD_OK;
}

int get_state(const char *who, gpd_hip_trainer *t, float *const *tensors) {
  if (!t || !tensors) {
    set_error("%s: null argument", who);
    return GPD_ERR_INVALID;
  }
  for (int i = 0; i < t->nt; i++)
    if (!tensors[i]) {
      set_error("%s: tensor %d is null", who, i);
      return GPD_ERR_INVALID;
    }
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipMemcpyAsync(t->h_all.data(), t->d_p, t->total * sizeof(float), hipMemcpyDeviceToHost, t->stream));
  HIP_RET(hipStreamSynchronize(t->stream));
  for (int i = 0; i < t->nt; i++) std::memcpy(tensors[i], t->h_all.data() + t->off[i], tensor_size(t, i) * sizeof(float));
  return GPD_OK;
}

int get_solver_state(const char *who, gpd_hip_trainer *t, float *const *m, float *const *v, long long *count) {
  if (!t || !m || !count || (t->d_v && !v)) {
    set_error("%s: null argument", who);
    return GPD_ERR_INVALID;
  }
  for (int i = 0; i < t->nt; i++)
    if (!m[i] || (t->d_v && !v[i])) {
      set_error("%s: tensor %d is null", who, i);
      return GPD_ERR_INVALID;
    }
  HIP_RET(hipSetDevice(t->device));
  const float *src[2] = {t->d_m, t->d_v};
  float *const *dst[2] = {m, v};
  for (int b = 0; b < 2; b++) {
    if (!src[b]) continue;
    HIP_RET(hipMemcpyAsync(t->h_all.data(), src[b], t->total * sizeof(float), hipMemcpyDeviceToHost, t->stream));
    HIP_RET(hipStreamSynchronize(t->stream));
    for (int i = 0; i < t->nt; i++) std::memcpy(dst[b][i], t->h_all.data() + t->off[i], tensor_size(t, i) * sizeof(float));
  }
  *count = t->step;
  return GPD_OK;
}

int set_solver_state(const char *who, gpd_hip_trainer *t, const float *const *m, const float *const *v, long long count) {
  if (!t || !m || (t->d_v && !v) || count < 0) {
    set_error("%s: null argument or a negative count", who);
    return GPD_ERR_INVALID;
  }
  const float *const *src[2] = {m, t->d_v ? v : nullptr};
  for (int b = 0; b < 2; b++)
    for (int i = 0; i < t->nt && src[b]; i++)
      if (!src[b][i] || !all_finite(src[b][i], tensor_size(t, i))) {
        set_error("%s: buffer %d, tensor %d is null or holds a non-finite value", who, b, i);
        return GPD_ERR_INVALID;
      }
  HIP_RET(hipSetDevice(t->device));
  float *dst[2] = {t->d_m, t->d_v};
  for (int b = 0; b < 2; b++) {
    if (!src[b]) continue;
    for (int i = 0; i < t->nt; i++) std::memcpy(t->h_all.data() + t->off[i], src[b][i], tensor_size(t, i) * sizeof(float));
    HIP_RET(hipMemcpyAsync(dst[b], t->h_all.data(), t->total * sizeof(float), hipMemcpyHostToDevice, t->stream));
    HIP_RET(hipStreamSynchronize(t->stream));
  }
  t->step = count;
  return GPD_OK;
}

int gradients(const char *who, gpd_hip_trainer *t, const int32_t *indices, int batch, float *const *grads, float *loss) {
  int rc = check_batch(who, t, indices, batch);
  if (rc) return rc;
  if (!grads || !loss) {
    set_error("%s: null argument", who);
    return GPD_ERR_INVALID;
  }
  for (int i = 0; i < t->nt; i++)
    if (!grads[i]) {
      set_error("%s: tensor %d is null", who, i);
      return GPD_ERR_INVALID;
    }
  rc = check_indices(who, indices, batch, t->n[0]);
  if (rc) return rc;
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipMemcpyAsync(t->d_idx, indices, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice, t->stream));
  int k = 0;
  enqueue_forward(t, 0, t->d_idx, batch, true, t->d_loss, false, k);
  enqueue_backward(t, t->d_idx, batch, false, k);
  HIP_RET(hipGetLastError());
  HIP_RET(hipMemcpyAsync(t->h_all.data(), t->d_g, t->total * sizeof(float), hipMemcpyDeviceToHost, t->stream));
  HIP_RET(hipMemcpyAsync(loss, t->d_loss, sizeof(float), hipMemcpyDeviceToHost, t->stream));
  HIP_RET(hipStreamSynchronize(t->stream));
  for (int i = 0; i < t->nt; i++) std::memcpy(grads[i], t->h_all.data() + t->off[i], tensor_size(t, i) * sizeof(float));
  return GPD_OK;
}

int apply(const char *who, gpd_hip_trainer *t, const float *const *grads) {
  if (!t || !grads) {
    set_error("%s: null argument", who);
    return GPD_ERR_INVALID;
  }
  for (int i = 0; i < t->nt; i++)
    if (!grads[i] || !all_finite(grads[i], tensor_size(t, i))) {
      set_error("%s: tensor %d is null or holds a non-finite value", who, i);
      return GPD_ERR_INVALID;
    }
  for (int i = 0; i < t->nt; i++) std::memcpy(t->h_all.data() + t->off[i], grads[i], tensor_size(t, i) * sizeof(float));
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipMemcpyAsync(t->d_g, t->h_all.data(), t->total * sizeof(float), hipMemcpyHostToDevice, t->stream));
  int k = 0;
  enqueue_update(t, false, k);
  HIP_RET(hipGetLastError());
  HIP_RET(hipStreamSynchronize(t->stream));
  return GPD_OK;
}

// every creation entry; shape == null: the stock widths at the parameters' channel count.  Everything is checked before anything is allocated
int create_trainer(gpd_hip_ctx *ctx, const gpd_train_params *params, const gpd_train_recipe *recipe, const gpd_lenet_shape *shape,
                   gpd_hip_trainer **out) {
  if (!ctx || !params || !out) {
    set_error("gpd_hip_train_create: null argument");
    return GPD_ERR_INVALID;
  }
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
    if (shape->channels != q.channels) {
      set_error("gpd_hip_train_create_net: the shape has %d channels, the parameters %d", shape->channels, q.channels);
      return GPD_ERR_INVALID;
    }
    for (int i = 0; i < 8 && shape->fc2_out > 0; i++)
      if (r.lr_mult[i] != 1.0 || r.decay_mult[i] != 1.0) {
        set_error("gpd_hip_train_create_net: a network with a third dense layer has ten tensors, the recipe eight multiplier slots: every multiplier must be 1");
        return GPD_ERR_INVALID;
      }
  }
  if (!channels_ok(q.channels)) {
    set_error("gpd_hip_train_create: %d channels (1, 3, 12 or 15)", q.channels);
    return GPD_ERR_INVALID;
  }
  if (q.max_batch < 1 || q.max_batch > kMaxBatch) {
    set_error("gpd_hip_train_create: max_batch %d is outside 1 .. %d", q.max_batch, kMaxBatch);
    return GPD_ERR_INVALID;
  }
  if (!(q.lr >= 0 && std::isfinite(q.lr)) || !(q.beta1 >= 0 && q.beta1 < 1) || !(q.beta2 >= 0 && q.beta2 < 1) ||
      !(q.eps >= 0 && std::isfinite(q.eps)) || !(q.weight_decay >= 0 && std::isfinite(q.weight_decay)) ||
      !(q.input_scale > 0 && std::isfinite(q.input_scale))) {
    set_error("gpd_hip_train_create: a hyper-parameter is out of range");
    return GPD_ERR_INVALID;
  }
  gpd_hip_trainer *t = new gpd_hip_trainer();
  ctx_device_stream(ctx, &t->device, &t->stream);
  t->p = q;
  t->r = r;
  t->C = q.channels;
  t->maxb = q.max_batch;
  t->shape = shape ? *shape : stock_shape(q.channels);
  t->F1 = t->shape.conv1_out, t->F2 = t->shape.conv2_out, t->H1 = t->shape.fc1_out, t->H2 = t->shape.fc2_out;
  t->nt = num_tensors(t->shape);
  t->names = step_names(t->H2 > 0, r.solver == GPD_TRAIN_SOLVER_SGD);
  size_t sz[10];
  tensor_sizes(t->shape, sz);
  for (int i = 0; i < t->nt; i++) t->off[i + 1] = t->off[i] + sz[i];
  t->total = t->off[t->nt];
  // every count below in size_t: at the limits (64, 128, 1024, 1024; batch 1024) conv2's partials alone are 0.8 GB
  const size_t total = t->total, B = (size_t)t->maxb, F1 = (size_t)t->F1, F2 = (size_t)t->F2, H1 = (size_t)t->H1, H2 = (size_t)t->H2;
  const size_t fc1_in = F2 * kP2;
  // d_part: fc1's forward partials, conv2's dW partials (one per image), conv1's dW partials (four per image)
  const size_t part = B * std::max(std::max(F2 * F1 * kTaps, 4 * F1 * kTaps * (size_t)t->C), kFc1Splits * H1);
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
  if (!r || which < 0 || which > 1) {
    set_error("gpd_hip_train_default_recipe: a null recipe or which = %d (0 or 1)", which);
    return GPD_ERR_INVALID;
  }
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
  if (!recipe || !lr || it < 0 || !(base_lr >= 0 && std::isfinite(base_lr))) {
    set_error("gpd_hip_train_learning_rate: a null argument, a negative count or a base_lr that is negative or not finite");
    return GPD_ERR_INVALID;
  }
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
  if (!shape) {
    set_error("gpd_hip_train_create_net: null argument");
    return GPD_ERR_INVALID;
  }
  return create_trainer(ctx, params, recipe, shape, out);
}

int gpd_hip_train_shape(const gpd_hip_trainer *t, gpd_lenet_shape *out) {
  if (!t || !out) {
    set_error("gpd_hip_train_shape: null argument");
    return GPD_ERR_INVALID;
  }
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
  if (!shape || !n) {
    set_error("gpd_hip_train_net_sizes: null argument");
    return GPD_ERR_INVALID;
  }
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
  if (!channels_ok(channels) || !tensors) {
    set_error("gpd_hip_train_init_state: %d channels (1, 3, 12 or 15) or a null argument", channels);
    return GPD_ERR_INVALID;
  }
  const gpd_lenet_shape stock = stock_shape(channels);
  return init_tensors("gpd_hip_train_init_state", &stock, seed, tensors, false);
}

int gpd_hip_train_init_xavier(int channels, uint32_t seed, float *const tensors[8]) {
  if (!channels_ok(channels) || !tensors) {
    set_error("gpd_hip_train_init_xavier: %d channels (1, 3, 12 or 15) or a null argument", channels);
    return GPD_ERR_INVALID;
  }
  const gpd_lenet_shape stock = stock_shape(channels);
  return init_tensors("gpd_hip_train_init_xavier", &stock, seed, tensors, true);
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

int gpd_hip_train_set_data(gpd_hip_trainer *t, int which, const uint8_t *images_hwc, const uint8_t *labels, int n) {
  if (!t || which < 0 || which > 1 || n < 0 || (n > 0 && (!images_hwc || !labels))) {
    set_error("gpd_hip_train_set_data: bad argument");
    return GPD_ERR_INVALID;
  }
  for (int i = 0; i < n; i++)
    if (labels[i] > 1) {
      set_error("gpd_hip_train_set_data: label %d of image %d (0 or 1)", (int)labels[i], i);
      return GPD_ERR_INVALID;
    }
  const size_t bytes = (size_t)n * kPix * t->C;
  if (bytes > ((size_t)4 << 30)) {
    set_error("gpd_hip_train_set_data: %d images of %d channels are %zu bytes; a resident set holds 4 GiB", n, t->C, bytes);
    return GPD_ERR_CAPACITY;
  }
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipStreamSynchronize(t->stream));
  device_release(t->d_img[which], t->d_lab[which]);
  t->n[which] = t->cap[which] = 0;
  if (n == 0) return GPD_OK;
  HIP_RET(device_alloc(t->d_img[which], bytes));
  HIP_RET(device_alloc(t->d_lab[which], (size_t)n));
  HIP_RET(hipMemcpyAsync(t->d_img[which], images_hwc, bytes, hipMemcpyHostToDevice, t->stream));
  HIP_RET(hipMemcpyAsync(t->d_lab[which], labels, (size_t)n, hipMemcpyHostToDevice, t->stream));
  HIP_RET(hipStreamSynchronize(t->stream));
  t->n[which] = t->cap[which] = n;
  return GPD_OK;
}

int gpd_hip_train_reserve(gpd_hip_trainer *t, int which, int capacity_images) {
  if (!t || which < 0 || which > 1 || capacity_images < 0) {
    set_error("gpd_hip_train_reserve: bad argument");
    return GPD_ERR_INVALID;
  }
  return pool_resize("gpd_hip_train_reserve", t, which, std::max(capacity_images, t->n[which]));
}

int gpd_hip_train_count(gpd_hip_trainer *t, int which, int *n, int *capacity) {
  if (!t || which < 0 || which > 1 || !n) {
    set_error("gpd_hip_train_count: bad argument");
    return GPD_ERR_INVALID;
  }
  *n = t->n[which];
  if (capacity) *capacity = t->cap[which];
  return GPD_OK;
}

int gpd_hip_train_append_data(gpd_hip_trainer *t, int which, const uint8_t *images_hwc, const uint8_t *labels, int n) {
  if (!t || which < 0 || which > 1 || n < 0 || (n > 0 && (!images_hwc || !labels))) {
    set_error("gpd_hip_train_append_data: bad argument");
    return GPD_ERR_INVALID;
  }
  int rc = check_labels("gpd_hip_train_append_data", labels, n);
  if (rc) return rc;
  if (n == 0) return GPD_OK;
  HIP_RET(hipSetDevice(t->device));
  rc = pool_grow("gpd_hip_train_append_data", t, which, n);
  if (rc) return rc;
  const size_t ib = image_bytes(t), at = (size_t)t->n[which];
  HIP_RET(hipMemcpyAsync(t->d_img[which] + at * ib, images_hwc, (size_t)n * ib, hipMemcpyHostToDevice, t->stream));
  HIP_RET(hipMemcpyAsync(t->d_lab[which] + at, labels, (size_t)n, hipMemcpyHostToDevice, t->stream));
  HIP_RET(hipStreamSynchronize(t->stream));
  t->n[which] += n;
  return GPD_OK;
}

int gpd_hip_train_get_data(gpd_hip_trainer *t, int which, int first, int count, uint8_t *images_hwc, uint8_t *labels) {
  if (!t || which < 0 || which > 1 || first < 0 || count < 0 || (long long)first + count > t->n[which] ||
      (count > 0 && (!images_hwc || !labels))) {
    set_error("gpd_hip_train_get_data: bad argument, or a range outside the %d images of the set", t && which >= 0 && which <= 1 ? t->n[which] : 0);
    return GPD_ERR_INVALID;
  }
  if (count == 0) return GPD_OK;
  const size_t ib = image_bytes(t);
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipMemcpyAsync(images_hwc, t->d_img[which] + (size_t)first * ib, (size_t)count * ib, hipMemcpyDeviceToHost, t->stream));
  HIP_RET(hipMemcpyAsync(labels, t->d_lab[which] + (size_t)first, (size_t)count, hipMemcpyDeviceToHost, t->stream));
  HIP_RET(hipStreamSynchronize(t->stream));
  return GPD_OK;
}

int gpd_hip_train_reorder(gpd_hip_trainer *t, int which, int first, int count, const int32_t *order) {
  if (!t || which < 0 || which > 1 || first < 0 || count < 0 || (long long)first + count > t->n[which] || (count > 0 && !order)) {
    set_error("gpd_hip_train_reorder: bad argument, or a range outside the %d images of the set", t && which >= 0 && which <= 1 ? t->n[which] : 0);
    return GPD_ERR_INVALID;
  }
  std::vector<uint8_t> seen((size_t)count, 0);
  bool identity = true;
  for (int k = 0; k < count; k++) {
    if (order[k] < 0 || order[k] >= count || seen[(size_t)order[k]]) {
      set_error("gpd_hip_train_reorder: order[%d] = %d: not a permutation of 0 .. %d", k, order[k], count - 1);
      return GPD_ERR_INVALID;
    }
    seen[(size_t)order[k]] = 1;
    identity = identity && order[k] == k;
  }
  if (identity) return GPD_OK;
  const size_t ib = image_bytes(t);
  const unsigned units = (unsigned)(ib / 16), per = (units + 255) / 256;  // 3600 C bytes: a multiple of 16
  if ((unsigned long long)count * per > 0x7fffffffull) {
    set_error("gpd_hip_train_reorder: %d images are more than one launch takes", count);
    return GPD_ERR_CAPACITY;
  }
  HIP_RET(hipSetDevice(t->device));
  // the scratch block: the range's images | its order | its labels
  const size_t off_order = (size_t)count * ib, off_lab = off_order + ((size_t)count * sizeof(int32_t) + 15) / 16 * 16;
  uint8_t *scratch = nullptr;
  if (device_alloc(scratch, off_lab + (size_t)count) != hipSuccess) {
    (void)hipGetLastError();
    set_error("gpd_hip_train_reorder: no room for a scratch block of %zu bytes", off_lab + (size_t)count);
    return GPD_ERR_CAPACITY;
  }
  uint8_t *img = t->d_img[which] + (size_t)first * ib, *lab = t->d_lab[which] + (size_t)first;
  hipError_t e = hipMemcpyAsync(scratch, img, (size_t)count * ib, hipMemcpyDeviceToDevice, t->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(scratch + off_lab, lab, (size_t)count, hipMemcpyDeviceToDevice, t->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(scratch + off_order, order, (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, t->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(pool_reorder_kernel, dim3((unsigned)count * per), dim3(256), 0, t->stream, reinterpret_cast<const uint4 *>(scratch),
                       scratch + off_lab, reinterpret_cast<const int32_t *>(scratch + off_order), reinterpret_cast<uint4 *>(img), lab, units, per);
    e = hipGetLastError();
  }
  const hipError_t e2 = hipStreamSynchronize(t->stream);
  device_release(scratch);
  if (e != hipSuccess || e2 != hipSuccess) {
    set_error("gpd_hip_train_reorder: %s", hipGetErrorString(e != hipSuccess ? e : e2));
    return GPD_ERR_HIP;
  }
  return GPD_OK;
}

int gpd_hip_train_append_view(gpd_hip_trainer *t, int which, gpd_hip_ctx *ctx, gpd_label_view_job *job) {
  if (!t || !ctx || !job || which < 0 || which > 1) {
    set_error("gpd_hip_train_append_view: bad argument");
    return GPD_ERR_INVALID;
  }
  if (ctx->device != t->device || ctx->params.image_num_channels != t->C) {
    set_error("gpd_hip_train_append_view: the context is on device %d with %d channels, the trainer on device %d with %d", ctx->device,
              ctx->params.image_num_channels, t->device, t->C);
    return GPD_ERR_INVALID;
  }
  ViewSink vs{t, which};
  const LabelSink sink{&vs, &ViewSink::place};
  const int rc = label_view_run(ctx, job, "gpd_hip_train_append_view", &sink);
  if (rc) return rc;
  t->n[which] += job->num_out;  // label_view_run returned after the gather's event: the next step sees the images
  return GPD_OK;
}

int gpd_hip_train_steps(gpd_hip_trainer *t, const int32_t *indices, int num_steps, int batch, float *losses) {
  int rc = check_batch("gpd_hip_train_steps", t, indices, batch);
  if (rc) return rc;
  if (num_steps < 0 || (num_steps > 0 && !losses)) {
    set_error("gpd_hip_train_steps: bad argument");
    return GPD_ERR_INVALID;
  }
  rc = check_indices("gpd_hip_train_steps", indices, (long long)num_steps * batch, t->n[0]);
  if (rc) return rc;
  HIP_RET(hipSetDevice(t->device));
  const int per = kIdxCap / batch;
  for (int s0 = 0; s0 < num_steps; s0 += per) {
    const int ns = std::min(per, num_steps - s0);
    HIP_RET(hipMemcpyAsync(t->d_idx, indices + (size_t)s0 * batch, (size_t)ns * batch * sizeof(int32_t), hipMemcpyHostToDevice, t->stream));
    for (int s = 0; s < ns; s++) {
      int k = 0;
      const int *idx = t->d_idx + (size_t)s * batch;
      enqueue_forward(t, 0, idx, batch, true, t->d_loss + s, false, k);
      enqueue_backward(t, idx, batch, false, k);
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
  if (!t || which < 0 || which > 1 || n < 0 || (n > 0 && !logits) || !num_correct) {
    set_error("gpd_hip_train_eval: bad argument");
    return GPD_ERR_INVALID;
  }
  if (n > 0 && t->n[which] < 1) {
    set_error("gpd_hip_train_eval: set %d is empty (gpd_hip_train_set_data)", which);
    return GPD_ERR_STATE;
  }
  if (indices) {
    const int rc = check_indices("gpd_hip_train_eval", indices, n, t->n[which]);
    if (rc) return rc;
  } else if (n > t->n[which]) {
    set_error("gpd_hip_train_eval: %d images asked for, set %d holds %d", n, which, t->n[which]);
    return GPD_ERR_INVALID;
  }
  HIP_RET(hipSetDevice(t->device));
  std::vector<int32_t> idx((size_t)n);
  std::vector<uint8_t> lab((size_t)n);
  for (int i = 0; i < n; i++) idx[(size_t)i] = indices ? indices[i] : i;
  for (int i0 = 0; i0 < n; i0 += t->maxb) {
    const int B = std::min(t->maxb, n - i0);
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
  const int launches = (int)t->names.size();  // kNumKernels, or kNumKernelsThird behind a third dense layer
  if (!ms || !num || capacity < launches) {
    set_error("gpd_hip_train_step_timed: ms must hold %d values", launches);
    return GPD_ERR_INVALID;
  }
  rc = check_indices("gpd_hip_train_step_timed", indices, batch, t->n[0]);
  if (rc) return rc;
  HIP_RET(hipSetDevice(t->device));
  HIP_RET(hipMemcpyAsync(t->d_idx, indices, (size_t)batch * sizeof(int32_t), hipMemcpyHostToDevice, t->stream));
  int k = 0;
  mark(t, true, k);
  enqueue_forward(t, 0, t->d_idx, batch, true, t->d_loss, true, k);
  enqueue_backward(t, t->d_idx, batch, true, k);
  enqueue_update(t, true, k);
  HIP_RET(hipGetLastError());
  HIP_RET(hipStreamSynchronize(t->stream));
  for (int i = 0; i + 1 < k; i++) HIP_RET(hipEventElapsedTime(&ms[i], t->ev[i], t->ev[i + 1]));
  *num = k - 1;
  return GPD_OK;
}

const char *gpd_hip_train_kernel_name(int i) { return i >= 0 && i < kNumKernels ? kKernelNames[i] : ""; }

const char *gpd_hip_train_kernel_name_of(const gpd_hip_trainer *t, int i) {
  if (!t) return gpd_hip_train_kernel_name(i);
  return i >= 0 && i < (int)t->names.size() ? t->names[(size_t)i] : "";
}

}  // extern "C"
