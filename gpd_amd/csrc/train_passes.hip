// Training of pytorch/network.py::Net and of the Caffe LeNet (the same network without the ReLUs behind the convolutions) on
// the device, what runs there and what enqueues it: forward with pooling argmax, backward, Adam or Caffe's SGD.
// The layer widths are the trainer's (gpd_hip_train_create_net: any gpd_lenet_shape, NetCCFFF's third dense layer included);
// the spatial sizes are constants.  The entries are train.hip's, the resident sets train_sets.hip's.
//
// Every GEMM-shaped pass is one instantiation of gemm32: a wave owns a 32 x 32 tile of the result and walks its K range with
// v_mfma_f32_32x32x2_f32, whose result is a k-ascending f32 fmaf chain.  The operands are never materialised: an operand type
// turns (row or column, k) into an address — a convolution patch, a transposed-convolution patch, the pooled gradient expanded
// to the one window position its argmax names, or a plain strided matrix — and an epilogue type turns the accumulators into
// what the pass leaves behind (pooled value + argmax byte, a raw partial, a masked gradient).  Long K ranges are split over
// grid.y into partials that sum_partials adds in a fixed tree: no floating-point atomics anywhere, so a step is a pure
// function of state, data and index list.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "train.h"

using namespace gpd;

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kP1W = 28;               // pool1: 28 x 28 (kP1)
constexpr int kP2W = 12;               // pool2: 12 x 12 (kP2)
constexpr int kO1 = 3136, kO1W = 56;   // conv1 output: 56 x 56
constexpr int kO2 = 576, kO2W = 24;    // conv2 output: 24 x 24
constexpr int kMasked = 4;             // argmax byte of a pooled value the ReLU clamped (value <= 0)

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

// ---- the launches of a step, in launch order, behind which the solver's follows; every mark() below is one of them -----------

enum { kEvery, kWithoutThird, kWithThird };  // which trainers make a launch: all, those without, those with a third dense layer
constexpr struct {
  const char *name;
  int of;
} kLaunches[] = {{"conv1_forward", kEvery}, {"conv2_forward", kEvery},    {"fc1_forward", kEvery},      {"fc1_sum_relu", kEvery},
                 {"fc2_forward", kWithThird}, {"head", kEvery},           {"loss", kEvery},             {"fc2_backward", kWithoutThird},
                 {"fc3_backward", kWithThird}, {"head_grads", kEvery},    {"fc2_dw", kWithThird},       {"fc2_dx", kWithThird},
                 {"fc1_db", kWithThird},    {"fc1_dw", kEvery},           {"fc1_dx", kEvery},           {"conv2_db", kEvery},
                 {"conv2_dw", kEvery},      {"conv2_dw_sum", kEvery},     {"conv2_dx", kEvery},         {"conv1_db", kEvery},
                 {"conv1_dw", kEvery},      {"conv1_dw_sum", kEvery}};

constexpr bool launched(int of, bool third) { return of == kEvery || of == (third ? kWithThird : kWithoutThird); }

// the launches of one step, the solver's included
constexpr int num_launches(bool third) {
  int n = 1;
  for (const auto &l : kLaunches) n += launched(l.of, third);
  return n;
}
// a timed step records an event in front of its first launch and one behind each
static_assert(num_launches(false) + 1 <= kMaxKernels && num_launches(true) + 1 <= kMaxKernels, "events");

void mark(gpd_hip_trainer *t, bool timed, int &k) {
  if (timed) (void)hipEventRecord(t->ev[k], t->stream);
  k++;
}

// forward over batch B of set `which` on the indices at d_idx; train: the loss of the batch into *d_loss_out and dlogits
template <bool RELU>
void forward_passes(gpd_hip_trainer *t, int which, const int *d_idx, int B, bool train, float *d_loss_out, bool timed, int &k) {
  hipStream_t st = t->stream;
  const gpd_lenet_shape &s = t->shape;
  const int C = s.channels, F1 = s.conv1_out, F2 = s.conv2_out, H1 = s.fc1_out, H2 = s.fc2_out, fc1_in = F2 * kP2;
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
  const gpd_lenet_shape &s = t->shape;
  const int C = s.channels, F1 = s.conv1_out, F2 = s.conv2_out, H1 = s.fc1_out, H2 = s.fc2_out, fc1_in = F2 * kP2;
  const float *p = t->d_p;
  float *g = t->d_g;
  // the layer that makes the logits (tensor `last`) and the W-wide one in front of it: its activations, its dZ, its bias gradient
  const int last = H2 > 0 ? 8 : 6;
  const int W = H2 > 0 ? H2 : H1;
  const float *act = H2 > 0 ? t->d_a2 : t->d_a1;
  float *dz = H2 > 0 ? t->d_dz2 : t->d_dz1;
  hipLaunchKernelGGL(fc2_back_kernel, dim3((B * W + 255) / 256), dim3(256), 0, st, t->d_dl, p + t->off[last], act, B, W, dz);
  mark(t, timed, k);
  hipLaunchKernelGGL(head_grads_kernel, dim3((3 * W + 2 + 255) / 256), dim3(256), 0, st, t->d_dl, act, dz, B, W, g + t->off[last],
                     g + t->off[last + 1], g + t->off[last - 1]);
  mark(t, timed, k);
  if (H2 > 0) {
    // fc2.weight [H2][H1] = dZ2^T A1, K = B
    launch_gemm(st, Plain{t->d_dz2, 1, H2, H2}, Plain{t->d_a1, 1, H1, H1}, RawStore{g + t->off[6], H2, H1}, H2, H1, B, (B + 1) & ~1);
    mark(t, timed, k);
    // dZ1 [B][H1] = dZ2 W2, K = H2, zero where fc1's ReLU clamped
    launch_gemm(st, Plain{t->d_dz2, H2, 1, B}, Plain{p + t->off[6], 1, H1, H1}, ActMaskStore{t->d_dz1, t->d_a1, B, H1}, B, H1, H2, H2);
    mark(t, timed, k);
    hipLaunchKernelGGL(batch_sum_kernel, dim3((H1 + 255) / 256), dim3(256), 0, st, t->d_dz1, B, H1, g + t->off[5]);
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

void gpd::enqueue_gradients(gpd_hip_trainer *t, const int *d_idx, int B, float *d_loss_out, bool timed, int &k) {
  enqueue_forward(t, 0, d_idx, B, true, d_loss_out, timed, k);
  if (t->r.network == GPD_TRAIN_NET_TORCH)
    backward_passes<true>(t, d_idx, B, timed, k);
  else
    backward_passes<false>(t, d_idx, B, timed, k);
}

double gpd::learning_rate(const gpd_train_recipe &r, double base_lr, long long it) {
  switch (r.lr_policy) {
    case GPD_LR_STEP: return base_lr * std::pow(r.gamma, (double)(it / r.stepsize));
    case GPD_LR_EXP: return base_lr * std::pow(r.gamma, (double)it);
    case GPD_LR_INV: return base_lr * std::pow(1.0 + r.gamma * (double)it, -r.power);
    default: return base_lr;
  }
}

std::vector<const char *> gpd::step_names(bool third, bool sgd) {
  std::vector<const char *> n;
  for (const auto &l : kLaunches)
    if (launched(l.of, third)) n.push_back(l.name);
  n.push_back(sgd ? "sgd" : "adam");
  return n;
}

namespace {

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
