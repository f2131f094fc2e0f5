// The shape-general scoring route (gpd_hip.h, "the shape-general scoring route"): the network family of the reference's
// pytorch/network.py — C -> F1 -> F2 -> H1 [-> H2] -> 2 with run-time widths — beside the kernels of lenet.hip and
// lenet_fast.hip, which are tiled for 20 / 50 / 500 and stay as they are.
//
// Definition: every output of a multiply-add layer is ONE f32 chain, acc = fmaf(w, x, acc) with k ascending from acc = 0,
// then acc + bias (the generic convolution of the CPU checker).  v_mfma_f32_32x32x2_f32 is bit for bit such a chain — lane half 0
// holds the lower k of a step, half 1 the higher — so the kernels below keep ONE accumulator set per output tile and walk k
// in order; zero steps (a k padded to an even count, a dense K padded to whole steps of 32) sit at the END of a chain, where
// fmaf(0, x, acc) leaves acc as it is.  Tiling by batch size changes which lanes work, never the order inside a chain.
// That holds for every finite weight, subnormal ones included: the kernels' f32 denormal mode is IEEE (the Makefile passes no
// denormal flag), and on the device the MFMA, the epilogues and the logit chains return subnormal operands, products, sums and
// planes bit for bit as the CPU chain does, beside values above 2^90 (tests/test_gpu_lenet_net_edges.py, the hostile set).
//
//   net_conv_pool_kernel   implicit GEMM of a 5x5 valid convolution, M = 32 filters, N = 32 POOLED pixels per wave: the four
//                          accumulators of a wave are the four pixels of the 2x2 pool windows, so the pool is a per-register
//                          max in the epilogue (max and "+ bias" commute: rounding is monotonic) and pre-pool values never
//                          leave the registers.  Loader = element type of the input planes: u8 (conv1, 60x60) or f32 (conv2,
//                          28x28).  A workgroup stages `cb` input channels and their rows of the k-major weights in the LDS
//                          at a time; cb is even whenever there is more than one chunk, so a chunk starts on an even k.
//   net_dense_kernel       out[n][U] = ReLU(X[n][K] W[K][U] + b): M = 128 units x N = 32 NB images per workgroup, K in LDS
//                          stages of 32
//   net_logits_kernel      the two logits of an image as two VALU fmaf chains, and the score y1 - y0
// That is GPD_LENET_NET_CHAIN, the default.  gpd_hip_set_lenet_net_mode (below) chooses the route's other arithmetic,
// GPD_LENET_NET_SPLIT: the kernels of lenet_net_split.hip on the bf16 matrix pipe, with the logits kernel of this file.
#include <algorithm>
#include <cstring>

#include "buffers.h"
#include "context.h"

namespace gpd {
namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int NC_MAX_WAVES = 5;  // waves of a conv workgroup, one pixel tile each: 4 for conv1 (7 workgroups per image and filter tile), 5 for conv2 (one)
constexpr int kLdsLimit = 160 * 1024;
constexpr int kConv1Waves = 4, kConv2Waves = 5;  // 25 pixel tiles: 7 workgroups of 4 (two workgroups per CU: two waves per SIMD); 5 tiles: one of 5

// input rows a workgroup of `nw` waves (tiles z * nw ...) reads: [r0, r0 + nrows) — the rows under its first to its last pooled pixel
__host__ __device__ inline void conv_rows(int P, int nw, int z, int &r0, int &nrows) {
  const int pfirst = z * nw * 32, plast = min(P * P, (z + 1) * nw * 32) - 1;
  r0 = 2 * (pfirst / P);
  nrows = 2 * (plast / P) + 6 - r0;
}

template <typename T, int HIN>
__global__ __launch_bounds__(NC_MAX_WAVES * 64) void net_conv_pool_kernel(const T *__restrict__ in, const float *__restrict__ wt,
                                                                          const float *__restrict__ bias, float *__restrict__ out, int cin,
                                                                          int cb, int a_off, int filters, int fpad, int relu, int stride_f,
                                                                          int stride_p) {
  constexpr int HW = HIN * HIN, P = (HIN - 4) / 2, PP = P * P;
  constexpr int ROW8 = HIN * sizeof(T), PLANE8 = HW * sizeof(T) / 8;  // (bytes of a row; 8-byte pieces of a plane)
  static_assert((HW * sizeof(T)) % 8 == 0 && (2 * ROW8) % 8 == 0, "planes and pairs of rows are whole 8-byte pieces");
  extern __shared__ __attribute__((aligned(16))) unsigned char net_smem[];
  T *s_in = reinterpret_cast<T *>(net_smem);                  // [cb][nrows][HIN]
  float *s_a = reinterpret_cast<float *>(net_smem + a_off);  // [cb * 25 (+ 1)][32]
  const int zero_at = (a_off + ((cb * 25 + 1) & ~1) * 128) / (int)sizeof(T);  // [HIN + 2] zeros behind the weight tile, as an index into s_in
  const int tid = threadIdx.x, nthreads = blockDim.x, nw = nthreads >> 6;
  const int wave = tid >> 6, lane = tid & 63, col = lane & 31, h = lane >> 5;
  const int img = blockIdx.x, m0 = blockIdx.y * 32;
  int r0, nrows;
  conv_rows(P, nw, blockIdx.z, r0, nrows);
  const int plane = nrows * HIN, per8 = nrows * ROW8 / 8;  // (r0 and nrows are even)
  const int nchunks = (cin + cb - 1) / cb;
  const uint2 *src8 = reinterpret_cast<const uint2 *>(in + (size_t)img * cin * HW) + r0 * ROW8 / 8;
  const int tile = blockIdx.z * nw + wave;
  const int pp = min(tile * 32 + col, PP - 1);  // (a lane past the last pixel computes the last pixel again and stores nothing)
  const int py = pp / P, px = pp - py * P;
  const int base = (2 * py - r0) * HIN + 2 * px;
  f32x16 acc0, acc1, acc2, acc3;
#pragma unroll
  for (int r = 0; r < 16; r++) acc0[r] = acc1[r] = acc2[r] = acc3[r] = 0.f;
  if (tid < HIN + 2) s_in[zero_at + tid] = T(0);  // (ahead of the first chunk's barrier)
  for (int ch = 0; ch < nchunks; ch++) {
    const int c0 = ch * cb, cc = min(cb, cin - c0);
    const int k0 = c0 * 25, kc = cc * 25, kce = (kc + 1) & ~1;
    if (ch > 0) __syncthreads();  // the readers of the previous chunk are done
    // (loads four deep and unconditional — a clamped index, a conditional store — so that they are in flight together)
    uint2 *d8 = reinterpret_cast<uint2 *>(s_in);
    const int n8 = cc * per8;
    for (int i0 = tid; i0 < n8; i0 += 4 * nthreads) {
      uint2 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int i = min(i0 + u * nthreads, n8 - 1), c = i / per8;
        v[u] = src8[(size_t)(c0 + c) * PLANE8 + (i - c * per8)];
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (i0 + u * nthreads < n8) d8[i0 + u * nthreads] = v[u];
    }
    const int n4 = kce * 8;
    for (int i0 = tid; i0 < n4; i0 += 4 * nthreads) {
      f32x4 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int i = min(i0 + u * nthreads, n4 - 1);
        v[u] = *reinterpret_cast<const f32x4 *>(wt + (size_t)(k0 + (i >> 3)) * fpad + m0 + 4 * (i & 7));
      }
#pragma unroll
      for (int u = 0; u < 4; u++)
        if (i0 + u * nthreads < n4) reinterpret_cast<f32x4 *>(s_a)[i0 + u * nthreads] = v[u];
    }
    __syncthreads();
    // the operands of step s: A[filter col][k], B[k][pixel col] for the four pixels of the pool window; k = s + h.  The odd
    // k past the last one (a zero step at the end of the chain: its weights are zeros) reads the zero area instead of a
    // plane — a select on the ADDRESS, so that the four reads stay unconditional and can be requested a step ahead
    auto fetch = [&](int s, float &a, float(&b)[4]) __attribute__((always_inline)) {
      const int kk = s + h;
      const int c = kk / 25, r = kk - 25 * c, kh = r / 5, kw = r - 5 * kh;
      const int off = kk < kc ? c * plane + kh * HIN + kw + base : zero_at;
      a = s_a[kk * 32 + col];
      b[0] = (float)s_in[off];
      b[1] = (float)s_in[off + 1];
      b[2] = (float)s_in[off + HIN];
      b[3] = (float)s_in[off + HIN + 1];
    };
    float a_cur, b_cur[4], a_nxt, b_nxt[4];
    fetch(0, a_cur, b_cur);
    for (int s = 0; s < kce; s += 2) {
      fetch(min(s + 2, kce - 2), a_nxt, b_nxt);  // requested before this step's MFMAs, arrives while they run
      __builtin_amdgcn_sched_barrier(0);
      // Grasp images have large blank areas.  A step whose 2 x 32 x 4 inputs are all zero leaves every chain where it is
      // (fmaf(w, 0, acc) = acc for the finite weights gpd_hip_set_lenet_net admits; only the sign of a zero sum can differ),
      // so the u8 loader passes it over: wave-uniform, and no reordering of what remains.
      bool work = true;
      if constexpr (sizeof(T) == 1) work = __any((b_cur[0] != 0.f) | (b_cur[1] != 0.f) | (b_cur[2] != 0.f) | (b_cur[3] != 0.f));
      if (work) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur, b_cur[0], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur, b_cur[1], acc1, 0, 0, 0);
        acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur, b_cur[2], acc2, 0, 0, 0);
        acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a_cur, b_cur[3], acc3, 0, 0, 0);
      }
      __builtin_amdgcn_sched_barrier(0);
      a_cur = a_nxt;
#pragma unroll
      for (int q = 0; q < 4; q++) b_cur[q] = b_nxt[q];
    }
  }
  if (tile * 32 + col < PP) {
    float *o = out + (size_t)img * filters * PP + (size_t)pp * stride_p;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int f = m0 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (f < filters) {
        float v = fmaxf(fmaxf(acc0[r], acc1[r]), fmaxf(acc2[r], acc3[r])) + bias[f];
        if (relu) v = fmaxf(v, 0.f);
        o[(size_t)f * stride_f] = v;
      }
    }
  }
}

constexpr int ND_THREADS = 256, ND_BK = 32, ND_BU = 128;
template <int NB>
__global__ __launch_bounds__(ND_THREADS) void net_dense_kernel(const float *__restrict__ X, int ldx, const float *__restrict__ W, int upad,
                                                               const float *__restrict__ bias, float *__restrict__ out, int ldo, int n,
                                                               int K, int U) {
  constexpr int BM = 32 * NB, SX = BM + 2;
  __shared__ __attribute__((aligned(16))) float s_w[ND_BK * ND_BU];
  __shared__ float s_x[ND_BK * SX];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, h = lane >> 5;
  const int m0 = blockIdx.x * BM, u0 = blockIdx.y * ND_BU;
  const int xm = tid >> 3, xq = tid & 7;  // X tile: eight lanes read the 128 bytes of an image's 32 k
  f32x16 acc[NB];
#pragma unroll
  for (int t = 0; t < NB; t++)
#pragma unroll
    for (int r = 0; r < 16; r++) acc[t][r] = 0.f;
  f32x4 rw[4], rx[NB];
  auto fetch = [&](int k0) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; i++) {
      const int idx = tid + ND_THREADS * i;
      rw[i] = *reinterpret_cast<const f32x4 *>(W + (size_t)(k0 + (idx >> 5)) * upad + u0 + 4 * (idx & 31));
    }
#pragma unroll
    for (int i = 0; i < NB; i++) {
      const int row = min(m0 + xm + 32 * i, n - 1);
      const int k = k0 + 4 * xq;
      f32x4 v = *reinterpret_cast<const f32x4 *>(X + (size_t)row * ldx + min(k, ldx - 4));
      // k >= K: zero steps at the end of the chain (the row's padding, or another k of the row when the address was clamped)
      if (k + 0 >= K) v.x = 0.f;
      if (k + 1 >= K) v.y = 0.f;
      if (k + 2 >= K) v.z = 0.f;
      if (k + 3 >= K) v.w = 0.f;
      rx[i] = v;
    }
  };
  const int steps = (K + ND_BK - 1) / ND_BK;
  fetch(0);
  for (int st = 0; st < steps; st++) {
    __syncthreads();  // the readers of the previous stage are done
#pragma unroll
    for (int i = 0; i < 4; i++) reinterpret_cast<f32x4 *>(s_w)[tid + ND_THREADS * i] = rw[i];
#pragma unroll
    for (int i = 0; i < NB; i++) {
      float *d = s_x + (4 * xq) * SX + xm + 32 * i;
      d[0] = rx[i].x;
      d[SX] = rx[i].y;
      d[2 * SX] = rx[i].z;
      d[3 * SX] = rx[i].w;
    }
    __syncthreads();
    fetch(min(st + 1, steps - 1) * ND_BK);  // (unconditional: the last step fetches itself again and nobody stores it)
#pragma unroll
    for (int s = 0; s < ND_BK; s += 2) {
      const float a = s_w[(s + h) * ND_BU + wave * 32 + col];
#pragma unroll
      for (int t = 0; t < NB; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, s_x[(s + h) * SX + 32 * t + col], acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < NB; t++) {
    const int m = m0 + 32 * t + col;
#pragma unroll
    for (int r = 0; r < 16; r++) {
      const int u = u0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (m < n && u < U) out[(size_t)m * ldo + u] = fmaxf(acc[t][r] + bias[u], 0.f);
    }
  }
}

constexpr int NL_THREADS = 256, NL_MAXK = 1024;
__global__ __launch_bounds__(NL_THREADS) void net_logits_kernel(const float *__restrict__ H, int ld, const float *__restrict__ w,
                                                                const float *__restrict__ b, float *__restrict__ logits,
                                                                float *__restrict__ scores, int n, int K) {
  __shared__ float ws[2 * NL_MAXK];
  for (int i = threadIdx.x; i < 2 * K; i += NL_THREADS) ws[i] = w[i];
  __syncthreads();
  const int m = blockIdx.x * NL_THREADS + threadIdx.x;
  if (m >= n) return;
  const float4 *row = reinterpret_cast<const float4 *>(H + (size_t)m * ld);
  float y0 = 0.f, y1 = 0.f;
  for (int j = 0; j < K; j += 4) {
    const float4 v = row[j >> 2];  // ld is a multiple of 4 and >= K
    const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (j + i < K) {
        y0 = __builtin_fmaf(ws[2 * (j + i)], x[i], y0);
        y1 = __builtin_fmaf(ws[2 * (j + i) + 1], x[i], y1);
      }
  }
  y0 += b[0];
  y1 += b[1];
  logits[2 * (size_t)m] = y0;
  logits[2 * (size_t)m + 1] = y1;
  scores[m] = y1 - y0;
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

// a conv launch that stages cb channels at a time, workgroups of nw waves: where the weight tile starts in the dynamic LDS
// (behind the most input rows any workgroup stages), and the LDS in all
int conv_a_off(int cb, int hin, int elem, int nw) {
  const int P = (hin - 4) / 2, zs = ((P * P + 31) / 32 + nw - 1) / nw;
  int rows = 0;
  for (int z = 0; z < zs; z++) {
    int r0, nrows;
    conv_rows(P, nw, z, r0, nrows);
    rows = std::max(rows, nrows);
  }
  return (cb * rows * hin * elem + 15) & ~15;
}
int conv_lds(int cb, int hin, int elem, int nw) {  // input rows, weight tile, hin + 2 zeros
  return conv_a_off(cb, hin, elem, nw) + ((cb * 25 + 1) & ~1) * 32 * (int)sizeof(float) + (((hin + 2) * elem + 15) & ~15);
}

template <int NB>
void dense_launch(const float *X, int ldx, const float *W, int upad, const float *bias, float *out, int ldo, int n, int K, int U, hipStream_t stream) {
  const dim3 grid((n + 32 * NB - 1) / (32 * NB), upad / ND_BU);
  net_dense_kernel<NB><<<grid, ND_THREADS, 0, stream>>>(X, ldx, W, upad, bias, out, ldo, n, K, U);
}
// image tiles of a workgroup by batch size: which lanes work, not the order of a chain
void dense(const float *X, int ldx, const float *W, int upad, const float *bias, float *out, int ldo, int n, int K, int U, hipStream_t stream) {
  if (n <= 32)
    dense_launch<1>(X, ldx, W, upad, bias, out, ldo, n, K, U, stream);
  else if (n <= 64)
    dense_launch<2>(X, ldx, W, upad, bias, out, ldo, n, K, U, stream);
  else
    dense_launch<4>(X, ldx, W, upad, bias, out, ldo, n, K, U, stream);
}

}  // namespace

void lenet_net_logits(const LeNetNet &net, const float *hid, int ldh, int K, float *logits, float *d_scores, int m, hipStream_t stream) {
  net_logits_kernel<<<(m + NL_THREADS - 1) / NL_THREADS, NL_THREADS, 0, stream>>>(hid, ldh, net.lw, net.lb, logits, d_scores, m, K);
}

void lenet_net_free(LeNetNet &net) {
  lenet_net_split_free(net);
  device_release(net.c1wt, net.c1b, net.c2wt, net.c2b, net.f1w, net.f1b, net.f2w, net.f2b, net.lw, net.lb);
  net = LeNetNet();
}

void lenet_net_scratch_free(LeNetNetScratch &s) {
  device_release(s.pool1, s.pool2, s.h1, s.h2, s.logits, s.p1s, s.xs, s.h1s);
  s = LeNetNetScratch();
}

hipError_t lenet_net_scratch_reserve(const LeNetNet &net, LeNetNetScratch &s, int n) {
  if (n <= s.capacity) return hipSuccess;
  note_alloc(__func__);
  lenet_net_scratch_free(s);
  const gpd_lenet_shape &sh = net.shape;
  const size_t cap = (size_t)std::min(net.chunk, slack_cap(n, 4));
  hipError_t e;
  if (net.mode == GPD_LENET_NET_SPLIT) {
    if ((e = lenet_net_split_scratch_alloc(net, s, cap)) != hipSuccess) return e;
    s.capacity = (int)cap;
    s.mode = net.mode;
    return hipSuccess;
  }
  if ((e = device_alloc(s.pool1, cap * sh.conv1_out * 784)) != hipSuccess) return e;
  if ((e = device_alloc(s.pool2, cap * sh.conv2_out * 144)) != hipSuccess) return e;
  if ((e = device_alloc(s.h1, cap * round_up(sh.fc1_out, 4))) != hipSuccess) return e;
  if (sh.fc2_out > 0 && (e = device_alloc(s.h2, cap * round_up(sh.fc2_out, 4))) != hipSuccess) return e;
  if ((e = device_alloc(s.logits, cap * 2)) != hipSuccess) return e;
  s.capacity = (int)cap;
  return hipSuccess;
}

hipError_t lenet_net_forward(const LeNetWeights &w, LeNetScratch &s, const uint8_t *d_images, int n, float *d_scores, hipStream_t stream,
                             hipEvent_t *kernel_events) {
  const LeNetNet &net = w.net;
  const gpd_lenet_shape &sh = net.shape;
  hipError_t e;
  // the fused entries copy the stock route's launch error word behind every scoring pass (lenet_check): it has to exist
  if (!s.c1_stats && (e = lenet_scratch_reserve(s, 1)) != hipSuccess) return e;
  LeNetNetScratch &t = s.net;
  if ((e = lenet_net_scratch_reserve(net, t, std::min(n, net.chunk))) != hipSuccess) return e;
  const int chunk = std::min(net.chunk, t.capacity);
  const int C = sh.channels, F1 = sh.conv1_out, F2 = sh.conv2_out, H1 = sh.fc1_out, H2 = sh.fc2_out;
  const int ld1 = round_up(H1, 4), ld2 = round_up(H2, 4);
  const int relu = w.conv_relu ? 1 : 0;
  for (int off = 0; off < n; off += chunk) {
    const int m = std::min(chunk, n - off);
    const bool ev = kernel_events && off == 0;
    const uint8_t *img = d_images + (size_t)off * kPix * C;
    if (net.mode == GPD_LENET_NET_SPLIT) {
      if ((e = lenet_net_split_forward(w, t, img, m, d_scores + off, stream, ev ? kernel_events : nullptr)) != hipSuccess) return e;
      continue;
    }
    net_conv_pool_kernel<uint8_t, 60><<<dim3(m, net.f1pad / 32, (25 + kConv1Waves - 1) / kConv1Waves), kConv1Waves * 64, net.lds1, stream>>>(
        img, net.c1wt, net.c1b, t.pool1, C, net.cb1, net.aoff1, F1, net.f1pad, relu, 784, 1);
    if (ev) (void)hipEventRecord(kernel_events[0], stream);
    net_conv_pool_kernel<float, 28><<<dim3(m, net.f2pad / 32, 1), kConv2Waves * 64, net.lds2, stream>>>(t.pool1, net.c2wt, net.c2b, t.pool2, F1, net.cb2,
                                                                                                       net.aoff2, F2, net.f2pad, relu, 1, F2);
    if (ev) (void)hipEventRecord(kernel_events[1], stream);
    dense(t.pool2, F2 * 144, net.f1w, net.u1pad, net.f1b, t.h1, ld1, m, F2 * 144, H1, stream);
    if (ev) (void)hipEventRecord(kernel_events[2], stream);
    const float *hid = t.h1;
    int ldh = ld1, Kl = H1;
    if (H2 > 0) {
      dense(t.h1, ld1, net.f2w, net.u2pad, net.f2b, t.h2, ld2, m, H1, H2, stream);
      hid = t.h2;
      ldh = ld2;
      Kl = H2;
    }
    net_logits_kernel<<<(m + NL_THREADS - 1) / NL_THREADS, NL_THREADS, 0, stream>>>(hid, ldh, net.lw, net.lb, t.logits, d_scores + off, m, Kl);
  }
  t.ran = true;
  return hipGetLastError();
}

}  // namespace gpd

using namespace gpd;

int gpd_hip_lenet_shape_check(const gpd_lenet_shape *s) {
  if (!s) {
    set_error("gpd_hip_lenet_shape_check: null argument");
    return GPD_ERR_INVALID;
  }
  const bool ok = (s->channels == 1 || s->channels == 3 || s->channels == 12 || s->channels == 15) && s->conv1_out >= 1 && s->conv1_out <= 64 &&
                  s->conv2_out >= 1 && s->conv2_out <= 128 && s->fc1_out >= 1 && s->fc1_out <= 1024 && s->fc2_out >= 0 && s->fc2_out <= 1024;
  if (!ok) {
    set_error("lenet shape [channels %d, conv1 %d, conv2 %d, fc1 %d, fc2 %d] is outside the limits: channels 1, 3, 12 or 15; conv1_out 1..64; "
              "conv2_out 1..128; fc1_out 1..1024; fc2_out 0..1024",
              s->channels, s->conv1_out, s->conv2_out, s->fc1_out, s->fc2_out);
    return GPD_ERR_INVALID;
  }
  return GPD_OK;
}

namespace {
// element counts of the ten tensors (either layout); 0: unused
void net_counts(const gpd_lenet_shape &s, size_t cnt[10]) {
  const size_t H2 = (size_t)s.fc2_out, N = H2 ? H2 : 2;
  cnt[0] = (size_t)s.conv1_out * s.channels * 25;
  cnt[1] = (size_t)s.conv1_out;
  cnt[2] = (size_t)s.conv2_out * s.conv1_out * 25;
  cnt[3] = (size_t)s.conv2_out;
  cnt[4] = (size_t)s.conv2_out * 144 * s.fc1_out;
  cnt[5] = (size_t)s.fc1_out;
  cnt[6] = (size_t)s.fc1_out * N;
  cnt[7] = N;
  cnt[8] = H2 ? H2 * 2 : 0;
  cnt[9] = H2 ? 2 : 0;
}
}  // namespace

int gpd_hip_lenet_net_from_torch(const gpd_lenet_shape *shape, double input_scale, const float *const t[10], float *const out[10]) {
  if (!shape || !t || !out) {
    set_error("gpd_hip_lenet_net_from_torch: null argument");
    return GPD_ERR_INVALID;
  }
  if (gpd_hip_lenet_shape_check(shape) != GPD_OK) return GPD_ERR_INVALID;
  if (!std::isfinite(input_scale) || !(input_scale > 0.0)) {
    set_error("gpd_hip_lenet_net_from_torch: input_scale must be finite and positive");
    return GPD_ERR_INVALID;
  }
  size_t cnt[10];
  net_counts(*shape, cnt);
  for (int i = 0; i < 10; i++)
    if (cnt[i] && (!t[i] || !out[i])) {
      set_error("gpd_hip_lenet_net_from_torch: tensor %d is null", i);
      return GPD_ERR_INVALID;
    }
  const int F2 = shape->conv2_out, H1 = shape->fc1_out, H2 = shape->fc2_out, N = H2 ? H2 : 2;
  for (size_t i = 0; i < cnt[0]; i++) out[0][i] = (float)((double)t[0][i] * input_scale);
  for (int i : {1, 2, 3, 5, 7, 9})
    if (cnt[i]) std::memcpy(out[i], t[i], cnt[i] * sizeof(float));
  for (int p = 0; p < 144; p++)
    for (int c = 0; c < F2; c++) {
      float *dst = out[4] + (size_t)(p * F2 + c) * H1;
      const float *src = t[4] + (size_t)c * 144 + p;
      for (int u = 0; u < H1; u++) dst[u] = src[(size_t)u * F2 * 144];
    }
  for (int j = 0; j < H1; j++)
    for (int u = 0; u < N; u++) out[6][(size_t)j * N + u] = t[6][(size_t)u * H1 + j];
  for (int j = 0; j < H2; j++)
    for (int u = 0; u < 2; u++) out[8][(size_t)j * 2 + u] = t[8][(size_t)u * H2 + j];
  return GPD_OK;
}

namespace {
// scratch bytes per image, images per pass and the largest LDS of `mode`'s kernels (lds1 / lds2: the chain's conv launches)
void net_costs(LeNetNet &net, int mode) {
  const gpd_lenet_shape &sh = net.shape;
  const int lds_dense = (ND_BK * ND_BU + ND_BK * (32 * 4 + 2)) * (int)sizeof(float), lds_logits = 2 * NL_MAXK * (int)sizeof(float);
  if (mode == GPD_LENET_NET_SPLIT) {
    net.scratch_per_image = lenet_net_split_scratch_per_image(sh);
    net.lds_max = std::max(lenet_net_split_lds(), lds_logits);
  } else {
    net.scratch_per_image = ((long long)sh.conv1_out * 784 + (long long)sh.conv2_out * 144 + round_up(sh.fc1_out, 4) + round_up(sh.fc2_out, 4) + 2) *
                            (long long)sizeof(float);
    net.lds_max = std::max(std::max(net.lds1, net.lds2), std::max(lds_dense, lds_logits));
  }
  // chunked like lenet_forward: at most 65536 images and at most 6 GiB of scratch per pass
  net.chunk = (int)std::max(1ll, std::min((long long)kLeNetChunk, (6ll << 30) / net.scratch_per_image));
}

// [rows][cols] -> device [rows_pad][cols_pad] (zeros in the padding); transpose: the source is [cols][rows]
int upload_padded(float *&dst, const float *src, int rows, int cols, int rows_pad, int cols_pad, bool transpose) {
  std::vector<float> h((size_t)rows_pad * cols_pad, 0.f);
  for (int r = 0; r < rows; r++)
    for (int c = 0; c < cols; c++) h[(size_t)r * cols_pad + c] = transpose ? src[(size_t)c * rows + r] : src[(size_t)r * cols + c];
  HIP_RET(device_alloc(dst, h.size()));
  HIP_RET(hipMemcpy(dst, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
  return GPD_OK;
}
}  // namespace

int gpd_hip_set_lenet_net(gpd_hip_ctx *ctx, const gpd_lenet_shape *shape, const float *const t[10]) {
  if (!ctx || !shape || !t) {
    set_error("gpd_hip_set_lenet_net: null argument");
    return GPD_ERR_INVALID;
  }
  if (gpd_hip_lenet_shape_check(shape) != GPD_OK) return GPD_ERR_INVALID;
  if (shape->channels != ctx->params.image_num_channels) {
    set_error("gpd_hip_set_lenet_net: channels %d != image_num_channels %d", shape->channels, ctx->params.image_num_channels);
    return GPD_ERR_INVALID;
  }
  size_t cnt[10];
  net_counts(*shape, cnt);
  static const char *names[10] = {"conv1 weight", "conv1 bias", "conv2 weight", "conv2 bias", "fc1 weight", "fc1 bias", "fc2 weight", "fc2 bias", "fc3 weight", "fc3 bias"};
  for (int i = 0; i < 10; i++) {
    if (cnt[i] && !t[i]) {
      set_error("gpd_hip_set_lenet_net: tensor %d (%s) is null", i, names[i]);
      return GPD_ERR_INVALID;
    }
    for (size_t j = 0; j < cnt[i]; j++)
      if (!std::isfinite(t[i][j])) {
        set_error("gpd_hip_set_lenet_net: %s %zu is not finite", names[i], j);
        return GPD_ERR_INVALID;
      }
  }
  const int C = shape->channels, F1 = shape->conv1_out, F2 = shape->conv2_out, H1 = shape->fc1_out, H2 = shape->fc2_out;
  LeNetNet net;
  net.shape = *shape;
  net.f1pad = round_up(F1, 32);
  net.f2pad = round_up(F2, 32);
  net.u1pad = round_up(H1, ND_BU);
  net.u2pad = H2 ? round_up(H2, ND_BU) : 0;
  // conv1 stages the (at most 16) rows its four pixel tiles read, conv2 whole planes — of at most 8 input channels at a
  // time, with their rows of the weight tile (an even count, so that a chunk starts on an even k): 33 KB and 51 KB at the
  // most, several workgroups per CU, so that one stages while another multiplies
  net.cb1 = C <= 8 ? C : 8;
  net.cb2 = F1 <= 8 ? F1 : 8;
  net.aoff1 = conv_a_off(net.cb1, 60, 1, kConv1Waves);
  net.aoff2 = conv_a_off(net.cb2, 28, 4, kConv2Waves);
  net.lds1 = conv_lds(net.cb1, 60, 1, kConv1Waves);
  net.lds2 = conv_lds(net.cb2, 28, 4, kConv2Waves);
  net_costs(net, GPD_LENET_NET_CHAIN);
  if (net.lds_max > kLdsLimit) {
    set_error("gpd_hip_set_lenet_net: the shape needs %d bytes of LDS (limit %d)", net.lds_max, kLdsLimit);
    return GPD_ERR_INVALID;
  }
  net.macs_per_image = (long long)F1 * 3136 * C * 25 + (long long)F2 * 576 * F1 * 25 + (long long)F2 * 144 * H1 + (long long)H1 * (H2 ? H2 : 2) + (long long)H2 * 2;
  HIP_RET(hipSetDevice(ctx->device));
  for (auto &L : ctx->lane)
    if (L.stream) HIP_RET(hipStreamSynchronize(L.stream));  // no kernel still reads the old network
  // until every upload has succeeded the context holds no network (as in gpd_hip_set_lenet_weights)
  ctx->lenet.channels = 0;
  lenet_net_free(ctx->lenet.net);
  for (auto &L : ctx->lane) lenet_net_scratch_free(L.lenet_scratch.net);  // sized for the previous shape
  HIP_RET(hipFuncSetAttribute(reinterpret_cast<const void *>(net_conv_pool_kernel<uint8_t, 60>), hipFuncAttributeMaxDynamicSharedMemorySize, net.lds1));
  HIP_RET(hipFuncSetAttribute(reinterpret_cast<const void *>(net_conv_pool_kernel<float, 28>), hipFuncAttributeMaxDynamicSharedMemorySize, net.lds2));
  int rc = GPD_OK;
  auto plain = [&](float *&dst, const float *src, size_t n) {
    if (rc != GPD_OK) return;
    if (device_alloc(dst, n) != hipSuccess || hipMemcpy(dst, src, n * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      set_error("gpd_hip_set_lenet_net: uploading the network failed: %s", hipGetErrorString(hipGetLastError()));
      rc = GPD_ERR_HIP;
    }
  };
  auto padded = [&](float *&dst, const float *src, int rows, int cols, int rows_pad, int cols_pad, bool transpose) {
    if (rc == GPD_OK) rc = upload_padded(dst, src, rows, cols, rows_pad, cols_pad, transpose);
  };
  const int K1 = C * 25, K2 = F1 * 25, Kf = F2 * 144;
  padded(net.c1wt, t[0], K1, F1, round_up(K1, 2), net.f1pad, true);  // [F1][K1] -> k-major
  plain(net.c1b, t[1], F1);
  padded(net.c2wt, t[2], K2, F2, round_up(K2, 2), net.f2pad, true);
  plain(net.c2b, t[3], F2);
  padded(net.f1w, t[4], Kf, H1, round_up(Kf, ND_BK), net.u1pad, false);
  plain(net.f1b, t[5], H1);
  if (H2 > 0) {
    padded(net.f2w, t[6], H1, H2, round_up(H1, ND_BK), net.u2pad, false);
    plain(net.f2b, t[7], H2);
    plain(net.lw, t[8], (size_t)H2 * 2);
    plain(net.lb, t[9], 2);
  } else {
    plain(net.lw, t[6], (size_t)H1 * 2);
    plain(net.lb, t[7], 2);
  }
  // the mode met the network: the piece tables, and the scratch, chunk and LDS of the mode in force
  if (rc == GPD_OK) rc = lenet_net_apply_mode(net, ctx->lenet.net_mode);
  if (rc != GPD_OK) {
    lenet_net_free(net);
    return rc;
  }
  net.active = true;
  ctx->lenet.net = net;
  ctx->lenet.channels = C;
  return GPD_OK;
}

namespace gpd {
int lenet_net_apply_mode(LeNetNet &net, int mode) {
  if (mode == GPD_LENET_NET_SPLIT) {
    if (lenet_net_split_lds() > kLdsLimit) {
      set_error("gpd_hip_set_lenet_net_mode: the split kernels need %d bytes of LDS (limit %d)", lenet_net_split_lds(), kLdsLimit);
      return GPD_ERR_INVALID;
    }
    if (int rc = lenet_net_split_prepare(net)) return rc;
  } else {
    lenet_net_split_free(net);
  }
  net.mode = mode;
  net_costs(net, mode);
  return GPD_OK;
}
}  // namespace gpd

// Context state like gpd_hip_set_lenet_conv_relu: kept across installs and gpd_hip_set_lenet_weights.  With a network installed
// the mode meets it here: the piece tables are built (or freed), and — the two modes' scratch differs — the general-route
// scratch of every lane is freed, as an install frees it.
int gpd_hip_set_lenet_net_mode(gpd_hip_ctx *ctx, int mode) {
  if (int rc = refuse("gpd_hip_set_lenet_net_mode", ctx, mode == GPD_LENET_NET_CHAIN || mode == GPD_LENET_NET_SPLIT)) return rc;
  LeNetNet &net = ctx->lenet.net;
  if (net.active && net.mode != mode) {
    HIP_RET(hipSetDevice(ctx->device));
    for (auto &L : ctx->lane)
      if (L.stream) HIP_RET(hipStreamSynchronize(L.stream));  // no kernel still reads the tables or the scratch
    for (auto &L : ctx->lane) lenet_net_scratch_free(L.lenet_scratch.net);
    if (int rc = lenet_net_apply_mode(net, mode)) return rc;  // (a failure leaves the mode and the network as they were, without piece tables)
  }
  ctx->lenet.net_mode = mode;
  return GPD_OK;
}

int gpd_hip_lenet_net_info(gpd_hip_ctx *ctx, long long info[4]) {
  if (!ctx || !info) {
    set_error("gpd_hip_lenet_net_info: null argument");
    return GPD_ERR_INVALID;
  }
  const LeNetNet &net = ctx->lenet.net;
  if (!net.active) {
    set_error("gpd_hip_lenet_net_info: no network installed by gpd_hip_set_lenet_net");
    return GPD_ERR_STATE;
  }
  info[0] = net.chunk;
  info[1] = net.scratch_per_image;
  info[2] = net.lds_max;
  info[3] = net.macs_per_image;
  return GPD_OK;
}

int gpd_hip_lenet_net_debug(gpd_hip_ctx *ctx, int which, int n, float *out) {
  if (!ctx || !out || n < 1 || which < 0 || which > 4) {
    set_error("gpd_hip_lenet_net_debug: bad argument");
    return GPD_ERR_INVALID;
  }
  Lane &L = ctx->lane[0];
  const LeNetNetScratch &t = L.lenet_scratch.net;
  const LeNetNet &net = ctx->lenet.net;
  if (!net.active || !t.ran) {
    set_error("gpd_hip_lenet_net_debug: the last scoring call did not take the general route");
    return GPD_ERR_INVALID;
  }
  if (n > t.capacity) {
    set_error("gpd_hip_lenet_net_debug: n = %d exceeds the first chunk (%d images)", n, t.capacity);
    return GPD_ERR_INVALID;
  }
  const gpd_lenet_shape &sh = net.shape;
  if (which == 3 && sh.fc2_out == 0) {
    set_error("gpd_hip_lenet_net_debug: which = 3 on a network without fc2");
    return GPD_ERR_INVALID;
  }
  HIP_RET(hipSetDevice(ctx->device));
  HIP_RET(hipStreamSynchronize(L.stream));
  if (net.mode == GPD_LENET_NET_SPLIT && (which <= 1 || (which == 2 && sh.fc2_out > 0))) return lenet_net_split_debug(net, t, which, n, out);
  if (which == 0) {
    HIP_RET(hipMemcpy(out, t.pool1, (size_t)n * sh.conv1_out * 784 * sizeof(float), hipMemcpyDeviceToHost));
  } else if (which == 1) {  // the device keeps pool2 pixel-major (fc1's k order)
    const int F2 = sh.conv2_out;
    std::vector<float> h((size_t)n * F2 * 144);
    HIP_RET(hipMemcpy(h.data(), t.pool2, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (int m = 0; m < n; m++)
      for (int p = 0; p < 144; p++)
        for (int c = 0; c < F2; c++) out[((size_t)m * F2 + c) * 144 + p] = h[((size_t)m * 144 + p) * F2 + c];
  } else if (which == 2 || which == 3) {
    const int U = which == 2 ? sh.fc1_out : sh.fc2_out;
    HIP_RET(hipMemcpy2D(out, (size_t)U * sizeof(float), which == 2 ? t.h1 : t.h2, (size_t)round_up(U, 4) * sizeof(float), (size_t)U * sizeof(float),
                        n, hipMemcpyDeviceToHost));
  } else {
    HIP_RET(hipMemcpy(out, t.logits, (size_t)n * 2 * sizeof(float), hipMemcpyDeviceToHost));
  }
  return GPD_OK;
}
