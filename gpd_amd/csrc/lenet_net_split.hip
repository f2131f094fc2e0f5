// GPD_LENET_NET_SPLIT: the shape-general route (lenet_net.hip) on the bf16 matrix pipe, v_mfma_f32_16x16x32_bf16 with exactly
// split operands (bf16_split.h: a = h + m + l) and f32 accumulation.
//
// Definition (gpd_hip.h, gpd_hip_set_lenet_net_mode).  conv1: the u8 inputs are ONE exact bf16 piece, the weights three: the
// products x*h, x*m, x*l per term, nothing dropped.  conv2, fc1, fc2: both operands three pieces, the six products
// h*h, h*m, m*h, h*l, l*h, m*m (activation piece first) in that order per k-step; m*l, l*m, l*l are dropped.  An output's
// products go into two f32 accumulators (the first product of the lists above into one, the others into the second: mfma6),
// which are added once behind the last k-step.  Then the max over the 2x2 window on those sums, + bias, the optional ReLU —
// as in the chain kernels.  The 2-logit layer is the chain's net_logits_kernel on the last hidden layer, which therefore leaves
// its dense kernel as f32.
// Order: k-steps of 32 ascending, that one pair of accumulators per output, no split-K, no atomics.  Which k a step holds is fixed by the shape:
//   convolutions   chunks of 8 input channels; inside a chunk k = tap * 8 + channel, 25 taps padded to 28 (7 k-steps: the
//                  padded taps multiply zero weights); the channels padded to whole chunks with zero weights AND zero activations
//   fc1            k = pixel * round_up(F2, 8) + channel (what conv2's epilogue writes), 144 * that: whole k-steps
//   fc2            k = the hidden index, padded to whole k-steps with zeros on both sides
// Activations are split where they are PRODUCED (the epilogues of conv1, conv2 and of a dense layer that feeds another write
// three bf16 planes in the layout the consumer's loader takes as 16-byte operand reads), as the stock conv2 does for ip1: a
// value is split once, not once per consumer tile, and the consumers stage plain copies.
//
//   net_conv_split_kernel   implicit GEMM, an MFMA tile = 16 conv pixels (four 2x2 pool windows, pixel = 4 window + position:
//                           a lane's four accumulator registers are ONE window, the pool needs no lane traffic) x 16 filters.
//                           A wave holds 4 pixel tiles x 2 filter tiles; a workgroup = the waves of 4 pooled rows of conv1 (7)
//                           or of the whole conv2 plane (9), and stages per chunk the input rows as [piece][row][col][8 ch] bf16
//                           and the chunk's weight fragments (16-byte operand reads of both, the weights' conflict-free).
//   net_dense_split_kernel  out[n][U] = ReLU(X W + b): 16 NT images x 128 units per workgroup (4 waves x 2 unit tiles); X in LDS
//                           stages of 128 k with the next stage's loads in flight, the weight fragments of a wave (nobody
//                           else's) straight from memory a k-step ahead.  NT = 1 / 2 / 4 by batch size: which lanes work, not the order.
#include <algorithm>
#include <cstring>
#include <vector>

#include "bf16_split.h"
#include "buffers.h"
#include "gpd_internal.h"

namespace gpd {
namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ inline bf16x8 as_bf16x8(const uint4 &v) {
  bf16x8 r;
  __builtin_memcpy(&r, &v, 16);
  return r;
}

int round_up(int v, int m) { return (v + m - 1) / m * m; }

constexpr int SC_PT = 4, SC_FT = 2, SC_KS = 7;
constexpr int SC_WTILE = SC_KS * 3 * 64;  // 16-byte fragments of a (chunk, filter tile): 21504 bytes

template <int HIN, bool U8IN>
struct ConvGeo {
  static constexpr int P = (HIN - 4) / 2, PP = P * P;
  static constexpr int RPW = U8IN ? 4 : P;            // pooled rows of a workgroup
  static constexpr int NW = RPW * P / (4 * SC_PT);    // its waves: 16 pooled pixels each
  static constexpr int NROWS = 2 * RPW + 4;           // input rows it stages
  static constexpr int NP = U8IN ? 1 : 3;             // pieces of the input
  static constexpr int IN_U4 = NP * NROWS * HIN;      // 16 bytes per (piece, pixel): 8 channels
  static constexpr int LDS = (IN_U4 + SC_FT * SC_WTILE) * 16;
  static_assert(RPW * P % (4 * SC_PT) == 0 && P % RPW == 0 && P % 4 == 0, "whole waves, whole workgroups, a tile inside a pooled row");
  static_assert(U8IN || NROWS == HIN, "conv2 stages whole planes");
};

// An output has TWO f32 accumulators: `hi` takes the h*h products, `lo` the cross products, which are 2^-8 of them and less;
// the output is hi + lo, added once behind the last k-step.  The large accumulator is then rounded once per k-step instead of
// six times, and the roundings of the small one weigh 2^-8 as much (measured: with one accumulator the 42 roundings of a
// K = 25 convolution reached 25 ulps, as many as a k = 150 chain's) — and the matrix pipe has two independent chains to fill.
// the six piece products of a k-step (a: activation pieces, b: weight pieces), in the order of the definition
__device__ inline void mfma6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 &hi, f32x4 &lo) {
  hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], hi, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], lo, 0, 0, 0);
}

// in: U8IN: planar u8 [n][cin][3600]; else the three bf16 planes conv1 wrote, [n][nchunks][3][784][8]
// out: U8IN: those planes; else fc1's rows [n][3][kpad], k = pixel * fstore + filter
template <int HIN, bool U8IN>
__global__ __launch_bounds__((ConvGeo<HIN, U8IN>::NW * 64)) void net_conv_split_kernel(const void *__restrict__ in, const uint4 *__restrict__ wfrag,
                                                                                    const float *__restrict__ bias, unsigned short *__restrict__ out,
                                                                                    int cin, int nchunks, int ftiles, int nf16, int filters, int fstore,
                                                                                    int relu, int kpad) {
  using G = ConvGeo<HIN, U8IN>;
  constexpr int NP = G::NP, PLANE = G::NROWS * HIN;
  extern __shared__ uint4 split_smem[];
  uint4 *s_w = split_smem;                                    // [live filter tiles of the launch][SC_KS][3][64]
  uint4 *s_in = split_smem + min(SC_FT, nf16) * SC_WTILE;     // [NP][NROWS][HIN]
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, g = lane >> 4;
  constexpr int nthreads = G::NW * 64;
  const int img = blockIdx.x, ft0 = blockIdx.y * SC_FT, r0 = 2 * G::RPW * blockIdx.z;
  const int unit = blockIdx.z * G::NW + wave;
  const int nft = min(SC_FT, nf16 - ft0);  // live filter tiles of this workgroup (>= 1)
  int abase[SC_PT];
#pragma unroll
  for (int t = 0; t < SC_PT; t++) {
    const int pp = 16 * unit + 4 * t + (m >> 2);
    const int py = pp / G::P, px = pp - py * G::P;
    abase[t] = (2 * py + ((m >> 1) & 1) - r0) * HIN + 2 * px + (m & 1);
  }
  f32x4 acc[SC_PT][SC_FT], low[SC_PT][SC_FT];
#pragma unroll
  for (int t = 0; t < SC_PT; t++)
#pragma unroll
    for (int f = 0; f < SC_FT; f++) acc[t][f] = low[t][f] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ch = 0; ch < nchunks; ch++) {
    if (ch > 0) __syncthreads();  // the readers of the previous chunk are done
    if constexpr (U8IN) {
      // eight channel planes -> one 16-byte pixel of bf16 (a u8 is exact in bf16's 8 significant bits); channels past cin: zeros
      const uint8_t *src = static_cast<const uint8_t *>(in) + (size_t)img * cin * (HIN * HIN) + r0 * HIN;
      const int c0 = ch * 8;
      for (int i = tid; i < PLANE; i += nthreads) {
        uint32_t wds[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const int ca = c0 + 2 * j, cb = ca + 1;
          const uint32_t lo = ca < cin ? __float_as_uint((float)src[(size_t)ca * (HIN * HIN) + i]) >> 16 : 0u;
          const uint32_t hi = cb < cin ? __float_as_uint((float)src[(size_t)cb * (HIN * HIN) + i]) & 0xffff0000u : 0u;
          wds[j] = lo | hi;
        }
        s_in[i] = make_uint4(wds[0], wds[1], wds[2], wds[3]);
      }
    } else {
      const uint4 *src = static_cast<const uint4 *>(in) + ((size_t)img * nchunks + ch) * (3 * PLANE);
      for (int i = tid; i < 3 * PLANE; i += nthreads) s_in[i] = src[i];
    }
    {
      const uint4 *src = wfrag + ((size_t)ch * ftiles + ft0) * SC_WTILE;
      for (int i = tid; i < nft * SC_WTILE; i += nthreads) s_w[i] = src[i];
    }
    __syncthreads();
    for (int s = 0; s < SC_KS; s++) {
      const int tap = min(4 * s + g, 24);  // (taps 25..27: zero weights; any finite activation will do)
      const int ky = tap / 5, kx = tap - 5 * ky, toff = ky * HIN + kx;
      bf16x8 a[SC_PT][NP];
#pragma unroll
      for (int t = 0; t < SC_PT; t++)
#pragma unroll
        for (int p = 0; p < NP; p++) a[t][p] = as_bf16x8(s_in[p * PLANE + abase[t] + toff]);
#pragma unroll
      for (int f = 0; f < SC_FT; f++) {
        if (f < nft) {
          bf16x8 b[3];
#pragma unroll
          for (int p = 0; p < 3; p++) b[p] = as_bf16x8(s_w[((f * SC_KS + s) * 3 + p) * 64 + lane]);
#pragma unroll
          for (int t = 0; t < SC_PT; t++) {
            if constexpr (U8IN) {
              acc[t][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t][0], b[0], acc[t][f], 0, 0, 0);
              low[t][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t][0], b[1], low[t][f], 0, 0, 0);
              low[t][f] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t][0], b[2], low[t][f], 0, 0, 0);
            } else {
              mfma6(a[t], b, acc[t][f], low[t][f]);
            }
          }
        }
      }
    }
  }
  // D: lane (filter m, window g), registers = the window's four pixels
#pragma unroll
  for (int f = 0; f < SC_FT; f++) {
    const int flt = 16 * (ft0 + f) + m;
    if (f < nft && flt < fstore) {
      const float bv = flt < filters ? bias[flt] : 0.f;
#pragma unroll
      for (int t = 0; t < SC_PT; t++) {
        const int pp = 16 * unit + 4 * t + g;
        const f32x4 sum = acc[t][f] + low[t][f];
        float v = fmaxf(fmaxf(sum[0], sum[1]), fmaxf(sum[2], sum[3])) + bv;
        if (relu) v = fmaxf(v, 0.f);
        if (flt >= filters) v = 0.f;  // the channel padding the consumer multiplies with zero weights
        const Bf3 sp = bf16_split3(v);
        if constexpr (U8IN) {
          unsigned short *o = out + (size_t)img * (fstore / 8) * (3 * G::PP * 8) + (size_t)(flt >> 3) * (3 * G::PP * 8) + pp * 8 + (flt & 7);
          o[0] = sp.h;
          o[G::PP * 8] = sp.m;
          o[2 * G::PP * 8] = sp.l;
        } else {
          unsigned short *o = out + (size_t)img * 3 * kpad + (size_t)pp * fstore + flt;
          o[0] = sp.h;
          o[kpad] = sp.m;
          o[2 * (size_t)kpad] = sp.l;
        }
      }
    }
  }
}

constexpr int SD_THREADS = 256, SD_UT = 2, SD_KST = 4;  // 4 waves x 2 unit tiles; k-steps per LDS stage
constexpr int SD_PITCH = 4 * SD_KST + 1;                // 16-byte pieces per (piece, image) row of a stage, + 1: conflict-free reads

// X: [n][3][kpad] bf16 (kpad = 32 ksteps, the padding zeros); wfrag: [unit tile][ksteps][3][64] fragments, the tiles padded to
// whole workgroups; out32 (the last hidden layer) [n][ldo] f32 and / or outs [n][3][kpad_out] bf16 planes
template <int NT>
__global__ __launch_bounds__(SD_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void net_dense_split_kernel(const unsigned short *__restrict__ X, const uint4 *__restrict__ wfrag,
                                                                     const float *__restrict__ bias, float *__restrict__ out32, int ldo,
                                                                     unsigned short *__restrict__ outs, int kpad_out, int n, int ksteps, int U,
                                                                     int nu16) {
  constexpr int BM = 16 * NT, ITEMS = 3 * NT;  // 16-byte loads of a thread per stage: 3 pieces x BM images x 16 / 256
  __shared__ uint4 s_x[3 * BM * SD_PITCH];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, m = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * BM, ut0 = (blockIdx.y * 4 + wave) * SD_UT;
  const int nut = min(SD_UT, nu16 - ut0);  // live unit tiles of this wave (may be <= 0: it only stages)
  const size_t kpad = (size_t)ksteps * 32;
  const int nstages = (ksteps + SD_KST - 1) / SD_KST;
  f32x4 acc[NT][SD_UT], low[NT][SD_UT];
#pragma unroll
  for (int t = 0; t < NT; t++)
#pragma unroll
    for (int u = 0; u < SD_UT; u++) acc[t][u] = low[t][u] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint4 rx[ITEMS];
  auto fetch_x = [&](int st) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
      const int idx = tid + SD_THREADS * i;
      const int q = idx & 15, row = (idx >> 4) % BM, p = idx / (16 * BM);
      const int ks = st * SD_KST + (q >> 2);
      const int r = min(m0 + row, n - 1);
      uint4 v = make_uint4(0u, 0u, 0u, 0u);
      if (ks < ksteps) v = *reinterpret_cast<const uint4 *>(X + ((size_t)r * 3 + p) * kpad + (size_t)ks * 32 + (q & 3) * 8);
      rx[i] = v;
    }
  };
  auto frag_w = [&](int ks, bf16x8(&b)[SD_UT][3]) __attribute__((always_inline)) {
#pragma unroll
    for (int u = 0; u < SD_UT; u++)
#pragma unroll
      for (int p = 0; p < 3; p++) b[u][p] = as_bf16x8(wfrag[(((size_t)(ut0 + u) * ksteps + ks) * 3 + p) * 64 + lane]);
  };
  bf16x8 b_cur[SD_UT][3], b_nxt[SD_UT][3];
  fetch_x(0);
  frag_w(0, b_cur);  // (the table is padded to whole workgroups: an idle wave reads zeros)
  for (int st = 0; st < nstages; st++) {
    __syncthreads();  // the readers of the previous stage are done
#pragma unroll
    for (int i = 0; i < ITEMS; i++) {
      const int idx = tid + SD_THREADS * i;
      s_x[(idx >> 4) * SD_PITCH + (idx & 15)] = rx[i];  // (idx >> 4 = piece * BM + image)
    }
    __syncthreads();
    fetch_x(min(st + 1, nstages - 1));  // (unconditional: the last stage fetches itself again and nobody stores it)
    const int kn = min(SD_KST, ksteps - st * SD_KST);
    for (int s = 0; s < kn; s++) {
      const int ks = st * SD_KST + s;
      frag_w(min(ks + 1, ksteps - 1), b_nxt);
      if (nut > 0) {
        bf16x8 a[NT][3];
#pragma unroll
        for (int t = 0; t < NT; t++)
#pragma unroll
          for (int p = 0; p < 3; p++) a[t][p] = as_bf16x8(s_x[(p * BM + 16 * t + m) * SD_PITCH + 4 * s + g]);
#pragma unroll
        for (int u = 0; u < SD_UT; u++)
          if (u < nut) {
#pragma unroll
            for (int t = 0; t < NT; t++) mfma6(a[t], b_cur[u], acc[t][u], low[t][u]);
          }
      }
#pragma unroll
      for (int u = 0; u < SD_UT; u++)
#pragma unroll
        for (int p = 0; p < 3; p++) b_cur[u][p] = b_nxt[u][p];
    }
  }
  // D: lane (unit m), registers = images 4 g + r of the tile
#pragma unroll
  for (int u = 0; u < SD_UT; u++) {
    const int unit = 16 * (ut0 + u) + m;
    if (u < nut && unit < U) {
      const float bv = bias[unit];
#pragma unroll
      for (int t = 0; t < NT; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int row = m0 + 16 * t + 4 * g + r;
          if (row < n) {
            const float v = fmaxf((acc[t][u][r] + low[t][u][r]) + bv, 0.f);
            if (out32) out32[(size_t)row * ldo + unit] = v;
            if (outs) {
              const Bf3 sp = bf16_split3(v);
              unsigned short *o = outs + (size_t)row * 3 * kpad_out + unit;
              o[0] = sp.h;
              o[kpad_out] = sp.m;
              o[2 * (size_t)kpad_out] = sp.l;
            }
          }
        }
    }
  }
}

template <int NT>
void dense_split_launch(const unsigned short *X, const uint4 *wfrag, const float *bias, float *out32, int ldo, unsigned short *outs, int kpad_out, int n,
                        int kpad, int U, hipStream_t stream) {
  const int nu16 = (U + 15) / 16;
  const dim3 grid((n + 16 * NT - 1) / (16 * NT), (nu16 + 4 * SD_UT - 1) / (4 * SD_UT));
  net_dense_split_kernel<NT><<<grid, SD_THREADS, 0, stream>>>(X, wfrag, bias, out32, ldo, outs, kpad_out, n, kpad / 32, U, nu16);
}
// image tiles of a workgroup by batch size: which lanes work, not the order of the k-steps
void dense_split(const unsigned short *X, const uint4 *wfrag, const float *bias, float *out32, int ldo, unsigned short *outs, int kpad_out, int n, int kpad,
                 int U, hipStream_t stream) {
  if (n <= 16)
    dense_split_launch<1>(X, wfrag, bias, out32, ldo, outs, kpad_out, n, kpad, U, stream);
  else if (n <= 32)
    dense_split_launch<2>(X, wfrag, bias, out32, ldo, outs, kpad_out, n, kpad, U, stream);
  else
    dense_split_launch<4>(X, wfrag, bias, out32, ldo, outs, kpad_out, n, kpad, U, stream);
}

using Conv1 = ConvGeo<60, true>;
using Conv2 = ConvGeo<28, false>;

int upload_u16(uint4 *&dst, const std::vector<unsigned short> &tab) {
  HIP_RET(device_alloc(dst, tab.size() / 8));
  HIP_RET(hipMemcpy(dst, tab.data(), tab.size() * sizeof(unsigned short), hipMemcpyHostToDevice));
  return GPD_OK;
}

// the chain's k-major conv table [round_up(cin * 25, 2)][fpad] (k = channel * 25 + tap) -> B fragments: lane (filter l & 15,
// k group l >> 4) of k-step s holds tap 4 s + (l >> 4), channels 8 chunk + 0..7
int conv_table(uint4 *&dst, int &ftiles, const float *dev_wt, int cin, int F, int fpad) {
  std::vector<float> w((size_t)round_up(cin * 25, 2) * fpad);
  HIP_RET(hipMemcpy(w.data(), dev_wt, w.size() * sizeof(float), hipMemcpyDeviceToHost));
  const int nch = (cin + 7) / 8, nf16 = (F + 15) / 16;
  ftiles = round_up(nf16, SC_FT);
  std::vector<unsigned short> tab((size_t)nch * ftiles * SC_WTILE * 8, 0);
  for (int ch = 0; ch < nch; ch++)
    for (int ft = 0; ft < nf16; ft++)
      for (int s = 0; s < SC_KS; s++)
        for (int lane = 0; lane < 64; lane++)
          for (int j = 0; j < 8; j++) {
            const int f = 16 * ft + (lane & 15), tap = 4 * s + (lane >> 4), c = 8 * ch + j;
            if (f >= F || tap >= 25 || c >= cin) continue;
            const Bf3 sp = bf16_split3(w[(size_t)(c * 25 + tap) * fpad + f]);
            const size_t at = ((((size_t)ch * ftiles + ft) * SC_KS + s) * 3 * 64 + lane) * 8 + j;
            tab[at] = sp.h;
            tab[at + 64 * 8] = sp.m;
            tab[at + 2 * 64 * 8] = sp.l;
          }
  return upload_u16(dst, tab);
}

// the chain's k-major dense table [..][upad] -> B fragments [unit tile][k-step][3][64] x 8; src_row(k): the chain's row of
// this route's k, or -1 for a k that multiplies zeros
template <typename RowOf>
int dense_table(uint4 *&dst, const float *dev_w, size_t dev_rows, int upad, int kpad, int U, RowOf src_row) {
  std::vector<float> w(dev_rows * upad);
  HIP_RET(hipMemcpy(w.data(), dev_w, w.size() * sizeof(float), hipMemcpyDeviceToHost));
  const int ksteps = kpad / 32, ut_pad = round_up((U + 15) / 16, 4 * SD_UT);
  std::vector<unsigned short> tab((size_t)ut_pad * ksteps * 3 * 64 * 8, 0);
  for (int k = 0; k < kpad; k++) {
    const long long row = src_row(k);
    if (row < 0) continue;
    const int s = k >> 5, kg = (k >> 3) & 3, j = k & 7;
    const float *wr = w.data() + (size_t)row * upad;
    for (int u = 0; u < U; u++) {
      const Bf3 sp = bf16_split3(wr[u]);
      const size_t at = ((((size_t)(u >> 4) * ksteps + s) * 3) * 64 + (kg * 16 + (u & 15))) * 8 + j;
      tab[at] = sp.h;
      tab[at + 64 * 8] = sp.m;
      tab[at + 2 * 64 * 8] = sp.l;
    }
  }
  return upload_u16(dst, tab);
}

}  // namespace

void lenet_net_split_free(LeNetNet &net) {
  device_release(net.s_c1, net.s_c2, net.s_f1, net.s_f2);
  net.s_ft1 = net.s_ft2 = net.s_k1 = net.s_k2 = 0;
}

int lenet_net_split_lds() { return std::max(std::max(Conv1::LDS, Conv2::LDS), 3 * 64 * SD_PITCH * 16); }

long long lenet_net_split_scratch_per_image(const gpd_lenet_shape &sh) {
  const long long F1p = round_up(sh.conv1_out, 8), K1 = 144ll * round_up(sh.conv2_out, 8), K2 = round_up(sh.fc1_out, 32);
  long long b = F1p * 784 * 6 + K1 * 6 + 2 * sizeof(float);
  if (sh.fc2_out > 0)
    b += K2 * 6 + (long long)round_up(sh.fc2_out, 4) * sizeof(float);
  else
    b += (long long)round_up(sh.fc1_out, 4) * sizeof(float);
  return b;
}

int lenet_net_split_prepare(LeNetNet &net) {
  lenet_net_split_free(net);
  const gpd_lenet_shape &sh = net.shape;
  const int C = sh.channels, F1 = sh.conv1_out, F2 = sh.conv2_out, H1 = sh.fc1_out, H2 = sh.fc2_out;
  const int F2p = round_up(F2, 8);
  net.s_k1 = 144 * F2p;
  net.s_k2 = H2 > 0 ? round_up(H1, 32) : 0;
  HIP_RET(hipFuncSetAttribute(reinterpret_cast<const void *>(net_conv_split_kernel<60, true>), hipFuncAttributeMaxDynamicSharedMemorySize, Conv1::LDS));
  HIP_RET(hipFuncSetAttribute(reinterpret_cast<const void *>(net_conv_split_kernel<28, false>), hipFuncAttributeMaxDynamicSharedMemorySize, Conv2::LDS));
  int rc = conv_table(net.s_c1, net.s_ft1, net.c1wt, C, F1, net.f1pad);
  if (!rc) rc = conv_table(net.s_c2, net.s_ft2, net.c2wt, F1, F2, net.f2pad);
  if (!rc)
    rc = dense_table(net.s_f1, net.f1w, (size_t)round_up(F2 * 144, 32), net.u1pad, net.s_k1, H1, [&](int k) -> long long {
      const int p = k / F2p, c = k - p * F2p;
      return c < F2 ? (long long)p * F2 + c : -1;
    });
  if (!rc && H2 > 0)
    rc = dense_table(net.s_f2, net.f2w, (size_t)round_up(H1, 32), net.u2pad, net.s_k2, H2, [&](int k) -> long long { return k < H1 ? k : -1; });
  if (rc) lenet_net_split_free(net);
  return rc;
}

hipError_t lenet_net_split_scratch_alloc(const LeNetNet &net, LeNetNetScratch &s, size_t cap) {
  const gpd_lenet_shape &sh = net.shape;
  hipError_t e;
  if ((e = device_alloc(s.p1s, cap * round_up(sh.conv1_out, 8) * 784 * 3)) != hipSuccess) return e;
  if ((e = device_alloc(s.xs, cap * 3 * net.s_k1)) != hipSuccess) return e;
  if (sh.fc2_out > 0) {
    if ((e = device_alloc(s.h1s, cap * 3 * net.s_k2)) != hipSuccess) return e;
    if ((e = hipMemset(s.h1s, 0, cap * 3 * net.s_k2 * sizeof(unsigned short))) != hipSuccess) return e;  // the k past fc1_out
    if ((e = device_alloc(s.h2, cap * round_up(sh.fc2_out, 4))) != hipSuccess) return e;
  } else if ((e = device_alloc(s.h1, cap * round_up(sh.fc1_out, 4))) != hipSuccess) {
    return e;
  }
  return device_alloc(s.logits, cap * 2);
}

hipError_t lenet_net_split_forward(const LeNetWeights &w, LeNetNetScratch &t, const uint8_t *img, int m, float *d_scores, hipStream_t stream,
                                   hipEvent_t *kernel_events) {
  const LeNetNet &net = w.net;
  const gpd_lenet_shape &sh = net.shape;
  const int C = sh.channels, F1 = sh.conv1_out, F2 = sh.conv2_out, H1 = sh.fc1_out, H2 = sh.fc2_out;
  const int F1p = round_up(F1, 8), F2p = round_up(F2, 8), nf1 = (F1 + 15) / 16, nf2 = (F2 + 15) / 16;
  const int relu = w.conv_relu ? 1 : 0;
  // (a network with one filter tile stages one: more workgroups share a CU)
  const int lds1 = Conv1::LDS - (SC_FT - std::min(SC_FT, nf1)) * SC_WTILE * 16, lds2 = Conv2::LDS - (SC_FT - std::min(SC_FT, nf2)) * SC_WTILE * 16;
  net_conv_split_kernel<60, true><<<dim3(m, (nf1 + SC_FT - 1) / SC_FT, Conv1::P / Conv1::RPW), Conv1::NW * 64, lds1, stream>>>(
      img, net.s_c1, net.c1b, t.p1s, C, (C + 7) / 8, net.s_ft1, nf1, F1, F1p, relu, 0);
  if (kernel_events) (void)hipEventRecord(kernel_events[0], stream);
  net_conv_split_kernel<28, false><<<dim3(m, (nf2 + SC_FT - 1) / SC_FT, 1), Conv2::NW * 64, lds2, stream>>>(
      t.p1s, net.s_c2, net.c2b, t.xs, F1, F1p / 8, net.s_ft2, nf2, F2, F2p, relu, net.s_k1);
  if (kernel_events) (void)hipEventRecord(kernel_events[1], stream);
  const int ld1 = round_up(H1, 4), ld2 = round_up(H2, 4);
  if (H2 > 0) {
    dense_split(t.xs, net.s_f1, net.f1b, nullptr, 0, t.h1s, net.s_k2, m, net.s_k1, H1, stream);
    if (kernel_events) (void)hipEventRecord(kernel_events[2], stream);
    dense_split(t.h1s, net.s_f2, net.f2b, t.h2, ld2, nullptr, 0, m, net.s_k2, H2, stream);
    lenet_net_logits(net, t.h2, ld2, H2, t.logits, d_scores, m, stream);
  } else {
    dense_split(t.xs, net.s_f1, net.f1b, t.h1, ld1, nullptr, 0, m, net.s_k1, H1, stream);
    if (kernel_events) (void)hipEventRecord(kernel_events[2], stream);
    lenet_net_logits(net, t.h1, ld1, H1, t.logits, d_scores, m, stream);
  }
  return hipGetLastError();
}

// which = 0, 1, or 2 on a network with fc2: the tensors held as pieces, as the exact sum of the pieces
int lenet_net_split_debug(const LeNetNet &net, const LeNetNetScratch &t, int which, int n, float *out) {
  const gpd_lenet_shape &sh = net.shape;
  auto sum3 = [](unsigned short h, unsigned short m, unsigned short l) {
    return (float)((double)bf16_value(h) + (double)bf16_value(m) + (double)bf16_value(l));
  };
  if (which == 0) {
    const int F1 = sh.conv1_out, nch = round_up(F1, 8) / 8;
    std::vector<unsigned short> h((size_t)n * nch * 3 * 784 * 8);
    HIP_RET(hipMemcpy(h.data(), t.p1s, h.size() * sizeof(unsigned short), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++)
      for (int f = 0; f < F1; f++)
        for (int pp = 0; pp < 784; pp++) {
          const unsigned short *q = h.data() + ((size_t)i * nch + (f >> 3)) * (3 * 784 * 8) + pp * 8 + (f & 7);
          out[((size_t)i * F1 + f) * 784 + pp] = sum3(q[0], q[784 * 8], q[2 * 784 * 8]);
        }
  } else if (which == 1) {
    const int F2 = sh.conv2_out, F2p = round_up(F2, 8), K = net.s_k1;
    std::vector<unsigned short> h((size_t)n * 3 * K);
    HIP_RET(hipMemcpy(h.data(), t.xs, h.size() * sizeof(unsigned short), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++)
      for (int c = 0; c < F2; c++)
        for (int p = 0; p < 144; p++) {
          const unsigned short *q = h.data() + (size_t)i * 3 * K + p * F2p + c;
          out[((size_t)i * F2 + c) * 144 + p] = sum3(q[0], q[K], q[2 * (size_t)K]);
        }
  } else {
    const int H1 = sh.fc1_out, K = net.s_k2;
    std::vector<unsigned short> h((size_t)n * 3 * K);
    HIP_RET(hipMemcpy(h.data(), t.h1s, h.size() * sizeof(unsigned short), hipMemcpyDeviceToHost));
    for (int i = 0; i < n; i++)
      for (int u = 0; u < H1; u++) {
        const unsigned short *q = h.data() + (size_t)i * 3 * K + u;
        out[(size_t)i * H1 + u] = sum3(q[0], q[K], q[2 * (size_t)K]);
      }
  }
  return GPD_OK;
}

}  // namespace gpd

using namespace gpd;

int gpd_hip_bf16_split3(const float *x, long long n, uint16_t *h, uint16_t *m, uint16_t *l) {
  if (n < 0 || (n > 0 && (!x || !h || !m || !l))) {
    set_error("gpd_hip_bf16_split3: bad argument");
    return GPD_ERR_INVALID;
  }
  for (long long i = 0; i < n; i++) {
    const Bf3 sp = bf16_split3(x[i]);
    h[i] = sp.h;
    m[i] = sp.m;
    l[i] = sp.l;
  }
  return GPD_OK;
}
