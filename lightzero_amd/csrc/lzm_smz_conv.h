// lzm_smz_conv.h — one simulation's network step of the conv StochasticMuZeroModel (stochastic_muzero_model.py:
// 233-273; the 2048 config: latent 64 x 4 x 4, 1 or 2 residual blocks per sub-network, head channels 16, one hidden
// layer of 32, categorical heads) in eval mode, one launch over B roots. BatchNorm is folded on the host.
//
// Root i's leaf is a chance node (is_chance[i]: reached by an action; afterstate dynamics + afterstate prediction ->
// afterstate, value logits [V], chance logits [C]) or a decision node (reached by an outcome; dynamics + prediction
// -> next latent, reward logits [V], value logits [V], policy logits [A]). The kernel reads the kind, the leaf
// latent pool[x[i]][i] and the option on the device and runs that kind's half only.
//
// A workgroup of 4 waves owns P positions. A convolution is a GEMM whose rows are a position's 16 cells (one row
// tile per position), N = the 64 out channels (wave w owns 16 w ..), K = tap x in channel (tap-major) on
// v_mfma_f32_16x16x4_f32: every output element is ONE chain of 144 MFMAs in one accumulator, so its bits depend on
// nothing but the position's own inputs. Activations live in LDS as zero-bordered 6 x 6 planes, two ping-pong
// buffers per position (even layers X -> Y, odd layers Y -> X); a lane's accumulator holds (channel 16 w + lane %
// 16, board row lane / 16), and the residual stays in those registers. The weights are B fragments streamed from
// L2 one tap ahead (across layer boundaries), as lzm_az_c4_net.h streams them. The option plane (input channel 65,
// constant option / space over the board) is not a K step: the epilogue of the first layer adds
// (option / space) * edge[out][cell], edge = the sum of that channel's taps that fall inside the board.
//
// With P = 2 the workgroup runs one pass per kind present among its positions, each over the MFMA tiles of that
// kind's positions only (smz_pass<NRES, NT> with NT = 1 or 2 tiles): positions of one kind share a weight stream,
// a mixed pair streams both sets and computes no tile twice.
//
// Heads: the 1x1 convolutions (16 out channels: one N tile, 16 MFMAs) into a [head][256] LDS block; then each
// (position, head) pair on one wave: FC1 256 -> 32 as 32 units x 2 lanes (128 products per lane in index order, the
// halves added by a DPP swap) + bias, ReLU, the 32 hidden values through LDS, FC2 as one output per lane and round,
// 32 FMAs over a transposed weight block. A chance pass computes no reward head.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_smz_conv_host.h"
#include "lzm_tree.h"  // xor_partner, readlane_f

namespace lzm {

typedef float smzf4 __attribute__((ext_vector_type(4)));

constexpr int kSmzThreads = 256;
constexpr int kSmzPlane = 36;                    // 6 x 6 zero-bordered plane
constexpr int kSmzBuf = 64 * kSmzPlane;          // one activation buffer
constexpr int kSmzHead = 3 * 256;                // 1x1 outputs: reward, value, policy planes
constexpr int kSmzPos = 2 * kSmzBuf + kSmzHead;  // LDS floats per position: X | Y | heads (21,504 B)

__device__ inline int smz_interior(int cell) { return (cell / 4 + 1) * 6 + cell % 4 + 1; }

// 1x1 convolution `head` over the planes in src, + bias, ReLU, into dst as [channel 16][cell 16]
__device__ __forceinline__ void smz_head_conv(const float *__restrict__ ws, const SmzConvLayout &L, const float *src,
                                     float *dst, int head) {
  const int lane = threadIdx.x & 63, q = lane >> 4, c16 = lane & 15;
  const float *bh = ws + L.hconv + head * 1024 + lane;
  const float *ap = src + q * kSmzPlane + smz_interior(c16);
  smzf4 a1 = smzf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < 16; ++k) a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[k * 4 * kSmzPlane], bh[k * 64], a1, 0, 0, 0);
  const float bv = ws[L.hconv_b + head * 16 + c16];
  smzf4 y;
#pragma unroll
  for (int v = 0; v < 4; ++v) {
    const float z = a1[v] + bv;
    y[v] = z > 0.0f ? z : 0.0f;
  }
  *reinterpret_cast<smzf4 *>(dst + head * 256 + c16 * 16 + 4 * q) = y;
}

// FC1 of (position, head) on one wave: 256 -> 32, + bias, ReLU, from the head block hd into hid [32]
__device__ __forceinline__ void smz_head_fc1(const float *__restrict__ ws, const SmzConvLayout &L, const float *hd,
                                             int head, float *hid) {
  const int lane = threadIdx.x & 63, unit = lane >> 1, half = lane & 1;
  const smzf4 *fw = reinterpret_cast<const smzf4 *>(ws + L.fc1) + head * 32 * 64 + lane;
  const smzf4 *in = reinterpret_cast<const smzf4 *>(hd + head * 256 + half * 128);
  float hsum = 0.0f;
#pragma unroll 8
  for (int i = 0; i < 32; ++i) {
    const smzf4 w4 = fw[i * 64], x4 = in[i];
    hsum = fmaf(w4[0], x4[0], hsum);
    hsum = fmaf(w4[1], x4[1], hsum);
    hsum = fmaf(w4[2], x4[2], hsum);
    hsum = fmaf(w4[3], x4[3], hsum);
  }
  hsum += xor_partner<1>(hsum);
  hsum += ws[L.fc1_b + head * 32 + unit];
  if (!half) hid[unit] = hsum > 0.0f ? hsum : 0.0f;
}

// FC2 of (position, head) on one wave: one output per lane and round, the hidden row read as LDS broadcasts
__device__ __forceinline__ void smz_head_fc2(const float *__restrict__ ws, const SmzConvLayout &L, const float *hid,
                                             int head, int n, float *out) {
  const int lane = threadIdx.x & 63;
  const int np = smz_fc2_np(L, head);
  const float *w2 = ws + smz_fc2_at(L, head);
  smzf4 h[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) h[u] = reinterpret_cast<const smzf4 *>(hid)[u];
  for (int o = lane; o < n; o += 64) {
    float z = w2[32 * np + o];
#pragma unroll
    for (int u = 0; u < 32; ++u) z = fmaf(w2[u * np + o], h[u >> 2][u & 3], z);
    out[o] = z;
  }
}

// One kind's half of the network over NT adjacent positions of the workgroup: p0 + t is position t's index within
// the workgroup, r0 + t its root.
template <int NRES, int NT>
__device__ __forceinline__ void smz_pass(const SmzConvArgs &a, const SmzConvLayout &L, float *smem, int kind,
                                int p0, int r0) {
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4, c16 = lane & 15;
  const float *__restrict__ ws = a.w + (size_t)kind * L.set;
  constexpr int layers = 1 + 4 * NRES, G = layers * 9;
  const int ch = 16 * wv + c16;
  // the stream's first group in flight while the residual and the option terms are set up
  const smzf4 *bw = reinterpret_cast<const smzf4 *>(ws + L.conv) + wv * 256 + lane;
  smzf4 bn[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bn[j] = bw[j * 64];

  // this lane's A rows: the window's top-left corner of cell lane % 16 in plane lane / 16; its outputs: channel ch,
  // board row q (cells 4 q .. 4 q + 3)
  const int ra = q * kSmzPlane + (c16 / 4) * 6 + c16 % 4;
  const int oo = ch * kSmzPlane + (q + 1) * 6 + 1;
  const smzf4 edge = *reinterpret_cast<const smzf4 *>(ws + L.edge + ch * 16 + 4 * q);
  const float space = (float)(kind ? a.A : a.C);
  smzf4 res[NT];
  float ov[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    ov[t] = (float)a.option[(r0 + t)] / space;
#pragma unroll
    for (int v = 0; v < 4; ++v) res[t][v] = smem[(p0 + t) * kSmzPos + oo + v];
  }

  int g = 0;
#pragma unroll 1
  for (int l = 0; l < layers; ++l) {
    const int so = (l & 1) ? kSmzBuf : 0, dO = (l & 1) ? 0 : kSmzBuf;  // even layers X -> Y, odd layers Y -> X
    smzf4 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[t] = smzf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap, ++g) {
      smzf4 bc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bc[j] = bn[j];
      const int gn = g + 1 < G ? g + 1 : g;
#pragma unroll
      for (int j = 0; j < 4; ++j) bn[j] = bw[(size_t)gn * 1024 + j * 64];
      const float *sp = smem + so + ra + (tap / 3) * 6 + tap % 3;
      float av[2][NT];
#pragma unroll
      for (int t = 0; t < NT; ++t) av[0][t] = sp[(p0 + t) * kSmzPos];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (j + 1 < 16) {
#pragma unroll
          for (int t = 0; t < NT; ++t) av[(j + 1) & 1][t] = sp[(p0 + t) * kSmzPos + (j + 1) * 4 * kSmzPlane];
        }
#pragma unroll
        for (int t = 0; t < NT; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j & 1][t], bc[j >> 2][j & 3], acc[t], 0, 0, 0);
      }
    }
    // + bias (+ the option term on the first layer) (+ the residual on even layers), ReLU. dst was the previous
    // layer's input: every wave's reads of it ended before the barrier that closed that layer.
    const float bv = ws[L.conv_b + l * 64 + ch];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        float y = acc[t][v] + bv;
        if (l == 0) y += ov[t] * edge[v];
        if (!(l & 1)) y += res[t][v];
        y = y > 0.0f ? y : 0.0f;
        if (!(l & 1)) res[t][v] = y;
        smem[(p0 + t) * kSmzPos + dO + oo + v] = y;
      }
    }
    __syncthreads();
    if (l == 2 * NRES) {  // the dynamics network's output is in Y and in the owners' registers
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        *reinterpret_cast<smzf4 *>(a.latent + (size_t)(r0 + t) * kSmzLat + ch * 16 + 4 * q) = res[t];
        if (kind == 0 && wv == t)
          smz_head_conv(ws, L, smem + (p0 + t) * kSmzPos + kSmzBuf, smem + (p0 + t) * kSmzPos + 2 * kSmzBuf, 0);
      }
    }
  }
  // value and policy 1x1 over the prediction network's output (Y: the last layer is even)
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int hd = 1; hd < 3; ++hd)
      if (((2 * t + hd - 1) & 3) == wv)
        smz_head_conv(ws, L, smem + (p0 + t) * kSmzPos + kSmzBuf, smem + (p0 + t) * kSmzPos + 2 * kSmzBuf, hd);
  __syncthreads();
  // (position, head) pair pr on wave pr % 4: FC1 into the position's X buffer (free now), then FC2
  for (int pr = wv; pr < 3 * NT; pr += 4) {  // wave-uniform
    const int t = pr / 3, hd = pr % 3;
    if (hd == 0 && kind) continue;
    smz_head_fc1(ws, L, smem + (p0 + t) * kSmzPos + 2 * kSmzBuf, hd, smem + (p0 + t) * kSmzPos + hd * 32);
  }
  __syncthreads();
  for (int pr = wv; pr < 3 * NT; pr += 4) {
    const int t = pr / 3, hd = pr % 3;
    if (hd == 0 && kind) continue;
    const int r = (r0 + t);
    float *out = hd == 0 ? a.reward + (size_t)r * a.V
                 : hd == 1 ? a.value + (size_t)r * a.V
                           : (kind ? a.policy_c + (size_t)r * a.C : a.policy_d + (size_t)r * a.A);
    smz_head_fc2(ws, L, smem + (p0 + t) * kSmzPos + hd * 32, hd, hd < 2 ? a.V : (kind ? a.C : a.A), out);
  }
}

template <int NRES, int P>
__global__ void __launch_bounds__(kSmzThreads) smz_conv_step_kernel(SmzConvArgs a) {
  static_assert(P == 1 || P == 2, "one or two positions per workgroup");
  __shared__ __attribute__((aligned(16))) float smem[P * kSmzPos];
  const int tid = threadIdx.x;
  const SmzConvLayout L = smz_conv_layout(NRES, a.V);
  const int b0 = blockIdx.x * P;
  // per position: its kind (-1: no root, or a slot outside the pool) and pool slot, wave-uniform
  int kind[P], slot[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    kind[p] = -1;
    slot[p] = 0;
    if (b0 + p < a.B) {
      slot[p] = __builtin_amdgcn_readfirstlane(a.x[b0 + p]);
      if (slot[p] >= 0 && slot[p] < a.nslots) kind[p] = __builtin_amdgcn_readfirstlane(a.is_chance[b0 + p]) != 0;
    }
  }
  for (int i = tid; i < P * kSmzPos / 4; i += kSmzThreads) reinterpret_cast<smzf4 *>(smem)[i] = smzf4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (kind[p] < 0) continue;
    const float *src = a.pool + ((size_t)slot[p] * a.B + b0 + p) * kSmzLat;
    for (int e = tid; e < kSmzLat; e += kSmzThreads) smem[p * kSmzPos + (e >> 4) * kSmzPlane + smz_interior(e & 15)] = src[e];
  }
  __syncthreads();
  if constexpr (P == 1) {
    if (kind[0] >= 0) smz_pass<NRES, 1>(a, L, smem, kind[0], 0, b0);
  } else {
    if (kind[0] >= 0 && kind[0] == kind[1]) {
      smz_pass<NRES, 2>(a, L, smem, kind[0], 0, b0);
    } else {
#pragma unroll 1
      for (int p = 0; p < 2; ++p) {
        const int k = p ? kind[1] : kind[0];
        if (k >= 0) smz_pass<NRES, 1>(a, L, smem, k, p, b0 + p);
      }
    }
  }
}

}  // namespace lzm
