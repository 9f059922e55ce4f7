// lzm_az_c4_net.h — the Connect4 config's AlphaZeroModel (alphazero_model.py:14-330; observation (3, 6, 7), 64
// channels, 1 or 2 residual blocks per network, head width 32, 7 actions, scalar value) in eval mode, one launch
// over n positions. BatchNorm is folded into the preceding convolution on the host.
//
//   conv3x3 3->64 +b, ReLU; per residual block: conv3x3 64->64 +b, ReLU, conv3x3 64->64 +b, + x, ReLU (the
//   representation's blocks, then the prediction's); 1x1 conv 64->16 (value) | 64->16 (policy) +b, ReLU; per
//   head: Linear 672->32, LayerNorm(32), ReLU, Linear 32->{1 | 7}; softmax over the 7 logits.
//
// A 64 -> 64 layer is 147 KB of f32 weights: they fit neither registers nor LDS (lzm_az_fused.h keeps its 16-channel
// layers in registers), so the roles are turned round. A workgroup of 4 waves owns kC4nBoards = 2 positions for the
// whole network; their activations stay in LDS as zero-bordered 8 x 9 planes (two buffers of 64 planes per board:
// the block's input / skip, and the intermediate); the weights stream from L2 in MFMA B-fragment order.
//
// A convolution is a GEMM with rows = (board, cell) (84 rows, 6 row tiles), N = out channels, K = tap x in
// channel on v_mfma_f32_16x16x4_f32 (exact f32). Wave w owns N tile w (out channels 16 w ..): it reads each of
// its B fragments once per layer and uses it for all 6 row tiles, so every output element is ONE k-ordered chain
// in one accumulator (K = 576: tap-major, in channel minor) and its bits do not depend on the tile, workgroup or
// batch the position lands in. With K ordered tap-major a lane's A address is (row corner + 72 (lane / 16)) +
// tap offset + 288 j: one add per tap and an immediate per step. The fragments of tap g + 1 (16 steps, four
// 16-byte loads per lane) are fetched while tap g's 96 MFMAs run, across layer boundaries as well. The outputs
// stay in the accumulators across the barrier that ends the layer's reads, so the second convolution of a block
// writes over the block's input in place. Only the input planes and 8 outputs per position touch HBM.
//
// Heads: the 1x1 convolutions are 12 (row tile, N tile) chains of 16 MFMAs; then each (board, head) pair runs on
// one wave: FC1 as 32 units x 2 lanes (336 products per lane in index order, the two halves added by a DPP
// swap), the 32 hidden values to wave-uniform registers, LayerNorm, ReLU, FC2 and the 7-lane softmax.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_az_c4_host.h"
#include "lzm_tree.h"  // xor_partner, readlane_f

namespace lzm {

typedef float c4f4 __attribute__((ext_vector_type(4)));

constexpr int kC4nThreads = 256;
constexpr int kC4nBoards = 2;                       // positions per workgroup
constexpr int kC4nC = 64;                           // channels
constexpr int kC4nPlane = 72;                       // 8 x 9 zero-bordered plane
constexpr int kC4nBoardX = kC4nC * kC4nPlane;       // one board's activations
constexpr int kC4nRows = kC4nBoards * 42;           // GEMM rows
constexpr int kC4nTiles = (kC4nRows + 15) / 16;     // 6
constexpr int kC4nFc = 32;                          // head hidden width
constexpr int kC4nFlat = 16 * 42;                   // 672 inputs of a head's FC1
constexpr int kC4nHd = 32 * 42;                     // 1x1 outputs of a board, value planes then policy planes
constexpr int kC4nLdsFloats = 2 * kC4nBoards * kC4nBoardX;  // 73,728 B

__device__ inline int c4n_interior(int p) { return (p / 7 + 1) * 9 + p % 7 + 1; }

// the layer's outputs from the accumulators: + bias (+ skip), ReLU, into the interior of dst's planes. The first
// barrier ends every wave's reads of the layer's input (dst may be that input), the second publishes dst.
__device__ inline void c4n_epilogue(const c4f4 (&acc)[kC4nTiles], const float *__restrict__ bias, const float *skip,
                                    float *dst) {
  const int lane = threadIdx.x & 63, ch = 16 * (threadIdx.x >> 6) + (lane & 15);
  const float bv = bias[ch];
  __syncthreads();
#pragma unroll
  for (int t = 0; t < kC4nTiles; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = 16 * t + 4 * (lane >> 4) + v;
      if (m >= kC4nRows) continue;
      const int o = (m / 42) * kC4nBoardX + ch * kC4nPlane + c4n_interior(m % 42);
      float y = acc[t][v] + bv;
      if (skip) y += skip[o];
      dst[o] = y > 0.0f ? y : 0.0f;
    }
  __syncthreads();
}

// state [n][3][6][7] -> probs [n][7], value [n]
template <int NRES>
__global__ void __launch_bounds__(kC4nThreads) c4_net_eval_kernel(const float *__restrict__ w,
                                                                  const float *__restrict__ state, int n,
                                                                  float *probs, float *value) {
  extern __shared__ float c4n_smem[];
  float *X = c4n_smem, *Y = c4n_smem + kC4nBoards * kC4nBoardX;
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4;
  const C4NetLayout L = c4_net_layout(NRES);
  constexpr int G = 4 * NRES * 9;  // (layer, tap) groups of the 64 -> 64 weight stream
  const int b0 = blockIdx.x * kC4nBoards;

  // the stream's first group and conv0's fragments, in flight while the planes are cleared
  const c4f4 *bw = reinterpret_cast<const c4f4 *>(w + L.conv) + wv * 256 + lane;
  c4f4 bn[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) bn[j] = bw[j * 64];
  float w0[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) w0[tap] = w[L.conv0 + (wv * 9 + tap) * 64 + lane];

  for (int i = tid; i < kC4nLdsFloats / 4; i += kC4nThreads) reinterpret_cast<c4f4 *>(c4n_smem)[i] = c4f4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  // the input planes into Y's planes 0..2 (plane 3 stays zero: conv0's fourth k of a step)
  for (int e = tid; e < kC4nBoards * 126; e += kC4nThreads) {
    const int r = e / 126, c = e % 126;
    if (b0 + r < n) Y[r * kC4nBoardX + (c / 42) * kC4nPlane + c4n_interior(c % 42)] = state[(size_t)(b0 + r) * 126 + c];
  }
  // this lane's A rows: the window's top-left corner in plane lane / 16 (rows past 84 read board 0, cell 0)
  int rb[kC4nTiles];
#pragma unroll
  for (int t = 0; t < kC4nTiles; ++t) {
    const int m = 16 * t + (lane & 15);
    const int r = m < kC4nRows ? m / 42 : 0, p = m < kC4nRows ? m % 42 : 0;
    rb[t] = r * kC4nBoardX + (p / 7) * 9 + p % 7 + q * kC4nPlane;
  }
  __syncthreads();

  c4f4 acc[kC4nTiles];
  // ---- conv0: 3 -> 64, one K step per tap
#pragma unroll
  for (int t = 0; t < kC4nTiles; ++t) acc[t] = c4f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int t = 0; t < kC4nTiles; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Y[rb[t] + (tap / 3) * 9 + tap % 3], w0[tap], acc[t], 0, 0, 0);
  c4n_epilogue(acc, w + L.conv0_b, nullptr, X);

  // ---- the residual blocks: even layers X -> Y, odd layers Y (+ X) -> X
  int g = 0;
#pragma unroll 1
  for (int l = 0; l < 4 * NRES; ++l) {
    const float *src = (l & 1) ? Y : X;
#pragma unroll
    for (int t = 0; t < kC4nTiles; ++t) acc[t] = c4f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap, ++g) {
      c4f4 bc[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bc[j] = bn[j];
      const int gn = g + 1 < G ? g + 1 : g;
#pragma unroll
      for (int j = 0; j < 4; ++j) bn[j] = bw[(size_t)gn * 1024 + j * 64];
      const float *sp = src + (tap / 3) * 9 + tap % 3;
      // step j + 1's six A values are read from LDS while step j's six MFMAs run
      float av[2][kC4nTiles];
#pragma unroll
      for (int t = 0; t < kC4nTiles; ++t) av[0][t] = sp[rb[t]];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        if (j + 1 < 16) {
#pragma unroll
          for (int t = 0; t < kC4nTiles; ++t) av[(j + 1) & 1][t] = sp[rb[t] + (j + 1) * 4 * kC4nPlane];
        }
#pragma unroll
        for (int t = 0; t < kC4nTiles; ++t)
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[j & 1][t], bc[j >> 2][j & 3], acc[t], 0, 0, 0);
      }
    }
    c4n_epilogue(acc, w + L.conv_b + l * 64, (l & 1) ? X : nullptr, (l & 1) ? X : Y);
  }

  // ---- 1x1 heads: 64 -> 32 (value 0..15 | policy 16..31) into Y as [board][32][42]. (row tile t, N tile nt)
  // runs on the wave with nt = wave & 1, t & 1 = wave >> 1: one chain of 16 MFMAs each
  {
    const int nt = wv & 1, ch = 16 * nt + (lane & 15);
    float bh[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) bh[k] = w[L.head + (nt * 16 + k) * 64 + lane];
    const float bv = w[L.head_b + ch];
#pragma unroll
    for (int t = 0; t < kC4nTiles; ++t) {
      if ((t & 1) != (wv >> 1)) continue;  // wave-uniform
      c4f4 a1 = c4f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 16; ++k)
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(X[rb[t] + 10 + k * 4 * kC4nPlane], bh[k], a1, 0, 0, 0);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int m = 16 * t + 4 * q + v;
        const float y = a1[v] + bv;
        if (m < kC4nRows) Y[(m / 42) * kC4nHd + ch * 42 + m % 42] = y > 0.0f ? y : 0.0f;
      }
    }
  }
  __syncthreads();

  // ---- (board, head) pair on wave `wv`
  const int r = wv >> 1, head = wv & 1, b = b0 + r;
  if (b >= n) return;  // wave-uniform, no barrier follows
  const int unit = lane >> 1, half = lane & 1;
  const c4f4 *fw = reinterpret_cast<const c4f4 *>(w + L.fc1) + head * 84 * 64 + lane;
  const c4f4 *in = reinterpret_cast<const c4f4 *>(Y + r * kC4nHd + head * kC4nFlat + half * 336);
  float hsum = 0.0f;
#pragma unroll 12
  for (int i = 0; i < 84; ++i) {
    const c4f4 a = fw[i * 64], x = in[i];
    hsum = fmaf(a[0], x[0], hsum);
    hsum = fmaf(a[1], x[1], hsum);
    hsum = fmaf(a[2], x[2], hsum);
    hsum = fmaf(a[3], x[3], hsum);
  }
  hsum += xor_partner<1>(hsum);
  const float *tw = w + (head ? L.tail_p : L.tail_v);
  hsum += tw[kC4nT1b + unit];
  float h[kC4nFc];
#pragma unroll
  for (int u = 0; u < kC4nFc; ++u) h[u] = readlane_f(hsum, 2 * u);
  float mean = 0.0f;
#pragma unroll
  for (int u = 0; u < kC4nFc; ++u) mean += h[u];
  mean *= 1.0f / kC4nFc;
  float var = 0.0f;
#pragma unroll
  for (int u = 0; u < kC4nFc; ++u) var = fmaf(h[u] - mean, h[u] - mean, var);
  var *= 1.0f / kC4nFc;
  const float rs = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
  for (int u = 0; u < kC4nFc; ++u) {
    const float z = (h[u] - mean) * rs * tw[kC4nTg + u] + tw[kC4nTb + u];
    h[u] = z > 0.0f ? z : 0.0f;
  }
  if (head == 0) {
    float v = tw[kC4nTv2b];
#pragma unroll
    for (int u = 0; u < kC4nFc; ++u) v = fmaf(tw[kC4nT2 + u], h[u], v);
    if (lane == 0) value[b] = v;
  } else {
    const int a = lane & 7;
    float z = -__builtin_inff();
    if (a < 7) {
      z = tw[kC4nTp2b + a];
#pragma unroll
      for (int u = 0; u < kC4nFc; ++u) z = fmaf(tw[kC4nT2 + a * kC4nFc + u], h[u], z);
    }
    float mx = z;
    mx = fmaxf(mx, xor_partner<1>(mx));
    mx = fmaxf(mx, xor_partner<2>(mx));
    mx = fmaxf(mx, xor_partner<4>(mx));
    const float e = a < 7 ? expf(z - mx) : 0.0f;
    float sum = e;
    sum += xor_partner<1>(sum);
    sum += xor_partner<2>(sum);
    sum += xor_partner<4>(sum);
    if (lane < 7) probs[(size_t)b * 7 + lane] = e / sum;
  }
}

}  // namespace lzm
