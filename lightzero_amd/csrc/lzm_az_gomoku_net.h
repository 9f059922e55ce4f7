// lzm_az_gomoku_net.h — the Gomoku config's AlphaZeroModel (alphazero_model.py:14-330; observation (3, 6, 6), 32
// channels, 1 or 2 residual blocks per network, head channels 16, head width 32, 36 actions, scalar value) in eval
// mode, one launch over n positions. BatchNorm is folded into the preceding convolution on the host.
//
//   conv3x3 3->32 +b, ReLU; per residual block: conv3x3 32->32 +b, ReLU, conv3x3 32->32 +b, + x, ReLU (the
//   representation's blocks, then the prediction's); 1x1 conv 32->16 (value) | 32->16 (policy) +b, ReLU; per
//   head: Linear 576->32, LayerNorm(32), ReLU, Linear 32->{1 | 36}; softmax over the 36 logits.
//
// A 32 -> 32 layer is 36 KB of f32 weights: a quarter of it is 36 registers per lane, so the weights live in the
// register file. A workgroup of 4 waves owns P positions for the whole network. A convolution is a GEMM with rows
// = (position, cell) (36 P rows: 3 / 5 row tiles for the built P = 1 / 2), N = out channels (2 tiles), K = tap x in
// channel (288, tap-major) on v_mfma_f32_16x16x4_f32 (exact f32). Wave w owns (N tile w & 1, K half w >> 1: in
// channels 16 (w >> 1) ..): its share of a layer's B fragments is 9 x 16-byte loads per lane, fetched once per
// workgroup per layer while the previous layer computes, and used for every row tile. Every output element is
//   (chain over in channels 0..15, 36 K steps) + (chain over in channels 16..31, 36 K steps), then + bias (+ skip):
// a fixed-order sum of two fixed K partitions, each one accumulator chain, so its bits do not depend on P, on the
// row tile or workgroup the position lands in, or on its neighbours. The two partner waves exchange the halves
// through LDS: each hands over the row tiles of the other parity and finishes its own (f32 + commutes, so which
// wave adds does not show).
//
// Activations stay in LDS as zero-bordered 8 x 8 planes, 32 per buffer and position, two buffers (the block's
// input / skip, and the intermediate); a plane is followed by 16 unused floats (plane c at 80 c), so the four
// planes a K step reads (in channels c .. c + 3) start 16 banks apart and the 64 lanes of an A read meet at most
// two to a bank. The outputs stay
// in the accumulators across the barrier that ends the layer's reads, so the second convolution of a block writes
// over the block's input in place. Only the input planes and 37 outputs per position touch HBM.
//
// Heads: the 1x1 convolutions are (row tile, N tile) chains of 8 MFMAs; FC1 runs as (position, head, pass) items
// spread over the four waves: 32 units x 2 lanes, 144 products per lane in index order, quarters 2 pass + half;
// a unit's sum is ((q0 + q1) + (q2 + q3)) + bias. Then LayerNorm, ReLU, FC2 and the 36-lane softmax per (position,
// head) on the VALU in a fixed order.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_az_gomoku_host.h"
#include "lzm_tree.h"  // xor_partner, xor_sum, xor_max

namespace lzm {

typedef float gmkf4 __attribute__((ext_vector_type(4)));

constexpr int kGmkNetThreads = 256;
constexpr int kGmkPlane = 80;             // an 8 x 8 plane and 16 floats of bank stagger
constexpr int kGmkPosX = kGmkC * kGmkPlane;  // one position's planes in one buffer
constexpr int kGmkHd = 32 * 36;            // 1x1 outputs of a position, value planes then policy planes

template <int P>
struct GmkNet {
  static constexpr int rows = 36 * P;
  static constexpr int tiles = (rows + 15) / 16;
  static constexpr int act_floats = 2 * P * kGmkPosX;      // X and Y
  static constexpr int part_floats = 2 * tiles * 256;      // the exchanged halves [nt][tile][lane][4]
  static constexpr int lds_bytes = (act_floats + part_floats) * 4;
};

__device__ inline int gmk_plane(int c) { return kGmkPlane * c; }
__device__ inline int gmk_interior(int p) { return (p / 6 + 1) * 8 + p % 6 + 1; }

// The layer's outputs from the accumulators. pair: the partner wave (same N tile, other K half) holds the other
// half of every element; each wave hands over the tiles of the other parity and finishes those of its own.
// Unpaired (conv0: one chain): the K-half-0 waves finish every tile. y = (half + half) + bias (+ skip), ReLU, into
// the interior of dst's planes. The first barrier ends every wave's reads of the layer's input (dst may be that
// input) and publishes the halves, the second publishes dst.
template <int P>
__device__ inline void gmk_epilogue(const gmkf4 (&acc)[GmkNet<P>::tiles], bool pair, const float *__restrict__ bias,
                                    const float *skip, float *dst, float *part, int wv) {
  constexpr int T = GmkNet<P>::tiles;
  const int lane = threadIdx.x & 63, nt = wv & 1, kh = wv >> 1, ch = 16 * nt + (lane & 15);
  const float bv = bias[ch];
  gmkf4 *part4 = reinterpret_cast<gmkf4 *>(part);
  if (pair) {
#pragma unroll
    for (int t = 0; t < T; ++t)
      if ((t & 1) != kh) part4[(nt * T + t) * 64 + lane] = acc[t];
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < T; ++t) {
    if (pair ? (t & 1) != kh : kh != 0) continue;  // wave-uniform
    gmkf4 o4 = gmkf4{0.f, 0.f, 0.f, 0.f};
    if (pair) o4 = part4[(nt * T + t) * 64 + lane];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = 16 * t + 4 * (lane >> 4) + v;
      if (m >= GmkNet<P>::rows) continue;
      const int o = (m / 36) * kGmkPosX + gmk_plane(ch) + gmk_interior(m % 36);
      float y = pair ? (acc[t][v] + o4[v]) + bv : acc[t][v] + bv;
      if (skip) y += skip[o];
      dst[o] = y > 0.0f ? y : 0.0f;
    }
  }
  __syncthreads();
}

// state [n][3][6][6] -> probs [n][36], value [n]
template <int NRES, int P>
__global__ void __launch_bounds__(kGmkNetThreads) gomoku_net_eval_kernel(const float *__restrict__ w,
                                                                         const float *__restrict__ state, int n,
                                                                         float *probs, float *value) {
  using G = GmkNet<P>;
  constexpr int T = G::tiles;
  extern __shared__ float gmk_smem[];
  float *X = gmk_smem, *Y = gmk_smem + P * kGmkPosX, *part = gmk_smem + G::act_floats;
  const int tid = threadIdx.x, lane = tid & 63, q = lane >> 4;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nt = wv & 1, kh = wv >> 1;
  const GmkNetLayout L = gmk_net_layout(NRES);
  constexpr int LAYERS = 4 * NRES;
  const int b0 = blockIdx.x * P;

  // this wave's share of layer 0 and conv0's fragments, in flight while the planes are cleared
  const gmkf4 *bw = reinterpret_cast<const gmkf4 *>(w + L.conv) + wv * 9 * 64 + lane;
  gmkf4 bn[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) bn[tap] = bw[tap * 64];
  float w0[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) w0[tap] = w[L.conv0 + (nt * 9 + tap) * 64 + lane];

  for (int i = tid; i < G::act_floats / 4; i += kGmkNetThreads)
    reinterpret_cast<gmkf4 *>(gmk_smem)[i] = gmkf4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  // the input planes into Y's planes 0..2 (plane 3 stays zero: conv0's fourth k of a step)
  for (int e = tid; e < P * 108; e += kGmkNetThreads) {
    const int r = e / 108, c = e % 108;
    if (b0 + r < n) Y[r * kGmkPosX + gmk_plane(c / 36) + gmk_interior(c % 36)] = state[(size_t)(b0 + r) * 108 + c];
  }
  // this lane's A rows: the window's top-left corner in plane lane / 16 (rows past 36 P read position 0, cell 0)
  int rb[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int m = 16 * t + (lane & 15);
    const int r = m < G::rows ? m / 36 : 0, p = m < G::rows ? m % 36 : 0;
    rb[t] = r * kGmkPosX + (p / 6) * 8 + p % 6 + gmk_plane(q);
  }
  __syncthreads();

  gmkf4 acc[T];
  // ---- conv0: 3 -> 32, one K step per tap, one chain per element on the K-half-0 waves
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = gmkf4{0.f, 0.f, 0.f, 0.f};
  if (kh == 0) {
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int t = 0; t < T; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Y[rb[t] + (tap / 3) * 8 + tap % 3], w0[tap], acc[t], 0, 0, 0);
  }
  gmk_epilogue<P>(acc, false, w + L.conv0_b, nullptr, X, part, wv);

  // ---- the residual blocks: even layers X -> Y, odd layers Y (+ X) -> X
#pragma unroll 1
  for (int l = 0; l < LAYERS; ++l) {
    const float *sp = ((l & 1) ? Y : X) + kh * 16 * kGmkPlane;  // this wave's K half: planes 16 kh ..
    gmkf4 bc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) bc[tap] = bn[tap];
    const int ln = l + 1 < LAYERS ? l + 1 : l;  // the next layer's share, in flight during this one
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) bn[tap] = bw[(size_t)(ln * 4 * 9 + tap) * 64];
#pragma unroll
    for (int t = 0; t < T; ++t) acc[t] = gmkf4{0.f, 0.f, 0.f, 0.f};
    // step s = 4 tap + j reads planes 4 j + q of the half at the tap's offset; step s + 1's A values are read from
    // LDS while step s's MFMAs run
    float av[2][T];
#pragma unroll
    for (int t = 0; t < T; ++t) av[0][t] = sp[rb[t]];
#pragma unroll
    for (int s = 0; s < 36; ++s) {
      if (s + 1 < 36) {
        const int tap = (s + 1) >> 2, j = (s + 1) & 3;
#pragma unroll
        for (int t = 0; t < T; ++t) av[(s + 1) & 1][t] = sp[rb[t] + (tap / 3) * 8 + tap % 3 + j * 4 * kGmkPlane];
      }
#pragma unroll
      for (int t = 0; t < T; ++t)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s & 1][t], bc[s >> 2][s & 3], acc[t], 0, 0, 0);
    }
    gmk_epilogue<P>(acc, true, w + L.conv_b + l * 32, (l & 1) ? X : nullptr, (l & 1) ? X : Y, part, wv);
  }

  // ---- 1x1 heads: 32 -> 32 (value 0..15 | policy 16..31) into Y as [position][32][36]. (row tile t, N tile nt)
  // runs on the wave with nt = wave & 1, t & 1 = wave >> 1: one chain of 8 MFMAs each
  {
    const int ch = 16 * nt + (lane & 15);
    float bh[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) bh[k] = w[L.head + (nt * 8 + k) * 64 + lane];
    const float bv = w[L.head_b + ch];
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if ((t & 1) != kh) continue;  // wave-uniform
      gmkf4 a1 = gmkf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 8; ++k)
        a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(X[rb[t] + 9 + k * 4 * kGmkPlane], bh[k], a1, 0, 0, 0);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int m = 16 * t + 4 * q + v;
        const float y = a1[v] + bv;
        if (m < G::rows) Y[(m / 36) * kGmkHd + ch * 36 + m % 36] = y > 0.0f ? y : 0.0f;
      }
    }
  }
  __syncthreads();

  // ---- FC1: item (position r, head, pass) on wave item % 4; lane = 2 unit + half, quarter 2 pass + half
  for (int it = wv; it < 4 * P; it += 4) {
    const int r = it >> 2, head = (it >> 1) & 1, pass = it & 1;
    const gmkf4 *fw = reinterpret_cast<const gmkf4 *>(w + L.fc1) + (head * 2 + pass) * 36 * 64 + lane;
    const gmkf4 *in = reinterpret_cast<const gmkf4 *>(Y + r * kGmkHd + head * kGmkFlat + (2 * pass + (lane & 1)) * 144);
    float hsum = 0.0f;
#pragma unroll 12
    for (int i = 0; i < 36; ++i) {
      const gmkf4 a = fw[i * 64], x = in[i];
      hsum = fmaf(a[0], x[0], hsum);
      hsum = fmaf(a[1], x[1], hsum);
      hsum = fmaf(a[2], x[2], hsum);
      hsum = fmaf(a[3], x[3], hsum);
    }
    hsum += xor_partner<1>(hsum);
    if ((lane & 1) == 0) part[it * 32 + (lane >> 1)] = hsum;
  }
  __syncthreads();

  // ---- (position, head) pair pr on wave pr % 4: LayerNorm, ReLU, FC2 (and the softmax over 36 lanes)
  for (int pr = wv; pr < 2 * P; pr += 4) {
    const int r = pr >> 1, head = pr & 1, b = b0 + r;
    if (b >= n) continue;  // wave-uniform, no barrier follows
    const float *tw = w + (head ? L.tail_p : L.tail_v);
    float h[kGmkFc];
#pragma unroll
    for (int u = 0; u < kGmkFc; ++u) h[u] = (part[(2 * pr) * 32 + u] + part[(2 * pr + 1) * 32 + u]) + tw[kGmkT1b + u];
    float mean = 0.0f;
#pragma unroll
    for (int u = 0; u < kGmkFc; ++u) mean += h[u];
    mean *= 1.0f / kGmkFc;
    float var = 0.0f;
#pragma unroll
    for (int u = 0; u < kGmkFc; ++u) var = fmaf(h[u] - mean, h[u] - mean, var);
    var *= 1.0f / kGmkFc;
    const float rs = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
    for (int u = 0; u < kGmkFc; ++u) {
      const float z = (h[u] - mean) * rs * tw[kGmkTg + u] + tw[kGmkTb + u];
      h[u] = z > 0.0f ? z : 0.0f;
    }
    if (head == 0) {
      float v = tw[kGmkTv2b];
#pragma unroll
      for (int u = 0; u < kGmkFc; ++u) v = fmaf(tw[kGmkT2 + u], h[u], v);
      if (lane == 0) value[b] = v;
    } else {
      const int a = lane < kGmkCells ? lane : 0;
      float z = tw[kGmkTp2b + a];
#pragma unroll
      for (int u = 0; u < kGmkFc; ++u) z = fmaf(tw[kGmkT2 + a * kGmkFc + u], h[u], z);
      if (lane >= kGmkCells) z = -__builtin_inff();
      const float mx = xor_max(z);
      const float e = lane < kGmkCells ? expf(z - mx) : 0.0f;
      const float sum = xor_sum(e);
      if (lane < kGmkCells) probs[(size_t)b * kGmkCells + lane] = e / sum;
    }
  }
}

}  // namespace lzm
