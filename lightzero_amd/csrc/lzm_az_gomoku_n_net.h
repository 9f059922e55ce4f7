// lzm_az_gomoku_n_net.h — the Gomoku AlphaZeroModel at observation (3, N, N), N = 9 or 15 (alphazero_model.py:
// 32 channels, 1 or 2 residual blocks per network, head channels 16, head width 32, N^2 actions, scalar value) in
// eval mode, one launch over n positions. BatchNorm is folded into the preceding convolution on the host.
//
//   conv3x3 3->32 +b, ReLU; per residual block: conv3x3 32->32 +b, ReLU, conv3x3 32->32 +b, + x, ReLU (the
//   representation's blocks, then the prediction's); 1x1 conv 32->16 (value) | 32->16 (policy) +b, ReLU; per
//   head: Linear 16 N^2->32, LayerNorm(32), ReLU, Linear 32->{1 | N^2}; softmax over the N^2 logits.
//
// A workgroup of 4 waves owns P positions for the whole network. A convolution is a GEMM with rows = (position,
// cell), a position's N^2 rows padded to whole 16-row tiles (6 at N = 9, 15 at N = 15, so no tile straddles two
// positions), N = out channels (2 tiles), K = tap x in channel (288, tap-major) on v_mfma_f32_16x16x4_f32 (exact
// f32). The row tiles are split over the waves: wave w owns N tile w & 1 and the row tiles of parity w >> 1, holds
// the whole layer's B fragments for its N tile in registers (72, and the next layer's 72 in flight behind the
// MFMAs: 18 x 16-byte loads per lane per layer) and runs one chain of 72 K steps per output element, 3 or 4 tiles
// at a time for independent accumulators. No partial sums are exchanged: every output element is
//   (one chain over K = 8 tap + j, in channels 4 j .. 4 j + 3), then + bias (+ skip), ReLU,
// a fixed-order sum whose bits do not depend on n, P, the slot, the workgroup or the neighbours. (The 6 x 6
// kernel's split, every wave on every row tile with a K half each, would need 15 x 4 accumulators per wave and a
// 30 KB exchange buffer at N = 15.)
//
// Registers per lane: 72 + 72 B, 12 / 16 accumulators, 6 / 8 A values, addresses; as compiled 198 VGPRs + 16 AGPRs
// at N = 9 and 256 + 80 at N = 15, of the 512 a 256-thread workgroup may use; no scratch, no spills
// (profiles/az_gomoku_n/resource_usage.diff). LDS per position: two buffers (the block's input / skip, and the
// intermediate) of 32
// zero-bordered (N + 2) x (N + 2) planes. A plane takes `stride` floats, the first value >= (N + 2)^2 that is
// 16 mod 64 (144 at N = 9, 336 at N = 15): the four planes a K step reads (lane / 16 picks the in channel) start
// 16 banks apart, and the 16 lanes of one plane read 16 consecutive cells, consecutive addresses but for a jump of
// 2 at each row end (at most 2 row ends in 16 cells at N = 9, 1 at N = 15): a span of at most 20 banks, all
// distinct. Neighbouring groups (the fourth wraps onto the first) overlap in at most 4 banks, so the 64 lanes of
// an A read meet at most two to a bank. 36,864 bytes per position at N = 9, 86,016 at N = 15. Built: P = 1 at both
// sizes. Two positions do not fit 160 KB at N = 15, and at N = 9 they measured slower for every n (DESIGN.md §10:
// one wave per SIMD instead of two workgroups per CU), so that instantiation is not built.
//
// Heads: the 1x1 convolutions are chains of 8 MFMAs per tile into the intermediate buffer as [32][N^2] (the value
// head's 16 N^2 FC1 inputs, then the policy head's, in the module's flatten order). FC1 is a VALU pass: wave w is
// head w >> 1, units 16 (w & 1) .. + 15; a lane is (unit, quarter of the inputs) and runs 4 N^2 products in index
// order, 16-byte weight loads coalesced over the wave, the inputs broadcast from LDS; a unit's sum is
// ((q0 + q1) + (q2 + q3)) + bias. The weights (2 x 32 x 16 N^2 floats: 165,888 bytes at N = 9, 921,600 at N = 15)
// are streamed from L2 once per workgroup and used for its P positions: 165,888 / P or 921,600 / P bytes of L2
// reads per position per call (no HBM traffic once the weights are in L2 / MALL).
// Then LayerNorm, ReLU, FC2 and the softmax (lane a, a + 64, ..) per (position, head) on the VALU in a fixed order.
// Only the input planes and N^2 + 1 outputs per position touch HBM.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_az_gomoku_n_host.h"
#include "lzm_tree.h"  // xor_partner, xor_sum, xor_max

namespace lzm {

typedef float gmknf4 __attribute__((ext_vector_type(4)));

constexpr int kGmkNNetThreads = 256;

template <int N, int P>
struct GmkNNet {
  static constexpr int cells = N * N;
  static constexpr int pw = N + 2;                                         // bordered plane width
  static constexpr int stride = ((pw * pw - 16 + 63) / 64) * 64 + 16;      // plane stride: 16 mod 64
  static constexpr int posx = 32 * stride;                                 // one position's planes in one buffer
  static constexpr int tiles = (cells + 15) / 16;                          // row tiles of a position
  static constexpr int tt = P * tiles;                                     // row tiles of the workgroup
  static constexpr int tw = (tt + 1) / 2;                                  // row tiles of a wave
  static constexpr int nb = (tw + 3) / 4;                                  // batches of
  static constexpr int tb = (tw + nb - 1) / nb;                            // tb tiles
  static constexpr int flat = 16 * cells;                                  // inputs of a head's FC1
  static constexpr int act_floats = 2 * P * posx;                          // X and Y
  static constexpr int part_floats = 2 * P * 32;                           // FC1 outputs [position][head][32]
  static constexpr int lds_bytes = (act_floats + part_floats) * 4;
  static_assert(stride >= pw * pw && stride % 64 == 16 && posx >= 32 * cells, "plane stride");
  static_assert(lds_bytes <= 160 * 1024, "LDS");
};

// One GEMM pass of this wave: for each of its row tiles, KS K steps (step s reads the planes 4 (s % TS) + lane / 16
// at tap s / TS's offset from `off0`) against the B fragments b[s], then emit(position, cell, channel, value) for
// every valid output element. g: the wave's row-tile parity; ch: this lane's out channel.
template <int N, int P, int KS, int TS, class Emit>
__device__ inline void gmkn_gemm(const float *src, int off0, const float (&b)[KS], int g, int ch, Emit emit) {
  using G = GmkNNet<N, P>;
  const int lane = threadIdx.x & 63, q = lane >> 4;
#pragma unroll 1
  for (int ib = 0; ib < G::nb; ++ib) {
    int rb[G::tb];
#pragma unroll
    for (int i = 0; i < G::tb; ++i) {
      const int t = 2 * (ib * G::tb + i) + g;
      const int m = 16 * (t % G::tiles) + (lane & 15);
      const bool ok = t < G::tt && m < G::cells;  // rows past N^2 and tiles past the last read position 0, cell 0
      const int r = ok ? t / G::tiles : 0, p = ok ? m : 0;
      rb[i] = r * G::posx + (p / N) * G::pw + p % N + q * G::stride + off0;
    }
    gmknf4 acc[G::tb];
    float av[2][G::tb];
#pragma unroll
    for (int i = 0; i < G::tb; ++i) {
      acc[i] = gmknf4{0.f, 0.f, 0.f, 0.f};
      av[0][i] = src[rb[i]];
    }
    // step s + 1's A values are read from LDS while step s's MFMAs run
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      if (s + 1 < KS) {
        const int tap = (s + 1) / TS, j = (s + 1) % TS;
#pragma unroll
        for (int i = 0; i < G::tb; ++i) av[(s + 1) & 1][i] = src[rb[i] + (tap / 3) * G::pw + tap % 3 + j * 4 * G::stride];
      }
#pragma unroll
      for (int i = 0; i < G::tb; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s & 1][i], b[s], acc[i], 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < G::tb; ++i) {
      const int t = 2 * (ib * G::tb + i) + g;
      if (t >= G::tt) continue;  // wave-uniform
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int m = 16 * (t % G::tiles) + 4 * q + v;
        if (m < G::cells) emit(t / G::tiles, m, ch, acc[i][v]);
      }
    }
  }
}

// state [n][3][N][N] -> probs [n][N^2], value [n]
template <int NRES, int N, int P>
__global__ void __launch_bounds__(kGmkNNetThreads) gomoku_n_net_eval_kernel(const float *__restrict__ w,
                                                                            const float *__restrict__ state, int n,
                                                                            float *probs, float *value) {
  using G = GmkNNet<N, P>;
  constexpr int C = G::cells, PW = G::pw;
  extern __shared__ float gmkn_smem[];
  float *X = gmkn_smem, *Y = gmkn_smem + P * G::posx, *part = gmkn_smem + G::act_floats;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6), nt = wv & 1, g = wv >> 1, ch = 16 * nt + (lane & 15);
  const GmkNNetLayout L = gmkn_net_layout(NRES, N);
  constexpr int LAYERS = 4 * NRES;
  const int b0 = blockIdx.x * P;
  auto interior = [](int p) { return (p / N + 1) * PW + p % N + 1; };

  // this wave's N tile of layer 0 and conv0's fragments, in flight while the planes are cleared
  const gmknf4 *bw = reinterpret_cast<const gmknf4 *>(w + L.conv) + nt * 18 * 64 + lane;
  gmknf4 bn[18];
#pragma unroll
  for (int i = 0; i < 18; ++i) bn[i] = bw[i * 64];
  float w0[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) w0[tap] = w[L.conv0 + (nt * 9 + tap) * 64 + lane];

  for (int i = tid; i < G::act_floats / 4; i += kGmkNNetThreads)
    reinterpret_cast<gmknf4 *>(gmkn_smem)[i] = gmknf4{0.f, 0.f, 0.f, 0.f};
  __syncthreads();
  // the input planes into Y's planes 0..2 (plane 3 stays zero: conv0's fourth k of a step)
  for (int e = tid; e < P * 3 * C; e += kGmkNNetThreads) {
    const int r = e / (3 * C), c = e % (3 * C);
    if (b0 + r < n) Y[r * G::posx + (c / C) * G::stride + interior(c % C)] = state[(size_t)(b0 + r) * 3 * C + c];
  }
  __syncthreads();

  // ---- conv0: 3 -> 32, one K step per tap, Y -> X
  {
    const float bv = w[L.conv0_b + ch];
    gmkn_gemm<N, P, 9, 1>(Y, 0, w0, g, ch, [&](int r, int m, int c, float a) {
      const float y = a + bv;
      X[r * G::posx + c * G::stride + interior(m)] = y > 0.0f ? y : 0.0f;
    });
  }
  __syncthreads();

  // ---- the residual blocks: even layers X -> Y, odd layers Y (+ X) -> X. A layer's reads and writes are in
  // different buffers (the skip is read and written by the same lane), so one barrier per layer
#pragma unroll 1
  for (int l = 0; l < LAYERS; ++l) {
    float bc[72];
#pragma unroll
    for (int i = 0; i < 18; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) bc[4 * i + e] = bn[i][e];
    const int ln = l + 1 < LAYERS ? l + 1 : l;  // the next layer's fragments, in flight during this one
#pragma unroll
    for (int i = 0; i < 18; ++i) bn[i] = bw[(size_t)(ln * 2 * 18 + i) * 64];
    const float bv = w[L.conv_b + l * 32 + ch];
    const float *src = (l & 1) ? Y : X;
    float *dst = (l & 1) ? X : Y;
    const bool skip = (l & 1) != 0;
    gmkn_gemm<N, P, 72, 8>(src, 0, bc, g, ch, [&](int r, int m, int c, float a) {
      const int o = r * G::posx + c * G::stride + interior(m);
      float y = a + bv;
      if (skip) y += dst[o];
      dst[o] = y > 0.0f ? y : 0.0f;
    });
    __syncthreads();
  }

  // ---- 1x1 heads: 32 -> 32 (value 0..15 | policy 16..31), X -> Y as [position][32][N^2]
  {
    float bh[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) bh[k] = w[L.head + (nt * 8 + k) * 64 + lane];
    const float bv = w[L.head_b + ch];
    gmkn_gemm<N, P, 8, 8>(X, PW + 1, bh, g, ch, [&](int r, int m, int c, float a) {
      const float y = a + bv;
      Y[r * G::posx + c * C + m] = y > 0.0f ? y : 0.0f;
    });
  }
  __syncthreads();

  // ---- FC1: wave = (head wv >> 1, units 16 (wv & 1) ..), lane = 4 unit + quarter; the weights are read once for
  // the workgroup's P positions
  {
    const int head = wv >> 1, qtr = lane & 3;
    const gmknf4 *fw = reinterpret_cast<const gmknf4 *>(w + L.fc1) + ((size_t)head * C * 2 + (wv & 1)) * 64 + lane;
    const gmknf4 *in = reinterpret_cast<const gmknf4 *>(Y + head * G::flat + qtr * 4 * C);
    float hs[P];
#pragma unroll
    for (int r = 0; r < P; ++r) hs[r] = 0.0f;
#pragma unroll 9
    for (int i = 0; i < C; ++i) {
      const gmknf4 a = fw[(size_t)i * 128];
#pragma unroll
      for (int r = 0; r < P; ++r) {
        const gmknf4 x = in[r * (G::posx / 4) + i];
        hs[r] = fmaf(a[0], x[0], hs[r]);
        hs[r] = fmaf(a[1], x[1], hs[r]);
        hs[r] = fmaf(a[2], x[2], hs[r]);
        hs[r] = fmaf(a[3], x[3], hs[r]);
      }
    }
#pragma unroll
    for (int r = 0; r < P; ++r) {
      float h = hs[r];
      h += xor_partner<1>(h);
      h += xor_partner<2>(h);
      if (qtr == 0) part[(r * 2 + head) * 32 + 16 * (wv & 1) + (lane >> 2)] = h;
    }
  }
  __syncthreads();

  // ---- (position, head) pair pr on wave pr % 4: LayerNorm, ReLU, FC2 (and the softmax, action lane + 64 k)
  for (int pr = wv; pr < 2 * P; pr += 4) {
    const int r = pr >> 1, head = pr & 1, b = b0 + r;
    if (b >= n) continue;  // wave-uniform, no barrier follows
    const float *tw = w + (head ? L.tail_p : L.tail_v);
    float h[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) h[u] = part[pr * 32 + u] + tw[kGmkNT1b + u];
    float mean = 0.0f;
#pragma unroll
    for (int u = 0; u < 32; ++u) mean += h[u];
    mean *= 1.0f / 32;
    float var = 0.0f;
#pragma unroll
    for (int u = 0; u < 32; ++u) var = fmaf(h[u] - mean, h[u] - mean, var);
    var *= 1.0f / 32;
    const float rs = 1.0f / sqrtf(var + 1e-5f);
#pragma unroll
    for (int u = 0; u < 32; ++u) {
      const float z = (h[u] - mean) * rs * tw[kGmkNTg + u] + tw[kGmkNTb + u];
      h[u] = z > 0.0f ? z : 0.0f;
    }
    if (head == 0) {
      float v = tw[kGmkNTv2b];
#pragma unroll
      for (int u = 0; u < 32; ++u) v = fmaf(tw[kGmkNT2 + u], h[u], v);
      if (lane == 0) value[b] = v;
    } else {
      constexpr int NA = (C + 63) / 64;  // actions per lane
      float z[NA];
      float mx = -__builtin_inff();
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        const int a = lane + 64 * k < C ? lane + 64 * k : 0;
        float zz = tw[gmkn_tp2b(C) + a];
#pragma unroll
        for (int u = 0; u < 32; ++u) zz = fmaf(tw[kGmkNT2 + a * 32 + u], h[u], zz);
        z[k] = lane + 64 * k < C ? zz : -__builtin_inff();
        mx = fmaxf(mx, z[k]);
      }
      mx = xor_max(mx);
      float sum = 0.0f;
#pragma unroll
      for (int k = 0; k < NA; ++k) {
        z[k] = lane + 64 * k < C ? expf(z[k] - mx) : 0.0f;
        sum += z[k];
      }
      sum = xor_sum(sum);
#pragma unroll
      for (int k = 0; k < NA; ++k)
        if (lane + 64 * k < C) probs[(size_t)b * C + lane + 64 * k] = z[k] / sum;
    }
  }
}

}  // namespace lzm
