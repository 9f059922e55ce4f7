// lzm_az_gomoku_n_net_split.h — the Gomoku 9 x 9 / 15 x 15 AlphaZeroModel of lzm_az_gomoku_n_net.h (same network,
// same outputs' meaning) with its 32 -> 32 3x3 layers and 1x1 heads on v_mfma_f32_16x16x32_f16 in the split-fp16
// scheme of lzm_conv.h: every f32 operand is two fp16 terms x = h + l, a product the sum of l_a h_b, h_a l_b, h_a h_b
// (in that order), error at the f32 level. Opt-in (GomokuAZNet(precision="split")); the exact-f32 kernel stays the
// default.
//
// GEMM. A workgroup of 4 waves owns one position for the whole network. Rows = cells, N^2 padded to whole 16-row
// tiles (6 at N = 9, 15 at N = 15); N = the 32 out channels (2 tiles); K = 288 = 9 chunks of 32, chunk = tap, the 32
// in channels minor; three MFMAs per chunk: 27 per (row tile, N tile, layer) against 72 on v_mfma_f32_16x16x4_f32.
// Every output element is one chain in one accumulator in chunk order, so its bits do not depend on n, the
// workgroup, the wave that ran it or the neighbours.
//
// Work split. Wave w owns row tiles w, w + 4, .. (2/2/1/1 at N = 9, 4/4/4/3 at N = 15) for BOTH N tiles, and holds
// the whole layer's B fragments in registers: 9 chunks x 2 N tiles x 2 terms x 4 VGPRs = 144. An A fragment read
// from LDS then feeds six MFMAs; the (N tile, row parity) split of the f32 kernel has the same MFMA count per wave
// and twice the A traffic. The outermost loop is the chunk: all of the wave's tiles (8 independent accumulators at
// N = 15) run chunk s before chunk s + 1, so a fragment is dead once its chunk has issued, and the NEXT layer's
// chunk s - 1 is loaded into its registers while chunk s runs (a rolling refill: the whole next layer is in flight
// or in place before the epilogue and the barrier, with no second set of registers). The two wave kinds (TW and
// TW - 1 tiles) are two instantiations of the layer body behind a wave-uniform branch; the barriers are outside it.
// LDS rate: a chunk of a 4-tile wave is 8 ds_read_b128 (8 KB per wave) against 24 MFMAs of 16 cycles on its SIMD;
// four waves ask for 32 KB per 384 cycles = 85 B / cycle / CU of the 128 the LDS delivers (an argument from the
// instruction rates, not a measurement).
//
// Activations in LDS: two ping-pong buffers [bordered cell (N + 2)^2][term 2][32 ch] of fp16, the two terms of a
// cell interleaved so that a cell is one 128-byte row (64 bytes of h, 64 of l): 2 x 15,488 B at N = 9, 2 x 36,992 B
// at N = 15. A lane's A fragment is one ds_read_b128: cell lane & 15 of the tile at the tap's offset, channels
// 8 (lane >> 4) .. + 7 of one term. The 16-byte chunk c = 4 term + channels / 8 of bordered cell (Y, X) is stored at
// chunk c ^ (k & 6), k = N Y + X. For row p = N y + x and tap (dy, dx) the cell read is (y + dy, x + dx), k = p +
// N dy + dx: k runs with the row index across plane rows, and so does the cell's address parity (bit 7 of the
// byte address: a step of 1 cell inside a plane row, 3 at its end). A ds_read_b128 lane group (lanes {0-3, 12-15,
// 20-27} and {4-11, 16-19, 28-31} of each wave half) holds rows {0-3, 12-15} of channel chunk c and rows {4-11} of
// chunk c ^ 1; per address parity that is four rows 2 apart twice, (k & 6) takes all four values over each, and the
// two sets differ in bit 0 of the chunk: sixteen lanes, sixteen distinct 16-byte bank slots. Rows past N^2 (the last
// tile has one valid row at both sizes) read row p - 16: the same key and parity as row p would have. Enumerated on
// the host over every tile, tap, term and lane group for both sizes: worst case one address per bank slot, four
// without the swizzle.
//
// Range (lzm_conv.h:248-262). Weight row c is packed as W_c 2^e_c (largest |w| in [2^14, 2^15), e_c within
// +-kGnsWExp = 48); the epilogue multiplies by 2^-e_c and by 2^-s, one after the other and each exactly. Each stored
// activation tensor — the position's 32 planes of one layer — is stored as x 2^s, s from a bound known before the
// store: Wb M_in + Bb (+ M_res) with M_in the exact max of the layer's input (the waves' maxima meet in LDS at the
// barrier after each epilogue). A tile never straddles two positions, so there is one scale per workgroup. Every
// stored tensor's exact max is checked against its scale; a failure of a position < n adds 1 to *err (atomicAdd).
// ReLU propagates NaN. A block's input stays in the owning lane's registers as exact f32 (the accumulator -> (row,
// channel) map is the same in every layer), so the buffers ping-pong with one barrier per layer.
//
// The rest: conv0 (3 -> 32, K = 27) stays on v_mfma_f32_16x16x4_f32 from an f32 staging of the input planes; its
// outputs are scaled from their own exact max (one more barrier). The 1x1 heads run split, one chunk on the A-read
// path of the 3x3 layers' centre tap, and write f32 [32][N^2] into the free buffer; the FC1 / LayerNorm / FC2 /
// softmax tail is lzm_az_gomoku_n_net.h's f32 VALU arithmetic in the same order (duplicated here: that header is not
// to change).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_az_gomoku_n_split_host.h"  // (this unit defines LZM_DEVICE_HELPERS_ONLY)
#include "lzm_tree.h"                    // xor_partner, xor_sum, xor_max

namespace lzm {

constexpr int kGnsThreads = 256;

template <int N>
struct Gns {
  static constexpr int cells = N * N;
  static constexpr int pw = N + 2, bcells = pw * pw;       // bordered plane
  static constexpr int tiles = (cells + 15) / 16;          // row tiles of the position
  static constexpr int tw = (tiles + 3) / 4;               // row tiles of a wave: tw on waves < full, tw - 1 above
  static constexpr int full = tiles - 4 * (tw - 1);
  static constexpr int buf_bytes = bcells * 128;           // one activation buffer: [cell][term][32 ch] fp16
  static constexpr int lds_bytes = 2 * buf_bytes;
  static constexpr int flat = 16 * cells;                  // inputs of a head's FC1
  static_assert(tw >= 2 && full >= 1 && full <= 4, "row tiles over four waves");
  static_assert(16 * (tiles - 1) < cells && 16 * (tiles - 1) >= 16, "rows past N^2 read row p - 16");
  static_assert(32 * cells * 4 <= buf_bytes, "the heads' f32 outputs fit one buffer");
  static_assert(lds_bytes + 4 * bcells * 4 + 1024 <= 160 * 1024, "LDS");
};

// the swizzle key of the cell that row (16 t + l15) reads at tap (dy, dx); rows are 16 apart across tiles, so the
// key does not depend on the tile
template <int N>
__device__ __forceinline__ int gns_key(int l15, int dy, int dx) {
  return (l15 + N * dy + dx) & 6;
}

// one 3x3 layer for this wave's NT row tiles x both N tiles. bw: the layer's fragments [chunk][N tile][term];
// wn: the next layer's, at this lane, loaded into bw behind the chunks as they retire. src: the input buffer
// (bytes); cb[i]: byte offset of row tile i's window corner for this lane. Per accumulator the chunks go in order
// and l h, h l, h h within a chunk; a chunk's MFMAs are term-major so that the independent accumulators separate an
// accumulator's uses.
template <int N, int NT, int TW>
__device__ __forceinline__ void gns_conv(const char *src, const int (&cb)[TW], uint4 (&bw)[9][2][kBxTerms],
                                         const uint4 *__restrict__ wn, int lane, bxf4 (&acc)[TW][2]) {
  constexpr int PW = Gns<N>::pw;
  const int l15 = lane & 15, g = lane >> 4;
  uint4 a[2][NT][kBxTerms];
  auto load_a = [&](int s) {
    const int dy = s / 3, dx = s % 3;
    const int koff = (g ^ gns_key<N>(l15, dy, dx)) << 4;  // the h term's chunk; the l term's is 64 bytes across
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int q = 0; q < kBxTerms; ++q)
        a[s & 1][i][q] = *reinterpret_cast<const uint4 *>(src + (cb[i] + (koff ^ (q << 6))) + (dy * PW + dx) * 128);
  };
  auto load_w = [&](int s) {
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int q = 0; q < kBxTerms; ++q) bw[s][nt][q] = wn[((s * 2 + nt) * kBxTerms + q) * 64];
  };
  load_a(0);
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[i][nt] = bxf4{0.f, 0.f, 0.f, 0.f};
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    if (s >= 1) load_w(s - 1);
    if (s + 1 < 9) load_a(s + 1);
    const uint4(&x)[NT][kBxTerms] = a[s & 1];
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        acc[i][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(x[i][1]), bx_ash(bw[s][nt][0]), acc[i][nt], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        acc[i][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(x[i][0]), bx_ash(bw[s][nt][1]), acc[i][nt], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
        acc[i][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(x[i][0]), bx_ash(bw[s][nt][0]), acc[i][nt], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
  load_w(8);
}

// this lane's outputs y (tile i, N tile nt, v: row 16 (wave + 4 i) + 4 (lane >> 4) + v, channel 16 nt + lane % 16;
// all >= +0 or NaN) times `so` as the two fp16 terms into dst; oc[i][v]: 64 x the row's bordered cell, < 0 for rows
// past N^2. Returns the max of the valid outputs as unsigned bits (a NaN of either sign above +inf).
template <int N, int NT, int TW>
__device__ __forceinline__ uint32_t gns_put(const float (&y)[TW][2][4], const int (&oc)[TW][4], uint16_t *dst,
                                            float so, int lane) {
  const int l15 = lane & 15, g = lane >> 4;
  uint32_t mx = 0u;
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        // the cell is the row's interior cell (y + 1, x + 1): key (p + N + 1) & 6, p = 4 g + v mod 8
        const int sub = (((2 * nt + (l15 >> 3)) ^ gns_key<N>(4 * g + v, 1, 1)) << 3) + (l15 & 7);
        uint16_t h, l;
        bx_split2(y[i][nt][v] * so, h, l);
        if (oc[i][v] >= 0) {
          mx = max(mx, __float_as_uint(y[i][nt][v]));
          dst[oc[i][v] + sub] = h;
          dst[oc[i][v] + (sub ^ 32)] = l;
        }
      }
  return mx;
}

// conv0 for this wave's NT tiles: 3 -> 32 on the f32 MFMA, one K step per tap (the fourth k is a zero plane);
// x = relu(acc + b) is block 0's input
template <int N, int NT, int TW>
__device__ __forceinline__ void gns_conv0(const float *in0, const int (&c0)[TW], const float *__restrict__ w0f,
                                          const float (&b0v)[2], int lane, float (&xres)[TW][2][4]) {
  constexpr int PW = Gns<N>::pw;
  float w0[2][9];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) w0[nt][tap] = w0f[(nt * 9 + tap) * 64 + lane];
  bxf4 acc[NT][2];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) acc[i][nt] = bxf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int i = 0; i < NT; ++i) {
      const float a = in0[c0[i] + (tap / 3) * PW + tap % 3];
#pragma unroll
      for (int nt = 0; nt < 2; ++nt) acc[i][nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, w0[nt][tap], acc[i][nt], 0, 0, 0);
    }
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float x = acc[i][nt][v] + b0v[nt];
        xres[i][nt][v] = x <= 0.f ? 0.f : x;
      }
}

// one residual-block layer for this wave's NT tiles: the convolution, then y = relu(acc 2^-e_c 2^-s_in + b (+ the
// block input)) stored at scale `so`; returns the lane's max (bits)
template <int N, int NT, int TW>
__device__ __forceinline__ uint32_t gns_layer(const char *src, uint16_t *dst, const int (&cb)[TW], const int (&oc)[TW][4],
                                              uint4 (&bw)[9][2][kBxTerms], const uint4 *__restrict__ wn,
                                              const float (&wsc)[2], const float (&bc)[2], float f, float so,
                                              bool second, float (&xres)[TW][2][4], int lane) {
  bxf4 acc[TW][2];
  gns_conv<N, NT, TW>(src, cb, bw, wn, lane, acc);
  float y[TW][2][4];
#pragma unroll
  for (int i = 0; i < NT; ++i)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        float x = __fmaf_rn(acc[i][nt][v] * wsc[nt], f, bc[nt]);
        if (second) x += xres[i][nt][v];
        x = x <= 0.f ? 0.f : x;  // NaN stays NaN, -0 becomes +0
        if (second) xres[i][nt][v] = x;
        y[i][nt][v] = x;
      }
  return gns_put<N, NT, TW>(y, oc, dst, so, lane);
}

// the 1x1 heads for this wave's NT tiles: 32 -> 32 (value 0..15 | policy 16..31), one split chunk at the centre tap,
// into hd as f32 [32][N^2]
template <int N, int NT, int TW>
__device__ __forceinline__ void gns_heads(const char *src, float *hd, const int (&cb)[TW], const int (&oc)[TW][4],
                                          const uint4 *__restrict__ hw, const float (&hsc)[2], const float (&bv)[2],
                                          float f, int wv, int lane) {
  constexpr int PW = Gns<N>::pw, C = Gns<N>::cells;
  const int l15 = lane & 15, g = lane >> 4;
  uint4 bh[2][kBxTerms];
#pragma unroll
  for (int nt = 0; nt < 2; ++nt)
#pragma unroll
    for (int q = 0; q < kBxTerms; ++q) bh[nt][q] = hw[(nt * kBxTerms + q) * 64];
  const int koff = (g ^ gns_key<N>(l15, 1, 1)) << 4;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    const uint4 xh = *reinterpret_cast<const uint4 *>(src + (cb[i] + koff) + (PW + 1) * 128);
    const uint4 xl = *reinterpret_cast<const uint4 *>(src + (cb[i] + (koff ^ 64)) + (PW + 1) * 128);
#pragma unroll
    for (int nt = 0; nt < 2; ++nt) {
      bxf4 a1 = bxf4{0.f, 0.f, 0.f, 0.f};
      a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(xl), bx_ash(bh[nt][0]), a1, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(xh), bx_ash(bh[nt][1]), a1, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(xh), bx_ash(bh[nt][0]), a1, 0, 0, 0);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int p = 16 * (wv + 4 * i) + 4 * g + v;
        const float yv = __fmaf_rn(a1[v] * hsc[nt], f, bv[nt]);
        if (oc[i][v] >= 0) hd[(16 * nt + l15) * C + p] = yv <= 0.f ? 0.f : yv;
      }
    }
  }
}

// state [n][3][N][N] -> probs [n][N^2], value [n]; *err += positions whose activations left the split's range
template <int NRES, int N>
__global__ void __launch_bounds__(kGnsThreads) gomoku_n_net_eval_split_kernel(const float *__restrict__ w,
                                                                              const float *__restrict__ state, int n,
                                                                              float *probs, float *value, int32_t *err) {
  using G = Gns<N>;
  constexpr int C = G::cells, PW = G::pw, TW = G::tw, NL = 4 * NRES;
  extern __shared__ uint4 gns_lds4[];
  __shared__ float s_in0[4 * G::bcells];  // the input planes, f32, zero-bordered (plane 3: zero)
  __shared__ __attribute__((aligned(16))) uint32_t s_wm[2][4];  // the waves' maxima, two layers' worth
  __shared__ float part[2 * 32];          // FC1 outputs [head][32]
  char *lds = reinterpret_cast<char *>(gns_lds4);
  const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, l15 = lane & 15;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool whole = G::full == 4 || wv < G::full;  // this wave owns TW row tiles (else TW - 1); wave-uniform
  const GmkNSplitLayout L = gmkn_split_layout(NRES, N);
  const int b0 = blockIdx.x;
  auto layer_w = [&](int l) { return reinterpret_cast<const uint4 *>(w + L.conv) + (size_t)l * (kGnsFrag3 / 4) + lane; };

  // layer 0's fragments, in flight while LDS is cleared and the input staged
  uint4 bw[9][2][kBxTerms];
  {
    const uint4 *w0 = layer_w(0);
#pragma unroll
    for (int s = 0; s < 9; ++s)
#pragma unroll
      for (int nt = 0; nt < 2; ++nt)
#pragma unroll
        for (int q = 0; q < kBxTerms; ++q) bw[s][nt][q] = w0[((s * 2 + nt) * kBxTerms + q) * 64];
  }
  for (int i = tid; i < G::lds_bytes / 16; i += kGnsThreads) gns_lds4[i] = uint4{0u, 0u, 0u, 0u};
  for (int i = tid; i < 4 * G::bcells; i += kGnsThreads) s_in0[i] = 0.0f;
  __syncthreads();
  if (b0 < n)
    for (int e = tid; e < 3 * C; e += kGnsThreads) {
      const int c = e / C, p = e % C;
      s_in0[c * G::bcells + (p / N + 1) * PW + p % N + 1] = state[(size_t)b0 * 3 * C + e];
    }
  // this lane's A rows: the window's top-left corner (rows past N^2 read row p - 16, see the header); a tile past
  // the wave's last is never used
  int cb[TW], c0[TW], oc[TW][4];
#pragma unroll
  for (int i = 0; i < TW; ++i) {
    const int t = wv + 4 * i < G::tiles ? wv + 4 * i : wv;
    int p = 16 * t + l15;
    if (p >= C) p -= 16;
    const int corner = (p / N) * PW + p % N;
    cb[i] = corner * 128;
    c0[i] = g * G::bcells + corner;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int po = 16 * t + 4 * g + v;
      oc[i][v] = po < C ? ((po / N + 1) * PW + po % N + 1) * 64 : -1;
    }
  }
  __syncthreads();

  float xres[TW][2][4];  // the current block's input, exact f32
  // ---- conv0, stored scaled from its own exact max
  {
    const float b0v[2] = {w[L.conv0_b + l15], w[L.conv0_b + 16 + l15]};
    if (whole)
      gns_conv0<N, TW, TW>(s_in0, c0, w + L.conv0, b0v, lane, xres);
    else
      gns_conv0<N, TW - 1, TW>(s_in0, c0, w + L.conv0, b0v, lane, xres);
    uint32_t mx = 0u;
#pragma unroll
    for (int i = 0; i < TW; ++i)
      if (i < TW - 1 || whole)
#pragma unroll
        for (int nt = 0; nt < 2; ++nt)
#pragma unroll
          for (int v = 0; v < 4; ++v) mx = max(mx, oc[i][v] >= 0 ? __float_as_uint(xres[i][nt][v]) : 0u);
    bx_post_umax(s_wm[1], mx, wv, lane);
  }
  __syncthreads();
  BxRange rg = bx_range_input(bx_read_max(s_wm[1]));
  {
    const float so = bx_pow2(rg.s_in);
    uint16_t *dst = reinterpret_cast<uint16_t *>(lds);
    if (whole)
      gns_put<N, TW, TW>(xres, oc, dst, so, lane);
    else
      gns_put<N, TW - 1, TW>(xres, oc, dst, so, lane);
  }
  __syncthreads();

  // ---- the residual blocks: layer l reads buffer l & 1 and writes the other; odd layers add the block input
#pragma unroll 1
  for (int l = 0; l < NL; ++l) {
    const bool second = l & 1;
    const float bc[2] = {w[L.conv_b + l * 32 + l15], w[L.conv_b + l * 32 + 16 + l15]};
    const float wsc[2] = {w[L.conv_inv + l * 32 + l15], w[L.conv_inv + l * 32 + 16 + l15]};
    const float4 bd = reinterpret_cast<const float4 *>(w + L.conv_bd)[l];
    const int s_out = bx_layer_scale(bd, second, rg);
    const float f = bx_pow2(-rg.s_in), so = bx_pow2(s_out);
    const char *src = lds + (l & 1) * G::buf_bytes;
    uint16_t *dst = reinterpret_cast<uint16_t *>(lds + ((l + 1) & 1) * G::buf_bytes);
    const uint4 *wn = layer_w(l + 1 < NL ? l + 1 : l);  // (the last layer reloads its own: no branch in the stream)
    const uint32_t mx = whole ? gns_layer<N, TW, TW>(src, dst, cb, oc, bw, wn, wsc, bc, f, so, second, xres, lane)
                              : gns_layer<N, TW - 1, TW>(src, dst, cb, oc, bw, wn, wsc, bc, f, so, second, xres, lane);
    bx_post_umax(s_wm[l & 1], mx, wv, lane);
    __syncthreads();
    bx_range_take(rg, s_wm[l & 1], s_out);
  }
  if (tid == 0 && rg.bad && b0 < n) atomicAdd(err, 1);

  // ---- 1x1 heads, split: from buffer 0 into buffer 1's bytes as f32 [32][N^2]
  float *hd = reinterpret_cast<float *>(lds + G::buf_bytes);
  {
    const float bv[2] = {w[L.head_b + l15], w[L.head_b + 16 + l15]};
    const float hsc[2] = {w[L.head_inv + l15], w[L.head_inv + 16 + l15]};
    const uint4 *hw = reinterpret_cast<const uint4 *>(w + L.head) + lane;
    const float f = bx_pow2(-rg.s_in);
    if (whole)
      gns_heads<N, TW, TW>(lds, hd, cb, oc, hw, hsc, bv, f, wv, lane);
    else
      gns_heads<N, TW - 1, TW>(lds, hd, cb, oc, hw, hsc, bv, f, wv, lane);
  }
  __syncthreads();
  if (b0 >= n) return;  // (the grid is n workgroups; no barrier follows)

  // ---- the tail of lzm_az_gomoku_n_net.h. FC1: wave = (head wv >> 1, units 16 (wv & 1) ..), lane = 4 unit + quarter
  {
    const int head = wv >> 1, qtr = lane & 3;
    const bxf4 *fw = reinterpret_cast<const bxf4 *>(w + L.fc1) + ((size_t)head * C * 2 + (wv & 1)) * 64 + lane;
    const bxf4 *in = reinterpret_cast<const bxf4 *>(hd + head * G::flat + qtr * 4 * C);
    float hs = 0.0f;
#pragma unroll 9
    for (int i = 0; i < C; ++i) {
      const bxf4 a = fw[(size_t)i * 128];
      const bxf4 x = in[i];
      hs = fmaf(a[0], x[0], hs);
      hs = fmaf(a[1], x[1], hs);
      hs = fmaf(a[2], x[2], hs);
      hs = fmaf(a[3], x[3], hs);
    }
    hs += xor_partner<1>(hs);
    hs += xor_partner<2>(hs);
    if (qtr == 0) part[head * 32 + 16 * (wv & 1) + (lane >> 2)] = hs;
  }
  __syncthreads();

  // ---- head wv on wave wv: LayerNorm, ReLU, FC2 (and the softmax, action lane + 64 k)
  if (wv < 2) {
    const int head = wv, b = b0;
    const float *tw = w + (head ? L.tail_p : L.tail_v);
    float h[32];
#pragma unroll
    for (int u = 0; u < 32; ++u) h[u] = part[head * 32 + u] + tw[kGmkNT1b + u];
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
