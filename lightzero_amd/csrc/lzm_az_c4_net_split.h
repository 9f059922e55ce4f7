// lzm_az_c4_net_split.h — the Connect4 AlphaZeroModel of lzm_az_c4_net.h (same network, same outputs' meaning) with
// its 64 -> 64 3x3 layers on v_mfma_f32_16x16x32_f16 in the split-fp16 scheme of lzm_conv.h: every f32 operand is two
// fp16 terms x = h + l, a product the sum of l_a h_b, h_a l_b, h_a h_b (in that order), error at the f32 level.
// Opt-in (Connect4AZNet(precision="split")); the exact-f32 kernel stays the default.
//
// GEMM. Rows = (position, cell): a workgroup of 4 waves owns P positions (template parameter, 2 or 4) for the whole
// network, 42 P rows in T = ceil(42 P / 16) row tiles. N = out channels, wave w owns 16 w .. 16 w + 15 and reads each
// B fragment once per layer for all T tiles. K = tap-major, in-channel-minor: 576 = 18 chunks of 32 (tap, channel
// half), three MFMAs per chunk: 54 MFMAs per (row tile, layer) against 144 on v_mfma_f32_16x16x4_f32. Every output
// element is one chain in one accumulator in chunk order, so its bits do not depend on the tile, the workgroup, n,
// P or the neighbouring positions (the scales below are per position as well).
//
// Activations in LDS: two buffers, each the two fp16 term planes [position][72 bordered cells (8 x 9)][64 ch],
// 36,864 B per position in all — the f32 kernel's bytes. A lane's A fragment is one ds_read_b128: cell lane & 15 of
// the tile, channels 32 j + 8 (lane >> 4) .. +7. The 16-byte chunk c of cell (position r, plane row y, column x) is
// stored at chunk c ^ (n & 6), n = 7 y + x + 42 r. For row m = 42 r + p and tap (dy, dx) the cell read has
// n = m + 7 dy + dx: n runs with the row index across plane rows and positions alike, and the cell's address
// parity (bit 7 of the byte address; 72 cells per position is even) alternates with m as well (a step of 1 or 3
// cells inside a position, 51 cells back at a position's end). A ds_read_b128 lane group (MI355X_MICROARCH.md:
// lanes {0-3, 12-15, 20-27} and {4-11, 16-19, 28-31} of each wave half) holds rows {0-3, 12-15} of one channel
// chunk c and rows {4-11} of chunk c ^ 1. Per address parity that is four rows 2 apart twice: (n & 6) takes all four
// values over {m, m + 2, m + 12, m + 14} and over {m + 4 .. m + 10}, and the two sets differ in bit 0 of the chunk,
// so the sixteen lanes hit sixteen distinct 16-byte bank slots. Rows past 42 P (the last tile) read row m - 16: the
// same key and parity as row m would have. Enumerated on the host for P = 2, 3, 4 over every tile, tap, channel
// half and the four lane groups: worst case one address per bank slot (4 without the swizzle; `chunk ^ column`,
// the 10-wide plane's key, gives 3 here). lzm_conv.h's `chunk ^ (pos % 10 & 7)` is this key's analogue for tiles
// that are two whole plane rows.
//
// Weights: host-packed [layer][wave][chunk][term][lane][8 fp16] (lzm_conv.h's bx_pack3 per layer), one 16-byte load
// per lane per term per chunk, in lzm_conv.h's register ring kC4sAhead chunks ahead; the next layer's first chunks
// are issued before the current epilogue and barrier. 147 KB per layer per workgroup from L2: more positions per
// workgroup amortise that stream (DESIGN.md §5.4c has the timings of P = 2 and 4).
//
// Range (lzm_conv.h:248-262). Weight row c is packed as W_c 2^e_c (largest |w| in [2^14, 2^15), e_c within
// +-kC4sWExp = 48: wider than the trunks' +-kBxWExp, so that a row as small as 2^-30 still keeps its 22 bits) and
// the epilogue multiplies by 2^-e_c and by 2^-s, one after the other and each exactly (their product could leave
// the normal f32 range; a product that underflows here is below 2^-126 either way). The heads' rows keep +-kBxWExp. Each stored activation tensor — one POSITION's 64
// planes of one layer — is stored as x 2^s, s from a bound known before the store: Wb M_in + Bb (+ M_res) with M_in
// the exact max of that position's layer input. A 16-row tile straddles two positions (42 rows each), so the lane
// maxima are bucketed by m / 42 (a tile's two positions are compile-time, the split point a compare); the waves'
// maxima meet in LDS at the barrier after each epilogue. No position's magnitude reaches another's scale. Every
// stored tensor's exact max is checked against its scale; a failure of a position < n adds 1 to *err (atomicAdd).
// ReLU propagates NaN. A block's input stays in the owning lane's registers as exact f32 (the accumulator ->
// (row, channel) map is the same in every layer), so the buffers ping-pong with one barrier per layer.
//
// The rest: conv0 (3 -> 64, K = 27, 0.5% of the work) stays on v_mfma_f32_16x16x4_f32 from a small f32 staging of
// the input planes; its outputs are scaled from their own exact max (one more barrier). The 1x1 heads (K = 64) run
// split, two chunks on the same A-read path as the 3x3 layers (no second activation format), and write f32 planes;
// the FC1 / LayerNorm / FC2 / softmax tail is lzm_az_c4_net.h's f32 VALU arithmetic in the same order (duplicated
// here: that header is not to change), with one difference in work split only: at P = 4 a wave runs its head for two
// positions off one read of the FC1 weights.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_az_c4_net.h"
#include "lzm_conv.h"  // the split scheme's helpers (bx_*); this unit defines LZM_DEVICE_HELPERS_ONLY

namespace lzm {

static_assert(kC4sFrag3 == kBx3Frag && kC4sFrag1 == kBx1Frag, "lzm_az_c4_host.h restates lzm_conv.h's fragment sizes");

constexpr int kC4sAhead = 3;  // weight read-ahead (chunks)

template <int P>
struct C4s {
  static_assert(P == 2 || P == 4, "positions per workgroup");
  static constexpr int rows = 42 * P, T = (rows + 15) / 16;
  static constexpr int plane = P * kC4nPlane * kC4nC;  // 16-bit elements per term plane
  static constexpr int buf = kBxTerms * plane;         // per activation buffer
  static constexpr int lds_bytes = 2 * buf * 2;        // 36,864 P
};

// the two positions a tile's 16 rows can belong to, and whether row m is in the second
__device__ __forceinline__ constexpr int c4s_rlo(int t) { return 16 * t / 42; }
template <int P>
__device__ __forceinline__ constexpr int c4s_rhi(int t) { return (16 * t + 15) / 42 < P ? (16 * t + 15) / 42 : P - 1; }

// one 3x3 layer for this wave's 16 out channels x T row tiles; its first kC4sAhead chunks are in the ring. The
// tiles go in NG groups of at most 6 (P = 4: 6 + 5), so that the A fragments in flight stay at two groups' worth of
// registers. Issue order per step (chunk s, group gr), pinned by the scheduling barriers as in bx_conv: weights of
// chunk s + AHEAD (group 0), activations of the next step, this step's 3 x (tiles of the group) MFMAs, term-major,
// so the group's independent accumulators separate an accumulator's uses. Each accumulator still sees the chunks in
// order and l h, h l, h h within a chunk. src: the input buffer (bytes); cb[t]: byte offset of row tile t's window
// corner for this lane
template <int P>
__device__ __forceinline__ void c4s_conv(const char *src, const int (&cb)[C4s<P>::T], const uint4 *__restrict__ wf,
                                         BxRing<kC4sAhead> &ring, int lane, bxf4 (&acc)[C4s<P>::T]) {
  constexpr int T = C4s<P>::T, PB = C4s<P>::plane * 2, AHEAD = kC4sAhead;
  constexpr int NG = (T + 5) / 6, TG = (T + NG - 1) / NG, NU = 18 * NG;
  uint4 a[2][TG][kBxTerms];
  const int l15 = lane & 15, g = lane >> 4;
  auto tiles = [](int gr) { return (gr + 1) * TG <= T ? TG : T - gr * TG; };
  auto load_a = [&](int u) {
    const int s = u / NG, gr = u % NG, tap = s >> 1, j = s & 1, dy = tap / 3, dx = tap % 3;
    const int koff = ((4 * j + g) ^ ((l15 + 7 * dy + dx) & 6)) << 4;
#pragma unroll
    for (int t = 0; t < tiles(gr); ++t)
#pragma unroll
      for (int q = 0; q < kBxTerms; ++q)
        a[u & 1][t][q] =
            *reinterpret_cast<const uint4 *>(src + (cb[gr * TG + t] + koff) + ((dy * 9 + dx) * 128 + q * PB));
  };
  load_a(0);
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = bxf4{0.f, 0.f, 0.f, 0.f};
  __builtin_amdgcn_sched_barrier(0);
#pragma unroll
  for (int u = 0; u < NU; ++u) {
    const int s = u / NG, gr = u % NG, t0 = gr * TG, nt = tiles(gr);
    const bool lw = gr == 0 && s + AHEAD < 18;
    if (lw) bx_load_w<AHEAD, 0>(ring, wf, s + AHEAD, lane);
    if (u + 1 < NU) load_a(u + 1);
    const uint4 *w = ring.w[s % (AHEAD + 1)];
    const uint4(&x)[TG][kBxTerms] = a[u & 1];
#pragma unroll
    for (int t = 0; t < nt; ++t)
      acc[t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(x[t][1]), bx_ash(w[0]), acc[t0 + t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < nt; ++t)
      acc[t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(x[t][0]), bx_ash(w[1]), acc[t0 + t], 0, 0, 0);
#pragma unroll
    for (int t = 0; t < nt; ++t)
      acc[t0 + t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(x[t][0]), bx_ash(w[0]), acc[t0 + t], 0, 0, 0);
    const int nw = lw ? kBxTerms : 0, na = u + 1 < NU ? tiles((u + 1) % NG) * kBxTerms : 0;
    static_assert(3 * (T - (NG - 1) * TG) >= kBxTerms + TG * kBxTerms, "a step's MFMAs cover its loads");
#pragma unroll
    for (int k = 0; k < nw; ++k) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
      __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);  // VMEM read
    }
#pragma unroll
    for (int k = 0; k < na; ++k) {
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);  // MFMA
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);  // DS read
    }
#pragma unroll
    for (int k = 0; k < 3 * nt - nw - na; ++k) __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// this lane's outputs y (accumulator (t, v): row 16 t + 4 (lane >> 4) + v; all >= +0 or NaN) into per-position
// maxima (unsigned bits: a NaN of either sign above +inf), one word per (position, wave) in slot[4 pp + wave]
template <int P>
__device__ __forceinline__ void c4s_post_max(const float (&y)[C4s<P>::T][4], uint32_t *slot, int wv, int lane) {
  constexpr int T = C4s<P>::T, rows = C4s<P>::rows;
  const int q4 = 4 * (lane >> 4);
  uint32_t mx[P];
#pragma unroll
  for (int pp = 0; pp < P; ++pp) mx[pp] = 0u;
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = 16 * t + q4 + v, rlo = c4s_rlo(t), rhi = c4s_rhi<P>(t);
      const uint32_t bits = m < rows ? __float_as_uint(y[t][v]) : 0u;
      const bool hi = rhi != rlo && m >= 42 * rhi;
      mx[rlo] = max(mx[rlo], hi ? 0u : bits);
      if (rhi != rlo) mx[rhi] = max(mx[rhi], hi ? bits : 0u);
    }
#pragma unroll
  for (int pp = 0; pp < P; ++pp) bx_post_umax(slot + 4 * pp, mx[pp], wv, lane);
}

// y 2^s (so[pp] = 2^s of position pp) as the two fp16 terms into dst's planes; ob[t][v >> 1], half v & 1: the
// element's index in a term plane (swizzled; < 2^15), 0xffff for rows past 42 P
template <int P>
__device__ __forceinline__ void c4s_put(const float (&y)[C4s<P>::T][4], const float (&so)[P], uint16_t *dst,
                                        const uint32_t (&ob)[C4s<P>::T][2], int lane) {
  constexpr int T = C4s<P>::T;
  const int q4 = 4 * (lane >> 4);
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = 16 * t + q4 + v, rlo = c4s_rlo(t), rhi = c4s_rhi<P>(t);
      const bool hi = rhi != rlo && m >= 42 * rhi;
      uint16_t h, l;
      bx_split2(y[t][v] * (hi ? so[rhi] : so[rlo]), h, l);
      const uint32_t o = (v & 1) ? ob[t][v >> 1] >> 16 : ob[t][v >> 1] & 0xffffu;
      if (o != 0xffffu) {
        dst[o] = h;
        dst[C4s<P>::plane + o] = l;
      }
    }
}

// state [n][3][6][7] -> probs [n][7], value [n]; *err += positions whose activations left the split's range
template <int NRES, int P>
__global__ void __launch_bounds__(kC4nThreads) __attribute__((amdgpu_waves_per_eu(1, 1)))
c4_net_eval_split_kernel(const float *__restrict__ w, const float *__restrict__ state, int n, float *probs,
                         float *value, int32_t *err) {
  constexpr int T = C4s<P>::T, rows = C4s<P>::rows, NL = 4 * NRES, AHEAD = kC4sAhead;
  extern __shared__ uint4 c4s_lds4[];
  __shared__ float s_in0[P * 4 * kC4nPlane];  // the input planes, f32, zero-bordered (plane 3: zero)
  __shared__ __attribute__((aligned(16))) uint32_t s_wm[2][4 * P];  // per (position, wave) maxima, two layers' worth
  __shared__ float4 s_bd[4 * 2];              // the layers' {Wb, Bb}
  uint16_t *lds = reinterpret_cast<uint16_t *>(c4s_lds4);
  const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, q = lane >> 4, l15 = lane & 15;
  const int ch = 16 * wv + l15;
  const C4SplitLayout L = c4_split_layout(NRES);
  const int b0 = blockIdx.x * P;
  auto wave_stream = [&](int l) {
    return reinterpret_cast<const uint4 *>(w + L.conv) + (size_t)(l * 4 + wv) * (18 * kBxTerms * 64);
  };

  // the stream's first chunks and conv0's fragments, in flight while LDS is cleared and the input staged
  BxRing<AHEAD> ring;
  bx_prefetch<18, AHEAD, 0>(ring, wave_stream(0), lane);
  float w0[9];
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) w0[tap] = w[L.conv0 + (wv * 9 + tap) * 64 + lane];
  const float b0v = w[L.conv0_b + ch];
  if (tid < NL) s_bd[tid] = reinterpret_cast<const float4 *>(w + L.conv_bd)[tid];
  for (int i = tid; i < C4s<P>::lds_bytes / 16; i += kC4nThreads) c4s_lds4[i] = uint4{0u, 0u, 0u, 0u};
  for (int i = tid; i < P * 4 * kC4nPlane; i += kC4nThreads) s_in0[i] = 0.0f;
  __syncthreads();
  for (int e = tid; e < P * 126; e += kC4nThreads) {
    const int r = e / 126, c = e % 126;
    if (b0 + r < n) s_in0[(r * 4 + c / 42) * kC4nPlane + c4n_interior(c % 42)] = state[(size_t)(b0 + r) * 126 + c];
  }
  // this lane's A rows: the window's top-left corner (rows past 42 P read row m - 16, see the header)
  int cb[T], c0[T];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    int m = 16 * t + l15;
    if (m >= rows) m -= 16;
    const int r = m / 42, p = m % 42, corner = (p / 7) * 9 + p % 7;
    cb[t] = (r * kC4nPlane + corner) * 128;
    c0[t] = (r * 4 + q) * kC4nPlane + corner;
  }
  // this lane's outputs: element index in a term plane
  static_assert(C4s<P>::plane < 0xffff, "element indices are packed in 16 bits");
  uint32_t ob[T][2];
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const int m = 16 * t + 4 * q + v, r = m / 42, p = m % 42;
      const uint32_t o =
          m < rows ? (r * kC4nPlane + c4n_interior(p)) * 64 + ((((ch >> 3) ^ ((m + 8) & 6)) & 7) << 3) + (ch & 7) : 0xffffu;
      ob[t][v >> 1] = (v & 1) ? ob[t][v >> 1] | (o << 16) : o;
    }
  __syncthreads();

  bxf4 acc[T];
  float xres[T][4];  // the current block's input, exact f32
  BxRange rg[P];
  float so[P];
  // ---- conv0: 3 -> 64 on the f32 MFMA, one K step per tap; stored scaled from its own exact max
#pragma unroll
  for (int t = 0; t < T; ++t) acc[t] = bxf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int tap = 0; tap < 9; ++tap)
#pragma unroll
    for (int t = 0; t < T; ++t)
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(s_in0[c0[t] + (tap / 3) * 9 + tap % 3], w0[tap], acc[t], 0, 0, 0);
#pragma unroll
  for (int t = 0; t < T; ++t)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float x = acc[t][v] + b0v;
      xres[t][v] = x <= 0.f ? 0.f : x;
    }
  c4s_post_max<P>(xres, s_wm[1], wv, lane);
  __syncthreads();
#pragma unroll
  for (int pp = 0; pp < P; ++pp) {
    rg[pp] = bx_range_input(bx_read_max(s_wm[1] + 4 * pp));
    so[pp] = bx_pow2(rg[pp].s_in);
  }
  c4s_put<P>(xres, so, lds, ob, lane);
  __syncthreads();

  // ---- the residual blocks: layer l reads buffer l & 1 and writes the other; odd layers add the block input
#pragma unroll 1
  for (int l = 0; l < NL; ++l) {
    const bool second = l & 1;
    const float bc = w[L.conv_b + l * 64 + ch], wsc = w[L.conv_inv + l * 64 + ch];
    const float4 bd = s_bd[l];
    c4s_conv<P>(reinterpret_cast<const char *>(lds + (l & 1) * C4s<P>::buf), cb, wave_stream(l), ring, lane, acc);
    if (l + 1 < NL) bx_prefetch<18, AHEAD, 0>(ring, wave_stream(l + 1), lane);
    float f[P];
    int s_out[P];
#pragma unroll
    for (int pp = 0; pp < P; ++pp) {
      s_out[pp] = bx_layer_scale(bd, second, rg[pp]);
      f[pp] = bx_pow2(-rg[pp].s_in);
      so[pp] = bx_pow2(s_out[pp]);
    }
    float y[T][4];
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int m = 16 * t + 4 * q + v, rlo = c4s_rlo(t), rhi = c4s_rhi<P>(t);
        const bool hi = rhi != rlo && m >= 42 * rhi;
        float x = __fmaf_rn(acc[t][v] * wsc, hi ? f[rhi] : f[rlo], bc);
        if (second) x += xres[t][v];
        x = x <= 0.f ? 0.f : x;  // NaN stays NaN, -0 becomes +0
        if (second) xres[t][v] = x;
        y[t][v] = x;
      }
    c4s_post_max<P>(y, s_wm[l & 1], wv, lane);
    c4s_put<P>(y, so, lds + ((l + 1) & 1) * C4s<P>::buf, ob, lane);
    __syncthreads();
#pragma unroll
    for (int pp = 0; pp < P; ++pp) bx_range_take(rg[pp], s_wm[l & 1] + 4 * pp, s_out[pp]);
  }
  if (tid == 0) {
    int bad = 0;
#pragma unroll
    for (int pp = 0; pp < P; ++pp) bad += (rg[pp].bad && b0 + pp < n) ? 1 : 0;
    if (bad) atomicAdd(err, bad);
  }

  // ---- 1x1 heads, split: 64 -> 32 (value 0..15 | policy 16..31) from buffer 0 into buffer 1's bytes as f32
  // [position][32][42]. (row tile t, N tile nt) runs on the wave with nt = wave & 1, t & 1 = wave >> 1
  float *hd = reinterpret_cast<float *>(lds + C4s<P>::buf);
  {
    const int nt = wv & 1, hc = 16 * nt + l15;
    const uint4 *hw = reinterpret_cast<const uint4 *>(w + L.head) + nt * 2 * kBxTerms * 64 + lane;
    uint4 bh[2][kBxTerms];
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < kBxTerms; ++k) bh[j][k] = hw[(j * kBxTerms + k) * 64];
    const float bv = w[L.head_b + hc], hsc = w[L.head_inv + hc];
    float f[P];
#pragma unroll
    for (int pp = 0; pp < P; ++pp) f[pp] = hsc * bx_pow2(-rg[pp].s_in);
    const char *src = reinterpret_cast<const char *>(lds);
#pragma unroll
    for (int t = 0; t < T; ++t) {
      if ((t & 1) != (wv >> 1)) continue;  // wave-uniform
      bxf4 a1 = bxf4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int koff = ((4 * j + q) ^ ((l15 + 8) & 6)) << 4;
        const uint4 xh = *reinterpret_cast<const uint4 *>(src + (cb[t] + koff) + 10 * 128);
        const uint4 xl = *reinterpret_cast<const uint4 *>(src + (cb[t] + koff) + (10 * 128 + C4s<P>::plane * 2));
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(xl), bx_ash(bh[j][0]), a1, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(xh), bx_ash(bh[j][1]), a1, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(bx_ash(xh), bx_ash(bh[j][0]), a1, 0, 0, 0);
      }
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int m = 16 * t + 4 * q + v, rlo = c4s_rlo(t), rhi = c4s_rhi<P>(t);
        const bool hi = rhi != rlo && m >= 42 * rhi;
        const float yv = __fmaf_rn(a1[v], hi ? f[rhi] : f[rlo], bv);
        if (m < rows) hd[(m / 42) * kC4nHd + hc * 42 + m % 42] = yv <= 0.f ? 0.f : yv;
      }
    }
  }
  __syncthreads();

  // ---- the tail of lzm_az_c4_net.h: head wave & 1 for positions (wave >> 1) + 2 k on this wave; FC1 as 32 units x
  // 2 lanes (336 products per lane in index order, the halves added by a DPP swap), LayerNorm, ReLU, FC2, softmax
  constexpr int NB = P / 2;
  const int head = wv & 1, unit = lane >> 1, half = lane & 1;
  if (b0 + (wv >> 1) >= n) return;  // wave-uniform, no barrier follows (positions ascend with k)
  const c4f4 *fw = reinterpret_cast<const c4f4 *>(w + L.fc1) + head * 84 * 64 + lane;
  const c4f4 *in = reinterpret_cast<const c4f4 *>(hd + (wv >> 1) * kC4nHd + head * kC4nFlat + half * 336);
  float hs[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) hs[k] = 0.0f;
#pragma unroll 6
  for (int i = 0; i < 84; ++i) {
    const c4f4 a = fw[i * 64];
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      const c4f4 x = in[k * 2 * (kC4nHd / 4) + i];
      hs[k] = fmaf(a[0], x[0], hs[k]);
      hs[k] = fmaf(a[1], x[1], hs[k]);
      hs[k] = fmaf(a[2], x[2], hs[k]);
      hs[k] = fmaf(a[3], x[3], hs[k]);
    }
  }
  const float *tw = w + (head ? L.tail_p : L.tail_v);
#pragma unroll 1
  for (int k = 0; k < NB; ++k) {
    const int b = b0 + (wv >> 1) + 2 * k;
    if (b >= n) return;
    float hsum = hs[k];
    hsum += xor_partner<1>(hsum);
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
}

}  // namespace lzm
