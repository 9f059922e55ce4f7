// lzm_az_gomoku_n_split_host.h — what the split-fp16 Gomoku 9 x 9 / 15 x 15 network (lzm_az_gomoku_n_net_split.h)
// shares with its entry points in lzm_kernels.hip: the prepared weight buffer's layout, the host packing and the
// launcher. A sibling of lzm_az_gomoku_n_host.h, which it leaves as it is. The includer decides how much of
// lzm_conv.h it takes (LZM_DEVICE_HELPERS_ONLY).
#pragma once
#include <vector>

#include "lzm_az_gomoku_n_host.h"
#include "lzm_conv.h"  // the split scheme's host helpers: bx_row_exp, bx_split2, bx_round_up, bx_bias_bound

namespace lzm {

// a 32 -> 32 3x3 layer: [chunk = tap 9][N tile 2][term 2][lane 64][8 fp16]; the 1x1 heads: one chunk
constexpr int kGnsFrag3 = 9 * 2 * kBxTerms * 64 * 4;  // floats
constexpr int kGnsFrag1 = 2 * kBxTerms * 64 * 4;
constexpr int kGnsWExp = 48;  // weight-row scale exponents within +-48: a row as small as 2^-30 keeps its 22 bits

// conv0, the biases, FC1 and the tails are the f32 network's blocks (GmkNNetLayout)
struct GmkNSplitLayout {
  int conv0, conv0_b;
  int conv;                    // [layer] kGnsFrag3
  int conv_b, conv_inv;        // bias [layers][32], 2^-e_c [layers][32]
  int conv_bd;                 // [layers] {Wb = max row L1 norm, Bb = max |bias|, 0, 0}
  int head, head_b, head_inv;  // kGnsFrag1, bias [32], 2^-e_c [32]
  int fc1, tail_v, tail_p;
  int total;
};

__host__ __device__ inline GmkNSplitLayout gmkn_split_layout(int nres, int n_board) {
  const int cells = n_board * n_board;
  GmkNSplitLayout L;
  int o = 0;
  auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
  L.conv0 = take(2 * 9 * 64); L.conv0_b = take(32);
  L.conv = take(4 * nres * kGnsFrag3);
  L.conv_b = take(4 * nres * 32); L.conv_inv = take(4 * nres * 32); L.conv_bd = take(4 * nres * 4);
  L.head = take(kGnsFrag1); L.head_b = take(32); L.head_inv = take(32);
  L.fc1 = take(2 * 32 * 16 * cells);
  L.tail_v = take(kGmkNTv2b + 1); L.tail_p = take(gmkn_tp2b(cells) + cells);
  L.total = o;
  return L;
}

// one K = 32 chunk of a weight matrix as the B operand of v_mfma_f32_16x16x32_f16, both terms: lane holds out
// channel 16 nt + lane % 16, in channels 8 (lane / 16) .. + 7. W(cout, cin) is the unscaled weight, e[cout] its row's
// scale exponent; out: [N tile 2][term 2][lane 64][8 fp16]
template <class Weight>
inline void gmkn_split_chunk(Weight W, const int *e, uint16_t *out) {
  for (int nt = 0; nt < 2; ++nt)
    for (int lane = 0; lane < 64; ++lane)
      for (int el = 0; el < 8; ++el) {
        const int cout = 16 * nt + (lane & 15), cin = 8 * (lane >> 4) + el;
        uint16_t t[kBxTerms];
        bx_split2(ldexpf(W(cout, cin), e[cout]), t[0], t[1]);
        for (int q = 0; q < kBxTerms; ++q) out[((nt * kBxTerms + q) * 64 + lane) * 8 + el] = t[q];
      }
}

// raw (the order of lzm_az_gmkn_net_prepare) -> the split kernel's buffer
inline void gmkn_split_pack(int nres, int n_board, const float *raw, float *out) {
  const int cells = n_board * n_board;
  const GmkNNetLayout F = gmkn_net_layout(nres, n_board);
  const GmkNSplitLayout L = gmkn_split_layout(nres, n_board);
  std::vector<float> f32((size_t)F.total);
  gmkn_net_pack(nres, n_board, raw, f32.data());
  memset(out, 0, sizeof(float) * (size_t)L.total);
  auto copy = [&](int dst, int src, int nf) { memcpy(out + dst, f32.data() + src, sizeof(float) * (size_t)nf); };
  copy(L.conv0, F.conv0, 2 * 9 * 64);
  copy(L.conv0_b, F.conv0_b, 32);
  copy(L.conv_b, F.conv_b, 4 * nres * 32);
  copy(L.head_b, F.head_b, 32);
  copy(L.fc1, F.fc1, 2 * 32 * 16 * cells);
  copy(L.tail_v, F.tail_v, kGmkNTv2b + 1);
  copy(L.tail_p, F.tail_p, gmkn_tp2b(cells) + cells);
  int e[32];
  const float *p = raw + 32 * 27 + 32;
  for (int l = 0; l < 4 * nres; ++l) {  // W [32 out][32 in][9], bias [32]
    double wb = 0.0;
    for (int co = 0; co < 32; ++co) {
      double l1;
      e[co] = bx_row_exp(p + co * 288, 288, &l1, kGnsWExp);
      out[L.conv_inv + l * 32 + co] = bx_pow2(-e[co]);
      wb = l1 > wb ? l1 : wb;
    }
    out[L.conv_bd + 4 * l] = bx_round_up(wb);
    out[L.conv_bd + 4 * l + 1] = bx_bias_bound(p + 32 * 288, 32);
    uint16_t *frag = reinterpret_cast<uint16_t *>(out + L.conv + (size_t)l * kGnsFrag3);
    for (int tap = 0; tap < 9; ++tap)
      gmkn_split_chunk([&](int co, int ci) { return p[(co * 32 + ci) * 9 + tap]; }, e, frag + tap * (kGnsFrag1 * 2));
    p += 32 * 288 + 32;
  }
  for (int co = 0; co < 32; ++co) {  // the heads: W [32 out][32 in]
    double l1;
    e[co] = bx_row_exp(p + co * 32, 32, &l1, kGnsWExp);
    out[L.head_inv + co] = bx_pow2(-e[co]);
  }
  gmkn_split_chunk([&](int co, int ci) { return p[co * 32 + ci]; }, e, reinterpret_cast<uint16_t *>(out + L.head));
}

// launcher (lzm_az_gomoku_n_split.hip); n_board 9 or 15, nres 1 or 2 (checked by the caller)
hipError_t gmkn_launch_net_split_eval(int n_board, int nres, const float *w, const float *state, int n, float *probs,
                                      float *value, int32_t *err, hipStream_t s);

}  // namespace lzm
