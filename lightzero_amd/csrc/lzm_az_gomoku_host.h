// lzm_az_gomoku_host.h — what the Gomoku AlphaZero kernels (lzm_az_gomoku.h, lzm_az_gomoku_net.h) share with the
// entry points in lzm_kernels.hip: the workspace and weight-buffer layouts, the host-side weight packer and the
// launchers. The kernels are their own translation unit (lzm_az_gomoku.hip), built as lzm_az_c4.hip is.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace lzm {

constexpr int kGmkN = 6;       // board size
constexpr int kGmkCells = 36;  // cells = actions
constexpr int kGmkPath = 37;   // root + at most 36 moves

struct GmkTree {
  int B, S, cap;
  int4 *rec;             // [B][cap] {first child (-1: leaf), visit, value_sum bits, prior bits}
  int32_t *nnodes;       // [B]
  uint64_t *root;        // [B][2] the root's stones of player 1 / 2 (bit 7 row + column)
  int32_t *root_player;  // [B] player to move at the root (1 / 2)
  int32_t *path;         // [B][kGmkPath] node indices of the current descent
  int32_t *leaf;         // [B][4] depth, done, winner, player to move at the leaf
  uint64_t *leaf_bb;     // [B][2]
  double *lut_pb;        // [S + 1] log((n + base + 1) / base) + init   (glibc, host-built)
  double *lut_sqrt;      // [S + 1] sqrt(n)
  double *noise;         // [36][36] row n-1: the reference's default-seeded Dirichlet vector for n children
};

struct GmkStepArgs {
  int sim;              // -1: expand the roots; k >= 0: finish simulation k
  int with_noise;
  double noise_weight;
  const float *probs;   // [B][pstride]
  int pstride;
  const float *values;  // [B] (element stride vstride)
  int vstride;
  float *state;         // [B][3][6][6] network input of the next positions to evaluate
};

// ---- the network (lzm_az_gomoku_net.h)
constexpr int kGmkC = 32;          // channels
constexpr int kGmkFc = 32;         // head hidden width
constexpr int kGmkFlat = 16 * 36;  // 576 inputs of a head's FC1
// positions per workgroup from n: 1 below this, 2 from there (measured)
constexpr int kGmkNetP2From = 513;
// head tails: FC1 bias [32], LayerNorm gamma [32], beta [32], FC2 (value [32], b @128 | policy [36][32], b [36] @1248)
constexpr int kGmkT1b = 0, kGmkTg = 32, kGmkTb = 64, kGmkT2 = 96, kGmkTv2b = 128, kGmkTp2b = 96 + 36 * 32;

// prepared weight buffer (float offsets, every block 16-byte aligned), see gmk_net_pack. Wave w of the network
// kernel is (N tile nt = w & 1: out channels 16 nt .., K half kh = w >> 1: in channels 16 kh ..).
struct GmkNetLayout {
  int conv0, conv0_b;  // frag [nt 2][tap 9][lane 64] (K step = the 3 in channels of a tap + a zero), bias [32]
  int conv, conv_b;    // frag [layer][wave 4][tap 9][lane 64][j 4] (in channel 16 kh + 4 j + lane / 16), bias [layers][32]
  int head, head_b;    // frag [nt 2][k 8][lane 64] (value rows 0..15, policy rows 16..31), bias [32]
  int fc1;             // [head 2][pass 2][i 36][lane 64][4]: lane = 2 unit + half, inputs 144 (2 pass + half) + 4 i ..
  int tail_v, tail_p;
  int total;
};

__host__ __device__ inline GmkNetLayout gmk_net_layout(int nres) {
  GmkNetLayout L;
  int o = 0;
  auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
  L.conv0 = take(2 * 9 * 64); L.conv0_b = take(32);
  L.conv = take(4 * nres * 4 * 9 * 256); L.conv_b = take(4 * nres * 32);
  L.head = take(2 * 8 * 64); L.head_b = take(32);
  L.fc1 = take(2 * 2 * 36 * 64 * 4);
  L.tail_v = take(kGmkTv2b + 1); L.tail_p = take(kGmkTp2b + 36);
  L.total = o;
  return L;
}

// raw (BatchNorm folded; include/lzmcts.h states the order) -> the kernel's order: a permutation plus zero padding.
// B fragment of v_mfma_f32_16x16x4_f32: lane holds B[k = lane / 16][n = lane % 16].
inline void gmk_net_pack(int nres, const float *raw, float *out) {
  const GmkNetLayout L = gmk_net_layout(nres);
  memset(out, 0, sizeof(float) * (size_t)L.total);
  const float *p = raw;
  const float *w0 = p; p += 32 * 27;
  for (int nt = 0; nt < 2; ++nt)
    for (int tap = 0; tap < 9; ++tap)
      for (int lane = 0; lane < 64; ++lane) {
        const int cin = lane >> 4;
        if (cin < 3) out[L.conv0 + (nt * 9 + tap) * 64 + lane] = w0[(16 * nt + (lane & 15)) * 27 + cin * 9 + tap];
      }
  memcpy(out + L.conv0_b, p, 32 * sizeof(float)); p += 32;
  for (int l = 0; l < 4 * nres; ++l) {
    const float *wl = p; p += 32 * 288;
    for (int wv = 0; wv < 4; ++wv)
      for (int tap = 0; tap < 9; ++tap)
        for (int lane = 0; lane < 64; ++lane)
          for (int j = 0; j < 4; ++j)
            out[L.conv + (size_t)(((l * 4 + wv) * 9 + tap) * 64 + lane) * 4 + j] =
                wl[(16 * (wv & 1) + (lane & 15)) * 288 + (16 * (wv >> 1) + 4 * j + (lane >> 4)) * 9 + tap];
    memcpy(out + L.conv_b + l * 32, p, 32 * sizeof(float)); p += 32;
  }
  const float *wh = p; p += 32 * 32;
  for (int nt = 0; nt < 2; ++nt)
    for (int k = 0; k < 8; ++k)
      for (int lane = 0; lane < 64; ++lane)
        out[L.head + (nt * 8 + k) * 64 + lane] = wh[(16 * nt + (lane & 15)) * 32 + 4 * k + (lane >> 4)];
  memcpy(out + L.head_b, p, 32 * sizeof(float)); p += 32;
  for (int head = 0; head < 2; ++head) {
    const float *f1 = p; p += 32 * kGmkFlat;
    for (int s = 0; s < 2; ++s)
      for (int i = 0; i < 36; ++i)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 4; ++e)
            out[L.fc1 + (((head * 2 + s) * 36 + i) * 64 + lane) * 4 + e] =
                f1[(lane >> 1) * kGmkFlat + 144 * (2 * s + (lane & 1)) + 4 * i + e];
    const int tail = head ? kGmkTp2b + 36 : kGmkTv2b + 1;  // FC1 bias, gamma, beta, FC2, FC2 bias: raw order
    memcpy(out + (head ? L.tail_p : L.tail_v), p, tail * sizeof(float)); p += tail;
  }
}

// launchers (lzm_az_gomoku.hip); each returns the launch's status
hipError_t gmk_launch_begin(const GmkTree &t, const int32_t *boards, const int32_t *start_index, float *state,
                            hipStream_t s);
hipError_t gmk_launch_step(const GmkTree &t, const GmkStepArgs &a, hipStream_t s);
hipError_t gmk_launch_finish(const GmkTree &t, double temperature, int sample, uint32_t seed, const int64_t *counter,
                             int32_t *visits, double *probs, int32_t *action, hipStream_t s);
hipError_t gmk_launch_export(const GmkTree &t, int32_t *visit, float *vsum, int32_t *first, float *prior,
                             int32_t *nnodes, hipStream_t s);
hipError_t gmk_launch_done_winner(const int32_t *boards, int n, int32_t *out, hipStream_t s);
// positions: positions per workgroup, 1 or 2 (0: chosen from n)
hipError_t gmk_launch_net_eval(int nres, int positions, const float *w, const float *state, int n, float *probs,
                               float *value, hipStream_t s);

}  // namespace lzm
