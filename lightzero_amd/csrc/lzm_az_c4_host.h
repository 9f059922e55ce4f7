// lzm_az_c4_host.h — what the Connect4 AlphaZero kernels (lzm_az_c4.h, lzm_az_c4_net.h) share with the entry
// points in lzm_kernels.hip: the workspace and weight-buffer layouts and the launchers. The kernels are their own
// translation unit (lzm_az_c4.hip); lightzero_amd/build.py says why and how it is built.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lzm {

constexpr int kC4Cols = 7;
constexpr int kC4Rows = 6;
constexpr int kC4Cells = 42;
constexpr int kC4Path = 43;  // root + at most 42 moves

struct C4Tree {
  int B, S, cap;
  int4 *rec;             // [B][cap] {first child (-1: leaf), visit, value_sum bits, prior bits}
  int32_t *nnodes;       // [B]
  uint64_t *root;        // [B][2] the root's stones of player 1 / 2 (bit 7 column + height)
  int32_t *root_player;  // [B] player to move at the root (1 / 2)
  int32_t *path;         // [B][kC4Path] node indices of the current descent
  int32_t *leaf;         // [B][4] depth, done, winner, player to move at the leaf
  uint64_t *leaf_bb;     // [B][2]
  double *lut_pb;        // [S + 1] log((n + base + 1) / base) + init   (glibc, host-built)
  double *lut_sqrt;      // [S + 1] sqrt(n)
  double *noise;         // [7][7] row n-1: the reference's default-seeded Dirichlet vector for n children
};

struct C4StepArgs {
  int sim;              // -1: expand the roots; k >= 0: finish simulation k
  int with_noise;
  double noise_weight;
  const float *probs;   // [B][pstride]
  int pstride;
  const float *values;  // [B] (element stride vstride)
  int vstride;
  float *state;         // [B][3][6][7] network input of the next positions to evaluate
};

// head tails: FC1 bias [32], LayerNorm gamma [32], beta [32], FC2 (value [32], b @128 | policy [7][32], b [7] @320)
constexpr int kC4nT1b = 0, kC4nTg = 32, kC4nTb = 64, kC4nT2 = 96, kC4nTv2b = 128, kC4nTp2b = 320;

// prepared weight buffer (float offsets, every block 16-byte aligned), see lzm_az_c4_net_prepare
struct C4NetLayout {
  int conv0, conv0_b;  // frag [wave 4][tap 9][lane 64] (K step = the 3 in channels of a tap + a zero), bias [64]
  int conv, conv_b;    // frag [layer * 9 + tap][wave 4][4][lane 64][4], bias [layers][64]
  int head, head_b;    // frag [N tile 2][16][lane 64], bias [32]
  int fc1;             // [head 2][84][lane 64][4]: lane = 2 unit + half, inputs 336 half + 4 i ..
  int tail_v, tail_p;
  int total;
};

__host__ __device__ inline C4NetLayout c4_net_layout(int nres) {
  C4NetLayout L;
  int o = 0;
  auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
  L.conv0 = take(4 * 9 * 64); L.conv0_b = take(64);
  L.conv = take(4 * nres * 9 * 4096); L.conv_b = take(4 * nres * 64);
  L.head = take(2 * 16 * 64); L.head_b = take(32);
  L.fc1 = take(2 * 84 * 64 * 4);
  L.tail_v = take(kC4nTv2b + 1); L.tail_p = take(kC4nTp2b + 7);
  L.total = o;
  return L;
}

// prepared weight buffer of the split-fp16 network (lzm_az_c4_net_split.h, lzm_az_c4_net_split_prepare): conv0,
// fc1 and the tails as above; the 64 -> 64 layers and the 1x1 heads as lzm_conv.h's split fragments
constexpr int kC4sFrag3 = 4 * 18 * 2 * 64 * 4;  // floats: [wave 4][chunk 18][term 2][lane 64][8 fp16]
constexpr int kC4sFrag1 = 2 * 2 * 2 * 64 * 4;   // floats: [N tile 2][chunk 2][term 2][lane 64][8 fp16]
constexpr int kC4sWExp = 48;                    // weight-row scale exponents within +-48 (lzm_az_c4_net_split.h)
constexpr int kC4sBoards = 2;                   // positions per workgroup by default
struct C4SplitLayout {
  int conv0, conv0_b;
  int conv;               // [layer] kC4sFrag3
  int conv_b, conv_inv;   // bias [layers][64], 2^-e_c [layers][64]
  int conv_bd;            // [layers] {Wb = max row L1 norm, Bb = max |bias|, 0, 0}
  int head, head_b, head_inv;  // kC4sFrag1, bias [32], 2^-e_c [32]
  int fc1, tail_v, tail_p;
  int total;
};

__host__ __device__ inline C4SplitLayout c4_split_layout(int nres) {
  C4SplitLayout L;
  int o = 0;
  auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
  L.conv0 = take(4 * 9 * 64); L.conv0_b = take(64);
  L.conv = take(4 * nres * kC4sFrag3);
  L.conv_b = take(4 * nres * 64); L.conv_inv = take(4 * nres * 64); L.conv_bd = take(4 * nres * 4);
  L.head = take(kC4sFrag1); L.head_b = take(32); L.head_inv = take(32);
  L.fc1 = take(2 * 84 * 64 * 4);
  L.tail_v = take(kC4nTv2b + 1); L.tail_p = take(kC4nTp2b + 7);
  L.total = o;
  return L;
}

// launchers (lzm_az_c4.hip); each returns the launch's status
hipError_t c4_launch_begin(const C4Tree &t, const int32_t *boards, const int32_t *start_index, float *state,
                           hipStream_t s);
hipError_t c4_launch_step(const C4Tree &t, const C4StepArgs &a, hipStream_t s);
hipError_t c4_launch_finish(const C4Tree &t, double temperature, int sample, uint32_t seed, const int64_t *counter,
                            int32_t *visits, double *probs, int32_t *action, hipStream_t s);
hipError_t c4_launch_export(const C4Tree &t, int32_t *visit, float *vsum, int32_t *first, float *prior,
                            int32_t *nnodes, hipStream_t s);
hipError_t c4_launch_done_winner(const int32_t *boards, int n, int32_t *out, hipStream_t s);
hipError_t c4_launch_net_eval(int nres, const float *w, const float *state, int n, float *probs, float *value,
                              hipStream_t s);
// boards: positions per workgroup, 2 or 4 (0: the default)
hipError_t c4_launch_net_split_eval(int nres, int boards, const float *w, const float *state, int n, float *probs,
                                    float *value, int32_t *err, hipStream_t s);

}  // namespace lzm
