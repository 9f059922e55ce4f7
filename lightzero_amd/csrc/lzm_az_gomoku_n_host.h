// lzm_az_gomoku_n_host.h — what the Gomoku 9 x 9 / 15 x 15 AlphaZero kernels (lzm_az_gomoku_n.h,
// lzm_az_gomoku_n_net.h) share with the entry points in lzm_kernels.hip: the board geometry, the workspace and
// weight-buffer layouts, the host-side weight packer and the launchers. The kernels are their own translation unit
// (lzm_az_gomoku_n.hip), built as lzm_az_gomoku.hip is. The 6 x 6 family (lzm_az_gomoku_host.h) is untouched.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace lzm {

inline bool gmkn_size_ok(int n_board) { return n_board == 9 || n_board == 15; }

// one wave per board; lane l owns the cpl consecutive cells cpl l .. cpl l + cpl - 1 (2 at 9 x 9, 4 at 15 x 15).
// A stone mask is `words` 64-bit words, bit rs row + column with rs = N + 1: the bit after a row's last cell is
// always clear, so shifts by 1, rs - 1, rs and rs + 1 never wrap (90 bits at 9 x 9, 240 at 15 x 15).
template <int N>
struct GmkNGeo {
  static constexpr int cells = N * N;
  static constexpr int cpl = (cells + 63) / 64;
  static constexpr int rs = N + 1;
  static constexpr int words = (N * rs + 63) / 64;
};
constexpr int kGmkNWords = 4;  // words a mask takes in the workspace, whatever the size

__host__ __device__ inline int gmkn_path_len(int cells, int S) { return (cells < S + 1 ? cells : S + 1) + 1; }

struct GmkNTree {
  int B, S, cap, path_len;
  int4 *rec;             // [B][cap] {first child (-1: leaf), visit, value_sum bits, prior bits}
  int32_t *nnodes;       // [B]
  uint64_t *root;        // [B][2][kGmkNWords] the root's stones of player 1 / 2
  int32_t *root_player;  // [B] player to move at the root (1 / 2)
  int32_t *path;         // [B][path_len] node indices of the current descent: root + min(N^2, S + 1) moves
  int32_t *leaf;         // [B][4] depth, done, winner, player to move at the leaf
  uint64_t *leaf_bb;     // [B][2][kGmkNWords]
  double *lut_pb;        // [S + 1] log((n + base + 1) / base) + init   (glibc, host-built)
  double *lut_sqrt;      // [S + 1] sqrt(n)
  double *noise;         // [N^2][N^2] row n-1: the reference's default-seeded Dirichlet vector for n children
};

struct GmkNStepArgs {
  int sim;              // -1: expand the roots; k >= 0: finish simulation k
  int with_noise;
  double noise_weight;
  const float *probs;   // [B][pstride]
  int pstride;
  const float *values;  // [B] (element stride vstride)
  int vstride;
  float *state;         // [B][3][N][N] network input of the next positions to evaluate
};

// ---- the network (lzm_az_gomoku_n_net.h)
// head tails: FC1 bias [32], LayerNorm gamma [32], beta [32], FC2 (value [32], b @128 | policy [N^2][32], b [N^2])
constexpr int kGmkNT1b = 0, kGmkNTg = 32, kGmkNTb = 64, kGmkNT2 = 96, kGmkNTv2b = 128;
__host__ __device__ constexpr int gmkn_tp2b(int cells) { return 96 + cells * 32; }

// prepared weight buffer (float offsets, every block 16-byte aligned), see gmkn_net_pack. Wave w of the network
// kernel is (N tile nt = w & 1: out channels 16 nt .., row-tile parity w >> 1).
struct GmkNNetLayout {
  int conv0, conv0_b;  // frag [nt 2][tap 9][lane 64] (K step = the 3 in channels of a tap + a zero), bias [32]
  int conv, conv_b;    // frag [layer][nt 2][i 18][lane 64][e 4]: K step s = 4 i + e = 8 tap + j, in channel
                       // 4 j + lane / 16; bias [layers][32]
  int head, head_b;    // frag [nt 2][k 8][lane 64] (value rows 0..15, policy rows 16..31), bias [32]
  int fc1;             // [head 2][i N^2][half 2][lane 64][e 4]: unit 16 half + lane / 4, quarter lane & 3, input
                       // 4 N^2 quarter + 4 i + e
  int tail_v, tail_p;
  int total;
};

__host__ __device__ inline GmkNNetLayout gmkn_net_layout(int nres, int n_board) {
  const int cells = n_board * n_board;
  GmkNNetLayout L;
  int o = 0;
  auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
  L.conv0 = take(2 * 9 * 64); L.conv0_b = take(32);
  L.conv = take(4 * nres * 2 * 18 * 256); L.conv_b = take(4 * nres * 32);
  L.head = take(2 * 8 * 64); L.head_b = take(32);
  L.fc1 = take(2 * 32 * 16 * cells);
  L.tail_v = take(kGmkNTv2b + 1); L.tail_p = take(gmkn_tp2b(cells) + cells);
  L.total = o;
  return L;
}

// raw (BatchNorm folded; include/lzmcts.h states the order) -> the kernel's order: a permutation plus zero padding.
// B fragment of v_mfma_f32_16x16x4_f32: lane holds B[k = lane / 16][n = lane % 16].
inline void gmkn_net_pack(int nres, int n_board, const float *raw, float *out) {
  const int cells = n_board * n_board, flat = 16 * cells;
  const GmkNNetLayout L = gmkn_net_layout(nres, n_board);
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
    for (int nt = 0; nt < 2; ++nt)
      for (int s = 0; s < 72; ++s)
        for (int lane = 0; lane < 64; ++lane)
          out[L.conv + (size_t)(((l * 2 + nt) * 18 + (s >> 2)) * 64 + lane) * 4 + (s & 3)] =
              wl[(16 * nt + (lane & 15)) * 288 + (4 * (s & 7) + (lane >> 4)) * 9 + (s >> 3)];
    memcpy(out + L.conv_b + l * 32, p, 32 * sizeof(float)); p += 32;
  }
  const float *wh = p; p += 32 * 32;
  for (int nt = 0; nt < 2; ++nt)
    for (int k = 0; k < 8; ++k)
      for (int lane = 0; lane < 64; ++lane)
        out[L.head + (nt * 8 + k) * 64 + lane] = wh[(16 * nt + (lane & 15)) * 32 + 4 * k + (lane >> 4)];
  memcpy(out + L.head_b, p, 32 * sizeof(float)); p += 32;
  for (int head = 0; head < 2; ++head) {
    const float *f1 = p; p += 32 * flat;
    for (int i = 0; i < cells; ++i)
      for (int half = 0; half < 2; ++half)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 4; ++e)
            out[L.fc1 + ((((size_t)head * cells + i) * 2 + half) * 64 + lane) * 4 + e] =
                f1[(size_t)(16 * half + (lane >> 2)) * flat + (lane & 3) * 4 * cells + 4 * i + e];
    const int tail = head ? gmkn_tp2b(cells) + cells : kGmkNTv2b + 1;  // FC1 bias, gamma, beta, FC2, FC2 bias: raw order
    memcpy(out + (head ? L.tail_p : L.tail_v), p, tail * sizeof(float)); p += tail;
  }
}

// launchers (lzm_az_gomoku_n.hip); n_board is 9 or 15 (checked by the callers); each returns the launch's status
hipError_t gmkn_launch_begin(int n_board, const GmkNTree &t, const int32_t *boards, const int32_t *start_index,
                             float *state, hipStream_t s);
hipError_t gmkn_launch_step(int n_board, const GmkNTree &t, const GmkNStepArgs &a, hipStream_t s);
hipError_t gmkn_launch_finish(int n_board, const GmkNTree &t, double temperature, int sample, uint32_t seed,
                              const int64_t *counter, int32_t *visits, double *probs, int32_t *action, hipStream_t s);
hipError_t gmkn_launch_export(const GmkNTree &t, int32_t *visit, float *vsum, int32_t *first, float *prior,
                              int32_t *nnodes, hipStream_t s);
hipError_t gmkn_launch_done_winner(int n_board, const int32_t *boards, int n, int32_t *out, hipStream_t s);
// one position per workgroup at both sizes (two per workgroup measured slower at 9 x 9 for
// every n, and do not fit LDS at 15 x 15)
hipError_t gmkn_launch_net_eval(int n_board, int nres, const float *w, const float *state, int n, float *probs,
                                float *value, hipStream_t s);

}  // namespace lzm
