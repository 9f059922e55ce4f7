// lzm_az_gomoku.h — batched AlphaZero tree search for Gomoku 6 x 6 on the device (the game of
// zoo/board_games/gomoku/envs/gomoku_env.py and get_done_winner_cython.pyx, the tree of mcts_alphazero.cpp as
// oracle/az_oracle.py restates it).
//
// Same per-simulation protocol as lzm_az_c4.h (begin, step(-1), S x step(k), finish): one launch finishes the
// previous simulation (expand the leaf with the network's priors or score the terminal position, back up with
// alternating signs), runs the next descent and writes the leaf's network input [3][6][6].
//
// Mapping: one wave per board, lane = cell (lanes 36..63 carry no cell). The position is two 41-bit masks
// (player 1's and player 2's stones; bit 7 row + column, so column 6 of every row is always clear and shifts by 1,
// 6, 7 and 8 never wrap), uniform over the wave. There is no gravity: action a is cell a, legal iff empty. A run
// of five starting at a cell (the lowest bit of the run, which is the cell the reference's row-major scan meets
// first) is m & m >> s & m >> 2 s & m >> 3 s & m >> 4 s for s = 6 (1, -1), 7 (1, 0), 8 (1, 1), 1 (0, 1); the
// winner is the player whose start-cell mask has the lower lowest bit, so a board where both players have five
// reports what the cell-major scan reports.
//
// A node is one 16-byte record {first child (-1: leaf), visit int, value_sum float, prior float}; a row of
// cap = 1 + 36 (S + 1) records per board, a node's children contiguous in action order. Child j of a node is the
// j-th empty cell of the node's position: lane a reads child first + popcount(empty & ((1 << a) - 1)), the wave
// arg-max (first maximum in action order: lowest lane among equal scores) picks one, and its {first, visit} go to
// every lane by a lane read. The backup is one lane per path node (depth <= 36).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_az_gomoku_host.h"
#include "lzm_numerics.h"

namespace lzm {

constexpr int kGmkThreads = 64;  // one board per workgroup

__host__ __device__ constexpr uint64_t gmk_full_mask() {
  uint64_t m = 0;
  for (int r = 0; r < kGmkN; ++r) m |= 0x3full << (7 * r);
  return m;
}

__device__ inline int gmk_bit(int cell) { return 7 * (cell / kGmkN) + cell % kGmkN; }

// the start cells of the player's runs of five (six in a row has two)
__device__ inline uint64_t gmk_fives(uint64_t m) {
  constexpr int kShift[4] = {6, 7, 8, 1};
  uint64_t u = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = kShift[i];
    u |= m & (m >> s) & (m >> (2 * s)) & (m >> (3 * s)) & (m >> (4 * s));
  }
  return u;
}

// get_done_winner: the owner of the first start cell in row-major order, else a full board is a draw
__device__ inline void gmk_done_winner(uint64_t m1, uint64_t m2, int &done, int &winner) {
  const uint64_t f1 = gmk_fives(m1), f2 = gmk_fives(m2);
  // (x & -x) isolates the lowest bit; an empty mask compares as the largest value
  const uint64_t l1 = (f1 & (0 - f1)) - 1, l2 = (f2 & (0 - f2)) - 1;
  winner = (f1 | f2) == 0 ? -1 : (l1 < l2 ? 1 : 2);
  done = (f1 | f2) != 0 || (m1 | m2) == gmk_full_mask();
}

// 36 cell flags (a ballot over the wave's lanes) -> bit 7 row + column
__device__ inline uint64_t gmk_spread(uint64_t cells) {
  uint64_t m = 0;
#pragma unroll
  for (int r = 0; r < kGmkN; ++r) m |= ((cells >> (kGmkN * r)) & 0x3full) << (7 * r);
  return m;
}

__device__ inline void gmk_load_board(const int32_t *bd, int l, uint64_t &m1, uint64_t &m2) {
  const int v = l < kGmkCells ? bd[l] : 0;
  m1 = gmk_spread(__ballot(v == 1));
  m2 = gmk_spread(__ballot(v == 2));
}

// the empty cells as lane flags (bit a: cell a is empty)
__device__ inline uint64_t gmk_empty(uint64_t occ, int l) {
  return __ballot(l < kGmkCells && !((occ >> gmk_bit(l < kGmkCells ? l : 0)) & 1));
}

// current_state()[1] with scale=True: the stones of the player to move, the stones of `to_play` (the other
// player), 0.5 * the player to move
__device__ inline void gmk_write_state(float *st, int l, uint64_t m1, uint64_t m2, int player) {
  if (l >= kGmkCells) return;
  const uint64_t mine = player == 1 ? m1 : m2, theirs = player == 1 ? m2 : m1;
  const int bit = gmk_bit(l);
  st[l] = ((mine >> bit) & 1) ? 0.5f : 0.0f;
  st[kGmkCells + l] = ((theirs >> bit) & 1) ? 0.5f : 0.0f;
  st[2 * kGmkCells + l] = 0.5f * (float)player;
}

// _expand_leaf_node: one child per empty cell in action order, prior = float(probs[a]); at the root, when
// sampling, _add_exploration_noise: float(double(prior) * (1 - w) + noise[i] * w)
__device__ inline void gmk_expand(const GmkTree &t, size_t nb, int b, int node, int base, int l, uint64_t occ,
                                  float pr, bool noise, double w) {
  const uint64_t em = gmk_empty(occ, l);
  const int n = __popcll(em), rank = __popcll(em & ((1ull << l) - 1ull));
  if ((em >> l) & 1) {
    float p = pr;
    if (noise) p = (float)((double)pr * (1.0 - w) + t.noise[(n - 1) * kGmkCells + rank] * w);
    t.rec[nb + base + rank] = make_int4(-1, 0, __float_as_int(0.0f), __float_as_int(p));
  }
  if (l == 0) {
    t.rec[nb + node].x = n > 0 ? base : -1;
    t.nnodes[b] = base + n;
  }
}

__global__ void __launch_bounds__(kGmkThreads) gmk_begin_kernel(GmkTree t, const int32_t *boards,
                                                                const int32_t *start_index, float *state) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= t.B) return;
  const int player = start_index[b] == 0 ? 1 : 2;
  uint64_t m1, m2;
  gmk_load_board(boards + (size_t)b * kGmkCells, l, m1, m2);
  if (l == 0) {
    t.root[2 * b] = m1;
    t.root[2 * b + 1] = m2;
    t.root_player[b] = player;
  }
  gmk_write_state(state + (size_t)b * 3 * kGmkCells, l, m1, m2, player);
}

__global__ void __launch_bounds__(kGmkThreads) gmk_step_kernel(GmkTree t, GmkStepArgs a) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= t.B) return;
  const size_t nb = (size_t)b * t.cap;
  int32_t *path = t.path + (size_t)b * kGmkPath;
  const float pr = l < kGmkCells ? a.probs[(size_t)b * a.pstride + l] : 0.0f;
  const uint64_t r1 = t.root[2 * b], r2 = t.root[2 * b + 1];
  if (a.sim < 0) {
    // a fresh root (Node()), expanded with the root evaluation; noise only when sampling
    if (l == 0) t.rec[nb] = make_int4(-1, 0, __float_as_int(0.0f), __float_as_int(1.0f));
    gmk_expand(t, nb, b, 0, 1, l, r1 | r2, pr, a.with_noise != 0, a.noise_weight);
  } else {
    const int depth = t.leaf[b * 4 + 0], done = t.leaf[b * 4 + 1], winner = t.leaf[b * 4 + 2],
              player = t.leaf[b * 4 + 3];
    double lv;
    if (!done) {
      gmk_expand(t, nb, b, path[depth], t.nnodes[b], l, t.leaf_bb[2 * b] | t.leaf_bb[2 * b + 1], pr, false, 0.0);
      lv = (double)a.values[(size_t)b * a.vstride];
    } else {
      lv = winner == -1 ? 0.0 : (player == winner ? 1.0 : -1.0);
    }
    // node->update_recursive(-leaf_value): + v at the leaf, - v at its parent, ...; lane k takes the k-th node up
    const float v = (float)(-lv);
    if (l <= depth) {
      int4 *n = t.rec + nb + path[depth - l];
      n->y += 1;
      n->z = __float_as_int(__int_as_float(n->z) + ((l & 1) ? -v : v));
    }
  }
  if (a.sim + 1 >= t.S) return;
  __threadfence_block();  // the descent reads what this wave just wrote

  // ---- _simulate: descend by the maximal pUCT child while the node has children
  uint64_t m1 = r1, m2 = r2;
  int player = t.root_player[b], d = 0;
  int first = t.rec[nb].x, pv = t.rec[nb].y;  // of the node the walk stands on
  if (l == 0) path[0] = 0;
  while (d < kGmkPath - 1 && first >= 0) {  // a board fills after 36 moves: bounded descent
    const uint64_t em = gmk_empty(m1 | m2, l);
    const bool mine = (em >> l) & 1;
    const int rank = __popcll(em & ((1ull << l) - 1ull));
    const int4 ch = t.rec[nb + first + (mine ? rank : 0)];
    double s = -__builtin_inf();
    if (mine) {
      const int cv = ch.y;
      const float val = cv == 0 ? 0.0f : __int_as_float(ch.z) / (float)cv;
      double pb = t.lut_pb[pv];
      pb *= t.lut_sqrt[pv] / (double)(cv + 1);
      s = pb * (double)__int_as_float(ch.w) + (double)val;
    }
    int bi = l;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double os = __shfl_xor(s, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (os > s || (os == s && oi < bi)) {
        s = os;
        bi = oi;
      }
    }
    const int node = first + __popcll(em & ((1ull << bi) - 1ull));
    first = __shfl(ch.x, bi, 64);
    pv = __shfl(ch.y, bi, 64);
    const uint64_t bit = 1ull << gmk_bit(bi);
    if (player == 1) m1 |= bit; else m2 |= bit;
    player = 3 - player;
    ++d;
    if (l == 0) path[d] = node;
  }
  int done, winner;
  gmk_done_winner(m1, m2, done, winner);
  if (l == 0) {
    t.leaf[b * 4 + 0] = d;
    t.leaf[b * 4 + 1] = done;
    t.leaf[b * 4 + 2] = winner;
    t.leaf[b * 4 + 3] = player;
    t.leaf_bb[2 * b] = m1;
    t.leaf_bb[2 * b + 1] = m2;
  }
  gmk_write_state(a.state + (size_t)b * 3 * kGmkCells, l, m1, m2, player);
}

// get_next_action's tail (as lzm_az_c4.h's, over 36 actions), one wave per board with lane = action: v / T summed
// in action order by every lane, divided; the first maximum, or a Philox draw keyed by seed, *counter and the board
__global__ void __launch_bounds__(kGmkThreads) gmk_finish_kernel(GmkTree t, double temperature, int sample,
                                                                 uint32_t seed, const int64_t *counter,
                                                                 int32_t *visits_out, double *probs_out,
                                                                 int32_t *action_out) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= t.B) return;
  const size_t nb = (size_t)b * t.cap;
  const uint64_t em = gmk_empty(t.root[2 * b] | t.root[2 * b + 1], l);
  const int f = t.rec[nb].x;
  const bool mine = f >= 0 && ((em >> l) & 1);
  const int v = mine ? t.rec[nb + f + __popcll(em & ((1ull << l) - 1ull))].y : 0;
  double x = (double)v / temperature, sum = 0.0;
  for (int k = 0; k < kGmkCells; ++k) sum += __shfl(x, k, 64);
  x = x / sum;
  if (l < kGmkCells) {
    visits_out[(size_t)b * kGmkCells + l] = v;
    probs_out[(size_t)b * kGmkCells + l] = x;
  }
  int best = 0;
  if (!sample) {
    double bx = __shfl(x, 0, 64);
    for (int k = 1; k < kGmkCells; ++k) {
      const double xk = __shfl(x, k, 64);
      if (xk > bx) {
        bx = xk;
        best = k;
      }
    }
  } else {
    const uint64_t step = counter ? (uint64_t)*counter : 0;
    const uint4 r = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)step, (uint32_t)(step >> 32), 0x4334u),
                                  make_uint2(seed, 0x414c5048u));
    const double u = ((double)(((uint64_t)(r.x >> 5) << 26) | (r.y >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
    double cum = 0.0;
    int last = -1;
    best = -1;
    for (int k = 0; k < kGmkCells; ++k) {
      const double xk = __shfl(x, k, 64);
      cum += xk;
      if (xk > 0.0) last = k;
      if (best < 0 && xk > 0.0 && u < cum) best = k;
    }
    if (best < 0) best = last;
  }
  if (l == 0) action_out[b] = best;
}

// test access: the records as arrays [B][cap] (any may be null); rows past the board's node count read 0 / -1
__global__ void gmk_export_kernel(GmkTree t, int32_t *visit, float *vsum, int32_t *first, float *prior,
                                  int32_t *nnodes) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (size_t)t.B * t.cap) return;
  const int b = (int)(i / t.cap), k = (int)(i % t.cap);
  const bool live = k < t.nnodes[b];
  const int4 r = live ? t.rec[i] : make_int4(-1, 0, 0, 0);
  if (visit) visit[i] = r.y;
  if (vsum) vsum[i] = __int_as_float(r.z);
  if (first) first[i] = r.x;
  if (prior) prior[i] = __int_as_float(r.w);
  if (nnodes && k == 0) nnodes[b] = t.nnodes[b];
}

// test access: get_done_winner of n boards, out [n][2] = {done, winner}
__global__ void __launch_bounds__(kGmkThreads) gmk_done_winner_kernel(const int32_t *boards, int n, int32_t *out) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= n) return;
  uint64_t m1, m2;
  gmk_load_board(boards + (size_t)b * kGmkCells, l, m1, m2);
  int done, winner;
  gmk_done_winner(m1, m2, done, winner);
  if (l == 0) {
    out[2 * b] = done;
    out[2 * b + 1] = winner;
  }
}

}  // namespace lzm
