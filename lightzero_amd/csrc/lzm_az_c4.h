// lzm_az_c4.h — batched AlphaZero tree search for Connect4 on the device (the game of
// zoo/board_games/connect4/envs/connect4_env.py, the tree of mcts_alphazero.cpp as oracle/az_oracle.py restates it).
//
// Same per-simulation protocol as lzm_az.h (begin, step(-1), S x step(k), finish): one launch finishes the
// previous simulation (expand the leaf with the network's priors or score the terminal position, back up with
// alternating signs), runs the next descent and writes the leaf's network input [3][6][7].
//
// Mapping: an 8-lane group per board, lane = column. The position is two 49-bit masks (player 1's and player 2's
// stones; bit 7 c + h is column c, height h from the bottom, bit 7 c + 6 always clear), uniform over the group's
// registers: a move is the lowest clear bit of a column of (m1 | m2), four in a line is x = m & (m >> s),
// x & (x >> 2 s) for s = 1 (vertical), 7 (horizontal), 6 and 8 (diagonals), player 1 first: the reference scans
// piece-major, so this is its answer on every board, boards where both players have four included.
//
// A node is one 16-byte record {first child (-1: leaf), visit int, value_sum float, prior float}; a row of
// cap = 1 + 7 (S + 1) records per board, a node's children contiguous in action order. Child j of a node is the
// j-th legal column of the node's position, which the descent holds anyway, so the tree stores neither the
// action nor the child count. A level of the descent is one round of record reads: lane j < n reads child j, the
// group arg-max (first strict maximum in action order) picks one, and its {first, visit} go to every lane by a
// lane read — the next level's parent.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_az_c4_host.h"
#include "lzm_numerics.h"

namespace lzm {

constexpr int kC4Group = 8;
constexpr int kC4Threads = 64;  // 8 boards per workgroup

__host__ __device__ constexpr uint64_t c4_full_mask() {
  uint64_t m = 0;
  for (int c = 0; c < kC4Cols; ++c) m |= 0x3full << (7 * c);
  return m;
}

__device__ inline bool c4_four(uint64_t m) {
  constexpr int kShift[4] = {1, 7, 6, 8};
  bool f = false;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int s = kShift[i];
    const uint64_t x = m & (m >> s);
    f |= (x & (x >> (2 * s))) != 0;
  }
  return f;
}

// get_done_winner: player 1's lines, then player 2's, then the full board (a draw)
__device__ inline void c4_done_winner(uint64_t m1, uint64_t m2, int &done, int &winner) {
  const bool w1 = c4_four(m1), w2 = c4_four(m2);
  winner = w1 ? 1 : (w2 ? 2 : -1);
  done = w1 || w2 || (m1 | m2) == c4_full_mask();
}

__device__ inline uint32_t c4_group_mask(bool pred, int gbase) {
  return (uint32_t)((__ballot(pred) >> gbase) & 0xffull);
}

// action a is legal iff board[a] == 0: the column's top cell
__device__ inline bool c4_legal(uint64_t occ, int l) { return l < kC4Cols && !((occ >> (7 * l + 5)) & 1); }

// the group's masks from board int32 [42] (row-major 6 x 7, row 0 on top): lane = column, then an OR butterfly
__device__ inline void c4_load_board(const int32_t *bd, int l, uint64_t &m1, uint64_t &m2) {
  uint32_t c1 = 0, c2 = 0;  // the column's 6 cells, bit = height
  if (l < kC4Cols) {
#pragma unroll
    for (int r = 0; r < kC4Rows; ++r) {
      const int v = bd[r * kC4Cols + l];
      c1 |= (uint32_t)(v == 1) << (5 - r);
      c2 |= (uint32_t)(v == 2) << (5 - r);
    }
  }
  m1 = (uint64_t)c1 << (7 * l);
  m2 = (uint64_t)c2 << (7 * l);
#pragma unroll
  for (int d = 4; d >= 1; d >>= 1) {
    m1 |= (uint64_t)__shfl_xor((unsigned long long)m1, d, kC4Group);
    m2 |= (uint64_t)__shfl_xor((unsigned long long)m2, d, kC4Group);
  }
}

// current_state()[1] with scale=True for the player to move: the mover's stones, the opponent's, 0.5 * player
__device__ inline void c4_write_state(float *st, int l, uint64_t m1, uint64_t m2, int player) {
  if (l >= kC4Cols) return;
  const uint64_t mine = player == 1 ? m1 : m2, theirs = player == 1 ? m2 : m1;
#pragma unroll
  for (int r = 0; r < kC4Rows; ++r) {
    const int i = r * kC4Cols + l, bit = 7 * l + 5 - r;
    st[i] = ((mine >> bit) & 1) ? 0.5f : 0.0f;
    st[kC4Cells + i] = ((theirs >> bit) & 1) ? 0.5f : 0.0f;
    st[2 * kC4Cells + i] = 0.5f * (float)player;
  }
}

// _expand_leaf_node: one child per legal column in action order, prior = float(probs[a]); at the root, when
// sampling, _add_exploration_noise: float(double(prior) * (1 - w) + noise[i] * w)
__device__ inline void c4_expand(const C4Tree &t, size_t nb, int b, int node, int base, int l, int gbase, uint64_t occ,
                                 float pr, bool noise, double w) {
  const bool legal = c4_legal(occ, l);
  const uint32_t gm = c4_group_mask(legal, gbase);
  const int n = __popc(gm), rank = __popc(gm & ((1u << l) - 1u));
  if (legal) {
    float p = pr;
    if (noise) p = (float)((double)pr * (1.0 - w) + t.noise[(n - 1) * kC4Cols + rank] * w);
    t.rec[nb + base + rank] = make_int4(-1, 0, __float_as_int(0.0f), __float_as_int(p));
  }
  if (l == 0) {
    t.rec[nb + node].x = n > 0 ? base : -1;
    t.nnodes[b] = base + n;
  }
}

__global__ void __launch_bounds__(kC4Threads) c4_begin_kernel(C4Tree t, const int32_t *boards,
                                                              const int32_t *start_index, float *state) {
  const int b = blockIdx.x * (kC4Threads / kC4Group) + threadIdx.x / kC4Group;
  const int l = threadIdx.x & (kC4Group - 1);
  if (b >= t.B) return;  // group-uniform
  const int player = start_index[b] == 0 ? 1 : 2;
  uint64_t m1, m2;
  c4_load_board(boards + (size_t)b * kC4Cells, l, m1, m2);
  if (l == 0) {
    t.root[2 * b] = m1;
    t.root[2 * b + 1] = m2;
    t.root_player[b] = player;
  }
  c4_write_state(state + (size_t)b * 3 * kC4Cells, l, m1, m2, player);
}

__global__ void __launch_bounds__(kC4Threads) c4_step_kernel(C4Tree t, C4StepArgs a) {
  const int b = blockIdx.x * (kC4Threads / kC4Group) + threadIdx.x / kC4Group;
  const int l = threadIdx.x & (kC4Group - 1);
  const int gbase = (threadIdx.x & 63) & ~(kC4Group - 1);
  if (b >= t.B) return;  // group-uniform
  const size_t nb = (size_t)b * t.cap;
  int32_t *path = t.path + (size_t)b * kC4Path;
  const float pr = l < kC4Cols ? a.probs[(size_t)b * a.pstride + l] : 0.0f;
  const uint64_t r1 = t.root[2 * b], r2 = t.root[2 * b + 1];
  if (a.sim < 0) {
    // a fresh root (Node()), expanded with the root evaluation; noise only when sampling
    if (l == 0) t.rec[nb] = make_int4(-1, 0, __float_as_int(0.0f), __float_as_int(1.0f));
    c4_expand(t, nb, b, 0, 1, l, gbase, r1 | r2, pr, a.with_noise != 0, a.noise_weight);
  } else {
    const int depth = t.leaf[b * 4 + 0], done = t.leaf[b * 4 + 1], winner = t.leaf[b * 4 + 2],
              player = t.leaf[b * 4 + 3];
    double lv;
    if (!done) {
      c4_expand(t, nb, b, path[depth], t.nnodes[b], l, gbase, t.leaf_bb[2 * b] | t.leaf_bb[2 * b + 1], pr, false, 0.0);
      lv = (double)a.values[(size_t)b * a.vstride];
    } else {
      lv = winner == -1 ? 0.0 : (player == winner ? 1.0 : -1.0);
    }
    // node->update_recursive(-leaf_value): + v at the leaf, - v at its parent, ...; a path has up to 43 nodes
    const float v = (float)(-lv);
    for (int k = l; k <= depth; k += kC4Group) {
      int4 *n = t.rec + nb + path[depth - k];
      n->y += 1;
      n->z = __float_as_int(__int_as_float(n->z) + ((k & 1) ? -v : v));
    }
  }
  if (a.sim + 1 >= t.S) return;
  __threadfence_block();  // the descent reads what this group just wrote

  // ---- _simulate: descend by the maximal pUCT child while the node has children
  uint64_t m1 = r1, m2 = r2;
  int player = t.root_player[b], d = 0;
  int first = t.rec[nb].x, pv = t.rec[nb].y;  // of the node the walk stands on
  if (l == 0) path[0] = 0;
  while (d < kC4Path - 1 && first >= 0) {  // a board fills after 42 moves: bounded descent
    const uint64_t occ = m1 | m2;
    const bool legal = c4_legal(occ, l);
    const uint32_t gm = c4_group_mask(legal, gbase);
    const int n = __popc(gm);
    const int4 ch = t.rec[nb + first + (l < n ? l : 0)];
    double s = -__builtin_inf();
    if (l < n) {
      const int cv = ch.y;
      const float val = cv == 0 ? 0.0f : __int_as_float(ch.z) / (float)cv;
      double pb = t.lut_pb[pv];
      pb *= t.lut_sqrt[pv] / (double)(cv + 1);
      s = pb * (double)__int_as_float(ch.w) + (double)val;
    }
    int bi = l;
#pragma unroll
    for (int m = 4; m >= 1; m >>= 1) {
      const double os = __shfl_xor(s, m, kC4Group);
      const int oi = __shfl_xor(bi, m, kC4Group);
      if (os > s || (os == s && oi < bi)) {
        s = os;
        bi = oi;
      }
    }
    const int node = first + bi;
    first = __shfl(ch.x, bi, kC4Group);
    pv = __shfl(ch.y, bi, kC4Group);
    // child bi is the bi-th legal column; the stone drops to the column's lowest empty cell
    const bool mine = legal && __popc(gm & ((1u << l) - 1u)) == bi;
    const int col = __builtin_ctz(c4_group_mask(mine, gbase));
    const int h = __builtin_ctz(~(uint32_t)(occ >> (7 * col)));
    const uint64_t bit = 1ull << (7 * col + h);
    if (player == 1) m1 |= bit; else m2 |= bit;
    player = 3 - player;
    ++d;
    if (l == 0) path[d] = node;
  }
  int done, winner;
  c4_done_winner(m1, m2, done, winner);
  if (l == 0) {
    t.leaf[b * 4 + 0] = d;
    t.leaf[b * 4 + 1] = done;
    t.leaf[b * 4 + 2] = winner;
    t.leaf[b * 4 + 3] = player;
    t.leaf_bb[2 * b] = m1;
    t.leaf_bb[2 * b + 1] = m2;
  }
  c4_write_state(a.state + (size_t)b * 3 * kC4Cells, l, m1, m2, player);
}

// get_next_action's tail for one board (as lzm_az.h's az_finalize, over 7 actions): v / T summed in action
// order, divided; the first maximum, or a Philox draw keyed by seed, *counter and the board
__global__ void c4_finish_kernel(C4Tree t, double temperature, int sample, uint32_t seed, const int64_t *counter,
                                 int32_t *visits_out, double *probs_out, int32_t *action_out) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= t.B) return;
  const size_t nb = (size_t)b * t.cap;
  const uint64_t occ = t.root[2 * b] | t.root[2 * b + 1];
  const int f = t.rec[nb].x;
  double x[kC4Cols], sum = 0.0;
  int v[kC4Cols];
  for (int k = 0, j = 0; k < kC4Cols; ++k) {
    v[k] = (f >= 0 && c4_legal(occ, k)) ? t.rec[nb + f + j++].y : 0;
    x[k] = (double)v[k] / temperature;
    sum += x[k];
  }
  int best = 0;
  for (int k = 0; k < kC4Cols; ++k) {
    x[k] = x[k] / sum;
    if (x[k] > x[best]) best = k;
    visits_out[(size_t)b * kC4Cols + k] = v[k];
    probs_out[(size_t)b * kC4Cols + k] = x[k];
  }
  if (sample) {
    const uint64_t step = counter ? (uint64_t)*counter : 0;
    const uint4 r = philox4x32_10(make_uint4((uint32_t)b, (uint32_t)step, (uint32_t)(step >> 32), 0x4334u),
                                  make_uint2(seed, 0x414c5048u));
    const double u = ((double)(((uint64_t)(r.x >> 5) << 26) | (r.y >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
    double cum = 0.0;
    best = -1;
    for (int k = 0; k < kC4Cols; ++k) {
      cum += x[k];
      if (best < 0 && x[k] > 0.0 && u < cum) best = k;
    }
    for (int k = kC4Cols - 1; k >= 0 && best < 0; --k)
      if (x[k] > 0.0) best = k;
  }
  action_out[b] = best;
}

// test access: the records as arrays [B][cap] (any may be null); rows past the board's node count read 0 / -1
__global__ void c4_export_kernel(C4Tree t, int32_t *visit, float *vsum, int32_t *first, float *prior,
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
__global__ void __launch_bounds__(kC4Threads) c4_done_winner_kernel(const int32_t *boards, int n, int32_t *out) {
  const int b = blockIdx.x * (kC4Threads / kC4Group) + threadIdx.x / kC4Group;
  const int l = threadIdx.x & (kC4Group - 1);
  if (b >= n) return;
  uint64_t m1, m2;
  c4_load_board(boards + (size_t)b * kC4Cells, l, m1, m2);
  int done, winner;
  c4_done_winner(m1, m2, done, winner);
  if (l == 0) {
    out[2 * b] = done;
    out[2 * b + 1] = winner;
  }
}

}  // namespace lzm
