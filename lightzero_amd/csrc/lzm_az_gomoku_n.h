// lzm_az_gomoku_n.h — batched AlphaZero tree search for Gomoku 9 x 9 and 15 x 15 on the device: the semantics of
// lzm_az_gomoku.h (the game of zoo/board_games/gomoku/envs/gomoku_env.py and get_done_winner_cython.pyx, the tree
// of mcts_alphazero.cpp as oracle/az_oracle.py restates it), templated on the board size N.
//
// Same per-simulation protocol (begin, step(-1), S x step(k), finish): one launch finishes the previous simulation
// (expand the leaf with the network's priors or score the terminal position, back up with alternating signs), runs
// the next descent and writes the leaf's network input [3][N][N].
//
// Mapping: one wave per board, no barrier on the walk. Lane l owns the cpl = ceil(N^2 / 64) consecutive cells
// cpl l .. cpl l + cpl - 1 (2 at N = 9: lanes 0..40; 4 at N = 15: lanes 0..56) and carries their empty flags in
// cpl bits of one register. The position is two stone masks of `words` 64-bit words each (2 at N = 9, 4 at N = 15;
// bit (N + 1) row + column, so the bit after every row is clear and shifts by 1, N, N + 1 and N + 2 never wrap),
// uniform over the wave: the chosen cell is made scalar by a first-lane read, so the masks live in scalar
// registers. A run of five starting at a cell (the lowest bit of the run: the cell the reference's row-major scan
// meets first) is m & m >> s & m >> 2 s & m >> 3 s & m >> 4 s, four shifts by s carried across the words, for
// s = N (1, -1), N + 1 (1, 0), N + 2 (1, 1), 1 (0, 1); the winner owns the lowest start bit of either colour.
//
// A node is one 16-byte record {first child (-1: leaf), visit int, value_sum float, prior float}; a row of
// cap = 1 + N^2 (S + 1) records per board, a node's children contiguous in action order. Child j of a node is the
// j-th empty cell: its rank is the popcount of the lane's lower flags plus a wave prefix, cpl ballots of the flag
// bits counted below the lane. Each lane scores its own cells in action order (strict >: the first maximum), a
// butterfly on (score, cell) with the lower cell winning ties picks the wave's, and the owner lane's {first, visit,
// child index} go to every lane by a lane read. The descent is bounded by min(N^2, S + 1) levels; the backup takes
// the path 64 nodes per pass. No per-thread array is indexed by a run-time value: nothing goes to scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_az_gomoku_n_host.h"
#include "lzm_numerics.h"

namespace lzm {

constexpr int kGmkNThreads = 64;  // one board per workgroup

template <int W>
struct GmkNBits {
  uint64_t w[W];
};

template <int N>
using GmkNMask = GmkNBits<GmkNGeo<N>::words>;

template <int N>
__device__ inline int gmkn_bit(int cell) { return GmkNGeo<N>::rs * (cell / N) + cell % N; }

// m >> s for 0 < s < 64
template <int W>
__device__ inline GmkNBits<W> gmkn_shr(const GmkNBits<W> &m, int s) {
  GmkNBits<W> r;
#pragma unroll
  for (int i = 0; i < W; ++i) r.w[i] = (m.w[i] >> s) | (i + 1 < W ? m.w[i + 1] << (64 - s) : 0ull);
  return r;
}

// m | bit (bit < 64 W), no run-time index into the words
template <int W>
__device__ inline void gmkn_set(GmkNBits<W> &m, int bit) {
#pragma unroll
  for (int i = 0; i < W; ++i) m.w[i] |= (bit >> 6) == i ? 1ull << (bit & 63) : 0ull;
}

template <int W>
__device__ inline int gmkn_test(const GmkNBits<W> &m, int bit) {
  uint64_t v = 0;
#pragma unroll
  for (int i = 0; i < W; ++i) v = (bit >> 6) == i ? m.w[i] : v;
  return (int)((v >> (bit & 63)) & 1);
}

// the start cells of the player's runs of five (six in a row has two)
template <int N>
__device__ inline GmkNMask<N> gmkn_fives(const GmkNMask<N> &m) {
  constexpr int W = GmkNGeo<N>::words;
  const int shift[4] = {N, N + 1, N + 2, 1};
  GmkNMask<N> u;
#pragma unroll
  for (int i = 0; i < W; ++i) u.w[i] = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    GmkNMask<N> run = m, t = m;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      t = gmkn_shr<W>(t, shift[d]);
#pragma unroll
      for (int i = 0; i < W; ++i) run.w[i] &= t.w[i];
    }
#pragma unroll
    for (int i = 0; i < W; ++i) u.w[i] |= run.w[i];
  }
  return u;
}

// the bits of word i of a full board
template <int N>
__host__ __device__ constexpr uint64_t gmkn_full_word(int i) {
  uint64_t m = 0;
  for (int r = 0; r < N; ++r)
    for (int c = 0; c < N; ++c) {
      const int bit = GmkNGeo<N>::rs * r + c;
      if ((bit >> 6) == i) m |= 1ull << (bit & 63);
    }
  return m;
}

// get_done_winner: the owner of the first start cell in row-major order, else a full board is a draw
template <int N>
__device__ inline void gmkn_done_winner(const GmkNMask<N> &m1, const GmkNMask<N> &m2, int &done, int &winner) {
  constexpr int W = GmkNGeo<N>::words;
  const GmkNMask<N> f1 = gmkn_fives<N>(m1), f2 = gmkn_fives<N>(m2);
  constexpr uint64_t fw0 = gmkn_full_word<N>(0), fw1 = gmkn_full_word<N>(1), fw2 = gmkn_full_word<N>(2),
                     fw3 = gmkn_full_word<N>(3);
  winner = -1;
  bool full = true;
#pragma unroll
  for (int i = 0; i < W; ++i) {
    const uint64_t a = f1.w[i], b = f2.w[i];
    // (x & -x) isolates the lowest bit; an empty word compares as the largest value
    const uint64_t la = (a & (0 - a)) - 1, lb = (b & (0 - b)) - 1;
    if (winner == -1 && (a | b) != 0) winner = la < lb ? 1 : 2;
    const uint64_t fw = i == 0 ? fw0 : i == 1 ? fw1 : i == 2 ? fw2 : fw3;
    full = full && (m1.w[i] | m2.w[i]) == fw;
  }
  done = winner != -1 || full;
}

// the lane's cells: flag j is set where cell cpl l + j holds a bit of the mask
template <int N>
__device__ inline uint32_t gmkn_flags(const GmkNMask<N> &m, int l) {
  using G = GmkNGeo<N>;
  uint32_t f = 0;
#pragma unroll
  for (int j = 0; j < G::cpl; ++j) {
    const int cell = G::cpl * l + j;
    if (cell < G::cells) f |= (uint32_t)gmkn_test<G::words>(m, gmkn_bit<N>(cell)) << j;
  }
  return f;
}

// flags of the lane's cells that exist (the last owning lane has fewer, the lanes after it none)
template <int N>
__device__ inline uint32_t gmkn_own(int l) {
  using G = GmkNGeo<N>;
  uint32_t f = 0;
#pragma unroll
  for (int j = 0; j < G::cpl; ++j)
    if (G::cpl * l + j < G::cells) f |= 1u << j;
  return f;
}

// the number of set flags in the lanes below this one, and in the whole wave
template <int N>
__device__ inline int gmkn_prefix(uint32_t flags, int l, int &total) {
  int below = 0;
  total = 0;
#pragma unroll
  for (int j = 0; j < GmkNGeo<N>::cpl; ++j) {
    const uint64_t bal = __ballot((flags >> j) & 1);
    below += __popcll(bal & ((1ull << l) - 1ull));
    total += __popcll(bal);
  }
  return below;
}

// the board's stones as masks, uniform over the wave: every lane's contribution, or-ed by a butterfly
template <int N>
__device__ inline void gmkn_load_board(const int32_t *bd, int l, GmkNMask<N> &m1, GmkNMask<N> &m2) {
  using G = GmkNGeo<N>;
#pragma unroll
  for (int i = 0; i < G::words; ++i) m1.w[i] = m2.w[i] = 0;
#pragma unroll
  for (int j = 0; j < G::cpl; ++j) {
    const int cell = G::cpl * l + j;
    const int v = cell < G::cells ? bd[cell] : 0;
    const int bit = gmkn_bit<N>(cell < G::cells ? cell : 0);
    if (v == 1) gmkn_set<G::words>(m1, bit);
    if (v == 2) gmkn_set<G::words>(m2, bit);
  }
#pragma unroll
  for (int i = 0; i < G::words; ++i) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
      m1.w[i] |= (uint64_t)__shfl_xor((unsigned long long)m1.w[i], d, 64);
      m2.w[i] |= (uint64_t)__shfl_xor((unsigned long long)m2.w[i], d, 64);
    }
  }
}

template <int N>
__device__ inline void gmkn_read_masks(const uint64_t *src, GmkNMask<N> &m1, GmkNMask<N> &m2) {
#pragma unroll
  for (int i = 0; i < GmkNGeo<N>::words; ++i) {
    m1.w[i] = src[i];
    m2.w[i] = src[kGmkNWords + i];
  }
}

template <int N>
__device__ inline void gmkn_write_masks(uint64_t *dst, const GmkNMask<N> &m1, const GmkNMask<N> &m2) {
#pragma unroll
  for (int i = 0; i < GmkNGeo<N>::words; ++i) {
    dst[i] = m1.w[i];
    dst[kGmkNWords + i] = m2.w[i];
  }
}

// current_state()[1] with scale=True: the stones of the player to move, the stones of `to_play` (the other
// player), 0.5 * the player to move
template <int N>
__device__ inline void gmkn_write_state(float *st, int l, const GmkNMask<N> &m1, const GmkNMask<N> &m2, int player) {
  using G = GmkNGeo<N>;
  const uint32_t f1 = gmkn_flags<N>(m1, l), f2 = gmkn_flags<N>(m2, l);
  const uint32_t mine = player == 1 ? f1 : f2, theirs = player == 1 ? f2 : f1;
#pragma unroll
  for (int j = 0; j < G::cpl; ++j) {
    const int cell = G::cpl * l + j;
    if (cell >= G::cells) continue;
    st[cell] = ((mine >> j) & 1) ? 0.5f : 0.0f;
    st[G::cells + cell] = ((theirs >> j) & 1) ? 0.5f : 0.0f;
    st[2 * G::cells + cell] = 0.5f * (float)player;
  }
}

// _expand_leaf_node: one child per empty cell in action order, prior = float(probs[a]); at the root, when
// sampling, _add_exploration_noise: float(double(prior) * (1 - w) + noise[i] * w)
template <int N>
__device__ inline void gmkn_expand(const GmkNTree &t, size_t nb, int b, int node, int base, int l,
                                   const GmkNMask<N> &m1, const GmkNMask<N> &m2, const float *probs, bool noise,
                                   double w) {
  using G = GmkNGeo<N>;
  const uint32_t em = gmkn_own<N>(l) & ~(gmkn_flags<N>(m1, l) | gmkn_flags<N>(m2, l));
  int n;
  const int below = gmkn_prefix<N>(em, l, n);
#pragma unroll
  for (int j = 0; j < G::cpl; ++j) {
    if (!((em >> j) & 1)) continue;
    const int rank = below + __popc(em & ((1u << j) - 1u));
    float p = probs[G::cpl * l + j];
    if (noise) p = (float)((double)p * (1.0 - w) + t.noise[(size_t)(n - 1) * G::cells + rank] * w);
    t.rec[nb + base + rank] = make_int4(-1, 0, __float_as_int(0.0f), __float_as_int(p));
  }
  if (l == 0) {
    t.rec[nb + node].x = n > 0 ? base : -1;
    t.nnodes[b] = base + n;
  }
}

template <int N>
__global__ void __launch_bounds__(kGmkNThreads) gmkn_begin_kernel(GmkNTree t, const int32_t *boards,
                                                                  const int32_t *start_index, float *state) {
  using G = GmkNGeo<N>;
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= t.B) return;
  const int player = start_index[b] == 0 ? 1 : 2;
  GmkNMask<N> m1, m2;
  gmkn_load_board<N>(boards + (size_t)b * G::cells, l, m1, m2);
  if (l == 0) {
    gmkn_write_masks<N>(t.root + (size_t)b * 2 * kGmkNWords, m1, m2);
    t.root_player[b] = player;
  }
  gmkn_write_state<N>(state + (size_t)b * 3 * G::cells, l, m1, m2, player);
}

template <int N>
__global__ void __launch_bounds__(kGmkNThreads) gmkn_step_kernel(GmkNTree t, GmkNStepArgs a) {
  using G = GmkNGeo<N>;
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= t.B) return;
  const size_t nb = (size_t)b * t.cap;
  int32_t *path = t.path + (size_t)b * t.path_len;
  const float *probs = a.probs + (size_t)b * a.pstride;
  GmkNMask<N> m1, m2;
  gmkn_read_masks<N>(t.root + (size_t)b * 2 * kGmkNWords, m1, m2);
  if (a.sim < 0) {
    // a fresh root (Node()), expanded with the root evaluation; noise only when sampling
    if (l == 0) t.rec[nb] = make_int4(-1, 0, __float_as_int(0.0f), __float_as_int(1.0f));
    gmkn_expand<N>(t, nb, b, 0, 1, l, m1, m2, probs, a.with_noise != 0, a.noise_weight);
  } else {
    const int depth = t.leaf[b * 4 + 0], done = t.leaf[b * 4 + 1], winner = t.leaf[b * 4 + 2],
              player = t.leaf[b * 4 + 3];
    double lv;
    if (!done) {
      GmkNMask<N> l1, l2;
      gmkn_read_masks<N>(t.leaf_bb + (size_t)b * 2 * kGmkNWords, l1, l2);
      gmkn_expand<N>(t, nb, b, path[depth], t.nnodes[b], l, l1, l2, probs, false, 0.0);
      lv = (double)a.values[(size_t)b * a.vstride];
    } else {
      lv = winner == -1 ? 0.0 : (player == winner ? 1.0 : -1.0);
    }
    // node->update_recursive(-leaf_value): + v at the leaf, - v at its parent, ...; the k-th node up the path goes
    // to lane k % 64 in pass k / 64 (the path's nodes are distinct)
    const float v = (float)(-lv);
    for (int k = l; k <= depth; k += kGmkNThreads) {
      int4 *n = t.rec + nb + path[depth - k];
      n->y += 1;
      n->z = __float_as_int(__int_as_float(n->z) + ((k & 1) ? -v : v));
    }
  }
  if (a.sim + 1 >= t.S) return;
  __threadfence_block();  // the descent reads what this wave just wrote

  // ---- _simulate: descend by the maximal pUCT child while the node has children
  uint32_t em = gmkn_own<N>(l) & ~(gmkn_flags<N>(m1, l) | gmkn_flags<N>(m2, l));  // the lane's empty cells
  int player = t.root_player[b], d = 0;
  int first = t.rec[nb].x, pv = t.rec[nb].y;  // of the node the walk stands on
  if (l == 0) path[0] = 0;
  while (d < t.path_len - 1 && first >= 0) {
    int total;
    const int below = gmkn_prefix<N>(em, l, total);
    int4 ch[G::cpl];
#pragma unroll
    for (int j = 0; j < G::cpl; ++j)
      ch[j] = t.rec[nb + first + (((em >> j) & 1) ? below + __popc(em & ((1u << j) - 1u)) : 0)];
    const double pb0 = t.lut_pb[pv], sq = t.lut_sqrt[pv];
    double s = -__builtin_inf();
    int bi = G::cpl * l, bx = -1, by = 0, bidx = 0;
#pragma unroll
    for (int j = 0; j < G::cpl; ++j) {
      if (!((em >> j) & 1)) continue;
      const int cv = ch[j].y;
      const float val = cv == 0 ? 0.0f : __int_as_float(ch[j].z) / (float)cv;
      double pb = pb0;
      pb *= sq / (double)(cv + 1);
      const double sj = pb * (double)__int_as_float(ch[j].w) + (double)val;
      if (sj > s) {
        s = sj;
        bi = G::cpl * l + j;
        bx = ch[j].x;
        by = ch[j].y;
        bidx = below + __popc(em & ((1u << j) - 1u));
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const double os = __shfl_xor(s, m, 64);
      const int oi = __shfl_xor(bi, m, 64);
      if (os > s || (os == s && oi < bi)) {
        s = os;
        bi = oi;
      }
    }
    bi = __builtin_amdgcn_readfirstlane(bi);
    const int owner = bi / G::cpl;
    const int node = first + __shfl(bidx, owner, 64);
    first = __shfl(bx, owner, 64);
    pv = __shfl(by, owner, 64);
    if (player == 1) gmkn_set<G::words>(m1, gmkn_bit<N>(bi)); else gmkn_set<G::words>(m2, gmkn_bit<N>(bi));
    if (l == owner) em &= ~(1u << (bi % G::cpl));
    player = 3 - player;
    ++d;
    if (l == 0) path[d] = node;
  }
  int done, winner;
  gmkn_done_winner<N>(m1, m2, done, winner);
  if (l == 0) {
    t.leaf[b * 4 + 0] = d;
    t.leaf[b * 4 + 1] = done;
    t.leaf[b * 4 + 2] = winner;
    t.leaf[b * 4 + 3] = player;
    gmkn_write_masks<N>(t.leaf_bb + (size_t)b * 2 * kGmkNWords, m1, m2);
  }
  gmkn_write_state<N>(a.state + (size_t)b * 3 * G::cells, l, m1, m2, player);
}

// get_next_action's tail (as lzm_az_gomoku.h's, over N^2 actions), one wave per board: v / T of every action in
// LDS, summed in action order by every lane, divided; the first maximum, or a Philox draw keyed by seed, *counter
// and the board
template <int N>
__global__ void __launch_bounds__(kGmkNThreads) gmkn_finish_kernel(GmkNTree t, double temperature, int sample,
                                                                   uint32_t seed, const int64_t *counter,
                                                                   int32_t *visits_out, double *probs_out,
                                                                   int32_t *action_out) {
  using G = GmkNGeo<N>;
  __shared__ double xs[G::cells];
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= t.B) return;
  const size_t nb = (size_t)b * t.cap;
  GmkNMask<N> m1, m2;
  gmkn_read_masks<N>(t.root + (size_t)b * 2 * kGmkNWords, m1, m2);
  const uint32_t em = gmkn_own<N>(l) & ~(gmkn_flags<N>(m1, l) | gmkn_flags<N>(m2, l));
  int total;
  const int below = gmkn_prefix<N>(em, l, total);
  const int f = t.rec[nb].x;
#pragma unroll
  for (int j = 0; j < G::cpl; ++j) {
    const int cell = G::cpl * l + j;
    if (cell >= G::cells) continue;
    const bool mine = f >= 0 && ((em >> j) & 1);
    const int v = mine ? t.rec[nb + f + below + __popc(em & ((1u << j) - 1u))].y : 0;
    visits_out[(size_t)b * G::cells + cell] = v;
    xs[cell] = (double)v / temperature;
  }
  __syncthreads();
  double sum = 0.0;
  for (int k = 0; k < G::cells; ++k) sum += xs[k];
#pragma unroll
  for (int j = 0; j < G::cpl; ++j) {
    const int cell = G::cpl * l + j;
    if (cell < G::cells) probs_out[(size_t)b * G::cells + cell] = xs[cell] / sum;
  }
  int best = 0;
  if (!sample) {
    double bx = xs[0] / sum;
    for (int k = 1; k < G::cells; ++k) {
      const double xk = xs[k] / sum;
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
    for (int k = 0; k < G::cells; ++k) {
      const double xk = xs[k] / sum;
      cum += xk;
      if (xk > 0.0) last = k;
      if (best < 0 && xk > 0.0 && u < cum) best = k;
    }
    if (best < 0) best = last;
  }
  if (l == 0) action_out[b] = best;
}

// test access: the records as arrays [B][cap] (any may be null); rows past the board's node count read 0 / -1
__global__ void gmkn_export_kernel(GmkNTree t, int32_t *visit, float *vsum, int32_t *first, float *prior,
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
template <int N>
__global__ void __launch_bounds__(kGmkNThreads) gmkn_done_winner_kernel(const int32_t *boards, int n, int32_t *out) {
  const int b = blockIdx.x, l = threadIdx.x;
  if (b >= n) return;
  GmkNMask<N> m1, m2;
  gmkn_load_board<N>(boards + (size_t)b * GmkNGeo<N>::cells, l, m1, m2);
  int done, winner;
  gmkn_done_winner<N>(m1, m2, done, winner);
  if (l == 0) {
    out[2 * b] = done;
    out[2 * b + 1] = winner;
  }
}

}  // namespace lzm
