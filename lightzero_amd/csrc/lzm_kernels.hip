// lzm_kernels.hip — MI355X (gfx950) batched MuZero / EfficientZero search tree.
//
// Replaces LightZero's ctree (lzero/mcts/ctree/ctree_{muzero,efficientzero}) and the per-
// simulation glue of lzero/mcts/tree_search/mcts_ctree.py with device kernels over a
// structure-of-arrays tree held in HBM. C ABI: include/lzmcts.h.
//
// Layout (per handle, B roots, A actions, node capacity C = 1 + A*(S_cap+1)):
//   stat[node][root]  16 B {visit, value_sum, prior, reward|value_prefix}
//   meta[node][root]  16 B {latent index (-1 = not expanded), to_play, best_action, is_reset}
// node-major with the root index fastest, so lanes of a wave that sit on the same node id
// (the root, its children) read one contiguous 1 KiB line per wave instruction. The node
// expanded with latent index L (root 0, simulation k's leaf k+1) owns children
// [1 + A*L, 1 + A*L + A) — the reference's std::map<int,CNode> children (cnode.h:26)
// without allocation. Search paths of the last traverse: path[level][root].
//
// Arithmetic follows the reference expression by expression in fp32 (compiled with
// -ffp-contract=off, IEEE division/sqrt), expf is the glibc port of lzm_numerics.h, and
// log((N+base+1)/base)+init and sqrt(N) over the integer parent count N come from a host
// table built with the host's libm (the very functions the reference calls).
//
// Generic search path (any PyTorch network between the launches): traverse_lookback_kernel (parity mode: one
// wave per root, the batch-serial rand() offsets by decoupled look-back, lzm_traverse_lb.h) or
// traverse_fast_kernel (Philox), then backprop_kernel from raw lists or decode_backprop_kernel from support
// logits; decode_traverse_kernel folds the next traverse into the decode's launch; the Gumbel MuZero tree
// (lzm_gumbel.h) has its own three. On the host one builder per argument struct serves every entry point.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <mutex>
#include <random>
#include <vector>

#include "../../include/lzmcts.h"
#include "lzm_numerics.h"
#include "lzm_collect.h"
#include "lzm_atari.h"
#include "lzm_traj.h"
#include "lzm_az.h"
#include "lzm_az_fused.h"
#include "lzm_tree.h"
#include "lzm_gumbel.h"
#include "lzm_search_mlp.h"
#include "lzm_search_res.h"
#include "lzm_conv.h"
#include "lzm_repr.h"
#include "lzm_heads.h"
#include "lzm_lstm.h"
#include "lzm_initial.h"
#include "lzm_traverse_lb.h"
#include "lzm_search_conv.h"

namespace lzm {

struct TraverseArgs {
  TreeView t;
  const float4 *minmax;
  const uint32_t *seed;
  const int32_t *vtp_in;
  WalkOut out;
  float disc;
};

__device__ inline int block_players(const int32_t *vtp, int B) {
  // players = (max(virtual_to_play) == -1) ? 1 : 2  (cnode.cpp:776-781)
  __shared__ int s_max;
  if (threadIdx.x == 0) s_max = INT_MIN;
  __syncthreads();
  int m = INT_MIN;
  for (int i = threadIdx.x; i < B; i += blockDim.x) m = max(m, vtp[i]);
  atomicMax(&s_max, m);
  __syncthreads();
  int p = (s_max == -1) ? 1 : 2;
  __syncthreads();
  return p;
}

// Fast-mode traverse: roots are independent (Philox4x32-10 draw per (seed, root, level)), so
// one lane per root over as many workgroups as needed.
template <bool EZ>
__global__ __launch_bounds__(256) void traverse_fast_kernel(TraverseArgs p) {
  const TreeView &t = p.t;
  const int players = block_players(p.vtp_in, t.B);
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.B) return;
  const uint32_t seed = *p.seed;
  auto draw = [&](int level) -> uint32_t {
    uint4 o = philox4x32_10(make_uint4((uint32_t)level, (uint32_t)i, 0u, 0u), make_uint2(seed, 0x4c5a4d43u));
    return o.x >> 1;
  };
  Descent d = descend<EZ>(t, i, p.minmax[i], players, p.vtp_in[i], p.disc, draw);
  store_walk(p.out, t, i, d.x, d.action, d.vtp, d.len);
  for (int l = 0; l < d.len; ++l) {
    const int node = t.path[(size_t)l * t.B + i];
    t.meta[nidx(t, node, i)].best = t.path_act[(size_t)l * t.B + i];
  }
}

struct BackpropArgs {
  TreeView t;
  float4 *minmax;
  const float *rewards, *values, *logits;
  const int32_t *to_play, *is_reset;
  int cur;
  float disc;
  const int32_t *reuse_action;  // optional: search-with-reuse, see reuse_leaf
  const float *reuse_value;
};

// cbatch_backpropagate_with_reuse (ctree_muzero/lib/cnode.cpp:502-546; EfficientZero
// ctree_efficientzero/lib/cnode.cpp:603-641, there with is_reset set on every leaf) for root i whose walk ended
// at `leaf` after `len` levels: no inference when the walk stopped on an expanded node (the root
// child of the true action: no expand, back up the reuse value); a walk that stopped at the
// unexpanded true-action child expands it but backs up the reuse value too.
__device__ inline void reuse_leaf(const TreeView &t, int i, int leaf, int len, const int32_t *ra, const float *rv,
                                  bool *no_inference, float *value) {
  *no_inference = false;
  if (!ra) return;
  const bool expanded = t.meta[nidx(t, leaf, i)].latent >= 0;
  const bool reuse = !expanded && len == 1 && t.path_act[i] == ra[i];
  if (expanded || reuse) *value = rv[i];
  *no_inference = expanded;
}

template <bool EZ>
__global__ __launch_bounds__(256) void backprop_kernel(BackpropArgs p) {
  const TreeView &t = p.t;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.B) return;
  const int len = t.pathlen[i];
  const int leaf = t.path[(size_t)len * t.B + i];
  const int tp = p.to_play[i];
  float v = p.values[i];
  bool no_inf;
  reuse_leaf(t, i, leaf, len, p.reuse_action, p.reuse_value, &no_inf, &v);
  if (!no_inf)
    expand_leaf(t, i, leaf, tp, p.cur, p.rewards[i], p.logits + (size_t)i * t.A, p.is_reset ? p.is_reset[i] : 0, EZ);
  else if (EZ)  // the reference sets every leaf's is_reset, expanded or not (ctree_efficientzero cnode.cpp:638)
    t.meta[nidx(t, leaf, i)].is_reset = p.is_reset ? p.is_reset[i] : 0;
  backup<EZ>(t, i, p.minmax + i, tp, v, p.disc);
}

struct DecodeArgs {
  TreeView t;
  float4 *minmax;
  const float *reward_logits, *value_logits, *policy_logits;
  const int32_t *to_play;
  int32_t *out_is_reset;
  const float *next_latent;
  float *pool_slot;
  long long row_elems;
  int V, Vv, categorical, cur, horizon;  // V: reward support length, Vv: value support length
  float disc;
  float *out_decoded;  // [B][2] {reward, value} after h^-1, optional
  const int32_t *reuse_action;  // optional: search-with-reuse, see reuse_leaf
  const float *reuse_value;
};

// ensure_softmax (scaling_transform.py:36-62): softmax is skipped only when EVERY row of the
// batch already sums to 1 within allclose(atol=1e-5, rtol=1e-5) — judged per tensor (the
// reference calls the transform once per head: a = reward rows, b = value rows). Each workgroup
// (4 rows) overwrites its own verdict words part[2 * block + head] (1: no row of that head in the
// block fails), so nothing has to be cleared between calls; consumers AND the words (norm_ok).
__global__ __launch_bounds__(256) void normalized_check_kernel(const float *a, const float *b, int rows, int V,
                                                               int Vb, int32_t *part) {
  __shared__ int s_ok[2];
  if (threadIdx.x == 0) s_ok[0] = s_ok[1] = 1;
  __syncthreads();
  const int w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (w < 2 * rows) {
    const float *row = (w < rows) ? a + (size_t)w * V : b + (size_t)(w - rows) * Vb;
    const float s = wave_row_sum(row, w < rows ? V : Vb);
    if ((threadIdx.x & 63) == 0 && !(fabsf(s - 1.0f) <= 1e-5f + 1e-5f)) atomicAnd(&s_ok[w < rows ? 0 : 1], 0);
  }
  __syncthreads();
  if (threadIdx.x < 2) part[2 * blockIdx.x + threadIdx.x] = s_ok[threadIdx.x];
}
__host__ __device__ inline int norm_parts(int rows) { return (2 * rows * 64 + 255) / 256; }
// head's verdict over every block's word (wave-uniform result)
__device__ inline bool norm_ok(const int32_t *part, int nparts, int head) {
  int bad = 0;
  for (int q = (threadIdx.x & 63); q < nparts; q += 64) bad |= part[2 * q + head] == 0;
  return __ballot(bad) == 0ull;
}

// the head part of decode_root: files root i's new latent row, decodes its reward and value rows (all 64 lanes)
__device__ inline void decode_heads(const DecodeArgs &p, const int32_t *norm_part, int i, float *out_r, float *out_v) {
  const TreeView &t = p.t;
  const int lane = threadIdx.x & 63;
  // new latent row into the pool slot (mcts_ctree.py:305)
  if (p.next_latent && p.pool_slot) {
    const float *src = p.next_latent + (size_t)i * p.row_elems;
    float *dst = p.pool_slot + (size_t)i * p.row_elems;
    for (long long e = lane; e < p.row_elems; e += 64) dst[e] = src[e];
  }
  float r, v;
  if (p.categorical) {
    const int np = norm_parts(t.B);
    r = wave_support_expectation(p.reward_logits + (size_t)i * p.V, p.V, !norm_ok(norm_part, np, 0));
    v = wave_support_expectation(p.value_logits + (size_t)i * p.Vv, p.Vv, !norm_ok(norm_part, np, 1));
  } else {
    r = p.reward_logits[(size_t)i * p.V];
    v = p.value_logits[(size_t)i * p.Vv];
  }
  r = h_inverse(r);
  v = h_inverse(v);
  if (p.out_decoded && lane == 0) {
    p.out_decoded[2 * i] = r;
    p.out_decoded[2 * i + 1] = v;
  }
  *out_r = r;
  *out_v = v;
}

// decode + expand + backup of root i by one wave (all 64 lanes call it)
template <bool EZ>
__device__ inline void decode_root(const DecodeArgs &p, const int32_t *norm_part, int i) {
  const TreeView &t = p.t;
  const int lane = threadIdx.x & 63;
  float r, v;
  decode_heads(p, norm_part, i, &r, &v);
  // one lane per child / path level (A <= kMaxActions = 64), bit-identical to backprop_kernel's
  // expand_leaf / backup (lzm_tree.h)
  const int len = t.pathlen[i];
  const int leaf = t.path[(size_t)len * t.B + i];
  const int tp = p.to_play[i];
  const int is_reset = (EZ && p.horizon > 0 && len % p.horizon == 0) ? 1 : 0;
  if (p.out_is_reset && lane == 0) p.out_is_reset[i] = is_reset;
  bool no_inf;
  reuse_leaf(t, i, leaf, len, p.reuse_action, p.reuse_value, &no_inf, &v);
  if (!no_inf) expand_wave(t, i, leaf, tp, p.cur, r, p.policy_logits + (size_t)i * t.A, EZ ? is_reset : -1);
  else if (EZ && lane == 0) t.meta[nidx(t, leaf, i)].is_reset = is_reset;  // (cnode.cpp:638, every leaf)
  if (EZ)
    backup_wave_ez(t, i, i, t.B, p.minmax + i, tp, v, p.disc);
  else
    backup_wave(t, i, i, t.B, p.minmax + i, tp, v, p.disc);
}

template <bool EZ>
__global__ __launch_bounds__(256) void decode_backprop_kernel(DecodeArgs p, const int32_t *norm_part) {
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // one wave per root
  if (i < p.t.B) decode_root<EZ>(p, norm_part, i);
}

__global__ __launch_bounds__(256) void inverse_transform_kernel(const float *logits, int rows, int V, int categorical,
                                                                const int32_t *norm_part, float *out) {
  const int i = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  if (i >= rows) return;
  float v;
  if (categorical) {
    v = wave_support_expectation(logits + (size_t)i * V, V, !norm_ok(norm_part, norm_parts(rows), 0));
  } else {
    v = logits[(size_t)i * V];
  }
  if ((threadIdx.x & 63) == 0) out[i] = h_inverse(v);
}


__global__ __launch_bounds__(256) void prepare_kernel(PrepareArgs p) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < p.B) prepare_root(p, i);
}

__global__ void minmax_init_kernel(float4 *mm, int n, float delta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) mm[i] = make_float4(kFloatMin, kFloatMax, delta, 0.0f);
}

// collect-step mode on the weight-streaming path (the network-resident kernel does both in-kernel):
// seeds of this step (seed_sequence_kernel's rule) and, optionally, fresh min-max bounds ...
__global__ void step_prologue_kernel(const int64_t *count, long long base, int S, int32_t *seeds, float4 *mm, int n,
                                     int fresh, float delta) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (count && i < S) seeds[i] = (int32_t)((base + *count * (long long)S + i) % 1000000ll);
  if (fresh && i < n) mm[i] = make_float4(kFloatMin, kFloatMax, delta, 0.0f);
}

__global__ void gather_kernel(const float *pool, long long row, int B, const int32_t *x, float *out) {
  const long long total = (long long)B * row;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(e / row);
    const long long c = e - (long long)i * row;
    const int xi = max(x[i], 0);
    out[e] = pool[((long long)xi * B + i) * row + c];
  }
}

__global__ void gather_kernel_v4(const float4 *pool, long long row4, int B, const int32_t *x, float4 *out) {
  const long long total = (long long)B * row4;
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(e / row4);
    const long long c = e - (long long)i * row4;
    const int xi = max(x[i], 0);  // an unexpanded root reports -1 (reference: UB); never read before the pool
    out[e] = pool[((long long)xi * B + i) * row4 + c];
  }
}

__global__ void distributions_kernel(TreeView t, int32_t *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.B) return;
  const NodeMeta rm = t.meta[i];
  for (int j = 0; j < t.A; ++j) {
    int v = -1;
    if (rm.latent >= 0 && j < t.nlegal[i]) v = t.stat[nidx(t, 1 + t.A * rm.latent + t.legal[(size_t)i * t.A + j], i)].visit;
    out[(size_t)i * t.A + j] = v;
  }
}

// get_distributions and get_values in one pass (the collect step reads both every env step)
__global__ void root_outputs_kernel(TreeView t, int32_t *dist, float *values) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.B) return;
  const NodeStat rs = t.stat[i];
  const NodeMeta rm = t.meta[i];
  for (int j = 0; j < t.A; ++j) {
    int v = -1;
    if (rm.latent >= 0 && j < t.nlegal[i]) v = t.stat[nidx(t, 1 + t.A * rm.latent + t.legal[(size_t)i * t.A + j], i)].visit;
    dist[(size_t)i * t.A + j] = v;
  }
  values[i] = node_value(rs);
}

// ... and after the search: the root outputs (root_outputs_kernel) and the step counter
__global__ void step_epilogue_kernel(TreeView t, int32_t *dist, float *values, int64_t *count) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (dist && i < t.B) {
    const NodeMeta rm = t.meta[i];
    for (int j = 0; j < t.A; ++j) {
      int v = -1;
      if (rm.latent >= 0 && j < t.nlegal[i]) v = t.stat[nidx(t, 1 + t.A * rm.latent + t.legal[(size_t)i * t.A + j], i)].visit;
      dist[(size_t)i * t.A + j] = v;
    }
  }
  if (values && i < t.B) values[i] = node_value(t.stat[i]);
  if (count && i == 0) *count += 1;
}

__global__ void values_kernel(TreeView t, float *out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < t.B) out[i] = node_value(t.stat[i]);
}

__global__ void trajectories_kernel(TreeView t, int32_t *out, int tmax) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= t.B) return;
  int node = 0, n = 0;
  NodeMeta m = t.meta[nidx(t, 0, i)];
  while (m.best >= 0 && n < tmax && m.latent >= 0) {
    out[(size_t)i * tmax + n++] = m.best;
    node = 1 + t.A * m.latent + m.best;
    m = t.meta[nidx(t, node, i)];
  }
  for (; n < tmax; ++n) out[(size_t)i * tmax + n] = -1;
}

__global__ void debug_expf_kernel(const float *x, float *out, long long n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
    out[e] = glibc_expf(x[e]);
}

__global__ void debug_div_small_kernel(const float *x, const int32_t *d, float *out, long long n) {
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x)
    out[e] = div_small(x[e], d[e]);
}

// lzm_debug_settle_chain: one wave, level l's latent is n - 1 - l (so the gather is no identity): lane L holds
// the record of latent L, lane l the latent of level l, as in descend_a2r
__global__ void __launch_bounds__(64) debug_settle_chain_kernel(const float *tq, const int32_t *tv, int n, float *out) {
  const int lane = threadIdx.x;
  const int lev = n - 1 - lane;  // the level whose latent is this lane
  const float rtq = lane < n ? tq[lev] : 0.0f;
  const int rpk = lane < n ? (tv[lev] & 3) << 5 : 0;
  const int plev = lane < n ? n - 1 - lane : 0;
  const bool fin = __ballot(lane < n && (__float_as_int(rtq) & 0x7f800000) == 0x7f800000) == 0ull;  // terms_finite_a2r
  for (int l = 0; l < n; ++l) {
    const float q = settle_chain(rtq, rpk, plev, fin, 0, l / 2, 0.0f);
    const float r = settle_chain(rtq, rpk, plev, fin, l / 2, l + 1, q);
    if (lane == 0) out[l] = r;
  }
}

// lzm_debug_xor: the DPP / permlane butterfly helpers (lzm_tree.h xor_partner / xor_sum / xor_max) beside
// the ds_bpermute __shfl_xor they replace, one 64-lane wave; rows of out [16][64]:
//   0-5 xor_partner<1..32>, 6-11 __shfl_xor(v, 1..32), 12 xor_sum, 13 the __shfl_xor butterfly sum,
//   14 xor_max, 15 the __shfl_xor butterfly max
__global__ void __launch_bounds__(64) debug_xor_kernel(const float *in, float *out) {
  const int l = threadIdx.x;
  const float v = in[l];
  out[0 * 64 + l] = xor_partner<1>(v);
  out[1 * 64 + l] = xor_partner<2>(v);
  out[2 * 64 + l] = xor_partner<4>(v);
  out[3 * 64 + l] = xor_partner<8>(v);
  out[4 * 64 + l] = xor_partner<16>(v);
  out[5 * 64 + l] = xor_partner<32>(v);
  for (int k = 0; k < 6; ++k) out[(6 + k) * 64 + l] = __shfl_xor(v, 1 << k, 64);
  out[12 * 64 + l] = xor_sum(v);
  float s = v, m = v;
  for (int d = 32; d >= 1; d >>= 1) {
    s += __shfl_xor(s, d, 64);
    m = fmaxf(m, __shfl_xor(m, d, 64));
  }
  out[13 * 64 + l] = s;
  out[14 * 64 + l] = xor_max(v);
  out[15 * 64 + l] = m;
}

// lzm_debug_az_rules: the fused AlphaZero search's mask / DPP forms beside the scans they replace, one board per
// 16-lane group: out[b][6] = {done, winner by az_done_winner (the reference's cell scan), done, winner by
// az_done_winner_mask, the lane az_group_argmax picks from scores[b][16], the first strict maximum of a scan}
__global__ void __launch_bounds__(64) debug_az_rules_kernel(int n, const int32_t *boards, const double *scores,
                                                            int32_t *out) {
  const int b = blockIdx.x * 4 + (threadIdx.x >> 4), l = threadIdx.x & 15, gbase = (threadIdx.x & 63) & ~15;
  const bool on = b < n;  // group-uniform
  const int cell = on && l < 9 ? boards[(size_t)b * 9 + l] : 0;
  const double sc = on ? scores[(size_t)b * 16 + l] : 0.0;
  const int bi = az_group_argmax(sc, gbase);  // (every lane of the wave takes part)
  int done_m, win_m;
  az_done_winner_mask(az_group_mask(l < 9 && cell == 1, gbase), az_group_mask(l < 9 && cell == 2, gbase), done_m, win_m);
  if (!on || l != 0) return;
  int bd[9];
  for (int k = 0; k < 9; ++k) bd[k] = boards[(size_t)b * 9 + k];
  int done_s, win_s;
  az_done_winner(bd, done_s, win_s);
  int best = 0;
  for (int k = 1; k < 16; ++k)
    if (scores[(size_t)b * 16 + k] > scores[(size_t)b * 16 + best]) best = k;
  int32_t *o = out + (size_t)b * 6;
  o[0] = done_s; o[1] = win_s; o[2] = done_m; o[3] = win_m; o[4] = bi; o[5] = best;
}

__global__ void debug_philox_kernel(const uint32_t *ck, uint32_t *out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint32_t *c = ck + (size_t)i * 6;
  uint4 o = philox4x32_10(make_uint4(c[0], c[1], c[2], c[3]), make_uint2(c[4], c[5]));
  out[(size_t)i * 4 + 0] = o.x;
  out[(size_t)i * 4 + 1] = o.y;
  out[(size_t)i * 4 + 2] = o.z;
  out[(size_t)i * 4 + 3] = o.w;
}

// lzm_debug_glibc_rand: rand() output p < n through the generator every parity search draws from — the
// coefficient table (glibc_coef_table, n positions) over seed_state_parallel's state — in the form asked
// for: 0 glibc_draw, one thread per position; 1 glibc_draw_wave, the position wave-uniform; 2 lane_draws,
// each wave over its 64 positions, read back through operator(). Workgroup g covers positions 256 g ..
__global__ __launch_bounds__(256) void debug_glibc_kernel(uint32_t seed, int n, int form, int32_t *out,
                                                          const uint32_t *coef, const uint32_t *pow16807,
                                                          int32_t *overflow) {
  __shared__ uint32_t s_z0[31], s_pow[31];
  const int tid = threadIdx.x, lane = tid & 63;
  if (tid < 31) s_pow[tid] = pow16807[tid];
  __syncthreads();
  seed_state_parallel(seed, s_pow, s_z0);
  __syncthreads();
  if (form == 0) {
    const int p = blockIdx.x * 256 + tid;
    if (p < n) out[p] = (int32_t)glibc_draw(coef, n, s_z0, p, overflow);
    return;
  }
  const int base = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 256 + (tid & ~63)));  // of this wave
  const LaneDraws draws = lane_draws(coef, n, s_z0, base, 0, 64, overflow);
  for (int l = 0; l < 64 && base + l < n; ++l) {
    const uint32_t r = form == 1 ? glibc_draw_wave(coef, n, s_z0, base + l, overflow) : draws(l);
    if (lane == 0) out[base + l] = (int32_t)r;
  }
}

// Simulation k's decode + expand + backup fused with simulation k + 1's traverse (generic search
// path, parity mode): the wave that backs up root i walks root i again at once, over the records it
// has just written (warm in this CU's caches) and without a launch of its own. The walk is the
// look-back traverse's (lzm_traverse_lb.h), so requests and draws are those of the separate launches.
template <bool EZ>
__global__ __launch_bounds__(kTlbThreads) void decode_traverse_kernel(DecodeArgs p, const int32_t *norm_part,
                                                                      TraverseLbArgs q) {
  __shared__ uint32_t s_z0[31], s_pow[31];
  __shared__ int s_epoch;
  int players;
  const unsigned long long epoch = traverse_lb_setup(q, s_z0, s_pow, &s_epoch, &players);
  const int i = blockIdx.x * (kTlbThreads / 64) + (threadIdx.x >> 6);
  if (i < p.t.B) {
    decode_root<EZ>(p, norm_part, i);
    // the backup's stores (other lanes of this wave) complete before the walk reads them; the walk
    // runs on the same CU, so workgroup scope suffices (agent scope would write back the L2)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    traverse_lb_root<EZ>(q, i, s_z0, epoch, players);
  }
  traverse_lb_finish(q, epoch);
}


// ---- Gumbel MuZero tree (lzm_gumbel.h): one wave per root, four roots per 256-thread workgroup ----
// root index of this wave, in a scalar register: every loop bound and readlane index below is wave-uniform
__device__ __forceinline__ int gumbel_wave_root() {
  return __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
}

__global__ __launch_bounds__(256) void gumbel_traverse_kernel(GumbelTraverseArgs q) {
  const int i = gumbel_wave_root();
  if (i < q.t.B) gumbel_traverse_root(q, i);
}

// CNode::expand (cnode.cpp:94-156, raw_value :111) + cback_propagate (:605-631) of root i's leaf
__device__ inline void gumbel_expand_backup(const TreeView &t, float *raw, float4 *minmax, int i, int to_play, int cur,
                                            float reward, float value, const float *logits, float disc) {
  const int len = t.pathlen[i];
  const int leaf = t.path[(size_t)len * t.B + i];
  expand_wave(t, i, leaf, to_play, cur, reward, logits);
  if ((threadIdx.x & 63) == 0) raw[nidx(t, leaf, i)] = value;
  backup_wave(t, i, i, t.B, minmax + i, -1, value, disc);  // no player sign (:617-630)
}

// cbatch_back_propagate (:633-652) from raw lists
__global__ __launch_bounds__(256) void gumbel_backprop_kernel(BackpropArgs p, GumbelView g) {
  const int i = gumbel_wave_root();
  if (i >= p.t.B) return;
  gumbel_expand_backup(p.t, g.raw, p.minmax, i, p.to_play[i], p.cur, p.rewards[i], p.values[i],
                       p.logits + (size_t)i * p.t.A, p.disc);
}

// decode + expand + backup of one simulation (decode_root's Gumbel form) and, with TRAVERSE, the next
// simulation's walk by the same wave over the records it has just written
template <bool TRAVERSE>
__global__ __launch_bounds__(256) void gumbel_decode_kernel(DecodeArgs p, const int32_t *norm_part, GumbelTraverseArgs q) {
  const int i = gumbel_wave_root();
  if (i >= p.t.B) return;
  float r, v;
  decode_heads(p, norm_part, i, &r, &v);
  gumbel_expand_backup(p.t, q.g.raw, p.minmax, i, p.to_play[i], p.cur, r, v, p.policy_logits + (size_t)i * p.t.A, p.disc);
  if (TRAVERSE) {
    // the backup's stores (other lanes of this wave) complete before the walk reads them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    gumbel_traverse_root(q, i);
  }
}

__global__ __launch_bounds__(256) void gumbel_output_kernel(TreeView t, GumbelView g, float disc, int policy, float *out) {
  const int i = gumbel_wave_root();
  if (i < t.B) gumbel_root_output(t, g, i, disc, policy, out);
}

// the root outputs of one collect step (gumbel_collect_output) and, with `count`, the step counter's increment
__global__ __launch_bounds__(256) void gumbel_collect_kernel(TreeView t, GumbelView g, float disc, GumbelCollectOut o,
                                                             int64_t *count) {
  const int i = gumbel_wave_root();
  if (i < t.B) gumbel_collect_output(t, g, i, disc, o);
  if (count && blockIdx.x == 0 && threadIdx.x == 0) *count += 1;
}

__global__ void debug_logf_kernel(const float *x, float *out, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = glibc_logf(x[i]);
}

}  // namespace lzm

// ============================================================================ host side
using namespace lzm;

static thread_local char g_err[512];
constexpr int kErrWords = 8;  // sticky error words per handle (lzm_check_errors)
static void set_err(const char *msg) { snprintf(g_err, sizeof(g_err), "%s", msg); }
#define LZM_HIP(call)                                                                              \
  do {                                                                                             \
    hipError_t e_ = (call);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      snprintf(g_err, sizeof(g_err), "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
      return LZM_ERR_HIP;                                                                          \
    }                                                                                              \
  } while (0)
#define LZM_CHECK_LAUNCH() LZM_HIP(hipGetLastError())

// Compute units of the CURRENT device, cached per device ordinal (a process may drive several GPUs,
// or switch devices between calls: a process-wide static would keep the first device's count).
static int device_cus() {
  static int cache[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return 256;
  if (dev >= 64) {
    int n = 0;
    return hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
  }
  if (!cache[dev]) {
    int n = 0;
    cache[dev] = hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0 ? n : 256;
  }
  return cache[dev];
}

struct lzm_handle {
  int B, A, flags, sims_cap, cap, depth_cap;
  NodeStat *stat = nullptr;
  NodeMeta *meta = nullptr;
  int32_t *legal = nullptr, *nlegal = nullptr, *path = nullptr, *path_act = nullptr, *pathlen = nullptr;
  int32_t *norm_flag = nullptr;
  int32_t *err = nullptr;  // [kErrWords] sticky error counters (lzm_check_errors)
  float2 *lut = nullptr;
  int lut_n = 0;
  int lut_base = -1;
  float lut_init = -1.0f;
  // fused whole-search state (lzm_search_mlp)
  uint32_t *coef = nullptr;  // [coef_positions][31] glibc draw coefficients
  int coef_positions = 0;
  uint32_t *pow16807 = nullptr;            // [31]
  unsigned long long *lb_flags = nullptr;  // [flag_sims][G] look-back words
  int flag_sims = 0;
  uint32_t *epoch = nullptr;               // [2] launch epoch, done counter
  int32_t *search_diag = nullptr;          // [4]
  // collect-step mode of the fused search (lzm_search_set_step)
  int64_t *step_count = nullptr;
  int step_inc = 0;
  long long step_base = 0;
  int step_fresh = 0;
  float step_delta = 0.0f;
  int32_t *step_dist = nullptr;
  float *step_vals = nullptr;
  int32_t *step_seeds = nullptr;  // [sims] the weight-streaming path's staged seeds
  int step_seeds_n = 0;
  unsigned long long *phase = nullptr;     // [64] diagnostic phase cycles (LZM_PHASE_TIMING=1)
  const int32_t *ext_norm = nullptr;       // lzm_set_norm_words: verdict words written by lzm_conv_heads
  int value_support = 0;                   // lzm_set_value_support: the value rows' length when it differs (0: same)
  const int32_t *reuse_action = nullptr;   // lzm_set_reuse: search-with-reuse inputs (device, [B])
  const float *reuse_value = nullptr;
  // lzm_search_conv_ez's hand-off workspace (LSTM input rows, outputs, split-K partials, flags)
  void *ez_ws = nullptr;
  size_t ez_ws_bytes = 0;
  // Gumbel MuZero handles (LZM_TREE_GUMBEL) only
  float *raw = nullptr;           // [cap][B] raw_value per node
  float *gumbel = nullptr;        // [64] the fixed Gumbel table
  int32_t *considered = nullptr;  // [cons_cap] considered-visits row of (cons_m, cons_S)
  int cons_cap = 0, cons_m = -1, cons_S = -1;
};

static TreeView view(lzm_handle *h) {
  TreeView t;
  t.stat = h->stat;
  t.meta = h->meta;
  t.legal = h->legal;
  t.nlegal = h->nlegal;
  t.path = h->path;
  t.path_act = h->path_act;
  t.pathlen = h->pathlen;
  t.lut = h->lut;
  t.B = h->B;
  t.A = h->A;
  t.cap = h->cap;
  t.lut_n = h->lut_n;
  t.depth_cap = h->depth_cap;
  return t;
}

static void dfree(void *p) {
  if (p) (void)hipFree(p);
}

static void free_tree(lzm_handle *h) {
  dfree(h->stat); dfree(h->meta); dfree(h->path); dfree(h->path_act); dfree(h->lut);
  dfree(h->step_seeds); dfree(h->raw);
  h->stat = nullptr; h->meta = nullptr; h->path = nullptr; h->path_act = nullptr; h->lut = nullptr;
  h->step_seeds = nullptr; h->raw = nullptr;
  h->step_seeds_n = 0;
}

// pb_c table over the integer parent count N = visit-1 (cucb_score, cnode.cpp:673-674):
// {logf(((N + base) + 1) / base) + init, sqrtf(N)} with the host libm, -ffp-contract=off.
static int fill_lut(lzm_handle *h, int base, float init) {
  if (h->lut_base == base && h->lut_init == init) return LZM_OK;
  std::vector<float2> lut(h->lut_n);
  const float fb = (float)base;
  for (int n = 0; n < h->lut_n; ++n) {
    volatile float N = (float)n;
    volatile float num = N + fb;
    num = num + 1;
    volatile float q = num / fb;
    float pbc = logf(q) + init;
    lut[n] = make_float2(pbc, sqrtf(N));
  }
  LZM_HIP(hipMemcpy(h->lut, lut.data(), sizeof(float2) * h->lut_n, hipMemcpyHostToDevice));
  h->lut_base = base;
  h->lut_init = init;
  return LZM_OK;
}

// The parity-mode draw table [positions][31]: row p holds the coefficients of z[344 + p] (the p-th rand()
// output before >> 1) over the 31 seeded words (random_r is linear over Z/2^32: z[n] = z[n-31] + z[n-3]).
static std::vector<uint32_t> glibc_coef_table(int positions) {
  std::vector<uint32_t> tab((size_t)positions * 31);
  std::vector<uint32_t> ring((size_t)34 * 31, 0u);  // z[n] for n mod 34
  auto row = [&](long n) { return &ring[(size_t)(n % 34) * 31]; };
  for (int j = 0; j < 31; ++j) {
    uint32_t *r = row(j);
    for (int c = 0; c < 31; ++c) r[c] = (c == j);
  }
  for (int j = 31; j < 34; ++j) memcpy(row(j), row(j - 31), 31 * sizeof(uint32_t));
  const long last = 344L + positions;
  for (long n = 34; n < last; ++n) {
    uint32_t tmp[31];
    const uint32_t *a = row(n - 31), *b = row(n - 3);
    for (int c = 0; c < 31; ++c) tmp[c] = a[c] + b[c];
    memcpy(row(n), tmp, sizeof(tmp));
    if (n >= 344) memcpy(&tab[(size_t)(n - 344) * 31], tmp, sizeof(tmp));
  }
  return tab;
}

// 16807^i mod (2^31 - 1), i < 31: srandom_r's state from a seed in one multiply each (seed_state_parallel)
static void glibc_pow16807(uint32_t pw[31]) {
  unsigned long long x = 1;
  for (int i = 0; i < 31; ++i) {
    pw[i] = (uint32_t)x;
    x = (x * 16807ull) % 2147483647ull;
  }
}

namespace {
int ensure_coef(lzm_handle *h, int positions);
int ensure_flags(lzm_handle *h, int sims, int G);
}  // namespace

static int alloc_tree(lzm_handle *h, int sims) {
  h->sims_cap = sims;
  h->cap = 1 + h->A * (sims + 1);
  h->depth_cap = sims + 2;
  const size_t nodes = (size_t)h->cap * h->B;
  LZM_HIP(hipMalloc(&h->stat, nodes * sizeof(NodeStat)));
  LZM_HIP(hipMalloc(&h->meta, nodes * sizeof(NodeMeta)));
  LZM_HIP(hipMemset(h->meta, 0xff, nodes * sizeof(NodeMeta)));  // latent -1: nothing expanded
  LZM_HIP(hipMemset(h->stat, 0, nodes * sizeof(NodeStat)));
  if (h->flags & LZM_TREE_GUMBEL) {
    LZM_HIP(hipMalloc(&h->raw, nodes * sizeof(float)));
    LZM_HIP(hipMemset(h->raw, 0, nodes * sizeof(float)));
  }
  LZM_HIP(hipMalloc(&h->path, sizeof(int32_t) * (size_t)h->depth_cap * h->B));
  LZM_HIP(hipMalloc(&h->path_act, sizeof(int32_t) * (size_t)h->depth_cap * h->B));
  h->lut_n = sims + 8;
  LZM_HIP(hipMalloc(&h->lut, sizeof(float2) * h->lut_n));
  h->lut_base = -1;
  // the collect-step seeds of the weight-streaming search (lzm_search_set_step): sized with the
  // tree, so a captured step never allocates and a reserve (generation bump) retires graphs that
  // point at the old buffer together with the tree's
  LZM_HIP(hipMalloc(&h->step_seeds, sizeof(int32_t) * (size_t)(sims + 1)));
  h->step_seeds_n = sims + 1;
  if (!(h->flags & (LZM_RNG_FAST | LZM_TREE_GUMBEL))) {
    // parity-mode draw tables and look-back words, allocated here rather than at first use so
    // that a search captured into a HIP graph never allocates
    int rc = ensure_coef(h, h->B * h->depth_cap + 64);
    if (rc != LZM_OK) return rc;
    rc = ensure_flags(h, sims, h->B);
    if (rc != LZM_OK) return rc;
  }
  return fill_lut(h, 19652, 1.25f);
}

// ---- the generic search path's host side: one refusal / one builder per argument struct, shared by the
// plain (lzm_traverse, lzm_backprop, lzm_decode_backprop*) and the lzm_gumbel_* entry points. `name` is the
// public entry point, which every message starts with.
static int refuse(int code, const char *name, const char *what) {
  snprintf(g_err, sizeof(g_err), "%s: %s", name, what);
  return code;
}

// the handle is there and of the kind `name` serves (gumbel: an lzm_gumbel_* entry point)
static int check_kind(const char *name, const lzm_handle *h, bool gumbel) {
  if (!h) return refuse(LZM_ERR_ARG, name, gumbel ? "null handle" : "null argument");
  if (gumbel == ((h->flags & LZM_TREE_GUMBEL) != 0)) return LZM_OK;
  return refuse(LZM_ERR_STATE, name, gumbel ? "not a Gumbel MuZero handle (create it with LZM_TREE_GUMBEL)"
                                            : "a Gumbel MuZero handle takes the lzm_gumbel_* entry points");
}

static int check_cur(lzm_handle *h, int cur) {
  if (cur < 1 || 1 + h->A * (cur + 1) > h->cap) {
    snprintf(g_err, sizeof(g_err), "latent index %d outside reserved capacity (%d simulations)", cur, h->sims_cap);
    return LZM_ERR_CAPACITY;
  }
  return LZM_OK;
}

static WalkOut walk_out(int32_t *out_x, int32_t *out_y, int32_t *out_a, int64_t *out_a64, int32_t *out_vtp,
                        int32_t *out_len) {
  return WalkOut{out_x, out_y, out_a, out_vtp, out_len, (long long *)out_a64};
}
static bool walk_out_complete(const WalkOut &o) { return o.out_x && o.out_y && o.out_a && o.out_vtp && o.out_len; }

// The look-back traverse's arguments (lzm_traverse_lb.h) with the handle's draw table and look-back words.
static int traverse_lb_args(lzm_handle *h, float discount, const float *minmax, const uint32_t *seed,
                            const int32_t *vtp_in, const WalkOut &out, TraverseLbArgs *q) {
  int rc = ensure_coef(h, h->B * h->depth_cap + 64);
  if (rc != LZM_OK) return rc;
  rc = ensure_flags(h, 1, 1);
  if (rc != LZM_OK) return rc;
  q->t = view(h);
  q->minmax = (const float4 *)minmax;
  q->seed = seed;
  q->vtp_in = vtp_in;
  q->out = out;
  q->disc = discount;
  q->coef = h->coef; q->coef_positions = h->coef_positions; q->pow16807 = h->pow16807;
  q->flags = h->lb_flags; q->epoch = h->epoch; q->err = h->err;
  q->reuse_action = h->reuse_action; q->reuse_value = h->reuse_value;
  q->stamps = nullptr;
  return LZM_OK;
}

// One backup from raw lists: checks the lists and the latent index, fills BackpropArgs.
static int backprop_args(const char *name, lzm_handle *h, int cur, float discount, float *minmax, const float *rewards,
                         const float *values, const float *logits, const int32_t *to_play, const int32_t *is_reset,
                         const int32_t *reuse_action, const float *reuse_value, BackpropArgs *p) {
  if (!minmax || !rewards || !values || !logits || !to_play) return refuse(LZM_ERR_ARG, name, "null argument");
  const int rc = check_cur(h, cur);
  if (rc != LZM_OK) return rc;
  p->t = view(h);
  p->minmax = (float4 *)minmax;
  p->rewards = rewards; p->values = values; p->logits = logits; p->to_play = to_play; p->is_reset = is_reset;
  p->cur = cur;
  p->disc = discount;
  p->reuse_action = reuse_action; p->reuse_value = reuse_value;
  return LZM_OK;
}

static int launch_norm_check(int32_t *flag, const float *a, const float *b, int rows, int V, int Vb, hipStream_t s) {
  hipLaunchKernelGGL(normalized_check_kernel, dim3(norm_parts(rows)), dim3(256), 0, s, a, b, rows, V, Vb, flag);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// One support decode: checks the rows, the support lengths (the value rows' own length when
// lzm_set_value_support gave one) and the latent index, fills DecodeArgs and launches the ensure_softmax
// check unless lzm_conv_heads wrote the verdict words already (lzm_set_norm_words). *nf: the words the decode
// kernel reads. Nothing is launched when a check refuses.
static int decode_args(const char *name, lzm_handle *h, int cur, float discount, float *minmax,
                       const float *reward_logits, const float *value_logits, int support_len, int categorical,
                       const float *policy_logits, const int32_t *to_play, int horizon, int32_t *out_is_reset,
                       const float *next_latent, float *pool_slot, int64_t row_elems, float *out_decoded,
                       const int32_t *reuse_action, const float *reuse_value, hipStream_t s, DecodeArgs *p,
                       const int32_t **nf) {
  if (!minmax || !reward_logits || !value_logits || !policy_logits || !to_play || support_len <= 0)
    return refuse(LZM_ERR_ARG, name, "null argument");
  const int value_len = h->value_support > 0 ? h->value_support : support_len;
  if (categorical && (support_len % 2 == 0 || value_len % 2 == 0))
    return refuse(LZM_ERR_ARG, name, "categorical support length must be odd (2*support_scale+1)");
  int rc = check_cur(h, cur);
  if (rc != LZM_OK) return rc;
  if (categorical && !h->ext_norm) {
    rc = launch_norm_check(h->norm_flag, reward_logits, value_logits, h->B, support_len, value_len, s);
    if (rc != LZM_OK) return rc;
  }
  p->t = view(h);
  p->minmax = (float4 *)minmax;
  p->reward_logits = reward_logits; p->value_logits = value_logits; p->policy_logits = policy_logits;
  p->to_play = to_play; p->out_is_reset = out_is_reset; p->next_latent = next_latent; p->pool_slot = pool_slot;
  p->row_elems = row_elems; p->V = support_len; p->Vv = value_len; p->categorical = categorical; p->cur = cur;
  p->horizon = horizon;
  p->disc = discount; p->out_decoded = out_decoded;
  p->reuse_action = reuse_action; p->reuse_value = reuse_value;
  *nf = categorical ? (h->ext_norm ? h->ext_norm : h->norm_flag) : nullptr;
  return LZM_OK;
}

extern "C" {

const char *lzm_last_error(void) { return g_err; }

int lzm_create(int B, int A, int max_sims, int flags, lzm_handle **out) {
  if (!out || B <= 0 || A <= 0 || A > kMaxActions || max_sims < 0) {
    set_err("lzm_create: need num_roots > 0, 0 < action_space <= 64, max_sims >= 0");
    return LZM_ERR_ARG;
  }
  if ((flags & LZM_TREE_GUMBEL) && (flags & LZM_TREE_EZ)) {
    set_err("lzm_create: LZM_TREE_GUMBEL and LZM_TREE_EZ are mutually exclusive");
    return LZM_ERR_ARG;
  }
  lzm_handle *h = new lzm_handle();
  h->B = B;
  h->A = A;
  h->flags = flags;
  int rc;
#define TRY(x) do { rc = (x); if (rc != LZM_OK) { lzm_destroy(h); return rc; } } while (0)
  TRY(hipMalloc(&h->legal, sizeof(int32_t) * (size_t)B * A) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
  TRY(hipMalloc(&h->nlegal, sizeof(int32_t) * B) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
  TRY(hipMalloc(&h->pathlen, sizeof(int32_t) * B) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
  TRY(hipMalloc(&h->err, sizeof(int32_t) * kErrWords) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
  TRY(hipMemset(h->err, 0, sizeof(int32_t) * kErrWords) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
  TRY(hipMalloc(&h->norm_flag, sizeof(int32_t) * 2 * norm_parts(B)) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
  TRY(hipMemset(h->pathlen, 0, sizeof(int32_t) * B) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
  if (flags & LZM_TREE_GUMBEL) {
    float tab[kMaxActions];
    lzm_gumbel_table(10.0f, kMaxActions, tab);  // CNode::CNode: gumbel_scale 10, gumbel_rng 0 (cnode.cpp:87-89)
    TRY(hipMalloc(&h->gumbel, sizeof(tab)) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
    TRY(hipMemcpy(h->gumbel, tab, sizeof(tab), hipMemcpyHostToDevice) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
    h->cons_cap = max_sims + 64;
    TRY(hipMalloc(&h->considered, sizeof(int32_t) * h->cons_cap) == hipSuccess ? LZM_OK : LZM_ERR_HIP);
  }
  TRY(alloc_tree(h, max_sims));
#undef TRY
  *out = h;
  return LZM_OK;
}

int lzm_destroy(lzm_handle *h) {
  if (!h) return LZM_OK;
  free_tree(h);
  dfree(h->legal); dfree(h->nlegal); dfree(h->pathlen); dfree(h->err); dfree(h->norm_flag);
  dfree(h->coef); dfree(h->pow16807); dfree(h->lb_flags); dfree(h->epoch); dfree(h->search_diag); dfree(h->phase);
  dfree(h->ez_ws); dfree(h->gumbel); dfree(h->considered);
  delete h;
  return LZM_OK;
}

// Grows the node pool, keeping the tree: node-major storage means the old pool is a prefix
// of the new one (same for the [level][root] path arrays). Synchronises the device.
int lzm_reserve(lzm_handle *h, int max_sims) {
  if (!h || max_sims < 0) return LZM_ERR_ARG;
  if (max_sims <= h->sims_cap) return LZM_OK;
  LZM_HIP(hipDeviceSynchronize());
  lzm_handle old = *h;
  h->stat = nullptr; h->meta = nullptr; h->path = nullptr; h->path_act = nullptr; h->lut = nullptr;
  h->step_seeds = nullptr; h->raw = nullptr;
  int rc = alloc_tree(h, max_sims);
  if (rc == LZM_OK) {
    const size_t nodes = (size_t)old.cap * old.B;
    LZM_HIP(hipMemcpy(h->stat, old.stat, nodes * sizeof(NodeStat), hipMemcpyDeviceToDevice));
    LZM_HIP(hipMemcpy(h->meta, old.meta, nodes * sizeof(NodeMeta), hipMemcpyDeviceToDevice));
    if (old.raw) LZM_HIP(hipMemcpy(h->raw, old.raw, nodes * sizeof(float), hipMemcpyDeviceToDevice));
    LZM_HIP(hipMemcpy(h->path, old.path, sizeof(int32_t) * (size_t)old.depth_cap * old.B, hipMemcpyDeviceToDevice));
    LZM_HIP(hipMemcpy(h->path_act, old.path_act, sizeof(int32_t) * (size_t)old.depth_cap * old.B, hipMemcpyDeviceToDevice));
    if (old.lut_base >= 0) rc = fill_lut(h, old.lut_base, old.lut_init);
  }
  free_tree(&old);
  return rc;
}

int lzm_set_pb_c(lzm_handle *h, int pb_c_base, float pb_c_init) {
  if (!h || pb_c_base <= 0) return LZM_ERR_ARG;
  return fill_lut(h, pb_c_base, pb_c_init);
}

int lzm_copy_tree(lzm_handle *dst, const lzm_handle *src, void *stream) {
  if (!dst || !src || dst->B != src->B || dst->A != src->A || dst->sims_cap < src->sims_cap ||
      ((dst->flags ^ src->flags) & LZM_TREE_GUMBEL)) {
    set_err("lzm_copy_tree: handles differ in shape or kind, or destination is smaller");
    return LZM_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  const size_t nodes = (size_t)src->cap * src->B;
  if (src->raw) LZM_HIP(hipMemcpyAsync(dst->raw, src->raw, nodes * sizeof(float), hipMemcpyDeviceToDevice, s));
  LZM_HIP(hipMemcpyAsync(dst->stat, src->stat, nodes * sizeof(NodeStat), hipMemcpyDeviceToDevice, s));
  LZM_HIP(hipMemcpyAsync(dst->meta, src->meta, nodes * sizeof(NodeMeta), hipMemcpyDeviceToDevice, s));
  LZM_HIP(hipMemcpyAsync(dst->legal, src->legal, sizeof(int32_t) * (size_t)src->B * src->A, hipMemcpyDeviceToDevice, s));
  LZM_HIP(hipMemcpyAsync(dst->nlegal, src->nlegal, sizeof(int32_t) * src->B, hipMemcpyDeviceToDevice, s));
  LZM_HIP(hipMemcpyAsync(dst->path, src->path, sizeof(int32_t) * (size_t)src->depth_cap * src->B, hipMemcpyDeviceToDevice, s));
  LZM_HIP(hipMemcpyAsync(dst->path_act, src->path_act, sizeof(int32_t) * (size_t)src->depth_cap * src->B, hipMemcpyDeviceToDevice, s));
  LZM_HIP(hipMemcpyAsync(dst->pathlen, src->pathlen, sizeof(int32_t) * src->B, hipMemcpyDeviceToDevice, s));
  return LZM_OK;
}

int lzm_num_roots(const lzm_handle *h) { return h ? h->B : LZM_ERR_ARG; }
int lzm_sims_capacity(const lzm_handle *h) { return h ? h->sims_cap : LZM_ERR_ARG; }
int lzm_action_space(const lzm_handle *h) { return h ? h->A : LZM_ERR_ARG; }
int lzm_flags(const lzm_handle *h) { return h ? h->flags : LZM_ERR_ARG; }

int lzm_minmax_init(float *mm, int n, float delta, void *stream) {
  if (!mm || n <= 0) return LZM_ERR_ARG;
  hipLaunchKernelGGL(minmax_init_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (float4 *)mm, n, delta);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_roots_prepare(lzm_handle *h, const int32_t *legal, const int32_t *count, const float *noises, float noise_weight,
                      const float *rewards, const float *logits, const int32_t *to_play, void *stream) {
  if (!h || !legal || !count || !rewards || !logits || !to_play) {
    set_err("lzm_roots_prepare: null argument");
    return LZM_ERR_ARG;
  }
  PrepareArgs p;
  p.stat = h->stat; p.meta = h->meta; p.legal = h->legal; p.nlegal = h->nlegal;
  p.legal_in = legal; p.count_in = count; p.to_play = to_play; p.noises = noises; p.rewards = rewards;
  p.logits = logits; p.noise_weight = noise_weight; p.B = h->B; p.A = h->A;
  hipLaunchKernelGGL(prepare_kernel, dim3((h->B + 255) / 256), dim3(256), 0, (hipStream_t)stream, p);
  LZM_CHECK_LAUNCH();
  // Gumbel handles: the roots' raw_value starts at 0 until lzm_gumbel_set_root_values stores the value pool
  if (h->raw) LZM_HIP(hipMemsetAsync(h->raw, 0, sizeof(float) * h->B, (hipStream_t)stream));
  return LZM_OK;
}

int lzm_traverse(lzm_handle *h, int pb_c_base, float pb_c_init, float discount, float *minmax, const uint32_t *seed,
                 const int32_t *vtp_in, int32_t *out_x, int32_t *out_y, int32_t *out_a, int64_t *out_a64,
                 int32_t *out_vtp, int32_t *out_len, void *stream) {
  const char *name = "lzm_traverse";
  int rc = check_kind(name, h, false);
  if (rc != LZM_OK) return rc;
  const WalkOut out = walk_out(out_x, out_y, out_a, out_a64, out_vtp, out_len);
  if (!minmax || !seed || !vtp_in || !walk_out_complete(out)) return refuse(LZM_ERR_ARG, name, "null argument");
  if (pb_c_base <= 0) return refuse(LZM_ERR_ARG, name, "pb_c_base must be positive");
  if (h->reuse_action && (h->flags & LZM_RNG_FAST))
    return refuse(LZM_ERR_ARG, name, "search-with-reuse needs parity mode with the look-back traverse");
  rc = fill_lut(h, pb_c_base, pb_c_init);
  if (rc != LZM_OK) return rc;
  const bool ez = h->flags & LZM_TREE_EZ;
  hipStream_t s = (hipStream_t)stream;
  if (h->flags & LZM_RNG_FAST) {
    TraverseArgs p;
    p.t = view(h);
    p.minmax = (const float4 *)minmax;
    p.seed = seed;
    p.vtp_in = vtp_in;
    p.out = out;
    p.disc = discount;
    dim3 g((h->B + 255) / 256), b(256);
    if (ez) hipLaunchKernelGGL(traverse_fast_kernel<true>, g, b, 0, s, p);
    else hipLaunchKernelGGL(traverse_fast_kernel<false>, g, b, 0, s, p);
  } else {
    // one wave per root and workgroup, decoupled look-back of the draw offsets (lzm_traverse_lb.h)
    TraverseLbArgs q;
    rc = traverse_lb_args(h, discount, minmax, seed, vtp_in, out, &q);
    if (rc != LZM_OK) return rc;
    dim3 g(h->B), b(64);
    static const bool stamps = getenv("LZM_PHASE_TIMING") && atoi(getenv("LZM_PHASE_TIMING")) > 0;
    if (stamps) {  // diagnostic instantiation: per-phase cycles into phase[32..38] (lzm_debug_phase_cycles)
      if (!h->phase) {
        LZM_HIP(hipMalloc(&h->phase, (64 + 1024) * sizeof(unsigned long long)));
        LZM_HIP(hipMemset(h->phase, 0, (64 + 1024) * sizeof(unsigned long long)));
      }
      q.stamps = h->phase;
      if (ez) hipLaunchKernelGGL((traverse_lookback_kernel<true, true>), g, b, 0, s, q);
      else hipLaunchKernelGGL((traverse_lookback_kernel<false, true>), g, b, 0, s, q);
    } else {
      if (ez) hipLaunchKernelGGL(traverse_lookback_kernel<true>, g, b, 0, s, q);
      else hipLaunchKernelGGL(traverse_lookback_kernel<false>, g, b, 0, s, q);
    }
  }
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_gather_latent(lzm_handle *h, const float *pool, int64_t row, const int32_t *x, float *out, void *stream) {
  if (!h || !pool || !x || !out || row <= 0) return LZM_ERR_ARG;
  const long long total = (long long)h->B * row;
  hipStream_t s = (hipStream_t)stream;
  if (row % 4 == 0 && ((uintptr_t)pool % 16 == 0) && ((uintptr_t)out % 16 == 0)) {
    const long long t4 = total / 4;
    int grid = (int)((t4 + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(gather_kernel_v4, dim3(grid), dim3(256), 0, s, (const float4 *)pool, (long long)(row / 4), h->B, x,
                       (float4 *)out);
  } else {
    int grid = (int)((total + 255) / 256);
    if (grid > 4096) grid = 4096;
    hipLaunchKernelGGL(gather_kernel, dim3(grid), dim3(256), 0, s, pool, (long long)row, h->B, x, out);
  }
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_backprop(lzm_handle *h, int cur, float discount, float *minmax, const float *rewards, const float *values,
                 const float *logits, const int32_t *to_play, const int32_t *is_reset, void *stream) {
  const char *name = "lzm_backprop";
  int rc = check_kind(name, h, false);
  if (rc != LZM_OK) return rc;
  BackpropArgs p;
  rc = backprop_args(name, h, cur, discount, minmax, rewards, values, logits, to_play, is_reset, h->reuse_action,
                     h->reuse_value, &p);
  if (rc != LZM_OK) return rc;
  dim3 g((h->B + 255) / 256), b(256);
  if (h->flags & LZM_TREE_EZ) hipLaunchKernelGGL(backprop_kernel<true>, g, b, 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(backprop_kernel<false>, g, b, 0, (hipStream_t)stream, p);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_decode_backprop(lzm_handle *h, int cur, float discount, float *minmax, const float *reward_logits,
                        const float *value_logits, int support_len, int categorical, const float *policy_logits,
                        const int32_t *to_play, int lstm_horizon, int32_t *out_is_reset, const float *next_latent,
                        float *pool_slot, int64_t row_elems, float *out_decoded, void *stream) {
  const char *name = "lzm_decode_backprop";
  int rc = check_kind(name, h, false);
  if (rc != LZM_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  DecodeArgs p;
  const int32_t *nf;
  rc = decode_args(name, h, cur, discount, minmax, reward_logits, value_logits, support_len, categorical, policy_logits,
                   to_play, lstm_horizon, out_is_reset, next_latent, pool_slot, row_elems, out_decoded, h->reuse_action,
                   h->reuse_value, s, &p, &nf);
  if (rc != LZM_OK) return rc;
  dim3 g((h->B * 64 + 255) / 256), b(256);
  if (h->flags & LZM_TREE_EZ) hipLaunchKernelGGL(decode_backprop_kernel<true>, g, b, 0, s, p, nf);
  else hipLaunchKernelGGL(decode_backprop_kernel<false>, g, b, 0, s, p, nf);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_decode_backprop_traverse(lzm_handle *h, int cur, float discount, float *minmax, const float *reward_logits,
                                 const float *value_logits, int support_len, int categorical,
                                 const float *policy_logits, const int32_t *to_play, int lstm_horizon,
                                 int32_t *out_is_reset, const float *next_latent, float *pool_slot, int64_t row_elems,
                                 float *out_decoded, int pb_c_base, float pb_c_init, const uint32_t *seed,
                                 const int32_t *vtp_in, int32_t *out_x, int32_t *out_y, int32_t *out_a,
                                 int64_t *out_a64, int32_t *out_vtp, int32_t *out_len, void *stream) {
  const char *name = "lzm_decode_backprop_traverse";
  int rc = check_kind(name, h, false);
  if (rc != LZM_OK) return rc;
  const WalkOut out = walk_out(out_x, out_y, out_a, out_a64, out_vtp, out_len);
  if (!seed || !vtp_in || !walk_out_complete(out)) return refuse(LZM_ERR_ARG, name, "null argument");
  if (pb_c_base <= 0) return refuse(LZM_ERR_ARG, name, "pb_c_base must be positive");
  if (h->flags & LZM_RNG_FAST)
    return refuse(LZM_ERR_ARG, name, "parity (glibc) mode only; use lzm_decode_backprop + lzm_traverse");
  // the host tables first (synchronous copies when they change), then the decode's checks and its launch
  rc = fill_lut(h, pb_c_base, pb_c_init);
  if (rc != LZM_OK) return rc;
  TraverseLbArgs q;
  rc = traverse_lb_args(h, discount, minmax, seed, vtp_in, out, &q);
  if (rc != LZM_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  DecodeArgs p;
  const int32_t *nf;
  rc = decode_args(name, h, cur, discount, minmax, reward_logits, value_logits, support_len, categorical, policy_logits,
                   to_play, lstm_horizon, out_is_reset, next_latent, pool_slot, row_elems, out_decoded, h->reuse_action,
                   h->reuse_value, s, &p, &nf);
  if (rc != LZM_OK) return rc;
  const int per = kTlbThreads / 64;
  dim3 g((h->B + per - 1) / per), b(kTlbThreads);
  if (h->flags & LZM_TREE_EZ) hipLaunchKernelGGL(decode_traverse_kernel<true>, g, b, 0, s, p, nf, q);
  else hipLaunchKernelGGL(decode_traverse_kernel<false>, g, b, 0, s, p, nf, q);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

static int32_t *g_scratch_flag = nullptr;
static int g_scratch_parts = 0;
static uint32_t *g_debug_coef = nullptr;  // lzm_debug_glibc_rand: [positions][31] draw table, [31] powers, overflow word
static int g_debug_positions = 0;
static std::mutex g_scratch_mu;

int lzm_inverse_scalar_transform(const float *logits, int rows, int V, int categorical, float *out, void *stream) {
  if (!logits || !out || rows <= 0 || V <= 0) return LZM_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    if (g_scratch_parts < norm_parts(rows)) {
      // (grows only outside graph capture in practice: the first call sizes it)
      if (g_scratch_flag) LZM_HIP(hipFree(g_scratch_flag));
      g_scratch_flag = nullptr;
      LZM_HIP(hipMalloc(&g_scratch_flag, sizeof(int32_t) * 2 * norm_parts(rows)));
      g_scratch_parts = norm_parts(rows);
    }
  }
  if (categorical)
    hipLaunchKernelGGL(normalized_check_kernel, dim3(norm_parts(rows)), dim3(256), 0, s, logits, logits, rows, V, V,
                       g_scratch_flag);
  hipLaunchKernelGGL(inverse_transform_kernel, dim3((rows * 64 + 255) / 256), dim3(256), 0, s, logits, rows, V,
                     categorical, g_scratch_flag, out);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_get_distributions(lzm_handle *h, int32_t *out, void *stream) {
  if (!h || !out) return LZM_ERR_ARG;
  hipLaunchKernelGGL(distributions_kernel, dim3((h->B + 255) / 256), dim3(256), 0, (hipStream_t)stream, view(h), out);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_get_values(lzm_handle *h, float *out, void *stream) {
  if (!h || !out) return LZM_ERR_ARG;
  hipLaunchKernelGGL(values_kernel, dim3((h->B + 255) / 256), dim3(256), 0, (hipStream_t)stream, view(h), out);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_get_trajectories(lzm_handle *h, int32_t *out, int tmax, void *stream) {
  if (!h || !out || tmax <= 0) return LZM_ERR_ARG;
  hipLaunchKernelGGL(trajectories_kernel, dim3((h->B + 255) / 256), dim3(256), 0, (hipStream_t)stream, view(h), out,
                     tmax);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// ---- Gumbel MuZero tree (ctree_gumbel_muzero/lib/cnode.cpp) ---------------------------------------------
// generate_gumbel (cnode.cpp:1134-1152) with gumbel_rng = 0: std::mt19937(0) through
// std::extreme_value_distribution<float>(0, 1), scaled. Host only.
int lzm_gumbel_table(float scale, int n, float *out) {
  if (!out || n < 0) return LZM_ERR_ARG;
  std::mt19937 gen(0u);
  std::extreme_value_distribution<float> d(0, 1);
  for (int i = 0; i < n; ++i) out[i] = scale * d(gen);
  return LZM_OK;
}

// The row of get_table_of_considered_visits (cnode.cpp:1079-1095) that cselect_root_child reads (:727-729):
// get_sequence_of_considered_visits (:1042-1077) for min(m, S) considered actions over S simulations. Host only.
int lzm_gumbel_considered_visits(int max_num_considered_actions, int num_simulations, int32_t *out) {
  const int S = num_simulations;
  if (!out || S < 1 || max_num_considered_actions < 0) return LZM_ERR_ARG;
  const int m = max_num_considered_actions < S ? max_num_considered_actions : S;
  if (m <= 1) {
    for (int i = 0; i < S; ++i) out[i] = i;
    return LZM_OK;
  }
  int log2max = 0;  // ceil(log2(m))
  while ((1 << log2max) < m) ++log2max;
  std::vector<int> visits(m, 0);
  int filled = 0, considered = m;
  while (filled < S) {
    int extra = S / (log2max * considered);
    if (extra < 1) extra = 1;
    for (int e = 0; e < extra; ++e) {
      for (int j = 0; j < considered && filled < S; ++j) out[filled++] = visits[j];
      for (int j = 0; j < considered; ++j) visits[j] += 1;
    }
    considered = considered / 2 > 2 ? considered / 2 : 2;
  }
  return LZM_OK;
}
}  // extern "C"

static GumbelView gumbel_view(lzm_handle *h) {
  GumbelView g;
  g.raw = h->raw;
  g.gumbel = h->gumbel;
  g.considered = h->considered;
  g.S = h->cons_S;
  return g;
}

// the device considered-visits row for (m, S): rebuilt (synchronous copy, outside stream capture) when they change
static int gumbel_set_considered(lzm_handle *h, int S, int m, const char *name) {
  if (S < 1 || m < 0) {
    snprintf(g_err, sizeof(g_err), "%s: need num_simulations >= 1 and max_num_considered_actions >= 0", name);
    return LZM_ERR_ARG;
  }
  if (h->cons_m == m && h->cons_S == S) return LZM_OK;
  std::vector<int32_t> row(S);
  lzm_gumbel_considered_visits(m, S, row.data());
  if (S > h->cons_cap) {
    LZM_HIP(hipDeviceSynchronize());
    dfree(h->considered);
    h->considered = nullptr;
    h->cons_cap = 0;
    LZM_HIP(hipMalloc(&h->considered, sizeof(int32_t) * (size_t)(S + 64)));
    h->cons_cap = S + 64;
  }
  LZM_HIP(hipMemcpy(h->considered, row.data(), sizeof(int32_t) * S, hipMemcpyHostToDevice));
  h->cons_m = m;
  h->cons_S = S;
  return LZM_OK;
}

static GumbelTraverseArgs gumbel_traverse_args(lzm_handle *h, float discount, const int32_t *vtp_in,
                                               const WalkOut &out) {
  GumbelTraverseArgs q;
  q.t = view(h);
  q.g = gumbel_view(h);
  q.vtp_in = vtp_in;
  q.out = out;
  q.disc = discount;
  return q;
}

static dim3 gumbel_grid(const lzm_handle *h) { return dim3((h->B + 3) / 4); }

// gumbel_decode_kernel for one simulation; with_traverse: q carries the next walk's request lists
static int gumbel_decode_launch(const char *name, bool with_traverse, lzm_handle *h, int cur, float discount,
                                float *minmax, const float *reward_logits, const float *value_logits, int support_len,
                                int categorical, const float *policy_logits, const int32_t *to_play,
                                const float *next_latent, float *pool_slot, int64_t row_elems, float *out_decoded,
                                const GumbelTraverseArgs &q, hipStream_t s) {
  DecodeArgs p;
  const int32_t *nf;
  const int rc = decode_args(name, h, cur, discount, minmax, reward_logits, value_logits, support_len, categorical,
                             policy_logits, to_play, 0, nullptr, next_latent, pool_slot, row_elems, out_decoded, nullptr,
                             nullptr, s, &p, &nf);
  if (rc != LZM_OK) return rc;
  if (with_traverse) hipLaunchKernelGGL(gumbel_decode_kernel<true>, gumbel_grid(h), dim3(256), 0, s, p, nf, q);
  else hipLaunchKernelGGL(gumbel_decode_kernel<false>, gumbel_grid(h), dim3(256), 0, s, p, nf, q);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

extern "C" {

int lzm_gumbel_set_considered(lzm_handle *h, int num_simulations, int max_num_considered_actions) {
  int rc = check_kind("lzm_gumbel_set_considered", h, true);
  if (rc != LZM_OK) return rc;
  return gumbel_set_considered(h, num_simulations, max_num_considered_actions, "lzm_gumbel_set_considered");
}

int lzm_gumbel_set_root_values(lzm_handle *h, const float *values, void *stream) {
  int rc = check_kind("lzm_gumbel_set_root_values", h, true);
  if (rc != LZM_OK) return rc;
  if (!values) return LZM_ERR_ARG;
  // node 0's row of raw[cap][B]
  LZM_HIP(hipMemcpyAsync(h->raw, values, sizeof(float) * h->B, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LZM_OK;
}

int lzm_gumbel_traverse(lzm_handle *h, int num_simulations, int max_num_considered_actions, float discount,
                        const int32_t *vtp_in, int32_t *out_x, int32_t *out_y, int32_t *out_a, int64_t *out_a64,
                        int32_t *out_vtp, int32_t *out_len, void *stream) {
  const char *name = "lzm_gumbel_traverse";
  int rc = check_kind(name, h, true);
  if (rc != LZM_OK) return rc;
  const WalkOut out = walk_out(out_x, out_y, out_a, out_a64, out_vtp, out_len);
  if (!vtp_in || !walk_out_complete(out)) return refuse(LZM_ERR_ARG, name, "null argument");
  rc = gumbel_set_considered(h, num_simulations, max_num_considered_actions, name);
  if (rc != LZM_OK) return rc;
  const GumbelTraverseArgs q = gumbel_traverse_args(h, discount, vtp_in, out);
  hipLaunchKernelGGL(gumbel_traverse_kernel, gumbel_grid(h), dim3(256), 0, (hipStream_t)stream, q);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_gumbel_backprop(lzm_handle *h, int cur, float discount, float *minmax, const float *rewards, const float *values,
                        const float *logits, const int32_t *to_play, void *stream) {
  const char *name = "lzm_gumbel_backprop";
  int rc = check_kind(name, h, true);
  if (rc != LZM_OK) return rc;
  BackpropArgs p;
  rc = backprop_args(name, h, cur, discount, minmax, rewards, values, logits, to_play, nullptr, nullptr, nullptr, &p);
  if (rc != LZM_OK) return rc;
  hipLaunchKernelGGL(gumbel_backprop_kernel, gumbel_grid(h), dim3(256), 0, (hipStream_t)stream, p, gumbel_view(h));
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_gumbel_decode_backprop(lzm_handle *h, int cur, float discount, float *minmax, const float *reward_logits,
                               const float *value_logits, int support_len, int categorical, const float *policy_logits,
                               const int32_t *to_play, const float *next_latent, float *pool_slot, int64_t row_elems,
                               float *out_decoded, void *stream) {
  const char *name = "lzm_gumbel_decode_backprop";
  int rc = check_kind(name, h, true);
  if (rc != LZM_OK) return rc;
  const GumbelTraverseArgs q = gumbel_traverse_args(h, discount, nullptr, WalkOut{});
  return gumbel_decode_launch(name, false, h, cur, discount, minmax, reward_logits, value_logits, support_len,
                              categorical, policy_logits, to_play, next_latent, pool_slot, row_elems, out_decoded, q,
                              (hipStream_t)stream);
}

int lzm_gumbel_decode_backprop_traverse(lzm_handle *h, int cur, float discount, float *minmax,
                                        const float *reward_logits, const float *value_logits, int support_len,
                                        int categorical, const float *policy_logits, const int32_t *to_play,
                                        const float *next_latent, float *pool_slot, int64_t row_elems,
                                        float *out_decoded, int num_simulations, int max_num_considered_actions,
                                        const int32_t *vtp_in, int32_t *out_x, int32_t *out_y, int32_t *out_a,
                                        int64_t *out_a64, int32_t *out_vtp, int32_t *out_len, void *stream) {
  const char *name = "lzm_gumbel_decode_backprop_traverse";
  int rc = check_kind(name, h, true);
  if (rc != LZM_OK) return rc;
  const WalkOut out = walk_out(out_x, out_y, out_a, out_a64, out_vtp, out_len);
  if (!vtp_in || !walk_out_complete(out)) return refuse(LZM_ERR_ARG, name, "null argument");
  rc = gumbel_set_considered(h, num_simulations, max_num_considered_actions, name);
  if (rc != LZM_OK) return rc;
  const GumbelTraverseArgs q = gumbel_traverse_args(h, discount, vtp_in, out);
  return gumbel_decode_launch(name, true, h, cur, discount, minmax, reward_logits, value_logits, support_len,
                              categorical, policy_logits, to_play, next_latent, pool_slot, row_elems, out_decoded, q,
                              (hipStream_t)stream);
}

static int gumbel_output(const char *name, lzm_handle *h, float discount, int policy, float *out, void *stream) {
  int rc = check_kind(name, h, true);
  if (rc != LZM_OK) return rc;
  if (!out) return LZM_ERR_ARG;
  hipLaunchKernelGGL(gumbel_output_kernel, gumbel_grid(h), dim3(256), 0, (hipStream_t)stream, view(h), gumbel_view(h),
                     discount, policy, out);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_gumbel_get_children_values(lzm_handle *h, float discount, float *out, void *stream) {
  return gumbel_output("lzm_gumbel_get_children_values", h, discount, 0, out, stream);
}

int lzm_gumbel_get_policies(lzm_handle *h, float discount, float *out, void *stream) {
  return gumbel_output("lzm_gumbel_get_policies", h, discount, 1, out, stream);
}

int lzm_gumbel_collect_outputs(lzm_handle *h, float discount, int32_t *dist, float *values, float *completed_q,
                               float *policy, int32_t *action, int64_t *count, void *stream) {
  const char *name = "lzm_gumbel_collect_outputs";
  int rc = check_kind(name, h, true);
  if (rc != LZM_OK) return rc;
  if (!dist || !values || !completed_q || !policy || !action) return refuse(LZM_ERR_ARG, name, "null argument");
  GumbelCollectOut o;
  o.dist = dist; o.values = values; o.cq = completed_q; o.policy = policy; o.action = action;
  hipLaunchKernelGGL(gumbel_collect_kernel, gumbel_grid(h), dim3(256), 0, (hipStream_t)stream, view(h), gumbel_view(h),
                     discount, o, count);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_debug_logf(const float *x, float *out, int64_t n, void *stream) {
  if (!x || !out || n <= 0) return LZM_ERR_ARG;
  hipLaunchKernelGGL(debug_logf_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, out,
                     (long long)n);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_debug_expf(const float *x, float *out, int64_t n, void *stream) {
  if (!x || !out || n <= 0) return LZM_ERR_ARG;
  long long grid = (n + 255) / 256;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(debug_expf_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, out, (long long)n);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_debug_div_small(const float *x, const int32_t *d, float *out, int64_t n, void *stream) {
  if (!x || !d || !out || n <= 0) return LZM_ERR_ARG;
  long long grid = (n + 255) / 256;
  if (grid > 65536) grid = 65536;
  hipLaunchKernelGGL(debug_div_small_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, x, d, out,
                     (long long)n);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_debug_settle_chain(const float *tq, const int32_t *tv, int n_levels, float *out_q, void *stream) {
  if (!tq || !tv || !out_q || n_levels <= 0 || n_levels > 64) return LZM_ERR_ARG;
  hipLaunchKernelGGL(debug_settle_chain_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, tq, tv, n_levels, out_q);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_debug_philox(const uint32_t *ck, uint32_t *out, int n, void *stream) {
  if (!ck || !out || n <= 0) return LZM_ERR_ARG;
  hipLaunchKernelGGL(debug_philox_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, ck, out, n);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// Process teardown (lightzero_amd registers it with atexit, before the interpreter finalises): wait for the
// device, then free the library's process-wide device buffers while the HIP runtime (and a profiler's
// hooks) are still in place, instead of leaving them to the runtime's own exit-time teardown. Live handles
// are destroyed by their owners first (lzm_destroy).
int lzm_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_scratch_mu);
  LZM_HIP(hipDeviceSynchronize());
  if (g_scratch_flag) LZM_HIP(hipFree(g_scratch_flag));
  g_scratch_flag = nullptr;
  g_scratch_parts = 0;
  if (g_debug_coef) LZM_HIP(hipFree(g_debug_coef));
  g_debug_coef = nullptr;
  g_debug_positions = 0;
  return LZM_OK;
}

int lzm_debug_az_rules(int n, const int32_t *boards, const double *scores, int32_t *out, void *stream) {
  if (n <= 0 || !boards || !scores || !out) return LZM_ERR_ARG;
  hipLaunchKernelGGL(debug_az_rules_kernel, dim3((n + 3) / 4), dim3(64), 0, (hipStream_t)stream, n, boards, scores, out);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_debug_xor(const float *in, float *out, void *stream) {
  if (!in || !out) return LZM_ERR_ARG;
  hipLaunchKernelGGL(debug_xor_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, in, out);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_debug_glibc_rand(uint32_t seed, int n, int form, int32_t *out, void *stream) {
  if (!out || n <= 0 || form < 0 || form > 2) return LZM_ERR_ARG;
  uint32_t *tab;
  size_t np;  // words of the table proper
  {
    std::lock_guard<std::mutex> lk(g_scratch_mu);
    if (g_debug_positions < n) {
      // ensure_coef's table and powers, for exactly n positions (synchronous; grows outside stream capture)
      std::vector<uint32_t> host = glibc_coef_table(n);
      host.resize((size_t)n * 31 + 32, 0u);  // + [31] powers, + the overflow word (stays 0: every p < n)
      glibc_pow16807(&host[(size_t)n * 31]);
      if (g_debug_coef) LZM_HIP(hipFree(g_debug_coef));
      g_debug_coef = nullptr;
      g_debug_positions = 0;
      LZM_HIP(hipMalloc(&g_debug_coef, host.size() * sizeof(uint32_t)));
      LZM_HIP(hipMemcpy(g_debug_coef, host.data(), host.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
      g_debug_positions = n;
    }
    tab = g_debug_coef;
    np = (size_t)g_debug_positions * 31;
  }
  hipLaunchKernelGGL(debug_glibc_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, seed, n, form, out,
                     tab, tab + np, (int32_t *)(tab + np + 31));
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

}  // extern "C"

// ------------------------- fused whole-search (MuZeroModelMLP and EfficientZeroModelMLP, reward LSTM in-kernel)
namespace {

// One packed layer (lightzero_amd/fused.py pack_muzero_mlp / pack_efficientzero_mlp): krows input rows in
// the packed (torch-transposed) layout, K = krows rounded up to kKC in the kernel's.
struct LayerShape {
  int krows, K, N;
};
// Kernel layers: the packed layers as the search kernel runs them. Two pairs are merged, each
// into one layer with columns [src0 | src1] over the same K: the value and policy head hiddens
// (fc_value_head[0] | fc_policy_head[0], same input) and the value and policy head outputs
// (fc_value_head[1] | fc_policy_head[1], inputs the two halves of that merged hidden) — fewer
// dependent steps per simulation, and fuller lanes.
struct KLayer {
  int src0, src1;  // packed layer indices (src1 < 0: single source)
  int K, N, N0;    // N0: columns taken from src0
};
// The packed MLP recurrent network of MuZeroModelMLP (Hl == 0) and EfficientZeroModelMLP (Hl > 0: the
// reward LSTM's width), the one description behind the packed sizes, the weight preparation, the plans and
// the schedule. Layers in packed order; the two fc_dynamics_2 layers are present with
// res_connection_in_dynamics, the LSTM gate layer — one dense layer over [x ; h_prev], columns in nn.LSTM
// order i, f, g, o — for EfficientZero, whose value-prefix head reads h1 (K = Hl) where MuZero's reward
// head reads the next latent (K = H).
constexpr int kMlpLayers = 13, kGateLayer = 4;
struct MlpNet {
  int H, Hl, A, F, V, res;
  LayerShape s[kMlpLayers];
  bool used[kMlpLayers];
  size_t pw[kMlpLayers], pb[kMlpLayers], packed_floats;  // float offsets (weights [krows][N], then bias [N])
  KLayer kl[kMlpLayers];
  int nk;
  size_t w_off[kMlpLayers], b_off[kMlpLayers], kernel_floats;  // kernel layout (16-B aligned) and its total
};
MlpNet mlp_net(int H, int Hl, int A, int F, int V, int res) {
  MlpNet n;
  n.H = H; n.Hl = Hl; n.A = A; n.F = F; n.V = V; n.res = res ? 1 : 0;
  const int Kr = Hl > 0 ? Hl : H;
  LayerShape *s = n.s;
  s[0] = {H + A, (H + A + kKC - 1) / kKC * kKC, H};  // fc_dynamics(_1)[0]: [latent; one-hot action]
  s[1] = {H, H, H};
  s[2] = {H, H, H};                 // fc_dynamics_2 (res_connection_in_dynamics)
  s[3] = {H, H, H};
  s[4] = {H + Hl, H + Hl, 4 * Hl};  // [weight_ih_l0 | weight_hh_l0], bias_ih_l0 + bias_hh_l0
  s[5] = {Kr, Kr, F};               // fc_reward_head
  s[6] = {F, F, V};
  s[7] = {H, H, H};                 // fc_prediction_common
  s[8] = {H, H, H};
  s[9] = {H, H, F};                 // fc_value_head
  s[10] = {F, F, V};
  s[11] = {H, H, F};                // fc_policy_head
  s[12] = {F, F, A};
  size_t off = 0;
  for (int l = 0; l < kMlpLayers; ++l) {
    n.used[l] = (l == 2 || l == 3) ? n.res != 0 : (l == kGateLayer ? Hl > 0 : true);
    n.pw[l] = n.pb[l] = off;
    if (!n.used[l]) continue;
    off += (size_t)s[l].krows * s[l].N;
    n.pb[l] = off;
    off += s[l].N;
  }
  n.packed_floats = off;
  n.nk = 0;
  for (int l = 0; l <= 8; ++l)
    if (n.used[l]) n.kl[n.nk++] = KLayer{l, -1, s[l].K, s[l].N, s[l].N};
  n.kl[n.nk++] = KLayer{9, 11, s[9].K, s[9].N + s[11].N, s[9].N};
  n.kl[n.nk++] = KLayer{10, 12, s[10].K, s[10].N + s[12].N, s[10].N};
  off = 0;
  for (int l = 0; l < n.nk; ++l) {
    n.w_off[l] = off;
    off += swz_floats(n.kl[l].K, n.kl[l].N);
    n.b_off[l] = off;
    off = (off + n.kl[l].N + 3) & ~(size_t)3;
  }
  n.kernel_floats = off;
  return n;
}

// kernel-layout float d <- packed (k, col): col < N0 from src0 [krows0][N0], else src1 [krows1][N - N0]
__global__ void mlp_swizzle_kernel(const float *src0, int krows0, const float *src1, int krows1, int K, int N, int N0,
                                   float *dst, size_t n) {
  const size_t d = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  int k, col;
  swz_source(K, N, d, &k, &col);
  float v = 0.0f;
  if (col < N0) {
    if (k < krows0) v = src0[(size_t)k * N0 + col];
  } else if (col < N) {
    if (k < krows1) v = src1[(size_t)k * (N - N0) + (col - N0)];
  }
  dst[d] = v;
}

// The handle's draw table (glibc_coef_table) for at least `positions` draws, and the 16807 powers.
int ensure_coef(lzm_handle *h, int positions) {
  if (h->coef_positions >= positions) return LZM_OK;
  const std::vector<uint32_t> tab = glibc_coef_table(positions);
  dfree(h->coef);
  h->coef = nullptr;
  LZM_HIP(hipMalloc(&h->coef, tab.size() * sizeof(uint32_t)));
  LZM_HIP(hipMemcpy(h->coef, tab.data(), tab.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
  h->coef_positions = positions;
  if (!h->pow16807) {
    uint32_t pw[31];
    glibc_pow16807(pw);
    LZM_HIP(hipMalloc(&h->pow16807, sizeof(pw)));
    LZM_HIP(hipMemcpy(h->pow16807, pw, sizeof(pw), hipMemcpyHostToDevice));
  }
  return LZM_OK;
}

int ensure_flags(lzm_handle *h, int sims, int G) {
  if (!h->epoch) {
    LZM_HIP(hipMalloc(&h->epoch, 2 * sizeof(uint32_t)));
    const uint32_t init[2] = {1u, 0u};
    LZM_HIP(hipMemcpy(h->epoch, init, sizeof(init), hipMemcpyHostToDevice));
    LZM_HIP(hipMalloc(&h->search_diag, 4 * sizeof(int32_t)));
    LZM_HIP(hipMemset(h->search_diag, 0, 4 * sizeof(int32_t)));
  }
  if (h->flag_sims >= sims) return LZM_OK;
  dfree(h->lb_flags);
  h->lb_flags = nullptr;
  const size_t n = (size_t)sims * std::max(G, h->B);  // any roots-per-workgroup choice fits
  LZM_HIP(hipMalloc(&h->lb_flags, n * sizeof(unsigned long long)));
  LZM_HIP(hipMemset(h->lb_flags, 0, n * sizeof(unsigned long long)));  // epoch 0 never matches
  h->flag_sims = sims;
  return LZM_OK;
}

// Roots per workgroup in the fused search: the smallest of 1, 2, 4, 8 that keeps the grid within
// one workgroup per CU (each simulation is a latency chain per workgroup, so spreading the batch
// over more CUs shortens it; fewer, fuller workgroups amortise each weight read over more rows).
// LZM_ROOTS_PER_WG overrides (experiments).
int roots_per_wg(int B) {
  const char *e = getenv("LZM_ROOTS_PER_WG");
  if (e) {
    const int r = atoi(e);
    if (r == 1 || r == 2 || r == 4 || r == 8) return r;
  }
  const int cus = device_cus();
  for (int r = 1; r < 8; r *= 2)
    if ((B + r - 1) / r <= cus) return r;
  return 8;
}

constexpr size_t kMaxLds = 160 * 1024 - 1024;

size_t round4(size_t x) { return (x + 3) & ~(size_t)3; }

// ---- shared by the four one-launch search families (MLP and conv, MuZero and EfficientZero)
// LZM_PHASE_TIMING > 0: the searches stamp their phases into the handle's phase buffer (diagnostics)
bool phase_timing() {
  const char *e = getenv("LZM_PHASE_TIMING");
  return e && atoi(e) > 0;
}
int ensure_phase(lzm_handle *h) {
  if (h->phase) return LZM_OK;
  LZM_HIP(hipMalloc(&h->phase, (64 + 1024) * sizeof(unsigned long long)));
  LZM_HIP(hipMemset(h->phase, 0, (64 + 1024) * sizeof(unsigned long long)));
  return LZM_OK;
}
// Before any one-launch search: the pb_c table, the parity-mode draw table, the look-back words (G: the
// launch's workgroups)
int search_preamble(lzm_handle *h, int pb_c_base, float pb_c_init, int S, int G) {
  int rc = fill_lut(h, pb_c_base, pb_c_init);
  if (rc != LZM_OK) return rc;
  if (!(h->flags & (LZM_RNG_FAST | LZM_TREE_GUMBEL))) {  // (the Gumbel walk draws nothing: no draw table)
    rc = ensure_coef(h, h->B * (S + 1) + 64);
    if (rc != LZM_OK) return rc;
  }
  return ensure_flags(h, S, G);
}
// The kernel arguments that SearchArgs and ConvSearchArgs name alike: the tree, the search, the draw tables,
// the look-back words and the record pointers
template <class Args>
void fill_common(Args &p, const lzm_handle *h, int S, float discount, const uint32_t *seeds, const int32_t *vtp_in,
                 float *minmax, float *pool, int32_t *rec_x, int32_t *rec_a, int32_t *rec_len, float *rec_decoded,
                 float *rec_logits) {
  p.stat = h->stat; p.meta = h->meta; p.legal = h->legal; p.nlegal = h->nlegal;
  p.path = h->path; p.path_act = h->path_act; p.pathlen = h->pathlen; p.lut = h->lut;
  p.B = h->B; p.A = h->A; p.cap = h->cap; p.lut_n = h->lut_n; p.depth_cap = h->depth_cap;
  p.S = S; p.disc = discount; p.seeds = seeds; p.vtp_in = vtp_in; p.minmax = (float4 *)minmax; p.pool = pool;
  p.coef = h->coef; p.coef_positions = h->coef_positions; p.pow16807 = h->pow16807;
  p.flags = h->lb_flags; p.epoch = h->epoch; p.fast = (h->flags & LZM_RNG_FAST) ? 1 : 0;
  p.rec_x = rec_x; p.rec_a = rec_a; p.rec_len = rec_len; p.rec_dec = rec_decoded; p.rec_logits = rec_logits;
}

// The recurrent network as a schedule of dense steps over the kernel layers (LDS activation
// buffers by float offset): fc_dynamics(_1) on [latent; one-hot] (+ latent residual),
// fc_dynamics_2, [EfficientZero: the gate layer on [x ; h_prev], the cell follows it in the kernel,]
// the reward head (decoded) on the next latent (EfficientZero: the value-prefix head on h1),
// fc_prediction_common, [value | policy] head hidden, [value | policy] head output: value decoded,
// policy logits [r][A] into X1 (muzero_model_mlp.py:179-204, :420-440; efficientzero_model_mlp.py:186-216,
// :452-468). Padded to an even length with an empty step (two weight-prefetch buffers alternate).
void build_schedule(SearchArgs &p, const MlpNet &net, const float *weights, int R) {
  const int x0 = (int)p.off_x0, x1 = (int)p.off_x1, x2 = (int)p.off_x2, nl = (int)p.off_n, hd = (int)p.off_h,
            lg = (int)p.off_logit, gx = (int)p.off_g, gt = (int)p.off_gates, hh = (int)p.off_hh;
  const int A = net.A, V = net.V, F = net.F, res = net.res;
  const bool gate = net.used[kGateLayer];
  int n = 0, l = 0;
  auto add = [&](int in, int out, int relu, int resid, int rowmajor, int ldout, int dec) -> StepRec & {
    const KLayer &k = net.kl[l];
    StepRec &q = p.sched[n++];
    q.w = weights + net.w_off[l];
    q.b = weights + net.b_off[l];
    q.K = k.K;
    q.N = k.N;
    q.wbytes = (int)(swz_floats(k.K, k.N) * sizeof(float));
    q.in = in; q.out = out; q.relu = relu; q.resid = resid; q.rowmajor = rowmajor; q.ldout = ldout; q.decode = dec;
    q.ncol1 = k.N;  // columns routed like the first source (all, unless set below)
    q.in2 = in; q.out2 = out; q.rowmajor2 = rowmajor; q.ldout2 = ldout;
    const Split sp = layer_split(k.K, k.N);
    q.Np = sp.Np; q.splits = sp.splits; q.cpl = sp.cpl; q.log2s = sp.log2s;
    ++l;
    return q;
  };
  // phase stamps after the dynamics, the reward head, fc_prediction_common and the heads: MuZero's only
  auto stamp = [&](int i) { p.stamp_at[i] = gate ? -1 : n - 1; };
  add(x0, x1, 1, -1, 0, 0, 0);                  // fc_dynamics(_1)[0]
  add(x1, nl, 1, res ? x0 : -1, 0, 0, 0);       // [1] (+ latent: res_connection_in_dynamics)
  int enc = nl;                                 // the dynamics' output (with a gate layer and no residual nl == gx)
  if (res) {
    enc = gate ? gx : x2;                       // (the gate layer's input rows)
    add(nl, x1, 1, -1, 0, 0, 0);                // fc_dynamics_2
    add(x1, enc, 1, -1, 0, 0, 0);
  }
  stamp(0);
  if (gate) {
    add(enc, gt, 0, -1, 0, 0, 0);               // gates = [x ; h_prev] . [W_ih | W_hh] + (b_ih + b_hh)
    p.cell_after = n - 1;
    enc = hh;                                   // the value-prefix head reads the unmasked h1
  }
  add(enc, hd, 1, -1, 0, 0, 0);                 // fc_reward_head
  add(hd, lg, 0, -1, 1, V + 1, 1);
  stamp(1);
  add(nl, x1, 1, -1, 0, 0, 0);                  // fc_prediction_common
  add(x1, x2, 1, -1, 0, 0, 0);
  stamp(2);
  add(x2, hd, 1, -1, 0, 0, 0);                  // [fc_value_head[0] | fc_policy_head[0]]: 2F rows of hd
  StepRec &o = add(hd, lg, 0, -1, 1, V + 1, 2);  // [fc_value_head[1] | fc_policy_head[1]]
  o.ncol1 = V;                                  // value support columns, decoded
  o.in2 = hd + F / kKC * (kKC * R + 4);         // policy columns read the policy half of hd
  o.out2 = x1; o.rowmajor2 = 1; o.ldout2 = A;   // logits [r][A]
  stamp(3);
  if (n & 1) {  // the empty step: no columns, no weights (every load out of range), one barrier
    StepRec &q = p.sched[n++];
    memset(&q, 0, sizeof(q));
    q.w = weights; q.b = weights;
    q.resid = -1;
    const Split sp = layer_split(0, 0);
    q.Np = sp.Np; q.splits = sp.splits; q.cpl = sp.cpl; q.log2s = sp.log2s;
  }
  p.nsteps = n;
}

// ---- network-resident search (lzm_search_res.h): the config-2 shape, one root per workgroup
bool res_shape_ok(int H, int A, int F, int V, int res) {
  return H == kRHid && F == kRF && V == kRV && res && A >= 1 && A <= kRMaxA;
}
bool res_enabled() {
  const char *e = getenv("LZM_FUSED_RES");  // "0": always the streaming kernel (experiments)
  return !(e && atoi(e) == 0);
}
struct ResSrc {
  size_t pw[12], pb[12];
  int N[12];
};
// resident float d <- packed network (res_source defines the layout)
__global__ void mlp_res_swizzle_kernel(const float *packed, ResSrc src, int A, float *dst, size_t n) {
  const size_t d = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (d >= n) return;
  int b = 0;
  size_t o = 0;
  while (b + 1 < kRbN && d >= o + res_block_floats(b, A)) o += res_block_floats(b++, A);
  int layer, k, col;
  res_source(b, d - o, A, &layer, &k, &col);
  float v = 0.0f;
  if (layer >= 0) v = k < 0 ? packed[src.pb[layer] + col] : packed[src.pw[layer] + (size_t)k * src.N[layer] + col];
  dst[d] = v;
}
// LDS plan of search_res_kernel (float offsets, 16-B aligned); returns bytes, or 0 if it does not fit
size_t plan_res(SearchArgs &p, ResNet &n, const lzm_handle *h, int S, int A) {
  const ResPlan q = res_plan(h->cap, h->lut_n, h->depth_cap, S, A);
  n.plan = q;
  p.tree_in_lds = 1;
  p.off_stat = q.stat; p.off_meta = q.meta; p.off_lut = q.lut; p.off_legal = q.legal; p.off_val = q.val;
  p.off_path = q.path; p.off_pact = q.pact; p.off_misc = q.misc; p.off_pbt = q.pbt;
  p.pbt_rows = q.pbt_rows;
  return (size_t)q.floats * sizeof(float) <= (size_t)kResMaxBytes ? (size_t)q.floats * sizeof(float) : 0;
}
// network shapes the search kernels take (the weight preparation's K padding, the dense steps' lane maps and
// the decode's rounds over the support); everything else is refused before any launch
bool mlp_shape_ok(int H, int A, int F, int V) {
  return H > 0 && H <= 1024 && F > 0 && F <= 1024 && V > 0 && A > 0 && V + A <= kMaxRounds * kThreads && A <= H &&
         H % kKC == 0 && F % kKC == 0;
}
// the EfficientZero kernel's own limits on top of the dense steps': the cell's lane map and the h1 rows
// (the value-prefix head's K) need Hl % kKC == 0, the gate layer at most four column rounds.
// Widths routed: see DESIGN.md 10 (every width the one-launch path was measured to win at).
bool ez_shape_ok(int H, int Hl, int A, int F, int V) {
  return mlp_shape_ok(H, A, F, V) && Hl > 0 && Hl % kKC == 0 && 4 * Hl <= 4 * kThreads;
}
// LDS plan of search_mlp_kernel with R roots per workgroup (float offsets, 16-B aligned); returns bytes.
// Hl > 0 (EfficientZero): then the gate layer's input [x ; h_prev], the gates, h1 and c_prev. gz (Gumbel MuZero):
// the raw_value slice [cap][R] beside the node records instead of the pUCT table and its caches, and the
// considered-visits row [S] with the Gumbel table [64] where the seeds would be
size_t plan_stream(SearchArgs &p, const lzm_handle *h, int R, int S, int H, int Hl, int A, int F, int V, int res,
                   bool gz) {
  size_t o = 0;
  const size_t tree_floats = (size_t)h->cap * R * 4;
  p.tree_in_lds = (2 * tree_floats * sizeof(float) <= 96 * 1024) ? 1 : 0;
  const bool puct = p.tree_in_lds && !gz;
  p.off_stat = o; if (p.tree_in_lds) o += tree_floats;
  p.off_meta = o; if (p.tree_in_lds) o += tree_floats;
  p.off_raw = o; if (p.tree_in_lds && gz) o += round4((size_t)h->cap * R);
  p.off_lut = o; if (puct) o += round4((size_t)2 * h->lut_n);
  p.off_legal = o; if (p.tree_in_lds) o += round4((size_t)R * A + R);
  p.off_val = o; if (puct) o += round4((size_t)h->cap * R);
  // pUCT visit table rows: all of lut when the triangle fits 32 KB (descent falls back to dividing)
  p.pbt_rows = (puct && (size_t)h->lut_n * (h->lut_n + 1) / 2 <= 8192) ? h->lut_n : 0;
  p.off_pbt = o; o += round4((size_t)p.pbt_rows * (p.pbt_rows + 1) / 2);
  p.off_path = o; o += round4((size_t)h->depth_cap * R);
  p.off_pact = o; o += round4((size_t)h->depth_cap * R);
  // transposed activations [k][r], 4-float pad per kKC rows (tpos in lzm_search_mlp.h)
  auto tfl = [R](int K) { return (size_t)((K + kKC - 1) / kKC) * (kKC * R + 4); };
  p.off_x0 = o; o += round4(tfl((H + A + kKC - 1) / kKC * kKC));  // [latent; one-hot] rows, zero-padded
  p.off_x1 = o; o += round4(tfl(H));          // also the policy logits [r][A]
  p.off_x2 = o; o += round4(tfl(H));
  p.off_n = o; o += round4(tfl(H));
  p.off_h = o; o += round4(tfl(2 * F));        // [value hidden; policy hidden] (merged layer)
  p.off_logit = o; if (V < kThreads) o += round4((size_t)(V + 1) * R);  // wide supports decode from registers
  p.off_part = o;  // (unused: split-K partials meet through DPP)
  p.off_misc = o; o += round4((size_t)S + (gz ? kMaxActions : 32));  // staged seeds[S] + 16807^i table
  if (Hl > 0) {
    p.off_g = o; o += round4(tfl(H + Hl));
    p.off_gates = o; o += round4(tfl(4 * Hl));
    p.off_hh = o; o += round4(tfl(Hl));
    p.off_cp = o; o += round4((size_t)Hl * R);
    if (!res) p.off_n = p.off_g;  // the next latent is the LSTM's input: the front rows of [x ; h_prev]
  }
  return o * sizeof(float);
}
// The three searches the MLP one-launch path serves, each on handles of its own kind: lzm_search_mlp,
// lzm_search_mlp_ez and lzm_search_mlp_gumbel
enum MlpFamily { kMlpMuZero, kMlpEz, kMlpGumbel };
MlpFamily handle_family(const lzm_handle *h) {
  return (h->flags & LZM_TREE_GUMBEL) ? kMlpGumbel : (h->flags & LZM_TREE_EZ) ? kMlpEz : kMlpMuZero;
}
// the Gumbel kernel's limit on top of the dense steps': one lane per action (lzm_gumbel.h)
bool gumbel_shape_ok(int H, int A, int F, int V) { return mlp_shape_ok(H, A, F, V) && A <= kMaxActions; }
bool family_shape_ok(MlpFamily fam, int H, int Hl, int A, int F, int V) {
  return fam == kMlpEz ? ez_shape_ok(H, Hl, A, F, V) : fam == kMlpGumbel ? gumbel_shape_ok(H, A, F, V)
                                                                        : mlp_shape_ok(H, A, F, V);
}
// What lzm_search_mlp, lzm_search_mlp_ez or lzm_search_mlp_gumbel (fam) launches for this handle, network shape
// and search length: the one decision behind the launch and the plan queries. kind: 1 network-resident (MuZero
// only), 0 weight-streaming, -1 none (the shape, or the LDS the streaming kernel would need for it, is
// refused). mode: the resident kernel's selection mode after its downgrades (0 for the streaming kernel).
// R: roots per workgroup by roots_per_wg's rule; the EfficientZero kernel takes 1, 2 or 4 (the gate rows
// of 8 would not leave the tree its LDS). The LDS offsets of the chosen kernel are left in p (and n.plan).
struct MlpPlan {
  int R, kind, mode, tree_in_lds;
  size_t lds;
};
MlpPlan mlp_plan(const lzm_handle *h, MlpFamily fam, int H, int Hl, int F, int V, int res_dynamics, int S,
                 SearchArgs &p, ResNet &n) {
  const int A = h->A;
  const bool ez = fam == kMlpEz;
  MlpPlan pl{ez ? std::min(roots_per_wg(h->B), 4) : roots_per_wg(h->B), -1, 0, 0, 0};
  if (!family_shape_ok(fam, H, Hl, A, F, V)) return pl;
  if (fam == kMlpMuZero && pl.R == 1 && res_enabled() && res_shape_ok(H, A, F, V, res_dynamics)) {
    pl.lds = plan_res(p, n, h, S, A);
    if (pl.lds) {
      // the selection mode (lzm_search_res.h, the simulation loop): 1 the wave walk; 4 the two-action
      // walk for A == 2; 5 is 4 with the walk on the terms pass's registers: one node per lane of wave
      // 0, so it serves S + 2 <= 64 (a path is then at most S levels: it fits the wave's lanes); larger
      // searches run mode 4. LZM_RES_SELECT = 1, 4 or 5 asks for a mode; any other value is ignored.
      const char *sm = getenv("LZM_RES_SELECT");
      const int asked = sm ? atoi(sm) : 0;
      int mode = (asked == 1 || asked == 4 || asked == 5) ? asked : (A == 2 ? 5 : 1);
      if (mode == 5 && (A != 2 || S + 2 > 64 || h->depth_cap < S + 2)) mode = 4;
      if (mode == 4 && A != 2) mode = 1;
      pl.kind = 1;
      pl.mode = mode;
      pl.tree_in_lds = 1;
      return pl;
    }
  }
  pl.lds = plan_stream(p, h, pl.R, S, H, ez ? Hl : 0, A, F, V, res_dynamics, fam == kMlpGumbel);
  pl.tree_in_lds = p.tree_in_lds;
  pl.kind = pl.lds <= kMaxLds ? 0 : -1;
  return pl;
}
// The plan queries' body (fam: whose query it is); a handle of another kind answers kind -1
int mlp_plan_query(const char *name, const lzm_handle *h, MlpFamily fam, int S, int H, int Hl, int F, int V,
                   int res_dynamics, int32_t *out) {
  if (!h || !out || S <= 0) {
    snprintf(g_err, sizeof(g_err), "%s: null argument or no simulations", name);
    return LZM_ERR_ARG;
  }
  if (S > h->sims_cap) {
    snprintf(g_err, sizeof(g_err), "%s: %d simulations > reserved %d (lzm_reserve)", name, S, h->sims_cap);
    return LZM_ERR_CAPACITY;
  }
  SearchArgs p;
  memset(&p, 0, sizeof(p));
  ResNet n;
  memset(&n, 0, sizeof(n));
  const MlpPlan pl = mlp_plan(h, fam, H, Hl, F, V, res_dynamics, S, p, n);
  out[0] = pl.R;
  out[1] = handle_family(h) == fam ? pl.kind : -1;
  out[2] = pl.mode;
  out[3] = pl.tree_in_lds;
  return LZM_OK;
}

// The network-resident layout (lzm_search_res.h) follows the kernel layout, for the MuZero shape it serves
bool net_resident(const MlpNet &n) { return n.Hl == 0 && res_shape_ok(n.H, n.A, n.F, n.V, n.res); }
// packed -> kernel layout: each kernel layer's weights in lane order (swz_source), then its bias
int mlp_prepare(const MlpNet &net, const float *packed, float *out, hipStream_t stream) {
  for (int l = 0; l < net.nk; ++l) {
    const KLayer &q = net.kl[l];
    const size_t n = swz_floats(q.K, q.N);
    const int s1 = q.src1 >= 0 ? q.src1 : q.src0;
    hipLaunchKernelGGL(mlp_swizzle_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                       packed + net.pw[q.src0], net.s[q.src0].krows, packed + net.pw[s1], net.s[s1].krows, q.K, q.N,
                       q.N0, out + net.w_off[l], n);
    LZM_CHECK_LAUNCH();
    LZM_HIP(hipMemcpyAsync(out + net.b_off[l], packed + net.pb[q.src0], (size_t)q.N0 * sizeof(float),
                           hipMemcpyDeviceToDevice, stream));
    if (q.src1 >= 0)
      LZM_HIP(hipMemcpyAsync(out + net.b_off[l] + q.N0, packed + net.pb[q.src1], (size_t)(q.N - q.N0) * sizeof(float),
                             hipMemcpyDeviceToDevice, stream));
  }
  if (net_resident(net)) {
    ResSrc src;  // res_source numbers the layers in MuZero's packed order: the gate layer's slot skipped
    for (int l = 0; l < 12; ++l) {
      const int u = l < kGateLayer ? l : l + 1;
      src.pw[l] = net.pw[u];
      src.pb[l] = net.pb[u];
      src.N[l] = net.s[u].N;
    }
    const size_t n = res_block_offset(kRbN, net.A);
    hipLaunchKernelGGL(mlp_res_swizzle_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, packed, src,
                       net.A, out + round4(net.kernel_floats), n);
    LZM_CHECK_LAUNCH();
  }
  return LZM_OK;
}

// The network-resident launch (search_res_kernel): one root per workgroup, collect-step mode in-kernel
int launch_resident(lzm_handle *h, SearchArgs &p, ResNet &n, const MlpNet &net, const float *weights,
                    const MlpPlan &plan, hipStream_t stream) {
  p.step_count = h->step_count; p.step_inc = h->step_inc; p.step_base = h->step_base;
  p.mm_fresh = h->step_fresh; p.mm_delta = h->step_delta;
  p.out_dist = h->step_dist; p.out_values = h->step_vals;
  n.w = weights + round4(net.kernel_floats);  // its weights follow the generic layout
  const char *sl = getenv("LZM_RES_LATE");
  n.late_draw = sl ? atoi(sl) : 1;
  const char *sd = getenv("LZM_RES_SPEC_DEPTH");
  n.spec_depth = sd ? atoi(sd) : 1;
  // one instantiation per selection mode (1, 4, 5) x variant: the production kernels fix the RNG at
  // compile time (0 glibc, 1 Philox); the stamps kernel reads the RNG and n.spec_depth at run time and
  // serves phase timing and LZM_RES_SPEC_DEPTH=0 (then without a phase buffer: it stamps nothing)
  typedef void (*ResKernel)(SearchArgs, ResNet);
  static const ResKernel kernels[3][3] = {
      {search_res_kernel<1, 0, false>, search_res_kernel<1, 1, false>, search_res_kernel<1, -1, true>},
      {search_res_kernel<4, 0, false>, search_res_kernel<4, 1, false>, search_res_kernel<4, -1, true>},
      {search_res_kernel<5, 0, false>, search_res_kernel<5, 1, false>, search_res_kernel<5, -1, true>}};
  const int mi = plan.mode == 5 ? 2 : plan.mode == 4 ? 1 : 0;
  const int vi = (p.phase || !n.spec_depth) ? 2 : p.fast ? 1 : 0;
  const ResKernel fn = kernels[mi][vi];
  LZM_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
  hipLaunchKernelGGL(fn, dim3(h->B), dim3(kRT), plan.lds, stream, p, n);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// The weight-streaming launch (search_mlp_kernel<R, tree in LDS, EZ, Gumbel>; the EfficientZero kernel serves
// R <= 4), with the collect-step mode's prologue (seeds, fresh min-max) and epilogue (root outputs,
// counter) as one launch each around the search. name: the entry point, for the messages.
int launch_stream(const char *name, lzm_handle *h, SearchArgs &p, int R, size_t lds, float *minmax, hipStream_t stream) {
  typedef void (*StreamKernel)(SearchArgs);
  static const StreamKernel kernels[3][4][2] = {  // [MuZero, EZ, Gumbel][R = 1, 2, 4, 8][tree in LDS, tree in HBM]
      {{search_mlp_kernel<1, true>, search_mlp_kernel<1, false>},
       {search_mlp_kernel<2, true>, search_mlp_kernel<2, false>},
       {search_mlp_kernel<4, true>, search_mlp_kernel<4, false>},
       {search_mlp_kernel<8, true>, search_mlp_kernel<8, false>}},
      {{search_mlp_kernel<1, true, true>, search_mlp_kernel<1, false, true>},
       {search_mlp_kernel<2, true, true>, search_mlp_kernel<2, false, true>},
       {search_mlp_kernel<4, true, true>, search_mlp_kernel<4, false, true>},
       {nullptr, nullptr}},
      {{search_mlp_kernel<1, true, false, true>, search_mlp_kernel<1, false, false, true>},
       {search_mlp_kernel<2, true, false, true>, search_mlp_kernel<2, false, false, true>},
       {search_mlp_kernel<4, true, false, true>, search_mlp_kernel<4, false, false, true>},
       {search_mlp_kernel<8, true, false, true>, search_mlp_kernel<8, false, false, true>}}};
  const int fam = p.raw ? 2 : p.Hl > 0 ? 1 : 0;  // (p.raw: the Gumbel search's raw_value array)
  const StreamKernel fn = kernels[fam][R == 1 ? 0 : R == 2 ? 1 : R == 4 ? 2 : 3][p.tree_in_lds ? 0 : 1];
  if (!fn) {
    snprintf(g_err, sizeof(g_err), "%s: no kernel for %d roots per workgroup", name, R);
    return LZM_ERR_STATE;
  }
  const int S = p.S;
  if (h->step_count || h->step_fresh) {
    if (h->step_count && h->step_seeds_n < S) {  // (allocated with the tree: S <= sims_cap)
      snprintf(g_err, sizeof(g_err), "%s: step seeds buffer smaller than num_simulations (reserve first)", name);
      return LZM_ERR_STATE;
    }
    const int n = std::max(S, h->B);
    hipLaunchKernelGGL(step_prologue_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, h->step_count,
                       h->step_base, S, h->step_seeds, (float4 *)minmax, h->B, h->step_fresh, h->step_delta);
    LZM_CHECK_LAUNCH();
    if (h->step_count) p.seeds = reinterpret_cast<const uint32_t *>(h->step_seeds);
  }
  LZM_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(fn, dim3((h->B + R - 1) / R), dim3(kThreads), lds, stream, p);
  LZM_CHECK_LAUNCH();
  if ((h->step_count && h->step_inc) || h->step_dist || h->step_vals) {
    hipLaunchKernelGGL(step_epilogue_kernel, dim3((h->B + 255) / 256), dim3(256), 0, stream, view(h),
                       h->step_dist, h->step_vals, h->step_inc ? h->step_count : nullptr);
    LZM_CHECK_LAUNCH();
  }
  return LZM_OK;
}

// lzm_search_mlp (Hl, horizon and the LSTM pools unused), lzm_search_mlp_ez and lzm_search_mlp_gumbel (fam; the
// last without seeds, with considered_m = max_num_considered_actions, refused on a handle in collect-step mode:
// there is no Gumbel collect step). name: the entry point, for the messages.
int search_mlp(const char *name, MlpFamily fam, lzm_handle *h, int H, int Hl, int F, int V, int res_dynamics,
               const float *weights, int S, int horizon, int considered_m, int pb_c_base, float pb_c_init,
               float discount, float *minmax, const uint32_t *seeds, const int32_t *vtp_in, float *latent_pool,
               float *h_pool, float *c_pool, int32_t *rec_x, int32_t *rec_a, int32_t *rec_len, int32_t *rec_reset,
               float *rec_decoded, float *rec_logits, hipStream_t stream) {
  const bool ez = fam == kMlpEz, gz = fam == kMlpGumbel;
  if (!h || !weights || !minmax || (!gz && !seeds && !h->step_count) || !vtp_in || !latent_pool ||
      (ez && (!h_pool || !c_pool)) || S <= 0) {
    snprintf(g_err, sizeof(g_err), "%s: null argument or no simulations", name);
    return LZM_ERR_ARG;
  }
  if (gz) {
    int rc = check_kind(name, h, true);
    if (rc != LZM_OK) return rc;
    if (considered_m < 0) return refuse(LZM_ERR_ARG, name, "max_num_considered_actions must be >= 0");
    if (h->step_count || h->step_fresh || h->step_dist || h->step_vals)
      return refuse(LZM_ERR_STATE, name, "collect-step mode (lzm_search_set_step) has no Gumbel search");
  } else if (h->flags & LZM_TREE_GUMBEL) {
    return refuse(LZM_ERR_STATE, name, "a Gumbel MuZero handle takes lzm_search_mlp_gumbel");
  }
  if ((uintptr_t)weights & 15) {
    snprintf(g_err, sizeof(g_err), "%s: weights must be 16-byte aligned (%s output)", name,
             ez ? "lzm_mlp_ez_prepare" : "lzm_mlp_prepare");
    return LZM_ERR_ARG;
  }
  if (((h->flags & LZM_TREE_EZ) != 0) != ez) {
    snprintf(g_err, sizeof(g_err), "%s: %s trees only", name, ez ? "EfficientZero" : "MuZero");
    return LZM_ERR_ARG;
  }
  if (ez && horizon <= 0) {
    snprintf(g_err, sizeof(g_err), "%s: lstm_horizon_len must be > 0", name);
    return LZM_ERR_ARG;
  }
  const int A = h->A;
  if (!family_shape_ok(fam, H, Hl, A, F, V)) {
    snprintf(g_err, sizeof(g_err), "%s: unsupported network shape (%s)", name,
             ez ? "lzm_search_mlp_ez_supported"
                : gz ? "lzm_search_mlp_supported, and at most 64 actions"
                     : "hidden and head widths must be multiples of 16");
    return LZM_ERR_ARG;
  }
  if (S > h->sims_cap) {
    snprintf(g_err, sizeof(g_err), "%s: %d simulations > reserved %d (lzm_reserve)", name, S, h->sims_cap);
    return LZM_ERR_CAPACITY;
  }
  SearchArgs p;
  memset(&p, 0, sizeof(p));
  ResNet n;
  memset(&n, 0, sizeof(n));
  const MlpPlan plan = mlp_plan(h, fam, H, Hl, F, V, res_dynamics, S, p, n);
  if (plan.kind < 0) {
    snprintf(g_err, sizeof(g_err), "%s: %zu B of LDS needed (network or tree too large)", name, plan.lds);
    return LZM_ERR_ARG;
  }
  int rc = search_preamble(h, pb_c_base, pb_c_init, S, (h->B + plan.R - 1) / plan.R);
  if (rc != LZM_OK) return rc;
  if (gz && (rc = gumbel_set_considered(h, S, considered_m, name)) != LZM_OK) return rc;
  const MlpNet net = mlp_net(H, ez ? Hl : 0, A, F, V, res_dynamics);
  fill_common(p, h, S, discount, seeds, vtp_in, minmax, latent_pool, rec_x, rec_a, rec_len, rec_decoded, rec_logits);
  p.H = H; p.F = F; p.V = V; p.res = net.res;
  p.diag = h->search_diag;
  p.hpool = h_pool; p.cpool = c_pool; p.Hl = net.Hl; p.horizon = horizon; p.rec_reset = rec_reset;
  if (gz) { p.raw = h->raw; p.gumbel = h->gumbel; p.considered = h->considered; }
  if (fam == kMlpMuZero) {  // the phase stamps and the timing experiments are the MuZero kernels'
    if (phase_timing() && (rc = ensure_phase(h)) != LZM_OK) return rc;
    p.phase = h->phase;
    p.diag_mode = getenv("LZM_DIAG_MODE") ? atoi(getenv("LZM_DIAG_MODE")) : 0;  // timing experiments only
  }
  if (plan.kind == 1) return launch_resident(h, p, n, net, weights, plan, stream);
  build_schedule(p, net, weights, plan.R);
  return launch_stream(name, h, p, plan.R, plan.lds, minmax, stream);
}

}  // namespace

extern "C" {

int64_t lzm_mlp_packed_floats(int hidden, int actions, int head_hidden, int support, int res_dynamics) {
  if (hidden <= 0 || actions <= 0 || head_hidden <= 0 || support <= 0) return -1;
  return (int64_t)mlp_net(hidden, 0, actions, head_hidden, support, res_dynamics).packed_floats;
}

int64_t lzm_mlp_kernel_floats(int hidden, int actions, int head_hidden, int support, int res_dynamics) {
  if (hidden <= 0 || actions <= 0 || head_hidden <= 0 || support <= 0) return -1;
  const MlpNet net = mlp_net(hidden, 0, actions, head_hidden, support, res_dynamics);
  return (int64_t)(net_resident(net) ? round4(net.kernel_floats) + res_block_offset(kRbN, actions) : net.kernel_floats);
}

int lzm_mlp_prepare(int hidden, int actions, int head_hidden, int support, int res_dynamics, const float *packed,
                    float *out, void *stream) {
  if (!packed || !out || hidden <= 0 || actions <= 0 || head_hidden <= 0 || support <= 0 ||
      hidden % kKC != 0 || head_hidden % kKC != 0) {
    set_err("lzm_mlp_prepare: bad arguments (hidden and head widths must be multiples of 16)");
    return LZM_ERR_ARG;
  }
  return mlp_prepare(mlp_net(hidden, 0, actions, head_hidden, support, res_dynamics), packed, out, (hipStream_t)stream);
}

int lzm_search_mlp_kind(int B, int actions, int hidden, int head_hidden, int support, int res_dynamics) {
  if (B <= 0) return 0;
  return (roots_per_wg(B) == 1 && res_enabled() && res_shape_ok(hidden, actions, head_hidden, support, res_dynamics))
             ? 1
             : 0;
}

int lzm_search_mlp_supported(int actions, int hidden, int head_hidden, int support) {
  return mlp_shape_ok(hidden, actions, head_hidden, support) ? 1 : 0;
}

int lzm_search_mlp_plan(const lzm_handle *h, int num_simulations, int hidden, int head_hidden, int support,
                        int res_dynamics, int32_t *out) {
  return mlp_plan_query("lzm_search_mlp_plan", h, kMlpMuZero, num_simulations, hidden, 0, head_hidden, support,
                        res_dynamics, out);
}

int lzm_search_mlp(lzm_handle *h, int hidden, int head_hidden, int support, int res_dynamics, const float *weights,
                   int num_simulations, int pb_c_base, float pb_c_init, float discount, float *minmax,
                   const uint32_t *seeds, const int32_t *vtp_in, float *latent_pool, int32_t *rec_x, int32_t *rec_a,
                   int32_t *rec_len, float *rec_decoded, float *rec_logits, void *stream) {
  return search_mlp("lzm_search_mlp", kMlpMuZero, h, hidden, 0, head_hidden, support, res_dynamics, weights,
                    num_simulations, 0, 0, pb_c_base, pb_c_init, discount, minmax, seeds, vtp_in, latent_pool, nullptr,
                    nullptr, rec_x, rec_a, rec_len, nullptr, rec_decoded, rec_logits, (hipStream_t)stream);
}

// The EfficientZeroModelMLP twins: the same network with the reward LSTM's gate layer (lstm_hidden wide)
int64_t lzm_mlp_ez_packed_floats(int hidden, int lstm_hidden, int actions, int head_hidden, int support,
                                 int res_dynamics) {
  if (hidden <= 0 || lstm_hidden <= 0 || actions <= 0 || head_hidden <= 0 || support <= 0) return -1;
  return (int64_t)mlp_net(hidden, lstm_hidden, actions, head_hidden, support, res_dynamics).packed_floats;
}

int64_t lzm_mlp_ez_kernel_floats(int hidden, int lstm_hidden, int actions, int head_hidden, int support,
                                 int res_dynamics) {
  if (hidden <= 0 || lstm_hidden <= 0 || actions <= 0 || head_hidden <= 0 || support <= 0) return -1;
  return (int64_t)mlp_net(hidden, lstm_hidden, actions, head_hidden, support, res_dynamics).kernel_floats;
}

int lzm_mlp_ez_prepare(int hidden, int lstm_hidden, int actions, int head_hidden, int support, int res_dynamics,
                       const float *packed, float *out, void *stream) {
  if (!packed || !out || hidden <= 0 || lstm_hidden <= 0 || actions <= 0 || head_hidden <= 0 || support <= 0 ||
      hidden % kKC != 0 || head_hidden % kKC != 0 || lstm_hidden % kKC != 0) {
    set_err("lzm_mlp_ez_prepare: bad arguments (hidden, LSTM and head widths must be multiples of 16)");
    return LZM_ERR_ARG;
  }
  return mlp_prepare(mlp_net(hidden, lstm_hidden, actions, head_hidden, support, res_dynamics), packed, out,
                     (hipStream_t)stream);
}

int lzm_search_mlp_ez_supported(int actions, int hidden, int lstm_hidden, int head_hidden, int support) {
  return ez_shape_ok(hidden, lstm_hidden, actions, head_hidden, support) ? 1 : 0;
}

int lzm_search_mlp_ez_plan(const lzm_handle *h, int num_simulations, int hidden, int lstm_hidden, int head_hidden,
                           int support, int res_dynamics, int32_t *out) {
  return mlp_plan_query("lzm_search_mlp_ez_plan", h, kMlpEz, num_simulations, hidden, lstm_hidden, head_hidden, support,
                        res_dynamics, out);
}

int lzm_search_mlp_ez(lzm_handle *h, int hidden, int lstm_hidden, int head_hidden, int support, int res_dynamics,
                      const float *weights, int num_simulations, int lstm_horizon_len, int pb_c_base, float pb_c_init,
                      float discount, float *minmax, const uint32_t *seeds, const int32_t *vtp_in, float *latent_pool,
                      float *h_pool, float *c_pool, int32_t *rec_x, int32_t *rec_a, int32_t *rec_len,
                      int32_t *rec_reset, float *rec_decoded, float *rec_logits, void *stream) {
  return search_mlp("lzm_search_mlp_ez", kMlpEz, h, hidden, lstm_hidden, head_hidden, support, res_dynamics, weights,
                    num_simulations, lstm_horizon_len, 0, pb_c_base, pb_c_init, discount, minmax, seeds, vtp_in,
                    latent_pool, h_pool, c_pool, rec_x, rec_a, rec_len, rec_reset, rec_decoded, rec_logits,
                    (hipStream_t)stream);
}

int lzm_search_mlp_gumbel_plan(const lzm_handle *h, int num_simulations, int hidden, int head_hidden, int support,
                               int res_dynamics, int32_t *out) {
  return mlp_plan_query("lzm_search_mlp_gumbel_plan", h, kMlpGumbel, num_simulations, hidden, 0, head_hidden, support,
                        res_dynamics, out);
}

// The Gumbel MuZero search over MuZeroModelMLP (lzm_mlp_prepare's weights) in one launch. Rebuilds the handle's
// considered-visits row when (S, m) changed: a synchronous copy, outside stream capture (lzm_gumbel_set_considered
// before a capture). No seeds and no draw table: the walk draws nothing. The pUCT constants are the handle's
// defaults (the table is never read).
int lzm_search_mlp_gumbel(lzm_handle *h, int hidden, int head_hidden, int support, int res_dynamics,
                          const float *weights, int num_simulations, int max_num_considered_actions, float discount,
                          float *minmax, const int32_t *vtp_in, float *latent_pool, int32_t *rec_x, int32_t *rec_a,
                          int32_t *rec_len, float *rec_decoded, float *rec_logits, void *stream) {
  return search_mlp("lzm_search_mlp_gumbel", kMlpGumbel, h, hidden, 0, head_hidden, support, res_dynamics, weights,
                    num_simulations, 0, max_num_considered_actions, 19652, 1.25f, discount, minmax, nullptr, vtp_in,
                    latent_pool, nullptr, nullptr, rec_x, rec_a, rec_len, nullptr, rec_decoded, rec_logits,
                    (hipStream_t)stream);
}

// Collect-step mode of lzm_search_mlp (sticky on the handle, host state only: a captured launch
// keeps the values it was launched with). See include/lzmcts.h.
int lzm_search_set_step(lzm_handle *h, int64_t *count, int64_t base, int increment, int32_t *root_dist,
                        float *root_values, int fresh_minmax, float value_delta_max) {
  if (!h || base < 0) return LZM_ERR_ARG;
  h->step_count = count;
  h->step_inc = increment ? 1 : 0;
  h->step_base = (long long)base;
  h->step_dist = root_dist;
  h->step_vals = root_values;
  h->step_fresh = fresh_minmax ? 1 : 0;
  h->step_delta = value_delta_max;
  return LZM_OK;
}

int lzm_debug_phase_cycles(lzm_handle *h, uint64_t *out_host, int reset) {
  if (!h || !out_host) return LZM_ERR_ARG;
  if (!h->phase) {
    memset(out_host, 0, 64 * sizeof(uint64_t));
    return LZM_OK;
  }
  LZM_HIP(hipDeviceSynchronize());
  LZM_HIP(hipMemcpy(out_host, h->phase, 64 * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (reset) LZM_HIP(hipMemset(h->phase, 0, 64 * sizeof(unsigned long long)));
  return LZM_OK;
}

// Diagnostics (LZM_PHASE_TIMING=1, resident kernel): shader-clock cycles each workgroup spent in
// the parity-mode look-back wait, summed over launches (phase[64 + g], up to 1024 workgroups).
int lzm_debug_root_wait_cycles(lzm_handle *h, uint64_t *out_host, int n, int reset) {
  if (!h || !out_host || n < 0 || n > 1024) return LZM_ERR_ARG;
  if (!h->phase) {
    memset(out_host, 0, n * sizeof(uint64_t));
    return LZM_OK;
  }
  LZM_HIP(hipDeviceSynchronize());
  LZM_HIP(hipMemcpy(out_host, h->phase + 64, n * sizeof(uint64_t), hipMemcpyDeviceToHost));
  if (reset) LZM_HIP(hipMemset(h->phase + 64, 0, 1024 * sizeof(unsigned long long)));
  return LZM_OK;
}

int lzm_search_diagnostics(lzm_handle *h, int32_t *out, void *stream) {
  if (!h || !out) return LZM_ERR_ARG;
  if (!h->search_diag) {
    LZM_HIP(hipMemsetAsync(out, 0, 4 * sizeof(int32_t), (hipStream_t)stream));
    return LZM_OK;
  }
  LZM_HIP(hipMemcpyAsync(out, h->search_diag, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LZM_OK;
}

// Sticky error counters of every search path on this handle (a look-back spin that
// times out, or a draw position beyond the coefficient table, would otherwise leave a silently
// wrong tie-break stream; round 6: split-fp16 activations out of range). Synchronises `stream`;
// out_host (nullable) gets the kErrWords words {look-back timeouts, draw-table overflows, reserved
// (no kernel writes it: always 0, checked like the others), fused-search errors, split-range errors, 0, 0, 0}.
int32_t *lzm_error_word(lzm_handle *h, int i) { return (h && i >= 0 && i < kErrWords) ? h->err + i : nullptr; }

int lzm_check_errors(lzm_handle *h, int32_t *out_host, int clear, void *stream) {
  if (!h) return LZM_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  int32_t w[kErrWords] = {};
  int32_t sd = 0;
  LZM_HIP(hipMemcpyAsync(w, h->err, kErrWords * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  if (h->search_diag) LZM_HIP(hipMemcpyAsync(&sd, h->search_diag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
  LZM_HIP(hipStreamSynchronize(s));
  w[3] += sd;  // err[3]: the EZ LSTM step's split-K hand-off timeouts (lzm_error_word(h, 3))
  if (out_host) memcpy(out_host, w, sizeof(w));
  const bool bad = w[0] || w[1] || w[2] || w[3] || w[4];
  if (bad && clear) {
    LZM_HIP(hipMemsetAsync(h->err, 0, kErrWords * sizeof(int32_t), s));
    if (h->search_diag) LZM_HIP(hipMemsetAsync(h->search_diag, 0, sizeof(int32_t), s));
    LZM_HIP(hipStreamSynchronize(s));
  }
  if (w[4]) {
    snprintf(g_err, sizeof(g_err),
             "split-fp16 network values out of range in %d workgroup-searches (non-finite, or beyond ~2^114): the "
             "search's network outputs are not f32-exact; run the conv network with precision='f32' "
             "(LZM_CONV_PRECISION=f32)", w[4]);
    return LZM_ERR_RANGE;
  }
  if (bad) {
    snprintf(g_err, sizeof(g_err),
             "search tie-break stream invalid: %d look-back timeouts, %d draw-table overflows, %d traverse "
             "fixed-point failures, %d fused-search errors (results differ from the reference)",
             w[0], w[1], w[2], w[3]);
    return LZM_ERR_STATE;
  }
  return LZM_OK;
}

int lzm_cartpole_reset(int n, double *state, int32_t *steps, float *obs, uint32_t seed, void *stream) {
  if (n <= 0 || !state || !steps || !obs) {
    set_err("lzm_cartpole_reset: bad arguments");
    return LZM_ERR_ARG;
  }
  hipLaunchKernelGGL(cartpole_reset_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, state,
                     steps, obs, seed);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// what the Gumbel collect steps take in place of (temperature, deterministic), and record on top
struct GumbelStepIO {
  const int32_t *action;
  const float *policy, *completed_q;
  float *rec_policy, *rec_cq;
  bool complete() const { return action && policy && completed_q && rec_policy && rec_cq; }
};

// lzm_cartpole_collect_step (gz null) and lzm_cartpole_collect_step_gumbel
static int cartpole_collect_step_g(const char *name, const GumbelStepIO *gz, int n, int A, int T, int E,
                                   const int32_t *visits, const float *root_value, const float *pred_value,
                                   double *state, int32_t *steps, float *obs, float *noises, float noise_alpha,
                                   float temperature, int deterministic, float *rec_obs, int32_t *rec_action,
                                   float *rec_reward, int32_t *rec_visits, float *rec_value, float *rec_pred,
                                   int32_t *ep_len, int32_t *ep_count, float *ep_return, int max_steps, uint32_t seed,
                                   const int64_t *counter, void *stream) {
  if (n <= 0 || A <= 0 || A > 64 || T <= 0 || E <= 0 || !visits || !root_value || !state || !steps || !obs ||
      !noises || !rec_obs || !rec_action || !rec_reward || !rec_visits || !rec_value || !ep_len || !ep_count ||
      !counter || !(temperature > 0.0f) || !(noise_alpha > 0.0f) || (!pred_value) != (!rec_pred) ||
      (gz && !gz->complete())) {
    snprintf(g_err, sizeof(g_err), "%s: bad arguments", name);
    return LZM_ERR_ARG;
  }
  CollectArgs a;
  a.n = n; a.A = A; a.T = T; a.E = E; a.max_steps = max_steps; a.deterministic = deterministic;
  a.temperature = temperature; a.noise_alpha = noise_alpha; a.seed = seed; a.counter = counter;
  a.visits = visits; a.root_value = root_value; a.state = state; a.steps = steps; a.obs = obs; a.noises = noises;
  a.rec_obs = rec_obs; a.rec_action = rec_action; a.rec_reward = rec_reward; a.rec_visits = rec_visits;
  a.rec_value = rec_value; a.pred_value = pred_value; a.rec_pred = rec_pred; a.ep_len = ep_len;
  a.ep_count = ep_count; a.ep_return = ep_return;
  a.action = gz ? gz->action : nullptr; a.policy = gz ? gz->policy : nullptr;
  a.completed_q = gz ? gz->completed_q : nullptr; a.rec_policy = gz ? gz->rec_policy : nullptr;
  a.rec_cq = gz ? gz->rec_cq : nullptr;
  hipLaunchKernelGGL(gz ? cartpole_collect_kernel<true> : cartpole_collect_kernel<false>, dim3((n + 127) / 128),
                     dim3(128), 0, (hipStream_t)stream, a);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_cartpole_collect_step(int n, int A, int T, int E, const int32_t *visits, const float *root_value,
                              const float *pred_value, double *state, int32_t *steps, float *obs, float *noises,
                              float noise_alpha, float temperature, int deterministic, float *rec_obs,
                              int32_t *rec_action, float *rec_reward, int32_t *rec_visits, float *rec_value,
                              float *rec_pred, int32_t *ep_len, int32_t *ep_count, float *ep_return, int max_steps,
                              uint32_t seed, const int64_t *counter, void *stream) {
  return cartpole_collect_step_g("lzm_cartpole_collect_step", nullptr, n, A, T, E, visits, root_value, pred_value,
                                 state, steps, obs, noises, noise_alpha, temperature, deterministic, rec_obs,
                                 rec_action, rec_reward, rec_visits, rec_value, rec_pred, ep_len, ep_count, ep_return,
                                 max_steps, seed, counter, stream);
}

int lzm_cartpole_collect_step_gumbel(int n, int A, int T, int E, const int32_t *visits, const float *root_value,
                                     const float *pred_value, const int32_t *action, const float *policy,
                                     const float *completed_q, double *state, int32_t *steps, float *obs,
                                     float *noises, float noise_alpha, float *rec_obs, int32_t *rec_action,
                                     float *rec_reward, int32_t *rec_visits, float *rec_value, float *rec_pred,
                                     float *rec_policy, float *rec_cq, int32_t *ep_len, int32_t *ep_count,
                                     float *ep_return, int max_steps, uint32_t seed, const int64_t *counter,
                                     void *stream) {
  const GumbelStepIO gz{action, policy, completed_q, rec_policy, rec_cq};
  return cartpole_collect_step_g("lzm_cartpole_collect_step_gumbel", &gz, n, A, T, E, visits, root_value, pred_value,
                                 state, steps, obs, noises, noise_alpha, 1.0f, 1, rec_obs, rec_action, rec_reward,
                                 rec_visits, rec_value, rec_pred, ep_len, ep_count, ep_return, max_steps, seed, counter,
                                 stream);
}

static int atari_reset_g(int game, const char *name, int n, int32_t *state, int32_t *steps, uint8_t *cur, float *obs,
                         uint32_t seed, void *stream) {
  if (n <= 0 || !state || !steps || !cur || !obs || (((uintptr_t)cur | (uintptr_t)obs) & 15)) {
    snprintf(g_err, sizeof(g_err), "%s: bad arguments (16-B aligned frame buffers)", name);
    return LZM_ERR_ARG;
  }
  hipLaunchKernelGGL(game ? atari_reset_kernel<1> : atari_reset_kernel<0>, dim3(n), dim3(kAtThreads), 0,
                     (hipStream_t)stream, n, state, steps, cur, obs, seed);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// gz: the Gumbel step's extra arrays (lzm_atari_collect_step_gumbel), else null
static int atari_collect_step_g(int game, const char *name, const GumbelStepIO *gz, int n, int A, int T, int E,
                                const int32_t *visits, const float *root_value, const float *pred_value,
                                int32_t *state, int32_t *steps,
                                uint8_t *cur, float *obs, float *noises, float noise_alpha, float temperature,
                                int deterministic, uint8_t *rec_frames, int32_t *rec_action, float *rec_reward,
                                int32_t *rec_visits, float *rec_value, float *rec_pred, int32_t *ep_len,
                                int32_t *ep_count, float *ep_return, int max_steps, uint32_t seed,
                                const int64_t *counter, void *stream) {
  if (n <= 0 || A <= 0 || A > 64 || T <= 0 || E <= 0 || max_steps <= 0 || !visits || !root_value || !state || !steps ||
      !cur || !obs || !noises || !rec_frames || !rec_action || !rec_reward || !rec_visits || !rec_value || !ep_len ||
      !ep_count || !counter || !(temperature > 0.0f) || !(noise_alpha > 0.0f) || (!pred_value) != (!rec_pred) ||
      (((uintptr_t)cur | (uintptr_t)obs | (uintptr_t)rec_frames) & 15) || (gz && (game || !gz->complete()))) {
    snprintf(g_err, sizeof(g_err), "%s: bad arguments", name);
    return LZM_ERR_ARG;
  }
  AtariArgs a;
  a.n = n; a.A = A; a.T = T; a.E = E; a.max_steps = max_steps; a.deterministic = deterministic;
  a.temperature = temperature; a.noise_alpha = noise_alpha; a.seed = seed; a.counter = counter;
  a.visits = visits; a.root_value = root_value; a.state = state; a.steps = steps; a.cur = cur; a.obs = obs;
  a.noises = noises; a.rec_frames = rec_frames; a.rec_action = rec_action; a.rec_reward = rec_reward;
  a.rec_visits = rec_visits; a.rec_value = rec_value; a.pred_value = pred_value; a.rec_pred = rec_pred;
  a.ep_len = ep_len; a.ep_count = ep_count; a.ep_return = ep_return;
  a.action = gz ? gz->action : nullptr; a.policy = gz ? gz->policy : nullptr;
  a.completed_q = gz ? gz->completed_q : nullptr; a.rec_policy = gz ? gz->rec_policy : nullptr;
  a.rec_cq = gz ? gz->rec_cq : nullptr;
  // (Pong is EfficientZero's game: no Gumbel step)
  void (*const kernel)(AtariArgs) = gz ? atari_collect_kernel<0, true>
                                       : game ? atari_collect_kernel<1, false> : atari_collect_kernel<0, false>;
  hipLaunchKernelGGL(kernel, dim3(n), dim3(kAtThreads), 0, (hipStream_t)stream, a);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_atari_reset(int n, int32_t *state, int32_t *steps, uint8_t *cur, float *obs, uint32_t seed, void *stream) {
  return atari_reset_g(0, "lzm_atari_reset", n, state, steps, cur, obs, seed, stream);
}

int lzm_atari_collect_step(int n, int A, int T, int E, const int32_t *visits, const float *root_value,
                           const float *pred_value, int32_t *state, int32_t *steps, uint8_t *cur, float *obs,
                           float *noises, float noise_alpha, float temperature, int deterministic, uint8_t *rec_frames,
                           int32_t *rec_action, float *rec_reward, int32_t *rec_visits, float *rec_value,
                           float *rec_pred, int32_t *ep_len, int32_t *ep_count, float *ep_return, int max_steps,
                           uint32_t seed, const int64_t *counter, void *stream) {
  return atari_collect_step_g(0, "lzm_atari_collect_step", nullptr, n, A, T, E, visits, root_value, pred_value, state,
                              steps, cur, obs, noises, noise_alpha, temperature, deterministic, rec_frames, rec_action,
                              rec_reward, rec_visits, rec_value, rec_pred, ep_len, ep_count, ep_return, max_steps, seed,
                              counter, stream);
}

int lzm_atari_collect_step_gumbel(int n, int A, int T, int E, const int32_t *visits, const float *root_value,
                                  const float *pred_value, const int32_t *action, const float *policy,
                                  const float *completed_q, int32_t *state, int32_t *steps, uint8_t *cur, float *obs,
                                  float *noises, float noise_alpha, uint8_t *rec_frames, int32_t *rec_action,
                                  float *rec_reward, int32_t *rec_visits, float *rec_value, float *rec_pred,
                                  float *rec_policy, float *rec_cq, int32_t *ep_len, int32_t *ep_count,
                                  float *ep_return, int max_steps, uint32_t seed, const int64_t *counter,
                                  void *stream) {
  const GumbelStepIO gz{action, policy, completed_q, rec_policy, rec_cq};
  return atari_collect_step_g(0, "lzm_atari_collect_step_gumbel", &gz, n, A, T, E, visits, root_value, pred_value,
                              state, steps, cur, obs, noises, noise_alpha, 1.0f, 1, rec_frames, rec_action, rec_reward,
                              rec_visits, rec_value, rec_pred, ep_len, ep_count, ep_return, max_steps, seed, counter,
                              stream);
}

int lzm_pong_reset(int n, int32_t *state, int32_t *steps, uint8_t *cur, float *obs, uint32_t seed, void *stream) {
  return atari_reset_g(1, "lzm_pong_reset", n, state, steps, cur, obs, seed, stream);
}

int lzm_pong_collect_step(int n, int A, int T, int E, const int32_t *visits, const float *root_value,
                          const float *pred_value, int32_t *state, int32_t *steps, uint8_t *cur, float *obs,
                          float *noises, float noise_alpha, float temperature, int deterministic, uint8_t *rec_frames,
                          int32_t *rec_action, float *rec_reward, int32_t *rec_visits, float *rec_value,
                          float *rec_pred, int32_t *ep_len, int32_t *ep_count, float *ep_return, int max_steps,
                          uint32_t seed, const int64_t *counter, void *stream) {
  return atari_collect_step_g(1, "lzm_pong_collect_step", nullptr, n, A, T, E, visits, root_value, pred_value, state,
                              steps, cur, obs, noises, noise_alpha, temperature, deterministic, rec_frames, rec_action,
                              rec_reward, rec_visits, rec_value, rec_pred, ep_len, ep_count, ep_return, max_steps, seed,
                              counter, stream);
}

int lzm_episodes_scan(int n, int E, const int32_t *ep_count, const int32_t *consumed, const int32_t *ep_len,
                      int32_t *env_ep_off, int64_t *env_row_off, int64_t *totals, void *stream) {
  if (n <= 0 || E <= 0 || !ep_count || !consumed || !ep_len || !env_ep_off || !env_row_off || !totals) {
    set_err("lzm_episodes_scan: bad arguments");
    return LZM_ERR_ARG;
  }
  hipLaunchKernelGGL(episodes_scan_kernel, dim3(1), dim3(kTrScanThreads), 0, (hipStream_t)stream, n, E, ep_count,
                     consumed, ep_len, env_ep_off, env_row_off, totals);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// the conv representation network's per-convolution epilogue (include/lzmcts.h lzm_bias_add_relu):
// one float4 per thread, HBM-bound (one read of y (and z), one write)
__global__ __launch_bounds__(256) void bias_add_relu_kernel(float4 *__restrict__ y, const float *__restrict__ bias,
                                                            const float4 *__restrict__ z, int C, int HW4, long long n4,
                                                            int relu) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  if (q >= n4) return;
  const float b = bias[(int)((q / HW4) % C)];
  float4 v = y[q];
  v.x += b; v.y += b; v.z += b; v.w += b;
  if (z) {
    const float4 r = z[q];
    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
  }
  if (relu) {
    v.x = fmaxf(v.x, 0.0f); v.y = fmaxf(v.y, 0.0f); v.z = fmaxf(v.z, 0.0f); v.w = fmaxf(v.w, 0.0f);
  }
  y[q] = v;
}

int lzm_bias_add_relu(float *y, const float *bias, const float *z, int N, int C, int HW, int relu, void *stream) {
  if (!y || !bias || N <= 0 || C <= 0 || HW <= 0 || HW % 4 || ((uintptr_t)y & 15) || ((uintptr_t)z & 15)) {
    set_err("lzm_bias_add_relu: bad arguments (HW % 4 == 0, 16-B aligned rows)");
    return LZM_ERR_ARG;
  }
  const long long n4 = (long long)N * C * (HW / 4);
  hipLaunchKernelGGL(bias_add_relu_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     reinterpret_cast<float4 *>(y), bias, reinterpret_cast<const float4 *>(z), C, HW / 4, n4,
                     relu ? 1 : 0);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

}  // extern "C"

// lzm_episodes_pack (rec_policy and rec_cq null) and lzm_episodes_pack_gumbel (both given: A + 1 more columns)
static int episodes_pack_g(const char *name, int n, int E, int T, int A, int has_pred, int64_t frame_bytes,
                           const int32_t *ep_count, const int32_t *ep_len, int32_t *consumed, const int32_t *env_ep_off,
                           const int64_t *env_row_off, const void *rec_frames, const int32_t *rec_action,
                           const float *rec_reward, const int32_t *rec_visits, const float *rec_value,
                           const float *rec_pred, const float *rec_policy, const float *rec_cq, const float *ep_return,
                           void *out_frames, float *out_scalars, int64_t *out_index, void *stream) {
  if (n <= 0 || E <= 0 || T <= 0 || A <= 0 || frame_bytes <= 0 || !ep_count || !ep_len || !consumed ||
      !env_ep_off || !env_row_off || !rec_frames || !rec_action || !rec_reward || !rec_visits || !rec_value ||
      (has_pred && !rec_pred) || (!rec_policy) != (!rec_cq) || !out_frames || !out_scalars || !out_index) {
    snprintf(g_err, sizeof(g_err), "%s: bad arguments", name);
    return LZM_ERR_ARG;
  }
  PackArgs a;
  a.n = n; a.E = E; a.T = T; a.A = A; a.has_pred = has_pred ? 1 : 0;
  a.W = 3 + A + a.has_pred + (rec_policy ? A + 1 : 0);
  a.rec_policy = rec_policy; a.rec_cq = rec_cq;
  a.frame_bytes = frame_bytes; a.ep_count = ep_count; a.ep_len = ep_len; a.env_ep_off = env_ep_off;
  a.consumed = consumed; a.env_row_off = env_row_off;
  a.rec_frames = (const uint8_t *)rec_frames; a.rec_action = rec_action; a.rec_reward = rec_reward;
  a.rec_visits = rec_visits; a.rec_value = rec_value; a.rec_pred = rec_pred; a.ep_return = ep_return;
  a.out_frames = (uint8_t *)out_frames; a.out_scalars = out_scalars; a.out_index = out_index;
  if ((frame_bytes & 15) == 0 && (((uintptr_t)rec_frames | (uintptr_t)out_frames) & 15)) {
    snprintf(g_err, sizeof(g_err), "%s: frame buffers must be 16-B aligned when frames are multiples of 16 B", name);
    return LZM_ERR_ARG;
  }
  hipLaunchKernelGGL(episodes_pack_kernel, dim3(n), dim3(kTrPackThreads), 0, (hipStream_t)stream, a);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

extern "C" {

int lzm_episodes_pack(int n, int E, int T, int A, int has_pred, int64_t frame_bytes, const int32_t *ep_count,
                      const int32_t *ep_len, int32_t *consumed, const int32_t *env_ep_off, const int64_t *env_row_off,
                      const void *rec_frames, const int32_t *rec_action, const float *rec_reward,
                      const int32_t *rec_visits, const float *rec_value, const float *rec_pred,
                      const float *ep_return, void *out_frames, float *out_scalars, int64_t *out_index,
                      void *stream) {
  return episodes_pack_g("lzm_episodes_pack", n, E, T, A, has_pred, frame_bytes, ep_count, ep_len, consumed, env_ep_off,
                         env_row_off, rec_frames, rec_action, rec_reward, rec_visits, rec_value, rec_pred, nullptr,
                         nullptr, ep_return, out_frames, out_scalars, out_index, stream);
}

int lzm_episodes_pack_gumbel(int n, int E, int T, int A, int has_pred, int64_t frame_bytes, const int32_t *ep_count,
                             const int32_t *ep_len, int32_t *consumed, const int32_t *env_ep_off,
                             const int64_t *env_row_off, const void *rec_frames, const int32_t *rec_action,
                             const float *rec_reward, const int32_t *rec_visits, const float *rec_value,
                             const float *rec_pred, const float *rec_policy, const float *rec_cq,
                             const float *ep_return, void *out_frames, float *out_scalars, int64_t *out_index,
                             void *stream) {
  if (!rec_policy || !rec_cq) {
    set_err("lzm_episodes_pack_gumbel: bad arguments");
    return LZM_ERR_ARG;
  }
  return episodes_pack_g("lzm_episodes_pack_gumbel", n, E, T, A, has_pred, frame_bytes, ep_count, ep_len, consumed,
                         env_ep_off, env_row_off, rec_frames, rec_action, rec_reward, rec_visits, rec_value, rec_pred,
                         rec_policy, rec_cq, ep_return, out_frames, out_scalars, out_index, stream);
}

}  // extern "C"

// ---- batched AlphaZero (lzm_az.h). One workspace buffer per (B, S), carved here.
static int64_t az_carve(int B, int S, void *ws, AzTree *t) {
  const int64_t cap = 1 + (int64_t)kAzCells * (S + 1);
  char *p = (char *)ws;
  int64_t off = 0;
  auto take = [&](int64_t bytes) -> void * {
    void *r = p ? (void *)(p + off) : nullptr;
    off += (bytes + 255) & ~(int64_t)255;
    return r;
  };
  AzTree x;
  x.B = B; x.S = S; x.cap = (int)cap;
  const int64_t nodes = (int64_t)B * cap;
  x.visit = (int32_t *)take(nodes * 4);
  x.vsum = (float *)take(nodes * 4);
  x.prior = (float *)take(nodes * 4);
  x.first = (int32_t *)take(nodes * 4);
  x.nch = (int32_t *)take(nodes * 4);
  x.act = (int32_t *)take(nodes * 4);
  x.nnodes = (int32_t *)take((int64_t)B * 4);
  x.root_board = (int32_t *)take((int64_t)B * kAzCells * 4);
  x.root_player = (int32_t *)take((int64_t)B * 4);
  x.path = (int32_t *)take((int64_t)B * kAzPath * 4);
  x.leaf = (int32_t *)take((int64_t)B * 4 * 4);
  x.leaf_board = (int32_t *)take((int64_t)B * kAzCells * 4);
  x.lut_pb = (double *)take((int64_t)(S + 1) * 8);
  x.lut_sqrt = (double *)take((int64_t)(S + 1) * 8);
  x.noise = (double *)take((int64_t)kAzCells * kAzCells * 8);
  if (t) *t = x;
  return off;
}

static bool az_args_ok(int B, int S, const void *ws, const char *what) {
  if (B <= 0 || S <= 0 || S > (1 << 20) || !ws) {
    snprintf(g_err, sizeof(g_err), "%s: need B > 0, 0 < num_simulations <= 2^20 and a workspace", what);
    return false;
  }
  return true;
}

extern "C" {

int lzm_az_workspace_bytes(int B, int S, int64_t *out) {
  if (B <= 0 || S <= 0 || S > (1 << 20) || !out) {
    set_err("lzm_az_workspace_bytes: need B > 0, 0 < num_simulations <= 2^20");
    return LZM_ERR_ARG;
  }
  *out = az_carve(B, S, nullptr, nullptr);
  return LZM_OK;
}

int lzm_az_noise_table(double alpha, int max_n, double *out) {
  if (!(alpha > 0.0) || max_n <= 0 || max_n > 4096 || !out) {
    set_err("lzm_az_noise_table: need alpha > 0, 0 < max_n <= 4096");
    return LZM_ERR_ARG;
  }
  // _add_exploration_noise (mcts_alphazero.cpp:57-83): a default-seeded engine per call, so the
  // vector for n children is fixed: n gamma(alpha, 1) draws, each divided by their sum
  for (int n = 1; n <= max_n; ++n) {
    std::default_random_engine gen;
    std::gamma_distribution<double> dist(alpha, 1.0);
    std::vector<double> g((size_t)n);
    double sum = 0;
    for (int i = 0; i < n; ++i) {
      g[(size_t)i] = dist(gen);
      sum += g[(size_t)i];
    }
    for (int i = 0; i < max_n; ++i) out[(size_t)(n - 1) * max_n + i] = i < n ? g[(size_t)i] / sum : 0.0;
  }
  return LZM_OK;
}

int lzm_az_set_constants(int B, int S, void *ws, double pb_c_base, double pb_c_init, double alpha, void *stream) {
  if (!az_args_ok(B, S, ws, "lzm_az_set_constants")) return LZM_ERR_ARG;
  if (!(pb_c_base > 0.0) || !(alpha > 0.0)) {
    set_err("lzm_az_set_constants: need pb_c_base > 0 and alpha > 0");
    return LZM_ERR_ARG;
  }
  AzTree t;
  az_carve(B, S, ws, &t);
  // _ucb_score (mcts_alphazero.cpp:47-54) over the integer parent count: glibc log / sqrt on the host
  std::vector<double> pb((size_t)S + 1), sq((size_t)S + 1), nz((size_t)kAzCells * kAzCells);
  for (int n = 0; n <= S; ++n) {
    pb[(size_t)n] = std::log((n + pb_c_base + 1) / pb_c_base) + pb_c_init;
    sq[(size_t)n] = std::sqrt((double)n);
  }
  lzm_az_noise_table(alpha, kAzCells, nz.data());
  hipStream_t s = (hipStream_t)stream;
  LZM_HIP(hipMemcpyAsync(t.lut_pb, pb.data(), pb.size() * 8, hipMemcpyHostToDevice, s));
  LZM_HIP(hipMemcpyAsync(t.lut_sqrt, sq.data(), sq.size() * 8, hipMemcpyHostToDevice, s));
  LZM_HIP(hipMemcpyAsync(t.noise, nz.data(), nz.size() * 8, hipMemcpyHostToDevice, s));
  LZM_HIP(hipStreamSynchronize(s));
  return LZM_OK;
}

int lzm_az_begin(int B, int S, void *ws, const int32_t *boards, const int32_t *start_index, float *state,
                 void *stream) {
  if (!az_args_ok(B, S, ws, "lzm_az_begin")) return LZM_ERR_ARG;
  if (!boards || !start_index || !state) {
    set_err("lzm_az_begin: null buffer");
    return LZM_ERR_ARG;
  }
  AzTree t;
  az_carve(B, S, ws, &t);
  const int per = kAzThreads / kAzGroup;
  hipLaunchKernelGGL(az_begin_kernel, dim3((B + per - 1) / per), dim3(kAzThreads), 0, (hipStream_t)stream, t,
                     boards, start_index, state);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_az_step(int B, int S, void *ws, int sim, const float *probs, int pstride, const float *values, int vstride,
                int with_noise, double noise_weight, float *state, void *stream) {
  if (!az_args_ok(B, S, ws, "lzm_az_step")) return LZM_ERR_ARG;
  if (sim < -1 || sim >= S || !probs || pstride < kAzCells || (sim >= 0 && (!values || vstride < 1)) || !state) {
    set_err("lzm_az_step: need -1 <= sim < num_simulations, probs [B][>=9], values [B] and a state buffer");
    return LZM_ERR_ARG;
  }
  AzTree t;
  az_carve(B, S, ws, &t);
  AzStepArgs a;
  a.sim = sim; a.with_noise = with_noise; a.noise_weight = noise_weight;
  a.probs = probs; a.pstride = pstride; a.values = values ? values : probs; a.vstride = vstride; a.state = state;
  const int per = kAzThreads / kAzGroup;
  hipLaunchKernelGGL(az_step_kernel, dim3((B + per - 1) / per), dim3(kAzThreads), 0, (hipStream_t)stream, t, a);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_az_finish(int B, int S, void *ws, double temperature, int sample, uint32_t seed, const int64_t *counter,
                  int32_t *visits, double *probs, int32_t *action, void *stream) {
  if (!az_args_ok(B, S, ws, "lzm_az_finish")) return LZM_ERR_ARG;
  if (temperature == 0.0 || !visits || !probs || !action) {
    set_err("lzm_az_finish: temperature cannot be 0; visits / probs / action buffers required");
    return LZM_ERR_ARG;
  }
  AzTree t;
  az_carve(B, S, ws, &t);
  hipLaunchKernelGGL(az_finish_kernel, dim3((B + 127) / 128), dim3(128), 0, (hipStream_t)stream, t, temperature,
                     sample, seed, counter, visits, probs, action);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_az_export_tree(int B, int S, void *ws, int32_t *visit, float *vsum, int32_t *first, int32_t *nnodes,
                       void *stream) {
  if (!az_args_ok(B, S, ws, "lzm_az_export_tree")) return LZM_ERR_ARG;
  AzTree t;
  az_carve(B, S, ws, &t);
  hipStream_t s = (hipStream_t)stream;
  const size_t nodes = (size_t)B * t.cap;
  if (visit) LZM_HIP(hipMemcpyAsync(visit, t.visit, nodes * 4, hipMemcpyDeviceToDevice, s));
  if (vsum) LZM_HIP(hipMemcpyAsync(vsum, t.vsum, nodes * 4, hipMemcpyDeviceToDevice, s));
  if (first) LZM_HIP(hipMemcpyAsync(first, t.first, nodes * 4, hipMemcpyDeviceToDevice, s));
  if (nnodes) LZM_HIP(hipMemcpyAsync(nnodes, t.nnodes, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
  return LZM_OK;
}

int lzm_az_export_priors(int B, int S, void *ws, float *prior, void *stream) {
  if (!az_args_ok(B, S, ws, "lzm_az_export_priors") || !prior) {
    if (B > 0 && S > 0 && S <= (1 << 20) && ws) set_err("lzm_az_export_priors: null output");
    return LZM_ERR_ARG;
  }
  AzTree t;
  az_carve(B, S, ws, &t);
  LZM_HIP(hipMemcpyAsync(prior, t.prior, (size_t)B * t.cap * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return LZM_OK;
}

}  // extern "C"

// ---- fused AlphaZero search (lzm_az_fused.h)
template <int R>
static size_t az_fused_lds(int cap, int S) {
  // the double tables padded to 16 B, the node records, the network (az_search_fused_kernel's carve)
  const size_t bytes = (size_t)((2 * (S + 1) + 81 + 1) & ~1) * 8 + (size_t)R * cap * 16 + 128;
  return bytes + (size_t)AzNetLds<R>::total * 4;
}

template <int R, int NRES>
static int az_fused_attr(bool stamps) {
  static bool attr[2] = {false, false};
  if (!attr[stamps]) {
    LZM_HIP(hipFuncSetAttribute(stamps ? (const void *)az_search_fused_kernel<R, NRES, true>
                                       : (const void *)az_search_fused_kernel<R, NRES, false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr[stamps] = true;
  }
  return LZM_OK;
}

// workgroups of R boards that one CU holds at once (0: the trees do not fit in LDS). *assumed: the occupancy
// query failed and one workgroup per CU is assumed (lzm_az_fused_plan reports it)
template <int R, int NRES>
static int az_fused_per_cu(int cap, int S, bool stamps, bool *assumed = nullptr) {
  if (assumed) *assumed = false;
  const size_t lds = az_fused_lds<R>(cap, S);
  if (lds > 160 * 1024) return 0;
  static size_t memo_lds[2] = {0, 0};
  static int memo[2] = {0, 0};
  static bool memo_assumed[2] = {false, false};
  if (memo_lds[stamps] == lds) {
    if (assumed) *assumed = memo_assumed[stamps];
    return memo[stamps];
  }
  if (az_fused_attr<R, NRES>(stamps) != LZM_OK) return 0;
  int per_cu = 0;
  const bool failed =
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, stamps ? (const void *)az_search_fused_kernel<R, NRES, true>
                                                                   : (const void *)az_search_fused_kernel<R, NRES, false>,
                                                   kAzfThreads, lds) != hipSuccess;
  if (failed) per_cu = 1;
  memo_lds[stamps] = lds;
  memo[stamps] = per_cu;
  memo_assumed[stamps] = failed;
  if (assumed) *assumed = failed;
  return per_cu;
}

// boards per workgroup: the fewest whose grid the GPU holds at once (B = 512 on 256 CUs: one board per
// workgroup, two workgroups per CU, so each CU interleaves two boards' latency chains); else the most that fit
template <int NRES>
static int az_fused_rows(int B, int cap, int S, bool stamps) {
  const char *e = getenv("LZM_AZ_BOARDS_PER_WG");
  if (e && atoi(e) > 0) return atoi(e);
  const int cus = device_cus();
  const int occ[4] = {az_fused_per_cu<1, NRES>(cap, S, stamps), az_fused_per_cu<2, NRES>(cap, S, stamps),
                      az_fused_per_cu<4, NRES>(cap, S, stamps), az_fused_per_cu<8, NRES>(cap, S, stamps)};
  int best = 0;
  for (int i = 0, r = 1; i < 4; ++i, r *= 2) {
    if (!occ[i]) continue;
    best = r;
    if ((B + r - 1) / r <= occ[i] * cus) return r;
  }
  return best ? best : 1;
}

// lzm_az_fused_plan: what az_fused_rows picks and what that instantiation needs
template <int NRES>
static int az_fused_plan(int B, int cap, int S, bool stamps, int32_t *out) {
  const int R = az_fused_rows<NRES>(B, cap, S, stamps);
  bool assumed = false;
  int per_cu = 0;
  size_t lds = 0;
  switch (R) {
    case 1: per_cu = az_fused_per_cu<1, NRES>(cap, S, stamps, &assumed); lds = az_fused_lds<1>(cap, S); break;
    case 2: per_cu = az_fused_per_cu<2, NRES>(cap, S, stamps, &assumed); lds = az_fused_lds<2>(cap, S); break;
    case 4: per_cu = az_fused_per_cu<4, NRES>(cap, S, stamps, &assumed); lds = az_fused_lds<4>(cap, S); break;
    case 8: per_cu = az_fused_per_cu<8, NRES>(cap, S, stamps, &assumed); lds = az_fused_lds<8>(cap, S); break;
    default:
      set_err("lzm_az_fused_plan: boards per workgroup must be 1, 2, 4 or 8");
      return LZM_ERR_ARG;
  }
  out[0] = R;
  out[1] = (B + R - 1) / R;
  out[2] = assumed ? -1 : per_cu;
  out[3] = (int32_t)lds;
  return LZM_OK;
}

template <int R, int NRES>
static int az_launch_fused(const AzFusedArgs &a, hipStream_t s) {
  const size_t lds = az_fused_lds<R>(a.cap, a.S);
  if (lds > 160 * 1024) {
    snprintf(g_err, sizeof(g_err), "lzm_az_search_fused: %d boards x %d simulations need %zu B of LDS per workgroup (> 160 KiB)",
             R, a.S, lds);
    return LZM_ERR_CAPACITY;
  }
  // diagnostics: lzm_debug_az_stamps selects the stamped instantiation
  if (int rc = az_fused_attr<R, NRES>(a.stamps != nullptr)) return rc;
  auto fn = a.stamps ? az_search_fused_kernel<R, NRES, true> : az_search_fused_kernel<R, NRES, false>;
  hipLaunchKernelGGL(fn, dim3((a.B + R - 1) / R), dim3(kAzfThreads), lds, s, a);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

template <int NRES>
static int az_launch_fused_r(int R, const AzFusedArgs &a, hipStream_t s) {
  switch (R) {
    case 1: return az_launch_fused<1, NRES>(a, s);
    case 2: return az_launch_fused<2, NRES>(a, s);
    case 4: return az_launch_fused<4, NRES>(a, s);
    case 8: return az_launch_fused<8, NRES>(a, s);
  }
  set_err("lzm_az_search_fused: boards per workgroup must be 1, 2, 4 or 8");
  return LZM_ERR_ARG;
}

template <int R, int NRES>
static int az_launch_eval(const float *w, const float *state, int n, float *probs, float *value, hipStream_t s) {
  const size_t lds = (size_t)AzNetLds<R>::total * 4;
  static bool attr = false;
  if (!attr) {
    LZM_HIP(hipFuncSetAttribute((const void *)az_net_eval_kernel<R, NRES>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr = true;
  }
  hipLaunchKernelGGL((az_net_eval_kernel<R, NRES>), dim3((n + R - 1) / R), dim3(kAzfThreads), lds, s, w, state, n,
                     probs, value);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

static unsigned long long *g_az_stamps = nullptr;  // diagnostics: lzm_debug_az_stamps

extern "C" {

// Diagnostics: a device uint64[8] that the fused AlphaZero search adds its per-phase shader-clock cycles to
// (AzFusedArgs::stamps); nullptr returns to the production instantiation.
int lzm_debug_az_stamps(void *buf) {
  g_az_stamps = reinterpret_cast<unsigned long long *>(buf);
  return LZM_OK;
}

int64_t lzm_az_net_floats(int nres) { return nres == 1 || nres == 2 ? az_net_layout(nres).total : -1; }

int lzm_az_net_prepare(int nres, const float *raw, float *out) {
  if ((nres != 1 && nres != 2) || !raw || !out) {
    set_err("lzm_az_net_prepare: num_res_blocks must be 1 or 2");
    return LZM_ERR_ARG;
  }
  const AzNetLayout L = az_net_layout(nres);
  memset(out, 0, sizeof(float) * (size_t)L.total);
  const float *p = raw;
  const float *w0 = p; p += 16 * 27;
  const float *b0 = p; p += 16;
  for (int s = 0; s < 7; ++s)
    for (int lane = 0; lane < 64; ++lane) {
      const int k = 4 * s + (lane >> 4);
      out[L.conv0 + s * 64 + lane] = k < 27 ? w0[(lane & 15) * 27 + k] : 0.0f;
    }
  memcpy(out + L.conv0_b, b0, 16 * sizeof(float));
  for (int l = 0; l < 4 * nres; ++l) {
    const float *wl = p; p += 16 * 144;
    const float *bl = p; p += 16;
    for (int s = 0; s < 36; ++s)
      for (int lane = 0; lane < 64; ++lane)
        out[L.res + (l * 36 + s) * 64 + lane] = wl[(lane & 15) * 144 + 4 * s + (lane >> 4)];
    memcpy(out + L.res_b + l * 16, bl, 16 * sizeof(float));
  }
  const float *wh = p; p += 32 * 16;
  const float *bh = p; p += 32;
  for (int s = 0; s < 4; ++s)
    for (int nt = 0; nt < 2; ++nt)
      for (int lane = 0; lane < 64; ++lane)
        out[L.head + (s * 2 + nt) * 64 + lane] = wh[(16 * nt + (lane & 15)) * 16 + 4 * s + (lane >> 4)];
  memcpy(out + L.head_b, bh, 32 * sizeof(float));
  memcpy(out + L.heads, p, kAzHeadFloats * sizeof(float));
  return LZM_OK;
}

int lzm_az_net_eval(int nres, const float *weights, const float *state, int n, float *probs, float *value,
                    void *stream) {
  if ((nres != 1 && nres != 2) || !weights || !state || n <= 0 || !probs || !value) {
    set_err("lzm_az_net_eval: need num_res_blocks 1 or 2, n > 0 and all buffers");
    return LZM_ERR_ARG;
  }
  hipStream_t s = (hipStream_t)stream;
  return nres == 1 ? az_launch_eval<2, 1>(weights, state, n, probs, value, s)
                   : az_launch_eval<2, 2>(weights, state, n, probs, value, s);
}

int lzm_az_search_fused(int B, int S, void *ws, int nres, const float *weights, const int32_t *boards,
                        const int32_t *start_index, int with_noise, double noise_weight, double temperature,
                        int sample, uint32_t seed, const int64_t *counter, int32_t *visits, double *probs,
                        int32_t *action, int export_tree, void *stream) {
  if (!az_args_ok(B, S, ws, "lzm_az_search_fused")) return LZM_ERR_ARG;
  if ((nres != 1 && nres != 2) || !weights || !boards || !start_index || temperature == 0.0 || !visits || !probs ||
      !action) {
    set_err("lzm_az_search_fused: need num_res_blocks 1 or 2, temperature != 0 and all buffers");
    return LZM_ERR_ARG;
  }
  if (1 + kAzCells * (S + 1) >= 0xffff) {
    set_err("lzm_az_search_fused: num_simulations too large for the LDS tree (16-bit node index)");
    return LZM_ERR_CAPACITY;
  }
  AzFusedArgs a;
  az_carve(B, S, ws, &a.t);
  a.B = B; a.S = S; a.cap = a.t.cap; a.with_noise = with_noise; a.sample = sample; a.export_tree = export_tree;
  a.noise_weight = noise_weight; a.temperature = temperature; a.seed = seed; a.counter = counter; a.w = weights;
  a.boards = boards; a.start_index = start_index; a.visits_out = visits; a.probs_out = probs; a.action_out = action;
  a.stamps = g_az_stamps;
  const int R = nres == 1 ? az_fused_rows<1>(B, a.cap, S, a.stamps != nullptr) : az_fused_rows<2>(B, a.cap, S, a.stamps != nullptr);
  hipStream_t s = (hipStream_t)stream;
  return nres == 1 ? az_launch_fused_r<1>(R, a, s) : az_launch_fused_r<2>(R, a, s);
}

int lzm_az_fused_plan(int B, int S, int nres, int32_t *out) {
  if (B <= 0 || S <= 0 || S > (1 << 20) || (nres != 1 && nres != 2) || !out) {
    set_err("lzm_az_fused_plan: need B > 0, 0 < num_simulations <= 2^20, num_res_blocks 1 or 2 and an output buffer");
    return LZM_ERR_ARG;
  }
  if (1 + kAzCells * (S + 1) >= 0xffff) {
    set_err("lzm_az_fused_plan: num_simulations too large for the LDS tree (16-bit node index)");
    return LZM_ERR_CAPACITY;
  }
  const int cap = 1 + kAzCells * (S + 1);
  const bool stamps = g_az_stamps != nullptr;
  return nres == 1 ? az_fused_plan<1>(B, cap, S, stamps, out) : az_fused_plan<2>(B, cap, S, stamps, out);
}


int64_t lzm_conv_trunk_floats_p(int n_dres, int n_pres, int precision) {
  if (n_dres < 0 || n_pres < 0 || n_dres > 8 || n_pres > 8 || (precision != LZM_CONV_F32 && precision != LZM_CONV_SPLIT))
    return -1;
  return conv_trunk_layout_p(n_dres, n_pres, precision).total;
}

int64_t lzm_conv_trunk_floats(int n_dres, int n_pres) { return lzm_conv_trunk_floats_p(n_dres, n_pres, LZM_CONV_F32); }

int lzm_conv_trunk_prepare_p(int precision, int n_dres, int n_pres, int r_ch, int h_ch, const float *raw, float *out) {
  if (lzm_conv_trunk_floats_p(n_dres, n_pres, precision) < 0 || r_ch < 1 || r_ch > 32 || h_ch < 1 || h_ch > 32 ||
      !raw || !out) {
    set_err("lzm_conv_trunk_prepare: need 0..8 residual blocks, 1..32 reward / head channels, a known precision and "
            "buffers");
    return LZM_ERR_ARG;
  }
  const bool bx = precision == LZM_CONV_SPLIT;
  const ConvTrunkLayout L = conv_trunk_layout_p(n_dres, n_pres, precision);
  const int frag3 = bx ? kBx3Frag : kCv3Frag, block = bx ? kBxBlock : kCvBlock;
  const int n3 = 1 + 2 * (n_dres + n_pres);
  // split: layer li's row scales at sc + 64 li, its bounds {Wb, Bb} at bd + 4 li (3x3 layers in order, then the
  // reward and head 1x1s); the dynamics conv's Bb (max |actmap|) is set by lzm_conv_trunk_actmap_bound
  auto pack3 = [&](const float *W, float *o, int li, const float *bias) {
    if (!bx) return conv_pack3(W, o);
    bx_pack3(W, o, out + L.sc + 64 * li, out + L.bd + 4 * li);
    out[L.bd + 4 * li + 1] = bias ? bx_bias_bound(bias, 64) : 0.f;
  };
  auto pack1 = [&](const float *W, int n, float *o, int li, const float *bias) {
    if (!bx) return conv_pack1(W, n, o);
    bx_pack1(W, n, o, out + L.sc + 64 * li, out + L.bd + 4 * li);
    out[L.bd + 4 * li + 1] = bx_bias_bound(bias, n);
  };
  memset(out, 0, sizeof(float) * (size_t)L.total);
  const float *r = raw;
  const int W3 = 64 * 64 * 9;
  pack3(r, out + L.dyn, 0, nullptr); r += W3;
  auto blocks = [&](int n, int base, int li0) {
    for (int k = 0; k < n; ++k) {
      float *o = out + base + k * block;
      pack3(r, o, li0 + 2 * k, r + W3); r += W3;
      memcpy(o + frag3, r, 64 * sizeof(float)); r += 64;
      pack3(r, o + frag3 + 64, li0 + 2 * k + 1, r + W3); r += W3;
      memcpy(o + 2 * frag3 + 64, r, 64 * sizeof(float)); r += 64;
    }
  };
  blocks(n_dres, L.dres, 1);
  pack1(r, r_ch, out + L.rw, n3, r + r_ch * 64); r += r_ch * 64;
  memcpy(out + L.rb, r, r_ch * sizeof(float)); r += r_ch;
  blocks(n_pres, L.pres, 1 + 2 * n_dres);
  pack1(r, h_ch, out + L.hw, n3 + 1, r + h_ch * 64); r += h_ch * 64;
  memcpy(out + L.hb, r, h_ch * sizeof(float));
  return LZM_OK;
}

int lzm_conv_trunk_actmap_bound(int n_dres, int n_pres, float actmap_absmax, float *packed) {
  if (lzm_conv_trunk_floats_p(n_dres, n_pres, LZM_CONV_SPLIT) < 0 || !packed || !(actmap_absmax >= 0.f)) {
    set_err("lzm_conv_trunk_actmap_bound: a split-layout blob and a finite max |actmap| >= 0");
    return LZM_ERR_ARG;
  }
  packed[conv_trunk_layout_p(n_dres, n_pres, LZM_CONV_SPLIT).bd + 1] = bx_round_up(actmap_absmax);
  return LZM_OK;
}

int lzm_conv_trunk_prepare(int n_dres, int n_pres, int r_ch, int h_ch, const float *raw, float *out) {
  return lzm_conv_trunk_prepare_p(LZM_CONV_F32, n_dres, n_pres, r_ch, h_ch, raw, out);
}

int lzm_conv_trunk_xin_p(int precision, int B, int n_dres, int n_pres, int r_ch, int h_ch, const float *weights,
                         const float *actmap, const float *pool, const int32_t *x, const int32_t *action,
                         float *out_latent, float *xin, int xin_stride, const float *hpool, int H, int32_t *xscale,
                         float *out_h, int32_t *err, void *stream) {
  if (B <= 0 || lzm_conv_trunk_floats_p(n_dres, n_pres, precision) < 0 || r_ch < 1 || r_ch > 32 || h_ch < 1 ||
      h_ch > 32 || !weights || !actmap || !pool || !action || !out_latent || !xin || !out_h ||
      xin_stride < r_ch * 64 + (hpool ? H : 0) || (hpool && (H <= 0 || H % 4)) || xin_stride % 4) {
    set_err("lzm_conv_trunk: bad arguments");
    return LZM_ERR_ARG;
  }
  if (((uintptr_t)weights | (uintptr_t)pool | (uintptr_t)xin | (uintptr_t)hpool) & 15) {
    set_err("lzm_conv_trunk: weights, pool, xin and hpool must be 16-byte aligned");
    return LZM_ERR_ARG;
  }
  float *out_r = xin;
  const bool bx = precision == LZM_CONV_SPLIT;
  static std::once_flag once;
  static hipError_t attr_err = hipSuccess;
  const size_t lds_f32 = 3 * kCvBuf * sizeof(float), lds_bx = 2 * kBxBuf * sizeof(uint16_t);
  std::call_once(once, [&] {
    attr_err = hipFuncSetAttribute((const void *)conv_trunk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)lds_f32);
    if (attr_err == hipSuccess)
      attr_err = hipFuncSetAttribute((const void *)conv_trunk_bx_kernel<kBxAhead>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bx);
  });
  LZM_HIP(attr_err);
  ConvTrunkArgs a;
  a.B = B; a.n_dres = n_dres; a.n_pres = n_pres; a.r_ch = r_ch; a.h_ch = h_ch; a.w = weights; a.actmap = actmap;
  a.pool = pool; a.x = x; a.action = action; a.out_latent = out_latent; a.out_r = out_r; a.out_h = out_h;
  a.r_stride = xin_stride; a.hpool = hpool; a.H = hpool ? H : 0; a.skip_dyn = 0; a.err = err;
  a.xscale = precision == LZM_CONV_SPLIT ? xscale : nullptr;
  if (bx)
    hipLaunchKernelGGL(conv_trunk_bx_kernel<kBxAhead>, dim3(B), dim3(kCvThreads), lds_bx, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(conv_trunk_kernel, dim3(B), dim3(kCvThreads), lds_f32, (hipStream_t)stream, a);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_conv_trunk_p(int precision, int B, int n_dres, int n_pres, int r_ch, int h_ch, const float *weights,
                     const float *actmap, const float *pool, const int32_t *x, const int32_t *action, float *out_latent,
                     float *out_r, float *out_h, int32_t *err, void *stream) {
  return lzm_conv_trunk_xin_p(precision, B, n_dres, n_pres, r_ch, h_ch, weights, actmap, pool, x, action, out_latent,
                              out_r, r_ch * 64, nullptr, 0, nullptr, out_h, err, stream);
}

int lzm_conv_resnet8_p(int B, int n_blocks, int n_pres, int h_ch, const float *weights, const float *in,
                       float *out_latent, float *out_h, int32_t *err, void *stream) {
  if (B <= 0 || n_blocks < 1 || lzm_conv_trunk_floats_p(n_blocks, n_pres, LZM_CONV_SPLIT) < 0 || h_ch < 1 ||
      h_ch > 32 || !weights || !in || !out_latent || !out_h || (((uintptr_t)weights | (uintptr_t)in) & 15)) {
    set_err("lzm_conv_resnet8_p: bad arguments (1..8 blocks, 1..32 head channels, 16-byte aligned weights / input)");
    return LZM_ERR_ARG;
  }
  static hipError_t attr_err = hipFuncSetAttribute((const void *)conv_trunk_bx_kernel<kBxAhead>,
                                                   hipFuncAttributeMaxDynamicSharedMemorySize,
                                                   (int)(2 * kBxBuf * sizeof(uint16_t)));
  LZM_HIP(attr_err);
  ConvTrunkArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.n_dres = n_blocks; a.n_pres = n_pres; a.r_ch = 0; a.h_ch = h_ch; a.w = weights;
  a.pool = in; a.out_latent = out_latent; a.out_h = out_h; a.skip_dyn = 1; a.err = err;
  hipLaunchKernelGGL((conv_trunk_bx_kernel<kBxAhead>), dim3(B), dim3(kCvThreads), 2 * kBxBuf * sizeof(uint16_t),
                     (hipStream_t)stream, a);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// ---- the representation network's DownSample stages (lzm_repr.h)
int64_t lzm_repr_floats(void) { return repr_layout().total; }

int lzm_repr_prepare(int cin, const float *raw, float *out) {
  if (cin < 1 || cin * 9 > 64 || !raw || !out) {
    set_err("lzm_repr_prepare: 1..7 observation channels and buffers");
    return LZM_ERR_ARG;
  }
  const ReprLayout L = repr_layout();
  memset(out, 0, sizeof(float) * (size_t)L.total);
  const float *r = raw;
  auto bias = [&](int off, int n) { memcpy(out + off, r, n * sizeof(float)); r += n; };
  repr_pack(r, 32, cin, true, out + L.w1, out + L.s1); r += 32 * cin * 9; bias(L.b1, 32);
  repr_pack(r, 32, 32, false, out + L.r1w1, out + L.r1s1); r += 32 * 32 * 9; bias(L.r1b1, 32);
  repr_pack(r, 32, 32, false, out + L.r1w2, out + L.r1s2); r += 32 * 32 * 9; bias(L.r1b2, 32);
  // the downsample block: conv1 (64) and the shortcut conv3 (64) stacked as one 128-channel layer
  std::vector<float> dual((size_t)128 * 32 * 9);
  memcpy(dual.data(), r, sizeof(float) * 64 * 32 * 9); r += 64 * 32 * 9;
  bias(L.db1, 64);
  const float *w2 = r; r += 64 * 64 * 9;
  bias(L.db2, 64);
  memcpy(dual.data() + 64 * 32 * 9, r, sizeof(float) * 64 * 32 * 9); r += 64 * 32 * 9;
  repr_pack(dual.data(), 128, 32, false, out + L.dw, out + L.ds);
  repr_pack(w2, 64, 64, false, out + L.dw2, out + L.ds2);
  repr_pack(r, 64, 64, false, out + L.r2w1, out + L.r2s1); r += 64 * 64 * 9; bias(L.r2b1, 64);
  repr_pack(r, 64, 64, false, out + L.r2w2, out + L.r2s2); r += 64 * 64 * 9; bias(L.r2b2, 64);
  return LZM_OK;
}

int64_t lzm_repr_workspace_floats(int B) { return B <= 0 ? -1 : (int64_t)B * (2 * 32 * 32 * 32 + 2 * 16 * 16 * 64); }

}  // extern "C"

template <int CIN, int COUT, int STRIDE, int WOUT, int MODE, bool RES>
static int repr_launch(const ReprConvArgs &a, hipStream_t s) {
  typedef ReprGeom<CIN, COUT, STRIDE, WOUT, MODE, RES> G;
  const size_t lds = G::LDSB;
  static hipError_t attr = hipFuncSetAttribute((const void *)repr_conv_kernel<CIN, COUT, STRIDE, WOUT, MODE, RES>,
                                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  LZM_HIP(attr);
  const int grid = std::min(a.ntiles, device_cus());
  hipLaunchKernelGGL((repr_conv_kernel<CIN, COUT, STRIDE, WOUT, MODE, RES>), dim3(grid), dim3(kRpThreads), lds, s, a);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

extern "C" {

int lzm_repr_downsample(int B, int cin, const float *w, const float *obs, float *ws, float *out, void *stream) {
  if (B <= 0 || cin < 1 || cin * 9 > 64 || !w || !obs || !ws || !out ||
      (((uintptr_t)w | (uintptr_t)ws | (uintptr_t)out) & 15)) {
    set_err("lzm_repr_downsample: bad arguments (1..7 observation channels, 16-byte aligned weights / workspace)");
    return LZM_ERR_ARG;
  }
  const ReprLayout L = repr_layout();
  hipStream_t s = (hipStream_t)stream;
  float *A0 = ws, *A1 = ws + (size_t)B * 32768, *D0 = ws + (size_t)B * 65536, *D1 = D0 + (size_t)B * 16384;
  ReprConvArgs a;
  memset(&a, 0, sizeof(a));
  a.B = B; a.cin_obs = cin;
  int rc;
  // L1: obs (NCHW 64 x 64) -> A0 [32][32][32] (128-pixel tiles: 8 per image)
  a.ntiles = B * 8; a.in = obs; a.w = w + L.w1; a.winv = w + L.s1; a.bias = w + L.b1; a.res = nullptr; a.out = A0;
  if ((rc = repr_launch<32, 32, 2, 32, 2, false>(a, s)) != LZM_OK) return rc;
  // resblocks1: A0 -> A1 -> A0 (+ A0)
  a.in = A0; a.w = w + L.r1w1; a.winv = w + L.r1s1; a.bias = w + L.r1b1; a.out = A1;
  if ((rc = repr_launch<32, 32, 1, 32, 0, false>(a, s)) != LZM_OK) return rc;
  a.in = A1; a.w = w + L.r1w2; a.winv = w + L.r1s2; a.bias = w + L.r1b2; a.res = A0; a.out = A0;
  if ((rc = repr_launch<32, 32, 1, 32, 0, true>(a, s)) != LZM_OK) return rc;
  // the downsample block: A0 -> D0 = relu(conv1 + b1), D1 = conv3 (shortcut); D1 = relu(conv2(D0) + b2 + D1)
  a.ntiles = B * 4; a.in = A0; a.w = w + L.dw; a.winv = w + L.ds; a.bias = w + L.db1; a.res = nullptr; a.out = D0;
  a.out2 = D1;
  if ((rc = repr_launch<32, 128, 2, 16, 1, false>(a, s)) != LZM_OK) return rc;
  a.in = D0; a.w = w + L.dw2; a.winv = w + L.ds2; a.bias = w + L.db2; a.res = D1; a.out = D1; a.out2 = nullptr;
  if ((rc = repr_launch<64, 64, 1, 16, 0, true>(a, s)) != LZM_OK) return rc;
  // resblocks2: D1 -> D0 -> D1 (+ D1)
  a.in = D1; a.w = w + L.r2w1; a.winv = w + L.r2s1; a.bias = w + L.r2b1; a.res = nullptr; a.out = D0;
  if ((rc = repr_launch<64, 64, 1, 16, 0, false>(a, s)) != LZM_OK) return rc;
  a.in = D0; a.w = w + L.r2w2; a.winv = w + L.r2s2; a.bias = w + L.r2b2; a.res = D1; a.out = D1;
  if ((rc = repr_launch<64, 64, 1, 16, 0, true>(a, s)) != LZM_OK) return rc;
  // avg pool -> out NCHW [B][64][8][8]
  hipLaunchKernelGGL(repr_avgpool_kernel, dim3(B), dim3(256), 0, s, D1, out, B);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

int lzm_conv_trunk(int B, int n_dres, int n_pres, int r_ch, int h_ch, const float *weights, const float *actmap,
                   const float *pool, const int32_t *x, const int32_t *action, float *out_latent, float *out_r,
                   float *out_h, void *stream) {
  return lzm_conv_trunk_p(LZM_CONV_F32, B, n_dres, n_pres, r_ch, h_ch, weights, actmap, pool, x, action, out_latent,
                          out_r, out_h, nullptr, stream);
}

}  // extern "C"

// the head shapes lzm_conv_heads takes (pred_only: no reward head, Kr unused): what conv_infer.pack_heads asks
// through lzm_conv_heads_supported before it hands a network's heads to the kernel
static bool heads_shape_ok(bool pred_only, int Kr, int Khd, int off_policy, int Vr, int Vv, int A) {
  constexpr int kMaxCols = kHdColsWide * kHdThreads;
  return (pred_only || (Kr > 0 && Kr <= kHdRMax && !(Kr & 3))) && Khd > 0 && Khd <= kHdHMax && off_policy > 0 &&
         off_policy < Khd && Khd - off_policy <= kHdKMax && off_policy <= kHdKMax && Vr > 0 && Vv > 0 && A > 0 &&
         Vr <= kMaxCols && Vv <= kMaxCols && A <= kMaxCols && !(Khd & 3) && !(off_policy & 3);
}
extern "C" int lzm_conv_heads_supported(int Kr, int Khd, int off_policy, int Vr, int Vv, int A) {
  return heads_shape_ok(false, Kr, Khd, off_policy, Vr, Vv, A) ? 1 : 0;
}

extern "C" int lzm_conv_heads(int B, int Kr, int Khd, int off_policy, const float *r, const float *r_scale,
                              const float *r_shift, const float *hd, const float *w1t, const float *b1,
                              const float *w2t, const float *b2, int Vr, int Vv, int A, float *reward, float *value,
                              float *policy, int32_t *norm_words, void *stream) {
  // r == NULL: the prediction heads only (value, policy: initial_inference), reward / norm_words unused
  const bool pred_only = !r;
  if (B <= 0 || !heads_shape_ok(pred_only, Kr, Khd, off_policy, Vr, Vv, A) || (!pred_only && !reward) || !hd || !w1t ||
      !b1 || !w2t || !b2 || !value || !policy || (!r_scale) != (!r_shift) || ((uintptr_t)w1t & 15)) {
    set_err("lzm_conv_heads: bad arguments (Kr <= 1024, head planes <= 2048, K per head <= 1024, supports and actions "
            "<= 1024, 16-B aligned w1t)");
    return LZM_ERR_ARG;
  }
  HeadsArgs p;
  p.B = B; p.Kr = Kr; p.Khd = Khd;
  p.r = r; p.r_scale = r_scale; p.r_shift = r_shift; p.hd = hd;
  p.src[0] = 0; p.off[0] = 0; p.K[0] = Kr;
  p.src[1] = 1; p.off[1] = 0; p.K[1] = off_policy;
  p.src[2] = 1; p.off[2] = off_policy; p.K[2] = Khd - off_policy;
  p.w1t = w1t; p.b1 = b1; p.w2t = w2t; p.b2 = b2;
  p.Vr = Vr; p.Vv = Vv; p.A = A;
  p.reward = reward; p.value = value; p.policy = policy;
  p.norm_words = pred_only ? nullptr : norm_words; p.norm_nparts = norm_parts(B);
  p.head0 = pred_only ? 1 : 0;
  p.prep_on = 0;
  // three output columns per thread (the Atari supports); the four-column instantiation past 768
  const dim3 grid((B + kHdEnvs - 1) / kHdEnvs, pred_only ? 2 : 3);
  if (std::max(Vr, std::max(Vv, A)) <= kHdCols * kHdThreads)
    hipLaunchKernelGGL(conv_heads_kernel<kHdCols>, grid, dim3(kHdThreads), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(conv_heads_kernel<kHdColsWide>, grid, dim3(kHdThreads), 0, (hipStream_t)stream, p);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// The initial inference's prediction heads (lzm_conv_heads with r == NULL) and, in the same launch, the root
// preparation from the policy logits (lzm_roots_prepare's arguments and bits): the policy-head workgroups run
// CRoots::prepare (cnode.cpp:301-358) for their envs from their LDS copy of the logits.
extern "C" int lzm_conv_heads_prepare(lzm_handle *h, int B, int Khd, int off_policy, const float *hd,
                                      const float *w1t, const float *b1, const float *w2t, const float *b2, int Vr,
                                      int Vv, int A, float *value, float *policy, const int32_t *legal,
                                      const int32_t *count, const float *noises, float noise_weight,
                                      const float *rewards, const int32_t *to_play, void *stream) {
  if (!h || h->B != B || h->A != A || A > kHdThreads || !legal || !count || !rewards || !to_play) {
    set_err("lzm_conv_heads_prepare: the handle must have B roots and A <= 256 actions; legal, count, rewards, "
            "to_play required");
    return LZM_ERR_ARG;
  }
  if (B <= 0 || !heads_shape_ok(true, 0, Khd, off_policy, Vr, Vv, A) || !hd || !w1t || !b1 || !w2t || !b2 || !value ||
      !policy || ((uintptr_t)w1t & 15)) {
    set_err("lzm_conv_heads_prepare: bad arguments (head planes <= 2048, K per head <= 1024, supports <= 1024, "
            "16-B aligned w1t)");
    return LZM_ERR_ARG;
  }
  HeadsArgs p;
  memset(&p, 0, sizeof(p));
  p.B = B; p.Kr = 0; p.Khd = Khd;
  p.hd = hd;
  p.src[0] = 0; p.off[0] = 0; p.K[0] = 0;
  p.src[1] = 1; p.off[1] = 0; p.K[1] = off_policy;
  p.src[2] = 1; p.off[2] = off_policy; p.K[2] = Khd - off_policy;
  p.w1t = w1t; p.b1 = b1; p.w2t = w2t; p.b2 = b2;
  p.Vr = Vr; p.Vv = Vv; p.A = A;
  p.value = value; p.policy = policy;
  p.norm_nparts = norm_parts(B);
  p.head0 = 1;
  PrepareArgs &q = p.prep;
  q.stat = h->stat; q.meta = h->meta; q.legal = h->legal; q.nlegal = h->nlegal;
  q.legal_in = legal; q.count_in = count; q.to_play = to_play; q.noises = noises; q.rewards = rewards;
  q.logits = policy; q.noise_weight = noise_weight; q.B = h->B; q.A = h->A;
  p.prep_on = 1;
  const dim3 grid((B + kHdEnvs - 1) / kHdEnvs, 2);
  if (Vv <= kHdCols * kHdThreads)  // (A <= 256 here)
    hipLaunchKernelGGL(conv_heads_kernel<kHdCols>, grid, dim3(kHdThreads), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(conv_heads_kernel<kHdColsWide>, grid, dim3(kHdThreads), 0, (hipStream_t)stream, p);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// What the one-launch conv searches do for a handle, a network shape and a search length: the one decision
// behind lzm_search_conv / lzm_search_conv_ez and lzm_search_conv_plan. rc is what the launch returns for this
// request (LZM_OK: it runs; the message is in g_err otherwise); the LDS offsets are left in p.
struct ConvPlan {
  int rc, G, T, npin, pbt_rows, out_rounds, r_one_round;
  size_t lds;
  int roots;  // roots per launch (the whole batch, or the slice rule's answer: G, T, npin are the largest slice's)
};

// The slice rule of the one-launch conv searches (lzm_search_conv.h "Root slices"): roots per launch for a
// batch of B roots. resident_workgroups: the co-resident bound R of the EfficientZero grid (occupancy x CUs);
// max_roots: the caller's cap, 0 = none. MuZero: min(kScMaxRoots, cap) (at most B). EfficientZero: the whole
// batch when it passes the single launch's check (B <= 256, max(B, 2 T) <= R, B <= cap), else 64 m roots with
// m the largest integer >= 1 such that 64 m <= min(256, cap) and max(64 m, 2 m H / 16) <= R;
// LZM_ERR_RESIDENCY when no m fits, LZM_ERR_ARG for a cap below 64 on a batch that needs slicing. Host
// arithmetic only.
extern "C" int lzm_conv_slice_roots(int ez, int B, int H, int resident_workgroups, int max_roots) {
  if (B <= 0 || max_roots < 0 || (ez && (H <= 0 || H % kLsUnits || resident_workgroups < 0))) {
    set_err("lzm_conv_slice_roots: B > 0, max_roots >= 0 (0: no cap), EfficientZero: H a multiple of 16, "
            "resident_workgroups >= 0");
    return LZM_ERR_ARG;
  }
  if (!ez) return std::min(B, max_roots ? std::min(kScMaxRoots, max_roots) : kScMaxRoots);
  const int R = resident_workgroups, nb = H / kLsUnits;
  const long long T = (long long)((B + kLsRows - 1) / kLsRows) * nb;
  if (B <= 256 && std::max<long long>(B, 2 * T) <= R && (!max_roots || B <= max_roots)) return B;
  if (max_roots && max_roots < kLsRows) {
    snprintf(g_err, sizeof(g_err), "lzm_conv_slice_roots: max_roots %d < %d (EfficientZero slices are whole row "
             "blocks of %d roots)", max_roots, kLsRows, kLsRows);
    return LZM_ERR_ARG;
  }
  int m = std::min(256, max_roots ? max_roots : 256) / kLsRows;
  while (m >= 1 && std::max(kLsRows * m, 2 * m * nb) > R) --m;
  if (m < 1) {
    snprintf(g_err, sizeof(g_err), "lzm_conv_slice_roots: a slice of %d roots needs %d workgroups (%d LSTM tiles x "
             "2) > %d resident", kLsRows, std::max(kLsRows, 2 * nb), nb, R);
    return LZM_ERR_RESIDENCY;
  }
  return kLsRows * m;
}
// lower bits shared by both kinds: tree, walk and head buffers after the activation buffers (float offsets).
// gz (the Gumbel instantiation): the root's raw_value slice where the value cache is, no pUCT table, and the
// Gumbel table with the considered-visits row (64 + S words) where the seeds and the 16807^i table are (S + 32).
static size_t conv_plan_lds(const lzm_handle *h, int S, int Kr, int Khd, int Vr, int Vv, size_t o, ConvSearchArgs &p,
                            bool gz = false) {
  p.off_stat = (int)o; o += (size_t)h->cap * 4;
  p.off_meta = (int)o; o += (size_t)h->cap * 4;
  p.off_val = (int)o; o += round4((size_t)h->cap);
  p.off_lut = (int)o; o += gz ? 0 : round4((size_t)2 * h->lut_n);
  p.off_legal = (int)o; o += round4((size_t)h->A + 1);
  p.off_path = (int)o; o += round4((size_t)h->depth_cap);
  p.off_pact = (int)o; o += round4((size_t)h->depth_cap);
  p.off_pbt = (int)o; o += round4((size_t)p.pbt_rows * (p.pbt_rows + 1) / 2);
  p.off_r = (int)o; o += round4((size_t)Kr);
  p.off_hd = (int)o; o += round4((size_t)Khd);
  p.off_hid = (int)o; o += 96;
  p.off_part = (int)o; o += 3 * kHdParts * 32;
  p.off_lg = (int)o; o += round4((size_t)Vr + Vv + h->A);
  p.off_seed = (int)o; o += round4((size_t)S + (gz ? kMaxActions : 32));
  p.off_lmax = (int)o; o += round4((size_t)S + 1);
  return o;
}
static bool conv_shape_ok(int n_dres, int n_pres, int r_ch, int h_ch, int Khd, int off_policy, int Vr, int Vv,
                          int categorical) {
  return lzm_conv_trunk_floats_p(n_dres, n_pres, LZM_CONV_SPLIT) >= 0 && r_ch > 0 && r_ch <= 32 &&
         h_ch > 0 && h_ch <= 32 && Khd == h_ch * 64 && off_policy > 0 && off_policy < Khd && off_policy <= kHdKMax &&
         Khd - off_policy <= kHdKMax && !(off_policy % 128) && !(Khd % 128) && Vr > 0 && Vv > 0 && Vr <= 1024 &&
         Vv <= 1024 && (categorical || (Vr == 1 && Vv == 1));
}
// max_roots < 0: the whole batch in one launch (lzm_search_conv); >= 0: root slices by lzm_conv_slice_roots.
// gz: lzm_search_conv_gumbel's plan — a Gumbel MuZero handle outside collect-step mode (LZM_ERR_STATE otherwise),
// the same network shapes, the Gumbel instantiation's LDS plan; always sliced (its roots are independent).
static ConvPlan conv_plan_mz(const lzm_handle *h, int S, int n_dres, int n_pres, int r_ch, int h_ch, int Kr, int Khd,
                             int off_policy, int Vr, int Vv, int categorical, ConvSearchArgs &p, int max_roots = -1,
                             bool gz = false) {
  ConvPlan pl{LZM_ERR_ARG, 0, 0, 0, 0, 0, 0, 0, 0};
  const char *name = gz ? "lzm_search_conv_gumbel" : "lzm_search_conv";
  if (gz) {
    if ((pl.rc = check_kind(name, h, true)) != LZM_OK) return pl;
    pl.rc = LZM_ERR_STATE;
    if (h->step_count || h->step_fresh || h->step_dist || h->step_vals) {
      refuse(LZM_ERR_STATE, name, "collect-step mode (lzm_search_set_step): there is no Gumbel collect step");
      return pl;
    }
    pl.rc = LZM_ERR_ARG;
  }
  if (h->flags & LZM_TREE_EZ) {
    set_err("lzm_search_conv: MuZero trees only");
    return pl;
  }
  if (!conv_shape_ok(n_dres, n_pres, r_ch, h_ch, Khd, off_policy, Vr, Vv, categorical) || Kr != r_ch * 64 ||
      (Kr % 128)) {
    snprintf(g_err, sizeof(g_err), "%s: unsupported network shape (64x8x8 latent, <= 8 residual blocks per network, "
             "<= 32 reward / head planes, K per head a multiple of 128 and <= 1024, supports <= 1024)", name);
    return pl;
  }
  if (S > h->sims_cap) {
    snprintf(g_err, sizeof(g_err), "%s: %d simulations > reserved %d (lzm_reserve)", name, S, h->sims_cap);
    pl.rc = LZM_ERR_CAPACITY;
    return pl;
  }
  // one workgroup per root; roots beyond the CUs queue behind the first ones (their look-back waits only on
  // lower roots: lzm_search_conv.h sc_lookback)
  const int roots = max_roots < 0 ? h->B : lzm_conv_slice_roots(0, h->B, 0, 0, max_roots);
  if (roots < 0) {
    pl.rc = roots;
    return pl;
  }
  if (roots > kScMaxRoots) {
    snprintf(g_err, sizeof(g_err), "%s: %d roots > %d", name, roots, kScMaxRoots);
    return pl;
  }
  // dynamic LDS plan (float offsets, 16-B aligned): the two split-fp16 activation buffers first
  p.pbt_rows = 0;  // (no pb_c table: the MuZero conv walk divides, same bits)
  size_t o = conv_plan_lds(h, S, Kr, Khd, Vr, Vv, (size_t)2 * kBxBuf / 2, p, gz);
  if (o * sizeof(float) > kMaxLds) {
    snprintf(g_err, sizeof(g_err), "%s: %zu B of LDS needed (tree too large: lower num_simulations)", name,
             o * sizeof(float));
    return pl;
  }
  // the head hidden layers' first half-head resident in LDS when it fits and every root of the launch (the
  // slice) has a CU of its own (more roots than CUs: the smaller footprint lets two workgroups share one)
  constexpr size_t kPinFloats = (size_t)kHdParts * 16 * 32 * 4;
  const char *pin_env = getenv("LZM_CONV_PIN");
  const int pin_max = pin_env ? atoi(pin_env) : 1;
  p.off_wpin = (int)o;
  p.npin = 0;
  while (p.npin < pin_max && p.npin < 6 && roots <= device_cus() && (o + kPinFloats) * sizeof(float) <= kMaxLds) {
    o += kPinFloats;
    ++p.npin;
  }
  pl.rc = LZM_OK;
  pl.G = pl.roots = roots;
  pl.npin = p.npin;
  pl.out_rounds = sc_out_rounds(Vr + Vv + h->A);
  pl.r_one_round = 0;
  pl.lds = o * sizeof(float);
  return pl;
}

// the conv search kernel for a tree kind, an RNG and phase stamps
typedef void (*ConvKernel)(ConvSearchArgs);
// (the Gumbel walk draws nothing: one instantiation per stamps setting, on the draw-free side of the RNG flag)
static ConvKernel conv_gumbel_kernel_fn(bool stamps) {
  return stamps ? search_conv_kernel<kBxAhead, true, true, true> : search_conv_kernel<kBxAhead, true, false, true>;
}
static ConvKernel conv_kernel_fn(bool ez, bool fast, bool stamps) {
  static const ConvKernel kernels[2][2][2] = {  // [EZ][stamps, none][Philox, glibc]
      {{search_conv_kernel<kBxAhead, true, true>, search_conv_kernel<kBxAhead, false, true>},
       {search_conv_kernel<kBxAhead, true>, search_conv_kernel<kBxAhead, false>}},
      {{search_conv_ez_kernel<kBxAheadEz, true, true>, search_conv_ez_kernel<kBxAheadEz, false, true>},
       {search_conv_ez_kernel<kBxAheadEz, true>, search_conv_ez_kernel<kBxAheadEz, false>}}};
  return kernels[ez][stamps ? 0 : 1][fast ? 0 : 1];
}

// conv_plan_mz's EfficientZero twin. The shape, capacity and grid checks touch no HIP state; a request that
// passes them is then measured against the occupancy of the kernel it would launch (residency = true).
// max_roots < 0: the whole batch in one launch (lzm_search_conv_ez); >= 0: root slices by lzm_conv_slice_roots,
// asked first with the CU count for R (host only: a refusal comes before any HIP call, as the single launch's)
// and again with the occupancy bound once the kernel's LDS need is known.
static ConvPlan conv_plan_ez(const lzm_handle *h, int S, int H, int horizon, int n_dres, int n_pres, int r_ch, int h_ch,
                             int Khd, int off_policy, int Vr, int Vv, int categorical, ConvSearchArgs &p,
                             int max_roots = -1) {
  ConvPlan pl{LZM_ERR_ARG, 0, 0, 0, 0, 0, 0, 0, 0};
  if (!(h->flags & LZM_TREE_EZ)) {
    set_err("lzm_search_conv_ez: EfficientZero trees only");
    return pl;
  }
  const int Kx = r_ch * 64 + H;
  if (!conv_shape_ok(n_dres, n_pres, r_ch, h_ch, Khd, off_policy, Vr, Vv, categorical) || H <= 0 || H % kLsUnits ||
      H % 128 || H > kHdKMax || H / kLsUnits > 64 || Kx % (2 * kLsKc) || horizon <= 0 || S > 4094) {
    set_err("lzm_search_conv_ez: unsupported network shape (64x8x8 latent, <= 8 residual blocks per network, <= 32 "
            "reward / head planes, K per head a multiple of 128 and <= 1024, supports <= 1024, LSTM width a multiple "
            "of 128, (r_ch * 64 + H) % 128 == 0, horizon > 0) or more than 4094 simulations");
    return pl;
  }
  if (S > h->sims_cap) {
    snprintf(g_err, sizeof(g_err), "lzm_search_conv_ez: %d simulations > reserved %d (lzm_reserve)", S, h->sims_cap);
    pl.rc = LZM_ERR_CAPACITY;
    return pl;
  }
  // LZM_RESIDENCY_CUS=<n> caps the CU count this check assumes (tests: force the refusal)
  int cus = device_cus();
  if (const char *ov = getenv("LZM_RESIDENCY_CUS"))
    if (atoi(ov) > 0) cus = std::min(cus, atoi(ov));
  int B = h->B;  // roots per launch
  if (max_roots >= 0) {
    B = lzm_conv_slice_roots(1, h->B, H, cus, max_roots);
    if (B < 0) {
      pl.rc = B;
      return pl;
    }
  }
  int nmb = (B + kLsRows - 1) / kLsRows, T = nmb * (H / kLsUnits), G = std::max(B, 2 * T);
  pl.G = G;
  pl.T = T;
  pl.roots = B;
  p.nmb = (h->B + kLsRows - 1) / kLsRows; p.T = p.nmb * (H / kLsUnits);  // (the whole batch's: hand-off words)
  p.nmb_s = nmb; p.T_s = T;
  if (B > 256 || G > cus) {
    snprintf(g_err, sizeof(g_err),
             "lzm_search_conv_ez: %d workgroups (%d roots, %d LSTM tiles x 2) > min(%d CUs) or B > 256 (the grid is "
             "co-resident)", G, B, T, cus);
    pl.rc = LZM_ERR_RESIDENCY;
    return pl;
  }
  // dynamic LDS plan (float offsets, 16-B aligned): the activation buffers / LSTM stage buffers first
  p.pbt_rows = ((size_t)h->lut_n * (h->lut_n + 1) / 2 <= 4096) ? h->lut_n : 0;
  const size_t o = conv_plan_lds(h, S, H, Khd, Vr, Vv, std::max((size_t)2 * kBxBuf / 2, (size_t)kLsLdsBytes / 4), p);
  pl.lds = o * sizeof(float);
  pl.pbt_rows = p.pbt_rows;
  pl.out_rounds = sc_one_round(Vv + h->A) ? 0 : sc_out_rounds(Vv + h->A);
  pl.r_one_round = sc_one_round(Vr) ? 1 : 0;
  if (pl.lds > kMaxLds) {
    snprintf(g_err, sizeof(g_err), "lzm_search_conv_ez: %zu B of LDS needed (tree too large: lower num_simulations)",
             pl.lds);
    return pl;
  }
  // The roots wait on LSTM tiles and the tiles on roots inside the launch, so every workgroup must be
  // resident at once. The check is static: resident workgroups per CU at this LDS / register use (the
  // occupancy API) x the CUs must cover the grid, else LZM_ERR_RESIDENCY and nothing ran (the caller takes
  // the generic per-simulation path). It cannot see other work on the GPU (a learner on another stream, a
  // second rank on the same GPU): every hand-off wait in the kernel is bounded and a timeout is counted in
  // the tree's error word (lzm_check_errors raises), never a hang. The launch is a plain one, eager and
  // captured alike: the cooperative launch it replaced applies the same static occupancy check (it is
  // not a residency guarantee against other streams), cannot be captured into a HIP graph, and its
  // runtime state was the one difference from the MuZero conv search in the EZ trace that faulted in
  // exit() after rocprofv3 finalised (profiles/r05/README.md).
  const void *fn = (const void *)conv_kernel_fn(true, (h->flags & LZM_RNG_FAST) != 0, phase_timing());
  int per_cu = 0;
  if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)pl.lds) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, kScThreads, pl.lds) != hipSuccess) {
    set_err("lzm_search_conv_ez: the occupancy query failed");
    pl.rc = LZM_ERR_HIP;
    return pl;
  }
  if (max_roots >= 0) {  // the slice rule again, with the occupancy bound (the CU cap above still holds)
    B = lzm_conv_slice_roots(1, h->B, H, (int)std::min<long long>((long long)per_cu * cus, cus), max_roots);
    if (B < 0) {
      pl.rc = B;
      return pl;
    }
    nmb = (B + kLsRows - 1) / kLsRows; T = nmb * (H / kLsUnits); G = std::max(B, 2 * T);
    pl.G = G; pl.T = T; pl.roots = B;
    p.nmb_s = nmb; p.T_s = T;
  }
  if ((long long)per_cu * cus < G) {
    snprintf(g_err, sizeof(g_err), "lzm_search_conv_ez: %d workgroups > %d resident (%d per CU x %d CUs)", G,
             per_cu * cus, per_cu, cus);
    pl.rc = LZM_ERR_RESIDENCY;
    return pl;
  }
  pl.rc = LZM_OK;
  return pl;
}

// The plan queries' body: what the launch would do for this request as the process stands, by the launches'
// own decision (conv_plan_mz / conv_plan_ez); launches nothing. max_roots < 0: the single launch, out[0 .. 7];
// >= 0: the sliced launch with that cap, out[8 .. 10] as well.
static int conv_plan_query(const lzm_handle *h, int S, int ez, int H, int horizon, int n_dres, int n_pres, int r_ch,
                           int h_ch, int Kr, int Khd, int off_policy, int Vr, int Vv, int categorical, int max_roots,
                           int32_t *out, bool gz = false) {
  ConvSearchArgs p;
  memset(&p, 0, sizeof(p));
  const ConvPlan pl = ez ? conv_plan_ez(h, S, H, horizon, n_dres, n_pres, r_ch, h_ch, Khd, off_policy, Vr, Vv,
                                        categorical, p, max_roots)
                         : conv_plan_mz(h, S, n_dres, n_pres, r_ch, h_ch, Kr, Khd, off_policy, Vr, Vv, categorical, p,
                                        max_roots, gz);
  out[0] = pl.rc; out[1] = pl.G; out[2] = pl.T; out[3] = (int32_t)pl.lds; out[4] = pl.npin; out[5] = pl.pbt_rows;
  out[6] = pl.out_rounds; out[7] = pl.r_one_round;
  if (max_roots < 0) return LZM_OK;
  const int n = pl.rc == LZM_OK && pl.roots > 0 ? (h->B + pl.roots - 1) / pl.roots : 0;
  out[8] = n; out[9] = n ? pl.roots : 0; out[10] = n ? h->B - (n - 1) * pl.roots : 0;
  return LZM_OK;
}

// What lzm_search_conv (ez = 0: H and horizon ignored, Kr = r_ch * 64) or lzm_search_conv_ez (ez = 1: Kr ignored)
// would do. out[8]: {rc the launch would return (LZM_OK: it runs), workgroups, LSTM tiles, dynamic LDS
// bytes, pinned head half-heads, pb_c table rows, rounds of the value | policy (MuZero: whole) output loop
// (0 = EfficientZero's single-round form), 1 if the EfficientZero reward output takes the single-round form}.
extern "C" int lzm_search_conv_plan(const lzm_handle *h, int num_simulations, int ez, int H, int horizon, int n_dres,
                                    int n_pres, int r_ch, int h_ch, int Kr, int Khd, int off_policy, int Vr, int Vv,
                                    int categorical, int32_t *out) {
  if (!h || !out || num_simulations <= 0) {
    set_err("lzm_search_conv_plan: null argument or no simulations");
    return LZM_ERR_ARG;
  }
  return conv_plan_query(h, num_simulations, ez, H, horizon, n_dres, n_pres, r_ch, h_ch, Kr, Khd, off_policy, Vr, Vv,
                         categorical, -1, out);
}

// lzm_search_conv_plan for lzm_search_conv_sliced / lzm_search_conv_ez_sliced with the same max_roots: out[0 .. 7]
// as above for the largest slice (the first), then out[8 .. 10] = {slices, roots per slice, roots in the last
// slice} (zeros when refused). Launches nothing.
extern "C" int lzm_search_conv_sliced_plan(const lzm_handle *h, int num_simulations, int ez, int H, int horizon,
                                           int n_dres, int n_pres, int r_ch, int h_ch, int Kr, int Khd,
                                           int off_policy, int Vr, int Vv, int categorical, int max_roots,
                                           int32_t *out) {
  if (!h || !out || num_simulations <= 0 || max_roots < 0) {
    set_err("lzm_search_conv_sliced_plan: null argument, no simulations or max_roots < 0");
    return LZM_ERR_ARG;
  }
  return conv_plan_query(h, num_simulations, ez, H, horizon, n_dres, n_pres, r_ch, h_ch, Kr, Khd, off_policy, Vr, Vv,
                         categorical, max_roots, out);
}

// The EfficientZero inputs of the conv search beside MuZero's: the reward LSTM's state pools, width and
// horizon, its prepared gate weights and bias, the value-prefix BatchNorm map, the is_reset record
struct ConvEzIn {
  float *hpool, *cpool;
  int H, horizon;
  const float *lstm_frag, *lstm_bias, *vp_s, *vp_t;
  int32_t *rec_reset;
};
// The EfficientZero step of the launch: the hand-off workspace (LSTM input rows, outputs, split-K partials,
// flags), grown on demand (flags zeroed: epoch 0 never matches), and the LSTM and value-prefix pointers.
// (p.T: the whole batch's tile grid — the hand-off words and partials are filed by the global tile index)
static int conv_ez_attach(lzm_handle *h, ConvSearchArgs &p, const ConvEzIn &z, int S, int r_ch) {
  const int H = z.H, Kx = r_ch * 64 + H, B = h->B, T = p.T;
  const size_t f_xin = round4((size_t)B * Kx), f_h1 = round4((size_t)B * H), f_part = (size_t)T * kLpThreads * 16;
  const size_t flag_words = (size_t)S * B + 2 * (size_t)S * T;
  const size_t need = (f_xin + f_h1 + f_part) * sizeof(float) + flag_words * sizeof(unsigned long long);
  if (h->ez_ws_bytes < need) {
    dfree(h->ez_ws);
    h->ez_ws = nullptr;
    h->ez_ws_bytes = 0;
    LZM_HIP(hipMalloc(&h->ez_ws, need));
    LZM_HIP(hipMemset(h->ez_ws, 0, need));
    h->ez_ws_bytes = need;
  }
  float *wsf = reinterpret_cast<float *>(h->ez_ws);
  unsigned long long *wsl = reinterpret_cast<unsigned long long *>(wsf + f_xin + f_h1 + f_part);
  p.rec_reset = z.rec_reset;
  p.xin = wsf; p.h1g = wsf + f_xin; p.kpart = wsf + f_xin + f_h1;
  p.xflags = wsl; p.tflags = wsl + (size_t)S * B; p.pflags = wsl + (size_t)S * B + (size_t)S * T;
  p.Kx = Kx; p.H = H; p.horizon = z.horizon; p.hpool = z.hpool; p.cpool = z.cpool;
  p.lwfrag = reinterpret_cast<const uint16_t *>(z.lstm_frag); p.lwinv = z.lstm_frag + ls_frag_floats(Kx, H);
  p.lbias = z.lstm_bias; p.vp_s = z.vp_s; p.vp_t = z.vp_t;
  return LZM_OK;
}

// Whole-search launch for the conv networks (lzm_search_conv.h): one workgroup per root, every simulation
// inside the kernel; parity-mode roots wait on their predecessors' depth flags. ez != null: the EfficientZero
// instantiation, the same flow plus the reward LSTM as split-K tiles spread over the grid (max(roots, 2 T)
// workgroups, co-resident: the tiles wait on the roots' LSTM input rows and the roots on their rows' tiles
// inside the launch; Kr is then the LSTM's width).
// max_roots < 0: the whole batch in one launch; >= 0: the sliced entry points (every root slice, EfficientZero's
// each a co-resident grid of its own, enqueued on the stream, lowest roots first).
// gumbel_m >= 0: lzm_search_conv_gumbel (max_num_considered_actions; -1: the pUCT searches) — the Gumbel
// instantiation on a Gumbel MuZero handle: no seeds, the considered-visits row set as lzm_search_mlp_gumbel does,
// the handle's raw_value array and tables attached, no collect step; its slices are independent launches.
static int search_conv_launch(lzm_handle *h, int num_simulations, int pb_c_base, float pb_c_init, float discount,
                              float *minmax, const uint32_t *seeds, const int32_t *vtp_in, float *latent_pool,
                              const float *trunk_w, const float *actmap, int n_dres, int n_pres, int r_ch, int h_ch,
                              const float *w1t, const float *b1, const float *w2q, const float *b2, int Kr, int Khd,
                              int off_policy, int Vr, int Vv, int categorical, int32_t *rec_x, int32_t *rec_a,
                              int32_t *rec_len, float *rec_decoded, float *rec_logits, void *stream, int max_roots,
                              const ConvEzIn *ez, int gumbel_m = -1) {
  const bool gz = gumbel_m >= 0;
  const char *name = gz ? "lzm_search_conv_gumbel" : ez ? "lzm_search_conv_ez" : "lzm_search_conv";
  const int S = num_simulations;
  if (!h || !minmax || (!gz && !seeds && !h->step_count) || !vtp_in || !latent_pool || !trunk_w || !actmap || !w1t ||
      !b1 || !w2q || !b2 || S <= 0 ||
      (ez && (!ez->hpool || !ez->cpool || !ez->lstm_frag || !ez->lstm_bias || !ez->vp_s || !ez->vp_t))) {
    snprintf(g_err, sizeof(g_err), "%s: null argument or no simulations", name);
    return LZM_ERR_ARG;
  }
  if (!gz && (h->flags & LZM_TREE_GUMBEL)) {
    set_err("one-launch searches do not take a Gumbel MuZero handle");
    return LZM_ERR_STATE;
  }
  uintptr_t bits = (uintptr_t)trunk_w | (uintptr_t)actmap | (uintptr_t)w1t | (uintptr_t)w2q | (uintptr_t)latent_pool;
  if (ez)
    bits |= (uintptr_t)ez->hpool | (uintptr_t)ez->cpool | (uintptr_t)ez->lstm_frag | (uintptr_t)ez->vp_s |
            (uintptr_t)ez->vp_t;
  if (bits & 15) {
    snprintf(g_err, sizeof(g_err), "%s: weights and pool%s must be 16-byte aligned", name, ez ? "s" : "");
    return LZM_ERR_ARG;
  }
  ConvSearchArgs p;
  memset(&p, 0, sizeof(p));
  const ConvPlan plan = ez ? conv_plan_ez(h, S, ez->H, ez->horizon, n_dres, n_pres, r_ch, h_ch, Khd, off_policy, Vr,
                                          Vv, categorical, p, max_roots)
                           : conv_plan_mz(h, S, n_dres, n_pres, r_ch, h_ch, Kr, Khd, off_policy, Vr, Vv, categorical,
                                          p, max_roots, gz);
  if (plan.rc != LZM_OK) return plan.rc;
  int rc = search_preamble(h, pb_c_base, pb_c_init, S, h->B);
  if (rc != LZM_OK) return rc;
  if (gz && (rc = gumbel_set_considered(h, S, gumbel_m, name)) != LZM_OK) return rc;
  if (ez && (rc = conv_ez_attach(h, p, *ez, S, r_ch)) != LZM_OK) return rc;
  fill_common(p, h, S, discount, seeds, vtp_in, minmax, latent_pool, rec_x, rec_a, rec_len, rec_decoded, rec_logits);
  p.w = trunk_w; p.actmap = actmap; p.n_dres = n_dres; p.n_pres = n_pres; p.r_ch = r_ch; p.h_ch = h_ch;
  p.w1t = w1t; p.b1 = b1; p.w2q = w2q; p.b2 = b2; p.Kr = ez ? ez->H : Kr; p.Khd = Khd; p.off_policy = off_policy;
  p.Vr = Vr; p.Vv = Vv; p.categorical = categorical ? 1 : 0;
  p.err = h->err; p.sdiag = h->search_diag;
  if (gz) {  // (the plan refused collect-step mode: the step fields stay zero)
    p.raw = h->raw; p.gumbel = h->gumbel; p.considered = h->considered;
  } else {
    p.step_count = h->step_count; p.step_base = h->step_base; p.step_inc = h->step_inc; p.step_fresh = h->step_fresh;
    p.step_delta = h->step_delta; p.out_dist = h->step_dist; p.out_values = h->step_vals;
  }
  const bool stamps = phase_timing();
  if (stamps && (rc = ensure_phase(h)) != LZM_OK) return rc;
  p.stamps = stamps ? h->phase : nullptr;
  const ConvKernel fn = gz ? conv_gumbel_kernel_fn(stamps) : conv_kernel_fn(ez != nullptr, p.fast != 0, stamps);
  LZM_HIP(hipFuncSetAttribute((const void *)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan.lds));
  for (int root0 = 0; root0 < h->B; root0 += plan.roots) {  // (EfficientZero slices start at multiples of 64 roots)
    p.root0 = root0;
    p.nroots = std::min(plan.roots, h->B - root0);
    p.last_slice = root0 + p.nroots >= h->B;
    int grid = p.nroots;
    if (ez) {  // the slice's own row blocks and LSTM tiles
      p.nmb_s = (p.nroots + kLsRows - 1) / kLsRows;
      p.T_s = p.nmb_s * (ez->H / kLsUnits);
      grid = std::max(p.nroots, 2 * p.T_s);
    }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(kScThreads), plan.lds, (hipStream_t)stream, p);
    LZM_CHECK_LAUNCH();
  }
  return LZM_OK;
}

extern "C" int lzm_search_conv(lzm_handle *h, int num_simulations, int pb_c_base, float pb_c_init, float discount,
                               float *minmax, const uint32_t *seeds, const int32_t *vtp_in, float *latent_pool,
                               const float *trunk_w, const float *actmap, int n_dres, int n_pres, int r_ch, int h_ch,
                               const float *w1t, const float *b1, const float *w2q, const float *b2, int Kr, int Khd,
                               int off_policy, int Vr, int Vv, int categorical, int32_t *rec_x, int32_t *rec_a,
                               int32_t *rec_len, float *rec_decoded, float *rec_logits, void *stream) {
  return search_conv_launch(h, num_simulations, pb_c_base, pb_c_init, discount, minmax, seeds, vtp_in, latent_pool,
                            trunk_w, actmap, n_dres, n_pres, r_ch, h_ch, w1t, b1, w2q, b2, Kr, Khd, off_policy, Vr, Vv,
                            categorical, rec_x, rec_a, rec_len, rec_decoded, rec_logits, stream, -1, nullptr);
}

// lzm_search_conv over root slices (lzm_conv_slice_roots; max_roots: the caller's cap on a slice, 0 = none): any
// number of roots, the slices enqueued one after another on `stream` (plain launches, capturable).
extern "C" int lzm_search_conv_sliced(lzm_handle *h, int num_simulations, int pb_c_base, float pb_c_init,
                                      float discount, float *minmax, const uint32_t *seeds, const int32_t *vtp_in,
                                      float *latent_pool, const float *trunk_w, const float *actmap, int n_dres,
                                      int n_pres, int r_ch, int h_ch, const float *w1t, const float *b1,
                                      const float *w2q, const float *b2, int Kr, int Khd, int off_policy, int Vr,
                                      int Vv, int categorical, int32_t *rec_x, int32_t *rec_a, int32_t *rec_len,
                                      float *rec_decoded, float *rec_logits, int max_roots, void *stream) {
  if (max_roots < 0) {
    set_err("lzm_search_conv_sliced: max_roots >= 0 (0: no cap)");
    return LZM_ERR_ARG;
  }
  return search_conv_launch(h, num_simulations, pb_c_base, pb_c_init, discount, minmax, seeds, vtp_in, latent_pool,
                            trunk_w, actmap, n_dres, n_pres, r_ch, h_ch, w1t, b1, w2q, b2, Kr, Khd, off_policy, Vr, Vv,
                            categorical, rec_x, rec_a, rec_len, rec_decoded, rec_logits, stream, max_roots, nullptr);
}

extern "C" int lzm_search_conv_ez(lzm_handle *h, int num_simulations, int pb_c_base, float pb_c_init, float discount,
                                  float *minmax, const uint32_t *seeds, const int32_t *vtp_in, float *latent_pool,
                                  float *hpool, float *cpool, int H, int horizon, const float *trunk_w,
                                  const float *actmap, int n_dres, int n_pres, int r_ch, int h_ch,
                                  const float *lstm_frag, const float *lstm_bias, const float *vp_s, const float *vp_t,
                                  const float *w1t, const float *b1, const float *w2q, const float *b2, int Khd,
                                  int off_policy, int Vr, int Vv, int categorical, int32_t *rec_x, int32_t *rec_a,
                                  int32_t *rec_len, float *rec_decoded, float *rec_logits, int32_t *rec_reset,
                                  void *stream) {
  const ConvEzIn ez{hpool, cpool, H, horizon, lstm_frag, lstm_bias, vp_s, vp_t, rec_reset};
  return search_conv_launch(h, num_simulations, pb_c_base, pb_c_init, discount, minmax, seeds, vtp_in, latent_pool,
                            trunk_w, actmap, n_dres, n_pres, r_ch, h_ch, w1t, b1, w2q, b2, 0, Khd, off_policy, Vr, Vv,
                            categorical, rec_x, rec_a, rec_len, rec_decoded, rec_logits, stream, -1, &ez);
}

// GumbelMuZeroMCTSCtree.search's whole loop over a conv MuZeroModel in one launch per root slice (lzm_search_conv.h,
// the GZ instantiation), on lzm_search_conv_sliced's plan-and-launch path. No seeds and no pb_c arguments (the
// handle's default table is set and never read). Rebuilds the considered-visits row when (S, m) changed: a
// synchronous copy, outside stream capture (lzm_gumbel_set_considered before a capture).
extern "C" int lzm_search_conv_gumbel(lzm_handle *h, int num_simulations, int max_num_considered_actions,
                                      float discount, float *minmax, const int32_t *vtp_in, float *latent_pool,
                                      const float *trunk_w, const float *actmap, int n_dres, int n_pres, int r_ch,
                                      int h_ch, const float *w1t, const float *b1, const float *w2q, const float *b2,
                                      int Kr, int Khd, int off_policy, int Vr, int Vv, int categorical,
                                      int32_t *rec_x, int32_t *rec_a, int32_t *rec_len, float *rec_decoded,
                                      float *rec_logits, int max_roots, void *stream) {
  if (max_roots < 0 || max_num_considered_actions < 0) {
    set_err("lzm_search_conv_gumbel: max_roots >= 0 (0: no cap) and max_num_considered_actions >= 0");
    return LZM_ERR_ARG;
  }
  return search_conv_launch(h, num_simulations, 19652, 1.25f, discount, minmax, nullptr, vtp_in, latent_pool, trunk_w,
                            actmap, n_dres, n_pres, r_ch, h_ch, w1t, b1, w2q, b2, Kr, Khd, off_policy, Vr, Vv,
                            categorical, rec_x, rec_a, rec_len, rec_decoded, rec_logits, stream, max_roots, nullptr,
                            max_num_considered_actions);
}

// What lzm_search_conv_gumbel would do with the same max_roots, by the launch's own decision (conv_plan_mz):
// lzm_search_conv_sliced_plan's eleven words. Launches nothing.
extern "C" int lzm_search_conv_gumbel_plan(const lzm_handle *h, int num_simulations, int n_dres, int n_pres, int r_ch,
                                           int h_ch, int Kr, int Khd, int off_policy, int Vr, int Vv, int categorical,
                                           int max_roots, int32_t *out) {
  if (!h || !out || num_simulations <= 0 || max_roots < 0) {
    set_err("lzm_search_conv_gumbel_plan: null argument, no simulations or max_roots < 0");
    return LZM_ERR_ARG;
  }
  return conv_plan_query(h, num_simulations, 0, 0, 0, n_dres, n_pres, r_ch, h_ch, Kr, Khd, off_policy, Vr, Vv,
                         categorical, max_roots, out, true);
}

// lzm_search_conv_ez over root slices (lzm_conv_slice_roots with the launch's own residency bound; max_roots: the
// caller's cap on a slice, 0 = none): batches past 256 roots or past the co-resident grid, the slices enqueued
// one after another on `stream` (plain launches, capturable). LZM_ERR_RESIDENCY, with nothing launched, when
// not even a 64-root slice is co-resident.
extern "C" int lzm_search_conv_ez_sliced(lzm_handle *h, int num_simulations, int pb_c_base, float pb_c_init,
                                         float discount, float *minmax, const uint32_t *seeds, const int32_t *vtp_in,
                                         float *latent_pool, float *hpool, float *cpool, int H, int horizon,
                                         const float *trunk_w, const float *actmap, int n_dres, int n_pres, int r_ch,
                                         int h_ch, const float *lstm_frag, const float *lstm_bias, const float *vp_s,
                                         const float *vp_t, const float *w1t, const float *b1, const float *w2q,
                                         const float *b2, int Khd, int off_policy, int Vr, int Vv, int categorical,
                                         int32_t *rec_x, int32_t *rec_a, int32_t *rec_len, float *rec_decoded,
                                         float *rec_logits, int32_t *rec_reset, int max_roots, void *stream) {
  if (max_roots < 0) {
    set_err("lzm_search_conv_ez_sliced: max_roots >= 0 (0: no cap)");
    return LZM_ERR_ARG;
  }
  const ConvEzIn ez{hpool, cpool, H, horizon, lstm_frag, lstm_bias, vp_s, vp_t, rec_reset};
  return search_conv_launch(h, num_simulations, pb_c_base, pb_c_init, discount, minmax, seeds, vtp_in, latent_pool,
                            trunk_w, actmap, n_dres, n_pres, r_ch, h_ch, w1t, b1, w2q, b2, 0, Khd, off_policy, Vr, Vv,
                            categorical, rec_x, rec_a, rec_len, rec_decoded, rec_logits, stream, max_roots, &ez);
}

// Test support: n workgroups that each occupy a CU (the whole LDS) for `usec` microseconds of the 100 MHz real-time
// clock, then exit — another stream's kernel holding CUs while a co-resident grid launches (tests only).
__global__ void hold_cu_kernel(unsigned long long ticks) {
  extern __shared__ uint4 hold_lds[];
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  if (threadIdx.x == 0) hold_lds[0] = uint4{0u, 0u, 0u, 0u};
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

extern "C" int lzm_debug_hold_cus(int n, int usec, void *stream) {
  if (n <= 0 || n > 4096 || usec <= 0 || usec > 2000000) {
    set_err("lzm_debug_hold_cus: 1..4096 workgroups for up to 2 s");
    return LZM_ERR_ARG;
  }
  static hipError_t attr = hipFuncSetAttribute((const void *)hold_cu_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)kMaxLds);
  LZM_HIP(attr);
  hipLaunchKernelGGL(hold_cu_kernel, dim3(n), dim3(64), kMaxLds, (hipStream_t)stream, (unsigned long long)usec * 100ull);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

extern "C" int lzm_ez_lstm_input(int B, int Kr, int H, const float *r, const float *hpool, const int32_t *x, float *xin,
                                 void *stream) {
  if (B <= 0 || Kr <= 0 || H <= 0 || (Kr & 3) || (H & 3) || !r || !hpool || !x || !xin ||
      (((uintptr_t)r | (uintptr_t)hpool | (uintptr_t)xin) & 15)) {
    set_err("lzm_ez_lstm_input: bad arguments (Kr, H multiples of 4, 16-B aligned buffers)");
    return LZM_ERR_ARG;
  }
  const long long n = (long long)B * ((Kr + H) >> 2);
  const int grid = (int)std::min<long long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(ez_lstm_input_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, B, Kr, H, r, hpool, x, xin);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

extern "C" int lzm_ez_lstm_cell(int B, int H, const float *gates, const float *cpool, const int32_t *x,
                                const int32_t *search_len, int horizon, float *h1, float *c1, float *hslot,
                                float *cslot, void *stream) {
  if (B <= 0 || H <= 0 || (H & 3) || !gates || !cpool || !x || !search_len || !h1 || !c1 || !hslot || !cslot ||
      (((uintptr_t)gates | (uintptr_t)cpool | (uintptr_t)h1 | (uintptr_t)c1 | (uintptr_t)hslot | (uintptr_t)cslot) & 15)) {
    set_err("lzm_ez_lstm_cell: bad arguments (H multiple of 4, 16-B aligned buffers)");
    return LZM_ERR_ARG;
  }
  const long long n = (long long)B * (H >> 2);
  const int grid = (int)std::min<long long>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(ez_lstm_cell_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, B, H, gates, cpool, x,
                     search_len, horizon, h1, c1, hslot, cslot);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

extern "C" int64_t lzm_ez_lstm_frag_floats(int K, int H) {
  if (K <= 0 || H <= 0 || K % kLsKc || H % kLsUnits) return -1;
  return ls_frag_floats(K, H) + 4 * (int64_t)H;  // the fragments, then the 4H column scales
}

extern "C" int lzm_ez_lstm_prepare(int K, int H, const float *W, float *out) {
  if (lzm_ez_lstm_frag_floats(K, H) < 0 || !W || !out) {
    set_err("lzm_ez_lstm_prepare: need K % 64 == 0, H % 16 == 0 and buffers");
    return LZM_ERR_ARG;
  }
  ls_pack(W, K, H, out);
  return LZM_OK;
}

static unsigned long long *g_ls_stamps = nullptr;  // diagnostics: lzm_debug_lstm_stamps
extern "C" int lzm_debug_lstm_stamps(void *buf) {
  g_ls_stamps = reinterpret_cast<unsigned long long *>(buf);
  return LZM_OK;
}

extern "C" int64_t lzm_ez_lstm_workspace_bytes(int B, int H) {
  if (B <= 0 || H <= 0 || H % kLsUnits) return -1;
  const int64_t tiles = (int64_t)((B + kLsRows - 1) / kLsRows) * (H / kLsUnits);
  return tiles * kLsPartFloats * 4 + tiles * 4;
}

extern "C" int lzm_ez_lstm_step(int B, int K, int H, const float *xin, const int32_t *xscale, const float *wfrag,
                                const float *bias, const float *cpool, const int32_t *x, const int32_t *search_len,
                                int horizon, float *h1, float *c1, float *hslot, float *cslot, void *workspace,
                                int32_t *err, int32_t *range_err, void *stream) {
  if (B <= 0 || lzm_ez_lstm_frag_floats(K, H) < 0 || !xin || !xscale || !wfrag || !bias || !cpool || !x || !search_len || !h1 ||
      !c1 || !hslot || !cslot || (((uintptr_t)xin | (uintptr_t)wfrag | (uintptr_t)workspace) & 15) ||
      (workspace && !err)) {
    set_err("lzm_ez_lstm_step: bad arguments (K % 64 == 0, H % 16 == 0, 16-B aligned xin / fragments / workspace, "
            "an error word with the workspace)");
    return LZM_ERR_ARG;
  }
  LstmArgs a;
  a.B = B; a.K = K; a.H = H; a.nmb = (B + kLsRows - 1) / kLsRows;
  a.xin = xin; a.xscale = xscale; a.range_err = range_err;
  a.wf = reinterpret_cast<const uint4 *>(wfrag); a.winv = wfrag + ls_frag_floats(K, H);
  a.bias = bias; a.cpool = cpool; a.x = x;
  a.search_len = search_len; a.horizon = horizon; a.h1 = h1; a.c1 = c1; a.hslot = hslot; a.cslot = cslot;
  const int tiles = a.nmb * (H / kLsUnits);
  // split K in two when a workspace is given and every workgroup is resident at once (the lower K
  // half waits for the upper; one 512-thread workgroup per CU by its LDS)
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    cus = 0;
  a.splitk = (workspace && K % (2 * kLsKc) == 0 && 2 * tiles <= cus) ? 2 : 1;
  a.part = reinterpret_cast<float *>(workspace);
  a.flags = workspace ? reinterpret_cast<uint32_t *>(a.part + (size_t)tiles * kLsPartFloats) : nullptr;
  a.err = err;
  a.stamps = g_ls_stamps;
  static bool attr = false;
  if (!attr) {
    LZM_HIP(hipFuncSetAttribute((const void *)ez_lstm_gemm_cell_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                kLsLdsBytes));
    attr = true;
  }
  hipLaunchKernelGGL(ez_lstm_gemm_cell_kernel, dim3(tiles * a.splitk), dim3(kLsThreads), kLsLdsBytes,
                     (hipStream_t)stream, a);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

// The shape initial_fast_kernel is compiled for (lzm_initial.h): the resident search kernel's widths
static bool ii_fast_shape(int O, int H, int F, int V, int A, int group) {
  return H == kIfH && F == kIfF && V == kIfV && group == kIfG && A >= 1 && A <= kIfMaxA && O >= 1 && O <= kIfMaxO;
}

static bool ii_fast_enabled() {
  const char *e = getenv("LZM_II_FAST");  // "0": always the generic kernel; read at each call
  return !(e && atoi(e) == 0);
}

extern "C" int lzm_mlp_initial_fast(int O, int H, int F, int V, int A, int group) {
  return (ii_fast_enabled() && ii_fast_shape(O, H, F, V, A, group)) ? 1 : 0;
}

// The fast kernel's weight block (offsets[16], 16-byte aligned), or null: the generic kernel
static const float4 *ii_fast_block(const IiArgs &p, const float *weights, const int64_t *offsets) {
  if (!ii_fast_enabled() || !ii_fast_shape(p.O, p.H, p.F, p.V, p.A, p.group) || offsets[16] < 0) return nullptr;
  const float *fw = weights + offsets[16];
  return (reinterpret_cast<uintptr_t>(fw) & 15) ? nullptr : reinterpret_cast<const float4 *>(fw);
}

extern "C" int lzm_mlp_initial_inference(int B, int O, int H, int F, int V, int A, int group, const float *obs,
                                         const float *weights, const int64_t *offsets, float *latent, float *value,
                                         float *policy, void *stream) {
  if (B <= 0 || O <= 0 || O > kIiMaxW || H <= 0 || H > kIiMaxW || F <= 0 || F > 256 || V <= 0 || V > kIiMaxW ||
      A <= 0 || A > kIiMaxW || group <= 0 || H % group || !obs || !weights || !offsets || !latent || !value ||
      !policy) {
    set_err("lzm_mlp_initial_inference: bad arguments (widths <= 1024, head hidden <= 256, H % group == 0)");
    return LZM_ERR_ARG;
  }
  IiArgs p;
  p.B = B; p.O = O; p.H = H; p.F = F; p.V = V; p.A = A; p.group = group;
  p.obs = obs;
  for (int l = 0; l < kIiLayers; ++l) {
    p.w[l] = l < 8 ? weights + offsets[2 * l] : nullptr;
    p.b[l] = l < 8 ? weights + offsets[2 * l + 1] : nullptr;
  }
  p.latent = latent; p.value = value; p.policy = policy;
  if (const float4 *fw = ii_fast_block(p, weights, offsets)) {
    hipLaunchKernelGGL(initial_fast_kernel<false>, dim3(B), dim3(kIiThreads), 0, (hipStream_t)stream, p, fw,
                       PrepareArgs{});
    LZM_CHECK_LAUNCH();
    return LZM_OK;
  }
  hipLaunchKernelGGL(initial_inference_kernel<false>, dim3((B + kIiEnvs - 1) / kIiEnvs), dim3(kIiThreads), 0,
                     (hipStream_t)stream, p, PrepareArgs{});
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

extern "C" int lzm_mlp_initial_inference_prepare(lzm_handle *h, int B, int O, int H, int F, int V, int A, int group,
                                                 const float *obs, const float *weights, const int64_t *offsets,
                                                 float *latent, float *value, float *policy, const int32_t *legal,
                                                 const int32_t *count, const float *noises, float noise_weight,
                                                 const float *rewards, const int32_t *to_play, void *stream) {
  if (!h || h->B != B || h->A != A || !legal || !count || !rewards || !to_play) {
    set_err("lzm_mlp_initial_inference_prepare: the handle must have B roots and A actions; legal, count, rewards, "
            "to_play required");
    return LZM_ERR_ARG;
  }
  if (B <= 0 || O <= 0 || O > kIiMaxW || H <= 0 || H > kIiMaxW || F <= 0 || F > 256 || V <= 0 || V > kIiMaxW ||
      A <= 0 || A > kIiMaxW || group <= 0 || H % group || !obs || !weights || !offsets || !latent || !value ||
      !policy) {
    set_err("lzm_mlp_initial_inference_prepare: bad arguments (widths <= 1024, head hidden <= 256, H % group == 0)");
    return LZM_ERR_ARG;
  }
  IiArgs p;
  p.B = B; p.O = O; p.H = H; p.F = F; p.V = V; p.A = A; p.group = group;
  p.obs = obs;
  for (int l = 0; l < kIiLayers; ++l) {
    p.w[l] = l < 8 ? weights + offsets[2 * l] : nullptr;
    p.b[l] = l < 8 ? weights + offsets[2 * l + 1] : nullptr;
  }
  p.latent = latent; p.value = value; p.policy = policy;
  PrepareArgs q;
  q.stat = h->stat; q.meta = h->meta; q.legal = h->legal; q.nlegal = h->nlegal;
  q.legal_in = legal; q.count_in = count; q.to_play = to_play; q.noises = noises; q.rewards = rewards;
  q.logits = policy; q.noise_weight = noise_weight; q.B = h->B; q.A = h->A;
  if (const float4 *fw = ii_fast_block(p, weights, offsets)) {
    hipLaunchKernelGGL(initial_fast_kernel<true>, dim3(B), dim3(kIiThreads), 0, (hipStream_t)stream, p, fw, q);
    LZM_CHECK_LAUNCH();
    return LZM_OK;
  }
  hipLaunchKernelGGL(initial_inference_kernel<true>, dim3((B + kIiEnvs - 1) / kIiEnvs), dim3(kIiThreads), 0,
                     (hipStream_t)stream, p, q);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

extern "C" int lzm_set_reuse(lzm_handle *h, const int32_t *true_action, const float *reuse_value) {
  if (!h || (!true_action) != (!reuse_value)) {
    set_err("lzm_set_reuse: both arrays or neither");
    return LZM_ERR_ARG;
  }
  h->reuse_action = true_action;
  h->reuse_value = reuse_value;
  return LZM_OK;
}

extern "C" int lzm_set_value_support(lzm_handle *h, int value_support_len) {
  if (!h || value_support_len < 0) {
    set_err("lzm_set_value_support: null handle or negative length");
    return LZM_ERR_ARG;
  }
  h->value_support = value_support_len;
  return LZM_OK;
}

extern "C" int lzm_set_norm_words(lzm_handle *h, const int32_t *words) {
  if (!h) return LZM_ERR_ARG;
  h->ext_norm = words;
  return LZM_OK;
}

// Traverse seeds of one collect step (SURVEY.md §8(d) rule, lightzero_amd.collect.DeviceSearchStep):
// seeds[k] = (base + count * S + k) mod 10^6, count read on the device (a captured graph replays it).
__global__ void seed_sequence_kernel(const int64_t *count, long long base, int S, int32_t *seeds) {
  const long long c = *count;
  for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < S; k += gridDim.x * blockDim.x)
    seeds[k] = (int32_t)((base + c * (long long)S + k) % 1000000ll);
}

extern "C" int lzm_seed_sequence(const int64_t *count, int64_t base, int S, int32_t *seeds, void *stream) {
  if (!count || !seeds || S <= 0 || base < 0) {
    set_err("lzm_seed_sequence: bad arguments");
    return LZM_ERR_ARG;
  }
  hipLaunchKernelGGL(seed_sequence_kernel, dim3((S + 255) / 256), dim3(256), 0, (hipStream_t)stream, count,
                     (long long)base, S, seeds);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}

extern "C" int lzm_get_root_outputs(lzm_handle *h, int32_t *dist, float *values, void *stream) {
  if (!h || !dist || !values) {
    set_err("lzm_get_root_outputs: null argument");
    return LZM_ERR_ARG;
  }
  hipLaunchKernelGGL(root_outputs_kernel, dim3((h->B + 255) / 256), dim3(256), 0, (hipStream_t)stream, view(h), dist,
                     values);
  LZM_CHECK_LAUNCH();
  return LZM_OK;
}
