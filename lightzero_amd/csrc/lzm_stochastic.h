// lzm_stochastic.h — the Stochastic MuZero tree (gfx950): decision / chance levels, one wave per root.
//
// Restates lzero/mcts/ctree/ctree_stochastic_muzero/lib/cnode.cpp (line numbers of that file): cbatch_traverse
// :711-786 with compute_mean_q :195-229 at every level, cselect_child :594-663 (pUCT with the order-dependent
// 1e-6 tie list at decision nodes, a draw from the children's priors at chance nodes :610-630) and cucb_score
// :665-709; CNode::expand :96-173 (the node's kind flips at every level whatever the caller says :116-122, so a
// node is a chance node iff its depth is odd; a chance node's reward is 0 :118; the child count is the logit
// row's length); cbackpropagate :496-557 is the MuZero rule over the whole path (backup_wave).
//
// Work split (the Gumbel family's, lzm_gumbel.h): one wave per root, four roots per 256-thread workgroup, the
// root index in a scalar register. Lane j is child j of the current node — action j (legal position j at the
// root) on a decision level, outcome j on a chance level — so A <= 64 and C <= 64. Roots exchange nothing: no
// look-back flags, no epochs, no spins. No LDS, no scratch: a level is one round of child reads, every score
// lives in its lane, and the chosen child's record comes from the lane that read it (readlane).
//
// Node storage is the MuZero tree's (NodeStat / NodeMeta, children of the node expanded by simulation L at
// 1 + W * L + j) with the block width W = max(A, C) in TreeView::A: the shared kernels (prepare, distributions,
// trajectories, gather) address such a handle unchanged. The kind comes from the depth's parity: no new field.
//
// Randomness: the reference seeds every chance draw from std::random_device, so there is no stream to stay in
// parity with; a stochastic handle always draws from per-root Philox4x32-10 streams under key (seed, 0x4c5a4d43):
//   tie draw at decision level l of root i:   counter (l, i, 0, 0), word x >> 1, modulo the tie count
//                                             (traverse_fast_kernel's draw);
//   chance draw at chance level l of root i:  counter (l, i, 1, 0), u = u01(x, y) in (0, 1) (lzm_collect.h), the
//                                             first outcome in outcome order whose running DOUBLE sum of the
//                                             float32 priors exceeds u * total (so a prior of exactly 0 is never
//                                             taken); if rounding leaves none, the last outcome with a non-zero
//                                             prior.
// Float sums run in the reference's order by wave-uniform readlane chains; max is order-free.
#pragma once
#include "lzm_collect.h"
#include "lzm_tree.h"

namespace lzm {

constexpr uint32_t kStochasticKey = 0x4c5a4d43u;

struct StochasticView {
  int A, C;            // action space / chance space (TreeView::A is the block width max(A, C))
  int32_t *is_chance;  // [B] kind of the last walk's leaf (results.leaf_node_is_chance, :782)
};

// players = (max(virtual_to_play) == -1) ? 1 : 2 (:732-737), by every wave for itself (no LDS)
__device__ inline int stochastic_players(const int32_t *vtp, int B) {
  int m = INT_MIN;
  for (int j = threadIdx.x & 63; j < B; j += 64) m = max(m, vtp[j]);
  return xor_max(m) == -1 ? 1 : 2;
}

// The chance draw: prior = the lane's outcome prior (0 past n). Wave-uniform result.
__device__ inline int stochastic_chance_pick(float prior, int n, double u) {
  const int lane = threadIdx.x & 63;
  double run = 0.0, pre = 0.0;  // pre: the running sum up to and including this lane's outcome
  for (int j = 0; j < n; ++j) {
    run += (double)readlane_f(prior, j);
    if (lane == j) pre = run;
  }
  const double thr = u * run;
  const uint64_t hit = __ballot(lane < n && pre > thr);
  if (hit) return __ffsll((long long)hit) - 1;
  const uint64_t nz = __ballot(lane < n && prior != 0.0f);
  return nz ? 63 - __clzll((long long)nz) : 0;
}

__device__ __forceinline__ double stochastic_chance_u(uint32_t seed, int level, int root) {
  const uint4 o = philox4x32_10(make_uint4((uint32_t)level, (uint32_t)root, 1u, 0u), make_uint2(seed, kStochasticKey));
  return u01(o.x, o.y);
}

// cbatch_traverse's walk of root i (:739-772), all 64 lanes of one wave, every argument wave-uniform. Writes path,
// path_act and best_action (:766) along the walk; the leaf is a chance node iff the returned len is odd.
// i: the root's index in the tree arrays; col / ps: where its path lives (path[l * ps + col]); root: its index in the
// batch, which keys the draws. stochastic_walk is the whole-batch form (all three the same, ps = t.B); the one-launch
// search (lzm_search_stoch_mlp.h) walks a workgroup's slice in LDS (gumbel_walk's li / R addressing).
__device__ inline Descent stochastic_walk_at(const TreeView &t, const StochasticView &sv, int i, int col, int ps,
                                             int root, float4 mm, int players, int vtp, float disc, uint32_t seed) {
  const int lane = threadIdx.x & 63;
  int node = 0, len = 0, last_action = -1, parent_latent = -1;
  float parent_q = 0.0f;  // per root; the reference's cross-root carry is 0 wherever it is read
  int latent = __builtin_amdgcn_readfirstlane(t.meta[nidx(t, 0, i)].latent);  // of `node`
  int visit = __builtin_amdgcn_readfirstlane(t.stat[nidx(t, 0, i)].visit);
  if (lane == 0) t.path[col] = 0;
  while (latent >= 0 && len < t.depth_cap - 1) {
    const bool chance = len & 1;
    // (A + (C - A) rather than a select between the two fields: a select of adjacent argument loads becomes an
    // indexed load of a scratch copy)
    const int n = __builtin_amdgcn_readfirstlane(len == 0 ? t.nlegal[i] : sv.A + (chance ? sv.C - sv.A : 0));
    const bool valid = lane < n;
    const int a = !valid ? 0 : (len == 0 ? t.legal[(size_t)i * t.A + lane] : lane);
    const int base = 1 + t.A * latent;
    // one round of reads per level: every child's record and latent index
    NodeStat c;
    c.visit = 0; c.value_sum = 0.0f; c.prior = 0.0f; c.reward = 0.0f;
    int clat = -1;
    if (valid) {
      c = t.stat[nidx(t, base + a, i)];
      clat = t.meta[nidx(t, base + a, i)].latent;
    }
    const float cv = node_value(c);
    // compute_mean_q (:195-229), chance levels included: visited children in child order
    const float qsa = c.reward + disc * cv;
    const uint64_t vis = __ballot(valid && c.visit > 0);
    const int total_v = __popcll(vis);
    float total_q = 0.0f;
    for (uint64_t q = vis; q; q &= q - 1) total_q += readlane_f(qsa, __ffsll((long long)q) - 1);
    const float mean_q = (len == 0 && total_v > 0) ? total_q / (float)total_v
                                                   : (parent_q + total_q) / (float)(total_v + 1);
    parent_q = mean_q;
    int jsel;
    if (chance) {
      jsel = stochastic_chance_pick(c.prior, n, stochastic_chance_u(seed, len, root));
    } else {
      // cucb_score of every child at once, the tie list by SURVEY A7's closed form (descend_wave)
      int N = visit - 1;
      N = N < 0 ? 0 : (N >= t.lut_n ? t.lut_n - 1 : N);
      const float2 L = t.lut[N];
      float pb_c = L.x;
      pb_c *= L.y / (float)(c.visit + 1);
      const float prior_score = pb_c * c.prior;
      float vs;
      if (c.visit == 0)
        vs = mean_q;
      else
        vs = (players == 1) ? c.reward + disc * cv : c.reward + disc * (-cv);
      vs = mm_normalize(mm, vs);
      if (vs < 0) vs = 0;
      if (vs > 1) vs = 1;
      const float score = prior_score + vs;
      const float M = wave_max_dpp(valid ? score : -INFINITY);
      const int r = __ffsll((long long)__ballot(valid && score == M)) - 1;
      uint64_t mask = __ballot(valid && lane > r && score >= M - 0.000001f) | (1ull << (r < 0 ? 0 : r));
      const uint4 o = philox4x32_10(make_uint4((uint32_t)len, (uint32_t)root, 0u, 0u), make_uint2(seed, kStochasticKey));
      int k = (int)((o.x >> 1) % (uint32_t)__popcll(mask));
      for (; k > 0; --k) mask &= mask - 1;
      jsel = __ffsll((long long)mask) - 1;
    }
    const int action = __builtin_amdgcn_readlane(a, jsel);
    if (players > 1) vtp = (vtp == 1) ? 2 : 1;  // at every level, chance levels too (:757-764)
    const int child = base + action;
    if (lane == 0) {
      t.meta[nidx(t, node, i)].best = action;
      t.path_act[(size_t)len * ps + col] = action;
      t.path[(size_t)(len + 1) * ps + col] = child;
    }
    parent_latent = latent;
    node = child;
    last_action = action;
    ++len;
    latent = __builtin_amdgcn_readlane(clat, jsel);
    visit = __builtin_amdgcn_readlane(c.visit, jsel);
  }
  Descent d;
  d.len = len; d.x = parent_latent; d.action = last_action; d.vtp = vtp; d.leaf = node;
  return d;
}

__device__ inline Descent stochastic_walk(const TreeView &t, const StochasticView &sv, int i, float4 mm, int players,
                                          int vtp, float disc, uint32_t seed) {
  return stochastic_walk_at(t, sv, i, i, t.B, i, mm, players, vtp, disc, seed);
}

struct StochasticTraverseArgs {
  TreeView t;
  StochasticView sv;
  const float4 *minmax;
  const uint32_t *seed;
  const int32_t *vtp_in;
  WalkOut out;
  int32_t *out_is_chance;  // optional copy of sv.is_chance for the caller
  float disc;
};

// cbatch_traverse's body for root i: the walk, pathlen, the request lists and the leaf kind
__device__ inline void stochastic_traverse_root(const StochasticTraverseArgs &p, int i) {
  const int players = stochastic_players(p.vtp_in, p.t.B);
  const Descent d = stochastic_walk(p.t, p.sv, i, p.minmax[i], players, p.vtp_in[i], p.disc, *p.seed);
  if ((threadIdx.x & 63) == 0) {
    store_walk(p.out, p.t, i, d.x, d.action, d.vtp, d.len);
    p.sv.is_chance[i] = d.len & 1;
    if (p.out_is_chance) p.out_is_chance[i] = d.len & 1;
  }
}

// CNode::expand (:96-173) of root i's leaf with a logit row of `width` entries (expand_wave with the child count
// apart from the block width t.A), then cbackpropagate (:496-557). A chance leaf's reward is 0 (:118).
__device__ inline void stochastic_expand_backup(const TreeView &t, const StochasticView &sv, float4 *minmax, int i,
                                                int to_play, int cur, float reward, float value, const float *logits,
                                                int width, float disc) {
  const int lane = threadIdx.x & 63;
  const int len = t.pathlen[i];
  const int leaf = t.path[(size_t)len * t.B + i];
  if (lane == 0) {
    NodeMeta m = t.meta[nidx(t, leaf, i)];
    m.latent = cur;
    m.to_play = to_play;
    t.meta[nidx(t, leaf, i)] = m;
    t.stat[nidx(t, leaf, i)].reward = sv.is_chance[i] ? 0.0f : reward;
  }
  const bool act = lane < width;
  const float lg = act ? logits[lane] : -INFINITY;
  const float pmax = fmaxf(kFloatMin, wave_max_dpp(lg));
  const float e = act ? glibc_expf(lg - pmax) : 0.0f;
  float sum = 0.0f;
  for (int a = 0; a < width; ++a) sum += readlane_f(e, a);
  if (act) {
    const int c = 1 + t.A * cur + lane;
    NodeStat cs;
    cs.visit = 0; cs.value_sum = 0.0f; cs.prior = e / sum; cs.reward = 0.0f;
    t.stat[nidx(t, c, i)] = cs;
    NodeMeta cm;
    cm.latent = -1; cm.to_play = 0; cm.best = -1; cm.is_reset = 0;
    t.meta[nidx(t, c, i)] = cm;
  }
  // (the backup reads the leaf's record in lane 0, the lane that has just stored it)
  backup_wave(t, i, i, t.B, minmax + i, to_play, value, disc);
}

// cbatch_backpropagate (:559-592) from raw lists: entry k serves root leaf_idx[k] (k itself without a list);
// rewards / values / logits rows are indexed by k, to_play by root (:588-589).
struct StochasticBackpropArgs {
  TreeView t;
  StochasticView sv;
  float4 *minmax;
  const float *rewards, *values, *logits;  // [n], [n], [n][width]
  const int32_t *to_play;                  // [B]
  const int32_t *leaf_idx;                 // [n] or null
  int n, width, cur;
  float disc;
};

__device__ inline void stochastic_backprop_entry(const StochasticBackpropArgs &p, int k) {
  const int i = __builtin_amdgcn_readfirstlane(p.leaf_idx ? p.leaf_idx[k] : k);
  if (i < 0 || i >= p.t.B) return;
  stochastic_expand_backup(p.t, p.sv, p.minmax, i, p.to_play[i], p.cur, p.rewards[k], p.values[k],
                           p.logits + (size_t)k * p.width, p.width, p.disc);
}

// The two sets of network heads of one simulation, each over the whole batch: the chance-leaf set from
// recurrent_inference(afterstate=False) (afterstate dynamics + afterstate prediction: value logits and a policy
// row of width C; its reward is overwritten by 0), the decision-leaf set from recurrent_inference(afterstate=True)
// (dynamics + prediction: reward logits, value logits and a policy row of width A). Root i reads the set of its
// leaf's kind.
struct StochasticDecodeArgs {
  TreeView t;
  StochasticView sv;
  float4 *minmax;
  const float *c_value, *c_policy, *c_latent;            // chance leaves
  const float *d_reward, *d_value, *d_policy, *d_latent;  // decision leaves
  const int32_t *to_play;
  float *pool_slot;
  long long row_elems;
  int V, Vv, categorical, cur;
  float disc;
  float *out_decoded;  // [B][2] {reward, value} after h^-1, optional
};

// decode + expand + backup of root i by one wave. sm_*: ensure_softmax's verdict per head tensor (true: apply the
// softmax), judged over every row of the batch as lzm_decode_backprop judges it.
__device__ inline void stochastic_decode_root(const StochasticDecodeArgs &p, int i, bool sm_cv, bool sm_dr, bool sm_dv) {
  const int lane = threadIdx.x & 63;
  const bool chance = __builtin_amdgcn_readfirstlane(p.sv.is_chance[i]) != 0;
  // the leaf's latent row (the afterstate for a chance leaf) into the pool slot
  const float *src = (chance ? p.c_latent : p.d_latent) + (size_t)i * p.row_elems;
  float *dst = p.pool_slot + (size_t)i * p.row_elems;
  for (long long e = lane; e < p.row_elems; e += 64) dst[e] = src[e];
  float r = 0.0f, v;
  const float *vrow = (chance ? p.c_value : p.d_value) + (size_t)i * p.Vv;
  if (p.categorical) {
    v = wave_support_expectation(vrow, p.Vv, chance ? sm_cv : sm_dv);
    if (!chance) r = wave_support_expectation(p.d_reward + (size_t)i * p.V, p.V, sm_dr);
  } else {
    v = vrow[0];
    if (!chance) r = p.d_reward[(size_t)i * p.V];
  }
  v = h_inverse(v);
  r = chance ? 0.0f : h_inverse(r);
  if (p.out_decoded && lane == 0) {
    p.out_decoded[2 * i] = r;
    p.out_decoded[2 * i + 1] = v;
  }
  const int width = p.sv.A + (chance ? p.sv.C - p.sv.A : 0);
  const float *logits = (chance ? p.c_policy : p.d_policy) + (size_t)i * width;
  stochastic_expand_backup(p.t, p.sv, p.minmax, i, p.to_play[i], p.cur, r, v, logits, width, p.disc);
}

}  // namespace lzm
