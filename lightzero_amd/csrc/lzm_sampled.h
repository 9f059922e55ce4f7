// lzm_sampled.h — the Sampled EfficientZero tree (gfx950): K sampled actions per node, one wave per root.
//
// Restates lzero/mcts/ctree/ctree_sampled_efficientzero/lib/cnode.cpp (line numbers of that file):
//   cucb_score :1026-1108. `empirical_distribution_type.compare("density")` (:1054-1055) returns 0 for equal
//     strings, so the "uniform" branch (:1076-1079) runs: prior_score = pb_c * 1 / parent->children.size(). The child
//     priors written by expand (:422-445: log-probs, or probs in discrete mode) and the root noise
//     (add_exploration_noise :454-481) are never read by selection. The device tree therefore keeps a uniform prior
//     over the node's K children and computes no log-probs; the "density" branch is out of scope.
//   compute_mean_q :483-523, cselect_child :973-1023 (the order-dependent 1e-6 tie list, one rand() per level),
//     cbatch_traverse :1110-1187, cbackpropagate :860-945 and cbatch_backpropagate :947-971 (is_reset stored on
//     the leaf) are EfficientZero's value-prefix rules over the K slots.
//   CNode::expand, continuous :238-284, :426-432: K vectors x_d ~ N(mu_d, sigma_d), d < D = len(policy_logits) / 2
//     (policy_logits[D:2D] is sigma itself), the action is tanh(x). Discrete :325-406: p_a = exp(l_a) / (sum exp(l)
//     + 1e-6) without max subtraction, keys u_a^(1 / p_a) in double, sorted descending, the first K actions are
//     slots 0..K-1; legal-action masks are ignored (the reference's own TODO :305). Both seed a
//     std::default_random_engine from system_clock::now(): there is no stream to stay in parity with.
//   The reference keys children by the action's hash, so two bit-identical sampled vectors share one child; the
//   device keeps K slots always.
//
// Work split (the Gumbel / stochastic families'): one wave per root, four roots per 256-thread workgroup, the
// root index in a scalar register, no cross-root communication, no LDS, no scratch. Lane j is slot j of the current
// node, so K <= 64; a level is one round of child reads, the chosen child's records come from the lane that read
// them (readlane). Float sums run in the reference's slot order by readlane chains.
//
// Node storage is the EfficientZero tree's (NodeStat / NodeMeta) with block width K in TreeView::A: children of the
// node expanded by simulation L at 1 + K * L + j, the root's legal list is 0..K-1, so the shared distribution, value,
// trajectory and latent-gather kernels address such a handle unchanged. The per-handle action table holds the
// sampled actions: float32 [(S+1)*K][B][D] (continuous) or int32 [(S+1)*K][B] (discrete); entry (L*K + j, i) is
// slot j of root i's node expanded by simulation L (0: the root). A slot's D floats are contiguous: the walk's
// last read is one access by lanes d < D, stored straight into the network's last_actions row.
//
// Randomness: Philox4x32-10 under key (seed, kSampledKey); every draw is a pure function of its counter:
//   tie draw at level l of root i:          counter (l, i, 0, 0), word x >> 1 modulo the tie count
//   continuous, node L, slot j, dims 2m, 2m+1: counter (L, i, 2 | j << 8, m), u1 = u01(x, y), u2 = u01(z, w)
//       (lzm_collect.h), Box-Muller in double: z0 = sqrt(-2 ln u1) cos(2 pi u2), z1 = .. sin(..);
//       x_d = (float)(mu_d + sigma_d * z), action_d = (float)tanh((double)x_d); an odd D drops the last z1
//   discrete, node L, action a:             counter (L, i, 3, a), u = u01(x, y), key pow(u, 1.0 / p_a) in double;
//       slot = the number of actions with a larger key (equal keys: the lower action first); slots < K are kept.
#pragma once
#include "lzm_collect.h"
#include "lzm_tree.h"

namespace lzm {

constexpr uint32_t kSampledKey = 0x53414d50u;
constexpr int kSampledMaxDim = 32;

struct SampledView {
  int K, D, A;     // slots per node; continuous: D dims (A = 0); discrete: A actions (D = 0)
  float *act_f;    // continuous action table
  int32_t *act_i;  // discrete action table
};

__device__ __forceinline__ double readlane_d(double v, int lane) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, lane);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), lane);
  return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
}

__device__ __forceinline__ float sampled_squash(float mu, float sigma, double z) {
  const float x = (float)((double)mu + (double)sigma * z);
  return (float)tanh((double)x);
}

// The K sampled vectors of root i's node L from its policy row {mu[D], sigma[D]}: one (slot, dim pair) per lane
// and round, K * ceil(D / 2) items in all. i: the root's index in the batch of tb roots (the draws' counters and the
// action table's addressing; the one-launch search's tree view is a slice, its table the whole batch's).
__device__ inline void sampled_draw_continuous(const SampledView &sv, int tb, int i, int L, const float *row,
                                               uint32_t seed) {
  const int D = sv.D, P = (D + 1) >> 1, n = sv.K * P;
  for (int e = threadIdx.x & 63; e < n; e += 64) {
    const int j = e / P, m = e - j * P, d0 = 2 * m;
    const uint4 o = philox4x32_10(make_uint4((uint32_t)L, (uint32_t)i, 2u | ((uint32_t)j << 8), (uint32_t)m),
                                  make_uint2(seed, kSampledKey));
    const double r = sqrt(-2.0 * log(u01(o.x, o.y))), a = 6.283185307179586 * u01(o.z, o.w);
    float *dst = sv.act_f + (((size_t)L * sv.K + j) * tb + i) * D;
    dst[d0] = sampled_squash(row[d0], row[D + d0], r * cos(a));
    if (d0 + 1 < D) dst[d0 + 1] = sampled_squash(row[d0 + 1], row[D + d0 + 1], r * sin(a));
  }
}

// The K of A actions of root i's node L, without replacement, from its logit row: lane a is action a.
__device__ inline void sampled_draw_discrete(const TreeView &t, const SampledView &sv, int i, int L, const float *row,
                                             uint32_t seed) {
  const int lane = threadIdx.x & 63;
  const int A = sv.A;
  const bool act = lane < A;
  const float e = act ? glibc_expf(row[lane]) : 0.0f;
  float sum = 0.0f;
  for (int a = 0; a < A; ++a) sum += readlane_f(e, a);
  const float p = (float)((double)e / ((double)sum + 1e-6));
  const uint4 o = philox4x32_10(make_uint4((uint32_t)L, (uint32_t)i, 3u, (uint32_t)lane), make_uint2(seed, kSampledKey));
  const double key = act ? pow(u01(o.x, o.y), 1.0 / (double)p) : -1.0;
  int rank = 0;
  for (int b = 0; b < A; ++b) {
    const double kb = readlane_d(key, b);
    rank += (kb > key || (kb == key && b < lane)) ? 1 : 0;
  }
  if (act && rank < sv.K) sv.act_i[((size_t)L * sv.K + rank) * t.B + i] = lane;
}

// CNode::expand (:194-452) of node `leaf` of root i as the node of simulation `cur` (0: the root, whose own
// record the caller writes): K fresh children and their sampled actions. All 64 lanes, wave-uniform arguments.
// i: the root's index in the tree arrays; root / tb: its index in the batch and the batch's size, which key the
// draws and address the action table. sampled_expand is the whole-batch form (i == root, tb == t.B); the one-launch
// search (lzm_search_sampled_mlp.h) expands into a workgroup's slice in LDS (continuous actions only).
template <bool CONT>
__device__ inline void sampled_expand_at(const TreeView &t, const SampledView &sv, int i, int root, int tb, int leaf,
                                         int to_play, int cur, float value_prefix, const float *row, int is_reset,
                                         uint32_t seed) {
  const int lane = threadIdx.x & 63;
  if (lane == 0 && cur > 0) {
    NodeMeta m = t.meta[nidx(t, leaf, i)];
    m.latent = cur;
    m.to_play = to_play;
    m.is_reset = is_reset;  // (:967)
    t.meta[nidx(t, leaf, i)] = m;
    t.stat[nidx(t, leaf, i)].reward = value_prefix;
  }
  if (lane < sv.K) {
    const int c = 1 + sv.K * cur + lane;
    NodeStat cs;
    cs.visit = 0; cs.value_sum = 0.0f; cs.prior = 0.0f; cs.reward = 0.0f;  // (the prior is never read, :1076-1079)
    t.stat[nidx(t, c, i)] = cs;
    NodeMeta cm;
    cm.latent = -1; cm.to_play = 0; cm.best = -1; cm.is_reset = 0;
    t.meta[nidx(t, c, i)] = cm;
  }
  if (CONT) sampled_draw_continuous(sv, tb, root, cur, row, seed);
  else sampled_draw_discrete(t, sv, i, cur, row, seed);
}

template <bool CONT>
__device__ inline void sampled_expand(const TreeView &t, const SampledView &sv, int i, int leaf, int to_play, int cur,
                                      float value_prefix, const float *row, int is_reset, uint32_t seed) {
  sampled_expand_at<CONT>(t, sv, i, i, t.B, leaf, to_play, cur, value_prefix, row, is_reset, seed);
}

// CRoots::prepare / prepare_no_noise (:677-715) of root i: the root's record, its legal list 0..K-1 (for the
// shared root kernels), expand, visit_count = 1. The noises do not influence the search (:454-481, :1076-1079).
struct SampledPrepareArgs {
  TreeView t;
  SampledView sv;
  int32_t *legal, *nlegal;
  const float *value_prefixs, *policy;  // [B], [B][2D or A]
  const int32_t *to_play;
  const uint32_t *seed;
};

template <bool CONT>
__device__ inline void sampled_prepare_root(const SampledPrepareArgs &p, int i) {
  const int lane = threadIdx.x & 63;
  const int K = p.sv.K;
  if (lane < K) p.legal[(size_t)i * K + lane] = lane;
  if (lane == 0) {
    p.nlegal[i] = K;
    p.t.pathlen[i] = 0;
    NodeStat r;
    r.visit = 1; r.value_sum = 0.0f; r.prior = 0.0f; r.reward = p.value_prefixs[i];
    p.t.stat[i] = r;
    NodeMeta rm;
    rm.latent = 0; rm.to_play = p.to_play[i]; rm.best = -1; rm.is_reset = 0;
    p.t.meta[i] = rm;
  }
  const int width = CONT ? 2 * p.sv.D : p.sv.A;
  sampled_expand<CONT>(p.t, p.sv, i, 0, 0, 0, 0.0f, p.policy + (size_t)i * width, 0, *p.seed);
}

struct SampledTraverseArgs {
  TreeView t;
  SampledView sv;
  const float4 *minmax;
  const uint32_t *seed;
  const int32_t *vtp_in;
  WalkOut out;      // out_a: the chosen slot of the leaf's parent; out_a64 unused
  void *out_action; // last_actions: float32 [B][D] (continuous) or int64 [B] (discrete)
  float disc;
};

// cbatch_traverse's walk of root i (:1145-1186), all 64 lanes of one wave, every argument wave-uniform. Writes path,
// path_act and best_action along the walk and returns {len, the leaf's parent's latent index, the chosen slot of
// that parent, the leaf's to_play, the leaf}. i: the root's index in the tree arrays; col / ps: where its path
// lives (path[l * ps + col]); root: its index in the batch, which keys the tie draws. sampled_traverse_root is the
// whole-batch form (all three the same, ps = t.B); the one-launch search (lzm_search_sampled_mlp.h) walks a
// workgroup's slice in LDS (stochastic_walk_at's addressing).
__device__ inline Descent sampled_walk_at(const TreeView &t, int K, int i, int col, int ps, int root, float4 mm,
                                          int players, int vtp, float disc, uint32_t seed) {
  const int lane = threadIdx.x & 63;
  const float Kf = (float)K;
  int node = 0, len = 0, slot = -1, parent_latent = -1;
  float parent_q = 0.0f;  // per root; the reference's cross-root carry is 0 wherever it is read
  NodeStat s = t.stat[nidx(t, 0, i)];
  NodeMeta m = t.meta[nidx(t, 0, i)];
  if (lane == 0) t.path[col] = 0;
  while (m.latent >= 0 && len < t.depth_cap - 1) {
    const int latent = __builtin_amdgcn_readfirstlane(m.latent);
    const int base = 1 + K * latent;
    const float pvp = s.reward;
    const int preset = m.is_reset;
    const bool valid = lane < K;
    NodeStat c;
    c.visit = 0; c.value_sum = 0.0f; c.prior = 0.0f; c.reward = 0.0f;
    NodeMeta cm;
    cm.latent = -1; cm.to_play = 0; cm.best = -1; cm.is_reset = 0;
    if (valid) {
      c = t.stat[nidx(t, base + lane, i)];
      cm = t.meta[nidx(t, base + lane, i)];
    }
    const float cv = node_value(c);
    const float tr = preset == 1 ? c.reward : c.reward - pvp;
    // compute_mean_q (:483-523): visited children in slot order
    const float qsa = tr + disc * cv;
    const uint64_t vis = __ballot(valid && c.visit > 0);
    const int total_v = __popcll(vis);
    float total_q = 0.0f;
    for (uint64_t q = vis; q; q &= q - 1) total_q += readlane_f(qsa, __ffsll((long long)q) - 1);
    const float mean_q = (len == 0 && total_v > 0) ? total_q / (float)total_v
                                                   : (parent_q + total_q) / (float)(total_v + 1);
    parent_q = mean_q;
    // cucb_score (:1026-1108) of every slot at once: the uniform prior, the value-prefix Q
    int N = s.visit - 1;
    N = N < 0 ? 0 : (N >= t.lut_n ? t.lut_n - 1 : N);
    const float2 L = t.lut[N];
    float pb_c = L.x;
    pb_c *= L.y / (float)(c.visit + 1);
    const float prior_score = pb_c / Kf;
    float vs;
    if (c.visit == 0)
      vs = mean_q;
    else
      vs = (players == 1) ? tr + disc * cv : tr + disc * (-cv);
    vs = mm_normalize(mm, vs);
    if (vs < 0) vs = 0;
    if (vs > 1) vs = 1;
    const float score = prior_score + vs;
    // the tie list by SURVEY A7's closed form, one draw per level
    const float M = wave_max_dpp(valid ? score : -INFINITY);
    const int r = __ffsll((long long)__ballot(valid && score == M)) - 1;
    uint64_t mask = __ballot(valid && lane > r && score >= M - 0.000001f) | (1ull << (r < 0 ? 0 : r));
    const uint4 o = philox4x32_10(make_uint4((uint32_t)len, (uint32_t)root, 0u, 0u), make_uint2(seed, kSampledKey));
    int k = (int)((o.x >> 1) % (uint32_t)__popcll(mask));
    for (; k > 0; --k) mask &= mask - 1;
    slot = __builtin_amdgcn_readfirstlane(__ffsll((long long)mask) - 1);
    if (players > 1) vtp = (vtp == 1) ? 2 : 1;
    const int child = base + slot;
    if (lane == 0) {
      t.meta[nidx(t, node, i)].best = slot;
      t.path_act[(size_t)len * ps + col] = slot;
      t.path[(size_t)(len + 1) * ps + col] = child;
    }
    parent_latent = latent;
    node = child;
    ++len;
    s.visit = __builtin_amdgcn_readlane(c.visit, slot);
    s.reward = readlane_f(c.reward, slot);
    m.latent = __builtin_amdgcn_readlane(cm.latent, slot);
    m.is_reset = __builtin_amdgcn_readlane(cm.is_reset, slot);
  }
  Descent d;
  d.len = len; d.x = parent_latent; d.action = slot; d.vtp = vtp; d.leaf = node;
  return d;
}

// cbatch_traverse's walk of root i and its request rows, all 64 lanes of one wave.
template <bool CONT>
__device__ inline void sampled_traverse_root(const SampledTraverseArgs &p, int i) {
  const TreeView &t = p.t;
  const int lane = threadIdx.x & 63;
  const int K = p.sv.K;
  // players = (max(virtual_to_play) == -1) ? 1 : 2 (:1138-1143), by every wave for itself
  int vmax = INT_MIN;
  for (int j = lane; j < t.B; j += 64) vmax = max(vmax, p.vtp_in[j]);
  const int players = xor_max(vmax) == -1 ? 1 : 2;
  const Descent d = sampled_walk_at(t, K, i, i, t.B, i, p.minmax[i], players, p.vtp_in[i], p.disc, *p.seed);
  const int len = d.len, parent_latent = d.x, slot = d.action, vtp = d.vtp;
  // the chosen slot's action, straight into the network's input row
  if (len > 0) {
    const size_t e = ((size_t)parent_latent * K + slot) * t.B + i;
    if (CONT) {
      if (lane < p.sv.D) ((float *)p.out_action)[(size_t)i * p.sv.D + lane] = p.sv.act_f[e * p.sv.D + lane];
    } else if (lane == 0) {
      ((long long *)p.out_action)[i] = p.sv.act_i[e];
    }
  }
  if (lane == 0) store_walk(p.out, t, i, parent_latent, slot, vtp, len);
}

// cbatch_backpropagate (:947-971) of root i: expand the last walk's leaf, store is_reset, back up.
template <bool CONT>
__device__ inline void sampled_expand_backup(const TreeView &t, const SampledView &sv, float4 *minmax, int i, int to_play,
                                             int cur, float value_prefix, float value, const float *row, int is_reset,
                                             uint32_t seed, float disc) {
  const int len = t.pathlen[i];
  const int leaf = t.path[(size_t)len * t.B + i];
  sampled_expand<CONT>(t, sv, i, leaf, to_play, cur, value_prefix, row, is_reset, seed);
  // (the backup reads the leaf's record in lane 0 only, the lane that has just stored it: backup_wave_ez's contract)
  backup_wave_ez(t, i, i, t.B, minmax + i, to_play, value, disc);
}

struct SampledBackpropArgs {
  TreeView t;
  SampledView sv;
  float4 *minmax;
  const float *value_prefixs, *values, *policy;  // [B], [B], [B][2D or A]
  const int32_t *to_play, *is_reset;             // [B]
  const uint32_t *seed;
  int cur;
  float disc;
};

// roots' sampled actions (CRoots::get_sampled_actions :759-787): [B][K][D] float32 or [B][K] int32
__device__ inline void sampled_root_actions(const TreeView &t, const SampledView &sv, int i, void *out) {
  const int lane = threadIdx.x & 63;
  if (sv.D > 0) {
    for (int e = lane; e < sv.K * sv.D; e += 64) {
      const int j = e / sv.D, d = e - j * sv.D;
      ((float *)out)[((size_t)i * sv.K + j) * sv.D + d] = sv.act_f[((size_t)j * t.B + i) * sv.D + d];
    }
  } else if (lane < sv.K) {
    ((int32_t *)out)[(size_t)i * sv.K + lane] = sv.act_i[(size_t)lane * t.B + i];
  }
}

}  // namespace lzm
