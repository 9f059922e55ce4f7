// lzm_gumbel.h — the Gumbel MuZero tree (gfx950): selection walk and outputs, one wave per root.
//
// Restates lzero/mcts/ctree/ctree_gumbel_muzero/lib/cnode.cpp (reference paths under /root/reference;
// line numbers of that file): cbatch_traverse :834-898 with cselect_root_child :701-745 (sequential
// halving over a fixed Gumbel vector) and cselect_interior_child :747-790 (deterministic argmax over
// completed Q), qtransform_completed_by_mix_value :989-1040 (get_q :181-197, csoftmax :904-933,
// compute_mixed_value :935-970, rescale_qvalues :972-987; defaults cnode.h:100-102), score_considered
// :1097-1132, get_children_value :309-338 and get_policy :355-385. Expansion and backup are the MuZero
// tree's (expand_wave; backup_wave with to_play = -1: cback_propagate :605-631 has no player sign) plus the
// node's raw_value (:111), kept in an array of its own [cap][B] that only Gumbel handles allocate.
//
// The walk never draws a random number: there is no batch-serial rand() stream, so roots are fully
// independent — no flags, no epochs, no look-back.
//
// Lane j holds legal position j at the root and action j below it (A <= 64). Element-wise work runs in
// lanes. Every float sum of the reference (csoftmax's sum, probs_sum, weighted_q_sum) is reproduced in
// ITS order by a wave-uniform serial loop of readlanes: a butterfly would add the same terms in another
// order, round differently in the last bit, and a one-bit difference in a completed Q flips the strict
// argmax between near-equal children. Visit sums are integer sums below 2^24, which the reference's
// float accumulator holds exactly in any order. Max and min are order-free (DPP).
#pragma once
#include "lzm_tree.h"

namespace lzm {

struct GumbelView {
  float *raw;                 // [cap][B] raw_value per node (cnode.cpp:111)
  const float *gumbel;        // [64] generate_gumbel(10, 0, .) (:1134-1152), indexed by legal position
  const int32_t *considered;  // [S] the row of get_table_of_considered_visits cselect_root_child reads (:727-729)
  int S;                      // length of `considered`
};

// sum of v over lanes [0, n) in lane order (wave-uniform chain)
__device__ __forceinline__ float ordered_sum(float v, int n) {
  float s = 0.0f;
  for (int j = 0; j < n; ++j) s += readlane_f(v, j);
  return s;
}
// sum of v over the lanes of `mask` in lane order
__device__ __forceinline__ float ordered_sum_mask(float v, uint64_t mask) {
  float s = 0.0f;
  for (uint64_t q = mask; q; q &= q - 1) s += readlane_f(v, __ffsll((long long)q) - 1);
  return s;
}
__device__ __forceinline__ float wave_min_dpp(float v) { return -wave_max_dpp(-v); }

// csoftmax (:904-933) of x over lanes [0, n) (x = -inf allowed: expf(-inf) = +0): max, the sum of
// expf(x - m) in order, then expf(x - m - logf(sum)). The sum lies in [1, n]: glibc_logf's checked range.
__device__ inline float gumbel_softmax(float x, bool valid, int n) {
  const float m = wave_max_dpp(valid ? x : -INFINITY);
  const float e = valid ? glibc_expf(x - m) : 0.0f;
  const float sum = ordered_sum(e, n);
  const float ls = glibc_logf(sum);
  return valid ? glibc_expf(x - m - ls) : 0.0f;
}

// The children of one expanded node, lane j = legal position j.
struct GumbelChildren {
  int a, visit, n, total_visits;
  int latent;       // the child's current_latent_state_index (-1: not expanded), read with its record
  float prior, cq;  // cq: completed Q (qtransform_completed_by_mix_value)
  bool valid;
};

__device__ inline GumbelChildren gumbel_children(const TreeView &t, const GumbelView &g, int i, int node, int latent,
                                                 float disc) {
  const int lane = threadIdx.x & 63;
  GumbelChildren c;
  c.n = __builtin_amdgcn_readfirstlane(legal_n(t, i, node));  // wave-uniform: the ordered sums' loop bound
  c.valid = lane < c.n;
  c.a = c.valid ? legal_at(t, i, node, lane) : 0;
  // one round of reads per level: every child's record and latent index, and the node's raw_value; the walk takes
  // the chosen child's latent index from the lane that read it instead of a second, dependent read
  NodeStat s;
  s.visit = 0; s.value_sum = 0.0f; s.prior = 0.0f; s.reward = 0.0f;
  c.latent = -1;
  if (c.valid) {
    s = t.stat[nidx(t, 1 + t.A * latent + c.a, i)];
    c.latent = t.meta[nidx(t, 1 + t.A * latent + c.a, i)].latent;
  }
  const float raw_value = g.raw[nidx(t, node, i)];
  c.visit = s.visit;
  c.prior = s.prior;
  const float q = s.reward + disc * node_value(s);  // get_q
  float p = gumbel_softmax(c.prior, c.valid, c.n);  // the priors, already probabilities, through csoftmax again
  p = (p < -10e7f) ? -10e7f : p;                    // std::max(prior, min_num) (:958)
  const uint64_t vis = __ballot(c.valid && c.visit > 0);
  c.total_visits = xor_sum(c.valid ? c.visit : 0);
  const float vsum = (float)c.total_visits;
  const float probs_sum = ordered_sum_mask(p, vis);
  const float weighted = ordered_sum_mask(p * q / probs_sum, vis);
  const float mixed = (raw_value + vsum * weighted) / (vsum + 1.0f);
  float cq = c.visit > 0 ? q : mixed;
  const float mx = wave_max_dpp(c.valid ? cq : -INFINITY);
  const float mn = wave_min_dpp(c.valid ? cq : INFINITY);
  float gap = mx - mn;
  gap = (gap < 1e-8f) ? 1e-8f : gap;  // rescale_qvalues
  cq = (cq - mn) / gap;
  const float scale = 50.0f + (float)xor_max(c.valid ? c.visit : 0);
  c.cq = cq * scale * 0.1f;
  return c;
}

// first strict maximum from -inf in legal order (:733-742, :778-787); position 0 when every score is -inf
__device__ __forceinline__ int gumbel_argmax(float score, bool valid) {
  const float M = wave_max_dpp(valid ? score : -INFINITY);
  const uint64_t hit = __ballot(valid && score == M && M > -INFINITY);
  return hit ? __ffsll((long long)hit) - 1 : 0;
}

// cbatch_traverse's walk of one root (:863-894), all 64 lanes of one wave; every argument wave-uniform. The root
// is tree index i of t (records, legal lists, raw_value); its path is column `col` of t.path / t.path_act, whose
// rows are `ps` apart (the generic kernels: i and t.B; the one-launch search: the workgroup's LDS slice, local
// root and roots per workgroup, wherever the tree itself lives). Writes path / path_act and best_action along
// the path (:879); returns the request (len, x = the leaf's parent's latent index, action), which the caller
// files where its kernel keeps requests.
__device__ inline Descent gumbel_walk(const TreeView &t, const GumbelView &g, float disc, int i, int col, int ps) {
  const int lane = threadIdx.x & 63;
  int node = 0, len = 0, last_action = -1, parent_latent = -1;
  // (scalar: the root's record is a per-lane read when the tree is a slice in LDS)
  int latent = __builtin_amdgcn_readfirstlane(t.meta[nidx(t, 0, i)].latent);  // of `node`
  if (lane == 0) t.path[col] = 0;
  while (latent >= 0 && len < t.depth_cap - 1) {
    const GumbelChildren c = gumbel_children(t, g, i, node, latent, disc);
    float score;
    if (len == 0) {
      // cselect_root_child: score_considered over the children with the considered visit count
      int si = c.total_visits;
      si = si < 0 ? 0 : (si >= g.S ? g.S - 1 : si);  // (past num_simulations the reference reads out of bounds)
      const int considered = g.considered[si];
      const float pm = wave_max_dpp(c.valid ? c.prior : -INFINITY);
      const float gl = c.valid ? g.gumbel[lane] : 0.0f;
      float sc = gl + (c.prior - pm) + c.cq;
      sc = (-1e9f < sc) ? sc : -1e9f;  // std::max(low_logit, .)
      score = sc + (c.visit == considered ? 0.0f : -INFINITY);
    } else {
      // cselect_interior_child
      const float pr = gumbel_softmax(c.prior + c.cq, c.valid, c.n);
      score = pr - (float)c.visit / (float)(1 + c.total_visits);
    }
    const int jsel = gumbel_argmax(score, c.valid);
    const int action = __builtin_amdgcn_readlane(c.a, jsel);
    const int child = 1 + t.A * latent + action;
    if (lane == 0) {
      t.meta[nidx(t, node, i)].best = action;
      t.path_act[(size_t)len * ps + col] = action;
      t.path[(size_t)(len + 1) * ps + col] = child;
    }
    parent_latent = latent;
    node = child;
    last_action = action;
    ++len;
    latent = __builtin_amdgcn_readlane(c.latent, jsel);
  }
  Descent d;
  d.len = len; d.x = parent_latent; d.action = last_action; d.vtp = 0; d.leaf = node;
  return d;
}

// cbatch_traverse's body for root i (:863-896) in the generic kernels: the walk, pathlen and the request lists.
struct GumbelTraverseArgs {
  TreeView t;
  GumbelView g;
  const int32_t *vtp_in;
  WalkOut out;
  float disc;
};

__device__ inline void gumbel_traverse_root(const GumbelTraverseArgs &p, int i) {
  const Descent d = gumbel_walk(p.t, p.g, p.disc, i, i, p.t.B);
  // virtual_to_play is passed through (:895): the Gumbel tree has no player bookkeeping
  if ((threadIdx.x & 63) == 0) store_walk(p.out, p.t, i, d.x, d.action, p.vtp_in[i], d.len);
}

// value of the lane holding legal position j, moved to lane legal[j] (action order); `fill` elsewhere
__device__ __forceinline__ float gumbel_scatter(float v, int a, int n, float fill) {
  const int lane = threadIdx.x & 63;
  float x = fill;
  for (int j = 0; j < n; ++j) {
    const int aj = __builtin_amdgcn_readlane(a, j);
    const float vj = readlane_f(v, j);
    if (lane == aj) x = vj;
  }
  return x;
}

// get_children_value (:309-338; policy == 0) / get_policy (:355-385; policy != 0) of root i into out[i][A].
__device__ inline void gumbel_root_output(const TreeView &t, const GumbelView &g, int i, float disc, int policy,
                                          float *out) {
  const int lane = threadIdx.x & 63;
  const NodeMeta m = t.meta[nidx(t, 0, i)];
  float *row = out + (size_t)i * t.A;
  if (m.latent < 0) {  // not prepared: no children
    if (lane < t.A) row[lane] = policy ? 0.0f : -INFINITY;
    return;
  }
  const GumbelChildren c = gumbel_children(t, g, i, 0, m.latent, disc);
  // to action order, -inf for illegal actions; the policy is csoftmax over all A entries (expf(-inf) = +0)
  float x = gumbel_scatter(policy ? c.prior + c.cq : c.cq, c.a, c.n, -INFINITY);
  if (policy) x = gumbel_softmax(x, lane < t.A, t.A);
  if (lane < t.A) row[lane] = x;
}

// What GumbelMuZeroPolicy._forward_collect reads from a root after the search (policy/gumbel_muzero.py:562-589),
// from ONE evaluation of the root's completed Q: get_distributions (visit counts in legal order, -1 past the legal
// count: lzm_get_root_outputs' rows), get_values, get_children_values with the policy's mask applied (0 where
// illegal), get_policies, and the action the policy takes — np.argmax over the masked policy row, its first maximum.
struct GumbelCollectOut {
  int32_t *dist;    // [B][A]
  float *values;    // [B]
  float *cq;        // [B][A] action order
  float *policy;    // [B][A] action order
  int32_t *action;  // [B]
};

__device__ inline void gumbel_collect_output(const TreeView &t, const GumbelView &g, int i, float disc,
                                             const GumbelCollectOut &o) {
  const int lane = threadIdx.x & 63;
  const NodeMeta m = t.meta[nidx(t, 0, i)];
  const size_t row = (size_t)i * t.A;
  if (lane == 0) o.values[i] = node_value(t.stat[nidx(t, 0, i)]);
  if (m.latent < 0) {  // not prepared: no children
    if (lane < t.A) {
      o.dist[row + lane] = -1;
      o.cq[row + lane] = 0.0f;
      o.policy[row + lane] = 0.0f;
    }
    if (lane == 0) o.action[i] = 0;
    return;
  }
  const GumbelChildren c = gumbel_children(t, g, i, 0, m.latent, disc);
  if (lane < t.A) o.dist[row + lane] = c.valid ? c.visit : -1;
  // to action order as gumbel_root_output does; the masked completed Q is 0 where the policy row is exactly 0
  const float q = gumbel_scatter(c.cq, c.a, c.n, 0.0f);
  float x = gumbel_scatter(c.prior + c.cq, c.a, c.n, -INFINITY);
  x = gumbel_softmax(x, lane < t.A, t.A);
  if (lane < t.A) {
    o.cq[row + lane] = q;
    o.policy[row + lane] = x;
  }
  // illegal entries are exact zeros below the row's maximum (the row sums to 1), so the first maximum over all A
  // lanes is the first maximum over the legal ones: the lane index is the action id
  const int a = gumbel_argmax(x, lane < t.A);
  if (lane == 0) o.action[i] = a;
}

}  // namespace lzm
