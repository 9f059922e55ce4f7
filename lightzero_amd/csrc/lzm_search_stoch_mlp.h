// lzm_search_stoch_mlp.h — one launch = one whole Stochastic MuZero search (all simulations) for
// StochasticMuZeroModelMLP (lzero/model/stochastic_muzero_model_mlp.py, recurrent_inference of
// stochastic_muzero_model.py:233-273; StochasticMuZeroMCTSCtree.search, mcts_ctree_stochastic.py:116-251).
//
// Decomposition: search_mlp_kernel's (lzm_search_mlp.h). Workgroup g owns roots [g R, g R + R), its tree slice
// staged in LDS for the whole search (or left in HBM when it does not fit), one wave per root for the walk
// (stochastic_walk_at, lzm_stochastic.h), the expansion and the backup, all 512 lanes for the network over the
// workgroup's R rows (dense_step: f32 FMAs over weights streamed from L2 in lane order). Roots exchange nothing.
//
// What is new here is that the leaves of one simulation are of two kinds and each kind has a network of its own:
//   branch 0, chance leaf (odd depth):    [state ; one-hot action]       -> afterstate, afterstate value, policy [C]
//   branch 1, decision leaf (even depth): [afterstate ; one-hot outcome] -> state, reward, value, policy [A]
// The kernel arguments carry one schedule of StepRecs per branch. After the walks the workgroup looks at the kinds
// of its rows (s_len & 1, in LDS) and runs a branch's schedule over all R rows only if some row has that kind: one
// pass or two, a workgroup-uniform decision. Both passes read the same gathered latent rows; the one-hot rows are
// rewritten per pass with the option clamped into the branch's range (a row of the other kind computes a valid,
// discarded result). After each pass the rows of ITS kind are harvested: the next latent goes to pool[k + 1], the
// logits row, the decoded value and reward to LDS regions no pass writes, so the first pass's results survive the
// second.
//
// Weight prefetch. dense_step refills its register buffer for the step two on. Inside a pass, and from the last two
// steps of a first pass into the first two of the second (both kinds are known when the passes start), that is
// search_mlp_kernel's rule. The last two steps of a simulation's LAST pass prefetch the idle step (every load out of
// range: zeros, no memory request), because the next simulation's first branch is unknown until its walk is done;
// the first two steps' weights are issued right after the walk, in front of the latent gather, whose pool reads and
// one-hot fill cover the round trip. So no step ever consumes weights fetched for the other branch, at the price of
// not overlapping two loads with the tree phase. (Prefetching both branches speculatively would double the two
// register buffers — up to 80 more registers at R = 1 — for the sake of one L2 round trip per simulation.)
#pragma once
#include "lzm_search_mlp.h"
#include "lzm_stochastic.h"

namespace lzm {

constexpr int kStochSteps = 12;            // schedule steps per branch at most
constexpr int kStochIdle = 2 * kStochSteps;  // sched[kStochIdle]: the idle step

struct StochSearchArgs {
  // tree (HBM, whole batch); W: the child-block width max(A, C)
  NodeStat *stat;
  NodeMeta *meta;
  const int32_t *legal, *nlegal;
  int32_t *path, *path_act, *pathlen, *is_chance;
  const float2 *lut;
  int B, W, A, C, cap, lut_n, depth_cap;
  // search
  int S;
  float disc;
  const uint32_t *seeds;  // [S]
  const int32_t *vtp_in;  // [B]
  float4 *minmax;         // [B]
  float *pool;            // [S + 1][B][H]
  int H, V;
  // optional per-simulation record, may be null: [S][B] each, rec_dec [S][B][2], rec_logits [S][B][W]
  int32_t *rec_x, *rec_a, *rec_len, *rec_chance, *rec_vtp;
  float *rec_dec, *rec_logits;
  // the two schedules (branch b: sched[b * kStochSteps ..], nsteps[b] steps, both even) and the idle step
  StepRec sched[2 * kStochSteps + 1];
  int nsteps[2];
  // dynamic LDS layout (float offsets)
  size_t off_stat, off_meta, off_lut, off_legal, off_path, off_pact, off_x0, off_x1, off_n, off_logit, off_keep,
      off_seeds;
};

// CNode::expand (:96-173) of a leaf by one wave, one lane per child, with the child count `width` apart from the
// block width t.A (stochastic_expand_backup's expansion, with the tree index i apart from the path's place).
__device__ inline void stochastic_expand_wave(const TreeView &t, int i, int leaf, int to_play, int cur, float reward,
                                              const float *logits, int width) {
  const int lane = threadIdx.x & 63;
  if (lane == 0) {
    NodeMeta m = t.meta[nidx(t, leaf, i)];
    m.latent = cur;
    m.to_play = to_play;
    t.meta[nidx(t, leaf, i)] = m;
    t.stat[nidx(t, leaf, i)].reward = reward;
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
}

// R roots per workgroup; TL: the tree slice (node records, pUCT table, root legal lists) is staged in LDS.
template <int R, bool TL>
__global__ __launch_bounds__(kThreads) void search_stoch_mlp_kernel(StochSearchArgs p) {
  extern __shared__ float4 smem4[];
  float *smem = reinterpret_cast<float *>(smem4);
  const int tid = threadIdx.x, g = blockIdx.x;
  const int B = p.B, W = p.W, H = p.H;
  const int i0 = g * R;
  const int nr = min(R, B - i0);  // roots in this slice

  __shared__ int s_players;
  __shared__ int s_x[R], s_act[R], s_len[R], s_vtp[R], s_lvtp[R];
  __shared__ float s_r[R], s_v[R], s_kr[R], s_kv[R];  // a pass's decoded reward / value; the kept ones of each row's kind
  __shared__ float4 s_mm[R];
  __shared__ float s_red[3 * kWaves * R];

  // ---- stage the tree slice and per-root state
  TreeView t;
  t.A = W;
  t.cap = p.cap;
  t.lut_n = p.lut_n;
  t.depth_cap = p.depth_cap;
  t.path = reinterpret_cast<int32_t *>(smem + p.off_path);
  t.path_act = reinterpret_cast<int32_t *>(smem + p.off_pact);
  t.pathlen = s_len;
  if constexpr (TL) {
    NodeStat *ls = reinterpret_cast<NodeStat *>(smem + p.off_stat);
    NodeMeta *lm = reinterpret_cast<NodeMeta *>(smem + p.off_meta);
    float2 *llut = reinterpret_cast<float2 *>(smem + p.off_lut);
    int32_t *llegal = reinterpret_cast<int32_t *>(smem + p.off_legal);
    for (int e = tid; e < p.cap * R; e += kThreads) {
      const int node = e / R, li = e % R;
      if (li < nr) {
        ls[e] = p.stat[(size_t)node * B + i0 + li];
        lm[e] = p.meta[(size_t)node * B + i0 + li];
      }
    }
    for (int e = tid; e < p.lut_n; e += kThreads) llut[e] = p.lut[e];
    for (int e = tid; e < R * W; e += kThreads) llegal[e] = (e / W < nr) ? p.legal[(size_t)i0 * W + e] : 0;
    for (int e = tid; e < R; e += kThreads) llegal[R * W + e] = (e < nr) ? p.nlegal[i0 + e] : 0;
    t.stat = ls;
    t.meta = lm;
    t.lut = llut;
    t.legal = llegal;
    t.nlegal = llegal + R * W;
    t.B = R;
  } else {
    t.stat = p.stat;
    t.meta = p.meta;
    t.lut = p.lut;
    t.legal = p.legal;
    t.nlegal = p.nlegal;
    t.B = B;
  }
  // tree index of local root li: li in the LDS slice, i0 + li in the HBM batch
  auto tix = [i0](int li) { return TL ? li : i0 + li; };
  StochasticView sv;
  sv.A = p.A;
  sv.C = p.C;
  sv.is_chance = nullptr;  // (the walk never reads it: the kind is the depth's parity)
  if (tid < nr) {
    s_mm[tid] = p.minmax[i0 + tid];
    s_vtp[tid] = p.vtp_in[i0 + tid];
  }
  if (tid < 64) {
    // players (cnode.cpp:732-737) over the whole batch by wave 0
    int m = INT_MIN;
    for (int q = tid; q < B; q += 64) m = max(m, p.vtp_in[q]);
    m = xor_max(m);
    if (tid == 0) s_players = (m == -1) ? 1 : 2;
  }
  uint32_t *s_seeds = reinterpret_cast<uint32_t *>(smem + p.off_seeds);
  for (int e = tid; e < p.S; e += kThreads) s_seeds[e] = p.seeds[e];
  __syncthreads();
  const int players = s_players;

  float *X0 = smem + p.off_x0, *X1 = smem + p.off_x1, *NL = smem + p.off_n, *LG = smem + p.off_logit;
  float *KEEP = smem + p.off_keep;  // [R][kMaxActions]: each row's logits from the pass of its kind
  // weight prefetch buffers: A serves a schedule's even steps, B its odd ones (lzm_search_mlp.h)
  constexpr int PA = pre_a<R>(), PB = pre_b<R>();
  float wA[PA * kKC], bA = 0.0f, wB[PB * kKC], bB = 0.0f;

  for (int k = 0; k < p.S; ++k) {
    const uint32_t seed = s_seeds[k];
    // ---- selection: wave w walks roots w, w + kWaves, ... (the root index in a scalar register)
    for (int li = __builtin_amdgcn_readfirstlane(tid >> 6); li < nr; li += kWaves) {
      const Descent d = stochastic_walk_at(t, sv, tix(li), li, R, i0 + li, s_mm[li], players, s_vtp[li], p.disc, seed);
      if ((tid & 63) == 0) { s_len[li] = d.len; s_x[li] = d.x; s_act[li] = d.action; s_lvtp[li] = d.vtp; }
    }
    __syncthreads();
    // ---- which branches this workgroup runs: one pass per kind present among its rows
    int has_chance = 0, has_decision = 0;
    for (int r = 0; r < nr; ++r) {
      if (s_len[r] & 1) has_chance = 1; else has_decision = 1;
    }
    has_chance = __builtin_amdgcn_readfirstlane(has_chance);
    has_decision = __builtin_amdgcn_readfirstlane(has_decision);
    const int first = has_chance ? 0 : 1, npass = has_chance + has_decision;
    // the first pass's first two steps, now that the branch is known
    prefetch_step<PA>(p.sched[first * kStochSteps], wA, bA);
    prefetch_step<PB>(p.sched[first * kStochSteps + 1], wB, bB);
    if (p.rec_x && tid < nr) {
      const size_t o = (size_t)k * B + i0 + tid;
      p.rec_x[o] = s_x[tid]; p.rec_a[o] = s_act[tid]; p.rec_len[o] = s_len[tid];
      p.rec_chance[o] = s_len[tid] & 1; p.rec_vtp[o] = s_lvtp[tid];
    }
    // ---- gather leaf latents (both passes read them): X0[h][r] = pool[x_r][i0 + r][h]
    for (int e = tid; e < H * R; e += kThreads) {
      const int r = e / H, h = e % H;
      float v = 0.0f;
      if (r < nr) v = p.pool[((size_t)max(s_x[r], 0) * B + i0 + r) * H + h];
      X0[tpos<R>(h, r)] = v;
    }
    for (int ps = 0; ps < npass; ++ps) {
      const int b = ps == 0 ? first : 1;  // (a second pass is always the decision branch)
      const int base = b * kStochSteps, n = p.nsteps[b];
      const int width = b == 0 ? p.C : p.A;  // the branch's policy row
      // one-hot option rows H .. K0 of the branch's first layer: an action for a chance leaf, an outcome for a
      // decision leaf, clamped into range for the rows of the other kind
      const int nopt = b == 0 ? p.A : p.C;
      for (int e = tid; e < (p.sched[base].K - H) * R; e += kThreads) {
        const int a = e / R, r = e % R;
        X0[tpos<R>(H + a, r)] = (r < nr && min(max(s_act[r], 0), nopt - 1) == a) ? 1.0f : 0.0f;
      }
      __syncthreads();
      // ---- the branch's network (BN folded): dynamics, [reward head,] prediction common, merged heads
#define LZM_STOCH_STEP(ST, WBUF, BIAS, P)                                                              \
  do {                                                                                                 \
    const int st_ = (ST);                                                                              \
    const StepRec &q = p.sched[base + st_];                                                            \
    const int nx = st_ + 2 < n ? base + st_ + 2 : (ps + 1 < npass ? kStochSteps + st_ + 2 - n : kStochIdle); \
    float *dec = q.decode == 1 ? s_r : s_v;                                                            \
    dense_step<R, P>(q, smem, WBUF, BIAS, s_red, dec, nr, p.sched[nx]);                                \
    __syncthreads();                                                                                   \
    if (q.decode && q.splits) { /* narrow support (< kThreads): logits in LG, one wave per row */      \
      for (int r = tid >> 6; r < nr; r += kWaves) {                                                    \
        const float e = wave_expect_lds(LG + r * (p.V + 1), p.V);                                      \
        if ((tid & 63) == 0) dec[r] = h_inverse(e);                                                    \
      }                                                                                                \
      __syncthreads();                                                                                 \
    }                                                                                                  \
  } while (0)
      for (int st = 0; st < n; st += 2) {
        LZM_STOCH_STEP(st, wA, bA, PA);
        LZM_STOCH_STEP(st + 1, wB, bB, PB);
      }
#undef LZM_STOCH_STEP
      // ---- harvest the rows of this pass's kind: the next latent into pool[k + 1], logits / value / reward kept
      for (int e = tid; e < H * R; e += kThreads) {
        const int r = e / H, h = e % H;
        if (r < nr && (s_len[r] & 1) == 1 - b) p.pool[((size_t)(k + 1) * B + i0 + r) * H + h] = NL[tpos<R>(h, r)];
      }
      for (int e = tid; e < R * kMaxActions; e += kThreads) {
        const int r = e / kMaxActions, j = e % kMaxActions;
        if (r < nr && (s_len[r] & 1) == 1 - b) KEEP[e] = j < width ? X1[r * width + j] : 0.0f;
      }
      if (tid < nr && (s_len[tid] & 1) == 1 - b) {
        s_kv[tid] = s_v[tid];
        s_kr[tid] = b == 1 ? s_r[tid] : 0.0f;  // a chance node's reward is 0 (:118)
      }
      __syncthreads();
    }
    if (p.rec_dec && tid < nr) {
      const size_t o = (size_t)k * B + i0 + tid;
      p.rec_dec[o * 2] = s_kr[tid];
      p.rec_dec[o * 2 + 1] = s_kv[tid];
      for (int a = 0; a < W; ++a) p.rec_logits[o * W + a] = KEEP[tid * kMaxActions + a];
    }
    // ---- expand + backup (cbatch_backpropagate :559-592): wave w takes root w with the child count of its kind
    for (int li = tid >> 6; li < nr; li += kWaves) {
      const int ti = tix(li);
      const int len = s_len[li];
      const int leaf = t.path[len * R + li];
      stochastic_expand_wave(t, ti, leaf, s_lvtp[li], k + 1, s_kr[li], KEEP + li * kMaxActions,
                             (len & 1) ? p.C : p.A);
      backup_wave(t, ti, li, R, &s_mm[li], s_lvtp[li], s_kv[li], p.disc);
    }
    __syncthreads();
  }
  // ---- write back the slice (tree, min-max, last paths and kinds)
  if constexpr (TL) {
    for (int e = tid; e < p.cap * R; e += kThreads) {
      const int node = e / R, li = e % R;
      if (li < nr) {
        p.stat[(size_t)node * B + i0 + li] = t.stat[e];
        p.meta[(size_t)node * B + i0 + li] = t.meta[e];
      }
    }
  }
  for (int e = tid; e < p.depth_cap * R; e += kThreads) {
    const int l = e / R, li = e % R;
    if (li < nr) {
      p.path[(size_t)l * B + i0 + li] = t.path[e];
      p.path_act[(size_t)l * B + i0 + li] = t.path_act[e];
    }
  }
  if (tid < nr) {
    p.minmax[i0 + tid] = s_mm[tid];
    p.pathlen[i0 + tid] = s_len[tid];
    p.is_chance[i0 + tid] = s_len[tid] & 1;
  }
}

// The launch (lzm_search_stoch_mlp.hip, a translation unit of its own: lightzero_amd/build.py): R = 1, 2, 4 or 8
// roots per workgroup, the tree slice in LDS or not, `lds` bytes of dynamic LDS.
hipError_t stoch_mlp_launch(const StochSearchArgs &p, int R, bool tree_in_lds, size_t lds, hipStream_t stream);

}  // namespace lzm
