// lzm_search_sampled_mlp.h — one launch = one whole Sampled EfficientZero search (all simulations) for the
// continuous SampledEfficientZeroModelMLP (lzero/model/sampled_efficientzero_model_mlp.py;
// SampledEfficientZeroMCTSCtree.search, mcts_ctree_sampled.py:133-232).
//
// Decomposition: search_mlp_kernel's (lzm_search_mlp.h). Workgroup g owns roots [g R, g R + R) for all S
// simulations: its tree slice [cap][R] staged in LDS for the whole search (or left in HBM when it does not fit), one
// wave per root for the walk (sampled_walk_at, lzm_sampled.h), the expansion and the backup, all 512 lanes for the
// network over the workgroup's R rows (dense_step: f32 FMAs over weights streamed from L2 in lane order). Roots
// exchange nothing: every draw is a Philox function of (seed, root, node, slot), so there is no look-back, no flag
// and no spin.
//
// What is new against the EfficientZero instantiation of search_mlp_kernel:
//   * the dynamics input row is [latent ; action] with the action as D floats: the walking wave's last read — the
//     chosen slot's D floats in the per-handle action table (HBM) — is stored straight into rows H .. H + D of the
//     transposed input X0[k][r]; rows H + D .. K0 are zeroed once and never written again. No one-hot, no clamp.
//   * the prediction tail has three heads: [fc_value_head[0] | main[0]] (one step over the common output),
//     main[1] (on the policy half), [fc_value_head[1] | mu | log_sigma] (value columns read the value half and are
//     decoded; the 2 D policy columns read main[1]'s output and land row-major in POL[r][2 D]). A pass over the
//     R x 2 D raw entries then makes the row the tree's: mu (tanhf when bound_type is 'tanh'), sigma =
//     glibc_expf(clamp(log_sigma, -20, 2)).
//   * the owning wave expands the leaf from that LDS row: sampled_expand_at draws the K x D Gaussians (Philox,
//     Box-Muller and tanh in double: lzm_sampled.h's draws, unchanged) into the action table, then backup_wave_ez.
//     The double-precision log / cos / sin / tanh live in this phase only.
//
// The action table stays in HBM: at K = 20, S = 50, D = 4, R = 4 a slice would be 65 KB beside the gates, and only
// the owning wave writes (expand) and reads (the next walks' last read) it — one D-float access per simulation on
// the read side, which the latent gather's round trip covers.
#pragma once
#include "lzm_sampled.h"
#include "lzm_search_mlp.h"

namespace lzm {

constexpr int kSampledSteps = 14;  // schedule steps at most (12 with residual dynamics; even, see build below)

struct SampledSearchArgs {
  // tree (HBM, whole batch); K: the child-block width
  NodeStat *stat;
  NodeMeta *meta;
  int32_t *path, *path_act, *pathlen;
  const float2 *lut;
  float *act_f;  // the handle's action table [(reserved simulations + 1) * K][B][D]
  int B, K, D, cap, lut_n, depth_cap;
  // search
  int S;
  float disc;
  const uint32_t *seeds;  // [S]: seeds[k] keys simulation k's tie draws and its leaf's sampling
  const int32_t *vtp_in;  // [B]
  float4 *minmax;         // [B]
  float *pool;            // [S + 1][B][H]
  float *hpool, *cpool;   // [S + 1][B][Hl], slot 0 = the roots' state
  int H, Hl, V, horizon, cell_after, tanh_mu;
  // optional per-simulation record, may be null (all or none): [S][B] each, rec_dec [S][B][2], rec_policy
  // [S][B][2 D] (the row the tree was given), rec_actions [S][B][D] (the rows the network was fed)
  int32_t *rec_x, *rec_slot, *rec_len, *rec_reset;
  float *rec_dec, *rec_policy, *rec_actions;
  // network schedule (host-built; an even number of steps)
  StepRec sched[kSampledSteps];
  int nsteps;
  // dynamic LDS layout (float offsets); [off_act, off_act + act_floats): the activation buffers, zeroed once
  size_t off_stat, off_meta, off_lut, off_path, off_pact, off_act, act_floats, off_x0, off_n, off_logit, off_pol,
      off_seeds, off_g, off_gates, off_hh, off_cp;
};

// R roots per workgroup (1, 2 or 4: the gate rows of 8 would not leave the tree its LDS); TL: the tree slice (node
// records, pb_c table) is staged in LDS.
template <int R, bool TL>
__global__ __launch_bounds__(kThreads) void search_sampled_mlp_kernel(SampledSearchArgs p) {
  extern __shared__ float4 smem4[];
  float *smem = reinterpret_cast<float *>(smem4);
  const int tid = threadIdx.x, g = blockIdx.x;
  const int B = p.B, H = p.H, D = p.D, K = p.K;
  const int i0 = g * R;
  const int nr = min(R, B - i0);  // roots in this slice

  __shared__ int s_players;
  __shared__ int s_x[R], s_slot[R], s_len[R], s_vtp[R], s_lvtp[R];
  __shared__ float s_r[R], s_v[R];
  __shared__ float4 s_mm[R];
  __shared__ float s_red[3 * kWaves * R];

  // ---- stage the tree slice and per-root state
  TreeView t;
  t.A = K;
  t.cap = p.cap;
  t.lut_n = p.lut_n;
  t.depth_cap = p.depth_cap;
  t.legal = nullptr;  // (a sampled node's children are its K slots: no legal list is read)
  t.nlegal = nullptr;
  t.path = reinterpret_cast<int32_t *>(smem + p.off_path);
  t.path_act = reinterpret_cast<int32_t *>(smem + p.off_pact);
  t.pathlen = s_len;
  if constexpr (TL) {
    NodeStat *ls = reinterpret_cast<NodeStat *>(smem + p.off_stat);
    NodeMeta *lm = reinterpret_cast<NodeMeta *>(smem + p.off_meta);
    float2 *llut = reinterpret_cast<float2 *>(smem + p.off_lut);
    for (int e = tid; e < p.cap * R; e += kThreads) {
      const int node = e / R, li = e % R;
      if (li < nr) {
        ls[e] = p.stat[(size_t)node * B + i0 + li];
        lm[e] = p.meta[(size_t)node * B + i0 + li];
      }
    }
    for (int e = tid; e < p.lut_n; e += kThreads) llut[e] = p.lut[e];
    t.stat = ls;
    t.meta = lm;
    t.lut = llut;
    t.B = R;
  } else {
    t.stat = p.stat;
    t.meta = p.meta;
    t.lut = p.lut;
    t.B = B;
  }
  // tree index of local root li: li in the LDS slice, i0 + li in the HBM batch
  auto tix = [i0](int li) { return TL ? li : i0 + li; };
  SampledView sv;
  sv.K = K;
  sv.D = D;
  sv.A = 0;
  sv.act_f = p.act_f;
  sv.act_i = nullptr;
  if (tid < nr) {
    s_mm[tid] = p.minmax[i0 + tid];
    s_vtp[tid] = p.vtp_in[i0 + tid];
  }
  if (tid < 64) {
    // players (cnode.cpp:1138-1143) over the whole batch by wave 0
    int m = INT_MIN;
    for (int q = tid; q < B; q += 64) m = max(m, p.vtp_in[q]);
    m = xor_max(m);
    if (tid == 0) s_players = (m == -1) ? 1 : 2;
  }
  uint32_t *s_seeds = reinterpret_cast<uint32_t *>(smem + p.off_seeds);
  for (int e = tid; e < p.S; e += kThreads) s_seeds[e] = p.seeds[e];
  // the activation buffers start as zeros: the pad rows of X0 past [latent ; action], the rows of absent roots and
  // the K padding of the merged head output's narrower source stay zero for the whole search
  for (size_t e = tid; e < p.act_floats; e += kThreads) smem[p.off_act + e] = 0.0f;
  __syncthreads();
  const int players = s_players;

  float *X0 = smem + p.off_x0, *NL = smem + p.off_n, *LG = smem + p.off_logit, *POL = smem + p.off_pol;
  // weight prefetch buffers: A serves the schedule's even steps, B its odd ones (lzm_search_mlp.h)
  constexpr int PA = pre_a<R>(), PB = pre_b<R>();
  float wA[PA * kKC], bA = 0.0f, wB[PB * kKC], bB = 0.0f;
  prefetch_step<PA>(p.sched[0], wA, bA);
  prefetch_step<PB>(p.sched[1], wB, bB);

  for (int k = 0; k < p.S; ++k) {
    const uint32_t seed = s_seeds[k];
    // ---- selection: wave w walks roots w, w + kWaves, ... (the root index in a scalar register); the walk's last
    // read, the chosen slot's D floats, goes into the tail of the root's [latent ; action] row
    for (int li = __builtin_amdgcn_readfirstlane(tid >> 6); li < nr; li += kWaves) {
      const Descent d = sampled_walk_at(t, K, tix(li), li, R, i0 + li, s_mm[li], players, s_vtp[li], p.disc, seed);
      const int lane = tid & 63;
      if (lane < D && d.len > 0)
        X0[tpos<R>(H + lane, li)] = p.act_f[(((size_t)d.x * K + d.action) * B + i0 + li) * D + lane];
      if (lane == 0) { s_len[li] = d.len; s_x[li] = d.x; s_slot[li] = d.action; s_lvtp[li] = d.vtp; }
    }
    __syncthreads();
    if (p.rec_x) {
      if (tid < nr) {
        const size_t o = (size_t)k * B + i0 + tid;
        p.rec_x[o] = s_x[tid]; p.rec_slot[o] = s_slot[tid]; p.rec_len[o] = s_len[tid];
        p.rec_reset[o] = (s_len[tid] % p.horizon) == 0 ? 1 : 0;
      }
      if (tid < nr * D) {
        const int r = tid / D, d = tid % D;
        p.rec_actions[((size_t)k * B + i0 + r) * D + d] = X0[tpos<R>(H + d, r)];
      }
    }
    // ---- gather leaf latents: X0[h][r] = pool[x_r][i0 + r][h], and the leaf's LSTM state (mcts_ctree_sampled.py:
    // 170-186): h_prev as rows H .. H + Hl of the gate layer's input, c_prev for the cell
    for (int e = tid; e < H * R; e += kThreads) {
      const int r = e / H, h = e % H;
      float v = 0.0f;
      if (r < nr) v = p.pool[((size_t)max(s_x[r], 0) * B + i0 + r) * H + h];
      X0[tpos<R>(h, r)] = v;
    }
    {
      float *GH = smem + p.off_g, *CP = smem + p.off_cp;
      for (int e = tid; e < p.Hl * R; e += kThreads) {
        const int r = e / p.Hl, u = e % p.Hl;
        float hv = 0.0f, cv = 0.0f;
        if (r < nr) {
          const size_t o = ((size_t)max(s_x[r], 0) * B + i0 + r) * p.Hl + u;
          hv = p.hpool[o];
          cv = p.cpool[o];
        }
        GH[tpos<R>(H + u, r)] = hv;
        CP[e] = cv;
      }
    }
    __syncthreads();
    // ---- network (recurrent_inference, BN folded): dynamics on [latent ; action] (+ latent residual,
    // fc_dynamics_2), the gate layer on [x ; h_prev] and the cell, the value-prefix head on h1 (decoded into s_r),
    // fc_prediction_common, the three-headed tail (value decoded into s_v, {mu, log_sigma} into POL)
#define LZM_SAMPLED_STEP(ST, WBUF, BIAS, P)                                                          \
  do {                                                                                               \
    const int st_ = (ST);                                                                            \
    const StepRec &q = p.sched[st_];                                                                 \
    const int nx = st_ + 2 < p.nsteps ? st_ + 2 : st_ + 2 - p.nsteps;                                \
    float *dec = q.decode == 1 ? s_r : s_v;                                                          \
    dense_step<R, P, true>(q, smem, WBUF, BIAS, s_red, dec, nr, p.sched[nx]);                        \
    __syncthreads();                                                                                 \
    if (q.decode && q.splits) { /* narrow support (< kThreads): logits in LG, one wave per row */    \
      for (int r = tid >> 6; r < nr; r += kWaves) {                                                  \
        const float e = wave_expect_lds(LG + r * (p.V + 1), p.V);                                    \
        if ((tid & 63) == 0) dec[r] = h_inverse(e);                                                  \
      }                                                                                              \
      __syncthreads();                                                                               \
    }                                                                                                \
    if (st_ == p.cell_after) { /* the gates are in LDS: the cell, h1 for the value-prefix head */    \
      ez_cell<R>(p, smem, k, i0, nr, s_len);                                                         \
      __syncthreads();                                                                               \
    }                                                                                                \
  } while (0)
    for (int st = 0; st < p.nsteps; st += 2) {
      LZM_SAMPLED_STEP(st, wA, bA, PA);
      LZM_SAMPLED_STEP(st + 1, wB, bB, PB);
    }
#undef LZM_SAMPLED_STEP
    // ---- the policy row as the tree reads it, {mu[D], sigma[D]} (ReparameterizationHead: mu, tanh-bounded or not;
    // sigma = exp(clamp(log_sigma, -20, 2))), and the new latents into pool[k + 1]
    for (int e = tid; e < nr * 2 * D; e += kThreads) {
      const float v = POL[e];
      POL[e] = (e % (2 * D)) < D ? (p.tanh_mu ? tanhf(v) : v) : glibc_expf(fminf(fmaxf(v, -20.0f), 2.0f));
    }
    for (int e = tid; e < H * R; e += kThreads) {
      const int r = e / H, h = e % H;
      if (r < nr) p.pool[((size_t)(k + 1) * B + i0 + r) * H + h] = NL[tpos<R>(h, r)];
    }
    __syncthreads();
    if (p.rec_dec) {
      if (tid < nr) {
        p.rec_dec[((size_t)k * B + i0 + tid) * 2] = s_r[tid];
        p.rec_dec[((size_t)k * B + i0 + tid) * 2 + 1] = s_v[tid];
      }
      for (int e = tid; e < nr * 2 * D; e += kThreads) p.rec_policy[((size_t)k * B + i0) * 2 * D + e] = POL[e];
    }
    // ---- expand + backup (cbatch_backpropagate :947-971): wave w takes root w — K fresh slots, their K x D
    // Gaussians under the simulation's seed into the action table, is_reset, the value-prefix backup
    for (int li = __builtin_amdgcn_readfirstlane(tid >> 6); li < nr; li += kWaves) {
      const int ti = tix(li);
      const int len = s_len[li];
      const int leaf = t.path[len * R + li];
      sampled_expand_at<true>(t, sv, ti, i0 + li, B, leaf, s_lvtp[li], k + 1, s_r[li], POL + li * 2 * D,
                              (len % p.horizon) == 0 ? 1 : 0, seed);
      backup_wave_ez(t, ti, li, R, &s_mm[li], s_lvtp[li], s_v[li], p.disc);
    }
    __syncthreads();
  }
  // ---- write back the slice (tree, min-max, last paths)
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
  }
}

// The launch (lzm_search_sampled_mlp.hip, a translation unit of its own: lightzero_amd/build.py): R = 1, 2 or 4
// roots per workgroup, the tree slice in LDS or not, `lds` bytes of dynamic LDS.
hipError_t sampled_mlp_launch(const SampledSearchArgs &p, int R, bool tree_in_lds, size_t lds, hipStream_t stream);

}  // namespace lzm
