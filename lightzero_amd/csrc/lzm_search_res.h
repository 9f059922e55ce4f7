// lzm_search_res.h — the fused MuZero search with the network resident on the CU (CartPole shape).
//
// Same contract as search_mlp_kernel (lzm_search_mlp.h: one launch = every simulation of a
// MuZeroMCTSCtree.search, mcts_ctree.py:255-321), specialised to the MuZeroModelMLP shape of
// BASELINE.json config 2 — latent 128, head hidden 32, reward/value supports 601,
// res_connection_in_dynamics (muzero_model_mlp.py:179-204, :327-440; common.py:883-971) — with one
// root per workgroup. What changes is where the 149 K weights live. search_mlp_kernel streams all
// of them from L2 every simulation (≈0.6 MiB per CU per simulation, which its phase stamps show
// as the largest cost). Here a 256-thread workgroup (one wave per SIMD, so up to ≈450 registers
// per lane) keeps them on the CU for the whole launch:
//   registers: fc_dynamics_2[1], fc_prediction_common[0..1], the reward / value / policy head
//              hiddens and the policy output                                  (≈245 floats/lane)
//   LDS:       fc_dynamics[1], fc_dynamics_2[0]                                (2 x 64 KiB)
//   streamed:  fc_dynamics[0] (latent rows) and the two 32 -> 601 support heads, ≈0.2 MiB per
//              simulation, each prefetched into one 80-register buffer several steps (or, for
//              the first layer, a whole tree phase) ahead of its use.
// Every 128 x 128 layer uses one lane mapping (the D-block lane map below). The one-hot action rows
// of fc_dynamics[0] are never multiplied: the action's row is added after the latent rows (the exact
// value of the one-hot product), so the layer can start before the action is known.
//
// Tree phase (R = 1): every thread computes the expanded nodes' walk-independent pUCT terms, then
// wave 0 walks the tree over them (descend_terms / descend_a2f / descend_a2r: descend_wave's float
// operations in the same order, so bit-exact with the reference). In parity
// mode the reference's single rand() stream makes root i's draws start at the sum of the
// depths of roots < i; every workgroup publishes its depth at once (lzm_search_mlp.h, decoupled
// look-back), but only a root whose walk stopped at a tie among unexpanded children needs the
// draw VALUE — and that tie leaves the leaf's parent (the gathered latent) known, only the action
// open. So the look-back wait is deferred behind the first layer's latent rows and skipped
// entirely when no draw value is needed. A tie reaching an expanded child (depth depends on the
// draw) is resolved by wave 0 after its look-back, which resumes the walk at the tie. The register
// walk (mode 5) hands its outcome to the workgroup as one word (hand_pack): the tie's candidates,
// the pick and wave 0's expand + backup (expand_wave_r, backup_wave_r) are arithmetic on its fields.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "lzm_search_mlp.h"
#include "lzm_tree.h"

namespace lzm {

constexpr int kRT = 256;  // threads: one wave per SIMD
constexpr int kRWaves = kRT / 64;
constexpr int kRHid = 128, kRF = 32, kRV = 601;
constexpr int kRMaxA = 32;                 // policy output: 8 lanes per action
constexpr int kRTail = kRV - 2 * kRT;      // support columns past two full lane rounds (89)
static_assert(kRTail > 0 && 2 * kRTail <= kRT, "support tail: two lanes per column");
// float4 slots (each kRT lanes wide) per resident block
constexpr int kRSlotsD = 16, kRSlotsRH = 4, kRSlotsVPH = 8, kRSlotsS = 20, kRSlotsPO = 1;

// D-block lane map (every 128 x 128 layer): lane l owns the four columns 4 (l >> 3) .. +3 over the K
// eighth 16 (l & 7) .. +15, so it reads 4 activation float4 per row (all in flight at once) and uses
// each for 4 columns; the 8 lanes of a column group meet by a 3-step DPP butterfly that leaves column
// 4 (l >> 3) + ((l & 7) >> 1) in lane pair (l, l ^ 1) (reduce_d4).
//
// The draw window (parity mode, A = 2): a tie between visited children (status 2/3: the walk's
// remaining levels need draws, the zero-init-heads regime at nearly every simulation) waits for its
// look-back with wave 0 alone (lookback_sum_w0) while waves 1-3 compute the window of draws around the
// previous look-back base, so the resumed walk reads its draws from LDS instead of a coefficient-row
// round trip per lane after the wait (positions outside the window: the rows).
constexpr int kDwinBack = 20;  // draw window [base_prev - kDwinBack, base_prev - kDwinBack + 64)

// Part `part` (0..2: coefficient words 11 part .. 11 part + 10) of the window's 64 dot products, added
// to win (the sums are mod 2^32, so the three waves' LDS adds may land in any order); win must be zero
// before the first add and holds (sum) before the >> 1 of the draw. Eleven loads per lane.
__device__ __forceinline__ void dwin_add_part(const uint32_t *coef, int npos, const uint32_t *z0, int lo, uint32_t *win,
                                              int part) {
  const int lane = threadIdx.x & 63;
  const int q = lo + lane;
  const int j0 = 11 * part, j1 = part == 2 ? 31 : j0 + 11;
  if (q < npos) {
    const uint32_t *c = coef + (size_t)q * 31;
    uint32_t v = 0;
#pragma unroll
    for (int j = 0; j < 11; ++j)
      if (j0 + j < j1) v += c[j0 + j] * z0[j0 + j];
    __hip_atomic_fetch_add(win + lane, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// The draw of this lane's level lo + lane of a resumed walk from the window win[0..64) of stream
// positions dlo..; *miss when a level below hi lies outside it.
__device__ __forceinline__ uint32_t window_draw(int npos, int base, int lo, int hi, const uint32_t *win, int dlo,
                                                bool *miss) {
  const int lane = threadIdx.x & 63;
  const int q = base + lo + lane, o = q - dlo;
  *miss = false;
  if (lo + lane >= hi || q >= npos) return 0u;
  if (o >= 0 && o < 64) return win[o] >> 1;
  *miss = true;
  return 0u;
}

// Resident weight layout (lzm_mlp_prepare writes it after the generic kernel layout; res_source
// below is its definition). Every block is [slot][lane] float4, so a wave-instruction of a block
// is one contiguous 1 KiB read.
//   D (128 x 128, six of them): slot j, lane l: W[16 (l & 7) + 4 (j >> 2) .. +3][4 (l >> 3) + (j & 3)]
//   RH (128 -> 32 reward head hidden): slot j < 4: W[16 (l & 7) + 4 j ..][l >> 3]
//   VPH (128 -> 64: [value hidden | policy hidden]): slot j < 8: W[32 (l & 3) + 4 j ..][l >> 2]
//   S (32 -> 601 support head): slots 0-7: column l, k = 4 j; slots 8-15: column 256 + l;
//      slots 16-19: column 512 + (l >> 1), k = 16 (l & 1) + 4 (j - 16), lanes < 2 * kRTail
//   PO (32 -> A policy output): one slot: W[4 (l & 7) ..][l >> 3], l >> 3 < A
// then the biases ([6][128] D, [32] RH, [64] VPH, [604] RS, [604] VS, [32] PO) and the one-hot
// action rows of fc_dynamics[0], [A][128].
// dynamic LDS plan of the resident kernel (float offsets; res_plan below)
struct ResPlan {
  int wd1, wd2, stat, meta, lut, legal, val, path, pact, act, l2n, nq, cs, dec, misc, pbt, pbt_rows, floats;
};
struct ResNet {
  // the resident layout (one base pointer: every block offset but the action rows' is a
  // compile-time constant, res_block_offset; the kernel derives the block addresses, which keeps
  // ~30 scalar registers of block pointers out of the simulation loop)
  const float *w;
  // LDS float offsets beyond SearchArgs' tree plan
  ResPlan plan;      // dynamic LDS plan (res_plan)
  int late_draw;    // two-way leaf ties run the dynamics layers for both candidates before the
                    // look-back wait (LZM_RES_LATE, default 1)
  int spec_depth;   // status-2 ties: publish the depth early when every draw outcome gives the same
                    // depth (speculate_depth_a2; LZM_RES_SPEC_DEPTH, default 1)
};

// floats of the bias blocks ([6][128] D, [32] RH, [64] VPH, [604] RS, [604] VS, [32] PO)
constexpr int kResBiasFloats = 6 * 128 + 32 + 64 + 2 * 604 + 32;
enum ResBlock { kRbD = 0, kRbRH = 6, kRbVPH, kRbRS, kRbVS, kRbPO, kRbBD, kRbBRH, kRbBVPH, kRbBRS, kRbBVS, kRbBPO, kRbAct, kRbN };

// float count of each block (A actions)
__host__ __device__ inline size_t res_block_floats(int b, int A) {
  if (b < kRbRH) return (size_t)kRSlotsD * kRT * 4;
  switch (b) {
    case kRbRH: return (size_t)kRSlotsRH * kRT * 4;
    case kRbVPH: return (size_t)kRSlotsVPH * kRT * 4;
    case kRbRS: case kRbVS: return (size_t)kRSlotsS * kRT * 4;
    case kRbPO: return (size_t)kRSlotsPO * kRT * 4;
    case kRbBD: return 6 * kRHid;
    case kRbBRH: return kRF;
    case kRbBVPH: return 2 * kRF;
    case kRbBRS: case kRbBVS: return (kRV + 3) & ~3;
    case kRbBPO: return kRMaxA;
    default: return (size_t)A * kRHid;
  }
}
__host__ __device__ inline size_t res_block_offset(int b, int A) {
  size_t o = 0;
  for (int q = 0; q < b; ++q) o += res_block_floats(q, A);
  return o;
}

// block b of the resident layout (b < kRbAct: a compile-time offset)
__device__ __forceinline__ const float4 *res_blk4(const ResNet &n, int b) {
  return reinterpret_cast<const float4 *>(n.w + res_block_offset(b, 0));
}
__device__ __forceinline__ const float *res_blk(const ResNet &n, int b, int A) { return n.w + res_block_offset(b, A); }

// Packed-network source of resident float d of block b: packed layer index (lzm_kernels.hip
// mlp_net order without the gate layer's slot: 0,1 fc_dynamics, 2,3 fc_dynamics_2, 4,5 reward head, 6,7 prediction common,
// 8,9 value head, 10,11 policy head), row k (k < 0: the bias) and column; layer < 0: zero padding.
__host__ __device__ inline void res_source(int b, size_t d, int A, int *layer, int *k, int *col) {
  *layer = -1; *k = 0; *col = 0;
  const int e = (int)(d & 3);
  const int f4 = (int)(d >> 2);
  const int j = f4 / kRT, l = f4 % kRT;
  if (b < kRbRH) {
    const int src[6] = {0, 1, 2, 3, 6, 7};
    *layer = src[b];
    *col = 4 * (l >> 3) + (j & 3); *k = 16 * (l & 7) + 4 * (j >> 2) + e;
    return;
  }
  switch (b) {
    case kRbRH: *layer = 4; *col = l >> 3; *k = 16 * (l & 7) + 4 * j + e; return;
    case kRbVPH: {
      const int c = l >> 2;
      *layer = c < kRF ? 8 : 10; *col = c < kRF ? c : c - kRF; *k = 32 * (l & 3) + 4 * j + e;
      return;
    }
    case kRbRS: case kRbVS: {
      const int ly = b == kRbRS ? 5 : 9;
      if (j < 8) { *layer = ly; *col = l; *k = 4 * j + e; }
      else if (j < 16) { *layer = ly; *col = kRT + l; *k = 4 * (j - 8) + e; }
      else if (l < 2 * kRTail) { *layer = ly; *col = 2 * kRT + (l >> 1); *k = 16 * (l & 1) + 4 * (j - 16) + e; }
      return;
    }
    case kRbPO: if ((l >> 3) < A) { *layer = 11; *col = l >> 3; *k = 4 * (l & 7) + e; } return;
    case kRbBD: {
      const int src[6] = {0, 1, 2, 3, 6, 7};
      *layer = src[d / kRHid]; *k = -1; *col = (int)(d % kRHid);
      return;
    }
    case kRbBRH: *layer = 4; *k = -1; *col = (int)d; return;
    case kRbBVPH: *layer = d < (size_t)kRF ? 8 : 10; *k = -1; *col = (int)(d % kRF); return;
    case kRbBRS: case kRbBVS: if (d < (size_t)kRV) { *layer = b == kRbBRS ? 5 : 9; *k = -1; *col = (int)d; } return;
    case kRbBPO: if (d < (size_t)A) { *layer = 11; *k = -1; *col = (int)d; } return;
    default: *layer = 0; *k = kRHid + (int)(d / kRHid); *col = (int)(d % kRHid); return;
  }
}

// NS float4 slots of a resident block into registers (buffer loads: the slot offset is scalar)
template <int NS, int J0 = 0, int J1 = NS>
__device__ __forceinline__ void res_fetch(const float4 *blk, float4 *dst) {
  const __amdgpu_buffer_rsrc_t r = wave_rsrc(blk, NS * kRT * 16);
  const int vo = (int)threadIdx.x * 16;
#pragma unroll
  for (int j = J0; j < J1; ++j) {
    const f32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, vo, j * kRT * 16, 0);
    dst[j] = make_float4(v.x, v.y, v.z, v.w);
  }
}

// Partial dot product of 4*NJ consecutive inputs x4[0..NJ) with weights w(j): four independent
// FMA chains (k mod 4), summed as (c0 + c1) + (c2 + c3). The chains run in pairs (v_pk_fma_f32: each
// half rounds exactly like v_fma_f32).
typedef float lzm_f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void fma4(float4 v, float4 q, float *a) {
  lzm_f2 lo = {a[0], a[1]}, hi = {a[2], a[3]};
  lo = __builtin_elementwise_fma((lzm_f2){v.x, v.y}, (lzm_f2){q.x, q.y}, lo);
  hi = __builtin_elementwise_fma((lzm_f2){v.z, v.w}, (lzm_f2){q.z, q.w}, hi);
  a[0] = lo.x; a[1] = lo.y; a[2] = hi.x; a[3] = hi.y;
}
template <int NJ, typename WF>
__device__ __forceinline__ float dot4(const float4 *x4, WF w) {
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < NJ; ++j) fma4(x4[j], w(j), a);
  return (a[0] + a[1]) + (a[2] + a[3]);
}

// 128-wide activation rows in LDS are padded: the upper 64 floats start 4 floats after the lower
// ones (row stride kRRow), so the two lanes of a pair, which read float4 j of their half, hit
// different banks (unpadded, the halves are 256 B apart: the same bank, a 2-way conflict on every
// activation read of every dense layer). rpad(c): column c's float offset in a padded row.
constexpr int kRRow = kRHid + 4;
__device__ __forceinline__ int rpad(int c) { return c + ((c >> 6) << 2); }

// The column of a 128 x 128 layer this lane's result holds (both lanes of the pair (l, l ^ 1) hold
// it; the even lane writes it).
__device__ __forceinline__ int d_col() { return 4 * ((int)threadIdx.x >> 3) + (((int)threadIdx.x & 7) >> 1); }

// The four column partials h0..h3 of the 8 lanes of a column group to full sums —
// lanes e and 7 - e (row_half_mirror) split the columns {0, 1} / {2, 3}, lanes e and e ^ 2 split the
// pair, lanes e and e ^ 1 add: column (e >> 1) ends in lanes e, e ^ 1 (the same bits in both: the last
// add is commutative). A fixed order, so every launch rounds the same way.
__device__ __forceinline__ float reduce_d4(float h0, float h1, float h2, float h3) {
  const int e = threadIdx.x & 7;
  const bool lo = e < 4;
  float k0 = lo ? h0 : h2, k1 = lo ? h1 : h3;
  const float s0 = lo ? h2 : h0, s1 = lo ? h3 : h1;
  k0 += dpp_f<0x141>(s0);
  k1 += dpp_f<0x141>(s1);
  const bool q = (e & 2) == 0;
  float m = q ? k0 : k1;
  const float snd = q ? k1 : k0;
  m += dpp_f<0x4E>(snd);
  return m + dpp_f<0xB1>(m);
}

// Full pre-activation of this lane's column (d_col) of a 128 x 128 layer.
template <typename WF>
__device__ __forceinline__ float dense128(const float *x, WF w) {
  const int e = threadIdx.x & 7;
  const float4 *x4 = reinterpret_cast<const float4 *>(x) + 4 * e + (e >> 2);
  float4 xv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) xv[j] = x4[j];
  float a[4][4];
#pragma unroll
  for (int c = 0; c < 4; ++c) a[c][0] = a[c][1] = a[c][2] = a[c][3] = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) fma4(xv[j], w(4 * j + c), a[c]);
  return reduce_d4((a[0][0] + a[0][1]) + (a[0][2] + a[0][3]), (a[1][0] + a[1][1]) + (a[1][2] + a[1][3]),
                   (a[2][0] + a[2][1]) + (a[2][2] + a[2][3]), (a[3][0] + a[3][1]) + (a[3][2] + a[3][3]));
}

// Logits of one support head (input: 32 floats in LDS; weights: the 20-slot buffer P): lane l
// gets columns l, 256 + l and (l < 2 * kRTail, l even) 512 + (l >> 1).
__device__ __forceinline__ void support_logits(const float *h, const float4 *P, const float *bias, float &z0, float &z1,
                                               float &z2) {
  const int tid = threadIdx.x;
  const float4 *h4 = reinterpret_cast<const float4 *>(h);
  z0 = dot4<8>(h4, [&](int j) { return P[j]; }) + bias[tid];
  z1 = dot4<8>(h4, [&](int j) { return P[8 + j]; }) + bias[kRT + tid];
  const float t = dot4<4>(h4 + 4 * (tid & 1), [&](int j) { return P[16 + j]; });
  z2 = (t + dpp_f<0xB1>(t)) + (tid < 2 * kRTail ? bias[2 * kRT + (tid >> 1)] : 0.0f);
}

// Two-action selection outcome of an expanded node when it does not depend on the walk (all
// children visited, or a single legal child): 0 / 1 = the legal position cselect_child picks,
// 3 = a tie between the two visited children (a draw decides), 2 = depends on the walk's mean-q
// (an unvisited child scores the normalised parent mean-q). Same operations as the walk's scores.
// 4 = a leaf tie: both children unvisited (so unexpanded) with bitwise-equal finite prior scores. An
// unvisited child scores x + vu with the walk's normalised mean-q vu, so with equal x the two scores
// are the same float for any non-NaN vu: M = s0 = s1, cselect_child's rule picks position 0 and
// lists position 1 (s1 >= M - 1e-6) — the tie {0, 1} whatever the mean-q is. (A fresh node has
// N = visit - 1 = 0, so both priors are pb_c * sqrtf(0) * prior = +0: every fresh node is one.) With
// a NaN vu the reference picks position 1 without a draw: the walk may use this code only when no
// NaN can reach vu (terms_finite_a2r); the LDS table dec[] keeps the walk-dependent code 2 for it.
__device__ __forceinline__ int a2_decision(float4 c0, float4 c1, int n) {
  if (n < 2) return 0;
  if (!__float_as_int(c0.w) && !__float_as_int(c1.w) && __float_as_int(c0.z) < 0 && __float_as_int(c1.z) < 0 &&
      __float_as_int(c0.x) == __float_as_int(c1.x) && (__float_as_int(c0.x) & 0x7f800000) != 0x7f800000)
    return 4;
  if (!__float_as_int(c0.w) || !__float_as_int(c1.w)) return 2;
  const float s0 = c0.x + c0.y, s1 = c1.x + c1.y;
  const float M = fmaxf(s0, s1);
  const int r = (s0 == M) ? 0 : 1;
  return (r == 0 && s1 >= M - 0.000001f) ? 3 : r;
}
// the code the LDS table dec[] holds (descend_a2, descend_a2f, speculate_depth_a2: a leaf tie is
// scored with the mean-q like any node with an unvisited child)
__device__ __forceinline__ int a2_table_code(int d) { return d == 4 ? 2 : d; }

// ---- selection split in two (MuZero, tree slice in LDS, one root):
// (1) every expanded node's pUCT terms that do not depend on the walk, one thread per node
//     (cucb_score, cnode.cpp:655-699: prior_score, and for visited children the normalised,
//     clamped value term; compute_mean_q's sums over visited children, cnode.cpp:169-203);
// (2) the walk itself (wave 0), left with the mean-q chain (the only walk-dependent term: it is
//     what unvisited children score) and the argmax / tie list per level.
// Same float operations in the same order as descend_wave, so the same bits.
// nq[latent] = {total_q, total_v}; cs[child node] = {prior_score, value term, child latent, visited}
// dec (nullable, A == 2): each node's walk-independent outcome (a2_decision) for descend_a2.
// node_terms: one expanded node n (latent L), by the calling thread.
__device__ inline void node_terms(const TreeView &t, int L, int n, float2 *nq, float4 *cs, float4 mm, int players,
                                  float disc, int *dec) {
  {
    const NodeStat s = t.stat[n];
    const int nleg = legal_n(t, 0, n);
    const int base = 1 + t.A * L;
    int N = s.visit - 1;
    N = N < 0 ? 0 : (N >= t.lut_n ? t.lut_n - 1 : N);
    const float2 Lx = t.lut[N];
    float total_q = 0.0f;
    int total_v = 0;
    float4 c01[2];
    for (int j = 0; j < nleg; ++j) {
      const int c = base + legal_at(t, 0, n, j);
      const NodeStat cst = t.stat[c];
      const float cv = t.val[c];
      const float tr = cst.reward;
      float vv = 0.0f;
      if (cst.visit > 0) {
        total_q += tr + disc * cv;
        ++total_v;
        float v = (players == 1) ? tr + disc * cv : tr + disc * (-cv);
        v = mm_normalize(mm, v);
        if (v < 0) v = 0;
        if (v > 1) v = 1;
        vv = v;
      }
      float pb_c = Lx.x;
      pb_c *= (t.pbt && cst.visit <= N) ? t.pbt[N * (N + 1) / 2 + cst.visit] : (Lx.y / (float)(cst.visit + 1));
      const float4 term = make_float4(pb_c * cst.prior, vv, __int_as_float(t.meta[c].latent),
                                      __int_as_float(cst.visit > 0 ? 1 : 0));
      cs[c] = term;
      if (j < 2) c01[j] = term;
    }
    nq[L] = make_float2(total_q, __int_as_float(total_v));
    if (dec) dec[L] = (t.A == 2 && nleg >= 1) ? a2_table_code(a2_decision(c01[0], c01[nleg > 1 ? 1 : 0], nleg)) : 2;
  }
}
__device__ inline void precompute_terms(const TreeView &t, int nlat, const int *lat2node, float2 *nq, float4 *cs,
                                        float4 mm, int players, float disc, int *dec = nullptr) {
  for (int L = threadIdx.x; L < nlat; L += kRT) {
    const int n = lat2node[L];
    if (n >= 0) node_terms(t, L, n, nq, cs, mm, players, disc, dec);
  }
}

// A2Rec: one expanded node's record as the register walk (descend_a2r) reads it from the lane that
// computed it. pk: bits 0-2 a2_decision's code, bit 3 / 4 child 0 / 1 visited, bits 5-6 total_v,
// then three latents as signed bytes (-1: unexpanded; latents < 64): bits 8-15 the decided child's
// (code 0 / 1: what the chase follows, one s_bfe_i32), bits 16-23 / 24-31 child 0 / 1's; tq = total_q;
// x0, y0, x1, y1 = the children's prior score and value term (cs[].x, cs[].y).
struct A2Rec {
  int pk;
  float tq, x0, y0, x1, y1;
};
__device__ __forceinline__ int a2rec_pack(int d, bool vis0, bool vis1, int total_v, int l0, int l1) {
  return d | (vis0 ? 8 : 0) | (vis1 ? 16 : 0) | (total_v << 5) | (((d == 1 ? l1 : l0) & 0xff) << 8) | ((l0 & 0xff) << 16) |
         (int)((unsigned)(l1 & 0xff) << 24);
}
// node_terms for two actions, written for few LDS round trips: a child's slot depends on the latent
// only (1 + 2 L + legal position; the root, latent 0, takes its legal actions from registers), so
// both children's records are read with the latent -> node map, the node's visit count next, then
// the pb_c table row; every read is unconditional and the branches are selects. Same float
// operations in the same order as node_terms (so the same bits), and also dec[L] and, when rec is
// given, the node's record in the calling lane's registers.
__device__ inline void node_terms_a2(const TreeView &t, int L, const int *lat2node, float2 *nq, float4 *cs, float4 mm,
                                     int players, float disc, int *dec, const int *rleg, int nleg_root, A2Rec *rec) {
  {
    const int n = lat2node[L];
    const bool root = L == 0;
    const int nleg = root ? nleg_root : 2;
    const int base = 1 + 2 * L;
    const int c0 = base + (root ? rleg[0] : 0);
    const int c1 = base + (root ? rleg[nleg > 1 ? 1 : 0] : 1);
    const NodeStat s0 = t.stat[c0], s1 = t.stat[c1];
    const float v0 = t.val[c0], v1 = t.val[c1];
    const int l0 = t.meta[c0].latent, l1 = t.meta[c1].latent;
    if (n < 0) return;
    int N = t.stat[n].visit - 1;
    N = N < 0 ? 0 : (N >= t.lut_n ? t.lut_n - 1 : N);
    const float2 Lx = t.lut[N];
    const int row = N * (N + 1) / 2;
    const bool p0 = t.pbt && s0.visit <= N, p1 = t.pbt && s1.visit <= N;
    const float f0 = p0 ? t.pbt[row + s0.visit] : (Lx.y / (float)(s0.visit + 1));
    const float f1 = p1 ? t.pbt[row + s1.visit] : (Lx.y / (float)(s1.visit + 1));
    float total_q = 0.0f;
    int total_v = 0;
    float vv0 = 0.0f, vv1 = 0.0f;
    if (s0.visit > 0) {
      total_q += s0.reward + disc * v0;
      ++total_v;
      float v = (players == 1) ? s0.reward + disc * v0 : s0.reward + disc * (-v0);
      v = mm_normalize(mm, v);
      if (v < 0) v = 0;
      if (v > 1) v = 1;
      vv0 = v;
    }
    if (nleg > 1 && s1.visit > 0) {
      total_q += s1.reward + disc * v1;
      ++total_v;
      float v = (players == 1) ? s1.reward + disc * v1 : s1.reward + disc * (-v1);
      v = mm_normalize(mm, v);
      if (v < 0) v = 0;
      if (v > 1) v = 1;
      vv1 = v;
    }
    float pb0 = Lx.x, pb1 = Lx.x;
    pb0 *= f0;
    pb1 *= f1;
    const float4 t0 = make_float4(pb0 * s0.prior, vv0, __int_as_float(l0), __int_as_float(s0.visit > 0 ? 1 : 0));
    const float4 t1 = make_float4(pb1 * s1.prior, vv1, __int_as_float(l1), __int_as_float(s1.visit > 0 ? 1 : 0));
    if (nleg > 0) cs[c0] = t0;
    if (nleg > 1) cs[c1] = t1;
    nq[L] = make_float2(total_q, __int_as_float(total_v));
    const int d = nleg >= 1 ? a2_decision(t0, nleg > 1 ? t1 : t0, nleg) : 2;
    dec[L] = a2_table_code(d);
    if (rec) {
      rec->pk = a2rec_pack(d, s0.visit > 0, s1.visit > 0, total_v, l0, l1);
      rec->tq = total_q; rec->x0 = t0.x; rec->y0 = t0.y; rec->x1 = t1.x; rec->y1 = t1.y;
    }
  }
}
__device__ inline void precompute_terms_a2(const TreeView &t, int nlat, const int *lat2node, float2 *nq, float4 *cs,
                                           float4 mm, int players, float disc, int *dec, const int *rleg,
                                           int nleg_root) {
  for (int L = threadIdx.x; L < nlat; L += kRT)
    node_terms_a2(t, L, lat2node, nq, cs, mm, players, disc, dec, rleg, nleg_root, nullptr);
}

// The walk over the precomputed terms (descend_wave's contract and outputs; wave 0).
// Where a walk stands at the top of a level (a classification walk stops at a tie with the
// state of that level, so the resolution resumes there instead of walking from the root).
struct WalkState {
  int node, lat, len, plat, last_action, is_root, vtp;
  float parent_q;
};
__device__ inline WalkState walk_start(const TreeView &t, int vtp) {
  WalkState w;
  w.node = 0; w.lat = t.meta[0].latent; w.len = 0; w.plat = -1; w.last_action = -1; w.is_root = 1; w.vtp = vtp;
  w.parent_q = 0.0f;
  return w;
}

template <bool CLASSIFY, typename Draw>
__device__ inline Descent descend_terms(const TreeView &t, const float2 *nq, const float4 *cs, float4 mm, int vtp,
                                        int players, Draw draw, TieInfo *tie, WalkState *resume = nullptr,
                                        WalkState *at_tie = nullptr) {
  const int lane = threadIdx.x & 63;
  WalkState w0 = resume ? *resume : walk_start(t, vtp);
  int node = w0.node, is_root = w0.is_root, len = w0.len, last_action = w0.last_action, plat = w0.plat;
  float parent_q = w0.parent_q;
  int lat = w0.lat;
  vtp = w0.vtp;
  if (lane == 0 && !resume) t.path[0] = 0;
  if (CLASSIFY) tie->status = 0;
  while (lat >= 0 && len < t.depth_cap - 1) {
    if (CLASSIFY && at_tie) {
      at_tie->node = node; at_tie->lat = lat; at_tie->len = len; at_tie->plat = plat;
      at_tie->last_action = last_action; at_tie->is_root = is_root; at_tie->vtp = vtp; at_tie->parent_q = parent_q;
    }
    const int n = legal_n(t, 0, node);
    const int base = 1 + t.A * lat;
    const bool valid = lane < n;
    const int a = valid ? legal_at(t, 0, node, lane) : 0;
    const float4 c = valid ? cs[base + a] : make_float4(0.0f, 0.0f, __int_as_float(-1), __int_as_float(0));
    const float2 q = nq[lat];
    const int total_v = __float_as_int(q.y);
    float mean_q;
    if (is_root && total_v > 0)
      mean_q = q.x / (float)total_v;
    else
      mean_q = (parent_q + q.x) / (float)(total_v + 1);
    is_root = 0;
    parent_q = mean_q;
    float vu = mm_normalize(mm, mean_q);
    if (vu < 0) vu = 0;
    if (vu > 1) vu = 1;
    const float score = c.x + (__float_as_int(c.w) ? c.y : vu);
    const float M = wave_max_dpp(valid ? score : -INFINITY);
    const int r = __ffsll((long long)__ballot(valid && score == M)) - 1;
    const uint64_t mask = __ballot(valid && lane > r && score >= M - 0.000001f) | (1ull << r);
    const int nl = __popcll(mask);
    if (CLASSIFY && nl > 1) {
      const bool leaf_child = !((mask >> lane) & 1ull) || __float_as_int(c.z) < 0;
      const bool all_leaves = __ballot(!leaf_child) == 0ull;
      if (players > 1) vtp = (vtp == 1) ? 2 : 1;
      tie->status = all_leaves ? 1 : 2;
      tie->level = len;
      tie->mask = mask;
      Descent d;
      d.len = len + 1;
      d.x = lat;
      d.action = -1;
      d.vtp = vtp;
      d.leaf = -1;
      return d;
    }
    const uint32_t rr = CLASSIFY ? 0u : draw(len);
    int kk = (int)(rr % (uint32_t)nl);
    uint64_t mm_ = mask;
    for (; kk > 0; --kk) mm_ &= mm_ - 1;
    const int jsel = __ffsll((long long)mm_) - 1;
    const int action = __builtin_amdgcn_readlane(a, jsel);
    if (players > 1) vtp = (vtp == 1) ? 2 : 1;
    node = base + action;
    last_action = action;
    if (lane == 0) {
      t.path_act[len] = action;
      t.path[len + 1] = node;
    }
    ++len;
    plat = lat;
    lat = __builtin_amdgcn_readlane(__float_as_int(c.z), jsel);
  }
  Descent d;
  d.len = len;
  d.x = plat;
  d.action = last_action;
  d.vtp = vtp;
  d.leaf = node;
  return d;
}

// descend_terms for exactly two actions, written for the shortest dependent chain per level: every
// lane of the wave evaluates the level (both children's terms as broadcast LDS reads, per-lane
// compares: no DPP reduction, ballots or readlanes on the chain), and the root's legal actions (rleg,
// nleg) are passed in registers. The terms phase precomputes each node's walk-independent outcome
// (dec[latent], a2_decision); where it is known the level takes it as it is, and only a node with an
// unvisited child scores its children with the normalised mean-q. The normaliser's divisor is fixed
// per walk (mm_normalize's branches become one division); same float operations as descend_terms,
// so the same bits.
__device__ __forceinline__ float mm_norm_fixed(bool scale, float lo, float div, float v) {
  return scale ? (v - lo) / div : v;
}

template <bool CLASSIFY, typename Draw>
__device__ inline Descent descend_a2(const TreeView &t, const float2 *nq, const int *dec, const float4 *cs, float4 mm,
                                     int vtp, int players, const int *rleg, int nleg, Draw draw, TieInfo *tie,
                                     WalkState *resume = nullptr, WalkState *at_tie = nullptr) {
  const int lane = threadIdx.x & 63;
  const float delta = mm.x - mm.y;
  const bool scale = delta > 0;
  const float div = (delta < mm.z) ? mm.z : delta;
  const float lo = mm.y;
  WalkState w0 = resume ? *resume : walk_start(t, vtp);
  int node = w0.node, len = w0.len, last_action = w0.last_action, plat = w0.plat, lat = w0.lat;
  float parent_q = w0.parent_q;
  bool is_root = w0.is_root;
  vtp = w0.vtp;
  if (lane == 0 && !resume) t.path[0] = 0;
  if (CLASSIFY) tie->status = 0;
  const int dmax = t.depth_cap - 1;
  int a0 = 0, a1 = 0, n = 2;
  float4 c0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), c1 = c0;
  float2 q = make_float2(0.0f, 0.0f);
  int dl = 2;
  auto fetch = [&](int nd, int lt) {
    const bool root = nd == 0;  // (only the first level of a walk from the root)
    a0 = root ? rleg[0] : 0;
    a1 = root ? rleg[1] : 1;
    n = root ? nleg : 2;
    const int base = 1 + 2 * lt;
    c0 = cs[base + a0];
    c1 = cs[base + (n > 1 ? a1 : a0)];
    q = nq[lt];
    dl = dec[lt];
  };
  while (lat >= 0 && len < dmax) {
    fetch(node, lat);
    const int base = 1 + 2 * lat;
    const int total_v = __float_as_int(q.y);
    const float qx = q.x;
    int jsel = dl;
    bool tie2 = dl == 3;
    const bool rootq = is_root && total_v > 0;
    const float mean_q = rootq ? qx / (float)total_v : (parent_q + qx) / (float)(total_v + 1);
    if (dl == 2) {
      float vu = mm_norm_fixed(scale, lo, div, mean_q);
      if (vu < 0) vu = 0;
      if (vu > 1) vu = 1;
      const float s0 = c0.x + (__float_as_int(c0.w) ? c0.y : vu);
      const float s1 = c1.x + (__float_as_int(c1.w) ? c1.y : vu);
      const float M = fmaxf(s0, s1);
      jsel = (s0 == M) ? 0 : 1;
      tie2 = jsel == 0 && s1 >= M - 0.000001f;
    }
    if (CLASSIFY && tie2) {
      if (at_tie) {
        at_tie->node = node; at_tie->lat = lat; at_tie->len = len; at_tie->plat = plat;
        at_tie->last_action = last_action; at_tie->is_root = is_root; at_tie->vtp = vtp; at_tie->parent_q = parent_q;
      }
      if (players > 1) vtp = (vtp == 1) ? 2 : 1;
      const bool all_leaves = __float_as_int(c0.z) < 0 && __float_as_int(c1.z) < 0;
      tie->status = all_leaves ? 1 : 2;
      tie->level = len;
      tie->mask = 3ull;
      Descent d;
      d.len = len + 1;
      d.x = lat;
      d.action = -1;
      d.vtp = vtp;
      d.leaf = -1;
      return d;
    }
    if (!CLASSIFY && tie2) jsel = (int)(draw(len) % 2u);
    const int action = jsel ? a1 : a0;
    const int nlat = __float_as_int(jsel ? c1.z : c0.z);
    const int nnode = base + action;
    is_root = false;
    parent_q = mean_q;
    if (players > 1) vtp = (vtp == 1) ? 2 : 1;
    node = nnode;
    last_action = action;
    if (lane == 0) {
      t.path_act[len] = action;
      t.path[len + 1] = node;
    }
    ++len;
    plat = lat;
    lat = nlat;
  }
  Descent d;
  d.len = len;
  d.x = plat;
  d.action = last_action;
  d.vtp = vtp;
  d.leaf = node;
  return d;
}

// Depth speculation for a classification walk stopped at a tie between children of which one is
// expanded (status 2, A == 2): lane `pattern` continues the walk from the tie's state taking, at the
// i-th tie on its way, the child that draw parity bit i of `pattern` selects (rr % 2 picks legal
// position 0 or 1); returns that walk's depth (Descent::len), or -1 when it meets more than 6 ties.
// If all 64 patterns give one depth, the root's draw count is known before any of its draw values:
// it is published at once and the path is resolved after the look-back (same walk, same bits).
// Same per-level operations as descend_a2.
// *choice gets bit l = the legal position taken at level w.len + l, *ties bit l
// when that level was a tie decided by the pattern, *leaf_tie the offset of a final tie between two
// unexpanded children (its draw picks the leaf; -1: none); *choice = ~0u when the walk is longer than
// 31 levels past w.len. The path of a walk is then its choice bits: the look-back's draw parities
// select the lane whose pattern matches, and the path is a pointer chase without the scores.
__device__ inline int speculate_depth_a2(const TreeView &t, const float2 *nq, const int *dec, const float4 *cs,
                                         float4 mm, const int *rleg, int nleg, const WalkState &w, int pattern,
                                         uint32_t *choice, uint32_t *ties, int *leaf_tie) {
  uint32_t ch = 0u, tm = 0u;
  *leaf_tie = -1;
  const float delta = mm.x - mm.y;
  const bool scale = delta > 0;
  const float div = (delta < mm.z) ? mm.z : delta;
  const float lo = mm.y;
  int node = w.node, len = w.len, lat = w.lat, used = 0;
  bool is_root = w.is_root;
  float parent_q = w.parent_q;
  const int dmax = t.depth_cap - 1;
  while (lat >= 0 && len < dmax) {
    const bool root = node == 0;
    const int a0 = root ? rleg[0] : 0, a1 = root ? rleg[1] : 1, n = root ? nleg : 2;
    const int base = 1 + 2 * lat;
    const float4 c0 = cs[base + a0];
    const float4 c1 = cs[base + (n > 1 ? a1 : a0)];
    const float2 q = nq[lat];
    const int dl = dec[lat];
    const int total_v = __float_as_int(q.y);
    const float mean_q = (is_root && total_v > 0) ? q.x / (float)total_v : (parent_q + q.x) / (float)(total_v + 1);
    int jsel = dl;
    bool tie2 = dl == 3;
    if (dl == 2) {
      float vu = mm_norm_fixed(scale, lo, div, mean_q);
      if (vu < 0) vu = 0;
      if (vu > 1) vu = 1;
      const float s0 = c0.x + (__float_as_int(c0.w) ? c0.y : vu);
      const float s1 = c1.x + (__float_as_int(c1.w) ? c1.y : vu);
      const float M = fmaxf(s0, s1);
      jsel = (s0 == M) ? 0 : 1;
      tie2 = jsel == 0 && s1 >= M - 0.000001f;
    }
    const int off = len - w.len;
    if (tie2) {
      if (__float_as_int(c0.z) < 0 && __float_as_int(c1.z) < 0) {  // either way a leaf
        *choice = off < 31 ? ch : ~0u; *ties = tm; *leaf_tie = off;
        return len + 1;
      }
      if (used == 6) return -1;
      jsel = (pattern >> used) & 1;
      ++used;
      if (off < 31) tm |= 1u << off;
    }
    if (off < 31) ch |= (uint32_t)jsel << off;
    is_root = false;
    parent_q = mean_q;
    node = base + (jsel ? a1 : a0);
    lat = __float_as_int(jsel ? c1.z : c0.z);
    ++len;
  }
  *choice = len - w.len <= 31 ? ch : ~0u; *ties = tm;
  return len;
}

// descend_a2 with the walk state cut to what a decided level needs: the root level runs through
// descend_a2's general body (legal list, root mean-q rule); below it a level whose outcome is
// known (dec 0 / 1) is a pointer chase plus the mean-q division for the next level, and any other
// level (an unvisited child or a tie) hands the walk back to descend_a2 at that level's state
// (same operations either way, so the same bits). vtp flips per level are applied at the end.
template <bool CLASSIFY, typename Draw>
__device__ inline Descent descend_a2f(const TreeView &t, const float2 *nq, const int *dec, const float4 *cs, float4 mm,
                                      int vtp, int players, const int *rleg, int nleg, Draw draw, TieInfo *tie,
                                      WalkState *at_tie = nullptr) {
  const int lane = threadIdx.x & 63;
  // root level: the general body for one level
  WalkState w = walk_start(t, vtp);
  if (w.lat < 0 || t.depth_cap <= 1) return descend_a2<CLASSIFY>(t, nq, dec, cs, mm, vtp, players, rleg, nleg, draw, tie,
                                                                  nullptr, at_tie);
  {
    const int dl = dec[w.lat];
    if (dl >= 2) return descend_a2<CLASSIFY>(t, nq, dec, cs, mm, vtp, players, rleg, nleg, draw, tie, nullptr, at_tie);
    const float2 q = nq[w.lat];
    const int action = rleg[dl];
    const float4 c = cs[1 + 2 * w.lat + action];
    const int tv = __float_as_int(q.y);
    w.parent_q = tv > 0 ? q.x / (float)tv : (0.0f + q.x) / (float)(tv + 1);
    if (lane == 0) {
      t.path[0] = 0;
      t.path_act[0] = action;
      t.path[1] = 1 + 2 * w.lat + action;
    }
    w.node = 1 + 2 * w.lat + action;
    w.last_action = action;
    w.plat = w.lat;
    w.lat = __float_as_int(c.z);
    w.len = 1;
    w.is_root = 0;
  }
  // non-root levels: two children at legal positions 0 / 1
  int lat = w.lat, node = w.node, len = w.len, plat = w.plat, last_action = w.last_action;
  float parent_q = w.parent_q;
  const int dmax = t.depth_cap - 1;
  int dl = 2;
  while (lat >= 0 && len < dmax) {
    dl = dec[lat];
    if (dl >= 2) break;
    const float2 q = nq[lat];
    const float4 c = cs[1 + 2 * lat + dl];
    const int nnode = 1 + 2 * lat + dl;
    if (lane == 0) {
      t.path_act[len] = dl;
      t.path[len + 1] = nnode;
    }
    parent_q = (parent_q + q.x) / (float)(__float_as_int(q.y) + 1);
    last_action = dl;
    node = nnode;
    plat = lat;
    lat = __float_as_int(c.z);
    ++len;
  }
  if (players > 1 && (len & 1)) vtp = (vtp == 1) ? 2 : 1;
  if (lat >= 0 && len < dmax) {
    // an undecided level: continue with the general body from this level's state
    WalkState r;
    r.node = node; r.lat = lat; r.len = len; r.plat = plat; r.last_action = last_action; r.is_root = 0;
    r.vtp = vtp; r.parent_q = parent_q;
    return descend_a2<CLASSIFY>(t, nq, dec, cs, mm, vtp, players, rleg, nleg, draw, tie, &r, at_tie);
  }
  if (CLASSIFY) tie->status = 0;
  Descent d;
  d.len = len;
  d.x = plat;
  d.action = last_action;
  d.vtp = vtp;
  d.leaf = node;
  return d;
}

// The NaN guard of descend_a2r's leaf-tie shortcut (wave 0, after the terms pass): every expanded
// node's total_q and the min-max bounds are finite. The mean-q chain's operands are then sums of
// finite terms over positive counts, so no NaN reaches a level's vu, and a leaf tie is the tie {0, 1}.
__device__ __forceinline__ bool terms_finite_a2r(const A2Rec &rc, float4 mm) {
  const auto fin = [](float v) { return (__float_as_int(v) & 0x7f800000) != 0x7f800000; };
  return __ballot(!fin(rc.tq)) == 0ull && fin(mm.x) && fin(mm.y) && fin(mm.z);
}

// The register walk's mean-q chain over the path levels [pend, upto) (wave 0; lane l holds level l's
// latent plev, lane L the record (rtq = total_q, rpk = A2Rec::pk) of latent L; parent_q: the chain's
// value through level pend - 1, 0.0f at pend == 0). Returns the value through level upto - 1:
//   q_0 = tv_0 > 0 ? tq_0 / tv_0 : (0.0f + tq_0) / 1,   q_l = (q_{l-1} + tq_l) / (tv_l + 1)
// with descend_a2's operations in level order, so the same bits. With two actions the divisors are
// 1, 2 or 3 (div_small). Two forms:
//  - serial: three v_readlane, the add and div_small per level;
//  - in lanes (kSettleLanesMin levels or more): one ds_bpermute pair gives every path lane its own
//    tq_l and divisor, then a systolic pass of upto - pend steps in which every lane takes its left
//    neighbour's value (DPP wave_shr:1; lane 0 reads 0.0f, the root's parent_q), adds its tq and
//    divides by its own divisor. Lane l's value is final from step l - pend + 1 on, and recomputing
//    it from final inputs gives the same bits; lanes below pend hold parent_q and stay. Five
//    vector instructions a step, no readlane, no scalar select: it pays from three levels on
//    (walk_ubench variant 8, profiles/settle_lanes/). The pass uses div_small's three
//    operations unguarded and 0.0f + tq for the root's tq, which is exact unless a tq is -0 or a
//    value of the chain is not finite (an overflowing sum: the terms are finite under leaf_ok): one
//    ballot after the pass then hands the levels to the serial form, as does !leaf_ok.
constexpr int kSettleLanesMin = 3;
__device__ __forceinline__ float settle_chain(float rtq, int rpk, int plev, bool leaf_ok, int pend, int upto,
                                              float parent_q) {
  if (upto <= pend) return parent_q;  // (the level above was scored: nothing pending)
  if (upto - pend >= kSettleLanesMin && leaf_ok) {
    const int lane = threadIdx.x & 63;
    const float tq = __int_as_float(__builtin_amdgcn_ds_bpermute(plev << 2, __float_as_int(rtq)));
    const int tv = (__builtin_amdgcn_ds_bpermute(plev << 2, rpk) >> 5) & 3;
    const int d = (lane == 0 && tv > 0) ? tv : tv + 1;
    const float y = div_small_y(d), nd = -(float)d;
    const bool below = lane < pend;
    float qv = parent_q;  // (lane pend - 1 is the one that is read)
    for (int i = pend; i < upto; ++i) {
      const float in = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(qv), 0x138, 0xF, 0xF, true));
      const float q = div_small_core(in + tq, y, nd);
      qv = below ? qv : q;
    }
    // lanes [pend, upto): a tq of -0, a value that is inf or NaN (v_cmp_class masks)
    const unsigned long long range = (~0ull >> (64 - (upto - pend))) << pend;
    const unsigned long long bad = __builtin_amdgcn_ballot_w64(__builtin_amdgcn_classf(tq, 0x020) ||
                                                               __builtin_amdgcn_classf(qv, sgpr_literal<0x207>()));
    if ((bad & range) == 0ull) return readlane_f(qv, upto - 1);
    parent_q = pend > 0 ? readlane_f(qv, pend - 1) : 0.0f;  // (as it came: it need not stay live over the pass)
  }
  const auto level = [&](int l, float &tq) {
    const int Ls = __builtin_amdgcn_readlane(plev, l);
    tq = readlane_f(rtq, Ls);
    return (__builtin_amdgcn_readlane(rpk, Ls) >> 5) & 3;
  };
  int l = pend;
  if (l == 0) {  // the root's rule
    float tq;
    const int tv = level(0, tq);
    parent_q = div_small(tv > 0 ? tq : parent_q + tq, tv > 0 ? tv : 1);
    l = 1;
  }
  for (; l < upto; ++l) {
    float tq;
    const int tv = level(l, tq);
    parent_q = div_small(parent_q + tq, tv + 1);
  }
  return parent_q;
}

// The walk on the terms pass's registers (selection mode 5; S + 2 <= 64, so lane L of wave 0 holds
// the record of the node with latent L): a chase of v_readlane reads with the current latent in a
// scalar register, no LDS read per level. A decided level (code 0 / 1) only moves the pointer; a
// leaf tie (code 4, when leaf_ok: terms_finite_a2r) ends the walk with no floating-point work. The
// mean-q chain is evaluated only where its value is read — a node with an unvisited child (code
// 2), a tie between visited children (code 3: the resume needs WalkState::parent_q) — by settle()
// (settle_chain above): the same quotients, in level order, over the (total_q, total_v) of the path's
// levels, so the same bits as descend_a2's level-by-level chain. The path is collected in lanes (lane l: level l's
// latent and action) and stored once. Same outputs as descend_a2f (Descent, TieInfo, at_tie, path,
// path_act), every lane returns the same values. With !leaf_ok a leaf tie is scored like code 2:
// the walk then does what descend_a2 does at every level.
template <bool CLASSIFY, typename Draw>
__device__ inline Descent descend_a2r(const TreeView &t, const A2Rec &rc, bool leaf_ok, float4 mm, int vtp, int players,
                                      const int *rleg, int nleg, Draw draw, TieInfo *tie, WalkState *at_tie = nullptr) {
  const int lane = threadIdx.x & 63;
  const int dmax = t.depth_cap - 1;
  const int lat0 = __builtin_amdgcn_readfirstlane(t.meta[0].latent);
  int lat = lat0, len = 0;
  int plev = 0, pact = 0;  // lane l: the latent and the action of level l
  float parent_q = 0.0f;
  int pend = 0;  // the chain is settled through level pend - 1
  const auto rl = [](int v, int l) { return __builtin_amdgcn_readlane(v, l); };
  const auto rlf = [](float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); };
  const auto child = [](int pk, int j) { return (int)((unsigned)pk << (8 - 8 * j)) >> 24; };  // (signed bytes)
  const auto decided = [](int pk) { return (int)((unsigned)pk << 16) >> 24; };
  auto step = [&](int action, int nlat) {  // cross the level at lat
    plev = lane == len ? lat : plev;
    pact = lane == len ? action : pact;
    ++len;
    lat = nlat;
  };
  // the last level crossed (len > 0): the leaf's parent latent and the action taken there
  const auto plat_of = [&]() { return len > 0 ? rl(plev, len - 1) : -1; };
  const auto act_of = [&]() { return len > 0 ? rl(pact, len - 1) : -1; };
  auto settle = [&](int upto) {
    parent_q = settle_chain(rc.tq, rc.pk, plev, leaf_ok, pend, upto, parent_q);
    pend = upto > pend ? upto : pend;
  };
  auto flush = [&]() {
    if (lane == 0) t.path[0] = 0;
    if (lane < len) {
      t.path_act[lane] = pact;
      t.path[lane + 1] = 1 + 2 * plev + pact;
    }
  };
  if (CLASSIFY) tie->status = 0;
  // A lone wave issues its instructions one after the other, so a level costs what its instruction
  // count costs (walk_ubench): the decided levels run in a loop of their own (the chase proper: about
  // fifteen instructions a level, the state two scalars) and only a level the chase stops at (pk, dl: a leaf
  // tie, an unvisited child, a tie between visited children) takes the general body. The chase needs
  // no depth check: it crosses expanded nodes only, at most S of them, and depth_cap >= S + 2 (host).
  int pk = 0, dl = 0;
  bool stop = false;
  if (lat >= 0 && len < dmax) {  // the root: legal position j is action rleg[j]
    pk = rl(rc.pk, lat);
    dl = pk & 7;
    if (dl <= 1)
      step(rleg[dl], decided(pk));
    else
      stop = true;
  }
  for (;;) {
    if (!stop && lat >= 0) {
      for (;;) {
        pk = rl(rc.pk, lat);
        dl = pk & 7;
        if (dl > 1) {
          stop = true;
          break;
        }
        step(dl, decided(pk));
        if (lat < 0) break;
      }
    }
    if (!stop || len >= dmax) break;  // a leaf (or the depth cap)
    stop = false;
    const bool root = len == 0;
    int jsel = 0;
    if (dl == 4 && leaf_ok) {
      // a leaf tie: the tie {0, 1} whatever the mean-q is (a2_decision)
      if (CLASSIFY) {
        flush();
        const int vt = (players > 1 && (len & 1)) ? ((vtp == 1) ? 2 : 1) : vtp;
        tie->status = 1;
        tie->level = len;
        tie->mask = 3ull;
        Descent d;
        d.len = len + 1;
        d.x = lat;
        d.action = -1;
        d.vtp = players > 1 ? ((vt == 1) ? 2 : 1) : vt;
        d.leaf = -1;
        return d;
      }
      jsel = __builtin_amdgcn_readfirstlane((int)(draw(len) % 2u));
    } else {
      settle(len);
      bool tie2 = dl == 3;
      float mean_q = 0.0f;
      if (dl != 3) {  // an unvisited child scores the normalised mean-q (code 2; 4 without leaf_ok)
        const float delta = mm.x - mm.y;
        const bool scale = delta > 0;
        const float div = (delta < mm.z) ? mm.z : delta;
        const float tq = rlf(rc.tq, lat);
        const int tv = (pk >> 5) & 3;
        const bool rootq = root && tv > 0;
        mean_q = div_small(rootq ? tq : parent_q + tq, rootq ? tv : tv + 1);
        float vu = mm_norm_fixed(scale, mm.y, div, mean_q);
        if (vu < 0) vu = 0;
        if (vu > 1) vu = 1;
        const float s0 = rlf(rc.x0, lat) + ((pk & 8) ? rlf(rc.y0, lat) : vu);
        const float s1 = rlf(rc.x1, lat) + ((pk & 16) ? rlf(rc.y1, lat) : vu);
        const float M = fmaxf(s0, s1);
        const int j = (s0 == M) ? 0 : 1;
        jsel = __builtin_amdgcn_readfirstlane(j);
        tie2 = __builtin_amdgcn_readfirstlane((j == 0 && s1 >= M - 0.000001f) ? 1 : 0) != 0;
      }
      if (CLASSIFY && tie2) {
        const int vt = (players > 1 && (len & 1)) ? ((vtp == 1) ? 2 : 1) : vtp;  // (one flip per level above)
        const bool all_leaves = ((unsigned)pk >> 16) == 0xffffu;
        if (at_tie && !all_leaves) {  // (read by the status-2 resume only)
          const int plat = plat_of(), last_action = act_of();
          at_tie->node = root ? 0 : 1 + 2 * plat + last_action; at_tie->lat = lat; at_tie->len = len; at_tie->plat = plat;
          at_tie->last_action = last_action; at_tie->is_root = root; at_tie->vtp = vt; at_tie->parent_q = parent_q;
        }
        flush();
        tie->status = all_leaves ? 1 : 2;
        tie->level = len;
        tie->mask = 3ull;
        Descent d;
        d.len = len + 1;
        d.x = lat;
        d.action = -1;
        d.vtp = players > 1 ? ((vt == 1) ? 2 : 1) : vt;
        d.leaf = -1;
        return d;
      }
      if (!CLASSIFY && tie2) jsel = __builtin_amdgcn_readfirstlane((int)(draw(len) % 2u));
      if (dl != 3) {
        parent_q = mean_q;
        pend = len + 1;
      }
    }
    step(root ? rleg[jsel] : jsel, child(pk, jsel));
  }
  flush();
  const int plat = plat_of(), last_action = act_of();
  Descent d;
  d.len = len;
  d.x = plat;
  d.action = last_action;
  d.vtp = (players > 1 && (len & 1)) ? ((vtp == 1) ? 2 : 1) : vtp;
  d.leaf = len == 0 ? 0 : 1 + 2 * plat + last_action;
  return d;
}

// NR rows of a 128 x 128 layer (inputs x + r * kRRow): each weight read once for all rows (NR = 2:
// the two candidates of a late draw through fc_dynamics[1]).
struct NoSide {
  __device__ __forceinline__ void operator()(int) const {}
};
// side(j) runs at the top of slot j: a weight prefetch spread over the layer, one or two buffer
// loads per slot, instead of a burst that stalls the wave at issue (the texture path takes a
// 1 KiB wave-load per 16 cycles and four waves share it). POST: side(j) runs behind slot j's
// FMAs instead, when w(j)'s register is free: the rolling refill of the stream buffer, whose slot j
// takes the next streamed layer's slot j
template <int NR, bool POST = false, typename WF, typename SF = NoSide>
__device__ __forceinline__ void dense128n(const float *x, WF w, float *z, SF side = SF()) {
  const int e = threadIdx.x & 7;
  float4 xv[NR][4];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int j = 0; j < 4; ++j) xv[r][j] = reinterpret_cast<const float4 *>(x + r * kRRow)[4 * e + (e >> 2) + j];
  float a[NR][4][4];
#pragma unroll
  for (int r = 0; r < NR; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) a[r][c][0] = a[r][c][1] = a[r][c][2] = a[r][c][3] = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (!POST) side(4 * j + c);
      const float4 q = w(4 * j + c);
#pragma unroll
      for (int r = 0; r < NR; ++r) fma4(xv[r][j], q, a[r][c]);
      if (POST) side(4 * j + c);
    }
#pragma unroll
  for (int r = 0; r < NR; ++r)
    z[r] = reduce_d4((a[r][0][0] + a[r][0][1]) + (a[r][0][2] + a[r][0][3]),
                     (a[r][1][0] + a[r][1][1]) + (a[r][1][2] + a[r][1][3]),
                     (a[r][2][0] + a[r][2][1]) + (a[r][2][2] + a[r][2][3]),
                     (a[r][3][0] + a[r][3][1]) + (a[r][3][2] + a[r][3][3]));
}

// NH supports decoded together (z[h] = this lane's logits of support h, see support_logits):
// the reductions of support_decode sharing its two barriers. red: 12 * NH floats of LDS.
template <int NH>
__device__ __forceinline__ void support_decode_n(const float (*z)[3], float *red, float *out) {
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const bool ok2 = tid < 2 * kRTail && !(tid & 1);
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    float m = fmaxf(z[h][0], z[h][1]);
    if (ok2) m = fmaxf(m, z[h][2]);
    m = wave_max_dpp(m);
    if (lane == 0) red[4 * h + wid] = m;
  }
  __syncthreads();
  const float half = (float)((kRV - 1) / 2);
  const float j0 = (float)tid - half, j1 = (float)(kRT + tid) - half, j2 = (float)(2 * kRT + (tid >> 1)) - half;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const float M = fmaxf(fmaxf(red[4 * h], red[4 * h + 1]), fmaxf(red[4 * h + 2], red[4 * h + 3]));
    const float e0 = expf(z[h][0] - M), e1 = expf(z[h][1] - M), e2 = ok2 ? expf(z[h][2] - M) : 0.0f;
    float se = (e0 + e1) + e2, sj = (e0 * j0 + e1 * j1) + e2 * j2;
    se = wave_sum(se);
    sj = wave_sum(sj);
    if (lane == 0) {
      red[4 * NH + 8 * h + wid] = se;
      red[4 * NH + 8 * h + 4 + wid] = sj;
    }
  }
  __syncthreads();
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const float *q = red + 4 * NH + 8 * h;
    out[h] = h_inverse(((q[4] + q[5]) + (q[6] + q[7])) / ((q[0] + q[1]) + (q[2] + q[3])));
  }
}

// A parity-mode tie among unexpanded children resolved with its draw rr: the chosen child ends
// the path (cselect_child's list[rand() % len], cnode.cpp:592); one thread.
__device__ inline void resolve_tie(const TreeView &t, int A, int lvl, unsigned long long m, uint32_t rr, int *act) {
  int kk = (int)(rr % (uint32_t)__popcll(m));
  for (; kk > 0; --kk) m &= m - 1;
  const int jsel = __ffsll((long long)m) - 1;
  const int parent = t.path[lvl];
  const int action = legal_at(t, 0, parent, jsel);
  t.path_act[lvl] = action;
  t.path[lvl + 1] = 1 + A * t.meta[parent].latent + action;
  *act = action;
}

// Sum of the draw counts published by workgroups < g for simulation k, by the whole workgroup: one
// flag per thread (every poll in flight at once, not one round per 64 predecessors), reduced
// through LDS (part: kRWaves ints). Bounded spin; ends with a barrier.
__device__ inline int lookback_sum(const SearchArgs &p, int k, int g, int G, unsigned long long epoch, int *part) {
  const int lane = threadIdx.x & 63;
  int sum = 0;
  for (int q = threadIdx.x; q < g; q += kRT) {
    unsigned long long v;
    long long spins = 0;
    while (true) {
      v = __hip_atomic_load(&p.flags[(size_t)k * G + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((v >> 32) == epoch) break;
      if (++spins > (1ll << 22)) {
        atomicAdd(p.diag, 1);
        v = 0;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    sum += (int)(v & 0xffffffffu);
  }
  sum = xor_sum(sum);
  if (lane == 0) part[threadIdx.x >> 6] = sum;
  __syncthreads();
  return (part[0] + part[1]) + (part[2] + part[3]);
}

// lookback_sum by one wave, for G <= 256 workgroups: lane l polls roots l, l + 64, ... (all
// loads in flight at once), the sum by DPP (exact: float sums of integers < 2^24), no LDS and no
// barrier. Returns the sum in every lane of the calling wave. Every wave of the late draw calls it on
// its own, so a spin timeout is counted in p.diag once per wave that met it, and two waves may then
// disagree on the base; any count invalidates the whole search (lzm_check_errors raises at the result
// getters, the collector and bench.py), so such a search is never used.
__device__ inline int lookback_sum_w0(const SearchArgs &p, int k, int g, int G, unsigned long long epoch) {
  const int lane = threadIdx.x & 63;
  const unsigned long long ok = epoch << 32;  // a published flag of depth 0
  unsigned long long v[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = lane + 64 * j;
    v[j] = q < g ? __hip_atomic_load(&p.flags[(size_t)k * G + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : ok;
  }
  float sum = 0.0f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int q = lane + 64 * j;
    long long spins = 0;
    while ((v[j] >> 32) != epoch) {
      if (++spins > (1ll << 22)) {
        atomicAdd(p.diag, 1);
        v[j] = ok;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
      v[j] = __hip_atomic_load(&p.flags[(size_t)k * G + q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    sum += (float)(int)(v[j] & 0xffffffffu);
  }
  return (int)wave_sum(sum);
}

// The register walk's hand-off word (selection mode 5): the walk's whole outcome in 32 bits, written
// by lane 0 of wave 0 at the end of the walk and read once by every wave after the walk's barrier.
// status: 2 bits; len: 8; x: 8, signed; action: 8, signed (-1 at a tie). S + 2 <= 64 bounds all three.
__device__ __forceinline__ int hand_pack(int status, int len, int x, int action) {
  return (status & 3) | ((len & 0xff) << 2) | ((x & 0xff) << 10) | ((action & 0xff) << 18);
}
struct HandOff {
  int status, len, x, action;
};
__device__ __forceinline__ HandOff hand_unpack(int w) {
  HandOff h;
  h.status = w & 3;
  h.len = (w >> 2) & 0xff;
  h.x = (int)((unsigned)w << 14) >> 24;
  h.action = (int)((unsigned)w << 6) >> 24;
  return h;
}

// The tail of a mode-5 simulation on wave 0, from the hand-off's scalars (expand_wave_r, then
// backup_wave_r): expand_wave's part 1 (the leaf's own record) and backup_wave, with no read of
// pathlen or path[len] on the way. len, leaf and to_play are wave-uniform; len <= 62 (one round of
// backup_wave). Lane l holds level l: the path reads do not depend on len and are masked by it
// afterwards. The bootstrap chain runs leaf to root and the min-max update is a max / min, both in
// backup_wave's exact operation order.
struct TailPath {
  int node, pact;  // lane l: level l's node (0 past the leaf) and action
};
// the expansion: the path reads in flight, then the leaf's own record (the fields expand_wave's part 1
// changes), stored before backup_wave_r's reads of the same wave
__device__ inline TailPath expand_wave_r(const TreeView &t, int len, int leaf, int to_play, int latent, float reward) {
  const int lane = threadIdx.x & 63;
  const int lv = min(lane, t.depth_cap - 1);
  TailPath tp;
  tp.node = t.path[lv];
  tp.pact = t.path_act[lv];
  tp.node = lane <= len ? tp.node : 0;
  if (lane == 0) {
    t.meta[leaf].latent = latent;
    t.meta[leaf].to_play = to_play;
    t.stat[leaf].reward = reward;
  }
  return tp;
}
__device__ inline void backup_wave_r(const TreeView &t, const TailPath &tp, int len, int to_play, float value,
                                     float disc, float4 *mm_ptr) {
  const int lane = threadIdx.x & 63;
  const int node = tp.node;
  const bool act = lane <= len;
  if (lane < len) t.meta[node].best = tp.pact;
  NodeStat s = t.stat[node];
  const int ntp = t.meta[node].to_play;
  float b = value;  // wave-uniform chain value
  float bl = 0.0f;
  for (int j = len; j >= 0; --j) {
    if (lane == j) bl = b;
    const float tr = readlane_f(s.reward, j);
    if (to_play == -1) {
      b = tr + disc * b;
    } else {
      const int nj = __builtin_amdgcn_readlane(ntp, j);
      b = (nj == to_play) ? (-tr + disc * b) : (tr + disc * b);
    }
  }
  float qmax = -INFINITY, qmin = INFINITY;
  if (act) {
    if (to_play == -1 || ntp == to_play)
      s.value_sum += bl;
    else
      s.value_sum += -bl;
    s.visit += 1;
    t.stat[node] = s;
    const float v = node_value(s);
    if (t.val) t.val[node] = v;
    const float q = (to_play == -1) ? s.reward + disc * v : s.reward + disc * -v;
    qmax = fmaxf(qmax, q);
    qmin = fminf(qmin, q);
  }
  qmax = wave_max_dpp(qmax);
  qmin = -wave_max_dpp(-qmin);
  if (lane == 0) {
    float4 mm = *mm_ptr;
    if (qmax > mm.x) mm.x = qmax;
    if (qmin < mm.y) mm.y = qmin;
    *mm_ptr = mm;
  }
}

// SMODE: the selection mode (1, 4 or 5: see the simulation loop); RNG: 0 glibc, 1 Philox, -1 p.fast
// at run time; STAMPS: phase stamps compiled in (LZM_PHASE_TIMING). Production launches fix all
// three, so the unused paths cost neither code nor registers.
// The kernel's dynamic LDS plan (float offsets from the dynamic base): the two LDS weight layers
// first (their slot addresses become instruction immediates), then the tree slice, the selection
// tables and the optional pUCT visit table. cap / lut_n / depth_cap: the handle's capacities;
// S: simulations the selection tables hold. (A compile-time plan for the production handle, which
// frees ~45 scalar registers of offsets, measured even: the scalar spills are not on the path.)
// static LDS of the kernel, an upper bound: activations (counted as two full network rows; the
// kernel holds one plus the late draw's second T1 / NL row), biases, scalars (below 2 KiB)
constexpr int kResStaticBytes = (kRRow + 4 * kRRow + 2 * (4 * kRRow + kRF + 2 * kRF + kRMaxA) + kResBiasFloats) * 4 + 2048;
constexpr int kResMaxBytes = 160 * 1024 - kResStaticBytes;
__host__ __device__ constexpr int res_round4(int x) { return (x + 3) & ~3; }
__host__ __device__ constexpr ResPlan res_plan(int cap, int lut_n, int depth_cap, int S, int A) {
  ResPlan q{};
  int o = 0;
  q.wd1 = o; o += kRSlotsD * kRT * 4;
  q.wd2 = o; o += kRSlotsD * kRT * 4;
  q.stat = o; o += cap * 4;
  q.meta = o; o += cap * 4;
  q.lut = o; o += res_round4(2 * lut_n);
  q.legal = o; o += res_round4(A + 1);
  q.val = o; o += res_round4(cap);
  q.path = o; o += res_round4(depth_cap);
  q.pact = o; o += res_round4(depth_cap);
  q.act = o; o += A * kRHid;
  q.l2n = o; o += res_round4(S + 2);
  q.nq = o; o += res_round4(2 * (S + 2));
  q.cs = o; o += 4 * cap;
  q.dec = o; o += res_round4(S + 2);
  q.misc = o; o += res_round4(S + 32);
  const int tri = res_round4(lut_n * (lut_n + 1) / 2);
  q.pbt = o;
  q.pbt_rows = ((o + tri) * 4 <= kResMaxBytes && tri <= 8192) ? lut_n : 0;
  if (q.pbt_rows) o += tri;
  q.floats = o;
  return q;
}

template <int SMODE, int RNG, bool STAMPS>
__global__ __launch_bounds__(kRT) __attribute__((amdgpu_waves_per_eu(1, 1))) void search_res_kernel(SearchArgs p, ResNet n) {
  if (!STAMPS) p.phase = nullptr;
  if (RNG >= 0) p.fast = RNG;
  const ResPlan L = n.plan;
  static_assert(SMODE == 1 || SMODE == 4 || SMODE == 5, "selection modes: 1, 4, 5");
  if ((SMODE == 4 || SMODE == 5) && RNG == 0 && !STAMPS) n.spec_depth = 1;  // production parity kernel
  extern __shared__ float4 smem4[];
  float *smem = reinterpret_cast<float *>(smem4);
  const int tid = threadIdx.x, g = blockIdx.x, G = gridDim.x, lane = tid & 63, wid = tid >> 6;
  const int B = p.B, A = p.A;
  const int i = g;  // one root per workgroup
  unsigned long long stamp_ = p.phase ? __builtin_amdgcn_s_memtime() : 0ull;
  unsigned long long isub_ = stamp_;  // init sub-stamps (diagnostics)
#define LZM_ISTAMP(n)                                                      \
  do {                                                                     \
    if (p.phase && tid == 0) {                                             \
      const unsigned long long now_ = __builtin_amdgcn_s_memtime();       \
      s_phase[n] += (now_ - isub_) * (unsigned long long)p.S;              \
      isub_ = now_;                                                        \
    }                                                                      \
  } while (0)

  __shared__ uint32_t s_z0[31];
  __shared__ int s_players, s_epoch, s_x, s_act, s_status, s_tlevel, s_vtp;
  __shared__ int s_len[1], s_part[kRWaves], s_nlat;
  __shared__ int s_hand;  // (mode 5) the walk's hand-off word: hand_pack
  __shared__ unsigned long long s_tmask;
  __shared__ WalkState s_walk;
  __shared__ float4 s_mm;
  __shared__ float s_red[12 * 2];  // support_decode_n<2>: the reward and the value support
  __shared__ uint32_t s_dwin[64];  // the draw window: draw sums at stream positions s_dlo + 0..63
  __shared__ int s_dlo, s_base_prev;
  if (tid == 0) { s_dlo = -1000000; s_base_prev = 0; }
  __shared__ uint64_t s_exptab[32];  // glibc_expf's table: expand reads it from LDS (no vmcnt wait
                                     // on the weight prefetch in flight)
  if (threadIdx.x < 32) s_exptab[threadIdx.x] = kExp2fTab[threadIdx.x];
  __shared__ unsigned long long s_phase[64];
  if (p.phase && tid < 64) s_phase[tid] = 0ull;
  unsigned long long s_wait = 0ull;  // (thread 0) look-back wait cycles, diagnostics

  // ---- tree slice into LDS (node records, value cache, pUCT tables, legal list, path)
  TreeView t;
  t.A = A; t.cap = p.cap; t.lut_n = p.lut_n; t.depth_cap = p.depth_cap; t.B = 1;
  t.path = reinterpret_cast<int32_t *>(smem + L.path);
  t.path_act = reinterpret_cast<int32_t *>(smem + L.pact);
  t.pathlen = s_len;
  {
    NodeStat *ls = reinterpret_cast<NodeStat *>(smem + L.stat);
    NodeMeta *lm = reinterpret_cast<NodeMeta *>(smem + L.meta);
    float2 *llut = reinterpret_cast<float2 *>(smem + L.lut);
    int32_t *llegal = reinterpret_cast<int32_t *>(smem + L.legal);
    float *lval = smem + L.val;
    for (int e = tid; e < p.cap; e += kRT) {
      const NodeStat s = p.stat[(size_t)e * B + i];
      ls[e] = s;
      lm[e] = p.meta[(size_t)e * B + i];
      lval[e] = node_value(s);
    }
    for (int e = tid; e < p.lut_n; e += kRT) llut[e] = p.lut[e];
    float *lpbt = smem + L.pbt;
    build_pbt(p.lut, p.pbt_rows, lpbt, tid, kRT);
    for (int e = tid; e < A; e += kRT) llegal[e] = p.legal[(size_t)i * A + e];
    if (tid == 0) llegal[A] = p.nlegal[i];
    t.stat = ls; t.meta = lm; t.lut = llut; t.legal = llegal; t.nlegal = llegal + A; t.val = lval;
    t.pbt = p.pbt_rows ? lpbt : nullptr;
  }
  LZM_ISTAMP(24);
  // latent -> node map of the expanded nodes (children of latent L sit at 1 + A L)
  int *L2N = reinterpret_cast<int *>(smem + L.l2n);
  float2 *NQ = reinterpret_cast<float2 *>(smem + L.nq);
  int *DEC = reinterpret_cast<int *>(smem + L.dec);
  float4 *CS = reinterpret_cast<float4 *>(smem + L.cs);
  // A search starts from prepared roots: only the root is expanded, with latent 0 (cnode.cpp:
  // 301-358); simulation k gives its leaf latent k + 1. (Nodes past the root's children may hold a
  // previous search's records: never scan them.)
  for (int e = tid; e < p.S + 2; e += kRT) L2N[e] = e == 0 ? 0 : -1;
  if (tid == 0) s_nlat = 1;
  if (tid == 0) {
    s_mm = p.mm_fresh ? make_float4(kFloatMin, kFloatMax, p.mm_delta, 0.0f) : p.minmax[i];
    s_vtp = p.vtp_in[i];
    s_epoch = (int)__hip_atomic_load(p.epoch, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (wid == 0) {
    // players: 2 unless every root's to_play is -1 (max over the batch), by wave 0 with all its
    // loads in flight (a serial loop over B was ~30 K cycles of the launch)
    int m = INT_MIN;
    for (int q = lane; q < B; q += 64) m = max(m, p.vtp_in[q]);
    m = xor_max(m);
    if (lane == 0) s_players = (m == -1) ? 1 : 2;
  }
  uint32_t *s_seeds = reinterpret_cast<uint32_t *>(smem + L.misc);
  uint32_t *s_pow = s_seeds + p.S;
  if (p.step_count) {
    const long long c = *p.step_count;  // (read before the last workgroup's increment below)
    for (int e = tid; e < p.S; e += kRT) s_seeds[e] = (uint32_t)((p.step_base + c * (long long)p.S + e) % 1000000ll);
  } else {
    for (int e = tid; e < p.S; e += kRT) s_seeds[e] = p.seeds[e];
  }
  if (!p.fast)
    for (int e = tid; e < 31; e += kRT) s_pow[e] = p.pow16807[e];

  LZM_ISTAMP(25);
  // ---- network residency: LDS layers, action rows, register layers and biases
  // activations and biases at static LDS addresses: lane-dependent addresses then share a few base
  // registers and fold the arrays' offsets into the instructions' immediates
  // T1 / NL hold two rows: the two candidates of a leaf tie run the dynamics layers side by side
  // while the draw offset is still unknown (the late draw, see the simulation loop)
  __shared__ float4 s_acts[(kRRow + 4 * kRRow + 4 * kRRow + kRF + 2 * kRF + kRMaxA) / 4];
  __shared__ float4 s_bias[kResBiasFloats / 4];
  float *X0 = reinterpret_cast<float *>(s_acts), *T1 = X0 + kRRow, *NL = T1 + 2 * kRRow, *T2 = NL + 2 * kRRow,
        *T3 = T2 + kRRow, *U2 = T3 + kRRow, *U3 = U2 + kRRow, *RHo = U3 + kRRow, *HV = RHo + kRF, *LG = HV + 2 * kRF;
  float *ACT = smem + L.act;
  const float4 *WD1 = reinterpret_cast<const float4 *>(smem + L.wd1);
  const float4 *WD2 = reinterpret_cast<const float4 *>(smem + L.wd2);
  {
    // the two LDS layers, each thread's 16 + 16 slots loaded before any is stored (one round trip
    // per block instead of one per slot: the registers are free before the weights arrive)
    float4 st[kRSlotsD];
    res_fetch<kRSlotsD>(res_blk4(n, kRbD + 1), st);
#pragma unroll
    for (int j = 0; j < kRSlotsD; ++j) reinterpret_cast<float4 *>(smem + L.wd1)[j * kRT + tid] = st[j];
    res_fetch<kRSlotsD>(res_blk4(n, kRbD + 2), st);
#pragma unroll
    for (int j = 0; j < kRSlotsD; ++j) reinterpret_cast<float4 *>(smem + L.wd2)[j * kRT + tid] = st[j];
  }
  for (int e = tid; e < A * kRHid; e += kRT) ACT[e] = res_blk(n, kRbAct, A)[e];
  LZM_ISTAMP(26);
  float4 wD3[kRSlotsD], wD4[kRSlotsD], wRS[kRSlotsS], wRH[kRSlotsRH], wVPH[kRSlotsVPH], wPO[1];
  res_fetch<kRSlotsD>(res_blk4(n, kRbD + 3), wD3);
  res_fetch<kRSlotsD>(res_blk4(n, kRbD + 4), wD4);
  res_fetch<kRSlotsS>(res_blk4(n, kRbRS), wRS);
  res_fetch<kRSlotsRH>(res_blk4(n, kRbRH), wRH);
  res_fetch<kRSlotsVPH>(res_blk4(n, kRbVPH), wVPH);
  res_fetch<kRSlotsPO>(res_blk4(n, kRbPO), wPO);
  const int cD = d_col(), pD = tid & 1, cRH = tid >> 3, pRH = tid & 7, cVP = tid >> 2, pVP = tid & 3, cPO = tid >> 3;
  LZM_ISTAMP(27);
  // biases live in LDS (registers are the scarce resource): the bias blocks are contiguous
  float *BB = reinterpret_cast<float *>(s_bias);
  {
    constexpr int kNB = (kResBiasFloats + kRT - 1) / kRT;
    float bv[kNB];
    const float *bsrc = res_blk(n, kRbBD, A);
#pragma unroll
    for (int j = 0; j < kNB; ++j) bv[j] = j * kRT + tid < kResBiasFloats ? bsrc[j * kRT + tid] : 0.0f;
#pragma unroll
    for (int j = 0; j < kNB; ++j)
      if (j * kRT + tid < kResBiasFloats) BB[j * kRT + tid] = bv[j];
  }
  const float *BD = BB, *BRH = BD + 6 * kRHid, *BVP = BRH + kRF, *BRS = BVP + 2 * kRF,
              *BVS = BRS + ((kRV + 3) & ~3), *BPO = BVS + ((kRV + 3) & ~3);
  // the streamed buffer: fc_dynamics[0] for the first simulation
  float4 P[kRSlotsS];
  res_fetch<kRSlotsD>(res_blk4(n, kRbD), P);
#pragma unroll
  for (int j = kRSlotsD; j < kRSlotsS; ++j) P[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  __syncthreads();
  const int players = s_players;
  const unsigned long long epoch = (unsigned long long)(uint32_t)s_epoch;
  // the root's legal actions in registers (the two-action walks)
  int rleg[2];
  const int nleg = t.nlegal[0];
#pragma unroll
  for (int j = 0; j < 2; ++j) rleg[j] = j < A ? t.legal[j] : 0;
  LZM_ISTAMP(28);
  LZM_STAMP(10);

  for (int k = 0; k < p.S; ++k) {
    const uint32_t seed = s_seeds[k];
    // ---- selection, part 1: every expanded node's walk-independent pUCT terms (all threads), then
    // part 2, the walk over them (wave 0). SMODE, chosen on the host:
    //   1: the wave walk, one lane per child (descend_terms), any A;
    //   4: the two-action walk over the LDS tables (descend_a2f), A == 2 (else as 1);
    //   5: 4 with the terms pass and the walk on wave 0's registers (descend_a2r), A == 2, S + 2 <= 64.
    const bool regwalk = SMODE == 5;
    const int smode = regwalk ? 4 : (SMODE == 4 && A != 2) ? 1 : SMODE;
    A2Rec rc = {0, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    __syncthreads();  // the previous simulation's backup (wave 0) and children (wave 1) are complete
    if (regwalk) {
      // one node per lane, all in wave 0, which alone reads the records (registers) and, after the
      // walk's barrier, the tables: no barrier between the pass and the walk
      if (tid < s_nlat + k) node_terms_a2(t, tid, L2N, NQ, CS, s_mm, players, p.disc, DEC, rleg, nleg, &rc);
    } else {
      if (smode == 4)
        precompute_terms_a2(t, s_nlat + k, L2N, NQ, CS, s_mm, players, p.disc, DEC, rleg, nleg);
      else
        precompute_terms(t, s_nlat + k, L2N, NQ, CS, s_mm, players, p.disc);
      __syncthreads();
    }
    LZM_STAMP(12);
    if (wid != 0 && k > 0) res_fetch<kRSlotsD>(res_blk4(n, kRbD), P);  // (see the expand)
    // this simulation's glibc seed state (s_z0, read only after the walk) by wave 1 during wave 0's
    // walk (the post-walk barrier orders it for its readers)
    if (!p.fast && wid == 1) {
      const uint32_t sd = seed == 0 ? 1u : seed;
      if (sd < 0x7fffffffu) {
        if (lane < 31) {
          unsigned long long x = (unsigned long long)sd * s_pow[lane];
          unsigned long long r = (x & 0x7fffffffull) + (x >> 31);
          r = (r & 0x7fffffffull) + (r >> 31);
          if (r >= 0x7fffffffull) r -= 0x7fffffffull;
          s_z0[lane] = (uint32_t)r;
        }
      } else if (lane == 0) {
        glibc_seed_state(seed, s_z0);
      }
    }
    if (RNG != 1 && wid == 1) s_dwin[lane] = 0u;  // (the status-2 window's adds follow a barrier)
    // ---- selection, part 2: the walk (wave 0)
    if (wid == 0) {
      const float4 mm = s_mm;
      int w_status = 0, w_x = 0;  // (mode 5) the walk's status and x, wave-uniform
      if (p.fast) {
        auto draw = [seed, i](int level) -> uint32_t {
          uint4 o = philox4x32_10(make_uint4((uint32_t)level, (uint32_t)i, 0u, 0u), make_uint2(seed, 0x4c5a4d43u));
          return o.x >> 1;
        };
        Descent d;
        if (regwalk) {
          d = descend_a2r<false>(t, rc, terms_finite_a2r(rc, mm), mm, s_vtp, players, rleg, nleg, draw, nullptr);
          w_x = d.x;
        } else if (smode == 4) {
          d = descend_a2f<false>(t, NQ, DEC, CS, mm, s_vtp, players, rleg, nleg, draw, nullptr);
        } else if (smode == 1) {  // (smode is 4 or 1)
          d = descend_terms<false>(t, NQ, CS, mm, s_vtp, players, draw, nullptr);
        }
        if (lane == 0) {
          if (regwalk) {
            s_hand = hand_pack(0, d.len, d.x, d.action);
          } else {
            s_len[0] = d.len; s_x = d.x; s_act = d.action; s_status = 0;
          }
        }
      } else {
        TieInfo ti;
        auto nodraw = [](int) -> uint32_t { return 0u; };
        Descent d;
        if (regwalk) {
          WalkState ws;
          d = descend_a2r<true>(t, rc, terms_finite_a2r(rc, mm), mm, s_vtp, players, rleg, nleg, nodraw, &ti, &ws);
          LZM_STAMP(13);
          if (lane == 0 && ti.status == 2) s_walk = ws;
          w_status = ti.status;
          w_x = d.x;
        } else if (smode == 4) {
          WalkState ws;
          d = descend_a2f<true>(t, NQ, DEC, CS, mm, s_vtp, players, rleg, nleg, nodraw, &ti, &ws);
          LZM_STAMP(13);
          if (lane == 0 && ti.status == 2) s_walk = ws;
        } else if (smode == 1) {
          WalkState ws;
          d = descend_terms<true>(t, NQ, CS, mm, s_vtp, players, nodraw, &ti, nullptr, &ws);
          if (lane == 0 && ti.status == 2) s_walk = ws;
        }
        if (lane == 0) {
          // mode 5 hands the outcome over in one word; the separate scalars only where the status-2
          // resume reads them (every mode-5 simulation files s_len / s_x / s_act in its tail)
          if (regwalk) s_hand = hand_pack(ti.status, d.len, d.x, d.action);
          if (!regwalk || ti.status == 2) {
            s_len[0] = d.len; s_x = d.x; s_act = d.action;
            s_status = ti.status; s_tlevel = ti.level; s_tmask = ti.mask;
          }
          // publish this root's draw count at once (its depth is known unless status 2)
          if (ti.status != 2)
            __hip_atomic_store(&p.flags[(size_t)k * G + g], (epoch << 32) | (unsigned)d.len, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      // gather the leaf's parent latent now, by the walking wave, when the walk's x is final (every
      // status but 2; a status-2 root gathers after its draw resolution below): the walk's barrier
      // then also orders the gather (mode 5: straight from the walk's registers, no LDS round trip)
      if (!regwalk) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // lane 0's s_status / s_x to the wave
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
      const int stw = __builtin_amdgcn_readfirstlane(regwalk ? w_status : s_status);
      const int x0 = __builtin_amdgcn_readfirstlane(regwalk ? w_x : s_x);
      if (stw != 2 && lane < kRHid / 4)
        reinterpret_cast<float4 *>(X0)[lane + (lane >= kRHid / 8)] =
            reinterpret_cast<const float4 *>(p.pool + ((size_t)max(x0, 0) * B + i) * kRHid)[lane];
    }
    __syncthreads();
    LZM_STAMP(0);
    // (mode 5) the walk's outcome: one LDS read per wave, scalar from here on
    HandOff ho = {0, 0, 0, 0};
    if (regwalk) ho = hand_unpack(__builtin_amdgcn_readfirstlane(s_hand));
    const int status = regwalk ? ho.status : s_status;
    if (__builtin_expect(status == 2, 0)) {
      // the depth depends on a draw: look back now, then resume the walk at the tie with the draws
      // (exact semantics; the draws of the forced levels above the tie are never read). First
      // (A == 2), when every draw outcome gives the same depth (speculate_depth_a2), publish it at
      // once so that the roots after this one need not wait for this root's look-back (st = 3).
      int st = 2, d0 = -1;
      uint32_t sp_choice = ~0u, sp_ties = 0u;
      int sp_leaf = -1;
      unsigned long long sub_ = p.phase ? __builtin_amdgcn_s_memtime() : 0ull;
      if (smode == 4 && n.spec_depth && wid == 0) {
        const int de = speculate_depth_a2(t, NQ, DEC, CS, s_mm, rleg, nleg, s_walk, lane, &sp_choice, &sp_ties, &sp_leaf);
        d0 = __builtin_amdgcn_readfirstlane(de);
        if (d0 >= 0 && __ballot(de != d0) == 0ull) {
          st = 3;
          if (lane == 0)
            __hip_atomic_store(&p.flags[(size_t)k * G + g], (epoch << 32) | (unsigned)d0, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
      }
      LZM_SUBSTAMP(20);
      // the draw window: wave 0 alone waits for the look-back while waves 1-3 fill the window
      const bool win2 = RNG != 1 && smode == 4 && G <= kRT;
      int base = 0;
      if (win2) {
        if (wid == 0) {
          base = lookback_sum_w0(p, k, g, G, epoch);
        } else {
          const int lo = max(s_base_prev - kDwinBack, 0);
          dwin_add_part(p.coef, p.coef_positions, s_z0, lo, s_dwin, wid - 1);
          if (tid == 64) s_dlo = lo;
        }
        __syncthreads();
      } else {
        base = lookback_sum(p, k, g, G, epoch, s_part);
      }
      LZM_SUBSTAMP(21);
      if (wid == 0) {
        if (lane == 0) atomicAdd(p.diag + (st == 2 ? 1 : 2), 1);
        WalkState ws = s_walk;
        // the levels whose draws the resumed walk can read: below the speculated depth (st 3)
        const int hi = st == 3 ? d0 : t.depth_cap;
        bool need = true;
        uint32_t wv = 0u;
        if (win2) {
          bool miss;
          wv = window_draw(p.coef_positions, base, ws.len, hi, s_dwin, s_dlo, &miss);
          need = __ballot(miss) != 0ull;
          if (lane == 0) s_base_prev = base;
          if (p.phase && lane == 0 && need) s_phase[41] += 1;  // window misses (diagnostics)
        }
        if (need) {  // (lane_draws' rows)
          const int q = base + ws.len + lane;
          wv = 0u;
          if (ws.len + lane < hi && q < p.coef_positions) {
            const uint32_t *c = p.coef + (size_t)q * 31;
#pragma unroll
            for (int j = 0; j < 31; ++j) wv += c[j] * s_z0[j];
            wv >>= 1;
          }
        }
        const LaneDraws draw{p.coef, s_z0, p.diag, p.coef_positions, base, ws.len, wv};
        Descent d;
        // a speculated depth (st 3): the lane whose pattern agrees with the draws' parities at its tie
        // levels (lane l holds the draw of level ws.len + l); that lane's choice bits are the path, a
        // pointer chase instead of re-walking the tie subtree with scores
        int m = -1;
        uint32_t pch = 0u;
        if (st == 3 && smode == 4) {
          const unsigned long long par = __ballot((wv & 1u) != 0u);
          const bool ok = sp_choice != ~0u && ((sp_choice ^ (uint32_t)par) & sp_ties) == 0u;
          const unsigned long long okm = __ballot(ok);
          if (okm) {
            m = __ffsll((long long)okm) - 1;
            pch = (uint32_t)__builtin_amdgcn_readlane((int)sp_choice, m);
            const int lt = __builtin_amdgcn_readlane(sp_leaf, m);
            if (lt >= 0) pch = (pch & ~(1u << lt)) | ((uint32_t)(par >> lt) & 1u) << lt;
          }
        }
        if (m >= 0) {
          int node = ws.node, lat = ws.lat, len = ws.len, plat = ws.plat, last_action = ws.last_action;
          const int dmax = t.depth_cap - 1;
          while (lat >= 0 && len < dmax) {
            const bool root = node == 0;
            const int j = (int)((pch >> (len - ws.len)) & 1u);
            const int action = j ? (root ? rleg[1] : 1) : (root ? rleg[0] : 0);
            const int nnode = 1 + 2 * lat + action;
            const int nlat = __float_as_int(CS[nnode].z);
            if (lane == 0) {
              t.path_act[len] = action;
              t.path[len + 1] = nnode;
            }
            ++len;
            plat = lat;
            lat = nlat;
            node = nnode;
            last_action = action;
          }
          d.len = len;
          d.x = plat;
          d.action = last_action;
          d.vtp = 0;
          d.leaf = node;
        } else if (smode == 4)
          d = descend_a2<false>(t, NQ, DEC, CS, s_mm, s_vtp, players, rleg, nleg, draw, nullptr, &ws);
        else
          d = descend_terms<false>(t, NQ, CS, s_mm, s_vtp, players, draw, nullptr, &ws);
        if (lane == 0) {
          if (st == 3 && d.len != d0) {
            // cannot happen (the speculation walked every draw outcome); counted as an integrity error
            atomicAdd(p.diag, 1);
            atomicAdd(p.diag + 3, 1);
          }
          s_len[0] = d.len; s_x = d.x; s_act = d.action;
          if (regwalk) s_hand = hand_pack(2, d.len, d.x, d.action);  // the resumed walk's outcome
          if (st == 2)
            __hip_atomic_store(&p.flags[(size_t)k * G + g], (epoch << 32) | (unsigned)d.len, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
        // X0 by this wave (the barrier below orders it)
        const int x0 = __builtin_amdgcn_readfirstlane(d.x);
        if (lane < kRHid / 4)
          reinterpret_cast<float4 *>(X0)[lane + (lane >= kRHid / 8)] =
              reinterpret_cast<const float4 *>(p.pool + ((size_t)max(x0, 0) * B + i) * kRHid)[lane];
      }
      LZM_SUBSTAMP(22);
      __syncthreads();
      if (regwalk) ho = hand_unpack(__builtin_amdgcn_readfirstlane(s_hand));
      LZM_SUBSTAMP(23);
    }
    // X0 = pool[x][i], the leaf's parent latent, is in LDS: gathered by the walking wave
    LZM_STAMP(1);
    LZM_STAMP(2);  // (the separate gather phase this stamp closed is gone; the stamp indices stay)
    unsigned long long sub_ = p.phase ? __builtin_amdgcn_s_memtime() : 0ull;
    // ---- fc_dynamics[0], latent rows (streamed weights in P): shared by the late draw's two rows
    const float z0 = dense128(X0, [&](int j) { return P[j]; });
    // the stream buffer is free until the next pair's prefetch: stage fc_dynamics[1]'s LDS slots in
    // it now, so the layer below reads registers (its LDS reads in flight during the action rows)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < kRSlotsD; ++j) P[j] = WD1[j * kRT + tid];
    LZM_SUBSTAMP(16);
    // A tie between exactly two unexpanded children (status 1) takes the late draw: the two dynamics
    // layers run for both candidates (rows act_r[0], act_r[1] of T1 / NL, shared weight reads) and only
    // then the look-back is waited for, which by then has mostly been published; the draw picks the
    // next-latent row the rest of the network reads. Other leaf ties wait for their draw here.
    bool late = false;
    int act_r[2];
    // (mode 5) a status-1 tie is between the two children of the node at level len - 1 (mask 3): its
    // candidates are the root's legal actions there, else {0, 1}; all from the hand-off word
    const int tlevel = regwalk ? ho.len - 1 : 0;
    if (regwalk) {
      if (status == 1) {
        act_r[0] = tlevel == 0 ? rleg[0] : 0;
        act_r[1] = tlevel == 0 ? rleg[1] : 1;
        if (n.late_draw) {
          late = true;
        } else {
          // the draw now: every wave draws for itself (as the late pick does), one lane files the pick
          const int base = lookback_sum(p, k, g, G, epoch, s_part);
          const uint32_t rr = glibc_draw_wave(p.coef, p.coef_positions, s_z0, base + tlevel, p.diag);
          ho.action = (rr & 1u) ? act_r[1] : act_r[0];
          if (tid == 0) {
            t.path_act[tlevel] = ho.action;
            t.path[tlevel + 1] = 1 + 2 * ho.x + ho.action;
            s_act = ho.action;
          }
        }
      }
      if (!late) act_r[0] = act_r[1] = ho.action;
    } else if (status == 1) {
      const unsigned long long m = s_tmask;
      const int parent = t.path[s_tlevel];
      if (__popcll(m) == 2 && n.late_draw) {
        late = true;
        act_r[0] = legal_at(t, 0, parent, __ffsll((long long)m) - 1);
        act_r[1] = legal_at(t, 0, parent, __ffsll((long long)(m & (m - 1))) - 1);
      } else {
        const int base = lookback_sum(p, k, g, G, epoch, s_part);
        if (tid == 0) resolve_tie(t, A, s_tlevel, m, glibc_draw(p.coef, p.coef_positions, s_z0, base + s_tlevel, p.diag), &s_act);
        __syncthreads();
      }
    }
    if (!regwalk && !late) act_r[0] = act_r[1] = s_act;
    LZM_SUBSTAMP(17);
    __builtin_amdgcn_sched_barrier(0);
    // + the action's one-hot row, bias, ReLU (muzero_model_mlp.py:188-190)
    if (pD == 0) {
#pragma unroll
      for (int r = 0; r < 2; ++r)
        if (r < 1 || late) T1[r * kRRow + rpad(cD)] = fmaxf((z0 + ACT[act_r[r] * kRHid + cD]) + BD[cD], 0.0f);
    }
    __syncthreads();
    LZM_SUBSTAMP(18);
    // ---- fc_dynamics[1] (its weights staged in P) + latent residual -> next latent
    if (late) {
      float z[2];
      dense128n<2>(T1, [&](int j) { return P[j]; }, z);
      LZM_SUBSTAMP(32);
      if (pD == 0) {
#pragma unroll
        for (int r = 0; r < 2; ++r) NL[r * kRRow + rpad(cD)] = fmaxf(z[r] + BD[kRHid + cD], 0.0f) + X0[rpad(cD)];
      }
    } else {
      float z;
      dense128n<1>(T1, [&](int j) { return P[j]; }, &z);
      if (pD == 0) NL[rpad(cD)] = fmaxf(z + BD[kRHid + cD], 0.0f) + X0[rpad(cD)];
    }
    __syncthreads();
    LZM_SUBSTAMP(33);
    // the stream buffer is free again: stage fc_dynamics_2[0]'s LDS slots in it, every read issued
    // here, behind the barrier (in front of it the barrier would wait for them) and in front of the
    // look-back's first flag load, so a late draw's wait covers them; glibc_draw_wave's seed-state
    // read is the first LDS consumer behind them. Every path to the layer passes here.
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int j = 0; j < kRSlotsD; ++j) P[j] = WD2[j * kRT + tid];
    __builtin_amdgcn_sched_barrier(0);
    int lrow = 0;  // the late draw's pick: the two-way tie's second candidate when rand() % 2 == 1
    if (late) {
      const unsigned long long w0_ = p.phase ? __builtin_amdgcn_s_memtime() : 0ull;
      if (regwalk) {
        // the pick in closed form (resolve_tie over mask 3 at level len - 1, whose node holds latent
        // x): three stores from registers, ordered for the tail by the barriers below
        uint32_t rr;
        if (G <= kRT) {
          const int base = lookback_sum_w0(p, k, g, G, epoch);
          if (p.phase && tid == 0) s_wait += __builtin_amdgcn_s_memtime() - w0_;
          rr = glibc_draw_wave(p.coef, p.coef_positions, s_z0, base + tlevel, p.diag);
        } else {
          const int base = lookback_sum(p, k, g, G, epoch, s_part);
          if (p.phase && tid == 0) s_wait += __builtin_amdgcn_s_memtime() - w0_;
          rr = glibc_draw_wave(p.coef, p.coef_positions, s_z0, base + tlevel, p.diag);
        }
        lrow = (int)(rr & 1u);
        ho.action = lrow ? act_r[1] : act_r[0];
        if (tid == 0) {
          t.path_act[tlevel] = ho.action;
          t.path[tlevel + 1] = 1 + 2 * ho.x + ho.action;
          s_act = ho.action;
        }
      } else if (G <= kRT) {
        // every wave looks back and draws for itself, so no barrier hands the pick over; wave 0 files it
        const int base = lookback_sum_w0(p, k, g, G, epoch);
        if (p.phase && tid == 0) s_wait += __builtin_amdgcn_s_memtime() - w0_;
        const uint32_t rr = glibc_draw_wave(p.coef, p.coef_positions, s_z0, base + s_tlevel, p.diag);
        lrow = (int)(rr & 1u);  // (resolve_tie: rr % 2 over the mask's two set bits)
        if (tid == 0) resolve_tie(t, A, s_tlevel, s_tmask, rr, &s_act);
      } else {
        const int base = lookback_sum(p, k, g, G, epoch, s_part);
        if (p.phase && tid == 0) s_wait += __builtin_amdgcn_s_memtime() - w0_;
        if (tid == 0) resolve_tie(t, A, s_tlevel, s_tmask, glibc_draw(p.coef, p.coef_positions, s_z0, base + s_tlevel, p.diag), &s_act);
        __syncthreads();
        lrow = s_act == act_r[1] ? 1 : 0;
      }
    }
    // the next latent row the rest of the network reads (the late draw's pick)
    const float *NLb = NL + ((late && lrow) ? kRRow : 0);
    LZM_SUBSTAMP(34);
    LZM_STAMP(3);
    // The reward chain (fc_dynamics_2 -> reward head) and the prediction chain (prediction
    // common -> value / policy heads) both start from the next latent: one step per layer pair.
    // ---- [fc_dynamics_2[0] (LDS, staged in P above) | fc_prediction_common[0] (registers)]
    {
      float z2, z6;
      // fc_prediction_common[1] into P (used by the next pair): slot j behind this layer's slot j
      const __amdgpu_buffer_rsrc_t rd5 = wave_rsrc(res_blk4(n, kRbD + 5), kRSlotsD * kRT * 16);
      dense128n<1, true>(NLb, [&](int j) { return P[j]; }, &z2, [&](int j) {
        const f32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rd5, tid * 16, j * kRT * 16, 0);
        P[j] = make_float4(v.x, v.y, v.z, v.w);
      });
      LZM_SUBSTAMP(35);
      dense128n<1>(NLb, [&](int j) { return wD4[j]; }, &z6);
      LZM_SUBSTAMP(36);
      if (pD == 0) {
        T2[rpad(cD)] = fmaxf(z2 + BD[2 * kRHid + cD], 0.0f);
        U2[rpad(cD)] = fmaxf(z6 + BD[4 * kRHid + cD], 0.0f);
      }
    }
    __syncthreads();
    LZM_SUBSTAMP(19);
    // ---- [fc_prediction_common[1] (streamed) | fc_dynamics_2[1] (registers)]
    {
      float z7, z3;
      // the value support head into P (two steps on): slot j behind this layer's slot j, slots
      // 16-19 (free since the previous simulation's support_logits) behind the layer
      const __amdgpu_buffer_rsrc_t rvs = wave_rsrc(res_blk4(n, kRbVS), kRSlotsS * kRT * 16);
      auto fetch_vs = [&](int q) {
        const f32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rvs, tid * 16, q * kRT * 16, 0);
        P[q] = make_float4(v.x, v.y, v.z, v.w);
      };
      dense128n<1, true>(U2, [&](int j) { return P[j]; }, &z7, fetch_vs);
      LZM_SUBSTAMP(37);
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = kRSlotsD; q < kRSlotsS; ++q) fetch_vs(q);
      dense128n<1>(T2, [&](int j) { return wD3[j]; }, &z3);
      LZM_SUBSTAMP(38);
      __builtin_amdgcn_sched_barrier(0);
      if (pD == 0) {
        T3[rpad(cD)] = fmaxf(z3 + BD[3 * kRHid + cD], 0.0f);
        U3[rpad(cD)] = fmaxf(z7 + BD[5 * kRHid + cD], 0.0f);
      }
    }
    __syncthreads();
    LZM_SUBSTAMP(39);
    LZM_STAMP(4);
    // ---- [reward head hidden | (value | policy) head hidden]
    {
      float h = dot4<kRSlotsRH>(reinterpret_cast<const float4 *>(T3) + 4 * pRH + (pRH >= 4), [&](int j) { return wRH[j]; });
      float u = dot4<kRSlotsVPH>(reinterpret_cast<const float4 *>(U3) + 8 * pVP + (pVP >= 2), [&](int j) { return wVPH[j]; });
      h += dpp_f<0xB1>(h);
      u += dpp_f<0xB1>(u);
      h += dpp_f<0x4E>(h);
      u += dpp_f<0x4E>(u);
      h += dpp_f<0x141>(h);
      if (pRH == 0) RHo[cRH] = fmaxf(h + BRH[cRH], 0.0f);
      if (pVP == 0) HV[cVP] = fmaxf(u + BVP[cVP], 0.0f);
    }
    __syncthreads();
    LZM_STAMP(5);
    // ---- reward support (registers), value support (streamed), policy logits; both supports
    // decoded together
    float dec[2];  // [reward, value]
    {
      float zz[2][3];
      const float4 hp = reinterpret_cast<const float4 *>(HV + kRF)[tid & 7];
      float q = __fmaf_rn(hp.x, wPO[0].x, 0.0f);
      q = __fmaf_rn(hp.y, wPO[0].y, q);
      q = __fmaf_rn(hp.z, wPO[0].z, q);
      q = __fmaf_rn(hp.w, wPO[0].w, q);
      q += dpp_f<0xB1>(q);
      q += dpp_f<0x4E>(q);
      q += dpp_f<0x141>(q);
      if ((tid & 7) == 0 && cPO < A) LG[cPO] = q + BPO[cPO];
      support_logits(HV, P, BVS, zz[1][0], zz[1][1], zz[1][2]);
      __builtin_amdgcn_sched_barrier(0);
      support_logits(RHo, wRS, BRS, zz[0][0], zz[0][1], zz[0][2]);
      __builtin_amdgcn_sched_barrier(0);
      LZM_STAMP(15);
      support_decode_n<2>(zz, s_red, dec);
    }
    const float rdec = dec[0], vdec = dec[1];
    LZM_STAMP(6);
    LZM_STAMP(7);  // (the tie resolution this stamp closed is gone; the stamp indices stay)
    if (p.phase && tid == 0) sub_ = __builtin_amdgcn_s_memtime();
    // file the next latent (mcts_ctree.py:305): pool[k + 1][i], by wave 1 (wave 0 expands)
    if (tid >= 64 && tid < 64 + kRHid / 4)
      reinterpret_cast<float4 *>(p.pool + ((size_t)(k + 1) * B + i) * kRHid)[tid - 64] =
          reinterpret_cast<const float4 *>(NLb)[(tid - 64) + (tid - 64 >= kRHid / 8)];
    if (p.rec_x && tid == 0) {
      p.rec_x[(size_t)k * B + i] = regwalk ? ho.x : s_x;
      p.rec_a[(size_t)k * B + i] = regwalk ? ho.action : s_act;
      p.rec_len[(size_t)k * B + i] = regwalk ? ho.len : s_len[0];
    }
    if (p.rec_dec && tid == 0) {
      p.rec_dec[((size_t)k * B + i) * 2] = rdec;
      p.rec_dec[((size_t)k * B + i) * 2 + 1] = vdec;
      for (int a = 0; a < A; ++a) p.rec_logits[((size_t)k * B + i) * A + a] = LG[a];
    }
    // fc_dynamics[0] for the next simulation: wave 0 now, alone on the texture path (16 loads
    // issue in a few hundred cycles), waves 1-3 during the next walk, which only wave 0 runs
    LZM_SUBSTAMP(29);
    if (wid == 0) res_fetch<kRSlotsD>(res_blk4(n, kRbD), P);
    LZM_SUBSTAMP(30);
    // ---- expand + backup (cbatch_backpropagate, cnode.cpp:480-500): wave 0 files the leaf's own
    // record and backs up; wave 1 meanwhile initialises the leaf's children (disjoint nodes; the
    // next simulation's terms pass reads both after its barrier)
    if (regwalk && wid == 0) {
      // (mode 5) len, the leaf and its player from the hand-off's scalars: no s_len -> path[len] chain
      const int len = ho.len;
      const int leaf = len > 0 ? 1 + 2 * ho.x + ho.action : 0;
      int vtp = s_vtp;
      if (players > 1 && len > 0) {  // len flips: the first takes any value to 1 / 2, the rest alternate
        vtp = (vtp == 1) ? 2 : 1;
        if ((len - 1) & 1) vtp = (vtp == 1) ? 2 : 1;
      }
      LZM_SUBSTAMP(31);
      const TailPath tp = expand_wave_r(t, len, leaf, vtp, k + 1, rdec);
      LZM_STAMP(14);
      if (lane == 0) L2N[s_nlat + k] = leaf;  // the leaf now holds latent k + 1 (= s_nlat + k)
      backup_wave_r(t, tp, len, vtp, vdec, p.disc, &s_mm);
      // the separate scalars for the write-back (p.pathlen) and any reader of the last walk
      if (lane == 0) { s_len[0] = len; s_x = ho.x; s_act = ho.action; }
    } else if (wid == 0) {
      const int len = s_len[0];
      const int leaf = t.path[len];
      int vtp = s_vtp;
      if (players > 1)
        for (int l = 0; l < len; ++l) vtp = (vtp == 1) ? 2 : 1;
      LZM_SUBSTAMP(31);
      expand_wave(t, 0, leaf, vtp, k + 1, rdec, LG, -1, s_exptab, 1);
      LZM_STAMP(14);
      if (lane == 0) L2N[s_nlat + k] = leaf;  // the leaf now holds latent k + 1 (= s_nlat + k)
      backup_wave(t, 0, 0, 1, &s_mm, vtp, vdec, p.disc);
    } else if (wid == 1) {
      expand_wave(t, 0, 0, 0, k + 1, 0.0f, LG, -1, s_exptab, 2);
    }
    LZM_STAMP(9);
  }
  __syncthreads();
  LZM_STAMP(11);
  // ---- write back the slice (tree, min-max, last path)
  for (int e = tid; e < p.cap; e += kRT) {
    p.stat[(size_t)e * B + i] = t.stat[e];
    p.meta[(size_t)e * B + i] = t.meta[e];
  }
  for (int e = tid; e < p.depth_cap; e += kRT) {
    p.path[(size_t)e * B + i] = t.path[e];
    p.path_act[(size_t)e * B + i] = t.path_act[e];
  }
  if (tid == 0) {
    p.minmax[i] = s_mm;
    p.pathlen[i] = s_len[0];
  }
  // root outputs (root_outputs_kernel's values: visit counts per legal action, the root's value)
  if (p.out_dist && tid < A) {
    const int rl = t.meta[0].latent;
    p.out_dist[(size_t)i * A + tid] = (rl >= 0 && tid < t.nlegal[0]) ? t.stat[1 + A * rl + t.legal[tid]].visit : -1;
  }
  if (p.out_values && tid == 0) p.out_values[i] = node_value(t.stat[0]);
  __syncthreads();
  if (p.phase && tid < 64 && s_phase[tid]) atomicAdd(p.phase + tid, s_phase[tid]);
  if (p.phase && tid == 0 && g < 1024) atomicAdd(p.phase + 64 + g, s_wait);
  if (tid == 0) {
    // the last workgroup advances the epoch; no release fence (an L2 writeback per workgroup on
    // gfx950): the kernel boundary orders the write-back above for every later reader
    const uint32_t done = atomicAdd(p.epoch + 1, 1u);
    if (done == (uint32_t)G - 1) {
      p.epoch[1] = 0;
      __hip_atomic_store(p.epoch, (uint32_t)(epoch + 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (p.step_count && p.step_inc) *p.step_count += 1;  // every workgroup has read it (its seeds)
    }
  }
}

}  // namespace lzm
