// lzm_initial.h — MuZeroModelMLP.initial_inference in one launch (the collect step's first op).
//
// MuZeroPolicy._forward_collect (muzero.py:617-690) runs the model's initial_inference on the
// observations before every search: representation (muzero_model_mlp.py:145-177,
// common.py:467-517: Linear O->H, BatchNorm, GELU(tanh), Linear H->H, SimNorm over groups of 8)
// then prediction (common.py:883-971: two Linear+BN+ReLU, value head Linear+BN+ReLU -> Linear to
// the support, policy head Linear+BN+ReLU -> Linear to A). As PyTorch modules that is ~20 launches
// (GEMMs, eval BatchNorm, activations, softmax) of a few microseconds each around tiny matrices; at
// the bench shape it was ~1/8 of the whole collect step. Here one workgroup takes kIiEnvs envs (1:
// 256 workgroups at B = 256, 18.6 us; 4 envs per workgroup: 24 us),
// keeps their activations in LDS and runs every layer (BatchNorm folded on the host in float64):
// a layer of N outputs over K inputs maps thread t to column t % N and K slice t / N (N < 256) or
// to columns t, t + 256, ... (N >= 256); K slices are summed in slice order (deterministic).
// Weights: per layer W[K][N] (torch weight transposed) + bias[N], read straight from L2 with the
// k loop unrolled so a batch of loads is in flight. The resident search kernel's shape has a kernel of
// its own below (initial_fast_kernel): the same arithmetic with every weight loaded ahead into registers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lzm {

constexpr int kIiThreads = 256;
constexpr int kIiEnvs = 1;
constexpr int kIiMaxW = 1024;  // widest activation row kept in LDS (support <= 1024)
constexpr int kIiLayers = 9;   // R1 R2 | P1 P2 | V1 V2 | Q1 Q2 (+ spare)

struct IiArgs {
  int B, O, H, F, V, A, group;
  const float *obs;                       // [B][O]
  const float *w[kIiLayers], *b[kIiLayers];  // 0 R1 (O->H, GELU), 1 R2 (H->H), 2 P1, 3 P2 (H->H, ReLU),
                                          // 4 V1 (H->F, ReLU), 5 V2 (F->V), 6 Q1 (H->F, ReLU), 7 Q2 (F->A)
  float *latent, *value, *policy;         // [B][H], [B][V], [B][A]
};

__device__ inline float ii_act(float v, int act) {
  if (act == 1) return fmaxf(v, 0.0f);
  if (act == 2) {
    // GELU, tanh approximation (torch: 0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3))))
    const float kBeta = 0.7978845608028654f, kKappa = 0.044715f;
    const float inner = kBeta * (v + kKappa * v * v * v);
    return 0.5f * v * (1.0f + tanhf(inner));
  }
  return v;
}

// out[e][n] = act(sum_k in[e][k] W[k][n] + b[n]) for the workgroup's envs; in / out / part in LDS
__device__ inline void ii_dense(const float *__restrict__ W, const float *__restrict__ bias, int K, int N,
                                const float *in, int ldi, float *out, int ldo, int act, float *part) {
  const int t = threadIdx.x;
  if (N >= kIiThreads) {
    for (int n = t; n < N; n += kIiThreads) {
      float acc[kIiEnvs];
#pragma unroll
      for (int e = 0; e < kIiEnvs; ++e) acc[e] = 0.0f;
#pragma unroll 16
      for (int k = 0; k < K; ++k) {
        const float w = W[(size_t)k * N + n];
#pragma unroll
        for (int e = 0; e < kIiEnvs; ++e) acc[e] = __fmaf_rn(in[e * ldi + k], w, acc[e]);
      }
      const float b = bias[n];
#pragma unroll
      for (int e = 0; e < kIiEnvs; ++e) out[e * ldo + n] = ii_act(acc[e] + b, act);
    }
  } else {
    const int KS = kIiThreads / N;  // K slices
    const int Kc = (K + KS - 1) / KS;
    const int n = t % N, ks = t / N;
    if (ks < KS) {
      const int k0 = ks * Kc, k1 = min(K, k0 + Kc);
      float acc[kIiEnvs];
#pragma unroll
      for (int e = 0; e < kIiEnvs; ++e) acc[e] = 0.0f;
#pragma unroll 16
      for (int k = k0; k < k1; ++k) {
        const float w = W[(size_t)k * N + n];
#pragma unroll
        for (int e = 0; e < kIiEnvs; ++e) acc[e] = __fmaf_rn(in[e * ldi + k], w, acc[e]);
      }
#pragma unroll
      for (int e = 0; e < kIiEnvs; ++e) part[(ks * kIiEnvs + e) * N + n] = acc[e];
    }
    __syncthreads();
    for (int q = t; q < kIiEnvs * N; q += kIiThreads) {
      const int e = q / N, c = q - e * N;
      float s = 0.0f;
      for (int j = 0; j < KS; ++j) s += part[(j * kIiEnvs + e) * N + c];
      out[e * ldo + c] = ii_act(s + bias[c], act);
    }
  }
  __syncthreads();
}

// PREP: also CRoots::prepare for the workgroup's envs (prepare_root, lzm_tree.h) from the policy
// logits just written — the collect step's root preparation without a launch of its own.
template <bool PREP = false>
__global__ __launch_bounds__(kIiThreads) void initial_inference_kernel(IiArgs p, PrepareArgs q = PrepareArgs{}) {
  __shared__ float s_a[kIiEnvs * kIiMaxW], s_b[kIiEnvs * kIiMaxW], s_c[kIiEnvs * 256];
  __shared__ float s_part[kIiEnvs * kIiThreads];
  const int t = threadIdx.x;
  const int e0 = blockIdx.x * kIiEnvs;
  const int ne = min(kIiEnvs, p.B - e0);
  const int H = p.H;
  // PREP: the root's preparation inputs read at the start, into LDS / registers, so the tail below
  // is arithmetic and stores only (kIiEnvs == 1: the workgroup's root is e0)
  static_assert(!PREP || kIiEnvs == 1, "the fused preparation assumes one env per workgroup");
  __shared__ int s_leg[PREP ? kIiMaxW : 1];
  __shared__ float s_nz[PREP ? kIiMaxW : 1];
  int pr_n = 0, pr_tp = 0;
  float pr_rw = 0.0f;
  if (PREP) {
    const int A = q.A, cnt = q.count_in[e0];
    for (int j = t; j < A; j += kIiThreads) {
      s_leg[j] = cnt <= 0 ? j : (j < cnt ? q.legal_in[(size_t)e0 * A + j] : -1);
      s_nz[j] = q.noises ? q.noises[(size_t)e0 * A + j] : 0.0f;
    }
    pr_n = cnt <= 0 ? A : cnt;
    pr_tp = q.to_play[e0];
    pr_rw = q.rewards[e0];
  }
  for (int q = t; q < kIiEnvs * p.O; q += kIiThreads) {
    const int e = q / p.O, k = q - e * p.O;
    s_a[e * kIiMaxW + k] = e < ne ? p.obs[(size_t)(e0 + e) * p.O + k] : 0.0f;
  }
  __syncthreads();
  // representation: R1 (GELU) -> R2 -> SimNorm
  ii_dense(p.w[0], p.b[0], p.O, H, s_a, kIiMaxW, s_b, kIiMaxW, 2, s_part);
  ii_dense(p.w[1], p.b[1], H, H, s_b, kIiMaxW, s_a, kIiMaxW, 0, s_part);
  const int G = p.group;
  for (int q = t; q < kIiEnvs * (H / G); q += kIiThreads) {
    const int e = q / (H / G), g = q - e * (H / G);
    float *x = s_a + e * kIiMaxW + g * G;
    float m = x[0];
    for (int j = 1; j < G; ++j) m = fmaxf(m, x[j]);
    float s = 0.0f;
    for (int j = 0; j < G; ++j) s += expf(x[j] - m);
    for (int j = 0; j < G; ++j) x[j] = expf(x[j] - m) / s;
  }
  __syncthreads();
  for (int q = t; q < ne * H; q += kIiThreads) {
    const int e = q / H, k = q - e * H;
    p.latent[(size_t)(e0 + e) * H + k] = s_a[e * kIiMaxW + k];
  }
  // prediction: P1, P2 (ReLU) -> value head, policy head
  ii_dense(p.w[2], p.b[2], H, H, s_a, kIiMaxW, s_b, kIiMaxW, 1, s_part);
  ii_dense(p.w[3], p.b[3], H, H, s_b, kIiMaxW, s_a, kIiMaxW, 1, s_part);
  ii_dense(p.w[4], p.b[4], H, p.F, s_a, kIiMaxW, s_c, 256, 1, s_part);
  ii_dense(p.w[5], p.b[5], p.F, p.V, s_c, 256, s_b, kIiMaxW, 0, s_part);
  for (int q = t; q < ne * p.V; q += kIiThreads) {
    const int e = q / p.V, k = q - e * p.V;
    p.value[(size_t)(e0 + e) * p.V + k] = s_b[e * kIiMaxW + k];
  }
  ii_dense(p.w[6], p.b[6], H, p.F, s_a, kIiMaxW, s_c, 256, 1, s_part);
  ii_dense(p.w[7], p.b[7], p.F, p.A, s_c, 256, s_b, kIiMaxW, 0, s_part);
  for (int q = t; q < ne * p.A; q += kIiThreads) {
    const int e = q / p.A, k = q - e * p.A;
    p.policy[(size_t)(e0 + e) * p.A + k] = s_b[e * kIiMaxW + k];
  }
  if (PREP) {
    // CRoots::prepare for root i = e0, the same operations in the same order as prepare_root
    // (lzm_tree.h), with the legal list, noises and policy logits read from LDS
    const int i = e0, A = q.A, n = pr_n;
    for (int j = t; j < A; j += kIiThreads) q.legal[(size_t)i * A + j] = s_leg[j];
    if (t == 0) {
      q.nlegal[i] = n;
      const float *lg = s_b;  // this env's policy logits (e = 0)
      float pmax = kFloatMin;
      for (int j = 0; j < n; ++j) {
        const float l = lg[s_leg[j]];
        if (pmax < l) pmax = l;
      }
      float sum = 0.0f;
      for (int j = 0; j < n; ++j) sum += glibc_expf(lg[s_leg[j]] - pmax);
      const float f = q.noise_weight;
      for (int j = 0; j < n; ++j) {
        const int a = s_leg[j];
        float prior = glibc_expf(lg[a] - pmax) / sum;
        if (q.noises) prior = prior * (1 - f) + s_nz[j] * f;
        NodeStat c;
        c.visit = 0; c.value_sum = 0.0f; c.prior = prior; c.reward = 0.0f;
        q.stat[(size_t)(1 + a) * q.B + i] = c;
        NodeMeta cm;
        cm.latent = -1; cm.to_play = 0; cm.best = -1; cm.is_reset = 0;
        q.meta[(size_t)(1 + a) * q.B + i] = cm;
      }
      NodeStat r;
      r.visit = 1; r.value_sum = 0.0f; r.prior = 0.0f; r.reward = pr_rw;
      q.stat[i] = r;
      NodeMeta rm;
      rm.latent = 0; rm.to_play = pr_tp; rm.best = -1; rm.is_reset = 0;
      q.meta[i] = rm;
    }
  }
}

// ---- The shape of the resident search kernel (H 128, F 32, V 601, SimNorm 8; A <= 32, O <= 16) ----
//
// initial_fast_kernel computes what initial_inference_kernel computes, bit for bit: ii_dense's map of
// columns and K slices to threads, one __fmaf_rn chain from 0.0f over the slice in ascending k, the
// slices added in slice order from 0.0f, + bias, ii_act; the same SimNorm and preparation tail. What
// changes is where the operands come from. No weight address depends on data, so a thread's whole
// share of the weights (80 float4 + a few scalars) is loaded into compile-time-indexed registers in
// three stages, each issued at least two layers ahead of its use, the first before anything else;
// ii_dense instead reads a layer from L2 inside its FMA loop, after the previous layer's barrier
// (~22 dependent trips at this shape). The float4 loads come from a second copy of the six wide
// layers in [slot][thread] order (kIfBlockFloats, packed by initial.py after the generic layout):
// slot s of thread t holds 4 consecutive k of the thread's column.
constexpr int kIfH = 128, kIfF = 32, kIfV = 601, kIfG = 8, kIfMaxA = 32, kIfMaxO = 16;
constexpr int kIfR1 = (kIfMaxO + 1) / 2;  // R1: 2 K slices of ceil(O / 2)
constexpr int kIfQ2 = 4;                  // Q2: 256 / A K slices of ceil(F / (256 / A)) <= 4 for A <= 32
constexpr int kIfHS = kIfH / 2 / 4;       // float4 slots of an H -> H layer (2 K slices of 64): 16
constexpr int kIfFS = kIfH / 8 / 4;       // of an H -> F layer (8 K slices of 16): 4
constexpr int kIfVC = (kIfV + kIiThreads - 1) / kIiThreads;  // V2: columns t, t + 256, t + 512
constexpr int kIfVS = kIfVC * (kIfF / 4);                    // 24 slots, 8 per column (zeros past V)
// float4 offsets of the layers in the fast block: R2 P1 P2 | V1 Q1 | V2
constexpr int kIfOffR2 = 0, kIfOffP1 = kIfHS * kIiThreads, kIfOffP2 = 2 * kIfHS * kIiThreads;
constexpr int kIfOffV1 = 3 * kIfHS * kIiThreads, kIfOffQ1 = kIfOffV1 + kIfFS * kIiThreads;
constexpr int kIfOffV2 = kIfOffQ1 + kIfFS * kIiThreads;
constexpr int kIfBlockFloats = 4 * (kIfOffV2 + kIfVS * kIiThreads);  // 81920

constexpr int ii_q2_slice(int A) { return (kIfF + kIiThreads / A - 1) / (kIiThreads / A); }
static_assert(ii_q2_slice(kIfMaxA) == kIfQ2 && ii_q2_slice(26) == kIfQ2 && ii_q2_slice(1) == 1, "Q2 K slice");

template <int S>
__device__ inline void ii_fast_issue(float4 (&w)[S], const float4 *__restrict__ blk, int t) {
#pragma unroll
  for (int s = 0; s < S; ++s) w[s] = blk[s * kIiThreads + t];
}

// the slice's chain: in (LDS, 16-byte aligned) holds the slice's inputs in ascending k
template <int S>
__device__ inline float ii_fast_chain(const float4 (&w)[S], const float *in) {
  float acc = 0.0f;
#pragma unroll
  for (int s = 0; s < S; ++s) {
    const float4 x = *reinterpret_cast<const float4 *>(in + 4 * s);
    acc = __fmaf_rn(x.x, w[s].x, acc);
    acc = __fmaf_rn(x.y, w[s].y, acc);
    acc = __fmaf_rn(x.z, w[s].z, acc);
    acc = __fmaf_rn(x.w, w[s].w, acc);
  }
  return acc;
}

template <int KS>
__device__ inline float ii_fast_sum(const float *part, int N, int c) {
  float s = 0.0f;
#pragma unroll
  for (int j = 0; j < KS; ++j) s += part[j * N + c];
  return s;
}

template <bool PREP>
__global__ __launch_bounds__(kIiThreads) void initial_fast_kernel(IiArgs p, const float4 *__restrict__ fw,
                                                                  PrepareArgs q) {
  __shared__ __attribute__((aligned(16))) float s_x[kIfH], s_y[kIfH], s_v[kIfF], s_q[kIfF];
  __shared__ float s_part[kIiThreads], s_part2[kIiThreads], s_pol[kIfMaxA], s_nz[kIfMaxA];
  __shared__ int s_leg[kIfMaxA];
  const int t = threadIdx.x, e0 = blockIdx.x, O = p.O, A = p.A;
  const int nh = t & (kIfH - 1), ksh = t >> 7;  // column and K slice in the H-wide layers
  const int nf = t & (kIfF - 1), ksf = t >> 5;  // in V1 and Q1
  // ---- stage 0, in order of use (the scheduling barriers keep the layers in this order, so that the
  // wait for one layer's registers leaves the later layers in flight): R1 with its inputs, R2, P1,
  // P2, the biases, the preparation inputs
  const int Kc1 = (O + 1) >> 1, k10 = ksh * Kc1, k11 = min(O, k10 + Kc1);
  float w1[kIfR1], x1[kIfR1];
#pragma unroll
  for (int i = 0; i < kIfR1; ++i) {
    const int k = min(k10 + i, O - 1);  // (past the slice: loaded, not used)
    w1[i] = p.w[0][k * kIfH + nh];
    x1[i] = p.obs[(size_t)e0 * O + k];
  }
  const float b0 = p.b[0][nh];
  __builtin_amdgcn_sched_barrier(0);
  float4 w2[kIfHS], w3[kIfHS], w4[kIfHS];
  ii_fast_issue(w2, fw + kIfOffR2, t);
  const float b1 = p.b[1][nh];
  __builtin_amdgcn_sched_barrier(0);
  ii_fast_issue(w3, fw + kIfOffP1, t);
  const float b2 = p.b[2][nh];
  __builtin_amdgcn_sched_barrier(0);
  ii_fast_issue(w4, fw + kIfOffP2, t);
  const float b3 = p.b[3][nh], b4 = p.b[4][nf], b6 = p.b[6][nf], b7 = p.b[7][min(t, A - 1)];
  float b5[kIfVC];
#pragma unroll
  for (int j = 0; j < kIfVC; ++j) b5[j] = p.b[5][min(t + j * kIiThreads, kIfV - 1)];
  // the preparation inputs, every load unconditional: the legal row is [A] whatever the count (what it
  // means is decided where it is stored, below), and without noises a bias stands in, never read back
  int pr_cnt = 0, pr_tp = 0, pr_li = 0;
  float pr_rw = 0.0f, pr_nz = 0.0f;
  if (PREP) {
    const int j = min(t, A - 1);
    const float *nz = q.noises ? q.noises + (size_t)e0 * A + j : p.b[7];
    pr_li = q.legal_in[(size_t)e0 * A + j];
    pr_nz = *nz;
    pr_cnt = q.count_in[e0];
    pr_tp = q.to_play[e0];
    pr_rw = q.rewards[e0];
  }
  __builtin_amdgcn_sched_barrier(0);
  // ---- representation: R1 (GELU) -> R2 -> SimNorm
  {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < kIfR1; ++i)
      if (k10 + i < k11) acc = __fmaf_rn(x1[i], w1[i], acc);
    s_part[t] = acc;
  }
  __syncthreads();
  if (t < kIfH) s_x[t] = ii_act(ii_fast_sum<2>(s_part, kIfH, t) + b0, 2);
  __syncthreads();
  s_part[t] = ii_fast_chain(w2, s_x + ksh * (kIfH / 2));
  __syncthreads();
  if (t < kIfH) s_y[t] = ii_fast_sum<2>(s_part, kIfH, t) + b1;
  // ---- stage 1 (w2's registers are free): V1, Q1 and Q2, used after P1 and P2
  float4 w5[kIfFS], w7[kIfFS];
  ii_fast_issue(w5, fw + kIfOffV1, t);
  ii_fast_issue(w7, fw + kIfOffQ1, t);
  const int KS8 = kIiThreads / A, Kc8 = (kIfF + KS8 - 1) / KS8;
  const int n8 = t % A, ks8 = t / A, k80 = ks8 * Kc8, k81 = min(kIfF, k80 + Kc8);
  float w8[kIfQ2];
#pragma unroll
  for (int i = 0; i < kIfQ2; ++i) w8[i] = p.w[7][min(k80 + i, kIfF - 1) * A + n8];
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();
  if (t < kIfH) {
    // the SimNorm of the thread's own element: its group's maximum and sum in the group's order
    const float *x = s_y + (t & ~(kIfG - 1));
    float m = x[0];
#pragma unroll
    for (int j = 1; j < kIfG; ++j) m = fmaxf(m, x[j]);
    float s = 0.0f;
#pragma unroll
    for (int j = 0; j < kIfG; ++j) s += expf(x[j] - m);
    const float l = expf(s_y[t] - m) / s;
    s_x[t] = l;
    p.latent[(size_t)e0 * kIfH + t] = l;
  }
  __syncthreads();
  // ---- prediction: P1, P2 (ReLU) -> value head, policy head
  s_part[t] = ii_fast_chain(w3, s_x + ksh * (kIfH / 2));
  __syncthreads();
  if (t < kIfH) s_y[t] = ii_act(ii_fast_sum<2>(s_part, kIfH, t) + b2, 1);
  // ---- stage 2 (w3's registers are free): V2, used after P2 and V1
  float4 w6[kIfVS];
  ii_fast_issue(w6, fw + kIfOffV2, t);
  __builtin_amdgcn_sched_barrier(0);
  __syncthreads();
  s_part[t] = ii_fast_chain(w4, s_y + ksh * (kIfH / 2));
  __syncthreads();
  if (t < kIfH) s_x[t] = ii_act(ii_fast_sum<2>(s_part, kIfH, t) + b3, 1);
  __syncthreads();
  // V1 and Q1 read the same row: both between one pair of barriers, reduced by waves 0 and 1
  s_part[t] = ii_fast_chain(w5, s_x + ksf * (kIfH / 8));
  s_part2[t] = ii_fast_chain(w7, s_x + ksf * (kIfH / 8));
  __syncthreads();
  if (t < kIfF) s_v[t] = ii_act(ii_fast_sum<8>(s_part, kIfF, t) + b4, 1);
  if (t >= 64 && t < 64 + kIfF) s_q[t - 64] = ii_act(ii_fast_sum<8>(s_part2, kIfF, t - 64) + b6, 1);
  __syncthreads();
  // V2 (one thread per column, no slices) straight to memory, and Q2's slices
#pragma unroll
  for (int j = 0; j < kIfVC; ++j) {
    float4 wv[kIfF / 4];
#pragma unroll
    for (int s = 0; s < kIfF / 4; ++s) wv[s] = w6[j * (kIfF / 4) + s];
    const int n = t + j * kIiThreads;
    const float v = ii_fast_chain(wv, s_v) + b5[j];
    if (n < kIfV) p.value[(size_t)e0 * kIfV + n] = v;
  }
  if (ks8 < KS8) {
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < kIfQ2; ++i)
      if (k80 + i < k81) acc = __fmaf_rn(s_q[min(k80 + i, kIfF - 1)], w8[i], acc);
    s_part[t] = acc;  // (ks8 * A + n8 == t)
  }
  if (PREP && t < A) {
    const int leg = pr_cnt <= 0 ? t : (t < pr_cnt ? pr_li : -1);
    s_leg[t] = leg;
    s_nz[t] = pr_nz;
    q.legal[(size_t)e0 * A + t] = leg;
  }
  __syncthreads();
  if (t < A) {
    // slices from ceil(F / Kc8) on are empty: each holds +0.0f, and adding it changes no bit, since a
    // sum that started from +0.0f is never -0.0f
    const int used = (kIfF + Kc8 - 1) / Kc8;
    float s = 0.0f;
    for (int j = 0; j < used; ++j) s += s_part[j * A + t];
    const float l = s + b7;
    p.policy[(size_t)e0 * A + t] = l;
    if (PREP) s_pol[t] = l;
  }
  if (PREP) {
    __syncthreads();
    // CRoots::prepare for root i = e0: initial_inference_kernel's tail, operation for operation
    if (t == 0) {
      const int i = e0, n = pr_cnt <= 0 ? A : pr_cnt;
      q.nlegal[i] = n;
      const float *lg = s_pol;
      float pmax = kFloatMin;
      for (int j = 0; j < n; ++j) {
        const float l = lg[s_leg[j]];
        if (pmax < l) pmax = l;
      }
      float sum = 0.0f;
      for (int j = 0; j < n; ++j) sum += glibc_expf(lg[s_leg[j]] - pmax);
      const float f = q.noise_weight;
      for (int j = 0; j < n; ++j) {
        const int a = s_leg[j];
        float prior = glibc_expf(lg[a] - pmax) / sum;
        if (q.noises) prior = prior * (1 - f) + s_nz[j] * f;
        NodeStat c;
        c.visit = 0; c.value_sum = 0.0f; c.prior = prior; c.reward = 0.0f;
        q.stat[(size_t)(1 + a) * q.B + i] = c;
        NodeMeta cm;
        cm.latent = -1; cm.to_play = 0; cm.best = -1; cm.is_reset = 0;
        q.meta[(size_t)(1 + a) * q.B + i] = cm;
      }
      NodeStat r;
      r.visit = 1; r.value_sum = 0.0f; r.prior = 0.0f; r.reward = pr_rw;
      q.stat[i] = r;
      NodeMeta rm;
      rm.latent = 0; rm.to_play = pr_tp; rm.best = -1; rm.is_reset = 0;
      q.meta[i] = rm;
    }
  }
}

}  // namespace lzm
