// lzm_smz_conv_host.h — what the Stochastic MuZero conv step kernel (lzm_smz_conv.h) shares with its entry points
// in lzm_kernels.hip: the prepared weight layout, the step's arguments and the launcher. The kernel is its own
// translation unit (lzm_smz_conv.hip); lightzero_amd/build.py says why and how it is built.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lzm {

constexpr int kSmzLat = 64 * 16;  // a latent row: 64 channels x 4 x 4
constexpr int kSmzMaxV = 601;     // categorical support at most
constexpr int kSmzMaxPol = 64;    // action space and chance space at most
constexpr int kSmzBoards = 1;     // positions per workgroup by default

// One kind's weight set (float offsets from the set's start, every block 16-byte aligned). Set 0 serves decision
// leaves (dynamics_network + prediction_network), set 1 chance leaves (afterstate_dynamics_network +
// afterstate_prediction_network; its reward-head blocks stay zero and are never read). Heads: 0 reward, 1 value,
// 2 policy.
struct SmzConvLayout {
  int layers;      // 1 + 4 nres 64 -> 64 3x3 layers: the dynamics convolution, its blocks, the prediction's blocks
  int conv;        // frag [layer * 9 + tap][wave 4][4][lane 64][4] (lzm_az_c4_net.h's B fragments)
  int conv_b;      // [layers][64]
  int edge;        // [out 64][cell 16]: the option plane's taps that fall inside the board
  int hconv;       // 1x1 frag [head 3][k 16][lane 64]
  int hconv_b;     // [head 3][16]
  int fc1;         // [head 3][i 32][lane 64][4]: lane = 2 unit + half, inputs 128 half + 4 i ..
  int fc1_b;       // [head 3][32]
  int fc2_r, fc2_v, fc2_p;  // per head: W transposed [32][np] then the bias [np]
  int npv;         // the reward and value heads' padded output width np (a multiple of 64; the policy's: kSmzMaxPol)
  int set;         // floats per set
  int total;       // both sets
};

__host__ __device__ inline SmzConvLayout smz_conv_layout(int nres, int V) {
  SmzConvLayout L;
  int o = 0;
  auto take = [&](int n) { int r = o; o += (n + 3) & ~3; return r; };
  L.layers = 1 + 4 * nres;
  L.conv = take(L.layers * 9 * 4096); L.conv_b = take(L.layers * 64);
  L.edge = take(64 * 16);
  L.hconv = take(3 * 16 * 64); L.hconv_b = take(3 * 16);
  L.fc1 = take(3 * 32 * 64 * 4); L.fc1_b = take(3 * 32);
  L.npv = (V + 63) & ~63;
  L.fc2_r = take(33 * L.npv); L.fc2_v = take(33 * L.npv); L.fc2_p = take(33 * kSmzMaxPol);
  L.set = o;
  L.total = 2 * o;
  return L;
}

__host__ __device__ inline int smz_fc2_np(const SmzConvLayout &L, int head) { return head < 2 ? L.npv : kSmzMaxPol; }
__host__ __device__ inline int smz_fc2_at(const SmzConvLayout &L, int head) {
  return L.fc2_r + head * 33 * L.npv;  // (the blocks follow each other)
}

inline bool smz_conv_shape_ok(int nres, int A, int C, int V) {
  return (nres == 1 || nres == 2) && A >= 1 && A <= kSmzMaxPol && C >= 1 && C <= kSmzMaxPol && V >= 1 &&
         V <= kSmzMaxV && (V & 1);
}

struct SmzConvArgs {
  const float *w;            // smz_conv_layout's buffer
  const float *pool;         // [nslots][B][1024] latent pool
  const int32_t *x;          // [B] pool slot of root i's leaf latent
  const int32_t *option;     // [B] the action (chance leaf) or outcome (decision leaf) that led to the leaf
  const int32_t *is_chance;  // [B] leaf kind
  float *latent;             // [B][1024] next latent / afterstate
  float *value;              // [B][V]
  float *reward;             // [B][V], decision rows only
  float *policy_d;           // [B][A], decision rows only
  float *policy_c;           // [B][C], chance rows only
  int nslots, B, A, C, V;
};

// positions: per workgroup, 1 or 2 (0: the default)
hipError_t smz_conv_launch_step(int nres, int positions, const SmzConvArgs &a, hipStream_t s);

}  // namespace lzm
