// lzm_numerics.h — bit-exact scalar numerics shared by the tree kernels (gfx950 device code).
//
// glibc_expf: the reference tree computes priors with the host libm expf
// (ctree_muzero/lib/cnode.cpp:129, float overload). On x86-64 glibc 2.35 dispatches to the
// FMA build of sysdeps/ieee754/flt-32/e_expf.c: a 32-entry 2^(k/32) table and a cubic in
// double precision. This is a restatement of that published algorithm with the same
// constants and the same fused multiply-adds; it equals host expf on every float in
// [-103.97, 0] (exhaustive check: tests/test_numerics.py, scripts under tests/).
//
// glibc rand(): srandom_r/random_r TYPE_3 (additive lagged Fibonacci, lags 31/3), used by
// cselect_child (cnode.cpp:592) after srand(tv_usec) (common_lib/utils.cpp:25).
//
// philox4x32_10: counter-based stream for the LZM_RNG_FAST mode (Salmon et al., SC'11).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lzm {

__device__ __constant__ static const uint64_t kExp2fTab[32] = {
    0x3ff0000000000000ull, 0x3fefd9b0d3158574ull, 0x3fefb5586cf9890full, 0x3fef9301d0125b51ull,
    0x3fef72b83c7d517bull, 0x3fef54873168b9aaull, 0x3fef387a6e756238ull, 0x3fef1e9df51fdee1ull,
    0x3fef06fe0a31b715ull, 0x3feef1a7373aa9cbull, 0x3feedea64c123422ull, 0x3feece086061892dull,
    0x3feebfdad5362a27ull, 0x3feeb42b569d4f82ull, 0x3feeab07dd485429ull, 0x3feea47eb03a5585ull,
    0x3feea09e667f3bcdull, 0x3fee9f75e8ec5f74ull, 0x3feea11473eb0187ull, 0x3feea589994cce13ull,
    0x3feeace5422aa0dbull, 0x3feeb737b0cdc5e5ull, 0x3feec49182a3f090ull, 0x3feed503b23e255dull,
    0x3feee89f995ad3adull, 0x3feeff76f2fb5e47ull, 0x3fef199bdd85529cull, 0x3fef3720dcef9069ull,
    0x3fef5818dcfba487ull, 0x3fef7c97337b9b5full, 0x3fefa4afa2a490daull, 0x3fefd0765b6e4540ull};

// tab: the 2^(k/32) table (kExp2fTab, or a copy of it in LDS: a kernel that keeps global loads
// in flight across the call then waits only for this LDS read, not for every outstanding load).
__device__ inline float glibc_expf(float x, const uint64_t *tab = kExp2fTab) {
  const double kInvLn2N = 0x1.71547652b82fep+5;  // 32/ln2
  const double kShift = 0x1.8p+52;
  const double C0 = 0x1.c6af84b912394p-20, C1 = 0x1.ebfce50fac4f3p-13, C2 = 0x1.62e42ff0c52d6p-6;
  uint32_t ux = __float_as_uint(x);
  uint32_t abstop = (ux >> 20) & 0x7ff;
  if (abstop >= 0x42b) {  // |x| >= 88 or x is nan
    if (ux == 0xff800000u) return 0.0f;
    if (abstop >= 0x7f8) return x + x;
    if (x > 0x1.62e42ep6f) return __uint_as_float(0x7f800000u);  // overflow
    if (x < -0x1.9fe368p6f) return 0.0f;                        // underflow
  }
  double xd = (double)x;
  double kd = __fma_rn(kInvLn2N, xd, kShift);
  uint64_t ki = (uint64_t)__double_as_longlong(kd);
  kd -= kShift;
  double r = __fma_rn(kInvLn2N, xd, -kd);
  uint64_t t = tab[ki % 32];
  t += ki << 47;
  double s = __longlong_as_double((long long)t);
  double z = __fma_rn(C0, r, C1);
  double r2 = r * r;
  double y = __fma_rn(C2, r, 1.0);
  y = __fma_rn(z, r2, y);
  y = y * s;
  return (float)y;
}

// glibc_logf: the Gumbel tree's csoftmax subtracts the host libm logf of its sum
// (ctree_gumbel_muzero/lib/cnode.cpp:931, float overload). glibc 2.35 on x86-64 dispatches to the FMA
// build of sysdeps/ieee754/flt-32/e_logf.c: a 16-entry {1/c, log c} table and a cubic in double
// precision. A restatement of that published algorithm with the same constants and the same fused
// multiply-adds, every input class included (1 -> +0, +-0 -> -inf, +inf, negative and NaN -> NaN,
// subnormals rescaled by 2^23). Checked on the host against libm (tools/gumbel_logf_check.c):
// every float in [1, 64] (the range the tree uses: sums of at most 64 terms in [0, 1], one of them 1)
// and in [0.5, 1], a stride over all other positive floats, the special classes; on the device by
// tests/test_gpu_gumbel.py.
__device__ __constant__ static const uint64_t kLogfTab[16][2] = {
#include "lzm_logf_tab.inc"
};

__device__ inline float glibc_logf(float x) {
  const double Ln2 = 0x1.62e42fefa39efp-1;
  const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
  uint32_t ix = __float_as_uint(x);
  if (ix == 0x3f800000u) return 0.0f;
  if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {  // x < 0x1p-126, inf or nan
    if (ix * 2 == 0) return -INFINITY;
    if (ix == 0x7f800000u) return x;
    if ((ix & 0x80000000u) || ix * 2 >= 0xff000000u) return __uint_as_float(0x7fc00000u);
    ix = __float_as_uint(x * 0x1p23f);  // subnormal: normalize
    ix -= 23u << 23;
  }
  const uint32_t tmp = ix - 0x3f330000u;
  const int i = (tmp >> 19) % 16;
  const int k = (int32_t)tmp >> 23;
  const uint32_t iz = ix - (tmp & 0xff800000u);
  const double invc = __longlong_as_double((long long)kLogfTab[i][0]);
  const double logc = __longlong_as_double((long long)kLogfTab[i][1]);
  const double z = (double)__uint_as_float(iz);
  const double r = __fma_rn(z, invc, -1.0);
  const double y0 = __fma_rn((double)k, Ln2, logc);
  const double r2 = r * r;
  double y = __fma_rn(A1, r, A2);
  y = __fma_rn(A0, r2, y);
  y = __fma_rn(y, r2, y0 + r);
  return (float)y;
}

// x / (float)d for d in {1, 2, 3} (the divisors of the two-action mean-q chain) without the IEEE
// division sequence: with y = RN(1/d), q0 = x * y, r = fma(-d, q0, x), q = fma(r, y, q0) is the
// correctly rounded quotient for every finite x but -0, subnormals included (f32 denormals are on in
// these kernels); +-inf give NaN (r is inf - inf) and -0 gives +0. For those and for a NaN, q0 itself
// is the quotient: +-inf, +-0, and a NaN stays a NaN. Same bits as the division for every non-NaN x
// (exhaustive check on the host: tools/div_small_check.c, tests/test_div_small.py). Explicit fmaf:
// the library is built -ffp-contract=off.
// A 32-bit literal in a scalar register at its point of use. The compiler otherwise materialises such a
// constant once in a vector register and keeps it there across the whole simulation loop, and the
// resident search kernel has no vector register to spare.
template <int C>
__device__ __forceinline__ int sgpr_literal() {
  int r;
  asm volatile("s_mov_b32 %0, %1" : "=s"(r) : "i"(C));
  return r;
}
__device__ __forceinline__ float div_small_y(int d) {
  // (selected as integers: scalar selects where d is uniform)
  return __uint_as_float(d == 1 ? 0x3F800000u : (d == 2 ? 0x3F000000u : 0x3EAAAAABu));
}
// the three operations alone (nd = -(float)d): for callers that check their operands themselves
__device__ __forceinline__ float div_small_core(float x, float y, float nd) {
  const float q0 = x * y;
  const float r = __fmaf_rn(nd, q0, x);
  return __fmaf_rn(r, y, q0);
}
__device__ __forceinline__ float div_small(float x, int d) {
  const float y = div_small_y(d);
  const float q0 = x * y;
  const float r = __fmaf_rn(-(float)d, q0, x);
  const float q = __fmaf_rn(r, y, q0);
  // +-0, +-inf, NaN (v_cmp_class_f32: sNaN 1, qNaN 2, -inf 4, -0 0x20, +0 0x40, +inf 0x200)
  return __builtin_amdgcn_classf(x, sgpr_literal<0x267>()) ? q0 : q;
}

// glibc srandom_r initial state (31 words) for `seed` (0 -> 1), Schrage's method.
__device__ inline void glibc_seed_state(uint32_t seed, uint32_t *z0) {
  if (seed == 0) seed = 1;
  int32_t word = (int32_t)seed;
  z0[0] = seed;
  for (int i = 1; i < 31; ++i) {
    long long hi = word / 127773;
    long long lo = word % 127773;
    long long w = 16807 * lo - 2836 * hi;
    if (w < 0) w += 2147483647;
    word = (int32_t)w;
    z0[i] = (uint32_t)word;
  }
}

__device__ inline uint4 philox4x32_10(uint4 ctr, uint2 key) {
  const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0 = __umulhi(M0, ctr.x), lo0 = M0 * ctr.x;
    uint32_t hi1 = __umulhi(M1, ctr.z), lo1 = M1 * ctr.z;
    ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
    key.x += W0;
    key.y += W1;
  }
  return ctr;
}

}  // namespace lzm
