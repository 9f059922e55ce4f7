/* Host check of div_small (lightzero_amd/csrc/lzm_numerics.h): the three-operation quotient
 *   y = RN(1/d), q0 = x * y, r = fmaf(-d, q0, x), q = fmaf(r, y, q0), and q0 itself where x is +-0, +-inf or NaN
 * against x / (float)d for d = 1, 2, 3, bit for bit (a NaN must stay a NaN).
 *
 *   div_small_check            every one of the 2^32 patterns of x, each divisor (minutes on one CPU)
 *   div_small_check --strided  every 251st pattern, every pattern with exponent field 0, 1, 254 or 255,
 *                              and +-0, +-inf and a NaN by name
 *
 * Build: cc -O2 -ffp-contract=off -o div_small_check tools/div_small_check.c -lm
 * (-ffp-contract=off as the library: the product x * y must round before the fused operations).
 * (add -fopenmp to spread the loops over the CPUs, -march=native to inline fmaf where the CPU has it)
 * Prints one line per divisor and "mismatches N"; exit status 1 when N != 0.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static float u2f(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
static uint32_t f2u(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

static float div_small(float x, int d) {
  const float y = d == 1 ? 1.0f : (d == 2 ? 0.5f : u2f(0x3EAAAAABu));
  const float q0 = x * y;
  const float r = fmaf(-(float)d, q0, x);
  const float q = fmaf(r, y, q0);
  const uint32_t u = f2u(x);
  const int special = (u & 0x7f800000u) == 0x7f800000u || (u << 1) == 0u;
  return special ? q0 : q;
}

/* the unguarded quotient, to count where the guard is needed */
static float div_core(float x, int d) {
  const float y = d == 1 ? 1.0f : (d == 2 ? 0.5f : u2f(0x3EAAAAABu));
  const float q0 = x * y;
  const float r = fmaf(-(float)d, q0, x);
  return fmaf(r, y, q0);
}

static int same(float a, float b) { return (isnan(a) && isnan(b)) || f2u(a) == f2u(b); }

/* bit 0: div_small differs from the division; bit 1: the unguarded quotient does (non-NaN x) */
static int check(uint32_t u, int d) {
  const float x = u2f(u), want = x / (float)d;
  return (same(div_small(x, d), want) ? 0 : 1) | ((isnan(x) || same(div_core(x, d), want)) ? 0 : 2);
}

int main(int argc, char **argv) {
  const int strided = argc > 1 && !strcmp(argv[1], "--strided");
  unsigned long long total = 0;
  for (int d = 1; d <= 3; ++d) {
    unsigned long long bad = 0, bad_core = 0, seen = 0;
#define CHECK(u)                  \
  do {                            \
    const int c_ = check((u), d); \
    bad += c_ & 1;                \
    bad_core += (c_ >> 1) & 1;    \
    ++seen;                       \
  } while (0)
    if (!strided) {
#pragma omp parallel for reduction(+ : bad, bad_core, seen)
      for (long long v = 0; v < (1ll << 32); ++v) CHECK((uint32_t)v);
    } else {
#pragma omp parallel for reduction(+ : bad, bad_core, seen)
      for (long long v = 0; v < (1ll << 32); v += 251) CHECK((uint32_t)v);
      const uint32_t exps[4] = {0u, 1u, 254u, 255u};
#pragma omp parallel for reduction(+ : bad, bad_core, seen)
      for (long long k = 0; k < (8ll << 23); ++k)  /* sign, exponent field, mantissa */
        CHECK(((uint32_t)(k >> 25) << 31) | (exps[(k >> 23) & 3] << 23) | ((uint32_t)k & 0x7fffffu));
      const uint32_t special[5] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u};
      for (int k = 0; k < 5; ++k) CHECK(special[k]);
    }
    printf("d %d: %llu patterns, %llu mismatches (unguarded, non-NaN x: %llu)\n", d, seen, bad, bad_core);
    total += bad;
  }
  printf("mismatches %llu\n", total);
  return total != 0;
}
