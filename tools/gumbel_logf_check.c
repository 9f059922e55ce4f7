/* One-off host check of the glibc logf port in lightzero_amd/csrc/lzm_numerics.h (glibc_logf): the same
 * operations, compiled for the host with explicit fma(), against the host libm's logf on EVERY float in
 * [1, 64] (the range the Gumbel tree's csoftmax calls it on: sums of up to 64 terms in [0, 1] with one term
 * equal to 1), then on a stride over all positive normal floats, the subnormals and the special classes.
 *
 *   cc -O2 -ffp-contract=off tools/gumbel_logf_check.c -lm -o /tmp/gumbel_logf_check && /tmp/gumbel_logf_check
 *
 * Prints the mismatch counts; exit status 0 when all are zero. Result noted in DESIGN.md §5.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

static const uint64_t kTab[16][2] = {
#include "../lightzero_amd/csrc/lzm_logf_tab.inc"
};

static double asd(uint64_t u) { double d; memcpy(&d, &u, 8); return d; }
static uint32_t asu(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static float asf(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }

static float port_logf(float x) {
  const double Ln2 = 0x1.62e42fefa39efp-1;
  const double A0 = -0x1.00ea348b88334p-2, A1 = 0x1.5575b0be00b6ap-2, A2 = -0x1.ffffef20a4123p-2;
  uint32_t ix = asu(x);
  if (ix == 0x3f800000u) return 0.0f;
  if (ix - 0x00800000u >= 0x7f800000u - 0x00800000u) {
    if (ix * 2 == 0) return -INFINITY;
    if (ix == 0x7f800000u) return x;
    if ((ix & 0x80000000u) || ix * 2 >= 0xff000000u) return NAN;
    ix = asu(x * 0x1p23f);
    ix -= 23u << 23;
  }
  const uint32_t tmp = ix - 0x3f330000u;
  const int i = (tmp >> 19) % 16;
  const int k = (int32_t)tmp >> 23;
  const uint32_t iz = ix - (tmp & 0xff800000u);
  const double invc = asd(kTab[i][0]), logc = asd(kTab[i][1]);
  const double z = (double)asf(iz);
  const double r = fma(z, invc, -1.0);
  const double y0 = fma((double)k, Ln2, logc);
  const double r2 = r * r;
  double y = fma(A1, r, A2);
  y = fma(A0, r2, y);
  y = fma(y, r2, y0 + r);
  return (float)y;
}

static long check(uint32_t lo, uint32_t hi, uint32_t stride, const char *what) {
  long bad = 0, n = 0;
  for (uint64_t u = lo; u <= hi; u += stride, ++n) {
    const float x = asf((uint32_t)u);
    const float a = port_logf(x), b = logf(x);
    if (asu(a) != asu(b) && !(a != a && b != b)) {
      if (bad < 5) printf("  mismatch x=%a port=%a libm=%a\n", x, a, b);
      ++bad;
    }
  }
  printf("%s: %ld values, %ld mismatches\n", what, n, bad);
  return bad;
}

int main(void) {
  long bad = 0;
  bad += check(0x3f800000u, 0x42800000u, 1, "[1, 64] exhaustive");
  bad += check(0x00800000u, 0x7f7fffffu, 97, "positive normals, stride 97");
  bad += check(0x00000001u, 0x007fffffu, 13, "subnormals, stride 13");
  bad += check(0x3f000000u, 0x3f800000u, 1, "[0.5, 1] exhaustive");
  const uint32_t special[] = {0x00000000u, 0x80000000u, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xbf800000u, 0x80000001u};
  for (unsigned s = 0; s < sizeof(special) / sizeof(special[0]); ++s) bad += check(special[s], special[s], 1, "special");
  return bad != 0;
}
