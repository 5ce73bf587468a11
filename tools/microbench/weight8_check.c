// weight8_check.c [STRIDE] -- CPU check that the 8-bit filter weights formed by adding and taking off
// 1.5 * 2^15 (vr_sampling.h frac8_rn / weight8_rn: no v_rndne) equal the rintf forms bit for bit, sign
// of zero included:
//   A  rintf(r * 256) * (1 / 256)               ==  (r + C) - C                  r in [0, 1]
//   B  fma(rintf(xb * 256), 1 / 256, -floor xb)  ==  ((xb + C) - C) - floor xb    xb in [-0.5, 1100]
// STRIDE 1 (default): every fp32 of both ranges.  STRIDE n: every n-th, plus every tie k / 512.
// Exit status 1 on a mismatch.  gcc -O2 -mfma -ffp-contract=off weight8_check.c -lm
#include <stdio.h>
#include <stdlib.h>
#include <math.h>
#include <stdint.h>
#include <string.h>
static const float C = 49152.f;  // 1.5 * 2^15: x + C is rounded to a multiple of 1/256 (ties to even) for |x| < 2^14
static uint64_t n, bad;
static float first;
static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
static float from(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }
static void note(float x, float a, float b) {
  n++;
  if (bits(a) != bits(b)) { if (!bad) first = x; bad++; }
}
static void check_a(float r) {
  const float old = rintf(r * 256.f) * (1.f / 256.f);
  volatile float q = r + C;  // (volatile: the sum is rounded to fp32 before the constant comes off)
  note(r, old, q - C);
}
static void check_b(float xb) {
  const float fl = floorf(xb);
  const float old = fmaf(rintf(xb * 256.f), 1.f / 256.f, -fl);
  volatile float q = xb + C;
  volatile float t = q - C;
  note(xb, old, t - fl);
}
int main(int argc, char **argv) {
  const uint32_t stride = argc > 1 ? (uint32_t)strtoul(argv[1], 0, 10) : 1u;
  if (!stride) return 2;
  for (uint64_t u = 0; u <= 0x3f800000u; u += stride) check_a(from((uint32_t)u));            // [0, 1]
  for (uint64_t u = 0; u <= bits(1100.f); u += stride) check_b(from((uint32_t)u));            // [0, 1100]
  for (uint64_t u = 0x80000000u; u <= 0xbf000000u; u += stride) check_b(from((uint32_t)u));   // [-0.5, -0]
  if (stride > 1) {
    for (int k = 0; k <= 512; ++k) check_a((float)k / 512.f);
    for (int k = -256; k <= 1100 * 512; ++k) check_b((float)k / 512.f);
  }
  printf("stride=%u n=%llu bad=%llu first=%a\n", stride, (unsigned long long)n, (unsigned long long)bad, first);
  return bad ? 1 : 0;
}
