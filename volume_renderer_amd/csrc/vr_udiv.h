// vr_udiv.h -- quotients of small unsigned values by small wave-uniform divisors as one multiply
// and one shift (the staging copy's lane -> (row slot, x, y, z) map and pass count, vr_stage.h
// stage_box).  Plain C++: also compiled on the host (tests/test_udiv_small_host.py).
//
// magic = ceil(2^20 / d), so magic * d = 2^20 + e with 0 <= e < d, and
//   n * magic / 2^20 = n / d + n * e / (d * 2^20).
// The second term is below 1 / d when n * e < 2^20, and then floor(n * magic / 2^20) = floor(n / d):
// a quotient n / d with remainder r has fraction r / d <= (d - 1) / d, which a term below 1 / d
// cannot carry over.  For 1 <= d <= 64 and n < 4096: n * e < 2^12 * 2^6 = 2^18, and the product
// n * magic <= 4095 * 2^20 fits 32 bits (both factors below 2^24: a 24-bit multiply on the device).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VR_UDIV_HD __host__ __device__
#else
#define VR_UDIV_HD
#endif

namespace vr {

constexpr uint32_t UDIV_SHIFT = 20;
constexpr uint32_t UDIV_MAX_D = 64;    // largest divisor
constexpr uint32_t UDIV_MAX_N = 4096;  // dividends lie below it

VR_UDIV_HD constexpr uint32_t udiv_magic(uint32_t d) { return ((1u << UDIV_SHIFT) + d - 1u) / d; }

// n / d for n < UDIV_MAX_N, magic = udiv_magic(d), 1 <= d <= UDIV_MAX_D
VR_UDIV_HD inline uint32_t udiv_small(uint32_t n, uint32_t magic) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul24(n, magic) >> UDIV_SHIFT;
#else
  return (n * magic) >> UDIV_SHIFT;
#endif
}

// n % d, with q = udiv_small(n, udiv_magic(d))
VR_UDIV_HD inline uint32_t urem_small(uint32_t n, uint32_t q, uint32_t d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return n - __umul24(q, d);
#else
  return n - q * d;
#endif
}

// The magics by divisor, for a scalar load with a wave-uniform index.  m: udiv_magic(d); mper: the
// magic of 64 / d, the staging copy's rows per pass.  Entry 0 is never read.
struct UdivEntry {
  uint32_t m, mper;
};
struct UdivTab {
  UdivEntry e[UDIV_MAX_D + 1];
};
constexpr UdivTab make_udiv_tab() {
  UdivTab t{};
  for (uint32_t d = 1; d <= UDIV_MAX_D; ++d) {
    t.e[d].m = udiv_magic(d);
    t.e[d].mper = udiv_magic(64u / d);
  }
  return t;
}

}  // namespace vr
