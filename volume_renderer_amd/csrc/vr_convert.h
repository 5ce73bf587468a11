// vr_convert.h -- the value contract of typed volumes (include/vrhip.h, vr_dtype): one definition of
// the element -> fp32 conversion for the device (the pad pass of the upload, vr_kernels.hip) and the
// host (vr_convert_host, vr_capi.hip), so that both give the same bits.
//   - uint8 / uint16 / int16 -> fp32 is exact (24 significand bits hold 16);
//   - binary16 -> fp32 is exact too, written with integer operations so that subnormals, +-0, +-inf
//     and NaN (payload widened, never quieted) do not depend on a conversion instruction's modes;
//   - UNORM is one IEEE fp32 division by 255.0f / 65535.0f (never a reciprocal multiply: the build
//     has -fno-fast-math, and HIP's fp32 division is correctly rounded).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VR_HD __host__ __device__
#else
#define VR_HD
#endif

namespace vr {

// dtype codes as include/vrhip.h (enum vr_dtype | VR_DTYPE_UNORM), for files that do not include it
constexpr int32_t DT_F32 = 0, DT_U8 = 1, DT_U16 = 2, DT_I16 = 3, DT_F16 = 4, DT_UNORM = 0x100;

// element size in bytes; 0 for an invalid code or flag combination
VR_HD inline uint32_t dtype_size(int32_t dtype) {
  switch (dtype) {
    case DT_F32: return 4;
    case DT_U8: case DT_U8 | DT_UNORM: return 1;
    case DT_U16: case DT_U16 | DT_UNORM: case DT_I16: case DT_F16: return 2;
    default: return 0;
  }
}

struct half_bits {  // an IEEE binary16 as stored
  uint16_t u;
};

VR_HD inline float widen(float x) { return x; }
VR_HD inline float widen(uint8_t x) { return (float)x; }
VR_HD inline float widen(uint16_t x) { return (float)x; }
VR_HD inline float widen(int16_t x) { return (float)x; }
VR_HD inline float widen(half_bits h) {
  const uint32_t sign = (uint32_t)(h.u & 0x8000u) << 16;
  const uint32_t e = (h.u >> 10) & 0x1Fu, m = h.u & 0x3FFu;
  if (e == 0x1Fu) return __builtin_bit_cast(float, sign | 0x7F800000u | (m << 13));  // inf / NaN
  if (e) return __builtin_bit_cast(float, sign | ((e + 112u) << 23) | (m << 13));
  // zero or subnormal: m * 2^-24, a normal fp32 for m != 0 (the product is exact)
  const float mag = (float)m * 5.9604644775390625e-8f;
  return __builtin_bit_cast(float, sign | __builtin_bit_cast(uint32_t, mag));
}

template <bool UNORM, class T>
VR_HD inline float to_f32(T x) {
  const float v = widen(x);
  if constexpr (UNORM) {
    static_assert(sizeof(T) <= 2, "UNORM: uint8 / uint16 only");
    return v / (sizeof(T) == 1 ? 255.0f : 65535.0f);
  } else {
    return v;
  }
}

}  // namespace vr
