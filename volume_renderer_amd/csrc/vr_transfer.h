// vr_transfer.h -- the transfer-function table lookup (include/vrhip.h vr_render_transfer), one
// inline function pair that the kernel (vr_transfer.hip) and the host (vr_capi.hip
// vr_transfer_lookup_host, the leap's A(+-0) test) both evaluate: the same operations in the same
// order, fp32, each rounded once (-ffp-contract=off on both sides, the fma explicit).
//
// A table T of n entries over the coordinate range [lo, hi] is read as n - 1 segments; segment i is
// the record {T[i], T[i+1] - T[i]} (the slope is formed once, on the host, with that fp32
// subtraction), and L(T, n, lo, hi, c) = fmaf(w, slope_i, T[i]) with (i, w) = vr_tf_segment(c).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VR_TF_FN __host__ __device__ __forceinline__
#else
#define VR_TF_FN static inline
#endif

// The segment i in [0, n - 2] and the weight w in [0, 1] of coordinate c; inv = 1.0f / (hi - lo).
// The two selects are fminf(fmaxf(x, 0), n - 1) with the cases those leave open decided: a NaN
// coordinate and -0 give +0 (entry 0), so host and device agree in every bit.
VR_TF_FN int32_t vr_tf_segment(float c, float lo, float inv, int32_t n, float *w) {
  const float top = (float)(n - 1);
  float x = ((c - lo) * inv) * top;
  x = x > 0.f ? x : 0.f;
  x = x < top ? x : top;
  int32_t i = (int32_t)x;
  i = i < n - 2 ? i : n - 2;
  *w = x - (float)i;
  return i;
}

// The value of a segment record at weight w.  A zero slope returns `base` bit for bit (w is finite;
// a base of -0 comes back as +0).
VR_TF_FN float vr_tf_value(float w, float base, float slope) { return fmaf(w, slope, base); }
