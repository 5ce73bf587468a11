// vr_smooth.h -- the value of a voxel under Gaussian smoothing (include/vrhip.h vr_set_smoothing): the
// weights of one axis, formed once on the host in double, and the one-axis pass, one inline function
// that the kernels (vr_smooth.hip) and the host (vr_capi.hip vr_smooth_host) both evaluate: one fp32
// multiplication and 2R fused multiply-adds, each rounded once (-ffp-contract=off on both sides).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VR_SM_FN __host__ __device__ __forceinline__
#else
#define VR_SM_FN static inline
#endif

#define VR_SMOOTH_MAX_RADIUS 12                          // ceil(2 * VR_SMOOTH_MAX_SIGMA)
#define VR_SMOOTH_MAX_TAPS (2 * VR_SMOOTH_MAX_RADIUS + 1)  // room for one axis' weights

// The weights of one axis: R = ceil(2 sigma), g_i = exp(-i^2 / (2 sigma^2)) for i = -R..R, S their sum
// in ascending i, w[k] = (float)(g_{k-R} / S), all in double.  sigma = 0: R = 0 and the one weight 1
// (such an axis is skipped, not filtered).  Returns R; sigma must be finite and in 0..VR_SMOOTH_MAX_SIGMA.
static inline int32_t vr_smooth_weights(float sigma, float *w) {
  if (!(sigma > 0.f)) {
    w[0] = 1.f;
    return 0;
  }
  const double s = (double)sigma;
  const int32_t R = (int32_t)ceil(2.0 * s);
  double g[VR_SMOOTH_MAX_TAPS], S = 0.0;
  for (int32_t i = -R; i <= R; ++i) {
    g[i + R] = exp(-(double)(i * i) / (2.0 * s * s));
    S += g[i + R];
  }
  for (int32_t k = 0; k <= 2 * R; ++k) w[k] = (float)(g[k] / S);
  return R;
}

// One output of an axis pass: x(k) is the line's value at clamp(i - R + k), k = 0..2R.
template <class X>
VR_SM_FN float vr_smooth_tap(const float *w, int32_t R, X x) {
  float acc = w[0] * x(0);
  for (int32_t k = 1; k <= 2 * R; ++k) acc = fmaf(w[k], x(k), acc);
  return acc;
}
