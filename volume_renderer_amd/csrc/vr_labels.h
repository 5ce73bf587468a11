// vr_labels.h -- the value of a voxel under a label gain table (include/vrhip.h vr_set_label_gains),
// one inline function that the kernel (vr_labels.hip) and the host (vr_capi.hip vr_label_gain_host)
// both evaluate: one fp32 multiplication rounded once (-ffp-contract=off on both sides), or a plain
// copy for a label the table does not cover.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VR_LG_FN __host__ __device__ __forceinline__
#else
#define VR_LG_FN static inline
#endif

#define VR_LABEL_GAINS_MAX 256  // one gain per uint8 label

// Voxel v with label `label` under the n gains of `gains`: labels at or above n have gain 1 and are
// copied, not multiplied (a NaN keeps its payload, -0 its sign).
VR_LG_FN float vr_label_gain(float v, uint32_t label, const float *gains, int32_t n) {
  return label < (uint32_t)n ? v * gains[label] : v;
}
