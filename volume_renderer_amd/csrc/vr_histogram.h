// vr_histogram.h -- the class of a voxel under a histogram's limits (include/vrhip.h vr_volume_histogram,
// DESIGN.md s18), one inline function that the kernel (vr_histogram.hip) and the host (vr_capi.hip
// vr_histogram_bin_host) both evaluate -- fp32, every operation rounded once (-ffp-contract=off on both
// sides) -- the order-preserving keys of the extrema, and the launch arguments of the kernel.
#pragma once
#include <stdint.h>

#include "vr_clip.h"
#include "vr_device.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define VR_HG_FN __host__ __device__ __forceinline__
#else
#define VR_HG_FN static inline
#endif

#define VR_HIST_BELOW (-1)
#define VR_HIST_ABOVE (-2)
#define VR_HIST_NAN (-3)

// Voxel v against [lo, hi] in nbins bins, inv = 1.0f / (hi - lo) formed once on the host: the bin
// 0 .. nbins - 1 (v == hi falls in the last one, as MATLAB's histcounts), or VR_HIST_BELOW / ABOVE / NAN.
// x is finite and >= 0 here (the host checks that inv is finite), so the conversion is defined.
VR_HG_FN int32_t vr_hist_bin(float v, float lo, float hi, float inv, int32_t nbins) {
  if (v != v) return VR_HIST_NAN;
  if (v < lo) return VR_HIST_BELOW;
  if (v > hi) return VR_HIST_ABOVE;
  const float x = ((v - lo) * inv) * (float)nbins;
  const int32_t b = (int32_t)x;
  return b < nbins - 1 ? b : nbins - 1;
}

// IEEE totalOrder of the non-NaN floats as unsigned integers: -inf < ... < -0 < +0 < ... < +inf.  No
// non-NaN float has key 0 or ~0, so a zeroed cell means "no voxel yet" for a maximum of keys and for a
// maximum of inverted keys (the minimum) alike.
VR_HG_FN uint32_t vr_hist_key(uint32_t bits) { return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u); }
VR_HG_FN uint32_t vr_hist_unkey(uint32_t key) { return (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key; }

namespace vr {

// The row accumulators in device memory between the count launch and the finalize launch, zeroed by the
// host: for rows rows, in this order, double sum[rows]; uint64 cnt[rows][4] (below, above, nan, ninf);
// uint32 kmax[rows]; uint32 kmin[rows] (the maximum of ~key).
inline size_t hist_acc_bytes(int32_t rows) { return (size_t)rows * (8 + 32 + 4 + 4); }

struct HistParams {
  DevTex tex;             // the source texture (bound: the count launch is skipped otherwise)
  const uint8_t *labels;  // the resident label bytes, dense, the texture's dims (label_count > 0)
  int32_t nbins, rows;    // rows = label_count + 1, or 1
  float lo, hi, inv;
  int32_t label_first, label_count;
  ClipSet clip;  // the handle's planes as they were set ({n0, n1, n2, offset} in q), n = 0: no clip
  unsigned long long *counts;  // [rows][nbins], zeroed by the host
  void *acc;                   // hist_acc_bytes(rows), zeroed by the host
};

}  // namespace vr
