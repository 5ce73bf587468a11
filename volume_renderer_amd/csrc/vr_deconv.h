// vr_deconv.h -- the elementwise steps of the Richardson-Lucy deconvolution (include/vrhip.h
// vr_set_deconvolution): inline functions that the kernels (vr_smooth.hip, the epilogues of the filter
// passes, and vr_deconv.hip) and the host (vr_capi.hip vr_deconvolve_host) both evaluate.  The blur
// between them is vr_smooth_tap (vr_smooth.h).  Every operation is rounded once to fp32
// (-ffp-contract=off on both sides; the division is HIP's default, correctly rounded one).
#pragma once
#include "vr_smooth.h"

// What a filter pass stores (vr_smooth.hip, template parameter EPI; 0 is the smoothing's own pass) and the
// flags of such a pass and of the elementwise launches (vr_deconv.hip).
#define VR_EPI_FILTER 1     // the filter's value
#define VR_EPI_RATIO 2      // vr_deconv_ratio(aux voxel, value, floor): the last pass of B(u)
#define VR_EPI_UPDATE 3     // vr_deconv_update(aux voxel, value): the last pass of B(r)
#define VR_EPI_LOAD_DATA 1u  // flag: src is the unmodified upload, read through vr_deconv_data (u_0)
#define VR_EPI_AUX_DATA 2u   // flag: the update's aux is the unmodified upload, read through vr_deconv_data

// The data the iteration fits: the upload with its negative voxels at 0 (NaN and -0 pass through).
VR_SM_FN float vr_deconv_data(float y) { return (y < 0.f) ? 0.f : y; }

// r = d / max(c, floor), c the blurred estimate: the comparison is written out, so a NaN in c gives floor.
VR_SM_FN float vr_deconv_ratio(float y, float c, float flr) {
  const float g = (c > flr) ? c : flr;
  return vr_deconv_data(y) / g;
}

// u_{k+1} = u_k * m, m the blurred ratio.
VR_SM_FN float vr_deconv_update(float u, float m) { return u * m; }
