// vr_clip.h -- clip planes (include/vrhip.h vr_set_clip): the plane set a clipped launch carries and
// the per-ray interval intersection, shared by render_kernel, project_kernel, isosurface_kernel and
// transfer_kernel.  The LDS-staged march (vr_march.hip) knows nothing of it.
//
// A plane keeps the half-space N . p + D >= 0 of world positions p: the host (vr_capi.hip clip_set)
// has folded the sampler's coordinate transform q = (p - bmin) * bscale into it, once per launch.
// Clipping only shortens a ray's interval [tnear, tfar] after ray_setup; the march that follows --
// pos_0 = fmaf(d, tnear, o), t_0 = tnear, the recurrences, the exit tests against tfar, the
// empty-space leap -- is the unclipped one.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

#ifndef VR_CLIP_MAX
#define VR_CLIP_MAX 6  // include/vrhip.h
#endif

namespace vr {

// At most 6 x 16 B plus a count: travels by value next to RenderParams (which must not grow,
// vr_device.h), on its own or inside a kernel's Extras struct.  Wave-uniform: the kernels read it
// from the kernel arguments with scalar loads.
struct ClipSet {
  float pl[VR_CLIP_MAX][4];  // N.x, N.y, N.z, D per plane, kernel axis order
  int32_t n;                 // planes in use, 0 .. VR_CLIP_MAX
  int32_t pad[3];
};

// The second kernel argument of a kernel that has no Extras struct: the plane set of a clipped
// instantiation, nothing (an empty argument) of an unclipped one.
template <bool CLIP>
struct ClipArg {};
template <>
struct ClipArg<true> {
  ClipSet set;
};

// The planes applied in order to the interval ray_setup produced (tnear already clamped to 0).
// Returns the clipped ray's hit flag: it hit the box and tnear <= tfar (a NaN fails).  A plane the
// ray is parallel to (sd == +-0, or NaN) makes the ray a miss unless its origin is on the kept side.
// The trip count and the plane constants are wave-uniform (SGPRs); six guarded iterations with
// constant indices, so that the set is never indexed dynamically (no private copy, no scratch).
// V3: the kernels' f3 (vr_sampling.h); a template so that the host driver can include this header for
// ClipSet alone.
template <class V3>
__device__ __forceinline__ bool clip_interval(const ClipSet &C, const V3 &o, const V3 &d, bool hit, float &tnear,
                                              float &tfar) {
#pragma unroll
  for (int i = 0; i < VR_CLIP_MAX; ++i) {
    if (i >= C.n) break;
    const float nx = C.pl[i][0], ny = C.pl[i][1], nz = C.pl[i][2], dd = C.pl[i][3];
    const float s0 = fmaf(nz, o.z, fmaf(ny, o.y, fmaf(nx, o.x, dd)));
    const float sd = fmaf(nz, d.z, fmaf(ny, d.y, nx * d.x));
    const float tc = (-s0) / sd;  // one IEEE division
    if (sd > 0.f) {
      if (tc > tnear) tnear = tc;
    } else if (sd < 0.f) {
      if (tc < tfar) tfar = tc;
    } else if (!(s0 >= 0.f)) {
      hit = false;
    }
  }
  return hit && tnear <= tfar;
}

}  // namespace vr
