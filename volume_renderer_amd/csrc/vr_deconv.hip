// vr_deconv.hip -- the two elementwise steps of the Richardson-Lucy deconvolution (include/vrhip.h
// vr_set_deconvolution) as launches of their own over a whole padded volume.  The derivation
// fuses both into the last filter pass of each blur (vr_smooth.hip, EPI); these launches serve a volume
// that has no axis to filter (every axis with a sigma has one voxel: B is the identity) and are what
// tools/deconv_bench.py measures the fused epilogues against.  An elementwise step over a padded volume
// whose apron replicates its interior leaves one that does.
#include <hip/hip_runtime.h>

#include "vr_deconv.h"
#include "vr_device.h"

namespace vr {

// dst[i] = RATIO ? vr_deconv_ratio(y[i], c[i], flr) : vr_deconv_update(u[i], m[i]) for n padded voxels; a is
// y or u, b is c or m.  dst may be a or b (voxel for voxel), so nothing is __restrict__.
template <bool RATIO>
__global__ __launch_bounds__(256) void deconv_pointwise_kernel(const float *a, const float *b, float *dst, uint64_t n,
                                                               float flr, uint32_t flags) {
  const uint64_t stride = (uint64_t)gridDim.x * 256u;
  for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += stride) {
    if (RATIO) {
      const float c = (flags & VR_EPI_LOAD_DATA) ? vr_deconv_data(b[i]) : b[i];
      dst[i] = vr_deconv_ratio(a[i], c, flr);
    } else {
      const float u = (flags & VR_EPI_AUX_DATA) ? vr_deconv_data(a[i]) : a[i];
      dst[i] = vr_deconv_update(u, b[i]);
    }
  }
}

// epi = VR_EPI_RATIO: dst = ratio of the upload `aux` and the blurred estimate `src` (VR_EPI_LOAD_DATA: src
// is the upload itself, read as u_0); VR_EPI_UPDATE: dst = aux * src (VR_EPI_AUX_DATA: aux is the upload).
// All padded (nx+2)(ny+2)(nz+2) floats.
hipError_t launch_deconv_pointwise(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, int epi,
                                   const float *aux, float flr, uint32_t flags, hipStream_t s) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || !src || !dst || !aux || (epi != VR_EPI_RATIO && epi != VR_EPI_UPDATE))
    return hipErrorInvalidValue;
  const uint64_t n = ((uint64_t)nx + 2) * ((uint64_t)ny + 2) * ((uint64_t)nz + 2);
  const uint64_t want = (n + 255) / 256;
  const unsigned blocks = (unsigned)(want < (1u << 16) ? want : (1u << 16));
  if (epi == VR_EPI_RATIO)
    hipLaunchKernelGGL(deconv_pointwise_kernel<true>, dim3(blocks), dim3(256), 0, s, aux, src, dst, n, flr, flags);
  else
    hipLaunchKernelGGL(deconv_pointwise_kernel<false>, dim3(blocks), dim3(256), 0, s, aux, src, dst, n, flr, flags);
  return hipGetLastError();
}

}  // namespace vr
