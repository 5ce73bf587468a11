// vr_labels.hip -- the label gain pass (include/vrhip.h vr_set_label_gains): the
// resident emission buffer re-derived from its unmodified copy, a dense uint8 label volume and a
// table of one fp32 gain per label, with the upload's statistics of the written values.
#include <hip/hip_runtime.h>

#include "vr_device.h"
#include "vr_labels.h"

namespace vr {

// One padded row per workgroup iteration, shaped like pad_planes_kernel (vr_kernels.hip): a coalesced
// read of the unmodified padded row (its apron replicates its interior already) and of the label row
// at clamped coordinates, one byte per lane; the gain table sits in LDS; a coalesced 4-byte store.
// Padded voxel (i, j, k) = src(i, j, k) * gain[label(clamp(i-1), clamp(j-1), clamp(k-1))], so the
// apron of dst is the edge replicate of its modulated interior.  nonfinite / max |x| of the written
// values fold in as in the upload: one wave reduction and one atomic pair per workgroup.
__global__ __launch_bounds__(256) void label_gain_kernel(const float *__restrict__ src,
                                                         const uint8_t *__restrict__ labels,
                                                         const float *__restrict__ gains, int32_t n, int32_t nx,
                                                         int32_t ny, int32_t nz, float *__restrict__ dst,
                                                         uint64_t rows, BufStats *st) {
  __shared__ float tab[VR_LABEL_GAINS_MAX];
  tab[threadIdx.x] = (int32_t)threadIdx.x < n ? gains[threadIdx.x] : 1.f;
  __syncthreads();
  const uint64_t px = (uint64_t)nx + 2, py = (uint64_t)ny + 2;
  uint32_t bad = 0;
  float mx = 0.f;
  for (uint64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const int64_t kk = (int64_t)(row / py) - 1, jj = (int64_t)(row % py) - 1;
    const int64_t sk = kk < 0 ? 0 : (kk > (int64_t)nz - 1 ? (int64_t)nz - 1 : kk);
    const int64_t sj = jj < 0 ? 0 : (jj > (int64_t)ny - 1 ? (int64_t)ny - 1 : jj);
    const uint8_t *l = labels + ((uint64_t)sk * (uint64_t)ny + (uint64_t)sj) * (uint64_t)nx;
    const float *s = src + row * px;
    float *d = dst + row * px;
    for (uint32_t i = threadIdx.x; i < px; i += blockDim.x) {
      const uint32_t si = i == 0 ? 0u : (i > (uint32_t)nx ? (uint32_t)nx - 1 : i - 1);
      const float v = vr_label_gain(s[i], l[si], tab, n);
      d[i] = v;
      if (!(fabsf(v) <= 3.4028234e38f)) bad = 1;
      else mx = fmaxf(mx, fabsf(v));
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    bad |= __shfl_xor(bad, off, 64);
    mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  }
  __shared__ uint32_t sb[4];
  __shared__ float sm[4];
  if ((threadIdx.x & 63) == 0) {
    sb[threadIdx.x >> 6] = bad;
    sm[threadIdx.x >> 6] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const uint32_t bb = sb[0] | sb[1] | sb[2] | sb[3];
    const float m = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    if (bb) atomicOr(&st->nonfinite, 1u);
    atomicMax(reinterpret_cast<unsigned int *>(&st->maxabs), __float_as_uint(m));  // m >= 0
  }
}

// src, dst: padded (nx+2)(ny+2)(nz+2) floats; labels: dense nx*ny*nz bytes; gains: n <= 256 floats
hipError_t launch_label_gain(const float *src, const uint8_t *labels, const float *gains, int32_t n, int32_t nx,
                             int32_t ny, int32_t nz, float *dst, BufStats *st, hipStream_t s) {
  if (nx <= 0 || ny <= 0 || nz <= 0 || n < 1 || n > VR_LABEL_GAINS_MAX) return hipErrorInvalidValue;
  const uint64_t rows = ((uint64_t)nz + 2) * ((uint64_t)ny + 2);
  const uint64_t blocks = rows < 2048 ? rows : 2048;  // as launch_pad_planes: workgroups that loop over rows
  hipLaunchKernelGGL(label_gain_kernel, dim3((unsigned)blocks), dim3(256), 0, s, src, labels, gains, n, nx, ny, nz, dst,
                     rows, st);
  return hipGetLastError();
}

}  // namespace vr
