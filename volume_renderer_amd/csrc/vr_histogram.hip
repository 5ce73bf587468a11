// vr_histogram.hip -- histogram and per-row statistics of a resident source texture (include/vrhip.h
// vr_volume_histogram): one streaming pass over the interior voxels of the padded buffer,
// optionally split by label and restricted to the clipped region, and a small finalize launch.
#include <hip/hip_runtime.h>

#include "../../include/vrhip.h"
#include "vr_histogram.h"

namespace vr {

constexpr uint32_t HIST_NONE = 0xFFFFFFFFu;  // a lane without a voxel to count
constexpr uint32_t HIST_UNROLL = 4;          // row loads in flight per lane

constexpr uint32_t HIST_BACKOFF = 7;          // batches a wave counts plainly after a batch that was not uniform

// The counts of one batch of HIST_UNROLL cells per lane (HIST_NONE: no voxel) into the workgroup's LDS
// table.  Called by whole waves.  UNI (the wave-uniform shortcut): when every cell of the
// wave's batch that is a cell is the same one, a single lane adds their number -- the test starts from
// lane 0's first cell and gives up at the first batch entry that differs, and after a batch that was not
// uniform the wave does not try again for HIST_BACKOFF batches (skip, wave-uniform), so that data
// without coherence pays next to nothing; otherwise, and without UNI, one LDS atomic per lane and cell.
template <bool UNI>
__device__ __forceinline__ void hist_count(uint32_t *cells, const uint32_t (&c)[HIST_UNROLL], uint32_t &skip) {
  if (UNI) {
    if (skip == 0) {
      const uint32_t c0 = __builtin_amdgcn_readfirstlane(c[0]);
      if (c0 != HIST_NONE && __all(c[0] == c0 || c[0] == HIST_NONE)) {
        bool same = true;
#pragma unroll
        for (uint32_t u = 1; u < HIST_UNROLL; ++u) same = same && (c[u] == c0 || c[u] == HIST_NONE);
        if (__all(same)) {
          uint32_t n = 0;
#pragma unroll
          for (uint32_t u = 0; u < HIST_UNROLL; ++u) n += (uint32_t)__popcll(__ballot(c[u] != HIST_NONE));
          if ((int)(threadIdx.x & 63) == __ffsll((unsigned long long)__ballot(1)) - 1) atomicAdd(&cells[c0], n);
          return;
        }
      }
      skip = HIST_BACKOFF;
    } else {
      --skip;
    }
  }
#pragma unroll
  for (uint32_t u = 0; u < HIST_UNROLL; ++u)
    if (c[u] != HIST_NONE) atomicAdd(&cells[c[u]], 1u);
}

// Up to 2048 workgroups of 256 threads loop over the interior rows of the padded layout, shaped like
// label_gain_kernel (vr_labels.hip): coalesced reads of the row and, with LABELS, of the label row, one
// byte per lane; with CLIP the j and k coordinates of the voxel centre are wave-uniform per row.  The
// workgroup's table lives in LDS (dynamic, sized by the host): double sum[R]; uint32 cells[R * NB];
// uint32 cnt[R][4] (below, above, nan, ninf) right behind the cells, so that every class of a voxel is
// one cell index; uint32 kmax[R], kmin[R] (keys of vr_histogram.h; kmin holds the maximum of ~key).
// Extrema and sum are kept in registers per lane for the row (of the table) of the lane's last voxel and
// folded into LDS when that row changes -- never without labels, rarely with coherent labels.  At the
// end the non-zero cells go to the global tables with one atomic each.  No cell can wrap: the host sizes
// the grid so that a workgroup sees fewer than 2^32 voxels.
template <bool LABELS, bool CLIP, bool UNI>
__global__ __launch_bounds__(256) void histogram_kernel(const HistParams H, uint64_t nrows) {
  extern __shared__ double hist_lds[];
  const uint32_t R = (uint32_t)H.rows, NB = (uint32_t)H.nbins, ncell = R * NB;
  double *ssum = hist_lds;
  uint32_t *cells = reinterpret_cast<uint32_t *>(ssum + R);
  uint32_t *cnt = cells + ncell;
  uint32_t *kmax = cnt + 4 * R;
  uint32_t *kmin = kmax + R;
  for (uint32_t i = threadIdx.x; i < ncell + 6 * R; i += blockDim.x) cells[i] = 0u;
  for (uint32_t i = threadIdx.x; i < R; i += blockDim.x) ssum[i] = 0.0;
  __syncthreads();

  const uint32_t nx = (uint32_t)H.tex.nx, ny = (uint32_t)H.tex.ny;
  const uint64_t px = (uint64_t)nx + 2, pxy = px * ((uint64_t)ny + 2);
  uint32_t cur = HIST_NONE, amax = 0u, aminv = 0u, skip = 0u;
  double asum = 0.0;
  auto fold = [&]() {
    if (cur == HIST_NONE) return;
    if (amax) {
      atomicMax(&kmax[cur], amax);
      atomicMax(&kmin[cur], aminv);
    }
    if (asum != 0.0) atomicAdd(&ssum[cur], asum);
  };

  for (uint64_t row = blockIdx.x; row < nrows; row += gridDim.x) {
    const uint64_t k = row / ny, j = row - k * ny;
    const float *s = H.tex.p + (k + 1) * pxy + (j + 1) * px + 1;
    const uint8_t *l = LABELS ? H.labels + row * (uint64_t)nx : nullptr;
    float q1 = 0.f, q2 = 0.f;
    if (CLIP) {
      q1 = ((float)(uint32_t)j + 0.5f) / H.tex.fny;
      q2 = ((float)(uint32_t)k + 0.5f) / H.tex.fnz;
    }
    for (uint32_t base = 0; base < nx; base += HIST_UNROLL * 256u) {
      float v[HIST_UNROLL];
      uint32_t lb[HIST_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < HIST_UNROLL; ++u) {
        const uint32_t i = base + u * 256u + threadIdx.x;
        v[u] = i < nx ? s[i] : 0.f;
        lb[u] = LABELS && i < nx ? (uint32_t)l[i] : 0u;
      }
      uint32_t cell[HIST_UNROLL];
#pragma unroll
      for (uint32_t u = 0; u < HIST_UNROLL; ++u) {
        const uint32_t i = base + u * 256u + threadIdx.x;
        bool keep = i < nx;
        if (CLIP) {
          const float q0 = ((float)i + 0.5f) / H.tex.fnx;  // one IEEE division
#pragma unroll
          for (int p = 0; p < VR_CLIP_MAX; ++p) {
            if (p >= H.clip.n) break;
            const float sd = fmaf(H.clip.pl[p][2], q2, fmaf(H.clip.pl[p][1], q1, fmaf(H.clip.pl[p][0], q0, H.clip.pl[p][3])));
            keep = keep && sd >= 0.f;  // a NaN is not kept
          }
        }
        uint32_t c = HIST_NONE;
        if (keep) {
          uint32_t r = 0u;
          if (LABELS) {
            const uint32_t d = (lb[u] - (uint32_t)H.label_first) & 0xFFu;
            r = d < (uint32_t)H.label_count ? d : (uint32_t)H.label_count;
          }
          if (r != cur) {
            fold();
            cur = r;
            amax = aminv = 0u;
            asum = 0.0;
          }
          const float x = v[u];
          const int32_t b = vr_hist_bin(x, H.lo, H.hi, H.inv, H.nbins);
          if (b != VR_HIST_NAN) {
            const uint32_t key = vr_hist_key(__float_as_uint(x));
            amax = key > amax ? key : amax;
            aminv = ~key > aminv ? ~key : aminv;
            if (fabsf(x) <= 3.4028234e38f) asum = asum + (double)x;
            else atomicAdd(&cnt[4 * r + 3], 1u);
          }
          c = b >= 0 ? r * NB + (uint32_t)b : ncell + 4 * r + (uint32_t)(-1 - b);
        }
        cell[u] = c;
      }
      hist_count<UNI>(cells, cell, skip);
    }
  }
  fold();
  __syncthreads();

  double *gsum = static_cast<double *>(H.acc);
  unsigned long long *gcnt = reinterpret_cast<unsigned long long *>(gsum + R);
  uint32_t *gkmax = reinterpret_cast<uint32_t *>(gcnt + 4 * R);
  uint32_t *gkmin = gkmax + R;
  for (uint32_t i = threadIdx.x; i < ncell; i += blockDim.x) {
    const uint32_t n = cells[i];
    if (n) atomicAdd(&H.counts[i], (unsigned long long)n);
  }
  for (uint32_t i = threadIdx.x; i < 4 * R; i += blockDim.x) {
    const uint32_t n = cnt[i];
    if (n) atomicAdd(&gcnt[i], (unsigned long long)n);
  }
  for (uint32_t i = threadIdx.x; i < R; i += blockDim.x) {
    if (kmax[i]) {
      atomicMax(&gkmax[i], kmax[i]);
      atomicMax(&gkmin[i], kmin[i]);
    }
    if (ssum[i] != 0.0) atomicAdd(&gsum[i], ssum[i]);
  }
}

// One workgroup per row: total = nan + below + above + the row's bins, keys turned into floats.
__global__ __launch_bounds__(256) void histogram_finalize_kernel(const unsigned long long *__restrict__ counts,
                                                                 const void *acc, int32_t rows, int32_t nbins,
                                                                 vr_hist_row *__restrict__ out) {
  const uint32_t r = blockIdx.x, R = (uint32_t)rows;
  unsigned long long n = 0;
  for (uint32_t b = threadIdx.x; b < (uint32_t)nbins; b += blockDim.x) n += counts[(uint64_t)r * (uint32_t)nbins + b];
  __shared__ unsigned long long part[256];
  part[threadIdx.x] = n;
  __syncthreads();
  for (uint32_t off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) part[threadIdx.x] += part[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  const double *gsum = static_cast<const double *>(acc);
  const unsigned long long *gcnt = reinterpret_cast<const unsigned long long *>(gsum + R);
  const uint32_t *gkmax = reinterpret_cast<const uint32_t *>(gcnt + 4 * R);
  const uint32_t *gkmin = gkmax + R;
  vr_hist_row o;
  o.below = gcnt[4 * r + 0];
  o.above = gcnt[4 * r + 1];
  o.nan = gcnt[4 * r + 2];
  o.ninf = gcnt[4 * r + 3];
  o.total = o.nan + o.below + o.above + part[0];
  const uint32_t kx = gkmax[r], kn = ~gkmin[r];
  o.max = __uint_as_float(kx ? vr_hist_unkey(kx) : 0x7fc00000u);
  o.min = __uint_as_float(kx ? vr_hist_unkey(kn) : 0x7fc00000u);
  o.sum = gsum[r];
  out[r] = o;
}

// LDS bytes of a workgroup's table (see histogram_kernel)
static size_t hist_lds_bytes(int32_t rows, int32_t nbins) {
  return (size_t)rows * 8 + ((size_t)rows * (size_t)nbins + 6 * (size_t)rows) * 4;
}

template <bool LABELS, bool CLIP, bool UNI>
static hipError_t launch_hist(const HistParams &H, uint64_t nrows, unsigned blocks, size_t lds, hipStream_t s) {
  auto *k = histogram_kernel<LABELS, CLIP, UNI>;
  if (lds > 48 * 1024) {
    const hipError_t rc = hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                              hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (rc != hipSuccess) return rc;
  }
  hipLaunchKernelGGL(k, dim3(blocks), dim3(256), lds, s, H, nrows);
  return hipGetLastError();
}

// Workgroups of the count launch for nrows interior rows of nx voxels: min(nrows, 2048), doubled until
// no workgroup's share of rows holds 2^32 voxels (a 32-bit LDS cell then cannot wrap).
uint64_t histogram_blocks(uint64_t nrows, uint64_t nx) {
  uint64_t blocks = nrows < 2048 ? nrows : 2048;
  while (blocks < nrows && ((nrows + blocks - 1) / blocks) * nx >= (1ull << 32)) blocks = blocks * 2 < nrows ? blocks * 2 : nrows;
  return blocks;
}

// H.counts and H.acc zeroed on s before; a bound texture with nx, ny, nz >= 1 (the caller skips the launch
// otherwise).  uniform: the wave-uniform shortcut of hist_count.
hipError_t launch_histogram(const HistParams &H, bool uniform, hipStream_t s) {
  if (!H.tex.p || H.tex.nx <= 0 || H.tex.ny <= 0 || H.tex.nz <= 0 || H.rows < 1 || H.nbins < 1 ||
      (H.label_count > 0 && !H.labels))
    return hipErrorInvalidValue;
  const size_t lds = hist_lds_bytes(H.rows, H.nbins);
  if (lds > 64 * 1024) return hipErrorInvalidValue;
  const uint64_t nrows = (uint64_t)H.tex.ny * (uint64_t)H.tex.nz;
  const uint64_t blocks = histogram_blocks(nrows, (uint64_t)H.tex.nx);
  if (((nrows + blocks - 1) / blocks) * (uint64_t)H.tex.nx >= (1ull << 32) || blocks > 0x7FFFFFFFull)
    return hipErrorInvalidValue;
  const bool labels = H.label_count > 0, clip = H.clip.n > 0;
  const unsigned g = (unsigned)blocks;
#define VR_HIST_CASE(L, C)                                             \
  if (labels == L && clip == C)                                        \
    return uniform ? launch_hist<L, C, true>(H, nrows, g, lds, s) : launch_hist<L, C, false>(H, nrows, g, lds, s);
  VR_HIST_CASE(false, false)
  VR_HIST_CASE(false, true)
  VR_HIST_CASE(true, false)
  VR_HIST_CASE(true, true)
#undef VR_HIST_CASE
  return hipErrorInvalidValue;
}

hipError_t launch_histogram_finalize(const unsigned long long *counts, const void *acc, int32_t rows, int32_t nbins,
                                     void *rows_out, hipStream_t s) {
  if (rows < 1 || nbins < 1 || !counts || !acc || !rows_out) return hipErrorInvalidValue;
  hipLaunchKernelGGL(histogram_finalize_kernel, dim3((unsigned)rows), dim3(256), 0, s, counts, acc, rows, nbins,
                     static_cast<vr_hist_row *>(rows_out));
  return hipGetLastError();
}

}  // namespace vr
