// vr_smooth.hip -- the Gaussian smoothing passes (include/vrhip.h vr_set_smoothing): one
// axis of the separable filter per launch over the padded fp32 layout, every output by vr_smooth_tap
// (vr_smooth.h), optionally with the upload's statistics of the written values.
// Every pass reads a padded volume whose apron replicates its interior and writes one: the interior
// outputs are computed at clamped coordinates, and the two apron cells of the filtered axis are stored
// with the edge outputs; along the other two axes the apron lines are filtered like any line (they
// replicate an interior line, so their outputs replicate that line's outputs bit for bit).
// The Richardson-Lucy deconvolution (vr_set_deconvolution) runs the same passes with an
// epilogue on the last axis of each blur (template parameter EPI): the output voxel's ratio or update
// (vr_deconv.h) is formed from the filter's value and the voxel of an auxiliary padded buffer at the same
// position, and stored in its place -- the apron cells as above, so no pad pass follows.
#include <hip/hip_runtime.h>

#include "vr_deconv.h"
#include "vr_device.h"
#include "vr_smooth.h"

namespace vr {

#define VR_SMOOTH_SEG 256   // x pass: outputs per staged row segment, one per lane
#define VR_SMOOTH_TX 64     // y / z pass: the tile's lanes along x, one wave wide
#define VR_SMOOTH_TA 32     // y / z pass: the tile's outputs along the filtered axis (8 per wave of the 4)

// EPI of a pass: 0 the smoothing's own (no epilogue, flags ignored); the others serve the deconvolution and
// take `flags`: VR_EPI_LOAD_DATA: the loads of src go through vr_deconv_data (src is the unmodified upload,
// iteration 0), VR_EPI_AUX_DATA: so does the update's auxiliary voxel.
//   VR_EPI_FILTER  the filter's value (a pass that only needs the load flag)
//   VR_EPI_RATIO   vr_deconv_ratio(aux, value, flr), aux the unmodified upload
//   VR_EPI_UPDATE  vr_deconv_update(aux, value), aux the estimate u; aux may be dst (each voxel is read
//                  by the thread that then writes it, and the filtered axis' apron cells are not read)
// With an epilogue neither dst nor aux is __restrict__.
template <int EPI>
struct smooth_dst {
  typedef float *type;
};
template <>
struct smooth_dst<0> {
  typedef float *__restrict__ type;
};

template <int EPI>
__device__ __forceinline__ float smooth_epilogue(float v, const float *aux, uint64_t at, float flr, uint32_t flags) {
  if (EPI == VR_EPI_RATIO) return vr_deconv_ratio(aux[at], v, flr);
  if (EPI == VR_EPI_UPDATE) {
    const float a = aux[at];
    return vr_deconv_update((flags & VR_EPI_AUX_DATA) ? vr_deconv_data(a) : a, v);
  }
  return v;
}

// nonfinite / max |x| of the written values, as in the upload and the label pass: one wave reduction
// and one atomic pair per workgroup (256 threads).
__device__ __forceinline__ void smooth_fold_stats(uint32_t bad, float mx, BufStats *st) {
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

// Along x: one padded row per workgroup iteration (as label_gain_kernel), in segments of VR_SMOOTH_SEG
// interior voxels staged in LDS with their halo of R on either side at clamped coordinates; lane t
// computes output t of the segment from consecutive LDS words (no bank conflict).
template <bool STATS, int EPI>
__global__ __launch_bounds__(256) void smooth_x_kernel(const float *__restrict__ src, typename smooth_dst<EPI>::type dst,
                                                       int32_t nx, uint64_t rows, const float *__restrict__ wts,
                                                       int32_t R, BufStats *st, const float *aux, float flr,
                                                       uint32_t flags) {
  __shared__ float w[VR_SMOOTH_MAX_TAPS];
  __shared__ float line[VR_SMOOTH_SEG + 2 * VR_SMOOTH_MAX_RADIUS];
  if ((int32_t)threadIdx.x <= 2 * R) w[threadIdx.x] = wts[threadIdx.x];
  const uint64_t px = (uint64_t)nx + 2;
  uint32_t bad = 0;
  float mx = 0.f;
  for (uint64_t row = blockIdx.x; row < rows; row += gridDim.x) {
    const float *s = src + row * px + 1;  // interior voxel 0 of the row
    float *d = dst + row * px + 1;
    for (int32_t a0 = 0; a0 < nx; a0 += VR_SMOOTH_SEG) {
      const int32_t cnt = nx - a0 < VR_SMOOTH_SEG ? nx - a0 : VR_SMOOTH_SEG;
      __syncthreads();  // the previous segment's reads (and the weights) are done / written
      for (int32_t t = (int32_t)threadIdx.x; t < cnt + 2 * R; t += 256) {
        int32_t c = a0 - R + t;
        c = c < 0 ? 0 : (c > nx - 1 ? nx - 1 : c);
        line[t] = (EPI && (flags & VR_EPI_LOAD_DATA)) ? vr_deconv_data(s[c]) : s[c];
      }
      __syncthreads();
      for (int32_t u = (int32_t)threadIdx.x; u < cnt; u += 256) {
        const float *x = line + u;
        const int32_t c = a0 + u;
        const float v = smooth_epilogue<EPI>(vr_smooth_tap(w, R, [x](int32_t k) { return x[k]; }), aux,
                                             row * px + 1 + (uint64_t)c, flr, flags);
        d[c] = v;
        if (c == 0) d[-1] = v;
        if (c == nx - 1) d[nx] = v;
        if (STATS) {
          if (!(fabsf(v) <= 3.4028234e38f)) bad = 1;
          else mx = fmaxf(mx, fabsf(v));
        }
      }
    }
  }
  if (STATS) smooth_fold_stats(bad, mx, st);
}

// Along y or z: lanes run along x, so every load and store is a line segment of 64 consecutive words.
// A workgroup iteration owns a tile of VR_SMOOTH_TX padded x positions by VR_SMOOTH_TA interior
// positions of the filtered axis at one position `o` of the third axis (all three padded ranges are
// covered: the apron lines of x and of the third axis are filtered like interior ones).  The tile and
// its halo of R lines on either side, at clamped coordinates, are staged in LDS, one line per wave and
// turn; wave v then computes the tile's outputs v, v + 4, ... from LDS column `lane`.
//   n: interior length of the filtered axis, astride its element stride, ostride the third axis',
//   no the third axis' padded length, px the padded row length.
template <bool STATS, int EPI>
__global__ __launch_bounds__(256) void smooth_s_kernel(const float *__restrict__ src, typename smooth_dst<EPI>::type dst,
                                                       uint32_t px, int32_t n, uint64_t astride, uint32_t no,
                                                       uint64_t ostride, uint64_t tiles,
                                                       const float *__restrict__ wts, int32_t R, BufStats *st,
                                                       const float *aux, float flr, uint32_t flags) {
  __shared__ float w[VR_SMOOTH_MAX_TAPS];
  __shared__ float tile[VR_SMOOTH_TA + 2 * VR_SMOOTH_MAX_RADIUS][VR_SMOOTH_TX];
  if ((int32_t)threadIdx.x <= 2 * R) w[threadIdx.x] = wts[threadIdx.x];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint32_t xchunks = (px + VR_SMOOTH_TX - 1) / VR_SMOOTH_TX;
  const uint32_t atiles = ((uint32_t)n + VR_SMOOTH_TA - 1) / VR_SMOOTH_TA;
  uint32_t bad = 0;
  float mx = 0.f;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const uint32_t xc = (uint32_t)(t % xchunks);
    const uint64_t r = t / xchunks;
    const int32_t a0 = (int32_t)(r % atiles) * VR_SMOOTH_TA;
    const uint64_t o = r / atiles;  // < no
    const uint32_t i = xc * VR_SMOOTH_TX + lane;
    const bool in = i < px;
    const int32_t cnt = n - a0 < VR_SMOOTH_TA ? n - a0 : VR_SMOOTH_TA;
    const uint64_t base = o * ostride + (uint64_t)i;  // position 0 of the filtered axis (its apron)
    __syncthreads();  // the previous tile's reads (and the weights) are done / written
    for (int32_t l = (int32_t)wave; l < cnt + 2 * R; l += 4) {
      int32_t c = a0 - R + l;
      c = c < 0 ? 0 : (c > n - 1 ? n - 1 : c);
      const float xv = in ? src[base + (uint64_t)(c + 1) * astride] : 0.f;
      tile[l][lane] = (EPI && (flags & VR_EPI_LOAD_DATA)) ? vr_deconv_data(xv) : xv;
    }
    __syncthreads();
    if (in) {
      for (int32_t u = (int32_t)wave; u < cnt; u += 4) {
        const float *x = &tile[u][lane];
        const int32_t c = a0 + u;
        const float v = smooth_epilogue<EPI>(vr_smooth_tap(w, R, [x](int32_t k) { return x[k * VR_SMOOTH_TX]; }), aux,
                                             base + (uint64_t)(c + 1) * astride, flr, flags);
        dst[base + (uint64_t)(c + 1) * astride] = v;
        if (c == 0) dst[base] = v;
        if (c == n - 1) dst[base + (uint64_t)(n + 1) * astride] = v;
        if (STATS) {
          if (!(fabsf(v) <= 3.4028234e38f)) bad = 1;
          else mx = fmaxf(mx, fabsf(v));
        }
      }
    }
  }
  (void)no;
  if (STATS) smooth_fold_stats(bad, mx, st);
}

// One axis pass, src -> dst (both padded (nx+2)(ny+2)(nz+2) floats, src with its apron in place, not
// aliasing): axis 0 / 1 / 2 along dims[0] / [1] / [2]; wts the 2R+1 weights in device memory, R in
// 1..VR_SMOOTH_MAX_RADIUS; st (may be null): *st += the statistics of dst.
template <bool STATS, int EPI>
static hipError_t launch_axis(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, int axis,
                              const float *wts, int32_t R, BufStats *st, const float *aux, float flr, uint32_t flags,
                              hipStream_t s) {
  const uint64_t px = (uint64_t)nx + 2, py = (uint64_t)ny + 2, pz = (uint64_t)nz + 2;
  if (axis == 0) {
    const uint64_t rows = py * pz;
    const unsigned blocks = (unsigned)(rows < 4096 ? rows : 4096);
    hipLaunchKernelGGL((smooth_x_kernel<STATS, EPI>), dim3(blocks), dim3(256), 0, s, src, dst, nx, rows, wts, R, st, aux,
                       flr, flags);
    return hipGetLastError();
  }
  const int32_t n = axis == 1 ? ny : nz;
  const uint64_t astride = axis == 1 ? px : px * py, ostride = axis == 1 ? px * py : px;
  const uint64_t no = axis == 1 ? pz : py;
  const uint64_t tiles = ((px + VR_SMOOTH_TX - 1) / VR_SMOOTH_TX) * (((uint64_t)n + VR_SMOOTH_TA - 1) / VR_SMOOTH_TA) * no;
  const unsigned blocks = (unsigned)(tiles < (1u << 16) ? tiles : (1u << 16));
  hipLaunchKernelGGL((smooth_s_kernel<STATS, EPI>), dim3(blocks), dim3(256), 0, s, src, dst, (uint32_t)px, n, astride,
                     (uint32_t)no, ostride, tiles, wts, R, st, aux, flr, flags);
  return hipGetLastError();
}

static bool axis_args_ok(const float *src, const float *dst, int32_t nx, int32_t ny, int32_t nz, int axis,
                         const float *wts, int32_t R) {
  return nx > 0 && ny > 0 && nz > 0 && axis >= 0 && axis <= 2 && R >= 1 && R <= VR_SMOOTH_MAX_RADIUS && src && dst &&
         src != dst && wts;
}

hipError_t launch_smooth_axis(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, int axis,
                              const float *wts, int32_t R, BufStats *st, hipStream_t s) {
  if (!axis_args_ok(src, dst, nx, ny, nz, axis, wts, R)) return hipErrorInvalidValue;
  return st ? launch_axis<true, 0>(src, dst, nx, ny, nz, axis, wts, R, st, nullptr, 0.f, 0u, s)
            : launch_axis<false, 0>(src, dst, nx, ny, nz, axis, wts, R, st, nullptr, 0.f, 0u, s);
}

// The same pass with an epilogue of the deconvolution (epi = VR_EPI_FILTER / RATIO / UPDATE and flags as
// above): aux the auxiliary padded buffer (RATIO, UPDATE; for UPDATE it may be dst), flr the rule's floor.
// Statistics are formed only by the update, whose output can be the final buffer.
hipError_t launch_deconv_axis(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, int axis,
                              const float *wts, int32_t R, int epi, const float *aux, float flr, uint32_t flags,
                              BufStats *st, hipStream_t s) {
  if (!axis_args_ok(src, dst, nx, ny, nz, axis, wts, R) || (epi != VR_EPI_FILTER && !aux) ||
      (epi != VR_EPI_UPDATE && (st || aux == dst)))
    return hipErrorInvalidValue;
  switch (epi) {
    case VR_EPI_FILTER:
      return launch_axis<false, VR_EPI_FILTER>(src, dst, nx, ny, nz, axis, wts, R, st, aux, flr, flags, s);
    case VR_EPI_RATIO:
      return launch_axis<false, VR_EPI_RATIO>(src, dst, nx, ny, nz, axis, wts, R, st, aux, flr, flags, s);
    case VR_EPI_UPDATE:
      return st ? launch_axis<true, VR_EPI_UPDATE>(src, dst, nx, ny, nz, axis, wts, R, st, aux, flr, flags, s)
                : launch_axis<false, VR_EPI_UPDATE>(src, dst, nx, ny, nz, axis, wts, R, st, aux, flr, flags, s);
  }
  return hipErrorInvalidValue;
}

// ---- the fused form: all three axes in one launch, each voxel read about once ---------------------------
// A workgroup owns a tile of VR_SMOOTH_FX x VR_SMOOTH_FY interior voxels and marches along z over a chunk
// of VR_SMOOTH_FZ planes.  Per input plane (clamped along z) it stages the tile with a halo of Rx columns
// and Ry rows at clamped coordinates (A), filters A along x into B (the tile's rows and their y halo),
// filters B along y into one slot of a ring of 2Rz+1 planes of the tile, and once the ring holds the
// planes c-Rz .. c+Rz writes output plane c as the z chain over the ring, oldest plane first.  Every value
// is the one the three passes form -- vr_smooth_tap over the same fp32 operands in the same order -- so
// the two forms agree bit for bit.  The apron of dst is stored with the edge outputs (up to 8 cells for a
// corner voxel).  LDS (dynamic): A, B, the ring and the three axes' weights, smooth_fused_lds() bytes.
#define VR_SMOOTH_FX 64
#define VR_SMOOTH_FY 16
#define VR_SMOOTH_FZ 256

static size_t smooth_fused_lds(int32_t Rx, int32_t Ry, int32_t Rz) {
  return sizeof(float) * ((size_t)(VR_SMOOTH_FY + 2 * Ry) * (size_t)(VR_SMOOTH_FX + 2 * Rx) +
                          (size_t)(VR_SMOOTH_FY + 2 * Ry) * VR_SMOOTH_FX +
                          (size_t)(2 * Rz + 1) * VR_SMOOTH_FY * VR_SMOOTH_FX + 3 * VR_SMOOTH_MAX_TAPS);
}

template <bool STATS>
__global__ __launch_bounds__(256) void smooth_fused_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                           int32_t nx, int32_t ny, int32_t nz,
                                                           const float *__restrict__ wts, int32_t Rx, int32_t Ry,
                                                           int32_t Rz, uint32_t tx, uint32_t ty, uint64_t tiles,
                                                           BufStats *st) {
  extern __shared__ float lds[];
  const int32_t AW = VR_SMOOTH_FX + 2 * Rx, AH = VR_SMOOTH_FY + 2 * Ry, RING = 2 * Rz + 1;
  float *w = lds;                          // [3][VR_SMOOTH_MAX_TAPS]
  float *A = w + 3 * VR_SMOOTH_MAX_TAPS;   // [AH][AW]
  float *B = A + AH * AW;                  // [AH][FX]
  float *ring = B + AH * VR_SMOOTH_FX;     // [RING][FY][FX]
  if (threadIdx.x < 3 * VR_SMOOTH_MAX_TAPS) w[threadIdx.x] = wts[threadIdx.x];
  const float *wx = w, *wy = w + VR_SMOOTH_MAX_TAPS, *wz = w + 2 * VR_SMOOTH_MAX_TAPS;
  const int32_t lane = (int32_t)(threadIdx.x & 63u), wave = (int32_t)(threadIdx.x >> 6);
  const uint64_t px = (uint64_t)nx + 2, pxy = px * ((uint64_t)ny + 2);
  uint32_t bad = 0;
  float mx = 0.f;
  for (uint64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    const int32_t i0 = (int32_t)(t % tx) * VR_SMOOTH_FX;
    const int32_t j0 = (int32_t)((t / tx) % ty) * VR_SMOOTH_FY;
    const int32_t zs = (int32_t)(t / ((uint64_t)tx * ty)) * VR_SMOOTH_FZ;
    const int32_t ze = nz - zs < VR_SMOOTH_FZ ? nz : zs + VR_SMOOTH_FZ;
    const int32_t i = i0 + lane;
    for (int32_t p = zs - Rz; p < ze + Rz; ++p) {  // input planes, unclamped index
      const int32_t pc = p < 0 ? 0 : (p > nz - 1 ? nz - 1 : p);
      const float *plane = src + (uint64_t)(pc + 1) * pxy;
      __syncthreads();  // the previous plane's reads of A, B and the ring (and the weights) are done / written
      for (int32_t r = wave; r < AH; r += 4) {
        int32_t j = j0 - Ry + r;
        j = j < 0 ? 0 : (j > ny - 1 ? ny - 1 : j);
        const float *row = plane + (uint64_t)(j + 1) * px + 1;
        for (int32_t q = lane; q < AW; q += 64) {
          int32_t c = i0 - Rx + q;
          c = c < 0 ? 0 : (c > nx - 1 ? nx - 1 : c);
          A[r * AW + q] = row[c];
        }
      }
      __syncthreads();
      for (int32_t r = wave; r < AH; r += 4) {
        const float *x = A + r * AW + lane;
        B[r * VR_SMOOTH_FX + lane] = vr_smooth_tap(wx, Rx, [x](int32_t k) { return x[k]; });
      }
      __syncthreads();
      float *slot = ring + (size_t)((p - (zs - Rz)) % RING) * (VR_SMOOTH_FY * VR_SMOOTH_FX);
      for (int32_t y = wave; y < VR_SMOOTH_FY; y += 4) {
        const float *x = B + y * VR_SMOOTH_FX + lane;
        slot[y * VR_SMOOTH_FX + lane] = vr_smooth_tap(wy, Ry, [x](int32_t k) { return x[k * VR_SMOOTH_FX]; });
      }
      const int32_t c = p - Rz;  // the output plane whose window the ring now holds
      if (c < zs) continue;      // (uniform: the ring is still filling)
      __syncthreads();
      const int32_t first = (c - zs) % RING;  // slot of plane c - Rz
      if (i < nx) {
        for (int32_t y = wave; y < VR_SMOOTH_FY; y += 4) {
          const int32_t j = j0 + y;
          if (j >= ny) break;
          const float *x = ring + y * VR_SMOOTH_FX + lane;
          const float v = vr_smooth_tap(wz, Rz, [x, first, RING](int32_t k) {
            int32_t sl = first + k;
            sl = sl >= RING ? sl - RING : sl;
            return x[(size_t)sl * (VR_SMOOTH_FY * VR_SMOOTH_FX)];
          });
          // the interior cell and the apron cells it replicates into
          const uint64_t xs[2] = {(uint64_t)i + 1, i == 0 ? 0u : (uint64_t)nx + 1};
          const uint64_t ys[2] = {(uint64_t)j + 1, j == 0 ? 0u : (uint64_t)ny + 1};
          const uint64_t zz[2] = {(uint64_t)c + 1, c == 0 ? 0u : (uint64_t)nz + 1};
          const int ax = (i == 0 || i == nx - 1) ? 2 : 1, ay = (j == 0 || j == ny - 1) ? 2 : 1,
                    az = (c == 0 || c == nz - 1) ? 2 : 1;
          for (int a = 0; a < az; ++a)
            for (int b = 0; b < ay; ++b)
              for (int e = 0; e < ax; ++e) dst[zz[a] * pxy + ys[b] * px + xs[e]] = v;
          if (STATS) {
            if (!(fabsf(v) <= 3.4028234e38f)) bad = 1;
            else mx = fmaxf(mx, fabsf(v));
          }
        }
      }
    }
  }
  if (STATS) smooth_fold_stats(bad, mx, st);
}

// All three axes at once, src -> dst (both padded, src with its apron in place, not aliasing): wts the
// three axes' weights in device memory, VR_SMOOTH_MAX_TAPS floats per axis; every dim at least 2 and every
// radius in 1..VR_SMOOTH_MAX_RADIUS; st (may be null): *st += the statistics of dst.
hipError_t launch_smooth_fused(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, const float *wts,
                               int32_t Rx, int32_t Ry, int32_t Rz, BufStats *st, hipStream_t s) {
  if (nx < 2 || ny < 2 || nz < 2 || !src || !dst || src == dst || !wts || Rx < 1 || Ry < 1 || Rz < 1 ||
      Rx > VR_SMOOTH_MAX_RADIUS || Ry > VR_SMOOTH_MAX_RADIUS || Rz > VR_SMOOTH_MAX_RADIUS)
    return hipErrorInvalidValue;
  const size_t lds = smooth_fused_lds(Rx, Ry, Rz);
  auto *k = st ? smooth_fused_kernel<true> : smooth_fused_kernel<false>;
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  const uint32_t tx = ((uint32_t)nx + VR_SMOOTH_FX - 1) / VR_SMOOTH_FX, ty = ((uint32_t)ny + VR_SMOOTH_FY - 1) / VR_SMOOTH_FY;
  const uint64_t tiles = (uint64_t)tx * ty * (((uint64_t)nz + VR_SMOOTH_FZ - 1) / VR_SMOOTH_FZ);
  const unsigned blocks = (unsigned)(tiles < (1u << 20) ? tiles : (1u << 20));
  hipLaunchKernelGGL(k, dim3(blocks), dim3(256), lds, s, src, dst, nx, ny, nz, wts, Rx, Ry, Rz, tx, ty, tiles, st);
  return hipGetLastError();
}

}  // namespace vr
