// vr_slice.hip -- gfx950 (MI355X, CDNA4) slice kernel: an axis-aligned or oblique section of a
// resident volume and its thick-slab reductions (include/vrhip.h vr_render_slice).
//
// slice_kernel evaluates the sampler of every render (vr_sampling.h axis / fetch<BIG>, the unbound and
// 1x1x1 cases as tex3d) on a plane instead of along camera rays: sample k of pixel (y, x) sits at
//   p_j = fmaf(dv_j, (float)y, fmaf(du_j, (float)x, origin_j)),  q_kj = fmaf(dw_j, (float)k, p_j)
// -- no recurrence, so no bit depends on how the samples are ordered or batched.  A sample outside
// [0, 1]^3 (a NaN coordinate included) is skipped; the inside ones are reduced in the order of k: a
// strict running maximum or minimum with the k of its first occurrence, or an fp32 sum with its count.
// One lane per output pixel.
//
// Loads in flight: the samples do not depend on each other, so a lane takes VR_SLICE_BATCH of them at
// a time -- all coordinates and row loads first, then the fold in order (the projections' scheme,
// vr_project.hip); what is left of n after the whole batches is taken one sample at a time, so no
// sample past n is computed.  The texture's kind is decided outside the sample loop.  A batch whose every sample
// is outside in every lane of the wave issues no load (a wave-uniform skip); a lane that is outside
// while its neighbours are inside loads from the clamped cell axis() gives every coordinate -- +-inf
// and NaN included, so every address stays inside the padded volume -- and its value is not folded.
//
// Lane axis (LANES_X): a gather's cost is the cache lines a wave touches.  The host (vr_capi.hip
// do_slice) picks per launch whether a wave's 64 lanes run along the output's rows y (the store of a
// column-major plane is then contiguous) or along its columns x; a workgroup is 4 waves side by side
// on the other axis.  A launch-wide decision that changes no bit.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <type_traits>

#include "vr_device.h"
#include "vr_sampling.h"
#include "vr_slice.h"

#ifndef VR_SLICE_BATCH
#define VR_SLICE_BATCH 2  // samples whose loads are issued before any is consumed (measured: DESIGN.md s16)
#endif

namespace vr {

// MODE 0: maximum (aux: k of the first maximum), 1: minimum (likewise), 2: sum (aux: inside samples).
// LABELS: the label plane is written from the resident label bytes (without them the host fills it).
template <int MODE, bool BIG, bool LABELS>
__global__ __launch_bounds__(256) void slice_kernel(const SliceParams S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // blocks along the lane axis fastest; a block is 64 pixels of the lane axis by 4 of the other
  const uint32_t nla = S.lanes_x ? ((uint32_t)S.width + 63u) >> 6 : ((uint32_t)S.height + 63u) >> 6;
  const uint32_t ba = blockIdx.x % nla, bo = blockIdx.x / nla;
  const int a = (int)(ba * 64u) + lane, o = (int)(bo * 4u) + wave;
  const int x = S.lanes_x ? a : o, y = S.lanes_x ? o : a;
  const bool active = x < S.width && y < S.height;
  const float fx = (float)x, fy = (float)y;
  const float p0 = fmaf(S.dv[0], fy, fmaf(S.du[0], fx, S.origin[0]));
  const float p1 = fmaf(S.dv[1], fy, fmaf(S.du[1], fx, S.origin[1]));
  const float p2 = fmaf(S.dv[2], fy, fmaf(S.du[2], fx, S.origin[2]));
  auto inside = [](float c0, float c1, float c2) {  // (a NaN fails every comparison)
    return c0 >= 0.f && c0 <= 1.f && c1 >= 0.f && c1 <= 1.f && c2 >= 0.f && c2 <= 1.f;
  };

  // the source texture's state, wave-uniform: 0 unbound (reads 0), 1 a single voxel, 2 a grid
  const int kind = S.tex.p == nullptr ? 0 : (S.tex.one ? 1 : 2);
  float one = 0.f;
  if (kind == 1) {
    const float q = S.tex.p[0];
    one = fmaf(0.5f, q - q, q);  // == lerp(q, q, w) for every w (tex3d)
  }

  float m = MODE == 0 ? -INFINITY : INFINITY;  // MODE 0 / 1: the extremum and the k of its first occurrence
  int km = -1;
  float s = 0.f;  // MODE 2: the sum and the count
  int cnt = 0;
  const int n = S.samples;
  // B consecutive samples from k on: coordinates and row loads of all of them, then the fold in order
  auto take = [&](int k, auto bc) __attribute__((always_inline)) {
    constexpr int B = decltype(bc)::value;
    float v[B];
    bool in[B];
    float q0[B], q1[B], q2[B];
    bool any = false;
#pragma unroll
    for (int j = 0; j < B; ++j) {
      const float fk = (float)(k + j);
      q0[j] = fmaf(S.dw[0], fk, p0);
      q1[j] = fmaf(S.dw[1], fk, p1);
      q2[j] = fmaf(S.dw[2], fk, p2);
      in[j] = active && inside(q0[j], q1[j], q2[j]);
      any = any || in[j];
    }
    if (!__any(any)) return;  // wave-uniform: the whole batch is outside, no load
    if (kind == 2) {
#pragma unroll
      for (int j = 0; j < B; ++j)
        v[j] = fetch<BIG>(S.tex, axis(q0[j], S.tex.nx, S.tex.fnx), axis(q1[j], S.tex.ny, S.tex.fny),
                          axis(q2[j], S.tex.nz, S.tex.fnz));
    } else {
#pragma unroll
      for (int j = 0; j < B; ++j) v[j] = one;  // (unbound: 0)
    }
#pragma unroll
    for (int j = 0; j < B; ++j) {
      if (MODE == 0) {
        if (in[j] && v[j] > m) {  // strictly greater: the first maximum wins, a NaN never does
          m = v[j];
          km = k + j;
        }
      } else if (MODE == 1) {
        if (in[j] && v[j] < m) {
          m = v[j];
          km = k + j;
        }
      } else {
        if (in[j]) {
          s = s + v[j];
          ++cnt;
        }
      }
    }
  };
  // whole batches, then the rest one by one: no sample past n is computed or loaded (n = 1, the plain
  // slice, is one sample)
  int k = 0;
  for (; k + VR_SLICE_BATCH <= n; k += VR_SLICE_BATCH) take(k, std::integral_constant<int, VR_SLICE_BATCH>{});
  for (; k < n; ++k) take(k, std::integral_constant<int, 1>{});

  if (!active) return;
  const float qnan = __uint_as_float(0x7fc00000u);
  const size_t idx = (size_t)x * (size_t)S.height + (size_t)y;  // [H, W] column-major
  float px, ax;
  if (MODE == 2) {
    px = cnt > 0 ? s : qnan;
    ax = (float)cnt;
  } else {
    px = km >= 0 ? m + 0.0f : qnan;  // (-0 -> +0)
    ax = km >= 0 ? (float)km : qnan;
  }
  S.out[idx] = px;
  if (S.aux != nullptr) S.aux[idx] = ax;
  if constexpr (LABELS) {
    const float fk = (float)((n - 1) / 2);
    const float c0 = fmaf(S.dw[0], fk, p0), c1 = fmaf(S.dw[1], fk, p1), c2 = fmaf(S.dw[2], fk, p2);
    float lv = qnan;
    if (inside(c0, c1, c2)) {  // c in [0, 1]: every index in [0, D - 1]
      const int i0 = min((int)(c0 * (float)S.ld[0]), S.ld[0] - 1);
      const int i1 = min((int)(c1 * (float)S.ld[1]), S.ld[1] - 1);
      const int i2 = min((int)(c2 * (float)S.ld[2]), S.ld[2] - 1);
      lv = (float)S.labels[(size_t)i0 + (size_t)S.ld[0] * ((size_t)i1 + (size_t)S.ld[1] * (size_t)i2)];
    }
    S.lab[idx] = lv;
  }
}

// ------------------------------------------------------------------------------------------------
// launch helper (called from vr_capi.hip)

template <int MODE, bool BIG>
static void launch_l(const SliceParams &S, dim3 grid, hipStream_t s) {
  if (S.lab != nullptr && S.labels != nullptr) hipLaunchKernelGGL((slice_kernel<MODE, BIG, true>), grid, dim3(256), 0, s, S);
  else hipLaunchKernelGGL((slice_kernel<MODE, BIG, false>), grid, dim3(256), 0, s, S);
}

template <int MODE>
static void launch_b(const SliceParams &S, bool big, dim3 grid, hipStream_t s) {
  if (big) launch_l<MODE, true>(S, grid, s);
  else launch_l<MODE, false>(S, grid, s);
}

// mode: vr_slice_mode.  S.lab without S.labels is not written here (the host fills it with NaN).
hipError_t launch_slice(const SliceParams &S, int mode, bool big, hipStream_t s) {
  if (S.width <= 0 || S.height <= 0) return hipSuccess;
  if (mode < 0 || mode > 2 || S.samples < 1 || S.out == nullptr) return hipErrorInvalidValue;
  const uint64_t la = (uint64_t)(S.lanes_x ? S.width : S.height), lo = (uint64_t)(S.lanes_x ? S.height : S.width);
  const uint64_t blocks = ((la + 63) / 64) * ((lo + 3) / 4);
  if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
  const dim3 grid((unsigned)blocks);
  if (mode == 0) launch_b<0>(S, big, grid, s);
  else if (mode == 1) launch_b<1>(S, big, grid, s);
  else launch_b<2>(S, big, grid, s);
  return hipGetLastError();
}

}  // namespace vr
