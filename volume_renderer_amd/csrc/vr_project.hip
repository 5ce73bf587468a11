// vr_project.hip -- gfx950 (MI355X, CDNA4) projection kernels: maximum-intensity projection with
// the depth of the maximum, and the ray sum (include/vrhip.h vr_render_projection).
//
// project_kernel marches exactly the ray of render_kernel (vr_kernels.hip): the same pixel-to-ray
// mapping and box intersection (ray_setup), tnear clamped to 0, the recurrences t += tstep and
// pos += step, the max_steps cap -- and no early exit, so a ray takes every sample render would take
// with an opacity threshold that is never reached.  Each sample is the trilinear fetch of the
// emission texture (axis / fetch<BIG>, the unbound and 1x1x1 cases as tex3d), reduced instead of
// composited: a strict running maximum with the t of its first occurrence, or an fp32 sum in sample
// order.  One lane per ray, no depth lanes: the addition order and the first-maximum rule are part
// of the contract.
//
// Loads in flight: samples do not depend on each other (there is no running opacity), so the wave
// takes VR_PROJ_BATCH consecutive samples at a time -- positions and row loads of all of them
// first, then the fold in sample order.  A lane whose ray ended inside a batch keeps its last
// position (its loads stay in bounds: axis() clamps every index into the padded volume) and its
// values are not folded.  VR_PROJ_BATCH=1 is the plain loop (an A/B build).
//
// The pixel mapping, the ray start, the emission sampler, the recurrence, the probe's state machine and
// the counters are vr_raycast.h's, shared with isosurface_kernel.
//
// Empty-space leap (PROBE): as the march's probe (vr_stage.h probe_run) -- when every centre tap of
// the live rays' next L samples lies in all-zero bricks of the emission texture's occupancy map,
// each of those samples is +-0 and only the recurrences are replayed (leap).  For the maximum a
// live lane takes the run as the value +0 at its first sample: the samples are +-0, the strict
// comparison lets only the first of them win, and the pixel is formed from m + 0.0f, so -0 and +0
// maxima write the same bits.  For the sum the run adds nothing: s starts at +0 and is never -0, so
// s + +-0 == s.  Both planes are bit-identical with and without the probe.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <type_traits>

#include "vr_raycast.h"

#ifndef VR_PROJ_BATCH
#define VR_PROJ_BATCH 2  // samples whose loads are issued before any is consumed (measured: DESIGN.md s10)
#endif
#ifndef VR_PROJ_PROBE_MIN
#define VR_PROJ_PROBE_MIN 64  // the probe's first run after the march enters empty space
#endif
#ifndef VR_PROJ_PROBE_REST
#define VR_PROJ_PROBE_REST 4  // batches marched after a failed probe before an all-zero batch re-arms it
#endif

namespace vr {

// The launch arguments that are not RenderParams (Args, vr_raycast.h): the aux plane --
// [plane_cols][H] as one plane of the image, or null.
struct ProjectExtras {
  float *aux;
};

// MODE 0: maximum-intensity projection (aux: t of the first maximum), 1: ray sum (aux: samples).
// COUNT: steps[0] += samples visited (leaped ones included), steps[1] += samples fetched.
// CLIP: the clip planes shorten [tnear, tfar] after ray_setup; the march and the leap start from there.
template <int MODE, bool BIG, bool PROBE, bool COUNT, bool CLIP>
__global__ __launch_bounds__(256) void project_kernel(const RenderParams P, const Args<ProjectExtras, CLIP> X) {
  int tx, ty;
  if (!tile_of_block(P, tx, ty)) return;  // whole workgroup: uniform
  const Pixel px = pixel_of_tile(P, tx, ty);
  const int lane = px.lane;
  const f3 bmin = mk(P.bmin[0], P.bmin[1], P.bmin[2]);
  const f3 bsc = mk(P.bscale[0], P.bscale[1], P.bscale[2]);
  const float tstep = P.tstep;

  const RayStart r = ray_start<CLIP>(P, X, px.active, px.lc, px.y, bmin, tstep);
  const bool hit = r.hit;
  const float tfar = r.tfar;
  const f3 step = r.step;
  float t = r.t;
  f3 pos = r.pos;
  bool alive = hit;
  int32_t nsteps = 0, nfetch = 0;
  float m = -INFINITY, tm = 0.f;  // MODE 0: the maximum and the t of its first occurrence
  float s = 0.f;                  // MODE 1

  const Emission em = emission_of(P);
  Probe prb;
  if constexpr (PROBE) prb = probe_arm<VR_PROJ_PROBE_MIN>(em.kind, tstep, alive, pos, step, t);

  while (__any(alive)) {
    if constexpr (PROBE) {
      const auto on_empty = [&](int ps) __attribute__((always_inline)) {
        if (MODE == 0 && alive && 0.f > m) {  // the run's samples are +-0: the first one wins
          m = 0.f;
          tm = t;
        }
        leap(P, ps, alive, nsteps, t, tfar, pos, step);
      };
      if (probe_step<VR_PROJ_PROBE_MIN, VR_PROJ_PROBE_REST>(P, prb, alive, pos, step, t, tfar, lane, on_empty)) continue;
    }
    // ---- a batch: positions and loads of VR_PROJ_BATCH consecutive samples, then the fold ------
    float v[VR_PROJ_BATCH], tt[VR_PROJ_BATCH];
    bool lv[VR_PROJ_BATCH];
    auto batch = [&](auto grid) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < VR_PROJ_BATCH; ++j) {
        lv[j] = alive;
        tt[j] = t;
        v[j] = em_at<BIG>(P, grid, em.one, bmin, bsc, pos);
        next_sample(P, tstep, tfar, step, alive, nsteps, t, pos);
      }
    };
    if (em.kind == 2) batch(std::true_type{});
    else batch(std::false_type{});
    bool nz = false;
#pragma unroll
    for (int j = 0; j < VR_PROJ_BATCH; ++j) {
      if (MODE == 0) {
        if (lv[j] && v[j] > m) {  // strictly greater: the first maximum wins, a NaN never does
          m = v[j];
          tm = tt[j];
        }
      } else {
        if (lv[j]) s = s + v[j];
      }
      if (COUNT) nfetch += lv[j] ? 1 : 0;
      if (PROBE) nz = nz || (lv[j] && !(v[j] == 0.f));
    }
    if constexpr (PROBE) probe_rearm<VR_PROJ_PROBE_MIN>(prb, nz);
  }

  if (px.active) {
    const size_t plane = px.plane(P), k = px.k(P);  // the aux plane as one plane of the image
    float p = 0.f, a;
    if (MODE == 0) {
      const bool won = m > -INFINITY;
      a = won ? tm : __uint_as_float(0x7fc00000u);
      if (won) p = P.fe * (m + 0.0f);  // (-0 -> +0)
    } else {
      a = (float)nsteps;
      if (hit) p = (P.fe * s) * tstep;
    }
    const bool wr = MODE == 0 ? (m > -INFINITY) : hit;
    P.out[k] = wr ? p * P.color[0] : 0.f;
    P.out[k + plane] = wr ? p * P.color[1] : 0.f;
    P.out[k + 2 * plane] = wr ? p * P.color[2] : 0.f;
    if (X.aux != nullptr) X.aux[k] = a;
  }
  if (COUNT) {
    unsigned long long c[2] = {(unsigned long long)nsteps, (unsigned long long)nfetch};
    add_steps(P.steps, lane, c);
  }
}

// ------------------------------------------------------------------------------------------------
// launch helper (called from vr_capi.hip)

// mode: vr_projection (0 maximum, 1 sum); probe: leap empty space (needs P.occ); clip: the launch's
// plane set, or null / n == 0: the unclipped instantiations
hipError_t launch_project(const RenderParams &P, int mode, float *aux, bool big, bool probe, hipStream_t s,
                          const ClipSet *clip) {
  if (P.part_cols <= 0 || P.height <= 0) return hipSuccess;
  if (mode != 0 && mode != 1) return hipErrorInvalidValue;
  WithClip<ProjectExtras> X{};
  X.aux = aux;
  if (clip) X.clip = *clip;
  probe = probe && P.occ != nullptr && P.occ_bx != 0u;
  with_bools(
      [&](auto big, auto probe, auto count, auto clipped) {
        constexpr bool B = decltype(big)::value, PR = decltype(probe)::value, C = decltype(count)::value,
                       CL = decltype(clipped)::value;
        const Args<ProjectExtras, CL> &A = X;
        if (mode == 0) hipLaunchKernelGGL((project_kernel<0, B, PR, C, CL>), tile_grid(P), dim3(256), 0, s, P, A);
        else hipLaunchKernelGGL((project_kernel<1, B, PR, C, CL>), tile_grid(P), dim3(256), 0, s, P, A);
      },
      big, probe, P.steps != nullptr, X.clip.n > 0);
  return hipGetLastError();
}

}  // namespace vr
