// vr_isosurface.hip -- gfx950 (MI355X, CDNA4) first-hit isosurface render: the opaque surface
// v = level of the emission texture, lit by the frame's lights, with its depth and normal planes
// (include/vrhip.h vr_render_isosurface).
//
// isosurface_kernel marches exactly the ray of render_kernel and project_kernel (ray_setup, tnear
// clamped to 0, t += tstep, pos += step, the max_steps cap), with no opacity exit, and stops a ray at
// its first sample k with v_k >= level (a NaN sample is never >=).  One lane per ray.
//
// Search: the loop of the one-lane feature kernels, built from vr_raycast.h (pixel, ray start, emission
// sampler, recurrence, probe) -- positions and row loads of VR_ISO_BATCH consecutive samples first, then
// the fold in sample order.  A lane that hits keeps pos_{k-1} and t_{k-1} (the position
// and t of the last sample below the level) and goes dead; the wave leaves the loop on !__any(alive).
//
// Empty-space leap (PROBE): the probe of vr_raycast.h (probe_step), launched only for level > 0: a
// leaped run's samples are +-0 and cannot reach a positive level.  The run is replayed as ps - 1
// samples and one more, so that a ray whose first sample after the run hits knows pos_{k-1}.
//
// After the loop, once per lane and under the lane's mask: VR_ISO_REFINE dependent bisection fetches
// on the segment (pos_{k-1}, pos_k], the sample at the surface point, the gradient by the handle's
// method with the oracle's expressions (never the half-texel fast taps), and shade_lights<false>.
// There is one shaded sample per pixel, so the exact arithmetic costs nothing measurable.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <type_traits>

#include "vr_raycast.h"

#ifndef VR_ISO_REFINE
#define VR_ISO_REFINE 6  // bisection steps between the last sample below the level and the hit (vrhip.h)
#endif
#ifndef VR_ISO_BATCH
#define VR_ISO_BATCH 4  // samples whose loads are issued before any is tested (measured: DESIGN.md s11)
#endif
#ifndef VR_ISO_PROBE_MIN
#define VR_ISO_PROBE_MIN 64  // the probe's first run after the march enters empty space
#endif
#ifndef VR_ISO_PROBE_REST
#define VR_ISO_PROBE_REST 4  // batches marched after a failed probe before an all-zero batch re-arms it
#endif

namespace vr {

// The launch arguments that are not RenderParams (Args, vr_raycast.h): the level, the depth plane --
// [plane_cols][H] as one plane of the image, or null -- and the normal planes -- [3][plane_cols][H] as
// the image, or null.
struct IsoExtras {
  float level;
  float *depth;
  float *normal;
};

// GRAD 1: on-the-fly gradient (six taps of the gem binding), 2: lookup (gx, gy, gz).
// COUNT: steps[0] += search samples visited (leaped ones included), steps[1] += search samples
// fetched, steps[2] += surface pixels.
// CLIP: the clip planes shorten [tnear, tfar] after ray_setup.  A hit at the first sample is then the
// surface point itself (k = 0): the plane cuts the object as the box face does, a capped cut face.
template <int GRAD, bool BIG, bool PROBE, bool COUNT, bool CLIP>
__global__ __launch_bounds__(256) void isosurface_kernel(const RenderParams P, const Args<IsoExtras, CLIP> X) {
  int tx, ty;
  if (!tile_of_block(P, tx, ty)) return;  // whole workgroup: uniform
  const Pixel px = pixel_of_tile(P, tx, ty);
  const int lane = px.lane;
  const f3 bmin = mk(P.bmin[0], P.bmin[1], P.bmin[2]);
  const f3 bsc = mk(P.bscale[0], P.bscale[1], P.bscale[2]);
  const float tstep = P.tstep, level = X.level;

  const RayStart r = ray_start<CLIP>(P, X, px.active, px.lc, px.y, bmin, tstep);
  const float tfar = r.tfar;
  const f3 step = r.step;
  float t = r.t;
  f3 pos = r.pos;
  bool alive = r.hit;
  int32_t nsteps = 0, nfetch = 0;
  // the search's result: found -- sample k reached the level; first -- k == 0; (bpos, bt) -- the
  // position and t of sample k - 1 (of sample 0 when first); (qpos, qt) -- those of the lane's last
  // sample below the level so far
  bool found = false, first = false;
  f3 bpos = bmin, qpos = bmin;
  float bt = 0.f, qt = 0.f;

  const Emission em = emission_of(P);
  Probe prb;
  if constexpr (PROBE) prb = probe_arm<VR_ISO_PROBE_MIN>(em.kind, tstep, alive, pos, step, t);

  while (__any(alive)) {
    if constexpr (PROBE) {
      // the run's samples are +-0 < level: none hits.  The last of them is a live ray's k - 1.
      const auto on_empty = [&](int ps) __attribute__((always_inline)) {
        leap(P, ps - 1, alive, nsteps, t, tfar, pos, step);
        if (alive) {
          qpos = pos;
          qt = t;
        }
        leap(P, 1, alive, nsteps, t, tfar, pos, step);
      };
      if (probe_step<VR_ISO_PROBE_MIN, VR_ISO_PROBE_REST>(P, prb, alive, pos, step, t, tfar, lane, on_empty)) continue;
    }
    // ---- a batch: positions and loads of VR_ISO_BATCH consecutive samples, then the fold -------
    float v[VR_ISO_BATCH], tt[VR_ISO_BATCH];
    f3 pp[VR_ISO_BATCH];
    bool lv[VR_ISO_BATCH];
    const int32_t n0 = nsteps;
    auto batch = [&](auto grid) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < VR_ISO_BATCH; ++j) {
        lv[j] = alive;
        tt[j] = t;
        pp[j] = pos;
        v[j] = em_at<BIG>(P, grid, em.one, bmin, bsc, pos);
        next_sample(P, tstep, tfar, step, alive, nsteps, t, pos);
      }
    };
    if (em.kind == 2) batch(std::true_type{});
    else batch(std::false_type{});
    bool nz = false;
#pragma unroll
    for (int j = 0; j < VR_ISO_BATCH; ++j) {
      if (lv[j] && !found) {  // (lv is monotone within a batch: samples 0 .. j of it were all taken)
        if (COUNT) ++nfetch;
        if (v[j] >= level) {  // the first sample at or above the level; a NaN never is
          found = true;
          first = (n0 + j) == 0;
          bpos = first ? pp[j] : qpos;
          bt = first ? tt[j] : qt;
          nsteps = n0 + j + 1;  // the ray stops here
        } else {
          qpos = pp[j];
          qt = tt[j];
        }
        if (PROBE) nz = nz || !(v[j] == 0.f);
      }
    }
    alive = alive && !found;
    if constexpr (PROBE) probe_rearm<VR_ISO_PROBE_MIN>(prb, nz);
  }

  // ---- the surface sample: once per lane, under the lane's mask -------------------------------------
  const float qnan = __uint_as_float(0x7fc00000u);
  float pr = 0.f, pg = 0.f, pb = 0.f, ts = qnan;
  f3 n = mk(qnan, qnan, qnan);
  if (__any(found)) {  // wave-uniform; a lane without a surface computes at the box corner, unwritten
    // refinement: hi in (0, 1] with the sample at fma(step, hi, pos_{k-1}) at or above the level
    float lo = 0.f, hi = 1.f;
#pragma unroll 1
    for (int i = 0; i < VR_ISO_REFINE; ++i) {
      const float c = (lo + hi) * 0.5f;  // exact
      const f3 pc = mk(fmaf(step.x, c, bpos.x), fmaf(step.y, c, bpos.y), fmaf(step.z, c, bpos.z));
      const float vc = em_at<BIG>(P, em.kind, em.one, bmin, bsc, pc);
      if (vc >= level) hi = c;
      else lo = c;
    }
    // hi = 1 gives pos_k and t_k bit for bit; k = 0: the first sample itself (the box face cuts the object)
    const f3 p = first ? bpos : mk(fmaf(step.x, hi, bpos.x), fmaf(step.y, hi, bpos.y), fmaf(step.z, hi, bpos.z));
    const float tsur = first ? bt : fmaf(tstep, hi, bt);
    const f3 s = tex_coord(bmin, bsc, p);
    const float vs = em_at<BIG>(P, em.kind, em.one, bmin, bsc, p);
    // the gradient render's exact shading takes (render_kernel without SHARE: the oracle's expressions)
    f3 g;
    if (GRAD == 1) {
      const float xp = ((p.x + P.gstep[0]) - bmin.x) * bsc.x;
      const float xm = ((p.x - P.gstep[0]) - bmin.x) * bsc.x;
      const float yp = ((p.y + P.gstep[1]) - bmin.y) * bsc.y;
      const float ym = ((p.y - P.gstep[1]) - bmin.y) * bsc.y;
      const float zp = ((p.z + P.gstep[2]) - bmin.z) * bsc.z;
      const float zm = ((p.z - P.gstep[2]) - bmin.z) * bsc.z;
      g.x = tex3d<BIG>(P.gem, xp, s.y, s.z) - tex3d<BIG>(P.gem, xm, s.y, s.z);
      g.y = tex3d<BIG>(P.gem, s.x, yp, s.z) - tex3d<BIG>(P.gem, s.x, ym, s.z);
      g.z = tex3d<BIG>(P.gem, s.x, s.y, zp) - tex3d<BIG>(P.gem, s.x, s.y, zm);
      g = mk(g.x * 0.5f, g.y * 0.5f, g.z * 0.5f);
    } else {
      g = mk(tex3d<BIG>(P.gx, s.x, s.y, s.z), tex3d<BIG>(P.gy, s.x, s.y, s.z), tex3d<BIG>(P.gz, s.x, s.y, s.z));
    }
    // n = -normalize(g) as shade_lights<false> forms it (a zero gradient: 0 * inf = NaN, as render)
    const float ginv = 1.f / sqrt_cr(dot3(g, g));
    float ir = 0.f, ig = 0.f, ib = 0.f;
    if (P.num_lights > 0) {  // (the host passes 0 without a LUT)
      const float refl = P.fr * (P.re_is_em ? vs : tex3d<BIG>(P.re, s.x, s.y, s.z));
      shade_lights<false>(P, g, p, mk(P.eye[0], P.eye[1], P.eye[2]), refl, ir, ig, ib);
    }
    if (found) {
      const float e = P.fe * vs;
      pr = fmaf(e, P.color[0], ir);
      pg = fmaf(e, P.color[1], ig);
      pb = fmaf(e, P.color[2], ib);
      ts = tsur;
      n = mk(-(g.x * ginv), -(g.y * ginv), -(g.z * ginv));
    }
  }

  if (px.active) {
    const size_t plane = px.plane(P), k = px.k(P);  // depth and normal as planes of the image
    P.out[k] = pr;
    P.out[k + plane] = pg;
    P.out[k + 2 * plane] = pb;
    if (X.depth != nullptr) X.depth[k] = ts;
    if (X.normal != nullptr) {
      X.normal[k] = n.x;
      X.normal[k + plane] = n.y;
      X.normal[k + 2 * plane] = n.z;
    }
  }
  if (COUNT) {
    unsigned long long c[3] = {(unsigned long long)nsteps, (unsigned long long)nfetch, found ? 1ull : 0ull};
    add_steps(P.steps, lane, c);
  }
}

// ------------------------------------------------------------------------------------------------
// launch helper (called from vr_capi.hip)

// grad: 1 on-the-fly, 2 lookup; probe: leap empty space (needs P.occ and a level above 0); clip: the
// launch's plane set, or null / n == 0: the unclipped instantiations
hipError_t launch_isosurface(const RenderParams &P, int grad, float level, float *depth, float *normal, bool big,
                             bool probe, hipStream_t s, const ClipSet *clip) {
  if (P.part_cols <= 0 || P.height <= 0) return hipSuccess;
  if (grad != 1 && grad != 2) return hipErrorInvalidValue;
  WithClip<IsoExtras> X{};
  X.level = level;
  X.depth = depth;
  X.normal = normal;
  if (clip) X.clip = *clip;
  probe = probe && P.occ != nullptr && P.occ_bx != 0u && level > 0.f;
  with_bools(
      [&](auto big, auto probe, auto count, auto clipped) {
        constexpr bool B = decltype(big)::value, PR = decltype(probe)::value, C = decltype(count)::value,
                       CL = decltype(clipped)::value;
        const Args<IsoExtras, CL> &A = X;
        if (grad == 1) hipLaunchKernelGGL((isosurface_kernel<1, B, PR, C, CL>), tile_grid(P), dim3(256), 0, s, P, A);
        else hipLaunchKernelGGL((isosurface_kernel<2, B, PR, C, CL>), tile_grid(P), dim3(256), 0, s, P, A);
      },
      big, probe, P.steps != nullptr, X.clip.n > 0);
  return hipGetLastError();
}

}  // namespace vr
