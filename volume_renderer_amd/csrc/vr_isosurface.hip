// vr_isosurface.hip -- gfx950 (MI355X, CDNA4) first-hit isosurface render: the opaque surface
// v = level of the emission texture, lit by the frame's lights, with its depth and normal planes
// (include/vrhip.h vr_render_isosurface).
//
// isosurface_kernel marches exactly the ray of render_kernel and project_kernel (ray_setup, tnear
// clamped to 0, t += tstep, pos += step, the max_steps cap), with no opacity exit, and stops a ray at
// its first sample k with v_k >= level (a NaN sample is never >=).  One lane per ray.
//
// Search: the projection kernel's loop -- positions and row loads of VR_ISO_BATCH consecutive samples
// first, then the fold in sample order.  A lane that hits keeps pos_{k-1} and t_{k-1} (the position
// and t of the last sample below the level) and goes dead; the wave leaves the loop on !__any(alive).
//
// Empty-space leap (PROBE): probe_run / leap as the projection kernel, launched only for level > 0: a
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

#include "vr_clip.h"
#include "vr_device.h"
#include "vr_sampling.h"
#include "vr_stage.h"

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

// The launch arguments that are not RenderParams (which must not grow, vr_device.h): the level, the
// depth plane -- [plane_cols][H] as one plane of the image, or null -- and the normal planes --
// [3][plane_cols][H] as the image, or null.
struct IsoExtras {
  float level;
  float *depth;
  float *normal;
};
// The same for a clipped instantiation, with the plane set (vr_clip.h).  The unclipped kernels keep
// the arguments they had before there were planes.
struct IsoExtrasClip : IsoExtras {
  ClipSet clip;
};
template <bool CLIP>
using IsoArgs = std::conditional_t<CLIP, IsoExtrasClip, IsoExtras>;

// GRAD 1: on-the-fly gradient (six taps of the gem binding), 2: lookup (gx, gy, gz).
// COUNT: steps[0] += search samples visited (leaped ones included), steps[1] += search samples
// fetched, steps[2] += surface pixels.
// CLIP: the clip planes shorten [tnear, tfar] after ray_setup.  A hit at the first sample is then the
// surface point itself (k = 0): the plane cuts the object as the box face does, a capped cut face.
template <int GRAD, bool BIG, bool PROBE, bool COUNT, bool CLIP>
__global__ __launch_bounds__(256) void isosurface_kernel(const RenderParams P, const IsoArgs<CLIP> X) {
  // tile and lane mapping of project_kernel / render_kernel
  int tx, ty;
  if (!tile_of_block(P, tx, ty)) return;  // whole workgroup: uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = tx * 16 + (wave & 1) * 8 + (lane >> 3);  // local (partition) column
  const int y = ty * 16 + (wave >> 1) * 8 + (lane & 7);
  const bool active = (lc < P.part_cols) && (y < P.height);
  const f3 bmin = mk(P.bmin[0], P.bmin[1], P.bmin[2]);
  const f3 bsc = mk(P.bscale[0], P.bscale[1], P.bscale[2]);
  const float tstep = P.tstep, level = X.level;

  bool hit = false;
  float t = 0.f, tfar = 0.f;
  f3 pos = bmin, step = mk(0.f, 0.f, 0.f);  // (a lane without a ray samples the box corner, untested)
  if (active) {
    const int blk = lc / P.block_cols, within = lc - blk * P.block_cols;
    const int x = (P.part + blk * P.num_parts) * P.block_cols + within;
    f3 o, d;
    float tnear;
    hit = ray_setup(P, x, y, o, d, tnear, tfar);  // volumeRender_kernel.cu:388-425
    if constexpr (CLIP) hit = clip_interval(X.clip, o, d, hit, tnear, tfar);
    if (hit) {
      pos = mk(fmaf(d.x, tnear, o.x), fmaf(d.y, tnear, o.y), fmaf(d.z, tnear, o.z));
      step = mk(d.x * tstep, d.y * tstep, d.z * tstep);
      t = tnear;
    }
  }
  bool alive = hit;
  int32_t nsteps = 0, nfetch = 0;
  // the search's result: found -- sample k reached the level; first -- k == 0; (bpos, bt) -- the
  // position and t of sample k - 1 (of sample 0 when first); (qpos, qt) -- those of the lane's last
  // sample below the level so far
  bool found = false, first = false;
  f3 bpos = bmin, qpos = bmin;
  float bt = 0.f, qt = 0.f;

  // the emission texture's state, wave-uniform: 0 unbound (reads 0), 1 a single voxel, 2 a grid
  const int kind = P.em.p == nullptr ? 0 : (P.em.one ? 1 : 2);
  float one = 0.f;
  if (kind == 1) {
    const float q = P.em.p[0];
    one = fmaf(0.5f, q - q, q);  // == lerp(q, q, w) for every w (tex3d)
  }
  // the emission sample at world position p (in bounds for any p: axis() clamps every index)
  auto em_at = [&](const f3 &p) __attribute__((always_inline)) {
    if (kind != 2) return one;
    const f3 q = mk((p.x - bmin.x) * bsc.x, (p.y - bmin.y) * bsc.y, (p.z - bmin.z) * bsc.z);
    return fetch<BIG>(P.em, axis(q.x, P.em.nx, P.em.fnx), axis(q.y, P.em.ny, P.em.fny),
                      axis(q.z, P.em.nz, P.em.fnz));
  };

  // Empty-space probe, as project_kernel: ps > 0 -- the next probe's run length; -1 -- a probe found
  // data: re-armed by an all-zero batch after `rest` batches; 0 -- never probed.
  int ps = 0, rest = 0;
  KParams kp = nullptr;
  if constexpr (PROBE) {
    kp = (KParams)__builtin_amdgcn_kernarg_segment_ptr();
    const bool fin = fabsf(pos.x) < INFINITY && fabsf(pos.y) < INFINITY && fabsf(pos.z) < INFINITY &&
                     fabsf(step.x) < INFINITY && fabsf(step.y) < INFINITY && fabsf(step.z) < INFINITY &&
                     fabsf(t) < INFINITY;
    if (kind == 2 && tstep > 0.f && tstep < INFINITY && __all(!alive || fin)) ps = VR_ISO_PROBE_MIN;
  }

  while (__any(alive)) {
    if constexpr (PROBE) {
      if (ps > 0) {
        int e = probe_run(P, kp, alive, pos, step, t, tfar, ps, lane);
        // an occupied (or too large) box: runs half as long until one is empty or the shortest fails
        while (e <= 0 && ps > VR_ISO_PROBE_MIN) {
          ps >>= 1;
          e = probe_run(P, kp, alive, pos, step, t, tfar, ps, lane);
        }
        if (e > 0) {
          // the run's samples are +-0 < level: none hits.  The last of them is a live ray's k - 1.
          leap(P, ps - 1, alive, nsteps, t, tfar, pos, step);
          if (alive) {
            qpos = pos;
            qt = t;
          }
          leap(P, 1, alive, nsteps, t, tfar, pos, step);
          ps = min(2 * ps, (int)VR_PROBE_MAX);
          continue;
        }
        ps = -1;  // off until re-armed
        rest = VR_ISO_PROBE_REST;
      }
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
        if constexpr (decltype(grid)::value) {
          const f3 q = mk((pos.x - bmin.x) * bsc.x, (pos.y - bmin.y) * bsc.y, (pos.z - bmin.z) * bsc.z);
          v[j] = fetch<BIG>(P.em, axis(q.x, P.em.nx, P.em.fnx), axis(q.y, P.em.ny, P.em.fny),
                            axis(q.z, P.em.nz, P.em.fnz));
        } else {
          v[j] = one;  // (unbound: 0)
        }
        // the march recurrences of render_kernel: ++n, the cap, t += tstep, the exit test, pos += step
        const int32_t n1 = nsteps + 1;
        const float t1 = t + tstep;
        const bool go = alive && n1 < P.max_steps && !(t1 > tfar);
        nsteps = alive ? n1 : nsteps;
        t = alive ? t1 : t;
        pos = go ? mk(pos.x + step.x, pos.y + step.y, pos.z + step.z) : pos;
        alive = go;
      }
    };
    if (kind == 2) batch(std::true_type{});
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
    if constexpr (PROBE) {
      if (ps < 0) {
        if (rest > 0) --rest;
        else if (!__any(nz)) ps = VR_ISO_PROBE_MIN;  // back in empty space: probe again
      }
    }
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
      const float vc = em_at(mk(fmaf(step.x, c, bpos.x), fmaf(step.y, c, bpos.y), fmaf(step.z, c, bpos.z)));
      if (vc >= level) hi = c;
      else lo = c;
    }
    // hi = 1 gives pos_k and t_k bit for bit; k = 0: the first sample itself (the box face cuts the object)
    const f3 p = first ? bpos : mk(fmaf(step.x, hi, bpos.x), fmaf(step.y, hi, bpos.y), fmaf(step.z, hi, bpos.z));
    const float tsur = first ? bt : fmaf(tstep, hi, bt);
    const f3 s = mk((p.x - bmin.x) * bsc.x, (p.y - bmin.y) * bsc.y, (p.z - bmin.z) * bsc.z);
    const float vs = em_at(p);
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

  if (active) {
    // column-major planar output of this partition (render_kernel); depth and normal likewise
    const size_t plane = (size_t)P.plane_cols * (size_t)P.height;
    const size_t k = (size_t)lc * (size_t)P.height + (size_t)y;
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
    unsigned long long sv = (unsigned long long)nsteps, sf = (unsigned long long)nfetch;
    unsigned long long sn = found ? 1ull : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sv += __shfl_xor(sv, off, 64);
      sf += __shfl_xor(sf, off, 64);
      sn += __shfl_xor(sn, off, 64);
    }
    if (lane == 0 && sv) atomicAdd(P.steps, sv);
    if (lane == 0 && sf) atomicAdd(P.steps + 1, sf);
    if (lane == 0 && sn) atomicAdd(P.steps + 2, sn);
  }
}

// ------------------------------------------------------------------------------------------------
// launch helper (called from vr_capi.hip)

template <int GRAD, bool BIG, bool PROBE, bool CLIP>
static void launch_k(const RenderParams &P, const IsoArgs<CLIP> &X, dim3 grid, hipStream_t s) {
  if (P.steps) hipLaunchKernelGGL((isosurface_kernel<GRAD, BIG, PROBE, true, CLIP>), grid, dim3(256), 0, s, P, X);
  else hipLaunchKernelGGL((isosurface_kernel<GRAD, BIG, PROBE, false, CLIP>), grid, dim3(256), 0, s, P, X);
}

template <int GRAD, bool BIG, bool PROBE>
static void launch_c(const RenderParams &P, const IsoExtrasClip &X, dim3 grid, hipStream_t s) {
  if (X.clip.n > 0) launch_k<GRAD, BIG, PROBE, true>(P, X, grid, s);
  else launch_k<GRAD, BIG, PROBE, false>(P, static_cast<const IsoExtras &>(X), grid, s);
}

template <int GRAD>
static void launch_g(const RenderParams &P, const IsoExtrasClip &X, bool big, bool probe, dim3 grid, hipStream_t s) {
  if (big) probe ? launch_c<GRAD, true, true>(P, X, grid, s) : launch_c<GRAD, true, false>(P, X, grid, s);
  else probe ? launch_c<GRAD, false, true>(P, X, grid, s) : launch_c<GRAD, false, false>(P, X, grid, s);
}

// grad: 1 on-the-fly, 2 lookup; probe: leap empty space (needs P.occ and a level above 0); clip: the
// launch's plane set, or null / n == 0: the unclipped instantiations
hipError_t launch_isosurface(const RenderParams &P, int grad, float level, float *depth, float *normal, bool big,
                             bool probe, hipStream_t s, const ClipSet *clip) {
  if (P.part_cols <= 0 || P.height <= 0) return hipSuccess;
  if (grad != 1 && grad != 2) return hipErrorInvalidValue;
  const uint64_t ntx = (P.part_cols + 15) / 16, nty = (P.height + 15) / 16;
  const dim3 grid((unsigned)(ntx * nty));  // (tile_mode 0: row-major tiles)
  IsoExtrasClip X{};
  X.level = level;
  X.depth = depth;
  X.normal = normal;
  if (clip) X.clip = *clip;
  probe = probe && P.occ != nullptr && P.occ_bx != 0u && level > 0.f;
  if (grad == 1) launch_g<1>(P, X, big, probe, grid, s);
  else launch_g<2>(P, X, big, probe, grid, s);
  return hipGetLastError();
}

}  // namespace vr
