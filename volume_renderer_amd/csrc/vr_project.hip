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

#include "vr_clip.h"
#include "vr_device.h"
#include "vr_sampling.h"
#include "vr_stage.h"

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

// The launch arguments that are not RenderParams (which must not grow: RenderViews passes four of
// them by value, vr_device.h): the aux plane -- [plane_cols][H] as one plane of the image, or null.
struct ProjectExtras {
  float *aux;
};
// The same for a clipped instantiation, with the plane set (vr_clip.h).  The unclipped kernels keep
// the arguments they had before there were planes.
struct ProjectExtrasClip : ProjectExtras {
  ClipSet clip;
};
template <bool CLIP>
using ProjectArgs = std::conditional_t<CLIP, ProjectExtrasClip, ProjectExtras>;

// MODE 0: maximum-intensity projection (aux: t of the first maximum), 1: ray sum (aux: samples).
// COUNT: steps[0] += samples visited (leaped ones included), steps[1] += samples fetched.
// CLIP: the clip planes shorten [tnear, tfar] after ray_setup; the march and the leap start from there.
template <int MODE, bool BIG, bool PROBE, bool COUNT, bool CLIP>
__global__ __launch_bounds__(256) void project_kernel(const RenderParams P, const ProjectArgs<CLIP> X) {
  // 16x16 pixel workgroup tile; wave w owns the 8x8 quadrant (w & 1, w >> 1); lane -> (x, y) with y
  // fastest so that the column-major output stores of a lane octet are contiguous (render_kernel).
  int tx, ty;
  if (!tile_of_block(P, tx, ty)) return;  // whole workgroup: uniform
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = tx * 16 + (wave & 1) * 8 + (lane >> 3);  // local (partition) column
  const int y = ty * 16 + (wave >> 1) * 8 + (lane & 7);
  const bool active = (lc < P.part_cols) && (y < P.height);
  const f3 bmin = mk(P.bmin[0], P.bmin[1], P.bmin[2]);
  const f3 bsc = mk(P.bscale[0], P.bscale[1], P.bscale[2]);
  const float tstep = P.tstep;

  bool hit = false;
  float t = 0.f, tfar = 0.f;
  f3 pos = bmin, step = mk(0.f, 0.f, 0.f);  // (a lane without a ray samples the box corner, unfolded)
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
  float m = -INFINITY, tm = 0.f;  // MODE 0: the maximum and the t of its first occurrence
  float s = 0.f;                  // MODE 1

  // the emission texture's state, wave-uniform: 0 unbound (reads 0), 1 a single voxel, 2 a grid
  const int kind = P.em.p == nullptr ? 0 : (P.em.one ? 1 : 2);
  float one = 0.f;
  if (kind == 1) {
    const float q = P.em.p[0];
    one = fmaf(0.5f, q - q, q);  // == lerp(q, q, w) for every w (tex3d)
  }

  // Empty-space probe: ps > 0 -- the next probe's run length (doubled after each empty run, up to
  // VR_PROBE_MAX); -1 -- a probe found data: re-armed by an all-zero batch after `rest` batches;
  // 0 -- never probed.
  // probe_run forms its box from fma(step, k, pos) and (tfar - t) / tstep: finite rays and a positive
  // finite step only (the margin probe_off bounds the drift of such rays).
  int ps = 0, rest = 0;
  KParams kp = nullptr;
  if constexpr (PROBE) {
    kp = (KParams)__builtin_amdgcn_kernarg_segment_ptr();
    const bool fin = fabsf(pos.x) < INFINITY && fabsf(pos.y) < INFINITY && fabsf(pos.z) < INFINITY &&
                     fabsf(step.x) < INFINITY && fabsf(step.y) < INFINITY && fabsf(step.z) < INFINITY &&
                     fabsf(t) < INFINITY;
    if (kind == 2 && tstep > 0.f && tstep < INFINITY && __all(!alive || fin)) ps = VR_PROJ_PROBE_MIN;
  }

  while (__any(alive)) {
    if constexpr (PROBE) {
      if (ps > 0) {
        int e = probe_run(P, kp, alive, pos, step, t, tfar, ps, lane);
        // an occupied (or too large) box: runs half as long until one is empty or the shortest fails
        while (e <= 0 && ps > VR_PROJ_PROBE_MIN) {
          ps >>= 1;
          e = probe_run(P, kp, alive, pos, step, t, tfar, ps, lane);
        }
        if (e > 0) {
          if (MODE == 0 && alive && 0.f > m) {  // the run's samples are +-0: the first one wins
            m = 0.f;
            tm = t;
          }
          leap(P, ps, alive, nsteps, t, tfar, pos, step);
          ps = min(2 * ps, (int)VR_PROBE_MAX);
          continue;
        }
        ps = -1;  // off until re-armed
        rest = VR_PROJ_PROBE_REST;
      }
    }
    // ---- a batch: positions and loads of VR_PROJ_BATCH consecutive samples, then the fold ------
    // (the texture's kind is decided outside the batch: a branch per sample would split the batch
    // into basic blocks and the loads would not be issued together)
    float v[VR_PROJ_BATCH], tt[VR_PROJ_BATCH];
    bool lv[VR_PROJ_BATCH];
    auto batch = [&](auto grid) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < VR_PROJ_BATCH; ++j) {
        lv[j] = alive;
        tt[j] = t;
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
    if constexpr (PROBE) {
      if (ps < 0) {
        if (rest > 0) --rest;
        else if (!__any(nz)) ps = VR_PROJ_PROBE_MIN;  // back in empty space: probe again
      }
    }
  }

  if (active) {
    // column-major planar output of this partition (render_kernel); the aux plane likewise
    const size_t plane = (size_t)P.plane_cols * (size_t)P.height;
    const size_t k = (size_t)lc * (size_t)P.height + (size_t)y;
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
    unsigned long long sv = (unsigned long long)nsteps, sf = (unsigned long long)nfetch;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sv += __shfl_xor(sv, off, 64);
      sf += __shfl_xor(sf, off, 64);
    }
    if (lane == 0 && sv) atomicAdd(P.steps, sv);
    if (lane == 0 && sf) atomicAdd(P.steps + 1, sf);
  }
}

// ------------------------------------------------------------------------------------------------
// launch helper (called from vr_capi.hip)

template <int MODE, bool BIG, bool PROBE, bool CLIP>
static void launch_k(const RenderParams &P, const ProjectArgs<CLIP> &X, dim3 grid, hipStream_t s) {
  if (P.steps) hipLaunchKernelGGL((project_kernel<MODE, BIG, PROBE, true, CLIP>), grid, dim3(256), 0, s, P, X);
  else hipLaunchKernelGGL((project_kernel<MODE, BIG, PROBE, false, CLIP>), grid, dim3(256), 0, s, P, X);
}

template <int MODE, bool BIG, bool PROBE>
static void launch_c(const RenderParams &P, const ProjectExtrasClip &X, dim3 grid, hipStream_t s) {
  if (X.clip.n > 0) launch_k<MODE, BIG, PROBE, true>(P, X, grid, s);
  else launch_k<MODE, BIG, PROBE, false>(P, static_cast<const ProjectExtras &>(X), grid, s);
}

template <int MODE>
static void launch_m(const RenderParams &P, const ProjectExtrasClip &X, bool big, bool probe, dim3 grid, hipStream_t s) {
  if (big) probe ? launch_c<MODE, true, true>(P, X, grid, s) : launch_c<MODE, true, false>(P, X, grid, s);
  else probe ? launch_c<MODE, false, true>(P, X, grid, s) : launch_c<MODE, false, false>(P, X, grid, s);
}

// mode: vr_projection (0 maximum, 1 sum); probe: leap empty space (needs P.occ); clip: the launch's
// plane set, or null / n == 0: the unclipped instantiations
hipError_t launch_project(const RenderParams &P, int mode, float *aux, bool big, bool probe, hipStream_t s,
                          const ClipSet *clip) {
  if (P.part_cols <= 0 || P.height <= 0) return hipSuccess;
  if (mode != 0 && mode != 1) return hipErrorInvalidValue;
  const uint64_t ntx = (P.part_cols + 15) / 16, nty = (P.height + 15) / 16;
  const dim3 grid((unsigned)(ntx * nty));  // (tile_mode 0: row-major tiles)
  ProjectExtrasClip X{};
  X.aux = aux;
  if (clip) X.clip = *clip;
  probe = probe && P.occ != nullptr && P.occ_bx != 0u;
  if (mode == 0) launch_m<0>(P, X, big, probe, grid, s);
  else launch_m<1>(P, X, big, probe, grid, s);
  return hipGetLastError();
}

}  // namespace vr
