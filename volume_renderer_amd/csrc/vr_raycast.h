// vr_raycast.h -- what the one-lane-per-ray feature kernels share (project_kernel, isosurface_kernel):
// the pixel of a thread, the start of its ray, the emission sample, the march recurrence, the
// empty-space probe's state machine, the step counters and the launch dispatch.  A kernel supplies
// what is its own: the action on an empty run, the fold of a batch and the stores.
// transfer_kernel (vr_transfer.hip) still carries its own copy of these pieces: built from this header
// its lit launches measured about 0.5 % slower (profiles/round18).  render_kernel (vr_kernels.hip) and
// the LDS-staged march (vr_march.hip) have loops of another shape and do not use this header.
#ifndef VR_RAYCAST_H
#define VR_RAYCAST_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <type_traits>

#include "vr_clip.h"
#include "vr_device.h"
#include "vr_sampling.h"
#include "vr_stage.h"

namespace vr {

// ---- launch arguments ------------------------------------------------------------------------------
// A kernel's launch arguments that are not RenderParams (which must not grow: RenderViews passes four of
// them by value, vr_device.h) are its Extras struct.  A clipped instantiation takes them with the plane
// set (vr_clip.h) behind; the unclipped kernels keep the arguments they had before there were planes.
template <class Extras>
struct WithClip : Extras {
  ClipSet clip;
};
template <class Extras, bool CLIP>
using Args = std::conditional_t<CLIP, WithClip<Extras>, Extras>;

// ---- pixel mapping ---------------------------------------------------------------------------------
// 16x16 pixel workgroup tile; wave w owns the 8x8 quadrant (w & 1, w >> 1); lane -> (x, y) with y
// fastest so that the column-major output stores of a lane octet are contiguous (render_kernel).
struct Pixel {
  int lane;
  int lc, y;    // local (partition) column and row
  bool active;  // inside the partition's image
  // column-major planar output of this partition (render_kernel): floats per plane, and this pixel's index
  __device__ __forceinline__ size_t plane(const RenderParams &P) const { return (size_t)P.plane_cols * (size_t)P.height; }
  __device__ __forceinline__ size_t k(const RenderParams &P) const { return (size_t)lc * (size_t)P.height + (size_t)y; }
};
// the thread's pixel in the workgroup's tile (tx, ty) of tile_of_block (vr_sampling.h)
__device__ __forceinline__ Pixel pixel_of_tile(const RenderParams &P, int tx, int ty) {
  Pixel px;
  const int wave = threadIdx.x >> 6;
  px.lane = threadIdx.x & 63;
  px.lc = tx * 16 + (wave & 1) * 8 + (px.lane >> 3);
  px.y = ty * 16 + (wave >> 1) * 8 + (px.lane & 7);
  px.active = (px.lc < P.part_cols) && (px.y < P.height);
  return px;
}

// ---- ray start -------------------------------------------------------------------------------------
// The ray of render_kernel: image column from the partition, ray_setup (tnear clamped to 0), with CLIP
// the planes of the launch arguments (Args<Extras, true>) shorten [tnear, tfar]; then the first
// position, the step and t.  A lane without a ray (inactive or a miss) keeps pos = bmin, step = 0,
// t = tfar = 0: it samples the box corner, unfolded.
struct RayStart {
  bool hit;
  float t, tfar;
  f3 pos, step;
};
template <bool CLIP, class X>
__device__ __forceinline__ RayStart ray_start(const RenderParams &P, const X &args, bool active, int lc, int y,
                                              const f3 &bmin, float tstep) {
  RayStart r;
  r.hit = false;
  r.t = 0.f;
  r.tfar = 0.f;
  r.pos = bmin;
  r.step = mk(0.f, 0.f, 0.f);
  if (active) {
    const int blk = lc / P.block_cols, within = lc - blk * P.block_cols;
    const int x = (P.part + blk * P.num_parts) * P.block_cols + within;
    f3 o, d;
    float tnear;
    r.hit = ray_setup(P, x, y, o, d, tnear, r.tfar);  // volumeRender_kernel.cu:388-425
    if constexpr (CLIP) r.hit = clip_interval(args.clip, o, d, r.hit, tnear, r.tfar);
    if (r.hit) {
      r.pos = mk(fmaf(d.x, tnear, o.x), fmaf(d.y, tnear, o.y), fmaf(d.z, tnear, o.z));
      r.step = mk(d.x * tstep, d.y * tstep, d.z * tstep);
      r.t = tnear;
    }
  }
  return r;
}

// ---- emission sampler ------------------------------------------------------------------------------
// The emission texture's state, wave-uniform: kind 0 unbound (reads 0), 1 a single voxel (reads `one`),
// 2 a grid.
struct Emission {
  int kind;
  float one;
};
__device__ __forceinline__ Emission emission_of(const RenderParams &P) {
  Emission e;
  e.kind = P.em.p == nullptr ? 0 : (P.em.one ? 1 : 2);
  e.one = 0.f;
  if (e.kind == 1) {
    const float q = P.em.p[0];
    e.one = fmaf(0.5f, q - q, q);  // == lerp(q, q, w) for every w (tex3d)
  }
  return e;
}
// world position -> normalized texture coordinate
__device__ __forceinline__ f3 tex_coord(const f3 &bmin, const f3 &bsc, const f3 &p) {
  return mk((p.x - bmin.x) * bsc.x, (p.y - bmin.y) * bsc.y, (p.z - bmin.z) * bsc.z);
}
// The emission sample at world position p (in bounds for any p: axis() clamps every index into the
// padded volume).  Inside a batch the kind is decided outside, as std::true_type (a grid) or
// std::false_type: a branch per sample would split the batch into basic blocks and the loads would not
// be issued together.  With the runtime kind: for single samples.
template <bool BIG>
__device__ __forceinline__ float em_at(const RenderParams &P, std::true_type, float, const f3 &bmin, const f3 &bsc,
                                       const f3 &p) {
  const f3 q = tex_coord(bmin, bsc, p);
  return fetch<BIG>(P.em, axis(q.x, P.em.nx, P.em.fnx), axis(q.y, P.em.ny, P.em.fny), axis(q.z, P.em.nz, P.em.fnz));
}
template <bool BIG>
__device__ __forceinline__ float em_at(const RenderParams &, std::false_type, float one, const f3 &, const f3 &,
                                       const f3 &) {
  return one;  // (unbound: 0)
}
template <bool BIG>
__device__ __forceinline__ float em_at(const RenderParams &P, int kind, float one, const f3 &bmin, const f3 &bsc,
                                       const f3 &p) {
  if (kind != 2) return one;
  return em_at<BIG>(P, std::true_type{}, one, bmin, bsc, p);
}

// ---- per-sample recurrence -------------------------------------------------------------------------
// The march recurrences of render_kernel after a sample: ++n, the cap, t += tstep, the exit test,
// pos += step.  A lane whose ray ended keeps its last position (its loads stay in bounds).
__device__ __forceinline__ void next_sample(const RenderParams &P, float tstep, float tfar, const f3 &step, bool &alive,
                                            int32_t &nsteps, float &t, f3 &pos) {
  const int32_t n1 = nsteps + 1;
  const float t1 = t + tstep;
  const bool go = alive && n1 < P.max_steps && !(t1 > tfar);
  nsteps = alive ? n1 : nsteps;
  t = alive ? t1 : t;
  pos = go ? mk(pos.x + step.x, pos.y + step.y, pos.z + step.z) : pos;
  alive = go;
}

// ---- empty-space probe -----------------------------------------------------------------------------
// As the march's probe (vr_stage.h probe_run): when every centre tap of the live rays' next ps samples
// lies in all-zero bricks of the emission texture's occupancy map, each of those samples is +-0 and only
// the recurrences are replayed (leap).  What an empty run means for the kernel's result is the kernel's
// own reasoning, and its action.
// ps > 0 -- the next probe's run length (doubled after each empty run, up to VR_PROBE_MAX);
// -1 -- a probe found data: re-armed by an all-zero batch after `rest` batches; 0 -- never probed.
struct Probe {
  int ps = 0, rest = 0;
  KParams kp = nullptr;
};
// probe_run forms its box from fma(step, k, pos) and (tfar - t) / tstep: finite rays and a positive
// finite step only (the margin probe_off bounds the drift of such rays); a grid texture only.
template <int MIN>
__device__ __forceinline__ Probe probe_arm(int kind, float tstep, bool alive, const f3 &pos, const f3 &step, float t) {
  Probe pr;
  pr.kp = (KParams)__builtin_amdgcn_kernarg_segment_ptr();
  const bool fin = fabsf(pos.x) < INFINITY && fabsf(pos.y) < INFINITY && fabsf(pos.z) < INFINITY &&
                   fabsf(step.x) < INFINITY && fabsf(step.y) < INFINITY && fabsf(step.z) < INFINITY &&
                   fabsf(t) < INFINITY;
  if (kind == 2 && tstep > 0.f && tstep < INFINITY && __all(!alive || fin)) pr.ps = MIN;
  return pr;
}
// The top of the sample loop.  true: the run of pr.ps samples was empty, on_empty(ps) has taken it (the
// kernel's action and its leap) and the loop continues with the next probe; false: march a batch.
template <int MIN, int REST, class F>
__device__ __forceinline__ bool probe_step(const RenderParams &P, Probe &pr, bool alive, const f3 &pos, const f3 &step,
                                           float t, float tfar, int lane, F &&on_empty) {
  if (pr.ps <= 0) return false;
  int e = probe_run(P, pr.kp, alive, pos, step, t, tfar, pr.ps, lane);
  // an occupied (or too large) box: runs half as long until one is empty or the shortest fails
  while (e <= 0 && pr.ps > MIN) {
    pr.ps >>= 1;
    e = probe_run(P, pr.kp, alive, pos, step, t, tfar, pr.ps, lane);
  }
  if (e > 0) {
    on_empty(pr.ps);
    pr.ps = min(2 * pr.ps, (int)VR_PROBE_MAX);
    return true;
  }
  pr.ps = -1;  // off until re-armed
  pr.rest = REST;
  return false;
}
// After a batch; nz: this lane folded a sample that was not +-0.
template <int MIN>
__device__ __forceinline__ void probe_rearm(Probe &pr, bool nz) {
  if (pr.ps < 0) {
    if (pr.rest > 0) --pr.rest;
    else if (!__any(nz)) pr.ps = MIN;  // back in empty space: probe again
  }
}

// ---- counters --------------------------------------------------------------------------------------
// steps[i] += the wave's sum of c[i] (COUNT instantiations: diagnostics)
template <int N>
__device__ __forceinline__ void add_steps(unsigned long long *steps, int lane, unsigned long long (&c)[N]) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int i = 0; i < N; ++i) c[i] += __shfl_xor(c[i], off, 64);
  }
#pragma unroll
  for (int i = 0; i < N; ++i)
    if (lane == 0 && c[i]) atomicAdd(steps + i, c[i]);
}

// ---- launch dispatch -------------------------------------------------------------------------------
// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...) for runtime b0, b1, ...: the host's flags
// as template arguments of the kernel f launches.
template <class F>
void with_bools(F &&f) {
  f();
}
template <class F, class... Rest>
void with_bools(F &&f, bool b, Rest... rest) {
  if (b) with_bools([&](auto... c) { f(std::true_type{}, c...); }, rest...);
  else with_bools([&](auto... c) { f(std::false_type{}, c...); }, rest...);
}
// one workgroup per 16x16 tile of the partition (tile_mode 0: row-major tiles)
inline dim3 tile_grid(const RenderParams &P) {
  const uint64_t ntx = (P.part_cols + 15) / 16, nty = (P.height + 15) / 16;
  return dim3((unsigned)(ntx * nty));
}

}  // namespace vr

#endif
