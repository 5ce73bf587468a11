// vr_transfer.hip -- gfx950 (MI355X, CDNA4) transfer-function render: 'render' with a colormap and
// an optional alphamap applied per sample, and the accumulated opacity as a plane (include/vrhip.h
// vr_render_transfer).
//
// transfer_kernel marches exactly the ray of render_kernel (vr_kernels.hip): ray_setup, tnear clamped
// to 0, t += tstep, pos += step, the max_steps cap, and render's three exit tests in their order.
// The sample is render_kernel<.., FAST = false>'s op sequence with the colour C_c = L(colormap) in
// place of color[c] in the emission term and, with an alphamap, A = L(alphamap, ab_s) in place of
// ab_s in the opacity (vr_transfer.h: the lookup shared with the host).  One lane per ray, no depth
// lanes, no volume staging: the compositing order is the contract.
//
// Tables: segment records {T[i], T[i+1] - T[i]} built by the host (vr_capi.hip do_transfer) -- per
// colour segment two 16-byte units {r, dr, g, dg}, {b, db, 0, 0}, then per alpha segment 8 bytes
// {A, dA}.  All 256 threads of a workgroup copy them to LDS (dynamic, sized from the tables: at most
// 1023 x 32 + 1023 x 8 bytes) before anything diverges; a colour lookup is then two ds_read_b128, an
// alpha lookup one ds_read_b64.  VR_TF_TABLE_GLOBAL=1 (an A/B build) reads the same records from
// global memory instead.
//
// Loads in flight: the positions of a ray do not depend on its opacity, so the wave takes
// VR_TF_BATCH consecutive samples' row loads first and composites them in sample order; a lane whose
// ray ends inside a batch (opacity above the threshold) does not fold the rest, so no bit depends on
// the batch length.  VR_TF_BATCH=1 is the plain loop.
//
// Empty-space leap (PROBE): probe_run / leap as the projection kernel.  The host launches it only
// where a leaped sample adds exactly 0: absorption aliases emission, Fa * A(+-0) * tstep == 0 (so
// alpha = 1 - exp(-0) = 0), Fe finite, and when lit the shading term proven finite (skip_empty).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include <type_traits>

#include "vr_clip.h"
#include "vr_device.h"
#include "vr_sampling.h"
#include "vr_stage.h"
#include "vr_transfer.h"

#ifndef VR_TF_BATCH
#define VR_TF_BATCH 2  // samples whose loads are issued before any is composited (measured: DESIGN.md s12)
#endif
#ifndef VR_TF_TABLE_GLOBAL
#define VR_TF_TABLE_GLOBAL 0  // 1: the table records read from global memory, no LDS copy (A/B build)
#endif
#ifndef VR_TF_PROBE_MIN
#define VR_TF_PROBE_MIN 64  // the probe's first run after the march enters empty space
#endif
#ifndef VR_TF_PROBE_REST
#define VR_TF_PROBE_REST 4  // batches marched after a failed probe before an all-zero batch re-arms it
#endif

namespace vr {

// The launch arguments that are not RenderParams (which must not grow, vr_device.h).
struct TransferExtras {
  const float4 *tab;     // the segment records: 2 (nc - 1) colour units, then the alpha records
  uint32_t n16;          // 16-byte units of `tab` (what a workgroup copies to LDS)
  int32_t nc, na;        // entries of the colormap and of the alphamap (na 0: no alphamap)
  float clo, cinv;       // colour coordinate range: lo and 1 / (hi - lo)
  float alo, ainv;       // the alphamap's
  int32_t coord;         // vr_transfer_coord
  int32_t ab_alias;      // the absorption texture is the emission texture (its sample is reused)
  float *alpha;          // the alpha plane, [plane_cols][H] as one plane of the image, or null
};
// The same for a clipped instantiation, with the plane set (vr_clip.h).  The unclipped kernels keep
// the arguments they had before there were planes.
struct TransferExtrasClip : TransferExtras {
  ClipSet clip;
};
template <bool CLIP>
using TransferArgs = std::conditional_t<CLIP, TransferExtrasClip, TransferExtras>;

extern __shared__ float4 tf_lds[];

// GRAD 0: no illumination term; 1: on-the-fly gradient (six taps of the gem binding); 2: lookup.
// COUNT: steps[0] += samples visited (leaped ones included), steps[1] += samples fetched.
// CLIP: the clip planes shorten [tnear, tfar] after ray_setup; the march and the leap start from there.
template <int GRAD, bool BIG, bool PROBE, bool COUNT, bool CLIP>
__global__ __launch_bounds__(256) void transfer_kernel(const RenderParams P, const TransferArgs<CLIP> X) {
  // tile and lane mapping of project_kernel / render_kernel
  int tx, ty;
  if (!tile_of_block(P, tx, ty)) return;  // whole workgroup: uniform
#if !VR_TF_TABLE_GLOBAL
  // every thread of the workgroup, whatever its ray: nothing diverges before the barrier
  for (uint32_t i = threadIdx.x; i < X.n16; i += 256u) tf_lds[i] = X.tab[i];
  __syncthreads();
  const float4 *const ctab = tf_lds;
  const float2 *const atab = reinterpret_cast<const float2 *>(tf_lds + 2 * (X.nc - 1));
#else
  const float4 *const ctab = X.tab;
  const float2 *const atab = reinterpret_cast<const float2 *>(X.tab + 2 * (X.nc - 1));
#endif
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int lc = tx * 16 + (wave & 1) * 8 + (lane >> 3);  // local (partition) column
  const int y = ty * 16 + (wave >> 1) * 8 + (lane & 7);
  const bool active = (lc < P.part_cols) && (y < P.height);
  const f3 bmin = mk(P.bmin[0], P.bmin[1], P.bmin[2]);
  const f3 bsc = mk(P.bscale[0], P.bscale[1], P.bscale[2]);
  const f3 eye = mk(P.eye[0], P.eye[1], P.eye[2]);
  const float tstep = P.tstep, thr = P.thr;

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
  float sr = 0.f, sg = 0.f, sb = 0.f, sa = 0.f;

  // the emission texture's state, wave-uniform: 0 unbound (reads 0), 1 a single voxel, 2 a grid
  const int kind = P.em.p == nullptr ? 0 : (P.em.one ? 1 : 2);
  float one = 0.f;
  if (kind == 1) {
    const float q = P.em.p[0];
    one = fmaf(0.5f, q - q, q);  // == lerp(q, q, w) for every w (tex3d)
  }

  // Empty-space probe, as project_kernel: ps > 0 -- the next probe's run length; -1 -- a probe found
  // data: re-armed by an all-zero batch after `rest` batches; 0 -- never probed.
  int ps = 0, rest = 0;
  KParams kp = nullptr;
  if constexpr (PROBE) {
    kp = (KParams)__builtin_amdgcn_kernarg_segment_ptr();
    const bool fin = fabsf(pos.x) < INFINITY && fabsf(pos.y) < INFINITY && fabsf(pos.z) < INFINITY &&
                     fabsf(step.x) < INFINITY && fabsf(step.y) < INFINITY && fabsf(step.z) < INFINITY &&
                     fabsf(t) < INFINITY;
    if (kind == 2 && tstep > 0.f && tstep < INFINITY && __all(!alive || fin)) ps = VR_TF_PROBE_MIN;
  }

  while (__any(alive)) {
    if constexpr (PROBE) {
      if (ps > 0) {
        int e = probe_run(P, kp, alive, pos, step, t, tfar, ps, lane);
        // an occupied (or too large) box: runs half as long until one is empty or the shortest fails
        while (e <= 0 && ps > VR_TF_PROBE_MIN) {
          ps >>= 1;
          e = probe_run(P, kp, alive, pos, step, t, tfar, ps, lane);
        }
        if (e > 0) {  // the run's samples add exactly 0 (the host's launch condition)
          leap(P, ps, alive, nsteps, t, tfar, pos, step);
          ps = min(2 * ps, (int)VR_PROBE_MAX);
          continue;
        }
        ps = -1;  // off until re-armed
        rest = VR_TF_PROBE_REST;
      }
    }
    // ---- a batch: positions and loads of VR_TF_BATCH consecutive samples, then the fold ---------
    float v[VR_TF_BATCH], vb[VR_TF_BATCH], tt[VR_TF_BATCH];
    f3 pp[VR_TF_BATCH];
    bool lv[VR_TF_BATCH];
    const int32_t n0 = nsteps;
    auto batch = [&](auto grid) __attribute__((always_inline)) {
#pragma unroll
      for (int j = 0; j < VR_TF_BATCH; ++j) {
        lv[j] = alive;
        tt[j] = t;
        pp[j] = pos;
        const f3 q = mk((pos.x - bmin.x) * bsc.x, (pos.y - bmin.y) * bsc.y, (pos.z - bmin.z) * bsc.z);
        if constexpr (decltype(grid)::value) {
          v[j] = fetch<BIG>(P.em, axis(q.x, P.em.nx, P.em.fnx), axis(q.y, P.em.ny, P.em.fny),
                            axis(q.z, P.em.nz, P.em.fnz));
        } else {
          v[j] = one;  // (unbound: 0)
        }
        vb[j] = X.ab_alias ? v[j] : tex3d<BIG>(P.ab, q.x, q.y, q.z);  // (wave-uniform branch)
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
    bool nz = false, done = false;
#pragma unroll
    for (int j = 0; j < VR_TF_BATCH; ++j) {
      if (lv[j] && !done) {  // (lv is monotone within a batch: samples 0 .. j of it were all taken)
        const float em_s = v[j], ab_s = vb[j];
        const f3 p = pp[j];
        if (COUNT) ++nfetch;
        if (PROBE) nz = nz || !(em_s == 0.f);
        // the classification
        float w;
        const int ci = vr_tf_segment(X.coord == 0 ? em_s : tt[j], X.clo, X.cinv, X.nc, &w);
        const float4 c0 = ctab[2 * ci], c1 = ctab[2 * ci + 1];
        const float cr = vr_tf_value(w, c0.x, c0.y), cg = vr_tf_value(w, c0.z, c0.w);
        const float cb = vr_tf_value(w, c1.x, c1.y);
        float A = ab_s;
        if (X.na != 0) {  // (wave-uniform)
          float wa;
          const int ai = vr_tf_segment(ab_s, X.alo, X.ainv, X.na, &wa);
          const float2 r = atab[ai];
          A = vr_tf_value(wa, r.x, r.y);
        }
        const float e = P.fe * em_s;
        const float a = P.fa * A;
        const float alpha = opacity<false>(a, tstep);
        const float eds = e * tstep;
        float ir = 0.f, ig = 0.f, ib = 0.f;
        if constexpr (GRAD != 0) {
          // render_kernel's skip: opacity exactly 0 and a finite emission term add exactly 0
          const bool skip = P.skip_empty && alpha == 0.f && fabsf(eds) <= 3.0e38f;
          if (!skip) {
            // the gradient render's exact shading takes (render_kernel without SHARE: the oracle's
            // expressions, as isosurface_kernel)
            const f3 s = mk((p.x - bmin.x) * bsc.x, (p.y - bmin.y) * bsc.y, (p.z - bmin.z) * bsc.z);
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
              g = mk(tex3d<BIG>(P.gx, s.x, s.y, s.z), tex3d<BIG>(P.gy, s.x, s.y, s.z),
                     tex3d<BIG>(P.gz, s.x, s.y, s.z));
            }
            const float refl = P.fr * (P.re_is_em ? em_s : tex3d<BIG>(P.re, s.x, s.y, s.z));
            shade_lights<false>(P, g, p, eye, refl, ir, ig, ib);
          }
        }
        const float r = fmaf(eds, cr, ir) * alpha;
        const float gg = fmaf(eds, cg, ig) * alpha;
        const float b = fmaf(eds, cb, ib) * alpha;
        const float om = 1.f - sa;
        sr = fmaf(om, r, sr);
        sg = fmaf(om, gg, sg);
        sb = fmaf(om, b, sb);
        sa = fmaf(om, alpha, sa);
        if (sa > thr) {  // render's first exit test: the ray stops at this sample
          done = true;
          nsteps = n0 + j + 1;
        }
      }
    }
    alive = alive && !done;
    if constexpr (PROBE) {
      if (ps < 0) {
        if (rest > 0) --rest;
        else if (!__any(nz)) ps = VR_TF_PROBE_MIN;  // back in empty space: probe again
      }
    }
  }

  if (active) {
    // column-major planar output of this partition (render_kernel); the alpha plane likewise.
    // A miss writes the initial zeros.
    const size_t plane = (size_t)P.plane_cols * (size_t)P.height;
    const size_t k = (size_t)lc * (size_t)P.height + (size_t)y;
    P.out[k] = sr;
    P.out[k + plane] = sg;
    P.out[k + 2 * plane] = sb;
    if (X.alpha != nullptr) X.alpha[k] = sa;
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

template <int GRAD, bool BIG, bool PROBE, bool CLIP>
static void launch_k(const RenderParams &P, const TransferArgs<CLIP> &X, dim3 grid, size_t lds, hipStream_t s) {
  if (P.steps) hipLaunchKernelGGL((transfer_kernel<GRAD, BIG, PROBE, true, CLIP>), grid, dim3(256), lds, s, P, X);
  else hipLaunchKernelGGL((transfer_kernel<GRAD, BIG, PROBE, false, CLIP>), grid, dim3(256), lds, s, P, X);
}

template <int GRAD, bool BIG, bool PROBE>
static void launch_c(const RenderParams &P, const TransferExtrasClip &X, dim3 grid, size_t lds, hipStream_t s) {
  if (X.clip.n > 0) launch_k<GRAD, BIG, PROBE, true>(P, X, grid, lds, s);
  else launch_k<GRAD, BIG, PROBE, false>(P, static_cast<const TransferExtras &>(X), grid, lds, s);
}

template <int GRAD>
static void launch_g(const RenderParams &P, const TransferExtrasClip &X, bool big, bool probe, dim3 grid, size_t lds,
                     hipStream_t s) {
  if (big) probe ? launch_c<GRAD, true, true>(P, X, grid, lds, s) : launch_c<GRAD, true, false>(P, X, grid, lds, s);
  else probe ? launch_c<GRAD, false, true>(P, X, grid, lds, s) : launch_c<GRAD, false, false>(P, X, grid, lds, s);
}

// 16-byte units of the record buffer of an nc-entry colormap and an na-entry alphamap (na 0: none)
uint32_t transfer_table_units(int32_t nc, int32_t na) {
  return 2u * (uint32_t)(nc - 1) + (na > 0 ? ((uint32_t)(na - 1) + 1u) / 2u : 0u);
}

// grad: 0 unlit, 1 on-the-fly, 2 lookup; probe: leap empty space (needs P.occ; the host has checked
// that a leaped sample adds exactly 0); clip: the launch's plane set, or null / n == 0: the unclipped
// instantiations
hipError_t launch_transfer(const RenderParams &P, int grad, const float *tab, int32_t nc, int32_t na, float clo,
                           float cinv, float alo, float ainv, int32_t coord, bool ab_alias, float *alpha, bool big,
                           bool probe, hipStream_t s, const ClipSet *clip) {
  if (P.part_cols <= 0 || P.height <= 0) return hipSuccess;
  if (grad < 0 || grad > 2 || nc < 2 || nc > 1024 || na == 1 || na < 0 || na > 1024 || !tab)
    return hipErrorInvalidValue;
  const uint64_t ntx = (P.part_cols + 15) / 16, nty = (P.height + 15) / 16;
  const dim3 grid((unsigned)(ntx * nty));  // (tile_mode 0: row-major tiles)
  TransferExtrasClip X{};
  if (clip) X.clip = *clip;
  X.tab = reinterpret_cast<const float4 *>(tab);
  X.n16 = transfer_table_units(nc, na);
  X.nc = nc;
  X.na = na;
  X.clo = clo;
  X.cinv = cinv;
  X.alo = alo;
  X.ainv = ainv;
  X.coord = coord;
  X.ab_alias = ab_alias ? 1 : 0;
  X.alpha = alpha;
  const size_t lds = VR_TF_TABLE_GLOBAL ? 0 : (size_t)X.n16 * 16;
  probe = probe && P.occ != nullptr && P.occ_bx != 0u;
  if (grad == 0) launch_g<0>(P, X, big, probe, grid, lds, s);
  else if (grad == 1) launch_g<1>(P, X, big, probe, grid, lds, s);
  else launch_g<2>(P, X, big, probe, grid, lds, s);
  return hipGetLastError();
}

}  // namespace vr
