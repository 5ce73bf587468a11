// vr_frame.hip -- from the render arguments to a launchable frame (vr_host.h): the clip planes'
// conversion, initRender and the per-frame constants (build_frame; the reference's vr/
// volumeRender.cpp:112-156), lights, the column partition, the depth lanes and the march object that
// serves them (march_entries), the launch schedules and their predictor.
#include "vr_host.h"

namespace vr_host {

vr::DevTex dev_tex(const BufPtr &b) {
  vr::DevTex t{};
  if (b && b->ptr) {
    t.p = b->ptr;
    t.nx = (int32_t)b->dims[0];
    t.ny = (int32_t)b->dims[1];
    t.nz = (int32_t)b->dims[2];
    t.px = (uint32_t)(b->dims[0] + 2);
    t.pxy = (uint32_t)((b->dims[0] + 2) * (b->dims[1] + 2));
    t.fnx = (float)t.nx;
    t.fny = (float)t.ny;
    t.fnz = (float)t.nz;
    t.one = (t.nx == 1 && t.ny == 1 && t.nz == 1);
    const uint64_t padded = (b->dims[0] + 2) * (b->dims[1] + 2) * (b->dims[2] + 2);
    t.small = padded < (1ull << 22) && !test_flag("VR_NO_SMALL_LUT");
    t.fpx4 = 4.f * (float)t.px;
    t.fpxy4 = 4.f * (float)t.pxy;
    t.fbase4 = 4.f * (float)(t.pxy + t.px + 1);
    t.zp = t.small ? b->zpair : nullptr;
  }
  return t;
}

bool is_big(const vr::DevTex &t) {
  return t.p && ((uint64_t)t.nx + 2) * ((uint64_t)t.ny + 2) * ((uint64_t)t.nz + 2) > 0xFFFFFFFFull;
}

static bool same_tex(const vr::DevTex &a, const vr::DevTex &b) {
  return a.p == b.p && a.nx == b.nx && a.ny == b.ny && a.nz == b.nz;
}
static bool same_dims(const vr::DevTex &a, const vr::DevTex &b) {
  return a.nx == b.nx && a.ny == b.ny && a.nz == b.nz;
}

// finite and comfortably below FLT_MAX (a texture that is unbound reads 0)
static bool tame(const BufPtr &b) { return !b || !b->ptr || (!b->nonfinite && b->maxabs < 1e30f); }

// Whether the fast variant may derive the on-the-fly gradient taps from the centre's axes
// (vr_sampling.h half_taps): a cube of power-of-two edge n with isotropic element
// size, i.e. on every axis box [-1, 1] (bscale 1/2), gstep = 1/n exact and a tap offset of exactly
// half a texel.  Then the reference's tap coordinate ((pos + 2^-k) + 1) * 1/2 * n - 1/2 equals the
// centre's xb +- 1/2 exactly -- adding 2^-k (a multiple of the ulp of pos + 1 in [1, 2)) commutes with
// the rounding of pos + 1 -- except for samples within half a texel of a plane where pos, pos +- 2^-k
// or pos + 1 changes binade (pos = 0, +-2^-j), where the two can differ by an ulp of pos before the
// 8-bit weight quantization (measured: tests/test_gpu_parity.py::test_half_texel_taps).
// VR_EXACT_TAPS=1 turns it off.
int32_t half_texel_taps(const vr::RenderParams &P, int mode, float fnz) {
  if (mode != 1 || test_flag("VR_EXACT_TAPS")) return 0;
  const float n[3] = {P.em.fnx, P.em.fny, fnz};
  for (int i = 0; i < 3; ++i) {
    int e = 0;
    if (!(n[i] >= 2.f) || std::frexp(n[i], &e) != 0.5f) return 0;  // power of two
    if (P.gstep[i] != 1.f / n[i] || P.bscale[i] != 0.5f || P.bmin[i] != -1.f) return 0;
  }
  return 1;
}

// The argument checks of vr_set_clip (include/vrhip.h): before the handle, no device needed.
int check_clip(const vr_clip_plane *planes, int32_t n) {
  if (n < 0 || n > VR_CLIP_MAX) return fail(VR_ERR_ARGUMENT, "clip planes: 0 .. " + std::to_string(VR_CLIP_MAX) + " planes");
  if (n > 0 && !planes) return fail(VR_ERR_ARGUMENT, "clip planes: planes is NULL");
  for (int32_t i = 0; i < n; ++i) {
    const vr_clip_plane &p = planes[i];
    if (!std::isfinite(p.normal[0]) || !std::isfinite(p.normal[1]) || !std::isfinite(p.normal[2]) ||
        !std::isfinite(p.offset))
      return fail(VR_ERR_ARGUMENT, "clip planes: non-finite plane");
    if (p.normal[0] == 0.f && p.normal[1] == 0.f && p.normal[2] == 0.f)
      return fail(VR_ERR_ARGUMENT, "clip planes: all-zero normal");
  }
  return VR_OK;
}

// The host conversion of the header: the plane normal . q + offset >= 0 of q = (p - bmin) * bscale as
// N . p + D >= 0 of the world position p, in fp32 (-ffp-contract=off: every operation rounded once).
void convert_clip(const vr_clip_plane &p, const float bmin[3], const float bscale[3], float out[4]) {
  for (int k = 0; k < 3; ++k) out[k] = p.normal[k] * bscale[k];
  out[3] = fmaf(-out[2], bmin[2], fmaf(-out[1], bmin[1], fmaf(-out[0], bmin[0], p.offset)));
}

// The plane set of a launch of frame P on handle h (n == 0: none, the unclipped kernels).
vr::ClipSet clip_set(const vr_context *h, const vr::RenderParams &P) {
  vr::ClipSet C{};
  C.n = h->nclip;
  for (int32_t i = 0; i < h->nclip; ++i) convert_clip(h->clip[i], P.bmin, P.bscale, C.pl[i]);
  return C;
}

int clip_unsupported(const char *what) {
  return fail(VR_ERR_UNSUPPORTED, std::string(what) + ": clip planes are set on the handle (vr_set_clip); they are "
                                                      "honoured by the single-handle render calls only");
}

// Per-sample bound of the drift between a predicted position fma(step, k, pos) and k sequentially
// rounded additions, in emission texels per axis: |pos| <= |box| + |eye| (fp32 rounding 1.2e-7 per
// operation, two per step).  eye2: the second eye of a fused stereo launch, whose rays start
// elsewhere (the bound must cover both eyes).
void drift_bound(Frame &F, const float *eye2) {
  const vr::RenderParams &P = F.P;
  double pmax = 0.0;
  for (int i = 0; i < 3; ++i) {
    double e = std::fabs(P.eye[i]);
    if (eye2) e = std::max(e, (double)std::fabs(eye2[i]));
    pmax = std::max(pmax, (double)std::fabs(P.bmin[i]) + e);
  }
  for (int i = 0; i < 3; ++i) {
    const float n = i == 0 ? P.em.fnx : (i == 1 ? P.em.fny : P.em.fnz);
    F.drift1[i] = 2.0 * pmax * 1.2e-7 * (double)P.bscale[i] * (double)n;
    // the empty-space probe's box: the centre taps (the cell of floor(c n - 1/2)) with the staging
    // margin of 1/16 texel, plus the drift of up to VR_PROBE_MAX sequential additions.  Set here, with
    // the drift, so that every launch path gets it -- the fused multi-view march included (ADVICE r5:
    // it copied F.P before set_chunk_halo and probed with a zero margin)
    F.P.probe_off[i] = (float)(0.0625 + (double)VR_PROBE_MAX * F.drift1[i]);
  }
}

int build_frame(vr_context *h, const vr_render_args *a, Frame &F, uint64_t depth_override) {
  vr::RenderParams &P = F.P;
  std::memset(&P, 0, sizeof(P));
  const uint64_t H = a->resolution[0], W = a->resolution[1];
  if (W > 0x7FFFFFFF || H > 0x7FFFFFFF || W * H > (1ull << 40))
    return fail(VR_ERR_UNSUPPORTED, "image resolution too large");
  P.width = (int32_t)W;
  P.height = (int32_t)H;
  P.fw = (float)W;
  P.fh = (float)H;
  P.ratio = (float)H / (float)W;
  // factors = [Fe Fr Fa] -> initRender(..., Fe, Fr, Fa, ...)
  P.fe = a->factors[0];
  P.fr = a->factors[1];
  P.fa = a->factors[2];
  // element size reversed (make_float3Inv, render.cpp:35-37,195)
  const float es[3] = {a->element_size_um[2], a->element_size_um[1], a->element_size_um[0]};
  const VolRec &ev = h->vol[T_EM];  // extent of the handle's emission volume (render.cpp:245)
  const uint64_t vw = ev.dims[0], vh = ev.dims[1], vd = depth_override ? depth_override : ev.dims[2];
  float bmax[3];
  bmax[0] = 1.f;
  bmax[1] = (es[1] * (float)vh) / ((float)vw * es[0]);
  bmax[2] = (es[2] * (float)vd) / ((float)vw * es[0]);
  for (int i = 0; i < 3; ++i) P.bmin[i] = -1.f * bmax[i];
  const float dxy = sqrtf((float)(vw * vw + vh * vh));
  const float dyz = sqrtf((float)(vh * vh + vd * vd));
  const float dxz = sqrtf((float)(vw * vw + vd * vd));
  const float mind = fminf(dxy, fminf(dyz, dxz));
  P.tstep = 1.f / (2.2f * mind);
  P.thr = a->opacity_threshold;
  for (int i = 0; i < 3; ++i) {
    P.bscale[i] = 1.f / (bmax[i] - P.bmin[i]);
    P.color[i] = a->color[i];
  }
  P.gstep[0] = 1.f / (float)vw;  // volumeRender.cpp:273-275
  P.gstep[1] = 1.f / (float)vh;
  P.gstep[2] = 1.f / (float)vd;
  // rotation: m[j] = column j of R, un-flipping MATLAB's flip(R) (render.cpp:211-221)
  const float *r = a->rotation_flipped;
  const float X[3] = {r[2], r[1], r[0]}, Y[3] = {r[5], r[4], r[3]}, Z[3] = {r[8], r[7], r[6]};
  const float xoff = a->props[0], f = a->props[1], dist = a->props[2];
  for (int i = 0; i < 3; ++i) {
    P.eye[i] = fmaf(-dist, Z[i], xoff * X[i]);
    P.ydir[i] = Y[i];
    P.zdir[i] = Z[i];
  }
  const float xx = fmaf(X[2], X[2], fmaf(X[1], X[1], X[0] * X[0]));
  const float xinv = 1.f / sqrtf(xx);
  for (int i = 0; i < 3; ++i) P.nx_[i] = X[i] * xinv;
  P.focal = f;
  // textures through the slot indices (getTexture, kernel.cu:127-144)
  P.em = dev_tex(g_tex.bind[g_tex.idx_em]);
  {  // the emission buffer's occupancy map (the empty-space probe; null: none, no probe)
    const BufPtr &eb = g_tex.bind[g_tex.idx_em];
    P.occ = (eb && eb->ptr && eb->occ) ? eb->occ : nullptr;
    constexpr uint64_t E = 1u << VR_OCC_LOG;
    P.occ_bx = P.occ ? (uint32_t)((eb->dims[0] + 2 + E - 1) / E) : 0u;
    P.occ_bxy = P.occ ? P.occ_bx * (uint32_t)((eb->dims[1] + 2 + E - 1) / E) : 0u;
  }
  P.ab = dev_tex(g_tex.bind[g_tex.idx_ab]);
  P.re = dev_tex(g_tex.bind[g_tex.idx_re]);
  P.gem = dev_tex(g_tex.bind[T_EM]);
  P.gx = dev_tex(g_tex.bind[T_DX]);
  P.gy = dev_tex(g_tex.bind[T_DY]);
  P.gz = dev_tex(g_tex.bind[T_DZ]);
  P.lut = dev_tex(g_tex.bind[T_LIGHT]);
  // the z-paired copy's offsets are twice the plain LUT's (exact: integers below 2^25)
  P.lutz_fpx8 = 2.f * P.lut.fpx4;
  P.lutz_fpxy8 = 2.f * P.lut.fpxy4;
  P.lutz_fbase8 = 2.f * P.lut.fbase4;
  P.lutz_px8 = 8u * P.lut.px;
  P.num_lights = (int32_t)g_tex.lights.size();
  P.lights = nullptr;  // staged per launch on the launch's stream (stage_frame)
  F.mode = P.num_lights == 0 ? 0 : (g_tex.grad_method == G_LOOKUP ? 2 : 1);
  F.ab_alias = same_tex(P.ab, P.em);
  const bool em_grid = P.em.p && !P.em.one;  // the centre sample computes its three axes
  if (F.mode == 1)
    F.share = em_grid && same_tex(P.gem, P.em);
  else if (F.mode == 2)
    F.share = em_grid && P.gx.p && P.gy.p && P.gz.p && !P.gx.one && same_dims(P.gx, P.em) &&
              same_dims(P.gy, P.em) && same_dims(P.gz, P.em);
  P.re_is_em = same_tex(P.re, P.em) && P.em.p != nullptr;
  // staging halo per axis, in emission texels (vr_stage.h axis_range): the gradient tap offset
  // gstep * bscale * n (0.5 for a cube) plus a margin that bounds the drift between a predicted
  // position fma(step, k, pos) and k sequentially rounded additions (|pos| <= |box| + |eye|), per
  // sample of the chunk; set_chunk_halo scales it by the launch's chunk length
  {
    drift_bound(F, nullptr);
    for (int i = 0; i < 3; ++i) {
      const float n = i == 0 ? P.em.fnx : (i == 1 ? P.em.fny : P.em.fnz);
      P.tap_off[i] = (float)((F.mode == 1 ? (double)P.gstep[i] * P.bscale[i] * n : 0.0) + 0.0625);
    }
    P.tap_half = half_texel_taps(P, F.mode, P.em.fnz);
    // (n / 2 per axis, exact: n a power of two)
    P.cube_hs[0] = P.tap_half ? P.em.fnx * 0.5f : 0.f;
    P.cube_hs[1] = P.tap_half ? P.em.fny * 0.5f : 0.f;
    P.cube_hs[2] = P.tap_half ? P.em.fnz * 0.5f : 0.f;
  }
  // Empty-sample skip: a sample with alpha == 0 adds fma(eds, c, ill) * 0 to the
  // sum; that is exactly +-0 (a no-op) whenever the illumination term `ill` is finite, which holds
  // if the reflection texture, the LUT, the light colours, the colour and Fr are finite and small.
  {
    const BufPtr &rb = g_tex.bind[g_tex.idx_re];
    const BufPtr &lb = g_tex.bind[T_LIGHT];
    bool ok = tame(rb) && tame(lb) && std::isfinite(P.fr) && std::fabs(P.fr) < 1e3f;
    double bound = 1.0;
    for (int i = 0; i < 3; ++i) {
      ok = ok && std::isfinite(P.color[i]) && std::fabs(P.color[i]) < 1e3f;
      bound = std::max(bound, (double)std::fabs(P.color[i]));
    }
    double lmax = 0.0;
    for (const auto &L : g_tex.lights) {
      for (float c : {L.cr, L.cg, L.cb}) {
        ok = ok && std::isfinite(c);
        lmax = std::max(lmax, (double)std::fabs(c));
      }
    }
    const double rmax = (rb && rb->ptr) ? rb->maxabs : 0.0, lutmax = (lb && lb->ptr) ? lb->maxabs : 0.0;
    ok = ok && (double)std::fabs(P.fr) * rmax * lutmax * lmax * bound * (double)(g_tex.lights.size() + 1) < 1e36;
    P.skip_empty = ok ? 1 : 0;
    if (const char *ev = test_env("VR_NO_EMPTY_SKIP"))  // A/B switch for measurements
      if (ev[0] == '1') P.skip_empty = 0;
    // test switch: chunks are staged without asking the occupancy map first (vr_march.hip)
    if (P.skip_empty && test_flag("VR_NO_BRICK_TEST")) P.skip_empty = 2;
  }
  // Per-sample range tests the upload statistics decide for the whole launch (vr_sampling.h): every
  // opacity argument |Fa * ab(p) * tstep| below 2^-7 (the exponential's Taylor form needs no
  // per-sample check), and every |Fe * em(p) * tstep| finite (the empty-sample skip needs no
  // per-sample magnitude test).  A trilinear sample never exceeds its texture's largest |voxel|.
  {
    const BufPtr &eb = g_tex.bind[g_tex.idx_em], &ab = g_tex.bind[g_tex.idx_ab];
    auto vmax = [](const BufPtr &b) { return (b && b->ptr) ? (b->nonfinite ? INFINITY : (double)b->maxabs) : 0.0; };
    const double xa = std::fabs((double)P.fa) * vmax(ab) * (double)P.tstep;
    const double xe = std::fabs((double)P.fe) * vmax(eb) * (double)P.tstep;
    P.small_x = (std::isfinite(xa) && xa < 0x1p-7 * 0.999) ? 1 : 0;
    P.eds_finite = (std::isfinite(xe) && xe < 1e38) ? 1 : 0;
    if (diag_flag("VR_NO_RANGE_FLAGS")) P.small_x = P.eds_finite = 0;  // A/B switch (DIAG build)
  }
  {
    const bool re_ok = P.re_is_em || (P.re.p && P.re.one);
    // (at most 8192 texels per LUT axis: the tame shading forms the LUT's filter weights with
    // vr_sampling.h weight8_rn, which needs a texel coordinate below 2^14)
    const bool lut_ok = g_tex.lights.empty() || (P.lut.p && P.lut.small && !P.lut.one && P.lut.zp &&
                                                 std::max(P.lut.nx, std::max(P.lut.ny, P.lut.nz)) <= 8192);
    // (tstep > 0: the march's t only grows, which advance_k relies on)
    const bool step_ok = std::isfinite(P.tstep) && P.tstep > 0.f;
    P.tame = (P.skip_empty && P.eds_finite && P.small_x && re_ok && lut_ok && step_ok && !diag_flag("VR_NO_TAME")) ? 1
                                                                                                            : 0;
    P.re_mask = P.re_is_em ? 0xffffffffu : 0u;
    F.flags = (re_ok ? VR_LF_RE_OK : 0u) | (lut_ok ? VR_LF_LUT_OK : 0u);
  }
  F.big = is_big(P.em) || is_big(P.ab) || is_big(P.re) || is_big(P.gem) || is_big(P.gx) || is_big(P.gy) ||
          is_big(P.gz) || test_flag("VR_FORCE_BIG");  // test switch: the 64-bit path on small volumes
  // the lookup gradient's bricked copy has 8 ceil(px/2) ceil(py/2) ceil(pz/2) entries, more than the
  // padded voxels: just under 2^32 voxels its 32-bit entry index would wrap (e.g. 1623^3)
  if (F.mode == 2 && P.gx.p &&
      vr::interleave3_entries(P.gx.px, P.gx.pxy / P.gx.px, (uint32_t)P.gx.nz + 2u) > 0xFFFFFFFFull)
    F.big = true;
  if (is_big(P.lut)) return fail(VR_ERR_UNSUPPORTED, "illumination volume larger than 2^32 voxels");
  bool finite = std::isfinite(P.tstep) && P.tstep > 0.f;
  for (int i = 0; i < 3; ++i) finite = finite && std::isfinite(P.bmin[i]) && std::isfinite(P.bscale[i]);
  // a sample-count cap every wave reaches: 2x the longest chord through the box in steps
  const double diag = std::sqrt(4.0 * ((double)bmax[0] * bmax[0] + (double)bmax[1] * bmax[1] +
                                       (double)bmax[2] * bmax[2]));
  const double cap = 2.0 * diag / (double)P.tstep + 64.0;
  P.max_steps = (finite && cap < 2.0e9) ? (int32_t)cap : 2000000000;
  // test switch: a lower cap, which ends rays inside the volume (and inside a chunk) -- the same for
  // every kernel of the frame, so renders with it compare across kernels like any others
  if (const char *ev = test_env("VR_MAX_STEPS")) {
    const long v = std::strtol(ev, nullptr, 10);
    if (v > 0 && v < (long)P.max_steps) P.max_steps = (int32_t)v;
  }
  F.degenerate = !finite;  // no synced emission volume: nothing to march through (renders zeros)
  F.flags |= (P.tame ? VR_LF_TAME : 0u) | (P.small_x ? VR_LF_SMALL_X : 0u) | (P.eds_finite ? VR_LF_EDS_FINITE : 0u) |
             (P.skip_empty ? VR_LF_SKIP_EMPTY : 0u) | (P.tap_half ? VR_LF_TAP_HALF : 0u) |
             (F.ab_alias ? VR_LF_AB_ALIAS : 0u) | (F.share ? VR_LF_SHARE : 0u) | (F.big ? VR_LF_BIG : 0u) |
             (P.occ ? VR_LF_OCC : 0u);
  g_last_launch_flags = F.flags;
  return VR_OK;
}

// copyLightSources + setIlluminationTexture (render.cpp:145-191, kernel.cu:600-609,682-689)
void upload_lights(vr_context *h, const vr_render_args *a) {
  if (a->num_lights < 0 || !a->illumination) return;  // either argument is the logical false
  const size_t n = (size_t)a->num_lights;
  g_tex.lights.resize(n);
  for (size_t l = 0; l < n; ++l) {
    const vr_light &L = a->lights[l];
    g_tex.lights[l] = vr::DevLight{L.position[2], L.position[1], L.position[0], L.color[0], L.color[1],
                                   L.color[2]};
  }
  h->vol[T_LIGHT] = make_rec(a->illumination);
  sync_volume_if_changed(h, T_LIGHT, T_LIGHT);
}

// The lights / LUT arguments of a lit render: the argument checks, the memory check of the LUT beside
// the handle's volumes, then upload_lights.  required (optional): that memory, for the caller's own
// check of what it allocates on top.
int check_lights(const vr_render_args *a) {
  if (a->num_lights > 0 && !a->lights) return fail(VR_ERR_ARGUMENT, "lights is NULL");
  if (a->num_lights >= 0)
    if (int rc = check_dtype(a->illumination, true, "illumination volume")) return rc;
  return VR_OK;
}
int check_and_upload_lights(vr_context *h, const vr_render_args *a, uint64_t *required) {
  if (int rc = check_lights(a)) return rc;
  uint64_t need = required_memory(h);
  if (a->num_lights >= 0 && a->illumination) {
    need += a->illumination->dims[0] * a->illumination->dims[1] * a->illumination->dims[2] * 4 +
            (uint64_t)a->num_lights * sizeof(vr::DevLight);
    if (int rc = check_free_device_memory(need)) return rc;
  }
  upload_lights(h, a);
  if (required) *required = need;
  return VR_OK;
}

// What a launch reads (vr_resources.h): every bound texture buffer (and the interleaved lookup
// gradient) is marked with the launch's completion event by finish(); the frame's light list is
// staged on the launch stream.
void wait_ready(const BufPtr &b, hipStream_t s) {  // a replica's peer copy, possibly on another stream
  if (b && !vr_host::done(b->ready)) VR_HIP(hipStreamWaitEvent(s, b->ready->e, 0));
}
static void bind_reads(LaunchRec &L) {
  for (const BufPtr &b : g_tex.bind)
    if (b) {
      wait_ready(b, L.stream);
      L.reads.push_back(b);
    }
  for (const auto &kv : g_tex.gvec)
    if (kv.second.buf && kv.first == L.device) {
      wait_ready(kv.second.buf, L.stream);  // built by a launch on another stream, maybe still running
      L.reads.push_back(kv.second.buf);
    }
}
LaunchRec launch_rec(const vr_context *h, hipStream_t stream) {  // a launch of h's device that reads the bound textures
  LaunchRec L;
  L.stream = stream;
  L.device = h->device;
  bind_reads(L);
  return L;
}
void stage_frame(LaunchRec &L, vr::RenderParams &P, const std::vector<vr::DevLight> &lights) {
  const void *d = nullptr;
  VR_HIP(L.stage(lights.data(), lights.size() * sizeof(vr::DevLight), &d));
  P.lights = static_cast<const vr::DevLight *>(d);
}

int64_t part_columns(int64_t w, int32_t bc, int32_t part, int32_t np) {
  if (w <= 0) return 0;
  if (np <= 1) return w;
  const int64_t nblocks = (w + bc - 1) / bc;
  int64_t cols = 0;
  for (int64_t b = part; b < nblocks; b += np) cols += std::min<int64_t>(bc, w - b * bc);
  return cols;
}

int validate_partition(const vr_partition *p) {
  if (!p) return VR_OK;
  if (p->num_parts < 1 || p->part < 0 || p->part >= p->num_parts || p->block_cols < 1)
    return fail(VR_ERR_ARGUMENT, "invalid partition");
  return VR_OK;
}

// The partition fields of a launch's RenderParams (part null: the whole image), its output and counters;
// row-major tiles.  plane_cols: the widest part's columns, the stride of every part's planes.
void set_partition(vr::RenderParams &P, const vr_partition *part, float *d_out, unsigned long long *d_steps) {
  P.block_cols = part ? part->block_cols : std::max<int32_t>(P.width, 1);
  P.part = part ? part->part : 0;
  P.num_parts = part ? part->num_parts : 1;
  P.part_cols = (int32_t)part_columns(P.width, P.block_cols, P.part, P.num_parts);
  P.plane_cols = (int32_t)part_columns(P.width, P.block_cols, 0, P.num_parts);
  P.out = d_out;
  P.steps = d_steps;
  P.tile_mode = 0;
}


// Longest chunk (samples per ray) of the march built for K depth lanes (vr_march.hip VR_CHUNK);
// the staging halo's rounding margin covers that many sequential additions.
int chunk_samples(int K) { return K >= 2 ? 16 * K : 32; }
void set_chunk_halo(Frame &F, int K) {
  for (int i = 0; i < 3; ++i) {
    F.P.tap_off[i] += (float)(chunk_samples(K) * F.drift1[i]);
  }
}

void free_schedules(vr_context *h) {
  for (auto &kv : h->sched) {
    if (kv.second.copied) (void)hipEventSynchronize(kv.second.copied);
    if (kv.second.d_cost) (void)hipFree(kv.second.d_cost);
    if (kv.second.d_order) (void)hipFree(kv.second.d_order);
    if (kv.second.h_cost) (void)hipHostFree(kv.second.h_cost);
    if (kv.second.pre_flag) (void)hipFree(kv.second.pre_flag);
    if (kv.second.pre_count) (void)hipFree(kv.second.pre_count);
    if (kv.second.pre_state) (void)hipFree(kv.second.pre_state);
    if (kv.second.copied) (void)hipEventDestroy(kv.second.copied);
  }
  h->sched.clear();
}

// The march objects of the library (Makefile KS / EKS): fast for K = 1, 2, 4; the exact-arithmetic
// variant (a parity reference, VR_EXACT_SHADE=1) for K = 1, 2 only (libvrhip.so size) -- the image is
// the same for every K; all of them and K = 8 in a VR_WITH_K8 build.  There is no K = 8 slab or views
// kernel: a K = 8 row carries the K = 4 ones (their callers cap K at 4).  tw x th: TileShape<K>.
#define VR_MARCH_ROW(ns, k, ks, tw, th)                                                                   \
  {k, tw, th, vr::ns::launch_march_k##k, vr::ns::launch_march_slab_k##ks, vr::ns::launch_march_views_k##ks, \
   vr::ns::march_blocks_k##k, vr::ns::launch_preleap_k##k}
const MarchEntries &march_entries(bool fast, int K) {
  static const MarchEntries fast_rows[] = {VR_MARCH_ROW(fast, 1, 1, 8, 8), VR_MARCH_ROW(fast, 2, 2, 4, 8),
                                           VR_MARCH_ROW(fast, 4, 4, 4, 4),
#if VR_WITH_K8
                                           VR_MARCH_ROW(fast, 8, 4, 2, 4),
#endif
  };
  static const MarchEntries exact_rows[] = {VR_MARCH_ROW(exact, 1, 1, 8, 8), VR_MARCH_ROW(exact, 2, 2, 4, 8),
#if VR_WITH_K8
                                            VR_MARCH_ROW(exact, 4, 4, 4, 4), VR_MARCH_ROW(exact, 8, 4, 2, 4),
#endif
  };
  const MarchEntries *rows = fast ? fast_rows : exact_rows;
  int i = (int)(fast ? sizeof fast_rows : sizeof exact_rows) / (int)sizeof(MarchEntries) - 1;
  while (i > 0 && rows[i].K > K) --i;
  return rows[i];
}
#undef VR_MARCH_ROW
int exact_lanes(int K, bool fast) { return march_entries(fast, K).K; }
// Depth lanes of the march kernel (lanes per ray).  One wave marches 64 / K rays;
// its run time is that of its longest ray, so the launch lasts at least as long as the slowest
// wave however many the GPU runs at once.  With few waves per wave slot of the device (a small
// image, or one GPU's share of a multi-GPU partition) K > 1 cuts that tail K-fold; with many,
// K = 1 avoids the per-group compositing overhead.  VR_DEPTH_LANES=1/2/4/8 overrides.
static int device_wave_slots() {
  static int slots = 0;
  if (!slots) {
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) {
      hipDeviceProp_t prop;
      if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        cus = prop.multiProcessorCount;
    }
    slots = cus * 16;  // the heuristics' unit: 16 waves per CU (the march runs 20-24 per CU)
  }
  return slots;
}

// Depth lanes of a launch from its length (K = 1 waves per device wave slot) and the texels a pixel
// spans (P.tau; 0 = unknown, taken as 1).  Few rounds: K = 4 shortens the tail.  Otherwise the
// staged box -- the hull of a wave's ray bundle over a chunk -- decides: its lateral extent grows
// with tau and with the tile (64 / K rays), and a hull that overflows the slot halves the chunk and
// restages.  Measured on MI355X (ms): tau 2.0 (C2, 1024x768, 3 rounds) K = 4 19.5, K = 2 29.8,
// K = 8 25.1; tau 1.07 (metric, 7.9 rounds) K = 2 36.5, K = 4 37.6, K = 1 51.7; tau 1.0 (C5,
// 4096^2, 64 rounds) K = 2 293.6, K = 4 338.5, K = 1 348.7.  K = 1 only for sparse sampling.

int depth_lanes(const vr::RenderParams &P) {
  if (const char *ev = test_env("VR_DEPTH_LANES")) {
    const int k = std::atoi(ev);
    if (k == 1 || k == 2 || k == 4 || (k == 8 && VR_WITH_K8)) return k;
  }
  const double waves = std::ceil(P.part_cols / 8.0) * std::ceil(P.height / 8.0);  // at K = 1
  const double rounds = waves / device_wave_slots();
  const double tau = P.tau > 0.f ? (double)P.tau : 1.0;
  // a lookup-gradient frame: K = 4, whose four consecutive samples per ray gather mostly the same
  // corner lines of the gradient copy -- C3 (tau 1.07, 7.9 rounds) 27.90-27.99 ms with 6.5 KiB slots
  // vs 28.87-28.94 at K = 2 (r5z); K = 4 with 10 KiB slots 29.8, K = 1 52.4 (r5y)
  if (P.lookup) return 4;
  if (rounds < VR_DEPTH_ROUNDS_K2 || tau >= VR_DEPTH_TAU_K4) return 4;
  if (rounds >= VR_DEPTH_ROUNDS_K1 && tau < VR_DEPTH_TAU_K1) return 1;
  return 2;
}

// texels a pixel spans at the volume, tau = dist * vw / (W * f) (pixel pitch 2/W on the image plane
// at f, box x-extent 2 = vw texels), and the wave slot size it asks for at the launch's depth lanes:
// wide (10 KiB, vr_stage.h) slots once the hull of a wave's tile passes tau 1.5 (K <= 2, tau 2.0:
// 18 % faster than 6.5 KiB), and for every K = 4 launch (round 5, below).  VR_WIDE_SLOT=0/1 overrides (A/B).
void set_tau_and_slot(vr::RenderParams &P, const vr_render_args *a, double vw) {
  const double f = std::fabs((double)a->props[1]), dist = std::fabs((double)a->props[2]);
  const double tau = (f > 0 && P.width > 0) ? dist * vw / ((double)P.width * f) : 1e30;
  P.tau = (float)std::min(tau, 1e30);
  // Round 5: with the empty-space probe the wide slots win for every K = 4 launch -- C2 (tau 2.0)
  // 12.18-12.20 vs 13.13 ms at 12 KiB (r5p), 10.90-10.93 ms at 10 KiB (r5u), the P = 8 / P = 4
  // parts of the metric frame (tau 1.07, short launches) 4.85-4.87 vs 5.26-5.27 / 8.48-8.51 vs
  // 8.81-8.83 ms (r5s; 10 KiB: 4.82-5.00 / 8.00, r5t-u); at K = 2 they still lose below
  // tau 1.5 (metric frame 30.2-30.3 vs 26.9-27.0 ms, P = 2 parts 15.15 vs 14.80-14.84 ms).  Round 4
  // measured the opposite at K = 4 (20.7 vs 19.5 ms at C2), when every empty chunk staged its box.
  const int K = P.steps ? 1 : depth_lanes(P);
  P.wide_slot = (tau > 1.5 || (K >= 4 && !P.lookup)) ? 1 : 0;  // (lookup frames: r5y above)
  if (const char *ev = test_env("VR_WIDE_SLOT")) P.wide_slot = std::atoi(ev) ? 1 : 0;
}

// Longest-first schedule: a frame of the same shape as an earlier one launches its workgroups in
// the order of that frame's measured block durations, so the long tiles start first instead of
// forming the tail (the image is the same for any order).  VR_SCHED=0: off.  Only for short
// launches (< VR_SCHED_ROUNDS K = 1 waves per device wave slot): with many rounds the tail is a
// small part of the frame and the row-major order keeps neighbouring tiles (which share voxels in
// L2) running together (metric frame: 43.6 ms row-major, 45.0 ms sorted).
// Full frames (>= VR_SCHED_ROUNDS) follow a heavy-first schedule (order_heavy_kernel: the previous
// launch's heaviest blocks first, the rest row-major): a block of rays grazing dense structure can
// last a whole frame (33 ms of 36 at rotate(30,10,0)) and, started in row-major order, forms a tail
// the rest of the frame cannot fill.  VR_SCHED=0: no schedule; VR_SCHED_FULL=0: none for full frames.
bool short_launch(const vr::RenderParams &P) {
  const double rounds = std::ceil(P.part_cols / 8.0) * std::ceil(P.height / 8.0) * std::max(1, (int)P.views) /
                        device_wave_slots();
  return rounds < VR_SCHED_ROUNDS;
}
// Very long launches (>= VR_SCHED_LPT_ROUNDS K = 1 waves per wave slot) take the short launches'
// longest-first schedule as well: C5 (V_shell(2048), 4096^2, 64 rounds) 216.6-217.1 vs 219.1-219.6 ms
// heavy-first (r5as); the metric frame (7.9 rounds) keeps heavy-first (26.58-26.60 vs 26.32-26.53, r5ae).
#ifndef VR_SCHED_LPT_ROUNDS
#define VR_SCHED_LPT_ROUNDS 32.0
#endif
static bool lpt_launch(const vr::RenderParams &P) {
  const double rounds = std::ceil(P.part_cols / 8.0) * std::ceil(P.height / 8.0) * std::max(1, (int)P.views) /
                        device_wave_slots();
  return rounds < VR_SCHED_ROUNDS || rounds >= VR_SCHED_LPT_ROUNDS;
}
bool want_schedule(const vr::RenderParams &P) {
  // fused stereo (two views in one launch, vr_render_stereo) is scheduled over both views' blocks;
  // not the paired-tile measurement (VR_STEREO_PAIR), nor the multi-view channel kernel
  if (P.views > 2 || (P.views == 2 && test_flag("VR_STEREO_PAIR")) || test_flag_off("VR_SCHED")) return false;
  return test_flag("VR_SCHED") || short_launch(P) || !test_flag_off("VR_SCHED_FULL");
}

// launch_order's tail argument: (tail_pct << 32) | resident workgroups; tail_pct 0 = heavy-first.
static uint64_t wg_tail_arg(uint32_t tail_pct) {
  return (uint64_t)tail_pct << 32 | (uint64_t)(device_wave_slots() / 16 * 6);
}

// What a tile block's cost depends on beyond the launch shape (round 6): the camera (eyes, axes,
// focal length), the sampling (box, step), the opacity parameters and the volume -- the emission
// buffer and the upload its occupancy map was built from.  A schedule measured or predicted under
// another key is stale (a movie turns the camera every frame, examples/example2.m:53-66).
static uint64_t frame_key(const vr::RenderParams &P) {
  uint64_t h = 1469598103934665603ull;  // FNV-1a
  auto mix = [&h](const void *p, size_t n) {
    const unsigned char *c = static_cast<const unsigned char *>(p);
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
  };
  mix(P.eye, sizeof P.eye);
  mix(P.eye2, sizeof P.eye2);
  mix(P.nx_, sizeof P.nx_);
  mix(P.ydir, sizeof P.ydir);
  mix(P.zdir, sizeof P.zdir);
  mix(&P.focal, sizeof P.focal);
  mix(P.bmin, sizeof P.bmin);
  mix(&P.tstep, sizeof P.tstep);
  mix(&P.thr, sizeof P.thr);
  mix(&P.fa, sizeof P.fa);
  mix(&P.fe, sizeof P.fe);
  mix(&P.em.p, sizeof P.em.p);
  mix(&P.occ, sizeof P.occ);
  const BufPtr &eb = g_tex.bind[g_tex.idx_em];
  const uint64_t ver = (eb && eb->ptr == P.em.p) ? eb->version : 0;
  mix(&ver, sizeof ver);
  return h | 1u;  // never 0
}

#ifndef VR_PRED_STEP_TEXELS
#define VR_PRED_STEP_TEXELS 8.0  // the predictor's step along a ray, in texels (one occupancy brick)
#endif
// The predicted block costs of this launch into cost[] (vr_kernels.hip predict_cost_kernel): from
// the emission texture's occupancy map, the early exit modelled with the absorption (= emission,
// the scheduled launches' aliasing) bricks' mean densities.
static hipError_t predict_costs(const vr::RenderParams &P, const MarchEntries &M, uint32_t nb_view, uint32_t *cost,
                                 hipStream_t stream) {
  const int K = M.K, TW = M.tile_w, TH = M.tile_h;
  const uint32_t nbx = (uint32_t)((P.part_cols + 2 * TW - 1) / (2 * TW));
  const BufPtr &eb = g_tex.bind[g_tex.idx_em];
  double dens = 0.0;
  if (eb && !eb->nonfinite && P.fa > 0.f && std::isfinite(P.fa))
    dens = (double)P.fa * (double)eb->maxabs / 255.0 * (double)P.tstep;
  const double xthr = P.thr < 1.f ? -std::log1p(-(double)std::max(P.thr, 0.f)) : 1e30;
  // samples per predictor step: ~VR_PRED_STEP_TEXELS texels along the axis a sample advances most on
  double tpa = 0.0;  // texels per world unit, largest axis
  for (int i = 0; i < 3; ++i) {
    const float n = i == 0 ? P.em.fnx : (i == 1 ? P.em.fny : P.em.fnz);
    tpa = std::max(tpa, (double)P.bscale[i] * (double)n);
  }
  const double per = (double)P.tstep * tpa;  // texels per sample at most
  const int m = (int)std::max(1.0, std::min(4096.0, std::floor(VR_PRED_STEP_TEXELS / std::max(per, 1e-9))));
  const hipError_t rc = vr::launch_predict_cost(P, nb_view, nbx, TW, TH, m, (float)dens, (float)std::min(xthr, 1e30),
                                                cost, stream);
  // VR_SCHED_PRED_DUMP=file (DIAG build): append the predicted costs as tools/sched_dump.py's records
  if (const char *dump = rc == hipSuccess ? diag_env("VR_SCHED_PRED_DUMP") : nullptr) {
    const uint32_t nb = nb_view * (uint32_t)std::max(1, (int)P.views);
    std::vector<uint32_t> c(nb);
    VR_HIP(hipMemcpyAsync(c.data(), cost, (size_t)nb * 4, hipMemcpyDeviceToHost, stream));
    VR_HIP(hipStreamSynchronize(stream));
    const uint32_t hdr[4] = {(uint32_t)K, (uint32_t)P.part, (uint32_t)P.num_parts, nb};
    if (FILE *f = std::fopen(dump, "ab")) {
      std::fwrite(hdr, 4, 4, f);
      std::fwrite(c.data(), 4, c.size(), f);
      std::fclose(f);
    }
  }
  return rc;
}

// Attach the schedule of this launch shape (`extra` tells launches of one shape apart, e.g. the
// slab and sweep of a sort-last launch) to P: wg_order / wg_cost / sched_blocks / prio_blocks.
hipError_t attach_schedule(vr_context *h, vr::RenderParams &P, Frame &F, int K, hipStream_t stream,
                           const char *extra) {
  const MarchEntries &M = march_entries(P.fast_shade != 0, K);
  const uint32_t nb_view = M.blocks(P);
  const uint32_t nb = nb_view * (uint32_t)std::max(1, (int)P.views);  // (fused stereo: both views' blocks)
  // keyed by stream too: the order buffer of one stream is never rewritten under another's launch
  char key[300];
  std::snprintf(key, sizeof key, "%d/%d/%d/%d/%d/%d/%d/%d/%d/%u/%p/%s", K, P.width, P.height, P.part, P.num_parts,
                P.block_cols, F.mode, P.wide_slot, P.fast_shade, nb, (void *)stream, extra);
  vr_context::Schedule &S = h->sched[key];
  F.sched = &S;
  if (!S.d_cost && nb) {
    hipError_t e = hipMalloc(&S.d_cost, nb * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&S.d_order, nb * sizeof(uint32_t));
    if (e != hipSuccess) {
      vr_host::consume(e, "hipMalloc (launch schedule; the launch runs unscheduled)");
      if (S.d_cost) (void)hipFree(S.d_cost);
      S.d_cost = nullptr;
      S.d_order = nullptr;
    }
    S.blocks = nb;
  }
  if (!(S.d_cost && S.blocks == nb)) return hipSuccess;
  hipError_t rc = hipSuccess;
  const bool full = !lpt_launch(P) && !test_flag("VR_SCHED");  // VR_SCHED=1: longest-first everywhere
  // Round 6: block costs predicted from the occupancy map (predict_costs) wherever no measurement of
  // this very frame exists -- every full frame, and a short launch whose camera or volume changed.
  // VR_SCHED_MEASURED=1 (DIAG build, A/B): the round-5 schedules from measured durations only.
  const uint64_t fkey = frame_key(P);
  const bool predict = P.occ && P.occ_bx && !diag_flag("VR_SCHED_MEASURED");
  if (!full) {  // short launch: every launch measured, ordered longest first by the previous one
    P.sched_full = 0;
    if (S.measured && S.key == fkey) {
      rc = vr::launch_order(S.d_cost, nb, S.d_order, stream, 0u, 0u);
    } else if (predict) {  // no measurement of this frame: longest first by the predicted costs
      rc = predict_costs(P, M, nb_view, S.d_cost, stream);
      if (rc == hipSuccess) rc = vr::launch_order(S.d_cost, nb, S.d_order, stream, 0u, 0u);
    } else {  // first launch of this frame without a map: row-major order, durations recorded
      rc = vr::launch_iota(S.d_order, nb, stream);
    }
    S.measured = true;  // (this launch records its durations)
    S.key = fkey;
    S.pred_key = 0;
  } else {
    // Full frame.  Round 6: the first render of a frame (camera, volume: frame_key) follows the
    // heavy-first order (order_heavy_kernel) of the block costs predicted from the occupancy map,
    // untimed -- a movie turns the camera every frame (examples/example2.m:53-66), so most of its
    // frames are first renders; the second render of the same frame runs timed in that order, and
    // once its durations have reached the host every later render follows the heavy-first order of
    // the measured durations (re-measured every VR_SCHED_REMEASURE-th render; a timed full-frame
    // kernel costs ~5 %).  Without a map (small volumes) the first render is the timed row-major
    // launch.  Whether the heaviest measured block would form a tail (>= VR_SCHED_TAIL_PCT % of the
    // packed frame: the sum of durations over the resident workgroups) decides between the
    // heavy-first order and none (round 5: VR_SCHED_TAIL_PCT 0, always heavy-first).
    if (S.key != fkey) {  // another camera or volume: what was measured does not describe this frame
      if (S.copy_pending) {
        (void)hipEventSynchronize(S.copied);
        S.copy_pending = false;
      }
      S.measured = S.decided = S.tail = S.order_stale = false;
      S.frames = S.renders = 0;
      S.key = fkey;
    }
    ++S.renders;
    uint32_t every = VR_SCHED_REMEASURE;
    if (const char *ev = test_env("VR_SCHED_REMEASURE")) every = (uint32_t)std::max(1, std::atoi(ev));
    uint32_t heavy_div = VR_SCHED_HEAVY_DIV;
    if (const char *ev = diag_env("VR_SCHED_HEAVY_DIV")) heavy_div = (uint32_t)std::max(1, std::atoi(ev));
    uint32_t tail_pct = VR_SCHED_TAIL_PCT;
    if (const char *ev = test_env("VR_SCHED_TAIL_PCT")) tail_pct = (uint32_t)std::max(0, std::atoi(ev));
    if (!S.h_cost) {
      hipError_t e = hipHostMalloc(reinterpret_cast<void **>(&S.h_cost), nb * sizeof(uint32_t));
      if (e == hipSuccess) e = hipEventCreateWithFlags(&S.copied, hipEventDisableTiming);
      if (e != hipSuccess) {
        vr_host::consume(e, "hipHostMalloc / hipEventCreate (full-frame schedule; none used)");
        return hipSuccess;  // no schedule
      }
    }
    if (S.copy_pending && vr_host::query_done(S.copied, "hipEventQuery (schedule durations)")) {  // arrived
      S.copy_pending = false;
      uint64_t sum = 0;
      uint32_t mx = 0;
      for (uint32_t i = 0; i < nb; ++i) {
        sum += S.h_cost[i];
        mx = std::max(mx, S.h_cost[i]);
      }
      const uint64_t wg_slots = std::max<uint64_t>(1, (uint64_t)(device_wave_slots() / 16 * 6));
      S.tail = (uint64_t)mx * 100u >= (sum / wg_slots) * tail_pct;
      S.decided = true;
      S.order_stale = true;
    }
    if (predict && !S.decided) {  // nothing measured of this frame (yet): the predicted order
      if (S.pred_key != fkey) {
        rc = predict_costs(P, M, nb_view, S.d_cost, stream);
        if (rc == hipSuccess) rc = vr::launch_order(S.d_cost, nb, S.d_order, stream, heavy_div, wg_tail_arg(0));
        S.pred_key = rc == hipSuccess ? fkey : 0;
      }
      // (VR_SCHED_PREDICT_ONLY=1, DIAG build: never measured -- the predictor's own order, A/B)
      if (S.renders >= 2 && !S.measured && !diag_flag("VR_SCHED_PREDICT_ONLY")) {  // a repeated frame: measured once
        S.measured = true;
        S.frames = 0;
        P.sched_full = 1;
        F.sched_copy = &S;
      } else {
        P.sched_full = 2;
      }
    } else {
      S.pred_key = 0;  // (d_cost holds durations from here on)
      bool measure = !S.measured;
      if (S.measured && !S.copy_pending && ++S.frames >= every) measure = true;
      if (measure) {
        S.frames = 0;
        if (S.decided && S.tail) {  // measured in the heavy-first order the frames use
          if (S.order_stale) rc = vr::launch_order(S.d_cost, nb, S.d_order, stream, heavy_div, wg_tail_arg(0));
        } else {
          rc = vr::launch_iota(S.d_order, nb, stream);
        }
        S.order_stale = false;
        S.measured = true;
        P.sched_full = 1;  // timed; the durations are copied back after the launch
        F.sched_copy = &S;
      } else if (S.decided && S.tail) {
        if (S.order_stale) {
          rc = vr::launch_order(S.d_cost, nb, S.d_order, stream, heavy_div, wg_tail_arg(0));
          S.order_stale = false;
        }
        P.sched_full = 2;  // the heavy-first order, untimed
      } else {
        return hipSuccess;  // no tail (or not known yet): the unscheduled row-major launch
      }
    }
  }
  if (rc != hipSuccess) return rc;
  P.wg_order = S.d_order;
  P.wg_cost = S.d_cost;
  P.sched_blocks = nb;
  // the first round of workgroups (the longest ones) at raised wave priority (A/B: VR_PRIO_BLOCKS);
  // none for a full frame, whose first blocks are only the heavy ones
  P.prio_blocks = P.sched_full ? 0u : (uint32_t)(device_wave_slots() / 4);
  if (const char *ev = diag_env("VR_PRIO_BLOCKS")) P.prio_blocks = (uint32_t)std::atoi(ev);
  return hipSuccess;
}

}  // namespace vr_host
