// vr_features.hip -- the feature renders on the host (vr_host.h): projection, slice, isosurface and
// transfer-function render, each on the frame of build_frame (vr_frame.hip) and its own kernel file, and
// the volume histogram (no frame: one source texture, as the slice).
#include <cassert>

#include "vr_host.h"
#include "vr_transfer.h"

namespace vr_host {

// `count` floats of an output plane set to one bit pattern (a degenerate frame's zeros and NaNs)
constexpr uint32_t VR_QNAN_BITS = 0x7fc00000u;  // the quiet NaN the kernels write for "no value"
static void fill_plane(float *d, uint32_t bits, size_t count, hipStream_t stream) {
  if (d && count) VR_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(d), (int)bits, count, stream));
}

// Projection render (vr_render_projection, vr_project.hip): the frame geometry, the probe margin and
// the occupancy pointers of build_frame and the partition fields of set_partition; no lights are
// uploaded or staged, and nothing of the texture unit, the slot indices or the march's schedules is
// written -- a render before and after a projection gives the same bits.
int do_project(vr_context *h, const vr_render_args *a, int32_t mode, const vr_partition *part, float *d_out,
               float *d_aux, unsigned long long *d_steps, hipStream_t stream) {
  Frame F;
  int rc = build_frame(h, a, F);
  if (rc) return rc;
  rc = validate_partition(part);
  if (rc) return rc;
  vr::RenderParams &P = F.P;
  set_partition(P, part, d_out, d_steps);
  P.views = 1;
  const size_t plane = (size_t)P.plane_cols * (size_t)P.height;
  if (plane && !d_out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  if (F.degenerate) {  // no synced emission volume: render's zeros, and every ray a miss
    fill_plane(d_out, 0u, plane * 3, stream);
    fill_plane(d_aux, mode == VR_PROJ_MIP ? VR_QNAN_BITS : 0u, plane, stream);
    return VR_OK;
  }
  // VR_PROJ_NO_PROBE=1 (test switch): every sample fetched, no empty-space leap
  const bool probe = P.occ != nullptr && !test_flag("VR_PROJ_NO_PROBE");
  LaunchRec L = launch_rec(h, stream);
  const vr::ClipSet clip = clip_set(h, P);
  VR_HIP(vr::launch_project(P, mode, d_aux, F.big, probe, stream, &clip));
  VR_HIP(L.finish());
  return VR_OK;
}

// The argument checks of vr_render_slice (include/vrhip.h): before the handle, no device needed.
int check_slice(const vr_slice *s) {
  if (!s) return fail(VR_ERR_ARGUMENT, "slice: the slice is NULL");
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(s->origin[i]) || !std::isfinite(s->du[i]) || !std::isfinite(s->dv[i]) ||
        !std::isfinite(s->dw[i]))
      return fail(VR_ERR_ARGUMENT, "slice: non-finite origin / du / dv / dw");
  if (s->samples < 1 || s->samples > VR_SLICE_MAX_SAMPLES)
    return fail(VR_ERR_ARGUMENT, "slice: 1 .. " + std::to_string(VR_SLICE_MAX_SAMPLES) + " samples");
  if (s->mode != VR_SLICE_MAX && s->mode != VR_SLICE_MIN && s->mode != VR_SLICE_SUM)
    return fail(VR_ERR_ARGUMENT, "slice: unknown slice mode");
  if (s->source != VR_SLICE_EMISSION && s->source != VR_SLICE_ABSORPTION && s->source != VR_SLICE_REFLECTION)
    return fail(VR_ERR_ARGUMENT, "slice: unknown slice source");
  const uint64_t H = s->resolution[0], W = s->resolution[1];
  if (H > 0x7FFFFFFFull || W > 0x7FFFFFFFull || H * W >= (1ull << 31))
    return fail(VR_ERR_ARGUMENT, "slice: image resolution too large (H * W must be below 2^31)");
  return VR_OK;
}

// Cache lines (128 B) one row load of a wave touches when neighbouring lanes are `step` apart in q: the
// lanes' cells lie a = step * dims voxels apart, so they fall into 1 + 63 min(1, |a1| + |a2|) rows of the
// volume, and a row's share of the lanes spans 63 |a0| / 32 more lines in all; at most one line per lane.
static double slice_lines(const float step[3], const vr::DevTex &t) {
  const double a0 = std::fabs((double)step[0] * t.nx), a1 = std::fabs((double)step[1] * t.ny),
               a2 = std::fabs((double)step[2] * t.nz);
  return std::min(64.0, 1.0 + 63.0 * std::min(1.0, a1 + a2) + 63.0 * a0 / 32.0);
}

// Which output axis runs along a wave's lanes: the lines a wave touches for its 4 row
// loads per slab sample plus the lines its stores touch -- 2 per plane along y, the contiguous axis of a
// column-major plane, 64 per plane along x -- a stored line weighted 4 times a loaded one (measured: a
// scattered store costs more than a scattered load, profiles/round17).  VR_SLICE_LANES=x|y (test
// switch) forces either side.
#define VR_SLICE_STORE_WEIGHT 4.0
static bool slice_lanes_x(const vr_slice *s, const vr::DevTex &t, int planes) {
  if (const char *ev = test_env("VR_SLICE_LANES")) {
    if (ev[0] == 'x') return true;
    if (ev[0] == 'y') return false;
  }
  if (!t.p || t.one) return false;  // no gather: the contiguous store decides
  const double loads = 4.0 * (double)s->samples;
  return loads * slice_lines(s->du, t) + VR_SLICE_STORE_WEIGHT * 64.0 * planes <
         loads * slice_lines(s->dv, t) + VR_SLICE_STORE_WEIGHT * 2.0 * planes;
}

// Slice render (vr_render_slice, vr_slice.hip): the DevTex of the one source texture through the slot
// indices, as build_frame binds it; no camera, no frame, no lights.  Nothing of the handle, the texture
// unit or the last launch flags is written.
int do_slice(vr_context *h, const vr_slice *s, float *d_out, float *d_aux, float *d_lab, hipStream_t stream) {
  vr::SliceParams S{};
  S.height = (int32_t)s->resolution[0];
  S.width = (int32_t)s->resolution[1];
  const size_t plane = (size_t)S.width * (size_t)S.height;
  if (plane && !d_out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  if (!plane) return VR_OK;
  const int32_t slot = s->source == VR_SLICE_EMISSION ? g_tex.idx_em
                       : s->source == VR_SLICE_ABSORPTION ? g_tex.idx_ab : g_tex.idx_re;
  S.tex = dev_tex(g_tex.bind[slot]);  // (getTexture, kernel.cu:127-144)
  for (int i = 0; i < 3; ++i) {
    S.origin[i] = s->origin[i];
    S.du[i] = s->du[i];
    S.dv[i] = s->dv[i];
    S.dw[i] = s->dw[i];
  }
  S.samples = s->samples;
  S.out = d_out;
  S.aux = d_aux;
  S.lab = d_lab;
  const bool labels = d_lab && h->d_labels && h->labels_bytes;
  if (labels) {
    S.labels = h->d_labels;
    for (int i = 0; i < 3; ++i) S.ld[i] = (int32_t)h->labels_dims[i];
  } else {  // no labels resident: the whole plane is NaN
    fill_plane(d_lab, VR_QNAN_BITS, plane, stream);
  }
  S.lanes_x = slice_lanes_x(s, S.tex, 1 + (d_aux ? 1 : 0) + (d_lab ? 1 : 0)) ? 1 : 0;
  const bool big = is_big(S.tex) || test_flag("VR_FORCE_BIG");
  LaunchRec L = launch_rec(h, stream);
  VR_HIP(vr::launch_slice(S, s->mode, big, stream));
  VR_HIP(L.finish());
  if (labels) {
    vr_host::EventPtr ev;
    if (vr_host::record_event(stream, ev) == hipSuccess) h->labels_readers.add(ev);
    else VR_HIP(hipStreamSynchronize(stream));
  }
  return VR_OK;
}

// The argument checks of vr_volume_histogram (include/vrhip.h): before the handle, no device needed.
int check_hist_bins(int32_t nbins, const float lim[2]) {
  if (nbins < 1 || nbins > VR_HIST_MAX_BINS)
    return fail(VR_ERR_ARGUMENT, "histogram: 1 .. " + std::to_string(VR_HIST_MAX_BINS) + " bins");
  if (!std::isfinite(lim[0]) || !std::isfinite(lim[1]) || !(lim[0] < lim[1]))
    return fail(VR_ERR_ARGUMENT, "histogram: limits must be finite with lo < hi");
  const float w = lim[1] - lim[0];
  if (!std::isfinite(w) || !std::isfinite(1.0f / w))
    return fail(VR_ERR_ARGUMENT, "histogram: hi - lo and 1 / (hi - lo) must be finite in fp32");
  return VR_OK;
}
int32_t histogram_rows(const vr_histogram *q) { return q->label_count > 0 ? q->label_count + 1 : 1; }
int check_histogram(const vr_histogram *q) {
  if (!q) return fail(VR_ERR_ARGUMENT, "histogram: the query is NULL");
  if (q->source != VR_SLICE_EMISSION && q->source != VR_SLICE_ABSORPTION && q->source != VR_SLICE_REFLECTION)
    return fail(VR_ERR_ARGUMENT, "histogram: unknown source");
  if (int rc = check_hist_bins(q->nbins, q->lim)) return rc;
  if (q->label_first < 0 || q->label_first > 255 || q->label_count < 0 || q->label_count > 256 ||
      q->label_first + q->label_count > 256)
    return fail(VR_ERR_ARGUMENT, "histogram: label_first 0 .. 255, label_count 0 .. 256, first + count <= 256");
  if ((int64_t)histogram_rows(q) * q->nbins > VR_HIST_MAX_CELLS)
    return fail(VR_ERR_ARGUMENT, "histogram: rows * nbins must not exceed " + std::to_string(VR_HIST_MAX_CELLS));
  if (q->use_clip != 0 && q->use_clip != 1) return fail(VR_ERR_ARGUMENT, "histogram: use_clip must be 0 or 1");
  return VR_OK;
}

// Volume histogram (vr_volume_histogram, vr_histogram.hip): the DevTex of the one source texture through
// the slot indices, as do_slice resolves it; the clip planes as they were set (q is the kernel's own
// coordinate, no conversion).  The counts and the row accumulators are zeroed on the launch's stream --
// the accumulators as a zero blob through the launch's staged constants -- then the count launch and,
// for d_rows, the finalize launch.  Nothing of the handle, the texture unit or the last launch flags is
// written.  The kernel's wave-uniform shortcut is off -- it won on the zero-heavy volume and lost on the
// incoherent one -- unless VR_HIST_UNIFORM=0|1 (test switch) forces either side.
#define VR_HIST_UNIFORM_DEFAULT false
static bool hist_uniform() {
  if (const char *ev = test_env("VR_HIST_UNIFORM")) {
    if (ev[0] == '0') return false;
    if (ev[0] == '1') return true;
  }
  return VR_HIST_UNIFORM_DEFAULT;
}
int do_histogram(vr_context *h, const vr_histogram *q, unsigned long long *d_counts, vr_hist_row *d_rows,
                 hipStream_t stream) {
  if (!d_counts) return fail(VR_ERR_ARGUMENT, "histogram: counts is NULL");
  vr::HistParams H{};
  H.rows = histogram_rows(q);
  H.nbins = q->nbins;
  const int32_t slot = q->source == VR_SLICE_EMISSION ? g_tex.idx_em
                       : q->source == VR_SLICE_ABSORPTION ? g_tex.idx_ab : g_tex.idx_re;
  H.tex = dev_tex(g_tex.bind[slot]);  // (getTexture, kernel.cu:127-144)
  const bool bound = H.tex.p && H.tex.nx > 0 && H.tex.ny > 0 && H.tex.nz > 0;
  const bool labels = q->label_count > 0;
  if (labels) {
    if (!h->d_labels || !h->labels_bytes)
      return fail(VR_ERR_ARGUMENT, "histogram: rows by label need resident labels (vr_sync_labels)");
    if (bound && (h->labels_dims[0] != (uint64_t)H.tex.nx || h->labels_dims[1] != (uint64_t)H.tex.ny ||
                  h->labels_dims[2] != (uint64_t)H.tex.nz)) {
      std::ostringstream os;
      os << "histogram: the labels' dims [" << h->labels_dims[0] << " " << h->labels_dims[1] << " "
         << h->labels_dims[2] << "] differ from the source texture's [" << H.tex.nx << " " << H.tex.ny << " "
         << H.tex.nz << "]";
      return fail(VR_ERR_ARGUMENT, os.str());
    }
    H.labels = h->d_labels;
  }
  H.lo = q->lim[0];
  H.hi = q->lim[1];
  H.inv = 1.0f / (q->lim[1] - q->lim[0]);
  H.label_first = q->label_first;
  H.label_count = q->label_count;
  if (q->use_clip)
    for (int32_t i = 0; i < h->nclip; ++i) {
      for (int c = 0; c < 3; ++c) H.clip.pl[i][c] = h->clip[i].normal[c];
      H.clip.pl[i][3] = h->clip[i].offset;
      H.clip.n = i + 1;
    }
  H.counts = d_counts;
  LaunchRec L = launch_rec(h, stream);
  VR_HIP(hipMemsetAsync(d_counts, 0, (size_t)H.rows * (size_t)H.nbins * sizeof(unsigned long long), stream));
  const std::vector<char> zeros(vr::hist_acc_bytes(H.rows), 0);
  const void *d_acc = nullptr;
  VR_HIP(L.stage(zeros.data(), zeros.size(), &d_acc));
  H.acc = const_cast<void *>(d_acc);
  if (bound) {
    // no workgroup may see 2^32 voxels: its 32-bit LDS cells could wrap
    const uint64_t nrows = (uint64_t)H.tex.ny * (uint64_t)H.tex.nz;
    const uint64_t blocks = vr::histogram_blocks(nrows, (uint64_t)H.tex.nx);
    assert(((nrows + blocks - 1) / blocks) * (uint64_t)H.tex.nx < (1ull << 32));
    (void)blocks;
    VR_HIP(vr::launch_histogram(H, hist_uniform(), stream));
  }
  if (d_rows) VR_HIP(vr::launch_histogram_finalize(d_counts, H.acc, H.rows, H.nbins, d_rows, stream));
  VR_HIP(L.finish());
  if (labels && bound) {
    vr_host::EventPtr ev;
    if (vr_host::record_event(stream, ev) == hipSuccess) h->labels_readers.add(ev);
    else VR_HIP(hipStreamSynchronize(stream));
  }
  return VR_OK;
}

// Isosurface render (vr_render_isosurface, vr_isosurface.hip): the lights and the LUT uploaded and
// checked (check_and_upload_lights), the frame geometry, the probe margin and the occupancy pointers of
// build_frame, the partition fields of set_partition.  The gradient method is the handle's whether or
// not there are lights (the normal plane needs it).  Only the handle's light and LUT state is
// written, as by a render: nothing of the texture unit, the slot indices or the march's schedules.
int do_isosurface(vr_context *h, const vr_render_args *a, float level, const vr_partition *part, float *d_out,
                  float *d_depth, float *d_normal, unsigned long long *d_steps, hipStream_t stream) {
  int rc = check_and_upload_lights(h, a);
  if (rc) return rc;
  Frame F;
  rc = build_frame(h, a, F);
  if (rc) return rc;
  rc = validate_partition(part);
  if (rc) return rc;
  vr::RenderParams &P = F.P;
  set_partition(P, part, d_out, d_steps);
  P.views = 1;
  P.fast_shade = 0;
  if (P.lut.p == nullptr) P.num_lights = 0;  // no LUT: no illumination term
  const size_t plane = (size_t)P.plane_cols * (size_t)P.height;
  if (plane && !d_out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  if (F.degenerate) {  // no synced emission volume: no surface anywhere
    fill_plane(d_out, 0u, plane * 3, stream);
    fill_plane(d_depth, VR_QNAN_BITS, plane, stream);
    fill_plane(d_normal, VR_QNAN_BITS, plane * 3, stream);
    return VR_OK;
  }
  // VR_ISO_NO_PROBE=1 (test switch): every sample fetched, no empty-space leap
  const bool probe = P.occ != nullptr && level > 0.f && !test_flag("VR_ISO_NO_PROBE");
  LaunchRec L = launch_rec(h, stream);
  stage_frame(L, P, g_tex.lights);
  const vr::ClipSet clip = clip_set(h, P);
  VR_HIP(vr::launch_isosurface(P, g_tex.grad_method == G_LOOKUP ? 2 : 1, level, d_depth, d_normal, F.big, probe,
                               stream, &clip));
  VR_HIP(L.finish());
  return VR_OK;
}

// The table checks of vr_render_transfer (include/vrhip.h): before the handle, no device needed.
static int check_table(const float *t, int32_t n, int32_t planes, const float lim[2], const char *what) {
  if (n < 2 || n > VR_TF_MAX_ENTRIES)
    return fail(VR_ERR_ARGUMENT, std::string(what) + ": 2 .. " + std::to_string(VR_TF_MAX_ENTRIES) + " entries");
  for (int64_t i = 0; i < (int64_t)n * planes; ++i)
    if (!std::isfinite(t[i])) return fail(VR_ERR_ARGUMENT, std::string(what) + ": non-finite entry");
  if (!std::isfinite(lim[0]) || !std::isfinite(lim[1]) || !(lim[0] < lim[1]))
    return fail(VR_ERR_ARGUMENT, std::string(what) + ": limits must be finite with lo < hi");
  return VR_OK;
}
int check_transfer(const vr_transfer *tf) {
  if (!tf || !tf->colormap) return fail(VR_ERR_ARGUMENT, "transfer function / colormap is NULL");
  if (int rc = check_table(tf->colormap, tf->n_color, 3, tf->clim, "colormap")) return rc;
  if (tf->alphamap)
    if (int rc = check_table(tf->alphamap, tf->n_alpha, 1, tf->alim, "alphamap")) return rc;
  if (tf->coord != VR_TF_VALUE && tf->coord != VR_TF_DEPTH) return fail(VR_ERR_ARGUMENT, "unknown colormap coordinate");
  return VR_OK;
}

// L(T, n, lim, c) on the host: the kernel's lookup (vr_transfer.h) on the segment record of c
float transfer_lookup(const float *T, int32_t n, const float lim[2], float c) {
  const float inv = 1.0f / (lim[1] - lim[0]);
  float w;
  const int32_t i = vr_tf_segment(c, lim[0], inv, n, &w);
  return vr_tf_value(w, T[i], T[i + 1] - T[i]);
}

// Staging ring of the transfer render's constants (segment records + light list) above the 4 KiB slots
// of vr_host::ConstRing -- a 256-entry colormap is 8160 B, the largest tables 40 920 B: pinned host slots
// and their device twins, a slot copied with hipMemcpyAsync on the launch's stream and rewritten only
// after the launch that last read it completed (its event), as ConstRing does.  No allocation, no
// null-stream copy per frame.  16 slots: a caller may have that many transfer launches in flight
// before the host waits for the oldest.
struct TableRing {
  static constexpr size_t SLOT = 48 * 1024;
  static constexpr unsigned N = 16;
  char *host = nullptr, *dev = nullptr;
  vr_host::EventPtr ev[N];
  unsigned next = 0;
  hipError_t init() {
    if (host && dev) return hipSuccess;
    hipError_t rc = hipHostMalloc(reinterpret_cast<void **>(&host), SLOT * N, hipHostMallocDefault);
    if (rc == hipSuccess) rc = vr_host::device_alloc(reinterpret_cast<void **>(&dev), SLOT * N);
    if (rc != hipSuccess) {  // all or nothing: a later call retries
      if (host) (void)hipHostFree(host);
      host = nullptr;
      dev = nullptr;
    }
    return rc;
  }
};
static std::map<int, TableRing> &table_rings() {
  static std::map<int, TableRing> &r = *new std::map<int, TableRing>();  // never destroyed (see g_tex)
  return r;
}

// Transfer-function render (vr_render_transfer, vr_transfer.hip): the lights and the LUT uploaded and
// checked (check_and_upload_lights), the frame of build_frame, the partition fields of set_partition.  The
// tables travel as segment records {T[i], T[i+1] - T[i]} in the launch's staged constants, in front of
// the light list: one copy ordered on the launch's stream, through ConstRing up to 4 KiB and through
// TableRing above (only a light list that pushes the payload past 48 KiB takes LaunchRec's dedicated
// allocation, as a render's would).  Only the handle's light and LUT state is written, as by a render.
int do_transfer(vr_context *h, const vr_render_args *a, const vr_transfer *tf, const vr_partition *part, float *d_out,
                float *d_alpha, unsigned long long *d_steps, hipStream_t stream) {
  int rc = check_and_upload_lights(h, a);
  if (rc) return rc;
  Frame F;
  rc = build_frame(h, a, F);
  if (rc) return rc;
  rc = validate_partition(part);
  if (rc) return rc;
  vr::RenderParams &P = F.P;
  set_partition(P, part, d_out, d_steps);
  P.views = 1;
  P.fast_shade = 0;
  if (P.lut.p == nullptr) P.num_lights = 0;  // no LUT: no illumination term
  const size_t plane = (size_t)P.plane_cols * (size_t)P.height;
  if (plane && !d_out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  if (F.degenerate) {  // no synced emission volume: zeros everywhere
    fill_plane(d_out, 0u, plane * 3, stream);
    fill_plane(d_alpha, 0u, plane, stream);
    return VR_OK;
  }
  const int grad = P.num_lights == 0 ? 0 : (g_tex.grad_method == G_LOOKUP ? 2 : 1);
  const int32_t nc = tf->n_color, na = tf->alphamap ? tf->n_alpha : 0;
  // the staged constants: the segment records (16-byte units), then the light list
  const size_t tab_bytes = (size_t)vr::transfer_table_units(nc, na) * 16;
  std::vector<float> blob((tab_bytes + g_tex.lights.size() * sizeof(vr::DevLight)) / sizeof(float), 0.f);
  for (int32_t i = 0; i + 1 < nc; ++i) {
    float *r = blob.data() + 8 * (size_t)i;  // {r, dr, g, dg}, {b, db, 0, 0}
    for (int c = 0; c < 3; ++c) {
      const float *T = tf->colormap + (size_t)c * (size_t)nc;
      r[2 * c] = T[i];
      r[2 * c + 1] = T[i + 1] - T[i];
    }
  }
  for (int32_t i = 0; i + 1 < na; ++i) {
    float *r = blob.data() + 8 * (size_t)(nc - 1) + 2 * (size_t)i;  // {A, dA}
    r[0] = tf->alphamap[i];
    r[1] = tf->alphamap[i + 1] - tf->alphamap[i];
  }
  if (!g_tex.lights.empty())
    std::memcpy(reinterpret_cast<char *>(blob.data()) + tab_bytes, g_tex.lights.data(),
                g_tex.lights.size() * sizeof(vr::DevLight));
  const float cinv = 1.0f / (tf->clim[1] - tf->clim[0]);
  const float ainv = na ? 1.0f / (tf->alim[1] - tf->alim[0]) : 0.f;
  // Empty-space leap: only where a leaped sample (em = ab = +-0) adds exactly 0 -- the absorption
  // sample is the emission sample, Fa * A(+-0) * tstep == 0 (alpha = 1 - exp(-0) = 0), Fe finite (the
  // emission term is +-0 times a finite table entry) and, when lit, the shading term proven finite.
  // As the projection and isosurface leaps, this takes the running sums for finite: table entries so
  // large that sa overflows to +-inf would make (1 - sa) * 0 a NaN on the marched path only.
  // VR_TF_NO_PROBE=1 (test switch): every sample fetched.
  bool probe = P.occ != nullptr && F.ab_alias && std::isfinite(P.fe) && (grad == 0 || P.skip_empty) &&
               !test_flag("VR_TF_NO_PROBE");
  for (float z : {0.f, -0.f}) {
    const float A = na ? transfer_lookup(tf->alphamap, na, tf->alim, z) : z;
    probe = probe && (P.fa * A) * P.tstep == 0.f;
  }
  LaunchRec L = launch_rec(h, stream);
  const void *d_blob = nullptr;
  const size_t blob_bytes = blob.size() * sizeof(float);
  TableRing *ring = nullptr;
  int slot = -1;
  if (blob_bytes > vr_host::ConstRing::SLOT && blob_bytes <= TableRing::SLOT) {
    ring = &table_rings()[h->device];
    VR_HIP(ring->init());
    slot = (int)(ring->next++ % TableRing::N);
    vr_host::wait(ring->ev[slot]);  // the launch that used this slot N launches ago
    ring->ev[slot].reset();
    char *hs = ring->host + (size_t)slot * TableRing::SLOT, *ds = ring->dev + (size_t)slot * TableRing::SLOT;
    std::memcpy(hs, blob.data(), blob_bytes);
    VR_HIP(hipMemcpyAsync(ds, hs, blob_bytes, hipMemcpyHostToDevice, stream));
    d_blob = ds;
  } else {
    VR_HIP(L.stage(blob.data(), blob_bytes, &d_blob));
  }
  P.lights = reinterpret_cast<const vr::DevLight *>(static_cast<const char *>(d_blob) + tab_bytes);
  const vr::ClipSet clip = clip_set(h, P);
  const hipError_t le = vr::launch_transfer(P, grad, static_cast<const float *>(d_blob), nc, na, tf->clim[0], cinv,
                                            na ? tf->alim[0] : 0.f, ainv, tf->coord, F.ab_alias, d_alpha, F.big, probe,
                                            stream, &clip);
  if (ring) {  // the slot is free again when everything enqueued so far (its copy, the launch) completed
    vr_host::EventPtr ev;
    const hipError_t re = vr_host::record_event(stream, ev);
    if (re != hipSuccess) {  // cannot track: wait here instead
      vr_host::consume(re, "record_event (transfer table slot; waited for instead)");
      (void)hipStreamSynchronize(stream);
    }
    ring->ev[slot] = ev;
  }
  VR_HIP(le);
  VR_HIP(L.finish());
  return VR_OK;
}

}  // namespace vr_host
