// vr_sync.hip -- what vr_sync_volumes and the label calls do to the device (vr_host.h):
//   - the persistent memory manager the reference (vr/mm/mmanager.hxx) (dedup by (ptr, last_update,
//     size), the memory checks)
//   - the upload / texture-binding state machine of the reference (vr/volumeRender_kernel.cu:600-867),
//     re-expressed as host state: "textures" are bindings of device buffers (fp32 volumes resident in HBM,
//     read by the software sampler of vr_kernels.hip), the slot indices d_idx* stay module-global exactly
//     as in the reference
//   - deconvolution, Gaussian smoothing and label gains, one derivation from the unmodified upload
//     
#include "vr_host.h"

namespace vr_host {

// operator== (volumeRender.cpp:24-26); the element type is part of the identity: two views of one
// buffer with different types are different volumes
bool same(const VolRec &a, const VolRec &b) {
  return a.data == b.data && a.last_update == b.last_update && a.memory_size == b.memory_size && a.dtype == b.dtype;
}

VolRec make_rec(const vr_volume *v) {
  VolRec r;
  if (!v) return r;
  r.data = v->data;
  for (int i = 0; i < 3; ++i) r.dims[i] = v->dims[i];
  r.memory_size = v->dims[0] * v->dims[1] * v->dims[2] * sizeof(float);  // the resident (fp32) size
  r.last_update = v->last_update;
  r.location = v->location;
  r.dtype = v->dtype;
  return r;
}

// A volume argument's element type (include/vrhip.h vr_dtype): VR_OK, or the error of an invalid
// code / flag combination or a data pointer not aligned to its element size; `fp32_only` for the
// illumination LUT and the gradient volumes.
int check_dtype(const vr_volume *v, bool fp32_only, const char *what) {
  if (!v) return VR_OK;
  const size_t es = vr::dtype_size(v->dtype);
  if (!es) return fail(VR_ERR_ARGUMENT, std::string(what) + ": invalid dtype");
  if (fp32_only && v->dtype != VR_F32)
    return fail(VR_ERR_UNSUPPORTED, std::string(what) + ": must be fp32 (typed volumes are for emission, reflection "
                                                       "and absorption)");
  if (reinterpret_cast<uintptr_t>(v->data) % es)
    return fail(VR_ERR_ARGUMENT, std::string(what) + ": data is not aligned to its element size");
  return VR_OK;
}

// syncVolume (kernel.cu:659-672): unbind the texture, drop the old array, upload the volume into a
// device buffer and bind it.  The handle's previous buffer of the slot is rewritten in place when
// nothing else holds it and no launch still reads it; otherwise a fresh buffer is taken and the old
// one is freed when its last launch completes (a render of the previous frame may be in flight on
// another stream while this frame's volumes upload, vr_resources.h).
// The LUT's z-paired copy (DevBuf::zpair) for a texture small enough for fetch_small and not a
// single voxel; rebuilt with every upload into the buffer (the buffer's readers have completed).
// VR_NO_ZPAIR=1: none (the fast kernels then shade without the tame path, an A/B switch).
static void build_zpair(DevBuf *b, hipStream_t s) {
  const uint64_t padded = (b->dims[0] + 2) * (b->dims[1] + 2) * (b->dims[2] + 2);
  const bool want = padded < (1ull << 22) && !(b->dims[0] == 1 && b->dims[1] == 1 && b->dims[2] == 1) &&
                    !diag_flag("VR_NO_ZPAIR");
  if (!want) {
    if (b->zpair) vr_host::pooled_free(b->zpair, b->zpair_bytes, b->device, vr_host::Readers(b->readers));
    b->zpair = nullptr;
    b->zpair_bytes = 0;
    return;
  }
  const uint64_t bytes = 2 * padded * sizeof(float);
  if (!b->zpair || b->zpair_bytes != bytes) {
    if (b->zpair) vr_host::pooled_free(b->zpair, b->zpair_bytes, b->device, vr_host::Readers(b->readers));
    b->zpair = nullptr;
    b->zpair_bytes = 0;
    // (the size is recorded only once the allocation exists: a failed allocation leaves no buffer
    // that a later upload of the same size would take for allocated)
    VR_HIP(vr_host::pooled_alloc(reinterpret_cast<void **>(&b->zpair), bytes, b->device));
    b->zpair_bytes = bytes;
  }
  const uint32_t pxy = (uint32_t)((b->dims[0] + 2) * (b->dims[1] + 2));
  VR_HIP(vr::launch_zpair(b->ptr, b->zpair, (uint32_t)padded, pxy, s));
  VR_HIP(hipStreamSynchronize(s));
}

// The occupancy map of buffer b (DevBuf::occ) for the march's empty-space probe, rebuilt with every
// upload into it (its readers have completed); none for small volumes (the probe needs a map only
// where leaps are long) or with VR_NO_PROBE=1.
#ifndef VR_OCC_MIN_VOXELS
#define VR_OCC_MIN_VOXELS (1ull << 18)
#endif
static void build_occupancy(DevBuf *b, hipStream_t s) {
  const uint64_t px = b->dims[0] + 2, py = b->dims[1] + 2, pz = b->dims[2] + 2;
  const bool want = px * py * pz >= VR_OCC_MIN_VOXELS && px < (1ull << 31) && !test_flag("VR_NO_PROBE");
  constexpr uint64_t E = 1u << VR_OCC_LOG;  // brick edge
  const uint64_t bytes = want ? ((px + E - 1) / E) * ((py + E - 1) / E) * ((pz + E - 1) / E) : 0;
  if (!want || b->occ_bytes != bytes) {
    if (b->occ) vr_host::pooled_free(b->occ, b->occ_bytes, b->device, vr_host::Readers(b->readers));
    b->occ = nullptr;
    b->occ_bytes = 0;
  }
  if (!want) return;
  if (!b->occ) {
    VR_HIP(vr_host::pooled_alloc(reinterpret_cast<void **>(&b->occ), bytes, b->device));
    b->occ_bytes = bytes;
  }
  // (the bytes also carry each brick's mean |voxel| for the schedule predictor, in 1/255 of the largest)
  const float inv = (!b->nonfinite && b->maxabs > 0.f) ? 255.f / b->maxabs : 0.f;
  VR_HIP(vr::launch_occupancy(b->ptr, (uint32_t)px, (uint32_t)py, (uint32_t)pz, b->occ, std::isfinite(inv) ? inv : 0.f,
                              s));
  VR_HIP(hipStreamSynchronize(s));
}

// Forget that b was smoothed or modulated by label gains: its unmodified copy goes back to the pool (no launch reads it).
static void drop_unmodified_copy(DevBuf *b) {
  if (b->orig) vr_host::pooled_free(b->orig, b->bytes, b->device, vr_host::Readers());
  b->orig = nullptr;
  b->mod_labels = b->mod_gains = b->mod_smooth = b->mod_deconv = 0;
}

static void sync_volume(vr_context *h, int tex, int slot) {
  g_tex.bind[tex].reset();
  const VolRec &v = h->vol[slot];
  const uint64_t n = v.dims[0] * v.dims[1] * v.dims[2];
  const uint64_t padded = n ? (v.dims[0] + 2) * (v.dims[1] + 2) * (v.dims[2] + 2) * sizeof(float) : 0;
  BufPtr b = h->buf[slot];
  if (!(b && b.use_count() == 2 && b->bytes == padded && b->device == h->device && b->readers.done())) {
    h->buf[slot].reset();
    b = std::make_shared<DevBuf>();
    b->device = h->device;
    b->bytes = padded;
    if (padded) VR_HIP(vr_host::pooled_alloc(reinterpret_cast<void **>(&b->ptr), padded, h->device));
  }
  drop_unmodified_copy(b.get());  // (the upload overwrites the derived values: apply_derived starts afresh)
  for (int i = 0; i < 3; ++i) b->dims[i] = v.dims[i];
  b->nonfinite = false;
  b->maxabs = 0.f;
  b->readers.clear();  // a fresh buffer, or one whose readers all completed
  if (n) {
    if (!v.data) throw HipError{hipErrorInvalidValue, "volume data is NULL"};
    vr_host::Uploader &U = vr_host::uploaders()[h->device];
    VR_HIP(U.init(h->device));
    vr::BufStats st{0u, 0.f};
    VR_HIP(U.upload(v.data, v.dtype, v.location == VR_DEVICE, (int32_t)v.dims[0], (int32_t)v.dims[1],
                    (int32_t)v.dims[2], b->ptr, &st));
    b->nonfinite = st.nonfinite != 0;
    b->maxabs = st.maxabs;
    if (tex == T_LIGHT) build_zpair(b.get(), U.stream);
    else if (tex <= T_RE) build_occupancy(b.get(), U.stream);  // (only these can be bound as emission)
  } else {
    build_occupancy(b.get(), nullptr);  // (an empty volume: drops a previous map)
  }
  b->version = next_version();
  b->src_data = v.data;
  b->src_last_update = v.last_update;
  b->src_bytes = v.memory_size;
  b->src_dtype = v.dtype;
  h->buf[slot] = b;
  g_tex.bind[tex] = b;
}

// setIlluminationTexture / setGradientTextures (kernel.cu:682-722) re-upload their volume on every
// call.  Here the upload is skipped when the texture is still bound to a buffer uploaded from the
// same Volume -- the identity the reference's own dedup uses for the emission / absorption /
// reflection volumes (data pointer, TimeLastUpdate, size; volumeRender.cpp:24-26).  The image is
// the same; the LUT (1 MiB) and in lookup mode the three gradient volumes (12 GiB at 1024^3) stop
// crossing PCIe per render.  VR_ALWAYS_REUPLOAD=1 restores the reference's behaviour.
void sync_volume_if_changed(vr_context *h, int tex, int slot) {
  const BufPtr &b = g_tex.bind[tex];
  const VolRec &v = h->vol[slot];
  if (b && h->buf[slot] == b && b->device == h->device && v.data && b->src_data == v.data &&
      b->src_last_update == v.last_update && b->src_bytes == v.memory_size && b->src_dtype == v.dtype &&
      v.last_update != 0 &&
      !env_flag("VR_ALWAYS_REUPLOAD"))
    return;
  sync_volume(h, tex, slot);
}

struct RealState {
  vr_context *h;
  int32_t idx_em, idx_ab, idx_re;  // shadow copies, written back after the decisions
  void upload(int slot) { sync_volume(h, slot, slot); }
  // referenceTexture (kernel.cu:631-648)
  void reference(int tex, int bufslot, int32_t RealState::*idx, int target) {
    if (h->buf[bufslot]) {
      g_tex.bind[tex].reset();
      h->buf[bufslot].reset();
    }
    this->*idx = target;
  }
};

// MManager::getRequiredMemory (mmanager.hxx:110-133)
uint64_t required_memory(const vr_context *h) {
  const VolRec &em = h->vol[T_EM], &ab = h->vol[T_AB], &re = h->vol[T_RE];
  uint64_t r = em.memory_size;
  if (!same(em, ab) && !same(re, ab)) r += ab.memory_size;
  if (!same(em, re) && !same(re, ab)) r += re.memory_size;
  r += h->vol[T_DX].memory_size + h->vol[T_DY].memory_size + h->vol[T_DZ].memory_size;
  // label gains: the label bytes, and the unmodified copy of the emission volume while gains are set
  r += h->labels_bytes;
  // (one copy, shared with the smoothing and the deconvolution while either is set)
  if ((h->d_labels && h->ngains > 0) || smoothing_set(h) || deconvolution_set(h)) r += em.memory_size;
  return r;
}

// MManager::checkFreeDeviceMemory (mmanager.hxx:144-173)
int check_free_device_memory(uint64_t required) {
  size_t free_b = 0, total_b = 0;
  VR_HIP(hipMemGetInfo(&free_b, &total_b));
  if (free_b >= required) return VR_OK;
  int dev = 0;  // pooled / retired buffers are free memory to MATLAB's eyes: release them, recheck
  VR_HIP(hipGetDevice(&dev));
  vr_host::pool_clear(dev);
  vr_host::prune_retired(true);
  VR_HIP(hipMemGetInfo(&free_b, &total_b));
  if (free_b >= required) return VR_OK;
  std::ostringstream os;
  os << "insufficient free VRAM!\n"
     << "\tTotal Memory (MB): \t" << total_b / (1024 * 1024) << "\n"
     << "\tFree Memory (MB): \t" << free_b / (1024 * 1024) << "\n"
     << "\tRequired memory (MB): \t" << required / (1024 * 1024) << "\n";
  return fail(VR_ERR_VRAM, os.str());
}

static void reset_gradients(vr_context *h) {  // MManager::resetGradients (mmanager.hxx:206-213)
  for (int s : {T_DX, T_DY, T_DZ}) {
    h->buf[s].reset();
    h->vol[s] = VolRec();
  }
}

// MManager::sync (mmanager.hxx:178-201)
static void mm_sync(vr_context *h) {
  if ((h->vol[T_DX].last_update == 0 && h->buf[T_DX]) || (h->vol[T_DY].last_update == 0 && h->buf[T_DY]) ||
      (h->vol[T_DZ].last_update == 0 && h->buf[T_DZ]))
    reset_gradients(h);
  const VolRec &em = h->vol[T_EM], &ab = h->vol[T_AB], &re = h->vol[T_RE];
  const uint64_t T = h->time_last_mem_sync;
  RealState s{h, g_tex.idx_em, g_tex.idx_ab, g_tex.idx_re};
  sync_decisions(s, same(em, ab), same(em, re), same(ab, re), em.last_update > T || T == 0,
                 ab.last_update > T || T == 0, re.last_update > T || T == 0);
  g_tex.idx_em = s.idx_em;
  g_tex.idx_ab = s.idx_ab;
  g_tex.idx_re = s.idx_re;
  if (h->vol[T_DX].last_update != 0 && h->vol[T_DY].last_update != 0 && h->vol[T_DZ].last_update != 0) {
    // setGradientTextures (kernel.cu:703-722): (re-)upload all three, then lookup mode
    sync_volume_if_changed(h, T_DX, T_DX);
    sync_volume_if_changed(h, T_DY, T_DY);
    sync_volume_if_changed(h, T_DZ, T_DZ);
    g_tex.grad_method = G_LOOKUP;
  }
}

// ---- label gains (include/vrhip.h vr_sync_labels / vr_set_label_gains) ----------------
// The buffer the handle's last sync bound as the emission texture (the slot index decides which).
BufPtr label_target(const vr_context *h) {
  if (!h->has_snap || h->snap_idx[0] < 0 || h->snap_idx[0] >= T_COUNT) return nullptr;
  return h->snap_bind[h->snap_idx[0]].lock();
}

// VR_OK, or the error of label dims that differ from the dims of the resident emission buffer b.
int check_label_dims(const uint64_t ld[3], const DevBuf *b) {
  if (!b || !b->ptr || (ld[0] == b->dims[0] && ld[1] == b->dims[1] && ld[2] == b->dims[2])) return VR_OK;
  std::ostringstream os;
  os << "labels: the label volume is " << ld[0] << " x " << ld[1] << " x " << ld[2] << ", the emission volume "
     << b->dims[0] << " x " << b->dims[1] << " x " << b->dims[2];
  return fail(VR_ERR_ARGUMENT, os.str());
}

static vr_host::Uploader &label_uploader(int device) {
  vr_host::Uploader &U = vr_host::uploaders()[device];
  VR_HIP(U.init(device));
  return U;
}

// b holds its unmodified upload again, with that upload's statistics and occupancy map.
static void restore_unmodified(DevBuf *b) {
  if (!b->orig) return;
  b->readers.wait();  // launches in flight read ptr and occ
  vr_host::pooled_free(b->ptr, b->bytes, b->device, vr_host::Readers());
  b->ptr = b->orig;
  b->orig = nullptr;
  b->nonfinite = b->orig_nonfinite;
  b->maxabs = b->orig_maxabs;
  b->mod_labels = b->mod_gains = b->mod_smooth = b->mod_deconv = 0;
  b->version = next_version();
  build_occupancy(b, label_uploader(b->device).pad_stream);
}

// ---- Gaussian smoothing (include/vrhip.h vr_set_smoothing) ----------------------------
bool smoothing_set(const vr_context *h) {
  return h->smooth_sigma[0] != 0.f || h->smooth_sigma[1] != 0.f || h->smooth_sigma[2] != 0.f;
}

int check_smoothing(const float sigma[3]) {
  if (!sigma) return VR_OK;
  for (int j = 0; j < 3; ++j) {
    if (!(sigma[j] >= 0.f) || !std::isfinite(sigma[j]))
      return fail(VR_ERR_ARGUMENT, "smoothing: every sigma must be finite and not negative");
    if (sigma[j] > VR_SMOOTH_MAX_SIGMA) return fail(VR_ERR_ARGUMENT, "smoothing: sigma must be at most 6 voxels");
  }
  return VR_OK;
}

int smoothing_unsupported(const char *what) {
  return fail(VR_ERR_UNSUPPORTED, std::string(what) + ": Gaussian smoothing (vr_set_smoothing) is not supported " +
                                      (std::strcmp(what, "vr_render_slab") ? "on a multi-device group handle"
                                                                           : "by a slab render: a slab's z border "
                                                                             "would be clamped"));
}

// Which form of the smoothing kernels serves three active axes: the fused launch reads
// each voxel about once and keeps a ring of 2Rz+1 tile planes in LDS, the three passes move the volume
// three times.  Measured at 1024^3, both forms interleaved (profiles/round22/smooth.json): the fused call
// takes 1.03 (V_shell) / 1.00 (random) times the passes' at sigma 1, 1.77 / 1.64 times at sigma 2 and
// 7.2 / 6.7 times at sigma 6 -- its halo recomputation and four barriers per plane cost more than the
// bytes it saves -- so the passes serve every radius and the fused form runs only when forced.
// VR_SMOOTH_FORM=fused|passes (test switch) forces either side; both give the same bits.
#ifndef VR_SMOOTH_FUSED_MAX_R
#define VR_SMOOTH_FUSED_MAX_R 0  // fused up to this largest radius of the three axes; 0: never
#endif
static bool smooth_fused(int32_t Rx, int32_t Ry, int32_t Rz) {
  if (const char *ev = test_env("VR_SMOOTH_FORM")) {
    if (ev[0] == 'f') return true;
    if (ev[0] == 'p') return false;
  }
  return std::max(Rx, std::max(Ry, Rz)) <= VR_SMOOTH_FUSED_MAX_R;
}

// ---- Richardson-Lucy deconvolution (include/vrhip.h vr_set_deconvolution) --------------
bool deconvolution_set(const vr_context *h) {
  return h->deconv_iterations > 0 &&
         (h->deconv_sigma[0] != 0.f || h->deconv_sigma[1] != 0.f || h->deconv_sigma[2] != 0.f);
}

int check_deconvolution(const float sigma[3], int32_t iterations, float flr) {
  if (sigma)
    for (int j = 0; j < 3; ++j) {
      if (!(sigma[j] >= 0.f) || !std::isfinite(sigma[j]))
        return fail(VR_ERR_ARGUMENT, "deconvolution: every sigma must be finite and not negative");
      if (sigma[j] > VR_SMOOTH_MAX_SIGMA)
        return fail(VR_ERR_ARGUMENT, "deconvolution: sigma must be at most 6 voxels");
    }
  if (iterations < 0 || iterations > VR_DECONV_MAX_ITERATIONS)
    return fail(VR_ERR_ARGUMENT, "deconvolution: iterations must be in 0..64");
  if (!(flr > 0.f) || !std::isfinite(flr))
    return fail(VR_ERR_ARGUMENT, "deconvolution: floor must be finite and greater than 0");
  return VR_OK;
}

int deconvolution_unsupported(const char *what) {
  return fail(VR_ERR_UNSUPPORTED, std::string(what) + ": the deconvolution (vr_set_deconvolution) is not supported " +
                                      (std::strcmp(what, "vr_render_slab") ? "on a multi-device group handle"
                                                                           : "by a slab render: a slab's z border "
                                                                             "would be clamped"));
}

// The iterations of the value rule on the device: y the unmodified upload, the estimate u_k in `u` (u_0 is
// never stored: iteration 0 reads y through vr_deconv_data), t1 and t2 two further volumes, all padded
// and distinct; axis[0..na-1] the active axes in ascending order with their radii R and the weights of
// axis j at wts + j * VR_SMOOTH_MAX_TAPS.  One iteration is 2 na launches: the passes of B(u), whose last
// stores the ratio into t1, and the passes of B(r), whose last stores the update into u -- reading u at
// the voxel it writes when k > 0.  t2 is needed only with more than one active axis.  With no active axis
// B is the identity and the two steps are elementwise launches.  st (may be null): the statistics of u_n.
static void run_deconvolution(const float *y, float *u, float *t1, float *t2, int32_t nx, int32_t ny, int32_t nz,
                              const int *axis, const int32_t *R, int na, const float *wts, int32_t iterations, float flr,
                              vr::BufStats *st, hipStream_t s) {
  for (int32_t k = 0; k < iterations; ++k) {
    const bool first = k == 0, last = k == iterations - 1;
    const float *cur = first ? y : u;
    if (!na) {
      VR_HIP(vr::launch_deconv_pointwise(cur, t1, nx, ny, nz, VR_EPI_RATIO, y, flr, first ? VR_EPI_LOAD_DATA : 0u, s));
      VR_HIP(vr::launch_deconv_pointwise(t1, u, nx, ny, nz, VR_EPI_UPDATE, cur, flr, first ? VR_EPI_AUX_DATA : 0u, s));
      if (last && st) VR_HIP(vr::launch_stats(u, ((uint64_t)nx + 2) * ((uint64_t)ny + 2) * ((uint64_t)nz + 2), st, s));
      continue;
    }
    const float *src = cur;
    for (int i = 0; i < na; ++i) {  // B(u); the last pass stores the ratio in t1
      float *dst = (na - 1 - i) % 2 ? t2 : t1;
      const float *w = wts + axis[i] * VR_SMOOTH_MAX_TAPS;
      const uint32_t flags = first && i == 0 ? VR_EPI_LOAD_DATA : 0u;
      if (i == na - 1)
        VR_HIP(vr::launch_deconv_axis(src, dst, nx, ny, nz, axis[i], w, R[i], VR_EPI_RATIO, y, flr, flags, nullptr, s));
      else if (flags)
        VR_HIP(vr::launch_deconv_axis(src, dst, nx, ny, nz, axis[i], w, R[i], VR_EPI_FILTER, nullptr, flr, flags, nullptr, s));
      else
        VR_HIP(vr::launch_smooth_axis(src, dst, nx, ny, nz, axis[i], w, R[i], nullptr, s));
      src = dst;
    }
    for (int i = 0; i < na; ++i) {  // B(r); the last pass stores the update in u
      const float *w = wts + axis[i] * VR_SMOOTH_MAX_TAPS;
      if (i == na - 1) {
        VR_HIP(vr::launch_deconv_axis(src, u, nx, ny, nz, axis[i], w, R[i], VR_EPI_UPDATE, cur, flr,
                                      first ? VR_EPI_AUX_DATA : 0u, last ? st : nullptr, s));
      } else {
        float *dst = src == t1 ? t2 : t1;
        VR_HIP(vr::launch_smooth_axis(src, dst, nx, ny, nz, axis[i], w, R[i], nullptr, s));
        src = dst;
      }
    }
  }
}

// Bring the handle's emission buffer up to date with its deconvolution, smoothing, labels and gains, one
// derivation from the unmodified upload: orig -> deconvolution (the iterations above over the axes with a
// PSF sigma > 0 and more than one voxel) -> smoothing (one pass per axis with sigma > 0 and more than one
// voxel, dims[0] first) -> label gains (when emission, labels and n > 0 are all present) -> ptr;
// unmodified when no pass is left; nothing is written when nothing changed.
// The first derivation of an upload takes a second buffer and swaps: the upload becomes the unmodified
// copy, the last pass writes the new ptr (no copy of the volume).  Passes in between alternate between
// ptr and one scratch volume from the pool, which goes back afterwards.  The deconvolution keeps its
// estimate in whichever of the two lets the passes after it end in ptr, and rotates through the other
// and, with more than one active axis, a second scratch volume.  The statistics fold into the
// last pass.  The state left is that of an upload of the host-rewritten volume: data and apron,
// statistics, occupancy map, a new version.  VR_ERR_VRAM (nothing changed) when the copy and the
// scratch volumes do not fit.
int apply_derived(vr_context *h) {
  BufPtr b = label_target(h);
  if (!b || !b->ptr) return VR_OK;
  bool gain = h->d_labels && h->ngains > 0;
  const int bad = gain ? check_label_dims(h->labels_dims, b.get()) : VR_OK;
  if (bad) gain = false;
  struct Pass {
    int axis;  // 0..2 a smoothing axis, 3 the gains, 4 the three axes fused
    int32_t R;
  } pass[4];
  int32_t radius[3] = {0, 0, 0};
  int np = 0;
  float wts[3 * VR_SMOOTH_MAX_TAPS] = {};
  for (int j = 0; j < 3; ++j)
    if (h->smooth_sigma[j] > 0.f && b->dims[j] > 1)
      pass[np++] = Pass{j, radius[j] = vr_smooth_weights(h->smooth_sigma[j], wts + j * VR_SMOOTH_MAX_TAPS)};
  const bool smooth = np > 0;
  if (np == 3 && smooth_fused(pass[0].R, pass[1].R, pass[2].R)) {  // the three axes in one launch
    pass[0].axis = 4;
    np = 1;
  }
  if (gain) pass[np++] = Pass{3, 0};
  // the deconvolution in front of them: its active axes (none: B is the identity, the rule still iterates)
  const bool deconv = deconvolution_set(h);
  int daxis[3], nda = 0;
  int32_t dR[3];
  float dwts[3 * VR_SMOOTH_MAX_TAPS] = {};
  if (deconv)
    for (int j = 0; j < 3; ++j)
      if (h->deconv_sigma[j] > 0.f && b->dims[j] > 1) {
        daxis[nda] = j;
        dR[nda++] = vr_smooth_weights(h->deconv_sigma[j], dwts + j * VR_SMOOTH_MAX_TAPS);
      }
  if (!np && !deconv) {
    restore_unmodified(b.get());
    return bad;
  }
  const uint64_t kl = gain ? h->labels_version : 0, kg = gain ? h->gains_version : 0,
                 ks = smooth ? h->smooth_version : 0, kd = deconv ? h->deconv_version : 0;
  if (b->orig && b->mod_labels == kl && b->mod_gains == kg && b->mod_smooth == ks && b->mod_deconv == kd) return bad;
  // scratch volumes: the passes alternate between ptr and one; the deconvolution's rotation takes that one
  // and, with more than one active axis, a second
  const int nscratch = deconv ? (nda > 1 ? 2 : 1) : (np > 1 ? 1 : 0);
  if (smooth || deconv) {  // (the gain pass alone was checked by its caller, as before)
    const uint64_t need = (b->orig ? 0 : b->bytes) + (uint64_t)nscratch * b->bytes;
    if (int rc = check_free_device_memory(need)) return rc;
  }
  vr_host::Uploader &U = label_uploader(b->device);
  if (gain && !h->d_gains)
    VR_HIP(vr_host::device_alloc(reinterpret_cast<void **>(&h->d_gains), sizeof(h->gains)));
  if (smooth && !h->d_smooth_w)
    VR_HIP(vr_host::device_alloc(reinterpret_cast<void **>(&h->d_smooth_w), sizeof(wts)));
  if (deconv && !h->d_deconv_w)
    VR_HIP(vr_host::device_alloc(reinterpret_cast<void **>(&h->d_deconv_w), sizeof(dwts)));
  b->readers.wait();  // "neither rewritten nor freed before all of them": renders in flight keep their volume
  if (!b->orig) {
    float *fresh = nullptr;
    VR_HIP(vr_host::pooled_alloc(reinterpret_cast<void **>(&fresh), b->bytes, b->device));
    b->orig = b->ptr;
    b->ptr = fresh;
    b->orig_nonfinite = b->nonfinite;
    b->orig_maxabs = b->maxabs;
  }
  b->mod_labels = b->mod_gains = b->mod_smooth = b->mod_deconv = 0;  // (until the passes below have completed)
  float *scratch = nullptr, *scratch2 = nullptr;
  try {
    if (nscratch > 0) VR_HIP(vr_host::pooled_alloc(reinterpret_cast<void **>(&scratch), b->bytes, b->device));
    if (nscratch > 1) VR_HIP(vr_host::pooled_alloc(reinterpret_cast<void **>(&scratch2), b->bytes, b->device));
    if (gain) VR_HIP(hipMemcpy(h->d_gains, h->gains, sizeof(float) * (size_t)h->ngains, hipMemcpyHostToDevice));
    if (smooth) VR_HIP(hipMemcpy(h->d_smooth_w, wts, sizeof(wts), hipMemcpyHostToDevice));
    if (deconv) VR_HIP(hipMemcpy(h->d_deconv_w, dwts, sizeof(dwts), hipMemcpyHostToDevice));
    VR_HIP(hipMemsetAsync(U.d_stats, 0, sizeof(vr::BufStats), U.pad_stream));
    const auto t0 = std::chrono::steady_clock::now();
    const int32_t nx = (int32_t)b->dims[0], ny = (int32_t)b->dims[1], nz = (int32_t)b->dims[2];
    const float *src = b->orig;
    if (deconv) {  // the estimate lives where an even number of passes after it ends in ptr
      float *u = np % 2 ? scratch : b->ptr;
      run_deconvolution(b->orig, u, np % 2 ? b->ptr : scratch, scratch2, nx, ny, nz, daxis, dR, nda, h->d_deconv_w,
                        h->deconv_iterations, h->deconv_floor, np ? nullptr : U.d_stats, U.pad_stream);
      src = u;
    }
    for (int i = 0; i < np; ++i) {
      float *dst = (np - 1 - i) % 2 ? scratch : b->ptr;  // the last pass writes ptr
      vr::BufStats *st = i == np - 1 ? U.d_stats : nullptr;
      if (pass[i].axis == 4)
        VR_HIP(vr::launch_smooth_fused(src, dst, nx, ny, nz, h->d_smooth_w, radius[0], radius[1], radius[2], st,
                                       U.pad_stream));
      else if (pass[i].axis == 3)
        VR_HIP(vr::launch_label_gain(src, h->d_labels, h->d_gains, h->ngains, nx, ny, nz, dst, st, U.pad_stream));
      else
        VR_HIP(vr::launch_smooth_axis(src, dst, nx, ny, nz, pass[i].axis,
                                      h->d_smooth_w + pass[i].axis * VR_SMOOTH_MAX_TAPS, pass[i].R, st, U.pad_stream));
      src = dst;
    }
    VR_HIP(hipMemcpyAsync(U.h_stats, U.d_stats, sizeof(vr::BufStats), hipMemcpyDeviceToHost, U.pad_stream));
    VR_HIP(hipStreamSynchronize(U.pad_stream));
    if (scratch) vr_host::pooled_free(scratch, b->bytes, b->device, vr_host::Readers());
    if (scratch2) vr_host::pooled_free(scratch2, b->bytes, b->device, vr_host::Readers());
    scratch = scratch2 = nullptr;
    b->nonfinite = U.h_stats->nonfinite != 0;
    b->maxabs = U.h_stats->maxabs;
    b->version = next_version();
    const auto t1 = std::chrono::steady_clock::now();
    build_occupancy(b.get(), U.pad_stream);
    const auto t2 = std::chrono::steady_clock::now();
    h->derive_ms[0] = std::chrono::duration<double, std::milli>(t1 - t0).count();
    h->derive_ms[1] = std::chrono::duration<double, std::milli>(t2 - t1).count();
  } catch (...) {  // the buffer must not stay half written: back to the unmodified upload
    (void)hipStreamSynchronize(U.pad_stream);
    if (scratch) vr_host::pooled_free(scratch, b->bytes, b->device, vr_host::Readers());
    if (scratch2) vr_host::pooled_free(scratch2, b->bytes, b->device, vr_host::Readers());
    vr_host::pooled_free(b->ptr, b->bytes, b->device, vr_host::Readers());
    b->ptr = b->orig;
    b->orig = nullptr;
    b->nonfinite = b->orig_nonfinite;
    b->maxabs = b->orig_maxabs;
    b->version = next_version();
    throw;
  }
  b->mod_labels = kl;
  b->mod_gains = kg;
  b->mod_smooth = ks;
  b->mod_deconv = kd;
  return bad;
}

void free_labels(vr_context *h) {
  h->labels_readers.wait();
  if (h->d_labels) (void)hipFree(h->d_labels);
  h->d_labels = nullptr;
  h->labels_bytes = 0;
  h->labels_src = nullptr;
  h->labels_last_update = 0;
  for (uint64_t &d : h->labels_dims) d = 0;
}

int labels_unsupported(const char *what) {
  return fail(VR_ERR_UNSUPPORTED, std::string(what) + ": labels and label gains are not supported on a multi-device "
                                                      "group handle");
}

int check_label_gains(const float *gains, int32_t n) {
  if (n < 0 || n > VR_LABEL_GAINS_MAX) return fail(VR_ERR_ARGUMENT, "label gains: n must be in 0..256");
  if (n > 0 && !gains) return fail(VR_ERR_ARGUMENT, "label gains: gains is NULL");
  for (int32_t i = 0; i < n; ++i)
    if (!std::isfinite(gains[i])) return fail(VR_ERR_ARGUMENT, "label gains: every gain must be finite");
  return VR_OK;
}

int do_sync_volumes(vr_context *h, uint64_t time_last_mem_sync, const vr_volume *emission,
                    const vr_volume *reflection, const vr_volume *absorption, const vr_volume *dx,
                    const vr_volume *dy, const vr_volume *dz) {
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  if (!emission || !reflection || !absorption) return fail(VR_ERR_ARGUMENT, "insufficient parameter!");
  // render.cpp:105-113 keys on the argument count: 9 takes the gradient volumes (lookup), 6 resets
  // them, 7 or 8 (dx or dx, dy given, the rest NULL) keeps the handle's previous gradient volumes
  // without reading the given ones; setGradientMethod(compute) then MManager::sync re-enters lookup
  // mode if kept gradient volumes exist (mmanager.hxx:193-200).
  const int given = (dx != nullptr) + (dy != nullptr) + (dz != nullptr);
  const bool lookup = given == 3;
  if (!lookup && given && !(dx && (dy || !dz)))
    return fail(VR_ERR_ARGUMENT, "sync_volumes: gradient volumes must be given in order (dx, dy, dz)");
  for (const vr_volume *v : {emission, reflection, absorption, lookup ? dx : nullptr, lookup ? dy : nullptr,
                             lookup ? dz : nullptr}) {
    if (!v) continue;
    const bool grad = v == dx || v == dy || v == dz;
    if (int rc = check_dtype(v, grad, grad ? "gradient volume" : "volume")) return rc;
    const uint64_t n = v->dims[0] * v->dims[1] * v->dims[2];
    if (n && !v->data) return fail(VR_ERR_ARGUMENT, "volume data is NULL");
    if (v->dims[0] > 0x7FFFFFFF || v->dims[1] > 0x7FFFFFFF || v->dims[2] > 0x7FFFFFFF)
      return fail(VR_ERR_UNSUPPORTED, "volume dimension too large");
  }
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();  // buffers whose last launch has completed
  uint64_t required = required_memory(h);  // render.cpp:90 (before the new volumes are recorded)
  h->time_last_mem_sync = time_last_mem_sync;
  h->vol[T_EM] = make_rec(emission);
  h->vol[T_RE] = make_rec(reflection);
  h->vol[T_AB] = make_rec(absorption);
  if (lookup) {
    h->vol[T_DX] = make_rec(dx);
    h->vol[T_DY] = make_rec(dy);
    h->vol[T_DZ] = make_rec(dz);
  } else if (given == 0) {
    reset_gradients(h);
  }
  required += required_memory(h);
  int rc = check_free_device_memory(required);
  if (rc) return rc;
  g_tex.grad_method = lookup ? G_LOOKUP : G_COMPUTE;  // setGradientMethod (render.cpp:121)
  mm_sync(h);  // returns with the volumes resident (vr_host::Uploader); renders in flight keep running
  for (int t = 0; t < T_COUNT; ++t) h->snap_bind[t] = g_tex.bind[t];
  h->snap_idx[0] = g_tex.idx_em;
  h->snap_idx[1] = g_tex.idx_ab;
  h->snap_idx[2] = g_tex.idx_re;
  h->snap_grad = g_tex.grad_method;
  h->has_snap = true;
  return apply_derived(h);  // smoothing, label gains: the freshly bound emission buffer follows the handle's state
  VR_GUARD_END
}

}  // namespace vr_host
