// vr_capi.hip -- the C-ABI of libvrhip.so (declared in include/vrhip.h): the extern "C" entries, each
// its lock, its argument checks and the call into the host driver (vr_host.h names the files), plus the
// host utilities that are themselves entries (HG LUT, resize, normalize, convert).
//
// Replaces, for the MI355X, the reference's mex command dispatcher (mex/render.cpp:50-278)
// (marshalling kept) and its handle (vr/mm/class_handle.hpp) (same handle
// contract: signature check).
// Every HIP call is checked (the reference ignores errors in release builds, common.h:43-47).
#include "vr_host.h"
#include "vr_transfer.h"

using namespace vr_host;

namespace {

void reset_tex_unit() {
  for (auto &b : g_tex.bind) b.reset();
  g_tex.gvec.clear();
  g_tex.idx_em = T_EM;
  g_tex.idx_ab = T_EM;
  g_tex.idx_re = T_RE;
  g_tex.grad_method = G_COMPUTE;
  g_tex.lights.clear();
}

// The handle's output buffer (the images and aux planes of the host-pointer renders), at least `bytes`.
void ensure_out(vr_context *h, size_t bytes) {
  if (bytes <= h->d_out_bytes) return;
  if (h->d_out) VR_HIP(hipFree(h->d_out));
  h->d_out = nullptr;
  h->d_out_bytes = 0;
  VR_HIP(hipMalloc(&h->d_out, bytes));
  h->d_out_bytes = bytes;
}

double mb(uint64_t b) { return (double)b / (1024.0 * 1024.0); }

// imresize's contributions along one axis (Volume.resize -> imresize3, Volume.m:93-106; MATLAB's
// default: cubic kernel of width 4, antialiasing when shrinking): per output index o (1-based x),
// u = x/scale + (1 - 1/scale)/2, the P = ceil(width) + 2 taps from floor(u - width/2), weights
// h(u - index) normalised by their row sum, indices mirrored at the ends ([1..n, n..1]), columns
// that are zero for every output removed.  Double precision throughout; 0-based indices out.
double cubic(double x) {
  const double ax = std::fabs(x), ax2 = ax * ax, ax3 = ax * ax * ax;
  return (1.5 * ax3 - 2.5 * ax2 + 1.0) * (ax <= 1.0 ? 1.0 : 0.0) +
         (-0.5 * ax3 + 2.5 * ax2 - 4.0 * ax + 2.0) * ((1.0 < ax && ax <= 2.0) ? 1.0 : 0.0);
}
void resize_contributions(uint64_t in_len, uint64_t out_len, std::vector<double> &w, std::vector<int32_t> &idx,
                          int32_t &P) {
  const double scale = (double)out_len / (double)in_len;
  const bool aa = scale < 1.0;
  const double width = aa ? 4.0 / scale : 4.0;
  const int32_t P0 = (int32_t)std::ceil(width) + 2;
  std::vector<double> w0((size_t)out_len * P0);
  std::vector<int64_t> i0((size_t)out_len * P0);
  for (uint64_t o = 0; o < out_len; ++o) {
    const double x = (double)(o + 1);
    const double u = x / scale + 0.5 * (1.0 - 1.0 / scale);
    const double left = std::floor(u - width / 2.0);
    double sum = 0.0;
    for (int32_t p = 0; p < P0; ++p) {
      const double ind = left + p;
      const double d = u - ind;
      const double h = aa ? scale * cubic(scale * d) : cubic(d);
      w0[o * P0 + p] = h;
      i0[o * P0 + p] = (int64_t)ind;
      sum = sum + h;
    }
    for (int32_t p = 0; p < P0; ++p) w0[o * P0 + p] = w0[o * P0 + p] / sum;
  }
  // mirror: aux = [1:n, n:-1:1], index -> aux(mod(index - 1, 2n) + 1)
  const int64_t n = (int64_t)in_len, m = 2 * n;
  for (auto &i : i0) {
    int64_t k = (i - 1) % m;
    if (k < 0) k += m;
    i = k < n ? k : (m - 1 - k);  // 0-based
  }
  std::vector<char> keep(P0, 0);
  for (uint64_t o = 0; o < out_len; ++o)
    for (int32_t p = 0; p < P0; ++p)
      if (w0[o * P0 + p] != 0.0) keep[p] = 1;
  P = 0;
  for (int32_t p = 0; p < P0; ++p) P += keep[p];
  w.assign((size_t)out_len * P, 0.0);
  idx.assign((size_t)out_len * P, 0);
  for (uint64_t o = 0; o < out_len; ++o) {
    int32_t q = 0;
    for (int32_t p = 0; p < P0; ++p) {
      if (!keep[p]) continue;
      w[o * P + q] = w0[o * P0 + p];
      idx[o * P + q] = (int32_t)i0[o * P0 + p];
      ++q;
    }
  }
}

// vr_convert_host: the upload's conversion (vr_convert.h) over a host array
template <class T, bool UNORM>
void convert_host(const void *src, uint64_t n, float *dst) {
  const T *s = static_cast<const T *>(src);
  for (uint64_t i = 0; i < n; ++i) dst[i] = vr::to_f32<UNORM>(s[i]);
}

}  // namespace

extern "C" {

int vr_new(vr_context **out) {
  if (!out) return fail(VR_ERR_ARGUMENT, "New: One output expected.");
  std::lock_guard<std::mutex> lk(g_mu);
  VR_GUARD_BEGIN
  int dev = 0;
  VR_HIP(hipGetDevice(&dev));
  vr_context *h = new vr_context();
  h->device = dev;
  g_contexts.insert(h);
  *out = h;
  g_last_error.clear();
  return VR_OK;
  VR_GUARD_END
}

int vr_new_multi(const int32_t *devices, int32_t n, vr_context **out) {
  if (!out) return fail(VR_ERR_ARGUMENT, "New: One output expected.");
  if (!devices || n < 1) return fail(VR_ERR_ARGUMENT, "no devices");
  std::lock_guard<std::mutex> lk(g_mu);
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return fail(VR_ERR_DEVICE, "no HIP device");
  for (int i = 0; i < n; ++i)
    if (devices[i] < 0 || devices[i] >= count) return fail(VR_ERR_ARGUMENT, "invalid device index");
  VR_GUARD_BEGIN
  DeviceGuard dg(devices[0]);
  vr_context *h = new vr_context();
  h->device = devices[0];
  VR_HIP(hipEventCreateWithFlags(&h->gdone, hipEventDisableTiming));
  // VR_GROUP_PEER=0 (test switch): every child as if without a peer mapping (host-staged copies)
  const bool no_peer = env_flag_off("VR_GROUP_PEER");
  for (int i = 1; i < n; ++i) {
    const bool peer = enable_peer(devices[0], devices[i]) && enable_peer(devices[i], devices[0]) && !no_peer;
    DeviceGuard dk(devices[i]);
    vr_context *c = new vr_context();
    c->device = devices[i];
    c->peer = peer;
    c->parent = h;
    h->children.push_back(c);
    VR_HIP(take_stream(c->device, &c->gstream));
    VR_HIP(hipEventCreateWithFlags(&c->gdone, hipEventDisableTiming));
  }
  g_contexts.insert(h);
  *out = h;
  g_last_error.clear();
  return VR_OK;
  VR_GUARD_END
}

int vr_delete(vr_context *h) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  VR_GUARD_BEGIN
  // ~MManager -> cudaDeviceReset(): every handle's device memory and the module globals go.
  reset_tex_unit();
  for (vr_context *c : g_contexts) {
    for (vr_context *k : c->children)  // a group's children: their buffers go with the device reset
      for (auto &b : k->buf) b.reset();
    for (auto &b : c->buf) b.reset();
    if (c->d_out) (void)hipFree(c->d_out);
    c->d_out = nullptr;
    c->d_out_bytes = 0;
    free_schedules(c);
    free_views(c);
  }
  delete_children(h);
  if (h->gdone) (void)hipEventDestroy(h->gdone);
  for (hipEvent_t e : h->tev)
    if (e) (void)hipEventDestroy(e);
  if (h->d_part) (void)hipFree(h->d_part);
  {  // the handle's label bytes and gain table (the unmodified copies went with the buffers above)
    DeviceGuard dl(h->device);
    free_labels(h);
    if (h->d_gains) (void)hipFree(h->d_gains);
    h->d_gains = nullptr;
    if (h->d_smooth_w) (void)hipFree(h->d_smooth_w);
    h->d_smooth_w = nullptr;
    if (h->d_deconv_w) (void)hipFree(h->d_deconv_w);
    h->d_deconv_w = nullptr;
  }
  g_contexts.erase(h);
  h->signature = 0;
  delete h;
  // cudaDeviceReset waits for and drops everything: so do the retired buffers here
  (void)hipDeviceSynchronize();
  vr_host::prune_retired(true);
  vr_host::pool_clear();
  return VR_OK;
  VR_GUARD_END
}

int vr_mem_info(vr_context *h, char *buf, size_t buflen) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();  // buffers whose last launch has completed
  size_t free_b = 0, total_b = 0;
  VR_HIP(hipMemGetInfo(&free_b, &total_b));
  const VolRec &em = h->vol[T_EM], &ab = h->vol[T_AB], &re = h->vol[T_RE];
  auto ptr = [&](int s) { return (const void *)(h->buf[s] ? h->buf[s]->ptr : nullptr); };
  std::ostringstream os;
  os << "Memory Information\n"
     << "------------------------------" << "last sync (timestamp): " << h->time_last_mem_sync << "\n\n"
     << "\tGPU\n\t---\n"
     << "\t\tTotal Memory (MB): \t" << mb(total_b) << "\n"
     << "\t\tFree Memory (MB): \t" << mb(free_b) << "\n"
     << "\t\tUsed Memory (MB): \t" << mb(total_b - free_b) << "\n\n"
     << "\t\tVolumes\n\t\t-------\n"
     << "\t\tEmission (MB): " << mb(em.memory_size) << " ptr: " << ptr(T_EM) << "\n"
     << "\t\tAbsorption (MB): " << mb(ab.memory_size) << " ptr: " << ptr(T_AB) << "\n"
     << "\t\tReflection (MB): " << mb(re.memory_size) << " ptr: " << ptr(T_RE) << "\n"
     << "\t\tdX (MB): " << mb(h->vol[T_DX].memory_size) << " ptr: " << ptr(T_DX) << "\n"
     << "\t\tdY (MB): " << mb(h->vol[T_DY].memory_size) << " ptr: " << ptr(T_DY) << "\n"
     << "\t\tdZ (MB): " << mb(h->vol[T_DZ].memory_size) << " ptr: " << ptr(T_DZ) << "\n"
     << "\t\tlight (MB): " << mb(h->vol[T_LIGHT].memory_size) << " ptr: " << ptr(T_LIGHT) << "\n"
     << "\t\tlabels (MB): " << mb(h->labels_bytes) << " ptr: " << (const void *)h->d_labels
     << ", label gains: " << h->ngains << ", unmodified emission copy (MB): "
     << mb(label_target(h) && label_target(h)->orig ? label_target(h)->bytes : 0) << "\n";
  if (smoothing_set(h))  // (only while one is set: without, the report is what it was)
    os << "\t\tsmoothing sigma (voxels): " << h->smooth_sigma[0] << " " << h->smooth_sigma[1] << " "
       << h->smooth_sigma[2] << ", derived from the unmodified emission copy above\n";
  if (deconvolution_set(h))
    os << "\t\tdeconvolution sigma (voxels): " << h->deconv_sigma[0] << " " << h->deconv_sigma[1] << " "
       << h->deconv_sigma[2] << ", iterations: " << h->deconv_iterations << ", floor: " << h->deconv_floor
       << ", derived from the unmodified emission copy above\n";
  os << "\t\treusable buffers (MB): " << mb(vr_host::pool_bytes(h->device)) << "\n\n"
     << "\t\tSimilarity of Volumes\n\t\t---------------------\n"
     << "\t\t\tEm\tAb\tRe\n"
     << "\t\tEm\t1\t\n"
     << "\t\tAb\t" << same(em, ab) << "\t1\n"
     << "\t\tRe\t" << same(em, re) << "\t" << same(ab, re) << "\t1\n\n"
     << "\t\tSlots (emission/absorption/reflection): " << g_tex.idx_em << " " << g_tex.idx_ab << " "
     << g_tex.idx_re << ", gradient method: " << (g_tex.grad_method == G_LOOKUP ? "lookup" : "compute")
     << ", lights: " << g_tex.lights.size() << "\n";
  // per-device residency and the last launch's kernel time (SURVEY.md s5 "Metrics"): the primary
  // and, for a group (vr_new_multi), every child with the replicas of the bound volumes it holds
  os << "\n\tDevices\n\t-------\n";
  static const char *const tex_names[T_COUNT] = {"Emission", "Absorption", "Reflection", "dX", "dY", "dZ", "light"};
  std::vector<vr_context *> ctxs{h};
  ctxs.insert(ctxs.end(), h->children.begin(), h->children.end());
  for (size_t k = 0; k < ctxs.size(); ++k) {
    vr_context *c = ctxs[k];
    DeviceGuard dk(c->device);
    size_t fb = 0, tb = 0;
    VR_HIP(hipMemGetInfo(&fb, &tb));
    os << "\t\tdevice " << c->device << (k == 0 ? " (primary)" : " (group member)") << ": used (MB) "
       << mb(tb - fb) << " of " << mb(tb) << ", part buffer (MB) " << mb(c->d_part_bytes)
       << ", reusable buffers (MB) " << mb(vr_host::pool_bytes(c->device)) << "\n";
    for (int t = 0; t < T_COUNT; ++t) {
      const BufPtr &b = g_tex.bind[t];
      if (!b) continue;
      const DevBuf *r = nullptr;
      if (k == 0) {
        r = b.get();
      } else if (t == T_LIGHT) {
        r = c->buf[T_LIGHT].get();
      } else {
        auto it = b->replicas.find(c->device);
        if (b->device == c->device && it == b->replicas.end()) r = b.get();
        else if (it != b->replicas.end() && b->replica_of[c->device] == b->version) r = it->second.get();
      }
      os << "\t\t\t" << tex_names[t] << ": ";
      if (r) os << mb(r->bytes) << " MB resident at " << (const void *)r->ptr << (k && t != T_LIGHT ? " (replica)" : "") << "\n";
      else os << "not resident (replicated at the next render)\n";
    }
    float ms = -1.f;
    bool have = c->timed && vr_host::query_done(c->tev[1], "hipEventQuery (mem_info launch timing)");
    if (have) {
      const hipError_t e = hipEventElapsedTime(&ms, c->tev[0], c->tev[1]);
      if (e != hipSuccess) vr_host::consume(e, "hipEventElapsedTime (mem_info launch timing)");
      have = e == hipSuccess;
    }
    if (have)
      os << "\t\t\tlast launch (ms): " << ms << "\n";
    else
      os << "\t\t\tlast launch (ms): n/a\n";
  }
  const std::string s = os.str();
  if (buf && buflen) {
    const size_t n = std::min(buflen - 1, s.size());
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return VR_OK;
  VR_GUARD_END
}

int vr_sync_volumes(vr_context *h, uint64_t time_last_mem_sync, const vr_volume *emission,
                    const vr_volume *reflection, const vr_volume *absorption, const vr_volume *dx,
                    const vr_volume *dy, const vr_volume *dz) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int rc = do_sync_volumes(h, time_last_mem_sync, emission, reflection, absorption, dx, dy, dz);
  if (rc || h->children.empty()) return rc;
  VR_GUARD_BEGIN
  group_sync(h);
  return VR_OK;
  VR_GUARD_END
}

int vr_render_channels_device(const vr_channel *ch, int32_t n, int32_t stereo, float base, float *d_out,
                              void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!ch || n < 1 || !valid(ch[0].handle)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  VR_GUARD_BEGIN
  DeviceGuard dg(ch[0].handle->device);
  vr_host::prune_retired();  // buffers whose last launch has completed
  return do_render_channels(ch, n, stereo, base, d_out, (hipStream_t)stream);
  VR_GUARD_END
}

int vr_render_channels(const vr_channel *ch, int32_t n, int32_t stereo, float base, float *out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!ch || n < 1 || !valid(ch[0].handle)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  if (!ch[0].args) return fail(VR_ERR_ARGUMENT, "insufficient parameter!");
  VR_GUARD_BEGIN
  vr_context *h = ch[0].handle;
  DeviceGuard dg(h->device);
  vr_host::prune_retired();  // buffers whose last launch has completed
  const size_t img = (size_t)ch[0].args->resolution[0] * (size_t)ch[0].args->resolution[1] * 3;
  if (img && !out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  const size_t bytes = img * sizeof(float) * (size_t)n * (stereo ? 2 : 1);
  if (bytes > h->d_chan_bytes) {
    if (h->d_chan) VR_HIP(hipFree(h->d_chan));
    h->d_chan = nullptr;
    h->d_chan_bytes = 0;
    VR_HIP(hipMalloc(&h->d_chan, bytes));
    h->d_chan_bytes = bytes;
  }
  int rc = do_render_channels(ch, n, stereo, base, h->d_chan, nullptr);
  if (rc) return rc;
  if (bytes) VR_HIP(hipMemcpy(out, h->d_chan, bytes, hipMemcpyDeviceToHost));
  return VR_OK;
  VR_GUARD_END
}

int vr_sum_channels_device(const float *d_in, int32_t n, int32_t views, uint64_t image_floats, float *d_out,
                           void *stream) {
  if (!d_in || !d_out || n < 1 || views < 1) return fail(VR_ERR_ARGUMENT, "invalid channel sum");
  VR_GUARD_BEGIN
  VR_HIP(vr::launch_sum_channels(d_in, (uint32_t)n, (uint32_t)views, image_floats, d_out, (hipStream_t)stream));
  return VR_OK;
  VR_GUARD_END
}

int vr_render(vr_context *h, const vr_render_args *a, float *out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  if (!a) return fail(VR_ERR_ARGUMENT, "insufficient parameter!");
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();  // buffers whose last launch has completed
  const size_t bytes = (size_t)a->resolution[0] * (size_t)a->resolution[1] * 3 * sizeof(float);
  if (bytes && !out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  ensure_out(h, bytes);
  if (!h->children.empty() && h->nclip) return clip_unsupported("vr_render on a multi-device group handle");
  Frame F;
  int rc = h->children.empty() ? do_render(h, a, nullptr, h->d_out, nullptr, nullptr, F)
                               : group_render(h, a, h->d_out, nullptr);
  if (rc) return rc;
  if (bytes) VR_HIP(hipMemcpy(out, h->d_out, bytes, hipMemcpyDeviceToHost));
  return VR_OK;
  VR_GUARD_END
}

int vr_render_stereo(vr_context *h, const vr_render_args *a, float base, float *out_left, float *out_right) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  if (!a) return fail(VR_ERR_ARGUMENT, "insufficient parameter!");
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();  // buffers whose last launch has completed
  const size_t bytes = (size_t)a->resolution[0] * (size_t)a->resolution[1] * 3 * sizeof(float);
  if (bytes && (!out_left || !out_right)) return fail(VR_ERR_ARGUMENT, "output is NULL");
  if (!h->children.empty() && h->nclip) return clip_unsupported("vr_render_stereo on a multi-device group handle");
  ensure_out(h, 2 * bytes);
  // left eye: camera x offset -base (the frame's own eye); right eye: +base, formed as build_frame
  // forms it (fma(-dist, Z, xoff * X), render.cpp:211-221 column order)
  vr_render_args al = *a;
  al.props[0] = -base;
  const float *r = a->rotation_flipped;
  const float X[3] = {r[2], r[1], r[0]}, Z[3] = {r[8], r[7], r[6]};
  const float dist = a->props[2];
  float eye2[3];
  for (int i = 0; i < 3; ++i) eye2[i] = fmaf(-dist, Z[i], base * X[i]);
  Frame F;
  float *d_left = h->d_out, *d_right = h->d_out + bytes / sizeof(float);
  int rc = h->children.empty() ? do_render(h, &al, nullptr, d_left, nullptr, nullptr, F, d_right, eye2)
                               : group_render(h, &al, d_left, nullptr, d_right, eye2);  // every device
  if (rc) return rc;
  if (bytes) {
    VR_HIP(hipMemcpy(out_left, d_left, bytes, hipMemcpyDeviceToHost));
    VR_HIP(hipMemcpy(out_right, d_right, bytes, hipMemcpyDeviceToHost));
  }
  return VR_OK;
  VR_GUARD_END
}

int vr_render_stereo_device(vr_context *h, const vr_render_args *a, float base, float *d_left, float *d_right,
                            unsigned long long *d_steps, void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  VR_ENTRY_BEGIN(h, a)
  if ((size_t)a->resolution[0] * (size_t)a->resolution[1] && (!d_left || !d_right))
    return fail(VR_ERR_ARGUMENT, "output is NULL");
  vr_render_args al = *a;  // as vr_render_stereo: left = -base (the frame's eye), right = +base
  al.props[0] = -base;
  const float *r = a->rotation_flipped;
  const float X[3] = {r[2], r[1], r[0]}, Z[3] = {r[8], r[7], r[6]};
  float eye2[3];
  for (int i = 0; i < 3; ++i) eye2[i] = fmaf(-a->props[2], Z[i], base * X[i]);
  Frame F;
  return do_render(h, &al, nullptr, d_left, d_steps, (hipStream_t)stream, F, d_right, eye2);
  VR_GUARD_END
}

int vr_render_device(vr_context *h, const vr_render_args *a, const vr_partition *part, float *d_out,
                     unsigned long long *d_steps, void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  if (!a) return fail(VR_ERR_ARGUMENT, "insufficient parameter!");
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();  // buffers whose last launch has completed
  if (!h->children.empty() && h->nclip) return clip_unsupported("vr_render_device on a multi-device group handle");
  if (!h->children.empty() && !part && !d_steps) return group_render(h, a, d_out, (hipStream_t)stream);
  Frame F;
  return do_render(h, a, part, d_out, d_steps, (hipStream_t)stream, F);
  VR_GUARD_END
}

int vr_render_projection_device(vr_context *h, const vr_render_args *a, int32_t mode, const vr_partition *part,
                                float *d_out, float *d_aux, unsigned long long *d_steps, void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (mode != VR_PROJ_MIP && mode != VR_PROJ_SUM) return fail(VR_ERR_ARGUMENT, "unknown projection mode");
  VR_ENTRY_BEGIN(h, a)
  return do_project(h, a, mode, part, d_out, d_aux, d_steps, (hipStream_t)stream);
  VR_GUARD_END
}

int vr_render_projection(vr_context *h, const vr_render_args *a, int32_t mode, float *out, float *out_aux) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (mode != VR_PROJ_MIP && mode != VR_PROJ_SUM) return fail(VR_ERR_ARGUMENT, "unknown projection mode");
  VR_ENTRY_BEGIN(h, a)
  // the image and, behind it, the aux plane in the handle's output buffer
  const size_t plane = (size_t)a->resolution[0] * (size_t)a->resolution[1] * sizeof(float);
  const size_t bytes = 4 * plane;
  if (plane && !out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  ensure_out(h, bytes);
  float *d_aux = out_aux ? h->d_out + 3 * (plane / sizeof(float)) : nullptr;
  const int rc = do_project(h, a, mode, nullptr, h->d_out, d_aux, nullptr, nullptr);
  if (rc) return rc;
  if (plane) VR_HIP(hipMemcpy(out, h->d_out, 3 * plane, hipMemcpyDeviceToHost));
  if (plane && out_aux) VR_HIP(hipMemcpy(out_aux, d_aux, plane, hipMemcpyDeviceToHost));
  return VR_OK;
  VR_GUARD_END
}

int vr_render_slice_device(vr_context *h, const vr_slice *s, float *d_out, float *d_aux, float *d_labels,
                           void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_slice(s)) return rc;
  VR_ENTRY_BEGIN(h, s)
  return do_slice(h, s, d_out, d_aux, d_labels, (hipStream_t)stream);
  VR_GUARD_END
}

int vr_render_slice(vr_context *h, const vr_slice *s, float *out, float *out_aux, float *out_labels) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_slice(s)) return rc;
  VR_ENTRY_BEGIN(h, s)
  // up to three planes in the handle's output buffer: the image, aux, labels
  const size_t count = (size_t)s->resolution[0] * (size_t)s->resolution[1];
  const size_t plane = count * sizeof(float);
  const size_t bytes = 3 * plane;
  if (plane && !out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  ensure_out(h, bytes);
  float *d_aux = out_aux ? h->d_out + count : nullptr;
  float *d_lab = out_labels ? h->d_out + 2 * count : nullptr;
  const int rc = do_slice(h, s, h->d_out, d_aux, d_lab, nullptr);
  if (rc) return rc;
  if (plane) VR_HIP(hipMemcpy(out, h->d_out, plane, hipMemcpyDeviceToHost));
  if (plane && out_aux) VR_HIP(hipMemcpy(out_aux, d_aux, plane, hipMemcpyDeviceToHost));
  if (plane && out_labels) VR_HIP(hipMemcpy(out_labels, d_lab, plane, hipMemcpyDeviceToHost));
  return VR_OK;
  VR_GUARD_END
}

int vr_volume_histogram_device(vr_context *h, const vr_histogram *q, unsigned long long *d_counts, vr_hist_row *d_rows,
                               void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_histogram(q)) return rc;
  if (!d_counts) return fail(VR_ERR_ARGUMENT, "histogram: counts is NULL");
  VR_ENTRY_BEGIN(h, q)
  return do_histogram(h, q, d_counts, d_rows, (hipStream_t)stream);
  VR_GUARD_END
}

int vr_volume_histogram(vr_context *h, const vr_histogram *q, uint64_t *counts, vr_hist_row *rows_out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_histogram(q)) return rc;
  if (!counts) return fail(VR_ERR_ARGUMENT, "histogram: counts is NULL");
  VR_ENTRY_BEGIN(h, q)
  // the counts and, behind them, the rows in the handle's output buffer
  const size_t rows = (size_t)histogram_rows(q);
  const size_t cbytes = rows * (size_t)q->nbins * sizeof(unsigned long long);
  ensure_out(h, cbytes + rows * sizeof(vr_hist_row));
  unsigned long long *d_counts = reinterpret_cast<unsigned long long *>(h->d_out);
  vr_hist_row *d_rows = rows_out ? reinterpret_cast<vr_hist_row *>(reinterpret_cast<char *>(h->d_out) + cbytes) : nullptr;
  const int rc = do_histogram(h, q, d_counts, d_rows, nullptr);
  if (rc) return rc;
  VR_HIP(hipMemcpy(counts, d_counts, cbytes, hipMemcpyDeviceToHost));
  if (rows_out) VR_HIP(hipMemcpy(rows_out, d_rows, rows * sizeof(vr_hist_row), hipMemcpyDeviceToHost));
  return VR_OK;
  VR_GUARD_END
}

int vr_histogram_bin_host(const float *v, uint64_t m, int32_t nbins, const float lim[2], int32_t *bin) {
  if (m && (!v || !bin)) return fail(VR_ERR_ARGUMENT, "histogram: v / bin is NULL");
  if (!lim) return fail(VR_ERR_ARGUMENT, "histogram: lim is NULL");
  if (int rc = check_hist_bins(nbins, lim)) return rc;
  const float inv = 1.0f / (lim[1] - lim[0]);
  for (uint64_t i = 0; i < m; ++i) bin[i] = vr_hist_bin(v[i], lim[0], lim[1], inv, nbins);
  return VR_OK;
}

static int check_slice_count(uint64_t thickness) {
  if (thickness < 1 || thickness > VR_SLICE_MAX_SAMPLES)
    return fail(VR_ERR_ARGUMENT, "slice: thickness must be 1 .. " + std::to_string(VR_SLICE_MAX_SAMPLES));
  return VR_OK;
}

int vr_slice_axis(const uint64_t dims[3], int32_t axis, double index, uint64_t thickness, vr_slice *out) {
  if (!dims || !out) return fail(VR_ERR_ARGUMENT, "slice: dims / out is NULL");
  if (!dims[0] || !dims[1] || !dims[2]) return fail(VR_ERR_ARGUMENT, "slice: empty volume");
  if (axis < 0 || axis > 2) return fail(VR_ERR_ARGUMENT, "slice: axis must be 0, 1 or 2");
  if (!std::isfinite(index)) return fail(VR_ERR_ARGUMENT, "slice: non-finite index");
  if (int rc = check_slice_count(thickness)) return rc;
  const int a = axis == 0 ? 1 : 0, b = axis == 2 ? 1 : 2;  // rows along a, columns along b, a < b
  if (dims[a] > 0x7FFFFFFFull || dims[b] > 0x7FFFFFFFull || dims[a] * dims[b] >= (1ull << 31))
    return fail(VR_ERR_ARGUMENT, "slice: image resolution too large (H * W must be below 2^31)");
  for (int j = 0; j < 3; ++j) out->origin[j] = out->du[j] = out->dv[j] = out->dw[j] = 0.f;
  const double first = index - (double)(thickness - 1) / 2.0;  // voxel index of slab sample 0
  out->origin[axis] = (float)((first + 0.5) / (double)dims[axis]);
  out->dw[axis] = (float)(1.0 / (double)dims[axis]);
  out->origin[a] = (float)(0.5 / (double)dims[a]);
  out->dv[a] = (float)(1.0 / (double)dims[a]);
  out->origin[b] = (float)(0.5 / (double)dims[b]);
  out->du[b] = (float)(1.0 / (double)dims[b]);
  out->resolution[0] = dims[a];
  out->resolution[1] = dims[b];
  out->samples = (int32_t)thickness;
  return VR_OK;
}

int vr_slice_oblique(const uint64_t dims[3], const float element_size_um[3], const double point_q[3],
                     const double normal_um[3], const double up_um[3], double pixel_um, uint64_t H, uint64_t W,
                     uint64_t thickness, vr_slice *out) {
  if (!dims || !element_size_um || !point_q || !normal_um || !up_um || !out)
    return fail(VR_ERR_ARGUMENT, "slice: a pointer is NULL");
  if (!dims[0] || !dims[1] || !dims[2]) return fail(VR_ERR_ARGUMENT, "slice: empty volume");
  if (int rc = check_slice_count(thickness)) return rc;
  if (H > 0x7FFFFFFFull || W > 0x7FFFFFFFull || H * W >= (1ull << 31))
    return fail(VR_ERR_ARGUMENT, "slice: image resolution too large (H * W must be below 2^31)");
  if (!std::isfinite(pixel_um) || !(pixel_um > 0.0)) return fail(VR_ERR_ARGUMENT, "slice: pixel size must be positive");
  double ext[3];  // physical extent of the volume along dims[j]: q_j * ext[j] is a position in um
  for (int j = 0; j < 3; ++j) {
    const double es = (double)element_size_um[2 - j];
    if (!std::isfinite(es) || !(es > 0.0)) return fail(VR_ERR_ARGUMENT, "slice: element size must be positive");
    if (!std::isfinite(point_q[j]) || !std::isfinite(normal_um[j]) || !std::isfinite(up_um[j]))
      return fail(VR_ERR_ARGUMENT, "slice: non-finite point / normal / up");
    ext[j] = (double)dims[j] * es;
  }
  auto dot = [](const double *p, const double *q) { return p[0] * q[0] + p[1] * q[1] + p[2] * q[2]; };
  // scale the directions by their largest component first: no overflow or underflow in the squares
  double w[3], v[3], u[3];
  double nmax = 0, umax = 0;
  for (int j = 0; j < 3; ++j) {
    nmax = std::max(nmax, std::fabs(normal_um[j]));
    umax = std::max(umax, std::fabs(up_um[j]));
  }
  if (nmax == 0.0) return fail(VR_ERR_ARGUMENT, "slice: zero normal");
  if (umax == 0.0) return fail(VR_ERR_ARGUMENT, "slice: up is parallel to the normal");
  for (int j = 0; j < 3; ++j) {
    w[j] = normal_um[j] / nmax;
    v[j] = up_um[j] / umax;
  }
  const double wl = std::sqrt(dot(w, w));
  for (int j = 0; j < 3; ++j) w[j] /= wl;
  const double vl0 = std::sqrt(dot(v, v));
  for (int j = 0; j < 3; ++j) v[j] /= vl0;
  const double vw = dot(v, w);
  for (int j = 0; j < 3; ++j) v[j] -= vw * w[j];
  const double vl = std::sqrt(dot(v, v));
  if (!(vl > 1e-9)) return fail(VR_ERR_ARGUMENT, "slice: up is parallel to the normal");
  for (int j = 0; j < 3; ++j) v[j] /= vl;
  u[0] = v[1] * w[2] - v[2] * w[1];
  u[1] = v[2] * w[0] - v[0] * w[2];
  u[2] = v[0] * w[1] - v[1] * w[0];
  const double cy = ((double)H - 1.0) / 2.0, cx = ((double)W - 1.0) / 2.0, ck = ((double)thickness - 1.0) / 2.0;
  for (int j = 0; j < 3; ++j) {
    const double duq = u[j] * pixel_um / ext[j], dvq = v[j] * pixel_um / ext[j], dwq = w[j] * pixel_um / ext[j];
    out->du[j] = (float)duq;
    out->dv[j] = (float)dvq;
    out->dw[j] = (float)dwq;
    out->origin[j] = (float)(point_q[j] - cx * duq - cy * dvq - ck * dwq);
  }
  out->resolution[0] = H;
  out->resolution[1] = W;
  out->samples = (int32_t)thickness;
  return VR_OK;
}

int vr_render_isosurface_device(vr_context *h, const vr_render_args *a, float level, const vr_partition *part,
                                float *d_out, float *d_depth, float *d_normal, unsigned long long *d_steps,
                                void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (level != level) return fail(VR_ERR_ARGUMENT, "isosurface level is NaN");
  VR_ENTRY_BEGIN(h, a)
  return do_isosurface(h, a, level, part, d_out, d_depth, d_normal, d_steps, (hipStream_t)stream);
  VR_GUARD_END
}

int vr_render_isosurface(vr_context *h, const vr_render_args *a, float level, float *out, float *out_depth,
                         float *out_normal) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (level != level) return fail(VR_ERR_ARGUMENT, "isosurface level is NaN");
  VR_ENTRY_BEGIN(h, a)
  // the image and, behind it, the depth plane and the three normal planes in the handle's output buffer
  const size_t plane = (size_t)a->resolution[0] * (size_t)a->resolution[1] * sizeof(float);
  const size_t bytes = 7 * plane;
  if (plane && !out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  ensure_out(h, bytes);
  float *d_depth = out_depth ? h->d_out + 3 * (plane / sizeof(float)) : nullptr;
  float *d_normal = out_normal ? h->d_out + 4 * (plane / sizeof(float)) : nullptr;
  const int rc = do_isosurface(h, a, level, nullptr, h->d_out, d_depth, d_normal, nullptr, nullptr);
  if (rc) return rc;
  if (plane) VR_HIP(hipMemcpy(out, h->d_out, 3 * plane, hipMemcpyDeviceToHost));
  if (plane && out_depth) VR_HIP(hipMemcpy(out_depth, d_depth, plane, hipMemcpyDeviceToHost));
  if (plane && out_normal) VR_HIP(hipMemcpy(out_normal, d_normal, 3 * plane, hipMemcpyDeviceToHost));
  return VR_OK;
  VR_GUARD_END
}

int vr_render_transfer_device(vr_context *h, const vr_render_args *a, const vr_transfer *tf, const vr_partition *part,
                              float *d_out, float *d_alpha, unsigned long long *d_steps, void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_transfer(tf)) return rc;
  VR_ENTRY_BEGIN(h, a)
  return do_transfer(h, a, tf, part, d_out, d_alpha, d_steps, (hipStream_t)stream);
  VR_GUARD_END
}

int vr_render_transfer(vr_context *h, const vr_render_args *a, const vr_transfer *tf, float *out, float *out_alpha) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_transfer(tf)) return rc;
  VR_ENTRY_BEGIN(h, a)
  // the image and, behind it, the alpha plane in the handle's output buffer
  const size_t plane = (size_t)a->resolution[0] * (size_t)a->resolution[1] * sizeof(float);
  const size_t bytes = 4 * plane;
  if (plane && !out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  ensure_out(h, bytes);
  float *d_alpha = out_alpha ? h->d_out + 3 * (plane / sizeof(float)) : nullptr;
  const int rc = do_transfer(h, a, tf, nullptr, h->d_out, d_alpha, nullptr, nullptr);
  if (rc) return rc;
  if (plane) VR_HIP(hipMemcpy(out, h->d_out, 3 * plane, hipMemcpyDeviceToHost));
  if (plane && out_alpha) VR_HIP(hipMemcpy(out_alpha, d_alpha, plane, hipMemcpyDeviceToHost));
  return VR_OK;
  VR_GUARD_END
}

int vr_set_clip(vr_context *h, const vr_clip_plane *planes, int32_t n) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_clip(planes, n)) return rc;
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  for (int32_t i = 0; i < n; ++i) h->clip[i] = planes[i];
  h->nclip = n;
  return VR_OK;
}

int vr_get_clip(vr_context *h, vr_clip_plane *planes, int32_t *n) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!planes || !n) return fail(VR_ERR_ARGUMENT, "clip planes: planes / n is NULL");
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  for (int32_t i = 0; i < h->nclip; ++i) planes[i] = h->clip[i];
  *n = h->nclip;
  return VR_OK;
}

int vr_sync_labels(vr_context *h, const vr_volume *labels) {
  std::lock_guard<std::mutex> lk(g_mu);
  uint64_t count = 0;
  if (labels) {
    if (labels->dtype != VR_U8)
      return fail(VR_ERR_ARGUMENT, "labels: the label volume must be uint8 (VR_U8 without VR_DTYPE_UNORM)");
    if (labels->location != VR_HOST && labels->location != VR_DEVICE)
      return fail(VR_ERR_ARGUMENT, "labels: invalid location");
    if (labels->dims[0] > 0x7FFFFFFF || labels->dims[1] > 0x7FFFFFFF || labels->dims[2] > 0x7FFFFFFF)
      return fail(VR_ERR_UNSUPPORTED, "labels: volume dimension too large");
    count = labels->dims[0] * labels->dims[1] * labels->dims[2];
    if (count && !labels->data) return fail(VR_ERR_ARGUMENT, "labels: volume data is NULL");
  }
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  if (!h->children.empty()) return labels_unsupported("vr_sync_labels");
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();
  if (!count) {  // NULL (or an empty volume) drops them
    if (h->d_labels) h->labels_version = next_version();
    free_labels(h);
    return apply_derived(h);
  }
  const BufPtr b = label_target(h);
  if (h->ngains > 0)
    if (int rc = check_label_dims(labels->dims, b.get())) return rc;  // (the old labels stay)
  // the same Volume identity (data pointer, TimeLastUpdate, size) is not uploaded again, as the LUT's
  const bool same_volume = h->d_labels && h->labels_src == labels->data && h->labels_last_update == labels->last_update &&
                           h->labels_location == labels->location && labels->last_update != 0 &&
                           h->labels_dims[0] == labels->dims[0] && h->labels_dims[1] == labels->dims[1] &&
                           h->labels_dims[2] == labels->dims[2] && !env_flag("VR_ALWAYS_REUPLOAD");
  if (!same_volume) {
    if (h->labels_bytes != count) {
      const bool copy = h->ngains > 0 && b && b->ptr && !b->orig;
      if (int rc = check_free_device_memory(count + (copy ? b->bytes : 0))) return rc;
      free_labels(h);
      VR_HIP(vr_host::device_alloc(reinterpret_cast<void **>(&h->d_labels), count));
      h->labels_bytes = count;
    }
    h->labels_readers.wait();  // slices in flight that read the label bytes
    // (no label pass is in flight: apply_derived waits for its own.)  Device data is read after the work
    // already queued on the null stream, as the upload path reads a device volume.
    const bool dev = labels->location == VR_DEVICE;
    VR_HIP(hipMemcpy(h->d_labels, labels->data, count, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
    if (dev) VR_HIP(hipStreamSynchronize(nullptr));
    for (int i = 0; i < 3; ++i) h->labels_dims[i] = labels->dims[i];
    h->labels_src = labels->data;
    h->labels_last_update = labels->last_update;
    h->labels_location = labels->location;
    h->labels_version = next_version();
  }
  return apply_derived(h);
  VR_GUARD_END
}

int vr_set_label_gains(vr_context *h, const float *gains, int32_t n) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_label_gains(gains, n)) return rc;
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  if (n > 0 && !h->children.empty()) return labels_unsupported("vr_set_label_gains");
  if (n == h->ngains && (n == 0 || !std::memcmp(gains, h->gains, sizeof(float) * (size_t)n))) return VR_OK;  // no change
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();
  const BufPtr b = label_target(h);
  if (n > 0 && h->d_labels) {
    if (int rc = check_label_dims(h->labels_dims, b.get())) return rc;  // (the old table stays)
    if (b && b->ptr && !b->orig)
      if (int rc = check_free_device_memory(b->bytes)) return rc;
  }
  for (int32_t i = 0; i < n; ++i) h->gains[i] = gains[i];
  h->ngains = n;
  h->gains_version = next_version();
  return apply_derived(h);
  VR_GUARD_END
}

int vr_get_label_gains(vr_context *h, float *gains, int32_t *n) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!gains || !n) return fail(VR_ERR_ARGUMENT, "label gains: gains / n is NULL");
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  for (int32_t i = 0; i < h->ngains; ++i) gains[i] = h->gains[i];
  *n = h->ngains;
  return VR_OK;
}

int vr_label_gain_host(const float *src, const uint8_t *labels, const float *gains, int32_t n, uint64_t count,
                       float *dst) {
  if (int rc = check_label_gains(gains, n)) return rc;
  if (count && (!src || !dst || (n > 0 && !labels))) return fail(VR_ERR_ARGUMENT, "label gains: src / labels / dst is NULL");
  for (uint64_t i = 0; i < count; ++i) dst[i] = vr_label_gain(src[i], n > 0 ? labels[i] : 0u, gains, n);
  return VR_OK;
}

int vr_set_smoothing(vr_context *h, const float sigma[3]) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_smoothing(sigma)) return rc;
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  const float zero[3] = {0.f, 0.f, 0.f};
  const float *sg = sigma ? sigma : zero;
  const bool any = sg[0] != 0.f || sg[1] != 0.f || sg[2] != 0.f;
  if (any && !h->children.empty()) return smoothing_unsupported("vr_set_smoothing");
  if (sg[0] == h->smooth_sigma[0] && sg[1] == h->smooth_sigma[1] && sg[2] == h->smooth_sigma[2]) return VR_OK;  // no change
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();
  const float old[3] = {h->smooth_sigma[0], h->smooth_sigma[1], h->smooth_sigma[2]};
  const uint64_t old_version = h->smooth_version;
  for (int j = 0; j < 3; ++j) h->smooth_sigma[j] = sg[j] + 0.f;  // (-0 is no smoothing)
  h->smooth_version = next_version();
  int rc = VR_OK;
  try {
    rc = apply_derived(h);
  } catch (...) {  // a failed pass left the unmodified upload: the handle says so (no sigma), and the same
    for (int j = 0; j < 3; ++j) h->smooth_sigma[j] = 0.f;  // sigma set again is a change and derives again
    h->smooth_version = next_version();
    throw;
  }
  if (rc == VR_ERR_VRAM) {  // nothing was written: the state stays as it was
    for (int j = 0; j < 3; ++j) h->smooth_sigma[j] = old[j];
    h->smooth_version = old_version;
  }
  return rc;
  VR_GUARD_END
}

int vr_get_smoothing(vr_context *h, float sigma[3]) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!sigma) return fail(VR_ERR_ARGUMENT, "smoothing: sigma is NULL");
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  for (int j = 0; j < 3; ++j) sigma[j] = h->smooth_sigma[j];
  return VR_OK;
}

int vr_smooth_weights_host(float sigma, int32_t *radius, float *w) {
  const float s3[3] = {sigma, 0.f, 0.f};
  if (int rc = check_smoothing(s3)) return rc;
  if (!radius || !w) return fail(VR_ERR_ARGUMENT, "smoothing: radius / w is NULL");
  *radius = vr_smooth_weights(sigma, w);
  return VR_OK;
}

int vr_smooth_host(const float *src, const uint64_t dims[3], const float sigma[3], float *dst) {
  if (int rc = check_smoothing(sigma)) return rc;
  if (!dims || !sigma) return fail(VR_ERR_ARGUMENT, "smoothing: dims / sigma is NULL");
  if (dims[0] > 0x7FFFFFFF || dims[1] > 0x7FFFFFFF || dims[2] > 0x7FFFFFFF)
    return fail(VR_ERR_UNSUPPORTED, "smoothing: volume dimension too large");
  const uint64_t count = dims[0] * dims[1] * dims[2];
  if (!count) return VR_OK;
  if (!src || !dst) return fail(VR_ERR_ARGUMENT, "smoothing: src / dst is NULL");
  try {
    int axes[3], np = 0;
    for (int j = 0; j < 3; ++j)
      if (sigma[j] > 0.f && dims[j] > 1) axes[np++] = j;
    if (!np) {
      if (dst != src) std::memcpy(dst, src, count * sizeof(float));
      return VR_OK;
    }
    // the passes alternate between dst and one temporary so that the last writes dst; a first pass
    // that would write the array it reads (dst == src) reads a copy
    std::vector<float> tmp(np > 1 ? count : 0), copy;
    const float *in = src;
    if (np % 2 == 1 && dst == src) {
      copy.assign(src, src + count);
      in = copy.data();
    }
    for (int i = 0; i < np; ++i) {
      const int j = axes[i];
      float w[VR_SMOOTH_MAX_TAPS];
      const int32_t R = vr_smooth_weights(sigma[j], w);
      float *out = (np - 1 - i) % 2 ? tmp.data() : dst;
      const int64_t n = (int64_t)dims[j];
      const uint64_t stride = j == 0 ? 1 : (j == 1 ? dims[0] : dims[0] * dims[1]);
      const uint64_t inner = stride, outer = count / (stride * dims[j]);
      for (uint64_t o = 0; o < outer; ++o)
        for (int64_t c = 0; c < n; ++c)
          for (uint64_t q = 0; q < inner; ++q) {
            const uint64_t base = o * stride * dims[j] + q;
            out[base + (uint64_t)c * stride] = vr_smooth_tap(w, R, [=](int32_t k) {
              int64_t t = c - R + k;
              t = t < 0 ? 0 : (t > n - 1 ? n - 1 : t);
              return in[base + (uint64_t)t * stride];
            });
          }
      in = out;
    }
  } catch (const std::bad_alloc &) {
    return fail(VR_ERR_DEVICE, "host out of memory");
  }
  return VR_OK;
}

int vr_set_deconvolution(vr_context *h, const float sigma[3], int32_t iterations, float flr) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (int rc = check_deconvolution(sigma, iterations, flr)) return rc;
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  // one form of "none": no sigma, no iterations, no floor
  const bool any = sigma && iterations > 0 && (sigma[0] != 0.f || sigma[1] != 0.f || sigma[2] != 0.f);
  const float sg[3] = {any ? sigma[0] + 0.f : 0.f, any ? sigma[1] + 0.f : 0.f, any ? sigma[2] + 0.f : 0.f};
  const int32_t it = any ? iterations : 0;
  const float fl = any ? flr : 0.f;
  if (any && !h->children.empty()) return deconvolution_unsupported("vr_set_deconvolution");
  if (sg[0] == h->deconv_sigma[0] && sg[1] == h->deconv_sigma[1] && sg[2] == h->deconv_sigma[2] &&
      it == h->deconv_iterations && fl == h->deconv_floor)
    return VR_OK;  // no change
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();
  const float old[3] = {h->deconv_sigma[0], h->deconv_sigma[1], h->deconv_sigma[2]};
  const int32_t old_it = h->deconv_iterations;
  const float old_fl = h->deconv_floor;
  const uint64_t old_version = h->deconv_version;
  auto set = [h](const float *s3, int32_t n, float f, uint64_t version) {
    for (int j = 0; j < 3; ++j) h->deconv_sigma[j] = s3[j];
    h->deconv_iterations = n;
    h->deconv_floor = f;
    h->deconv_version = version;
  };
  set(sg, it, fl, next_version());
  int rc = VR_OK;
  try {
    rc = apply_derived(h);
  } catch (...) {  // a failed pass left the unmodified upload: the handle says so (no deconvolution), and the
    const float zero[3] = {0.f, 0.f, 0.f};  // same setting given again is a change and derives again
    set(zero, 0, 0.f, next_version());
    throw;
  }
  if (rc == VR_ERR_VRAM) set(old, old_it, old_fl, old_version);  // nothing was written: the state stays as it was
  return rc;
  VR_GUARD_END
}

int vr_get_deconvolution(vr_context *h, float sigma[3], int32_t *iterations, float *flr) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!sigma || !iterations || !flr) return fail(VR_ERR_ARGUMENT, "deconvolution: sigma / iterations / floor is NULL");
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  for (int j = 0; j < 3; ++j) sigma[j] = h->deconv_sigma[j];
  *iterations = h->deconv_iterations;
  *flr = h->deconv_floor;
  return VR_OK;
}

int vr_deconvolve_host(const float *src, const uint64_t dims[3], const float sigma[3], int32_t iterations, float flr,
                       float *dst) {
  if (int rc = check_deconvolution(sigma, iterations, flr)) return rc;
  if (!dims || !sigma) return fail(VR_ERR_ARGUMENT, "deconvolution: dims / sigma is NULL");
  if (dims[0] > 0x7FFFFFFF || dims[1] > 0x7FFFFFFF || dims[2] > 0x7FFFFFFF)
    return fail(VR_ERR_UNSUPPORTED, "deconvolution: volume dimension too large");
  const uint64_t count = dims[0] * dims[1] * dims[2];
  if (!count) return VR_OK;
  if (!src || !dst) return fail(VR_ERR_ARGUMENT, "deconvolution: src / dst is NULL");
  if (iterations == 0 || (sigma[0] == 0.f && sigma[1] == 0.f && sigma[2] == 0.f)) {  // off: a copy
    if (dst != src) std::memcpy(dst, src, count * sizeof(float));
    return VR_OK;
  }
  try {
    // y is read to the end (dst may be src); u the estimate, t the blurred estimate, then the ratio and
    // the blurred ratio.  B is vr_smooth_host: vr_smooth_tap per active axis, which may work in place.
    const std::vector<float> y(src, src + count);
    std::vector<float> u(count), t(count);
    for (uint64_t i = 0; i < count; ++i) u[i] = vr_deconv_data(y[i]);
    for (int32_t k = 0; k < iterations; ++k) {
      if (int rc = vr_smooth_host(u.data(), dims, sigma, t.data())) return rc;
      for (uint64_t i = 0; i < count; ++i) t[i] = vr_deconv_ratio(y[i], t[i], flr);
      if (int rc = vr_smooth_host(t.data(), dims, sigma, t.data())) return rc;
      for (uint64_t i = 0; i < count; ++i) u[i] = vr_deconv_update(u[i], t[i]);
    }
    std::memcpy(dst, u.data(), count * sizeof(float));
  } catch (const std::bad_alloc &) {
    return fail(VR_ERR_DEVICE, "host out of memory");
  }
  return VR_OK;
}

// Measurement entries of tools/deconv_bench.py, not part of include/vrhip.h: one filter pass with an epilogue
// of the deconvolution (epi, flags: csrc/vr_deconv.h VR_EPI_*; d_aux may be d_dst for the update), or one of
// the two elementwise steps as a launch of its own, between caller-owned padded device buffers.
extern "C" int vr_deconv_axis_device(const float *d_src, float *d_dst, const uint64_t dims[3], int32_t axis,
                                     const float *d_weights, int32_t radius, int32_t epi, const float *d_aux, float flr,
                                     uint32_t flags, void *d_stats, void *stream) {
  if (!d_src || !d_dst || d_src == d_dst || !dims || !d_weights || axis < 0 || axis > 2 || radius < 1 ||
      radius > VR_SMOOTH_MAX_RADIUS || !dims[0] || !dims[1] || !dims[2] || dims[0] > 0x7FFFFFFF ||
      dims[1] > 0x7FFFFFFF || dims[2] > 0x7FFFFFFF || epi < VR_EPI_FILTER || epi > VR_EPI_UPDATE ||
      (epi != VR_EPI_FILTER && !d_aux) || (epi != VR_EPI_UPDATE && (d_stats || d_aux == d_dst)))
    return fail(VR_ERR_ARGUMENT, "deconvolution: invalid pass arguments");
  VR_GUARD_BEGIN
  VR_HIP(vr::launch_deconv_axis(d_src, d_dst, (int32_t)dims[0], (int32_t)dims[1], (int32_t)dims[2], axis, d_weights,
                                radius, epi, d_aux, flr, flags, static_cast<vr::BufStats *>(d_stats),
                                (hipStream_t)stream));
  return VR_OK;
  VR_GUARD_END
}

extern "C" int vr_deconv_pointwise_device(const float *d_src, float *d_dst, const uint64_t dims[3], int32_t epi,
                                          const float *d_aux, float flr, uint32_t flags, void *stream) {
  if (!d_src || !d_dst || !d_aux || !dims || !dims[0] || !dims[1] || !dims[2] || dims[0] > 0x7FFFFFFF ||
      dims[1] > 0x7FFFFFFF || dims[2] > 0x7FFFFFFF || (epi != VR_EPI_RATIO && epi != VR_EPI_UPDATE))
    return fail(VR_ERR_ARGUMENT, "deconvolution: invalid pass arguments");
  VR_GUARD_BEGIN
  VR_HIP(vr::launch_deconv_pointwise(d_src, d_dst, (int32_t)dims[0], (int32_t)dims[1], (int32_t)dims[2], epi, d_aux,
                                     flr, flags, (hipStream_t)stream));
  return VR_OK;
  VR_GUARD_END
}

// Measurement entries of tools/smooth_bench.py, not part of include/vrhip.h: one axis pass, or the fused
// launch, between two padded device buffers (d_weights: 3 x 25 floats for the fused form, 2 radius + 1 for
// a pass), and a read-back of `count` floats at element `offset` of the handle's resident emission buffer.
extern "C" int vr_smooth_axis_device(const float *d_src, float *d_dst, const uint64_t dims[3], int32_t axis,
                                     const float *d_weights, int32_t radius, void *d_stats, void *stream) {
  if (!d_src || !d_dst || d_src == d_dst || !dims || !d_weights || axis < 0 || axis > 2 || radius < 1 ||
      radius > VR_SMOOTH_MAX_RADIUS || !dims[0] || !dims[1] || !dims[2] || dims[0] > 0x7FFFFFFF ||
      dims[1] > 0x7FFFFFFF || dims[2] > 0x7FFFFFFF)
    return fail(VR_ERR_ARGUMENT, "smoothing: invalid pass arguments");
  VR_GUARD_BEGIN
  VR_HIP(vr::launch_smooth_axis(d_src, d_dst, (int32_t)dims[0], (int32_t)dims[1], (int32_t)dims[2], axis, d_weights,
                                radius, static_cast<vr::BufStats *>(d_stats), (hipStream_t)stream));
  return VR_OK;
  VR_GUARD_END
}

extern "C" int vr_smooth_fused_device(const float *d_src, float *d_dst, const uint64_t dims[3], const float *d_weights,
                                      const int32_t radius[3], void *d_stats, void *stream) {
  if (!d_src || !d_dst || d_src == d_dst || !dims || !d_weights || !radius || dims[0] > 0x7FFFFFFF ||
      dims[1] > 0x7FFFFFFF || dims[2] > 0x7FFFFFFF)
    return fail(VR_ERR_ARGUMENT, "smoothing: invalid pass arguments");
  VR_GUARD_BEGIN
  VR_HIP(vr::launch_smooth_fused(d_src, d_dst, (int32_t)dims[0], (int32_t)dims[1], (int32_t)dims[2], d_weights,
                                 radius[0], radius[1], radius[2], static_cast<vr::BufStats *>(d_stats),
                                 (hipStream_t)stream));
  return VR_OK;
  VR_GUARD_END
}

extern "C" int vr_debug_derive_times(vr_context *h, double out[2]) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!valid(h) || !out) return fail(VR_ERR_HANDLE, "Handle not valid.");
  out[0] = h->derive_ms[0];
  out[1] = h->derive_ms[1];
  return VR_OK;
}

// The upload version of the handle's resident emission buffer (0: none): every upload and every derivation
// takes a new one, so an unchanged version says that nothing was written.
extern "C" int vr_debug_emission_version(vr_context *h, uint64_t *version) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!valid(h) || !version) return fail(VR_ERR_HANDLE, "Handle not valid.");
  const BufPtr b = label_target(h);
  *version = b ? b->version : 0;
  return VR_OK;
}

extern "C" int vr_debug_read_emission(vr_context *h, uint64_t offset, uint64_t count, float *out) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  const BufPtr b = label_target(h);
  if (!b || !b->ptr || !out || offset + count > b->bytes / sizeof(float))
    return fail(VR_ERR_ARGUMENT, "read_emission: no resident emission buffer, or a range outside it");
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  VR_HIP(hipMemcpy(out, b->ptr + offset, count * sizeof(float), hipMemcpyDeviceToHost));
  return VR_OK;
  VR_GUARD_END
}

int vr_clip_convert_host(const vr_clip_plane *planes, int32_t n, const float bmin[3], const float bscale[3],
                         float *out) {
  if (int rc = check_clip(planes, n)) return rc;
  if (!bmin || !bscale || (n > 0 && !out)) return fail(VR_ERR_ARGUMENT, "clip planes: box / output is NULL");
  for (int32_t i = 0; i < n; ++i) convert_clip(planes[i], bmin, bscale, out + 4 * (size_t)i);
  return VR_OK;
}

int vr_transfer_lookup_host(const float *table, int32_t n, int32_t ncomp, const float lim[2], const float *c,
                            uint64_t m, float *out) {
  if (n < 2 || n > VR_TF_MAX_ENTRIES || ncomp < 1) return fail(VR_ERR_ARGUMENT, "table: 2 .. 1024 entries, ncomp >= 1");
  if (!lim || !std::isfinite(lim[0]) || !std::isfinite(lim[1]) || !(lim[0] < lim[1]))
    return fail(VR_ERR_ARGUMENT, "table: limits must be finite with lo < hi");
  if (m && (!table || !c || !out)) return fail(VR_ERR_ARGUMENT, "table / coordinates / output is NULL");
  for (int32_t k = 0; k < ncomp; ++k)
    for (uint64_t j = 0; j < m; ++j) out[(uint64_t)k * m + j] = transfer_lookup(table + (size_t)k * (size_t)n, n, lim, c[j]);
  return VR_OK;
}

int64_t vr_partition_columns(int64_t w, const vr_partition *p) {
  if (!p) return w < 0 ? 0 : w;
  if (p->num_parts < 1 || p->block_cols < 1 || p->part < 0 || p->part >= p->num_parts) return -1;
  return part_columns(w, p->block_cols, p->part, p->num_parts);
}

int vr_assemble_partitions(const float *d_parts, int64_t w, int64_t h, int32_t block_cols, int32_t num_parts,
                           int64_t max_cols, float *d_out, void *stream) {
  if (w < 0 || h < 0 || block_cols < 1 || num_parts < 1) return fail(VR_ERR_ARGUMENT, "invalid partition");
  VR_GUARD_BEGIN
  VR_HIP(vr::launch_assemble(d_parts, w, h, block_cols, num_parts, max_cols, d_out, (hipStream_t)stream));
  return VR_OK;
  VR_GUARD_END
}

int vr_render_slab(vr_context *h, const vr_render_args *a, const vr_slab *slab, const vr_partition *part,
                   const float *d_state_in, float *d_state_out, void *stream) {
  std::lock_guard<std::mutex> lk(g_mu);
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");
  if (!a) return fail(VR_ERR_ARGUMENT, "insufficient parameter!");
  if (h->nclip) return clip_unsupported("vr_render_slab");
  if (smoothing_set(h)) return smoothing_unsupported("vr_render_slab");
  if (deconvolution_set(h)) return deconvolution_unsupported("vr_render_slab");
  VR_GUARD_BEGIN
  DeviceGuard dg(h->device);
  vr_host::prune_retired();  // buffers whose last launch has completed
  Frame F;
  return do_render_slab(h, a, slab, part, d_state_in, d_state_out, (hipStream_t)stream, F);
  VR_GUARD_END
}

int vr_slab_planes(const uint64_t dims[3], const float element_size_um[3], double z0, double z1, uint64_t *first,
                   uint64_t *count) {
  if (!dims || !element_size_um || !first || !count || dims[0] == 0 || dims[2] == 0)
    return fail(VR_ERR_ARGUMENT, "invalid slab geometry");
  // gradient tap offset along z in texels (volumeRender.cpp:273-275 through initRender's box):
  // gstep_z * bscale_z * D = vw * es_x / (2 * es_z * D), es reversed as render.cpp:195 does
  const double esx = element_size_um[2], esz = element_size_um[0];
  const double D = (double)dims[2];
  const double off = (double)dims[0] * esx / (2.0 * esz * D) + 0.5;
  const double lo = std::isfinite(z0) ? std::floor(z0 - 0.5 - off) - 1.0 : 0.0;
  const double hi = std::isfinite(z1) ? std::floor(z1 - 0.5 + off) + 3.0 : D;
  const double a = std::min(std::max(lo, 0.0), D), b = std::min(std::max(hi, 0.0), D);
  *first = (uint64_t)a;
  *count = b > a ? (uint64_t)(b - a) : 0;
  return VR_OK;
}

int vr_depth_lanes(int64_t part_cols, int64_t height) {
  vr::RenderParams P;
  std::memset(&P, 0, sizeof(P));
  P.part_cols = (int32_t)std::min<int64_t>(part_cols, 0x7fffffff);
  P.height = (int32_t)std::min<int64_t>(height, 0x7fffffff);
  return depth_lanes(P);
}

int vr_depth_lanes_tau(int64_t part_cols, int64_t height, double texels_per_pixel) {
  vr::RenderParams P;
  std::memset(&P, 0, sizeof(P));
  P.part_cols = (int32_t)std::min<int64_t>(part_cols, 0x7fffffff);
  P.height = (int32_t)std::min<int64_t>(height, 0x7fffffff);
  P.tau = (float)texels_per_pixel;
  return depth_lanes(P);
}

int vr_synth_shell_device(float *d_out, uint64_t n, void *stream) {
  VR_GUARD_BEGIN
  VR_HIP(vr::launch_synth_shell(d_out, n, 0, n, (hipStream_t)stream));
  return VR_OK;
  VR_GUARD_END
}

int vr_synth_shell_planes_device(float *d_out, uint64_t n, uint64_t z_first, uint64_t count, void *stream) {
  if (z_first + count > n) return fail(VR_ERR_ARGUMENT, "planes outside the volume");
  VR_GUARD_BEGIN
  VR_HIP(vr::launch_synth_shell(d_out, n, z_first, count, (hipStream_t)stream));
  return VR_OK;
  VR_GUARD_END
}

int vr_gradient_device(const float *d_data, const uint64_t dims[3], float *d_gx, float *d_gy, float *d_gz,
                       void *stream) {
  if (!dims) return fail(VR_ERR_ARGUMENT, "dims is NULL");
  if (dims[0] > 0xFFFFFFFFull || dims[1] > 0xFFFFFFFFull || dims[2] > 0xFFFFFFFFull)
    return fail(VR_ERR_UNSUPPORTED, "dimension above 2^32");
  if (dims[0] * dims[1] * dims[2] && (!d_data || !d_gx || !d_gy || !d_gz)) return fail(VR_ERR_ARGUMENT, "NULL buffer");
  VR_GUARD_BEGIN
  VR_HIP(vr::launch_gradient(d_data, dims, d_gx, d_gy, d_gz, (hipStream_t)stream));
  return VR_OK;
  VR_GUARD_END
}

int vr_debug_slot_transition(const int32_t idx_in[3], int32_t sim_em_ab, int32_t sim_em_re, int32_t sim_ab_re,
                             int32_t req_em, int32_t req_ab, int32_t req_re, int32_t idx_out[3],
                             int32_t unbound_out[3]) {
  DebugState s;
  s.idx_em = idx_in[0];
  s.idx_ab = idx_in[1];
  s.idx_re = idx_in[2];
  sync_decisions(s, sim_em_ab, sim_em_re, sim_ab_re, req_em, req_ab, req_re);
  idx_out[0] = s.idx_em;
  idx_out[1] = s.idx_ab;
  idx_out[2] = s.idx_re;
  for (int i = 0; i < 3; ++i) unbound_out[i] = !s.bound[i];
  return VR_OK;
}

#define HG_PI ((float)3.141592653589793238462643383279502884197169399375105820)

// HenyeyGreenstein on the device: the generator's expression per element on
// the GPU, with the sines / cosines of k*pi/N computed here exactly as the host generator does.
int vr_henyey_greenstein_device(uint32_t n, float g, float *d_out, void *stream) {
  if (g > 1 || g < -1) return fail(VR_ERR_ARGUMENT, "g must be in interval [-1,1]");
  if (n && !d_out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  if (!n) return VR_OK;
  VR_GUARD_BEGIN
  const float frac_half = HG_PI / n;
  std::vector<float> tab(2 * (size_t)n);
  for (uint32_t k = 0; k < n; ++k) {
    const float ang = k * frac_half;
    tab[k] = sinf(ang);
    tab[n + k] = cosf(ang);
  }
  hipStream_t s = (hipStream_t)stream;
  float *d_tab = nullptr;
  VR_HIP(hipMallocAsync(reinterpret_cast<void **>(&d_tab), tab.size() * sizeof(float), s));
  VR_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, s));
  VR_HIP(vr::launch_hg_lut(n, d_tab, d_tab + n, g, powf(g, 2.f), 1.f - powf(g, 2.f), d_out, s));
  VR_HIP(hipFreeAsync(d_tab, s));
  VR_HIP(hipStreamSynchronize(s));  // the host table is borrowed by the copy
  return VR_OK;
  VR_GUARD_END
}

// Volume.normalize(newMin, newMax) on the device (Volume.m:208-220), d_out may equal d_in.
int vr_normalize_device(const float *d_in, uint64_t n, double new_min, double new_max, float *d_out, void *stream) {
  if (n && (!d_in || !d_out)) return fail(VR_ERR_ARGUMENT, "NULL buffer");
  if (!n) return VR_OK;
  VR_GUARD_BEGIN
  hipStream_t s = (hipStream_t)stream;
  uint32_t *mm = nullptr;
  VR_HIP(hipMallocAsync(reinterpret_cast<void **>(&mm), 2 * sizeof(uint32_t), s));
  // MATLAB: (newMax - newMin) in double, then single with the single data; newMin single likewise
  VR_HIP(vr::launch_normalize(d_in, n, mm, (float)(new_max - new_min), (float)new_min, d_out, s));
  VR_HIP(hipFreeAsync(mm, s));
  return VR_OK;
  VR_GUARD_END
}

// Volume.resize(newsize) on the device (Volume.m:93-106 -> imresize3 / imresize): separable cubic
// passes with antialiasing when shrinking, the axes in order of increasing scale (stable), an axis
// whose length does not change skipped (its contributions are the identity).
int vr_resize_device(const float *d_in, const uint64_t in_dims[3], const uint64_t out_dims[3], float *d_out,
                     void *stream) {
  if (!in_dims || !out_dims) return fail(VR_ERR_ARGUMENT, "dims is NULL");
  uint64_t nin = 1, nout = 1;
  for (int i = 0; i < 3; ++i) {
    if (in_dims[i] > 0x7FFFFFFFull || out_dims[i] > 0x7FFFFFFFull) return fail(VR_ERR_UNSUPPORTED, "dimension too large");
    nin *= in_dims[i];
    nout *= out_dims[i];
  }
  if (!nout) return VR_OK;
  if (!nin) return fail(VR_ERR_ARGUMENT, "cannot resize an empty volume");
  if (!d_in || !d_out) return fail(VR_ERR_ARGUMENT, "NULL buffer");
  VR_GUARD_BEGIN
  hipStream_t s = (hipStream_t)stream;
  int order[3] = {0, 1, 2};
  double sc[3];
  for (int i = 0; i < 3; ++i) sc[i] = (double)out_dims[i] / (double)in_dims[i];
  std::stable_sort(order, order + 3, [&](int a, int b) { return sc[a] < sc[b]; });
  std::vector<int> passes;
  for (int k = 0; k < 3; ++k)
    if (out_dims[order[k]] != in_dims[order[k]]) passes.push_back(order[k]);
  if (passes.empty()) {
    VR_HIP(hipMemcpyAsync(d_out, d_in, nin * sizeof(float), hipMemcpyDeviceToDevice, s));
    return VR_OK;
  }
  uint64_t cur[3] = {in_dims[0], in_dims[1], in_dims[2]};
  const float *src = d_in;
  // the device temporaries and the host contributions their copies read: all kept until the stream
  // has drained (the final synchronize, or the guard's on an error part-way)
  struct Temps {
    hipStream_t s;
    std::vector<void *> dev;
    std::vector<std::vector<double>> w;
    std::vector<std::vector<int32_t>> idx;
    ~Temps() {  // stream-ordered frees after the passes, then the host data is released
      hipError_t e = hipSuccess;
      for (void *t : dev) {
        const hipError_t r = hipFreeAsync(t, s);
        if (e == hipSuccess) e = r;
      }
      const hipError_t r = hipStreamSynchronize(s);
      if (e == hipSuccess) e = r;
      // (a destructor: not thrown -- a device fault stays pending for the next entry's check)
      if (e != hipSuccess && !vr_host::device_fault(e)) {
        (void)hipGetLastError();
        vr_host::log_error(e, "handled", "vr_resize_device temporaries", true);
      }
    }
  } temps{s, {}, {}, {}};
  temps.w.reserve(passes.size());
  temps.idx.reserve(passes.size());
  for (size_t k = 0; k < passes.size(); ++k) {
    const int dim = passes[k];
    temps.w.emplace_back();
    temps.idx.emplace_back();
    std::vector<double> &w = temps.w.back();
    std::vector<int32_t> &idx = temps.idx.back();
    int32_t P = 0;
    resize_contributions(cur[dim], out_dims[dim], w, idx, P);
    double *d_w = nullptr;
    int32_t *d_idx = nullptr;
    VR_HIP(hipMallocAsync(reinterpret_cast<void **>(&d_w), w.size() * sizeof(double), s));
    temps.dev.push_back(d_w);
    VR_HIP(hipMallocAsync(reinterpret_cast<void **>(&d_idx), idx.size() * sizeof(int32_t), s));
    temps.dev.push_back(d_idx);
    VR_HIP(hipMemcpyAsync(d_w, w.data(), w.size() * sizeof(double), hipMemcpyHostToDevice, s));
    VR_HIP(hipMemcpyAsync(d_idx, idx.data(), idx.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
    uint64_t nxt[3] = {cur[0], cur[1], cur[2]};
    nxt[dim] = out_dims[dim];
    float *dst = d_out;
    if (k + 1 < passes.size()) {
      VR_HIP(hipMallocAsync(reinterpret_cast<void **>(&dst), nxt[0] * nxt[1] * nxt[2] * sizeof(float), s));
      temps.dev.push_back(dst);
    }
    VR_HIP(vr::launch_resize_dim(src, cur, dim, out_dims[dim], d_w, d_idx, P, dst, s));
    src = dst;
    for (int i = 0; i < 3; ++i) cur[i] = nxt[i];
  }
  return VR_OK;  // ~Temps: free, then synchronize
  VR_GUARD_END
}

// The contributions of one resize axis, for tests: writes P (taps kept) and, if w / idx are not
// NULL, out_len * P weights and 0-based indices.
int vr_resize_contributions(uint64_t in_len, uint64_t out_len, int32_t *P, double *w, int32_t *idx) {
  if (!P || !in_len || !out_len) return fail(VR_ERR_ARGUMENT, "invalid resize axis");
  std::vector<double> ww;
  std::vector<int32_t> ii;
  resize_contributions(in_len, out_len, ww, ii, *P);
  if (w) std::memcpy(w, ww.data(), ww.size() * sizeof(double));
  if (idx) std::memcpy(idx, ii.data(), ii.size() * sizeof(int32_t));
  return VR_OK;
}

// HenyeyGreenstein.cc:39-91 (g in [-1, 1], value at c*N*N + a*N + b)
int vr_henyey_greenstein(uint32_t n, float g, float *out) {
  if (g > 1 || g < -1) return fail(VR_ERR_ARGUMENT, "g must be in interval [-1,1]");
  if (n && !out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  const float frac_half = HG_PI / n;
  const size_t page = (size_t)n * n;
  const float num = 1.f - powf(g, 2.f);
  const float g2 = powf(g, 2.f);
  for (uint32_t c = 0; c < n; ++c) {
    const float gamma = c * frac_half;
    const float s = sinf(gamma), co = cosf(gamma);
    for (uint32_t a = 0; a < n; ++a) {
      const float alpha = a * frac_half;
      const float lx = sinf(alpha), lz = cosf(alpha);
      // lightOut (sin a, 0, cos a) rotated about X by gamma (float3.h:77-106)
      const float rx = 1.f * lx + 0.f * 0.f + 0.f * lz;
      const float ry = 0.f * lx + co * 0.f + s * lz;
      const float rz = 0.f * lx + -s * 0.f + co * lz;
      for (uint32_t b = 0; b < n; ++b) {
        const float beta = b * frac_half;
        const float ix = sinf(beta), iz = cosf(beta);
        const float cosTheta = rx * ix + ry * 0.f + rz * iz;
        const float den = sqrtf(powf((1.f + g2 - (2.f * g * cosTheta)), 3.f));
        out[(size_t)c * page + (size_t)a * n + b] = 1.f / (4.f * HG_PI) * (num / den);
      }
    }
  }
  return VR_OK;
}

// ---- typed volumes: the value contract on the host (no device needed) ---------------------------
static_assert(vr::DT_F32 == VR_F32 && vr::DT_U8 == VR_U8 && vr::DT_U16 == VR_U16 && vr::DT_I16 == VR_I16 &&
                  vr::DT_F16 == VR_F16 && vr::DT_UNORM == VR_DTYPE_UNORM,
              "vr_convert.h codes = include/vrhip.h vr_dtype");

size_t vr_dtype_size(int32_t dtype) { return vr::dtype_size(dtype); }

int vr_convert_host(const void *src, int32_t dtype, uint64_t n, float *dst) {
  const size_t es = vr::dtype_size(dtype);
  if (!es) return fail(VR_ERR_ARGUMENT, "vr_convert_host: invalid dtype");
  if (n && (!src || !dst)) return fail(VR_ERR_ARGUMENT, "vr_convert_host: NULL pointer");
  if (reinterpret_cast<uintptr_t>(src) % es)
    return fail(VR_ERR_ARGUMENT, "vr_convert_host: src is not aligned to its element size");
  switch (dtype) {
    case VR_F32: convert_host<float, false>(src, n, dst); break;
    case VR_U8: convert_host<uint8_t, false>(src, n, dst); break;
    case VR_U8 | VR_DTYPE_UNORM: convert_host<uint8_t, true>(src, n, dst); break;
    case VR_U16: convert_host<uint16_t, false>(src, n, dst); break;
    case VR_U16 | VR_DTYPE_UNORM: convert_host<uint16_t, true>(src, n, dst); break;
    case VR_I16: convert_host<int16_t, false>(src, n, dst); break;
    case VR_F16: convert_host<vr::half_bits, false>(src, n, dst); break;
  }
  return VR_OK;
}

uint64_t vr_timestamp(void) {
  const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                      std::chrono::system_clock::now().time_since_epoch())
                      .count();
  return (uint64_t)(uint32_t)(uint64_t)ms;  // stored through an int* (timestamp.cpp:25,33)
}

const char *vr_last_error(void) { return g_last_error.c_str(); }

int64_t vr_hip_errors(char *buf, size_t buflen) {
  vr_host::ErrLog &L = vr_host::errlog();
  std::lock_guard<std::mutex> g(L.mu);
  if (buf && buflen) {
    std::string s;
    for (const std::string &l : L.lines) s += l + "\n";
    const size_t n = std::min(buflen - 1, s.size());
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return (int64_t)L.count;
}

int vr_set_option(const char *name, int64_t value) {
  if (name && std::strcmp(name, "test_switches") == 0) {
    g_test_switches.store(value ? 1 : 0);
    return VR_OK;
  }
  return fail(VR_ERR_ARGUMENT, std::string("unknown option ") + (name ? name : "(null)"));
}

int vr_last_march_kernel(char *buf, size_t buflen) {
  std::lock_guard<std::mutex> lk(g_mu);
  const std::string &s = vr::last_march_kernel();
  if (buf && buflen) {
    const size_t n = std::min(buflen - 1, s.size());
    std::memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return VR_OK;
}

int vr_last_launch_flags(uint32_t *flags) {
  if (!flags) return fail(VR_ERR_ARGUMENT, "vr_last_launch_flags: flags is NULL");
  std::lock_guard<std::mutex> lk(g_mu);
  *flags = g_last_launch_flags;
  return VR_OK;
}

const char *vr_version(void) { return "libvrhip 0.1 gfx950 (MI355X) volume ray-marcher"; }

}  // extern "C"
