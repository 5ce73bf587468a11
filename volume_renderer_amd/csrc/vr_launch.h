// vr_launch.h -- what crosses between the host driver and the kernel files, declared once: the launchers
// the kernel files define (each named below with its file), the callbacks they call back into the host
// for (vr_state.hip), and the entry table of the march objects (vr_frame.hip march_entries).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "vr_clip.h"
#include "vr_device.h"
#include "vr_histogram.h"
#include "vr_slice.h"

#ifndef VR_WITH_K8
#define VR_WITH_K8 0  // the K = 8 march objects (diagnostic build, make DIAG=1)
#endif

namespace vr {
// clip (here and below): the launch's plane set (vr_clip.h), or null / n == 0 -- the unclipped kernels
hipError_t launch_render(const RenderParams &P, int mode, bool ab_alias, bool big, bool share, hipStream_t s,
                         const ClipSet *clip);
// vr_project.hip: mode = vr_projection; aux: the [plane_cols][H] aux plane or null
hipError_t launch_project(const RenderParams &P, int mode, float *aux, bool big, bool probe, hipStream_t s,
                          const ClipSet *clip);
hipError_t launch_isosurface(const RenderParams &P, int grad, float level, float *depth, float *normal, bool big,
                             bool probe, hipStream_t s, const ClipSet *clip);
// vr_transfer.hip: tab = the segment records of transfer_table_units(nc, na) 16-byte units
uint32_t transfer_table_units(int32_t nc, int32_t na);
hipError_t launch_transfer(const RenderParams &P, int grad, const float *tab, int32_t nc, int32_t na, float clo,
                           float cinv, float alo, float ainv, int32_t coord, bool ab_alias, float *alpha, bool big,
                           bool probe, hipStream_t s, const ClipSet *clip);
// vr_march.hip built with VR_MARCH_FAST=1 / 0 (namespaces fast / exact) and VR_MARCH_K = 1, 2, 4, 8
#define VR_DECL_MARCH(ns)                                                                                 \
  namespace ns {                                                                                         \
  hipError_t launch_march_k1(const RenderParams &, int, bool, bool, bool, hipStream_t);                  \
  hipError_t launch_march_k2(const RenderParams &, int, bool, bool, bool, hipStream_t);                  \
  hipError_t launch_march_k4(const RenderParams &, int, bool, bool, bool, hipStream_t);                  \
  hipError_t launch_march_k8(const RenderParams &, int, bool, bool, bool, hipStream_t);                  \
  hipError_t launch_march_slab_k1(const RenderParams &, int, hipStream_t);                                \
  hipError_t launch_march_views_k1(const RenderViews &, uint32_t, int, bool, hipStream_t);                 \
  hipError_t launch_march_views_k2(const RenderViews &, uint32_t, int, bool, hipStream_t);                 \
  hipError_t launch_march_views_k4(const RenderViews &, uint32_t, int, bool, hipStream_t);                 \
  hipError_t launch_march_slab_k2(const RenderParams &, int, hipStream_t);                                \
  hipError_t launch_march_slab_k4(const RenderParams &, int, hipStream_t);                                \
  uint32_t march_blocks_k1(const RenderParams &);                                                        \
  uint32_t march_blocks_k2(const RenderParams &);                                                        \
  uint32_t march_blocks_k4(const RenderParams &);                                                        \
  uint32_t march_blocks_k8(const RenderParams &);                                                        \
  hipError_t launch_preleap_k1(const RenderParams &, hipStream_t);                                       \
  hipError_t launch_preleap_k2(const RenderParams &, hipStream_t);                                       \
  hipError_t launch_preleap_k4(const RenderParams &, hipStream_t);                                       \
  hipError_t launch_preleap_k8(const RenderParams &, hipStream_t);                                       \
  }
VR_DECL_MARCH(fast)
VR_DECL_MARCH(exact)
#undef VR_DECL_MARCH
hipError_t launch_order(const uint32_t *cost, uint32_t n, uint32_t *order, hipStream_t s, uint32_t heavy_div,
                        uint64_t tail);
hipError_t launch_iota(uint32_t *order, uint32_t n, hipStream_t s);
hipError_t launch_pad(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, hipStream_t s);
hipError_t launch_stats(const float *src, uint64_t n, BufStats *st, hipStream_t s);
hipError_t launch_zpair(const float *src, float *dst, uint32_t n, uint32_t pxy, hipStream_t s);
hipError_t launch_occupancy(const float *p, uint32_t px, uint32_t py, uint32_t pz, uint8_t *occ, float inv_scale,
                            hipStream_t s);
// vr_slice.hip: mode = vr_slice_mode
hipError_t launch_slice(const SliceParams &S, int mode, bool big, hipStream_t s);
// vr_histogram.hip: the count launch into H.counts / H.acc (zeroed on s before; uniform: the wave-uniform
// shortcut), its grid for nrows rows of nx voxels, and the finalize launch that writes rows vr_hist_row
hipError_t launch_histogram(const HistParams &H, bool uniform, hipStream_t s);
uint64_t histogram_blocks(uint64_t nrows, uint64_t nx);
hipError_t launch_histogram_finalize(const unsigned long long *counts, const void *acc, int32_t rows, int32_t nbins,
                                     void *rows_out, hipStream_t s);
// vr_labels.hip: dst = src under the n gains of `gains` by the dense label bytes; *st += the statistics of dst
hipError_t launch_label_gain(const float *src, const uint8_t *labels, const float *gains, int32_t n, int32_t nx,
                             int32_t ny, int32_t nz, float *dst, BufStats *st, hipStream_t s);
// vr_smooth.hip: one axis (0 / 1 / 2 along dims[0] / [1] / [2]) of the Gaussian smoothing, src -> dst, both
// padded; wts: the 2R+1 weights in device memory; st null, or *st += the statistics of dst
hipError_t launch_smooth_axis(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, int axis,
                              const float *wts, int32_t R, BufStats *st, hipStream_t s);
// vr_smooth.hip: the same pass with an epilogue of the deconvolution (vr_deconv.h VR_EPI_*): aux the
// auxiliary padded buffer (for VR_EPI_UPDATE it may be dst), flr the floor; st only with VR_EPI_UPDATE
hipError_t launch_deconv_axis(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, int axis,
                              const float *wts, int32_t R, int epi, const float *aux, float flr, uint32_t flags,
                              BufStats *st, hipStream_t s);
// vr_deconv.hip: the ratio or the update as an elementwise launch over the padded volume (dst may be src or aux)
hipError_t launch_deconv_pointwise(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, int epi,
                                   const float *aux, float flr, uint32_t flags, hipStream_t s);
// vr_smooth.hip: the three axes in one launch (every dim >= 2, every radius >= 1); wts: 3 x 25 weights
hipError_t launch_smooth_fused(const float *src, float *dst, int32_t nx, int32_t ny, int32_t nz, const float *wts,
                               int32_t Rx, int32_t Ry, int32_t Rz, BufStats *st, hipStream_t s);
hipError_t launch_predict_cost(const RenderParams &P, uint32_t nb_view, uint32_t nbx, int32_t tw, int32_t th,
                               int32_t m, float dens, float xthr, uint32_t *cost, hipStream_t s);
uint64_t interleave3_entries(uint32_t px, uint32_t py, uint32_t pz);
hipError_t launch_interleave3(const float *a, const float *b, const float *c, float *out, uint32_t px,
                              uint32_t py, uint32_t pz, hipStream_t s);
hipError_t launch_sum_channels(const float *in, uint32_t nch, uint32_t nv, uint64_t img, float *out, hipStream_t s);
hipError_t launch_assemble(const float *parts, int64_t w, int64_t h, int32_t bc, int32_t np,
                           int64_t max_cols, float *out, hipStream_t s);
hipError_t launch_synth_shell(float *out, uint64_t n, uint64_t z_first, uint64_t nz, hipStream_t s);
hipError_t launch_gradient(const float *d, const uint64_t dims[3], float *gx, float *gy, float *gz, hipStream_t s);
hipError_t launch_hg_lut(uint32_t n, const float *sn, const float *cs, float g, float g2, float num, float *out,
                         hipStream_t s);
hipError_t launch_normalize(const float *d, uint64_t n, uint32_t *mm, float range, float new_min, float *out,
                            hipStream_t s);
hipError_t launch_resize_dim(const float *in, const uint64_t dims[3], int dim, uint64_t out_len, const double *w,
                             const int32_t *idx, int32_t P, float *out, hipStream_t s);
// vr_state.hip, called by the kernel files' launchers (vr_device.h declares the first two for them)
bool test_switches_on();
void note_march_kernel(bool fast, int K, int mode, bool ab, bool count, bool share, bool big, int cap, int sched,
                       int nl);
std::string &last_march_kernel();
}  // namespace vr

namespace vr_host {
// Everything the host calls in one march object (vr_march_<variant>_k<K>.o).
struct MarchEntries {
  int K, tile_w, tile_h;  // the object's depth lanes and its tile, vr_march.hip TileShape<K>::TW / TH
  hipError_t (*launch)(const vr::RenderParams &, int, bool, bool, bool, hipStream_t);
  hipError_t (*launch_slab)(const vr::RenderParams &, int, hipStream_t);
  hipError_t (*launch_views)(const vr::RenderViews &, uint32_t, int, bool, hipStream_t);
  uint32_t (*blocks)(const vr::RenderParams &);
  hipError_t (*preleap)(const vr::RenderParams &, hipStream_t);
};
// The object that serves (variant, K): the one built for it, or else the same variant's with the most
// depth lanes below K.  The only place that knows which objects the library holds.
const MarchEntries &march_entries(bool fast, int K);
// The depth lanes a launch that asks for K gets: march_entries(fast, K).K
int exact_lanes(int K, bool fast);
}  // namespace vr_host
