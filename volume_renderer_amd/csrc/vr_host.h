// vr_host.h -- what the host translation units of libvrhip.so share (internal, not installed): the
// handle and the module state's types, the checked-call and entry-guard macros, the tuning constants,
// the shared state (vr_state.hip) and the functions that cross files, all in namespace vr_host.
//   vr_state.hip     the shared state, the switches, the stream pool, the kernel files' callbacks
//   vr_sync.hip      upload and slot state machine, memory checks, deconvolution, smoothing and label gains, do_sync_volumes
//   vr_frame.hip     clip conversion, build_frame, lights, partition, depth lanes, the march entry table, schedules
//   vr_render.hip    do_render, do_render_slab, the multi-device group, view sets / channels
//   vr_features.hip  projection, slice, isosurface and transfer renders, the volume histogram
//   vr_capi.hip      the extern "C" entries of include/vrhip.h
#pragma once

#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <cmath>
#include <set>
#include <sstream>

#include "../../include/vrhip.h"
#include "vr_clip.h"
#include "vr_device.h"
#include "vr_labels.h"
#include "vr_launch.h"
#include "vr_resources.h"
#include "vr_slice.h"
#include "vr_deconv.h"
#include "vr_smooth.h"

#ifndef VR_DEPTH_ROUNDS_K1
#define VR_DEPTH_ROUNDS_K1 16.0  // K = 1 needs >= this many K = 1 waves per device wave slot (and sparse sampling)
#endif
#ifndef VR_DEPTH_ROUNDS_K2
#define VR_DEPTH_ROUNDS_K2 3.0   // K = 2 at >= this many, K = 4 below
#endif
#ifndef VR_SCHED_HEAVY_DIV
#define VR_SCHED_HEAVY_DIV 16  // full-frame schedule: heavy = duration >= the longest block's / this
#endif
#ifndef VR_SCHED_TAIL_PCT
// heavy-first only when the longest block >= this % of the packed frame.  Round 5: 0, i.e. every full
// frame heavy-first -- with the empty-space probe the metric frame's ramp-down (the blocks started
// last, ~3.5 ms each, 3.9-4.5 ms below 90 % residency, r5ad) outweighs the row-major order's L2
// locality: 27.50-27.62 -> 26.42-26.51 ms same box (heavy = longest / 16; / 8 26.47-26.62, / 32
// 26.37-26.64, / 4 26.80-27.17, / 2 28.27-28.82; r5ae, r5af); C3 28.83 -> 28.62, C2 and C5 unchanged
#define VR_SCHED_TAIL_PCT 0
#endif
#ifndef VR_SCHED_REMEASURE
#define VR_SCHED_REMEASURE 16  // full frames: block durations re-measured every this many launches
#endif
#ifndef VR_DEPTH_TAU_K4
#define VR_DEPTH_TAU_K4 1.5      // K = 4 from this many texels per pixel (depth_lanes)
#endif
#ifndef VR_DEPTH_TAU_K1
#define VR_DEPTH_TAU_K1 0.5      // K = 1 (with >= VR_DEPTH_ROUNDS_K1 rounds) below this many
#endif

#ifndef VR_PRELEAP_LAUNCH
#define VR_PRELEAP_LAUNCH 1  // round 6: the pre-leap launch before scheduled tame marches (vr_march.hip preleap_kernel)
#endif
#define VR_WG_WAVES_HOST 4  // waves per march workgroup (vr_march.hip VR_WG_WAVES)
#ifndef VR_SCHED_ROUNDS
#define VR_SCHED_ROUNDS 6.0      // longest-first schedule below this many K = 1 waves per wave slot
#endif
#ifndef VR_COUNT_K
#define VR_COUNT_K 0  // 1 (diagnostic build, as vr_march.hip): counter variants at every depth-lane count
#endif
#ifndef VR_XCD_RUN
#define VR_XCD_RUN 0  // march workgroups -> XCD runs (vr_march.hip xcd_block); 0: dispatch order
#endif

namespace vr_host {

#define VR_HIP(call)                                 \
  do {                                               \
    trace_pending(#call);                            \
    hipError_t e_ = (call);                          \
    if (e_ != hipSuccess) throw HipError{e_, #call}; \
  } while (0)

// VR_TRACE_STALE=1 (diagnostics): name the checked call before which this thread's HIP error state
// already held an error (one a later hipGetLastError-based check would otherwise report)
inline void trace_pending(const char *what) {
  static const bool on = [] {
    const char *ev = std::getenv("VR_TRACE_STALE");
    return ev && ev[0] == '1';
  }();
  if (!on) return;
  const hipError_t e = hipPeekAtLastError();
  if (e != hipSuccess) std::fprintf(stderr, "VR_TRACE_STALE before %s: %s\n", what, hipGetErrorString(e));
}

// texture ids = the reference's vr::VolumeType (volumeRender.h:149-157)
enum TexId { T_EM = 0, T_AB = 1, T_RE = 2, T_DX = 3, T_DY = 4, T_DZ = 5, T_LIGHT = 6, T_COUNT = 7 };
enum GradMethod { G_COMPUTE = 0, G_LOOKUP = 1 };

// Host-side record of a MATLAB Volume (vr::Volume, volumeRender.h:61-70).
struct VolRec {
  const float *data = nullptr;
  uint64_t dims[3] = {0, 0, 0};
  uint64_t memory_size = 0;
  uint64_t last_update = 0;
  int32_t location = VR_HOST;
  int32_t dtype = VR_F32;  // element type of data (vr_dtype | VR_DTYPE_UNORM); the host never reads voxels
};

// A device-resident volume (the cudaArray analog): fp32 in HBM in the apron layout of
// vr_device.h ((d0+2) x (d1+2) x (d2+2), edge-replicated border), plus its upload statistics.
struct DevBuf {
  float *ptr = nullptr;
  uint64_t dims[3] = {0, 0, 0};
  uint64_t bytes = 0;  // padded allocation size
  int device = 0;
  bool nonfinite = false;
  float maxabs = 0.f;
  uint64_t version = 0;  // bumped by every upload into this buffer
  // the MATLAB Volume it was uploaded from (VolRec identity: data pointer, TimeLastUpdate, size,
  // element type)
  const float *src_data = nullptr;
  uint64_t src_last_update = 0, src_bytes = 0;
  int32_t src_dtype = VR_F32;
  // completions of the launches / peer copies that read it (vr_resources.h): it is neither
  // rewritten nor freed before all of them
  vr_host::Readers readers;
  // a replica: completion of the peer copy that fills it (a launch on any stream waits for it)
  vr_host::EventPtr ready;
  // multi-device group (vr_new_multi): its copies on the other devices, and the version each copies
  std::map<int, std::shared_ptr<DevBuf>> replicas;
  std::map<int, uint64_t> replica_of;
  // the illumination LUT (small textures bound to the LUT slot): its z-paired copy (zpair_kernel),
  // from which the fast shading's lookups take two 16-byte loads per light instead of four 8-byte
  float *zpair = nullptr;
  uint64_t zpair_bytes = 0;
  // occupancy map (volumes of at least VR_OCC_MIN_VOXELS padded voxels; vr_kernels.hip
  // occupancy_kernel): one byte per 8^3 brick, read by the march's empty-space probe
  uint8_t *occ = nullptr;
  uint64_t occ_bytes = 0;
  // label gains (vr_set_label_gains): while the buffer is modulated, `orig` is the
  // unmodified padded upload (`bytes` long) with its statistics, and ptr, nonfinite, maxabs and occ
  // are those of the modulated values; mod_labels / mod_gains name the label upload and the gain
  // table that ptr was derived from.  Only the label pass reads orig, and the host waits for it.
  // Smoothing (vr_set_smoothing) shares the copy: ptr is orig smoothed, then modulated;
  // mod_smooth names the sigma it was smoothed with (0: not smoothed).  The deconvolution
  // (vr_set_deconvolution) runs in front of both from the same copy; mod_deconv names its
  // setting (0: none).
  float *orig = nullptr;
  bool orig_nonfinite = false;
  float orig_maxabs = 0.f;
  uint64_t mod_labels = 0, mod_gains = 0, mod_smooth = 0, mod_deconv = 0;
  ~DevBuf() {
    if (orig) vr_host::pooled_free(orig, bytes, device, vr_host::Readers());
    if (zpair) vr_host::pooled_free(zpair, zpair_bytes, device, vr_host::Readers(readers));
    if (occ) vr_host::pooled_free(occ, occ_bytes, device, vr_host::Readers(readers));
    vr_host::pooled_free(ptr, bytes, device, std::move(readers));
  }
};
using BufPtr = std::shared_ptr<DevBuf>;

}  // namespace vr_host

// The MManager analog: per-handle last-synced volumes and their device buffers.
struct vr_context {
  uint32_t signature = 0xFF00F0A5u;  // class_handle.hpp:40
  int device = 0;
  uint64_t time_last_mem_sync = 0;
  vr_host::VolRec vol[vr_host::T_COUNT];
  vr_host::BufPtr buf[vr_host::T_COUNT];
  float *d_out = nullptr;  // cached output buffer for the host-return path
  size_t d_out_bytes = 0;
  // launch schedules of the march, one per frame shape: per tile block the
  // duration measured by its last launch, and the longest-first order built from it
  struct Schedule {
    uint32_t *d_cost = nullptr, *d_order = nullptr;
    uint32_t blocks = 0;
    bool measured = false;
    uint32_t frames = 0;       // full frames launched since the last measured one
    bool order_stale = false;  // costs measured since the order was last computed
    // full frames: the measured durations copied to the host (asynchronously, after the launch) to
    // decide whether the heaviest block would form a tail
    uint32_t *h_cost = nullptr;
    hipEvent_t copied = nullptr;
    uint32_t renders = 0;  // full frames: renders of this frame key so far
    bool copy_pending = false, decided = false, tail = false;
    // round 6: the frame (camera, volume upload, opacity parameters, frame_key) the durations were
    // measured on, and the one the order in d_order was predicted for (0: none)
    uint64_t key = 0, pred_key = 0;
    // round 6: the pre-leap launch's buffers (vr_march.hip preleap_kernel): a flag per march wave,
    // ray-state slots for pre_cap waves, the slot counter
    uint32_t *pre_flag = nullptr, *pre_count = nullptr;
    float4 *pre_state = nullptr;
    uint32_t pre_waves = 0, pre_cap = 0;
  };
  std::map<std::string, Schedule> sched;
  // vr_render_channels: the views' RenderParams and lights in device memory (reused per call)
  float *d_chan = nullptr;             // per-view images of the host entry
  size_t d_chan_bytes = 0;
  // the module-global texture bindings as this handle's last sync left them (vr_render_channels
  // restores them before the channel's sync); weak: they never keep a buffer alive
  std::weak_ptr<vr_host::DevBuf> snap_bind[vr_host::T_COUNT];
  int32_t snap_idx[3] = {0, 0, 0};
  int32_t snap_grad = 0;
  bool has_snap = false;
  // multi-device group (vr_new_multi, SURVEY.md 8e inside the library): the primary (this handle,
  // the API's) holds one child per further device; each child renders a column partition of the
  // frame with replicas of the primary's bound volumes on its device, and its part is gathered
  // to the primary over xGMI (peer copies) and assembled there
  std::vector<vr_context *> children;
  vr_context *parent = nullptr;
  hipStream_t gstream = nullptr;  // child: its device's stream (replica copies, render, gather)
  hipEvent_t gdone = nullptr;     // child: its part has landed on the primary
  // child: whether copies between it and the primary go over a peer mapping (xGMI); without one
  // (hipDeviceCanAccessPeer 0, or VR_GROUP_PEER=0) they are staged through pinned host memory
  bool peer = true;
  float *d_part = nullptr;        // child: its part image; primary: all parts
  size_t d_part_bytes = 0;
  // child without a peer mapping: the pinned staging buffer of its part gather, kept across frames
  // (the gather's D2H waits for the previous frame's assembly, so the last H2D has read it), and the
  // completion of the last H2D that read it
  void *pin = nullptr;
  size_t pin_bytes = 0;
  vr_host::EventPtr pin_read;
  // the last launch's kernel time on this context's device (events around the march launch of
  // do_render / a fused channel launch), reported by mem_info; created on first use
  hipEvent_t tev[2] = {nullptr, nullptr};
  bool timed = false;
  // clip planes (vr_set_clip), as the caller gave them; converted per launch (clip_set)
  vr_clip_plane clip[VR_CLIP_MAX] = {};
  int32_t nclip = 0;
  // label volume and gain table (vr_sync_labels, vr_set_label_gains): the labels dense
  // on the device, one byte per voxel, with the identity of the Volume they were uploaded from; the
  // gains as the caller gave them and their device copy.  The versions key DevBuf::mod_labels / mod_gains.
  uint8_t *d_labels = nullptr;
  uint64_t labels_bytes = 0, labels_dims[3] = {0, 0, 0};
  const void *labels_src = nullptr;
  uint64_t labels_last_update = 0;
  int32_t labels_location = VR_HOST;
  uint64_t labels_version = 0;
  float gains[VR_LABEL_GAINS_MAX] = {};
  int32_t ngains = 0;
  uint64_t gains_version = 0;
  float *d_gains = nullptr;
  // slices in flight that read d_labels (vr_render_slice_device's label plane): the label bytes are
  // neither overwritten nor freed before all of them have completed
  vr_host::Readers labels_readers;
  // Gaussian smoothing (vr_set_smoothing): sigma per axis of Data as the caller gave it
  // (all zero: none), the version that keys DevBuf::mod_smooth, and the device copy of the three axes'
  // weights (VR_SMOOTH_MAX_TAPS floats each)
  float smooth_sigma[3] = {0.f, 0.f, 0.f};
  uint64_t smooth_version = 0;
  float *d_smooth_w = nullptr;
  // Richardson-Lucy deconvolution (vr_set_deconvolution): the PSF's sigma per axis of Data,
  // the iteration count (0: none) and the floor as the caller gave them, the version that keys
  // DevBuf::mod_deconv, and the device copy of the three axes' weights
  float deconv_sigma[3] = {0.f, 0.f, 0.f};
  int32_t deconv_iterations = 0;
  float deconv_floor = 0.f;
  uint64_t deconv_version = 0;
  float *d_deconv_w = nullptr;
  // the last derivation's host-clock times (ms), each ending in a stream synchronise: the passes with the
  // statistics read-back, the occupancy rebuild (tools/smooth_bench.py reads them)
  double derive_ms[2] = {0.0, 0.0};
};

namespace vr_host {

// Module-global device state of the reference (volumeRender_kernel.cu:49-120): texture bindings,
// slot indices, gradient method, light list.  Shared by all handles, reset by 'delete'.
struct TexUnit {
  BufPtr bind[T_COUNT];
  int32_t idx_em = T_EM, idx_ab = T_EM, idx_re = T_RE;  // kernel.cu:75-85
  int32_t grad_method = G_COMPUTE;                       // kernel.cu:55
  std::vector<vr::DevLight> lights;                      // c_numLightSources = lights.size(); staged
                                                         // per launch (vr_host::LaunchRec::stage)
  // lookup gradient, interleaved (gx, gy, gz, 0) per padded voxel, built from the bound gradient
  // textures when their dims equal the emission's; rebuilt when any of them changes
  struct GVec {
    std::shared_ptr<DevBuf> buf;
    const DevBuf *src[3] = {nullptr, nullptr, nullptr};
    uint64_t ver[3] = {0, 0, 0};
  };
  std::map<int, GVec> gvec;  // per device (a multi-device group renders on every device)
};

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) VR_HIP(hipSetDevice(dev));
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// The decisions of syncWithDevice (kernel.cu:739-867) over an abstract state, so that the real
// state and vr_debug_slot_transition run the very same code.
template <class S>
void sync_decisions(S &s, bool simEmAb, bool simEmRe, bool simAbRe, bool reqEm, bool reqAb, bool reqRe) {
  bool updEm = false, updAb = false, updRe = false;
  if (reqEm) {
    if (!updEm) { s.upload(T_EM); updEm = true; }
    if (simEmRe && !updRe) { s.reference(T_RE, T_RE, &S::idx_re, T_EM); updRe = true; }
    if (simEmAb && !updAb) { s.reference(T_AB, T_AB, &S::idx_ab, T_EM); updAb = true; }
  }
  if (reqAb) {
    if (!updAb) { s.upload(T_AB); updAb = true; }
    if (simAbRe && !updRe) { s.reference(T_RE, T_RE, &S::idx_re, T_AB); updRe = true; }
    // kernel.cu:817-819 passes the absorption array for the emission texture (unreachable)
    if (simEmAb && !updEm) { s.reference(T_EM, T_AB, &S::idx_em, T_AB); updEm = true; }
  }
  if (reqRe) {
    if (!updRe) { s.upload(T_RE); updRe = true; }
    if (simAbRe && !updAb) { s.reference(T_AB, T_AB, &S::idx_ab, T_RE); updAb = true; }
    // kernel.cu:853-856: the "simEmAb" test guards Emission <- Reflection (reachable)
    if (simEmAb && !updEm) { s.reference(T_EM, T_EM, &S::idx_em, T_RE); updEm = true; }
  }
}

struct DebugState {
  bool present[3] = {true, true, true};
  bool bound[3] = {true, true, true};
  int32_t idx_em, idx_ab, idx_re;
  void upload(int slot) { present[slot] = true; bound[slot] = true; }
  void reference(int tex, int bufslot, int32_t DebugState::*idx, int target) {
    if (present[bufslot]) {
      bound[tex] = false;
      present[bufslot] = false;
    }
    this->*idx = target;
  }
};

// initRender (volumeRender.cpp:112-156) + the per-frame constants of d_render.
struct Frame {
  vr::RenderParams P;
  double drift1[3] = {0, 0, 0};  // staging-halo rounding margin per chunk sample (set_chunk_halo)
  int mode = 0;
  bool ab_alias = false, big = false, share = false;
  uint32_t flags = 0;  // enum vr_launch_flag: what vr_last_launch_flags reports of this frame
  bool degenerate = false;
  vr_context::Schedule *sched_copy = nullptr;  // a timed full-frame launch: copy its durations back
  vr_context::Schedule *sched = nullptr;       // the launch shape's schedule (attach_schedule)
};

// What a launch reads (vr_resources.h), see vr_frame.hip launch_rec
using LaunchRec = LaunchRecOf<BufPtr>;

// ---- shared state (defined in vr_state.hip; nothing elsewhere uses it during static initialisation) ----
extern std::atomic<int> g_test_switches;  // vr_set_option("test_switches"), see test_env
extern uint32_t g_last_launch_flags;      // vr_last_launch_flags: set by build_frame, under g_mu like the frame itself
extern thread_local std::string g_last_error;
extern std::mutex g_mu;
extern TexUnit &g_tex;
extern std::set<vr_context *> g_contexts;

// ---- vr_state.hip ----
int fail(int code, const std::string &msg);
uint64_t next_version();
bool valid(vr_context *h);
bool env_flag(const char *name);
bool env_flag_off(const char *name);
const char *diag_env(const char *name);
bool diag_flag(const char *name);
const char *test_env(const char *name);
bool test_flag(const char *name);
bool test_flag_off(const char *name);
hipError_t take_stream(int dev, hipStream_t *s);
void give_stream(int dev, hipStream_t s);

// ---- vr_sync.hip ----
bool same(const VolRec &a, const VolRec &b);
VolRec make_rec(const vr_volume *v);
int check_dtype(const vr_volume *v, bool fp32_only, const char *what);
void sync_volume_if_changed(vr_context *h, int tex, int slot);
uint64_t required_memory(const vr_context *h);
int check_free_device_memory(uint64_t required);
BufPtr label_target(const vr_context *h);
int check_label_dims(const uint64_t ld[3], const DevBuf *b);
int apply_derived(vr_context *h);
bool smoothing_set(const vr_context *h);
int check_smoothing(const float sigma[3]);
int smoothing_unsupported(const char *what);
bool deconvolution_set(const vr_context *h);
int check_deconvolution(const float sigma[3], int32_t iterations, float flr);
int deconvolution_unsupported(const char *what);
void free_labels(vr_context *h);
int labels_unsupported(const char *what);
int check_label_gains(const float *gains, int32_t n);
int do_sync_volumes(vr_context *h, uint64_t time_last_mem_sync, const vr_volume *emission,
                    const vr_volume *reflection, const vr_volume *absorption, const vr_volume *dx,
                    const vr_volume *dy, const vr_volume *dz);

// ---- vr_frame.hip ----
vr::DevTex dev_tex(const BufPtr &b);
bool is_big(const vr::DevTex &t);
int32_t half_texel_taps(const vr::RenderParams &P, int mode, float fnz);
int check_clip(const vr_clip_plane *planes, int32_t n);
void convert_clip(const vr_clip_plane &p, const float bmin[3], const float bscale[3], float out[4]);
vr::ClipSet clip_set(const vr_context *h, const vr::RenderParams &P);
int clip_unsupported(const char *what);
void drift_bound(Frame &F, const float *eye2);
int build_frame(vr_context *h, const vr_render_args *a, Frame &F, uint64_t depth_override = 0);
void upload_lights(vr_context *h, const vr_render_args *a);
int check_lights(const vr_render_args *a);
int check_and_upload_lights(vr_context *h, const vr_render_args *a, uint64_t *required = nullptr);
void wait_ready(const BufPtr &b, hipStream_t s);
LaunchRec launch_rec(const vr_context *h, hipStream_t stream);
void stage_frame(LaunchRec &L, vr::RenderParams &P, const std::vector<vr::DevLight> &lights);
int64_t part_columns(int64_t w, int32_t bc, int32_t part, int32_t np);
int validate_partition(const vr_partition *p);
void set_partition(vr::RenderParams &P, const vr_partition *part, float *d_out, unsigned long long *d_steps);
int chunk_samples(int K);
void set_chunk_halo(Frame &F, int K);
void free_schedules(vr_context *h);
int depth_lanes(const vr::RenderParams &P);
void set_tau_and_slot(vr::RenderParams &P, const vr_render_args *a, double vw);
bool short_launch(const vr::RenderParams &P);
bool want_schedule(const vr::RenderParams &P);
hipError_t attach_schedule(vr_context *h, vr::RenderParams &P, Frame &F, int K, hipStream_t stream,
                           const char *extra);

// ---- vr_render.hip ----
void free_views(vr_context *h);
int do_render(vr_context *h, const vr_render_args *a, const vr_partition *part, float *d_out,
              unsigned long long *d_steps, hipStream_t stream, Frame &F, float *d_out2 = nullptr,
              const float *eye2 = nullptr, int *fusable = nullptr);
int do_render_slab(vr_context *h, const vr_render_args *a, const vr_slab *sl, const vr_partition *part,
                   const float *d_in, float *d_out, hipStream_t stream, Frame &F);
bool enable_peer(int a, int b);
void group_sync(vr_context *h);
int group_render(vr_context *h, const vr_render_args *a, float *d_out, hipStream_t stream, float *d_out2 = nullptr,
                 const float *eye2 = nullptr);
void delete_children(vr_context *h);
int do_render_channels(const vr_channel *ch, int32_t n, int32_t stereo, float base, float *d_out,
                       hipStream_t stream);

// ---- vr_features.hip ----
int do_project(vr_context *h, const vr_render_args *a, int32_t mode, const vr_partition *part, float *d_out,
               float *d_aux, unsigned long long *d_steps, hipStream_t stream);
int check_slice(const vr_slice *s);
int do_slice(vr_context *h, const vr_slice *s, float *d_out, float *d_aux, float *d_lab, hipStream_t stream);
int check_hist_bins(int32_t nbins, const float lim[2]);
int check_histogram(const vr_histogram *q);
int32_t histogram_rows(const vr_histogram *q);
int do_histogram(vr_context *h, const vr_histogram *q, unsigned long long *d_counts, vr_hist_row *d_rows,
                 hipStream_t stream);
int do_isosurface(vr_context *h, const vr_render_args *a, float level, const vr_partition *part, float *d_out,
                  float *d_depth, float *d_normal, unsigned long long *d_steps, hipStream_t stream);
int check_transfer(const vr_transfer *tf);
float transfer_lookup(const float *T, int32_t n, const float lim[2], float c);
int do_transfer(vr_context *h, const vr_render_args *a, const vr_transfer *tf, const vr_partition *part, float *d_out,
                float *d_alpha, unsigned long long *d_steps, hipStream_t stream);

}  // namespace vr_host

// At entry, an error already in this thread's HIP error state (another library's, or an
// asynchronous device fault) is logged, and a device fault fails the call (vr_host::check_pending):
// this call's own checks then see only its own errors.
#define VR_GUARD_BEGIN \
  try {                \
    vr_host::check_pending(__func__);
#define VR_GUARD_END                                                                             \
  }                                                                                              \
  catch (const HipError &e) {                                                                    \
    return fail(VR_ERR_DEVICE, std::string(hipGetErrorString(e.e)) + " in " + e.what);           \
  }                                                                                              \
  catch (const std::bad_alloc &) {                                                               \
    return fail(VR_ERR_DEVICE, "host out of memory");                                            \
  }
// The preamble of a single-handle entry, after its lock and its own argument checks (which win over
// these): the handle, the arguments `a`, one device; then the guard opens on the handle's device and
// buffers whose last launch has completed are released.  Closed by VR_GUARD_END.
#define VR_ENTRY_BEGIN(h, a)                                                                        \
  if (!valid(h)) return fail(VR_ERR_HANDLE, "Handle not valid.");                                   \
  if (!(a)) return fail(VR_ERR_ARGUMENT, "insufficient parameter!");                                \
  if (!(h)->children.empty())                                                                       \
    return fail(VR_ERR_UNSUPPORTED, std::string(__func__) + ": one-device handles only");           \
  VR_GUARD_BEGIN                                                                                    \
  DeviceGuard dg((h)->device);                                                                      \
  vr_host::prune_retired();
