// vr_render.hip -- the render command (vr_host.h): the reference's host render driver vr/
// volumeRender.cpp:112-300 as do_render, the sort-last slab render, the multi-device group and the
// fused view sets of the multi-channel render.
#include "vr_host.h"

namespace vr_host {

// Launch timing for mem_info (the context's device must be current).
static void time_mark(vr_context *h, int which, hipStream_t stream) {
  if (!h->tev[0]) {
    hipError_t e = hipEventCreate(&h->tev[0]);
    if (e == hipSuccess) e = hipEventCreate(&h->tev[1]);
    if (e != hipSuccess) {
      vr_host::consume(e, "hipEventCreate (mem_info kernel timing; not timed)");
      return;
    }
  }
  const hipError_t e = hipEventRecord(h->tev[which], stream);
  if (e != hipSuccess) vr_host::consume(e, "hipEventRecord (mem_info kernel timing; not timed)");
  if (which == 1) h->timed = true;
}

void free_views(vr_context *h) {
  if (h->d_chan) (void)hipFree(h->d_chan);
  h->d_chan = nullptr;
  h->d_chan_bytes = 0;
}

// The render command proper (render.cpp:134-259 minus the mxArray plumbing).
// d_out2 / eye2 (optional): fused stereo -- the same frame seen from a second eye position, into a
// second image, in the same launch (vr_render_stereo).
// fusable (optional, vr_render_channels): a frame the multi-view march can take (staged march,
// gradient mode 0/1, 32-bit addressing) is only prepared -- F.P complete, *fusable = 1, nothing
// launched; any other frame is rendered here as usual and *fusable = 0.
int do_render(vr_context *h, const vr_render_args *a, const vr_partition *part, float *d_out,
              unsigned long long *d_steps, hipStream_t stream, Frame &F, float *d_out2,
              const float *eye2, int *fusable) {
  if (fusable) *fusable = 0;
  uint64_t required = 0;
  int rc = check_and_upload_lights(h, a, &required);
  if (rc) return rc;
  required += a->resolution[0] * a->resolution[1] * sizeof(float) * 3;
  rc = check_free_device_memory(required);
  if (rc) return rc;
  rc = build_frame(h, a, F);
  if (rc) return rc;
  rc = validate_partition(part);
  if (rc) return rc;
  vr::RenderParams &P = F.P;
  set_partition(P, part, d_out, d_steps);
  P.lookup = F.mode == 2 ? 1 : 0;
  set_tau_and_slot(P, a, (double)h->vol[T_EM].dims[0]);  // depth lanes and wave slot size
  // shading arithmetic: hardware rsq / exp2 by default; VR_EXACT_SHADE=1 selects
  // the oracle's correctly rounded op sequence (bit-identical to oracle/vr_oracle.c up to acosf)
  P.fast_shade = env_flag("VR_EXACT_SHADE") ? 0 : 1;
  if (const char *ev = test_env("VR_TILE_MODE")) P.tile_mode = std::atoi(ev) ? 1 : 0;  // A/B switch
  // XCD runs of 16 blocks for lookup-gradient frames (their gathers of the gradient copy are the
  // launch's HBM traffic: C3 36.4 -> 35.7 ms, round 4); the compute-gradient march is indifferent
  P.xcd_run = F.mode == 2 ? 32 : VR_XCD_RUN;  // (round 5: 32 / 16 -> 31.24-31.26 / 31.43-31.67 ms, r5p)
  if (const char *ev = test_env("VR_XCD_RUN")) P.xcd_run = std::max(0, std::atoi(ev));  // A/B switch
  P.block_rot = 0;  // set at the launch (block rows of the launch's depth lanes)
  const size_t out_bytes = (size_t)P.plane_cols * (size_t)P.height * 3 * sizeof(float);
  if (d_out2) {
    P.views = 2;
    P.out2 = d_out2;
    for (int i = 0; i < 3; ++i) P.eye2[i] = eye2[i];
    drift_bound(F, eye2);  // the staging halo covers the second eye's rays too
  }
  if (F.degenerate) {
    if (out_bytes) VR_HIP(hipMemsetAsync(d_out, 0, out_bytes, stream));
    if (out_bytes && d_out2) VR_HIP(hipMemsetAsync(d_out2, 0, out_bytes, stream));
    return VR_OK;
  }
  // LDS-staged march (vr_march.hip) whenever the emission texture is a real grid and, for the
  // on-the-fly gradient, is also the gradient texture; the plain kernel covers everything else.
  // Both produce bit-identical images (tests/test_gpu_parity.py::test_kernel_variants...).
  // Clip planes (vr_set_clip) go through the general kernel: the staged march knows nothing of them.
  const vr::ClipSet clip = clip_set(h, P);
  const bool march = P.em.p && !P.em.one && (F.mode != 1 || F.share) && !test_flag("VR_NO_LDS") && clip.n == 0;
  P.gvec = nullptr;
  if (march && F.mode == 2 && F.share && !test_flag("VR_NO_GVEC")) {
    // interleave the three gradient textures (one 16-byte load per voxel instead of three 4-byte
    // gathers from three volumes); without memory for it the kernel gathers them separately
    const BufPtr &bx = g_tex.bind[T_DX], &by = g_tex.bind[T_DY], &bz = g_tex.bind[T_DZ];
    TexUnit::GVec &G = g_tex.gvec[h->device];
    const uint32_t gpx = P.gx.px, gpy = P.gx.pxy / P.gx.px, gpz = (uint32_t)P.gx.nz + 2u;
    bool fresh = G.buf != nullptr;
    const DevBuf *src[3] = {bx.get(), by.get(), bz.get()};
    for (int i = 0; i < 3 && fresh; ++i) fresh = G.src[i] == src[i] && G.ver[i] == src[i]->version;
    if (!fresh) {
      G.buf.reset();
      const uint64_t n = vr::interleave3_entries(gpx, gpy, gpz);
      auto gv = std::make_shared<DevBuf>();
      gv->device = h->device;
      gv->bytes = n * 4 * sizeof(float);
      const hipError_t ea = vr_host::pooled_alloc(reinterpret_cast<void **>(&gv->ptr), gv->bytes, h->device);
      if (ea == hipSuccess) {
        for (const BufPtr *b : {&bx, &by, &bz}) wait_ready(*b, stream);
        VR_HIP(vr::launch_interleave3(bx->ptr, by->ptr, bz->ptr, gv->ptr, gpx, gpy, gpz, stream));
        // launches on other streams (another handle, a group's other children on this device) find
        // the copy fresh and wait for this event before reading it (bind_reads)
        VR_HIP(vr_host::record_event(stream, gv->ready));
        G.buf = gv;
        for (int i = 0; i < 3; ++i) {
          G.src[i] = src[i];
          G.ver[i] = src[i]->version;
        }
      } else {
        vr_host::consume(ea, "pooled_alloc (interleaved lookup gradient; three separate gathers instead)");
        gv->ptr = nullptr;
      }
    }
    if (G.buf) {
      P.gvec = G.buf->ptr;
      P.gv_row8 = 8u * ((gpx + 1) >> 1);
      P.gv_plane8 = P.gv_row8 * ((gpy + 1) >> 1);
    }
  }
  if (fusable && march && F.mode <= 1 && !F.big && !P.steps) {
    *fusable = 1;
    return VR_OK;
  }
  LaunchRec L = launch_rec(h, stream);
  stage_frame(L, P, g_tex.lights);
  if (march) {
    // the counter variant: K = 1 (VR_COUNT_PROD=1 with a VR_COUNT_K=1 build: the production K's chunk
    // statistics; its sample sums are then 0)
    // (VR_COUNT_PROD is honoured by a VR_COUNT_K build only: a normal build has no counted K > 1 kernel)
    const int K = (P.steps && !(VR_COUNT_K && test_flag("VR_COUNT_PROD"))) ? 1
                                                                          : exact_lanes(depth_lanes(P), P.fast_shade);
    set_chunk_halo(F, K);
    const MarchEntries &M = march_entries(P.fast_shade != 0, K);
    // (the exact-arithmetic variant is a parity reference: built without the scheduled kernels)
    // (scheduled kernels exist for absorption = emission only: vr_march.hip launch_c)
    if (!P.steps && K > 1 && P.fast_shade && F.ab_alias && want_schedule(P))
      VR_HIP(attach_schedule(h, P, F, K, stream, ""));
    if (P.views > 1) {
      P.view_blocks = M.blocks(P);
      // VR_STEREO_PAIR=1 (measurement): paired tiles -- the left eye's rays of
      // column c + shift share a wave (and its staged box) with the right eye's of column c, the
      // shift (whole tiles) making the two bundles meet at the volume's centre, at distance `dist`
      // from the eyes: base * W * f / dist columns
      if (test_flag("VR_STEREO_PAIR") && K > 1 && P.fast_shade && F.mode == 1 && F.ab_alias && P.tap_half &&
          !P.wide_slot && !F.big && P.num_parts == 1 && !P.wg_order) {
        const double base = std::fabs((double)a->props[0]), f = std::fabs((double)a->props[1]),
                     dist = std::fabs((double)a->props[2]);
        const int TW = M.tile_w;
        const double cols = dist > 0 ? base * (double)P.width * f / dist : 0.0;
        P.pair_shift = (int32_t)std::min<double>(std::floor(cols / TW + 0.5) * TW, (double)P.width);
        if (const char *ev = test_env("VR_STEREO_PAIR_SHIFT")) P.pair_shift = std::max(0, std::atoi(ev));
      }
    }
    // diagnostics (VR_SCHED_DUMP): a timed launch also records its blocks' start ticks
    const char *dump = (P.wg_cost && P.sched_full != 2) ? test_env("VR_SCHED_DUMP") : nullptr;
    uint32_t *d_start = nullptr;
    if (dump) {
      const hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_start), (size_t)P.sched_blocks * 4);
      if (e == hipSuccess) P.wg_start = d_start;
      else vr_host::consume(e, "hipMalloc (VR_SCHED_DUMP start ticks; not recorded)");
    }
    // VR_BLOCK_ROT_ROWS=r (A/B): the unscheduled launch starts at block row r of the row-major order
    // and wraps (the light top rows then fill the ramp-down of the heavy middle band)
    if (const char *ev = test_env("VR_BLOCK_ROT_ROWS")) {
      const uint32_t nbx = (uint32_t)((P.part_cols + 2 * M.tile_w - 1) / (2 * M.tile_w));
      const uint32_t nb = M.blocks(P) * (P.views > 1 ? 2u : 1u);
      const uint64_t rot = (uint64_t)std::max(0, std::atoi(ev)) * nbx;
      P.block_rot = nb ? (uint32_t)(rot % nb) : 0u;
    }
    // the pre-leap launch (vr_march.hip preleap_kernel, round 6): scheduled tame launches with an
    // occupancy map; its buffers live with the launch shape's schedule (one per stream)
    if (VR_PRELEAP_LAUNCH && F.sched && F.sched->blocks && P.occ && P.tame && !P.pair_shift && P.fast_shade &&
        !test_flag("VR_NO_PRELEAP")) {
      vr_context::Schedule &S = *F.sched;
      const uint32_t waves = S.blocks * (uint32_t)VR_WG_WAVES_HOST;
      if (S.pre_waves != waves) {
        if (S.pre_flag) (void)hipFree(S.pre_flag);
        if (S.pre_state) (void)hipFree(S.pre_state);
        S.pre_flag = nullptr;
        S.pre_state = nullptr;
        S.pre_waves = S.pre_cap = 0;
        const uint32_t cap = std::max<uint32_t>(64u, waves / 8u);  // slots: an eighth of the waves
        hipError_t e = S.pre_count ? hipSuccess : hipMalloc(reinterpret_cast<void **>(&S.pre_count), 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&S.pre_flag), (size_t)waves * 4);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&S.pre_state), (size_t)cap * 64 * 2 * sizeof(float4));
        if (e == hipSuccess) {
          S.pre_waves = waves;
          S.pre_cap = cap;
        } else {
          vr_host::consume(e, "hipMalloc (pre-leap buffers; the launch marches without)");
        }
      }
      if (S.pre_waves == waves) {
        P.pre_flag = S.pre_flag;
        P.pre_state = S.pre_state;
        P.pre_count = S.pre_count;
        P.pre_cap = S.pre_cap;
        VR_HIP(hipMemsetAsync(S.pre_count, 0, 4, stream));
        VR_HIP(M.preleap(P, stream));
      }
    }
    time_mark(h, 0, stream);
    {
      const hipError_t e = M.launch(P, F.mode, F.ab_alias, F.share, F.big, stream);
      if (e != hipSuccess) throw HipError{e, "the march kernel launch (launch_march_k)"};
    }
    time_mark(h, 1, stream);
    if (F.sched_copy) {  // a timed full frame: its block durations to the host, for the tail test
      vr_context::Schedule &S = *F.sched_copy;
      VR_HIP(hipMemcpyAsync(S.h_cost, S.d_cost, (size_t)S.blocks * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
      VR_HIP(hipEventRecord(S.copied, stream));
      S.copy_pending = true;
      F.sched_copy = nullptr;
    }
    if (dump) {  // diagnostics: append block durations (and, in DUMP.start, their start ticks)
      std::vector<uint32_t> c(P.sched_blocks), st(d_start ? P.sched_blocks : 0);
      VR_HIP(hipMemcpyAsync(c.data(), P.wg_cost, c.size() * 4, hipMemcpyDeviceToHost, stream));
      if (d_start) VR_HIP(hipMemcpyAsync(st.data(), d_start, st.size() * 4, hipMemcpyDeviceToHost, stream));
      VR_HIP(hipStreamSynchronize(stream));
      if (d_start) (void)hipFree(d_start);
      const uint32_t hdr[4] = {(uint32_t)K, (uint32_t)P.part, (uint32_t)P.num_parts, P.sched_blocks};
      if (FILE *f = std::fopen(dump, "ab")) {
        std::fwrite(hdr, 4, 4, f);
        std::fwrite(c.data(), 4, c.size(), f);
        std::fclose(f);
      }
      if (d_start)
        if (FILE *f = std::fopen((std::string(dump) + ".start").c_str(), "ab")) {
          std::fwrite(hdr, 4, 4, f);
          std::fwrite(st.data(), 4, st.size(), f);
          std::fclose(f);
        }
    }
  } else {
    VR_HIP(vr::launch_render(P, F.mode, F.ab_alias, F.big, F.share, stream, &clip));
    if (P.views > 1) {  // the general kernel renders one view per launch
      for (int i = 0; i < 3; ++i) P.eye[i] = P.eye2[i];
      P.out = P.out2;
      VR_HIP(vr::launch_render(P, F.mode, F.ab_alias, F.big, F.share, stream, &clip));
    }
  }
  VR_HIP(L.finish());
  return VR_OK;
}

// Sort-last slab render: the handle's emission volume holds planes
// [z_first, z_first + d2) of a volume of depth `depth`; the frame is built for the whole volume
// (box, step, gradient offsets) and the march takes the samples of [z0, z1) only.
int do_render_slab(vr_context *h, const vr_render_args *a, const vr_slab *sl, const vr_partition *part,
                   const float *d_in, float *d_out, hipStream_t stream, Frame &F) {
  if (!sl || !d_out) return fail(VR_ERR_ARGUMENT, "slab / output is NULL");
  if (sl->depth == 0 || sl->z_first >= sl->depth || (sl->direction < -1 || sl->direction > 1))
    return fail(VR_ERR_ARGUMENT, "invalid slab");
  int rc = check_lights(a);  // (the argument checks alone: a slab render makes no memory check)
  if (rc) return rc;
  upload_lights(h, a);
  rc = build_frame(h, a, F, sl->depth);
  if (rc) return rc;
  vr::RenderParams &P = F.P;
  if (F.degenerate || !P.em.p || P.em.one) return fail(VR_ERR_UNSUPPORTED, "slab render needs a synced emission volume");
  // the planes resident are those of the BOUND emission texture (the last sync_volumes of any
  // handle, as every render reads -- render.cpp binds globally); the slab must lie inside them
  const uint64_t res_nz = (uint64_t)P.em.nz, res_nx = (uint64_t)P.em.nx;
  if (sl->z_first + res_nz > sl->depth) return fail(VR_ERR_ARGUMENT, "invalid slab: bound planes exceed the depth");
  if (F.mode == 2 || !F.ab_alias) return fail(VR_ERR_UNSUPPORTED, "slab render: lookup gradients / separate absorption");
  // the resident planes addressed by their global padded index: virtual base z_first planes back
  const bool re_em = P.re_is_em != 0;
  P.occ = nullptr;  // (the probe is not used by the slab march; the map would be the slab's own)
  P.em.p = P.em.p - (ptrdiff_t)(sl->z_first * (uint64_t)P.em.pxy);
  P.em.nz = (int32_t)sl->depth;
  P.em.fnz = (float)sl->depth;
  P.gem = P.em;
  if (re_em) P.re = P.em;
  P.ab = P.em;
  // resident padded planes holding the right data: the synced planes, plus the edge-replicating
  // apron planes only at the ends of the whole volume
  P.slab_pk0 = (int32_t)(sl->z_first + (sl->z_first > 0 ? 1 : 0));
  P.slab_pk1 = (int32_t)(sl->z_first + res_nz + 1 + (sl->z_first + res_nz == sl->depth ? 1 : 0));
  const double D = (double)sl->depth;
  P.slab_z0 = std::isfinite(sl->z0) ? (float)(sl->z0 / D) : -INFINITY;
  P.slab_z1 = std::isfinite(sl->z1) ? (float)(sl->z1 / D) : INFINITY;
  // the z halo of build_frame was sized by the resident depth: redo it for the whole volume
  {
    double pmax = 0.0;
    for (int i = 0; i < 3; ++i) pmax = std::max(pmax, (double)std::fabs(P.bmin[i]) + std::fabs(P.eye[i]));
    F.drift1[2] = 2.0 * pmax * 1.2e-7 * (double)P.bscale[2] * D;
    P.tap_off[2] = (float)((F.mode == 1 ? (double)P.gstep[2] * P.bscale[2] * D : 0.0) + 0.0625);
    P.tap_half = half_texel_taps(P, F.mode, (float)D);  // judged on the whole volume, as one render
    for (int i = 0; i < 3; ++i)  // (the cube's n / 2 per axis, the whole volume's depth on z)
      P.cube_hs[i] = P.tap_half ? (i == 0 ? P.em.fnx : i == 1 ? P.em.fny : (float)D) * 0.5f : 0.f;
    g_last_launch_flags = F.flags = (F.flags & ~(uint32_t)VR_LF_TAP_HALF) | (P.tap_half ? VR_LF_TAP_HALF : 0u);
  }
  P.slab_dir = sl->direction;
  P.slab_in = d_in;
  rc = validate_partition(part);
  if (rc) return rc;
  set_partition(P, part, d_out, nullptr);
  P.plane_cols = P.part_cols;  // the state of a part is dense: VR_SLAB_PLANES [part_cols][H] planes
  if ((uint64_t)P.part_cols * (uint64_t)P.height >= (1ull << 32))
    return fail(VR_ERR_UNSUPPORTED, "slab render: more than 2^32 rays in one part");
  P.fast_shade = env_flag("VR_EXACT_SHADE") ? 0 : 1;
  // depth lanes (and slot) as for the one-volume march of the whole frame: the tiles of a sweep run
  // back to back and overlap on the sweep's streams, so one tile's launch tail is not the frame's
  // (4 tiles on one MI355X: 1.25x the plain render at the frame's K = 2, 1.36x at a tile's K = 4)
  const int32_t tile_cols = P.part_cols;
  P.part_cols = P.width;
  set_tau_and_slot(P, a, (double)res_nx);
  int K = depth_lanes(P);
  P.part_cols = tile_cols;
  if (K > 4) K = 4;
  K = exact_lanes(K, P.fast_shade);
  set_chunk_halo(F, K);
  P.slab_margin = P.tap_off[2] / P.em.fnz;  // bound of the chunk ownership test, normalized
  LaunchRec L = launch_rec(h, stream);
  stage_frame(L, P, g_tex.lights);
  if (K > 1 && want_schedule(P) && short_launch(P)) {  // a tile of a sweep: longest-first schedule
    char extra[120];
    std::snprintf(extra, sizeof extra, "slab/%llu/%llu/%g/%g/%d", (unsigned long long)sl->depth,
                  (unsigned long long)sl->z_first, sl->z0, sl->z1, sl->direction);
    VR_HIP(attach_schedule(h, P, F, K, stream, extra));
  }
  VR_HIP(march_entries(P.fast_shade != 0, K).launch_slab(P, F.mode, stream));
  VR_HIP(L.finish());
  return VR_OK;
}

// ---- multi-device group (vr_new_multi) ----------------------------------------------------------

// A device-to-device copy through pinned host memory, for device pairs without a peer mapping: the
// D2H is issued on `ss` (a stream of sdev) -- synchronously when ss is null --, the H2D on `ds` (a
// stream of ddev) after it.  Through the caller's pinned buffer `stage` (which the caller keeps
// until the H2D has completed), or through one allocated here and released when the H2D has
// completed (or at once if a call fails).  Returns the completion event of the H2D.
static vr_host::EventPtr staged_copy(void *dst, int ddev, hipStream_t ds, const void *src, int sdev, hipStream_t ss,
                              size_t bytes, void *stage = nullptr) {
  struct Own {  // the buffer allocated here, freed on an error path
    void *p = nullptr;
    ~Own() {
      if (p) (void)hipHostFree(p);
    }
  } own;
  void *pin = stage;
  if (!pin) {
    VR_HIP(hipHostMalloc(&own.p, bytes, hipHostMallocDefault));
    pin = own.p;
  }
  vr_host::EventPtr e1, e2;
  {
    DeviceGuard g(sdev);
    if (ss) {
      VR_HIP(hipMemcpyAsync(pin, src, bytes, hipMemcpyDeviceToHost, ss));
      VR_HIP(vr_host::record_event(ss, e1));
    } else {
      VR_HIP(hipMemcpy(pin, src, bytes, hipMemcpyDeviceToHost));
    }
  }
  DeviceGuard g(ddev);
  if (e1) VR_HIP(hipStreamWaitEvent(ds, e1->e, 0));
  VR_HIP(hipMemcpyAsync(dst, pin, bytes, hipMemcpyHostToDevice, ds));
  VR_HIP(vr_host::record_event(ds, e2));
  if (own.p) {
    vr_host::free_when_done(own.p, ddev, vr_host::readers_of(e2), true);
    own.p = nullptr;
  }
  return e2;
}

// The copy of buffer b on device `dev`, refreshed when b was re-uploaded since (peer copy over xGMI on
// the device's group stream; a replica a launch still reads is replaced, not overwritten).
static BufPtr replicate(const BufPtr &b, int dev, hipStream_t s, bool peer = true) {
  if (!b) return b;
  if (b->device == dev && !test_flag("VR_GROUP_REPLICATE")) return b;  // test switch: copy on one device too
  BufPtr &r = b->replicas[dev];
  if (r && r->bytes == b->bytes && b->replica_of[dev] == b->version) return r;
  if (!(r && r->bytes == b->bytes && r->readers.done())) {
    r = std::make_shared<DevBuf>();
    r->device = dev;
    r->bytes = b->bytes;
    if (b->bytes) {
      DeviceGuard dg(dev);
      VR_HIP(vr_host::pooled_alloc(reinterpret_cast<void **>(&r->ptr), b->bytes, dev));
    }
  }
  if (b->bytes) {
    vr_host::EventPtr ev;
    if (peer) {
      VR_HIP(hipMemcpyPeerAsync(r->ptr, dev, b->ptr, b->device, b->bytes, s));
      // the occupancy map along with it (peer copies only; a staged replica marches without probes)
      if (b->occ && r->occ_bytes != b->occ_bytes) {
        if (r->occ) vr_host::pooled_free(r->occ, r->occ_bytes, dev, vr_host::Readers(r->readers));
        r->occ = nullptr;
        r->occ_bytes = 0;
        DeviceGuard dg(dev);
        VR_HIP(vr_host::pooled_alloc(reinterpret_cast<void **>(&r->occ), b->occ_bytes, dev));
        r->occ_bytes = b->occ_bytes;
      }
      if (b->occ) VR_HIP(hipMemcpyPeerAsync(r->occ, dev, b->occ, b->device, b->occ_bytes, s));
      VR_HIP(vr_host::record_event(s, ev));
    }
    if (!(peer && b->occ) && r->occ) {  // no map copied: none (a stale one would leap wrongly)
      vr_host::pooled_free(r->occ, r->occ_bytes, dev, vr_host::Readers(r->readers));
      r->occ = nullptr;
      r->occ_bytes = 0;
    }
    if (!peer) {  // no peer mapping: through pinned host memory (b is resident: its D2H runs now)
      if (b->ready) vr_host::wait(b->ready);
      ev = staged_copy(r->ptr, dev, s, b->ptr, b->device, nullptr, b->bytes);
    }
    // the copy reads b and writes r: neither is rewritten, pooled or freed before it completes
    b->readers.add(ev);
    r->readers.add(ev);
    r->ready = ev;
  }
  for (int i = 0; i < 3; ++i) r->dims[i] = b->dims[i];
  r->nonfinite = b->nonfinite;
  r->maxabs = b->maxabs;
  r->src_data = b->src_data;
  r->src_last_update = b->src_last_update;
  r->src_bytes = b->src_bytes;
  r->src_dtype = b->src_dtype;
  r->version = next_version();
  b->replica_of[dev] = b->version;
  return r;
}

// Whether device a may map b's memory (the mapping enabled); false: copies between them are staged
// through pinned host memory (staged_copy).
bool enable_peer(int a, int b) {
  if (a == b) return true;
  int ok = 0;
  const hipError_t q = hipDeviceCanAccessPeer(&ok, a, b);
  if (q != hipSuccess) {
    vr_host::consume(q, "hipDeviceCanAccessPeer (group peer mapping; copies staged through the host)");
    return false;
  }
  if (!ok) return false;
  DeviceGuard dg(a);
  const hipError_t e = hipDeviceEnablePeerAccess(b, 0);
  if (e == hipSuccess) return true;
  vr_host::consume(e, "hipDeviceEnablePeerAccess (group peer mapping)");
  return e == hipErrorPeerAccessAlreadyEnabled;
}

// After a sync of the primary: the children record the same volumes, and the bound volumes are
// copied to their devices now (one H2D to the primary, then peer copies), not in the render.
void group_sync(vr_context *h) {
  for (vr_context *c : h->children) {
    DeviceGuard dg(c->device);
    for (int t = 0; t < T_COUNT; ++t) c->vol[t] = h->vol[t];
    c->time_last_mem_sync = h->time_last_mem_sync;
    for (int t = 0; t < T_COUNT; ++t)
      if (t != T_LIGHT && g_tex.bind[t]) (void)replicate(g_tex.bind[t], c->device, c->gstream, c->peer);
  }
}

// Part buffers of a group frame of `nviews` images: the primary's h->d_part holds every device's
// parts view-major (view v, device k at (v * n + k) * part_floats: one view's parts are contiguous,
// as vr_assemble_partitions reads them); a child's d_part its own nviews parts.
static void ensure_part_buffers(vr_context *h, int n, size_t part_floats, int nviews) {
  const size_t pb = (size_t)n * (size_t)nviews * part_floats * sizeof(float);
  if (h->d_part_bytes < pb) {
    if (h->d_part) VR_HIP(hipFree(h->d_part));
    h->d_part = nullptr;
    h->d_part_bytes = 0;
    VR_HIP(vr_host::device_alloc(reinterpret_cast<void **>(&h->d_part), pb));
    h->d_part_bytes = pb;
  }
  for (vr_context *c : h->children) {
    DeviceGuard dg(c->device);
    const size_t cb = (size_t)nviews * part_floats * sizeof(float);
    if (c->d_part_bytes < cb) {
      if (c->d_part) VR_HIP(hipFree(c->d_part));
      c->d_part = nullptr;
      c->d_part_bytes = 0;
      VR_HIP(vr_host::device_alloc(reinterpret_cast<void **>(&c->d_part), cb));
      c->d_part_bytes = cb;
    }
  }
}

// Bind, for a render on child c, the replicas of the primary's bindings `saved` on c's device (the
// LUT is c's own upload, which do_render keeps resident).
static void bind_replicas(vr_context *h, vr_context *c, const BufPtr (&saved)[T_COUNT]) {
  for (int t = 0; t < T_COUNT; ++t) c->vol[t] = h->vol[t];
  for (int t = 0; t < T_COUNT; ++t)
    g_tex.bind[t] = t == T_LIGHT ? c->buf[T_LIGHT] : replicate(saved[t], c->device, c->gstream, c->peer);
}

// Gather every child's parts (nviews images each) into the primary's part buffer over xGMI and
// assemble each view into d_outs[v] on the primary's `stream`.
static void group_gather_assemble(vr_context *h, int nviews, size_t part_floats, int64_t W, int64_t H, int32_t bc,
                           int64_t maxc, float *const *d_outs, hipStream_t stream) {
  const int n = 1 + (int)h->children.size();
  for (int k = 1; k < n; ++k) {
    vr_context *c = h->children[k - 1];
    DeviceGuard dg(c->device);
    // the previous frame's assembly has read these slots of the primary's part buffer
    VR_HIP(hipStreamWaitEvent(c->gstream, h->gdone, 0));
    if (c->peer) {
      for (int v = 0; v < nviews; ++v)
        VR_HIP(hipMemcpyPeerAsync(h->d_part + ((size_t)v * n + k) * part_floats, h->device,
                                  c->d_part + (size_t)v * part_floats, c->device, part_floats * sizeof(float),
                                  c->gstream));
    } else {  // no peer mapping: D2H on the child's stream, H2D on the primary's (after the previous
              // frame's assembly, which read these slots, in that stream's order), through the
              // child's persistent pinned buffer (its previous contents read by that assembly's H2Ds)
      const size_t vb = part_floats * sizeof(float);
      if (c->pin_bytes < (size_t)nviews * vb) {
        if (c->pin) vr_host::free_when_done(c->pin, c->device, vr_host::readers_of(c->pin_read), true);
        c->pin = nullptr;
        c->pin_bytes = 0;
        c->pin_read.reset();
        VR_HIP(hipHostMalloc(&c->pin, (size_t)nviews * vb, hipHostMallocDefault));
        c->pin_bytes = (size_t)nviews * vb;
      }
      for (int v = 0; v < nviews; ++v)
        c->pin_read = staged_copy(h->d_part + ((size_t)v * n + k) * part_floats, h->device, stream,
                                  c->d_part + (size_t)v * part_floats, c->device, c->gstream, vb,
                                  static_cast<char *>(c->pin) + (size_t)v * vb);
    }
    VR_HIP(hipEventRecord(c->gdone, c->gstream));
  }
  for (vr_context *c : h->children) VR_HIP(hipStreamWaitEvent(stream, c->gdone, 0));
  for (int v = 0; v < nviews; ++v)
    VR_HIP(vr::launch_assemble(h->d_part + (size_t)v * n * part_floats, W, H, bc, n, maxc, d_outs[v], stream));
  VR_HIP(hipEventRecord(h->gdone, stream));
}

// 'render' on a group: child k renders column part k (16-column blocks dealt round-robin, as
// bench.py's ranks), the primary part 0; the children's parts are peer-copied into the primary's
// part buffer and assembled there into d_out (the primary's device, on `stream`).  With d_out2 /
// eye2 every device renders its part of both eyes of a stereo pair (vr_render_stereo) in one launch.
// The module-global bindings are the primary's again when this returns.
int group_render(vr_context *h, const vr_render_args *a, float *d_out, hipStream_t stream, float *d_out2,
                 const float *eye2) {
  const int n = 1 + (int)h->children.size();
  const int nviews = d_out2 ? 2 : 1;
  const int32_t bc = 16;
  const int64_t W = (int64_t)a->resolution[1], H = (int64_t)a->resolution[0];
  vr_partition p0{bc, 0, n, 0};
  const int64_t maxc = part_columns(W, bc, 0, n);
  const size_t part_floats = (size_t)maxc * (size_t)H * 3;
  if (!part_floats) {
    Frame F;
    return do_render(h, a, nullptr, d_out, nullptr, stream, F, d_out2, eye2);
  }
  ensure_part_buffers(h, n, part_floats, nviews);
  // the primary's part first: it uploads the frame's lights / LUT and binds them.  Its slots of the
  // part buffer are read by the previous frame's assembly, which may run on another stream.
  VR_HIP(hipStreamWaitEvent(stream, h->gdone, 0));
  Frame F0;
  int rc = do_render(h, a, &p0, h->d_part, nullptr, stream, F0, d_out2 ? h->d_part + (size_t)n * part_floats : nullptr,
                     eye2);
  if (rc) return rc;
  BufPtr saved[T_COUNT];
  for (int t = 0; t < T_COUNT; ++t) saved[t] = g_tex.bind[t];
  for (int k = 1; k < n && !rc; ++k) {
    vr_context *c = h->children[k - 1];
    DeviceGuard dg(c->device);
    bind_replicas(h, c, saved);
    vr_partition pk{bc, k, n, 0};
    Frame F;
    rc = do_render(c, a, &pk, c->d_part, nullptr, c->gstream, F, d_out2 ? c->d_part + part_floats : nullptr, eye2);
  }
  for (int t = 0; t < T_COUNT; ++t) g_tex.bind[t] = saved[t];
  if (rc) return rc;
  float *outs[2] = {d_out, d_out2};
  group_gather_assemble(h, nviews, part_floats, W, H, bc, maxc, outs, stream);
  return VR_OK;
}

void delete_children(vr_context *h) {
  for (vr_context *c : h->children) {
    DeviceGuard dg(c->device);
    (void)hipStreamSynchronize(c->gstream);
    for (auto &b : c->buf) b.reset();
    if (c->d_part) (void)hipFree(c->d_part);
    if (c->d_out) (void)hipFree(c->d_out);
    if (c->pin) vr_host::free_when_done(c->pin, c->device, vr_host::readers_of(c->pin_read), true);
    c->pin = nullptr;
    free_schedules(c);
    free_views(c);
    if (c->gdone) (void)hipEventDestroy(c->gdone);
    for (hipEvent_t e : c->tev)
      if (e) (void)hipEventDestroy(e);
    give_stream(c->device, c->gstream);
    delete c;
  }
  h->children.clear();
}

// The fusable views one device collects for its march_views launches.
struct ViewSet {
  std::vector<BufPtr> keep;
  std::vector<vr::RenderParams> views;
  std::vector<std::array<double, 3>> drift;
  std::vector<int> vmode, vab;
  std::vector<vr::DevLight> lights;
  std::vector<size_t> loff;
};

// Launch the collected views of one device on `stream` (the device current): one march_views launch
// per (gradient mode, absorption aliasing, slot size, shading) group, in channel order within a group.
static void launch_view_set(ViewSet &VS, int device, hipStream_t stream, vr_context *timer) {
  if (VS.views.empty()) return;
  std::vector<vr::RenderParams> &views = VS.views;
  const size_t nvw = views.size();
  std::vector<size_t> order(nvw);
  for (size_t k = 0; k < nvw; ++k) order[k] = k;
  auto key = [&](size_t k) {
    return ((VS.vmode[k] * 2 + VS.vab[k]) * 2 + views[k].wide_slot) * 2 + views[k].fast_shade;
  };
  std::stable_sort(order.begin(), order.end(), [&](size_t x, size_t y) { return key(x) < key(y); });
  // the views' lights, staged for these launches on their stream (each channel's own list)
  LaunchRec L;
  L.stream = stream;
  L.device = device;
  L.reads = std::move(VS.keep);
  for (const BufPtr &b : L.reads) wait_ready(b, stream);
  const void *dl = nullptr;
  VR_HIP(L.stage(VS.lights.data(), VS.lights.size() * sizeof(vr::DevLight), &dl));
  const vr::DevLight *d_lights = static_cast<const vr::DevLight *>(dl);
  time_mark(timer, 0, stream);
  size_t g0 = 0;
  while (g0 < nvw) {
    size_t g1 = g0;
    while (g1 < nvw && key(order[g1]) == key(order[g0])) ++g1;
    // depth lanes as for one view: the frame's own tail sets them, and K = 2 stays ahead of K = 1
    // per sample even at many waves per slot
    const int K = exact_lanes(std::min(depth_lanes(views[order[g0]]), 4), views[order[g0]].fast_shade);
    vr::RenderViews V;
    std::memset(&V, 0, sizeof V);
    for (size_t k = g0; k < g1; ++k) {
      vr::RenderParams &P = V.p[k - g0];
      P = views[order[k]];
      for (int d = 0; d < 3; ++d) P.tap_off[d] += (float)(chunk_samples(K) * VS.drift[order[k]][d]);
      P.lights = d_lights ? d_lights + VS.loff[order[k]] : nullptr;
    }
    const size_t v0 = order[g0];
    VR_HIP(march_entries(views[v0].fast_shade != 0, K).launch_views(V, (uint32_t)(g1 - g0), VS.vmode[v0],
                                                                    VS.vab[v0] != 0, stream));
    g0 = g1;
  }
  time_mark(timer, 1, stream);
  // a prepared frame's buffer that no handle or binding holds any more is freed when these launches
  // complete (vr_host::free_when_done); the launches stay asynchronous
  VR_HIP(L.finish());
}

// Multi-channel render (vr_render_channels): channel i is what vr_sync_volumes +
// vr_render (or vr_render_stereo) on ch[i] would produce were it the only object -- before its
// sync the texture bindings its handle's last sync left are restored (the reference's textures are
// module globals: with one object per channel an unchanged channel would otherwise render the
// previous channel's volumes); the syncs run in channel order, each channel's frame is prepared
// against the textures its own sync bound, and the frames the staged march can take are marched
// together in one launch per (gradient mode, absorption aliasing, slot size, shading) group, their
// views' parameters in kernel arguments.  The buffers a prepared frame reads stay referenced until
// its launch completes; a later channel's sync never overwrites them (each handle owns its buffers).
// Group handles (vr_new_multi, all channels on the same devices): every device renders its column
// part of every view (the channel's bindings replicated to it, as group_render does), the parts are
// gathered to the primary of channel 0 over xGMI and assembled there, view by view.
int do_render_channels(const vr_channel *ch, int32_t n, int32_t stereo, float base, float *d_out,
                              hipStream_t stream) {
  if (!ch || n < 1) return fail(VR_ERR_ARGUMENT, "no channels");
  const int nv = stereo ? 2 : 1;
  if (n * nv > VR_VIEWS_MAX) return fail(VR_ERR_ARGUMENT, "too many channels");
  for (int i = 0; i < n; ++i) {
    if (!valid(ch[i].handle)) return fail(VR_ERR_HANDLE, "Handle not valid.");
    if (!ch[i].args) return fail(VR_ERR_ARGUMENT, "insufficient parameter!");
    if (ch[i].handle->nclip) return clip_unsupported("vr_render_channels");
    for (int j = 0; j < i; ++j)
      if (ch[j].handle == ch[i].handle) return fail(VR_ERR_ARGUMENT, "channels need distinct handles");
    if (ch[i].args->resolution[0] != ch[0].args->resolution[0] || ch[i].args->resolution[1] != ch[0].args->resolution[1])
      return fail(VR_ERR_ARGUMENT, "channels differ in image resolution");
    if (ch[i].handle->device != ch[0].handle->device) return fail(VR_ERR_ARGUMENT, "channels on different devices");
    if (ch[i].handle->children.size() != ch[0].handle->children.size())
      return fail(VR_ERR_ARGUMENT, "channels on different device groups");
    for (size_t k = 0; k < ch[i].handle->children.size(); ++k)
      if (ch[i].handle->children[k]->device != ch[0].handle->children[k]->device)
        return fail(VR_ERR_ARGUMENT, "channels on different device groups");
  }
  const size_t img = (size_t)ch[0].args->resolution[0] * (size_t)ch[0].args->resolution[1] * 3;
  if (img && !d_out) return fail(VR_ERR_ARGUMENT, "output is NULL");
  const bool fuse = !test_flag("VR_NO_FUSED_CHANNELS");
  vr_context *h0 = ch[0].handle;
  const int ndev = 1 + (int)h0->children.size();
  const int32_t bc = 16;
  const int64_t W = (int64_t)ch[0].args->resolution[1], H = (int64_t)ch[0].args->resolution[0];
  const int64_t maxc = part_columns(W, bc, 0, ndev);
  const size_t part_floats = (size_t)maxc * (size_t)H * 3;
  const bool grouped = ndev > 1 && part_floats > 0;
  const int nviews = n * nv;  // view vi = i * nv + e
  if (grouped) {
    ensure_part_buffers(h0, ndev, part_floats, nviews);
    VR_HIP(hipStreamWaitEvent(stream, h0->gdone, 0));  // the previous frame's assembly read part 0
  }
  // where view vi of device k goes: the caller's image (one device) or the part buffers
  auto out_of = [&](int k, int vi) -> float * {
    if (!grouped) return d_out + (size_t)vi * img;
    if (k == 0) return h0->d_part + ((size_t)vi * ndev) * part_floats;
    return h0->children[k - 1]->d_part + (size_t)vi * part_floats;
  };
  std::vector<ViewSet> sets(grouped ? ndev : 1);
  for (int i = 0; i < n; ++i) {
    vr_context *h = ch[i].handle;
    if (h->has_snap) {  // this channel's own bindings, not the previous channel's
      for (int t = 0; t < T_COUNT; ++t) g_tex.bind[t] = h->snap_bind[t].lock();
      g_tex.idx_em = h->snap_idx[0];
      g_tex.idx_ab = h->snap_idx[1];
      g_tex.idx_re = h->snap_idx[2];
      g_tex.grad_method = h->snap_grad;
    }
    int rc = do_sync_volumes(h, ch[i].time_last_mem_sync, ch[i].emission, ch[i].reflection, ch[i].absorption,
                             ch[i].dx, ch[i].dy, ch[i].dz);
    if (rc) return rc;
    if (grouped) group_sync(h);
    vr_render_args a = *ch[i].args;
    float eye2[3] = {0.f, 0.f, 0.f};
    if (stereo) {  // as vr_render_stereo: left = the frame's eye at -base, right at +base
      a.props[0] = -base;
      const float *r = a.rotation_flipped;
      const float X[3] = {r[2], r[1], r[0]}, Z[3] = {r[8], r[7], r[6]};
      for (int k = 0; k < 3; ++k) eye2[k] = fmaf(-a.props[2], Z[k], base * X[k]);
    }
    BufPtr saved[T_COUNT];
    for (int t = 0; t < T_COUNT; ++t) saved[t] = g_tex.bind[t];
    for (int k = 0; k < (grouped ? ndev : 1) && !rc; ++k) {
      vr_context *ctx = k == 0 ? h : h->children[k - 1];
      DeviceGuard dg(ctx->device);
      hipStream_t s = k == 0 ? stream : h0->children[k - 1]->gstream;
      if (k > 0) bind_replicas(h, ctx, saved);
      vr_partition pk{bc, k, ndev, 0};
      float *dl = out_of(k, i * nv), *dr = stereo ? out_of(k, i * nv + 1) : nullptr;
      Frame F;
      int fz = 0;
      rc = do_render(ctx, &a, grouped ? &pk : nullptr, dl, nullptr, s, F, dr, stereo ? eye2 : nullptr,
                     fuse ? &fz : nullptr);
      if (rc || !fz) continue;  // (rendered by its own launch against the textures bound now)
      ViewSet &VS = sets[k];
      for (const BufPtr &b : g_tex.bind)
        if (b) VS.keep.push_back(b);
      for (int v = 0; v < nv; ++v) {
        vr::RenderParams P = F.P;
        P.views = 1;
        P.out2 = nullptr;
        P.view_blocks = 0;
        P.out = v ? dr : dl;
        if (v)
          for (int d = 0; d < 3; ++d) P.eye[d] = eye2[d];
        VS.views.push_back(P);
        VS.drift.push_back({F.drift1[0], F.drift1[1], F.drift1[2]});
        VS.vmode.push_back(F.mode);
        VS.vab.push_back(F.ab_alias ? 1 : 0);
        VS.loff.push_back(VS.lights.size());
      }
      VS.lights.insert(VS.lights.end(), g_tex.lights.begin(), g_tex.lights.end());
    }
    for (int t = 0; t < T_COUNT; ++t) g_tex.bind[t] = saved[t];
    if (rc) return rc;
  }
  for (int k = 0; k < (int)sets.size(); ++k) {
    vr_context *ctx = k == 0 ? h0 : h0->children[k - 1];
    DeviceGuard dg(ctx->device);
    launch_view_set(sets[k], ctx->device, k == 0 ? stream : ctx->gstream, ctx);
  }
  if (grouped) {
    std::vector<float *> outs(nviews);
    for (int vi = 0; vi < nviews; ++vi) outs[vi] = d_out + (size_t)vi * img;
    group_gather_assemble(h0, nviews, part_floats, W, H, bc, maxc, outs.data(), stream);
  }
  return VR_OK;
}

}  // namespace vr_host
