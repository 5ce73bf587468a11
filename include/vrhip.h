/*
 * vrhip.h -- C-ABI of libvrhip.so, the MI355X (gfx950) volume ray-marcher.
 *
 * The entry points mirror, one for one, the command protocol of the reference's CUDA mex
 * `volumeRender` (/root/reference/src/C/mex/render.cpp:50-278) plus its two helper mex files, so
 * that a thin mexFunction adaptor (mex/volumeRender_mex.cpp) keeps the MATLAB
 * classes VolumeRender / Volume / LightSource working unchanged.  Plain pointers and sizes only.
 *
 * Conventions (identical to what the mex receives from MATLAB):
 *   - volumes are MATLAB single arrays Data(d0,d1,d2), column-major, d0 fastest; a 2-D array has
 *     d2 = 1 (volumeRender.cpp:320-339).  Data pointers are borrowed for the call only.  Emission,
 *     reflection and absorption data may also be uint8, uint16, int16 or binary16 (vr_dtype below):
 *     converted exactly to single on the device during the upload.
 *   - the rendered image is MATLAB single [H, W, 3], column-major: out[x*H + y + c*W*H]
 *     (volumeRender_kernel.cu:496-506, render.cpp:248).
 *   - every function returns VR_OK (0) or an error code; vr_last_error() gives the message
 *     (the reference's mexErrMsgTxt text where one exists).  Errors are thread-local.
 */
#ifndef VRHIP_H_
#define VRHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum vr_status {
  VR_OK = 0,
  VR_ERR_ARGUMENT = 1,   /* bad argument count/shape (render.cpp:51-56,60-61,68-69,136-140) */
  VR_ERR_HANDLE = 2,     /* "Handle not valid." (class_handle.hpp:64-72)                      */
  VR_ERR_VRAM = 3,       /* "insufficient free VRAM!" (mmanager.hxx:144-173)                   */
  VR_ERR_DEVICE = 4,     /* a HIP runtime error (reference ignores them, common.h:43-47)        */
  VR_ERR_UNSUPPORTED = 5 /* request outside what this build implements                          */
};

/* Where vr_volume.data lives. */
enum vr_location { VR_HOST = 0, VR_DEVICE = 1 };

/* Element type of vr_volume.data.  The resident volume is always fp32: a narrow volume crosses the
 * host link in its own width and is widened on the device in the pad pass of the upload, so the
 * resident buffer and every image are bit for bit what MATLAB's single(Data) gives.
 *   - without VR_DTYPE_UNORM the resident voxel is the source element converted to fp32 -- exact
 *     for all four narrow types; for VR_F16 (IEEE binary16) that includes subnormals, +-0, +-inf
 *     and NaN (a NaN stays a NaN, its payload widened);
 *   - with VR_DTYPE_UNORM (VR_U8 / VR_U16 only) it is one correctly rounded fp32 division of the
 *     converted value by 255.0f resp. 65535.0f: MATLAB's single(x) / single(255).
 * Typed volumes are for emission, reflection and absorption.  The illumination LUT and the
 * gradient volumes dx, dy, dz must be VR_F32 (VR_ERR_UNSUPPORTED otherwise).  An unknown code, or
 * VR_DTYPE_UNORM on anything but VR_U8 / VR_U16, and a data pointer not aligned to its element
 * size, are VR_ERR_ARGUMENT.  The dtype is part of a volume's identity: two views of one buffer
 * with different element types are different volumes. */
enum vr_dtype { VR_F32 = 0, VR_U8 = 1, VR_U16 = 2, VR_I16 = 3, VR_F16 = 4 };
#define VR_DTYPE_UNORM 0x100 /* VR_U8 / VR_U16 only: value = (float)x / 255.0f resp. 65535.0f */

/* A MATLAB `Volume` as the mex reads it (mxMake_volume, volumeRender.cpp:307-342):
 * Data, its dims, and TimeLastUpdate.  `location` VR_DEVICE lets device-resident data
 * (e.g. a torch tensor) be synced without a host round trip.  `data` keeps its declared type; for
 * dtype != VR_F32 it points to d0*d1*d2 elements of that type, column-major, on the host or the
 * device per `location`.  A zero-initialised dtype is VR_F32 (MATLAB single). */
typedef struct vr_volume {
  const float *data;
  uint64_t dims[3];      /* d0, d1, d2 (d2 = 1 for 2-D data)          */
  uint64_t last_update;  /* TimeLastUpdate (ms timestamp, see vr_timestamp) */
  int32_t location;      /* enum vr_location                           */
  int32_t dtype;         /* enum vr_dtype, optionally | VR_DTYPE_UNORM  */
} vr_volume;

/* Element size in bytes of a dtype code (flag included), or 0 for an invalid code or an invalid
 * flag combination.  Needs no device. */
size_t vr_dtype_size(int32_t dtype);

/* The upload's conversion on the CPU (the contract above): dst[i] = fp32 of element i of src, for
 * n elements.  VR_ERR_ARGUMENT for an invalid dtype, a NULL pointer with n > 0, or a src not
 * aligned to its element size.  Needs no device. */
int vr_convert_host(const void *src, int32_t dtype, uint64_t n, float *dst);

/* A MATLAB `LightSource` (LightSource.m:40-64): Position and Color exactly as stored in MATLAB.
 * The position is reversed into kernel order internally (render.cpp:167-168). */
typedef struct vr_light {
  float position[3];
  float color[3];
} vr_light;

/* The positional arguments of volumeRender('render', h, ...) (render.cpp:142-240,
 * caller VolumeRender.m:563-581), in the order and units MATLAB passes them. */
typedef struct vr_render_args {
  const vr_light *lights;         /* LightSources (prhs[2])                                  */
  int64_t num_lights;             /* mxGetN(LightSources); < 0: the logical `false`           */
  const vr_volume *illumination;  /* VolumeIllumination (prhs[3]); NULL: the logical `false`  */
  float factors[3];               /* single([FactorEmission FactorReflection FactorAbsorption]) */
  float element_size_um[3];       /* single(ElementSizeUm), MATLAB order (reversed inside)    */
  uint64_t resolution[2];         /* uint64([H W]) = flip(ImageResolution)                    */
  float rotation_flipped[9];      /* single(flip(RotationMatrix)), column-major as passed      */
  float props[3];                 /* single([CameraXOffset FocalLength DistanceToObject])     */
  float opacity_threshold;        /* single(OpacityThreshold)                                 */
  float color[3];                 /* single(Color)                                            */
} vr_render_args;

/* Image-space partition for multi-GPU rendering: columns are cut into blocks of
 * `block_cols`; block b belongs to part (b % num_parts).  A part's output is the column-major
 * planar image of only its columns, in increasing x, with a fixed column stride max_cols =
 * vr_partition_columns(w, {block_cols, part 0, num_parts}) (part 0 owns the most columns):
 * element (y, local column j, channel c) at c*max_cols*H + j*H + y. */
typedef struct vr_partition {
  int32_t block_cols;
  int32_t part;
  int32_t num_parts;
  int32_t reserved;
} vr_partition;

typedef struct vr_context vr_context; /* the reference's MManager handle (mmanager.hxx:25) */

/* --- the mex commands --------------------------------------------------------------------- */

/* 'new' (render.cpp:58-65): a persistent handle bound to the current HIP device. */
int vr_new(vr_context **out);

/* 'new' for a multi-device group (SURVEY.md 8e inside the library, so that the MATLAB classes reach
 * every GPU of the node through the unchanged mex protocol; the reference picks one device,
 * volumeRender.cpp:77-87).  devices[0] is the primary: 'sync_volumes' uploads there once and copies
 * the bound volumes to the other devices over xGMI (peer copies); 'render' (and vr_render_device
 * without a partition or counters) renders column part k of the frame (16-column blocks dealt
 * round-robin) on devices[k], gathers the parts to the primary with peer copies and assembles the
 * image there -- bit-identical to the one-device render.  vr_render_stereo and vr_render_channels on
 * group handles split their fused launches across the devices the same way; vr_render_slab and a
 * vr_render_device call with a partition or counters run on the primary only.  A device may repeat
 * (a rehearsal on one GPU). */
int vr_new_multi(const int32_t *devices, int32_t n, vr_context **out);

/* 'delete' (render.cpp:72-79 -> ~MManager, mmanager.hxx:103-105).  Like the reference's
 * cudaDeviceReset this frees every handle's device volumes and resets the module-global render
 * state (texture bindings, slot indices, lights, gradient method). */
int vr_delete(vr_context *h);

/* 'mem_info' (render.cpp:85-87, mmanager.hxx:218-284): writes the report into buf. */
int vr_mem_info(vr_context *h, char *buf, size_t buflen);

/* 'sync_volumes' (render.cpp:93-129): note the order Emission, Reflection, Absorption.
 * The reference keys on the argument count (render.cpp:105-113), mapped to the gradient pointers:
 *   dx, dy, dz all non-NULL  -- nrhs == 9: the gradient volumes are taken (gradient lookup);
 *   all NULL                 -- nrhs == 6: the handle's gradient volumes are reset (on-the-fly);
 *   dx (nrhs 7) or dx, dy (nrhs 8) non-NULL, the rest NULL -- any other count (an adaptor passes
 *                              nrhs 7, 8 or > 9 this way): the handle KEEPS its previous gradient
 *                              volumes and the given ones are not read; the method is set to
 *                              on-the-fly, and the sync re-enters lookup mode if kept gradient
 *                              volumes exist (mmanager.hxx:193-200). */
int vr_sync_volumes(vr_context *h, uint64_t time_last_mem_sync, const vr_volume *emission,
                    const vr_volume *reflection, const vr_volume *absorption, const vr_volume *dx,
                    const vr_volume *dy, const vr_volume *dz);

/* 'render' (render.cpp:134-277): renders into the caller-owned host image out[H*W*3]. */
int vr_render(vr_context *h, const vr_render_args *args, float *out);

/* --- the helper mex files ------------------------------------------------------------------- */

/* HenyeyGreenstein(N[, g]) (HenyeyGreenstein.cc:29-96): out[N*N*N], MATLAB array (b, a, c). */
int vr_henyey_greenstein(uint32_t n, float g, float *out);

/* timestamp (timestamp.cpp:17-33): ms since the epoch, low 32 bits only (it is stored through an
 * int*), zero-extended -- exactly the value the reference hands to MATLAB. */
uint64_t vr_timestamp(void);

/* Fused stereo: VolumeRender.render with CameraXOffset != 0
 * (VolumeRender.m:278-307) renders the pair as two 'render' calls with camera offsets +base and
 * -base.  This renders both eyes of the same frame in one launch: args->props[0] is ignored, the
 * left image (offset -base) goes to out_left, the right (+base) to out_right, each [H, W, 3] as
 * vr_render writes it, bit-identical to the two separate renders. */
int vr_render_stereo(vr_context *h, const vr_render_args *args, float base, float *out_left, float *out_right);

/* vr_render_stereo into device memory on `stream` (asynchronous, as vr_render_device; one-device
 * handles; d_steps as vr_render_device's, over both eyes).  VR_STEREO_PAIR=1 marches the pair with
 * paired tiles (a wave holds the right eye's column c and the left eye's column
 * c + shift, one staged box for both) -- a measurement switch, images bit-identical. */
int vr_render_stereo_device(vr_context *h, const vr_render_args *args, float base, float *d_left, float *d_right,
                            unsigned long long *d_steps, void *stream);

/* Multi-channel frame (replaces the per-channel loops of examples/example3.m:
 * 61-233 -- sync a channel's volumes, render, next channel -- and the sum at example3.m:239).  A
 * channel is one VolumeRender object: its handle (distinct per channel), the arguments of its
 * 'sync_volumes' (volumeRender.cpp:600-633; dx/dy/dz NULL = on-the-fly gradient) and of its
 * 'render'.  Channel i equals vr_sync_volumes + vr_render on it (stereo != 0: vr_render_stereo
 * with `base`, left then right) were its handle the only one: before the channel's sync, the
 * texture bindings its handle's last sync left are restored (the reference's textures are module
 * globals, kernel.cu:49-120, so with one object per channel an unchanged channel would render the
 * previous channel's volumes).  Every channel must have the same resolution.
 * The channels' frames are marched together (one launch per gradient-mode / absorption / shading
 * group).  vr_render_channels writes channel i's view e (e = 0 left / only, 1 right; eyes = 1 or
 * 2) to out[(i * eyes + e) * H*W*3 ...], each laid out as vr_render's image; the caller adds them
 * (example3.m:239 adds in double). */
typedef struct vr_channel {
  vr_context *handle;
  uint64_t time_last_mem_sync;
  const vr_volume *emission, *reflection, *absorption;
  const vr_volume *dx, *dy, *dz;
  const vr_render_args *args;
} vr_channel;
int vr_render_channels(const vr_channel *channels, int32_t n, int32_t stereo, float base, float *out);
/* Device variant: channel i's view e (e = 0 left / only, 1 right) into
 * d_out + (i * eyes + e) * H*W*3, on `stream` (asynchronous; the syncs are not). */
int vr_render_channels_device(const vr_channel *channels, int32_t n, int32_t stereo, float base, float *d_out,
                              void *stream);
/* fp32 channel sum on the device: d_out[e][k] = d_in[0][e][k] + d_in[1][e][k] + ... (channel order,
 * fp32 additions) for n channels x views images of image_floats floats each. */
int vr_sum_channels_device(const float *d_in, int32_t n, int32_t views, uint64_t image_floats, float *d_out,
                           void *stream);

/* --- device-side extensions (multi-GPU, benchmarking; no MATLAB counterpart) ------------------ */

/* 'render' without the host round trip: writes the (partitioned, if part != NULL) image to the
 * device buffer d_out on `stream` (a hipStream_t; NULL = default stream).  Asynchronous.
 * If d_steps != NULL it points to VR_NUM_COUNTERS (48) counters: d_steps[0] += ray-march samples
 * taken, d_steps[1] += samples that evaluated gradient + shading (the others had opacity exactly
 * 0), d_steps[2..4] += LDS-staged chunks, all-empty (leaped) chunks, global-memory chunks,
 * d_steps[5..6] += wave sample iterations, of which any lane shaded; d_steps[7] += empty-space
 * probe runs leaped; d_steps[8..39] histogram of the box volume (floats, bins of
 * 256, last bin open) of chunks that fell back to global memory; d_steps[40..43] staged chunks with
 * S = 32, 16, 8, 4; d_steps[44] += probes that found data; d_steps[45] += floats staged into LDS;
 * d_steps[46] += chunks leaped on the occupancy map's word, without a copy; d_steps[47] |= 1 << (ex mod 4)
 * for the row length ex of every staged box (a bit set, not a count).
 * [2..47] are filled by the LDS-staged kernel only. */
#define VR_NUM_COUNTERS 48
int vr_render_device(vr_context *h, const vr_render_args *args, const vr_partition *part,
                     float *d_out, unsigned long long *d_steps, void *stream);

/* --- projections through the current camera (no reference counterpart) ------------------------
 * A projection marches exactly the ray of 'render': the same pixel-to-ray mapping and box
 * intersection, tnear clamped to 0, the same tstep, the recurrences t += tstep and pos += step and
 * the same max_steps cap.  It has no early exit on opacity: the loop ends only when t > tfar or on
 * the cap, so every ray takes the samples k = 0 .. n-1 that 'render' would take with an opacity
 * threshold that is never reached.  v_k is the trilinear sample of the EMISSION texture at sample k,
 * fetched through the slot index as 'render' does (an unbound texture gives 0, a 1x1x1 texture its
 * voxel through the same lerp algebra).  Ignored in vr_render_args: the lights and the illumination
 * LUT (not uploaded; the handle's light state is left as it is), factors[1], factors[2] and
 * opacity_threshold.  props[0] (the camera x offset) is honoured.  With Fe = factors[0]:
 *   VR_PROJ_MIP  m = -inf, no winner; for k = 0 .. n-1: if v_k > m then m = v_k, t* = the march's t
 *                at sample k (strictly greater: the first sample that attains the maximum wins; a
 *                NaN sample never wins).  pixel = (Fe * (m + 0.0f)) * color[c] (the + 0.0f turns -0
 *                into +0); aux = t*, the distance from the eye in the march's units, exactly the
 *                value of the t recurrence.  A ray that misses the box, or one with no winning
 *                sample (every sample NaN or -inf): pixel 0, aux NaN.
 *   VR_PROJ_SUM  s = 0; s = s + v_k in sample order, one fp32 addition per sample.
 *                pixel = ((Fe * s) * tstep) * color[c]; aux = (float)n (the mean projection is
 *                pixel / (n * tstep)).  A miss: pixel 0, aux 0.  NaN and inf propagate.
 * The image is laid out as 'render' writes it: [H, W, 3] column-major, or for a part the
 * plane_cols stride documented at vr_partition; the aux plane is [H, W], resp. [max_cols][H].
 * Empty space is leaped through the emission texture's occupancy map where it has one (both planes
 * bit-identical to the march without; VR_PROJ_NO_PROBE=1, a test switch, turns the leap off).
 * The mode is checked first (unknown: VR_ERR_ARGUMENT, before the handle: needs no device); a
 * multi-device group handle is VR_ERR_UNSUPPORTED; a NULL out / d_out with a non-empty image is
 * VR_ERR_ARGUMENT.  A degenerate frame (no emission volume synced) writes zeros, and the miss
 * values to aux. */
enum vr_projection { VR_PROJ_MIP = 0, VR_PROJ_SUM = 1 };

/* Into the caller-owned host image out[H*W*3] and, if not NULL, out_aux[H*W]. */
int vr_render_projection(vr_context *h, const vr_render_args *args, int32_t mode, float *out,
                         float *out_aux /* may be NULL */);

/* Into device memory on `stream` (asynchronous, as vr_render_device), the whole image or a part.
 * d_steps, if not NULL, points to at least two counters: d_steps[0] += samples visited, leaped
 * ones included (the sum of n over the rays); d_steps[1] += samples actually fetched. */
int vr_render_projection_device(vr_context *h, const vr_render_args *args, int32_t mode,
                                const vr_partition *part, float *d_out, float *d_aux /* may be NULL */,
                                unsigned long long *d_steps /* may be NULL */, void *stream);

/* --- first-hit isosurface through the current camera (no reference counterpart) ---------------
 * The opaque surface v = level of the EMISSION texture, lit by the scene's lights, with its depth and
 * normal planes.
 * Search.  The ray is exactly that of 'render' and of the projections: the same pixel-to-ray mapping
 * and box intersection, tnear clamped to 0, tstep, the recurrences t += tstep and pos += step, and
 * the max_steps cap; there is no opacity exit.  v_k is the trilinear emission sample at sample k,
 * fetched through the slot index as the projections do (an unbound texture reads 0, a 1x1x1 texture
 * gives its voxel through the lerp algebra).  The hit is the first k with v_k >= level; a NaN sample
 * is never >=, in the search and in the refinement alike.  The ray stops at the hit.  No hit before
 * t > tfar or before the cap: no surface.
 * Refinement (VR_ISO_REFINE = 6 bisection steps, a compile-time constant).  k = 0: the surface point
 * is the first sample itself, p* = pos_0, t* = t_0 (the box face cuts the object).  k > 0: lo = 0,
 * hi = 1; six times c = (lo + hi) * 0.5f, q_i = fmaf(step_i, c, pos_{k-1,i}), v = the emission sample
 * at (q - bmin) * bscale, v >= level ? hi = c : lo = c; then p*_i = fmaf(step_i, hi, pos_{k-1,i}) and
 * t* = fmaf(tstep, hi, t_{k-1}) (hi = 1 gives pos_k and t_k bit for bit).  v* is the emission sample
 * at p*.
 * Surface sample.  g is the gradient 'render''s exact shading takes at a sample at p*, by the handle's
 * gradient method whether or not there are lights: on the fly, the six taps at
 * ((pos +- gstep) - bmin) * bscale of the emission binding, times 0.5 (never the half-texel fast
 * taps); lookup, the three gradient textures at p*.  n = -(g * (1 / sqrtf(dot(g, g)))); a zero
 * gradient gives NaN, as in 'render'.  ill is 'render''s exact (oracle-order) shading at p* with
 * refl = Fr * reflection(p*); the lights and the illumination LUT are uploaded and checked exactly as
 * 'render' does (a typed LUT: VR_ERR_UNSUPPORTED) and stay the handle's light state; without lights
 * or without a LUT ill = 0.  pixel_c = fmaf(Fe * v*, color[c], ill_c).  opacity_threshold and
 * factors[2] are ignored; props[0] is honoured.
 * Outputs.  The image is laid out as 'render' writes it, whole or as a part; the depth plane, t*, as
 * the projections' aux plane ([H, W], resp. [max_cols][H]); the normal plane, n.x, n.y, n.z, in three
 * planes laid out like the image.  A pixel without a surface (the ray misses the box, or no sample
 * hits): image 0, depth NaN, normal NaN; a degenerate frame (no emission volume synced) writes those
 * everywhere.  Empty space is leaped through the emission texture's occupancy map when level > 0 (a
 * leaped run's samples are +-0 and cannot hit; every plane bit-identical to the march without;
 * VR_ISO_NO_PROBE=1, a test switch, turns the leap off).
 * A NaN level is VR_ERR_ARGUMENT, checked before the handle (needs no device); +-inf is allowed.  A
 * multi-device group handle is VR_ERR_UNSUPPORTED; a NULL out / d_out with a non-empty image is
 * VR_ERR_ARGUMENT.  The call changes only what 'render' changes, the handle's light and LUT state: a
 * 'render' before and after gives the same bits. */
#define VR_ISO_REFINE 6

/* Into the caller-owned host image out[H*W*3] and, where not NULL, out_depth[H*W], out_normal[H*W*3]. */
int vr_render_isosurface(vr_context *h, const vr_render_args *args, float level, float *out,
                         float *out_depth /* [H,W], may be NULL */, float *out_normal /* [H,W,3], may be NULL */);

/* Into device memory on `stream` (asynchronous, as vr_render_device), the whole image or a part.
 * d_steps, if not NULL, points to at least three counters: d_steps[0] += search samples visited,
 * leaped ones included; d_steps[1] += search samples fetched; d_steps[2] += surface pixels. */
int vr_render_isosurface_device(vr_context *h, const vr_render_args *args, float level, const vr_partition *part,
                                float *d_out, float *d_depth, float *d_normal,
                                unsigned long long *d_steps /* 3 counters, may be NULL */, void *stream);

/* --- transfer-function render: a colormap and an alphamap per sample (no reference counterpart) ---
 * 'render' with a classification: each sample's colour comes from a colormap instead of the constant
 * color, and its opacity optionally from an alphamap -- what MATLAB's volshow calls Colormap and
 * Alphamap over a data range -- and the accumulated opacity is an output plane.
 * Table lookup L(T, n, lo, hi, c), in fp32, every operation rounded once:
 *   inv = 1.0f / (hi - lo), formed once on the host;
 *   x = ((c - lo) * inv) * (float)(n - 1);
 *   x = fminf(fmaxf(x, 0.0f), (float)(n - 1)), where a NaN coordinate and -0 give +0: the coordinate
 *       clamps at both ends and a NaN reads entry 0;
 *   i = min((int)x, n - 2);  w = x - (float)i;  the value is fmaf(w, T[i+1] - T[i], T[i]).
 * A constant table returns its constant bit for bit for every c (a constant -0 reads +0).  The kernel
 * and vr_transfer_lookup_host evaluate one shared inline function (csrc/vr_transfer.h).
 * The ray is exactly that of 'render': the same pixel-to-ray mapping and box intersection, tnear
 * clamped to 0, tstep, t += tstep and pos += step, the max_steps cap, and render's exit tests in
 * their order -- the accumulated opacity above opacity_threshold after compositing, then the cap,
 * then t > tfar.  props[0] is honoured.
 * The sample is that of 'render' with exact (oracle-order) shading, with two substitutions.  em_s and
 * ab_s are render's emission and absorption samples (slot indices, the alias rule, the unbound and
 * 1x1x1 cases).  cc = coord == VR_TF_VALUE ? em_s : t, t the march's t at this sample;
 * C_c = L(colormap plane c, n_color, clim, cc) for c = 0..2;  A = alphamap ? L(alphamap, n_alpha,
 * alim, ab_s) : ab_s;  e = Fe * em_s, a = Fa * A, alpha = 1 - expf(-(a * tstep)), eds = e * tstep;
 * ill is render's exact shading at the sample (the handle's gradient method, refl = Fr * reflection,
 * args->color inside ill as in 'render'; without lights or without a LUT ill = 0);
 *   r_c = fmaf(eds, C_c, ill_c) * alpha
 * -- C_c stands where color[c] stands in 'render' -- and the four compositing fmas follow unchanged.
 * So with a colormap whose every entry is color[c] and no alphamap the image is the exact-shading
 * 'render' image bit for bit.  The lights and the illumination LUT are uploaded and checked as
 * 'render' does (a typed LUT: VR_ERR_UNSUPPORTED) and stay the handle's light state; nothing else of
 * the handle is written: a 'render' before and after gives the same bits.
 * Outputs.  The image (the composited r, g, b) is laid out as 'render' writes it, whole or as a part;
 * the alpha plane, the accumulated opacity, as the projections' aux plane ([H, W], resp.
 * [max_cols][H]).  A ray that misses the box writes 0 to both; a degenerate frame (no emission volume
 * synced) writes zeros everywhere.  Empty space is leaped through the emission texture's occupancy
 * map where a leaped sample adds exactly 0 (absorption aliases emission and Fa * A(+-0) * tstep == 0;
 * both planes bit-identical to the march without; VR_TF_NO_PROBE=1, a test switch, turns it off).
 * Errors.  The table checks come first and need no device, each VR_ERR_ARGUMENT: tf or colormap NULL,
 * an n outside 2..VR_TF_MAX_ENTRIES, a non-finite table entry, a non-finite limit or !(lo < hi) (alim
 * only with an alphamap), an unknown coord.  A NULL out / d_out with a non-empty image is
 * VR_ERR_ARGUMENT; a multi-device group handle is VR_ERR_UNSUPPORTED. */
#define VR_TF_MAX_ENTRIES 1024
enum vr_transfer_coord { VR_TF_VALUE = 0, VR_TF_DEPTH = 1 };
typedef struct vr_transfer {
  const float *colormap; /* host, n_color x 3 as MATLAB stores an N x 3 single matrix: colormap[c * n_color + i] */
  int32_t n_color;       /* 2 .. VR_TF_MAX_ENTRIES */
  float clim[2];         /* colour coordinate range, lo < hi, finite */
  const float *alphamap; /* host, n_alpha values, or NULL: the opacity of 'render' (a = Fa * ab_s) */
  int32_t n_alpha;       /* 2 .. VR_TF_MAX_ENTRIES when alphamap != NULL */
  float alim[2];         /* absorption-sample range of the alphamap, lo < hi, finite */
  int32_t coord;         /* vr_transfer_coord: what indexes the colormap */
  int32_t reserved;
} vr_transfer;

/* Into the caller-owned host image out[H*W*3] and, if not NULL, out_alpha[H*W]. */
int vr_render_transfer(vr_context *h, const vr_render_args *args, const vr_transfer *tf, float *out,
                       float *out_alpha /* [H,W], may be NULL */);

/* Into device memory on `stream` (asynchronous, as vr_render_device), the whole image or a part.
 * d_steps, if not NULL, points to at least two counters: d_steps[0] += samples visited, leaped ones
 * included; d_steps[1] += samples fetched. */
int vr_render_transfer_device(vr_context *h, const vr_render_args *args, const vr_transfer *tf,
                              const vr_partition *part, float *d_out, float *d_alpha /* may be NULL */,
                              unsigned long long *d_steps /* 2 counters, may be NULL */, void *stream);

/* --- clip planes: cut-away views for the single-handle render calls (no reference counterpart) ---
 * A geometric cut-away: no volume data changes, each ray's interval [tnear, tfar] is shortened.
 * Coordinates.  A plane keeps the half-space normal . q + offset >= 0 of the normalized volume
 * coordinate q in the dimension order of Data: q_j runs from 0 to 1 across dimension j (dims[j]) of the
 * emission volume, the centre of voxel i (0-based) at (i + 0.5) / d_j.  q is the sampler's own
 * coordinate (pos - bmin) * bscale; normal[j] pairs with dims[j] -- the axis order that
 * element_size_um, the light positions and the rotation matrix have reversed (element_size_um[2 - j]
 * belongs to dims[j]).  The kept region is the intersection of the planes and of the box.
 * State.  The planes are state of the handle: vr_set_clip replaces the set (n = 0 clears it, planes may
 * then be NULL), vr_delete drops it with the handle.  vr_get_clip writes the n planes as they were set
 * into planes[0 .. n-1] (room for VR_CLIP_MAX) and their count into *n.
 * Errors of vr_set_clip, checked before the handle (they need no device), each VR_ERR_ARGUMENT: n
 * outside 0..VR_CLIP_MAX; planes NULL with n > 0; a non-finite normal component or offset; an all-zero
 * normal.  vr_get_clip: planes or n NULL is VR_ERR_ARGUMENT.
 * Host conversion, once per launch, in fp32, every operation rounded once.  With bmin_k and bscale_k
 * the box of the frame (k the kernel axis = the dimension of Data) and n_k = normal[k]:
 *   N_k = n_k * bscale_k;
 *   D   = fmaf(-N_2, bmin_2, fmaf(-N_1, bmin_1, fmaf(-N_0, bmin_0, offset))).
 * Per ray.  After the ray set-up of 'render' has produced the origin o, the direction d, the box hit
 * and tnear (clamped to 0) and tfar, the planes are applied in the order they were set:
 *   s0 = fmaf(N_2, o_2, fmaf(N_1, o_1, fmaf(N_0, o_0, D)));
 *   sd = fmaf(N_2, d_2, fmaf(N_1, d_1, N_0 * d_0));
 *   tc = (-s0) / sd                                   (one IEEE division);
 *   sd > 0:  if (tc > tnear) tnear = tc;    sd < 0:  if (tc < tfar) tfar = tc;
 *   sd == +-0 or NaN: the ray is a miss unless s0 >= 0.
 * After the last plane the ray is a hit only if it hit the box and tnear <= tfar (a NaN fails).  A hit
 * ray runs exactly as without planes from the new tnear: pos_0 = fmaf(d, tnear, o), t_0 = tnear, the
 * unchanged recurrences, the cap and the exit tests against the new tfar; a miss writes each render's
 * miss values.  Clipping acts on sample positions only: the gradient taps, the reflection and LUT
 * fetches and the isosurface's bisection read the unclipped volume.  The isosurface's rule that a hit
 * at sample 0 is the surface point itself gives a cut object a capped cut face, its depth the clipped
 * tnear.
 * Which calls honour the planes.
 *   vr_render_projection[_device], vr_render_isosurface[_device], vr_render_transfer[_device]: clipped
 *     instantiations of their kernels, the empty-space leap left on; partition and d_steps as without.
 *   vr_render, vr_render_device: the general one-lane kernel (not the LDS-staged march) in a clipped
 *     instantiation, with the handle's shading variant (fast; exact under VR_EXACT_SHADE=1); partition
 *     and d_steps[0..1] as without.  Much slower than the march (about seven times on a whole
 *     frame; less the more is cut away): DESIGN.md s13.
 *   vr_render_stereo[_device]: the two clipped renders with props[0] = -base and +base, bit for bit.
 *   vr_render_channels[_device] (any channel's handle), vr_render_slab and every render call on a
 *     multi-device group handle: VR_ERR_UNSUPPORTED, the message names the clip planes.
 * With no planes set every call launches the kernels it launches without this feature, and
 * vr_last_march_kernel reports what it did. */
#define VR_CLIP_MAX 6 /* enough for a crop box */
typedef struct vr_clip_plane {
  float normal[3]; /* pairs with dims[0..2] of Data */
  float offset;
} vr_clip_plane;
int vr_set_clip(vr_context *h, const vr_clip_plane *planes, int32_t n); /* n = 0 clears */
int vr_get_clip(vr_context *h, vr_clip_plane *planes /* VR_CLIP_MAX */, int32_t *n);

/* The host conversion above on the CPU (needs no device), for tests: out[i] = {N_0, N_1, N_2, D} of
 * planes[i] for the box bmin[3], bscale[3].  The argument checks of vr_set_clip; a NULL bmin or
 * bscale, or a NULL out with n > 0, is VR_ERR_ARGUMENT. */
int vr_clip_convert_host(const vr_clip_plane *planes, int32_t n, const float bmin[3], const float bscale[3],
                         float *out /* [n][4] */);

/* --- label volume with per-label gains: fade segmented regions without a re-upload (no reference
 * counterpart; examples/example4.m rewrites VolumeEmission.Data(mask) on the host per frame) ---------
 * A label volume (uint8, one label per voxel) stays resident beside the handle's emission volume, and a
 * gain table (one fp32 gain per label) is state of the handle.  The resident emission buffer, its upload
 * statistics and its occupancy map are re-derived on the device from the unmodified upload; the render
 * calls read an ordinary resident volume and are unchanged.
 * Value.  For voxel i with label l = labels[i] the resident voxel is l < n ? src[i] * gains[l] : src[i]:
 * one fp32 multiplication rounded once -- MATLAB's single(gain) * Data(i), numpy's float32 product --
 * of src[i], the resident fp32 voxel after the typed upload's widening or UNORM division.  Labels at or
 * above n have gain 1 and are copied, not multiplied.  A NaN voxel stays NaN; +-0 and inf follow IEEE
 * (x * 0.0f keeps the sign, inf * 0 is NaN).  With n = 0 or no labels the buffer holds the unmodified
 * voxels bit for bit.  So the state equals vr_sync_volumes of the host-rewritten volume bit for bit: the
 * padded data and its apron (the edge replicate of the modulated interior), nonfinite and maxabs of the
 * modulated values (the launch-wide decisions of vr_last_launch_flags follow them), an occupancy map of
 * the modulated data, and a new upload version (launch schedules keyed on the upload are not reused).
 * Labels.  dtype must be VR_U8 without VR_DTYPE_UNORM (VR_ERR_ARGUMENT otherwise); location host or
 * device; stored dense on the device, one byte per voxel.  A repeated vr_sync_labels of the same Volume
 * identity (data pointer, TimeLastUpdate != 0, dims, location) is not uploaded again.  NULL, or an empty
 * volume, drops the labels.  The dims must equal those of the handle's emission volume whenever both are
 * present and n > 0: the call that notices -- vr_sync_labels (the previous labels stay),
 * vr_set_label_gains (the previous table stays) or vr_sync_volumes (the new volume is resident,
 * unmodified) -- returns VR_ERR_ARGUMENT with a message that names the labels.
 * Gains.  n in 0..256 (n = 0 clears the table, gains may then be NULL), every gain finite, negative
 * allowed; gains NULL with n > 0: each VR_ERR_ARGUMENT, checked before the handle (they need no device).
 * vr_get_label_gains writes the n gains as set into gains[0 .. n-1] (room for 256) and n into *n.
 * What is modulated.  The device buffer that the handle's last vr_sync_volumes bound as the emission
 * texture.  Absorption or reflection that alias it (the reference's default: VolumeAbsorption is the
 * same Volume) sample the same buffer and follow; a separately uploaded absorption or reflection
 * volume, the gradient volumes of lookup mode and the LUT are not touched.
 * When.  Eagerly: inside vr_sync_labels, inside vr_set_label_gains and at the end of vr_sync_volumes
 * (also per channel in vr_render_channels), whenever emission, labels and n > 0 are all present, in
 * whatever order they arrived; nothing is written when nothing changed.  A sync of a changed emission
 * volume uploads it and re-applies the gains; a sync of an unchanged one keeps the modulation.  A rewrite
 * waits for every launch that reads the buffer, so a *_device render in flight on any stream sees the
 * gains that were set when it was launched.
 * Memory.  The label bytes and, while gains are set, an unmodified copy of the emission volume count in
 * the handle's required memory (VR_ERR_VRAM when they do not fit) and appear in 'mem_info'; vr_delete
 * frees them.
 * vr_sync_labels, and vr_set_label_gains with n > 0, on a multi-device group handle: VR_ERR_UNSUPPORTED,
 * the message names the labels.  With no labels and no gains every call allocates, uploads and launches
 * what it does without this feature. */
int vr_sync_labels(vr_context *h, const vr_volume *labels);           /* NULL drops them */
int vr_set_label_gains(vr_context *h, const float *gains, int32_t n); /* n = 0 clears   */
int vr_get_label_gains(vr_context *h, float *gains /* 256 */, int32_t *n);

/* The value rule above on the CPU (needs no device): dst[i] = labels[i] < n ? src[i] * gains[labels[i]] :
 * src[i] for count voxels, by the inline function the kernel evaluates (csrc/vr_labels.h).  The argument
 * checks of vr_set_label_gains; a NULL src or dst, or NULL labels with n > 0, with count > 0 is
 * VR_ERR_ARGUMENT. */
int vr_label_gain_host(const float *src, const uint8_t *labels, const float *gains, int32_t n, uint64_t count,
                       float *dst);

/* --- Gaussian smoothing of the resident emission volume (no reference counterpart; the usual first step
 * on a noisy stack is imgaussfilt3(Data, sigma) on the host and a full re-upload) ----------------------
 * sigma[j], in voxels along dims[j] of Data (the axis order of the clip planes' normals), is state of the
 * handle.  The resident emission buffer, its upload statistics and its occupancy map are re-derived on the
 * device from the unmodified upload -- the derivation of the label gains, with the smoothing in front:
 * unmodified upload -> smoothing -> label gains -> resident buffer.  Every render, slice and histogram
 * call reads an ordinary resident volume and is unchanged.
 * Value.  The weights of one axis are formed once on the host in double: R = (int)ceil(2.0 * (double)sigma),
 * g_i = exp(-(double)(i*i) / (2 sigma^2)) for i = -R..R, S the sum of the g_i in ascending i,
 * w_k = (float)(g_{k-R} / S), k = 0..2R -- the shape of imgaussfilt3's defaults (size 2*ceil(2 sigma)+1,
 * replicate padding); the arithmetic is this library's own.  One axis pass over a line x[0..n-1] is, in
 * fp32 with every operation rounded once,
 *     acc = w[0] * x[c(i-R)];  acc = fmaf(w[k], x[c(i-R+k)], acc) for k = 1..2R;  y[i] = acc
 * with c clamping to 0..n-1.  The passes run along dims[0], then dims[1], then dims[2], each reading the
 * fp32 result of the one before.  An axis with sigma[j] == 0 or dims[j] == 1 is skipped (2-D data needs no
 * special call); with every axis skipped the buffer holds the unmodified voxels bit for bit.  NaN, inf,
 * +-0 and subnormals follow IEEE through the chain; nothing is flushed or tested.  No bit depends on how
 * the kernels tile or order their work: the library holds two kernel forms (one launch per axis, which
 * serves every radius; all three axes fused in one launch, which measured slower and runs only under the
 * test switch VR_SMOOTH_FORM=fused), and they give the same bits.  A label's gain multiplies the smoothed voxel: the result equals
 * vr_label_gain_host applied to the output of vr_smooth_host.
 * State left.  That of vr_sync_volumes of the host-filtered volume, bit for bit: the padded data with its
 * apron (the edge replicate of the written interior), nonfinite and maxabs of the final values, a rebuilt
 * occupancy map (the support grows by R), a new upload version.  What is smoothed is the buffer the
 * handle's last vr_sync_volumes bound as emission; an absorption or reflection that aliases it follows; a
 * separately uploaded volume, the gradient volumes of lookup mode and the LUT are not touched.
 * When.  Eagerly inside vr_set_smoothing, at the end of vr_sync_volumes (also per channel in
 * vr_render_channels), inside vr_sync_labels and vr_set_label_gains; nothing is written when nothing
 * changed.  A rewrite waits for every launch that reads the buffer, so a *_device call in flight sees the
 * volume it was launched on.  A failed pass leaves the unmodified upload behind, and a vr_set_smoothing that
 * failed so leaves no sigma set.
 * Memory.  While a sigma is set the one unmodified copy, shared with the label gains, counts in the
 * handle's required memory; during a derivation of more than one pass one further scratch volume comes from
 * the buffer pool and goes back afterwards.  When they do not fit: VR_ERR_VRAM, and the state stays as it
 * was.  'mem_info' has a line for the smoothing while one is set.
 * Errors.  Checked before the handle (they need no device), each VR_ERR_ARGUMENT: a NaN, negative or
 * infinite sigma; a sigma above VR_SMOOTH_MAX_SIGMA.  VR_ERR_UNSUPPORTED, the message names the smoothing:
 * a non-zero sigma on a multi-device group handle; vr_render_slab on a handle with smoothing set (a slab's
 * z border would be clamped where the whole volume has neighbouring planes).  With no smoothing set every
 * call allocates, uploads and launches what it does without this feature. */
#define VR_SMOOTH_MAX_SIGMA 6.0f /* radius ceil(2 sigma) <= 12 */
int vr_set_smoothing(vr_context *h, const float sigma[3]); /* NULL or all zero clears */
int vr_get_smoothing(vr_context *h, float sigma[3]);

/* The value rule above on the CPU (needs no device), by the inline functions the kernels evaluate
 * (csrc/vr_smooth.h).  vr_smooth_weights_host: *radius = R and w[0..2R] for one sigma (room for 25;
 * sigma = 0: R = 0, w[0] = 1).  vr_smooth_host: dst = src smoothed, both dense dims[0] x dims[1] x dims[2]
 * column-major (dims[0] fastest); dst may be src.  The sigma checks of vr_set_smoothing; a NULL pointer is
 * VR_ERR_ARGUMENT. */
int vr_smooth_weights_host(float sigma, int32_t *radius, float *w /* room for 25 */);
int vr_smooth_host(const float *src, const uint64_t dims[3], const float sigma[3], float *dst);

/* --- Richardson-Lucy deconvolution of the resident emission volume (no reference counterpart; on the host
 * it is deconvlucy(Data, psf, n) with a Gaussian PSF whose axial sigma exceeds the lateral one, and a full
 * re-upload) ---------------------------------------------------------------------------------------------
 * sigma[j] (the PSF's width in voxels along dims[j] of Data), the iteration count and the floor are state of
 * the handle.  The resident emission buffer, its upload statistics and its occupancy map are re-derived on
 * the device from the unmodified upload, the deconvolution in front of the other derived steps:
 * unmodified upload -> deconvolution -> smoothing -> label gains -> resident buffer.  Every render, slice
 * and histogram call reads an ordinary resident volume and is unchanged.
 * Value.  Let B(x) be exactly vr_smooth_host(x, sigma): the weights of vr_smooth_weights_host
 * (R = ceil(2 sigma)), the one-axis pass of the smoothing along dims[0], dims[1], dims[2] in that order,
 * indices clamped at the border, an axis with sigma 0 or one voxel skipped.  With y the unmodified upload
 * (after the widening of a typed upload), n = iterations and every operation rounded once to fp32:
 *     d = (y < 0.f) ? 0.f : y                     (NaN and -0 pass through)
 *     u_0 = d
 *     for k = 0 .. n-1:   c = B(u_k)
 *                         g = (c > floor) ? c : floor      (a NaN in c gives floor)
 *                         r = d / g                        (one correctly rounded fp32 division)
 *                         m = B(r)
 *                         u_{k+1} = u_k * m
 * and the resident voxel is u_n.  The correlation step m = B(r) uses the same clamped filter as the blur:
 * with symmetric weights that is the adjoint of B away from the border and not at it (within R voxels of a
 * face the clamped filter's transpose would weigh the edge voxels differently; an exact border adjoint is
 * not provided).  Nothing is flushed or tested beyond what is written above; NaN, inf, +-0 and subnormals
 * follow IEEE.  No bit depends on how the kernels tile their work, on which buffers the iteration rotates
 * through, or on whether an elementwise step is fused into a filter pass.  When every axis with a sigma
 * has one voxel B is the identity and the iteration is still evaluated as written.  Smoothing and label
 * gains apply to u_n: the result equals vr_label_gain_host(vr_smooth_host(vr_deconvolve_host(y))).
 * Off.  With iterations = 0, with every sigma zero or with sigma NULL no deconvolution is set (the getter
 * then reports zeros), and every call does what it does without this feature.
 * State left.  That of vr_sync_volumes of the host-deconvolved volume, bit for bit: the padded data with its
 * apron (the edge replicate of the written interior), nonfinite and maxabs of the final values, a rebuilt
 * occupancy map, a new upload version.  What is deconvolved is the buffer the handle's last
 * vr_sync_volumes bound as emission; an absorption or reflection that aliases it follows; a separately
 * uploaded volume, the gradient volumes of lookup mode and the LUT are not touched.
 * When.  Eagerly inside vr_set_deconvolution, at the end of vr_sync_volumes (also per channel in
 * vr_render_channels), inside vr_set_smoothing, vr_sync_labels and vr_set_label_gains (they derive again
 * from the upload, the iterations included); nothing is written when nothing changed.  A rewrite waits for
 * every launch that reads the buffer, so a *_device call in flight sees the volume it was launched on.  A
 * failed pass leaves the unmodified upload behind, and a vr_set_deconvolution that failed so leaves no
 * deconvolution set.
 * Memory.  While a deconvolution is set the one unmodified copy, shared with the smoothing and the label
 * gains, counts in the handle's required memory; during a derivation one scratch volume, and a second one
 * when more than one axis is filtered, come from the buffer pool and go back afterwards (the estimate
 * lives in the resident buffer or the first scratch volume, and the update may write the buffer it reads).
 * When they do not fit: VR_ERR_VRAM, and the state stays as it was.  'mem_info' has a line for the
 * deconvolution while one is set.
 * Errors.  Checked before the handle (they need no device), each VR_ERR_ARGUMENT: a NaN, negative or
 * infinite sigma; a sigma above VR_SMOOTH_MAX_SIGMA; iterations outside 0..VR_DECONV_MAX_ITERATIONS; a
 * floor that is not finite and greater than 0 (also when the call clears).  VR_ERR_UNSUPPORTED, the message
 * names the deconvolution: setting one on a multi-device group handle; vr_render_slab on a handle with one
 * set (a slab's z border would be clamped where the whole volume has neighbouring planes). */
#define VR_DECONV_MAX_ITERATIONS 64
int vr_set_deconvolution(vr_context *h, const float sigma[3], int32_t iterations, float floor); /* NULL, zeros or 0 iterations clear */
int vr_get_deconvolution(vr_context *h, float sigma[3], int32_t *iterations, float *floor);

/* The value rule above on the CPU (needs no device), by vr_smooth_host's one-axis pass and the inline
 * functions the kernels evaluate (csrc/vr_deconv.h): dst = u_n of src, both dense dims[0] x dims[1] x
 * dims[2] column-major; dst may be src.  iterations = 0 or every sigma zero: a bit-exact copy.  The argument
 * checks of vr_set_deconvolution; a NULL pointer is VR_ERR_ARGUMENT. */
int vr_deconvolve_host(const float *src, const uint64_t dims[3], const float sigma[3], int32_t iterations, float floor,
                       float *dst);

/* --- slice views: axis-aligned, oblique and thick-slab sections of a resident volume (no reference
 * counterpart; MATLAB's sliceViewer / obliqueslice, a radiologist's MPR) ------------------------------
 * The sampler of every render evaluated on a plane instead of along camera rays: what the renderer shows
 * -- typed uploads widened, label gains applied -- not what the host array holds.  No camera is involved.
 * Coordinates.  q is the normalized volume coordinate in the dimension order of Data, exactly the
 * coordinate of the clip planes (q_j from 0 to 1 across dims[j], the centre of voxel i at (i + 0.5) / d_j):
 * the sampler's own argument.  Sample k of the pixel in row y, column x, in fp32 with every operation
 * rounded once:
 *   p_j  = fmaf(dv_j, (float)y, fmaf(du_j, (float)x, origin_j));
 *   q_kj = fmaf(dw_j, (float)k, p_j)
 * -- no recurrence, so no bit depends on how the kernel orders or batches the samples.  A sample is inside
 * iff q_kj >= 0 && q_kj <= 1 for j = 0, 1, 2 (a NaN coordinate is outside).  Outside samples are skipped,
 * not clamped.  An inside sample is v_k = tex3d(source texture, q_k0, q_k1, q_k2) with the clamp addressing
 * and the 8-bit weights of every other render.
 * Source.  The texture a 'render' on this handle would sample as emission, absorption or reflection: the
 * slot indices, the alias rule and the module-global bindings included (the last vr_sync_volumes on any
 * handle decides what is bound; as in 'render', the absorption index follows the reference: it points at
 * the emission texture unless the alias rule moved it, also after a separate absorption volume was
 * synced); an unbound texture reads 0, a 1x1x1 texture gives its voxel through the lerp algebra.  The emission source is the resident buffer: label gains show, a typed upload shows as
 * widened.  Clip planes set on the handle are ignored: the slice is itself the cut.
 * Reduction over k = 0 .. n-1, in this order:
 *   VR_SLICE_MAX  m = -inf; an inside sample with v_k > m (strictly: the first maximum wins, a NaN never
 *                 does) sets m = v_k, kk = k.  pixel = m + 0.0f (-0 becomes +0), aux = (float)kk; with no
 *                 winner both are NaN.
 *   VR_SLICE_MIN  the mirror image: m = +inf, v_k < m.
 *   VR_SLICE_SUM  s = 0, c = 0; per inside sample s = s + v_k (one fp32 addition each) and ++c.
 *                 pixel = c > 0 ? s : NaN, aux = (float)c (the mean is pixel ./ aux).
 *   label plane   at the centre sample kc = (n - 1) / 2 (integer division): if it is inside and labels
 *                 are resident (vr_sync_labels), (float)labels[i0 + D0 * (i1 + D1 * i2)] with
 *                 i_j = min((int)(q_j * (float)D_j), D_j - 1), D the label volume's own dims; otherwise
 *                 NaN.  Without labels the whole plane is NaN.
 * Outputs.  Planes [H, W] column-major (out[x * H + y]) like the projections' aux plane; out_aux and
 * out_labels may be NULL.
 * Errors, checked before the handle (no device needed), each VR_ERR_ARGUMENT: s NULL; a non-finite
 * component of origin / du / dv / dw; samples outside 1 .. VR_SLICE_MAX_SAMPLES; an unknown mode or source;
 * H * W >= 2^31.  A NULL out / d_out with a non-empty image is VR_ERR_ARGUMENT; a multi-device group
 * handle is VR_ERR_UNSUPPORTED.  The call writes nothing of the handle's state: a 'render' before and
 * after it gives the same bits.  The device variant is asynchronous on `stream` and registers its reads
 * like the other *_device calls: a label-gain rewrite waits for it, so a slice in flight shows the gains
 * that were set when it was launched.  VR_SLICE_LANES=x|y (a test switch) forces which output axis runs
 * along a wave's lanes; no bit depends on it. */
enum vr_slice_mode { VR_SLICE_MAX = 0, VR_SLICE_MIN = 1, VR_SLICE_SUM = 2 };
enum vr_slice_source { VR_SLICE_EMISSION = 0, VR_SLICE_ABSORPTION = 1, VR_SLICE_REFLECTION = 2 };
#define VR_SLICE_MAX_SAMPLES 4096
typedef struct vr_slice {
  float origin[3];        /* q of output pixel (row 0, column 0), slab sample 0 */
  float du[3];            /* q step per output column x */
  float dv[3];            /* q step per output row y    */
  float dw[3];            /* q step per slab sample k   */
  uint64_t resolution[2]; /* [H W], as vr_render_args.resolution */
  int32_t samples;        /* n, 1 .. VR_SLICE_MAX_SAMPLES; 1 = a plain slice */
  int32_t mode;           /* vr_slice_mode */
  int32_t source;         /* vr_slice_source */
  int32_t reserved;
} vr_slice;

/* Into the caller-owned host planes out[H*W] and, where not NULL, out_aux[H*W], out_labels[H*W]. */
int vr_render_slice(vr_context *h, const vr_slice *s, float *out, float *out_aux, float *out_labels);

/* Into device memory on `stream` (asynchronous, as vr_render_device). */
int vr_render_slice_device(vr_context *h, const vr_slice *s, float *d_out, float *d_aux, float *d_labels,
                           void *stream);

/* Two host helpers that fill in a vr_slice's geometry and samples (mode, source and reserved are left as
 * they are); they need no device.  Everything is computed in double and rounded once to fp32.
 * vr_slice_axis: the voxel plane at 0-based `index` (fractions allowed) along `axis` (0, 1, 2) of a volume
 * of `dims`, one output pixel per voxel at the voxel centres: with (a, b) the two remaining dimensions,
 * a < b, rows run along a (H = dims[a], dv_a = 1 / dims[a]) and columns along b (W = dims[b]); the slab
 * of `thickness` samples one voxel apart is centred on `index`: sample k at voxel index
 * index - (thickness - 1) / 2 + k along `axis`.  VR_ERR_ARGUMENT: dims or out NULL, a zero dim, an axis
 * outside 0..2, a non-finite index, a thickness outside 1 .. VR_SLICE_MAX_SAMPLES.
 * vr_slice_oblique: an H x W plane through point_q (the image centre, (H - 1) / 2 and (W - 1) / 2, of the
 * slab's middle (thickness - 1) / 2) that is orthonormal in physical space: with the physical position
 * of q along dims[j] being q_j * dims[j] * element_size_um[2 - j] (element_size_um in MATLAB order, as in
 * vr_render_args), w = normal / |normal|, the row direction v = up projected into the plane, normalized,
 * the column direction u = v x w; pixels pixel_um apart in the plane and slab samples pixel_um apart along
 * w.  normal_um and up_um are physical directions with component j along dims[j].  VR_ERR_ARGUMENT: a
 * NULL pointer, a zero dim, a non-positive or non-finite element size or pixel_um, non-finite inputs, a
 * zero normal, an up parallel to the normal (or zero), H * W >= 2^31, thickness outside
 * 1 .. VR_SLICE_MAX_SAMPLES. */
int vr_slice_axis(const uint64_t dims[3], int32_t axis, double index, uint64_t thickness, vr_slice *out);
int vr_slice_oblique(const uint64_t dims[3], const float element_size_um[3], const double point_q[3],
                     const double normal_um[3], const double up_um[3], double pixel_um, uint64_t H, uint64_t W,
                     uint64_t thickness, vr_slice *out);

/* --- volume histogram and per-label statistics of a resident source texture (no reference counterpart;
 * MATLAB's histcounts(Data(:)) on the host array) -------------------------------------------------------
 * The numbers an isosurface level, a transfer function's limits or a label gain are chosen from, taken
 * from what the renderer holds -- typed uploads widened, label gains applied -- not from the host array.
 * Voxels.  The d0*d1*d2 interior voxels of the source texture's padded resident buffer; apron voxels are
 * never counted.  The source is resolved exactly as vr_render_slice resolves it (slot indices, alias rule,
 * module-global bindings).  A 1x1x1 texture contributes its one voxel; an unbound texture contributes
 * nothing: all counts 0, every total 0, min = max = NaN, sum = 0.
 * Class of a voxel v, in fp32 with every operation rounded once (csrc/vr_histogram.h, one inline function
 * that the kernel and vr_histogram_bin_host both evaluate), inv = 1.0f / (hi - lo) formed once on the host:
 *   NaN -> nan;  v < lo -> below;  v > hi -> above;  otherwise
 *   x = ((v - lo) * inv) * (float)nbins,  b = min((int)x, nbins - 1)
 * so v == hi falls in the last bin, as MATLAB's histcounts does.  ninf counts the +-inf voxels, which are
 * also counted in below / above.  total = nan + below + above + the sum of the row's bins.
 * Extrema.  min / max over the row's non-NaN voxels, inf included, compared in IEEE totalOrder (-0 below
 * +0), so the result bits do not depend on the visiting order; NaN for both in a row without such a voxel.
 * Sum.  The double-precision sum of the row's finite voxels (the conversion from fp32 is exact); the order
 * of the additions is the kernel's own and may differ between runs -- the one field that is not
 * reproducible bit for bit.
 * Rows.  label_count = 0: one row, the labels are not read.  label_count = n in 1..256: the voxel with
 * label l goes to row (uint8)(l - label_first) < n ? l - label_first : n, i.e. rows 0..n-1 are the labels
 * label_first .. label_first+n-1 and row n collects every other label; rows = n + 1.  This needs resident
 * labels (vr_sync_labels) whose dims equal the source texture's.
 * Clip.  With use_clip and planes set on the handle (vr_set_clip) only voxels whose centre every plane
 * keeps are counted: q_j = ((float)i_j + 0.5f) / (float)d_j (one IEEE division per axis), kept iff
 * fmaf(n2, q2, fmaf(n1, q1, fmaf(n0, q0, offset))) >= 0 for every plane as it was set (a NaN is not kept).
 * With no planes set use_clip changes nothing.
 * Outputs.  counts[r * nbins + b], fully overwritten by each call; rows_out[r] (may be NULL).  The device
 * variant is asynchronous on `stream` and registers its reads of the source buffer and of the labels like
 * the other *_device calls, so a label-gain rewrite or a label upload waits for it; d_rows holds final
 * floats, not keys.
 * Errors, checked before the handle (no device needed), each VR_ERR_ARGUMENT: q NULL; an unknown source;
 * nbins outside 1 .. VR_HIST_MAX_BINS; non-finite limits, !(lo < hi), hi - lo or 1 / (hi - lo) not finite;
 * label_first outside 0..255, label_count outside 0..256 or label_first + label_count > 256;
 * rows * nbins > VR_HIST_MAX_CELLS; use_clip not 0 / 1; counts / d_counts NULL.  label_count > 0 without
 * resident labels, or with labels whose dims differ from the source's, is VR_ERR_ARGUMENT with a message
 * that names the labels.  A multi-device group handle is VR_ERR_UNSUPPORTED.  The call writes nothing of
 * the handle's state: a 'render' before and after it gives the same bits.  VR_HIST_UNIFORM=0|1 (a test
 * switch) forces the kernel's wave-uniform shortcut off or on; no count depends on it. */
#define VR_HIST_MAX_BINS  4096
#define VR_HIST_MAX_CELLS 12288          /* rows * nbins; 48 KiB of uint32 in LDS */
typedef struct vr_histogram {
  int32_t source;       /* vr_slice_source: EMISSION / ABSORPTION / REFLECTION, resolved exactly as vr_render_slice does */
  int32_t nbins;        /* 1 .. VR_HIST_MAX_BINS */
  float   lim[2];       /* lo < hi, both finite, hi - lo finite */
  int32_t label_first;  /* 0 .. 255 */
  int32_t label_count;  /* 0: one row, labels not read.  n in 1..256: rows 0..n-1 are labels
                           label_first .. label_first+n-1, row n collects every other label; rows = n + 1 */
  int32_t use_clip;     /* 0 / 1: count only voxels whose centre the handle's clip planes keep */
  int32_t reserved;
} vr_histogram;
typedef struct vr_hist_row {
  uint64_t total, below, above, nan, ninf;
  float min, max;
  double sum;
} vr_hist_row;

/* Into the caller-owned host arrays counts[rows * nbins] and, where not NULL, rows_out[rows]. */
int vr_volume_histogram(vr_context *h, const vr_histogram *q, uint64_t *counts /* [rows][nbins] */,
                        vr_hist_row *rows_out /* [rows], may be NULL */);

/* Into device memory on `stream` (asynchronous, as vr_render_device). */
int vr_volume_histogram_device(vr_context *h, const vr_histogram *q, unsigned long long *d_counts,
                               vr_hist_row *d_rows /* may be NULL */, void *stream);

/* The class rule above on the CPU (needs no device): bin[i] = the bin of v[i], or -1 below, -2 above,
 * -3 NaN, for m values.  The nbins and limit checks above; a NULL v, bin or lim with m > 0 is
 * VR_ERR_ARGUMENT. */
int vr_histogram_bin_host(const float *v, uint64_t m, int32_t nbins, const float lim[2], int32_t *bin /* [m] */);

/* The kernel's table lookup on the CPU (needs no device): out[k * m + j] = L(table plane k, n, lim,
 * c[j]) for the ncomp planes table[k * n + i].  VR_ERR_ARGUMENT for a NULL pointer with m > 0, an n
 * outside 2..VR_TF_MAX_ENTRIES, ncomp < 1, or limits that are not finite with lo < hi. */
int vr_transfer_lookup_host(const float *table, int32_t n, int32_t ncomp, const float lim[2], const float *c,
                            uint64_t m, float *out /* [ncomp][m] */);

/* Number of columns a part owns for image width w. */
int64_t vr_partition_columns(int64_t w, const vr_partition *part);

/* Scatter gathered part images (num_parts slabs of max_cols*H*3 floats each, part p at
 * d_parts + p*max_cols*H*3) into the full [H, W, 3] image d_out, on `stream`. */
int vr_assemble_partitions(const float *d_parts, int64_t w, int64_t h, int32_t block_cols,
                           int32_t num_parts, int64_t max_cols, float *d_out, void *stream);

/* --- sort-last slabs (volumes larger than one GPU; no MATLAB counterpart: the
 * reference aborts when a volume does not fit, mmanager.hxx:144-173) ----------------------------
 * The bound emission volume (the last vr_sync_volumes on any handle, as for vr_render) holds
 * planes [z_first, z_first + d2) of a volume of depth `depth` (d0, d1 as synced).  The render marches every ray of the full W x H image over the
 * samples it owns, those with z0 <= p.z * depth < z1 (p the normalized sample position; z0 = -inf
 * / z1 = +inf for the end slabs), with positions, step counts and early exit exactly as the
 * one-volume march.  part (NULL = the whole image) restricts the render to the columns of an
 * image partition (the tiles of a pipelined multi-GPU sweep).  Ray state: VR_SLAB_PLANES planes
 * of cols*H floats, [c][local column][y] (cols = vr_partition_columns): premultiplied r, g, b,
 * alpha; 1 if the ray continues past this slab; and for such a ray its resume point -- t, the
 * position x, y, z and the sample index (int32 bits) of its next sample -- from which the next
 * slab continues the march without replaying it.  d_state_in NULL = fresh rays, may equal
 * d_state_out.  direction +1 handles the rays with dir.z >= 0 (run the slabs in ascending z),
 * -1 those with dir.z < 0 (descending), 0 both (the top slab, where the descending rays start:
 * its ascending launch marches them too); other rays pass through.  Chaining both sweeps over all
 * slabs gives the one-volume image bit for bit in the first three planes.  Compute gradient or
 * emission-absorption only; absorption must alias emission (the reference's default). */
#define VR_SLAB_PLANES 10
typedef struct vr_slab {
  uint64_t depth;    /* global depth D of the emission volume                          */
  uint64_t z_first;  /* global index of the first synced plane                         */
  double z0, z1;     /* owned range of p.z * D                                         */
  int32_t direction; /* +1 / -1 / 0                                                     */
  int32_t reserved;
} vr_slab;
int vr_render_slab(vr_context *h, const vr_render_args *args, const vr_slab *slab, const vr_partition *part,
                   const float *d_state_in, float *d_state_out, void *stream);

/* Planes [*first, *first + *count) of a volume of dims (d0, d1, D) a slab owning [z0, z1) must
 * hold: the trilinear taps and the gradient taps of its samples (element size in MATLAB order). */
int vr_slab_planes(const uint64_t dims[3], const float element_size_um[3], double z0, double z1, uint64_t *first,
                   uint64_t *count);

/* Depth lanes (lanes per ray) the march kernel uses for a launch of part_cols x
 * height rays on the current device at about one texel per pixel: 1, 2, 4 or 8 (VR_DEPTH_LANES
 * overrides).  A render also weighs the texels its pixels span (denser sampling: more lanes).
 * Launches with few waves per wave slot of the device also follow a longest-first schedule. */
int vr_depth_lanes(int64_t part_cols, int64_t height);
/* The same for a render whose pixels span `texels_per_pixel` texels at the volume
 * (dist * d0 / (W * f) for the reference's camera). */
int vr_depth_lanes_tau(int64_t part_cols, int64_t height, double texels_per_pixel);

/* Synthetic test volume V_shell(n) of SURVEY.md 8d, generated on the device into d_out[n^3]. */
int vr_synth_shell_device(float *d_out, uint64_t n, void *stream);

/* Planes [z_first, z_first + count) of V_shell(n) into d_out[n*n*count] (a sort-last slab's share). */
int vr_synth_shell_planes_device(float *d_out, uint64_t n, uint64_t z_first, uint64_t count, void *stream);

/* Volume.grad on the device (Volume.m:181-205, MATLAB gradient() of single data): for the
 * column-major d_data[d0*d1*d2] writes d_gx (along dim 2), d_gy (along dim 1), d_gz (along dim 3),
 * central differences inside and one-sided at the ends, bit-identical to MATLAB's single-precision
 * gradient.  All pointers are device memory; asynchronous on `stream`. */
int vr_gradient_device(const float *d_data, const uint64_t dims[3], float *d_gx, float *d_gy, float *d_gz,
                       void *stream);

/* --- the MATLAB-side volume preprocessing on the device ----------------- */

/* HenyeyGreenstein(N, g) (HenyeyGreenstein.cc:29-96) into device memory d_out[N*N*N], same layout as
 * vr_henyey_greenstein.  The sines / cosines are the host generator's; the power of 3 comes from the
 * device math library, so elements can differ from the host LUT in the last bits (measured at
 * most 3 ulp, ~91 % bit-identical; tests/test_volume_ops.py bounds it at 4 ulp).  Returns when the LUT is written. */
int vr_henyey_greenstein_device(uint32_t n, float g, float *d_out, void *stream);

/* Volume.normalize(newMin, newMax) (Volume.m:208-220) of n single values on the device:
 * (x - min) * single(newMax - newMin) / (max - min) + single(newMin) in MATLAB's single arithmetic,
 * min / max omitting NaN.  d_out may equal d_in.  Asynchronous on `stream`. */
int vr_normalize_device(const float *d_in, uint64_t n, double new_min, double new_max, float *d_out, void *stream);

/* Volume.resize(newsize) (Volume.m:93-106: imresize3, or imresize for 2-D data) of a column-major
 * (d0, d1, d2) single volume on the device into d_out[out0*out1*out2]: MATLAB's default cubic
 * kernel, antialiasing when shrinking, mirrored ends, separable passes (double accumulation, single
 * result) along the axes in order of increasing scale.  Returns when done. */
int vr_resize_device(const float *d_in, const uint64_t in_dims[3], const uint64_t out_dims[3], float *d_out,
                     void *stream);

/* The weights / 0-based indices of one resize axis (out_len x *P, row-major), for tests. */
int vr_resize_contributions(uint64_t in_len, uint64_t out_len, int32_t *P, double *w, int32_t *idx);

/* Host-side reproduction of the upload/slot state machine (syncWithDevice,
 * volumeRender_kernel.cu:739-867) for unit tests: returns the slot indices after a sync with the
 * given similarity/update flags starting from `idx` (emission, absorption, reflection). */
int vr_debug_slot_transition(const int32_t idx_in[3], int32_t sim_em_ab, int32_t sim_em_re,
                             int32_t sim_ab_re, int32_t req_em, int32_t req_ab, int32_t req_re,
                             int32_t idx_out[3], int32_t unbound_out[3]);

/* Last error message of this thread ("" if none). */
const char *vr_last_error(void);

/* HIP errors the library did not return to a caller (process-wide; the reference ignores every CUDA
 * error, common.h:43-47): errors of its own calls that it handled with a fallback (an optional
 * buffer, a launch schedule, timing events, an already enabled peer mapping) and errors found
 * pending in the calling thread's HIP error state at an API entry (raised elsewhere; a device fault
 * found there fails that call with VR_ERR_DEVICE).  Every other HIP error fails the call that met
 * it.  Returns how many since the library was loaded and writes the last (up to 32) into buf, one
 * per line, newest last: "<kind>: <hipError name> (<code>) at <site>". */
int64_t vr_hip_errors(char *buf, size_t buflen);

/* The demangled name of the march kernel instantiation the last render launched (the process's
 * last staged-march launch), e.g. "vr::fast::march_kernel<2, 1, true, false, true, false, 1664, 0>":
 * bench.py names the kernel it times with it and keys the profiler's counters to it. */
int vr_last_march_kernel(char *buf, size_t buflen);

/* The launch-wide decisions of the last frame this process built (vr_capi.hip build_frame: every
 * render call builds one per view before it launches), one bit each.  The host takes them from the
 * upload statistics of the bound buffers, the factors, the colours and the bindings, and the kernels
 * trust them (DESIGN.md "Launch-wide decisions"); the tests read them back to assert which side of a
 * decision a scene took.  Read-only: nothing is selected through this call. */
enum vr_launch_flag {
  VR_LF_TAME = 1 << 0,       /* every flag below up to LUT_OK holds and tstep is finite and positive: the march
                                runs without per-sample range and coordinate tests, and probes, leaps and pre-leaps */
  VR_LF_SMALL_X = 1 << 1,    /* every |Fa * ab(p) * tstep| < 2^-7: the exponential's Taylor form, no range test */
  VR_LF_EDS_FINITE = 1 << 2, /* every |Fe * em(p) * tstep| is finite */
  VR_LF_SKIP_EMPTY = 1 << 3, /* skip_empty is non-zero: a sample with alpha == 0 is an exact no-op and is skipped */
  VR_LF_RE_OK = 1 << 4,      /* the reflection texture is the emission texture or a single voxel */
  VR_LF_LUT_OK = 1 << 5,     /* no lights, or a small, z-paired, non-1x1x1 LUT of at most 8192 texels per axis */
  VR_LF_TAP_HALF = 1 << 6,   /* the on-the-fly gradient's taps lie exactly half a texel from the centre */
  VR_LF_AB_ALIAS = 1 << 7,   /* the absorption texture is the emission texture */
  VR_LF_SHARE = 1 << 8,      /* the gradient reads share the centre sample's axes */
  VR_LF_BIG = 1 << 9,        /* 64-bit texture offsets */
  VR_LF_OCC = 1 << 10        /* an occupancy map is bound (the emission buffer has one) */
};
int vr_last_launch_flags(uint32_t *flags);

/* Process-wide options (round 6; no reference counterpart).  "test_switches" = 1 lets the library
 * read the kernel-variant and schedule switches the GPU tests and the measurement tools set through
 * the environment (VR_NO_LDS, VR_DEPTH_LANES, VR_SCHED, ... -- INTEGRATION.md "Runtime switches");
 * by default (0) they are ignored, so a MATLAB session's environment cannot select them.  Returns
 * VR_ERR_ARGUMENT for an unknown name. */
int vr_set_option(const char *name, int64_t value);

/* Library build identification ("libvrhip <version> gfx950 ..."). */
const char *vr_version(void);

#ifdef __cplusplus
}
#endif
#endif /* VRHIP_H_ */
