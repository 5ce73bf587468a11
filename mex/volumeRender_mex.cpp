// volumeRender_mex.cpp -- the MATLAB-side binding of libvrhip.so: a mexFunction named
// `volumeRender` that keeps the reference's command protocol (src/C/mex/render.cpp:50-278) so that
// VolumeRender.m / Volume.m / LightSource.m run unchanged on MI355X.
//
// Built here only against the test stand-in of MATLAB's API (tests/mexstub/: a test-only mex.h and
// mxArray model, driven by tests/test_mex_adaptor.py); a maintainer builds the real MEX with
//   mex -R2018a -I<repo>/include -L<repo>/volume_renderer_amd -lvrhip volumeRender_mex.cpp -output volumeRender
// and puts the result where src/make.m put the CUDA mex (src/matlab/VolumeRender/).  See
// INTEGRATION.md.  All marshalling permutations (reversed ElementSizeUm and light positions,
// flip(R) un-flipping, [H W] order) happen inside libvrhip exactly as the reference's mex did them;
// this file only unpacks mxArrays into the C-ABI structs of include/vrhip.h.
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "mex.h"
#include "vrhip.h"

namespace {

[[noreturn]] void fail(int rc) {
  const char *msg = vr_last_error();
  mexErrMsgTxt((msg && *msg) ? msg : (rc == VR_ERR_HANDLE ? "Handle not valid." : "volumeRender failed"));
  throw 0;  // not reached: mexErrMsgTxt does not return
}

void check(int rc) {
  if (rc != VR_OK) fail(rc);
}

// A MATLAB `Volume` object (Data, TimeLastUpdate uint64), borrowed for this call.  Data is single,
// or uint8 / uint16 / int16 (vr_dtype: widened to single on the device during the upload).  The
// Volume class itself casts to single, so integer data comes from a RawVolume (mex/matlab/
// RawVolume.m): when the object has a non-empty RawData it is taken instead of Data, with the
// logical Unorm selecting single(x) / single(255 resp. 65535).
vr_volume make_volume(const mxArray *obj) {
  const mxArray *data = mxGetPropertyShared(obj, 0, "Data");
  const mxArray *stamp = mxGetPropertyShared(obj, 0, "TimeLastUpdate");
  const mxArray *raw = mxGetPropertyShared(obj, 0, "RawData");
  bool unorm = false;
  if (raw && mxGetNumberOfElements(raw) > 0) {
    data = raw;
    const mxArray *u = mxGetPropertyShared(obj, 0, "Unorm");
    unorm = u && mxGetNumberOfElements(u) > 0 && mxGetScalar(u) != 0.0;
  }
  vr_volume v{};
  switch (data ? mxGetClassID(data) : mxUNKNOWN_CLASS) {
    case mxSINGLE_CLASS: v.dtype = VR_F32; break;
    case mxUINT8_CLASS: v.dtype = VR_U8; break;
    case mxUINT16_CLASS: v.dtype = VR_U16; break;
    case mxINT16_CLASS: v.dtype = VR_I16; break;
    default: mexErrMsgTxt("Volume.Data must be single.");
  }
  if (unorm) v.dtype |= VR_DTYPE_UNORM;  // (the library rejects it on int16 / single)
  v.data = static_cast<const float *>(mxGetData(data));
  const mwSize nd = mxGetNumberOfDimensions(data);
  const mwSize *d = mxGetDimensions(data);
  v.dims[0] = d[0];
  v.dims[1] = nd > 1 ? d[1] : 1;
  v.dims[2] = nd > 2 ? d[2] : 1;
  v.last_update = stamp ? (uint64_t)mxGetScalar(stamp) : 0;
  v.location = VR_HOST;
  return v;
}

vr_context *handle(const mxArray *a) {
  if (mxGetNumberOfElements(a) != 1 || mxGetClassID(a) != mxUINT64_CLASS || mxIsComplex(a))
    mexErrMsgTxt("Input must be a real uint64 scalar.");
  return reinterpret_cast<vr_context *>(*static_cast<uint64_t *>(mxGetData(a)));
}

template <typename T>
const T *data_of(const mxArray *a, size_t n, const char *what) {
  if (mxGetNumberOfElements(a) < n) mexErrMsgTxt(what);
  return static_cast<const T *>(mxGetData(a));
}

// The 'render' arguments Lights, Illum, factors, ElementSizeUm, [H W], flip(R), props, thr, Color
// (render.cpp:134-221), p[0] = Lights.  `lights` / `illum` own what a.lights / a.illumination point to.
void unpack_render(const mxArray *const *p, vr_render_args &a, std::vector<vr_light> &lights, vr_volume &illum) {
  a = vr_render_args{};
  const bool lit = !(mxIsClass(p[0], "logical") || mxIsClass(p[1], "logical"));
  if (lit) {
    const size_t n = mxGetN(p[0]);
    lights.resize(n);
    for (size_t l = 0; l < n; ++l) {
      const float *pos = static_cast<const float *>(mxGetData(mxGetProperty(p[0], l, "Position")));
      const float *col = static_cast<const float *>(mxGetData(mxGetProperty(p[0], l, "Color")));
      memcpy(lights[l].position, pos, sizeof(lights[l].position));
      memcpy(lights[l].color, col, sizeof(lights[l].color));
    }
    illum = make_volume(p[1]);
    a.lights = lights.data();
    a.num_lights = (int64_t)n;
    a.illumination = &illum;
  } else {
    a.num_lights = -1;  // the logical `false`
    a.illumination = nullptr;
  }
  memcpy(a.factors, data_of<float>(p[2], 3, "factors: 3 singles expected"), sizeof(a.factors));
  memcpy(a.element_size_um, data_of<float>(p[3], 3, "ElementSizeUm: 3 singles expected"),
         sizeof(a.element_size_um));
  memcpy(a.resolution, data_of<uint64_t>(p[4], 2, "resolution: uint64 [H W] expected"), sizeof(a.resolution));
  memcpy(a.rotation_flipped, data_of<float>(p[5], 9, "rotation: 3x3 single expected"), sizeof(a.rotation_flipped));
  memcpy(a.props, data_of<float>(p[6], 3, "properties: 3 singles expected"), sizeof(a.props));
  a.opacity_threshold = (float)mxGetScalar(p[7]);
  memcpy(a.color, data_of<float>(p[8], 3, "Color: 3 singles expected"), sizeof(a.color));
}

mxArray *new_image(const vr_render_args &a, mwSize views) {
  const mwSize dim[4] = {(mwSize)a.resolution[0], (mwSize)a.resolution[1], 3, views};
  return mxCreateNumericArray(views > 1 ? 4 : 3, dim, mxSINGLE_CLASS, mxREAL);
}

// volumeRender('render_channels', {ch1, ch2, ...}, stereo, base) -> single [H W 3 n*eyes]
// (vr_render_channels; examples/example3.m:61-239 as one call).  A channel is a cell
// {h, TimeLastMemSync, Em, Re, Ab, Lights, Illum, factors, ElementSizeUm, [H W], flip(R), props,
// thr, Color} -- the arguments of its 'sync_volumes' and 'render' -- optionally followed by
// Gx, Gy, Gz (gradient lookup).  Page (i * eyes + e) is channel i's view e; MATLAB adds them.
void render_channels(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nlhs > 1) mexErrMsgTxt("Too many output arguments.");
  if (nrhs < 4 || !mxIsCell(prhs[1])) mexErrMsgTxt("render_channels: {channels}, stereo, base expected");
  const mwSize n = mxGetNumberOfElements(prhs[1]);
  if (n == 0) mexErrMsgTxt("render_channels: no channels");
  const int32_t stereo = mxGetScalar(prhs[2]) != 0.0;
  const float base = (float)mxGetScalar(prhs[3]);
  std::vector<vr_volume> vols(6 * n);
  std::vector<vr_render_args> args(n);
  std::vector<std::vector<vr_light>> lights(n);
  std::vector<vr_volume> illum(n);
  std::vector<vr_channel> ch(n);
  for (mwSize i = 0; i < n; ++i) {
    const mxArray *c = mxGetCell(prhs[1], i);
    const mwSize m = c && mxIsCell(c) ? mxGetNumberOfElements(c) : 0;
    if (m != 14 && m != 17) mexErrMsgTxt("render_channels: a channel is a cell of 14 or 17 elements");
    const mxArray *e[17];
    for (mwSize k = 0; k < m; ++k) e[k] = mxGetCell(c, k);
    ch[i].handle = handle(e[0]);
    ch[i].time_last_mem_sync = (uint64_t)mxGetScalar(e[1]);
    for (int k = 0; k < 3; ++k) vols[6 * i + k] = make_volume(e[2 + k]);
    ch[i].emission = &vols[6 * i];
    ch[i].reflection = &vols[6 * i + 1];
    ch[i].absorption = &vols[6 * i + 2];
    if (m == 17) {
      for (int k = 0; k < 3; ++k) vols[6 * i + 3 + k] = make_volume(e[14 + k]);
      ch[i].dx = &vols[6 * i + 3];
      ch[i].dy = &vols[6 * i + 4];
      ch[i].dz = &vols[6 * i + 5];
    }
    unpack_render(e + 5, args[i], lights[i], illum[i]);
    ch[i].args = &args[i];
  }
  mxArray *img = new_image(args[0], n * (stereo ? 2 : 1));
  check(vr_render_channels(ch.data(), (int32_t)n, stereo, base, static_cast<float *>(mxGetData(img))));
  plhs[0] = img;
}

}  // namespace

void mexFunction(int nlhs, mxArray *plhs[], int nrhs, const mxArray *prhs[]) {
  if (nrhs == 0) mexErrMsgTxt("no parameter!");
  char cmd[64];
  if (mxGetString(prhs[0], cmd, sizeof(cmd)))
    mexErrMsgTxt("First input should be a command string less than 64 characters long.");

  if (!strcmp(cmd, "new")) {
    if (nlhs != 1) mexErrMsgTxt("New: One output expected.");
    vr_context *h = nullptr;
    // VR_DEVICES="0,1,...,7": every render of this handle spans those GPUs (vr_new_multi)
    std::vector<int32_t> devs;
    if (const char *ev = getenv("VR_DEVICES")) {
      for (const char *q = ev; *q;) {
        char *end = nullptr;
        const long d = strtol(q, &end, 10);
        if (end == q) break;
        devs.push_back((int32_t)d);
        q = (*end == ',') ? end + 1 : end;
      }
    }
    check(devs.empty() ? vr_new(&h) : vr_new_multi(devs.data(), (int32_t)devs.size(), &h));
    mexLock();  // the module-global device state must outlive `clear functions`
    plhs[0] = mxCreateNumericMatrix(1, 1, mxUINT64_CLASS, mxREAL);
    *static_cast<uint64_t *>(mxGetData(plhs[0])) = reinterpret_cast<uint64_t>(h);
    return;
  }
  if (!strcmp(cmd, "render_channels")) {
    render_channels(nlhs, plhs, nrhs, prhs);
    return;
  }
  if (nrhs < 2) mexErrMsgTxt("Second input should be a class instance handle.");
  vr_context *h = handle(prhs[1]);

  if (!strcmp(cmd, "delete")) {
    check(vr_delete(h));
    mexUnlock();
    if (nlhs != 0 || nrhs != 2) mexWarnMsgTxt("Delete: Unexpected arguments ignored.");
    return;
  }
  if (!strcmp(cmd, "mem_info")) {
    std::vector<char> buf(1 << 16);
    check(vr_mem_info(h, buf.data(), buf.size()));
    mexPrintf("%s", buf.data());
    return;
  }
  if (!strcmp(cmd, "sync_volumes")) {
    if (nrhs < 6) mexErrMsgTxt("insufficient parameter!");
    const uint64_t t_sync = (uint64_t)mxGetScalar(prhs[2]);
    const vr_volume em = make_volume(prhs[3]), re = make_volume(prhs[4]), ab = make_volume(prhs[5]);
    if (nrhs == 9) {  // gradient volumes given (render.cpp:105-110)
      const vr_volume dx = make_volume(prhs[6]), dy = make_volume(prhs[7]), dz = make_volume(prhs[8]);
      check(vr_sync_volumes(h, t_sync, &em, &re, &ab, &dx, &dy, &dz));
    } else if (nrhs == 6) {  // gradient volumes reset (render.cpp:111-112)
      check(vr_sync_volumes(h, t_sync, &em, &re, &ab, nullptr, nullptr, nullptr));
    } else {  // 7, 8, > 9: the previous gradient volumes are kept; the extra arguments are not read
      const vr_volume unread{};
      check(vr_sync_volumes(h, t_sync, &em, &re, &ab, &unread, nrhs == 7 ? nullptr : &unread, nullptr));
    }
    if (nlhs != 0 || nrhs > 9) mexWarnMsgTxt("SyncVolumes: Unexpected arguments ignored.");
    return;
  }
  if (!strcmp(cmd, "render") || !strcmp(cmd, "render_stereo")) {
    const bool stereo = cmd[6] != '\0';
    if (nlhs > (stereo ? 2 : 1)) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < (stereo ? 12 : 11)) mexErrMsgTxt("insufficient parameter!");
    vr_render_args a;
    std::vector<vr_light> lights;
    vr_volume illum{};
    unpack_render(prhs + 2, a, lights, illum);
    if (!stereo) {
      mxArray *img = new_image(a, 1);
      check(vr_render(h, &a, static_cast<float *>(mxGetData(img))));
      plhs[0] = img;
      return;
    }
    // volumeRender('render_stereo', h, <render args>, base) -> [left, right] (vr_render_stereo;
    // VolumeRender.m:278-307's two renders at camera offsets -base / +base in one launch)
    mxArray *left = new_image(a, 1), *right = new_image(a, 1);
    check(vr_render_stereo(h, &a, (float)mxGetScalar(prhs[11]), static_cast<float *>(mxGetData(left)),
                           static_cast<float *>(mxGetData(right))));
    plhs[0] = left;
    if (nlhs > 1) plhs[1] = right; else mxDestroyArray(right);
    return;
  }
  if (!strcmp(cmd, "render_projection")) {
    // volumeRender('render_projection', h, <render args>, mode) -> [img, aux] (vr_render_projection):
    // mode 'mip' -- the maximum of the emission volume along each ray, aux the depth of the first
    // maximum (NaN: no volume hit) -- or 'sum' -- the ray sum, aux the ray's sample count
    if (nlhs > 2) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 12) mexErrMsgTxt("insufficient parameter!");
    char mode[16];
    if (mxGetString(prhs[11], mode, sizeof(mode))) mexErrMsgTxt("render_projection: mode must be 'mip' or 'sum'");
    int32_t m = VR_PROJ_MIP;
    if (!strcmp(mode, "sum")) m = VR_PROJ_SUM;
    else if (strcmp(mode, "mip")) mexErrMsgTxt("render_projection: mode must be 'mip' or 'sum'");
    vr_render_args a;
    std::vector<vr_light> lights;
    vr_volume illum{};
    unpack_render(prhs + 2, a, lights, illum);
    mxArray *img = new_image(a, 1);
    mxArray *aux = mxCreateNumericMatrix((mwSize)a.resolution[0], (mwSize)a.resolution[1], mxSINGLE_CLASS, mxREAL);
    check(vr_render_projection(h, &a, m, static_cast<float *>(mxGetData(img)), static_cast<float *>(mxGetData(aux))));
    plhs[0] = img;
    if (nlhs > 1) plhs[1] = aux; else mxDestroyArray(aux);
    return;
  }
  if (!strcmp(cmd, "render_slice")) {
    // volumeRender('render_slice', h, geom, res, n, mode, source) -> [img, aux, labels] (vr_render_slice):
    // geom single 3 x 4 [origin du dv dw] in the normalized volume coordinate (dimension order of Data),
    // res uint64 [H W], n slab samples, mode 'max' | 'min' | 'sum', source 'emission' | 'absorption' |
    // 'reflection' (or their codes); aux [H W] the index of the extremum resp. the count of inside samples,
    // labels [H W] the label at the slab's centre sample (NaN: outside, or no labels resident)
    if (nlhs > 3) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 7) mexErrMsgTxt("insufficient parameter!");
    if (nrhs > 7) mexErrMsgTxt("render_slice: too many input arguments");
    const mxArray *g = prhs[2];
    if (mxGetClassID(g) != mxSINGLE_CLASS || mxIsComplex(g) || mxGetNumberOfDimensions(g) != 2 || mxGetM(g) != 3 ||
        mxGetN(g) != 4)
      mexErrMsgTxt("render_slice: geom must be a single 3 x 4 matrix [origin du dv dw]");
    if (mxGetClassID(prhs[3]) != mxUINT64_CLASS || mxGetNumberOfElements(prhs[3]) != 2)
      mexErrMsgTxt("render_slice: res must be uint64 [H W]");
    vr_slice s{};
    const float *gd = static_cast<const float *>(mxGetData(g));
    memcpy(s.origin, gd, sizeof(s.origin));
    memcpy(s.du, gd + 3, sizeof(s.du));
    memcpy(s.dv, gd + 6, sizeof(s.dv));
    memcpy(s.dw, gd + 9, sizeof(s.dw));
    memcpy(s.resolution, mxGetData(prhs[3]), sizeof(s.resolution));
    if (mxGetNumberOfElements(prhs[4]) != 1 || mxIsComplex(prhs[4])) mexErrMsgTxt("render_slice: n must be a real scalar");
    const double n = mxGetScalar(prhs[4]);
    s.samples = (n >= 1.0 && n <= (double)VR_SLICE_MAX_SAMPLES && n == (double)(int32_t)n) ? (int32_t)n : 0;  // (0: refused below)
    // a name or a code; an unknown name becomes the invalid code -1, which the library refuses
    auto code = [](const mxArray *a, const char *const *names, int count, const char *what) -> int32_t {
      char buf[16];
      if (mxGetClassID(a) == mxCHAR_CLASS) {
        if (mxGetString(a, buf, sizeof(buf))) return -1;
        for (int i = 0; i < count; ++i)
          if (!strcmp(buf, names[i])) return i;
        return -1;
      }
      if (mxGetNumberOfElements(a) != 1 || mxIsComplex(a)) mexErrMsgTxt(what);
      const double v = mxGetScalar(a);
      return (v >= 0.0 && v < (double)count && v == (double)(int32_t)v) ? (int32_t)v : -1;
    };
    static const char *const modes[3] = {"max", "min", "sum"};
    static const char *const sources[3] = {"emission", "absorption", "reflection"};
    s.mode = code(prhs[5], modes, 3, "render_slice: mode must be 'max', 'min', 'sum' or a code");
    s.source = code(prhs[6], sources, 3, "render_slice: source must be 'emission', 'absorption', 'reflection' or a code");
    if (s.resolution[0] > 0x7FFFFFFFull || s.resolution[1] > 0x7FFFFFFFull ||
        s.resolution[0] * s.resolution[1] >= (1ull << 31))
      check(vr_render_slice(h, &s, nullptr, nullptr, nullptr));  // (refused before the handle, with its message)
    const mwSize H = (mwSize)s.resolution[0], W = (mwSize)s.resolution[1];
    mxArray *img = mxCreateNumericMatrix(H, W, mxSINGLE_CLASS, mxREAL);
    mxArray *aux = mxCreateNumericMatrix(H, W, mxSINGLE_CLASS, mxREAL);
    mxArray *lab = mxCreateNumericMatrix(H, W, mxSINGLE_CLASS, mxREAL);
    check(vr_render_slice(h, &s, static_cast<float *>(mxGetData(img)), static_cast<float *>(mxGetData(aux)),
                          static_cast<float *>(mxGetData(lab))));
    plhs[0] = img;
    if (nlhs > 1) plhs[1] = aux; else mxDestroyArray(aux);
    if (nlhs > 2) plhs[2] = lab; else mxDestroyArray(lab);
    return;
  }
  if (!strcmp(cmd, "volume_histogram")) {
    // volumeRender('volume_histogram', h, source, nbins, single([lo hi]), int32([first count]), use_clip)
    // -> [counts, summary] (vr_volume_histogram): source 'emission' | 'absorption' | 'reflection' (or its
    // code), count = 0: one row; counts uint64 [nbins rows] (counts(:, r) is row r), summary double
    // [rows 8] = total, below, above, nan, ninf, min, max, sum per row
    if (nlhs > 2) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 7) mexErrMsgTxt("insufficient parameter!");
    if (nrhs > 7) mexErrMsgTxt("volume_histogram: too many input arguments");
    vr_histogram q{};
    static const char *const sources[3] = {"emission", "absorption", "reflection"};
    q.source = -1;  // an unknown name or code stays invalid, which the library refuses
    if (mxGetClassID(prhs[2]) == mxCHAR_CLASS) {
      char buf[16];
      if (!mxGetString(prhs[2], buf, sizeof(buf)))
        for (int i = 0; i < 3; ++i)
          if (!strcmp(buf, sources[i])) q.source = i;
    } else {
      if (mxGetNumberOfElements(prhs[2]) != 1 || mxIsComplex(prhs[2]))
        mexErrMsgTxt("volume_histogram: source must be 'emission', 'absorption', 'reflection' or a code");
      const double v = mxGetScalar(prhs[2]);
      if (v >= 0.0 && v < 3.0 && v == (double)(int32_t)v) q.source = (int32_t)v;
    }
    if (mxGetNumberOfElements(prhs[3]) != 1 || mxIsComplex(prhs[3])) mexErrMsgTxt("volume_histogram: nbins must be a real scalar");
    const double nb = mxGetScalar(prhs[3]);
    q.nbins = (nb >= 1.0 && nb <= (double)VR_HIST_MAX_BINS && nb == (double)(int32_t)nb) ? (int32_t)nb : 0;  // (0: refused below)
    if (mxGetClassID(prhs[4]) != mxSINGLE_CLASS || mxIsComplex(prhs[4]) || mxGetNumberOfElements(prhs[4]) != 2)
      mexErrMsgTxt("volume_histogram: limits must be a single vector [lo hi]");
    memcpy(q.lim, mxGetData(prhs[4]), sizeof(q.lim));
    if (mxGetClassID(prhs[5]) != mxINT32_CLASS || mxGetNumberOfElements(prhs[5]) != 2)
      mexErrMsgTxt("volume_histogram: labels must be an int32 vector [first count]");
    const int32_t *lab = static_cast<const int32_t *>(mxGetData(prhs[5]));
    q.label_first = lab[0];
    q.label_count = lab[1];
    if (mxGetNumberOfElements(prhs[6]) != 1 || mxIsComplex(prhs[6])) mexErrMsgTxt("volume_histogram: use_clip must be a scalar");
    const double uc = mxGetScalar(prhs[6]);
    q.use_clip = uc == 0.0 ? 0 : (uc == 1.0 ? 1 : -1);
    const bool sized = q.nbins >= 1 && q.label_count >= 0 && q.label_count <= 256;  // (else refused, with its message)
    const mwSize rows = sized ? (mwSize)(q.label_count > 0 ? q.label_count + 1 : 1) : 1;
    const mwSize nbins = sized ? (mwSize)q.nbins : 1;
    mxArray *counts = mxCreateNumericMatrix(nbins, rows, mxUINT64_CLASS, mxREAL);
    std::vector<vr_hist_row> rr(rows);
    check(vr_volume_histogram(h, &q, static_cast<uint64_t *>(mxGetData(counts)), rr.data()));
    mxArray *summary = mxCreateNumericMatrix(rows, 8, mxDOUBLE_CLASS, mxREAL);
    double *s = static_cast<double *>(mxGetData(summary));
    for (mwSize r = 0; r < rows; ++r) {
      const double col[8] = {(double)rr[r].total, (double)rr[r].below, (double)rr[r].above, (double)rr[r].nan,
                             (double)rr[r].ninf,  (double)rr[r].min,   (double)rr[r].max,   rr[r].sum};
      for (int c = 0; c < 8; ++c) s[(size_t)c * rows + r] = col[c];
    }
    plhs[0] = counts;
    if (nlhs > 1) plhs[1] = summary; else mxDestroyArray(summary);
    return;
  }
  if (!strcmp(cmd, "render_isosurface")) {
    // volumeRender('render_isosurface', h, <render args>, level) -> [img, depth, normal]
    // (vr_render_isosurface): the first-hit surface emission == level lit by the lights, the depth of
    // the surface point [H W] and its unit normal [H W 3] (NaN where there is no surface)
    if (nlhs > 3) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 12) mexErrMsgTxt("insufficient parameter!");
    const mxClassID lc = mxGetClassID(prhs[11]);
    const bool numeric = lc == mxDOUBLE_CLASS || lc == mxSINGLE_CLASS || lc == mxINT8_CLASS || lc == mxUINT8_CLASS ||
                         lc == mxINT16_CLASS || lc == mxUINT16_CLASS || lc == mxINT32_CLASS || lc == mxUINT32_CLASS ||
                         lc == mxINT64_CLASS || lc == mxUINT64_CLASS;
    if (!numeric || mxIsComplex(prhs[11]) || mxGetNumberOfElements(prhs[11]) != 1)
      mexErrMsgTxt("render_isosurface: level must be a real scalar");
    const float level = (float)mxGetScalar(prhs[11]);
    vr_render_args a;
    std::vector<vr_light> lights;
    vr_volume illum{};
    unpack_render(prhs + 2, a, lights, illum);
    mxArray *img = new_image(a, 1), *normal = new_image(a, 1);
    mxArray *depth = mxCreateNumericMatrix((mwSize)a.resolution[0], (mwSize)a.resolution[1], mxSINGLE_CLASS, mxREAL);
    check(vr_render_isosurface(h, &a, level, static_cast<float *>(mxGetData(img)),
                               static_cast<float *>(mxGetData(depth)), static_cast<float *>(mxGetData(normal))));
    plhs[0] = img;
    if (nlhs > 1) plhs[1] = depth; else mxDestroyArray(depth);
    if (nlhs > 2) plhs[2] = normal; else mxDestroyArray(normal);
    return;
  }
  if (!strcmp(cmd, "render_transfer")) {
    // volumeRender('render_transfer', h, <render args>, colormap [N 3], clim [lo hi], alphamap [M 1] | false,
    // alim [lo hi], 'value' | 'depth') -> [img, alpha] (vr_render_transfer): 'render' with the sample's
    // colour read from the colormap and, with an alphamap, its absorption from that table; alpha [H W]
    // is the accumulated opacity
    if (nlhs > 2) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 16) mexErrMsgTxt("insufficient parameter!");
    if (nrhs > 16) mexErrMsgTxt("render_transfer: too many input arguments");
    const mxArray *cm = prhs[11], *am = prhs[13];
    if (mxGetClassID(cm) != mxSINGLE_CLASS || mxIsComplex(cm) || mxGetNumberOfDimensions(cm) != 2 || mxGetN(cm) != 3)
      mexErrMsgTxt("render_transfer: colormap must be a single N x 3 matrix");
    vr_transfer tf{};
    tf.colormap = static_cast<const float *>(mxGetData(cm));
    tf.n_color = (int32_t)mxGetM(cm);
    if (mxGetClassID(prhs[12]) != mxSINGLE_CLASS) mexErrMsgTxt("render_transfer: clim must be single [lo hi]");
    memcpy(tf.clim, data_of<float>(prhs[12], 2, "render_transfer: clim must be single [lo hi]"), sizeof(tf.clim));
    if (!mxIsClass(am, "logical")) {  // the logical false: the opacity of 'render'
      if (mxGetClassID(am) != mxSINGLE_CLASS || mxIsComplex(am) || mxGetNumberOfDimensions(am) != 2 ||
          (mxGetM(am) != 1 && mxGetN(am) != 1))
        mexErrMsgTxt("render_transfer: alphamap must be a single vector or false");
      tf.alphamap = static_cast<const float *>(mxGetData(am));
      tf.n_alpha = (int32_t)mxGetNumberOfElements(am);
      if (mxGetClassID(prhs[14]) != mxSINGLE_CLASS) mexErrMsgTxt("render_transfer: alim must be single [lo hi]");
      memcpy(tf.alim, data_of<float>(prhs[14], 2, "render_transfer: alim must be single [lo hi]"), sizeof(tf.alim));
    }
    char coord[16];
    if (mxGetString(prhs[15], coord, sizeof(coord))) mexErrMsgTxt("render_transfer: coord must be 'value' or 'depth'");
    if (!strcmp(coord, "depth")) tf.coord = VR_TF_DEPTH;
    else if (!strcmp(coord, "value")) tf.coord = VR_TF_VALUE;
    else mexErrMsgTxt("render_transfer: coord must be 'value' or 'depth'");
    vr_render_args a;
    std::vector<vr_light> lights;
    vr_volume illum{};
    unpack_render(prhs + 2, a, lights, illum);
    mxArray *img = new_image(a, 1);
    mxArray *alpha = mxCreateNumericMatrix((mwSize)a.resolution[0], (mwSize)a.resolution[1], mxSINGLE_CLASS, mxREAL);
    check(vr_render_transfer(h, &a, &tf, static_cast<float *>(mxGetData(img)), static_cast<float *>(mxGetData(alpha))));
    plhs[0] = img;
    if (nlhs > 1) plhs[1] = alpha; else mxDestroyArray(alpha);
    return;
  }
  if (!strcmp(cmd, "set_clip")) {
    // volumeRender('set_clip', h, planes) (vr_set_clip): planes single 4 x n, columns [n0; n1; n2; offset]
    // keeping n . q + offset >= 0 of the normalized volume coordinate q (dimension order of Data);
    // [] or false clears the set.  The planes stay with the handle until the next 'set_clip'.
    if (nlhs > 0) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 3) mexErrMsgTxt("insufficient parameter!");
    if (nrhs > 3) mexErrMsgTxt("set_clip: too many input arguments");
    const mxArray *pl = prhs[2];
    if (mxIsClass(pl, "logical")) {
      if (mxGetNumberOfElements(pl) != 1 || mxGetScalar(pl) != 0.0)
        mexErrMsgTxt("set_clip: planes must be a single 4 x n matrix, [] or false");
      check(vr_set_clip(h, nullptr, 0));
      return;
    }
    if (mxGetNumberOfElements(pl) == 0) {
      check(vr_set_clip(h, nullptr, 0));
      return;
    }
    if (mxGetClassID(pl) != mxSINGLE_CLASS || mxIsComplex(pl) || mxGetNumberOfDimensions(pl) != 2 || mxGetM(pl) != 4)
      mexErrMsgTxt("set_clip: planes must be a single 4 x n matrix, [] or false");
    const mwSize n = mxGetN(pl);
    if (n > 0x7fffffff) mexErrMsgTxt("set_clip: too many planes");
    // a 4 x n single matrix is n vr_clip_plane records in memory (column-major)
    static_assert(sizeof(vr_clip_plane) == 4 * sizeof(float), "vr_clip_plane is four floats");
    check(vr_set_clip(h, static_cast<const vr_clip_plane *>(mxGetData(pl)), (int32_t)n));
    return;
  }
  if (!strcmp(cmd, "sync_labels")) {
    // volumeRender('sync_labels', h, labels) (vr_sync_labels): labels a uint8 array of the size of the
    // emission volume's Data (one label per voxel), or a RawVolume of uint8 (its TimeLastUpdate spares a
    // repeated upload); [] or false drops them.  The labels stay with the handle until the next 'sync_labels'.
    if (nlhs > 0) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 3) mexErrMsgTxt("insufficient parameter!");
    if (nrhs > 3) mexErrMsgTxt("sync_labels: too many input arguments");
    const mxArray *lb = prhs[2];
    if (mxIsClass(lb, "logical")) {
      if (mxGetNumberOfElements(lb) != 1 || mxGetScalar(lb) != 0.0)
        mexErrMsgTxt("sync_labels: labels must be a uint8 array, a RawVolume of uint8, [] or false");
      check(vr_sync_labels(h, nullptr));
      return;
    }
    if (mxGetPropertyShared(lb, 0, "TimeLastUpdate")) {  // a Volume object: the library checks its element type
      const vr_volume v = make_volume(lb);
      check(vr_sync_labels(h, &v));
      return;
    }
    if (mxGetNumberOfElements(lb) == 0) {
      check(vr_sync_labels(h, nullptr));
      return;
    }
    if (mxGetClassID(lb) != mxUINT8_CLASS || mxIsComplex(lb) || mxGetNumberOfDimensions(lb) > 3)
      mexErrMsgTxt("sync_labels: labels must be a uint8 array, a RawVolume of uint8, [] or false");
    vr_volume v{};
    v.dtype = VR_U8;
    v.data = static_cast<const float *>(mxGetData(lb));
    const mwSize nd = mxGetNumberOfDimensions(lb);
    const mwSize *d = mxGetDimensions(lb);
    v.dims[0] = d[0];
    v.dims[1] = nd > 1 ? d[1] : 1;
    v.dims[2] = nd > 2 ? d[2] : 1;
    v.last_update = 0;  // a bare array has no Volume identity: uploaded by every call
    v.location = VR_HOST;
    check(vr_sync_labels(h, &v));
    return;
  }
  if (!strcmp(cmd, "set_label_gains")) {
    // volumeRender('set_label_gains', h, gains) (vr_set_label_gains): gains a single vector of at most 256
    // entries, gains(l + 1) the factor of the voxels labelled l; [] or false clears the table.  The
    // emission volume on the device follows at once; the gains stay with the handle.
    if (nlhs > 0) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 3) mexErrMsgTxt("insufficient parameter!");
    if (nrhs > 3) mexErrMsgTxt("set_label_gains: too many input arguments");
    const mxArray *g = prhs[2];
    if (mxIsClass(g, "logical")) {
      if (mxGetNumberOfElements(g) != 1 || mxGetScalar(g) != 0.0)
        mexErrMsgTxt("set_label_gains: gains must be a single vector of at most 256 entries, [] or false");
      check(vr_set_label_gains(h, nullptr, 0));
      return;
    }
    if (mxGetNumberOfElements(g) == 0) {
      check(vr_set_label_gains(h, nullptr, 0));
      return;
    }
    if (mxGetClassID(g) != mxSINGLE_CLASS || mxIsComplex(g) || mxGetNumberOfDimensions(g) != 2 ||
        (mxGetM(g) != 1 && mxGetN(g) != 1) || mxGetNumberOfElements(g) > 256)
      mexErrMsgTxt("set_label_gains: gains must be a single vector of at most 256 entries, [] or false");
    check(vr_set_label_gains(h, static_cast<const float *>(mxGetData(g)), (int32_t)mxGetNumberOfElements(g)));
    return;
  }
  if (!strcmp(cmd, "set_smoothing")) {
    // volumeRender('set_smoothing', h, sigma) (vr_set_smoothing): sigma in voxels, a single or double scalar
    // (all three dimensions of Data) or 3-vector; [] or false clears.  The emission volume on the device
    // follows at once; the sigma stays with the handle.
    if (nlhs > 0) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 3) mexErrMsgTxt("insufficient parameter!");
    if (nrhs > 3) mexErrMsgTxt("set_smoothing: too many input arguments");
    const mxArray *g = prhs[2];
    const char *bad = "set_smoothing: sigma must be a single or double scalar or 3-vector, [] or false";
    if (mxIsClass(g, "logical")) {
      if (mxGetNumberOfElements(g) != 1 || mxGetScalar(g) != 0.0) mexErrMsgTxt(bad);
      check(vr_set_smoothing(h, nullptr));
      return;
    }
    const size_t n = mxGetNumberOfElements(g);
    const bool f32 = mxGetClassID(g) == mxSINGLE_CLASS;
    if ((!f32 && mxGetClassID(g) != mxDOUBLE_CLASS) || mxIsComplex(g) || mxGetNumberOfDimensions(g) != 2)
      mexErrMsgTxt(bad);  // (an empty char or cell array is no sigma either)
    if (n == 0) {
      check(vr_set_smoothing(h, nullptr));
      return;
    }
    if ((mxGetM(g) != 1 && mxGetN(g) != 1) || (n != 1 && n != 3)) mexErrMsgTxt(bad);
    float sigma[3];
    for (size_t j = 0; j < 3; ++j) {
      const size_t k = n == 1 ? 0 : j;
      sigma[j] = f32 ? static_cast<const float *>(mxGetData(g))[k] : (float)static_cast<const double *>(mxGetData(g))[k];
    }
    check(vr_set_smoothing(h, sigma));
    return;
  }
  if (!strcmp(cmd, "set_deconvolution")) {
    // volumeRender('set_deconvolution', h, sigma, iterations[, floor]) (vr_set_deconvolution): the Gaussian
    // PSF's sigma in voxels, a single or double scalar (all three dimensions of Data) or 3-vector; iterations
    // an integer-valued real scalar in 0..64; floor a single or double scalar (default 1e-6 single).  [] or
    // false as sigma, or iterations = 0, clears.  The emission volume on the device follows at once; the
    // setting stays with the handle.
    if (nlhs > 0) mexErrMsgTxt("Too many output arguments.");
    if (nrhs < 3) mexErrMsgTxt("insufficient parameter!");
    if (nrhs > 5) mexErrMsgTxt("set_deconvolution: too many input arguments");
    const mxArray *g = prhs[2];
    const char *bad = "set_deconvolution: sigma must be a single or double scalar or 3-vector, [] or false";
    const float default_floor = 1e-6f;
    float flr = default_floor;
    if (nrhs > 4) {
      const mxArray *f = prhs[4];
      const bool f32 = mxGetClassID(f) == mxSINGLE_CLASS;
      if ((!f32 && mxGetClassID(f) != mxDOUBLE_CLASS) || mxIsComplex(f) || mxGetNumberOfElements(f) != 1)
        mexErrMsgTxt("set_deconvolution: floor must be a real scalar greater than 0");
      flr = f32 ? *static_cast<const float *>(mxGetData(f)) : (float)*static_cast<const double *>(mxGetData(f));
    }
    int32_t iterations = 0;
    if (nrhs > 3) {
      const mxArray *it = prhs[3];
      const char *badn = "set_deconvolution: iterations must be an integer scalar in 0..64";
      const mxClassID cls = mxGetClassID(it);  // any real numeric class
      if (cls < mxDOUBLE_CLASS || cls > mxUINT64_CLASS || mxIsComplex(it) || mxGetNumberOfElements(it) != 1)
        mexErrMsgTxt(badn);
      const double v = mxGetScalar(it);
      if (!(v >= 0.0 && v <= (double)VR_DECONV_MAX_ITERATIONS) || v != (double)(int32_t)v) mexErrMsgTxt(badn);
      iterations = (int32_t)v;
    }
    if (mxIsClass(g, "logical")) {
      if (mxGetNumberOfElements(g) != 1 || mxGetScalar(g) != 0.0) mexErrMsgTxt(bad);
      check(vr_set_deconvolution(h, nullptr, 0, flr));
      return;
    }
    const size_t n = mxGetNumberOfElements(g);
    const bool f32 = mxGetClassID(g) == mxSINGLE_CLASS;
    if ((!f32 && mxGetClassID(g) != mxDOUBLE_CLASS) || mxIsComplex(g) || mxGetNumberOfDimensions(g) != 2)
      mexErrMsgTxt(bad);
    if (n == 0) {
      check(vr_set_deconvolution(h, nullptr, 0, flr));
      return;
    }
    if ((mxGetM(g) != 1 && mxGetN(g) != 1) || (n != 1 && n != 3)) mexErrMsgTxt(bad);
    if (nrhs < 4) mexErrMsgTxt("set_deconvolution: iterations is missing");
    float sigma[3];
    for (size_t j = 0; j < 3; ++j) {
      const size_t k = n == 1 ? 0 : j;
      sigma[j] = f32 ? static_cast<const float *>(mxGetData(g))[k] : (float)static_cast<const double *>(mxGetData(g))[k];
    }
    check(vr_set_deconvolution(h, sigma, iterations, flr));
    return;
  }
  mexErrMsgTxt(("Unknown command: " + std::string(cmd)).c_str());
}
