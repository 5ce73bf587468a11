"""The three MEX entry points of the reference, re-exposed over libvrhip's C-ABI.

``volumeRender(cmd, ...)`` keeps the command protocol and the argument marshalling of
/root/reference/src/C/mex/render.cpp:50-278 (positional MATLAB arguments, same order, same
permutations -- done inside libvrhip exactly where the reference does them), ``HenyeyGreenstein``
mirrors /root/reference/src/C/mex/HenyeyGreenstein.cc:29-96 and ``timestamp`` mirrors
/root/reference/src/C/mex/timestamp.cpp:17-33.  MATLAB values map to Python as:
logical ``false`` -> ``False``; ``single``/``uint64`` arrays -> numpy arrays (column-major);
``Volume``/``LightSource`` objects -> the classes of this package.
"""
from __future__ import annotations

import ctypes
import warnings

import numpy as np

from . import _lib
from ._lib import VrLight, VrRenderArgs, VrVolume, check, lib

_clock = None


def set_clock(fn) -> None:
    """Replace the millisecond clock behind ``timestamp`` (tests use a deterministic counter;
    the reference's change tracking misses updates made within the same millisecond,
    SURVEY.md A.9).  ``None`` restores the real clock."""
    global _clock
    _clock = fn


def timestamp() -> np.uint64:
    """ms since the epoch, low 32 bits (timestamp.cpp stores it through an int*)."""
    if _clock is not None:
        return np.uint64(_clock())
    return np.uint64(lib().vr_timestamp())


def HenyeyGreenstein(n, g=0.8) -> np.ndarray:
    """N x N x N single LUT of the Henyey-Greenstein phase function (HenyeyGreenstein.cc)."""
    n = int(n)
    out = np.empty((n, n, n), dtype=np.float32, order="F")
    check(lib().vr_henyey_greenstein(ctypes.c_uint32(n), ctypes.c_float(g), out.ctypes.data_as(ctypes.c_void_p)))
    return out


def _is_false(x) -> bool:
    return isinstance(x, (bool, np.bool_)) and not bool(x)


def _matlab_dims(a: np.ndarray):
    """mxGetDimensions as the mex reads them: (d0, d1, d2) with d2 = 1 for 2-D data."""
    if a.ndim == 0:
        return (1, 1, 1)
    if a.ndim == 1:
        return (a.shape[0], 1, 1)
    if a.ndim == 2:
        return (a.shape[0], a.shape[1], 1)
    if a.ndim == 3:
        return tuple(a.shape)
    raise ValueError("volumes must have at most 3 dimensions")


# numpy element types a volume may have -> vr_dtype (include/vrhip.h): converted exactly to fp32 on
# the device during the upload
_NP_DTYPES = {np.dtype(np.float32): _lib.VR_F32, np.dtype(np.uint8): _lib.VR_U8, np.dtype(np.uint16): _lib.VR_U16,
              np.dtype(np.int16): _lib.VR_I16, np.dtype(np.float16): _lib.VR_F16}


def dtype_code(np_dtype, unorm: bool = False) -> int:
    """The vr_dtype code of a numpy element type (| VR_DTYPE_UNORM if `unorm`: uint8 / uint16 only,
    value = single(x) / single(255 resp. 65535)); TypeError for a type volumes cannot have."""
    code = _NP_DTYPES.get(np.dtype(np_dtype))
    if code is None:
        raise TypeError(f"volume data must be float32, uint8, uint16, int16 or float16, not {np.dtype(np_dtype)}")
    return code | (_lib.VR_DTYPE_UNORM if unorm else 0)


def dtype_size(code: int) -> int:
    """vr_dtype_size: element size in bytes of a dtype code, 0 if the code is invalid."""
    return int(lib().vr_dtype_size(int(code)))


def convert_host(src: np.ndarray, unorm: bool = False, code=None) -> np.ndarray:
    """vr_convert_host: the upload's element -> fp32 conversion on the CPU (same shape and order)."""
    src = np.asarray(src)
    code = dtype_code(src.dtype, unorm) if code is None else int(code)
    flat = np.ascontiguousarray(src.reshape(-1, order="F"))
    out = np.empty(flat.size, np.float32)
    check(lib().vr_convert_host(flat.ctypes.data_as(ctypes.c_void_p), code, flat.size,
                                out.ctypes.data_as(ctypes.c_void_p)))
    return out.reshape(src.shape, order="F")


class DeviceVolume:
    """A Volume whose Data already lives in HBM (e.g. a torch tensor on cuda): MATLAB-shaped dims
    (d0, d1, d2), column-major at device address `ptr`, elements of `dtype` (a vr_dtype code; fp32
    by default).  Synced device-to-device."""

    def __init__(self, ptr: int, dims, last_update=None, owner=None, dtype=_lib.VR_F32):
        self.ptr = int(ptr)
        self.dtype = int(dtype)
        d = tuple(int(x) for x in dims) + (1,) * (3 - len(dims))
        self.dims = d[:3]
        self.TimeLastUpdate = timestamp() if last_update is None else np.uint64(last_update)
        self.owner = owner  # keeps the backing allocation alive

    @classmethod
    def from_tensor(cls, t, dims=None, last_update=None, unorm=False):
        """`t` is a contiguous cuda tensor holding the column-major data: float32, or uint8, int16,
        float16 (and uint16 where the installed torch has it), widened to fp32 by the upload.
        `unorm` (uint8 / uint16 only): voxel = single(x) / single(255 resp. 65535)."""
        import torch
        codes = {torch.float32: _lib.VR_F32, torch.uint8: _lib.VR_U8, torch.int16: _lib.VR_I16,
                 torch.float16: _lib.VR_F16}
        if hasattr(torch, "uint16"):
            codes[torch.uint16] = _lib.VR_U16
        if t.dtype not in codes or not t.is_cuda or not t.is_contiguous():
            raise TypeError("DeviceVolume needs a contiguous float32, uint8, uint16, int16 or float16 cuda tensor")
        code = codes[t.dtype]
        if unorm:
            if code not in (_lib.VR_U8, _lib.VR_U16):
                raise TypeError("unorm is for uint8 / uint16 tensors only")
            code |= _lib.VR_DTYPE_UNORM
        dims = dims if dims is not None else tuple(reversed(t.shape))  # C-order (z,y,x) tensor -> (x,y,z)
        return cls(t.data_ptr(), dims, last_update, owner=t, dtype=code)

    def min(self):
        return 0.0


def _vr_volume(vol) -> VrVolume:
    """mxMake_volume (volumeRender.cpp:307-342): zero-copy view of Data + TimeLastUpdate."""
    v = VrVolume()
    if isinstance(vol, DeviceVolume):
        v.data = vol.ptr
        for i in range(3):
            v.dims[i] = vol.dims[i]
        v.last_update = int(vol.TimeLastUpdate)
        v.location = _lib.VR_DEVICE
        v.dtype = vol.dtype
        return v
    data = vol.Data
    raw = getattr(vol, "RawData", None)  # a RawVolume: its native-typed array instead of Data
    unorm = False
    if raw is not None and getattr(raw, "size", 0):
        data = raw
        unorm = bool(getattr(vol, "Unorm", False))
    if not (isinstance(data, np.ndarray) and data.dtype in _NP_DTYPES and
            (data.flags.f_contiguous or data.ndim <= 1)):
        raise TypeError("Volume.Data must be a column-major single (or uint8, uint16, int16, float16) array")
    if unorm and data.dtype not in (np.uint8, np.uint16):
        raise TypeError("Unorm is for uint8 / uint16 data only")
    v.dtype = dtype_code(data.dtype, unorm)
    v.data = data.ctypes.data if data.size else None
    d = _matlab_dims(data)
    for i in range(3):
        v.dims[i] = d[i]
    v.last_update = int(vol.TimeLastUpdate)
    v.location = _lib.VR_HOST
    return v


def _handle(h) -> ctypes.c_void_p:
    a = np.asarray(h)
    if a.size != 1 or a.dtype != np.uint64:
        raise _lib.VrError(_lib.VR_OK + 1, "Input must be a real uint64 scalar.")
    return ctypes.c_void_p(int(a.reshape(-1)[0]))


def _f32(x, n: int, name: str) -> np.ndarray:
    a = np.asarray(x, dtype=np.float32).reshape(-1, order="F")
    if a.size < n:
        raise ValueError(f"{name}: expected {n} values")
    return a


def render_args(lights_arg, illum_arg, factors, element_size_um, resolution, rotation_flipped, props,
                opacity_threshold, color):
    """Marshal the positional 'render' arguments (prhs[2..10], render.cpp:142-240) into the
    C-ABI struct.  Returns (VrRenderArgs, keep-alive list)."""
    ra = VrRenderArgs()
    keep = []
    if not (_is_false(lights_arg) or _is_false(illum_arg)):
        lights = list(lights_arg) if isinstance(lights_arg, (list, tuple, np.ndarray)) else [lights_arg]
        arr = (VrLight * max(len(lights), 1))()
        for i, ls in enumerate(lights):
            pos = _f32(ls.Position, 3, "Position")
            col = _f32(ls.Color, 3, "Color")
            for k in range(3):
                arr[i].position[k] = pos[k]
                arr[i].color[k] = col[k]
        illum = _vr_volume(illum_arg)
        keep += [arr, illum, getattr(illum_arg, "Data", None), getattr(illum_arg, "RawData", None)]
        ra.lights = ctypes.cast(arr, ctypes.POINTER(VrLight))
        ra.num_lights = len(lights)
        ra.illumination = ctypes.pointer(illum)
    else:
        ra.num_lights = -1
        ra.illumination = None
    fac = _f32(factors, 3, "factors")
    es = _f32(element_size_um, 3, "ElementSizeUm")
    res = np.asarray(resolution).reshape(-1)
    rot = _f32(rotation_flipped, 9, "RotationMatrix")
    pr = _f32(props, 3, "props")
    thr = np.float32(np.asarray(opacity_threshold).reshape(-1)[0])
    col = _f32(color, 3, "Color")
    for k in range(3):
        ra.factors[k] = fac[k]
        ra.element_size_um[k] = es[k]
        ra.props[k] = pr[k]
        ra.color[k] = col[k]
    for k in range(9):
        ra.rotation_flipped[k] = rot[k]
    ra.resolution[0] = int(res[0])
    ra.resolution[1] = int(res[1])
    ra.opacity_threshold = thr
    return ra, keep


def partition(block_cols: int, part: int, num_parts: int) -> _lib.VrPartition:
    p = _lib.VrPartition()
    p.block_cols, p.part, p.num_parts = int(block_cols), int(part), int(num_parts)
    return p


def partition_columns(width: int, part) -> int:
    return int(lib().vr_partition_columns(int(width), ctypes.byref(part) if part is not None else None))


SLAB_PLANES = 10  # include/vrhip.h VR_SLAB_PLANES


def slab(depth: int, z_first: int, z0: float, z1: float, direction: int) -> _lib.VrSlab:
    """vr_slab: the synced emission volume holds planes [z_first, ...) of a volume of depth
    `depth`; the render owns the samples with z0 <= p.z * depth < z1; direction +1 / -1, or 0
    (both: the top slab's ascending launch, where the descending rays start)."""
    s = _lib.VrSlab()
    s.depth, s.z_first, s.z0, s.z1, s.direction = int(depth), int(z_first), float(z0), float(z1), int(direction)
    return s


def slab_planes(dims, element_size_um, z0: float, z1: float):
    """(first, count): the planes a slab owning [z0, z1) of a (d0, d1, D) volume must hold."""
    d = (ctypes.c_uint64 * 3)(*[int(x) for x in dims])
    es = (ctypes.c_float * 3)(*[float(x) for x in element_size_um])
    first, count = ctypes.c_uint64(0), ctypes.c_uint64(0)
    check(lib().vr_slab_planes(d, es, float(z0), float(z1), ctypes.byref(first), ctypes.byref(count)))
    return int(first.value), int(count.value)


def render_slab(handle, ra: VrRenderArgs, sl, d_state_in: int, d_state_out: int, stream: int = 0,
                part=None) -> None:
    """vr_render_slab: march this slab's samples of every ray (of the part's columns, if a
    partition is given); state = SLAB_PLANES planes of cols*H floats (colour, alpha, goes-on,
    and the resume point t, x, y, z, sample index of a ray that goes on)."""
    check(lib().vr_render_slab(_handle(handle), ctypes.byref(ra), ctypes.byref(sl),
                               ctypes.byref(part) if part is not None else None,
                               ctypes.c_void_p(int(d_state_in)) if d_state_in else None,
                               ctypes.c_void_p(int(d_state_out)), ctypes.c_void_p(int(stream))))


def depth_lanes(part_cols: int, height: int, texels_per_pixel=None) -> int:
    """Depth lanes the march uses for a launch of this shape on the current device (vr_depth_lanes;
    with texels_per_pixel, vr_depth_lanes_tau: the choice a render at that sampling density makes)."""
    if texels_per_pixel is None:
        return int(lib().vr_depth_lanes(int(part_cols), int(height)))
    return int(lib().vr_depth_lanes_tau(int(part_cols), int(height), float(texels_per_pixel)))


def render_device(handle, ra: VrRenderArgs, d_out: int, part=None, d_steps: int = 0, stream: int = 0) -> None:
    """'render' into device memory (vr_render_device): asynchronous on `stream`."""
    check(lib().vr_render_device(_handle(handle), ctypes.byref(ra), ctypes.byref(part) if part is not None else None,
                                 ctypes.c_void_p(int(d_out)), ctypes.c_void_p(int(d_steps)) if d_steps else None,
                                 ctypes.c_void_p(int(stream)) if stream else None))


def render_stereo_device(handle, ra: VrRenderArgs, base: float, d_left: int, d_right: int, d_steps: int = 0,
                         stream: int = 0) -> None:
    """Both eyes of a stereo pair into device memory in one launch (vr_render_stereo_device): the
    left eye (camera offset -base) to d_left, the right (+base) to d_right; ra.props[0] is ignored."""
    check(lib().vr_render_stereo_device(_handle(handle), ctypes.byref(ra), ctypes.c_float(base),
                                        ctypes.c_void_p(int(d_left)), ctypes.c_void_p(int(d_right)),
                                        ctypes.c_void_p(int(d_steps)) if d_steps else None,
                                        ctypes.c_void_p(int(stream)) if stream else None))


PROJECTION_MODES = {"mip": _lib.VR_PROJ_MIP, "sum": _lib.VR_PROJ_SUM}


def projection_mode(mode) -> int:
    """The vr_projection code of 'mip' / 'sum' (or of a code itself)."""
    if isinstance(mode, str):
        if mode.lower() not in PROJECTION_MODES:
            raise _lib.VrError(1, "unknown projection mode")
        return PROJECTION_MODES[mode.lower()]
    return int(mode)


def render_projection_device(handle, ra: VrRenderArgs, mode, d_out: int, d_aux: int = 0, part=None, d_steps: int = 0,
                             stream: int = 0) -> None:
    """A projection into device memory (vr_render_projection_device), asynchronous on `stream`:
    mode 'mip' (aux: the depth t of the first maximum) or 'sum' (aux: the ray's sample count);
    d_aux = 0: no aux plane; d_steps: two counters, samples visited and samples fetched."""
    check(lib().vr_render_projection_device(_handle(handle), ctypes.byref(ra), projection_mode(mode),
                                            ctypes.byref(part) if part is not None else None,
                                            ctypes.c_void_p(int(d_out)) if d_out else None,
                                            ctypes.c_void_p(int(d_aux)) if d_aux else None,
                                            ctypes.c_void_p(int(d_steps)) if d_steps else None,
                                            ctypes.c_void_p(int(stream)) if stream else None))


def isosurface_level(level) -> float:
    """The level of an isosurface render: a real scalar."""
    v = np.asarray(level)
    if v.size != 1 or v.dtype.kind not in "fiu":
        raise _lib.VrError(1, "render_isosurface: level must be a real scalar")
    return float(v.reshape(-1)[0])


def render_isosurface_device(handle, ra: VrRenderArgs, level, d_out: int, d_depth: int = 0, d_normal: int = 0,
                             part=None, d_steps: int = 0, stream: int = 0) -> None:
    """The first-hit isosurface emission == level into device memory (vr_render_isosurface_device),
    asynchronous on `stream`: the lit image, the depth plane t* (d_depth = 0: none) and the three
    normal planes (d_normal = 0: none); d_steps: three counters, search samples visited, search
    samples fetched, surface pixels."""
    lv = ctypes.c_float(isosurface_level(level))
    check(lib().vr_render_isosurface_device(_handle(handle), ctypes.byref(ra), lv,
                                            ctypes.byref(part) if part is not None else None,
                                            ctypes.c_void_p(int(d_out)) if d_out else None,
                                            ctypes.c_void_p(int(d_depth)) if d_depth else None,
                                            ctypes.c_void_p(int(d_normal)) if d_normal else None,
                                            ctypes.c_void_p(int(d_steps)) if d_steps else None,
                                            ctypes.c_void_p(int(stream)) if stream else None))


TRANSFER_COORDS = {"value": _lib.VR_TF_VALUE, "depth": _lib.VR_TF_DEPTH}


def transfer(colormap, clim=(0, 1), alphamap=None, alim=(0, 1), coord="value"):
    """The vr_transfer of a transfer-function render: colormap [N, 3] single (rows R G B, column-major
    as MATLAB stores it), clim = [lo hi], alphamap [M] single or None / False (the opacity of
    'render'), alim = [lo hi], coord 'value' | 'depth' (or a vr_transfer_coord code).  Returns
    (VrTransfer, keep-alive list)."""
    cm = np.asarray(colormap)
    if cm.dtype != np.float32 or cm.ndim != 2 or cm.shape[1] != 3:
        raise _lib.VrError(1, "render_transfer: colormap must be a single N x 3 matrix")
    cm = np.asfortranarray(cm)
    tf = _lib.VrTransfer()
    tf.colormap = cm.ctypes.data
    tf.n_color = cm.shape[0]
    lim = _f32(clim, 2, "clim")
    tf.clim[0], tf.clim[1] = lim[0], lim[1]
    am = None
    if alphamap is not None and not _is_false(alphamap):
        am = np.asarray(alphamap)
        if am.dtype != np.float32 or am.size != max(am.shape, default=0):
            raise _lib.VrError(1, "render_transfer: alphamap must be a single vector or false")
        am = np.ascontiguousarray(am.reshape(-1))
        tf.alphamap = am.ctypes.data
        tf.n_alpha = am.size
        lim = _f32(alim, 2, "alim")
        tf.alim[0], tf.alim[1] = lim[0], lim[1]
    if isinstance(coord, str):
        if coord.lower() not in TRANSFER_COORDS:
            raise _lib.VrError(1, "unknown colormap coordinate")
        tf.coord = TRANSFER_COORDS[coord.lower()]
    else:
        tf.coord = int(coord)
    return tf, [cm, am]


def render_transfer_device(handle, ra: VrRenderArgs, tf, d_out: int, d_alpha: int = 0, part=None, d_steps: int = 0,
                           stream: int = 0) -> None:
    """A transfer-function render into device memory (vr_render_transfer_device), asynchronous on
    `stream`: tf from transfer(); d_alpha = 0: no alpha plane; d_steps: two counters, samples visited
    and samples fetched."""
    check(lib().vr_render_transfer_device(_handle(handle), ctypes.byref(ra), ctypes.byref(tf),
                                          ctypes.byref(part) if part is not None else None,
                                          ctypes.c_void_p(int(d_out)) if d_out else None,
                                          ctypes.c_void_p(int(d_alpha)) if d_alpha else None,
                                          ctypes.c_void_p(int(d_steps)) if d_steps else None,
                                          ctypes.c_void_p(int(stream)) if stream else None))


def transfer_lookup_host(table, lim, c) -> np.ndarray:
    """vr_transfer_lookup_host: the kernel's table lookup on the CPU.  table [n] or [n, ncomp] single,
    lim = [lo hi], c the coordinates; returns [ncomp, len(c)] (or [len(c)] for a vector table)."""
    t = np.asarray(table, dtype=np.float32)
    vec = t.ndim == 1
    t = np.asfortranarray(t.reshape(t.shape[0], -1))
    cc = np.ascontiguousarray(np.asarray(c, dtype=np.float32).reshape(-1))
    out = np.empty((t.shape[1], cc.size), np.float32)
    l2 = (ctypes.c_float * 2)(*[float(x) for x in _f32(lim, 2, "lim")])
    check(lib().vr_transfer_lookup_host(t.ctypes.data, t.shape[0], t.shape[1], l2, cc.ctypes.data, cc.size,
                                        out.ctypes.data))
    return out[0] if vec else out


def clip_planes(planes):
    """The vr_clip_plane array of a plane set: `planes` n x 4, rows [n0 n1 n2 offset] keeping
    n . q + offset >= 0 of the normalized volume coordinate q in the dimension order of Data (None,
    False or an empty array: no planes).  Returns (array or None, n); the library checks the values."""
    if planes is None or _is_false(planes):
        return None, 0
    a = np.asarray(planes, dtype=np.float32)
    if a.size == 0:
        return None, 0
    if a.ndim == 1 and a.size == 4:
        a = a.reshape(1, 4)
    if a.ndim != 2 or a.shape[1] != 4:
        raise _lib.VrError(1, "clip planes must be an n x 4 matrix with rows [n0 n1 n2 offset]")
    arr = (_lib.VrClipPlane * a.shape[0])()
    for i in range(a.shape[0]):
        for k in range(3):
            arr[i].normal[k] = a[i, k]
        arr[i].offset = a[i, 3]
    return arr, int(a.shape[0])


def set_clip(handle, planes) -> None:
    """vr_set_clip: replace the handle's clip planes (clip_planes(); None / False / [] clears them)."""
    arr, n = clip_planes(planes)
    check(lib().vr_set_clip(_handle(handle), arr, n))


def get_clip(handle) -> np.ndarray:
    """vr_get_clip: the handle's clip planes as set, n x 4 single (0 x 4: none)."""
    arr = (_lib.VrClipPlane * _lib.VR_CLIP_MAX)()
    n = ctypes.c_int32(0)
    check(lib().vr_get_clip(_handle(handle), arr, ctypes.byref(n)))
    return np.array([[arr[i].normal[0], arr[i].normal[1], arr[i].normal[2], arr[i].offset] for i in range(n.value)],
                    np.float32).reshape(n.value, 4)


def clip_convert_host(planes, bmin, bscale) -> np.ndarray:
    """vr_clip_convert_host: the per-launch conversion of a plane set for the box (bmin, bscale), rows
    [N0 N1 N2 D] keeping N . p + D >= 0 of the world position p."""
    arr, n = clip_planes(planes)
    out = np.zeros((n, 4), np.float32)
    b0 = (ctypes.c_float * 3)(*[float(x) for x in _f32(bmin, 3, "bmin")])
    b1 = (ctypes.c_float * 3)(*[float(x) for x in _f32(bscale, 3, "bscale")])
    check(lib().vr_clip_convert_host(arr, n, b0, b1, out.ctypes.data_as(ctypes.c_void_p)))
    return out


def label_volume(labels):
    """The vr_volume of a label volume: a uint8 array (column-major; no Volume identity, so it is
    uploaded by every call), a RawVolume of uint8 or a DeviceVolume of uint8 (their TimeLastUpdate
    spares a repeated upload); None, False or an empty array: no labels.  Returns (VrVolume or None,
    keep-alive); the library checks the element type."""
    if labels is None or _is_false(labels):
        return None, None
    if isinstance(labels, DeviceVolume) or hasattr(labels, "TimeLastUpdate"):
        v = _vr_volume(labels)
        return (v if v.dims[0] * v.dims[1] * v.dims[2] else None), labels
    a = np.asarray(labels)
    if a.size == 0:
        return None, None
    if a.dtype != np.uint8:
        raise _lib.VrError(1, "sync_labels: labels must be a uint8 array, a RawVolume of uint8, [] or false")
    if a.ndim > 3:
        raise _lib.VrError(1, "sync_labels: labels must have at most 3 dimensions")
    a = np.asfortranarray(a)
    v = VrVolume()
    v.data = a.ctypes.data
    for i, d in enumerate(_matlab_dims(a)):
        v.dims[i] = d
    v.last_update = 0
    v.location = _lib.VR_HOST
    v.dtype = _lib.VR_U8
    return v, a


def sync_labels(handle, labels) -> None:
    """vr_sync_labels: the handle's label volume (label_volume(); None / False / [] drops it)."""
    v, keep = label_volume(labels)
    check(lib().vr_sync_labels(_handle(handle), ctypes.byref(v) if v is not None else None))
    del keep


def label_gains(gains):
    """A gain table as a contiguous single vector (None, False or empty: no gains).  Returns (array or
    None, n); the library checks the count and the values."""
    if gains is None or _is_false(gains):
        return None, 0
    a = np.asarray(gains)
    if a.size == 0:
        return None, 0
    if a.dtype.kind not in "fiu" or a.size != max(a.shape, default=0):
        raise _lib.VrError(1, "set_label_gains: gains must be a real vector of at most 256 entries, [] or false")
    a = np.ascontiguousarray(a.reshape(-1), dtype=np.float32)
    return a, int(a.size)


def set_label_gains(handle, gains) -> None:
    """vr_set_label_gains: replace the handle's gain table, one fp32 gain per label (label_gains();
    None / False / [] clears it)."""
    a, n = label_gains(gains)
    check(lib().vr_set_label_gains(_handle(handle), a.ctypes.data if a is not None else None, n))


def get_label_gains(handle) -> np.ndarray:
    """vr_get_label_gains: the handle's gain table as set, [n] single (empty: none)."""
    out = np.zeros(_lib.VR_LABEL_GAINS_MAX, np.float32)
    n = ctypes.c_int32(0)
    check(lib().vr_get_label_gains(_handle(handle), out.ctypes.data, ctypes.byref(n)))
    return out[:n.value].copy()


def label_gain_host(src, labels, gains) -> np.ndarray:
    """vr_label_gain_host: the label pass's value rule on the CPU -- src single, labels uint8 of the same
    shape, gains as label_gains(); returns labels < n ? src * gains[labels] : src, shaped like src."""
    s = np.asarray(src, dtype=np.float32)
    l = np.asarray(labels, dtype=np.uint8)
    if l.shape != s.shape:
        raise _lib.VrError(1, "label_gain_host: src and labels differ in shape")
    sf = np.ascontiguousarray(s.reshape(-1, order="F"))
    lf = np.ascontiguousarray(l.reshape(-1, order="F"))
    a, n = label_gains(gains)
    out = np.empty(sf.size, np.float32)
    check(lib().vr_label_gain_host(sf.ctypes.data, lf.ctypes.data, a.ctypes.data if a is not None else None, n, sf.size,
                                   out.ctypes.data))
    return out.reshape(s.shape, order="F")


def smoothing_sigma(sigma):
    """A smoothing sigma as three singles along dims[0..2] of Data: a real scalar (all three axes) or a
    3-vector; None, False or empty: none (all zero).  The library checks the values."""
    if sigma is None or _is_false(sigma):
        return np.zeros(3, np.float32)
    a = np.asarray(sigma)
    if a.size == 0:
        return np.zeros(3, np.float32)
    if a.dtype.kind not in "fiu" or a.size not in (1, 3) or a.size != max(a.shape, default=1):
        raise _lib.VrError(1, "set_smoothing: sigma must be a real scalar or 3-vector, [] or false")
    a = a.reshape(-1).astype(np.float32)
    return np.ascontiguousarray(np.repeat(a, 3) if a.size == 1 else a)


def set_smoothing(handle, sigma) -> None:
    """vr_set_smoothing: Gaussian smoothing of the handle's resident emission volume, sigma in voxels
    (smoothing_sigma(); None / False / [] / zeros clear it)."""
    a = smoothing_sigma(sigma)
    check(lib().vr_set_smoothing(_handle(handle), a.ctypes.data))


def get_smoothing(handle) -> np.ndarray:
    """vr_get_smoothing: the handle's sigma as set, [3] single (zeros: none)."""
    out = np.zeros(3, np.float32)
    check(lib().vr_get_smoothing(_handle(handle), out.ctypes.data))
    return out


def smooth_weights_host(sigma):
    """vr_smooth_weights_host: (R, the 2R+1 fp32 weights) of one axis."""
    w = np.zeros(_lib.VR_SMOOTH_MAX_TAPS, np.float32)
    r = ctypes.c_int32(0)
    check(lib().vr_smooth_weights_host(float(np.float32(sigma)), ctypes.byref(r), w.ctypes.data))
    return int(r.value), w[:2 * r.value + 1].copy()


def smooth_host(src, sigma) -> np.ndarray:
    """vr_smooth_host: the smoothing's value rule on the CPU -- src single with at most 3 dimensions
    (column-major: axis j of the array is dims[j]), sigma as smoothing_sigma(); shaped like src."""
    s = np.asarray(src, dtype=np.float32)
    if s.ndim > 3:
        raise _lib.VrError(1, "smooth_host: src must have at most 3 dimensions")
    dims = (ctypes.c_uint64 * 3)(*(list(s.shape) + [1] * (3 - s.ndim)))
    sf = np.ascontiguousarray(s.reshape(-1, order="F"))
    a = smoothing_sigma(sigma)
    out = np.empty(sf.size, np.float32)
    check(lib().vr_smooth_host(sf.ctypes.data, dims, a.ctypes.data, out.ctypes.data))
    return out.reshape(s.shape, order="F")


DECONV_FLOOR = np.float32(1e-6)  # the default floor of 'set_deconvolution'


def deconvolution_sigma(sigma):
    """A PSF sigma as three singles along dims[0..2] of Data, as smoothing_sigma()."""
    try:
        return smoothing_sigma(sigma)
    except _lib.VrError:
        raise _lib.VrError(1, "set_deconvolution: sigma must be a real scalar or 3-vector, [] or false") from None


def _deconvolution_count(iterations) -> int:
    a = np.asarray(iterations)
    if a.size != 1 or a.dtype.kind not in "fiu" or not np.isfinite(a.reshape(-1)[0]) or \
            float(a.reshape(-1)[0]) != int(a.reshape(-1)[0]):
        raise _lib.VrError(1, "set_deconvolution: iterations must be an integer scalar in 0..64")
    n = int(a.reshape(-1)[0])
    if n < 0 or n > _lib.VR_DECONV_MAX_ITERATIONS:
        raise _lib.VrError(1, "set_deconvolution: iterations must be an integer scalar in 0..64")
    return n


def _deconvolution_floor(floor) -> float:
    if floor is None:
        return float(DECONV_FLOOR)
    a = np.asarray(floor)
    if a.size != 1 or a.dtype.kind not in "fiu":
        raise _lib.VrError(1, "set_deconvolution: floor must be a real scalar greater than 0")
    return float(np.float32(a.reshape(-1)[0]))  # (the library checks the value)


def set_deconvolution(handle, sigma, iterations=0, floor=None) -> None:
    """vr_set_deconvolution: Richardson-Lucy deconvolution of the handle's resident emission volume with a
    Gaussian PSF of `sigma` voxels (deconvolution_sigma()), `iterations` in 0..64, `floor` (default 1e-6
    single) under the division; None / False / [] / zeros as sigma, or 0 iterations, clear it."""
    a = deconvolution_sigma(sigma)
    check(lib().vr_set_deconvolution(_handle(handle), a.ctypes.data, _deconvolution_count(iterations),
                                     _deconvolution_floor(floor)))


def get_deconvolution(handle):
    """vr_get_deconvolution: (sigma [3] single, iterations, floor) as set; (zeros, 0, 0.0): none."""
    sg = np.zeros(3, np.float32)
    n = ctypes.c_int32(0)
    fl = ctypes.c_float(0.0)
    check(lib().vr_get_deconvolution(_handle(handle), sg.ctypes.data, ctypes.byref(n), ctypes.byref(fl)))
    return sg, int(n.value), np.float32(fl.value)


def deconvolve_host(src, sigma, iterations, floor=None) -> np.ndarray:
    """vr_deconvolve_host: the deconvolution's value rule on the CPU -- src single with at most 3 dimensions
    (column-major: axis j of the array is dims[j]); shaped like src."""
    s = np.asarray(src, dtype=np.float32)
    if s.ndim > 3:
        raise _lib.VrError(1, "deconvolve_host: src must have at most 3 dimensions")
    dims = (ctypes.c_uint64 * 3)(*(list(s.shape) + [1] * (3 - s.ndim)))
    sf = np.ascontiguousarray(s.reshape(-1, order="F"))
    a = deconvolution_sigma(sigma)
    out = np.empty(sf.size, np.float32)
    check(lib().vr_deconvolve_host(sf.ctypes.data, dims, a.ctypes.data, _deconvolution_count(iterations),
                                   _deconvolution_floor(floor), out.ctypes.data))
    return out.reshape(s.shape, order="F")


def deconv_axis_device(d_src: int, d_dst: int, dims, axis: int, d_weights: int, radius: int, epi: int, d_aux: int = 0,
                       floor=DECONV_FLOOR, flags: int = 0, d_stats: int = 0, stream: int = 0) -> None:
    """vr_deconv_axis_device: one filter pass with an epilogue of the deconvolution (_lib.VR_EPI_*) between
    padded device buffers (measurements); d_aux may be d_dst for the update."""
    d = (ctypes.c_uint64 * 3)(*(int(x) for x in dims))
    check(lib().vr_deconv_axis_device(ctypes.c_void_p(int(d_src)), ctypes.c_void_p(int(d_dst)), d, int(axis),
                                      ctypes.c_void_p(int(d_weights)), int(radius), int(epi),
                                      ctypes.c_void_p(int(d_aux)) if d_aux else None, float(floor), int(flags),
                                      ctypes.c_void_p(int(d_stats)) if d_stats else None,
                                      ctypes.c_void_p(int(stream)) if stream else None))


def deconv_pointwise_device(d_src: int, d_dst: int, dims, epi: int, d_aux: int, floor=DECONV_FLOOR, flags: int = 0,
                            stream: int = 0) -> None:
    """vr_deconv_pointwise_device: the ratio or the update as an elementwise launch over padded device
    buffers (measurements)."""
    d = (ctypes.c_uint64 * 3)(*(int(x) for x in dims))
    check(lib().vr_deconv_pointwise_device(ctypes.c_void_p(int(d_src)), ctypes.c_void_p(int(d_dst)), d, int(epi),
                                           ctypes.c_void_p(int(d_aux)), float(floor), int(flags),
                                           ctypes.c_void_p(int(stream)) if stream else None))


def smooth_fused_device(d_src: int, d_dst: int, dims, d_weights: int, radius, d_stats: int = 0, stream: int = 0) -> None:
    """vr_smooth_fused_device: the fused launch between two padded device buffers (measurements); d_weights
    3 x 25 floats, radius three ints."""
    d = (ctypes.c_uint64 * 3)(*(int(x) for x in dims))
    r = (ctypes.c_int32 * 3)(*(int(x) for x in radius))
    check(lib().vr_smooth_fused_device(ctypes.c_void_p(int(d_src)), ctypes.c_void_p(int(d_dst)), d,
                                       ctypes.c_void_p(int(d_weights)), r,
                                       ctypes.c_void_p(int(d_stats)) if d_stats else None,
                                       ctypes.c_void_p(int(stream)) if stream else None))


def read_emission(handle, offset: int, count: int) -> np.ndarray:
    """vr_debug_read_emission: `count` floats at element `offset` of the handle's padded resident emission
    buffer (measurements)."""
    out = np.empty(int(count), np.float32)
    check(lib().vr_debug_read_emission(_handle(handle), int(offset), int(count), out.ctypes.data))
    return out


def emission_version(handle) -> int:
    """vr_debug_emission_version: the upload version of the handle's resident emission buffer (every upload
    and every derivation takes a new one; 0: no buffer)."""
    v = ctypes.c_uint64(0)
    check(lib().vr_debug_emission_version(_handle(handle), ctypes.byref(v)))
    return int(v.value)


def derive_times(handle):
    """vr_debug_derive_times: (ms of the last derivation's passes with the statistics read-back, ms of its
    occupancy rebuild), host clock (measurements)."""
    out = (ctypes.c_double * 2)()
    check(lib().vr_debug_derive_times(_handle(handle), out))
    return float(out[0]), float(out[1])


def smooth_axis_device(d_src: int, d_dst: int, dims, axis: int, d_weights: int, radius: int, d_stats: int = 0,
                       stream: int = 0) -> None:
    """vr_smooth_axis_device: one axis pass between two padded device buffers (measurements)."""
    d = (ctypes.c_uint64 * 3)(*(int(x) for x in dims))
    check(lib().vr_smooth_axis_device(ctypes.c_void_p(int(d_src)), ctypes.c_void_p(int(d_dst)), d, int(axis),
                                      ctypes.c_void_p(int(d_weights)), int(radius),
                                      ctypes.c_void_p(int(d_stats)) if d_stats else None,
                                      ctypes.c_void_p(int(stream)) if stream else None))


SLICE_MODES = {"max": _lib.VR_SLICE_MAX, "min": _lib.VR_SLICE_MIN, "sum": _lib.VR_SLICE_SUM}
SLICE_SOURCES = {"emission": _lib.VR_SLICE_EMISSION, "absorption": _lib.VR_SLICE_ABSORPTION,
                 "reflection": _lib.VR_SLICE_REFLECTION}


def slice_mode(mode) -> int:
    """The vr_slice_mode code of 'max' / 'min' / 'sum' (or of a code itself)."""
    if isinstance(mode, str):
        if mode.lower() not in SLICE_MODES:
            raise _lib.VrError(1, "slice: unknown slice mode")
        return SLICE_MODES[mode.lower()]
    return int(np.asarray(mode).reshape(-1)[0])


def slice_source(source) -> int:
    """The vr_slice_source code of 'emission' / 'absorption' / 'reflection' (or of a code itself)."""
    if isinstance(source, str):
        if source.lower() not in SLICE_SOURCES:
            raise _lib.VrError(1, "slice: unknown slice source")
        return SLICE_SOURCES[source.lower()]
    return int(np.asarray(source).reshape(-1)[0])


def make_slice(geom, res, n=1, mode="max", source="emission") -> _lib.VrSlice:
    """A vr_slice from the mex command's arguments: geom 3 x 4 single [origin du dv dw] (columns),
    res [H W], n slab samples, mode and source as strings or codes.  The library checks the values."""
    g = np.asarray(geom)
    if g.dtype != np.float32 or g.shape != (3, 4):
        raise _lib.VrError(1, "render_slice: geom must be a single 3 x 4 matrix [origin du dv dw]")
    r = np.asarray(res).reshape(-1)
    if r.size != 2:
        raise _lib.VrError(1, "render_slice: res must be [H W]")
    s = _lib.VrSlice()
    for j in range(3):
        s.origin[j], s.du[j], s.dv[j], s.dw[j] = g[j, 0], g[j, 1], g[j, 2], g[j, 3]
    s.resolution[0], s.resolution[1] = int(r[0]), int(r[1])
    s.samples = int(np.asarray(n).reshape(-1)[0])
    s.mode, s.source = slice_mode(mode), slice_source(source)
    return s


def slice_geom(s) -> np.ndarray:
    """The 3 x 4 single matrix [origin du dv dw] of a vr_slice (the mex command's geom)."""
    return np.asfortranarray(np.array([list(s.origin), list(s.du), list(s.dv), list(s.dw)], np.float32).T)


def slice_axis(dims, axis: int, index: float, thickness: int = 1) -> _lib.VrSlice:
    """vr_slice_axis: the voxel plane at 0-based `index` along `axis` (0-based) of a volume of `dims`, one
    pixel per voxel, the lower-numbered remaining dimension along the rows; a slab of `thickness` samples
    one voxel apart centred on the index.  mode and source are left 0 ('max', 'emission')."""
    d = (ctypes.c_uint64 * 3)(*(list(int(x) for x in dims) + [1] * (3 - len(dims))))
    s = _lib.VrSlice()
    check(lib().vr_slice_axis(d, int(axis), float(index), int(thickness), ctypes.byref(s)))
    return s


def slice_oblique(dims, element_size_um, point_q, normal_um, up_um, pixel_um: float, H: int, W: int,
                  thickness: int = 1) -> _lib.VrSlice:
    """vr_slice_oblique: the H x W plane through point_q (normalized volume coordinate, the image centre)
    with physical normal normal_um and rows along up_um projected into the plane, pixels and slab samples
    pixel_um apart; element_size_um in MATLAB order, the directions with component j along dims[j]."""
    d = (ctypes.c_uint64 * 3)(*(list(int(x) for x in dims) + [1] * (3 - len(dims))))
    es = (ctypes.c_float * 3)(*[float(x) for x in _f32(element_size_um, 3, "ElementSizeUm")])
    vec = [(ctypes.c_double * 3)(*[float(x) for x in np.asarray(v, np.float64).reshape(-1)[:3]])
           for v in (point_q, normal_um, up_um)]
    s = _lib.VrSlice()
    check(lib().vr_slice_oblique(d, es, vec[0], vec[1], vec[2], float(pixel_um), int(H), int(W), int(thickness),
                                 ctypes.byref(s)))
    return s


def render_slice_device(handle, s, d_out: int, d_aux: int = 0, d_labels: int = 0, stream: int = 0) -> None:
    """A slice into device memory (vr_render_slice_device), asynchronous on `stream`: s from make_slice /
    slice_axis / slice_oblique; planes [H, W] column-major; d_aux = 0 / d_labels = 0: no such plane."""
    check(lib().vr_render_slice_device(_handle(handle), ctypes.byref(s),
                                       ctypes.c_void_p(int(d_out)) if d_out else None,
                                       ctypes.c_void_p(int(d_aux)) if d_aux else None,
                                       ctypes.c_void_p(int(d_labels)) if d_labels else None,
                                       ctypes.c_void_p(int(stream)) if stream else None))


# numpy view of vr_hist_row (include/vrhip.h), and the column order of the mex command's summary
HIST_ROW_DTYPE = np.dtype([("total", "<u8"), ("below", "<u8"), ("above", "<u8"), ("nan", "<u8"), ("ninf", "<u8"),
                           ("min", "<f4"), ("max", "<f4"), ("sum", "<f8")])
HIST_SUMMARY = ("total", "below", "above", "nan", "ninf", "min", "max", "sum")


def make_histogram(source, nbins, limits, labels=None, use_clip=0) -> _lib.VrHistogram:
    """A vr_histogram from the mex command's arguments: source as a string or code, nbins, limits single
    [lo hi], labels int32 [first count] (count 0, or None: one row, labels not read), use_clip 0 / 1 / false /
    true.  The library checks the values."""
    lim = np.asarray(limits)
    if lim.dtype != np.float32 or lim.size != 2:
        raise _lib.VrError(1, "volume_histogram: limits must be a single vector [lo hi]")
    lab = np.int32([0, 0]) if labels is None else np.asarray(labels)
    if lab.dtype != np.int32 or lab.size != 2:
        raise _lib.VrError(1, "volume_histogram: labels must be an int32 vector [first count]")
    q = _lib.VrHistogram()
    q.source = slice_source(source)
    q.nbins = int(np.asarray(nbins).reshape(-1)[0])
    q.lim[0], q.lim[1] = lim.reshape(-1)
    q.label_first, q.label_count = (int(x) for x in lab.reshape(-1))
    q.use_clip = int(np.asarray(use_clip).reshape(-1)[0])
    return q


def histogram_rows(q) -> int:
    """Rows of a vr_histogram's tables: label_count + 1, or 1 without labels."""
    return q.label_count + 1 if q.label_count > 0 else 1


def volume_histogram(handle, q):
    """vr_volume_histogram: (counts uint64 [rows, nbins], rows as a HIST_ROW_DTYPE record array [rows])."""
    rows = histogram_rows(q)
    if not (1 <= q.nbins <= _lib.VR_HIST_MAX_BINS and 1 <= rows <= 257):  # the library says why
        rows, nb = 1, 1
    else:
        nb = q.nbins
    counts = np.zeros((rows, nb), dtype=np.uint64)
    summ = np.zeros(rows, dtype=HIST_ROW_DTYPE)
    check(lib().vr_volume_histogram(_handle(handle), ctypes.byref(q), counts.ctypes.data_as(ctypes.c_void_p),
                                    summ.ctypes.data_as(ctypes.c_void_p)))
    return counts, summ


def volume_histogram_device(handle, q, d_counts: int, d_rows: int = 0, stream: int = 0) -> None:
    """A histogram into device memory (vr_volume_histogram_device), asynchronous on `stream`: q from
    make_histogram; d_counts uint64 [rows][nbins]; d_rows rows vr_hist_row records of 56 bytes, 0: none."""
    check(lib().vr_volume_histogram_device(_handle(handle), ctypes.byref(q),
                                           ctypes.c_void_p(int(d_counts)) if d_counts else None,
                                           ctypes.c_void_p(int(d_rows)) if d_rows else None,
                                           ctypes.c_void_p(int(stream)) if stream else None))


def histogram_bin_host(v, nbins: int, limits) -> np.ndarray:
    """vr_histogram_bin_host: the kernel's class rule on the CPU -- per value its bin, or -1 below, -2 above,
    -3 NaN."""
    a = np.ascontiguousarray(v, dtype=np.float32).reshape(-1)
    lim = (ctypes.c_float * 2)(*[float(x) for x in np.asarray(limits, np.float32).reshape(-1)[:2]])
    out = np.zeros(a.size, dtype=np.int32)
    check(lib().vr_histogram_bin_host(a.ctypes.data_as(ctypes.c_void_p) if a.size else None, a.size, int(nbins), lim,
                                      out.ctypes.data_as(ctypes.c_void_p) if a.size else None))
    return out


def set_option(name: str, value: int) -> None:
    """vr_set_option: a process-wide library option (include/vrhip.h)."""
    check(lib().vr_set_option(name.encode(), int(value)))


def enable_test_switches(on: bool = True) -> None:
    """Let the library read the kernel-variant / schedule switches of the environment (VR_NO_LDS,
    VR_DEPTH_LANES, VR_SCHED, ...; INTEGRATION.md "Runtime switches") -- the GPU tests and the
    measurement tools; the MATLAB MEX never does, so a MATLAB session's environment cannot.  (An A/B
    build of an earlier tree, VR_LIB_PATH, may predate the option: a DIAG=1 build reads them anyway.)"""
    if not hasattr(lib(), "vr_set_option"):
        return
    set_option("test_switches", 1 if on else 0)


def last_march_kernel() -> str:
    """The demangled name of the march kernel instantiation the last render launched."""
    buf = ctypes.create_string_buffer(256)
    check(lib().vr_last_march_kernel(buf, len(buf)))
    return buf.value.decode()


def last_launch_flags() -> dict:
    """The launch-wide decisions of the last frame this process built (vr_last_launch_flags), by
    name: tame, small_x, eds_finite, skip_empty, re_ok, lut_ok, tap_half, ab_alias, share, big and
    occ (an occupancy map is bound), each a bool."""
    word = ctypes.c_uint32(0)
    check(lib().vr_last_launch_flags(ctypes.byref(word)))
    return {name: bool(word.value >> bit & 1) for bit, name in enumerate(_lib.LAUNCH_FLAGS)}


def assemble_partitions(d_parts: int, width: int, height: int, block_cols: int, num_parts: int, max_cols: int,
                        d_out: int, stream: int = 0) -> None:
    check(lib().vr_assemble_partitions(ctypes.c_void_p(int(d_parts)), int(width), int(height), int(block_cols),
                                       int(num_parts), int(max_cols), ctypes.c_void_p(int(d_out)),
                                       ctypes.c_void_p(int(stream)) if stream else None))


def synth_shell_device(d_out: int, n: int, stream: int = 0) -> None:
    check(lib().vr_synth_shell_device(ctypes.c_void_p(int(d_out)), int(n),
                                      ctypes.c_void_p(int(stream)) if stream else None))


def synth_shell_planes_device(d_out: int, n: int, z_first: int, count: int, stream: int = 0) -> None:
    check(lib().vr_synth_shell_planes_device(ctypes.c_void_p(int(d_out)), int(n), int(z_first), int(count),
                                             ctypes.c_void_p(int(stream))))


def gradient_device(d_data: int, dims, d_gx: int, d_gy: int, d_gz: int, stream: int = 0) -> None:
    """Volume.grad on the device (vr_gradient_device): MATLAB gradient() of the column-major single
    array at d_data with dims (d0, d1, d2) into d_gx (dim 2), d_gy (dim 1), d_gz (dim 3)."""
    dd = (ctypes.c_uint64 * 3)(*[int(x) for x in dims])
    _lib.check(_lib.lib().vr_gradient_device(d_data, dd, d_gx, d_gy, d_gz, stream))


def henyey_greenstein_device(n: int, g: float, d_out: int, stream: int = 0) -> None:
    """vr_henyey_greenstein_device: HenyeyGreenstein(n, g) into device memory (n^3 floats)."""
    check(lib().vr_henyey_greenstein_device(ctypes.c_uint32(int(n)), ctypes.c_float(g), ctypes.c_void_p(int(d_out)),
                                            ctypes.c_void_p(int(stream)) if stream else None))


def normalize_device(d_in: int, n: int, new_min: float, new_max: float, d_out: int, stream: int = 0) -> None:
    """vr_normalize_device: Volume.normalize of n single values in device memory (d_out may be d_in)."""
    check(lib().vr_normalize_device(ctypes.c_void_p(int(d_in)), int(n), float(new_min), float(new_max),
                                    ctypes.c_void_p(int(d_out)), ctypes.c_void_p(int(stream)) if stream else None))


def resize_device(d_in: int, in_dims, out_dims, d_out: int, stream: int = 0) -> None:
    """vr_resize_device: Volume.resize (imresize3 cubic) of a column-major device volume."""
    a = (ctypes.c_uint64 * 3)(*(list(int(x) for x in in_dims) + [1] * (3 - len(in_dims))))
    b = (ctypes.c_uint64 * 3)(*(list(int(x) for x in out_dims) + [1] * (3 - len(out_dims))))
    check(lib().vr_resize_device(ctypes.c_void_p(int(d_in)), a, b, ctypes.c_void_p(int(d_out)),
                                 ctypes.c_void_p(int(stream)) if stream else None))


def resize_contributions(in_len: int, out_len: int):
    """(weights [out_len, P] float64, 0-based indices [out_len, P] int32) of one resize axis."""
    P = ctypes.c_int32(0)
    check(lib().vr_resize_contributions(int(in_len), int(out_len), ctypes.byref(P), None, None))
    w = np.zeros((int(out_len), P.value), np.float64)
    i = np.zeros((int(out_len), P.value), np.int32)
    check(lib().vr_resize_contributions(int(in_len), int(out_len), ctypes.byref(P), w.ctypes.data_as(ctypes.c_void_p),
                                        i.ctypes.data_as(ctypes.c_void_p)))
    return w, i


def channel(handle, t_sync, volumes, render_argv):
    """One vr_channel: handle, the 'sync_volumes' arguments after the handle (t_sync, Emission,
    Reflection, Absorption[, dx, dy, dz]) and the positional 'render' arguments after the handle.
    Returns (VrChannel, keep-alive list)."""
    c = _lib.VrChannel()
    c.handle = _handle(handle)
    c.time_last_mem_sync = int(np.asarray(t_sync).reshape(-1)[0])
    vols = [_vr_volume(v) for v in volumes]
    if len(vols) not in (3, 6):
        raise _lib.VrError(5, "channel: expected 3 or 6 volumes")
    c.emission, c.reflection, c.absorption = (ctypes.pointer(v) for v in vols[:3])
    if len(vols) == 6:
        c.dx, c.dy, c.dz = (ctypes.pointer(v) for v in vols[3:])
    ra, keep = render_args(*render_argv)
    c.args = ctypes.pointer(ra)
    return c, [vols, ra, keep, [(getattr(v, "Data", None), getattr(v, "RawData", None)) for v in volumes]]


def render_channels(channels, stereo: bool = False, base: float = 0.0):
    """Multi-channel frame (vr_render_channels): `channels` = [(handle, t_sync, volumes,
    render_argv), ...]; returns one image (H, W, 3) per channel, or per channel a (left, right)
    pair when stereo."""
    built = [channel(*c) for c in channels]
    arr = (_lib.VrChannel * len(built))(*[b[0] for b in built])
    res = np.asarray(channels[0][3][4]).reshape(-1)
    H, W = int(res[0]), int(res[1])
    nv = 2 if stereo else 1
    out = np.zeros((len(built) * nv, H * W * 3), dtype=np.float32)
    check(lib().vr_render_channels(arr, len(built), 1 if stereo else 0, float(base),
                                   out.ctypes.data_as(ctypes.c_void_p) if out.size else None))
    del built
    imgs = [out[k].reshape((H, W, 3), order="F") for k in range(out.shape[0])]
    return [(imgs[2 * i], imgs[2 * i + 1]) for i in range(len(channels))] if stereo else imgs


def render_channels_device(channels, d_out: int, stereo: bool = False, base: float = 0.0, stream: int = 0) -> None:
    """vr_render_channels_device: channel i's view e into d_out + (i * eyes + e) * H*W*3 floats."""
    built = [channel(*c) for c in channels]
    arr = (_lib.VrChannel * len(built))(*[b[0] for b in built])
    check(lib().vr_render_channels_device(arr, len(built), 1 if stereo else 0, float(base),
                                          ctypes.c_void_p(int(d_out)), ctypes.c_void_p(int(stream)) if stream else None))
    del built


def sum_channels_device(d_in: int, n: int, views: int, image_floats: int, d_out: int, stream: int = 0) -> None:
    """vr_sum_channels_device: d_out[e] = d_in[0][e] + d_in[1][e] + ... (fp32, channel order)."""
    check(lib().vr_sum_channels_device(ctypes.c_void_p(int(d_in)), int(n), int(views), int(image_floats),
                                       ctypes.c_void_p(int(d_out)), ctypes.c_void_p(int(stream)) if stream else None))


def _group_devices():
    """VR_DEVICES (comma-separated device indices, primary first) selects multi-device handles."""
    import os
    ev = os.environ.get("VR_DEVICES", "").strip()
    return [int(x) for x in ev.split(",") if x.strip()] if ev else []


def volumeRender(cmd, *args):
    """The `volumeRender` mex: commands 'new', 'delete', 'mem_info', 'sync_volumes', 'render' (and
    'render_stereo', 'render_channels', 'render_projection', 'render_isosurface', 'render_transfer',
    'render_slice', 'volume_histogram', 'set_clip', 'sync_labels', 'set_label_gains', 'set_smoothing', 'set_deconvolution', which the reference does
    not have)."""
    nrhs = 1 + len(args)
    if not isinstance(cmd, str) or len(cmd) >= 64:
        raise _lib.VrError(1, "First input should be a command string less than 64 characters long.")
    L = lib()
    if cmd == "new":
        p = ctypes.c_void_p()
        devs = _group_devices()
        if devs:  # VR_DEVICES="0,1,...": a multi-device group (vr_new_multi), as the MEX adaptor does
            arr = (ctypes.c_int32 * len(devs))(*devs)
            check(L.vr_new_multi(arr, len(devs), ctypes.byref(p)))
        else:
            check(L.vr_new(ctypes.byref(p)))
        return np.uint64(p.value)
    if cmd == "render_channels":  # vr_render_channels: ('render_channels', channels[, stereo, base])
        return render_channels(*args)
    if nrhs < 2:
        raise _lib.VrError(1, "Second input should be a class instance handle.")
    h = _handle(args[0])
    if cmd == "delete":
        check(L.vr_delete(h))
        if nrhs != 2:
            warnings.warn("Delete: Unexpected arguments ignored.")
        return None
    if cmd == "mem_info":
        buf = ctypes.create_string_buffer(1 << 14)
        check(L.vr_mem_info(h, buf, len(buf)))
        print(buf.value.decode(), end="")
        return None
    if cmd == "sync_volumes":
        if nrhs < 6:
            raise _lib.VrError(1, "insufficient parameter!")
        t_sync = int(np.asarray(args[1]).reshape(-1)[0])
        em, re, ab = (_vr_volume(v) for v in args[2:5])  # order: Emission, Reflection, Absorption
        if nrhs == 9:
            gx, gy, gz = (_vr_volume(v) for v in args[5:8])
            check(L.vr_sync_volumes(h, t_sync, ctypes.byref(em), ctypes.byref(re), ctypes.byref(ab),
                                    ctypes.byref(gx), ctypes.byref(gy), ctypes.byref(gz)))
        elif nrhs == 6:
            check(L.vr_sync_volumes(h, t_sync, ctypes.byref(em), ctypes.byref(re), ctypes.byref(ab),
                                    None, None, None))
        else:  # 7, 8 or > 9 arguments: the previous gradient volumes are kept (render.cpp:105-113)
            flag = VrVolume()  # not read: only its presence selects the form
            check(L.vr_sync_volumes(h, t_sync, ctypes.byref(em), ctypes.byref(re), ctypes.byref(ab),
                                    ctypes.byref(flag), ctypes.byref(flag) if nrhs != 7 else None, None))
        if nrhs > 9:
            warnings.warn("SyncVolumes: Unexpected arguments ignored.")
        return None
    if cmd == "set_clip":  # ('set_clip', h, planes): planes 4 x n single, columns [n0; n1; n2; offset]; [] / false clears
        if nrhs < 3:
            raise _lib.VrError(1, "insufficient parameter!")
        pl = args[1]
        if not (pl is None or _is_false(pl)):
            pl = np.asarray(pl)
            if pl.size and (pl.ndim != 2 or pl.shape[0] != 4):
                raise _lib.VrError(1, "set_clip: planes must be a 4 x n matrix with columns [n0; n1; n2; offset]")
            pl = pl.T
        arr, n = clip_planes(pl)
        check(L.vr_set_clip(h, arr, n))
        return None
    if cmd == "sync_labels":  # ('sync_labels', h, labels): a uint8 array or a RawVolume of uint8; [] / false drops
        if nrhs < 3:
            raise _lib.VrError(1, "insufficient parameter!")
        if nrhs > 3:
            raise _lib.VrError(1, "sync_labels: too many input arguments")
        lb = args[1]
        if isinstance(lb, (bool, np.bool_)) and bool(lb):
            raise _lib.VrError(1, "sync_labels: labels must be a uint8 array, a RawVolume of uint8, [] or false")
        sync_labels(args[0], lb)
        return None
    if cmd == "set_label_gains":  # ('set_label_gains', h, gains): a single vector of at most 256 entries; [] / false clears
        if nrhs < 3:
            raise _lib.VrError(1, "insufficient parameter!")
        if nrhs > 3:
            raise _lib.VrError(1, "set_label_gains: too many input arguments")
        g = args[1]
        if not (g is None or _is_false(g)):
            g = np.asarray(g)
            if g.size and (g.dtype != np.float32 or g.size != max(g.shape, default=0)):
                raise _lib.VrError(1, "set_label_gains: gains must be a single vector of at most 256 entries, [] or false")
            if g.size > _lib.VR_LABEL_GAINS_MAX:
                raise _lib.VrError(1, "set_label_gains: gains must be a single vector of at most 256 entries, [] or false")
        set_label_gains(args[0], g)
        return None
    if cmd == "set_smoothing":  # ('set_smoothing', h, sigma): a single or double scalar or 3-vector; [] / false clears
        if nrhs < 3:
            raise _lib.VrError(1, "insufficient parameter!")
        if nrhs > 3:
            raise _lib.VrError(1, "set_smoothing: too many input arguments")
        sg = args[1]
        if not (sg is None or _is_false(sg)):
            sg = np.asarray(sg)
            if sg.dtype not in (np.float32, np.float64) or sg.ndim > 2 or (sg.size and (
                    sg.size not in (1, 3) or sg.size != max(sg.shape, default=1))):
                raise _lib.VrError(1, "set_smoothing: sigma must be a single or double scalar or 3-vector, [] or false")
        set_smoothing(args[0], sg)
        return None
    if cmd == "set_deconvolution":
        # ('set_deconvolution', h, sigma, iterations[, floor]): sigma a single or double scalar or 3-vector,
        # iterations an integer-valued real scalar in 0..64, floor a single or double scalar (default 1e-6
        # single); [] / false as sigma, or iterations = 0, clears
        if nrhs < 3:
            raise _lib.VrError(1, "insufficient parameter!")
        if nrhs > 5:
            raise _lib.VrError(1, "set_deconvolution: too many input arguments")
        sg = args[1]
        cleared = sg is None or _is_false(sg) or np.asarray(sg).size == 0
        if not cleared:
            sg = np.asarray(sg)
            if sg.dtype not in (np.float32, np.float64) or sg.ndim > 2 or sg.size not in (1, 3) or \
                    sg.size != max(sg.shape, default=1):
                raise _lib.VrError(1, "set_deconvolution: sigma must be a single or double scalar or 3-vector, [] or false")
        if nrhs < 4 and not cleared:
            raise _lib.VrError(1, "set_deconvolution: iterations is missing")
        if nrhs > 4 and np.asarray(args[3]).dtype not in (np.float32, np.float64):
            raise _lib.VrError(1, "set_deconvolution: floor must be a real scalar greater than 0")
        set_deconvolution(args[0], None if cleared else sg, args[2] if nrhs > 3 else 0, args[3] if nrhs > 4 else None)
        return None
    if cmd == "render_stereo":  # fused stereo pair (vr_render_stereo): args as 'render' + base
        ra, keep = render_args(*args[1:10])
        res = np.asarray(args[5]).reshape(-1)
        H, W = int(res[0]), int(res[1])
        left = np.zeros((H, W, 3), dtype=np.float32, order="F")
        right = np.zeros((H, W, 3), dtype=np.float32, order="F")
        check(L.vr_render_stereo(h, ctypes.byref(ra), float(args[10]),
                                 left.ctypes.data_as(ctypes.c_void_p) if left.size else None,
                                 right.ctypes.data_as(ctypes.c_void_p) if right.size else None))
        del keep
        return left, right
    if cmd == "render_projection":  # ('render_projection', h, <the nine render arguments>, mode)
        if nrhs < 12:
            raise _lib.VrError(1, "insufficient parameter!")
        ra, keep = render_args(*args[1:10])
        res = np.asarray(args[5]).reshape(-1)
        H, W = int(res[0]), int(res[1])
        out = np.zeros((H, W, 3), dtype=np.float32, order="F")
        aux = np.zeros((H, W), dtype=np.float32, order="F")
        check(L.vr_render_projection(h, ctypes.byref(ra), projection_mode(args[10]),
                                     out.ctypes.data_as(ctypes.c_void_p) if out.size else None,
                                     aux.ctypes.data_as(ctypes.c_void_p) if aux.size else None))
        del keep
        return out, aux
    if cmd == "render_slice":  # ('render_slice', h, geom 3 x 4 single, res [H W], n, mode, source)
        if nrhs < 7:
            raise _lib.VrError(1, "insufficient parameter!")
        if nrhs > 7:
            raise _lib.VrError(1, "render_slice: too many input arguments")
        s = make_slice(*args[1:6])
        H, W = int(s.resolution[0]), int(s.resolution[1])
        if H >= 2 ** 31 or W >= 2 ** 31 or H * W >= 2 ** 31:
            raise _lib.VrError(1, "slice: image resolution too large (H * W must be below 2^31)")
        img, aux, lab = (np.zeros((H, W), dtype=np.float32, order="F") for _ in range(3))
        check(L.vr_render_slice(h, ctypes.byref(s), *(p.ctypes.data_as(ctypes.c_void_p) if p.size else None
                                                      for p in (img, aux, lab))))
        return img, aux, lab
    if cmd == "volume_histogram":  # ('volume_histogram', h, source, nbins, single([lo hi]), int32([first count]), use_clip)
        if nrhs < 7:
            raise _lib.VrError(1, "insufficient parameter!")
        if nrhs > 7:
            raise _lib.VrError(1, "volume_histogram: too many input arguments")
        counts, summ = volume_histogram(args[0], make_histogram(*args[1:6]))
        # counts [nbins, rows] column-major: counts(:, r) is row r; summary [rows, 8] double
        summary = np.asfortranarray(np.stack([summ[k].astype(np.float64) for k in HIST_SUMMARY], axis=1))
        return np.asfortranarray(counts.T), summary
    if cmd == "render_isosurface":  # ('render_isosurface', h, <the nine render arguments>, level)
        if nrhs < 12:
            raise _lib.VrError(1, "insufficient parameter!")
        level = isosurface_level(args[10])
        ra, keep = render_args(*args[1:10])
        res = np.asarray(args[5]).reshape(-1)
        H, W = int(res[0]), int(res[1])
        out = np.zeros((H, W, 3), dtype=np.float32, order="F")
        depth = np.zeros((H, W), dtype=np.float32, order="F")
        normal = np.zeros((H, W, 3), dtype=np.float32, order="F")
        check(L.vr_render_isosurface(h, ctypes.byref(ra), ctypes.c_float(level),
                                     out.ctypes.data_as(ctypes.c_void_p) if out.size else None,
                                     depth.ctypes.data_as(ctypes.c_void_p) if depth.size else None,
                                     normal.ctypes.data_as(ctypes.c_void_p) if normal.size else None))
        del keep
        return out, depth, normal
    if cmd == "render_transfer":  # ('render_transfer', h, <the nine render arguments>, colormap [N 3],
        #                            clim [lo hi], alphamap [M 1] | false, alim [lo hi], 'value' | 'depth')
        if nrhs < 16:
            raise _lib.VrError(1, "insufficient parameter!")
        tf, tkeep = transfer(args[10], args[11], args[12], args[13], args[14])
        ra, keep = render_args(*args[1:10])
        res = np.asarray(args[5]).reshape(-1)
        H, W = int(res[0]), int(res[1])
        out = np.zeros((H, W, 3), dtype=np.float32, order="F")
        alpha = np.zeros((H, W), dtype=np.float32, order="F")
        check(L.vr_render_transfer(h, ctypes.byref(ra), ctypes.byref(tf),
                                   out.ctypes.data_as(ctypes.c_void_p) if out.size else None,
                                   alpha.ctypes.data_as(ctypes.c_void_p) if alpha.size else None))
        del keep, tkeep
        return out, alpha
    if cmd == "render":
        if nrhs < 11:
            raise _lib.VrError(1, "insufficient parameter!")
        ra, keep = render_args(*args[1:10])
        res = np.asarray(args[5]).reshape(-1)
        H, W = int(res[0]), int(res[1])
        out = np.zeros((H, W, 3), dtype=np.float32, order="F")
        check(L.vr_render(h, ctypes.byref(ra), out.ctypes.data_as(ctypes.c_void_p) if out.size else None))
        del keep
        return out
    return None
