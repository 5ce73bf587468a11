"""ctypes binding of libvrhip.so (the C-ABI of include/vrhip.h).

The shared object is built in-tree by ``volume_renderer_amd/csrc/Makefile`` (``__graft_entry__.build``).
There is no fallback: if the library is missing, importing the bindings raises.
"""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_float, c_int, c_int32, c_int64, c_size_t, c_uint32, c_uint64, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
_DEFAULT_PATH = os.path.join(_HERE, "libvrhip.so")
LIB_PATH = os.environ.get("VR_LIB_PATH") or _DEFAULT_PATH  # override: A/B builds

VR_OK = 0
VR_HOST = 0
VR_DEVICE = 1
# enum vr_dtype (include/vrhip.h): element type of VrVolume.data; VR_DTYPE_UNORM ORed onto U8 / U16
VR_F32, VR_U8, VR_U16, VR_I16, VR_F16 = 0, 1, 2, 3, 4
VR_DTYPE_UNORM = 0x100
# enum vr_projection
VR_PROJ_MIP, VR_PROJ_SUM = 0, 1
# enum vr_transfer_coord, VR_TF_MAX_ENTRIES
VR_TF_VALUE, VR_TF_DEPTH = 0, 1
VR_TF_MAX_ENTRIES = 1024
VR_CLIP_MAX = 6
VR_LABEL_GAINS_MAX = 256
VR_SMOOTH_MAX_SIGMA = 6.0
VR_SMOOTH_MAX_TAPS = 25
VR_DECONV_MAX_ITERATIONS = 64
VR_EPI_FILTER, VR_EPI_RATIO, VR_EPI_UPDATE = 1, 2, 3  # csrc/vr_deconv.h
VR_EPI_LOAD_DATA, VR_EPI_AUX_DATA = 1, 2
# enum vr_slice_mode, enum vr_slice_source, VR_SLICE_MAX_SAMPLES
VR_SLICE_MAX, VR_SLICE_MIN, VR_SLICE_SUM = 0, 1, 2
VR_SLICE_EMISSION, VR_SLICE_ABSORPTION, VR_SLICE_REFLECTION = 0, 1, 2
VR_SLICE_MAX_SAMPLES = 4096
# vr_volume_histogram
VR_HIST_MAX_BINS = 4096
VR_HIST_MAX_CELLS = 12288
# enum vr_launch_flag: the bits of vr_last_launch_flags, in bit order
LAUNCH_FLAGS = ("tame", "small_x", "eds_finite", "skip_empty", "re_ok", "lut_ok", "tap_half", "ab_alias", "share",
                "big", "occ")


class VrVolume(ctypes.Structure):
    _fields_ = [("data", c_void_p), ("dims", c_uint64 * 3), ("last_update", c_uint64),
                ("location", c_int32), ("dtype", c_int32)]


class VrLight(ctypes.Structure):
    _fields_ = [("position", c_float * 3), ("color", c_float * 3)]


class VrRenderArgs(ctypes.Structure):
    _fields_ = [("lights", POINTER(VrLight)), ("num_lights", c_int64),
                ("illumination", POINTER(VrVolume)), ("factors", c_float * 3),
                ("element_size_um", c_float * 3), ("resolution", c_uint64 * 2),
                ("rotation_flipped", c_float * 9), ("props", c_float * 3),
                ("opacity_threshold", c_float), ("color", c_float * 3)]


class VrSlab(ctypes.Structure):
    _fields_ = [("depth", c_uint64), ("z_first", c_uint64), ("z0", ctypes.c_double), ("z1", ctypes.c_double),
                ("direction", c_int32), ("reserved", c_int32)]


class VrPartition(ctypes.Structure):
    _fields_ = [("block_cols", c_int32), ("part", c_int32), ("num_parts", c_int32),
                ("reserved", c_int32)]


class VrTransfer(ctypes.Structure):
    _fields_ = [("colormap", c_void_p), ("n_color", c_int32), ("clim", c_float * 2),
                ("alphamap", c_void_p), ("n_alpha", c_int32), ("alim", c_float * 2),
                ("coord", c_int32), ("reserved", c_int32)]


class VrClipPlane(ctypes.Structure):
    _fields_ = [("normal", c_float * 3), ("offset", c_float)]


class VrSlice(ctypes.Structure):
    _fields_ = [("origin", c_float * 3), ("du", c_float * 3), ("dv", c_float * 3), ("dw", c_float * 3),
                ("resolution", c_uint64 * 2), ("samples", c_int32), ("mode", c_int32), ("source", c_int32),
                ("reserved", c_int32)]


class VrHistogram(ctypes.Structure):
    _fields_ = [("source", c_int32), ("nbins", c_int32), ("lim", c_float * 2), ("label_first", c_int32),
                ("label_count", c_int32), ("use_clip", c_int32), ("reserved", c_int32)]


class VrHistRow(ctypes.Structure):
    _fields_ = [("total", c_uint64), ("below", c_uint64), ("above", c_uint64), ("nan", c_uint64),
                ("ninf", c_uint64), ("min", c_float), ("max", c_float), ("sum", ctypes.c_double)]


class VrChannel(ctypes.Structure):
    _fields_ = [("handle", c_void_p), ("time_last_mem_sync", c_uint64),
                ("emission", POINTER(VrVolume)), ("reflection", POINTER(VrVolume)),
                ("absorption", POINTER(VrVolume)), ("dx", POINTER(VrVolume)), ("dy", POINTER(VrVolume)),
                ("dz", POINTER(VrVolume)), ("args", POINTER(VrRenderArgs))]


class VrError(RuntimeError):
    """A non-zero status from libvrhip; ``code`` is the vr_status value."""

    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


_lib = None

# measurement entries that tools/ bind and include/vrhip.h does not declare (csrc/vr_capi.hip)
TOOL_SIGNATURES = [
    ("vr_smooth_axis_device", c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p]),
    ("vr_smooth_fused_device", c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    ("vr_deconv_axis_device", c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_float,
                                      c_uint32, c_void_p, c_void_p]),
    ("vr_debug_emission_version", c_int, [c_void_p, POINTER(c_uint64)]),
    ("vr_deconv_pointwise_device", c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_float, c_uint32, c_void_p]),
    ("vr_debug_read_emission", c_int, [c_void_p, c_uint64, c_uint64, c_void_p]),
    ("vr_debug_derive_times", c_int, [c_void_p, c_void_p]),
]

# (name, restype, argtypes) for every symbol of include/vrhip.h
SIGNATURES = [
    ("vr_new", c_int, [POINTER(c_void_p)]),
    ("vr_new_multi", c_int, [POINTER(c_int32), c_int32, POINTER(c_void_p)]),
    ("vr_delete", c_int, [c_void_p]),
    ("vr_mem_info", c_int, [c_void_p, c_char_p, c_size_t]),
    ("vr_sync_volumes", c_int, [c_void_p, c_uint64, POINTER(VrVolume), POINTER(VrVolume), POINTER(VrVolume),
                                POINTER(VrVolume), POINTER(VrVolume), POINTER(VrVolume)]),
    ("vr_render", c_int, [c_void_p, POINTER(VrRenderArgs), c_void_p]),
    ("vr_render_stereo", c_int, [c_void_p, POINTER(VrRenderArgs), c_float, c_void_p, c_void_p]),
    ("vr_render_channels", c_int, [POINTER(VrChannel), c_int32, c_int32, c_float, c_void_p]),
    ("vr_render_channels_device", c_int, [POINTER(VrChannel), c_int32, c_int32, c_float, c_void_p, c_void_p]),
    ("vr_sum_channels_device", c_int, [c_void_p, c_int32, c_int32, c_uint64, c_void_p, c_void_p]),
    ("vr_henyey_greenstein", c_int, [c_uint32, c_float, c_void_p]),
    ("vr_timestamp", c_uint64, []),
    ("vr_dtype_size", c_size_t, [c_int32]),
    ("vr_convert_host", c_int, [c_void_p, c_int32, c_uint64, c_void_p]),
    ("vr_render_device", c_int, [c_void_p, POINTER(VrRenderArgs), POINTER(VrPartition), c_void_p, c_void_p,
                                 c_void_p]),
    ("vr_render_stereo_device", c_int, [c_void_p, POINTER(VrRenderArgs), c_float, c_void_p, c_void_p, c_void_p,
                                        c_void_p]),
    ("vr_render_projection", c_int, [c_void_p, POINTER(VrRenderArgs), c_int32, c_void_p, c_void_p]),
    ("vr_render_projection_device", c_int, [c_void_p, POINTER(VrRenderArgs), c_int32, POINTER(VrPartition), c_void_p,
                                            c_void_p, c_void_p, c_void_p]),
    ("vr_render_isosurface", c_int, [c_void_p, POINTER(VrRenderArgs), c_float, c_void_p, c_void_p, c_void_p]),
    ("vr_render_isosurface_device", c_int, [c_void_p, POINTER(VrRenderArgs), c_float, POINTER(VrPartition), c_void_p,
                                            c_void_p, c_void_p, c_void_p, c_void_p]),
    ("vr_render_transfer", c_int, [c_void_p, POINTER(VrRenderArgs), POINTER(VrTransfer), c_void_p, c_void_p]),
    ("vr_render_transfer_device", c_int, [c_void_p, POINTER(VrRenderArgs), POINTER(VrTransfer), POINTER(VrPartition),
                                          c_void_p, c_void_p, c_void_p, c_void_p]),
    ("vr_transfer_lookup_host", c_int, [c_void_p, c_int32, c_int32, POINTER(c_float), c_void_p, c_uint64, c_void_p]),
    ("vr_set_clip", c_int, [c_void_p, POINTER(VrClipPlane), c_int32]),
    ("vr_get_clip", c_int, [c_void_p, POINTER(VrClipPlane), POINTER(c_int32)]),
    ("vr_clip_convert_host", c_int, [POINTER(VrClipPlane), c_int32, POINTER(c_float), POINTER(c_float), c_void_p]),
    ("vr_sync_labels", c_int, [c_void_p, POINTER(VrVolume)]),
    ("vr_set_label_gains", c_int, [c_void_p, c_void_p, c_int32]),
    ("vr_get_label_gains", c_int, [c_void_p, c_void_p, POINTER(c_int32)]),
    ("vr_label_gain_host", c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_uint64, c_void_p]),
    ("vr_set_smoothing", c_int, [c_void_p, c_void_p]),
    ("vr_get_smoothing", c_int, [c_void_p, c_void_p]),
    ("vr_smooth_weights_host", c_int, [c_float, POINTER(c_int32), c_void_p]),
    ("vr_smooth_host", c_int, [c_void_p, c_void_p, c_void_p, c_void_p]),
    ("vr_set_deconvolution", c_int, [c_void_p, c_void_p, c_int32, c_float]),
    ("vr_get_deconvolution", c_int, [c_void_p, c_void_p, POINTER(c_int32), POINTER(c_float)]),
    ("vr_deconvolve_host", c_int, [c_void_p, c_void_p, c_void_p, c_int32, c_float, c_void_p]),
    ("vr_render_slice", c_int, [c_void_p, POINTER(VrSlice), c_void_p, c_void_p, c_void_p]),
    ("vr_render_slice_device", c_int, [c_void_p, POINTER(VrSlice), c_void_p, c_void_p, c_void_p, c_void_p]),
    ("vr_slice_axis", c_int, [POINTER(c_uint64), c_int32, ctypes.c_double, c_uint64, POINTER(VrSlice)]),
    ("vr_slice_oblique", c_int, [POINTER(c_uint64), POINTER(c_float), POINTER(ctypes.c_double),
                                 POINTER(ctypes.c_double), POINTER(ctypes.c_double), ctypes.c_double, c_uint64,
                                 c_uint64, c_uint64, POINTER(VrSlice)]),
    ("vr_volume_histogram", c_int, [c_void_p, POINTER(VrHistogram), c_void_p, c_void_p]),
    ("vr_volume_histogram_device", c_int, [c_void_p, POINTER(VrHistogram), c_void_p, c_void_p, c_void_p]),
    ("vr_histogram_bin_host", c_int, [c_void_p, c_uint64, c_int32, POINTER(c_float), c_void_p]),
    ("vr_partition_columns", c_int64, [c_int64, POINTER(VrPartition)]),
    ("vr_assemble_partitions", c_int, [c_void_p, c_int64, c_int64, c_int32, c_int32, c_int64, c_void_p,
                                       c_void_p]),
    ("vr_depth_lanes", c_int, [c_int64, c_int64]),
    ("vr_depth_lanes_tau", c_int, [c_int64, c_int64, ctypes.c_double]),
    ("vr_render_slab", c_int, [c_void_p, POINTER(VrRenderArgs), POINTER(VrSlab), POINTER(VrPartition), c_void_p,
                                c_void_p, c_void_p]),
    ("vr_slab_planes", c_int, [POINTER(c_uint64), POINTER(c_float), ctypes.c_double, ctypes.c_double,
                               POINTER(c_uint64), POINTER(c_uint64)]),
    ("vr_synth_shell_device", c_int, [c_void_p, c_uint64, c_void_p]),
    ("vr_synth_shell_planes_device", c_int, [c_void_p, c_uint64, c_uint64, c_uint64, c_void_p]),
    ("vr_gradient_device", c_int, [c_void_p, POINTER(c_uint64), c_void_p, c_void_p, c_void_p, c_void_p]),
    ("vr_henyey_greenstein_device", c_int, [c_uint32, c_float, c_void_p, c_void_p]),
    ("vr_normalize_device", c_int, [c_void_p, c_uint64, ctypes.c_double, ctypes.c_double, c_void_p, c_void_p]),
    ("vr_resize_device", c_int, [c_void_p, POINTER(c_uint64), POINTER(c_uint64), c_void_p, c_void_p]),
    ("vr_resize_contributions", c_int, [c_uint64, c_uint64, POINTER(c_int32), c_void_p, c_void_p]),
    ("vr_debug_slot_transition", c_int, [POINTER(c_int32), c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                                         POINTER(c_int32), POINTER(c_int32)]),
    ("vr_last_error", c_char_p, []),
    ("vr_hip_errors", c_int64, [c_char_p, c_size_t]),
    ("vr_last_march_kernel", c_int, [c_char_p, c_size_t]),
    ("vr_last_launch_flags", c_int, [POINTER(c_uint32)]),
    ("vr_set_option", c_int, [c_char_p, c_int64]),
    ("vr_version", c_char_p, []),
]


def lib():
    """Load libvrhip.so once; raise (never fall back) if it is absent."""
    global _lib
    if _lib is None:
        # One HIP runtime per process: when PyTorch-ROCm is installed it carries its own
        # libamdhip64.so.7 / libhsa-runtime64.so.1; loading it first makes libvrhip bind to the
        # same copy (same SONAMEs), so torch tensors and libvrhip buffers share one device context.
        try:
            import torch  # noqa: F401
        except Exception:
            pass
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"libvrhip.so not built at {LIB_PATH}: run __graft_entry__.build() "
                              "(make -C volume_renderer_amd/csrc)")
        handle = ctypes.CDLL(LIB_PATH)
        for name, res, args in SIGNATURES + TOOL_SIGNATURES:
            if LIB_PATH != _DEFAULT_PATH and not hasattr(handle, name):
                continue  # an A/B build of an earlier tree (VR_LIB_PATH) may predate a diagnostic entry
            fn = getattr(handle, name)
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc: int) -> None:
    if rc != VR_OK:
        msg = lib().vr_last_error().decode(errors="replace")
        raise VrError(rc, msg)


def hip_errors() -> tuple[int, list[str]]:
    """HIP errors the library handled or found pending at an API entry (vr_hip_errors): the count
    since load and the last log lines, newest last."""
    buf = ctypes.create_string_buffer(32 * 400)
    n = lib().vr_hip_errors(buf, len(buf))
    return int(n), [l for l in buf.value.decode(errors="replace").splitlines() if l]
