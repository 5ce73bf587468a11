"""Label gains without a device: the value rule of the label pass on the CPU (vr_label_gain_host, the
inline function the kernel evaluates, csrc/vr_labels.h) against the numpy float32 product bit for bit,
the argument checks that arrive before the handle, and the count and type checks of the 'sync_labels'
and 'set_label_gains' commands of the C++ MEX adaptor (mex/volumeRender_mex.cpp against tests/mexstub/)
and of the Python `volumeRender`."""
import ctypes

import numpy as np
import pytest

import mexsim as M

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402

F = np.float32
SPECIAL = F([0.0, -0.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 1.0, -1.0])


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def numpy_product(src, labels, gains):
    """em2 of the issue: (src * table[labels]).astype(float32), table padded with ones to 256."""
    table = np.ones(256, F)
    table[:len(gains)] = F(gains)
    with np.errstate(all="ignore"):
        return (src * table[labels]).astype(F)


def sample(seed, n):
    rng = np.random.default_rng(seed)
    src = (rng.standard_normal(n) * F(10) ** rng.integers(-20, 20, n)).astype(F)
    src[:SPECIAL.size * 8] = np.repeat(SPECIAL, 8)
    rng.shuffle(src)
    return src, rng.integers(0, 256, n).astype(np.uint8)


@pytest.mark.parametrize("gains", [F([1, 0.35, 0]), F([-2.5, 0.0, -0.0, 1e-30, 3e38, 1.0, 0.1]),
                                   np.linspace(-3, 3, 256).astype(F), F([0.5])])
def test_label_gain_host_is_the_numpy_product_bit_for_bit(gains):
    src, labels = sample(20260101 + gains.size, 5000)
    labels[::3] = (labels[::3].astype(np.int32) % gains.size).astype(np.uint8)  # (a third of the voxels inside the table, whatever its length)
    sp = np.flatnonzero(np.isinf(src))[:8]  # and eight inf voxels walk through the table's first entries
    labels[sp] = (np.arange(sp.size) % gains.size).astype(np.uint8)
    got = mex.label_gain_host(src, labels, gains)
    want = numpy_product(src, labels, gains)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and nan.any()
    assert np.array_equal(bits(got)[~nan], bits(want)[~nan])
    outside = labels >= gains.size  # labels at or above n: copied, not multiplied -- NaN payloads included
    assert np.array_equal(bits(got)[outside], bits(src)[outside]) and (outside.any() or gains.size == 256)
    # +-0 keep IEEE's sign rule and inf * 0 is NaN (both are in the sample with a zero gain)
    if (gains == 0).any():
        zero = (~outside) & (F(gains)[np.minimum(labels, gains.size - 1)] == 0)
        assert np.isnan(got[zero & np.isinf(src)]).all() and (zero & np.isinf(src)).any()
    assert (np.abs(src[np.isfinite(src)]) < 1.2e-38).any()  # (subnormals are in the sample)


def test_label_gain_host_with_no_gains_copies_and_keeps_the_shape():
    src, labels = sample(7, 600)
    src3 = np.asfortranarray(src.reshape(10, 12, 5))
    got = mex.label_gain_host(src3, labels.reshape(10, 12, 5), None)
    assert got.shape == (10, 12, 5) and np.array_equal(bits(got), bits(src3))
    L = _lib.lib()
    out = np.zeros(4, F)
    assert L.vr_label_gain_host(src.ctypes.data, None, None, 0, 4, out.ctypes.data) == 0  # n = 0 needs no labels
    assert np.array_equal(bits(out), bits(src[:4]))
    assert L.vr_label_gain_host(None, None, None, 0, 0, None) == 0


def test_argument_checks_arrive_before_the_handle():
    L = _lib.lib()
    bad = ctypes.c_void_p(12345)  # not a handle: a check that comes first answers VR_ERR_ARGUMENT, not VR_ERR_HANDLE
    g = np.ones(300, F)
    for n in (-1, 257):
        assert L.vr_set_label_gains(bad, g.ctypes.data, n) == 1 and b"label gains" in L.vr_last_error()
    assert L.vr_set_label_gains(bad, None, 3) == 1 and b"NULL" in L.vr_last_error()
    for v in (np.nan, np.inf, -np.inf):
        g2 = F([1, v, 1])
        assert L.vr_set_label_gains(bad, g2.ctypes.data, 3) == 1 and b"finite" in L.vr_last_error()
        assert L.vr_set_label_gains(bad, g2.ctypes.data, 1) == 2  # (only the first n are read)
    assert L.vr_set_label_gains(bad, F([-1.5]).ctypes.data, 1) == 2  # a negative gain is allowed
    assert L.vr_set_label_gains(bad, None, 0) == 2 and b"Handle not valid" in L.vr_last_error()
    assert L.vr_set_label_gains(bad, g.ctypes.data, 256) == 2
    n = ctypes.c_int32(0)
    assert L.vr_get_label_gains(bad, None, ctypes.byref(n)) == 1
    assert L.vr_get_label_gains(bad, g.ctypes.data, None) == 1
    assert L.vr_get_label_gains(bad, g.ctypes.data, ctypes.byref(n)) == 2
    # the host function applies the same checks
    src, lab = np.ones(4, F), np.zeros(4, np.uint8)
    assert L.vr_label_gain_host(src.ctypes.data, lab.ctypes.data, g.ctypes.data, 257, 4, src.ctypes.data) == 1
    assert L.vr_label_gain_host(src.ctypes.data, lab.ctypes.data, F([np.nan]).ctypes.data, 1, 4, src.ctypes.data) == 1
    assert L.vr_label_gain_host(src.ctypes.data, None, g.ctypes.data, 1, 4, src.ctypes.data) == 1
    assert L.vr_label_gain_host(None, lab.ctypes.data, g.ctypes.data, 1, 4, src.ctypes.data) == 1
    # labels: the element type is checked before the handle too
    v = _lib.VrVolume()
    data = np.zeros(8, np.uint16)
    v.data, v.location = data.ctypes.data, _lib.VR_HOST
    v.dims[0], v.dims[1], v.dims[2] = 2, 2, 2
    for dt in (_lib.VR_F32, _lib.VR_U16, _lib.VR_I16, _lib.VR_F16, _lib.VR_U8 | _lib.VR_DTYPE_UNORM, 77):
        v.dtype = dt
        assert L.vr_sync_labels(bad, ctypes.byref(v)) == 1 and b"labels" in L.vr_last_error()
    v.dtype = _lib.VR_U8
    assert L.vr_sync_labels(bad, ctypes.byref(v)) == 2
    v.data = None
    assert L.vr_sync_labels(bad, ctypes.byref(v)) == 1 and b"labels" in L.vr_last_error()
    assert L.vr_sync_labels(bad, None) == 2


def test_mex_commands_argument_and_output_counts():
    h = np.uint64(1)
    lab, gains = np.zeros((3, 2, 2), np.uint8), F([1, 0.5])
    for cmd, arg in (("sync_labels", lab), ("set_label_gains", gains)):
        with pytest.raises(M.MexError, match="insufficient parameter!"):
            M.call("volumeRender", 0, cmd, h)
        with pytest.raises(M.MexError, match="too many input arguments"):
            M.call("volumeRender", 0, cmd, h, arg, arg)
        with pytest.raises(M.MexError, match="Too many output arguments."):
            M.call("volumeRender", 1, cmd, h, arg)
        with pytest.raises(M.MexError, match="Second input should be a class instance handle."):
            M.call("volumeRender", 0, cmd)
        # the Python `volumeRender` keeps the input counts
        with pytest.raises(vr.VrError, match="insufficient parameter!"):
            vr.volumeRender(cmd, h)
        with pytest.raises(vr.VrError, match="too many input arguments"):
            vr.volumeRender(cmd, h, arg, arg)


def test_mex_commands_type_checks_and_handle():
    h = np.uint64(1)
    bad = "labels must be a uint8 array"
    for lab in (np.zeros((3, 2, 2), F), np.zeros((3, 2, 2), np.uint16), np.zeros((3, 2, 2), np.int8), True, "none"):
        with pytest.raises(M.MexError, match=bad):
            M.call("volumeRender", 0, "sync_labels", h, lab)
    with pytest.raises(M.MexError, match=bad):
        M.call("volumeRender", 0, "sync_labels", h, np.zeros((2, 2, 2, 2), np.uint8))
    with pytest.raises(M.MexError, match="labels: the label volume must be uint8"):  # a Volume is single: the library's
        M.call("volumeRender", 0, "sync_labels", h, vr.Volume(np.zeros((2, 2, 2), F)))
    for lab in (np.zeros((3, 2, 2), np.uint8), np.zeros((5, 4), np.uint8), np.zeros((0, 0), np.uint8),
                np.zeros((0, 0), np.float64), False):
        with pytest.raises(M.MexError, match="Handle not valid."):
            M.call("volumeRender", 0, "sync_labels", h, lab)
    bad = "gains must be a single vector of at most 256 entries"
    for g in (np.float64([1, 0.5]), np.ones((2, 2), F), np.ones((1, 2, 2), F), np.ones(257, F), np.uint8([1, 0]), True,
              "none"):
        with pytest.raises(M.MexError, match=bad):
            M.call("volumeRender", 0, "set_label_gains", h, g)
    with pytest.raises(M.MexError, match="every gain must be finite"):  # the library's own check, before the handle
        M.call("volumeRender", 0, "set_label_gains", h, F([1, np.nan]))
    for g in (F([1, 0.5]), F([[1], [0.5], [-2]]), np.ones(256, F), np.zeros((0, 0), F), np.zeros((0, 0), np.float64),
              False):
        with pytest.raises(M.MexError, match="Handle not valid."):
            M.call("volumeRender", 0, "set_label_gains", h, g)
    # the Python `volumeRender` applies the same type checks
    for lab in (np.zeros((3, 2, 2), F), True):
        with pytest.raises(vr.VrError, match="labels must be a uint8 array"):
            vr.volumeRender("sync_labels", h, lab)
    for g in (np.float64([1, 0.5]), np.ones((2, 2), F), np.ones(257, F)):
        with pytest.raises(vr.VrError, match=bad):
            vr.volumeRender("set_label_gains", h, g)
    for cmd, arg in (("sync_labels", np.zeros((3, 2, 2), np.uint8)), ("sync_labels", False), ("set_label_gains", F([1])),
                     ("set_label_gains", []), ("set_label_gains", False)):
        with pytest.raises(vr.VrError, match="Handle not valid."):
            vr.volumeRender(cmd, h, arg)


def test_mirror_properties_validate():
    """VolumeLabels / LabelGains of the Python VolumeRender are checked on assignment; the class itself
    needs a device (its constructor makes a handle), so only the setter's rules are exercised here."""
    from volume_renderer_amd.volume_render import VolumeRender
    r = object.__new__(VolumeRender)
    r.VolumeLabels = np.zeros((2, 3, 4), np.uint8)
    assert r.VolumeLabels.flags.f_contiguous and r._labels_applied == "assigned"
    r.LabelGains = [1, 0.5, 0]
    assert r.LabelGains.dtype == np.float32 and r.LabelGains.shape == (3,)
    r.LabelGains = None
    assert r.LabelGains.size == 0
    for bad in (np.zeros((2, 3), F), True, np.zeros((2, 2, 2, 2), np.uint8)):
        with pytest.raises(TypeError, match="VolumeLabels"):
            r.VolumeLabels = bad
    for bad in (np.ones((2, 2)), np.ones(257)):
        with pytest.raises(TypeError, match="LabelGains"):
            r.LabelGains = bad
    object.__setattr__(r, "objectHandle", None)  # (nothing to delete)
