"""Typed volumes through the MATLAB boundary: mexFunction of mex/volumeRender_mex.cpp (built against
the stand-in of MATLAB's API, tests/mexstub/) given a Volume whose Data is uint8, and a
RawVolume-shaped object (mex/matlab/RawVolume.m: RawData uint16, Unorm true) -- both bit for bit the
Python binding's image of the same volumes; a double Data still raises the adaptor's error."""
import numpy as np
import pytest

import golden_cases as GC
import mexsim as M

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("volume_renderer_amd")

SC = GC.SCENES["hg2_compute_32"]


class TypedVolume(vr.Volume):
    """A Volume whose Data keeps the element type it is given (what MATLAB holds in a property that
    is not cast); mexsim hands Data to the adaptor with its numpy dtype as the MATLAB class."""

    def __init__(self, data, stamp):
        self._data = np.asfortranarray(data)
        self.TimeLastUpdate = np.uint64(stamp)

    @property
    def Data(self):
        return self._data


def _argv(lut, scale):
    f = SC["factors"]
    sc = dict(SC, res=[40, 48], factors=[f[0] * scale, f[1], f[2] * scale])
    lights = [vr.LightSource(l[:3], l[3:]) for l in GC.EX1_LIGHTS]
    return list(GC.render_argv(sc, lights, lut))


def _raw_object(L, rv):
    """A RawVolume as MATLAB hands it over: class 'RawVolume' with Data (the single placeholder),
    TimeLastUpdate, RawData and the logical Unorm."""
    o = L.stub_object(b"RawVolume", 1)
    L.stub_set_prop(o, 0, b"Data", M._numeric(L, rv.Data))
    L.stub_set_prop(o, 0, b"TimeLastUpdate", M._numeric(L, np.uint64(rv.TimeLastUpdate)))
    L.stub_set_prop(o, 0, b"RawData", M._numeric(L, rv.RawData))
    L.stub_set_prop(o, 0, b"Unorm", M._numeric(L, np.array(bool(rv.Unorm))))
    return o


def _call_with_objects(nlhs, *args):
    """mexsim.call, with arguments that already are mxArrays (ints from stub_object) passed through."""
    import ctypes
    L = M.lib("volumeRender")
    L.stub_clear_log()
    mx = [a if isinstance(a, int) and not isinstance(a, bool) else M.to_mx(L, a) for a in args]
    prhs = (ctypes.c_void_p * max(len(mx), 1))(*mx)
    plhs = (ctypes.c_void_p * max(nlhs, 1))()
    try:
        if L.stub_call(nlhs, plhs, len(mx), prhs):
            raise M.MexError(L.stub_last_error().decode())
        return [M.from_mx(L, plhs[i]) for i in range(nlhs)]
    finally:
        for p in mx:
            L.stub_free(p)
        for i in range(max(nlhs, 1)):
            if plhs[i]:
                L.stub_free(plhs[i])


@pytest.fixture(scope="module")
def lut():
    v = vr.Volume(vr.HenyeyGreenstein(SC["lut"]))
    v.TimeLastUpdate = np.uint64(GC.STAMP_LUT)
    return v


def _refl():
    v = vr.Volume(np.float32(1.0))
    v.TimeLastUpdate = np.uint64(GC.STAMP_RE)
    return v


def test_uint8_data_through_mexfunction(lut):
    rng = np.random.default_rng(31)
    d = np.asfortranarray(rng.integers(0, 256, (37, 21, 13)).astype(np.uint8))
    em, re = TypedVolume(d, 5), _refl()
    argv = _argv(lut, 1 / 255)
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    (img,) = M.call("volumeRender", 1, "render", h, *argv)
    M.call("volumeRender", 0, "delete", h)
    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    ref = vr.volumeRender("render", hp, *argv)
    twin = vr.Volume(d.astype(np.float32))
    twin.TimeLastUpdate = np.uint64(5)
    vr.volumeRender("sync_volumes", hp, np.uint64(0), twin, re, twin)
    ref32 = vr.volumeRender("render", hp, *argv)
    vr.volumeRender("delete", hp)
    assert ref.max() > 0 and img.shape == (40, 48, 3)
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(img.view(np.uint32), ref32.view(np.uint32))


def test_raw_volume_unorm_uint16_through_mexfunction(lut):
    rng = np.random.default_rng(32)
    d = np.asfortranarray(rng.integers(0, 65536, (37, 21, 13)).astype(np.uint16))
    rv = vr.RawVolume(d, True)
    rv.TimeLastUpdate = np.uint64(5)
    re = _refl()
    argv = _argv(lut, 1.0)
    L = M.lib("volumeRender")
    (h,) = M.call("volumeRender", 1, "new")
    _call_with_objects(0, "sync_volumes", h, np.uint64(0), _raw_object(L, rv), re, _raw_object(L, rv))
    (img,) = M.call("volumeRender", 1, "render", h, *argv)
    M.call("volumeRender", 0, "delete", h)
    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), rv, re, rv)
    ref = vr.volumeRender("render", hp, *argv)
    twin = vr.Volume(d.astype(np.float32) / np.float32(65535))
    twin.TimeLastUpdate = np.uint64(5)
    vr.volumeRender("sync_volumes", hp, np.uint64(0), twin, re, twin)
    ref32 = vr.volumeRender("render", hp, *argv)
    vr.volumeRender("delete", hp)
    assert ref.max() > 0
    assert np.array_equal(img.view(np.uint32), ref.view(np.uint32))
    assert np.array_equal(img.view(np.uint32), ref32.view(np.uint32))


def test_double_data_still_raises():
    em = TypedVolume(np.zeros((4, 4, 4), np.float64), 5)
    (h,) = M.call("volumeRender", 1, "new")
    try:
        with pytest.raises(M.MexError, match=r"Volume\.Data must be single\."):
            M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, _refl(), em)
        for dt in (np.int8, np.int32, np.uint64):
            with pytest.raises(M.MexError, match=r"Volume\.Data must be single\."):
                M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), TypedVolume(np.zeros((2, 2, 2), dt), 5),
                       _refl(), _refl())
    finally:
        M.call("volumeRender", 0, "delete", h)
