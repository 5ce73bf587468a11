"""The 'set_smoothing' command at the MATLAB boundary: its count and type checks through the C++ MEX
adaptor (mex/volumeRender_mex.cpp against tests/mexstub/) and the Python `volumeRender`, which need no
device; and on the GPU, a sigma set through the adaptor -- scalar, 3-vector, [] and false -- renders exactly
as through the ctypes path and as the host-filtered volume, and the Smoothing property of the Python
VolumeRender mirror sends it before a render whenever it changed."""
import numpy as np
import pytest

import mexsim as M
import oracle as O

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import mex  # noqa: E402

F = np.float32
R = np.flip(O.rotation(125, 25, 0), 0).astype(F)
ARGV = [False, False, F([1.5, 0.4, 0.6]), F([1, 1, 1]), np.uint64([40, 52]), R, F([0, 3, 6]), F(0.9), F([1, 1, 0])]
BAD = "set_smoothing: sigma must be a single or double scalar or 3-vector, \\[\\] or false"


def _stamped(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- without a device ---------------------------------------------------------------------------------------

def test_argument_and_output_counts():
    h = np.uint64(1)
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 0, "set_smoothing", h)
    with pytest.raises(M.MexError, match="set_smoothing: too many input arguments"):
        M.call("volumeRender", 0, "set_smoothing", h, F(1), F(1))
    with pytest.raises(M.MexError, match="Too many output arguments."):
        M.call("volumeRender", 1, "set_smoothing", h, F(1))
    with pytest.raises(M.MexError, match="Second input should be a class instance handle."):
        M.call("volumeRender", 0, "set_smoothing")
    with pytest.raises(vr.VrError, match="insufficient parameter!"):
        vr.volumeRender("set_smoothing", h)
    with pytest.raises(vr.VrError, match="set_smoothing: too many input arguments"):
        vr.volumeRender("set_smoothing", h, F(1), F(1))


def test_type_checks_and_the_librarys_own_errors():
    h = np.uint64(1)
    for sg in (np.int32([1, 1, 1]), np.uint8(2), np.ones(2, F), np.ones(4, F), np.ones((3, 3), F), np.ones((1, 3, 1), F),
               np.zeros((0, 0), np.uint8), np.zeros((0, 0), np.int32), True, "one", ""):
        with pytest.raises(M.MexError, match=BAD):
            M.call("volumeRender", 0, "set_smoothing", h, sg)
        if not isinstance(sg, str):  # (one rule on both sides; a Python str is no array at all)
            with pytest.raises(vr.VrError, match=BAD):
                vr.volumeRender("set_smoothing", h, sg)
    # accepted forms reach the library: its sigma checks come before the handle, then the handle is refused
    for sg in (F(1.5), np.float64(1.5), F([1, 2, 0.5]), np.float64([[1], [2], [0.5]]), np.zeros((0, 0)), False):
        with pytest.raises(M.MexError, match="Handle not valid."):
            M.call("volumeRender", 0, "set_smoothing", h, sg)
        with pytest.raises(vr.VrError, match="Handle not valid."):
            vr.volumeRender("set_smoothing", h, sg)
    for sg, text in ((F(-1), "finite and not negative"), (F([1, np.nan, 1]), "finite and not negative"),
                     (np.float64(np.inf), "finite and not negative"), (F([0, 0, 6.5]), "at most 6 voxels")):
        with pytest.raises(M.MexError, match="smoothing: .*" + text):
            M.call("volumeRender", 0, "set_smoothing", h, sg)
        with pytest.raises(vr.VrError, match="smoothing: .*" + text) as e:
            vr.volumeRender("set_smoothing", h, sg)
        assert e.value.code == 1


def test_the_property_validates_its_value():
    r = vr.VolumeRender.__new__(vr.VolumeRender)  # (no handle: the property check alone)
    for bad in (np.ones(2), np.ones((3, 3)), True, "one"):
        with pytest.raises(TypeError, match="Smoothing"):
            r.Smoothing = bad
    for val, want in ((1.5, [1.5] * 3), ([1, 2, 0], [1, 2, 0]), (None, [0] * 3), (False, [0] * 3), ([], [0] * 3),
                      (np.float64([[1], [2], [3]]), [1, 2, 3])):
        r.Smoothing = val
        assert r.Smoothing.dtype == np.float32 and np.array_equal(r.Smoothing, F(want))
    object.__setattr__(r, "objectHandle", None)


# ---- on the GPU ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_sigma_through_mexfunction_equals_the_python_path_and_the_host_filter():
    data = O.shell_volume(24)
    em, re = _stamped(data, 11), _stamped(np.float32(1.0), 12)
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    (plain,) = M.call("volumeRender", 1, "render", h, *ARGV)
    got = {}
    for name, sg, want in (("single scalar", F(1.5), [1.5] * 3), ("double scalar", np.float64(0.75), [0.75] * 3),
                           ("single row", F([[1, 2, 0.5]]), [1, 2, 0.5]), ("double column", np.float64([[1], [2], [0.5]]), [1, 2, 0.5])):
        assert M.call("volumeRender", 0, "set_smoothing", h, sg) == []
        assert _same(mex.get_smoothing(h), F(want)), name  # (one library: the ctypes path reads the same handle)
        (got[name],) = M.call("volumeRender", 1, "render", h, *ARGV)
    for clear in (np.zeros((0, 0)), False, F(0), np.zeros(3)):
        M.call("volumeRender", 0, "set_smoothing", h, F(2))
        M.call("volumeRender", 0, "set_smoothing", h, clear)
        assert not mex.get_smoothing(h).any()
        (again,) = M.call("volumeRender", 1, "render", h, *ARGV)
        assert _same(again, plain), clear
    M.call("volumeRender", 0, "delete", h)

    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    vr.volumeRender("set_smoothing", hp, F([1, 2, 0.5]))
    want = vr.volumeRender("render", hp, *ARGV)
    vr.volumeRender("delete", hp)
    ref = {}
    for name, sg in (("single scalar", 1.5), ("double scalar", 0.75), ("single row", [1, 2, 0.5])):
        hr = vr.volumeRender("new")
        e2 = _stamped(mex.smooth_host(data, sg), 11)
        vr.volumeRender("sync_volumes", hr, np.uint64(0), e2, re, e2)
        ref[name] = vr.volumeRender("render", hr, *ARGV)
        vr.volumeRender("delete", hr)
    assert _same(got["single row"], want) and _same(got["double column"], want)
    for name in ref:
        assert _same(got[name], ref[name]), name
    assert not _same(got["single row"], plain) and not _same(got["single scalar"], got["double scalar"])


def _renderer(data):
    r = vr.VolumeRender()
    r.FocalLength, r.DistanceToObject = 3.0, 6
    r.rotate(125, 25, 0)
    r.ImageResolution = [52, 40]
    v = vr.Volume(data)
    r.VolumeEmission = v
    r.VolumeAbsorption = v
    r.VolumeReflection = vr.Volume(1)  # (its own, stamped by this test's clock: tests/test_mex_labels.py)
    r.FactorEmission = 1.5
    r.Color = [1, 1, 0]
    return r


@pytest.mark.gpu
def test_the_smoothing_property_is_sent_before_a_render_when_it_changed(counter_clock):
    data = O.shell_volume(24)
    r = _renderer(data)
    assert not r.Smoothing.any()
    plain = r.render()
    frames, sums = [], []
    sigmas = (1.0, [2, 0.5, 1], [0, 0, 1.5])
    for sg in sigmas:
        r.Smoothing = sg
        frames.append(r.render())
        assert _same(mex.get_smoothing(r.objectHandle), r.Smoothing)
        sums.append(r.renderProjection("sum"))
    r.Smoothing = 1.0
    section = r.renderSlice(2, 12)  # a slice shows what is rendered
    r.Smoothing = False
    back = r.render()
    assert not mex.get_smoothing(r.objectHandle).any()
    r.delete()
    for sg, frame, s in zip(sigmas, frames, sums):
        r2 = _renderer(mex.smooth_host(data, sg))
        want, wsum = r2.render(), r2.renderProjection("sum")
        if sg == 1.0:
            wsec = r2.renderSlice(2, 12)
        r2.delete()
        assert _same(frame, want) and _same(s, wsum), f"sigma {sg}"
    assert _same(section, wsec) and _same(back, plain)
    assert not _same(frames[0], plain) and not _same(frames[1], frames[0])
