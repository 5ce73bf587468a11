"""The 'set_deconvolution' command at the MATLAB boundary: its count and type checks through the C++ MEX
adaptor (mex/volumeRender_mex.cpp against tests/mexstub/) and the Python `volumeRender`, which need no
device; and on the GPU, a setting sent through the adaptor -- scalar or 3-vector sigma, with and without a
floor, cleared by [], false and 0 iterations -- renders exactly as through the ctypes path and as the
host-deconvolved volume, and the Deconvolution property of the Python VolumeRender mirror sends it before a
render whenever it changed."""
import numpy as np
import pytest

import mexsim as M
import oracle as O

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import mex  # noqa: E402
from test_mex_smoothing import ARGV, _renderer, _same, _stamped  # noqa: E402

F = np.float32
BAD = "set_deconvolution: sigma must be a single or double scalar or 3-vector, \\[\\] or false"
BAD_N = "set_deconvolution: iterations must be an integer scalar in 0..64"
BAD_FLOOR = "set_deconvolution: floor must be a real scalar greater than 0"


def both(match, *args, nlhs=0):
    """The command through mexFunction and through the Python volumeRender: one rule, one message."""
    with pytest.raises(M.MexError, match=match):
        M.call("volumeRender", nlhs, "set_deconvolution", *args)
    with pytest.raises(vr.VrError, match=match):
        vr.volumeRender("set_deconvolution", *args)


# ---- without a device ---------------------------------------------------------------------------------------

def test_argument_and_output_counts():
    h = np.uint64(1)
    both("insufficient parameter!", h)
    both("set_deconvolution: too many input arguments", h, F(1), F(2), F(1e-6), F(1))
    both("set_deconvolution: iterations is missing", h, F(1))
    with pytest.raises(M.MexError, match="Too many output arguments."):
        M.call("volumeRender", 1, "set_deconvolution", h, F(1), F(2))
    with pytest.raises(M.MexError, match="Second input should be a class instance handle."):
        M.call("volumeRender", 0, "set_deconvolution")


def test_type_checks_and_the_librarys_own_errors():
    h = np.uint64(1)
    for sg in (np.int32([1, 1, 1]), np.uint8(2), np.ones(2, F), np.ones(4, F), np.ones((3, 3), F), np.ones((1, 3, 1), F), True):
        both(BAD, h, sg, F(2))
    for n in (F(1.5), np.float64(-1), np.float64(65), F(np.nan), True, np.ones(2), np.int32(-3), np.uint8(70)):
        both(BAD_N, h, F(1), n)
    for fl in (np.int32(1), np.ones(2, F), True):
        both(BAD_FLOOR, h, F(1), F(2), fl)
    # accepted forms reach the library: its checks come before the handle, then the handle is refused
    for args in ((F(1.5), F(2)), (np.float64(1.5), np.float64(10)), (F([1, 2, 0.5]), np.int32(3)),
                 (np.float64([[1], [2], [0.5]]), np.uint8(64), F(1e-4)), (F(1), np.float64(1), np.float64(1e-3)),
                 (np.zeros((0, 0)),), (False,), (False, F(3)), (F(2), F(0)), (np.zeros((0, 0)), F(2), F(1e-3))):
        both("Handle not valid.", h, *args)
    for args, text in (((F(-1), F(2)), "finite and not negative"), ((F([1, np.nan, 1]), F(2)), "finite and not negative"),
                       ((np.float64(np.inf), F(2)), "finite and not negative"), ((F([0, 0, 6.5]), F(2)), "at most 6 voxels"),
                       ((F(1), F(2), F(0)), "floor must be finite and greater than 0"),
                       ((F(1), F(2), np.float64(-1e-6)), "floor must be finite and greater than 0"),
                       ((F(1), F(2), F(np.inf)), "floor must be finite and greater than 0"),
                       ((False, F(0), F(np.nan)), "floor must be finite and greater than 0")):
        both("deconvolution: .*" + text, h, *args)
        with pytest.raises(vr.VrError) as e:
            vr.volumeRender("set_deconvolution", h, *args)
        assert e.value.code == 1


def test_the_property_validates_its_value():
    r = vr.VolumeRender.__new__(vr.VolumeRender)  # (no handle: the property check alone)
    for bad in (1.5, np.ones(3), True, "one", (1.5,), (np.ones(2), 3), (np.ones((3, 3)), 3), (1.0, 2.5), (1.0, 65), (1.0, -1),
                (1.0, 2, 0.0), (1.0, 2, np.nan), (1.0, 2, 1e-6, 4)):
        with pytest.raises(TypeError, match="Deconvolution"):
            r.Deconvolution = bad
    for val in (None, False, [], (1.0, 0), (0.0, 5), ([0, 0, 0], 5, 1e-3)):
        r.Deconvolution = val
        assert r.Deconvolution is False
    for val, want in (((1.5, 3), ([1.5] * 3, 3, 1e-6)), (([1, 2, 0], 10, 1e-4), ([1, 2, 0], 10, 1e-4)),
                      ([np.float64([[1], [2], [3]]), np.int32(64)], ([1, 2, 3], 64, 1e-6))):
        r.Deconvolution = val
        sg, n, fl = r.Deconvolution
        assert sg.dtype == np.float32 and np.array_equal(sg, F(want[0])) and n == want[1] and type(n) is int
        assert fl.dtype == np.float32 and fl == F(want[2])
    object.__setattr__(r, "objectHandle", None)


# ---- on the GPU ---------------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_a_setting_through_mexfunction_equals_the_python_path_and_the_host_rule():
    data = O.shell_volume(24)
    em, re = _stamped(data, 11), _stamped(np.float32(1.0), 12)
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    (plain,) = M.call("volumeRender", 1, "render", h, *ARGV)
    cases = (("single scalar", (F(1.5), F(2)), ([1.5] * 3, 2, 1e-6)),
             ("double scalar, double count", (np.float64(0.75), np.float64(3)), ([0.75] * 3, 3, 1e-6)),
             ("single row, int count, floor", (F([[1, 2, 0.5]]), np.int32(2), F(1e-3)), ([1, 2, 0.5], 2, 1e-3)),
             ("double column, double floor", (np.float64([[1], [2], [0.5]]), np.uint8(2), np.float64(1e-3)), ([1, 2, 0.5], 2, 1e-3)))
    got = {}
    for name, args, want in cases:
        assert M.call("volumeRender", 0, "set_deconvolution", h, *args) == []
        sg, n, fl = mex.get_deconvolution(h)  # (one library: the ctypes path reads the same handle)
        assert _same(sg, F(want[0])) and n == want[1] and fl == F(want[2]), name
        (got[name],) = M.call("volumeRender", 1, "render", h, *ARGV)
    for clear in ((np.zeros((0, 0)),), (False,), (F(1.5), F(0)), (np.zeros(3), F(4)), (False, F(4), F(1e-3))):
        M.call("volumeRender", 0, "set_deconvolution", h, F(2), F(1))
        assert mex.get_deconvolution(h)[1] == 1
        M.call("volumeRender", 0, "set_deconvolution", h, *clear)
        sg, n, fl = mex.get_deconvolution(h)
        assert not sg.any() and n == 0 and fl == 0
        (again,) = M.call("volumeRender", 1, "render", h, *ARGV)
        assert _same(again, plain), clear
    M.call("volumeRender", 0, "delete", h)

    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    vr.volumeRender("set_deconvolution", hp, F([1, 2, 0.5]), 2, np.float64(1e-3))
    want = vr.volumeRender("render", hp, *ARGV)
    vr.volumeRender("set_deconvolution", hp, F(1.5), F(2))  # the default floor on the Python side
    assert mex.get_deconvolution(hp)[2] == F(1e-6)
    want_default = vr.volumeRender("render", hp, *ARGV)
    vr.volumeRender("delete", hp)
    ref = {}
    for name, _, (sg, n, fl) in cases[:3]:
        hr = vr.volumeRender("new")
        e2 = _stamped(mex.deconvolve_host(data, sg, n, F(fl)), 11)
        vr.volumeRender("sync_volumes", hr, np.uint64(0), e2, re, e2)
        ref[name] = vr.volumeRender("render", hr, *ARGV)
        vr.volumeRender("delete", hr)
    assert _same(got[cases[2][0]], want) and _same(got[cases[3][0]], want) and _same(got["single scalar"], want_default)
    for name in ref:
        assert _same(got[name], ref[name]), name
    assert not _same(got["single scalar"], plain) and not _same(got["single scalar"], got[cases[1][0]])


@pytest.mark.gpu
def test_the_deconvolution_property_is_sent_before_a_render_when_it_changed(counter_clock):
    data = O.shell_volume(24)
    r = _renderer(data)
    assert r.Deconvolution is False
    plain = r.render()
    frames, sums = [], []
    settings = ((1.0, 2), ([2, 0.5, 1], 3, 1e-4), ([0, 0, 1.5], 1))
    for s in settings:
        r.Deconvolution = s
        frames.append(r.render())
        sg, n, fl = mex.get_deconvolution(r.objectHandle)
        assert _same(sg, r.Deconvolution[0]) and n == r.Deconvolution[1] and fl == r.Deconvolution[2]
        sums.append(r.renderProjection("sum"))
    r.Deconvolution = (1.0, 2)
    r.Smoothing = 0.75  # both: the smoothing applies to the deconvolved volume
    section = r.renderSlice(2, 12)  # a slice shows what is rendered
    r.Smoothing = False
    r.Deconvolution = False
    back = r.render()
    assert mex.get_deconvolution(r.objectHandle)[1] == 0
    r.delete()
    for s, frame, sm in zip(settings, frames, sums):
        r2 = _renderer(mex.deconvolve_host(data, *s))
        want, wsum = r2.render(), r2.renderProjection("sum")
        r2.delete()
        assert _same(frame, want) and _same(sm, wsum), f"setting {s}"
    r2 = _renderer(mex.smooth_host(mex.deconvolve_host(data, 1.0, 2), 0.75))
    wsec = r2.renderSlice(2, 12)
    r2.delete()
    assert _same(section, wsec) and _same(back, plain)
    assert not _same(frames[0], plain) and not _same(frames[1], frames[0])
