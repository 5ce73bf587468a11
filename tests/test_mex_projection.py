"""The 'render_projection' command at the MATLAB boundary: the C++ MEX adaptor (mex/volumeRender_mex.cpp
against tests/mexstub/) returns the bits of the ctypes path, its argument checks, and the Python
class method VolumeRender.renderProjection on top of the command."""
import numpy as np
import pytest

import mexsim as M
import oracle as O

vr = pytest.importorskip("volume_renderer_amd")

R = np.flip(O.rotation(125, 25, 0), 0).astype(np.float32)
ARGV = [False, False, np.float32([1.5, 0.4, 0.6]), np.float32([1, 1, 1]), np.uint64([40, 52]), R,
        np.float32([0, 3, 6]), np.float32(0.9), np.float32([1, 1, 0])]


def _stamped(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def test_render_projection_argument_count():
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 2, "render_projection", np.uint64(1), *ARGV)  # no mode
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 1, "render_projection", np.uint64(1), False, False)


def test_render_projection_too_many_outputs_and_bad_mode():
    with pytest.raises(M.MexError, match="Too many output arguments."):
        M.call("volumeRender", 3, "render_projection", np.uint64(1), *ARGV, "mip")
    with pytest.raises(M.MexError, match="mode must be 'mip' or 'sum'"):
        M.call("volumeRender", 2, "render_projection", np.uint64(1), *ARGV, "min")
    with pytest.raises(M.MexError, match="mode must be 'mip' or 'sum'"):
        M.call("volumeRender", 2, "render_projection", np.uint64(1), *ARGV, np.float64(0))
    with pytest.raises(M.MexError, match="Handle not valid."):
        M.call("volumeRender", 2, "render_projection", np.uint64(1), *ARGV, "sum")


@pytest.mark.gpu
def test_render_projection_through_mexfunction_equals_python_path():
    em = _stamped(O.shell_volume(24), 11)
    re = _stamped(np.float32(1.0), 12)
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    got = {m: M.call("volumeRender", 2, "render_projection", h, *ARGV, m) for m in ("mip", "sum")}
    (only,) = M.call("volumeRender", 1, "render_projection", h, *ARGV, "mip")
    M.call("volumeRender", 0, "delete", h)
    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    for m in ("mip", "sum"):
        img, aux = vr.volumeRender("render_projection", hp, *ARGV, m)
        assert got[m][0].dtype == np.float32 and got[m][0].shape == (40, 52, 3) and got[m][1].shape == (40, 52)
        assert np.array_equal(got[m][0].view(np.uint32), img.view(np.uint32))
        assert np.array_equal(got[m][1].view(np.uint32), aux.view(np.uint32))
        assert img.max() > 0
    assert np.array_equal(only.view(np.uint32), got["mip"][0].view(np.uint32))
    assert np.isnan(got["mip"][1]).any() and (got["sum"][1] == 0).any()  # misses
    vr.volumeRender("delete", hp)


@pytest.mark.gpu
def test_render_projection_method(counter_clock):
    r = vr.VolumeRender()
    r.FocalLength, r.DistanceToObject = 3.0, 6
    r.rotate(125, 25, 0)
    r.ImageResolution = [52, 40]
    v = vr.Volume(O.shell_volume(24))
    r.VolumeEmission = v
    r.VolumeAbsorption = v
    r.FactorEmission = 1.5
    r.Color = [1, 1, 0]
    img, depth = r.renderProjection("mip", aux=True)
    assert img.shape == (40, 52, 3) and depth.shape == (40, 52)
    argv = r._render_argv(np.float32(0), np.flip(r.ImageResolution))
    want, want_aux = vr.volumeRender("render_projection", r.objectHandle, *argv, "mip")
    assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(depth.view(np.uint32), want_aux.view(np.uint32))
    only = r.renderProjection("sum")
    assert isinstance(only, np.ndarray) and only.shape == (40, 52, 3)
    hit = depth == depth
    assert hit.any() and (~hit).any() and (img[:, :, 0] > 0).any() and (img[~hit] == 0).all() and (img[:, :, 2] == 0).all()
    # stereo: the two eyes composed as render() composes them; no aux plane
    r.CameraXOffset = 0.1
    st = r.renderProjection("mip")
    assert st.shape == r.render().shape
    with pytest.raises(ValueError, match="no aux plane"):
        r.renderProjection("mip", aux=True)
    with pytest.raises(vr.VrError, match="projection mode"):
        r.renderProjection("min")
    r.delete()
