"""The 'render_isosurface' command at the MATLAB boundary: the C++ MEX adaptor (mex/volumeRender_mex.cpp
against tests/mexstub/) returns the bits of the ctypes path, its argument checks, and the Python
class method VolumeRender.renderIsosurface on top of the command."""
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


def same(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_render_isosurface_argument_count():
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 3, "render_isosurface", np.uint64(1), *ARGV)  # no level
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 1, "render_isosurface", np.uint64(1), False, False)
    with pytest.raises(M.MexError, match="Too many output arguments."):
        M.call("volumeRender", 4, "render_isosurface", np.uint64(1), *ARGV, np.float32(0.3))


def test_render_isosurface_argument_types():
    with pytest.raises(M.MexError, match="level must be a real scalar"):
        M.call("volumeRender", 3, "render_isosurface", np.uint64(1), *ARGV, "0.3")
    with pytest.raises(M.MexError, match="level must be a real scalar"):
        M.call("volumeRender", 3, "render_isosurface", np.uint64(1), *ARGV, np.float32([0.3, 0.4]))
    with pytest.raises(M.MexError, match="level must be a real scalar"):
        M.call("volumeRender", 3, "render_isosurface", np.uint64(1), *ARGV, np.True_)  # a logical is not numeric
    with pytest.raises(M.MexError, match="level is NaN"):  # the library's check, before the handle's
        M.call("volumeRender", 3, "render_isosurface", np.uint64(1), *ARGV, np.float64("nan"))
    with pytest.raises(M.MexError, match="Handle not valid."):
        M.call("volumeRender", 3, "render_isosurface", np.uint64(1), *ARGV, np.float64(0.3))


def _lit_argv():
    lights = [vr.LightSource([500, 1000, 550], [0, 1, 1]), vr.LightSource([0, 550, 90], [1, 0.5, 1])]
    return [lights, _stamped(vr.HenyeyGreenstein(32), 13)] + ARGV[2:]


@pytest.mark.gpu
def test_render_isosurface_through_mexfunction_equals_python_path():
    em = _stamped(O.shell_volume(24), 11)
    re = _stamped(np.float32(1.0), 12)
    argv = _lit_argv()
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    got = M.call("volumeRender", 3, "render_isosurface", h, *argv, np.float32(0.3))
    (only,) = M.call("volumeRender", 1, "render_isosurface", h, *argv, np.float64(0.3))  # a double level: (float)
    M.call("volumeRender", 0, "delete", h)
    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    img, depth, normal = vr.volumeRender("render_isosurface", hp, *argv, np.float32(0.3))
    vr.volumeRender("delete", hp)
    assert got[0].dtype == np.float32 and got[0].shape == (40, 52, 3) and got[1].shape == (40, 52)
    assert got[2].shape == (40, 52, 3)
    assert same(got[0], img) and same(got[1], depth) and same(got[2], normal) and same(only, img)
    surf = ~np.isnan(depth)
    assert surf.sum() > 200 and (~surf).any() and (img[surf].max(1) > 0).all() and (img[~surf] == 0).all()
    assert np.allclose(np.linalg.norm(normal[surf], axis=1), 1, atol=1e-5) and np.isnan(normal[~surf]).all()


@pytest.mark.gpu
def test_render_isosurface_method(counter_clock):
    r = vr.VolumeRender()
    r.FocalLength, r.DistanceToObject = 3.0, 6
    r.rotate(125, 25, 0)
    r.ImageResolution = [52, 40]
    v = vr.Volume(O.shell_volume(24))
    r.VolumeEmission = v
    r.VolumeAbsorption = v
    r.VolumeIllumination = vr.Volume(vr.HenyeyGreenstein(32))
    r.LightSources = [vr.LightSource([500, 1000, 550], [0, 1, 1])]
    r.FactorEmission, r.FactorReflection = 1.5, 0.4
    r.Color = [1, 1, 0]
    img, depth, normal = r.renderIsosurface(0.3, aux=True)
    assert img.shape == (40, 52, 3) and depth.shape == (40, 52) and normal.shape == (40, 52, 3)
    argv = r._render_argv(np.float32(0), np.flip(r.ImageResolution))
    want = vr.volumeRender("render_isosurface", r.objectHandle, *argv, 0.3)
    assert same(img, want[0]) and same(depth, want[1]) and same(normal, want[2])
    only = r.renderIsosurface(0.3)
    assert isinstance(only, np.ndarray) and same(only, img)
    surf = depth == depth
    assert surf.any() and (~surf).any() and (img[:, :, 0][surf] > 0).all() and (img[~surf] == 0).all()
    assert (img[:, :, 2] == 0).all()
    # stereo: the two eyes composed as render() composes them; no aux planes
    r.CameraXOffset = 0.1
    st = r.renderIsosurface(0.3)
    assert st.shape == r.render().shape
    with pytest.raises(ValueError, match="no aux planes"):
        r.renderIsosurface(0.3, aux=True)
    with pytest.raises(vr.VrError, match="real scalar"):
        r.renderIsosurface("high")
    r.delete()
