"""The 'render_transfer' command at the MATLAB boundary: the C++ MEX adaptor (mex/volumeRender_mex.cpp
against tests/mexstub/) returns the bits of the ctypes path, and the Python class method
VolumeRender.renderTransfer on top of the command.  (The adaptor's argument checks need no device:
tests/test_transfer_host.py.)"""
import numpy as np
import pytest

import mexsim as M
import oracle as O

vr = pytest.importorskip("volume_renderer_amd")

pytestmark = pytest.mark.gpu
F = np.float32
R = np.flip(O.rotation(125, 25, 0), 0).astype(np.float32)
ARGV = [False, False, F([1.5, 0.4, 0.6]), F([1, 1, 1]), np.uint64([40, 52]), R, F([0, 3, 6]), F(0.9), F([1, 1, 0])]
CMAP = np.asfortranarray(F([[0.1, 0.9, 0.3], [1.0, 0.2, 0.0], [0.3, 0.3, 1.2], [0.8, 1.0, 0.1]]))
AMAP = F([0.0, 0.4, 1.2]).reshape(-1, 1)
TAILS = {"value": [CMAP, F([0.2, 0.7]), AMAP, F([0.05, 0.8]), "value"],
         "no_alphamap": [CMAP, F([0.2, 0.7]), False, F([0, 1]), "value"],
         "depth": [CMAP, F([4.5, 7.5]), AMAP, F([0.05, 0.8]), "depth"]}


def _stamped(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_render_transfer_through_mexfunction_equals_python_path():
    em = _stamped(O.shell_volume(24), 11)
    re = _stamped(np.float32(1.0), 12)
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    got = {k: M.call("volumeRender", 2, "render_transfer", h, *ARGV, *t) for k, t in TAILS.items()}
    (only,) = M.call("volumeRender", 1, "render_transfer", h, *ARGV, *TAILS["value"])
    row = M.call("volumeRender", 2, "render_transfer", h, *ARGV, CMAP, F([0.2, 0.7]), AMAP.reshape(-1), F([0.05, 0.8]),
                 "value")  # a 1 x M alphamap
    M.call("volumeRender", 0, "delete", h)
    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    for k, t in TAILS.items():
        img, alpha = vr.volumeRender("render_transfer", hp, *ARGV, *t)
        assert got[k][0].dtype == np.float32 and got[k][0].shape == (40, 52, 3) and got[k][1].shape == (40, 52)
        assert bits_equal(got[k][0], img) and bits_equal(got[k][1], alpha)
        assert img.max() > 0 and 0 < alpha.max() <= 1
    assert bits_equal(only, got["value"][0])
    assert bits_equal(row[0], got["value"][0]) and bits_equal(row[1], got["value"][1])
    assert not bits_equal(got["value"][0], got["depth"][0]) and bits_equal(got["value"][1], got["depth"][1])
    assert not bits_equal(got["value"][1], got["no_alphamap"][1])
    assert (got["value"][1] == 0).any()  # misses
    vr.volumeRender("delete", hp)


def test_render_transfer_method(counter_clock, monkeypatch):
    r = vr.VolumeRender()
    r.FocalLength, r.DistanceToObject = 3.0, 6
    r.rotate(125, 25, 0)
    r.ImageResolution = [52, 40]
    v = vr.Volume(O.shell_volume(24))
    r.VolumeEmission = v
    r.VolumeAbsorption = v
    r.FactorEmission = 1.5
    r.Color = [1, 1, 0]
    cmap64 = CMAP.astype(np.float64)  # parula(256)-style double maps are cast to single
    img, alpha = r.renderTransfer(cmap64, clim=(0.2, 0.7), alphamap=[0.0, 0.4, 1.2], alim=(0.05, 0.8), alpha=True)
    assert img.shape == (40, 52, 3) and alpha.shape == (40, 52)
    argv = r._render_argv(np.float32(0), np.flip(r.ImageResolution))
    want, want_alpha = vr.volumeRender("render_transfer", r.objectHandle, *argv, *TAILS["value"])
    assert bits_equal(img, want) and bits_equal(alpha, want_alpha)
    only = r.renderTransfer(CMAP)
    assert isinstance(only, np.ndarray) and only.shape == (40, 52, 3)
    hit = alpha > 0
    assert hit.any() and (~hit).any() and (img[~hit] == 0).all() and (img[hit].max(axis=1) > 0).any()
    # a constant colormap equal to Color and no alphamap: the exact-shading render's image bit for bit
    const = r.renderTransfer(np.tile(F([1, 1, 0]), (2, 1)))
    monkeypatch.setenv("VR_EXACT_SHADE", "1")
    assert bits_equal(const, r.render())
    monkeypatch.delenv("VR_EXACT_SHADE")
    # stereo: the two eyes composed as render() composes them; no alpha plane
    r.CameraXOffset = 0.1
    st = r.renderTransfer(CMAP, clim=(0.2, 0.7))
    base, delta, resolution = r._stereo_geometry()
    eyes = [vr.volumeRender("render_transfer", r.objectHandle, *r._render_argv(np.float32(b), resolution), CMAP,
                            F([0.2, 0.7]), False, F([0, 1]), "value")[0] for b in (-base, base)]
    want_st = r._compose(eyes[0], eyes[1], delta)
    assert st.shape == want_st.shape == r.render().shape and np.array_equal(st, want_st)
    assert not bits_equal(eyes[0], eyes[1]) and st.max() > 0
    with pytest.raises(ValueError, match="no alpha plane"):
        r.renderTransfer(CMAP, alpha=True)
    with pytest.raises(vr.VrError, match="coordinate"):
        r.renderTransfer(CMAP, coord="time")
    with pytest.raises(vr.VrError, match="lo < hi"):
        r.renderTransfer(CMAP, clim=(1, 1))
    r.delete()
