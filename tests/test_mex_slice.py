"""The 'render_slice' command at the MATLAB boundary: the C++ MEX adaptor (mex/volumeRender_mex.cpp
against tests/mexstub/) returns the bits of the ctypes path, its argument checks, and the Python class
method VolumeRender.renderSlice on top of the command."""
import numpy as np
import pytest

import mexsim as M
import oracle as O

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import mex  # noqa: E402

F = np.float32
GEOM = mex.slice_geom(mex.slice_oblique((24, 24, 24), [1, 1, 1], [0.5, 0.5, 0.5], [1, 0.5, 0.25], [0, 0, 1], 0.9, 23, 37, 5))
RES = np.uint64([23, 37])
ARGV = [GEOM, RES, np.int32(5), "max", "emission"]


def _stamped(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def test_render_slice_argument_checks():
    h = np.uint64(1)
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 3, "render_slice", h, *ARGV[:4])  # no source
    with pytest.raises(M.MexError, match="too many input arguments"):
        M.call("volumeRender", 3, "render_slice", h, *ARGV, 0.0)
    with pytest.raises(M.MexError, match="Too many output arguments."):
        M.call("volumeRender", 4, "render_slice", h, *ARGV)
    for geom in (np.asfortranarray(GEOM.T), GEOM.astype(np.float64), GEOM[:, :3]):
        with pytest.raises(M.MexError, match="geom must be a single 3 x 4"):
            M.call("volumeRender", 1, "render_slice", h, geom, *ARGV[1:])
    with pytest.raises(M.MexError, match="res must be uint64"):
        M.call("volumeRender", 1, "render_slice", h, GEOM, np.float64([23, 37]), *ARGV[2:])
    # values the library refuses, before the handle: the slab length, the names, non-finite geometry
    for n in (np.int32(0), np.float64(2.5), np.float64(4097)):
        with pytest.raises(M.MexError, match="samples"):
            M.call("volumeRender", 1, "render_slice", h, GEOM, RES, n, "max", "emission")
    with pytest.raises(M.MexError, match="unknown slice mode"):
        M.call("volumeRender", 1, "render_slice", h, GEOM, RES, np.int32(1), "mean", "emission")
    with pytest.raises(M.MexError, match="unknown slice source"):
        M.call("volumeRender", 1, "render_slice", h, GEOM, RES, np.int32(1), "max", np.float64(3))
    bad = GEOM.copy()
    bad[1, 2] = np.inf
    with pytest.raises(M.MexError, match="non-finite"):
        M.call("volumeRender", 1, "render_slice", h, bad, *ARGV[1:])
    with pytest.raises(M.MexError, match="too large"):
        M.call("volumeRender", 1, "render_slice", h, GEOM, np.uint64([1 << 20, 1 << 20]), *ARGV[2:])
    for mode, source in (("max", "emission"), (np.float64(2), np.int32(1)), ("min", "reflection")):
        with pytest.raises(M.MexError, match="Handle not valid."):
            M.call("volumeRender", 3, "render_slice", h, GEOM, RES, np.float64(5), mode, source)


@pytest.mark.gpu
def test_render_slice_through_mexfunction_equals_python_path():
    em = _stamped(O.shell_volume(24), 11)
    re = _stamped(np.float32(1.0), 12)
    lab = np.asfortranarray((np.arange(24 ** 3).reshape(24, 24, 24) % 5).astype(np.uint8))
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    M.call("volumeRender", 0, "sync_labels", h, lab)
    got = {m: M.call("volumeRender", 3, "render_slice", h, GEOM, RES, np.int32(5), m, "emission")
           for m in ("max", "min", "sum")}
    (only,) = M.call("volumeRender", 1, "render_slice", h, GEOM, RES, np.float64(5), np.float64(0), np.float64(0))
    M.call("volumeRender", 0, "delete", h)
    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    vr.volumeRender("sync_labels", hp, lab)
    for m in ("max", "min", "sum"):
        want = vr.volumeRender("render_slice", hp, GEOM, RES, 5, m, "emission")
        for g, w in zip(got[m], want):
            assert g.dtype == np.float32 and g.shape == (23, 37) and w.shape == (23, 37)
            assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), m
    assert np.array_equal(only.view(np.uint32), got["max"][0].view(np.uint32))
    img, aux, lb = got["sum"]
    assert np.isnan(img).any() and (img[~np.isnan(img)] > 0).any() and (aux == 5).any()
    assert np.isfinite(lb).any() and set(np.unique(lb[np.isfinite(lb)])) <= {0, 1, 2, 3, 4}
    vr.volumeRender("delete", hp)


@pytest.mark.gpu
def test_render_slice_method(counter_clock):
    r = vr.VolumeRender()
    data = np.asfortranarray(np.random.default_rng(2).integers(0, 200, (14, 11, 9), dtype=np.uint8).astype(F))
    v = vr.Volume(data)
    r.VolumeEmission = v
    r.VolumeAbsorption = v
    r.ElementSizeUm = [1, 1, 2]
    img = r.renderSlice(axis=3, index=4)
    assert isinstance(img, np.ndarray) and np.array_equal(img.view(np.uint32), data[:, :, 3].view(np.uint32))
    img, aux = r.renderSlice(axis=2, index=6, thickness=5, mode="mean", aux=True)
    assert img.shape == (14, 9) and (aux == 5).all()
    want = np.zeros((14, 9), F)
    for k in range(3, 8):
        want = want + data[:, k, :]
    assert np.array_equal(img, (want / F(5)).astype(F))
    mx, k = r.renderSlice(axis=1, index=2, thickness=3, mode="max", aux=True)
    assert np.array_equal(mx, data[0:3].max(axis=0)) and np.array_equal(k, data[0:3].argmax(axis=0).astype(F))
    # oblique, with labels; without VolumeLabels the label plane is NaN
    r.ImageResolution = [31, 27]
    img, lab = r.renderSlice(point=[0.5, 0.5, 0.5], normal=[1, 1, 0.5], labels=True)
    assert img.shape == (27, 31) and np.isnan(lab).all()
    assert np.isnan(img).any() and np.isfinite(img).any()
    want = vr.volumeRender("render_slice", r.objectHandle,
                           mex.slice_geom(mex.slice_oblique((14, 11, 9), [1, 1, 2], [0.5, 0.5, 0.5], [1, 1, 0.5],
                                                            [0, 0, 1], 1.0, 27, 31, 1)),
                           np.uint64([27, 31]), 1, "max", "emission")[0]
    assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
    r.VolumeLabels = (data > 100).astype(np.uint8)
    lab = r.renderSlice(axis=3, index=4, labels=True)[1]
    assert np.array_equal(lab, (data[:, :, 3] > 100).astype(F))
    with pytest.raises(ValueError, match="axis"):
        r.renderSlice(axis=1)
    with pytest.raises(vr.VrError, match="slice mode"):
        r.renderSlice(axis=1, index=1, mode="median")
    r.delete()
