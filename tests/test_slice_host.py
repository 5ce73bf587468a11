"""The slice views' host side that needs no device (include/vrhip.h vr_render_slice): the argument
checks, which come before the handle, the two geometry helpers against their restatements, and the
Python layer's marshalling.  The renders themselves need a device: tests/test_gpu_slice.py."""
import ctypes

import numpy as np
import pytest

import slice_ref as SR
import volume_renderer_amd as vr
from volume_renderer_amd import _lib, mex

F = np.float32
GEOM = np.asfortranarray(F([[0.1, 0.02, 0, 0], [0.1, 0, 0.02, 0], [0.5, 0, 0, 0.01]]))


def good():
    return mex.make_slice(GEOM, [8, 9], 3, "sum", "absorption")


def _set(s, field, k, value):
    getattr(s, field)[k] = value


BAD = {}
for _f in ("origin", "du", "dv", "dw"):
    for _k, _v in ((0, np.nan), (1, np.inf), (2, -np.inf)):
        BAD[f"{_f}[{_k}] = {_v}"] = (lambda s, f=_f, k=_k, v=_v: _set(s, f, k, v))
BAD["samples 0"] = lambda s: setattr(s, "samples", 0)
BAD["samples -1"] = lambda s: setattr(s, "samples", -1)
BAD["samples 4097"] = lambda s: setattr(s, "samples", 4097)
BAD["mode 3"] = lambda s: setattr(s, "mode", 3)
BAD["mode -1"] = lambda s: setattr(s, "mode", -1)
BAD["source 3"] = lambda s: setattr(s, "source", 3)
BAD["source -1"] = lambda s: setattr(s, "source", -1)
BAD["H * W = 2^31"] = lambda s: (_set(s, "resolution", 0, 1 << 16), _set(s, "resolution", 1, 1 << 15))
BAD["H = 2^33"] = lambda s: _set(s, "resolution", 0, 1 << 33)
BAD["H * W wraps"] = lambda s: (_set(s, "resolution", 0, 1 << 32), _set(s, "resolution", 1, 1 << 32))


@pytest.mark.parametrize("case", sorted(BAD))
def test_slice_validation_comes_before_the_handle(case):
    L = _lib.lib()
    s = good()
    BAD[case](s)
    out = np.zeros(72, F)
    for h in (ctypes.c_void_p(12345), None):
        assert L.vr_render_slice(h, ctypes.byref(s), out.ctypes.data, None, None) == 1, case
        assert b"slice" in L.vr_last_error() and b"Handle" not in L.vr_last_error()
        assert L.vr_render_slice_device(h, ctypes.byref(s), None, None, None, None) == 1, case


def test_null_slice_and_the_handle_check():
    L = _lib.lib()
    h = ctypes.c_void_p(12345)
    out = np.zeros(72, F)
    assert L.vr_render_slice(h, None, out.ctypes.data, None, None) == 1 and b"NULL" in L.vr_last_error()
    assert L.vr_render_slice_device(h, None, None, None, None, None) == 1
    # valid arguments reach the handle check, the limits included
    for n, mode, source in ((1, 0, 0), (4096, 2, 2), (33, 1, 1)):
        s = good()
        s.samples, s.mode, s.source = n, mode, source
        assert L.vr_render_slice(h, ctypes.byref(s), out.ctypes.data, None, None) == 2
        assert b"Handle not valid" in L.vr_last_error()
        assert L.vr_render_slice_device(None, ctypes.byref(s), None, None, None, None) == 2
    s = good()
    s.resolution[0], s.resolution[1] = (1 << 16), (1 << 15) - 1  # H * W just below 2^31
    assert L.vr_render_slice(h, ctypes.byref(s), out.ctypes.data, None, None) == 2
    assert ctypes.sizeof(_lib.VrSlice) == 80 and _lib.VR_SLICE_MAX_SAMPLES == 4096


@pytest.mark.parametrize("dims", [(16, 12, 20), (17, 9, 5), (9, 7, 1), (1, 1, 1), (1024, 1000, 3)])
def test_slice_axis_equals_its_numpy_restatement(dims):
    n = 0
    for axis in range(3):
        for index, t in ((0, 1), (dims[axis] - 1, 1), ((dims[axis] - 1) / 2, dims[axis]), (2.25, 4), (-3, 5)):
            got = SR.Slice.of(mex.slice_axis(dims, axis, index, t))
            want = SR.axis_slice(dims, axis, index, t)
            for f in ("origin", "du", "dv", "dw"):
                assert np.array_equal(getattr(got, f).view(np.uint32), getattr(want, f).view(np.uint32)), (axis, f)
            assert (got.H, got.W, got.n) == (want.H, want.W, want.n)
            a, b = [j for j in range(3) if j != axis]
            assert (got.H, got.W) == (dims[a], dims[b]) and a < b  # the lower remaining dimension: rows
            n += 1
    assert n == 15


def test_slice_axis_refusals():
    L = _lib.lib()
    d = (ctypes.c_uint64 * 3)(4, 5, 6)
    s = _lib.VrSlice()
    ok = lambda *a: L.vr_slice_axis(*a)  # noqa: E731
    assert ok(d, 0, 1.0, 1, ctypes.byref(s)) == 0
    assert ok(None, 0, 1.0, 1, ctypes.byref(s)) == 1 and ok(d, 0, 1.0, 1, None) == 1
    assert ok(d, 3, 1.0, 1, ctypes.byref(s)) == 1 and ok(d, -1, 1.0, 1, ctypes.byref(s)) == 1
    assert ok(d, 0, float("nan"), 1, ctypes.byref(s)) == 1 and ok(d, 0, float("inf"), 1, ctypes.byref(s)) == 1
    assert ok(d, 0, 1.0, 0, ctypes.byref(s)) == 1 and ok(d, 0, 1.0, 4097, ctypes.byref(s)) == 1
    assert ok((ctypes.c_uint64 * 3)(4, 0, 6), 0, 1.0, 1, ctypes.byref(s)) == 1
    assert ok(d, 0, 1.0, 4096, ctypes.byref(s)) == 0 and s.samples == 4096


OBLIQUE = [
    dict(dims=(16, 12, 20), es=[1, 1, 1], p=[0.5, 0.45, 0.55], n=[1, 0.6, -0.4], up=[0, 0, 1], px=0.43, H=37, W=41, t=1),
    dict(dims=(64, 64, 40), es=[2.5, 0.8, 0.8], p=[0.3, 0.6, 0.5], n=[0.2, -1, 0.7], up=[1, 1, 0], px=0.8, H=23, W=64, t=5),
    dict(dims=(17, 9, 5), es=[3, 1, 0.5], p=[0.5, 0.5, 0.5], n=[0, 0, 2], up=[0, 5, 0], px=0.25, H=8, W=8, t=32),
]


@pytest.mark.parametrize("case", range(len(OBLIQUE)))
def test_slice_oblique_is_orthonormal_in_physical_space(case):
    c = OBLIQUE[case]
    s = SR.Slice.of(mex.slice_oblique(c["dims"], c["es"], c["p"], c["n"], c["up"], c["px"], c["H"], c["W"], c["t"]))
    assert (s.H, s.W, s.n) == (c["H"], c["W"], c["t"])
    # q -> um: q_j * dims[j] * element_size_um[2 - j]
    ext = np.array([c["dims"][j] * np.float64(F(c["es"][2 - j])) for j in range(3)])
    u, v, w = (np.float64(x) * ext for x in (s.du, s.dv, s.dw))
    tol = 1e-6
    for a in (u, v, w):
        assert abs(np.linalg.norm(a) / c["px"] - 1) < tol
    for a, b in ((u, v), (u, w), (v, w)):
        assert abs(a @ b) / c["px"] ** 2 < tol
    nrm = np.float64(c["n"]) / np.linalg.norm(c["n"])
    assert np.linalg.norm(w / c["px"] - nrm) < tol  # the slab runs along the normal
    assert (v / c["px"]) @ np.float64(c["up"]) > 0  # rows along up, projected
    assert np.linalg.norm(np.cross(v, w) / c["px"] ** 2 - u / c["px"]) < tol  # u = v x w
    centre = (np.float64(s.origin) + np.float64(s.du) * (c["W"] - 1) / 2 + np.float64(s.dv) * (c["H"] - 1) / 2
              + np.float64(s.dw) * (c["t"] - 1) / 2)
    # relative to the largest of the four terms (each carries one fp32 rounding, 2^-24), at least 1
    scale = max(1.0, np.abs(np.float64(s.origin)).max(), np.abs(np.float64(s.du)).max() * (c["W"] - 1) / 2,
                np.abs(np.float64(s.dv)).max() * (c["H"] - 1) / 2, np.abs(np.float64(s.dw)).max() * (c["t"] - 1) / 2)
    assert np.abs(centre - np.float64(c["p"])).max() < tol * scale


def test_slice_oblique_refusals():
    with pytest.raises(vr.VrError, match="zero normal") as e:
        mex.slice_oblique((8, 8, 8), [1, 1, 1], [.5, .5, .5], [0, 0, 0], [0, 0, 1], 1, 4, 4)
    assert e.value.code == 1
    for up in ([0, 0, 0], [0, 0, 3], [0, 0, -1e-3]):
        with pytest.raises(vr.VrError, match="parallel"):
            mex.slice_oblique((8, 8, 8), [1, 1, 1], [.5, .5, .5], [0, 0, 2], up, 1, 4, 4)
    bad = [dict(px=0), dict(px=-1), dict(px=float("nan")), dict(t=0), dict(t=4097), dict(H=1 << 16, W=1 << 15),
           dict(p=[.5, float("nan"), .5]), dict(n=[float("inf"), 0, 1]), dict(es=[1, 0, 1]), dict(dims=(8, 0, 8))]
    for b in bad:
        a = dict(dims=(8, 8, 8), es=[1, 1, 1], p=[.5, .5, .5], n=[0, 1, 2], up=[0, 0, 1], px=1, H=4, W=4, t=1)
        a.update(b)
        with pytest.raises(vr.VrError) as e:
            mex.slice_oblique(a["dims"], a["es"], a["p"], a["n"], a["up"], a["px"], a["H"], a["W"], a["t"])
        assert e.value.code == 1, b
    L = _lib.lib()
    assert L.vr_slice_oblique(None, None, None, None, None, 1.0, 4, 4, 1, None) == 1


def test_python_marshalling():
    h = np.uint64(12345)
    s = good()
    assert (s.samples, s.mode, s.source) == (3, 2, 1) and list(s.resolution) == [8, 9]
    assert [s.origin[2], s.du[0], s.dv[1], s.dw[2]] == [F(0.5), F(0.02), F(0.02), F(0.01)]
    assert np.array_equal(mex.slice_geom(s), GEOM)
    assert mex.slice_mode("MAX") == 0 and mex.slice_mode(1) == 1 and mex.slice_source("Reflection") == 2
    with pytest.raises(vr.VrError, match="slice mode"):
        mex.slice_mode("mean")
    with pytest.raises(vr.VrError, match="slice source"):
        mex.slice_source("gradient")
    with pytest.raises(vr.VrError, match="3 x 4"):
        mex.make_slice(GEOM.T, [8, 9])
    with pytest.raises(vr.VrError, match="3 x 4"):
        mex.make_slice(GEOM.astype(np.float64), [8, 9])
    with pytest.raises(vr.VrError, match="insufficient parameter"):
        vr.volumeRender("render_slice", h, GEOM, np.uint64([8, 9]), 1, "max")
    with pytest.raises(vr.VrError, match="too many"):
        vr.volumeRender("render_slice", h, GEOM, np.uint64([8, 9]), 1, "max", "emission", 0)
    with pytest.raises(vr.VrError, match="samples") as e:
        vr.volumeRender("render_slice", h, GEOM, np.uint64([8, 9]), 0, "max", "emission")
    assert e.value.code == 1
    with pytest.raises(vr.VrError, match="too large"):
        vr.volumeRender("render_slice", h, GEOM, np.uint64([1 << 20, 1 << 20]), 1, "max", "emission")
    for mode, source in (("max", "emission"), (2, 1), ("Sum", "ABSORPTION")):
        with pytest.raises(vr.VrError, match="Handle not valid") as e:
            vr.volumeRender("render_slice", h, GEOM, np.uint64([8, 9]), 2, mode, source)
        assert e.value.code == 2
    with pytest.raises(vr.VrError, match="Handle not valid"):
        mex.render_slice_device(h, s, 0)
