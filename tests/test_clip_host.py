"""The clip planes' host side that needs no device (include/vrhip.h vr_set_clip): the argument checks,
which come before the handle, the host conversion against its numpy restatement (tests/clip_ref.py),
and the Python layer's marshalling.  The set / get round trip needs a handle, which needs a device:
tests/test_gpu_clip.py has it."""
import ctypes

import numpy as np
import pytest

import clip_ref as CR
import volume_renderer_amd as vr
from volume_renderer_amd import _lib, mex

F = np.float32
GOOD = F([[0.6, -0.3, 0.74, -0.52]])

BAD_PLANES = {
    "NaN normal": F([[np.nan, 0, 1, 0]]),
    "NaN offset": F([[0, 0, 1, np.nan]]),
    "inf normal": F([[0, np.inf, 0, 0]]),
    "-inf offset": F([[0, 1, 0, -np.inf]]),
    "all-zero normal": F([[0, 0, 0, 0.5]]),
    "minus-zero normal": F([[-0.0, 0.0, -0.0, 1]]),
    "bad second plane": F([[1, 0, 0, 0], [0, 0, 0, 0]]),
    "bad sixth plane": np.concatenate([np.tile(GOOD, (5, 1)), F([[0, np.nan, 0, 0]])]),
    "seven planes": np.tile(GOOD, (7, 1)),
}


def _arr(planes):
    arr = (_lib.VrClipPlane * max(len(planes), 1))()
    for i, p in enumerate(planes):
        arr[i].normal[0], arr[i].normal[1], arr[i].normal[2], arr[i].offset = (float(x) for x in p)
    return arr


@pytest.mark.parametrize("case", sorted(BAD_PLANES))
def test_plane_validation_comes_before_the_handle(case):
    L = _lib.lib()
    pl = BAD_PLANES[case]
    for h in (ctypes.c_void_p(12345), None):
        assert L.vr_set_clip(h, _arr(pl), len(pl)) == 1, case
        assert b"clip planes" in L.vr_last_error() and b"Handle" not in L.vr_last_error()
    out = np.zeros((len(pl), 4), F)
    box = (ctypes.c_float * 3)(-1, -1, -1), (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert L.vr_clip_convert_host(_arr(pl), len(pl), box[0], box[1], out.ctypes.data) == 1


def test_counts_and_null_pointers():
    L = _lib.lib()
    h = ctypes.c_void_p(12345)
    assert L.vr_set_clip(h, _arr(GOOD), -1) == 1
    assert L.vr_set_clip(h, _arr(GOOD), 7) == 1
    assert L.vr_set_clip(h, None, 1) == 1 and b"NULL" in L.vr_last_error()
    # valid arguments reach the handle check: 0 planes with a NULL pointer, 1 and 6 planes
    for arr, n in ((None, 0), (_arr(GOOD), 0), (_arr(GOOD), 1), (_arr(np.tile(GOOD, (6, 1))), 6)):
        assert L.vr_set_clip(h, arr, n) == 2, n
        assert b"Handle not valid" in L.vr_last_error()
        assert L.vr_set_clip(None, arr, n) == 2
    n = ctypes.c_int32(-5)
    got = (_lib.VrClipPlane * _lib.VR_CLIP_MAX)()
    assert L.vr_get_clip(h, None, ctypes.byref(n)) == 1
    assert L.vr_get_clip(h, got, None) == 1
    assert L.vr_get_clip(h, got, ctypes.byref(n)) == 2 and n.value == -5
    assert _lib.VR_CLIP_MAX == CR.CLIP_MAX == 6 and ctypes.sizeof(_lib.VrClipPlane) == 16


BOXES = [([-1, -1, -1], [0.5, 0.5, 0.5]), ([-1, -0.75, -1.25], [0.5, 1 / 1.5, 0.4]),
         ([-1, -0.3333333, -2.7], [0.5, 1.5000001, 0.18518518])]


@pytest.mark.parametrize("box", range(len(BOXES)))
def test_host_conversion_equals_its_numpy_restatement(box):
    bmin, bsc = (F(v) for v in BOXES[box])
    rng = np.random.default_rng(7 + box)
    planes = np.concatenate([CR.WEDGE, CR.KEEP_ALL, (rng.random((2, 4), dtype=F) - F(0.5)) * F(3)])
    got = mex.clip_convert_host(planes, bmin, bsc)
    want = CR.convert(planes, bmin, bsc)
    assert got.dtype == np.float32 and got.shape == (6, 4)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the converted plane is the same half-space: N . p + D == n . q + offset at q = (p - bmin) * bscale
    p = rng.random((50, 3)) * 2 - 1
    q = (p - bmin.astype(np.float64)) * bsc.astype(np.float64)
    lhs = p @ got[:, :3].astype(np.float64).T + got[:, 3].astype(np.float64)
    rhs = q @ planes[:, :3].astype(np.float64).T + planes[:, 3].astype(np.float64)
    assert np.allclose(lhs, rhs, rtol=0, atol=2e-5)
    assert mex.clip_convert_host(None, bmin, bsc).shape == (0, 4)


def test_host_conversion_null_box():
    L = _lib.lib()
    out = np.zeros(4, F)
    b = (ctypes.c_float * 3)(-1, -1, -1)
    assert L.vr_clip_convert_host(_arr(GOOD), 1, None, b, out.ctypes.data) == 1
    assert L.vr_clip_convert_host(_arr(GOOD), 1, b, None, out.ctypes.data) == 1
    assert L.vr_clip_convert_host(_arr(GOOD), 1, b, b, None) == 1
    assert L.vr_clip_convert_host(None, 0, b, b, None) == 0  # nothing to do


def test_python_marshalling():
    h = np.uint64(12345)
    arr, n = mex.clip_planes(CR.WEDGE)
    assert n == 3 and [arr[1].normal[k] for k in range(3)] + [arr[1].offset] == list(CR.WEDGE[1])
    assert mex.clip_planes([1, 0, 0, -0.5])[1] == 1  # one plane as a vector
    for empty in (None, False, [], np.zeros((0, 4), F)):
        assert mex.clip_planes(empty) == (None, 0)
    with pytest.raises(vr.VrError, match="n x 4"):
        mex.clip_planes(np.zeros((4, 3), F))
    with pytest.raises(vr.VrError, match="Handle not valid") as e:
        mex.set_clip(h, CR.OBLIQUE)
    assert e.value.code == 2
    with pytest.raises(vr.VrError, match="clip planes") as e:
        mex.set_clip(h, np.tile(GOOD, (7, 1)))
    assert e.value.code == 1
    with pytest.raises(vr.VrError, match="all-zero normal"):
        mex.set_clip(h, [[0, 0, 0, 1]])
    with pytest.raises(vr.VrError, match="Handle not valid"):
        mex.get_clip(h)
    # the command takes the planes as MATLAB passes them: 4 x n, columns [n0; n1; n2; offset]
    with pytest.raises(vr.VrError, match="insufficient parameter"):
        vr.volumeRender("set_clip", h)
    with pytest.raises(vr.VrError, match="4 x n"):
        vr.volumeRender("set_clip", h, CR.WEDGE)  # (3 x 4: rows, not columns)
    with pytest.raises(vr.VrError, match="non-finite"):
        vr.volumeRender("set_clip", h, F([[1], [0], [np.inf], [0]]))
    for clear in (np.zeros((0, 0), F), False, np.asfortranarray(CR.WEDGE.T)):
        with pytest.raises(vr.VrError, match="Handle not valid"):
            vr.volumeRender("set_clip", h, clear)
