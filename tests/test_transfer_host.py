"""The transfer-function render's argument checks that need no device: the table validation of the two
entry points (before the handle), the Python command's checks, and the C++ MEX adaptor's
(mex/volumeRender_mex.cpp against tests/mexstub/)."""
import ctypes

import numpy as np
import pytest

import mexsim as M
import volume_renderer_amd as vr
from volume_renderer_amd import _lib, mex

F = np.float32
ARGV = [False, False, F([1, 1, 1]), F([1, 1, 1]), np.uint64([4, 4]), np.eye(3, dtype=F), F([0, 3, 6]), F(0.9),
        F([1, 1, 1])]
CMAP = np.asfortranarray(F([[0, 0, 1], [0, 1, 0], [1, 0, 0]]))
TAIL = [CMAP, F([0, 1]), False, F([0, 1]), "value"]


def _tf(n_color=3, clim=(0, 1), alphamap=None, n_alpha=None, alim=(0, 1), coord=0, colormap=CMAP):
    tf = _lib.VrTransfer()
    keep = [np.asfortranarray(colormap, dtype=F) if colormap is not None else None,
            None if alphamap is None else np.ascontiguousarray(alphamap, dtype=F)]
    tf.colormap = keep[0].ctypes.data if keep[0] is not None else None
    tf.n_color = n_color
    tf.clim[0], tf.clim[1] = clim
    if keep[1] is not None:
        tf.alphamap = keep[1].ctypes.data
        tf.n_alpha = keep[1].size if n_alpha is None else n_alpha
    tf.alim[0], tf.alim[1] = alim
    tf.coord = coord
    return tf, keep


BIG = np.zeros((1025, 3), F)
BAD_TABLES = {
    "colormap NULL": dict(colormap=None),
    "one colour entry": dict(n_color=1),
    "1025 colour entries": dict(colormap=BIG, n_color=1025),
    "NaN colour entry": dict(colormap=F([[0, 0, 1], [0, np.nan, 0], [1, 0, 0]])),
    "inf colour entry": dict(colormap=F([[0, 0, 1], [0, 1, 0], [1, 0, np.inf]])),
    "clim lo == hi": dict(clim=(0.5, 0.5)),
    "clim lo > hi": dict(clim=(1, 0)),
    "clim NaN": dict(clim=(np.nan, 1)),
    "clim inf": dict(clim=(0, np.inf)),
    "one alpha entry": dict(alphamap=F([0, 1]), n_alpha=1),
    "1025 alpha entries": dict(alphamap=np.zeros(1025, F)),
    "inf alpha entry": dict(alphamap=F([0, -np.inf, 1])),
    "alim lo >= hi": dict(alphamap=F([0, 1]), alim=(2, 2)),
    "alim NaN": dict(alphamap=F([0, 1]), alim=(0, np.nan)),
    "unknown coord": dict(coord=2),
    "negative coord": dict(coord=-1),
}


@pytest.mark.parametrize("case", sorted(BAD_TABLES))
def test_table_validation_comes_before_the_handle(case):
    L = _lib.lib()
    ra, keep = mex.render_args(*ARGV)
    out = np.zeros(4 * 4 * 3, F)
    tf, tkeep = _tf(**BAD_TABLES[case])
    for h in (ctypes.c_void_p(12345), None):
        assert L.vr_render_transfer(h, ctypes.byref(ra), ctypes.byref(tf), out.ctypes.data, None) == 1, case
        assert len(L.vr_last_error()) > 0 and b"Handle" not in L.vr_last_error()
        assert L.vr_render_transfer_device(h, ctypes.byref(ra), ctypes.byref(tf), None, None, None, None, None) == 1
        assert len(L.vr_last_error()) > 0 and b"Handle" not in L.vr_last_error()
    del keep, tkeep


def test_null_transfer_and_valid_tables():
    L = _lib.lib()
    ra, keep = mex.render_args(*ARGV)
    out = np.zeros(4 * 4 * 3, F)
    assert L.vr_render_transfer(ctypes.c_void_p(12345), ctypes.byref(ra), None, out.ctypes.data, None) == 1
    assert L.vr_render_transfer_device(None, ctypes.byref(ra), None, None, None, None, None, None) == 1
    # valid tables reach the handle check; alim is not looked at without an alphamap
    for kw in (dict(), dict(alim=(np.nan, 0)), dict(alphamap=F([0, 0.5, 1]), alim=(0, 2)), dict(coord=1),
               dict(colormap=np.zeros((1024, 3), F), n_color=1024)):
        tf, tkeep = _tf(**kw)
        assert L.vr_render_transfer(ctypes.c_void_p(12345), ctypes.byref(ra), ctypes.byref(tf), out.ctypes.data, None) == 2
        assert b"Handle not valid" in L.vr_last_error()
        assert L.vr_render_transfer_device(None, ctypes.byref(ra), ctypes.byref(tf), None, None, None, None, None) == 2
    del keep


def test_lookup_host_argument_errors():
    L = _lib.lib()
    t, c, out = F([0, 1]), F([0.5]), np.zeros(1, F)
    lim = (ctypes.c_float * 2)(0, 1)
    ok = L.vr_transfer_lookup_host(t.ctypes.data, 2, 1, lim, c.ctypes.data, 1, out.ctypes.data)
    assert ok == 0 and out[0] == 0.5
    assert L.vr_transfer_lookup_host(t.ctypes.data, 1, 1, lim, c.ctypes.data, 1, out.ctypes.data) == 1
    assert L.vr_transfer_lookup_host(t.ctypes.data, 1025, 1, lim, c.ctypes.data, 1, out.ctypes.data) == 1
    assert L.vr_transfer_lookup_host(t.ctypes.data, 2, 0, lim, c.ctypes.data, 1, out.ctypes.data) == 1
    assert L.vr_transfer_lookup_host(None, 2, 1, lim, c.ctypes.data, 1, out.ctypes.data) == 1
    assert L.vr_transfer_lookup_host(t.ctypes.data, 2, 1, (ctypes.c_float * 2)(1, 1), c.ctypes.data, 1, out.ctypes.data) == 1
    assert L.vr_transfer_lookup_host(None, 2, 1, lim, None, 0, None) == 0  # nothing to do


def test_python_command_checks():
    h = np.uint64(12345)
    with pytest.raises(vr.VrError, match="insufficient parameter"):
        vr.volumeRender("render_transfer", h, *ARGV, *TAIL[:4])
    with pytest.raises(vr.VrError, match="Handle not valid") as e:
        vr.volumeRender("render_transfer", h, *ARGV, *TAIL)
    assert e.value.code == 2
    with pytest.raises(vr.VrError, match="single N x 3"):
        vr.volumeRender("render_transfer", h, *ARGV, CMAP.astype(np.float64), *TAIL[1:])
    with pytest.raises(vr.VrError, match="single N x 3"):
        vr.volumeRender("render_transfer", h, *ARGV, F([[0, 1], [1, 0]]), *TAIL[1:])
    with pytest.raises(vr.VrError, match="alphamap"):
        vr.volumeRender("render_transfer", h, *ARGV, CMAP, F([0, 1]), np.zeros((2, 2), F), F([0, 1]), "value")
    with pytest.raises(vr.VrError, match="coordinate"):
        vr.volumeRender("render_transfer", h, *ARGV, *TAIL[:4], "time")
    with pytest.raises(vr.VrError, match="lo < hi") as e:
        vr.volumeRender("render_transfer", h, *ARGV, CMAP, F([1, 0]), False, F([0, 1]), "depth")
    assert e.value.code == 1


def test_mex_argument_and_output_counts():
    h = np.uint64(1)
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, *TAIL[:4])  # no coord
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 1, "render_transfer", h, False, False)
    with pytest.raises(M.MexError, match="too many input arguments"):
        M.call("volumeRender", 1, "render_transfer", h, *ARGV, *TAIL, "extra")
    with pytest.raises(M.MexError, match="Too many output arguments."):
        M.call("volumeRender", 3, "render_transfer", h, *ARGV, *TAIL)


def test_mex_type_checks_and_handle():
    h = np.uint64(1)
    with pytest.raises(M.MexError, match="colormap must be a single N x 3 matrix"):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, CMAP.astype(np.float64), *TAIL[1:])
    with pytest.raises(M.MexError, match="colormap must be a single N x 3 matrix"):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, np.asfortranarray(CMAP.T[:, :2]), *TAIL[1:])
    with pytest.raises(M.MexError, match="clim must be single"):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, CMAP, np.float64([0, 1]), *TAIL[2:])
    with pytest.raises(M.MexError, match="alphamap must be a single vector or false"):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, CMAP, F([0, 1]), np.float64([0, 1]), F([0, 1]), "value")
    with pytest.raises(M.MexError, match="coord must be 'value' or 'depth'"):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, *TAIL[:4], "time")
    with pytest.raises(M.MexError, match="coord must be 'value' or 'depth'"):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, *TAIL[:4], np.float64(0))
    # the library's own table checks arrive as its message
    with pytest.raises(M.MexError, match="lo < hi"):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, CMAP, F([1, 1]), *TAIL[2:])
    with pytest.raises(M.MexError, match="Handle not valid."):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, *TAIL)
    with pytest.raises(M.MexError, match="Handle not valid."):
        M.call("volumeRender", 2, "render_transfer", h, *ARGV, CMAP, F([0, 1]), F([0, 0.5, 1]), F([0, 2]), "depth")
