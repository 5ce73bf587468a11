"""The 'set_clip' command at the MATLAB boundary: the C++ MEX adaptor (mex/volumeRender_mex.cpp against
tests/mexstub/) -- its argument checks without a device, and on the GPU that planes set through it
clip exactly as planes set through the ctypes path -- and the ClipPlanes property of the Python
VolumeRender mirror on top of the command."""
import numpy as np
import pytest

import clip_ref as CR
import mexsim as M
import oracle as O

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import mex  # noqa: E402

F = np.float32
R = np.flip(O.rotation(125, 25, 0), 0).astype(F)
ARGV = [False, False, F([1.5, 0.4, 0.6]), F([1, 1, 1]), np.uint64([40, 52]), R, F([0, 3, 6]), F(0.9), F([1, 1, 0])]
PLANES = np.asfortranarray(CR.WEDGE.T)  # 4 x 3, columns [n0; n1; n2; offset]


def _stamped(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def test_set_clip_argument_and_output_counts():
    h = np.uint64(1)
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 0, "set_clip", h)
    with pytest.raises(M.MexError, match="too many input arguments"):
        M.call("volumeRender", 0, "set_clip", h, PLANES, PLANES)
    with pytest.raises(M.MexError, match="Too many output arguments."):
        M.call("volumeRender", 1, "set_clip", h, PLANES)
    with pytest.raises(M.MexError, match="Second input should be a class instance handle."):
        M.call("volumeRender", 0, "set_clip")


def test_set_clip_type_checks_and_handle():
    h = np.uint64(1)
    bad = "planes must be a single 4 x n matrix"
    with pytest.raises(M.MexError, match=bad):
        M.call("volumeRender", 0, "set_clip", h, PLANES.astype(np.float64))
    with pytest.raises(M.MexError, match=bad):
        M.call("volumeRender", 0, "set_clip", h, np.asfortranarray(CR.WEDGE))  # 3 x 4: rows, not columns
    with pytest.raises(M.MexError, match=bad):
        M.call("volumeRender", 0, "set_clip", h, np.zeros((4, 2, 2), F))
    with pytest.raises(M.MexError, match=bad):
        M.call("volumeRender", 0, "set_clip", h, True)
    with pytest.raises(M.MexError, match=bad):
        M.call("volumeRender", 0, "set_clip", h, "none")
    # the library's own checks arrive as its message, before the handle
    with pytest.raises(M.MexError, match="clip planes: 0 .. 6 planes"):
        M.call("volumeRender", 0, "set_clip", h, np.asfortranarray(np.tile(CR.OBLIQUE.T, (1, 7))))
    with pytest.raises(M.MexError, match="all-zero normal"):
        M.call("volumeRender", 0, "set_clip", h, F([[0], [0], [0], [1]]))
    with pytest.raises(M.MexError, match="non-finite"):
        M.call("volumeRender", 0, "set_clip", h, F([[1], [np.nan], [0], [1]]))
    # valid planes, [] and false reach the handle check
    for planes in (PLANES, np.asfortranarray(np.tile(CR.OBLIQUE.T, (1, 6))), np.zeros((0, 0), F),
                   np.zeros((0, 0), np.float64), False):
        with pytest.raises(M.MexError, match="Handle not valid."):
            M.call("volumeRender", 0, "set_clip", h, planes)


@pytest.mark.gpu
def test_set_clip_through_mexfunction_equals_python_path():
    em = _stamped(O.shell_volume(24), 11)
    re = _stamped(np.float32(1.0), 12)
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    plain = M.call("volumeRender", 2, "render_projection", h, *ARGV, "sum")
    assert M.call("volumeRender", 0, "set_clip", h, PLANES) == []
    assert np.array_equal(mex.get_clip(h), CR.WEDGE)  # (one library: the ctypes path reads the same handle)
    got = M.call("volumeRender", 2, "render_projection", h, *ARGV, "sum")
    (lit,) = M.call("volumeRender", 1, "render", h, *ARGV)
    for clear in (np.zeros((0, 0), F), False):
        M.call("volumeRender", 0, "set_clip", h, PLANES)
        M.call("volumeRender", 0, "set_clip", h, clear)
        assert mex.get_clip(h).shape == (0, 4)
        again = M.call("volumeRender", 2, "render_projection", h, *ARGV, "sum")
        assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(plain, again))
    M.call("volumeRender", 0, "delete", h)
    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    vr.volumeRender("set_clip", hp, PLANES)
    img, aux = vr.volumeRender("render_projection", hp, *ARGV, "sum")
    want = vr.volumeRender("render", hp, *ARGV)
    vr.volumeRender("delete", hp)
    assert np.array_equal(got[0].view(np.uint32), img.view(np.uint32))
    assert np.array_equal(got[1].view(np.uint32), aux.view(np.uint32))
    assert np.array_equal(lit.view(np.uint32), want.view(np.uint32)) and lit.max() > 0
    # the planes cut: fewer samples on some rays, some rays lost, none gained
    assert (aux <= plain[1]).all() and ((aux < plain[1]) & (aux > 0)).sum() >= 50
    assert ((aux == 0) & (plain[1] > 0)).sum() >= 50


@pytest.mark.gpu
def test_clip_planes_property_of_the_mirror(counter_clock):
    r = vr.VolumeRender()
    r.FocalLength, r.DistanceToObject = 3.0, 6
    r.rotate(125, 25, 0)
    r.ImageResolution = [52, 40]
    v = vr.Volume(O.shell_volume(24))
    r.VolumeEmission = v
    r.VolumeAbsorption = v
    r.FactorEmission = 1.5
    r.Color = [1, 1, 0]
    assert r.ClipPlanes.shape == (0, 4) and r.ClipPlanes.dtype == np.float32
    plain = {"render": r.render(), "sum": r.renderProjection("sum", aux=True), "iso": r.renderIsosurface(0.3, aux=True),
             "tf": r.renderTransfer(np.eye(3, dtype=F), alpha=True)}
    assert mex.get_clip(r.objectHandle).shape == (0, 4)
    r.ClipPlanes = CR.WEDGE
    cut = {"render": r.render(), "sum": r.renderProjection("sum", aux=True), "iso": r.renderIsosurface(0.3, aux=True),
           "tf": r.renderTransfer(np.eye(3, dtype=F), alpha=True)}
    assert np.array_equal(mex.get_clip(r.objectHandle), CR.WEDGE)
    # every render method of the mirror applied them: what the commands give with the planes on the handle
    argv = r._render_argv(np.float32(0), np.flip(r.ImageResolution))
    want = vr.volumeRender("render", r.objectHandle, *argv)
    assert np.array_equal(cut["render"].view(np.uint32), want.view(np.uint32))
    wsum = vr.volumeRender("render_projection", r.objectHandle, *argv, "sum")
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(cut["sum"], wsum))
    n0, n1 = plain["sum"][1], cut["sum"][1]
    lost = (n0 > 0) & (n1 == 0)
    assert lost.sum() >= 50 and ((n1 < n0) & (n1 > 0)).sum() >= 50
    assert (cut["render"][lost] == 0).all() and (plain["render"][lost] != 0).any()
    assert np.isnan(cut["iso"][1][lost]).all() and (cut["tf"][1][lost] == 0).all()
    assert not np.array_equal(cut["iso"][0], plain["iso"][0]) and not np.array_equal(cut["tf"][0], plain["tf"][0])
    # a channel frame refuses while planes are set; clearing the property restores every bit
    with pytest.raises(vr.VrError, match="clip planes") as e:
        vr.VolumeRender.renderChannels([r])
    assert e.value.code == 5
    with pytest.raises(TypeError, match="n x 4"):
        r.ClipPlanes = np.zeros((3, 3))
    r.ClipPlanes = []
    again = {"render": r.render(), "sum": r.renderProjection("sum", aux=True)}
    assert mex.get_clip(r.objectHandle).shape == (0, 4)
    assert np.array_equal(again["render"].view(np.uint32), plain["render"].view(np.uint32))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(again["sum"], plain["sum"]))
    assert len(vr.VolumeRender.renderChannels([r])) == 1
    r.delete()
