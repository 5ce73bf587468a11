"""The 'sync_labels' and 'set_label_gains' commands at the MATLAB boundary on the GPU: labels and gains
set through the C++ MEX adaptor (mex/volumeRender_mex.cpp against tests/mexstub/) render exactly as
through the ctypes path, and the VolumeLabels / LabelGains properties of the Python VolumeRender mirror
reproduce an example4-style fade (examples/example4.m: the masked region times factor(i), frame by
frame) against the renders of the host-rewritten volumes.  The count and type checks of the commands
need no device: tests/test_labels_host.py."""
import numpy as np
import pytest

import mexsim as M
import oracle as O

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import mex  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
R = np.flip(O.rotation(125, 25, 0), 0).astype(F)
ARGV = [False, False, F([1.5, 0.4, 0.6]), F([1, 1, 1]), np.uint64([40, 52]), R, F([0, 3, 6]), F(0.9), F([1, 1, 0])]
GAINS = F([1, 0.35, 0])


def _stamped(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def _labels(shape):
    lab = np.zeros(shape, np.uint8, order="F")
    lab[:, shape[1] // 2:, :] = 1  # example4's mask: a half-space
    lab[:shape[0] // 3, :shape[1] // 3, :shape[2] // 3] = 2
    return lab


def _em2(em, labels, gains):
    table = np.ones(256, F)
    table[:len(gains)] = F(gains)
    return np.asfortranarray((em * table[labels]).astype(F))


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_labels_through_mexfunction_equal_the_python_path():
    data = O.shell_volume(24)
    labels = _labels(data.shape)
    em, re = _stamped(data, 11), _stamped(np.float32(1.0), 12)
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    (plain,) = M.call("volumeRender", 1, "render", h, *ARGV)
    assert M.call("volumeRender", 0, "sync_labels", h, labels) == []
    assert M.call("volumeRender", 0, "set_label_gains", h, GAINS) == []
    assert _same(mex.get_label_gains(h), GAINS)  # (one library: the ctypes path reads the same handle)
    (got,) = M.call("volumeRender", 1, "render", h, *ARGV)
    gsum = M.call("volumeRender", 2, "render_projection", h, *ARGV, "sum")
    M.call("volumeRender", 0, "set_label_gains", h, GAINS.reshape(-1, 1))  # a column vector: the same table
    assert _same(mex.get_label_gains(h), GAINS)
    for clear_cmd, clear in (("set_label_gains", np.zeros((0, 0), F)), ("set_label_gains", False),
                             ("sync_labels", np.zeros((0, 0), np.uint8)), ("sync_labels", False)):
        M.call("volumeRender", 0, "sync_labels", h, labels)
        M.call("volumeRender", 0, "set_label_gains", h, GAINS)
        M.call("volumeRender", 0, clear_cmd, h, clear)
        (again,) = M.call("volumeRender", 1, "render", h, *ARGV)
        assert _same(again, plain), (clear_cmd, clear)
    M.call("volumeRender", 0, "delete", h)

    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    vr.volumeRender("sync_labels", hp, labels)
    vr.volumeRender("set_label_gains", hp, GAINS)
    want = vr.volumeRender("render", hp, *ARGV)
    wsum = vr.volumeRender("render_projection", hp, *ARGV, "sum")
    vr.volumeRender("delete", hp)
    hr = vr.volumeRender("new")
    e2 = _stamped(_em2(data, labels, GAINS), 11)
    vr.volumeRender("sync_volumes", hr, np.uint64(0), e2, re, e2)
    ref = vr.volumeRender("render", hr, *ARGV)
    vr.volumeRender("delete", hr)
    assert _same(got, want) and _same(got, ref) and all(_same(a, b) for a, b in zip(gsum, wsum))
    assert not _same(got, plain) and got.max() > 0


def _fade_renderer(data):
    r = vr.VolumeRender()
    r.FocalLength, r.DistanceToObject = 3.0, 6
    r.rotate(125, 25, 0)
    r.ImageResolution = [52, 40]
    v = vr.Volume(data)
    r.VolumeEmission = v
    r.VolumeAbsorption = v
    # (its own reflection volume, stamped by this test's clock: the class default carries the stamp of
    # whichever clock ran when the class was first used, and a reflection newer than TimeLastMemSync
    # re-points the emission slot at it, the reference's sync quirk)
    r.VolumeReflection = vr.Volume(1)
    r.FactorEmission = 1.5
    r.Color = [1, 1, 0]
    return r


def test_mirror_properties_reproduce_an_example4_fade(counter_clock):
    data = O.shell_volume(24)
    mask = _labels(data.shape) == 1
    factors = F([1.0, 0.5, 0.0])
    r = _fade_renderer(data)
    assert r.VolumeLabels is False and r.LabelGains.shape == (0,)
    plain = r.render()
    assert mex.get_label_gains(r.objectHandle).shape == (0,)
    r.VolumeLabels = mask.astype(np.uint8)
    frames, sums = [], []
    for f in factors:  # the movie: one scalar per frame, no volume crosses the host link
        r.LabelGains = [1, f]
        frames.append(r.render())
        assert _same(mex.get_label_gains(r.objectHandle), F([1, f]))
        sums.append(r.renderProjection("sum"))
    with pytest.raises(TypeError, match="LabelGains"):
        r.LabelGains = np.ones(257)
    r.VolumeLabels = False
    back = r.render()
    r.delete()
    for f, frame, s in zip(factors, frames, sums):
        d2 = np.array(data, order="F")
        d2[mask] = f * data[mask]  # example4.m: Data(logical(mask)) = factor(i) * Data(logical(mask))
        r2 = _fade_renderer(d2)
        want, wsum = r2.render(), r2.renderProjection("sum")
        r2.delete()
        assert _same(frame, want) and _same(s, wsum), f"factor {f}"
    assert _same(frames[0], plain) and _same(back, plain)
    assert not _same(frames[1], plain) and not _same(frames[2], frames[1])
