"""The 'volume_histogram' command at the MATLAB boundary: the C++ MEX adaptor (mex/volumeRender_mex.cpp
against tests/mexstub/) and the Python path -- their argument checks without a device, and on a device the
adaptor's outputs against the ctypes path and the class method VolumeRender.histogram on top of the command.
mex/matlab/volumeHistogram.m itself is not run: there is no MATLAB here."""
import numpy as np
import pytest

import histogram_ref as HR
import mexsim as M

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import mex  # noqa: E402

F = np.float32
ARGV = ["emission", np.float64(16), F([0, 1]), np.int32([0, 0]), False]


def _stamped(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def test_volume_histogram_argument_checks_of_the_adaptor():
    h = np.uint64(1)
    with pytest.raises(M.MexError, match="insufficient parameter!"):
        M.call("volumeRender", 2, "volume_histogram", h, *ARGV[:4])  # no use_clip
    with pytest.raises(M.MexError, match="too many input arguments"):
        M.call("volumeRender", 2, "volume_histogram", h, *ARGV, 0.0)
    with pytest.raises(M.MexError, match="Too many output arguments."):
        M.call("volumeRender", 3, "volume_histogram", h, *ARGV)
    for lim in (np.float64([0, 1]), F([0, 1, 2]), F([0])):
        with pytest.raises(M.MexError, match="limits must be a single vector"):
            M.call("volumeRender", 1, "volume_histogram", h, "emission", np.float64(16), lim, *ARGV[3:])
    for lab in (np.float64([0, 0]), np.int32([0]), np.int32([0, 1, 2])):
        with pytest.raises(M.MexError, match="labels must be an int32 vector"):
            M.call("volumeRender", 1, "volume_histogram", h, *ARGV[:3], lab, False)
    with pytest.raises(M.MexError, match="nbins must be a real scalar"):
        M.call("volumeRender", 1, "volume_histogram", h, "emission", np.float64([4, 4]), *ARGV[2:])
    # values the library refuses, before the handle
    for nb in (np.int32(0), np.float64(2.5), np.float64(4097)):
        with pytest.raises(M.MexError, match="bins"):
            M.call("volumeRender", 1, "volume_histogram", h, "emission", nb, *ARGV[2:])
    for src in ("emision", np.float64(3), np.float64(0.5)):
        with pytest.raises(M.MexError, match="unknown source"):
            M.call("volumeRender", 1, "volume_histogram", h, src, *ARGV[1:])
    for lim in (F([1, 0]), F([0, np.inf]), F([np.nan, 1])):
        with pytest.raises(M.MexError, match="limits must be finite"):
            M.call("volumeRender", 1, "volume_histogram", h, *ARGV[:2], lim, *ARGV[3:])
    for lab in (np.int32([-1, 2]), np.int32([250, 7]), np.int32([0, 257])):
        with pytest.raises(M.MexError, match="label_first"):
            M.call("volumeRender", 1, "volume_histogram", h, *ARGV[:3], lab, False)
    with pytest.raises(M.MexError, match="rows \\* nbins"):
        M.call("volumeRender", 1, "volume_histogram", h, "emission", np.float64(4096), F([0, 1]), np.int32([0, 3]), False)
    with pytest.raises(M.MexError, match="use_clip"):
        M.call("volumeRender", 1, "volume_histogram", h, *ARGV[:4], np.float64(2))
    for src, clip in (("emission", False), (np.float64(2), True), ("absorption", np.float64(1)), (np.int32(1), np.int32(0))):
        with pytest.raises(M.MexError, match="Handle not valid."):
            M.call("volumeRender", 2, "volume_histogram", h, src, np.int32(47), F([-1, 1]), np.int32([0, 256]), clip)


def test_volume_histogram_argument_checks_of_the_python_path():
    h = np.uint64(1)
    with pytest.raises(vr.VrError, match="insufficient parameter!"):
        vr.volumeRender("volume_histogram", h, *ARGV[:4])
    with pytest.raises(vr.VrError, match="too many input arguments"):
        vr.volumeRender("volume_histogram", h, *ARGV, 0.0)
    with pytest.raises(vr.VrError, match="limits must be a single vector"):
        vr.volumeRender("volume_histogram", h, "emission", 16, np.float64([0, 1]), np.int32([0, 0]), False)
    with pytest.raises(vr.VrError, match="labels must be an int32 vector"):
        vr.volumeRender("volume_histogram", h, "emission", 16, F([0, 1]), [0, 0], False)
    with pytest.raises(vr.VrError, match="unknown slice source"):
        vr.volumeRender("volume_histogram", h, "emision", *ARGV[1:])
    for bad, what in (((1, 0), "bins"), ((1, 4097), "bins"), ((2, F([1, 0])), "limits"), ((3, np.int32([250, 7])), "label_first"),
                      ((4, 2), "use_clip"), ((0, 3), "unknown source")):
        a = list(ARGV)
        a[bad[0]] = bad[1]
        with pytest.raises(vr.VrError, match=what) as e:
            vr.volumeRender("volume_histogram", h, *a)
        assert e.value.code == 1
    with pytest.raises(vr.VrError, match="Handle not valid.") as e:
        vr.volumeRender("volume_histogram", h, "reflection", np.int32(47), F([-1, 1]), np.int32([0, 256]), True)
    assert e.value.code == 2
    q = mex.make_histogram(1, 7, F([0, 2]), np.int32([3, 5]), True)
    assert (q.source, q.nbins, q.lim[0], q.lim[1], q.label_first, q.label_count, q.use_clip) == (1, 7, 0, 2, 3, 5, 1)
    assert mex.histogram_rows(q) == 6 and mex.histogram_rows(mex.make_histogram("emission", 7, F([0, 2]))) == 1


@pytest.mark.gpu
def test_volume_histogram_through_mexfunction_equals_python_path_and_reference():
    rng = np.random.default_rng(21)
    data = np.asfortranarray(rng.integers(0, 9, (14, 11, 9)).astype(F))
    lab = np.asfortranarray(rng.integers(0, 7, data.shape, dtype=np.uint8))
    em, re = _stamped(data, 11), _stamped(np.float32(1.0), 12)
    argv = ["emission", np.float64(8), F([0, 8]), np.int32([2, 3]), False]
    (h,) = M.call("volumeRender", 1, "new")
    M.call("volumeRender", 0, "sync_volumes", h, np.uint64(0), em, re, em)
    M.call("volumeRender", 0, "sync_labels", h, lab)
    counts, summary = M.call("volumeRender", 2, "volume_histogram", h, *argv)
    (only,) = M.call("volumeRender", 1, "volume_histogram", h, np.float64(0), np.int32(8), F([0, 8]), np.int32([2, 3]),
                     np.float64(0))
    M.call("volumeRender", 0, "delete", h)
    hp = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hp, np.uint64(0), em, re, em)
    vr.volumeRender("sync_labels", hp, lab)
    pc, ps = vr.volumeRender("volume_histogram", hp, *argv)
    vr.volumeRender("delete", hp)
    wc, ws = HR.histogram(data, 8, (0, 8), lab, 2, 3)
    for c in (counts, only, pc):
        assert c.dtype == np.uint64 and c.shape == (8, 4) and np.array_equal(c, wc.T)
    for s in (summary, ps):
        assert s.dtype == np.float64 and s.shape == (4, 8)
        for i, k in enumerate(HR.SUMMARY):  # integer data: the sum is exact too
            assert np.array_equal(s[:, i], ws[k].astype(np.float64)), k
    assert wc.sum() == data.size and (wc.sum(axis=1) > 0).all()


@pytest.mark.gpu
def test_histogram_method(counter_clock):
    r = vr.VolumeRender()
    rng = np.random.default_rng(2)
    u8 = np.asfortranarray(rng.integers(0, 200, (14, 11, 9), dtype=np.uint8))
    data = u8.astype(F)
    r.VolumeEmission = vr.Volume(data)
    r.VolumeAbsorption = r.VolumeEmission
    counts, s = r.histogram(10, [0, 200])
    wc, ws = HR.histogram(data, 10, (0, 200))
    assert counts.shape == (10, 1) and np.array_equal(counts, wc.T) and s["total"][0] == data.size
    assert s["min"].dtype == np.float32 and s["min"][0] == data.min() and s["max"][0] == data.max()
    assert s["sum"][0] == data.sum(dtype=np.float64)
    # labels and gains: the histogram of what the renderer holds; clip planes: the kept voxels only
    lab = np.asfortranarray(rng.integers(0, 3, data.shape, dtype=np.uint8))
    r.VolumeLabels = lab
    r.LabelGains = [1, 0.5, 0]
    r.ClipPlanes = [[1, 0, 0, -0.5]]
    held = mex.label_gain_host(data, lab, F([1, 0.5, 0]))
    counts, s = r.histogram(10, [0, 200], labels=(0, 3), use_clip=True)
    wc, ws = HR.histogram(held, 10, (0, 200), lab, 0, 3, F([[1, 0, 0, -0.5]]))
    assert counts.shape == (10, 4) and np.array_equal(counts, wc.T)
    for k in HR.SUMMARY:
        assert np.array_equal(s[k], ws[k], equal_nan=True), k
    assert s["total"].sum() == 7 * 11 * 9 and s["total"][3] == 0 and np.isnan(s["min"][3])
    counts, s = r.histogram(10, [0, 200], source="absorption")
    assert np.array_equal(counts, HR.histogram(held, 10, (0, 200))[0].T)  # the alias follows the gains
    r.delete()
