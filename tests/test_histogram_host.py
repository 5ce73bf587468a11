"""The volume histogram's host side that needs no device (include/vrhip.h vr_volume_histogram): the
argument checks, which come before the handle, and vr_histogram_bin_host -- the inline function the kernel
evaluates -- against the numpy restatement of tests/histogram_ref.py.  The histograms themselves need a
device: tests/test_gpu_histogram.py."""
import ctypes

import numpy as np
import pytest

import histogram_ref as HR
from volume_renderer_amd import _lib, mex

F = np.float32
FMAX = np.finfo(F).max


def good():
    return mex.make_histogram("absorption", 64, F([-0.5, 0.5]), np.int32([3, 5]), 1)


def _lim(q, lo, hi):
    q.lim[0], q.lim[1] = lo, hi


BAD = {
    "source 3": lambda q: setattr(q, "source", 3),
    "source -1": lambda q: setattr(q, "source", -1),
    "nbins 0": lambda q: setattr(q, "nbins", 0),
    "nbins -1": lambda q: setattr(q, "nbins", -1),
    "nbins 4097": lambda q: setattr(q, "nbins", 4097),
    "lo nan": lambda q: _lim(q, np.nan, 1),
    "hi nan": lambda q: _lim(q, 0, np.nan),
    "lo -inf": lambda q: _lim(q, -np.inf, 1),
    "hi inf": lambda q: _lim(q, 0, np.inf),
    "lo == hi": lambda q: _lim(q, 0.25, 0.25),
    "lo > hi": lambda q: _lim(q, 1, 0),
    "hi - lo overflows": lambda q: _lim(q, -FMAX, FMAX),
    "label_first -1": lambda q: setattr(q, "label_first", -1),
    "label_first 256": lambda q: (setattr(q, "label_first", 256), setattr(q, "label_count", 0)),
    "label_count -1": lambda q: setattr(q, "label_count", -1),
    "label_count 257": lambda q: (setattr(q, "label_first", 0), setattr(q, "label_count", 257)),
    "first + count 257": lambda q: (setattr(q, "label_first", 250), setattr(q, "label_count", 7)),
    "rows * nbins 12289": lambda q: (setattr(q, "label_count", 0), setattr(q, "nbins", 4096),
                                     setattr(q, "label_count", 3)),  # 4 x 4096
    "257 rows x 48 bins": lambda q: (setattr(q, "label_first", 0), setattr(q, "label_count", 256),
                                     setattr(q, "nbins", 48)),
    "use_clip 2": lambda q: setattr(q, "use_clip", 2),
    "use_clip -1": lambda q: setattr(q, "use_clip", -1),
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_histogram_validation_comes_before_the_handle(case):
    L = _lib.lib()
    q = good()
    BAD[case](q)
    counts = np.zeros(257 * 4096, np.uint64)
    for h in (ctypes.c_void_p(12345), None):
        assert L.vr_volume_histogram(h, ctypes.byref(q), counts.ctypes.data, None) == 1, case
        assert b"histogram" in L.vr_last_error() and b"Handle" not in L.vr_last_error()
        assert L.vr_volume_histogram_device(h, ctypes.byref(q), counts.ctypes.data, None, None) == 1, case
    assert not counts.any()


def test_null_query_null_counts_and_the_handle_check():
    L = _lib.lib()
    h = ctypes.c_void_p(12345)
    counts = np.zeros(257 * 47, np.uint64)
    assert L.vr_volume_histogram(h, None, counts.ctypes.data, None) == 1 and b"NULL" in L.vr_last_error()
    assert L.vr_volume_histogram_device(h, None, counts.ctypes.data, None, None) == 1
    q = good()
    assert L.vr_volume_histogram(h, ctypes.byref(q), None, None) == 1 and b"counts is NULL" in L.vr_last_error()
    assert L.vr_volume_histogram_device(h, ctypes.byref(q), None, None, None) == 1
    # valid arguments reach the handle check, the limits of every range included
    for source, nbins, first, count, clip in ((0, 1, 0, 0, 0), (2, 4096, 255, 0, 1), (1, 4096, 0, 2, 0), (0, 47, 0, 256, 1),
                                              (1, 2048, 250, 5, 0), (0, 12288 // 7, 255, 1, 1)):
        q = good()
        q.source, q.nbins, q.label_first, q.label_count, q.use_clip = source, nbins, first, count, clip
        assert L.vr_volume_histogram(h, ctypes.byref(q), counts.ctypes.data, None) == 2, (source, nbins, first, count)
        assert b"Handle not valid" in L.vr_last_error()
        assert L.vr_volume_histogram_device(None, ctypes.byref(q), counts.ctypes.data, None, None) == 2
    q = good()
    _lim(q, -FMAX, 0)  # hi - lo finite at the edge
    assert L.vr_volume_histogram(h, ctypes.byref(q), counts.ctypes.data, None) == 2
    assert ctypes.sizeof(_lib.VrHistogram) == 32 and ctypes.sizeof(_lib.VrHistRow) == 56 == mex.HIST_ROW_DTYPE.itemsize
    assert _lib.VR_HIST_MAX_BINS == 4096 and _lib.VR_HIST_MAX_CELLS == 12288


def values(nbins, lo, hi):
    """10^4 random floats around [lo, hi] plus the values where a class changes: the limits and their
    neighbours, every bin edge (as computed in double and in float, with neighbours), +-0, +-inf, NaN."""
    rng = np.random.default_rng(nbins)
    lo, hi = F(lo), F(hi)
    with np.errstate(all="ignore"):  # (the widest limits overflow on purpose)
        return _values(rng, nbins, lo, hi)


def _values(rng, nbins, lo, hi):
    w = float(hi) - float(lo)
    v = [(rng.random(10000, dtype=F) * F(1.5 * w) + F(float(lo) - 0.25 * w)).astype(F)]
    edge = [lo, hi] + [F(float(lo) + w * k / nbins) for k in range(nbins + 1)] + \
           [F(lo + F(hi - lo) * F(k) / F(nbins)) for k in range(nbins + 1)]
    edge = np.array(edge, F)
    v += [edge, np.nextafter(edge, F(np.inf)), np.nextafter(edge, F(-np.inf))]
    v.append(F([0.0, -0.0, np.inf, -np.inf, np.nan, FMAX, -FMAX, np.finfo(F).tiny, -np.finfo(F).tiny]))
    return np.concatenate(v)


@pytest.mark.parametrize("nbins", [1, 2, 7, 256, 4096])
def test_bin_host_equals_the_reference(nbins):
    classes = set()
    for lo, hi in ((0.0, 1.0), (-0.5, 0.37), (-3.0, 1021.0), (1e-3, 2e-3), (-FMAX, 0.0)):
        v = values(nbins, lo, hi)
        got = mex.histogram_bin_host(v, nbins, (lo, hi))
        want = HR.bins(v, nbins, (lo, hi))
        assert got.dtype == np.int32 and np.array_equal(got, want), (nbins, lo, hi, v[got != want][:5])
        assert got.max() == nbins - 1 and got[np.flatnonzero(v == F(hi))].min() == nbins - 1
        assert got[np.flatnonzero(v == F(lo))].max() == 0
        classes |= set(np.unique(got[got < 0]))
        if (lo, hi) == (0.0, 1.0):  # (every edge k / nbins is in the list: no bin stays empty)
            assert set(np.unique(got[got >= 0])) == set(range(nbins))
    assert classes == {HR.BELOW, HR.ABOVE, HR.NAN}


def test_bin_host_argument_checks():
    L = _lib.lib()
    v, out = F([0.5]), np.zeros(1, np.int32)
    lim = (ctypes.c_float * 2)(0, 1)
    assert L.vr_histogram_bin_host(v.ctypes.data, 1, 4, lim, out.ctypes.data) == 0 and out[0] == 2
    assert L.vr_histogram_bin_host(None, 1, 4, lim, out.ctypes.data) == 1
    assert L.vr_histogram_bin_host(v.ctypes.data, 1, 4, lim, None) == 1
    assert L.vr_histogram_bin_host(v.ctypes.data, 1, 4, None, out.ctypes.data) == 1
    assert L.vr_histogram_bin_host(v.ctypes.data, 1, 0, lim, out.ctypes.data) == 1
    assert L.vr_histogram_bin_host(v.ctypes.data, 1, 4097, lim, out.ctypes.data) == 1
    assert L.vr_histogram_bin_host(v.ctypes.data, 1, 4, (ctypes.c_float * 2)(1, 1), out.ctypes.data) == 1
    assert L.vr_histogram_bin_host(None, 0, 4, lim, None) == 0
    assert mex.histogram_bin_host(F([]), 4, (0, 1)).size == 0
