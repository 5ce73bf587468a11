"""CPU test of tests/histogram_ref.py, the numpy restatement the GPU tests compare against: on
integer-valued data with integer limits, where every float32 step is exact, it must equal numpy's own
np.histogram and np.bincount; its keys order the floats as IEEE totalOrder; its clip rule is the plane test."""
import numpy as np

import histogram_ref as HR

F = np.float32


def test_integer_data_equals_numpy_histogram_and_bincount():
    rng = np.random.default_rng(3)
    data = np.asfortranarray(rng.integers(0, 9, (13, 7, 5)).astype(F))
    counts, s = HR.histogram(data, 8, (0, 8))
    want, _ = np.histogram(data, bins=8, range=(0, 8))  # the last bin closed, as histcounts
    assert np.array_equal(counts[0], want.astype(np.uint64))
    bc = np.bincount(data.astype(np.int64).reshape(-1), minlength=9)
    assert np.array_equal(counts[0][:7], bc[:7].astype(np.uint64)) and counts[0][7] == bc[7] + bc[8]
    assert s["total"][0] == data.size and s["below"][0] == s["above"][0] == s["nan"][0] == s["ninf"][0] == 0
    assert s["min"][0] == data.min() and s["max"][0] == data.max() and s["sum"][0] == data.sum(dtype=np.float64)
    # limits inside the data: the rest is below / above
    counts, s = HR.histogram(data, 4, (2, 6))
    want, _ = np.histogram(data, bins=4, range=(2, 6))
    assert np.array_equal(counts[0], want.astype(np.uint64))
    assert s["below"][0] == (data < 2).sum() and s["above"][0] == (data > 6).sum()


def test_rows_by_label_equal_numpy_on_the_masked_data():
    rng = np.random.default_rng(4)
    data = np.asfortranarray(rng.integers(0, 17, (11, 6, 4)).astype(F))
    labels = np.asfortranarray(rng.integers(0, 9, data.shape, dtype=np.uint8))
    counts, s = HR.histogram(data, 16, (0, 16), labels, 3, 4)
    assert counts.shape == (5, 16)
    for r, l in enumerate(range(3, 7)):
        want, _ = np.histogram(data[labels == l], bins=16, range=(0, 16))
        assert np.array_equal(counts[r], want.astype(np.uint64)) and s["total"][r] == (labels == l).sum()
    other = (labels < 3) | (labels > 6)
    want, _ = np.histogram(data[other], bins=16, range=(0, 16))
    assert np.array_equal(counts[4], want.astype(np.uint64)) and s["total"].sum() == data.size
    # a range that wraps nothing: labels 250..255 and the rest
    assert np.array_equal(HR.rows_of(np.uint8([0, 249, 250, 255]), 250, 6), [6, 6, 0, 5])


def test_special_values_and_total_order():
    v = F([np.nan, -np.inf, -1.0, -0.0, 0.0, 1.0, np.inf])
    k = HR.keys(v[1:])
    assert (np.diff(k.astype(np.int64)) > 0).all() and k.min() > 0 and k.max() < 0xFFFFFFFF
    for x, kk in zip(v[1:], k):
        assert HR.unkey(kk).view(np.uint32) == x.view(np.uint32)
    assert list(HR.bins(v, 4, (-1, 1))) == [HR.NAN, HR.BELOW, 0, 2, 2, 3, HR.ABOVE]
    counts, s = HR.histogram(v.reshape(7, 1, 1), 4, (-1, 1))
    assert s["nan"][0] == 1 and s["ninf"][0] == 2 and s["below"][0] == 1 and s["above"][0] == 1 and s["total"][0] == 7
    assert np.isneginf(s["min"][0]) and np.isposinf(s["max"][0]) and s["sum"][0] == 0.0
    zeros = np.asfortranarray(F([0.0, -0.0, 0.0]).reshape(3, 1, 1))
    _, s = HR.histogram(zeros, 2, (-1, 1))
    assert np.signbit(s["min"][0]) and not np.signbit(s["max"][0])
    _, s = HR.histogram(np.full((2, 1, 1), np.nan, F), 2, (0, 1))
    assert np.isnan(s["min"][0]) and np.isnan(s["max"][0]) and s["nan"][0] == 2
    counts, s = HR.histogram(None, 3, (0, 1), None, 0, 2)
    assert counts.shape == (3, 3) and not counts.any() and not s["total"].any() and np.isnan(s["min"]).all()


def test_clip_rule_is_the_plane_test_at_voxel_centres():
    keep = HR.clip_keep((4, 2, 2), F([[1, 0, 0, -0.5]]))  # q0 >= 0.5: i0 = 2, 3
    assert np.array_equal(keep.reshape((4, 2, 2), order="F")[:, 0, 0], [False, False, True, True]) and keep.sum() == 8
    box = F([[1, 0, 0, -0.25], [-1, 0, 0, 0.75], [0, 1, 0, -0.25], [0, -1, 0, 0.75], [0, 0, 1, -0.25], [0, 0, -1, 0.75]])
    keep = HR.clip_keep((8, 8, 8), box).reshape((8, 8, 8), order="F")
    assert keep.sum() == 64 and keep[2:6, 2:6, 2:6].all()
    assert not HR.clip_keep((3, 3, 3), F([[np.nan, 0, 0, 0]])).any()
