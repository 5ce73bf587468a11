"""The slice reference (tests/slice_ref.py) against facts that need no reference: on integer data an
axis slice through the voxel centres IS the indexed array, a full-thickness slab is numpy's reduction of
the planes, the inside test is the closed unit cube, and the special values follow the header's rules.
Each test states the counts it relies on, so that none passes on an empty set."""
import numpy as np
import pytest

import slice_ref as SR
from volume_renderer_amd import mex

F = np.float32
DIMS = (16, 12, 20)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@pytest.fixture(scope="module")
def ints():
    """16 x 12 x 20 of random uint8 values as float32: every lerp of the sampler is exact on them."""
    return np.asfortranarray(np.random.default_rng(17).integers(0, 256, DIMS, dtype=np.uint8).astype(F))


def plane_of(vol, axis, i):
    """Data indexed at plane i of `axis`: rows along the lower remaining dimension."""
    return np.take(vol, i, axis=axis)


def test_every_axis_slice_is_the_indexed_array(ints):
    count = 0
    for axis in range(3):
        for i in range(DIMS[axis]):
            s = SR.Slice.of(mex.slice_axis(DIMS, axis, i, 1))
            want = plane_of(ints, axis, i)
            assert (s.H, s.W) == want.shape
            for mode in (SR.MAX, SR.SUM):
                img, aux, lab = SR.render(ints, s, mode)
                assert np.array_equal(bits(img), bits(want)), (axis, i, mode)
                assert (aux == (0 if mode == SR.MAX else 1)).all() and np.isnan(lab).all()
            # the other orientation: rows and columns swapped gives the transpose
            t = SR.Slice(s.origin, s.dv, s.du, s.dw, s.W, s.H, 1)
            assert np.array_equal(bits(SR.render(ints, t, SR.MIN)[0]), bits(want.T)), (axis, i)
            count += 1
    assert count == 16 + 12 + 20


def test_coordinates_land_on_the_texel_for_many_sizes():
    """The fp32 coordinate fma(1/d, i, 0.5/d) lands on texel i after the 8-bit weight quantisation --
    cell i with weight 0, or cell i - 1 with weight 1 (the lerp a + 1 * (b - a) is exact on integers) --
    for every voxel i of every d checked: 0 misses."""
    misses = total = 0
    for d in list(range(1, 300)) + [511, 512, 1000, 1023, 1024, 2047, 4096, 8191]:
        i = np.arange(d, dtype=F)
        q = SR.fma(F(1.0 / d), i, F(0.5 / d))
        xb = (q * F(d) - F(0.5)).astype(F)
        fl = np.floor(xb)
        w = np.rint((xb - fl) * F(256)) * F(1 / 256)
        hit = ((fl == i) & (w == 0)) | ((fl == i - 1) & (w == 1))
        misses += int((~hit).sum())
        total += d
    assert total > 60000 and misses == 0


def test_full_thickness_slabs_are_numpys_reductions(ints):
    for axis in range(3):
        d = DIMS[axis]
        s = SR.Slice.of(mex.slice_axis(DIMS, axis, (d - 1) / 2, d))
        assert s.n == d
        planes = [plane_of(ints, axis, i) for i in range(d)]
        acc = np.zeros_like(planes[0])
        for p in planes:
            acc = (acc + p).astype(F)  # the sequential fp32 sum (exact here: integers below 2^24)
        img, aux, _ = SR.render(ints, s, SR.SUM)
        assert np.array_equal(bits(img), bits(acc)) and (aux == d).all()
        img, aux, _ = SR.render(ints, s, SR.MAX)
        assert np.array_equal(bits(img), bits(ints.max(axis=axis)))
        assert np.array_equal(aux, ints.argmax(axis=axis).astype(F))  # (argmax: the first occurrence)
        img, aux, _ = SR.render(ints, s, SR.MIN)
        assert np.array_equal(bits(img), bits(ints.min(axis=axis)))
        assert np.array_equal(aux, ints.argmin(axis=axis).astype(F))
        # ties exist, so that the first-occurrence rule is exercised: 256 values over d >= 12 samples
        assert (np.sort(ints, axis=axis).take(-1, axis=axis) == np.sort(ints, axis=axis).take(-2, axis=axis)).any()


def test_an_oblique_plane_is_nan_exactly_outside_the_box(ints):
    s = SR.Slice.of(mex.slice_oblique(DIMS, [1, 1, 1], [0.5, 0.45, 0.55], [1, 0.6, -0.4], [0, 0, 1], 0.43, 37, 41, 1))
    img, aux, _ = SR.render(ints, s, SR.MAX)
    # the inside test restated in float64 (products of floats are exact there)
    y, x = np.meshgrid(np.arange(s.H, dtype=np.float64), np.arange(s.W, dtype=np.float64), indexing="ij")
    q = [np.float64(s.origin[j]) + np.float64(s.du[j]) * x + np.float64(s.dv[j]) * y for j in range(3)]
    ins = np.ones((s.H, s.W), bool)
    margin = np.inf
    for c in q:
        ins &= (c >= 0) & (c <= 1)
        margin = min(margin, np.abs(c).min(), np.abs(c - 1).min())
    assert margin > 1e-5  # no pixel so close to a face that fp32 and fp64 could disagree
    share = ins.mean()
    assert 0.2 <= share <= 0.8, share
    assert np.array_equal(np.isnan(img), ~ins) and np.array_equal(np.isnan(aux), ~ins)
    # it leaves the box on two sides at least: outside pixels in the first and in the last row or column
    edges = [~ins[0], ~ins[-1], ~ins[:, 0], ~ins[:, -1]]
    assert sum(bool(e.any()) for e in edges) >= 2
    assert np.isfinite(img[ins]).all()


def test_the_unit_cube_is_closed(ints):
    up, dn = np.nextafter(F(1), F(2)), np.nextafter(F(0), F(-1))
    z = np.zeros(3, F)
    for j in range(3):
        for q, want in ((F(0), True), (F(1), True), (-F(0), True), (up, False), (dn, False), (F(np.nan), False)):
            o = np.full(3, 0.5, F)
            o[j] = q
            for mode in (SR.MAX, SR.MIN, SR.SUM):
                img, aux, _ = SR.render(ints, SR.Slice(o, z, z, z, 1, 1, 1), mode)
                assert np.isnan(img[0, 0]) != want, (j, q, mode)
                assert aux[0, 0] == (1 if mode == SR.SUM else 0) if want else (aux[0, 0] == 0 or np.isnan(aux[0, 0]))
    # outside samples are skipped, not clamped: a slab that starts outside counts only the inside ones
    s = SR.Slice([0.5, 0.5, -0.26], z, z, [0, 0, 0.25], 1, 1, 7)  # q2 = -0.26, -0.01, 0.24, .. 0.99, 1.24
    img, aux, _ = SR.render(ints, s, SR.SUM)
    assert aux[0, 0] == 4
    assert SR.render(ints, s, SR.MAX)[1][0, 0] >= 2  # the winner's k is the slab index, not a count


def test_special_voxels():
    z = np.zeros(3, F)
    centre = lambda n=1, dw=z: SR.Slice([0.5, 0.5, 0.5], z, z, dw, 1, 1, n)  # noqa: E731
    const = lambda v: np.full((3, 3, 3), v, F)  # noqa: E731
    # -0: the pixel is m + 0.0f = +0 for both extrema; the sum of one -0 sample is 0 + -0 = +0
    for mode in (SR.MAX, SR.MIN, SR.SUM):
        img, aux, _ = SR.render(const(-0.0), centre(), mode)
        assert bits(img)[0, 0] == 0 and aux[0, 0] == (1 if mode == SR.SUM else 0)
    # all +inf: the minimum has no winner (inf < inf never holds -- and the sampler's lerp of two
    # infinities, inf + w * (inf - inf), is NaN anyway, which never wins either extremum); the sum is
    # NaN with every sample counted
    for v in (np.inf, -np.inf):
        for mode in (SR.MIN, SR.MAX):
            img, aux, _ = SR.render(const(v), centre(3), mode)
            assert np.isnan(img[0, 0]) and np.isnan(aux[0, 0])
        img, aux, _ = SR.render(const(v), centre(3), SR.SUM)
        assert np.isnan(img[0, 0]) and aux[0, 0] == 3
    # a NaN sample never wins an extremum and poisons the sum, and it still counts
    # (a NaN voxel makes every sample whose cell touches it NaN, whatever the weight: w * (NaN - a) + a)
    v = np.full((3, 3, 6), 1.0, F)
    v[:, :, 5] = np.nan
    slab = SR.Slice([0.5, 0.5, 0.5 / 6], z, z, [0, 0, 1 / 6], 1, 1, 6)  # the six voxel centres along z
    img, aux, _ = SR.render(v, slab, SR.MAX)
    assert img[0, 0] == 1 and aux[0, 0] == 0
    img, aux, _ = SR.render(v, slab, SR.MIN)
    assert img[0, 0] == 1 and aux[0, 0] == 0
    img, aux, _ = SR.render(v, slab, SR.SUM)
    assert np.isnan(img[0, 0]) and aux[0, 0] == 6
    only_nan = SR.render(const(np.nan), centre(2), SR.MIN)
    assert np.isnan(only_nan[0][0, 0]) and np.isnan(only_nan[1][0, 0])
    # an unbound texture reads 0 inside and is skipped outside
    img, aux, _ = SR.render(None, SR.Slice([0.5, 0.5, 0.5], [0.5, 0, 0], z, z, 1, 3, 1), SR.SUM)
    assert img[0, 0] == 0 and img[0, 1] == 0 and np.isnan(img[0, 2]) and list(aux[0]) == [1, 1, 0]


def test_label_plane_follows_the_nearest_rule(ints):
    lab = np.asfortranarray(np.random.default_rng(3).integers(0, 7, DIMS, dtype=np.uint8))
    hits = 0
    for axis in range(3):
        i = DIMS[axis] // 3
        s = SR.Slice.of(mex.slice_axis(DIMS, axis, i + 0.75, 4))  # centre sample kc = 1: i + 0.75 - 1.5 + 1
        got = SR.render(ints, s, SR.MAX, labels=lab)[2]
        # the centre sample (n even) lies a quarter voxel above the centre of plane i: still voxel i
        s3 = SR.Slice.of(mex.slice_axis(DIMS, axis, i, 3))  # n odd: the centre sample is plane i itself
        assert np.array_equal(got, SR.render(ints, s3, SR.MAX, labels=lab)[2])
        want = plane_of(lab, axis, i).astype(F)
        assert np.array_equal(got, want), axis
        hits += got.size
    assert hits == 12 * 20 + 16 * 20 + 16 * 12
    # another label resolution than the volume's: the label volume's own dims index it
    half = lab[::2, ::2, ::2]
    s = SR.Slice.of(mex.slice_axis(DIMS, 2, 6, 1))
    got = SR.render(ints, s, SR.MAX, labels=half)[2]
    assert np.array_equal(got, np.repeat(np.repeat(half[:, :, 3], 2, 0), 2, 1).astype(F))
