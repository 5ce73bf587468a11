"""CPU tests of the transfer-function render's reference and table lookup: vr_transfer_lookup_host
(the kernel's lookup, csrc/vr_transfer.h) equals the numpy lookup of tests/transfer_ref.py bit for bit,
and that reference, given a constant colormap equal to `color` and no alphamap, is the C oracle's
render bit for bit, sample counts included."""
import numpy as np
import pytest

import oracle as O
import projection_ref as PR
import transfer_ref as TR
import volume_renderer_amd as vr  # noqa: F401
from golden_cases import STAMP_LUT
from volume_renderer_amd import mex

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def coordinates(lo, hi, seed):
    rng = np.random.default_rng(seed)
    span = hi - lo
    special = [lo, hi, lo - span, hi + span, np.nextafter(F(lo), F(-np.inf)), np.nextafter(F(hi), F(np.inf)), 0.0, -0.0,
               np.nan, np.inf, -np.inf, 3e38, -3e38, 1e-45]
    rand = lo - 0.25 * span + 1.5 * span * rng.random(10000)
    return np.concatenate([F(special), rand.astype(F)])


@pytest.mark.parametrize("n", [2, 3, 7, 256, 257, 1024])
def test_host_lookup_equals_the_numpy_lookup(n):
    rng = np.random.default_rng(100 + n)
    for lim in ((0.0, 1.0), (-0.37, 2.9), (0.25, 0.2500001), (-1e30, 1e30)):
        lim = (F(lim[0]), F(lim[1]))
        table = np.asfortranarray((rng.random((n, 3)) * 4 - 2).astype(F))
        c = coordinates(float(lim[0]), float(lim[1]), n)
        got = mex.transfer_lookup_host(table, lim, c)
        assert got.shape == (3, c.size)
        for k in range(3):
            want = TR.lookup(table[:, k], lim, c)
            assert np.array_equal(bits(got[k]), bits(want)), (n, lim, k, int((bits(got[k]) != bits(want)).sum()))
        # the ends clamp, a NaN coordinate reads entry 0; the top end is the last segment at w = 1,
        # fma(1, T[n-1] - T[n-2], T[n-2]) (T[n-1] up to the slope's rounding)
        ends = mex.transfer_lookup_host(table[:, 0], lim, F([lim[0], lim[1], -np.inf, np.inf, np.nan]))
        top = PR.fma(F(1), table[n - 1, 0] - table[n - 2, 0], table[n - 2, 0])
        assert np.array_equal(bits(ends), bits(F([table[0, 0], top, table[0, 0], top, table[0, 0]])))
        assert abs(float(top) - float(table[n - 1, 0])) <= 2.0 ** -22
        vec = mex.transfer_lookup_host(table[:, 1], lim, c)
        assert np.array_equal(bits(vec), bits(got[1]))


@pytest.mark.parametrize("n", [2, 3, 7, 256, 257, 1024])
def test_constant_table_returns_its_constant(n):
    for const in (F(0.7), F(-3.25e-7), F(1e30), F(0)):
        c = coordinates(0.1, 0.9, n)
        got = mex.transfer_lookup_host(np.full(n, const, F), (F(0.1), F(0.9)), c)
        assert np.array_equal(bits(got), np.full(c.size, bits(const))), (n, const)


def test_kernel_exponential_restatement_is_within_an_ulp_of_glibc():
    """transfer_ref.exp_neg_kernel (the product's exp_neg_rn restated) against glibc's expf: both are
    within about half an ulp of exp(-x), so never more than one ulp apart (the share that differs is
    printed: 0.19 % of arguments drawn uniformly from the Taylor range); outside the range it is exp in
    double, rounded."""
    rng = np.random.default_rng(9)
    x = ((rng.random(200000) * 2 - 1) * 2.0 ** -7).astype(F)
    a, b = TR.exp_neg_kernel(x), TR.exp_neg_glibc(x)
    d = np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64))
    print(f"exp_neg_kernel != expf on {float((d != 0).mean()):.5f} of the arguments")
    assert d.max() <= 1 and (d == 0).any()
    assert np.array_equal(bits(TR.exp_neg_kernel(F([0.0, -0.0]))), bits(F([1, 1])))
    big = F([0.01, 1.5, -2.0, 80.0, np.inf])
    assert np.array_equal(bits(TR.exp_neg_kernel(big)), bits(np.exp(-big.astype(np.float64)).astype(F)))
    assert np.isnan(TR.exp_neg_kernel(F([np.nan]))[0])


def test_interior_entries_are_hit_exactly():
    """A coordinate at entry i of a power-of-two-spaced table reads T[i]; midway, the mean."""
    table = F([0, 1, 4, 9, 16])
    got = mex.transfer_lookup_host(table, (F(0), F(4)), F([0, 1, 2, 3, 4, 0.5, 2.5, -1, 7]))
    assert np.array_equal(got, F([0, 1, 4, 9, 16, 0.5, 6.5, 0, 16]))


@pytest.mark.parametrize("name,factors", [(n, None) for n in sorted(PR.FRAMES)] + [("hg2_compute_32", [1, 0.4, 40])],
                         ids=sorted(PR.FRAMES) + ["hg2_compute_32-opaque"])
def test_reference_with_a_constant_colormap_is_the_oracles_render(name, factors):
    S, h, sc, em = PR.scene_session(name)
    args = PR.frame_args(sc, PR.FRAMES[name], factors=factors)
    lights = sc["lights"]
    lut = O.OVolume(O.hg_lut(sc["lut"]), STAMP_LUT)
    want, total = S.render(h, lights, lut, *args)
    H, W = PR.FRAMES[name]
    ys, xs = np.mgrid[0:H, 0:W]
    _, steps = S.render(h, lights, lut, *args, pixels=(xs.reshape(-1), ys.reshape(-1)))
    tf = TR.make_tf(TR.constant_colormap(args[6], 3))
    ref = TR.transfer(S, h, tf, lights, lut, *args, double=False)
    assert want.max() > 0 and (ref["n"] > 0).any() and (ref["n"] == 0).any()
    assert np.array_equal(bits(ref["img"]), bits(want)), int((bits(ref["img"]) != bits(want)).sum())
    assert np.array_equal(ref["n"].reshape(-1), steps.astype(np.int64)) and int(ref["n"].sum()) == total
    # the alpha plane: 0 on a miss, within [0, 1], positive wherever the image is
    a = ref["alpha"]
    assert (a[~ref["hit"]] == 0).all() and (a >= 0).all() and (a <= 1).all()
    assert (a > 0).any() and (a[want.max(axis=2) > 0] > 0).all()
    if factors is not None:  # opaque enough for the early exit: those rays stop above the threshold
        early = a > args[5]
        assert early.any() and (ref["n"][early] < ref["n"].max()).all()
