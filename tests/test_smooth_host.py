"""Gaussian smoothing without a device (include/vrhip.h vr_set_smoothing): the weights of one axis
(vr_smooth_weights_host) against their formula, the value rule on the CPU (vr_smooth_host, the inline
functions the kernels evaluate, csrc/vr_smooth.h) against its numpy restatement (tests/smooth_ref.py) bit
for bit, and the argument checks that arrive before the handle.

The bit-exact comparisons take their weights from the product (mex.smooth_weights_host), so a libm that
rounds exp differently from Python's cannot fail them; the weights themselves are held to 1 ulp."""
import ctypes
import math

import numpy as np
import pytest

import smooth_ref as SR

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402

F = np.float32
SHAPES = [(37, 5, 3), (2, 3, 70), (33, 17, 1), (1, 1, 1), (300, 4, 3)]
SIGMAS = [(0.5, 0.5, 0.5), (1, 2, 0), (0, 0, 1.5), (6, 6, 6)]


def bits(a):
    return np.ascontiguousarray(np.asarray(a, F).reshape(-1, order="F")).view(np.uint32)


def bits_nan(a):
    return np.isnan(np.asarray(a, F).reshape(-1, order="F"))


def same_bits(a, b):
    """NaN positions equal, every other bit equal."""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), nan) and np.array_equal(bits(a)[~bits_nan(b)], bits(b)[~bits_nan(b)])


def volume(shape, seed=7):
    """Noise with the special values of the rule: a NaN, +-inf, -0, a subnormal -- each where the shape has
    room, apart from each other -- so that most of the volume stays finite at small sigma."""
    rng = np.random.default_rng(seed)
    v = np.asfortranarray((rng.random(shape, dtype=F) - F(0.25)) * F(3))
    flat = v.reshape(-1, order="F")
    n = flat.size
    for at, x in zip((n // 7, n // 3, n // 2, (2 * n) // 3, (5 * n) // 6), (np.nan, np.inf, -np.inf, -0.0, 1e-40)):
        if n > 6:
            flat[at] = F(x)
    return np.asfortranarray(flat.reshape(shape, order="F"))


# ---- weights ----------------------------------------------------------------------------------------------------

def test_weights_follow_the_formula():
    worst = 0.0
    for k in range(1, 601):
        sigma = F(0.01 * k)
        R, w = mex.smooth_weights_host(sigma)
        assert R == int(math.ceil(2.0 * float(sigma))) and w.shape == (2 * R + 1,) and w.dtype == np.float32
        assert np.array_equal(bits(w), bits(w[::-1])), f"sigma {sigma}: not symmetric"
        assert (w >= 0).all() and w[R] > 0
        s = float(np.sum(w.astype(np.float64)))
        worst = max(worst, abs(s - 1.0))
        assert abs(s - 1.0) <= 25 * 2.0 ** -24, f"sigma {sigma}: sum {s}"
        Rr, wr = SR.weights(sigma)
        assert Rr == R
        ulp = np.spacing(np.maximum(np.abs(wr), np.finfo(F).tiny).astype(F)).astype(np.float64)
        assert (np.abs(w.astype(np.float64) - wr.astype(np.float64)) <= ulp).all(), f"sigma {sigma}: beyond 1 ulp"
    print("largest |sum w - 1|:", worst)


def test_weights_edges_and_errors():
    R, w = mex.smooth_weights_host(0.0)
    assert R == 0 and np.array_equal(w, F([1]))
    R, w = mex.smooth_weights_host(_lib.VR_SMOOTH_MAX_SIGMA)
    assert R == 12 and w.size == 25 == _lib.VR_SMOOTH_MAX_TAPS
    R, w = mex.smooth_weights_host(0.01)  # the neighbours underflow: the centre alone
    assert R == 1 and np.array_equal(w, F([0, 1, 0]))
    for bad in (np.nan, -0.5, np.inf, -np.inf, np.nextafter(F(6), F(7))):
        with pytest.raises(vr.VrError, match="smoothing") as e:
            mex.smooth_weights_host(bad)
        assert e.value.code == 1
    L = _lib.lib()
    r = ctypes.c_int32(0)
    buf = np.zeros(25, F)
    assert L.vr_smooth_weights_host(1.0, None, buf.ctypes.data) == 1
    assert L.vr_smooth_weights_host(1.0, ctypes.byref(r), None) == 1


# ---- the value rule ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_smooth_host_is_the_rule_bit_for_bit(shape, sigma):
    v = volume(shape)
    got = mex.smooth_host(v, sigma)
    want = SR.smooth(v, sigma, weights_of=mex.smooth_weights_host)
    assert got.shape == v.shape and got.dtype == np.float32
    assert same_bits(got, want), f"{shape} {sigma}: {np.count_nonzero(bits(got) != bits(want))} voxels differ"
    filtered = any(s > 0 and d > 1 for s, d in zip(sigma, shape))
    if filtered and v.size > 6:
        assert np.isnan(want).any(), "the NaN and the infs of the sample left no trace"
        assert not same_bits(got, v)
    else:
        assert np.array_equal(bits(got), bits(v)), "every axis skipped: a bit-exact copy, NaN payloads included"


def test_special_values_follow_ieee():
    """One line, sigma 0.5 (R = 1), each special value alone among finite neighbours."""
    x = F([1, 2, np.nan, 3, 4, 5, np.inf, 6, 7, 8, -np.inf, 9, 1, 1, -0.0, -0.0, -0.0, -0.0, 1, 1e-40, 1e-40, 1e-40, 2])
    R, w = mex.smooth_weights_host(0.5)
    assert R == 1
    got = mex.smooth_host(x, (0.5, 0, 0))
    want = SR.smooth_axis(x, 0, R, w)
    assert same_bits(got, want)
    assert np.isnan(got[1:4]).all() and not np.isnan(got[[0, 4]]).any()  # a NaN spreads R to either side
    assert (got[5:8] == np.inf).all() and (got[9:12] == -np.inf).all()
    # all-(-0) window: w0 * -0 = -0, fma(w, -0, -0) = -0; the sign survives
    assert bits(got[15:17]).tolist() == [0x80000000, 0x80000000]
    # an all-subnormal window stays subnormal: nothing is flushed
    assert 0 < got[20] < np.finfo(F).tiny and same_bits(got[20:21], want[20:21])


@pytest.mark.parametrize("sigma", [0.5, 2.0, 6.0])
def test_a_zero_block_wider_than_the_window_keeps_an_exact_zero_centre(sigma):
    R = int(math.ceil(2 * sigma))
    n = 2 * R + 3  # the zero block, one voxel wider than the window on either side of its centre
    shape = (n + 8, n + 6, n + 4)
    v = np.asfortranarray(np.random.default_rng(2).random(shape, dtype=F) + F(1))
    v[4:4 + n, 3:3 + n, 2:2 + n] = 0
    got = mex.smooth_host(v, (sigma, sigma, sigma))
    c = (4 + n // 2, 3 + n // 2, 2 + n // 2)
    assert bits(got[c]) == 0, got[c]
    assert got[c[0] + 2, c[1], c[2]] > 0 and (got[:2] > 0).all()
    assert same_bits(got, SR.smooth(v, (sigma,) * 3, weights_of=mex.smooth_weights_host))


def test_sigma_all_zero_is_a_bit_exact_copy():
    v = volume((9, 7, 5))
    v.reshape(-1, order="F")[3] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), F)[0]  # a NaN with a payload
    for sigma in ((0, 0, 0), None, False, [], (-0.0, 0, 0)):
        got = mex.smooth_host(v, sigma)
        assert np.array_equal(bits(got), bits(v))
    flat = np.asfortranarray(volume((9, 7)))  # 2-D data: the third axis is skipped whatever its sigma
    assert same_bits(mex.smooth_host(flat, (1, 1, 3)), mex.smooth_host(flat, (1, 1, 0)))
    assert same_bits(mex.smooth_host(flat, (0, 0, 3)), flat)


def test_a_scalar_sigma_is_all_three_axes_and_in_place_is_allowed():
    v = volume((11, 6, 4))
    assert same_bits(mex.smooth_host(v, 1.25), mex.smooth_host(v, (1.25, 1.25, 1.25)))
    L = _lib.lib()
    dims = (ctypes.c_uint64 * 3)(*v.shape)
    for sigma in ((1, 0, 0), (1, 1, 0), (1, 1, 1)):  # one, two, three passes
        want = mex.smooth_host(v, sigma)
        buf = np.ascontiguousarray(v.reshape(-1, order="F")).copy()
        sg = F(sigma)
        assert L.vr_smooth_host(buf.ctypes.data, dims, sg.ctypes.data, buf.ctypes.data) == 0
        assert same_bits(buf.reshape(v.shape, order="F"), want)


# ---- argument errors --------------------------------------------------------------------------------------------

def test_argument_errors_need_no_device():
    L = _lib.lib()
    v = np.zeros(8, F)
    out = np.zeros(8, F)
    dims = (ctypes.c_uint64 * 3)(2, 2, 2)
    ok = F([1, 1, 1])
    for bad in ([np.nan, 1, 1], [1, -1, 1], [1, 1, np.inf], [6.5, 0, 0], [0, 0, -np.inf]):
        sg = F(bad)
        assert L.vr_smooth_host(v.ctypes.data, dims, sg.ctypes.data, out.ctypes.data) == 1
        # vr_set_smoothing checks its arguments before the handle: a NULL handle still reports the sigma
        assert L.vr_set_smoothing(None, sg.ctypes.data) == 1
    assert L.vr_set_smoothing(None, ok.ctypes.data) == 2  # (valid arguments: now the handle is looked at)
    assert L.vr_set_smoothing(None, None) == 2
    assert L.vr_get_smoothing(None, None) == 1
    assert L.vr_get_smoothing(None, out.ctypes.data) == 2
    assert L.vr_smooth_host(None, dims, ok.ctypes.data, out.ctypes.data) == 1
    assert L.vr_smooth_host(v.ctypes.data, None, ok.ctypes.data, out.ctypes.data) == 1
    assert L.vr_smooth_host(v.ctypes.data, dims, None, out.ctypes.data) == 1
    assert L.vr_smooth_host(v.ctypes.data, dims, ok.ctypes.data, None) == 1
    empty = (ctypes.c_uint64 * 3)(0, 2, 2)
    assert L.vr_smooth_host(None, empty, ok.ctypes.data, None) == 0  # (nothing to read or write)
    with pytest.raises(vr.VrError, match="sigma"):
        mex.smooth_host(v, (1, 2))
    with pytest.raises(vr.VrError, match="sigma"):
        mex.smoothing_sigma("1")
    with pytest.raises(vr.VrError, match="sigma"):
        mex.smoothing_sigma(np.ones((3, 3)))
