"""Richardson-Lucy deconvolution without a device (include/vrhip.h vr_set_deconvolution): the value rule on
the CPU (vr_deconvolve_host: vr_smooth_host's passes and the inline functions the kernels evaluate,
csrc/vr_deconv.h) against its numpy restatement (tests/deconv_ref.py) bit for bit, the rule's exact
properties, and the argument checks that arrive before the handle.

The bit-exact comparisons take their weights from the product (mex.smooth_weights_host), as
tests/test_smooth_host.py does, so a libm that rounds exp differently from Python's cannot fail them.

Recorded, not asserted (nobody has derived a bound): the relative flux change |sum u_n - sum d| / sum d of
the sparse-truth case below, printed by its test: 1.7e-3 after 2 iterations, 2.1e-3 after 10."""
import ctypes
import math

import numpy as np
import pytest

import deconv_ref as DR
import smooth_ref as SR  # noqa: F401  (deconv_ref's blur)

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402
from test_smooth_host import bits, same_bits  # noqa: E402

F = np.float32
SHAPES = [(7,), (9, 6), (11, 5, 4), (3, 2, 2), (1, 1, 13)]
SIGMAS = [(1, 0.75, 1.5), (0, 2, 0), (6, 6, 6), (0.3, 0.3, 0.3)]
ITERATIONS = (1, 2, 3, 5)
FLOOR = F(1e-6)


def volume(shape, special, seed=5):
    """Noise around zero (a quarter of it negative), a run of exact zeros and of values far below the floor
    -- where the blurred estimate stays under the floor at small sigma -- and, with `special`, a NaN, +-inf,
    -0 and a subnormal spread over the volume."""
    rng = np.random.default_rng(seed + len(shape))
    flat = ((rng.random(int(np.prod(shape)), dtype=F) - F(0.25)) * F(3)).astype(F)
    n = flat.size
    flat[: max(2, n // 4)] = 0
    flat[n // 4: n // 4 + max(1, n // 8)] = F(1e-9)
    if special:
        for at, x in zip((n // 7, n // 3, n // 2, (2 * n) // 3, (5 * n) // 6, n - 1), (np.nan, np.inf, -np.inf, -0.0, 1e-40, -2.5)):
            flat[at] = F(x)
    return np.asfortranarray(flat.reshape(shape, order="F"))


def dims3(shape):
    return (ctypes.c_uint64 * 3)(*(list(shape) + [1] * (3 - len(shape))))


# ---- the value rule ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("sigma", SIGMAS)
@pytest.mark.parametrize("shape", SHAPES)
def test_deconvolve_host_is_the_rule_bit_for_bit(shape, sigma, special):
    v = volume(shape, special)
    for n in ITERATIONS:
        got = mex.deconvolve_host(v, sigma, n, FLOOR)
        want = DR.deconvolve(v, sigma, n, FLOOR, weights_of=mex.smooth_weights_host)
        assert got.shape == v.shape and got.dtype == np.float32
        assert same_bits(got, want), f"{shape} {sigma} n={n}: {np.count_nonzero(bits(got) != bits(want))} voxels differ"
        if not special:
            assert np.isfinite(got).all() and (got >= 0).all()
            assert not same_bits(got, v), "the iteration changed nothing"
    if special:
        assert np.isnan(want).any()


def test_the_floor_region_and_the_special_values_are_in_the_data():
    v = volume((11, 5, 4), True)
    c = mex.smooth_host(DR.data(v), (0.3, 0.3, 0.3))
    with np.errstate(invalid="ignore"):
        assert (c < FLOOR).sum() > 5, "no voxel whose blurred estimate lies under the floor"
    assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any() and (v < 0).any()
    assert (bits(v) == 0x80000000).any() and ((v > 0) & (v < np.finfo(F).tiny)).any() and (bits(v) == 0).any()
    # NaN and -0 pass through d, a negative becomes +0
    d = DR.data(F([np.nan, -0.0, -1.0, 2.0, -np.inf]))
    assert np.isnan(d[0]) and bits(d[1:]).tolist() == [0x80000000, 0, 0x40000000, 0]


def test_no_iterations_and_all_zero_sigma_copy_bit_for_bit():
    v = volume((9, 7, 5), True)
    v.reshape(-1, order="F")[3] = np.frombuffer(np.uint32(0x7FC12345).tobytes(), F)[0]  # a NaN with a payload
    for sigma, n in (((1, 1, 1), 0), ((0, 0, 0), 5), (None, 5), (False, 3), ([], 3), ((-0.0, 0, 0), 2)):
        got = mex.deconvolve_host(v, sigma, n)
        assert np.array_equal(bits(got), bits(v)), (sigma, n)  # (negative voxels included: nothing is clamped)
    # sigma only on axes of one voxel: B is the identity and the rule is still evaluated
    line = volume((1, 1, 13), False)
    got = mex.deconvolve_host(line, (2, 2, 0), 3)
    assert same_bits(got, DR.deconvolve(line, (2, 2, 0), 3)) and not same_bits(got, line)


@pytest.mark.parametrize("sigma", SIGMAS)
def test_a_voxel_with_no_data_stays_zero(sigma):
    v = volume((11, 5, 4), False)
    d = DR.data(v)
    for n in ITERATIONS:
        u = mex.deconvolve_host(v, sigma, n)
        assert np.isfinite(u).all()
        assert (d == 0).sum() > 20 and (u[d == 0] == 0).all(), f"{sigma} n={n}"


def test_iterations_approach_a_sparse_truth():
    sigma = (1, 1, 2)
    R = [int(math.ceil(2 * s)) for s in sigma]
    shape = (28, 28, 36)
    rng = np.random.default_rng(11)
    truth = np.zeros(shape, F, order="F")
    for _ in range(14):  # points at least R from every face (the blur's support stays inside)
        at = tuple(int(rng.integers(r, n - r)) for r, n in zip(R, shape))
        truth[at] += F(1 + 4 * rng.random())
    blurred = mex.smooth_host(truth, sigma)
    assert (blurred >= 0).all()

    def dist(a):
        return float(np.sqrt(((a.astype(np.float64) - truth.astype(np.float64)) ** 2).sum()))

    u2, u10 = mex.deconvolve_host(blurred, sigma, 2), mex.deconvolve_host(blurred, sigma, 10)
    d0, d2, d10 = dist(blurred), dist(u2), dist(u10)
    flux = float(blurred.astype(np.float64).sum())
    for n, u in ((2, u2), (10, u10)):
        print(f"sparse truth, {n} iterations: relative flux change {abs(float(u.astype(np.float64).sum()) - flux) / flux:.3g}")
    print(f"L2 distance to the truth: blurred {d0:.6g}, 2 iterations {d2:.6g}, 10 iterations {d10:.6g}")
    assert d10 < d0 and d10 < d2


def test_in_place_is_allowed():
    v = volume((11, 5, 4), True)
    L = _lib.lib()
    for sigma in ((1, 0, 0), (1, 1, 0), (1, 0.75, 1.5), (0, 0, 0)):
        for n in (0, 1, 2, 3):
            want = mex.deconvolve_host(v, sigma, n)
            buf = np.ascontiguousarray(v.reshape(-1, order="F")).copy()
            sg = F(sigma)
            assert L.vr_deconvolve_host(buf.ctypes.data, dims3(v.shape), sg.ctypes.data, n, FLOOR, buf.ctypes.data) == 0
            assert same_bits(buf.reshape(v.shape, order="F"), want), (sigma, n)


def test_a_scalar_sigma_is_all_three_axes_and_the_default_floor_is_1e_6():
    v = volume((11, 5, 4), False)
    assert same_bits(mex.deconvolve_host(v, 1.25, 2), mex.deconvolve_host(v, (1.25, 1.25, 1.25), 2, F(1e-6)))
    assert not same_bits(mex.deconvolve_host(v, 0.3, 2), mex.deconvolve_host(v, 0.3, 2, F(1e-2)))  # (voxels under either floor)
    assert mex.DECONV_FLOOR == F(1e-6)


# ---- argument errors --------------------------------------------------------------------------------------------

def test_argument_errors_need_no_device():
    L = _lib.lib()
    v, out = np.zeros(8, F), np.zeros(8, F)
    dims = dims3((2, 2, 2))
    ok = F([1, 1, 1])

    def host(sg, n, fl, src=v, dst=out, d=dims):
        return L.vr_deconvolve_host(src.ctypes.data if src is not None else None, d,
                                    sg.ctypes.data if sg is not None else None, n, fl,
                                    dst.ctypes.data if dst is not None else None)

    for bad in ([np.nan, 1, 1], [1, -1, 1], [1, 1, np.inf], [6.5, 0, 0], [0, 0, -np.inf]):
        sg = F(bad)
        assert host(sg, 1, FLOOR) == 1
        # vr_set_deconvolution checks its arguments before the handle: a NULL handle still reports them
        assert L.vr_set_deconvolution(None, sg.ctypes.data, 1, FLOOR) == 1
        assert "deconvolution" in L.vr_last_error().decode()
    for n in (-1, 65, 1 << 20):
        assert host(ok, n, FLOOR) == 1 and L.vr_set_deconvolution(None, ok.ctypes.data, n, FLOOR) == 1
        assert "iterations" in L.vr_last_error().decode()
    for fl in (0.0, -0.0, -1e-6, np.nan, np.inf, -np.inf):
        assert host(ok, 1, fl) == 1 and L.vr_set_deconvolution(None, ok.ctypes.data, 1, fl) == 1
        assert "floor" in L.vr_last_error().decode()
        assert L.vr_set_deconvolution(None, None, 0, fl) == 1  # (also when the call clears)
    assert host(ok, 64, np.finfo(F).tiny) == 0 and host(ok, 0, FLOOR) == 0
    for args in ((ok, 1), (ok, 0), (None, 3), (F([0, 0, 0]), 3)):  # (valid arguments: now the handle is looked at)
        assert L.vr_set_deconvolution(None, args[0].ctypes.data if args[0] is not None else None, args[1], FLOOR) == 2
    n, fl = ctypes.c_int32(0), ctypes.c_float(0)
    assert L.vr_get_deconvolution(None, None, ctypes.byref(n), ctypes.byref(fl)) == 1
    assert L.vr_get_deconvolution(None, out.ctypes.data, None, ctypes.byref(fl)) == 1
    assert L.vr_get_deconvolution(None, out.ctypes.data, ctypes.byref(n), None) == 1
    assert L.vr_get_deconvolution(None, out.ctypes.data, ctypes.byref(n), ctypes.byref(fl)) == 2
    assert host(ok, 1, FLOOR, src=None) == 1 and host(ok, 1, FLOOR, dst=None) == 1
    assert host(ok, 1, FLOOR, d=None) == 1 and host(None, 1, FLOOR) == 1
    assert host(ok, 1, FLOOR, src=None, dst=None, d=dims3((0, 2, 2))) == 0  # (nothing to read or write)
    assert host(ok, 1, FLOOR, d=(ctypes.c_uint64 * 3)(1 << 31, 1, 1)) == 5
    with pytest.raises(vr.VrError, match="sigma"):
        mex.deconvolve_host(v, (1, 2), 1)
    with pytest.raises(vr.VrError, match="iterations"):
        mex.deconvolve_host(v, 1, 1.5)
    with pytest.raises(vr.VrError, match="iterations"):
        mex.deconvolve_host(v, 1, 65)
    with pytest.raises(vr.VrError, match="floor"):
        mex.deconvolve_host(v, 1, 1, "tiny")
