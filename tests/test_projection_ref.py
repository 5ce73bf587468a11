"""CPU tests of the projection renders: the numpy reference (tests/projection_ref.py) is pinned to
the oracle, its reduction rules are checked on hand-made volumes, and the new entry points'
argument checks that need no device."""
import ctypes

import numpy as np
import pytest

import oracle as O
import projection_ref as PR
import volume_renderer_amd as vr
from volume_renderer_amd import _lib, mex

FRAMES, scene_session, frame_args = PR.FRAMES, PR.scene_session, PR.frame_args


@pytest.mark.parametrize("name", sorted(FRAMES))
def test_sample_counts_equal_the_oracles(name):
    S, h, sc, em = scene_session(name)
    H, W = FRAMES[name]
    args = frame_args(sc, [H, W])
    img, aux, n = PR.project(S, h, PR.SUM, *args)
    # the oracle with an opacity threshold that is never reached: Fa = 0, thr = 1
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    _, steps = S.render(h, None, None, *frame_args(sc, [H, W], factors=[1, .4, 0], thr=1),
                        pixels=(xs.reshape(-1), ys.reshape(-1)))
    assert np.array_equal(n.reshape(-1), steps.astype(np.int64)), int((n.reshape(-1) != steps).sum())
    assert np.array_equal(aux, n.astype(np.float32))
    assert n.max() > 8 and (n == 0).any()  # hits and misses both occur
    # the maximum lies between the volume's extremes on every hit pixel
    mip, t, _ = PR.project(S, h, PR.MIP, *args)
    fe, col = np.float32(sc["factors"][0]), np.float32(sc["color"])
    hit = n > 0
    assert np.array_equal(np.isnan(t), ~hit)
    c = int(np.argmax(col))
    m = mip[:, :, c][hit] / (fe * col[c])
    assert (m <= em.max() * (1 + 1e-6)).all() and (m >= em.min() * (1 - 1e-6)).all()
    assert (mip[~hit] == 0).all() and (img[~hit] == 0).all()
    assert (t[hit] >= 0).all()


def centre_ray(col3, mode, fe=1.0):
    """A 3x3x3 volume whose centre column along the view axis holds col3, the rest 0.25 (below),
    seen by the 2x2 image's pixel (1, 1), whose ray runs along the axis through the voxel centres:
    (pixel value, aux, tnear of that ray)."""
    vol = np.full((3, 3, 3), 0.25, np.float32, order="F")
    # unrotated camera: the ray's direction is the kernel's z axis, the volume's third dimension
    vol[1, 1, :] = col3
    S, h = PR.session(vol)
    args = [np.float32([fe, 1, 1]), np.float32([1, 1, 1]), np.uint64([2, 2]), np.flip(np.eye(3), 0).astype(np.float32),
            np.float32([0, 2, 4]), np.float32(0.9), np.float32([1, 1, 1])]
    img, aux, n = PR.project(S, h, mode, *args)
    P, keep, _ = S.params(h, None, None, *args)
    R = PR.rays(P)
    assert n[1, 1] > 12
    return img[1, 1, 0], aux[1, 1], R["tnear"][1, 1], n[1, 1], np.float32(P.tstep)


def test_the_ray_runs_along_the_centre_column():
    # (guards the hand-made cases below: the samples depend on the centre column only)
    a = centre_ray([1, 2, 3], PR.SUM)
    vol_sum = a[0]
    assert vol_sum > 0
    p, t, tnear, n, tstep = centre_ray([3, 3, 3], PR.MIP)
    assert p == 3 and t == tnear


def test_first_maximum_wins():
    # the maximum 2 is attained by the first samples (clamped to the front voxel) and again at the back
    p, t, tnear, n, tstep = centre_ray([2, 1, 2], PR.MIP)
    assert p == 2 and t == tnear
    # a rising column: the maximum is attained first deep in the volume, in the last voxel's half
    p, t, tnear, n, tstep = centre_ray([0.5, 1, 2], PR.MIP)
    assert p == 2 and t > tnear + np.float32(0.5) * n * tstep
    # a negative maximum and the -0 rule
    p, t, tnear, n, tstep = centre_ray([-3, -1, -2], PR.MIP)
    assert -1.5 < p <= -1  # (no sample need fall on the middle voxel's centre)
    p, t, tnear, n, tstep = centre_ray([-0.0, -0.0, -0.0], PR.MIP)
    assert p == 0 and not np.signbit(p) and t == tnear


def test_nan_never_wins():
    p, t, tnear, n, tstep = centre_ray([np.nan, 1, 0.5], PR.MIP)
    assert 0.5 < p <= 1 and t > tnear  # the first sample past the NaN voxel's reach
    p, t, tnear, n, tstep = centre_ray([np.nan] * 3, PR.MIP)
    assert p == 0 and np.isnan(t)
    p, t, tnear, n, tstep = centre_ray([-np.inf] * 3, PR.MIP)
    assert p == 0 and np.isnan(t)
    # (an inf voxel lerps to NaN with any neighbour -- inf - inf, or 0 * inf -- so it never wins either)
    p, t, tnear, n, tstep = centre_ray([1, 1, np.inf], PR.MIP)
    assert p == 1 and t == tnear
    # the sum propagates them
    assert np.isnan(centre_ray([np.nan, 1, 0.5], PR.SUM)[0])
    assert np.isnan(centre_ray([1, 1, np.inf], PR.SUM)[0])  # inf, then inf + NaN
    s, cnt, tnear, n, tstep = centre_ray([1, 1, 1], PR.SUM, fe=2.0)
    assert cnt == n and s == (np.float32(2) * np.float32(n)) * tstep  # n exact additions of 1


def test_fma_is_singly_rounded():
    # a * a = 1 + 2^-11 + 2^-24 exactly, a tie of float32; c = +-2^-80 decides it, but vanishes in the
    # double sum, which alone would then round the tie to even
    a, tiny = np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -80)
    assert PR.fma(a, a, tiny) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    assert PR.fma(a, a, -tiny) == np.float32(1 + 2.0 ** -11)
    assert PR.fma(a, a, np.float32(0)) == np.float32(1 + 2.0 ** -11)  # the tie itself: to even
    x = np.float32([1.5, -2.25, 3e38, np.inf])
    assert np.array_equal(PR.fma(x, np.float32(2), np.float32(1)), np.float32([4, -3.5, np.inf, np.inf]))


def _args():
    ra, keep = mex.render_args(False, False, np.float32([1, 1, 1]), np.float32([1, 1, 1]), np.uint64([4, 4]),
                               np.eye(3, dtype=np.float32), np.float32([0, 3, 6]), np.float32(0.9),
                               np.float32([1, 1, 1]))
    return ra


def test_projection_entry_points_reject_an_invalid_handle():
    L, ra = _lib.lib(), _args()
    out = np.zeros(4 * 4 * 3, np.float32)
    rc = L.vr_render_projection(ctypes.c_void_p(12345), ctypes.byref(ra), _lib.VR_PROJ_MIP, out.ctypes.data, None)
    assert rc == 2 and b"Handle not valid" in L.vr_last_error()
    rc = L.vr_render_projection_device(None, ctypes.byref(ra), _lib.VR_PROJ_SUM, None, None, None, None, None)
    assert rc == 2
    with pytest.raises(vr.VrError, match="Handle not valid") as e:
        vr.volumeRender("render_projection", np.uint64(12345), False, False, np.float32([1, 1, 1]),
                        np.float32([1, 1, 1]), np.uint64([4, 4]), np.eye(3, dtype=np.float32), np.float32([0, 3, 6]),
                        np.float32(0.9), np.float32([1, 1, 1]), "mip")
    assert e.value.code == 2


def test_projection_entry_points_reject_a_bad_mode():
    L, ra = _lib.lib(), _args()
    out = np.zeros(4 * 4 * 3, np.float32)
    for mode in (2, -1, 7):
        assert L.vr_render_projection(ctypes.c_void_p(12345), ctypes.byref(ra), mode, out.ctypes.data, None) == 1
        assert b"projection mode" in L.vr_last_error()
        assert L.vr_render_projection_device(None, ctypes.byref(ra), mode, None, None, None, None, None) == 1
    with pytest.raises(vr.VrError, match="projection mode"):
        mex.projection_mode("min")
    with pytest.raises(vr.VrError, match="insufficient parameter"):
        vr.volumeRender("render_projection", np.uint64(12345), False, False)
    assert mex.projection_mode("MIP") == 0 and mex.projection_mode("sum") == 1
