"""CPU tests of the isosurface render: the numpy reference (tests/isosurface_ref.py) is pinned to the
oracle's gradient and shading, the search and refinement rules are checked on the shared scenes and
on hand-made volumes, and the new entry points' argument checks that need no device."""
import ctypes

import numpy as np
import pytest

import isosurface_ref as IR
import oracle as O
import projection_ref as PR
import volume_renderer_amd as vr
from golden_cases import EX1_LIGHTS, EX1_R, STAMP_LUT
from volume_renderer_amd import _lib, mex

F = np.float32


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


# ---- 1. gradient and shading equal the oracle's, bit for bit ---------------------------------------

@pytest.mark.parametrize("lookup", [False, True], ids=["compute", "lookup"])
def test_surface_sample_equals_the_oracles_first_sample(lookup):
    """render with thr = -1 stops after one sample: sr = fma(1, fma(eds, col, ill) * alpha, 0).  The
    same from surface_sample() at pos_0, with the oracle's expf for the opacity."""
    em = O.rand_volume(12)
    S = O.OracleSession()
    h = S.new()
    v = O.OVolume(em, 5)
    g = [O.OVolume(x, 9) for x in O.matlab_gradient(em)] if lookup else []
    S.sync_volumes(h, 0, v, O.OVolume(O.rand_volume(8), 3), v, *g)
    H, W = 20, 24
    args = [EX1_LIGHTS, O.OVolume(O.hg_lut(32), STAMP_LUT), F([1.5, 0.4, 0.6]), F([1, 1, 1]), np.uint64([H, W]),
            np.flip(EX1_R, 0).astype(F), F([0, 3, 6]), F(-1), F([1, 0.5, 0.25])]
    P, keep, _ = S.params(h, *args)
    assert int(P.grad_method) == (1 if lookup else 0) and IR.lit(P)
    R = PR.rays(P)
    ys, xs = np.nonzero(R["hit"])
    assert len(xs) > 150
    want, steps = S.render(h, *args, pixels=(xs, ys))
    assert (steps == 1).all()
    t0 = R["tnear"][ys, xs]
    pos0 = [PR.fma(R["d"][i][ys, xs], t0, R["o"][i]) for i in range(3)]
    vs, _, n, ill = IR.surface_sample(P, pos0)
    tstep = F(P.tstep)
    with np.errstate(all="ignore"):
        alpha = F(1) - IR.expf(-(F(P.factor_absorption) * vs) * tstep)
        eds = (F(P.factor_emission) * vs) * tstep
        got = np.stack([PR.fma(F(1), PR.fma(eds, F(P.color[c]), ill[c]) * alpha, F(0)) for c in range(3)], 1)
    assert np.array_equal(bits(got), bits(want)), int((bits(got) != bits(want)).any(1).sum())
    assert (np.abs(want).max(0) > 0).all() and not np.isnan(np.stack(n)).any()


# ---- 2. the search and the refinement on the shared scenes ----------------------------------------

@pytest.mark.parametrize("name", sorted(PR.FRAMES))
def test_search_and_refinement_rules(name):
    # Fe = 1 and a white colour: the MIP image is the maximum itself
    sc = IR.scene(name, res=PR.FRAMES[name], color=[1, 1, 1], factors=[1, 0.4, 0.6])
    ref, level = sc["ref"], F(sc["level"])
    mip, tmax, _ = PR.project(sc["S"], sc["h"], PR.MIP, *sc["args"])
    surf = ref["k"] >= 0
    won = ~np.isnan(tmax)  # (a ray with a winning sample)
    assert np.array_equal(surf, won & (mip[:, :, 0] >= level))
    assert surf.sum() > 100 and (~surf).any()
    assert np.array_equal(np.isnan(ref["depth"]), ~surf) and (ref["img"][~surf] == 0).all()
    assert np.isnan(ref["normal"][~surf]).all() and not np.isnan(ref["normal"][surf]).any()
    deep = ref["k"] > 0
    assert deep.any()
    t, hi = ref["depth"][deep], ref["hi"][deep]
    assert (ref["tprev"][deep] < t).all() and (t <= ref["tk"][deep]).all()
    assert (ref["vstar"][surf] >= level).all()
    assert (hi >= F(2.0 ** -6)).all() and (hi <= 1).all() and (np.round(hi * 64) == hi * 64).all()
    # one step of 2^-6 before hi the sample is below the level (hi = 2^-6: that is sample k - 1 itself)
    inner = hi > F(2.0 ** -6)
    P, keep, _ = sc["S"].params(sc["h"], None, None, *sc["args"])
    q = [PR.fma(ref["step"][i][deep][inner], hi[inner] - F(2.0 ** -6), ref["pos_prev"][i][deep][inner])
         for i in range(3)]
    bmin = [F(P.boxmin[i]) for i in range(3)]
    bsc = [F(1) / (F(P.boxmax[i]) - bmin[i]) for i in range(3)]
    below = IR.tex32(P.em, *[((q[i] - bmin[i]) * bsc[i]).astype(F) for i in range(3)])
    assert inner.sum() > 50 and (below < level).all()
    # hi = 1 is sample k itself, bit for bit
    at = hi == 1
    assert np.array_equal(bits(t[at]), bits(ref["tk"][deep][at]))
    first = ref["k"] == 0
    assert np.array_equal(bits(ref["depth"][first]), bits(ref["tnear"][first]))


def test_first_sample_hits_have_the_bits_of_tnear():
    sc = IR.scene(IR.RAND)
    ref = sc["ref"]
    first, deep = ref["k"] == 0, ref["k"] > 0
    assert first.sum() > 50 and deep.sum() > 50
    assert np.array_equal(bits(ref["depth"][first]), bits(ref["tnear"][first]))
    assert (ref["n"][first] == 1).all() and np.array_equal(ref["n"][deep], ref["k"][deep] + 1)
    # level 0 on a shell scene: every ray that meets the box has its surface at the first sample
    z = IR.scene("hg2_compute_32", res=PR.FRAMES["hg2_compute_32"], level=0.0)["ref"]
    assert np.array_equal(z["k"] == 0, z["hit"]) and (z["k"][~z["hit"]] == -1).all()


# ---- 3. hand-made volumes --------------------------------------------------------------------------

def centre_column(col3, level):
    """The centre_ray construction of tests/test_projection_ref.py: a 3x3x3 volume whose centre column
    along the view axis holds col3, seen by pixel (1, 1) of a 2x2 image, whose ray runs through the
    column's voxel centres.  (reference of that pixel's frame, P, rays)"""
    vol = np.full((3, 3, 3), 0.25, F, order="F")
    vol[1, 1, :] = col3
    S, h = PR.session(vol)
    args = [F([1, 1, 1]), F([1, 1, 1]), np.uint64([2, 2]), np.flip(np.eye(3), 0).astype(F), F([0, 2, 4]), F(0.9),
            F([1, 1, 1])]
    ref = IR.isosurface(S, h, level, None, None, *args)
    P, keep, _ = S.params(h, None, None, *args)
    return ref, P, PR.rays(P), keep


def test_depth_of_a_ramp_is_the_analytic_crossing():
    """Between the centres of voxels 1 and 2 the column [-1, 0, 1] samples to the filter weight w =
    rint(frac * 256) / 256 itself.  The level 76.5 / 256 lies between two weights, so the sampled
    value reaches it exactly where the linear ramp does, at frac = 76.5 / 256, and the refined depth
    lies within one bisection cell, tstep / 64, of that crossing."""
    level = F(76.5 / 256)
    ref, P, R, keep = centre_column([-1, 0, 1], level)
    assert ref["k"][1, 1] > 2
    o, d = float(R["o"][2]), float(R["d"][2][1, 1])
    bmin, bmax = float(P.boxmin[2]), float(P.boxmax[2])
    # texel coordinate xb = ((z - bmin) / (bmax - bmin)) * 3 - 0.5 = 1 + 76.5 / 256 along z = o + d t
    z = bmin + (1 + 76.5 / 256 + 0.5) / 3 * (bmax - bmin)
    t_cross = (z - o) / d
    assert d > 0 and R["tnear"][1, 1] < t_cross < R["tfar"][1, 1]
    assert abs(float(ref["depth"][1, 1]) - t_cross) <= float(P.tstep) / 64
    assert ref["img"][1, 1, 0] == ref["vstar"][1, 1] >= level  # Fe = 1, white, no lights
    assert ref["vstar"][1, 1] <= F(78 / 256)


def test_nan_volume_has_no_surface():
    for level in (0.5, -np.inf):
        ref, _, R, keep = centre_column([np.nan] * 3, level)
        assert R["hit"][1, 1] and ref["k"][1, 1] == -1 and np.isnan(ref["depth"][1, 1]) and ref["img"][1, 1, 0] == 0
    ref, _, R, keep = centre_column([1, 1, 1], -np.inf)  # -inf: every real sample hits at once
    assert ref["k"][1, 1] == 0
    ref, _, R, keep = centre_column([1, 1, 1], np.inf)
    assert ref["k"][1, 1] == -1


# ---- 4. entry points -------------------------------------------------------------------------------

def _args():
    ra, keep = mex.render_args(False, False, F([1, 1, 1]), F([1, 1, 1]), np.uint64([4, 4]), np.eye(3, dtype=F),
                               F([0, 3, 6]), F(0.9), F([1, 1, 1]))
    return ra


def test_isosurface_entry_points_check_the_level_before_the_handle():
    L, ra = _lib.lib(), _args()
    out = np.zeros(4 * 4 * 3, F)
    nan = ctypes.c_float(float("nan"))
    assert L.vr_render_isosurface(ctypes.c_void_p(12345), ctypes.byref(ra), nan, out.ctypes.data, None, None) == 1
    assert b"level" in L.vr_last_error()
    assert L.vr_render_isosurface_device(None, ctypes.byref(ra), nan, None, None, None, None, None, None) == 1
    for level in (0.3, float("inf"), float("-inf")):
        lv = ctypes.c_float(level)
        rc = L.vr_render_isosurface(ctypes.c_void_p(12345), ctypes.byref(ra), lv, out.ctypes.data, None, None)
        assert rc == 2 and b"Handle not valid" in L.vr_last_error()
        assert L.vr_render_isosurface_device(None, ctypes.byref(ra), lv, None, None, None, None, None, None) == 2
    argv = [False, False, F([1, 1, 1]), F([1, 1, 1]), np.uint64([4, 4]), np.eye(3, dtype=F), F([0, 3, 6]), F(0.9),
            F([1, 1, 1])]
    with pytest.raises(vr.VrError, match="Handle not valid") as e:
        vr.volumeRender("render_isosurface", np.uint64(12345), *argv, 0.3)
    assert e.value.code == 2
    with pytest.raises(vr.VrError, match="level is NaN") as e:
        vr.volumeRender("render_isosurface", np.uint64(12345), *argv, np.float32("nan"))
    assert e.value.code == 1
    with pytest.raises(vr.VrError, match="real scalar"):
        vr.volumeRender("render_isosurface", np.uint64(12345), *argv, "0.3")
    with pytest.raises(vr.VrError, match="insufficient parameter"):
        vr.volumeRender("render_isosurface", np.uint64(12345), *argv)
