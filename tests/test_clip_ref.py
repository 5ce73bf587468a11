"""The CPU reference of the clip planes (tests/clip_ref.py) checked against itself and against the
unclipped references it wraps: the plane rule on hand-made rays, the geometry of the clipped interval,
the wrapper's hygiene, a plane set that contains the whole box (every output bit-identical), and that
the plane sets the GPU tests use are not vacuous on any of their scenes."""
import numpy as np
import pytest

import clip_ref as CR
import isosurface_ref as IR
import projection_ref as PR
import transfer_ref as TR

F = np.float32
SCENES = sorted(PR.FRAMES)
NONE = np.zeros((0, 4), F)


def _rays(o, d, tnear, tfar, hit=None):
    """A hand-made ray set-up in the unit box bmin = 0, bscale = 1 (q is the world position)."""
    d = np.asarray(d, F).reshape(-1, 3)
    n = d.shape[0]
    return dict(o=[F(c) for c in o], d=[d[:, k].reshape(1, n).copy() for k in range(3)],
                tnear=np.full((1, n), tnear, F), tfar=np.full((1, n), tfar, F),
                hit=np.ones((1, n), bool) if hit is None else np.asarray(hit, bool).reshape(1, n),
                bmin=[F(0)] * 3, bscale=[F(1)] * 3)


def test_plane_rule_on_hand_made_rays():
    # rays from o = (0.5, 0.5, -1) along +z, -z, +x (parallel to a z-plane), and a NaN direction
    R = _rays([0.5, 0.5, -1], [[0, 0, 1], [0, 0, -1], [1, 0, 0], [np.nan, 0, 1]], 1.0, 2.0)
    keep_above = CR.apply(R, F([[0, 0, 1, -0.25]]))  # keeps z >= 0.25: entered at t = 1.25
    assert keep_above["tnear"].tolist() == [[1.25, 1.0, 1.0, 1.0]]
    # +z: shortened from the front.  -z: sd < 0, tc = -1.25 < tfar -> tfar = -1.25 < tnear, a miss.
    # +x: parallel, origin z = -1 on the cut side, a miss.  NaN: sd NaN, origin on the cut side, a miss.
    assert keep_above["hit"].tolist() == [[True, False, False, False]]
    assert keep_above["tfar"][0, 1] == F(-1.25) and keep_above["tfar"][0, 0] == F(2.0)
    keep_below = CR.apply(R, F([[0, 0, -1, 0.75]]))  # keeps z <= 0.75: left at t = 1.75
    assert keep_below["tfar"].tolist()[0][0] == 1.75 and keep_below["tnear"][0, 0] == F(1.0)
    # the parallel and the NaN ray start on the kept side (s0 = 1.75 >= 0): untouched
    assert keep_below["hit"].tolist() == [[True, True, True, True]]
    assert keep_below["tfar"][0, 2] == F(2.0) and keep_below["tnear"][0, 1] == F(1.0)
    # both planes, in either order: the slab 0.25 <= z <= 0.75
    for order in ([0, 1], [1, 0]):
        both = CR.apply(R, F([[0, 0, 1, -0.25], [0, 0, -1, 0.75]])[order])
        assert (both["tnear"][0, 0], both["tfar"][0, 0]) == (F(1.25), F(1.75))
        assert both["hit"].tolist() == [[True, False, False, False]]
    # an empty kept region, a plane that only touches (tnear == tfar stays a hit), a box miss stays one
    assert not CR.apply(R, F([[0, 0, 1, -0.8], [0, 0, -1, 0.7]]))["hit"][0, 0]
    touch = CR.apply(R, F([[0, 0, 1, -1.0]]))
    assert touch["hit"][0, 0] and touch["tnear"][0, 0] == touch["tfar"][0, 0] == F(2.0)
    assert not CR.apply(_rays([0.5, 0.5, -1], [[0, 0, 1]], 1.0, 2.0, hit=[False]), CR.KEEP_ALL)["hit"].any()
    # a plane exactly through the origin of a parallel ray: s0 == 0 is kept, just below is not
    on = _rays([0.5, 0.5, 0.5], [[1, 0, 0]], 0.0, 0.5)
    assert CR.apply(on, F([[0, 0, 1, -0.5]]))["hit"].all()
    assert not CR.apply(on, F([[0, 0, 1, np.nextafter(F(-0.5), F(-1))]]))["hit"].any()


def test_float64_rule_agrees_with_float32():
    rng = np.random.default_rng(3)
    d = rng.standard_normal((200, 3)).astype(F)
    d /= np.linalg.norm(d, axis=1, keepdims=True).astype(F)
    R = _rays([0.3, -0.4, -1.5], d, 0.5, 3.0)
    a, b = CR.apply(R, CR.WEDGE), CR.apply(R, CR.WEDGE, IR._A64)
    assert b["tnear"].dtype == np.float64 and a["tnear"].dtype == np.float32
    # (on rays hit in both: a ray nearly parallel to a plane has a huge tc that carries the rounding
    # of its tiny sd, and is a miss; a hit ray's tc is at most tfar = 3, so |sd| is not small)
    both = a["hit"] & b["hit"]
    assert np.allclose(a["tnear"][both], b["tnear"][both], rtol=1e-5, atol=1e-5)
    assert np.allclose(a["tfar"][both], b["tfar"][both], rtol=1e-5, atol=1e-5)
    assert (a["hit"] != b["hit"]).sum() <= 2 and a["hit"].any() and (~a["hit"]).any()


def test_wrapper_replaces_and_restores_the_ray_set_ups():
    pr, tr = PR.rays, TR.rays
    with CR.clipped(NONE):  # no planes: nothing is wrapped
        assert PR.rays is pr and TR.rays is tr
    with pytest.raises(RuntimeError):
        with CR.clipped(CR.OBLIQUE):
            assert PR.rays is not pr and TR.rays is not tr
            raise RuntimeError("restored on the way out")
    assert PR.rays is pr and TR.rays is tr
    s = CR.scene("hg2_compute_32")
    P, keep, _ = s["S"].params(s["h"], None, None, *s["args"])
    plain = PR.rays(P)
    with CR.clipped(CR.OBLIQUE):
        c32, t32, t64 = PR.rays(P), TR.rays(P), TR.rays(P, IR._A64)
    del keep
    # transfer_ref's float32 rays are projection_ref's, clipped once; its float64 rays are clipped too
    for k in ("tnear", "tfar", "hit"):
        assert np.array_equal(c32[k], t32[k])
    assert np.array_equal(c32["tnear0"], plain["tnear"]) and np.array_equal(c32["hit0"], plain["hit"])
    assert t64["tnear"].dtype == np.float64 and t64["hit"].sum() < plain["hit"].sum()
    assert abs(int(t64["hit"].sum()) - int(c32["hit"].sum())) <= 2
    assert c32["hit"].sum() < plain["hit"].sum() and not (c32["hit"] & ~plain["hit"]).any()
    assert (c32["tnear"] >= plain["tnear"]).all() and (c32["tfar"] <= plain["tfar"]).all()


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("pset", sorted(CR.PLANE_SETS))
def test_clipped_interval_lies_in_the_kept_region(name, pset):
    """Geometry: the ends the planes moved lie on a plane, and both ends of every hit ray's interval
    satisfy every plane (to rounding), in the normalized coordinate q = (pos - bmin) * bscale."""
    planes = CR.PLANE_SETS[pset].astype(np.float64)
    R = CR.rays_of(name, CR.PLANE_SETS[pset])
    hit = R["hit"]
    o = [np.float64(c) for c in R["o"]]
    ends_moved = 0
    for end, moved in (("tnear", R["tnear"] > R["tnear0"]), ("tfar", R["tfar"] < R["tfar0"])):
        t = R[end].astype(np.float64)
        q = np.stack([(o[k] + R["d"][k].astype(np.float64) * t - np.float64(R["bmin"][k])) * np.float64(R["bscale"][k])
                      for k in range(3)], -1)
        s = q @ planes[:, :3].T + planes[:, 3]  # [H, W, planes]
        assert (s[hit] >= -1e-5).all(), (name, pset, end, float(s[hit].min()))
        m = hit & moved
        ends_moved += int(m.sum())
        assert (np.abs(s[m]).min(axis=-1) <= 1e-5).all()
    assert ends_moved >= 50


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("pset", sorted(CR.PLANE_SETS))
def test_plane_sets_of_the_gpu_tests_are_not_vacuous(name, pset):
    before, after, shortened, lost = CR.effect(name, CR.PLANE_SETS[pset])
    print(f"{name} {pset}: hit rays {before} -> {after}, still hit and shortened {shortened}, hit -> miss {lost}")
    assert shortened >= 50 and lost >= 50 and after + lost == before
    # and the clipped outputs differ from the unclipped ones where it matters
    (out0, n0), (out1, n1) = CR.projections(name, NONE), CR.projections(name, CR.PLANE_SETS[pset])
    assert (n1 <= n0).all() and n1.sum() < n0.sum()
    assert not np.array_equal(out0[PR.SUM][0], out1[PR.SUM][0])
    assert np.isnan(out1[PR.MIP][1]).sum() >= np.isnan(out0[PR.MIP][1]).sum() + 50  # misses: aux NaN


@pytest.mark.parametrize("name", SCENES)
def test_a_plane_set_that_contains_the_box_changes_no_bit(name):
    """Offset 100: every ray keeps its interval, so all four reference outputs -- both projections, the
    isosurface, the transfer render and with it the constant-colormap 'render' -- are bit-identical."""
    (p0, n0), (p1, n1) = CR.projections(name, NONE), CR.projections(name, CR.KEEP_ALL)
    assert np.array_equal(n0, n1) and n0.sum() > 0
    for mode in (PR.MIP, PR.SUM):
        for a, b in zip(p0[mode], p1[mode]):
            assert PR.same_bits(a, b) == 1.0
    i0, i1 = CR.isosurface(name, NONE), CR.isosurface(name, CR.KEEP_ALL)
    for k in ("img", "depth", "normal"):
        assert PR.same_bits(i0[k], i1[k]) == 1.0, k
    assert np.array_equal(i0["n"], i1["n"]) and (i0["k"] >= 0).any()
    lit = name == "hg1_lookup_24"  # (the lit reference takes seconds per frame: one scene has the lights)
    # (exp "kernel": the vectorised exponential; which one is taken does not matter to an identity)
    r0 = CR.render(name, NONE, lit, double=False, exp="kernel")
    r1 = CR.render(name, CR.KEEP_ALL, lit, double=False, exp="kernel")
    for k in ("img", "alpha"):
        assert PR.same_bits(r0[k], r1[k]) == 1.0, k
    assert np.array_equal(r0["n"], r1["n"]) and r0["img"].max() > 0
    if not lit:  # (one more transfer reference, with a real table, on one scene)
        return
    tf = TR.make_tf(F([[0.1, 0.9, 0.3], [1.0, 0.2, 0.0], [0.3, 0.3, 1.2]]), (0.2, 0.7), F([0, 0.4, 1.5]), (0.05, 0.8))
    t0 = CR.transfer(name, NONE, tf, "v3", lights=False, double=False, exp="kernel")
    t1 = CR.transfer(name, CR.KEEP_ALL, tf, "v3", lights=False, double=False, exp="kernel")
    assert PR.same_bits(t0["img"], t1["img"]) == 1.0 and PR.same_bits(t0["alpha"], t1["alpha"]) == 1.0


def test_clipped_isosurface_shows_a_cut_face():
    """A plane through the object: rays that enter through it and start inside the object hit at
    sample 0, and their depth is the clipped tnear bit for bit."""
    name = "hg2_compute_32"
    ref = CR.isosurface(name, CR.OBLIQUE, level=0.3, lights=False)
    R = CR.rays_of(name, CR.OBLIQUE)
    face = (ref["k"] == 0) & (R["tnear"] > R["tnear0"])
    assert face.sum() >= 10
    assert np.array_equal(ref["depth"][face].view(np.uint32), R["tnear"][face].view(np.uint32))
    assert np.array_equal(np.isnan(ref["depth"]), ref["k"] < 0) and (ref["k"][~R["hit"]] < 0).all()
