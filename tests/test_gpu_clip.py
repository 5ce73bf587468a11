"""GPU tests of the clip planes (vr_set_clip; csrc/vr_clip.h and the CLIP instantiations of the four
one-lane kernels) against the CPU reference of tests/clip_ref.py, which wraps the ray set-ups of the
projection, isosurface and transfer references, and against the product itself where the contract
equates two paths (stereo = two renders, the leap, a cleared set = no set).

Parity conditions are those of the unclipped tests: projection image and aux and the isosurface's
depth and normal bit for bit; the isosurface image by test_gpu_isosurface.check_against_reference; the
transfer planes and 'render' by conftest.assert_parity against the glibc reference (an unlit transfer
render also bit for bit against the reference with the kernel's exponential); sample counters equal
to the reference's totals.  tests/test_clip_ref.py shows that no plane set here is vacuous."""
import ctypes

import numpy as np
import pytest

import clip_ref as CR
import isosurface_ref as IR
import oracle as O
import projection_ref as PR
import transfer_ref as TR
from conftest import assert_parity
from golden_cases import STAMP_EM, STAMP_LUT, STAMP_RE

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402
from test_gpu_isosurface import check_against_reference as check_iso, gpu_iso  # noqa: E402
from test_gpu_projection import BLOCK_ARGS, bits_equal, block_volume, gpu_project, new_handle  # noqa: E402
from test_gpu_transfer import TF_VALUE, V, gpu_transfer, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SCENES = sorted(PR.FRAMES)
PSETS = sorted(CR.PLANE_SETS)
MODES = (("mip", PR.MIP), ("sum", PR.SUM))
NONE = np.zeros((0, 4), F)
_gold = {}


def product_scene(name):
    """The product-side volumes and arguments of a scene of projection_ref.FRAMES."""
    if name not in _gold:
        s = CR.scene(name)
        sc, em = s["sc"], s["em"]
        _gold[name] = dict(em=em, re=sc["re"]() if sc["re"] else None,
                           grads=O.matlab_gradient(em) if sc["grads"] else None,
                           lights=[vr.LightSource(l[:3], l[3:]) for l in sc["lights"]],
                           lut=V(vr.HenyeyGreenstein(sc["lut"]), STAMP_LUT), args=s["args"])
    return _gold[name]


def argv_of(p, lit=True):
    return ([p["lights"], p["lut"]] if lit else [False, False]) + list(p["args"])


def handle_of(p, planes=None):
    h = new_handle(p["em"], p["re"], p["grads"])
    if planes is not None:
        mex.set_clip(h, planes)
    return h


def gpu_render(h, argv, count=True, exact=None, monkeypatch=None):
    """vr_render_device of the frame `argv`: (image [H, W, 3], (samples, shaded samples))."""
    import torch
    if exact is not None:
        monkeypatch.setenv("VR_EXACT_SHADE", "1" if exact else "0")
    ra, keep = mex.render_args(*argv)
    H, W = (int(x) for x in np.asarray(argv[4]).reshape(-1))
    out = torch.full((3, W, H), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.zeros(48, dtype=torch.int64, device="cuda")  # VR_NUM_COUNTERS
    mex.render_device(h, ra, out.data_ptr(), None, steps.data_ptr() if count else 0)
    torch.cuda.synchronize()
    del keep
    if exact is not None:
        monkeypatch.delenv("VR_EXACT_SHADE")
    s = steps.cpu().numpy()
    return np.asfortranarray(out.cpu().numpy().transpose(2, 1, 0)), (int(s[0]), int(s[1]))


# ---- 0. the state of the handle -------------------------------------------------------------------------

def test_set_get_round_trip_and_clear():
    h = vr.volumeRender("new")
    assert mex.get_clip(h).shape == (0, 4)
    for planes in (CR.WEDGE, CR.OBLIQUE, np.tile(CR.OBLIQUE, (6, 1)) * F([[1], [2], [3], [4], [5], [6]])):
        mex.set_clip(h, planes)
        got = mex.get_clip(h)
        assert got.dtype == np.float32 and bits_equal(got, np.asarray(planes, F))  # as set: not normalized
    with pytest.raises(vr.VrError, match="clip planes"):  # a refused set leaves the old one
        mex.set_clip(h, np.tile(CR.OBLIQUE, (7, 1)))
    assert mex.get_clip(h).shape == (6, 4)
    other = vr.volumeRender("new")  # state of the handle, not of the module
    assert mex.get_clip(other).shape == (0, 4)
    mex.set_clip(h, None)
    assert mex.get_clip(h).shape == (0, 4)
    L = _lib.lib()
    assert L.vr_set_clip(mex._handle(h), None, 0) == 0
    mex.set_clip(h, CR.WEDGE)
    vr.volumeRender("delete", h)
    with pytest.raises(vr.VrError, match="Handle not valid"):
        mex.get_clip(h)
    assert mex.get_clip(other).shape == (0, 4)
    vr.volumeRender("delete", other)


# ---- 1. parity with the reference, per scene and plane set -----------------------------------------------

@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("name", SCENES)
def test_clipped_projection_equals_the_reference(name, pset):
    planes = CR.PLANE_SETS[pset]
    ref, n = CR.projections(name, planes)
    p = product_scene(name)
    h = handle_of(p, planes)
    for mode, code in MODES:
        img, aux, (visited, fetched) = gpu_project(h, argv_of(p), mode, count=True)
        assert PR.same_bits(img, ref[code][0]) == 1.0, f"{name} {pset} {mode}: image differs"
        assert PR.same_bits(aux, ref[code][1]) == 1.0, f"{name} {pset} {mode}: aux differs"
        assert visited == int(n.sum()) and fetched == visited  # (no occupancy map at these sizes)
        plain = gpu_project(h, argv_of(p), mode)  # (the kernel without the counters)
        assert bits_equal(plain[0], img) and bits_equal(plain[1], aux)
        himg, haux = vr.volumeRender("render_projection", h, *argv_of(p), mode)  # the host entry point
        assert bits_equal(himg, img) and bits_equal(haux, aux)
    assert ref[PR.SUM][0].max() > 0
    vr.volumeRender("delete", h)


@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("name", SCENES)
def test_clipped_isosurface_equals_the_reference(name, pset):
    planes = CR.PLANE_SETS[pset]
    ref = CR.isosurface(name, planes, level=0.3)
    assert (ref["k"] == 0).any() and (ref["k"] > 0).sum() >= 10  # cut-face pixels and marched hits
    p = product_scene(name)
    h = handle_of(p, planes)
    got = gpu_iso(h, argv_of(p), 0.3, count=True)
    assert PR.same_bits(got[1], ref["depth"]) == 1.0, f"{name} {pset}: depth differs"
    assert PR.same_bits(got[2], ref["normal"]) == 1.0, f"{name} {pset}: normal differs"
    check_iso(got, ref, f"{name} {pset}")
    assert got[3][0] == int(ref["n"].sum()) and got[3][2] == int((ref["k"] >= 0).sum())
    img, depth, normal = vr.volumeRender("render_isosurface", h, *argv_of(p), 0.3)
    assert bits_equal(img, got[0]) and bits_equal(depth, got[1]) and bits_equal(normal, got[2])
    vr.volumeRender("delete", h)


@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("name", SCENES)
def test_clipped_transfer_equals_the_reference(name, pset):
    """Lit on the two example scenes; unlit on stereo_right_24 (its camera offset is not 0), where
    nothing is left between the kernel and the reference with the kernel's exponential."""
    planes = CR.PLANE_SETS[pset]
    lit = name != "stereo_right_24"
    tf = TR.make_tf(TF_VALUE["colormap"], TF_VALUE["clim"], TF_VALUE["alphamap"], TF_VALUE["alim"], TF_VALUE["coord"])
    ref = CR.transfer(name, planes, tf, "value", lights=lit)
    p = product_scene(name)
    h = handle_of(p, planes)
    img, alpha, (visited, _) = gpu_transfer(h, argv_of(p, lit), TF_VALUE, count=True)
    assert_parity(img, ref["img"], ref["img64"].astype(F), f"{name} {pset} transfer image")
    assert_parity(alpha, ref["alpha"], ref["alpha64"].astype(F), f"{name} {pset} transfer alpha")
    assert visited == int(ref["n"].sum()) and (ref["alpha"] > 0).any()
    if not lit:
        ex = CR.transfer(name, planes, tf, "value", lights=False, double=False, exp="kernel")
        assert same_bits(img, ex["img"]) and same_bits(alpha, ex["alpha"])
    vr.volumeRender("delete", h)


@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("name", SCENES)
def test_clipped_render_equals_the_constant_colormap_reference(name, pset, monkeypatch):
    planes = CR.PLANE_SETS[pset]
    ref = CR.render(name, planes)
    total = int(ref["n"].sum())
    p = product_scene(name)
    h = handle_of(p, planes)
    exact, (samples, _) = gpu_render(h, argv_of(p), exact=True, monkeypatch=monkeypatch)
    st = assert_parity(exact, ref["img"], ref["img64"].astype(F), f"{name} {pset} render, exact shading")
    fast, (fsamples, _) = gpu_render(h, argv_of(p))
    sf = assert_parity(fast, ref["img"], ref["img64"].astype(F), f"{name} {pset} render, default shading")
    print(f"{name} {pset}: bit-identical share exact {st['bit_exact']:.6f}, default {sf['bit_exact']:.6f}; "
          f"samples reference {total}, exact {samples}, default {fsamples}")
    assert samples == total and ref["img"].max() > 0
    # the clipped transfer kernel with the constant colormap is the exact-shading render bit for bit
    const = dict(colormap=TR.constant_colormap(p["args"][6]), clim=(0, 1))
    assert bits_equal(gpu_transfer(h, argv_of(p), const)[0], exact)
    # the host entry point and the uncounted kernel write the same image
    assert bits_equal(vr.volumeRender("render", h, *argv_of(p)), fast)
    assert bits_equal(gpu_render(h, argv_of(p), count=False)[0], fast)
    vr.volumeRender("delete", h)


# ---- 2. axis mapping and orientation, self-checking -------------------------------------------------------

AXIS_DIMS = (16, 12, 20)
AXIS_ARGS = [F([1.5, 0.4, 0.6]), F([1, 1, 1]), np.uint64([40, 48]), np.flip(O.rotation(125, 25, 0), 0).astype(F),
             F([0, 3, 6]), F(0.9), F([1, 0.5, 0.25])]


@pytest.mark.parametrize("j", [0, 1, 2])
def test_plane_normal_pairs_with_the_dimension_of_data(j):
    """V_j is 1 where the index along dimension j is >= d_j / 2; the plane e_j . q >= 0.5 + 1 / d_j keeps
    only samples whose trilinear cell lies in that half (half a texel of margin): every kept sample
    reads exactly 1, and exactly 0 in the complementary volume."""
    d = AXIS_DIMS
    idx = np.arange(d[j]).reshape([-1 if k == j else 1 for k in range(3)])
    vj = np.asfortranarray(np.broadcast_to((idx >= d[j] // 2).astype(F), d))
    plane = np.zeros((1, 4), F)
    plane[0, j], plane[0, 3] = 1, -(0.5 + 1.0 / d[j])
    argv = [False, False] + AXIS_ARGS
    S, hs = PR.session(vj, STAMP_EM)
    P, keep, _ = S.params(hs, None, None, *AXIS_ARGS)
    tstep, Fe = F(P.tstep), F(AXIS_ARGS[0][0])
    del keep
    h = new_handle(vj)
    _, n_plain, _ = gpu_project(h, argv, "sum")
    mex.set_clip(h, plane)
    img, n, _ = gpu_project(h, argv, "sum")
    assert (n > 0).sum() >= 50 and ((n == 0) & (n_plain > 0)).sum() >= 50 and (n <= n_plain).all()
    for c in range(3):
        want = (((Fe * n) * tstep) * AXIS_ARGS[6][c]).astype(F)
        assert bits_equal(img[:, :, c], want), f"dimension {j}, channel {c}"
    with CR.clipped(plane):  # and the reference agrees
        ref, rn = PR.project_both(S, hs, *AXIS_ARGS)
    assert PR.same_bits(img, ref[PR.SUM][0]) == 1.0 and PR.same_bits(n, ref[PR.SUM][1]) == 1.0
    vr.volumeRender("delete", h)
    h = new_handle(np.asfortranarray(F(1) - vj))
    mex.set_clip(h, plane)
    img0, n0, _ = gpu_project(h, argv, "sum")
    assert bits_equal(n0, n) and (img0[n0 > 0] == 0).all()
    mex.set_clip(h, None)
    assert gpu_project(h, argv, "sum")[0].max() > 0  # (the complementary half is there)
    vr.volumeRender("delete", h)


# ---- 3. a plane parallel to a ray -------------------------------------------------------------------------

def test_plane_parallel_to_the_central_ray():
    """Unrotated camera, focal length 2: the central pixel's ray is o = (0, 0, -6), d = (0, 0, 1)
    exactly, q_ray = (0.5, 0.5, .).  A plane with normal e_0 has sd == 0 on it: the ray is kept for
    offset >= -0.5 = -n . q_ray and a miss just below."""
    em = np.asfortranarray(np.random.default_rng(9).random((8, 8, 8), dtype=F) + F(0.25))
    args = [F([1, 0.4, 0.6]), F([1, 1, 1]), np.uint64([16, 20]), np.flip(np.eye(3), 0).astype(F), F([0, 2, 6]), F(0.9),
            F([1, 1, 1])]
    S, hs = PR.session(em, STAMP_EM)
    P, keep, _ = S.params(hs, None, None, *args)
    R = PR.rays(P)
    cy, cx = 8, 10
    assert [float(R["d"][k][cy, cx]) for k in range(3)] == [0.0, 0.0, 1.0] and R["hit"][cy, cx]
    del keep
    h = new_handle(em)
    argv = [False, False] + args
    seen = {}
    for tag, off in (("on", F(-0.5)), ("above", np.nextafter(F(-0.5), F(0))), ("below", np.nextafter(F(-0.5), F(-1)))):
        plane = F([[1, 0, 0, off]])
        mex.set_clip(h, plane)
        with CR.clipped(plane):
            ref, n = PR.project_both(S, hs, *args)
        for mode, code in MODES:
            img, aux, _ = gpu_project(h, argv, mode)
            assert PR.same_bits(img, ref[code][0]) == 1.0 and PR.same_bits(aux, ref[code][1]) == 1.0, (tag, mode)
        seen[tag] = int(n[cy, cx]), float(aux[cy, cx])
    assert seen["on"][0] > 0 and seen["on"] == seen["above"] and seen["below"] == (0, 0.0)
    # (kept whole: the parallel plane moves neither end of the ray)
    mex.set_clip(h, None)
    assert gpu_project(h, argv, "sum")[1][cy, cx] == seen["on"][1]
    vr.volumeRender("delete", h)


# ---- 4. the cut face of an isosurface ---------------------------------------------------------------------

def test_cut_face_depth_is_the_clipped_tnear():
    em = np.ones((24, 24, 24), F, order="F")
    args = [F([1, 0.4, 0.6]), F([1, 1, 1]), np.uint64([40, 48]), np.flip(O.rotation(125, 25, 0), 0).astype(F),
            F([0, 3, 6]), F(0.9), F([1, 1, 0])]
    S, hs = PR.session(em, STAMP_EM)
    # through the centre, facing the camera (the normal is about the viewing direction): the far half is kept
    plane = F([[0.42, -0.74, -0.52, 0.42]])
    with CR.clipped(plane):
        ref = IR.isosurface(S, hs, 0.5, None, None, *args)
        P, keep, _ = S.params(hs, None, None, *args)
        R = PR.rays(P)
        del keep
    h = new_handle(em)
    mex.set_clip(h, plane)
    img, depth, normal, (visited, _, surface) = gpu_iso(h, [False, False] + args, 0.5, count=True)
    face = R["hit"] & (R["tnear"] > R["tnear0"])  # rays that enter through the plane
    assert face.sum() >= 50 and (R["hit"] & ~face).sum() >= 50  # (and rays that enter through a box face)
    assert np.array_equal(depth[face].view(np.uint32), R["tnear"][face].view(np.uint32))
    assert PR.same_bits(depth, ref["depth"]) == 1.0 and np.array_equal(np.isnan(depth), ~R["hit"])
    assert (ref["k"][R["hit"]] == 0).all() and surface == visited == int(R["hit"].sum())
    assert PR.same_bits(img, ref["img"]) == 1.0 and (img[R["hit"]][:, 0] == F(1)).all()  # Fe * 1 * color
    vr.volumeRender("delete", h)


# ---- 5. stereo ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("exact", [False, True])
def test_clipped_stereo_is_the_two_clipped_renders(exact, monkeypatch):
    p = product_scene("hg2_compute_32")
    h = handle_of(p, CR.WEDGE)
    base = F(0.1)
    monkeypatch.setenv("VR_EXACT_SHADE", "1" if exact else "0")
    left, right = vr.volumeRender("render_stereo", h, *argv_of(p), base)
    eyes = []
    for off in (-base, base):
        a = argv_of(p)
        a[6] = F([off, a[6][1], a[6][2]])
        eyes.append(vr.volumeRender("render", h, *a))
    monkeypatch.delenv("VR_EXACT_SHADE")
    assert bits_equal(left, eyes[0]) and bits_equal(right, eyes[1])
    assert left.max() > 0 and not bits_equal(left, right)
    mex.set_clip(h, None)
    l0, r0 = vr.volumeRender("render_stereo", h, *argv_of(p), base)
    assert not bits_equal(l0, left) and not bits_equal(r0, right)  # (the planes cut both eyes)
    vr.volumeRender("delete", h)


# ---- 6. unsupported paths, and everything restored once the set is cleared ------------------------------------

def test_unsupported_paths_and_restore(monkeypatch):
    import torch
    p = product_scene("hg2_compute_32")
    argv = argv_of(p)
    H, W = PR.FRAMES["hg2_compute_32"]
    em, re = V(p["em"], STAMP_EM), V(F(1.0), STAMP_RE)
    L = _lib.lib()
    state = torch.zeros(mex.SLAB_PLANES * W * H, dtype=torch.float32, device="cuda")
    ra, keep = mex.render_args(*argv)
    d = p["em"].shape[2]

    def slab(h):
        state.zero_()
        mex.render_slab(h, ra, mex.slab(d, 0, -np.inf, np.inf, 0), 0, state.data_ptr())
        torch.cuda.synchronize()
        return state.cpu().numpy().copy()

    def paths(h):
        tf = TF_VALUE
        out = dict(render=vr.volumeRender("render", h, *argv), kernel=mex.last_march_kernel(),
                   stereo=np.stack(vr.volumeRender("render_stereo", h, *argv, F(0.1))),
                   channels=vr.volumeRender("render_channels", [(h, np.uint64(0), [em, re, em], argv)])[0],
                   slab=slab(h), mip=np.stack(gpu_project(h, argv, "mip")[0:1]), iso=gpu_iso(h, argv, 0.3)[1],
                   tf=gpu_transfer(h, argv, tf)[0])
        return out

    h = handle_of(p)
    before = paths(h)
    assert before["render"].max() > 0 and "march_kernel" in before["kernel"]
    mex.set_clip(h, CR.WEDGE)
    cut = vr.volumeRender("render", h, *argv)
    assert not bits_equal(cut, before["render"])
    assert mex.last_march_kernel() == before["kernel"]  # (the clipped render is not a march launch)
    with pytest.raises(vr.VrError, match="clip planes") as e:
        vr.volumeRender("render_channels", [(h, np.uint64(0), [em, re, em], argv)])
    assert e.value.code == 5
    with pytest.raises(vr.VrError, match="clip planes") as e:
        mex.render_slab(h, ra, mex.slab(d, 0, -np.inf, np.inf, 0), 0, state.data_ptr())
    assert e.value.code == 5
    mex.set_clip(h, None)
    after = paths(h)
    assert after["kernel"] == before["kernel"]
    for k in before:
        if k != "kernel":
            assert PR.same_bits(after[k], before[k]) == 1.0, k
    vr.volumeRender("delete", h)
    # a multi-device group handle (device 0 twice, as tests/test_gpu_group.py): every render call refuses
    monkeypatch.setenv("VR_DEVICES", "0,0")
    g = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    vr.volumeRender("sync_volumes", g, np.uint64(0), em, re, em)
    gbefore = vr.volumeRender("render", g, *argv)
    assert bits_equal(gbefore, before["render"])
    mex.set_clip(g, CR.WEDGE)
    assert bits_equal(mex.get_clip(g), CR.WEDGE)
    out = np.zeros(H * W * 3, F)
    d_out = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    gp = mex._handle(g)
    assert L.vr_render(gp, ctypes.byref(ra), out.ctypes.data) == 5 and b"clip planes" in L.vr_last_error()
    assert L.vr_render_stereo(gp, ctypes.byref(ra), ctypes.c_float(0.1), out.ctypes.data, out.ctypes.data) == 5
    assert b"clip planes" in L.vr_last_error()
    assert L.vr_render_device(gp, ctypes.byref(ra), None, d_out.data_ptr(), None, None) == 5
    assert b"clip planes" in L.vr_last_error()
    with pytest.raises(vr.VrError, match="clip planes"):
        vr.volumeRender("render_channels", [(g, np.uint64(0), [em, re, em], argv)])
    mex.set_clip(g, None)
    assert bits_equal(vr.volumeRender("render", g, *argv), gbefore)
    vr.volumeRender("delete", g)
    del keep


# ---- 7. the empty-space leap under a plane -------------------------------------------------------------------

def test_clipped_mip_is_the_same_with_and_without_the_leap(monkeypatch):
    em = block_volume(False)
    # through the block (voxels 34..45, 14..25, 25..36 of 64): part of it is cut away
    plane = F([[0.6, -0.3, 0.74, -(0.6 * 0.62 - 0.3 * 0.31 + 0.74 * 0.48)]])
    argv = [False, False] + BLOCK_ARGS
    h = new_handle(em)
    unclipped = gpu_project(h, argv, "mip", count=True)
    mex.set_clip(h, plane)
    monkeypatch.delenv("VR_PROJ_NO_PROBE", raising=False)
    leap = gpu_project(h, argv, "mip", count=True)
    monkeypatch.setenv("VR_PROJ_NO_PROBE", "1")
    plain = gpu_project(h, argv, "mip", count=True)
    monkeypatch.delenv("VR_PROJ_NO_PROBE")
    assert bits_equal(leap[0], plain[0]) and bits_equal(leap[1], plain[1])
    assert leap[2][0] == plain[2][0] == plain[2][1] and leap[2][1] < leap[2][0]  # the leap ran
    assert leap[2][0] < unclipped[2][0] and not bits_equal(leap[0], unclipped[0])  # and the plane cut
    assert leap[0].max() > 0
    S, hs = PR.session(em, STAMP_EM)
    with CR.clipped(plane):
        ref, n = PR.project_both(S, hs, *BLOCK_ARGS)
    assert PR.same_bits(leap[0], ref[PR.MIP][0]) == 1.0 and PR.same_bits(leap[1], ref[PR.MIP][1]) == 1.0
    assert leap[2][0] == int(n.sum())
    vr.volumeRender("delete", h)
