"""GPU tests of the first-hit isosurface render (vr_render_isosurface / vr_render_isosurface_device,
vr_isosurface.hip) against the CPU reference of tests/isosurface_ref.py and against itself across
the kernel's variants (empty-space leap, column partitions, 64-bit indexing, no lights).

Parity.  Positions, sampler, bisection, gradient and normal are the oracle's operations, so the depth
plane and the three normal planes meet the projections' condition (isosurface_ref.assert_plane: NaN
positions equal, >= 99.9 % of the values identical in bits, none off by more than 1e-2 of the plane's
scale) and are expected identical.  The image differs from the reference only through the device's
acosf, whose last bit can flip one 8-bit LUT weight: the zero and NaN masks are equal, at most 1 % of
the surface pixels have a channel that differs in bits, and no channel differs by more than 1e-2 of
the image maximum.  The measured shares are printed (and recorded in DESIGN.md s11)."""
import ctypes

import numpy as np
import pytest

import isosurface_ref as IR
import oracle as O
import projection_ref as PR
from golden_cases import EX1_LIGHTS, STAMP_EM, STAMP_GRAD, STAMP_LUT, STAMP_RE

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
EX1_R = np.flip(O.rotation(125, 25, 0), 0).astype(F)
BLOCK_ARGS = [F([1, 0.4, 0.6]), F([1, 1, 1]), np.uint64([48, 40]), EX1_R, F([0, 3, 6]), F(0.9), F([1, 1, 0])]
LEAP_ARGS = BLOCK_ARGS[:2] + [np.uint64([96, 80])] + BLOCK_ARGS[3:]  # (the block spans few pixels of 48 x 40)


def V(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def new_handle(em, re=None, grads=None):
    """A fresh handle with `em` synced as emission and absorption (re: the class default Volume(1))."""
    h = vr.volumeRender("new")
    e = V(em, STAMP_EM)
    r = V(F(1.0) if re is None else re, STAMP_RE)
    g = [V(x, STAMP_GRAD) for x in grads] if grads else []
    vr.volumeRender("sync_volumes", h, np.uint64(0), e, r, e, *g)
    return h


def lights_of(arr):
    return [vr.LightSource(l[:3], l[3:]) for l in arr] if arr is not None else False


def argv_of(sc):
    """The nine 'render' arguments of a scene of isosurface_ref.scene()."""
    lut = V(sc["lut"], STAMP_LUT) if sc["lut"] is not None else False
    return [lights_of(sc["lights"]), lut] + list(sc["args"])


def gpu_iso(h, argv, level, part=None, count=False):
    """vr_render_isosurface_device of the frame `argv`: (image [H, W, 3], depth [H, W], normal
    [H, W, 3], (visited, fetched, surface pixels)); for a part the planes are [H, max_cols(, 3)]."""
    import torch
    ra, keep = mex.render_args(*argv)
    H, W = (int(x) for x in np.asarray(argv[4]).reshape(-1))
    cols = W if part is None else mex.partition_columns(W, mex.partition(part.block_cols, 0, part.num_parts))
    out = torch.full((3, cols, H), -7.0, dtype=torch.float32, device="cuda")
    depth = torch.full((cols, H), -7.0, dtype=torch.float32, device="cuda")
    normal = torch.full((3, cols, H), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.zeros(3, dtype=torch.int64, device="cuda")
    mex.render_isosurface_device(h, ra, level, out.data_ptr(), depth.data_ptr(), normal.data_ptr(), part,
                                 steps.data_ptr() if count else 0)
    torch.cuda.synchronize()
    del keep
    s = steps.cpu().numpy()
    return (np.asfortranarray(out.cpu().numpy().transpose(2, 1, 0)), np.asfortranarray(depth.cpu().numpy().T),
            np.asfortranarray(normal.cpu().numpy().transpose(2, 1, 0)), (int(s[0]), int(s[1]), int(s[2])))


def bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32),
                                                 np.ascontiguousarray(b).view(np.uint32))


def planes_equal(a, b):
    return all(bits_equal(x, y) for x, y in zip(a[:3], b[:3]))


def check_against_reference(got, ref, what):
    """The parity condition of the module docstring; returns (share of identical depth / normal values,
    share of surface pixels whose image differs in bits)."""
    img, depth, normal = got[:3]
    shares = [IR.assert_plane(depth, ref["depth"], f"{what} depth")]
    shares += [IR.assert_plane(normal[:, :, c], ref["normal"][:, :, c], f"{what} normal {'xyz'[c]}") for c in range(3)]
    want = ref["img"]
    assert np.array_equal(img == 0, want == 0), f"{what}: zero masks differ"
    assert np.array_equal(np.isnan(img), np.isnan(want)), f"{what}: NaN masks differ"
    surf = ref["k"] >= 0
    nan = np.isnan(want)
    differ = ((img.view(np.uint32) != want.view(np.uint32)) & ~nan).any(2)
    assert not differ[~surf].any()
    share = float(differ[surf].mean()) if surf.any() else 0.0
    fin = np.isfinite(want)
    scale = max(float(np.abs(want[fin]).max()) if fin.any() else 0.0, 1e-30)
    assert np.array_equal(np.isfinite(img), fin)
    dmax = float(np.abs(img[fin].astype(np.float64) - want[fin]).max()) if fin.any() else 0.0
    env = float(np.abs(ref["img64"][fin] - want[fin]).max()) if fin.any() and "img64" in ref else 0.0
    print(f"{what} image: {int(differ.sum())} of {int(surf.sum())} surface pixels differ in bits ({share:.5f}), "
          f"max |d| {dmax:.3g} of maximum {scale:.3g}; |fp32 - fp64| reference envelope {env:.3g}")
    assert share <= 0.01, f"{what}: {share:.5f} of the surface pixels differ in bits"
    assert dmax <= 1e-2 * scale, f"{what}: |d| {dmax} > 1e-2 * {scale}"
    return min(shares), share


# ---- 1. parity with the reference -------------------------------------------------------------------

@pytest.mark.parametrize("name", list(IR.SCENES))
def test_isosurface_equals_the_reference(name):
    sc = IR.scene(name)
    ref, level = sc["ref"], sc["level"]
    # the reference alone: enough surface, and on the random scene both kinds of hit
    assert (ref["k"] >= 0).sum() >= (400 if name == IR.RAND else 1000)
    if name == IR.RAND:
        assert (ref["k"] == 0).sum() > 50 and (ref["k"] > 0).sum() > 50
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    got = gpu_iso(h, argv_of(sc), level, count=True)
    check_against_reference(got, ref, name)
    assert got[3][0] == int(ref["n"].sum()) and got[3][2] == int((ref["k"] >= 0).sum())
    assert planes_equal(gpu_iso(h, argv_of(sc), level), got)  # (the kernel without the counters)
    # the host entry point writes the same planes
    img, depth, normal = vr.volumeRender("render_isosurface", h, *argv_of(sc), level)
    assert bits_equal(img, got[0]) and bits_equal(depth, got[1]) and bits_equal(normal, got[2])
    vr.volumeRender("delete", h)


# ---- 2. the empty-space leap -------------------------------------------------------------------------

def block_volume():
    """64^3 (padded 66^3 >= 2^18 voxels: the smallest with an occupancy map), zero except an
    off-centre 12^3 block of signed random values (the projection leap test's volume)."""
    v = np.zeros((64, 64, 64), F, order="F")
    v[34:46, 14:26, 25:37] = np.random.default_rng(7).random((12, 12, 12), dtype=F) - F(0.5)
    return v


def test_empty_space_leap_changes_no_bit(monkeypatch):
    em, level = block_volume(), 0.05
    S, hs = PR.session(em, STAMP_EM)
    lut = O.hg_lut(32)
    ref = IR.isosurface(S, hs, level, EX1_LIGHTS, O.OVolume(lut, STAMP_LUT), *LEAP_ARGS)
    argv = [lights_of(EX1_LIGHTS), V(lut, STAMP_LUT)] + LEAP_ARGS
    h = new_handle(em)
    monkeypatch.delenv("VR_ISO_NO_PROBE", raising=False)
    leap = gpu_iso(h, argv, level, count=True)
    monkeypatch.setenv("VR_ISO_NO_PROBE", "1")
    plain = gpu_iso(h, argv, level, count=True)
    monkeypatch.delenv("VR_ISO_NO_PROBE")
    assert planes_equal(leap, plain) and planes_equal(leap, gpu_iso(h, argv, level))
    check_against_reference(leap, ref, "block")
    total, surface = int(ref["n"].sum()), int((ref["k"] >= 0).sum())
    assert surface > 50
    assert leap[3][0] == total and plain[3][0] == total
    assert plain[3][1] == plain[3][0]
    assert leap[3][1] < leap[3][0], leap[3]  # the leap ran
    assert leap[3][2] == surface and plain[3][2] == surface
    # level <= 0: a leaped sample (+-0) would hit, so the probe stays off
    zero = gpu_iso(h, argv, 0.0, count=True)
    assert zero[3][1] == zero[3][0] == zero[3][2] == int(ref["hit"].sum())
    vr.volumeRender("delete", h)


# ---- 3. level 0: every ray that meets the box has its surface at the first sample -------------------------

def test_level_zero_on_a_shell_scene():
    sc = IR.scene("hg2_compute_32", level=0.0)
    ref = sc["ref"]
    assert np.array_equal(ref["k"] == 0, ref["hit"]) and ref["hit"].sum() > 1000 and (ref["k"][~ref["hit"]] == -1).all()
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    got = gpu_iso(h, argv_of(sc), 0.0, count=True)
    check_against_reference(got, ref, "level 0")
    assert bits_equal(got[1][ref["hit"]], ref["tnear"][ref["hit"]])
    assert got[3][1] == got[3][0] == got[3][2] == int(ref["hit"].sum())
    vr.volumeRender("delete", h)


# ---- 4. column partition ----------------------------------------------------------------------------

def test_partitioned_isosurface_assembles_to_the_whole_frame():
    import torch
    sc = IR.scene("stereo_right_24")
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    (H, W), level = sc["res"], sc["level"]
    bc, nparts = 16, 3
    assert W == 82
    maxc = mex.partition_columns(W, mex.partition(bc, 0, nparts))
    whole = gpu_iso(h, argv_of(sc), level, count=True)
    parts = torch.zeros((2, nparts, 3, maxc, H), dtype=torch.float32, device="cuda")  # image, normal
    depth = np.full((H, W), -7.0, F, order="F")
    counts = np.zeros(3, np.int64)
    for p in range(nparts):
        pt = mex.partition(bc, p, nparts)
        img_p, depth_p, normal_p, st = gpu_iso(h, argv_of(sc), level, part=pt, count=True)
        parts[0, p] = torch.from_numpy(np.ascontiguousarray(img_p.transpose(2, 1, 0))).cuda()
        parts[1, p] = torch.from_numpy(np.ascontiguousarray(normal_p.transpose(2, 1, 0))).cuda()
        counts += st
        lc = 0  # the part's local columns, in increasing x: blocks p, p + nparts, ...
        for b in range(p, (W + bc - 1) // bc, nparts):
            for x in range(b * bc, min((b + 1) * bc, W)):
                depth[:, x] = depth_p[:, lc]
                lc += 1
        assert lc == mex.partition_columns(W, pt)
    planes = []
    for i in range(2):
        out = torch.zeros((3, W, H), dtype=torch.float32, device="cuda")
        mex.assemble_partitions(parts[i].data_ptr(), W, H, bc, nparts, maxc, out.data_ptr())
        torch.cuda.synchronize()
        planes.append(np.asfortranarray(out.cpu().numpy().transpose(2, 1, 0)))
    assert bits_equal(planes[0], whole[0]) and bits_equal(depth, whole[1]) and bits_equal(planes[1], whole[2])
    assert tuple(counts) == whole[3]
    vr.volumeRender("delete", h)


# ---- 5. forced 64-bit indexing ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hg2_compute_32", "hg1_lookup_24"])
def test_forced_64_bit_indexing_changes_no_bit(name, monkeypatch):
    sc = IR.scene(name)
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    monkeypatch.delenv("VR_FORCE_BIG", raising=False)
    a = gpu_iso(h, argv_of(sc), sc["level"])
    monkeypatch.setenv("VR_FORCE_BIG", "1")
    b = gpu_iso(h, argv_of(sc), sc["level"])
    monkeypatch.delenv("VR_FORCE_BIG")
    assert planes_equal(a, b) and (~np.isnan(a[1])).sum() > 1000
    vr.volumeRender("delete", h)


# ---- 6. no lights -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hg2_compute_32", "hg1_lookup_24"])
def test_without_lights_the_image_is_the_emission_term(name):
    sc = IR.scene(name, lights=False)
    ref = sc["ref"]
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    got = gpu_iso(h, argv_of(sc), sc["level"])
    surf = ref["k"] >= 0
    fe, col = F(sc["args"][0][0]), F(sc["args"][6])
    want = np.zeros_like(ref["img"])
    for c in range(3):
        want[:, :, c][surf] = (fe * ref["vstar"][surf]) * col[c]
    assert bits_equal(got[0], want) and bits_equal(got[0], ref["img"]) and (got[0][surf].max(1) > 0).all()
    # the normal plane is still written, by the handle's gradient method
    assert IR.same_bits(got[2], ref["normal"]) == 1.0 and not np.isnan(got[2][surf]).any()
    assert IR.same_bits(got[1], ref["depth"]) == 1.0
    lit = IR.scene(name)["ref"]
    assert IR.same_bits(lit["normal"], ref["normal"]) == 1.0  # (the lights do not enter the normal)
    vr.volumeRender("delete", h)


# ---- 7. degenerate inputs ---------------------------------------------------------------------------

def test_one_voxel_emission():
    em = np.full((1, 1), 2.5, F)
    S, hs = PR.session(em, STAMP_EM)
    argv = [False, False] + BLOCK_ARGS
    h = new_handle(em)
    for level in (3.0, 0.5):  # above the voxel: no surface; below: every ray hits at its first sample
        ref = IR.isosurface(S, hs, level, None, None, *BLOCK_ARGS)
        got = gpu_iso(h, argv, level, count=True)
        check_against_reference(got, ref, f"one voxel, level {level}")
        assert got[3][2] == int((ref["k"] >= 0).sum()) and got[3][0] == int(ref["n"].sum())
        if level > 2.5:
            assert (got[0] == 0).all() and np.isnan(got[1]).all() and np.isnan(got[2]).all() and ref["hit"].any()
        else:
            assert np.array_equal(~np.isnan(got[1]), ref["hit"]) and np.isnan(got[2]).all()  # (a zero gradient)
            assert (got[0][ref["hit"]][:, 0] == F(2.5)).all()
    vr.volumeRender("delete", h)


def test_no_volume_synced_writes_the_miss_values():
    h = vr.volumeRender("new")
    argv = [False, False] + BLOCK_ARGS
    img, depth, normal, _ = gpu_iso(h, argv, 0.3)
    assert (img == 0).all() and np.isnan(depth).all() and np.isnan(normal).all()
    img, depth, normal = vr.volumeRender("render_isosurface", h, *argv, -np.inf)
    assert (img == 0).all() and np.isnan(depth).all() and np.isnan(normal).all()
    vr.volumeRender("delete", h)


# ---- 8. no side effects -----------------------------------------------------------------------------

def test_an_isosurface_between_two_renders_changes_neither():
    sc = IR.scene("hg2_compute_32")
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    first = vr.volumeRender("render", h, *argv_of(sc))
    assert first.max() > 0
    gpu_iso(h, argv_of(sc), sc["level"], count=True)
    vr.volumeRender("render_isosurface", h, *argv_of(sc), sc["level"])
    vr.volumeRender("render_isosurface", h, False, False, *sc["args"], 0.0)  # (the uploaded lights are kept)
    again = vr.volumeRender("render", h, *argv_of(sc))
    assert bits_equal(first, again)
    vr.volumeRender("delete", h)


# ---- 9. errors --------------------------------------------------------------------------------------

def test_isosurface_argument_errors(monkeypatch):
    import torch
    sc = IR.scene("hg2_compute_32")
    L = _lib.lib()
    h = new_handle(sc["em"])
    hp = mex._handle(h)
    ra, keep = mex.render_args(*argv_of(sc))
    H, W = sc["res"]
    out = np.zeros(H * W * 3, F)
    d_out = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    lv = ctypes.c_float(0.3)
    assert L.vr_render_isosurface(hp, ctypes.byref(ra), lv, None, None, None) == 1
    assert b"output is NULL" in L.vr_last_error()
    assert L.vr_render_isosurface_device(hp, ctypes.byref(ra), lv, None, None, None, None, None, None) == 1
    assert b"output is NULL" in L.vr_last_error()
    assert L.vr_render_isosurface(hp, ctypes.byref(ra), ctypes.c_float(float("nan")), out.ctypes.data, None, None) == 1
    bad = mex.partition(8, 3, 3)
    assert L.vr_render_isosurface_device(hp, ctypes.byref(ra), lv, ctypes.byref(bad), d_out.data_ptr(), None, None,
                                         None, None) == 1
    assert L.vr_render_isosurface(hp, ctypes.byref(ra), lv, out.ctypes.data, None, None) == 0  # planes may be NULL
    assert out.max() > 0
    vr.volumeRender("delete", h)
    # a multi-device group handle (device 0 twice): one-device handles only
    monkeypatch.setenv("VR_DEVICES", "0,0")
    g = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    vr.volumeRender("sync_volumes", g, np.uint64(0), V(sc["em"], STAMP_EM), V(F(1.0), STAMP_RE), V(sc["em"], STAMP_EM))
    gp = mex._handle(g)
    assert L.vr_render_isosurface(gp, ctypes.byref(ra), lv, out.ctypes.data, None, None) == 5
    assert b"one-device handles only" in L.vr_last_error()
    assert L.vr_render_isosurface_device(gp, ctypes.byref(ra), lv, None, d_out.data_ptr(), None, None, None, None) == 5
    vr.volumeRender("delete", g)
    del keep
