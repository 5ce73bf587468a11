"""GPU tests of the projection renders (vr_render_projection / vr_render_projection_device,
vr_project.hip): maximum-intensity projection with the depth of the maximum, and the ray sum,
against the CPU reference of tests/projection_ref.py and against themselves across the kernel's
variants (empty-space leap, column partitions, 64-bit indexing, typed uploads).

The parity condition (projection_ref.assert_plane): positions, sampler and addition order are all
the oracle's, so the planes are expected bit-identical; at most 0.1 % of a plane's values may differ
in bits and none by more than 1e-2 x the plane's maximum, NaN positions equal."""
import ctypes

import numpy as np
import pytest

import oracle as O
import projection_ref as PR
from golden_cases import SCENES, STAMP_EM, STAMP_GRAD, STAMP_LUT, STAMP_RE

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402

pytestmark = pytest.mark.gpu

MODES = (("mip", PR.MIP), ("sum", PR.SUM))
EX1_R = np.flip(O.rotation(125, 25, 0), 0).astype(np.float32)


def V(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def new_handle(em, re=None, grads=None):
    """A fresh handle with `em` synced as emission and absorption (re: the class default Volume(1))."""
    h = vr.volumeRender("new")
    e = em if isinstance(em, vr.Volume) else V(em, STAMP_EM)
    r = V(np.float32(1.0) if re is None else re, STAMP_RE)
    g = [V(x, STAMP_GRAD) for x in grads] if grads else []
    vr.volumeRender("sync_volumes", h, np.uint64(0), e, r, e, *g)
    return h


def gpu_project(h, argv, mode, part=None, count=False):
    """vr_render_projection_device of the frame `argv` (the nine 'render' arguments): (image
    [H, W, 3], aux [H, W], (visited, fetched)); for a part the planes are [H, max_cols(, 3)]."""
    import torch
    ra, keep = mex.render_args(*argv)
    H, W = (int(x) for x in np.asarray(argv[4]).reshape(-1))
    cols = W if part is None else mex.partition_columns(W, mex.partition(part.block_cols, 0, part.num_parts))
    out = torch.full((3, cols, H), -7.0, dtype=torch.float32, device="cuda")
    aux = torch.full((cols, H), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.zeros(2, dtype=torch.int64, device="cuda")
    mex.render_projection_device(h, ra, mode, out.data_ptr(), aux.data_ptr(), part, steps.data_ptr() if count else 0)
    torch.cuda.synchronize()
    del keep
    s = steps.cpu().numpy()
    return (np.asfortranarray(out.cpu().numpy().transpose(2, 1, 0)), np.asfortranarray(aux.cpu().numpy().T),
            (int(s[0]), int(s[1])))


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


# ---- the scenes: product-side arguments and, computed once per scene, the reference -------------------

def ragged_volume():
    """17 x 9 x 5, signed, with one +inf and one NaN voxel."""
    v = np.random.default_rng(20241218).random((17, 9, 5), dtype=np.float32) - np.float32(0.5)
    v[12, 2, 1] = np.inf
    v[3, 6, 3] = np.nan
    return np.asfortranarray(v)


def block_volume(negative):
    """64^3 (padded 66^3 >= 2^18 voxels: the smallest with an occupancy map), zero except an
    off-centre 12^3 block of signed random values (negative: only negative ones)."""
    v = np.zeros((64, 64, 64), np.float32, order="F")
    b = np.random.default_rng(7).random((12, 12, 12), dtype=np.float32) - np.float32(0.5)
    v[34:46, 14:26, 25:37] = -np.abs(b) - np.float32(0.01) if negative else b
    return v


RAGGED_ARGS = [np.float32([1.5, 1, 1]), np.float32([1, 2, 3]), np.uint64([41, 32]), EX1_R, np.float32([0, 3, 6]),
               np.float32(0.9), np.float32([1, 0.5, 0.25])]
BLOCK_ARGS = [np.float32([1, 0.4, 0.6]), np.float32([1, 1, 1]), np.uint64([48, 40]), EX1_R, np.float32([0, 3, 6]),
              np.float32(0.9), np.float32([1, 1, 0])]

_cache = {}


def scene(name):
    """name -> dict(em, re, grads, lights, lut, args (the seven arguments after the LUT), ref
    ({mode: (image, aux)}), n (samples per ray), S, hs (the oracle session and handle))."""
    if name in _cache:
        return _cache[name]
    if name in PR.FRAMES:
        S, hs, sc, em = PR.scene_session(name)
        args = PR.frame_args(sc, PR.FRAMES[name])
        lights = [vr.LightSource(l[:3], l[3:]) for l in sc["lights"]]
        d = dict(em=em, re=sc["re"]() if sc["re"] else None, grads=O.matlab_gradient(em) if sc["grads"] else None,
                 lights=lights, lut=V(vr.HenyeyGreenstein(sc["lut"]), STAMP_LUT))
    else:
        em, args = {"ragged": (ragged_volume, RAGGED_ARGS), "block": (lambda: block_volume(False), BLOCK_ARGS),
                    "block_neg": (lambda: block_volume(True), BLOCK_ARGS),
                    "one_voxel": (lambda: np.full((1, 1), 2.5, np.float32), RAGGED_ARGS),
                    "flat": (lambda: np.asfortranarray(np.random.default_rng(5).random((9, 7), dtype=np.float32)),
                             RAGGED_ARGS)}[name]
        em = em()
        S, hs = PR.session(em, STAMP_EM)
        d = dict(em=em, re=None, grads=None, lights=False, lut=False)
    ref, n = PR.project_both(S, hs, *args)
    d.update(args=args, ref=ref, n=n, S=S, hs=hs)
    _cache[name] = d
    return d


def argv_of(sc):
    return [sc["lights"], sc["lut"]] + list(sc["args"])


def check_against_reference(sc, got, mode, code, what):
    img, aux, _ = got
    shares = (PR.assert_plane(img, sc["ref"][code][0], f"{what} {mode} image"),
              PR.assert_plane(aux, sc["ref"][code][1], f"{what} {mode} aux"))
    return shares


# ---- 1. parity with the reference -------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hg2_compute_32", "stereo_right_24", "hg1_lookup_24", "ragged"])
def test_projection_equals_the_reference(name):
    sc = scene(name)
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    for mode, code in MODES:
        got = gpu_project(h, argv_of(sc), mode)
        check_against_reference(sc, got, mode, code, name)
        # the host entry point writes the same planes
        img, aux = vr.volumeRender("render_projection", h, *argv_of(sc), mode)
        assert img.shape == got[0].shape and aux.shape == got[1].shape
        assert bits_equal(img, got[0]) and bits_equal(aux, got[1])
    if name == "ragged":  # the non-finite voxels reach the sum, never the maximum
        assert np.isnan(sc["ref"][PR.SUM][0]).any() and not np.isnan(sc["ref"][PR.MIP][0]).any()
    vr.volumeRender("delete", h)


# ---- 2. counters -------------------------------------------------------------------------------------

def test_visited_samples_equal_the_oracles_count():
    sc = scene("hg2_compute_32")
    h = new_handle(sc["em"])
    # the oracle with an opacity threshold that is never reached: Fa = 0, thr = 1, no lights
    _, total = sc["S"].render(sc["hs"], None, None, *PR.frame_args(SCENES["hg2_compute_32"], PR.FRAMES["hg2_compute_32"],
                                                                   factors=[1, .4, 0], thr=1))
    assert total == int(sc["n"].sum())
    for mode, _ in MODES:
        _, _, (visited, fetched) = gpu_project(h, argv_of(sc), mode, count=True)
        assert visited == total
        assert fetched == visited  # (a 32^3 volume has no occupancy map: nothing is leaped)
    vr.volumeRender("delete", h)


# ---- 3. the empty-space leap -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["block", "block_neg"])
def test_empty_space_leap_changes_no_bit(name, monkeypatch):
    sc = scene(name)
    h = new_handle(sc["em"])
    total = int(sc["n"].sum())
    for mode, code in MODES:
        monkeypatch.delenv("VR_PROJ_NO_PROBE", raising=False)
        leap = gpu_project(h, argv_of(sc), mode, count=True)
        monkeypatch.setenv("VR_PROJ_NO_PROBE", "1")
        plain = gpu_project(h, argv_of(sc), mode, count=True)
        monkeypatch.delenv("VR_PROJ_NO_PROBE")
        uncounted = gpu_project(h, argv_of(sc), mode)  # (the kernel without the counters)
        assert bits_equal(leap[0], plain[0]) and bits_equal(leap[1], plain[1]), mode
        assert bits_equal(leap[0], uncounted[0]) and bits_equal(leap[1], uncounted[1]), mode
        check_against_reference(sc, leap, mode, code, name)
        assert leap[2][0] == total and plain[2][0] == total
        assert plain[2][1] == plain[2][0]
        assert leap[2][1] < leap[2][0], leap[2]  # the leap ran
    if name == "block_neg":  # rays through the block still see the zeros around it: maximum +0
        m = sc["ref"][PR.MIP][0][:, :, 0]
        assert (m[sc["n"] > 0] == 0).all() and not np.signbit(m).any()
    vr.volumeRender("delete", h)


# ---- 4. column partition ----------------------------------------------------------------------------

def test_partitioned_projection_assembles_to_the_whole_frame():
    import torch
    sc = scene("stereo_right_24")
    h = new_handle(sc["em"], sc["re"])
    H, W = PR.FRAMES["stereo_right_24"]
    bc, nparts = 8, 3
    assert W == 41
    maxc = mex.partition_columns(W, mex.partition(bc, 0, nparts))
    for mode, _ in MODES:
        whole = gpu_project(h, argv_of(sc), mode, count=True)
        parts = torch.zeros((nparts, 3, maxc, H), dtype=torch.float32, device="cuda")
        aux = np.full((H, W), -7.0, np.float32, order="F")
        visited = 0
        for p in range(nparts):
            pt = mex.partition(bc, p, nparts)
            img_p, aux_p, st = gpu_project(h, argv_of(sc), mode, part=pt, count=True)
            parts[p] = torch.from_numpy(np.ascontiguousarray(img_p.transpose(2, 1, 0))).cuda()
            visited += st[0]
            lc = 0  # the part's local columns, in increasing x: blocks p, p + nparts, ...
            for b in range(p, (W + bc - 1) // bc, nparts):
                for x in range(b * bc, min((b + 1) * bc, W)):
                    aux[:, x] = aux_p[:, lc]
                    lc += 1
            assert lc == mex.partition_columns(W, pt)
        out = torch.zeros((3, W, H), dtype=torch.float32, device="cuda")
        mex.assemble_partitions(parts.data_ptr(), W, H, bc, nparts, maxc, out.data_ptr())
        torch.cuda.synchronize()
        img = np.asfortranarray(out.cpu().numpy().transpose(2, 1, 0))
        assert bits_equal(img, whole[0]) and bits_equal(aux, whole[1]), mode
        assert visited == whole[2][0]
    vr.volumeRender("delete", h)


# ---- 5. forced 64-bit indexing ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hg2_compute_32", "block"])
def test_forced_64_bit_indexing_changes_no_bit(name, monkeypatch):
    sc = scene(name)
    h = new_handle(sc["em"])
    for mode, _ in MODES:
        monkeypatch.delenv("VR_FORCE_BIG", raising=False)
        a = gpu_project(h, argv_of(sc), mode)
        monkeypatch.setenv("VR_FORCE_BIG", "1")
        b = gpu_project(h, argv_of(sc), mode)
        monkeypatch.delenv("VR_FORCE_BIG")
        assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]), mode
    vr.volumeRender("delete", h)


# ---- 6. typed upload --------------------------------------------------------------------------------

def test_uint8_volume_projects_as_its_fp32_twin():
    u8 = np.asfortranarray(np.random.default_rng(11).integers(0, 256, (19, 13, 11), dtype=np.uint8))
    raw = vr.RawVolume(u8)
    raw.TimeLastUpdate = np.uint64(STAMP_EM)
    argv = [False, False] + RAGGED_ARGS
    h8, h32 = new_handle(raw), new_handle(u8.astype(np.float32))
    for mode, _ in MODES:
        a, b = gpu_project(h8, argv, mode), gpu_project(h32, argv, mode)
        assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1]), mode
        assert a[0].max() > 0
    vr.volumeRender("delete", h8)
    vr.volumeRender("delete", h32)


# ---- 7. degenerate textures -------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["one_voxel", "flat"])
def test_degenerate_textures(name):
    sc = scene(name)
    h = new_handle(sc["em"])
    for mode, code in MODES:
        got = gpu_project(h, argv_of(sc), mode)
        check_against_reference(sc, got, mode, code, name)
    assert (sc["n"] > 0).any()
    vr.volumeRender("delete", h)


def test_no_volume_synced_writes_the_miss_values():
    h = vr.volumeRender("new")
    argv = [False, False] + RAGGED_ARGS
    for mode, code in MODES:
        img, aux, _ = gpu_project(h, argv, mode)
        assert (img == 0).all()
        assert np.isnan(aux).all() if code == PR.MIP else (aux == 0).all()
    vr.volumeRender("delete", h)


# ---- 8. no side effects -----------------------------------------------------------------------------

def test_a_projection_between_two_renders_changes_neither():
    sc = scene("hg2_compute_32")
    h = new_handle(sc["em"])
    first = vr.volumeRender("render", h, *argv_of(sc))
    assert first.max() > 0
    for mode, _ in MODES:
        gpu_project(h, argv_of(sc), mode, count=True)
        vr.volumeRender("render_projection", h, False, False, *sc["args"], mode)
    # (lights and LUT as the logical false: a 'render' would keep the uploaded ones too, render.cpp:145)
    again = vr.volumeRender("render", h, *argv_of(sc))
    assert bits_equal(first, again)
    vr.volumeRender("delete", h)


# ---- 9. errors --------------------------------------------------------------------------------------

def test_projection_argument_errors(monkeypatch):
    import torch
    sc = scene("hg2_compute_32")
    L = _lib.lib()
    h = new_handle(sc["em"])
    hp = mex._handle(h)
    ra, keep = mex.render_args(*argv_of(sc))
    H, W = PR.FRAMES["hg2_compute_32"]
    out = np.zeros(H * W * 3, np.float32)
    d_out = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    assert L.vr_render_projection(hp, ctypes.byref(ra), 2, out.ctypes.data, None) == 1
    assert b"projection mode" in L.vr_last_error()
    assert L.vr_render_projection_device(hp, ctypes.byref(ra), -1, None, d_out.data_ptr(), None, None, None) == 1
    assert L.vr_render_projection(hp, ctypes.byref(ra), 0, None, None) == 1
    assert b"output is NULL" in L.vr_last_error()
    assert L.vr_render_projection_device(hp, ctypes.byref(ra), 1, None, None, None, None, None) == 1
    assert b"output is NULL" in L.vr_last_error()
    bad = mex.partition(8, 3, 3)
    assert L.vr_render_projection_device(hp, ctypes.byref(ra), 0, ctypes.byref(bad), d_out.data_ptr(), None, None,
                                         None) == 1
    assert L.vr_render_projection(hp, ctypes.byref(ra), 0, out.ctypes.data, None) == 0  # aux may be NULL
    vr.volumeRender("delete", h)
    # a multi-device group handle (device 0 twice): one-device handles only
    monkeypatch.setenv("VR_DEVICES", "0,0")
    g = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    vr.volumeRender("sync_volumes", g, np.uint64(0), V(sc["em"], STAMP_EM), V(np.float32(1.0), STAMP_RE),
                    V(sc["em"], STAMP_EM))
    gp = mex._handle(g)
    assert L.vr_render_projection(gp, ctypes.byref(ra), 0, out.ctypes.data, None) == 5
    assert b"one-device handles only" in L.vr_last_error()
    assert L.vr_render_projection_device(gp, ctypes.byref(ra), 0, None, d_out.data_ptr(), None, None, None) == 5
    vr.volumeRender("delete", g)
    del keep
