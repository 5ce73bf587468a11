"""GPU tests of the slice views (vr_render_slice / vr_render_slice_device, vr_slice.hip) against the CPU
reference of tests/slice_ref.py.  The sampler, the coordinates and the reduction order are all the
contract's and there is no transcendental: every plane -- image, aux, labels -- is expected
bit-identical (projection_ref.same_bits(...) == 1.0), on both sides of VR_SLICE_LANES."""
import ctypes

import numpy as np
import pytest

import projection_ref as PR
import slice_ref as SR

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
STAMP_EM, STAMP_RE, STAMP_AB = 21, 22, 23
NS = (1, 2, 5, 33)
SOURCES = ("emission", "absorption", "reflection")


def V(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def fresh_handle():
    """A new handle on reset module-global bindings and slot indices ('delete' resets them, as the
    reference's cudaDeviceReset): whatever an earlier test left bound is gone."""
    vr.volumeRender("delete", vr.volumeRender("new"))
    return vr.volumeRender("new")


def new_handle(em, ab=None, re=None):
    """A fresh handle with `em` synced as emission, `ab` (default: em itself) as absorption and `re`
    (default: the class default Volume(1)) as reflection."""
    h = fresh_handle()
    e = em if isinstance(em, (vr.Volume, vr.RawVolume)) else V(em, STAMP_EM)
    a = e if ab is None else V(ab, STAMP_AB)
    r = V(F(1.0) if re is None else re, STAMP_RE)
    vr.volumeRender("sync_volumes", h, np.uint64(0), e, r, a)
    return h


def gpu_slice(h, s, mode, source="emission"):
    """The host command: (image, aux, labels), each [H, W]."""
    return vr.volumeRender("render_slice", h, s.geom(), np.uint64([s.H, s.W]), np.int32(s.n), mode, source)


def gpu_slice_device(h, s, mode, source="emission", stream=0):
    """vr_render_slice_device into torch buffers prefilled with -7: (image, aux, labels) tensors."""
    import torch
    out = torch.full((3, s.W, s.H), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()  # (the fill runs on torch's stream, the slice maybe on another)
    mex.render_slice_device(h, mex.make_slice(s.geom(), [s.H, s.W], s.n, mode, source), out[0].data_ptr(),
                            out[1].data_ptr(), out[2].data_ptr(), stream)
    return out


def planes_of(t):
    import torch
    torch.cuda.synchronize()
    return tuple(np.asfortranarray(t[i].cpu().numpy().T) for i in range(3))


def both_lanes(monkeypatch, fn):
    """fn() under VR_SLICE_LANES=x, =y and unset: the three results."""
    out = []
    for side in ("x", "y", None):
        if side:
            monkeypatch.setenv("VR_SLICE_LANES", side)
        else:
            monkeypatch.delenv("VR_SLICE_LANES", raising=False)
        out.append(fn())
    monkeypatch.delenv("VR_SLICE_LANES", raising=False)
    return out


def assert_same(got, want, what):
    for name, g, w in zip(("image", "aux", "labels"), got, want):
        assert g.shape == w.shape and g.dtype == np.float32, (what, name, g.shape, w.shape)
        assert PR.same_bits(g, w) == 1.0, (what, name)


# ---- scenes and geometries, the reference computed once per (volume, geometry) -----------------------------

def ragged_volume():
    """17 x 9 x 5, signed, with one +inf and one NaN voxel (tests/test_gpu_projection.py's)."""
    v = np.random.default_rng(20241218).random((17, 9, 5), dtype=F) - F(0.5)
    v[12, 2, 1] = np.inf
    v[3, 6, 3] = np.nan
    return np.asfortranarray(v)


def geometries(dims, n):
    """name -> Slice: the three axis families, an oblique plane inside the box and one leaving it; the
    oblique planes 23 x 37, so that a wave and a workgroup are partial on either lane axis."""
    d = list(dims) + [1] * (3 - len(dims))
    g = {f"axis{a}": SR.Slice.of(mex.slice_axis(d, a, (d[a] - 1) * 0.4, n)) for a in range(3)}
    ext = float(min(x for x in d if x > 1)) if max(d) > 1 else 1.0
    g["oblique_in"] = SR.Slice.of(mex.slice_oblique(d, [1, 1, 1], [0.5, 0.5, 0.5], [0.3, -0.5, 1], [1, 0.2, 0],
                                                    ext / 90, 23, 37, n))
    g["oblique_out"] = SR.Slice.of(mex.slice_oblique(d, [1, 1.5, 0.7], [0.45, 0.55, 0.5], [1, 0.6, -0.4], [0, 0, 1],
                                                     max(d) / 30, 37, 23, n))
    return g


_ref = {}


def reference(key, vol, s, labels=None):
    if key not in _ref:
        _ref[key] = SR.render_all(vol, s, labels)
    return _ref[key]


# ---- 1. parity with the reference: sources, modes, slab lengths, both lane axes ----------------------------

def oracle_sources(em, ab, re):
    """What a 'render' samples as emission, absorption and reflection after this sync on a fresh process
    state, by the reference's host model (oracle.OracleSession: a separately uploaded absorption volume
    is NOT what the absorption slot index points to -- the index moves only through the alias rule)."""
    import oracle as O
    S = O.OracleSession()
    hs = S.new()
    e, a, r = O.OVolume(em, STAMP_EM), O.OVolume(ab, STAMP_AB), O.OVolume(re, STAMP_RE)
    S.sync_volumes(hs, 0, e, a if re is ab else r, a)  # (Emission, Reflection, Absorption)
    return [SR.source_volume(S, i) for i in range(3)]


# (name of the binding case) -> (absorption, reflection) given the emission volume
SEPARATE = np.asfortranarray(np.random.default_rng(5).random((7, 11, 6), dtype=F))  # its own dims
BINDINGS = {"separate": lambda em: (SEPARATE, np.full((1, 1), 1.0, F)),  # reflection: the class default Volume(1)
            "ab_is_re": lambda em: (SEPARATE, SEPARATE)}                 # one Volume as absorption and reflection


@pytest.mark.parametrize("n", NS)
def test_ragged_volume_equals_the_reference(n, monkeypatch):
    em = ragged_volume()
    nan_pixels = inside_pixels = 0
    grids = set()
    for case, mk in BINDINGS.items():
        ab, re = mk(em)
        vols = oracle_sources(em, ab, re)
        grids |= {v.shape for v in vols if v is not None}
        h = fresh_handle()
        va = V(ab, STAMP_AB)
        vr.volumeRender("sync_volumes", h, np.uint64(0), V(em, STAMP_EM), va if re is ab else V(re, STAMP_RE), va)
        for name, s in geometries(em.shape, n).items():
            for i, source in enumerate(SOURCES):
                ref = reference((case, name, n, source), vols[i], s)
                for mode, code in SR.MODES:
                    for got in both_lanes(monkeypatch, lambda: gpu_slice(h, s, mode, source)):
                        assert_same(got, ref[code], (case, name, n, source, mode))
                nan_pixels += int(np.isnan(ref[SR.SUM][0]).sum())
                inside_pixels += int((ref[SR.SUM][1] > 0).sum())
            dev = planes_of(gpu_slice_device(h, s, "sum"))
            assert_same(dev, reference((case, name, n, "emission"), vols[0], s)[SR.SUM], (case, name, n, "device"))
        vr.volumeRender("delete", h)
    assert nan_pixels > 100 and inside_pixels > 1000  # pixels outside the box, NaN voxels; and real samples
    assert grids == {(17, 9, 5), (7, 11, 6), (1, 1, 1)}  # a grid through another slot, and the single voxel


@pytest.mark.parametrize("scene", ["flat", "one_voxel"])
def test_degenerate_textures(scene, monkeypatch):
    em = {"flat": lambda: np.asfortranarray(np.random.default_rng(5).random((9, 7), dtype=F)),
          "one_voxel": lambda: np.full((1, 1), 2.5, F)}[scene]()
    h = new_handle(em)
    for n in (1, 5):
        for name, s in geometries(em.shape, n).items():
            ref = reference((scene, name, n), em, s)
            for mode, code in SR.MODES:
                for got in both_lanes(monkeypatch, lambda: gpu_slice(h, s, mode)):
                    assert_same(got, ref[code], (scene, name, n, mode))
            if scene == "one_voxel":
                ins = ref[SR.SUM][1] > 0
                assert ins.any() and (ref[SR.MAX][0][ins] == 2.5).all()
    vr.volumeRender("delete", h)


def test_unbound_sources_read_zero(monkeypatch):
    h = fresh_handle()  # nothing synced: every texture unbound
    s = geometries((8, 8, 8), 5)["oblique_out"]
    ref = SR.render_all(None, s)
    assert (ref[SR.SUM][1] > 0).any() and np.isnan(ref[SR.SUM][0]).any()
    for source in SOURCES:
        for mode, code in SR.MODES:
            for got in both_lanes(monkeypatch, lambda: gpu_slice(h, s, mode, source)):
                assert_same(got, ref[code], (source, mode))
    vr.volumeRender("delete", h)


def test_an_empty_image_writes_nothing():
    h = new_handle(ragged_volume())
    for H, W in ((0, 5), (5, 0), (0, 0)):
        s = SR.Slice([0.5, 0.5, 0.5], [0.01, 0, 0], [0, 0.01, 0], [0, 0, 0.01], H, W, 2)
        got = gpu_slice(h, s, "max")
        assert all(p.shape == (H, W) for p in got)
        L = _lib.lib()
        cs = mex.make_slice(s.geom(), [H, W], 2, "max", "emission")
        assert L.vr_render_slice_device(mex._handle(h), ctypes.byref(cs), None, None, None, None) == 0
    vr.volumeRender("delete", h)


# ---- 2. the axis identity against Data itself ---------------------------------------------------------------

def test_every_axis_slice_of_integer_data_is_the_indexed_array(monkeypatch):
    dims = (16, 12, 20)
    data = np.asfortranarray(np.random.default_rng(17).integers(0, 256, dims, dtype=np.uint8).astype(F))
    h = new_handle(data)
    count = 0
    for axis in range(3):
        for i in range(dims[axis]):
            s = SR.Slice.of(mex.slice_axis(dims, axis, i, 1))
            want = np.take(data, i, axis=axis)
            for got in both_lanes(monkeypatch, lambda: gpu_slice(h, s, "max")):
                assert PR.same_bits(got[0], want) == 1.0 and (got[1] == 0).all() and np.isnan(got[2]).all()
            count += 1
        d = dims[axis]
        s = SR.Slice.of(mex.slice_axis(dims, axis, (d - 1) / 2, d))
        for (img, aux, _), (wi, wa) in ((gpu_slice(h, s, "max"), (data.max(axis=axis), data.argmax(axis=axis))),
                                        (gpu_slice(h, s, "min"), (data.min(axis=axis), data.argmin(axis=axis))),
                                        (gpu_slice(h, s, "sum"), (data.sum(axis=axis, dtype=np.float64), d))):
            assert np.array_equal(img, np.asarray(wi, F)) and np.array_equal(aux, np.broadcast_to(F(wa), aux.shape))
    assert count == 16 + 12 + 20
    vr.volumeRender("delete", h)


def test_uint8_upload_slices_as_single_of_data(monkeypatch):
    u8 = np.asfortranarray(np.random.default_rng(11).integers(0, 256, (19, 13, 11), dtype=np.uint8))
    raw = vr.RawVolume(u8)
    raw.TimeLastUpdate = np.uint64(STAMP_EM)
    h = new_handle(raw)
    for axis, i in ((0, 7), (1, 12), (2, 0)):
        s = SR.Slice.of(mex.slice_axis(u8.shape, axis, i, 1))
        for got in both_lanes(monkeypatch, lambda: gpu_slice(h, s, "max")):
            assert PR.same_bits(got[0], np.take(u8, i, axis=axis).astype(F)) == 1.0
    vr.volumeRender("delete", h)


# ---- 3. 64-bit indexing ---------------------------------------------------------------------------------------

def test_forced_64_bit_indexing_equals_the_reference(monkeypatch):
    em = np.asfortranarray(np.random.default_rng(64).random((64, 64, 64), dtype=F) - F(0.25))
    h = new_handle(em)
    g = geometries(em.shape, 5)
    big_oblique = SR.Slice.of(mex.slice_oblique(em.shape, [1, 1, 1], [0.5, 0.5, 0.5], [0.3, -0.5, 1], [1, 0.2, 0],
                                                1.3, 64, 64, 2))
    for name, s in (("axis1", g["axis1"]), ("oblique_out", g["oblique_out"]), ("big_oblique", big_oblique)):
        ref = reference(("r64", name), em, s)
        for mode, code in SR.MODES:
            plain = gpu_slice(h, s, mode)
            monkeypatch.setenv("VR_FORCE_BIG", "1")
            for got in both_lanes(monkeypatch, lambda: gpu_slice(h, s, mode)):
                assert_same(got, ref[code], (name, mode, "big"))
            monkeypatch.delenv("VR_FORCE_BIG")
            assert_same(plain, ref[code], (name, mode))
    assert np.isnan(reference(("r64", "big_oblique"), em, big_oblique)[SR.SUM][0]).any()
    vr.volumeRender("delete", h)


# ---- 4. labels ------------------------------------------------------------------------------------------------

def test_label_plane_and_label_gains(monkeypatch):
    em = ragged_volume()
    labels = np.asfortranarray(np.random.default_rng(9).integers(0, 4, em.shape, dtype=np.uint8))
    gains = F([1, 0.25, -2, 0])
    h = new_handle(em)
    slices = geometries(em.shape, 5)
    for name, s in slices.items():  # without labels the plane is all NaN
        assert np.isnan(gpu_slice(h, s, "max")[2]).all()
    mex.sync_labels(h, labels)
    seen = set()
    for name, s in slices.items():
        ref = reference(("labels", name), em, s, labels)
        for mode, code in SR.MODES:
            for got in both_lanes(monkeypatch, lambda: gpu_slice(h, s, mode)):
                assert_same(got, ref[code], (name, mode))
        lab = ref[SR.MAX][2]
        seen |= set(np.unique(lab[np.isfinite(lab)]))
    assert seen == {0, 1, 2, 3} and np.isnan(reference(("labels", "oblique_out"), em, slices["oblique_out"], labels)[0][2]).any()
    # with gains the emission slice is the slice of the host-rewritten volume; the labels stay
    mex.set_label_gains(h, gains)
    em2 = mex.label_gain_host(em, labels, gains)
    assert not np.array_equal(em2.view(np.uint32), em.view(np.uint32))
    for name, s in slices.items():
        ref = reference(("gains", name), em2, s, labels)
        for mode, code in SR.MODES:
            for got in both_lanes(monkeypatch, lambda: gpu_slice(h, s, mode)):
                assert_same(got, ref[code], (name, mode, "gains"))
    mex.sync_labels(h, None)
    assert np.isnan(gpu_slice(h, slices["axis2"], "max")[2]).all()
    vr.volumeRender("delete", h)


def test_a_slice_in_flight_keeps_the_gains_it_was_launched_with():
    import torch
    em = ragged_volume()
    labels = np.asfortranarray(np.random.default_rng(9).integers(0, 4, em.shape, dtype=np.uint8))
    g1, g2 = F([1, 0.25, -2, 0]), F([0.5, 2, 1, 3])
    s = geometries(em.shape, 33)["oblique_out"]
    stream = torch.cuda.Stream()
    h = new_handle(em)
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, g1)
    torch.cuda.synchronize()
    first = gpu_slice_device(h, s, "sum", stream=stream.cuda_stream)
    mex.set_label_gains(h, g2)
    second = gpu_slice_device(h, s, "sum", stream=stream.cuda_stream)
    got = planes_of(first), planes_of(second)
    vr.volumeRender("delete", h)
    for g, planes in zip((g1, g2), got):
        assert_same(planes, SR.render_all(mex.label_gain_host(em, labels, g), s, labels)[SR.SUM], "in flight")
    assert PR.same_bits(got[0][1], got[1][1]) == 1.0 and not np.array_equal(got[0][0].view(np.uint32), got[1][0].view(np.uint32))


# ---- 5. state -------------------------------------------------------------------------------------------------

def test_a_slice_changes_nothing_of_the_handle(monkeypatch):
    import oracle as O
    em = O.shell_volume(24)
    R = np.flip(O.rotation(125, 25, 0), 0).astype(F)
    argv = [False, False, F([1.5, 0.4, 0.6]), F([1, 1, 1]), np.uint64([40, 52]), R, F([0, 3, 6]), F(0.9), F([1, 1, 0])]
    h = new_handle(em)
    s = geometries(em.shape, 5)["oblique_out"]
    before = vr.volumeRender("render", h, *argv)
    flags = mex.last_launch_flags()
    mip = vr.volumeRender("render_projection", h, *argv, "mip")
    assert mex.last_launch_flags() == flags and before.max() > 0
    plain = [gpu_slice(h, s, m, src) for m in ("max", "sum") for src in SOURCES]
    planes_of(gpu_slice_device(h, s, "min"))
    assert mex.last_launch_flags() == flags
    after = vr.volumeRender("render", h, *argv)
    assert mex.last_launch_flags() == flags
    mip2 = vr.volumeRender("render_projection", h, *argv, "mip")
    assert PR.same_bits(before, after) == 1.0 and PR.same_bits(mip[0], mip2[0]) == 1.0 and PR.same_bits(mip[1], mip2[1]) == 1.0
    # clip planes on the handle do not change a slice
    mex.set_clip(h, F([[1, 0, 0, -0.5], [0, 0.6, 0.8, -0.7]]))
    clipped = [gpu_slice(h, s, m, src) for m in ("max", "sum") for src in SOURCES]
    for a, b in zip(plain, clipped):
        assert_same(a, b, "clip planes set")
    assert np.isfinite(plain[0][0]).any()
    vr.volumeRender("delete", h)
    # a multi-device group handle (device 0 twice): one-device handles only
    monkeypatch.setenv("VR_DEVICES", "0,0")
    g = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    vr.volumeRender("sync_volumes", g, np.uint64(0), V(em, STAMP_EM), V(F(1.0), STAMP_RE), V(em, STAMP_EM))
    with pytest.raises(vr.VrError, match="one-device handles only") as e:
        gpu_slice(g, s, "max")
    assert e.value.code == 5
    with pytest.raises(vr.VrError, match="one-device handles only") as e:
        gpu_slice_device(g, s, "max")
    assert e.value.code == 5
    vr.volumeRender("delete", g)


def test_null_output_is_refused():
    h = new_handle(ragged_volume())
    L = _lib.lib()
    s = mex.make_slice(geometries((17, 9, 5), 1)["axis0"].geom(), [9, 5], 1, "max", "emission")
    out = np.zeros(45, F)
    assert L.vr_render_slice(mex._handle(h), ctypes.byref(s), None, None, None) == 1
    assert b"output is NULL" in L.vr_last_error()
    assert L.vr_render_slice_device(mex._handle(h), ctypes.byref(s), None, None, None, None) == 1
    assert L.vr_render_slice(mex._handle(h), ctypes.byref(s), out.ctypes.data, None, None) == 0  # aux, labels may be NULL
    assert np.isfinite(out).all() and out.any()
    vr.volumeRender("delete", h)
