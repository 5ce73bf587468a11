"""Typed volumes on the GPU (include/vrhip.h vr_dtype): a uint8 / uint16 / int16 / half volume crosses
the link in its own width and the upload's pad pass widens it to fp32, so the resident buffer -- and
with it every image -- is bit for bit that of the fp32 upload of the converted array.  Every test
renders the small HG frame (48 x 40, two lights, on-the-fly gradient: the hg2_compute_32 set-up of
golden_cases.py) from a typed upload and from its fp32 twin and compares the images' uint32 views
with np.array_equal: no tolerance.  (What the fp32 path renders is pinned to the oracle by the
rest of the suite.)"""
import ctypes

import numpy as np
import pytest

import golden_cases as GC

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("volume_renderer_amd")
torch = pytest.importorskip("torch")
from volume_renderer_amd import _lib, mex  # noqa: E402

SC = GC.SCENES["hg2_compute_32"]
RES = [40, 48]  # [H W]
ERR_ARGUMENT, ERR_UNSUPPORTED = 1, 5


class V:
    """Volume-shaped: what the binding reads (Data, TimeLastUpdate), any element type, no cast."""

    def __init__(self, data, stamp):
        self.Data = data if isinstance(data, np.ndarray) and data.flags.f_contiguous else np.asfortranarray(data)
        self.TimeLastUpdate = np.uint64(stamp)


def raw(data, stamp, unorm=False):
    v = vr.RawVolume(data, unorm)
    v.TimeLastUpdate = np.uint64(stamp)
    return v


@pytest.fixture(scope="module")
def lut():
    return V(vr.HenyeyGreenstein(SC["lut"]), GC.STAMP_LUT)


REFL = V(np.ones((1, 1), np.float32), GC.STAMP_RE)


def argv(lut, scale=1.0):
    """The 'render' arguments of the scene; `scale` on the emission and absorption factors brings
    integer voxel values into the range the scene was made for."""
    f = SC["factors"]
    sc = dict(SC, res=RES, factors=[f[0] * scale, f[1], f[2] * scale])
    lights = [vr.LightSource(l[:3], l[3:]) for l in GC.EX1_LIGHTS]
    return GC.render_argv(sc, lights, lut)


def render(lut, em, ab=None, scale=1.0, handle=None):
    h = vr.volumeRender("new") if handle is None else handle
    try:
        vr.volumeRender("sync_volumes", h, np.uint64(0), em, REFL, em if ab is None else ab)
        return vr.volumeRender("render", h, *argv(lut, scale))
    finally:
        if handle is None:
            vr.volumeRender("delete", h)


def bits(img):
    return np.ascontiguousarray(img).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def twin_of(data, unorm=False):
    t = data.astype(np.float32)
    return t / np.float32(np.iinfo(data.dtype).max) if unorm else t


def ragged(dtype, rng):
    """(37, 21, 13): every dimension odd, so no source row starts aligned.  Random, with 0 and the
    type's extremes (negatives for int16; subnormals and -0 for half) in the ray's way."""
    shape = (37, 21, 13)
    if dtype == np.float16:
        d = rng.random(shape, np.float32).astype(np.float16)
        d[10:14, 8:12, 5] = np.array([6e-8, 3e-5, -6e-8, 6.1e-5], np.float16)[:, None]  # subnormals
        d[15, 8:12, 6] = np.float16(-0.0)
        d[20, 10, 6] = np.float16(0.0)
        return np.asfortranarray(d), 1.0
    info = np.iinfo(dtype)
    d = rng.integers(info.min, int(info.max) + 1, shape).astype(dtype)
    d[18, 10, 6], d[19, 10, 6], d[20, 10, 6] = 0, info.max, info.min
    d[0, 0, 0], d[-1, -1, -1] = info.max, info.min
    return np.asfortranarray(d), 1.0 / float(info.max)


@pytest.mark.parametrize("dtype,unorm", [(np.uint8, False), (np.uint8, True), (np.uint16, False), (np.uint16, True),
                                         (np.int16, False), (np.float16, False)])
def test_each_dtype_equals_its_fp32_twin(lut, dtype, unorm):
    d, scale = ragged(dtype, np.random.default_rng(11))
    if unorm:
        scale = 1.0
    ref = render(lut, V(twin_of(d, unorm), 5), scale=scale)
    got = render(lut, raw(d, 5, unorm), scale=scale)
    assert np.isfinite(ref).all() and ref.max() > 0 and len(np.unique(ref)) > 100
    assert same(got, ref)
    # (the twin is also what vr_convert_host gives: host and device share one conversion)
    assert np.array_equal(mex.convert_host(d, unorm).view(np.uint32), twin_of(d, unorm).view(np.uint32))


def test_half_inf_and_nan(lut):
    """One +inf and one NaN, on opposite faces (one of them faces the camera): the converted volume
    is nonfinite exactly as its fp32 twin (the pad folds the statistics of the converted values),
    and the images agree NaN for NaN."""
    d, _ = ragged(np.float16, np.random.default_rng(12))
    d[18, 10, 12] = np.float16(np.inf)
    d[18, 10, 0] = np.float16(np.nan)
    ref = render(lut, V(d.astype(np.float32), 5))
    got = render(lut, raw(d, 5))
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(bits(got)[~nan], bits(ref)[~nan])
    assert not same(ref, render(lut, V(np.nan_to_num(d.astype(np.float32), nan=0.0, posinf=0.0), 5)))


def blob(shape, dtype, rng, lo, hi):
    """Mostly zero with a dense random box [lo, hi) per axis."""
    d = np.zeros(shape, dtype, order="F")
    box = tuple(slice(a, b) for a, b in zip(lo, hi))
    d[box] = rng.integers(1, int(np.iinfo(dtype).max) + 1, d[box].shape).astype(dtype)
    return d


def test_occupancy_map_path(lut):
    """(70, 64, 66): 72 * 66 * 68 padded voxels, above VR_OCC_MIN_VOXELS (2^18), so the occupancy map
    is built from the converted buffer and the march's empty-space probe leaps through it."""
    d = blob((70, 64, 66), np.uint8, np.random.default_rng(13), (20, 18, 25), (45, 40, 50))
    ref = render(lut, V(twin_of(d), 5), scale=1 / 255)
    got = render(lut, raw(d, 5), scale=1 / 255)
    assert ref.max() > 0 and (ref == 0).mean() > 0.2
    assert same(got, ref)


def test_chunked_ring_wraps(lut, monkeypatch):
    """(192, 160, 176) uint8 with VR_UPLOAD_CHUNK_MB=1: 34 planes per chunk, 6 chunks through the
    4-slot staging ring, so slots are reused; against the unchunked upload and the fp32 twin."""
    d = blob((192, 160, 176), np.uint8, np.random.default_rng(14), (40, 30, 3), (150, 130, 173))
    whole = render(lut, raw(d, 5), scale=1 / 255)
    monkeypatch.setenv("VR_UPLOAD_CHUNK_MB", "1")
    chunked = render(lut, raw(d, 5), scale=1 / 255)
    monkeypatch.delenv("VR_UPLOAD_CHUNK_MB")
    ref = render(lut, V(twin_of(d), 5), scale=1 / 255)
    assert ref.max() > 0
    assert same(chunked, whole) and same(whole, ref)


def test_bounce_ring(lut, monkeypatch):
    """VR_UPLOAD_BOUNCE=1, (272, 272, 272) uint16: 40 MB through the pinned bounce ring in three
    16 MiB pieces, the last partial."""
    d = blob((272, 272, 272), np.uint16, np.random.default_rng(15), (60, 50, 1), (210, 220, 271))
    monkeypatch.setenv("VR_UPLOAD_BOUNCE", "1")
    got = render(lut, raw(d, 5), scale=1 / 65535)
    monkeypatch.delenv("VR_UPLOAD_BOUNCE")
    ref = render(lut, V(twin_of(d), 5), scale=1 / 65535)
    assert ref.max() > 0
    assert same(got, ref)


@pytest.mark.parametrize("dtype,unorm", [(np.uint8, False), (np.uint8, True), (np.int16, False), (np.float16, False)])
def test_device_resident_source(lut, dtype, unorm):
    d, scale = ragged(dtype, np.random.default_rng(16))
    if unorm:
        scale = 1.0
    t = torch.from_numpy(np.ascontiguousarray(d.reshape(-1, order="F"))).cuda()
    assert t.dtype in (torch.uint8, torch.int16, torch.float16)
    dv = mex.DeviceVolume.from_tensor(t, dims=d.shape, last_update=5, unorm=unorm)
    got = render(lut, dv, scale=scale)
    ref = render(lut, V(twin_of(d, unorm), 5), scale=scale)
    assert ref.max() > 0
    assert same(got, ref)
    if dtype != np.uint8:
        with pytest.raises(TypeError):
            mex.DeviceVolume.from_tensor(t, dims=d.shape, unorm=True)


def test_dtype_is_part_of_the_identity(lut):
    """One buffer bound as emission through a uint16 view and as absorption through an int16 view,
    same TimeLastUpdate: were the dtype not part of the identity the two would alias (one upload,
    absorption = emission).  Then the emission slot re-synced with the int16 view at the unchanged
    timestamp: now they do alias, and the render changes accordingly."""
    rng = np.random.default_rng(17)
    u = np.asfortranarray(rng.integers(32768 - 600, 32768 + 600, (37, 21, 13)).astype(np.uint16))
    i = u.view(np.int16)
    assert i.ctypes.data == u.ctypes.data and (i < 0).any() and (i > 0).any()
    scale = 1 / 33368
    h = vr.volumeRender("new")
    first = render(lut, V(u, 9), V(i, 9), scale=scale, handle=h)
    second = render(lut, V(i, 9), V(i, 9), scale=scale, handle=h)
    vr.volumeRender("delete", h)
    ref1 = render(lut, V(u.astype(np.float32), 5), V(i.astype(np.float32), 6), scale=scale)
    ref2 = render(lut, V(i.astype(np.float32), 5), scale=scale)
    assert not same(ref1, ref2)
    assert same(first, ref1)
    assert same(second, ref2)


def test_group_handle(lut, monkeypatch):
    """vr_new_multi with device 0 repeated (as test_gpu_group.py): a uint8 sync on the primary, the
    replicas copied from its converted buffer; the assembled image equals the one-device fp32 one."""
    monkeypatch.setenv("VR_GROUP_REPLICATE", "1")
    d = blob((70, 64, 66), np.uint8, np.random.default_rng(18), (10, 8, 5), (60, 50, 60))
    ref = render(lut, V(twin_of(d), 5), scale=1 / 255)
    monkeypatch.setenv("VR_DEVICES", "0,0,0")
    h = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    got = render(lut, raw(d, 5), scale=1 / 255, handle=h)
    vr.volumeRender("delete", h)
    assert ref.max() > 0
    assert same(got, ref)


def test_fused_channels(lut):
    """vr_channel carries vr_volume pointers: a uint8 channel and an fp32 channel through
    render_channels equal their own renders."""
    rng = np.random.default_rng(19)
    d8, _ = ragged(np.uint8, rng)
    f32 = np.asfortranarray(rng.random((24, 30, 17), np.float32))
    # one scale for both channels would change the fp32 one: each channel has its own arguments
    a8, a32 = argv(lut, 1 / 255), argv(lut, 1.0)
    h1, h2 = vr.volumeRender("new"), vr.volumeRender("new")
    e8, e32 = raw(d8, 5), V(f32, 6)
    imgs = vr.volumeRender("render_channels", [(h1, np.uint64(0), [e8, REFL, e8], a8),
                                               (h2, np.uint64(0), [e32, REFL, e32], a32)])
    for h in (h1, h2):
        vr.volumeRender("delete", h)
    ref8 = render(lut, V(twin_of(d8), 5), scale=1 / 255)
    ref32 = render(lut, V(f32, 6))
    assert ref8.max() > 0 and ref32.max() > 0 and not same(ref8, ref32)
    assert same(imgs[0], ref8) and same(imgs[1], ref32)


def _vol(arr, dtype, stamp=5, offset=0):
    v = _lib.VrVolume()
    v.data = arr.ctypes.data + offset
    d = mex._matlab_dims(arr)
    for k in range(3):
        v.dims[k] = d[k]
    v.last_update = stamp
    v.location = _lib.VR_HOST
    v.dtype = dtype
    return v


def test_errors_leave_the_handle_usable(lut):
    L = vr.lib()
    rng = np.random.default_rng(20)
    f32 = np.asfortranarray(rng.random((24, 30, 17), np.float32))
    ref = render(lut, V(f32, 5))
    d16 = np.zeros((8, 6, 4), np.uint16, order="F")
    d8 = np.zeros(8 * 6 * 4 * 2 + 2, np.uint8)
    h = vr.volumeRender("new")
    hp = mex._handle(h)
    refl = mex._vr_volume(REFL)

    def sync(em, dx=None):
        g = [ctypes.byref(dx)] * 3 if dx is not None else [None] * 3
        return L.vr_sync_volumes(hp, 0, ctypes.byref(em), ctypes.byref(refl), ctypes.byref(em), *g)

    def still_fine():
        assert same(render(lut, V(f32, 5), handle=h), ref)

    U = _lib.VR_DTYPE_UNORM
    for code in (5, 99, -1, 0x200 | _lib.VR_U8):  # unknown codes
        assert sync(_vol(d16, code)) == ERR_ARGUMENT, code
        assert "dtype" in L.vr_last_error().decode()
        still_fine()
    for code in (_lib.VR_I16 | U, _lib.VR_F16 | U, _lib.VR_F32 | U):  # UNORM is for U8 / U16
        assert sync(_vol(d16, code)) == ERR_ARGUMENT, code
        still_fine()
    odd = _lib.VrVolume()
    odd.data = d8.ctypes.data + (1 - d8.ctypes.data % 2)
    assert odd.data % 2 == 1
    odd.dims[0], odd.dims[1], odd.dims[2] = 8, 6, 4
    odd.last_update, odd.location = 5, _lib.VR_HOST
    for code in (_lib.VR_U16, _lib.VR_I16, _lib.VR_F16, _lib.VR_U16 | U):  # an odd address, 16-bit types
        odd.dtype = code
        assert sync(odd) == ERR_ARGUMENT, code
        still_fine()
    odd.dtype = _lib.VR_U8  # (bytes may start anywhere)
    assert sync(odd) == 0
    still_fine()
    # a typed gradient volume
    em = mex._vr_volume(V(f32, 5))
    assert sync(em, _vol(np.zeros((24, 30, 17), np.uint8, order="F"), _lib.VR_U8)) == ERR_UNSUPPORTED
    still_fine()
    # a typed illumination LUT
    lut8 = V(np.zeros((16, 16, 16), np.uint8, order="F"), 7)
    vr.volumeRender("sync_volumes", h, np.uint64(0), V(f32, 5), REFL, V(f32, 5))
    with pytest.raises(vr.VrError) as e:
        vr.volumeRender("render", h, *argv(lut8))
    assert e.value.code == ERR_UNSUPPORTED
    still_fine()
    vr.volumeRender("delete", h)


def test_dtype_zero_is_fp32_as_before(lut):
    """A vr_volume whose dtype field is 0 (every existing caller zero-initialises it) renders what
    the Python path renders."""
    L = vr.lib()
    f32 = np.asfortranarray(np.random.default_rng(21).random((24, 30, 17), np.float32))
    ref = render(lut, V(f32, 5))
    h = vr.volumeRender("new")
    em, refl = _vol(f32, 0), mex._vr_volume(REFL)
    assert em.dtype == _lib.VR_F32 == 0
    mex.check(L.vr_sync_volumes(mex._handle(h), 0, ctypes.byref(em), ctypes.byref(refl), ctypes.byref(em),
                                None, None, None))
    got = vr.volumeRender("render", h, *argv(lut))
    vr.volumeRender("delete", h)
    assert ref.max() > 0 and same(got, ref)
