"""GPU tests of the Gaussian smoothing of the resident emission volume (vr_set_smoothing, the passes of
csrc/vr_smooth.hip).

The reference of every test is the product itself on the host-filtered volume: em_s = vr_smooth_host(em,
sigma) -- tied to the numpy restatement of the rule by tests/test_smooth_host.py -- synced the ordinary way
into a fresh handle.  The smoothed handle's result must equal the em_s handle's bit for bit (NaN positions
equal, every other bit equal); nothing is compared under a tolerance except the histogram's double sum,
which has the bound of tests/test_gpu_histogram.py.

The kernels' tiles (csrc/vr_smooth.hip): the pass along dims[0] stages row segments of VR_SMOOTH_SEG = 256
voxels; the passes along dims[1] and dims[2] work on tiles of VR_SMOOTH_TX = 64 voxels along dims[0] by
VR_SMOOTH_TA = 32 along the filtered axis; the fused form works on tiles of VR_SMOOTH_FX = 64 by
VR_SMOOTH_FY = 16 voxels and marches along dims[2] in chunks of VR_SMOOTH_FZ = 256 planes.  Both forms ship
(the host picks by radius); VR_SMOOTH_FORM=passes|fused, a test switch, forces either, and the tests by
position run under both.

Each handle lives alone (the texture bindings are module globals): made, used, deleted."""
import numpy as np
import pytest

from golden_cases import STAMP_EM, STAMP_RE

vr = pytest.importorskip("volume_renderer_amd")
torch = pytest.importorskip("torch")
from volume_renderer_amd import _lib, mex  # noqa: E402
import slice_ref as SLR  # noqa: E402
from test_gpu_clip import argv_of, product_scene  # noqa: E402
from test_gpu_histogram import gpu_hist, query  # noqa: E402
from test_gpu_labels import (GAINS, SCENES, _frames, _same_frames, assert_outputs_equal, channel_volumes, em2_of,  # noqa: E402
                             every_call, mask_labels)
from test_gpu_projection import RAGGED_ARGS, V, gpu_project, new_handle  # noqa: E402
from test_gpu_slice import gpu_slice  # noqa: E402
from test_gpu_transfer import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SIGMA = F([1.0, 0.75, 1.5])
SEG, TX, TA = 256, 64, 32  # csrc/vr_smooth.hip
FX, FY, FZ = 64, 16, 256
FORMS = ("passes", "fused")


def smoothed(em, sigma):
    return np.asfortranarray(mex.smooth_host(np.asarray(em, F), sigma))


def histogram_of(h, data):
    """The emission histogram with the whole finite range of `data` in 64 bins."""
    fin = data[np.isfinite(data)]
    return gpu_hist(h, query(64, (fin.min(), fin.max() if fin.max() > fin.min() else fin.min() + 1)))


def assert_histograms_equal(got, want, data, what):
    (gc, gs), (wc, ws) = got, want
    assert np.array_equal(gc, wc), (what, "counts")
    for k in ("total", "below", "above", "nan", "ninf"):
        assert np.array_equal(gs[k], ws[k]), (what, k, gs[k], ws[k])
    for k in ("min", "max"):
        assert same_bits(gs[k], ws[k]), (what, k, gs[k], ws[k])
    fin = data[np.isfinite(data)].astype(np.float64)
    bound = fin.size * 2.0 ** -53 * float(np.abs(fin).sum())  # n - 1 rounded double additions in any order
    d = abs(float(gs["sum"][0]) - float(ws["sum"][0]))
    print(f"{what}: sum {gs['sum'][0]!r} vs {ws['sum'][0]!r}, |d| {d:.3g}, bound {bound:.3g}")
    assert d <= bound, (what, d, bound)
    assert int(gs["total"][0]) == data.size


# ---- 1. every call ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_every_call_equals_the_host_filtered_volume(name, monkeypatch):
    p = product_scene(name)
    em = p["em"]
    em_s = smoothed(em, SIGMA)
    other = np.asfortranarray(np.flip(em, 0))  # the second channel's volume
    argv = argv_of(p)

    h = new_handle(em, p["re"], p["grads"])
    plain = vr.volumeRender("render", h, *argv)
    mex.set_smoothing(h, SIGMA)
    assert same_bits(mex.get_smoothing(h), SIGMA)
    got = every_call(h, p, monkeypatch)
    got_hist = histogram_of(h, em_s)
    h2 = vr.volumeRender("new")
    chans = vr.volumeRender("render_channels", [(h, np.uint64(0), channel_volumes(em, p), argv),
                                                (h2, np.uint64(0), channel_volumes(other, p), argv)])
    vr.volumeRender("delete", h)
    vr.volumeRender("delete", h2)

    q = dict(p, em=em_s)  # (the gradient volumes of lookup mode stay those of the unmodified data)
    hr = new_handle(em_s, p["re"], p["grads"])
    want = every_call(hr, q, monkeypatch)
    want_hist = histogram_of(hr, em_s)
    h3 = vr.volumeRender("new")
    rchans = vr.volumeRender("render_channels", [(hr, np.uint64(0), channel_volumes(em_s, p), argv),
                                                 (h3, np.uint64(0), channel_volumes(other, p), argv)])
    vr.volumeRender("delete", hr)
    vr.volumeRender("delete", h3)

    assert_outputs_equal(got, want, name)
    assert_histograms_equal(got_hist, want_hist, em_s, name)
    assert same_bits(chans[0], rchans[0]) and same_bits(chans[1], rchans[1]), f"{name}: render_channels differs"
    assert same_bits(chans[0], got["render"]) and not same_bits(chans[1], chans[0])
    assert not same_bits(got["render"], plain) and got["render"].max() > 0, f"{name}: the smoothing changed nothing"


# ---- 2. resident voxels by position -------------------------------------------------------------------------

def _noise(shape, seed):
    return np.asfortranarray(np.random.default_rng(seed).random(shape, dtype=F) - F(0.25))


def all_axis_slices(h, dims):
    """Every voxel plane along every axis: the resident volume by position (one pixel per voxel)."""
    dims = tuple(dims) + (1,) * (3 - len(dims))
    return [gpu_slice(h, SLR.Slice.of(mex.slice_axis(dims, axis, i, 1)), "max")[0]
            for axis in range(3) for i in range(dims[axis])]


# the shapes of tests/test_smooth_host.py, one with every dim beyond its tile (SEG, TA, TA; its padded
# size is also beyond the occupancy map's threshold of 2^18), one with every dim below R = 12
POSITION_CASES = {
    "ragged": ((37, 5, 3), (1, 2, 0.5)), "long_z": ((2, 3, 70), (6, 1, 6)), "flat": ((33, 17, 1), (2, 2, 2)),
    "one_voxel": ((1, 1, 1), (3, 3, 3)), "long_x": ((300, 4, 3), (6, 0, 1)),
    "beyond_the_tiles": ((SEG + 3, TA + 1, TA + 2), (1.5, 6, 2.5)), "below_the_radius": ((7, 11, 5), (6, 6, 6)),
    "one_axis": ((37, 5, 3), (0, 0, 1.5)),
    # beyond the fused form's tile along dims[0] and dims[1] and its chunk along dims[2]; ragged in all three
    "beyond_the_fused_tiles": ((FX + 5, FY + 3, FZ + 7), (1, 1.5, 2)),
    "fused_radius_12": ((FX + 5, FY + 3, 29), (6, 6, 6)),
}


def slices_and_projections(h, shape):
    """Every axis slice (the interior by position), and the two projections of the ragged frame: their
    rays enter through every face, where the trilinear taps weigh the apron."""
    argv = [False, False] + RAGGED_ARGS
    return all_axis_slices(h, shape) + [plane for mode in ("mip", "sum") for plane in gpu_project(h, argv, mode)[:2]]


_position_reference = {}


def position_reference(name):
    """The reference handle's planes, computed once per case and shared by the forms."""
    if name not in _position_reference:
        shape, sigma = POSITION_CASES[name]
        em = _noise(shape, len(name))
        em_s = smoothed(em, sigma)
        hr = new_handle(em_s)
        _position_reference[name] = (em, em_s, slices_and_projections(hr, shape))
        vr.volumeRender("delete", hr)
    return _position_reference[name]


@pytest.mark.parametrize("form", FORMS + (None,))
@pytest.mark.parametrize("name", sorted(POSITION_CASES))
def test_resident_voxels_equal_the_host_filtered_volume_by_position(name, form, monkeypatch):
    """Under each forced form and under the host's own choice (a case with a skipped axis runs the passes
    whatever is forced: the fused form takes three active axes)."""
    shape, sigma = POSITION_CASES[name]
    em, em_s, want = position_reference(name)
    if form:
        monkeypatch.setenv("VR_SMOOTH_FORM", form)
    else:
        monkeypatch.delenv("VR_SMOOTH_FORM", raising=False)
    h = new_handle(em)
    mex.set_smoothing(h, sigma)
    got = slices_and_projections(h, shape)
    vr.volumeRender("delete", h)
    assert len(got) == sum(shape) + 4
    for k, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), f"{name} {form}: plane {k} differs"
    if name.startswith(("beyond", "fused")):  # (a thin rod such as long_x lies between the frame's rays)
        assert want[-2].max() > 0
    assert same_bits(em_s, em) == (name == "one_voxel")


def test_special_values_spread_as_the_rule_says():
    em = _noise((21, 9, 6), 4)
    em[3, 2, 1], em[15, 6, 4], em[9, 4, 2], em[10, 4, 2] = np.nan, np.inf, -0.0, 1e-40
    sigma = (0.5, 1, 0.5)
    em_s = smoothed(em, sigma)
    assert np.isnan(em_s).any() and np.isinf(em_s).any()
    h = new_handle(em)
    mex.set_smoothing(h, sigma)
    got = _slices_and_hist(h, em.shape, em_s)
    vr.volumeRender("delete", h)
    hr = new_handle(em_s)
    want = _slices_and_hist(hr, em.shape, em_s)
    vr.volumeRender("delete", hr)
    for g, w in zip(got[0], want[0]):
        assert same_bits(g, w)
    assert_histograms_equal(got[1], want[1], em_s, "special values")
    assert int(want[1][1]["nan"][0]) == int(np.isnan(em_s).sum()) > 1


def _slices_and_hist(h, shape, data):
    return all_axis_slices(h, shape), histogram_of(h, data)


# ---- 3. sigma changes ---------------------------------------------------------------------------------------

def test_a_second_sigma_derives_from_the_upload_and_clearing_restores_it(monkeypatch):
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    s1, s2 = F([2, 2, 2]), F([0.5, 0, 1])

    def state(h):
        o = {"frames": _frames(h, argv)}
        o["flags"], o["kernel"] = mex.last_launch_flags(), mex.last_march_kernel()
        return o

    def same_state(a, b):
        return _same_frames(a["frames"], b["frames"]) and a["flags"] == b["flags"] and a["kernel"] == b["kernel"]

    h = new_handle(em)
    plain = state(h)
    mex.set_smoothing(h, s1)
    first = state(h)
    mex.set_smoothing(h, s2)
    second = state(h)
    mex.set_smoothing(h, s2)  # (no change: nothing is written)
    again = state(h)
    mex.set_smoothing(h, None)
    assert not mex.get_smoothing(h).any()
    cleared = state(h)
    mex.set_smoothing(h, s1)
    mex.set_smoothing(h, np.zeros(3, F))
    cleared_by_zeros = state(h)
    with pytest.raises(vr.VrError, match="smoothing") as e:  # a refused sigma leaves the state
        mex.set_smoothing(h, F([1, 7, 1]))
    assert e.value.code == 1
    vr.volumeRender("delete", h)

    want = []
    for s in (s1, s2):
        hr = new_handle(smoothed(em, s))
        want.append(state(hr))
        vr.volumeRender("delete", hr)
    assert same_state(first, want[0]) and same_state(second, want[1]) and same_state(again, want[1])
    assert same_state(cleared, plain) and same_state(cleared_by_zeros, plain)
    assert not _same_frames(want[0]["frames"], want[1]["frames"]) and not _same_frames(want[1]["frames"], plain["frames"])
    # (smoothing the smoothed data would give neither)
    twice = smoothed(smoothed(em, s1), s2)
    assert not same_bits(twice, smoothed(em, s2))


# ---- 4. order and other state --------------------------------------------------------------------------------

def test_labels_gains_and_smoothing_in_both_orders():
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    labels = mask_labels(em.shape)
    em_sg = em2_of(smoothed(em, SIGMA), labels, GAINS)  # the gain multiplies the smoothed voxel
    seen = {}
    h = new_handle(em)
    plain = _frames(h, argv)
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, GAINS)
    mex.set_smoothing(h, SIGMA)
    seen["labels, gains, smoothing"] = _frames(h, argv)
    mex.set_label_gains(h, None)
    only_smoothing = _frames(h, argv)
    mex.set_label_gains(h, GAINS)
    seen["gains cleared and set again"] = _frames(h, argv)
    mex.set_smoothing(h, None)
    only_gains = _frames(h, argv)
    mex.set_label_gains(h, None)
    back = _frames(h, argv)
    vr.volumeRender("delete", h)

    h = vr.volumeRender("new")  # smoothing and gains before any volume, labels last
    mex.set_smoothing(h, SIGMA)
    mex.set_label_gains(h, GAINS)
    e = V(em, STAMP_EM)
    vr.volumeRender("sync_volumes", h, np.uint64(0), e, V(F(1.0), STAMP_RE), e)
    mex.sync_labels(h, labels)
    seen["smoothing, gains, em, labels"] = _frames(h, argv)
    vr.volumeRender("delete", h)

    def ref(data):
        hr = new_handle(data)
        out = _frames(hr, argv)
        vr.volumeRender("delete", hr)
        return out

    want = ref(em_sg)
    for k, v in seen.items():
        assert _same_frames(v, want), k
    assert _same_frames(only_smoothing, ref(smoothed(em, SIGMA)))
    assert _same_frames(only_gains, ref(em2_of(em, labels, GAINS)))
    assert _same_frames(back, plain) and not _same_frames(want, only_smoothing) and not _same_frames(want, only_gains)


@pytest.mark.parametrize("unorm", [False, True])
def test_a_uint8_upload_is_smoothed_after_its_conversion(unorm):
    p = product_scene("hg2_compute_32")
    argv = argv_of(p)
    raw = np.asfortranarray(np.clip(p["em"] * F(255), 0, 255).astype(np.uint8))
    fa = argv[2].copy()
    if not unorm:
        fa = (fa / F(255)).astype(F)  # (voxels up to 255: the same optical depth)
    argv = argv[:2] + [fa] + argv[3:]
    rv = vr.RawVolume(raw, unorm)
    rv.TimeLastUpdate = np.uint64(STAMP_EM)
    h = new_handle(rv)
    mex.set_smoothing(h, SIGMA)
    got = _frames(h, argv)
    vr.volumeRender("delete", h)
    hr = new_handle(smoothed(mex.convert_host(raw, unorm), SIGMA))
    want = _frames(hr, argv)
    vr.volumeRender("delete", hr)
    assert _same_frames(got, want) and want[0].max() > 0


def test_a_sync_of_changed_emission_is_smoothed_again():
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    em_b = np.asfortranarray(np.flip(em, 2) * F(0.75))
    sync = lambda h, e: vr.volumeRender("sync_volumes", h, np.uint64(0), e, V(F(1.0), STAMP_RE), e)  # noqa: E731
    h = new_handle(em)
    mex.set_smoothing(h, SIGMA)
    first = _frames(h, argv)
    ev = V(em, STAMP_EM)  # an unchanged emission (no upload) keeps the smoothed volume
    vr.volumeRender("sync_volumes", h, np.uint64(STAMP_EM + 100), ev, V(F(1.0), STAMP_RE), ev)
    kept = _frames(h, argv)
    sync(h, V(em_b, STAMP_EM + 1))
    changed = _frames(h, argv)
    sync(h, V(em_b[:, :, :-3].copy(order="F"), STAMP_EM + 2))  # other dims: another buffer
    smaller = _frames(h, argv)
    vr.volumeRender("delete", h)
    want = []
    for data in (em, em_b, em_b[:, :, :-3]):
        hr = new_handle(smoothed(data, SIGMA))
        want.append(_frames(hr, argv))
        vr.volumeRender("delete", hr)
    assert _same_frames(first, want[0]) and _same_frames(kept, want[0])
    assert _same_frames(changed, want[1]), "a changed emission lost the smoothing"
    assert _same_frames(smaller, want[2]) and not _same_frames(want[0], want[1])


def test_a_render_in_flight_keeps_the_volume_it_was_launched_on():
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    ra, keep = mex.render_args(*argv)
    H, W = (int(x) for x in np.asarray(argv[4]).reshape(-1))
    out = torch.full((2, 3, W, H), -7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    h = new_handle(em)
    torch.cuda.synchronize()
    mex.render_device(h, ra, out[0].data_ptr(), None, 0, stream.cuda_stream)
    mex.set_smoothing(h, SIGMA)
    mex.render_device(h, ra, out[1].data_ptr(), None, 0, stream.cuda_stream)
    torch.cuda.synchronize()
    got = [np.asfortranarray(out[i].cpu().numpy().transpose(2, 1, 0)) for i in range(2)]
    vr.volumeRender("delete", h)
    for data, img in zip((em, smoothed(em, SIGMA)), got):
        hr = new_handle(data)
        want = vr.volumeRender("render", hr, *argv)
        vr.volumeRender("delete", hr)
        assert same_bits(img, want)
    assert not same_bits(got[0], got[1])
    del keep


def test_a_separate_absorption_volume_is_not_smoothed_and_mem_info_names_the_smoothing(capfd):
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    re = V(F(1.0), STAMP_RE)
    ab = V(np.array(em, order="F"), STAMP_EM + 5)  # equal content, another Volume
    h = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", h, np.uint64(0), V(em, STAMP_EM), re, ab)
    _frames(h, argv)  # (a render first: the report then has its launch-time line on both sides)
    capfd.readouterr()
    vr.volumeRender("mem_info", h)
    before = capfd.readouterr().out
    mex.set_smoothing(h, SIGMA)
    got = _frames(h, argv)
    vr.volumeRender("mem_info", h)
    during = capfd.readouterr().out
    mex.set_smoothing(h, None)
    vr.volumeRender("mem_info", h)
    after = capfd.readouterr().out
    vr.volumeRender("delete", h)
    hr = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hr, np.uint64(0), V(smoothed(em, SIGMA), STAMP_EM), re, ab)
    want = _frames(hr, argv)
    vr.volumeRender("delete", hr)
    assert _same_frames(got, want)
    assert "smoothing" not in before and "smoothing" not in after and "smoothing sigma (voxels): 1 0.75 1.5" in during
    assert [ln.split(":")[0] for ln in before.splitlines()] == [ln.split(":")[0] for ln in after.splitlines()]


# ---- 5. refusals --------------------------------------------------------------------------------------------

def test_group_handles_and_slab_renders_are_refused(monkeypatch):
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    monkeypatch.setenv("VR_DEVICES", "0,0")  # device 0 twice, as tests/test_gpu_group.py
    g = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    with pytest.raises(vr.VrError, match="smoothing") as e:
        mex.set_smoothing(g, SIGMA)
    assert e.value.code == 5 and "group" in str(e.value)
    mex.set_smoothing(g, None)  # (clearing is not refused)
    assert not mex.get_smoothing(g).any()
    vr.volumeRender("delete", g)

    h = new_handle(em)
    ra, keep = mex.render_args(*argv)
    H, W = (int(x) for x in np.asarray(argv[4]).reshape(-1))
    state = torch.zeros(mex.SLAB_PLANES * W * H, dtype=torch.float32, device="cuda")
    d = em.shape[2]
    mex.render_slab(h, ra, mex.slab(d, 0, -np.inf, np.inf, 0), 0, state.data_ptr())  # (without smoothing: fine)
    torch.cuda.synchronize()
    mex.set_smoothing(h, SIGMA)
    with pytest.raises(vr.VrError, match="smoothing") as e:
        mex.render_slab(h, ra, mex.slab(d, 0, -np.inf, np.inf, 0), 0, state.data_ptr())
    assert e.value.code == 5 and "slab" in str(e.value)
    mex.set_smoothing(h, None)
    mex.render_slab(h, ra, mex.slab(d, 0, -np.inf, np.inf, 0), 0, state.data_ptr())
    torch.cuda.synchronize()
    vr.volumeRender("delete", h)
    del keep
    assert _lib.lib().vr_set_smoothing(None, SIGMA.ctypes.data) == 2  # (the arguments pass: the handle is looked at)
