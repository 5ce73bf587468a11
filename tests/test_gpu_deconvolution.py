"""GPU tests of the Richardson-Lucy deconvolution of the resident emission volume (vr_set_deconvolution: the
filter passes of csrc/vr_smooth.hip with their ratio and update epilogues, csrc/vr_deconv.hip).

The reference of every test is the product itself on the host-deconvolved volume: em_d =
vr_deconvolve_host(em, ...) -- tied to the numpy restatement of the rule by tests/test_deconv_host.py --
synced the ordinary way into a fresh handle.  The deconvolved handle's result must equal the em_d handle's
bit for bit (NaN positions equal, every other bit equal); nothing is compared under a tolerance except the
histogram's double sum, which has the bound of tests/test_gpu_histogram.py.  This is the pattern of
tests/test_gpu_smoothing.py, whose helpers are used.

Each handle lives alone (the texture bindings are module globals): made, used, deleted."""
import itertools

import numpy as np
import pytest

from golden_cases import STAMP_EM, STAMP_RE

vr = pytest.importorskip("volume_renderer_amd")
torch = pytest.importorskip("torch")
from volume_renderer_amd import _lib, mex  # noqa: E402
from test_gpu_clip import argv_of, product_scene  # noqa: E402
from test_gpu_labels import (GAINS, SCENES, _frames, _same_frames, assert_outputs_equal, channel_volumes, em2_of,  # noqa: E402
                             every_call, mask_labels)
from test_gpu_projection import V, new_handle  # noqa: E402
from test_gpu_smoothing import (SEG, TA, TX, all_axis_slices, assert_histograms_equal, histogram_of,  # noqa: E402
                                slices_and_projections, smoothed)
from test_gpu_transfer import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
SIGMA = F([1.0, 0.75, 1.5])
FLOOR = F(1e-6)


def deconvolved(em, sigma=SIGMA, n=2, floor=FLOOR):
    return np.asfortranarray(mex.deconvolve_host(np.asarray(em, F), sigma, n, floor))


# ---- 1. every call ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_every_call_equals_the_host_deconvolved_volume(name, monkeypatch):
    p = product_scene(name)
    em = p["em"]
    em_d = deconvolved(em)
    other = np.asfortranarray(np.flip(em, 0))  # the second channel's volume
    argv = argv_of(p)

    h = new_handle(em, p["re"], p["grads"])
    plain = vr.volumeRender("render", h, *argv)
    mex.set_deconvolution(h, SIGMA, 2)
    sg, n, fl = mex.get_deconvolution(h)
    assert same_bits(sg, SIGMA) and n == 2 and fl == FLOOR
    got = every_call(h, p, monkeypatch)
    got_hist = histogram_of(h, em_d)
    h2 = vr.volumeRender("new")
    chans = vr.volumeRender("render_channels", [(h, np.uint64(0), channel_volumes(em, p), argv),
                                                (h2, np.uint64(0), channel_volumes(other, p), argv)])
    vr.volumeRender("delete", h)
    vr.volumeRender("delete", h2)

    q = dict(p, em=em_d)  # (the gradient volumes of lookup mode stay those of the unmodified data)
    hr = new_handle(em_d, p["re"], p["grads"])
    want = every_call(hr, q, monkeypatch)
    want_hist = histogram_of(hr, em_d)
    h3 = vr.volumeRender("new")
    rchans = vr.volumeRender("render_channels", [(hr, np.uint64(0), channel_volumes(em_d, p), argv),
                                                 (h3, np.uint64(0), channel_volumes(other, p), argv)])
    vr.volumeRender("delete", hr)
    vr.volumeRender("delete", h3)

    assert_outputs_equal(got, want, name)
    assert_histograms_equal(got_hist, want_hist, em_d, name)
    assert same_bits(chans[0], rchans[0]) and same_bits(chans[1], rchans[1]), f"{name}: render_channels differs"
    assert same_bits(chans[0], got["render"]) and not same_bits(chans[1], chans[0])
    assert not same_bits(got["render"], plain) and got["render"].max() > 0, f"{name}: the deconvolution changed nothing"


# ---- 2. resident voxels by position -------------------------------------------------------------------------

def _noise(shape, seed):
    return np.asfortranarray(np.random.default_rng(seed).random(shape, dtype=F) - F(0.25))


# beyond every tile of the passes (SEG along dims[0], TA along the filtered axis, TX lanes: 259 + 2 padded
# columns are five chunks of 64); ragged; every dim below the radius; one and two active axes; no axis along
# dims[0]; and a volume whose only sigma lies on an axis of one voxel (B the identity: the elementwise launches)
POSITION_CASES = {
    "beyond_the_tiles": ((SEG + 3, TA + 3, TA + 2), SIGMA), "ragged": ((TX + 3, 3, TA + 1), SIGMA),
    "below_the_radius": ((5, 4, 3), (6, 6, 6)), "one_axis_x": ((40, 1, 1), SIGMA), "one_axis_y": ((1, 37, 1), SIGMA),
    "two_axes": ((20, 18, 1), (1, 1, 1)), "z_only": ((9, 8, 7), (0, 0, 2)), "no_axis": ((6, 1, 5), (0, 2, 0)),
}
assert POSITION_CASES["beyond_the_tiles"][0] == (259, 35, 34) and POSITION_CASES["ragged"][0] == (67, 3, 33)

_position_input = {}


def position_reference(name, n):
    shape, sigma = POSITION_CASES[name]
    if name not in _position_input:
        _position_input[name] = _noise(shape, len(name))
    em = _position_input[name]
    em_d = deconvolved(em, sigma, n)
    hr = new_handle(em_d)
    want = slices_and_projections(hr, shape)
    vr.volumeRender("delete", hr)
    return em, em_d, want


@pytest.mark.parametrize("n", [1, 2, 3])  # odd and even counts: both ends of the buffer rotation
@pytest.mark.parametrize("name", sorted(POSITION_CASES))
def test_resident_voxels_equal_the_host_deconvolved_volume_by_position(name, n):
    shape, sigma = POSITION_CASES[name]
    em, em_d, want = position_reference(name, n)
    h = new_handle(em)
    mex.set_deconvolution(h, sigma, n)
    got = slices_and_projections(h, shape)
    vr.volumeRender("delete", h)
    assert len(got) == sum(shape) + 4
    for k, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), f"{name} n={n}: plane {k} differs"
    if name == "beyond_the_tiles":
        assert want[-2].max() > 0
    assert not same_bits(em_d, em)


def test_64_iterations():
    shape = (12, 10, 8)
    em = _noise(shape, 3)
    em_d = deconvolved(em, SIGMA, 64)
    assert np.isfinite(em_d).all() and em_d.max() > 0
    h = new_handle(em)
    mex.set_deconvolution(h, SIGMA, _lib.VR_DECONV_MAX_ITERATIONS)
    got = all_axis_slices(h, shape)
    vr.volumeRender("delete", h)
    hr = new_handle(em_d)
    want = all_axis_slices(hr, shape)
    vr.volumeRender("delete", hr)
    for k, (g, w) in enumerate(zip(got, want)):
        assert same_bits(g, w), f"plane {k} differs"


def test_special_values_spread_as_the_rule_says():
    em = _noise((21, 9, 6), 4)
    em[3, 2, 1], em[15, 6, 4], em[9, 4, 2], em[10, 4, 2], em[18, 1, 5] = np.nan, np.inf, -0.0, 1e-40, -np.inf
    em[0:6, 5:9, 0:3] = 0  # exact zeros: the blurred estimate lies under the floor inside
    em[6:9, 5:9, 0:3] = 1e-9
    sigma = (0.5, 1, 0.5)
    for n in (1, 2):
        em_d = deconvolved(em, sigma, n)
        assert np.isnan(em_d).any() and np.isfinite(em_d).any()
        h = new_handle(em)
        mex.set_deconvolution(h, sigma, n)
        got = all_axis_slices(h, em.shape), histogram_of(h, em_d)
        vr.volumeRender("delete", h)
        hr = new_handle(em_d)
        want = all_axis_slices(hr, em.shape), histogram_of(hr, em_d)
        vr.volumeRender("delete", hr)
        for g, w in zip(got[0], want[0]):
            assert same_bits(g, w)
        assert_histograms_equal(got[1], want[1], em_d, f"special values n={n}")
        assert int(want[1][1]["nan"][0]) == int(np.isnan(em_d).sum()) > 1


# ---- 3. setting changes -------------------------------------------------------------------------------------

def test_a_second_setting_derives_from_the_upload_and_clearing_restores_it():
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    a, b = (F([2, 2, 2]), 3, FLOOR), (F([0.5, 0, 1]), 2, F(1e-3))

    def state(h):
        o = {"frames": _frames(h, argv)}
        o["flags"], o["kernel"] = mex.last_launch_flags(), mex.last_march_kernel()
        return o

    def same_state(x, y):
        return _same_frames(x["frames"], y["frames"]) and x["flags"] == y["flags"] and x["kernel"] == y["kernel"]

    h = new_handle(em)
    plain = state(h)
    mex.set_deconvolution(h, *a)
    first = state(h)
    mex.set_deconvolution(h, *b)
    second = state(h)
    cleared = []
    for clear in ((None, 0), (b[0], 0), (np.zeros(3, F), 4), (False, 2)):
        mex.set_deconvolution(h, *clear)
        sg, n, fl = mex.get_deconvolution(h)
        assert not sg.any() and n == 0 and fl == 0
        cleared.append(state(h))
        mex.set_deconvolution(h, *a)
    for bad in ((F([1, 7, 1]), 2, FLOOR), (a[0], 65, FLOOR), (a[0], 2, F(0))):  # a refused setting leaves the state
        with pytest.raises(vr.VrError, match="deconvolution") as e:
            mex.set_deconvolution(h, *bad)
        assert e.value.code == 1
    kept = state(h)
    vr.volumeRender("delete", h)

    want = []
    for s in (a, b):
        hr = new_handle(deconvolved(em, *s))
        want.append(state(hr))
        vr.volumeRender("delete", hr)
    assert same_state(first, want[0]) and same_state(second, want[1]) and same_state(kept, want[0])
    assert all(same_state(c, plain) for c in cleared)
    assert not _same_frames(want[0]["frames"], want[1]["frames"]) and not _same_frames(want[1]["frames"], plain["frames"])


def test_the_current_setting_again_launches_nothing():
    """Every upload and every derivation takes a new upload version (launch schedules are keyed on it)."""
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    h = new_handle(em)
    mex.set_deconvolution(h, SIGMA, 2)
    first = _frames(h, argv)
    v0, t0 = mex.emission_version(h), mex.derive_times(h)
    L = _lib.lib()
    for _ in range(3):
        mex.set_deconvolution(h, SIGMA, 2, FLOOR)
    assert mex.emission_version(h) == v0 != 0 and mex.derive_times(h) == t0, "a derivation ran"
    assert _same_frames(_frames(h, argv), first)
    mex.set_smoothing(h, None)  # (nor do the other setters derive again when their own state is unchanged)
    mex.set_label_gains(h, None)
    assert mex.emission_version(h) == v0
    mex.set_deconvolution(h, SIGMA, 2, F(1e-5))  # (a change of the floor alone is a change)
    assert mex.emission_version(h) > v0
    assert L.vr_set_deconvolution(None, SIGMA.ctypes.data, 2, FLOOR) == 2
    vr.volumeRender("delete", h)


# ---- 4. order and other state --------------------------------------------------------------------------------

def test_smoothing_labels_and_gains_in_every_arrival_order():
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    labels = mask_labels(em.shape)
    s2 = F([0.75, 1, 0.5])
    em_all = em2_of(smoothed(deconvolved(em), s2), labels, GAINS)  # gain(smooth(deconv(y)))
    steps = {"deconvolution": lambda h: mex.set_deconvolution(h, SIGMA, 2), "smoothing": lambda h: mex.set_smoothing(h, s2),
             "labels": lambda h: mex.sync_labels(h, labels), "gains": lambda h: mex.set_label_gains(h, GAINS)}

    def ref(data):
        hr = new_handle(data)
        out = _frames(hr, argv)
        vr.volumeRender("delete", hr)
        return out

    want = ref(em_all)
    for order in itertools.permutations(steps):
        h = new_handle(em)
        for k in order:
            steps[k](h)
        got = _frames(h, argv)
        vr.volumeRender("delete", h)
        assert _same_frames(got, want), order

    h = vr.volumeRender("new")  # everything before any volume
    for k in ("gains", "deconvolution", "smoothing"):
        steps[k](h)
    e = V(em, STAMP_EM)
    vr.volumeRender("sync_volumes", h, np.uint64(0), e, V(F(1.0), STAMP_RE), e)
    steps["labels"](h)
    early = _frames(h, argv)
    mex.set_label_gains(h, None)  # one and two passes after the iterations: the estimate changes its buffer
    no_gains = _frames(h, argv)
    mex.set_smoothing(h, None)
    only_deconvolution = _frames(h, argv)
    mex.set_smoothing(h, s2)
    mex.set_deconvolution(h, None)
    only_smoothing = _frames(h, argv)
    vr.volumeRender("delete", h)
    assert _same_frames(early, want)
    assert _same_frames(no_gains, ref(smoothed(deconvolved(em), s2)))
    assert _same_frames(only_deconvolution, ref(deconvolved(em)))
    assert _same_frames(only_smoothing, ref(smoothed(em, s2)))
    assert not _same_frames(want, no_gains) and not _same_frames(no_gains, only_deconvolution)
    assert not _same_frames(ref(deconvolved(smoothed(em, s2))), no_gains)  # (the other order is another volume)


@pytest.mark.parametrize("unorm", [False, True])
def test_a_uint8_upload_is_deconvolved_after_its_conversion(unorm):
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
    mex.set_deconvolution(h, SIGMA, 2)
    got = _frames(h, argv)
    vr.volumeRender("delete", h)
    hr = new_handle(deconvolved(mex.convert_host(raw, unorm)))
    want = _frames(hr, argv)
    vr.volumeRender("delete", hr)
    assert _same_frames(got, want) and want[0].max() > 0


def test_a_sync_of_changed_emission_is_deconvolved_again():
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    em_b = np.asfortranarray(np.flip(em, 2) * F(0.75))
    sync = lambda h, e: vr.volumeRender("sync_volumes", h, np.uint64(0), e, V(F(1.0), STAMP_RE), e)  # noqa: E731
    h = new_handle(em)
    mex.set_deconvolution(h, SIGMA, 2)
    first = _frames(h, argv)
    ev = V(em, STAMP_EM)  # an unchanged emission (no upload) keeps the deconvolved volume
    vr.volumeRender("sync_volumes", h, np.uint64(STAMP_EM + 100), ev, V(F(1.0), STAMP_RE), ev)
    kept = _frames(h, argv)
    sync(h, V(em_b, STAMP_EM + 1))
    changed = _frames(h, argv)
    sync(h, V(em_b[:, :, :-3].copy(order="F"), STAMP_EM + 2))  # other dims: another buffer
    smaller = _frames(h, argv)
    vr.volumeRender("delete", h)
    want = []
    for data in (em, em_b, em_b[:, :, :-3]):
        hr = new_handle(deconvolved(data))
        want.append(_frames(hr, argv))
        vr.volumeRender("delete", hr)
    assert _same_frames(first, want[0]) and _same_frames(kept, want[0])
    assert _same_frames(changed, want[1]), "a changed emission lost the deconvolution"
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
    mex.set_deconvolution(h, SIGMA, 2)
    mex.render_device(h, ra, out[1].data_ptr(), None, 0, stream.cuda_stream)
    torch.cuda.synchronize()
    got = [np.asfortranarray(out[i].cpu().numpy().transpose(2, 1, 0)) for i in range(2)]
    vr.volumeRender("delete", h)
    for data, img in zip((em, deconvolved(em)), got):
        hr = new_handle(data)
        want = vr.volumeRender("render", hr, *argv)
        vr.volumeRender("delete", hr)
        assert same_bits(img, want)
    assert not same_bits(got[0], got[1])
    del keep


def test_a_separate_absorption_volume_is_untouched_and_mem_info_names_the_deconvolution(capfd):
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
    mex.set_deconvolution(h, SIGMA, 2)
    got = _frames(h, argv)
    vr.volumeRender("mem_info", h)
    during = capfd.readouterr().out
    mex.set_deconvolution(h, None)
    vr.volumeRender("mem_info", h)
    after = capfd.readouterr().out
    vr.volumeRender("delete", h)
    hr = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", hr, np.uint64(0), V(deconvolved(em), STAMP_EM), re, ab)
    want = _frames(hr, argv)
    vr.volumeRender("delete", hr)
    assert _same_frames(got, want)
    assert "deconvolution" not in before and "deconvolution" not in after
    assert "deconvolution sigma (voxels): 1 0.75 1.5, iterations: 2, floor: 1e-06" in during
    assert [ln.split(":")[0] for ln in before.splitlines()] == [ln.split(":")[0] for ln in after.splitlines()]


# ---- 5. refusals --------------------------------------------------------------------------------------------

def test_group_handles_and_slab_renders_are_refused(monkeypatch):
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    monkeypatch.setenv("VR_DEVICES", "0,0")  # device 0 twice, as tests/test_gpu_group.py
    g = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    with pytest.raises(vr.VrError, match="deconvolution") as e:
        mex.set_deconvolution(g, SIGMA, 2)
    assert e.value.code == 5 and "group" in str(e.value)
    mex.set_deconvolution(g, None)  # (clearing is not refused)
    mex.set_deconvolution(g, SIGMA, 0)
    assert mex.get_deconvolution(g)[1] == 0
    vr.volumeRender("delete", g)

    h = new_handle(em)
    ra, keep = mex.render_args(*argv)
    H, W = (int(x) for x in np.asarray(argv[4]).reshape(-1))
    state = torch.zeros(mex.SLAB_PLANES * W * H, dtype=torch.float32, device="cuda")
    d = em.shape[2]
    mex.render_slab(h, ra, mex.slab(d, 0, -np.inf, np.inf, 0), 0, state.data_ptr())  # (without: fine)
    torch.cuda.synchronize()
    mex.set_deconvolution(h, SIGMA, 2)
    with pytest.raises(vr.VrError, match="deconvolution") as e:
        mex.render_slab(h, ra, mex.slab(d, 0, -np.inf, np.inf, 0), 0, state.data_ptr())
    assert e.value.code == 5 and "slab" in str(e.value)
    mex.set_deconvolution(h, None)
    mex.render_slab(h, ra, mex.slab(d, 0, -np.inf, np.inf, 0), 0, state.data_ptr())
    torch.cuda.synchronize()
    vr.volumeRender("delete", h)
    del keep
