"""GPU tests of the label volume with per-label gains (vr_sync_labels / vr_set_label_gains, the label
pass of csrc/vr_labels.hip).

The reference of every test is the product itself on the host-rewritten volume: em2 = (em *
table[labels]).astype(float32) formed in numpy (table padded with ones to 256) and synced the ordinary
way into a fresh handle.  The labelled handle's result must equal the em2 handle's bit for bit (NaN
positions equal, every other bit equal: test_gpu_transfer.same_bits) -- the em2 renders are tied to the C
oracle by the existing parity tests, so no tolerance appears here.

The texture bindings are module globals (as the reference's) and 'delete' resets the device state of
every handle, so each handle here lives alone: made, used for all its renders, deleted."""
import ctypes

import numpy as np
import pytest

import oracle as O
from golden_cases import STAMP_EM, STAMP_GRAD, STAMP_RE

vr = pytest.importorskip("volume_renderer_amd")
torch = pytest.importorskip("torch")
from volume_renderer_amd import _lib, mex  # noqa: E402
from test_gpu_clip import argv_of, gpu_render, product_scene  # noqa: E402
from test_gpu_isosurface import gpu_iso  # noqa: E402
from test_gpu_launch_flags import edge_of, renderer  # noqa: E402
from test_gpu_projection import (BLOCK_ARGS, RAGGED_ARGS, V, bits_equal, block_volume, gpu_project, new_handle,  # noqa: E402
                                 ragged_volume)
from test_gpu_transfer import TF_VALUE, gpu_transfer, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32
GAINS = F([1, 0.35, 0])
SCENES = ("hg2_compute_32", "hg1_lookup_24", "stereo_right_24")


def em2_of(em, labels, gains):
    table = np.ones(256, F)
    table[:len(gains)] = F(gains)
    with np.errstate(all="ignore"):
        return np.asfortranarray((em * table[labels]).astype(F))


def mask_labels(shape):
    """Label 1 on the half-space i1 >= d1 / 2 (example4's mask); label 2 on a box at the origin corner,
    which touches three faces, three edges and a corner of the volume (the apron is sampled); 0 elsewhere."""
    shape = tuple(shape) + (1,) * (3 - len(shape))
    lab = np.zeros(shape, np.uint8, order="F")
    lab[:, shape[1] // 2:, :] = 1
    lab[:shape[0] // 3 + 1, :shape[1] // 3 + 1, :shape[2] // 3 + 1] = 2
    return lab


def labelled_handle(p, labels, gains):
    h = new_handle(p["em"], p["re"], p["grads"])
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, gains)
    return h


def every_call(h, p, monkeypatch):
    """Every single-handle render call of the frame: name -> plane (or the launch's flags / kernel name)."""
    argv = argv_of(p)
    o = {"render": gpu_render(h, argv, count=False)[0]}
    o["flags"], o["kernel"] = mex.last_launch_flags(), mex.last_march_kernel()
    o["exact"] = gpu_render(h, argv, count=False, exact=True, monkeypatch=monkeypatch)[0]
    o["exact_flags"], o["exact_kernel"] = mex.last_launch_flags(), mex.last_march_kernel()
    o["stereo_left"], o["stereo_right"] = vr.volumeRender("render_stereo", h, *argv, F(0.1))
    for mode in ("mip", "sum"):
        o[mode], o[mode + "_aux"], _ = gpu_project(h, argv, mode)
    o["iso"], o["iso_depth"], o["iso_normal"], _ = gpu_iso(h, argv, 0.3)
    o["tf"], o["tf_alpha"], _ = gpu_transfer(h, argv, TF_VALUE)
    return o


def assert_outputs_equal(got, want, what):
    assert set(got) == set(want)
    for k in want:
        if isinstance(want[k], np.ndarray):
            assert same_bits(got[k], want[k]), f"{what}: {k} differs"
        else:
            assert got[k] == want[k], f"{what}: {k}: {got[k]} != {want[k]}"


def channel_volumes(em, p):
    e = V(em, STAMP_EM)
    vols = [e, V(F(1.0) if p["re"] is None else p["re"], STAMP_RE), e]
    return vols + ([V(g, STAMP_GRAD) for g in p["grads"]] if p["grads"] else [])


# ---- 1. every call ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", SCENES)
def test_every_render_call_equals_the_rewritten_volume(name, monkeypatch):
    p = product_scene(name)
    em = p["em"]
    labels = mask_labels(em.shape)
    assert {0, 1, 2} == set(np.unique(labels))
    em2 = em2_of(em, labels, GAINS)
    other = np.asfortranarray(np.flip(em, 0))  # the second channel's volume
    argv = argv_of(p)

    h = new_handle(em, p["re"], p["grads"])
    plain = gpu_render(h, argv, count=False)[0]
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, GAINS)
    got = every_call(h, p, monkeypatch)
    h2 = vr.volumeRender("new")
    chans = vr.volumeRender("render_channels", [(h, np.uint64(0), channel_volumes(em, p), argv),
                                                (h2, np.uint64(0), channel_volumes(other, p), argv)])
    vr.volumeRender("delete", h)
    vr.volumeRender("delete", h2)

    q = dict(p, em=em2)  # (the gradient volumes of lookup mode stay those of the unmodified data)
    hr = new_handle(em2, p["re"], p["grads"])
    want = every_call(hr, q, monkeypatch)
    h3 = vr.volumeRender("new")
    rchans = vr.volumeRender("render_channels", [(hr, np.uint64(0), channel_volumes(em2, p), argv),
                                                 (h3, np.uint64(0), channel_volumes(other, p), argv)])
    vr.volumeRender("delete", hr)
    vr.volumeRender("delete", h3)

    assert_outputs_equal(got, want, name)
    assert same_bits(chans[0], rchans[0]) and same_bits(chans[1], rchans[1]), f"{name}: render_channels differs"
    assert same_bits(chans[0], got["render"]) and not same_bits(chans[1], chans[0])
    assert not same_bits(got["render"], plain) and got["render"].max() > 0, f"{name}: the labels changed nothing"


# ---- 2. ragged shapes ---------------------------------------------------------------------------------------

def _long_rows():
    return np.asfortranarray(np.random.default_rng(3).random((300, 3, 2), dtype=F) - F(0.25))


RAGGED = {"ragged": ragged_volume, "flat": lambda: np.asfortranarray(np.random.default_rng(5).random((9, 7), dtype=F)),
          "one_voxel": lambda: np.full((1, 1), 2.5, F), "long_rows": _long_rows}


@pytest.mark.parametrize("name", sorted(RAGGED))
def test_ragged_shapes_project_as_the_rewritten_volume(name):
    em = RAGGED[name]()
    labels = np.asfortranarray(np.random.default_rng(11).integers(0, 5, em.shape).astype(np.uint8))
    if name == "ragged":  # the inf voxel meets a zero gain (NaN) and the NaN voxel a label outside the table
        labels[12, 2, 1], labels[3, 6, 3] = 2, 4
    if name == "one_voxel":
        labels[...] = 1
    gains = F([1, 0.35, 0, -2])
    em2 = em2_of(em, labels, gains)
    argv = [False, False] + RAGGED_ARGS
    if name == "long_rows":  # thick elements along the two short dims: a 300 x 150 x 150 box, not a rod between the rays
        argv[3] = F([75, 50, 1])
    h = new_handle(em)
    plain = gpu_project(h, argv, "sum")[0]
    mex.set_label_gains(h, gains)  # (gains first, labels second)
    mex.sync_labels(h, labels)
    got = [gpu_project(h, argv, mode)[:2] for mode in ("mip", "sum")]
    vr.volumeRender("delete", h)
    hr = new_handle(em2)
    want = [gpu_project(hr, argv, mode)[:2] for mode in ("mip", "sum")]
    vr.volumeRender("delete", hr)
    for g, w, mode in zip(got, want, ("mip", "sum")):
        assert same_bits(g[0], w[0]) and same_bits(g[1], w[1]), f"{name} {mode}"
    assert not same_bits(got[1][0], plain)


# ---- 3. statistics ------------------------------------------------------------------------------------------

def test_statistics_follow_the_modulated_values():
    """The small_x side of tests/test_gpu_launch_flags.py (V_shell(64), FactorAbsorption just below the
    edge at which Fa * maxabs * tstep crosses 2^-7); the largest voxel carries label 1, and a gain of 1.5
    lifts the product across: a stale maxabs would keep small_x and tame and skip the range test."""
    data = O.shell_volume(64)
    store = dict(lut64=vr.HenyeyGreenstein(64))
    at = np.unravel_index(np.argmax(np.abs(data)), data.shape)
    labels = np.zeros(data.shape, np.uint8, order="F")
    labels[at] = 1
    gains = F([1, 1.5])
    fa = 0.998 * edge_of(data)

    r = renderer(store, data)
    r.FactorAbsorption = fa
    plain = r.render()
    plain_flags = mex.last_launch_flags()
    assert plain_flags["small_x"] and plain_flags["tame"]
    r.VolumeLabels, r.LabelGains = labels, gains
    got = r.render()
    got_flags = mex.last_launch_flags()
    r.LabelGains = []
    back = r.render()
    back_flags = mex.last_launch_flags()
    r.delete()

    r2 = renderer(store, em2_of(data, labels, gains))
    r2.FactorAbsorption = fa
    want = r2.render()
    want_flags = mex.last_launch_flags()
    r2.delete()

    assert not want_flags["small_x"] and not want_flags["tame"]
    assert got_flags == want_flags and same_bits(got, want)
    assert back_flags == plain_flags and same_bits(back, plain)
    assert not same_bits(got, plain)


# ---- 4. occupancy -------------------------------------------------------------------------------------------

def render_counted(h, argv):
    """The counter variant of 'render': (image, the 48 counters)."""
    ra, keep = mex.render_args(*argv)
    H, W = (int(x) for x in np.asarray(argv[4]).reshape(-1))
    out = torch.full((3, W, H), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.zeros(48, dtype=torch.int64, device="cuda")
    mex.render_device(h, ra, out.data_ptr(), None, steps.data_ptr())
    torch.cuda.synchronize()
    del keep
    return np.asfortranarray(out.cpu().numpy().transpose(2, 1, 0)), steps.cpu().numpy()


def test_occupancy_map_follows_the_gains():
    em = block_volume(False)
    labels = np.zeros(em.shape, np.uint8, order="F")
    labels[34:46, 14:26, 25:37] = 1  # the whole block
    argv = [False, False] + BLOCK_ARGS

    def both(h):
        return render_counted(h, argv), gpu_project(h, argv, "mip", count=True)

    h = new_handle(em)
    plain = both(h)
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, F([1, 0]))
    faded = both(h)
    mex.set_label_gains(h, F([1, 1]))
    back = both(h)
    vr.volumeRender("delete", h)
    hz = new_handle(em2_of(em, labels, F([1, 0])))
    zero = both(hz)
    vr.volumeRender("delete", hz)

    def same(a, b):
        (ri, rs), (pi, pa, pc) = a
        (ri2, rs2), (pi2, pa2, pc2) = b
        return (same_bits(ri, ri2) and np.array_equal(rs[:8], rs2[:8]) and same_bits(pi, pi2) and same_bits(pa, pa2)
                and pc == pc2)

    assert same(faded, zero), "gain 0: image or leap counters differ from the all-zero volume's"
    assert same(back, plain), "gain back to 1: a stale map loses the block"
    assert not same_bits(faded[0][0], plain[0][0]) and not np.array_equal(faded[0][1][:8], plain[0][1][:8])
    assert faded[1][2] != plain[1][2] and plain[1][2][1] < plain[1][2][0]  # (the unlabelled MIP leaps, but less)
    assert plain[0][0].max() > 0 and faded[0][0].max() == 0


# ---- 5. state -----------------------------------------------------------------------------------------------

def test_gain_table_round_trip_and_refusals():
    h = vr.volumeRender("new")
    assert mex.get_label_gains(h).shape == (0,)
    for g in (GAINS, F([-2]), np.linspace(-1, 1, 256).astype(F)):
        mex.set_label_gains(h, g)
        got = mex.get_label_gains(h)
        assert got.dtype == np.float32 and bits_equal(got, g)
    with pytest.raises(vr.VrError, match="label gains"):  # a refused set leaves the old table
        mex.set_label_gains(h, F([1, np.inf]))
    with pytest.raises(vr.VrError, match="label gains"):
        mex.set_label_gains(h, np.ones(257, F))
    assert mex.get_label_gains(h).shape == (256,)
    other = vr.volumeRender("new")  # state of the handle, not of the module
    assert mex.get_label_gains(other).shape == (0,)
    mex.set_label_gains(h, None)
    assert mex.get_label_gains(h).shape == (0,)
    mex.set_label_gains(h, GAINS)
    vr.volumeRender("delete", h)
    with pytest.raises(vr.VrError, match="Handle not valid"):
        mex.get_label_gains(h)
    assert mex.get_label_gains(other).shape == (0,)
    vr.volumeRender("delete", other)


def _frames(h, argv):
    return [vr.volumeRender("render", h, *argv)] + list(gpu_project(h, argv, "sum")[:2])


def _same_frames(a, b):
    return all(same_bits(x, y) for x, y in zip(a, b))


def test_state_orders_resyncs_and_refusals(monkeypatch):
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    labels = mask_labels(em.shape)
    em_b = np.asfortranarray(np.flip(em, 2) * F(0.75))  # a changed emission volume
    sync = lambda h, e: vr.volumeRender("sync_volumes", h, np.uint64(0), e, V(F(1.0), STAMP_RE), e)  # noqa: E731

    seen = {}
    # the three arrivals, each last once: one image
    h = new_handle(em)
    plain = _frames(h, argv)
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, GAINS)
    seen["em, labels, gains"] = _frames(h, argv)
    # labels of other dims: refused with the message, the old labels and the render stay
    with pytest.raises(vr.VrError, match="labels") as e:
        mex.sync_labels(h, np.zeros((em.shape[0], em.shape[1], em.shape[2] + 1), np.uint8))
    assert e.value.code == 1
    seen["after a refused sync_labels"] = _frames(h, argv)
    # an unchanged emission (no upload: TimeLastMemSync is past its stamp) keeps the modulation
    ev = V(em, STAMP_EM)
    vr.volumeRender("sync_volumes", h, np.uint64(STAMP_EM + 100), ev, V(F(1.0), STAMP_RE), ev)
    seen["unchanged emission re-synced"] = _frames(h, argv)
    # the same emission uploaded again (TimeLastMemSync 0) is modulated again
    sync(h, ev)
    seen["emission uploaded again"] = _frames(h, argv)
    # a changed emission keeps the modulation: checked against its own em2 below
    sync(h, V(em_b, STAMP_EM + 1))
    changed = _frames(h, argv)
    sync(h, ev)
    # sync_labels(None) restores the unmodified bits; the labels coming back, the modulated ones
    mex.sync_labels(h, None)
    dropped = _frames(h, argv)
    mex.sync_labels(h, labels)
    seen["labels dropped and synced again"] = _frames(h, argv)
    mex.set_label_gains(h, None)
    cleared = _frames(h, argv)
    vr.volumeRender("delete", h)

    h = vr.volumeRender("new")  # gains, labels, emission
    mex.set_label_gains(h, GAINS)
    mex.sync_labels(h, labels)
    sync(h, V(em, STAMP_EM))
    seen["gains, labels, em"] = _frames(h, argv)
    vr.volumeRender("delete", h)

    h = vr.volumeRender("new")  # labels, emission, gains -- and mismatching labels noticed by each call
    bad = np.zeros((em.shape[0] + 1, em.shape[1], em.shape[2]), np.uint8)
    mex.sync_labels(h, bad)  # (no emission, no gains: nothing to compare with)
    sync(h, V(em, STAMP_EM))  # (no gains yet)
    with pytest.raises(vr.VrError, match="labels") as e:
        mex.set_label_gains(h, GAINS)
    assert e.value.code == 1 and mex.get_label_gains(h).shape == (0,)
    assert _same_frames(_frames(h, argv), plain), "a refused set_label_gains modulated the volume"
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, GAINS)
    seen["labels, em, gains"] = _frames(h, argv)
    with pytest.raises(vr.VrError, match="labels") as e:  # sync_volumes notices: the new volume is resident, unmodified
        sync(h, V(em_b[:, :, :-1].copy(order="F"), STAMP_EM + 2))
    assert e.value.code == 1
    unmod_small = _frames(h, argv)
    vr.volumeRender("delete", h)

    hr = new_handle(em2_of(em, labels, GAINS))
    want = _frames(hr, argv)
    vr.volumeRender("delete", hr)
    hr = new_handle(em2_of(em_b, labels, GAINS))
    want_changed = _frames(hr, argv)
    vr.volumeRender("delete", hr)
    hr = new_handle(np.asfortranarray(em_b[:, :, :-1]))
    want_small = _frames(hr, argv)
    vr.volumeRender("delete", hr)

    for k, v in seen.items():
        assert _same_frames(v, want), k
    assert _same_frames(changed, want_changed), "a changed emission lost the modulation"
    assert _same_frames(dropped, plain) and _same_frames(cleared, plain)
    assert _same_frames(unmod_small, want_small)
    assert not _same_frames(want, plain) and not _same_frames(want_changed, want)


# ---- 6. aliasing --------------------------------------------------------------------------------------------

def test_a_separate_absorption_volume_is_not_modulated():
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    labels = mask_labels(em.shape)
    re = V(F(1.0), STAMP_RE)
    ab = V(np.array(em, order="F"), STAMP_EM + 5)  # equal content, another Volume
    h = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", h, np.uint64(0), V(em, STAMP_EM), re, ab)
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, GAINS)
    got = _frames(h, argv)
    mex.set_label_gains(h, None)
    plain = _frames(h, argv)
    vr.volumeRender("delete", h)
    # (the absorption slot index keeps the reference's default, the emission texture, SURVEY.md s0.1: the
    # separately uploaded absorption buffer is resident, is not rewritten, and is sampled by neither handle)
    hr = vr.volumeRender("new")
    e2 = V(em2_of(em, labels, GAINS), STAMP_EM)
    vr.volumeRender("sync_volumes", hr, np.uint64(0), e2, re, ab)
    want = _frames(hr, argv)
    vr.volumeRender("delete", hr)
    assert _same_frames(got, want) and not _same_frames(got, plain)


# ---- 7. typed and device sources -----------------------------------------------------------------------------

@pytest.mark.parametrize("unorm", [False, True])
def test_typed_emission_is_modulated_after_its_conversion(unorm):
    p = product_scene("hg2_compute_32")
    argv = argv_of(p)
    raw = np.asfortranarray(np.clip(p["em"] * F(255), 0, 255).astype(np.uint8))
    labels = mask_labels(raw.shape)
    fa = argv[2].copy()
    if not unorm:
        fa = (fa / F(255)).astype(F)  # (voxels up to 255: the same optical depth)
    argv = argv[:2] + [fa] + argv[3:]
    rv = vr.RawVolume(raw, unorm)
    rv.TimeLastUpdate = np.uint64(STAMP_EM)
    h = new_handle(rv)
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, GAINS)
    got = _frames(h, argv)
    vr.volumeRender("delete", h)
    # labels given as a device-resident uint8 tensor: the same
    t = torch.from_numpy(np.ascontiguousarray(labels.reshape(-1, order="F"))).cuda()
    h = new_handle(rv)
    mex.set_label_gains(h, GAINS)
    mex.sync_labels(h, mex.DeviceVolume.from_tensor(t, dims=labels.shape, last_update=77))
    got_dev = _frames(h, argv)
    vr.volumeRender("delete", h)
    hr = new_handle(em2_of(mex.convert_host(raw, unorm), labels, GAINS))
    want = _frames(hr, argv)
    vr.volumeRender("delete", hr)
    assert _same_frames(got, want) and _same_frames(got_dev, want) and want[0].max() > 0


# ---- 8. in flight -------------------------------------------------------------------------------------------

def test_a_render_in_flight_keeps_the_gains_it_was_launched_with():
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    labels = mask_labels(em.shape)
    g1, g2 = GAINS, F([0.5, 2, 1])
    ra, keep = mex.render_args(*argv)
    H, W = (int(x) for x in np.asarray(argv[4]).reshape(-1))
    out = torch.full((2, 3, W, H), -7.0, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    h = new_handle(em)
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, g1)
    torch.cuda.synchronize()
    mex.render_device(h, ra, out[0].data_ptr(), None, 0, stream.cuda_stream)
    mex.set_label_gains(h, g2)
    mex.render_device(h, ra, out[1].data_ptr(), None, 0, stream.cuda_stream)
    torch.cuda.synchronize()
    got = [np.asfortranarray(out[i].cpu().numpy().transpose(2, 1, 0)) for i in range(2)]
    vr.volumeRender("delete", h)
    for g, img in zip((g1, g2), got):
        hr = new_handle(em2_of(em, labels, g))
        want = vr.volumeRender("render", hr, *argv)
        vr.volumeRender("delete", hr)
        assert same_bits(img, want)
    assert not same_bits(got[0], got[1])
    del keep


# ---- 9. group handle ----------------------------------------------------------------------------------------

def test_group_handle_refuses_and_other_handles_keep_their_labels(monkeypatch):
    p = product_scene("hg2_compute_32")
    em, argv = p["em"], argv_of(p)
    labels = mask_labels(em.shape)
    h = labelled_handle(p, labels, GAINS)
    monkeypatch.setenv("VR_DEVICES", "0,0")  # device 0 twice, as tests/test_gpu_group.py
    g = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    for call in (lambda: mex.sync_labels(g, labels), lambda: mex.sync_labels(g, None),
                 lambda: mex.set_label_gains(g, GAINS)):
        with pytest.raises(vr.VrError, match="labels") as e:
            call()
        assert e.value.code == 5
    mex.set_label_gains(g, None)  # nothing else refuses
    assert mex.get_label_gains(g).shape == (0,)
    vr.volumeRender("delete", g)  # ('delete' resets every handle's device volumes; the label state stays)
    assert bits_equal(mex.get_label_gains(h), GAINS)
    e = V(em, STAMP_EM)
    vr.volumeRender("sync_volumes", h, np.uint64(0), e, V(F(1.0), STAMP_RE), e)
    got = vr.volumeRender("render", h, *argv)
    vr.volumeRender("delete", h)
    hr = new_handle(em2_of(em, labels, GAINS))
    want = vr.volumeRender("render", hr, *argv)
    vr.volumeRender("delete", hr)
    assert same_bits(got, want)
    L = _lib.lib()
    assert L.vr_sync_labels(ctypes.c_void_p(int(h)), None) == 2  # (the deleted handle is gone)
