"""GPU tests of the volume histogram (vr_volume_histogram / vr_volume_histogram_device, vr_histogram.hip)
against the numpy restatement of tests/histogram_ref.py.  Counts, counters and extrema are integer or
order-independent and are expected exactly -- the extrema bit for bit, -0 and +0 told apart -- on both
sides of VR_HIST_UNIFORM; only `sum` has a bound (see assert_equal)."""
import ctypes

import numpy as np
import pytest

import histogram_ref as HR
import projection_ref as PR
import slice_ref as SR

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
STAMP_EM, STAMP_RE, STAMP_AB = 31, 32, 33
SOURCES = ("emission", "absorption", "reflection")
NBINS = (1, 7, 256, 4096)


def V(data, t):
    v = vr.Volume(data)
    v.TimeLastUpdate = np.uint64(t)
    return v


def fresh_handle():
    """A new handle on reset module-global bindings and slot indices ('delete' resets them)."""
    vr.volumeRender("delete", vr.volumeRender("new"))
    return vr.volumeRender("new")


def new_handle(em):
    h = fresh_handle()
    e = em if isinstance(em, (vr.Volume, vr.RawVolume)) else V(em, STAMP_EM)
    vr.volumeRender("sync_volumes", h, np.uint64(0), e, V(F(1.0), STAMP_RE), e)
    return h


def query(nbins, lim, source="emission", labels=(0, 0), clip=False):
    return mex.make_histogram(source, nbins, F(lim), np.int32(labels), clip)


def gpu_hist(h, q):
    """The host entry: (counts [rows, nbins] uint64, rows as a record array)."""
    return mex.volume_histogram(h, q)


def gpu_hist_device(h, q, stream=0, rows=True):
    """vr_volume_histogram_device into torch buffers prefilled with garbage."""
    import torch
    n = mex.histogram_rows(q)
    d_counts = torch.full((n, q.nbins), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    d_rows = torch.full((n * 56,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # (the fills run on torch's stream, the histogram maybe on another)
    mex.volume_histogram_device(h, q, d_counts.data_ptr(), d_rows.data_ptr() if rows else 0, stream)
    torch.cuda.synchronize()
    counts = d_counts.cpu().numpy().view(np.uint64)
    summ = d_rows.cpu().numpy().view(mex.HIST_ROW_DTYPE) if rows else None
    return counts, summ


def both_paths(monkeypatch, fn):
    """fn() with the kernel's wave-uniform shortcut forced on (VR_HIST_UNIFORM=1) and off (=0)."""
    monkeypatch.setenv("VR_HIST_UNIFORM", "1")
    a = fn()
    monkeypatch.setenv("VR_HIST_UNIFORM", "0")
    b = fn()
    monkeypatch.delenv("VR_HIST_UNIFORM")
    return a, b


def assert_equal(got, want, what, exact_sum=False):
    """Everything exactly; `sum` exactly where every partial sum is exact in double (integer-valued data),
    otherwise |got - fsum(finite)| <= n * 2^-53 * sum|x| for the n finite voxels of the row: the standard
    bound of n - 1 rounded double additions in any order."""
    (gc, gs), (wc, ws) = got, want
    assert gc.shape == wc.shape and gc.dtype == np.uint64, (what, gc.shape, wc.shape)
    assert np.array_equal(gc, wc), (what, "counts", np.argwhere(gc != wc)[:5])
    for k in HR.SUMMARY[:5]:
        assert np.array_equal(gs[k], ws[k]), (what, k, gs[k], ws[k])
    for k in ("min", "max"):
        assert PR.same_bits(gs[k], ws[k]) == 1.0, (what, k, gs[k], ws[k])
    for r in range(len(ws["sum"])):
        d = abs(float(gs["sum"][r]) - float(ws["sum"][r]))
        bound = 0.0 if exact_sum else float(ws["finite"][r]) * 2.0 ** -53 * float(ws["abs_sum"][r])
        print(f"{what} row {r}: sum {gs['sum'][r]!r} vs {ws['sum'][r]!r}, |d| {d:.3g}, bound {bound:.3g}")
        assert d <= bound, (what, "sum", r, d, bound)


# ---- the volumes: each shape the smallest that reaches a distinct path ---------------------------------------

def ragged_volume():
    """17 x 9 x 5, signed, with +inf and NaN (tests/test_gpu_slice.py's), plus a -inf and a -0."""
    v = np.random.default_rng(20241218).random((17, 9, 5), dtype=F) - F(0.5)
    v[12, 2, 1] = np.inf
    v[3, 6, 3] = np.nan
    v[0, 8, 4] = -np.inf
    v[16, 0, 0] = -0.0
    return np.asfortranarray(v)


def _rand(shape, seed):
    return np.asfortranarray(np.random.default_rng(seed).random(shape, dtype=F) - F(0.25))


def _one_per_row():
    v = np.zeros((64, 8, 4), F)
    for k in range(4):
        for j in range(8):
            v[(7 * j + 13 * k) % 64, j, k] = F(0.5) + F(j) / F(16)
    return np.asfortranarray(v)


# name -> (volume, limits, integer-valued)
VOLUMES = {
    "ragged": (ragged_volume, (-0.4, 0.45), False),
    "row_longer_than_a_wave": (lambda: _rand((70, 3, 2), 70), (-0.25, 0.75), False),
    "row_longer_than_a_workgroup": (lambda: _rand((300, 2, 3), 300), (0.0, 0.5), False),
    "flat": (lambda: _rand((33, 7), 33), (-0.25, 0.75), False),
    "one_voxel": (lambda: np.full((1, 1), 2.5, F), (0.0, 2.5), True),
    "zeros": (lambda: np.zeros((64, 8, 4), F, order="F"), (0.0, 1.0), True),
    "zeros_but_one_per_row": (_one_per_row, (0.0, 1.0), True),
    "integers": (lambda: np.asfortranarray(np.random.default_rng(8).integers(0, 9, (21, 6, 5)).astype(F)), (0.0, 8.0), True),
}


@pytest.mark.parametrize("name", sorted(VOLUMES))
def test_volume_equals_the_reference(name, monkeypatch):
    mk, lim, integer = VOLUMES[name]
    vol = mk()
    h = new_handle(vol)
    for nbins in NBINS:
        want = HR.histogram(vol, nbins, lim)
        q = query(nbins, lim)
        for i, got in enumerate(both_paths(monkeypatch, lambda: gpu_hist(h, q))):
            assert_equal(got, want, (name, nbins, "uniform" if i == 0 else "plain"), integer)
        assert_equal(gpu_hist_device(h, q), want, (name, nbins, "device"), integer)
        assert want[1]["total"][0] == vol.size
    vr.volumeRender("delete", h)
    if name == "ragged":
        s = HR.histogram(vol, 7, lim)[1]
        assert s["nan"][0] == 1 and s["ninf"][0] == 2 and s["below"][0] > 1 and s["above"][0] > 1
        assert np.isneginf(s["min"][0]) and np.isposinf(s["max"][0])
    if name == "integers":  # value k lands in bin k, and 8 in bin 7
        c = HR.histogram(vol, 8, lim)[0][0]
        bc = np.bincount(vol.astype(np.int64).reshape(-1), minlength=9)
        assert np.array_equal(c[:7], bc[:7].astype(np.uint64)) and c[7] == bc[7] + bc[8] and bc[8] > 0
    if name == "zeros_but_one_per_row":
        c = HR.histogram(vol, 256, lim)[0][0]
        assert c[0] == vol.size - 32 and c.sum() == vol.size and (c[1:] > 0).sum() == 8


def test_minus_zero_and_plus_zero_extrema_keep_their_sign():
    for vals, smin, smax in (([0.0, -0.0, 0.0], True, False), ([-0.0, -0.0], True, True), ([0.0, 0.0], False, False)):
        vol = np.asfortranarray(F(vals).reshape(-1, 1, 1))
        h = new_handle(vol)
        got = gpu_hist(h, query(4, (-1, 1)))
        assert_equal(got, HR.histogram(vol, 4, (-1, 1)), vals, True)
        assert bool(np.signbit(got[1]["min"][0])) == smin and bool(np.signbit(got[1]["max"][0])) == smax
        vr.volumeRender("delete", h)


def test_unbound_sources_contribute_nothing():
    h = fresh_handle()  # nothing synced: every texture unbound
    for source in SOURCES:
        for nbins, labels in ((1, (0, 0)), (256, (0, 0)), (4096, (0, 0))):
            q = query(nbins, (0, 1), source, labels)
            want = HR.histogram(None, nbins, (0, 1))
            assert_equal(gpu_hist(h, q), want, (source, nbins), True)
            assert_equal(gpu_hist_device(h, q), want, (source, nbins, "device"), True)
    # with labels resident the rows by label are empty too
    mex.sync_labels(h, np.zeros((4, 4, 4), np.uint8, order="F"))
    got = gpu_hist(h, query(16, (0, 1), "emission", (0, 3)))
    assert_equal(got, HR.histogram(None, 16, (0, 1), None, 0, 3), "unbound, labels", True)
    assert np.isnan(got[1]["min"]).all() and np.isnan(got[1]["max"]).all() and not got[1]["total"].any()
    vr.volumeRender("delete", h)


# ---- sources: the slot indices and the alias rule, as vr_render_slice resolves them ----------------------------

SEPARATE = np.asfortranarray(np.random.default_rng(5).random((7, 11, 6), dtype=F))
BINDINGS = {"separate": lambda em: (SEPARATE, np.full((1, 1), 1.0, F)),
            "ab_is_re": lambda em: (SEPARATE, SEPARATE)}


def oracle_sources(em, ab, re):
    """What a 'render' samples as emission, absorption and reflection after this sync on a fresh process
    state, by the reference's host model (tests/test_gpu_slice.py's)."""
    import oracle as O
    S = O.OracleSession()
    hs = S.new()
    e, a, r = O.OVolume(em, STAMP_EM), O.OVolume(ab, STAMP_AB), O.OVolume(re, STAMP_RE)
    S.sync_volumes(hs, 0, e, a if re is ab else r, a)
    return [SR.source_volume(S, i) for i in range(3)]


def test_every_source_through_the_slot_indices_and_the_alias_rule():
    em = ragged_volume()
    grids = set()
    for case, mk in BINDINGS.items():
        ab, re = mk(em)
        vols = oracle_sources(em, ab, re)
        grids |= {v.shape for v in vols if v is not None}
        h = fresh_handle()
        va = V(ab, STAMP_AB)
        vr.volumeRender("sync_volumes", h, np.uint64(0), V(em, STAMP_EM), va if re is ab else V(re, STAMP_RE), va)
        for i, source in enumerate(SOURCES):
            want = HR.histogram(vols[i], 47, (-0.4, 0.9))
            assert_equal(gpu_hist(h, query(47, (-0.4, 0.9), source)), want, (case, source))
            assert_equal(gpu_hist(h, query(47, (-0.4, 0.9), i)), want, (case, source, "code"))
        vr.volumeRender("delete", h)
    assert grids == {(17, 9, 5), (7, 11, 6), (1, 1, 1)}


def test_uint8_unorm_upload_counts_as_single_of_data_over_255():
    u8 = np.asfortranarray(np.random.default_rng(11).integers(0, 256, (19, 13, 11), dtype=np.uint8))
    raw = vr.RawVolume(u8, unorm=True)
    raw.TimeLastUpdate = np.uint64(STAMP_EM)
    h = new_handle(raw)
    held = (u8.astype(F) / F(255)).astype(F)
    assert np.array_equal(held, mex.convert_host(u8, unorm=True).reshape(u8.shape, order="F"))
    for nbins, lim in ((256, (0, 1)), (255, (0, 1)), (7, (0.25, 0.5))):
        assert_equal(gpu_hist(h, query(nbins, lim)), HR.histogram(held, nbins, lim), ("unorm", nbins))
    vr.volumeRender("delete", h)


# ---- labels ---------------------------------------------------------------------------------------------------

LABEL_CASES = {"one": (0, 1, 256), "all": (0, 256, 47), "mid": (3, 5, 256), "top": (250, 6, 256)}


def label_volume(shape):
    """Labels 0..9 and, sprinkled in, 249..255: present below, inside and above every range of LABEL_CASES."""
    rng = np.random.default_rng(9)
    lab = rng.integers(0, 10, shape, dtype=np.uint8)
    hi = rng.random(shape) < 0.2
    lab[hi] = rng.integers(249, 256, int(hi.sum()), dtype=np.uint8)
    return np.asfortranarray(lab)


@pytest.mark.parametrize("case", sorted(LABEL_CASES))
def test_rows_by_label_equal_the_reference_on_the_masked_data(case, monkeypatch):
    first, count, nbins = LABEL_CASES[case]
    em = ragged_volume()
    labels = label_volume(em.shape)
    h = new_handle(em)
    mex.sync_labels(h, labels)
    lim = (-0.4, 0.45)
    want = HR.histogram(em, nbins, lim, labels, first, count)
    q = query(nbins, lim, "emission", (first, count))
    for i, got in enumerate(both_paths(monkeypatch, lambda: gpu_hist(h, q))):
        assert_equal(got, want, (case, "uniform" if i == 0 else "plain"))
    assert_equal(gpu_hist_device(h, q), want, (case, "device"))
    # each row is the one-row histogram of Data(labels == l); the last row collects every other label
    for r in sorted({0, count // 2, count - 1}):
        l = first + r
        alone = HR.histogram(em.reshape(-1, order="F")[labels.reshape(-1, order="F") == l].reshape(-1, 1, 1), nbins, lim)
        assert np.array_equal(want[0][r], alone[0][0]) and want[1]["total"][r] == (labels == l).sum()
    outside = (labels < first) | (labels >= first + count)
    assert want[1]["total"][count] == outside.sum() and want[1]["total"].sum() == em.size
    assert (labels >= first + count).any() or first + count == 256
    if case != "all":
        assert outside.sum() > 0
    vr.volumeRender("delete", h)


def test_label_gains_show_in_the_emission_histogram():
    em = ragged_volume()
    labels = np.asfortranarray(np.random.default_rng(9).integers(0, 4, em.shape, dtype=np.uint8))
    gains = F([1, 0.25, -2, 0])
    h = new_handle(em)
    mex.sync_labels(h, labels)
    mex.set_label_gains(h, gains)
    held = mex.label_gain_host(em, labels, gains)
    assert not np.array_equal(held.view(np.uint32), em.view(np.uint32))
    for source in ("emission", "absorption"):  # the alias follows
        assert_equal(gpu_hist(h, query(256, (-1, 1), source)), HR.histogram(held, 256, (-1, 1)), ("gains", source))
    assert_equal(gpu_hist(h, query(64, (-1, 1), "emission", (0, 4))), HR.histogram(held, 64, (-1, 1), labels, 0, 4),
                 "gains by label")
    mex.set_label_gains(h, None)
    assert_equal(gpu_hist(h, query(256, (-1, 1))), HR.histogram(em, 256, (-1, 1)), "gains cleared")
    vr.volumeRender("delete", h)


# ---- clip -----------------------------------------------------------------------------------------------------

OBLIQUE = F([[0.6, -0.3, 0.8, -0.35]])
CROP = F([[1, 0, 0, -0.25], [-1, 0, 0, 0.75], [0, 1, 0, -0.2], [0, -1, 0, 0.8], [0, 0, 1, -0.3], [0, 0, -1, 0.9]])


@pytest.mark.parametrize("planes", ["oblique", "crop"])
def test_clip_counts_the_voxels_whose_centre_the_planes_keep(planes, monkeypatch):
    pl = {"oblique": OBLIQUE, "crop": CROP}[planes]
    labels_of = label_volume
    for name in ("ragged", "row_longer_than_a_workgroup"):
        mk, lim, _ = VOLUMES[name]
        em = mk()
        labels = labels_of(em.shape)
        h = new_handle(em)
        mex.sync_labels(h, labels)
        unclipped = HR.histogram(em, 64, lim)
        assert_equal(gpu_hist(h, query(64, lim, clip=True)), unclipped, (name, "no planes, use_clip"))
        mex.set_clip(h, pl)
        assert_equal(gpu_hist(h, query(64, lim, clip=False)), unclipped, (name, "planes, use_clip = 0"))
        want = HR.histogram(em, 64, lim, planes=pl)
        for i, got in enumerate(both_paths(monkeypatch, lambda: gpu_hist(h, query(64, lim, clip=True)))):
            assert_equal(got, want, (name, planes, i))
        assert 0 < want[1]["total"][0] < em.size
        wantl = HR.histogram(em, 64, lim, labels, 3, 5, planes=pl)
        assert_equal(gpu_hist(h, query(64, lim, "emission", (3, 5), True)), wantl, (name, planes, "labels"))
        assert_equal(gpu_hist_device(h, query(64, lim, "emission", (3, 5), True)), wantl, (name, planes, "device"))
        assert wantl[1]["total"].sum() == want[1]["total"][0]
        vr.volumeRender("delete", h)


def test_a_plane_whose_terms_overflow_follows_the_fma_chain():
    em = _rand((12, 5, 3), 1)
    h = new_handle(em)
    for pl in (F([[3e38, -3e38, 0, 3e38]]), F([[-3e38, 3e38, 0, -3e38]])):  # the innermost fmaf overflows to +-inf
        mex.set_clip(h, pl)
        want = HR.histogram(em, 8, (0, 1), planes=pl)
        assert_equal(gpu_hist(h, query(8, (0, 1), clip=True)), want, ("overflowing plane", pl))
    vr.volumeRender("delete", h)


# ---- outputs --------------------------------------------------------------------------------------------------

def test_outputs_are_overwritten_and_repeatable():
    import torch
    em = ragged_volume()
    labels = label_volume(em.shape)
    h = new_handle(em)
    mex.sync_labels(h, labels)
    q = query(47, (-0.4, 0.45), "emission", (0, 256))
    want = HR.histogram(em, 47, (-0.4, 0.45), labels, 0, 256)
    assert (want[0] == 0).sum() > 1000  # cells no voxel touches: the garbage must go from them too
    a = gpu_hist_device(h, q)
    b = gpu_hist_device(h, q, stream=torch.cuda.Stream().cuda_stream)
    c = gpu_hist(h, q)
    for got, what in ((a, "device"), (b, "device, own stream"), (c, "host")):
        assert_equal(got, want, what)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], c[0])
    only_counts, none = gpu_hist_device(h, q, rows=False)  # d_rows may be NULL
    assert none is None and np.array_equal(only_counts, want[0])
    L = _lib.lib()
    counts = np.full((257, 47), 0xFFFFFFFFFFFFFFFF, np.uint64)
    assert L.vr_volume_histogram(mex._handle(h), ctypes.byref(q), counts.ctypes.data, None) == 0  # rows_out may be NULL
    assert np.array_equal(counts, want[0])
    vr.volumeRender("delete", h)


# ---- errors ---------------------------------------------------------------------------------------------------

def test_label_rows_need_labels_of_the_source_dims(monkeypatch):
    em = ragged_volume()
    h = new_handle(em)
    with pytest.raises(vr.VrError, match="labels") as e:
        gpu_hist(h, query(8, (0, 1), "emission", (0, 2)))
    assert e.value.code == 1
    mex.sync_labels(h, np.zeros((17, 9, 4), np.uint8, order="F"))
    for fn in (gpu_hist, gpu_hist_device):
        with pytest.raises(vr.VrError, match="labels' dims") as e:
            fn(h, query(8, (0, 1), "emission", (0, 2)))
        assert e.value.code == 1
    with pytest.raises(vr.VrError, match="labels' dims"):  # the reflection texture is the 1 x 1 x 1 default
        gpu_hist(h, query(8, (0, 1), "reflection", (0, 2)))
    assert_equal(gpu_hist(h, query(8, (0, 1))), HR.histogram(em, 8, (0, 1)), "labels not read")
    vr.volumeRender("delete", h)
    # a multi-device group handle (device 0 twice): one-device handles only
    monkeypatch.setenv("VR_DEVICES", "0,0")
    g = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    vr.volumeRender("sync_volumes", g, np.uint64(0), V(em, STAMP_EM), V(F(1.0), STAMP_RE), V(em, STAMP_EM))
    for fn in (gpu_hist, gpu_hist_device):
        with pytest.raises(vr.VrError, match="one-device handles only") as e:
            fn(g, query(8, (0, 1)))
        assert e.value.code == 5
    vr.volumeRender("delete", g)


# ---- state ----------------------------------------------------------------------------------------------------

def test_a_histogram_changes_nothing_of_the_handle():
    import oracle as O
    em = O.shell_volume(24)
    R = np.flip(O.rotation(125, 25, 0), 0).astype(F)
    argv = [False, False, F([1.5, 0.4, 0.6]), F([1, 1, 1]), np.uint64([40, 52]), R, F([0, 3, 6]), F(0.9), F([1, 1, 0])]
    h = new_handle(em)
    mex.sync_labels(h, label_volume(em.shape))
    mex.set_clip(h, OBLIQUE)
    before = vr.volumeRender("render", h, *argv)
    flags = mex.last_launch_flags()
    assert before.max() > 0
    for source in SOURCES:
        gpu_hist(h, query(256, (0, 1), source, (0, 0), True))
    gpu_hist(h, query(47, (0, 1), "emission", (0, 256), True))
    gpu_hist_device(h, query(4096, (0, 1)))
    assert mex.last_launch_flags() == flags
    after = vr.volumeRender("render", h, *argv)
    assert mex.last_launch_flags() == flags and PR.same_bits(before, after) == 1.0
    assert np.array_equal(mex.get_clip(h), OBLIQUE)
    vr.volumeRender("delete", h)
