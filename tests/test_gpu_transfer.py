"""GPU tests of the transfer-function render (vr_render_transfer / vr_render_transfer_device,
vr_transfer.hip) against the CPU reference of tests/transfer_ref.py, against 'render' (a constant
colormap is render's exact-shading image bit for bit) and against itself across the kernel's variants
(table sizes, column partitions, the empty-space leap, 64-bit indexing, typed uploads).

Parity (conftest.assert_parity, the SURVEY 8c condition) against the reference with glibc's expf:
positions, sampler, lookup, shading and compositing order are the reference's op for op; the expected
differences are the opacity's exponential, exp_neg_rn against glibc's expf (one ulp on 0.0065 % of
uniformly drawn arguments; 0.056 % of the arguments of these frames, s12), and in lit
images the device acosf.  The bit-identical shares are printed, not asserted.

Bit for bit against the reference with the kernel's exponential restated (transfer_ref "kernel"): the
alpha plane of every parity scene, lit or not (no shading enters it), and the image of the unlit ones.
That reference is computed without lights: the opacity and the exit tests do not depend on them."""
import ctypes

import numpy as np
import pytest

import oracle as O
import projection_ref as PR
import transfer_ref as TR
from conftest import assert_parity
from golden_cases import STAMP_EM, STAMP_GRAD, STAMP_LUT, STAMP_RE

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import _lib, mex  # noqa: E402
from test_gpu_projection import BLOCK_ARGS, RAGGED_ARGS, block_volume  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32

# 7 distinct, non-monotone rows; a 5-entry alphamap that starts at 0
CMAP7 = np.asfortranarray(F([[0.1, 0.9, 0.3], [1.0, 0.2, 0.0], [0.3, 0.3, 1.2], [0.8, 1.0, 0.1], [0.0, 0.5, 0.7],
                             [0.9, 0.1, 0.4], [0.2, 0.7, 1.0]]))
AMAP5 = F([0.0, 0.2, 1.0, 0.6, 1.5])
# narrower than the shell volumes' data (0 .. ~1.05): both clamps are hit
TF_VALUE = dict(colormap=CMAP7, clim=(0.2, 0.7), alphamap=AMAP5, alim=(0.05, 0.8), coord="value")


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


def tail(tf):
    """The five 'render_transfer' arguments after the nine 'render' arguments."""
    am = tf.get("alphamap")
    return [np.asfortranarray(tf["colormap"], dtype=F), F(tf["clim"]), False if am is None else F(am).reshape(-1, 1),
            F(tf.get("alim", (0, 1))), tf.get("coord", "value")]


def gpu_transfer(h, argv, tf, part=None, count=False, alpha=True):
    """vr_render_transfer_device of the frame `argv` (the nine 'render' arguments) with the transfer
    function tf (a dict as TF_VALUE): (image [H, W, 3], alpha [H, W], (visited, fetched)); for a part
    the planes are [H, max_cols(, 3)]."""
    import torch
    ra, keep = mex.render_args(*argv)
    t, tkeep = mex.transfer(tf["colormap"], tf["clim"], tf.get("alphamap"), tf.get("alim", (0, 1)),
                            tf.get("coord", "value"))
    H, W = (int(x) for x in np.asarray(argv[4]).reshape(-1))
    cols = W if part is None else mex.partition_columns(W, mex.partition(part.block_cols, 0, part.num_parts))
    out = torch.full((3, cols, H), -7.0, dtype=torch.float32, device="cuda")
    al = torch.full((cols, H), -7.0, dtype=torch.float32, device="cuda")
    steps = torch.zeros(2, dtype=torch.int64, device="cuda")
    mex.render_transfer_device(h, ra, t, out.data_ptr(), al.data_ptr() if alpha else 0, part,
                               steps.data_ptr() if count else 0)
    torch.cuda.synchronize()
    del keep, tkeep
    s = steps.cpu().numpy()
    return (np.asfortranarray(out.cpu().numpy().transpose(2, 1, 0)), np.asfortranarray(al.cpu().numpy().T),
            (int(s[0]), int(s[1])))


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def share(a, b):
    a, b = np.ascontiguousarray(a, F).view(np.uint32), np.ascontiguousarray(b, F).view(np.uint32)
    return float((a == b).mean()) if a.size else 1.0


# ---- the scenes: product-side arguments and the oracle session, once per scene ------------------------

def nan_volume():
    """17 x 9 x 5, signed, with one NaN voxel."""
    v = np.random.default_rng(20241218).random((17, 9, 5), dtype=np.float32) - np.float32(0.5)
    v[3, 6, 3] = np.nan
    return np.asfortranarray(v)


UNLIT_ARGS = [F([1, 0.4, 0.6]), F([1, 1, 1]), np.uint64([36, 44]), np.flip(O.rotation(125, 25, 0), 0).astype(F),
              F([0, 3, 6]), F(0.9), F([1, 1, 0])]
_scenes, _refs = {}, {}


def scene(name):
    """name -> dict(em, re, grads, lights (LightSource list or False), lut (Volume or False), olights,
    olut (the oracle's), args (the seven arguments after the LUT), S, hs, fresh (() -> a new oracle session
    and handle with the scene's volumes synced and no lights uploaded))."""
    if name in _scenes:
        return _scenes[name]
    if name in PR.FRAMES:
        S, hs, sc, em = PR.scene_session(name)
        args = PR.frame_args(sc, PR.FRAMES[name])
        lit = name != "stereo_right_24"  # (rendered unlit here; its props[0] is not 0)
        lut = vr.HenyeyGreenstein(sc["lut"])
        d = dict(em=em, re=sc["re"]() if sc["re"] else None, grads=O.matlab_gradient(em) if sc["grads"] else None,
                 lights=[vr.LightSource(l[:3], l[3:]) for l in sc["lights"]] if lit else False,
                 lut=V(lut, STAMP_LUT) if lit else False, olights=sc["lights"] if lit else None,
                 olut=O.OVolume(O.hg_lut(sc["lut"]), STAMP_LUT) if lit else None,
                 fresh=lambda: PR.scene_session(name)[:2])
    else:
        em, args = {"c1_40": (lambda: O.shell_volume(40), UNLIT_ARGS), "block": (lambda: block_volume(False), BLOCK_ARGS),
                    "nan": (nan_volume, RAGGED_ARGS), "one_voxel": (lambda: np.full((1, 1), 2.5, F), RAGGED_ARGS),
                    "flat": (lambda: np.asfortranarray(np.random.default_rng(5).random((9, 7), dtype=F)),
                             RAGGED_ARGS)}[name]
        em = em()
        S, hs = PR.session(em, STAMP_EM)
        d = dict(em=em, re=None, grads=None, lights=False, lut=False, olights=None, olut=None,
                 fresh=lambda: PR.session(em, STAMP_EM))
    d.update(args=args, S=S, hs=hs)
    _scenes[name] = d
    return d


def argv_of(sc):
    return [sc["lights"], sc["lut"]] + list(sc["args"])


def reference(name, tf, key, exact=False):
    """transfer_ref.transfer of scene `name` with tf, computed once per (name, key).  exact: the fp32
    reference alone, unlit, with the kernel's exponential (the bit-for-bit planes of the module docstring)."""
    if (name, key, exact) not in _refs:
        sc = scene(name)
        t = TR.make_tf(tf["colormap"], tf["clim"], tf.get("alphamap"), tf.get("alim", (0, 1)), tf.get("coord", "value"))
        if exact:  # (a session of its own: one that has rendered lit keeps its lights)
            S, hs = sc["fresh"]()
            _refs[(name, key, exact)] = TR.transfer(S, hs, t, None, None, *sc["args"], double=False, exp="kernel")
        else:
            _refs[(name, key, exact)] = TR.transfer(sc["S"], sc["hs"], t, sc["olights"], sc["olut"], *sc["args"])
    return _refs[(name, key, exact)]


def check_parity(got, name, tf, key, what):
    """Image and alpha plane of scene `name` within the SURVEY 8c condition of the glibc reference (the
    identical shares printed); the alpha plane, and the image of an unlit scene, bit for bit those of
    the reference with the kernel's exponential.  Returns the glibc reference."""
    ref = reference(name, tf, key)
    print(f"{what}: bit-identical share image {share(got[0], ref['img']):.6f}, alpha {share(got[1], ref['alpha']):.6f}")
    assert_parity(got[0], ref["img"], ref["img64"].astype(F), f"{what} image")
    assert_parity(got[1], ref["alpha"], ref["alpha64"].astype(F), f"{what} alpha")
    ex = reference(name, tf, key, exact=True)
    assert same_bits(got[1], ex["alpha"]), f"{what}: alpha differs from the exact reference in " \
        f"{int((got[1].view(np.uint32) != ex['alpha'].view(np.uint32)).sum())} pixels"
    if scene(name)["lights"] is False:
        assert same_bits(got[0], ex["img"]), f"{what}: the unlit image differs from the exact reference"
    return ref


def same_bits(a, b):
    """Identical bits, NaN == NaN whatever the payload; NaN positions must agree."""
    return PR.same_bits(a, b) == 1.0


def constant_tf(color, n=2):
    return dict(colormap=TR.constant_colormap(color, n), clim=(0, 1))


# ---- 1. anchor: a constant colormap is render's exact-shading image ------------------------------------

@pytest.mark.parametrize("name", ["hg2_compute_32", "hg1_lookup_24", "c1_40"])
def test_constant_colormap_is_the_exact_render_bit_for_bit(name, monkeypatch):
    sc = scene(name)
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    tf = constant_tf(sc["args"][6])
    monkeypatch.setenv("VR_EXACT_SHADE", "1")
    want = vr.volumeRender("render", h, *argv_of(sc))
    monkeypatch.delenv("VR_EXACT_SHADE")
    got = gpu_transfer(h, argv_of(sc), tf, count=True)
    assert want.max() > 0
    assert bits_equal(got[0], want), f"{int((got[0].view(np.uint32) != want.view(np.uint32)).sum())} values differ"
    ref = check_parity(got, name, tf, "const", name + " anchor")
    # (check_parity: the alpha plane bit for bit the exact reference's, within parity of the glibc one's)
    _, total = sc["S"].render(sc["hs"], sc["olights"], sc["olut"], *sc["args"])
    assert got[2][0] == total == int(ref["n"].sum())
    # the host entry point and the command write the same planes
    img, alpha = vr.volumeRender("render_transfer", h, *argv_of(sc), *tail(tf))
    assert bits_equal(img, got[0]) and bits_equal(alpha, got[1])
    vr.volumeRender("delete", h)


# ---- 2. parity with the reference ----------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hg2_compute_32", "hg1_lookup_24", "stereo_right_24"])
def test_value_coded_transfer_equals_the_reference(name):
    sc = scene(name)
    assert name != "stereo_right_24" or sc["args"][4][0] != 0  # props[0]
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    got = gpu_transfer(h, argv_of(sc), TF_VALUE)
    ref = check_parity(got, name, TF_VALUE, "value", name)
    assert got[0].max() > 0 and (ref["alpha"] > 0).any()
    vr.volumeRender("delete", h)


def test_depth_coded_transfer_equals_the_reference():
    name = "hg2_compute_32"
    sc = scene(name)
    P, keep, _ = sc["S"].params(sc["hs"], None, None, *sc["args"])
    R = PR.rays(P)
    hit = R["hit"]
    lo, hi = float(R["tnear"][hit].min()), float(R["tfar"][hit].max())  # the t range of the box
    tf = dict(colormap=CMAP7, clim=(lo, hi), alphamap=AMAP5, alim=(0.05, 0.8), coord="depth")
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    got = gpu_transfer(h, argv_of(sc), tf)
    check_parity(got, name, tf, "depth", name + " depth")
    value = gpu_transfer(h, argv_of(sc), dict(tf, coord="value"))
    assert not bits_equal(got[0], value[0]) and bits_equal(got[1], value[1])  # (colour only)
    vr.volumeRender("delete", h)


# ---- 3. table sizes: the looped LDS fill and the largest allocation -----------------------------------

@pytest.mark.parametrize("n", [2, 257, 1024])
def test_table_sizes(n):
    sc = scene("c1_40")
    rng = np.random.default_rng(n)
    tf = dict(colormap=np.asfortranarray(rng.random((n, 3), dtype=F)), clim=(0.1, 0.9),
              alphamap=np.concatenate([F([0]), rng.random(n - 1, dtype=F) * F(2)]), alim=(0.0, 1.0))
    h = new_handle(sc["em"])
    got = gpu_transfer(h, argv_of(sc), tf)
    check_parity(got, "c1_40", tf, f"n{n}", f"n = {n}")
    vr.volumeRender("delete", h)


def test_back_to_back_launches_each_read_their_own_tables():
    """More launches in flight than the table staging ring has slots (16), each with its own 257-entry
    colormap (8 KiB: above the 4 KiB constants ring), none synchronised in between: every image is the
    one its colormap gives alone."""
    import torch
    sc = scene("c1_40")
    h = new_handle(sc["em"])
    ra, keep = mex.render_args(*argv_of(sc))
    H, W = (int(x) for x in sc["args"][2])
    rng = np.random.default_rng(3)
    maps = [np.asfortranarray(rng.random((257, 3), dtype=F)) for _ in range(20)]
    outs = torch.zeros((len(maps), 3, W, H), dtype=torch.float32, device="cuda")
    tfs = [mex.transfer(m, (0.1, 0.9)) for m in maps]
    for k, (t, _) in enumerate(tfs):
        mex.render_transfer_device(h, ra, t, outs[k].data_ptr())
    torch.cuda.synchronize()
    got = outs.cpu().numpy()
    for k in (0, 3, 15, 16, 19):
        alone = gpu_transfer(h, argv_of(sc), dict(colormap=maps[k], clim=(0.1, 0.9)))[0]
        assert bits_equal(np.asfortranarray(got[k].transpose(2, 1, 0)), alone), k
    assert not np.array_equal(got[0], got[19]) and got.max() > 0
    vr.volumeRender("delete", h)
    del keep, tfs


# ---- 4. partial tiles and column partitions -------------------------------------------------------------

def test_partitioned_transfer_assembles_to_the_whole_frame():
    import torch
    sc = scene("stereo_right_24")
    h = new_handle(sc["em"], sc["re"])
    H, W = PR.FRAMES["stereo_right_24"]
    bc, nparts = 8, 3
    assert W == 41
    maxc = mex.partition_columns(W, mex.partition(bc, 0, nparts))
    whole = gpu_transfer(h, argv_of(sc), TF_VALUE, count=True)
    parts = torch.zeros((nparts, 3, maxc, H), dtype=torch.float32, device="cuda")
    alpha = np.full((H, W), -7.0, np.float32, order="F")
    visited = fetched = 0
    for p in range(nparts):
        pt = mex.partition(bc, p, nparts)
        img_p, alpha_p, st = gpu_transfer(h, argv_of(sc), TF_VALUE, part=pt, count=True)
        parts[p] = torch.from_numpy(np.ascontiguousarray(img_p.transpose(2, 1, 0))).cuda()
        visited += st[0]
        fetched += st[1]
        lc = 0  # the part's local columns, in increasing x: blocks p, p + nparts, ...
        for b in range(p, (W + bc - 1) // bc, nparts):
            for x in range(b * bc, min((b + 1) * bc, W)):
                alpha[:, x] = alpha_p[:, lc]
                lc += 1
        assert lc == mex.partition_columns(W, pt)
    out = torch.zeros((3, W, H), dtype=torch.float32, device="cuda")
    mex.assemble_partitions(parts.data_ptr(), W, H, bc, nparts, maxc, out.data_ptr())
    torch.cuda.synchronize()
    img = np.asfortranarray(out.cpu().numpy().transpose(2, 1, 0))
    assert bits_equal(img, whole[0]) and bits_equal(alpha, whole[1])
    assert visited == whole[2][0] and fetched == whole[2][1]
    vr.volumeRender("delete", h)


# ---- 5. the empty-space leap ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", ["value", "depth", "lit"])
def test_empty_space_leap_changes_no_bit(case, monkeypatch):
    """value: against the reference too.  depth: the colormap coordinate is the t the leap replays.
    lit: two lights on the block volume, the leap legal through skip_empty."""
    sc = scene("block")
    argv, tf = argv_of(sc), TF_VALUE
    if case == "depth":
        P, keep, _ = sc["S"].params(sc["hs"], None, None, *sc["args"])
        R = PR.rays(P)
        tf = dict(TF_VALUE, coord="depth", clim=(float(R["tnear"][R["hit"]].min()), float(R["tfar"][R["hit"]].max())))
    if case == "lit":
        lit = scene("hg2_compute_32")
        argv = [lit["lights"], lit["lut"]] + list(sc["args"])
    h = new_handle(sc["em"])
    monkeypatch.delenv("VR_TF_NO_PROBE", raising=False)
    # (first: the logical false for the lights keeps whatever a lit call uploaded, as 'render' does)
    value = gpu_transfer(h, argv_of(sc), TF_VALUE)
    leap = gpu_transfer(h, argv, tf, count=True)
    monkeypatch.setenv("VR_TF_NO_PROBE", "1")
    plain = gpu_transfer(h, argv, tf, count=True)
    monkeypatch.delenv("VR_TF_NO_PROBE")
    uncounted = gpu_transfer(h, argv, tf)  # (the kernel without the counters)
    for other in (plain, uncounted):
        assert bits_equal(leap[0], other[0]) and bits_equal(leap[1], other[1])
    total = int(reference("block", TF_VALUE, "value")["n"].sum())  # (the same rays and opacities in every case)
    if case == "value":
        check_parity(leap, "block", TF_VALUE, "value", "block")
    else:
        assert not bits_equal(leap[0], value[0]) and bits_equal(leap[1], value[1])  # (colour only)
    assert leap[2][0] == total and plain[2][0] == total
    assert plain[2][1] == plain[2][0]
    assert leap[2][1] < leap[2][0], leap[2]  # the leap ran
    assert leap[0].max() > 0
    vr.volumeRender("delete", h)


def test_an_alphamap_that_is_opaque_at_zero_does_not_leap():
    sc = scene("block")
    tf = dict(TF_VALUE, alphamap=F([0.3, 0.2, 1.0, 0.6, 1.5]), alim=(0.0, 0.8))  # A(0) = 0.3
    h = new_handle(sc["em"])
    got = gpu_transfer(h, argv_of(sc), tf, count=True)
    ref = check_parity(got, "block", tf, "opaque0", "block, A(0) > 0")
    assert got[2][1] == got[2][0] == int(ref["n"].sum())
    assert (ref["alpha"][ref["hit"]] > 0).all()  # empty space is not empty under this map
    vr.volumeRender("delete", h)


# ---- 6. variants ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["hg2_compute_32", "hg1_lookup_24", "block"])
def test_forced_64_bit_indexing_changes_no_bit(name, monkeypatch):
    sc = scene(name)
    h = new_handle(sc["em"], sc["re"], sc["grads"])
    monkeypatch.delenv("VR_FORCE_BIG", raising=False)
    a = gpu_transfer(h, argv_of(sc), TF_VALUE)
    monkeypatch.setenv("VR_FORCE_BIG", "1")
    b = gpu_transfer(h, argv_of(sc), TF_VALUE)
    monkeypatch.delenv("VR_FORCE_BIG")
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])
    assert a[0].max() > 0
    vr.volumeRender("delete", h)


def test_uint8_volume_renders_as_its_fp32_twin():
    u8 = np.asfortranarray(np.random.default_rng(11).integers(0, 256, (19, 13, 11), dtype=np.uint8))
    raw = vr.RawVolume(u8)
    raw.TimeLastUpdate = np.uint64(STAMP_EM)
    argv = [False, False, F([1, 0.4, 0.01])] + RAGGED_ARGS[1:]
    tf = dict(TF_VALUE, clim=(20, 200), alim=(10, 250))
    h8, h32 = new_handle(raw), new_handle(u8.astype(np.float32))
    a, b = gpu_transfer(h8, argv, tf), gpu_transfer(h32, argv, tf)
    assert bits_equal(a[0], b[0]) and bits_equal(a[1], b[1])
    assert a[0].max() > 0 and 0 < a[1].max() <= 1
    vr.volumeRender("delete", h8)
    vr.volumeRender("delete", h32)


# ---- 7. degenerate and hostile inputs -------------------------------------------------------------------

def test_no_volume_synced_writes_zeros():
    h = vr.volumeRender("new")
    img, alpha, _ = gpu_transfer(h, [False, False] + RAGGED_ARGS, TF_VALUE)
    assert (img == 0).all() and (alpha == 0).all()
    img, alpha = vr.volumeRender("render_transfer", h, False, False, *RAGGED_ARGS, *tail(TF_VALUE))
    assert (img == 0).all() and (alpha == 0).all()
    vr.volumeRender("delete", h)


@pytest.mark.parametrize("name", ["one_voxel", "flat"])
def test_degenerate_textures(name):
    sc = scene(name)
    tf = dict(TF_VALUE, clim=(0.2, 3.0), alim=(0.0, 3.0))
    h = new_handle(sc["em"])
    got = gpu_transfer(h, argv_of(sc), tf)
    ref = check_parity(got, name, tf, "value", name)
    assert (ref["n"] > 0).any() and got[0].max() > 0
    vr.volumeRender("delete", h)


def test_nan_voxel_reaches_the_same_pixels():
    sc = scene("nan")
    tf = dict(TF_VALUE, clim=(-0.3, 0.3), alim=(-0.5, 0.5))
    h = new_handle(sc["em"])
    got = gpu_transfer(h, argv_of(sc), tf)
    ref = reference("nan", tf, "value")
    assert np.isnan(ref["img"]).any() and not np.isnan(ref["img"]).all()
    assert np.array_equal(np.isnan(got[0]), np.isnan(ref["img"]))
    assert np.array_equal(np.isnan(got[1]), np.isnan(ref["alpha"]))
    check_parity(got, "nan", tf, "value", "nan voxel")  # (NaN masks equal, the finite pixels within the envelope)
    vr.volumeRender("delete", h)


# ---- 8. no side effects ---------------------------------------------------------------------------------

def test_a_transfer_render_between_two_renders_changes_neither():
    sc = scene("hg2_compute_32")
    h = new_handle(sc["em"])
    first = vr.volumeRender("render", h, *argv_of(sc))
    assert first.max() > 0
    gpu_transfer(h, argv_of(sc), TF_VALUE, count=True)
    vr.volumeRender("render_transfer", h, *argv_of(sc), *tail(TF_VALUE))
    again = vr.volumeRender("render", h, *argv_of(sc))
    assert bits_equal(first, again)
    vr.volumeRender("delete", h)


# ---- 9. errors that need a handle -------------------------------------------------------------------------

def test_transfer_errors_with_a_handle(monkeypatch):
    import torch
    sc = scene("hg2_compute_32")
    L = _lib.lib()
    h = new_handle(sc["em"])
    hp = mex._handle(h)
    ra, keep = mex.render_args(*argv_of(sc))
    tf, tkeep = mex.transfer(CMAP7, (0, 1))
    H, W = PR.FRAMES["hg2_compute_32"]
    out = np.zeros(H * W * 3, np.float32)
    d_out = torch.zeros(H * W * 3, dtype=torch.float32, device="cuda")
    assert L.vr_render_transfer(hp, ctypes.byref(ra), ctypes.byref(tf), None, None) == 1
    assert b"output is NULL" in L.vr_last_error()
    assert L.vr_render_transfer_device(hp, ctypes.byref(ra), ctypes.byref(tf), None, None, None, None, None) == 1
    assert b"output is NULL" in L.vr_last_error()
    bad = mex.partition(8, 3, 3)
    assert L.vr_render_transfer_device(hp, ctypes.byref(ra), ctypes.byref(tf), ctypes.byref(bad), d_out.data_ptr(), None,
                                       None, None) == 1
    assert L.vr_render_transfer(hp, ctypes.byref(ra), ctypes.byref(tf), out.ctypes.data, None) == 0  # alpha may be NULL
    assert out.max() > 0
    vr.volumeRender("delete", h)
    # a multi-device group handle (device 0 twice): one-device handles only
    monkeypatch.setenv("VR_DEVICES", "0,0")
    g = vr.volumeRender("new")
    monkeypatch.delenv("VR_DEVICES")
    vr.volumeRender("sync_volumes", g, np.uint64(0), V(sc["em"], STAMP_EM), V(np.float32(1.0), STAMP_RE),
                    V(sc["em"], STAMP_EM))
    gp = mex._handle(g)
    assert L.vr_render_transfer(gp, ctypes.byref(ra), ctypes.byref(tf), out.ctypes.data, None) == 5
    assert b"one-device handles only" in L.vr_last_error()
    assert L.vr_render_transfer_device(gp, ctypes.byref(ra), ctypes.byref(tf), None, d_out.data_ptr(), None, None,
                                       None) == 5
    assert b"one-device handles only" in L.vr_last_error()
    vr.volumeRender("delete", g)
    del keep, tkeep
