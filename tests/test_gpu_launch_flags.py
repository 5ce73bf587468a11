"""Both sides of every launch-wide decision the host takes for the march, against the oracle.

While it builds a frame the host reads the upload statistics of the bound buffers, the factors, the
colours and the bindings and sets launch-wide flags (vr_capi.hip build_frame: small_x, eds_finite,
skip_empty, re_ok, lut_ok and, from all of them, tame); the kernels trust them (DESIGN.md "Launch-wide
decisions").  A proof that is wrong in the unsafe direction gives a silently wrong image, and the
march's variants read the same flags (of the kernels compared here only the plain one, VR_NO_LDS=1,
keeps the exponential's range test whatever small_x says), so what can tell is a reference that
does not know them: the oracle.

Volumes: the smallest that still get an occupancy map (2^18 padded voxels), so that a tame launch
probes and leaps: V_shell(64) (66^3 padded; a power-of-two cube, the half-texel-tap path) and the
non-cube V_shell(80)[:72, :56, :64] (74 * 58 * 66 padded).  Frame: the ex1_renderer set-up of
test_gpu_parity.py (two lights, 64^3 LUT, rotate(125, 25, 0), threshold 0.9) at 96 x 80.

Every scene gets three checks:
(a) oracle parity: the default render goes through tests/harness.py, i.e. conftest.assert_parity
    against the fp32 oracle inside the fp64 envelope (unchanged);
(b) kernel identity: the default render equals the renders under VR_NO_LDS=1, VR_DEPTH_LANES=1, 2, 4
    and (where skip_empty is set and the image is finite) VR_NO_EMPTY_SKIP=1, bit for bit, NaN
    positions equal;
(c) side taken: mex.last_launch_flags() is the word the scene's name promises, all eleven bits, and
    the counted launch of the frame probes or leaps (steps[7] + steps[46] > 0) exactly if it is tame.
"""
import gc

import numpy as np
import pytest

import oracle as O
from conftest import assert_parity

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("volume_renderer_amd")
torch = pytest.importorskip("torch")
import volume_renderer_amd.volume_render as vrmod  # noqa: E402
from volume_renderer_amd import mex  # noqa: E402

RES = (96, 80)  # (W, H)
THREADS = 8     # of the oracle
KEYS = ("VR_NO_LDS", "VR_NO_EMPTY_SKIP", "VR_DEPTH_LANES")
VARIANTS = [{"VR_NO_LDS": "1"}, {"VR_DEPTH_LANES": "1"}, {"VR_DEPTH_LANES": "2"}, {"VR_DEPTH_LANES": "4"}]
SPIKE_AT, SPIKE = (40, 30, 20), 1000.0


@pytest.fixture(autouse=True)
def _clean():
    gc.collect()
    yield
    gc.collect()


@pytest.fixture(scope="module")
def store():
    """Computed once, shared and left unchanged: the two volumes and the two Henyey-Greenstein LUTs."""
    s = dict(cube=O.shell_volume(64), slab=np.asfortranarray(O.shell_volume(80)[:72, :56, :64]),
             lut64=vr.HenyeyGreenstein(64), lut168=vr.HenyeyGreenstein(168))
    for a in s.values():
        a.setflags(write=False)
    return s


def tstep_of(dims):
    """The march's step of a volume with these dims and unit elements, in the host's fp32 arithmetic
    (vr_capi.hip build_frame): 1 / (2.2 * the shortest face diagonal)."""
    w, h, d = (np.float32(int(x) * int(x)) for x in dims)
    mind = min(np.sqrt(np.float32(w + h)), np.sqrt(np.float32(h + d)), np.sqrt(np.float32(w + d)))
    return np.float32(1) / (np.float32(2.2) * np.float32(mind))


def edge_of(data):
    """The FactorAbsorption at which small_x flips: |Fa * max|ab| * tstep| = 2^-7 * 0.999."""
    return 2.0 ** -7 * 0.999 / (float(tstep_of(data.shape)) * float(np.abs(data).max()))


def spiked(data, at=SPIKE_AT, value=SPIKE):
    d = np.array(data, order="F")
    d[at] = np.float32(value)
    return d


def renderer(store, data, lights=True):
    """tests/test_gpu_parity.py ex1_renderer (examples/example1.m:32-58 on synthetic data)."""
    r = vr.VolumeRender()
    if lights:
        r.VolumeIllumination = vr.Volume(store["lut64"])
        r.LightSources = [vr.LightSource([500, 1000, 550], [0, 1, 1]), vr.LightSource([0, 550, 90], [1, 0.5, 1])]
    r.ElementSizeUm = [1, 1, 1]
    r.FocalLength = 3.0
    r.DistanceToObject = 6
    r.rotate(125, 25, 0)
    r.OpacityThreshold = 0.9
    r.ImageResolution = list(RES)
    v = vr.Volume(data)
    r.VolumeEmission = v
    r.VolumeAbsorption = v
    r.FactorAbsorption = 0.6
    r.FactorReflection = 0.4
    r.Color = [1, 1, 0]
    return r


def flags(cube, lit=True, **changed):
    """The word of the plain scene (tame, on-the-fly gradient, absorption = emission, a map bound;
    half-texel taps on the power-of-two cube only), with the named bits changed."""
    f = dict(tame=True, small_x=True, eds_finite=True, skip_empty=True, re_ok=True, lut_ok=True,
             tap_half=cube and lit, ab_alias=True, share=lit, big=False, occ=True)
    assert set(changed) <= set(f)
    f.update(changed)
    return f


# name -> (what sets the scene up on the plain renderer, the bits that differ from the plain scene's)
def _fa(factor):
    def f(r, store, data):
        r.FactorAbsorption = factor(data) if callable(factor) else factor
    return f


def _re_em(r, store, data):
    r.VolumeReflection = r.VolumeEmission


def _re_rand(r, store, data):
    r.VolumeReflection = vr.Volume(O.rand_volume(16))


def _lut168(r, store, data):
    r.VolumeIllumination = vr.Volume(store["lut168"])


def _lut1(r, store, data):
    r.VolumeIllumination = vr.Volume(np.full((1, 1, 1), 0.37, np.float32))


def _color(c):
    def f(r, store, data):
        r.Color = c
    return f


NOT_SMALL = dict(small_x=False, tame=False)
SCENES = {
    # small_x
    "fa_0.6": (_fa(0.6), {}),  # (also: the default one-voxel reflection, the 64^3 LUT)
    "fa_below_edge": (_fa(lambda d: 0.998 * edge_of(d)), {}),
    "fa_above_edge": (_fa(lambda d: 1.002 * edge_of(d)), NOT_SMALL),
    "fa_40": (_fa(40.0), NOT_SMALL),
    "fa_1000": (_fa(1000.0), NOT_SMALL),
    # re_ok
    "re_is_emission": (_re_em, {}),
    "re_rand_16": (_re_rand, dict(re_ok=False, tame=False)),
    # lut_ok
    "lut_168": (_lut168, dict(lut_ok=False, tame=False)),
    "lut_one_texel": (_lut1, dict(lut_ok=False, tame=False)),
    # skip_empty
    "color_999": (_color([999, 1, 0]), {}),
    "color_1000": (_color([1000, 1, 0]), dict(skip_empty=False, tame=False)),
}
BOTH = ["fa_0.6", "fa_below_edge", "fa_above_edge", "fa_40", "fa_1000", "re_is_emission", "re_rand_16", "lut_168",
        "lut_one_texel"]
CASES = [(s, v) for s in BOTH for v in ("cube", "slab")] + [("color_999", "cube"), ("color_1000", "cube")]


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def assert_same(img, base, what):
    """Bit for bit, NaN positions equal (a NaN's sign and payload are not pinned across kernels)."""
    n = np.isnan(base)
    assert np.array_equal(np.isnan(img), n), (what, "NaN positions")
    assert np.array_equal(bits(img)[~n], bits(base)[~n]), what


def render_with(monkeypatch, r, env):
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    img = r.render()
    for k in env:
        monkeypatch.delenv(k)
    return img


def counted(r):
    """The counter variant's launch of the renderer's current frame (as test_gpu_chunk_setup.py): its
    48 counters and its image."""
    W, H = RES
    ra, keep = mex.render_args(r.LightSources, r.VolumeIllumination,
                               np.float32([r.FactorEmission, r.FactorReflection, r.FactorAbsorption]),
                               np.float32(r.ElementSizeUm), np.uint64([H, W]),
                               np.flip(r.RotationMatrix, 0).astype(np.float32),
                               np.float32([0, r.FocalLength, r.DistanceToObject]), np.float32(r.OpacityThreshold),
                               np.float32(r.Color))
    out = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    steps = torch.zeros(48, dtype=torch.int64, device="cuda")
    mex.render_device(r.objectHandle, ra, out.data_ptr(), None, steps.data_ptr())
    torch.cuda.synchronize()
    del keep
    return steps.cpu().numpy(), out.cpu().numpy()


def oracle_render(r, data=None, double=False):
    """The renderer's frame through the oracle's model of the reference, outside the harness (`data`:
    in place of the emission = absorption volume)."""
    S = O.OracleSession()
    h = S.new()
    ov = lambda v: O.OVolume(v.Data, int(v.TimeLastUpdate))  # noqa: E731
    em = ov(r.VolumeEmission) if data is None else O.OVolume(np.asfortranarray(data, dtype=np.float32), 1)
    re = em if r.VolumeReflection is r.VolumeEmission else ov(r.VolumeReflection)
    S.sync_volumes(h, 0, em, re, em)
    argv = r._render_argv(np.float32(0), np.flip(r.ImageResolution))
    lit = not isinstance(r.LightSources, (bool, np.bool_))
    L = np.float32([list(l.Position) + list(l.Color) for l in r.LightSources]).reshape(-1, 6) if lit else None
    img, _ = S.render(h, L, ov(r.VolumeIllumination) if lit else None, *argv[2:], double=double, threads=THREADS)
    return img


def check_identity_and_side(monkeypatch, r, base, want):
    """Checks (b) and (c) of a renderer whose default render `base` was just made."""
    got = mex.last_launch_flags()
    assert got == want, {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    variants = list(VARIANTS)
    if want["skip_empty"] and np.isfinite(base).all():
        variants.append({"VR_NO_EMPTY_SKIP": "1"})
    for env in variants:
        assert_same(render_with(monkeypatch, r, env), base, env)
    steps, img = counted(r)
    assert mex.last_launch_flags() == want  # (the counted launch is the same frame)
    assert_same(img, np.asarray(base, np.float32).reshape(-1, order="F"), "counted launch")
    print("flags", {k for k, v in got.items() if v}, "probes", steps[7], "failed", steps[44], "leaped unstaged", steps[46])
    if want["tame"]:
        assert steps[7] + steps[46] > 0
    else:
        assert steps[7] == 0 and steps[46] == 0 and steps[44] == 0


def harnessed(monkeypatch, make):
    """Check (a): the renderer `make` returns, made and rendered once through the lock-step harness
    (the oracle's fp32 and fp64 renders of the same calls, conftest.assert_parity inside).  Returns
    (renderer, image, fp32 oracle); what the renderer does afterwards goes to the library alone."""
    from harness import install
    real = vrmod.volumeRender
    tee = install(monkeypatch, threads=THREADS)
    r = make()
    img = r.render()
    monkeypatch.setattr(vrmod, "volumeRender", real)
    assert len(tee.renders) == 1
    print("parity", tee.renders[0][2])
    return r, img, tee.renders[0][1]


@pytest.mark.parametrize("scene,volume", CASES)
def test_each_side_of_each_decision(monkeypatch, counter_clock, store, scene, volume):
    """The table of the module docstring's decisions: FactorAbsorption below and above the small_x
    edge (computed from the data and the dims: 2^-7 * 0.999 / (tstep * max)), within 0.2 % of it on
    either side, and far above it (40: the opacity argument reaches 0.18 and most rays end within a
    few samples; 1000: it reaches 4.5).  The Taylor form's remainder is x^5 / 120: 1.6e-6 at 0.18,
    which is 1e-5 of the sample's opacity and inside the parity tolerance, so at 40 a wrongly set
    small_x shows in check (c) alone.  At 1000 the non-cube volume, whose wall crosses the box faces,
    meets x of several units on a ray's first sample and check (a) sees it too (measured with
    small_x forced: 171 NaN channels); on the cube the shell's ramp is 56 samples long, a ray ends
    near x = 0.5 and the image moves by 2e-5 of its maximum, so there (a) needs the one-voxel spike
    of test_one_voxel_spike.  The reflection texture the default single voxel, the emission volume,
    or a 16^3 volume of its own.  The LUT 64^3, 168^3 (not small) or a single texel.  Color just below
    and at the bound of the empty-sample skip.  Checks (a), (b) and (c) on each."""
    setup, changed = SCENES[scene]
    data = store[volume]

    def make():
        r = renderer(store, data)
        setup(r, store, data)
        return r

    r, img, ref32 = harnessed(monkeypatch, make)
    assert np.isfinite(img).all() and img.max() > 0 and (ref32 > 0).any(axis=2).mean() > 0.1
    check_identity_and_side(monkeypatch, r, img, flags(volume == "cube", **changed))
    r.delete()


@pytest.mark.parametrize("volume", ["cube", "slab"])
def test_one_voxel_spike(monkeypatch, counter_clock, store, volume):
    """One voxel of 1000 at (40, 30, 20) with FactorAbsorption 0.6: the opacity argument is about 3 on
    the samples that touch it (the Taylor form would give exp(-3) = 1.375), so small_x must be clear.
    The spike inflates the image scale (the oracle's maximum rises from 0.127 to 0.773 on the cube
    while 6 of 7680 pixels change), which would hide an error on every other pixel inside
    1e-5 * max: assert_parity is called on the whole frame (the harness) and again on the pixels whose
    fp32 oracle value differs between the spiked and the unspiked volume.  That subset has fewer than
    1000 channels, where a 99.9 % share would allow no channel anyway: every channel of it must lie
    within the envelope (min_frac = 1); from 1000 channels on it keeps the 99.9 % share."""
    data = spiked(store[volume])
    r, img, ref32 = harnessed(monkeypatch, lambda: renderer(store, data))
    ref64 = oracle_render(r, double=True)
    plain = oracle_render(r, data=store[volume])
    hit = (bits(plain) != bits(ref32)).any(axis=2)
    print("spike: oracle max", plain.max(), "->", ref32.max(), "pixels changed", int(hit.sum()))
    assert 0 < hit.sum() < hit.size // 10 and ref32.max() > 3 * plain.max()
    sub = [np.ascontiguousarray(a[hit]).reshape(-1) for a in (img, ref32, ref64)]
    st = assert_parity(*sub, what="pixels the spike changes", min_frac=0.999 if sub[0].size >= 1000 else 1.0)
    print("parity on the spike's pixels", st)
    check_identity_and_side(monkeypatch, r, img, flags(volume == "cube", **NOT_SMALL))
    r.delete()


@pytest.mark.parametrize("spike", [False, True])
def test_emission_range(monkeypatch, counter_clock, store, spike):
    """FactorEmission = 3e38, unlit: every |Fe * em(p) * tstep| of V_shell(64) is finite (about 1e36),
    so eds_finite holds and the launch is tame; with the one-voxel spike of 1000 the product leaves
    the range (1.5e39) and it does not.  With the spike the image holds infinities and NaNs, which
    assert_parity cannot score: checks (b) and (c), and the isfinite and isnan masks equal those of
    the oracle's fp32 render.  Without it the image stays finite (the oracle's maximum is 3.2e35), so
    check (a) applies as well."""
    data = spiked(store["cube"]) if spike else store["cube"]
    r = renderer(store, data, lights=False)
    r.FactorEmission = 3e38
    xe = float(np.float32(3e38)) * float(data.max()) * float(tstep_of(data.shape))
    assert (xe < 1e38) == (not spike)
    img = r.render()
    ref32 = oracle_render(r)
    print("emission range: finite", np.isfinite(img).mean(), "nan", np.isnan(img).mean(), "inf", np.isinf(img).mean())
    assert np.array_equal(np.isfinite(img), np.isfinite(ref32))
    assert np.array_equal(np.isnan(img), np.isnan(ref32))
    assert np.isfinite(img).all() == (not spike)
    if not spike:
        print("parity", assert_parity(img, ref32, oracle_render(r, double=True), what="FactorEmission 3e38"))
    want = flags(True, lit=False, small_x=not spike, eds_finite=not spike, tame=not spike)
    check_identity_and_side(monkeypatch, r, img, want)
    r.delete()


# ---- the statistics see one voxel, on every upload route -----------------------------------------

CORNERS = {"first": lambda s: (0, 0, 0), "last": lambda s: (s[0] - 1, s[1] - 1, s[2] - 1),
           "row_end": lambda s: (s[0] - 1, 0, 0)}
ROUTES = ["pageable", "bounce", "uint16_chunked", "int16_min", "device"]
U16_SHAPE = (128, 128, 80)  # uint16: 32 planes per MiB, three chunks, the last one partial


def route_volume(store, route, at):
    """(volume as the binding takes it, FactorAbsorption, environment of the upload) of a route; the
    spike at index `at` (None: none), every other |voxel| far below the small_x edge at that factor."""
    if route in ("pageable", "bounce", "device"):
        d = np.array(store["cube"], order="F")
        if at is not None:
            d[at] = SPIKE
        if route == "device":
            t = torch.from_numpy(np.ascontiguousarray(d.reshape(-1, order="F"))).cuda()
            return mex.DeviceVolume.from_tensor(t, dims=d.shape), 0.6, {}
        return vr.Volume(d), 0.6, ({"VR_UPLOAD_BOUNCE": "1"} if route == "bounce" else {})
    rng = np.random.default_rng(5)
    if route == "uint16_chunked":
        d = np.asfortranarray(rng.integers(0, 61, U16_SHAPE).astype(np.uint16))
        if at is not None:
            d[at] = 65535
        return vr.RawVolume(d), 0.01, {"VR_UPLOAD_CHUNK_MB": "1"}
    d = np.asfortranarray(rng.integers(-60, 61, store["cube"].shape).astype(np.int16))
    if at is not None:
        d[at] = -32768
    return vr.RawVolume(d), 0.01, {}


def route_flags(monkeypatch, store, route, corner):
    r = renderer(store, store["cube"])
    shape = U16_SHAPE if route == "uint16_chunked" else store["cube"].shape
    v, fa, env = route_volume(store, route, CORNERS[corner](shape) if corner else None)
    r.FactorAbsorption = fa
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    vr.volumeRender("sync_volumes", r.objectHandle, np.uint64(0), v, r.VolumeReflection, v)
    for k in env:
        monkeypatch.delenv(k)
    img = vr.volumeRender("render", r.objectHandle, *r._render_argv(np.float32(0), np.flip(r.ImageResolution)))
    got = mex.last_launch_flags()
    r.delete()
    assert np.isfinite(img).all() and (img != 0).any()
    return got


@pytest.mark.parametrize("corner", list(CORNERS))
@pytest.mark.parametrize("route", ROUTES)
def test_statistics_see_one_voxel(monkeypatch, counter_clock, store, route, corner):
    """One voxel that alone takes the opacity argument past 2^-7, at the first index, the last index
    and the end of the first row of the volume, through each upload route: a pageable fp32 array, the
    pinned bounce ring (VR_UPLOAD_BOUNCE=1), a uint16 RawVolume (65535 among values <= 60, not UNORM)
    in 1 MiB chunks (VR_UPLOAD_CHUNK_MB=1: 128 x 128 x 80, so that there are three chunks and the
    corners lie in the first and in the last, partial one -- the 64^3 volume would cross in one), an
    int16 RawVolume whose only large value is -32768 (the statistic is of |voxel|), and a
    device-resident DeviceVolume.  The flags only: small_x, and with it tame, must be clear."""
    got = route_flags(monkeypatch, store, route, corner)
    assert got["occ"] and got["eds_finite"] and got["skip_empty"]
    assert not got["small_x"] and not got["tame"], got


@pytest.mark.parametrize("route", ROUTES)
def test_statistics_without_the_voxel(monkeypatch, counter_clock, store, route):
    """The control of test_statistics_see_one_voxel: the same volume without the voxel is small_x and
    tame on every route, so it is the voxel that clears the flags there."""
    got = route_flags(monkeypatch, store, route, None)
    assert got == flags(route != "uint16_chunked"), got  # (128 x 128 x 80 is no cube: exact taps)
