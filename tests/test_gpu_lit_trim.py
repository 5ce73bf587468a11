"""Round-13 GPU tests of the lit sample's address, constant and flag arithmetic: the slot address of
a whole chunk with the box origin folded out and the gradient taps' byte offsets (vr_march.hip
sample_at, vr_stage.h half_grad_lds), the z-paired LUT's doubled offset terms (vr_sampling.h
fetch_small_z) and the ray flags of the depth-lane loop -- each against a render that does not take
the path (no staging, the general LUT fetch, no empty skip, another depth-lane count, the 64-bit
kernels), bit for bit, NaN positions equal.

The production path (half-texel taps, whole boxes) needs a power-of-two cube.  The volumes are
shells whose wall crosses all six faces of the cube, so that cells at i = -1 and i = n - 1 occur
and the boxes' origins take every small value."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("volume_renderer_amd")

RES = (64, 48)
KEYS = ("VR_NO_LDS", "VR_NO_EMPTY_SKIP", "VR_NO_SMALL_LUT", "VR_DEPTH_LANES", "VR_FORCE_BIG", "VR_MAX_STEPS")
# (rotation, distance to the object): along +-x, +-y, +-z, the metric frame's oblique view, and an
# eye close to a face of the box [-1, 1]^3
CAMERAS = [((0, 0, 0), 6), ((180, 0, 0), 6), ((90, 0, 0), 6), ((-90, 0, 0), 6), ((0, 90, 0), 6), ((0, -90, 0), 6),
           ((125, 25, 0), 6), ((20, 10, 0), 1.15)]
LIGHTS = [([500, 1000, 550], [0, 1, 1]), ([0, 550, 90], [1, 0.5, 1])]


@pytest.fixture(autouse=True)
def _clean():
    gc.collect()
    yield
    gc.collect()


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def same(a, b):
    """Bit for bit outside NaNs, NaN positions equal (a NaN's sign and payload are not pinned)."""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(bits(a)[~na], bits(b)[~nb])


def face_shell(n):
    """A spherical shell of radius 0.45 +- 0.12 (in units of the cube's edge) about the centre: its
    wall crosses every face of the cube (0.58 at a face's centre), the cube's centre and corners are
    empty (+0), and a ripple makes every gradient component non-trivial."""
    c = (np.arange(n, dtype=np.float64) + 0.5) / n
    x, y, z = c[:, None, None], c[None, :, None], c[None, None, :]
    r = np.sqrt((x - 0.5) ** 2 + (y - 0.5) ** 2 + (z - 0.5) ** 2)
    v = np.clip(1.0 - np.abs(r - 0.45) / 0.12, 0.0, 1.0)
    tp = 6.0 * np.pi
    v = v * (0.6 + 0.4 * np.sin(tp * x) * np.sin(tp * y) * np.sin(tp * z))
    return np.asfortranarray(np.maximum(v, 0.0).astype(np.float32))


_VOLUMES = {}
_LUTS = {}


def volume(n):
    """One upload per cube edge for the whole module (the renders only read it)."""
    if n not in _VOLUMES:
        data = face_shell(n)
        for f in (data[0], data[-1], data[:, 0], data[:, -1], data[:, :, 0], data[:, :, -1]):
            assert f.max() > 0  # the data reaches all six faces
        _VOLUMES[n] = vr.Volume(data)
    return _VOLUMES[n]


def lut(m):
    if m not in _LUTS:
        _LUTS[m] = vr.Volume(vr.HenyeyGreenstein(m))
    return _LUTS[m]


def renderer(vol, nl, m, rot, dist, thr=0.9):
    """examples/example1.m:32-58 on synthetic data: nl lights, on-the-fly gradient."""
    r = vr.VolumeRender()
    r.VolumeIllumination = lut(m)
    r.LightSources = [vr.LightSource(p, c) for p, c in LIGHTS[:nl]]
    r.ElementSizeUm = [1, 1, 1]
    r.FocalLength = 3.0
    r.DistanceToObject = dist
    r.rotate(*rot)
    r.OpacityThreshold = thr
    r.ImageResolution = list(RES)
    r.VolumeEmission = vol
    r.VolumeAbsorption = vol
    r.FactorAbsorption = 0.6
    r.FactorReflection = 0.4
    r.Color = [1, 1, 0]
    return r


def render_with(monkeypatch, r, env):
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    img = r.render()
    for k in env:
        monkeypatch.delenv(k)
    return img


def counted(r, env, monkeypatch):
    """The counter variant's launch of the renderer's current frame: its 48 counters."""
    import torch
    from volume_renderer_amd import mex
    W, H = RES
    for k in KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
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
    for k in env:
        monkeypatch.delenv(k)
    return steps.cpu().numpy(), out.cpu().numpy()


def check_frame(monkeypatch, r, what, extra=None):
    """Every identity of the module for one frame; `extra`: switches set in every render of it."""
    extra = dict(extra or {})
    by_k = {}
    for k in ("2", "4"):
        base = render_with(monkeypatch, r, dict(extra, VR_DEPTH_LANES=k))
        assert np.nanmax(base) > 0, (what, k)
        by_k[k] = base
        for sw in ("VR_NO_LDS", "VR_NO_SMALL_LUT", "VR_NO_EMPTY_SKIP"):
            other = render_with(monkeypatch, r, dict(extra, **{"VR_DEPTH_LANES": k, sw: "1"}))
            assert same(other, base), (what, "K=" + k, sw)
    by_k["1"] = render_with(monkeypatch, r, dict(extra, VR_DEPTH_LANES="1"))
    assert same(by_k["2"], by_k["4"]), (what, "K = 2 against K = 4")
    assert same(by_k["2"], by_k["1"]), (what, "K = 2 against K = 1")
    # the default launch (no depth-lane switch) is one of these kernels
    assert same(render_with(monkeypatch, r, extra), by_k["2"]), (what, "default")
    return by_k["2"]


def check_paths_taken(monkeypatch, r, img, what, extra=None):
    """The counted launch of the frame staged chunks and ran lit iterations, and renders the same
    image."""
    st, out = counted(r, dict(extra or {}), monkeypatch)
    print(f"{what}: staged {st[2]} leaped {st[3]} fall {st[4]} iterations {st[5]} lit {st[6]} "
          f"probes {st[7]} + {st[44]}")
    assert st[2] > 0 and st[6] > 0, (what, st[:9])
    # (the probe counters are printed only: a volume too small for an occupancy map has no probes)
    assert same(out, np.asarray(img, np.float32).reshape(-1, order="F")), (what, "counted launch")


@pytest.mark.parametrize("m", [16, 64])
@pytest.mark.parametrize("nl", [2, 1])
@pytest.mark.parametrize("n", [32, 64, 128])
def test_lit_sample_paths_agree(monkeypatch, counter_clock, n, nl, m):
    """For every camera: the default render equals the unstaged one (VR_NO_LDS=1: no slot address, no
    tap offsets), the one with the general LUT fetch (VR_NO_SMALL_LUT=1) and the one without the empty
    skip (VR_NO_EMPTY_SKIP=1), at 2 and at 4 depth lanes, and the renders at 1, 2 and 4 depth lanes
    are equal; the counted launch shows that chunks were staged and lit iterations ran."""
    vol = volume(n)
    for rot, dist in CAMERAS:
        what = f"n={n} lights={nl} lut={m} rot={rot} dist={dist}"
        r = renderer(vol, nl, m, rot, dist)
        img = check_frame(monkeypatch, r, what)
        check_paths_taken(monkeypatch, r, img, what)
        r.delete()


@pytest.mark.parametrize("nl", [2, 1])
def test_step_cap_ends_rays_inside_a_chunk(monkeypatch, counter_clock, nl):
    """A sample cap far below the chord length (VR_MAX_STEPS: 41 and 58 samples, no multiple of the
    chunk length or of a depth-lane count, where the 64^3 cube is about 140 steps across) ends every
    ray that enters the data inside a chunk, some lanes of a depth-lane group before the others."""
    vol = volume(64)
    for cap in ("41", "58"):
        for rot, dist in (CAMERAS[0], CAMERAS[6], CAMERAS[7]):
            what = f"cap={cap} lights={nl} rot={rot} dist={dist}"
            r = renderer(vol, nl, 64, rot, dist)
            free = render_with(monkeypatch, r, {})
            img = check_frame(monkeypatch, r, what, {"VR_MAX_STEPS": cap})
            assert not same(img, free), (what, "the cap did not end any ray")
            check_paths_taken(monkeypatch, r, img, what, {"VR_MAX_STEPS": cap})
            r.delete()


@pytest.mark.parametrize("nl", [2, 1])
def test_opacity_exit_inside_a_group(monkeypatch, counter_clock, nl):
    """An opacity threshold of 0.05 stops most rays a few samples into the shell's wall -- on the first
    or the second sample of a depth-lane pair, and on any of a group of four."""
    vol = volume(64)
    for rot, dist in (CAMERAS[2], CAMERAS[6], CAMERAS[7]):
        what = f"thr=0.05 lights={nl} rot={rot} dist={dist}"
        r = renderer(vol, nl, 64, rot, dist, thr=0.05)
        img = check_frame(monkeypatch, r, what)
        check_paths_taken(monkeypatch, r, img, what)
        r.delete()


def test_64_bit_kernels_share_the_shading(monkeypatch, counter_clock):
    """The 64-bit kernels (VR_FORCE_BIG=1) share shade_fast and the LUT fetch: the 64^3 frame equals
    the default's, at every depth-lane count."""
    vol = volume(64)
    for nl in (2, 1):
        for rot, dist in (CAMERAS[6], CAMERAS[4]):
            r = renderer(vol, nl, 64, rot, dist)
            for k in ("1", "2", "4"):
                base = render_with(monkeypatch, r, {"VR_DEPTH_LANES": k})
                big = render_with(monkeypatch, r, {"VR_DEPTH_LANES": k, "VR_FORCE_BIG": "1"})
                assert np.nanmax(base) > 0
                assert same(big, base), (nl, rot, k)
            r.delete()
