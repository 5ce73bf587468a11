"""Round-12 GPU tests of the march's chunk set-up: the occupancy map asked about a chunk's box
before the box is staged (vr_stage.h box_bricks_empty), the box of rays that end inside a chunk, and
the staging copy over boxes of every row length -- each against a render that does not take the
path (staging without the map's word, no empty skip, no staging at all), bit for bit."""
import gc

import numpy as np
import pytest

import oracle as O

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("volume_renderer_amd")

CAMERAS = [(125, 25, 0), (0, 0, 0), (90, 0, 0), (30, 10, 0)]  # two axis-aligned: rays along brick faces
KEYS = ("VR_NO_LDS", "VR_NO_EMPTY_SKIP", "VR_NO_BRICK_TEST", "VR_DEPTH_LANES")


@pytest.fixture(autouse=True)
def _clean():
    gc.collect()
    yield
    gc.collect()


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def renderer(vol, res, rot=(125, 25, 0)):
    """examples/example1.m:32-58 on synthetic data: two lights, on-the-fly gradient."""
    r = vr.VolumeRender()
    r.VolumeIllumination = vr.Volume(vr.HenyeyGreenstein(64))
    r.LightSources = [vr.LightSource([500, 1000, 550], [0, 1, 1]), vr.LightSource([0, 550, 90], [1, 0.5, 1])]
    r.ElementSizeUm = [1, 1, 1]
    r.FocalLength = 3.0
    r.DistanceToObject = 6
    r.rotate(*rot)
    r.OpacityThreshold = 0.9
    r.ImageResolution = list(res)
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


def brick_volume(n, nan):
    """Mostly +-0, as tests/test_gpu_round6.py adversarial_volume builds it: single voxels on faces,
    edges and corners of the map's 8^3 bricks (padded index i + 1: voxel 7 opens brick 1, voxel 6
    closes brick 0), a -0 plane, a subnormal voxel, a thin slab two voxels from a brick boundary
    (voxel plane 41 = padded 42, bricks begin at padded 40) and, if asked, a NaN voxel -- so that
    empty chunk boxes touch occupied bricks and occupied boxes lie next to empty bricks."""
    v = np.zeros((n, n, n), np.float32, order="F")
    v[:, :, n // 3] = -0.0
    pts = {(7, n // 2, n // 2): 0.9, (n // 2, 15, n // 2 + 1): 0.8, (n // 2 - 3, n // 2 + 2, 23): 0.7,  # faces
           (15, 15, n // 2 - 5): 0.95,                                                                  # edge
           (23, 23, 23): 1.0, (6, 6, 6): 0.6, (31, 39, 47): 0.85, (39, 31, 7): 0.5,                     # corners
           (n - 1, n - 1, n - 1): 0.75, (0, 0, 0): 0.65, (0, n - 1, 7): 0.7,
           (n // 2 + 9, 12, n // 2 + 1): -0.7,
           (n // 2 - 11, n // 2 - 9, n // 2 + 7): 1e-39}                                                # subnormal
    for (x, y, z), val in pts.items():
        v[x, y, z] = np.float32(val)
    v[10:38, 12:36, 41] = np.float32(0.3)
    if nan:
        v[n // 2 + 5, n // 2 - 6, 9] = np.float32("nan")
    return v


def counted(r, res, env, monkeypatch):
    """The counter variant's launch of the renderer's current frame: its 48 counters."""
    import torch
    from volume_renderer_amd import mex
    W, H = res
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


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("n", [64, 72])
def test_box_brick_test_is_exact_and_exercised(monkeypatch, counter_clock, n, nan):
    """A chunk whose box touches only +-0 bricks is leaped without being staged.  On volumes that are
    empty but for voxels on brick faces, edges and corners, a -0 plane, a subnormal voxel, a thin slab
    next to a brick boundary (and, in the `nan` flavour, a NaN voxel), under four cameras, the default
    render equals the render that stages every chunk (VR_NO_BRICK_TEST=1) and the render without the
    empty skip (VR_NO_EMPTY_SKIP=1), bit for bit, at every depth-lane count of the default build.
    The counted launch of the same frames leaps chunks on the map's word (steps[46] > 0), and the
    chunks it stages plus those equal the chunks the switched-off run stages.
    A volume with a NaN voxel is not a tame launch: its march checks every coordinate and has no
    probe and no box-brick test (vr_march.hip PROBE), so its frames count steps[46] == 0 by design;
    the bit identity with the switch and the chunk-count identity are asserted for it all the same.
    Against VR_NO_EMPTY_SKIP=1 that flavour is equal only outside the pixels which the unskipped
    render makes NaN (see the comment at the assertion: a property of the empty-sample skip, not of
    the chunk set-up), and a NaN pixel's sign and payload are not compared across kernels."""
    res = (96, 64)
    vol = vr.Volume(brick_volume(n, nan))
    asked = 0
    for rot in CAMERAS:
        r = renderer(vol, res, rot)
        for k in ("1", "2", "4"):
            base = render_with(monkeypatch, r, {"VR_DEPTH_LANES": k})
            assert np.nanmax(base) > 0
            off = render_with(monkeypatch, r, {"VR_DEPTH_LANES": k, "VR_NO_BRICK_TEST": "1"})
            noskip = render_with(monkeypatch, r, {"VR_DEPTH_LANES": k, "VR_NO_EMPTY_SKIP": "1"})
            assert np.array_equal(bits(off), bits(base)), (rot, k, "staged without the map's word")
            if nan:
                # (the empty-sample skip itself is not exact next to a NaN voxel, before this round as
                # after it: a +-0 sample whose gradient taps touch the NaN has a NaN shading term,
                # which VR_NO_EMPTY_SKIP=1 multiplies by its zero opacity and adds.  Such a pixel is
                # NaN without the skip; every other pixel is equal bit for bit.)
                assert not (np.isnan(base) & ~np.isnan(noskip)).any(), (rot, k, "no empty skip, NaN set")
                assert np.array_equal(bits(noskip)[~np.isnan(noskip)], bits(base)[~np.isnan(noskip)]), (rot, k)
            else:
                assert np.array_equal(bits(noskip), bits(base)), (rot, k, "no empty skip")
        on, img_on = counted(r, res, {}, monkeypatch)
        sw, img_sw = counted(r, res, {"VR_NO_BRICK_TEST": "1"}, monkeypatch)
        print(f"n={n} nan={nan} rot={rot}: staged {on[2]} leaped {on[3]} (unstaged {on[46]}) fall {on[4]}; "
              f"switched off: staged {sw[2]} leaped {sw[3]} fall {sw[4]}")
        assert np.array_equal(bits(img_on), bits(img_sw))
        flat = np.asarray(base, np.float32).reshape(-1, order="F")
        if nan:  # (the counter kernel's NaN pixels are the render's; a NaN's sign and payload are not pinned)
            assert np.array_equal(np.isnan(img_on), np.isnan(flat))
            assert np.array_equal(bits(img_on)[~np.isnan(flat)], bits(flat)[~np.isnan(flat)])
        else:
            assert np.array_equal(bits(img_on), bits(flat))
        assert sw[46] == 0
        # steps[2]: chunks staged and sampled, [3]: chunks leaped (staged all-zero, or unstaged: [46])
        staged_on = on[2] + on[3] - on[46]  # chunks copied into the slot
        assert staged_on + on[46] == sw[2] + sw[3]
        assert on[2] == sw[2] and on[3] == sw[3] and on[4] == sw[4] and on[0] == sw[0]
        assert on[46] <= on[3]
        asked += int(on[46])
        if not nan:
            assert on[46] > 0, rot
        r.delete()
    assert (asked > 0) == (not nan)


def shaped_volume(dims):
    """V_shell cut to dims (the shell's wall crosses the box faces of a non-cube)."""
    m = max(dims)
    return np.asfortranarray(O.shell_volume(m)[:dims[0], :dims[1], :dims[2]])


@pytest.mark.parametrize("dims", [(16, 16, 16), (24, 24, 24), (40, 56, 72)])
def test_rays_that_end_inside_a_chunk(monkeypatch, counter_clock, dims):
    """Chords shorter than a chunk (16^3, 24^3: fewer than 32 samples across) and box faces hit at
    grazing angles: the chunk's box is planned from each ray's remaining samples, (tfar - t) / tstep
    with tstep = 1 / (2.2 * the shortest face diagonal), never a power of two.  A box that missed a tap
    of a whole chunk would change a pixel: the staged render equals the unstaged one (VR_NO_LDS=1, the
    plain kernel, which plans no box), bit for bit, at every depth-lane count."""
    vol = vr.Volume(shaped_volume(dims))
    for rot in [(125, 25, 0), (0, 0, 0), (30, 10, 0), (90, 89, 0)]:
        r = renderer(vol, (64, 64), rot)
        plain = render_with(monkeypatch, r, {"VR_NO_LDS": "1"})
        assert plain.max() > 0
        for k in ("1", "2", "4"):
            staged = render_with(monkeypatch, r, {"VR_DEPTH_LANES": k})
            assert np.array_equal(bits(staged), bits(plain)), (rot, k)
        r.delete()


@pytest.mark.parametrize("rot", [(125, 25, 0), (0, 0, 0), (90, 0, 0)])
def test_staging_copy_over_box_shapes(monkeypatch, counter_clock, rot):
    """The staging copy moves 64 / ex whole rows per wave pass: boxes with ex * ey below, equal to and
    above 64, odd extents, and boxes one plane thick at a volume face all occur in the 40x56x72
    volume under an oblique and two axis-aligned cameras, at image sizes that make the tiles' footprints
    narrow and wide.  Staged equals unstaged, bit for bit, with the narrow and the wide wave slot."""
    vol = vr.Volume(shaped_volume((40, 56, 72)))
    for res in [(64, 64), (200, 24), (24, 200)]:
        r = renderer(vol, res, rot)
        plain = render_with(monkeypatch, r, {"VR_NO_LDS": "1"})
        assert plain.max() > 0
        for k in ("1", "2", "4"):
            for wide in ("0", "1"):
                monkeypatch.setenv("VR_WIDE_SLOT", wide)
                staged = render_with(monkeypatch, r, {"VR_DEPTH_LANES": k})
                monkeypatch.delenv("VR_WIDE_SLOT")
                assert np.array_equal(bits(staged), bits(plain)), (res, k, wide)
        r.delete()
