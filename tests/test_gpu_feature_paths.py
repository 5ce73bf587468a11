"""GPU tests of what the feature renders share on the host and in the kernels (vr_capi.hip ensure_out,
vr_raycast.h): one handle's output buffer grown and reused across every host-pointer render, and the step
counters of the three one-lane kernels on an image so small that whole waves have no pixel.

The column partitions of the three features and their probed / unprobed counters on full images are in
test_gpu_projection.py, test_gpu_isosurface.py and test_gpu_transfer.py (the partitioned ... assembles and
empty_space_leap tests)."""
import numpy as np
import pytest

import oracle as O
from golden_cases import EX1_LIGHTS, STAMP_LUT

vr = pytest.importorskip("volume_renderer_amd")
from volume_renderer_amd import mex  # noqa: E402
from test_gpu_isosurface import gpu_iso  # noqa: E402
from test_gpu_projection import BLOCK_ARGS, block_volume, gpu_project  # noqa: E402
from test_gpu_slice import V, gpu_slice, new_handle  # noqa: E402
from test_gpu_transfer import TF_VALUE, gpu_transfer, tail  # noqa: E402
import slice_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint32),
                                                                          np.ascontiguousarray(y).view(np.uint32))
                                    for x, y in zip(a, b))


# ---- 1. the handle's output buffer across the host-pointer renders -----------------------------------------

def test_one_output_buffer_serves_every_host_render_in_turn():
    """'render' (3 planes), the isosurface with depth and normal (7), the projection with aux (4), a slice
    with aux and labels at another resolution (3), the transfer render with alpha (4) and 'render' again on
    one handle: each call's planes are those of the same call on a fresh handle, bit for bit."""
    em = np.asfortranarray(np.random.default_rng(18).random((24, 20, 16), dtype=F))
    labels = np.asfortranarray(np.random.default_rng(9).integers(0, 4, em.shape, dtype=np.uint8))
    lights = [vr.LightSource(l[:3], l[3:]) for l in EX1_LIGHTS]
    lut = V(vr.HenyeyGreenstein(32), STAMP_LUT)
    argv = [lights, lut, F([1, 0.4, 0.6]), F([1, 1, 1]), np.uint64([24, 40]), np.flip(O.rotation(125, 25, 0), 0).astype(F),
            F([0, 3, 6]), F(0.9), F([1, 0.5, 0.25])]
    s = SR.Slice.of(mex.slice_oblique(list(em.shape), [1, 1, 1], [0.5, 0.5, 0.5], [0.3, -0.5, 1], [1, 0.2, 0],
                                      16 / 90, 23, 37, 5))

    def as_tuple(x):
        return x if isinstance(x, tuple) else (x,)

    calls = [("render", lambda h: vr.volumeRender("render", h, *argv)),
             ("isosurface", lambda h: vr.volumeRender("render_isosurface", h, *argv, F(0.6))),
             ("projection", lambda h: vr.volumeRender("render_projection", h, *argv, "mip")),
             ("slice", lambda h: gpu_slice(h, s, "sum")),
             ("transfer", lambda h: vr.volumeRender("render_transfer", h, *argv, *tail(TF_VALUE))),
             ("render again", lambda h: vr.volumeRender("render", h, *argv))]

    def handle():
        h = new_handle(em)
        mex.sync_labels(h, labels)
        return h

    want = []
    for _, fn in calls:  # each on a handle of its own
        h = handle()
        want.append(as_tuple(fn(h)))
        vr.volumeRender("delete", h)
    assert [len(w) for w in want] == [1, 3, 2, 3, 2, 1]
    assert want[0][0].max() > 0 and np.isfinite(want[1][1]).any()
    assert np.isfinite(want[3][2]).any() and want[4][1].max() > 0
    h = handle()
    for (name, fn), w in zip(calls, want):
        assert same_bits(as_tuple(fn(h)), w), name
    vr.volumeRender("delete", h)


# ---- 2. counters on an image with waves that have no pixel ---------------------------------------------------

TINY_ARGS = BLOCK_ARGS[:2] + [np.uint64([5, 9])] + BLOCK_ARGS[3:]  # 9 x 5: waves 2 and 3 of the one tile are idle


@pytest.mark.parametrize("feature", ["projection", "isosurface", "transfer"])
def test_counters_on_a_tiny_image_with_and_without_the_probe(feature, monkeypatch):
    """The probed and the unprobed launch visit the same samples and write the same planes; the probed one
    fetches no more.  The volume is the leap tests' (the smallest with an occupancy map)."""
    argv = [False, False] + TINY_ARGS
    run, switch = {"projection": (lambda h: gpu_project(h, argv, "sum", count=True), "VR_PROJ_NO_PROBE"),
                   "isosurface": (lambda h: gpu_iso(h, argv, 0.05, count=True), "VR_ISO_NO_PROBE"),
                   "transfer": (lambda h: gpu_transfer(h, argv, TF_VALUE, count=True), "VR_TF_NO_PROBE")}[feature]
    h = new_handle(block_volume(False))
    monkeypatch.delenv(switch, raising=False)
    leap = run(h)
    monkeypatch.setenv(switch, "1")
    plain = run(h)
    monkeypatch.delenv(switch)
    vr.volumeRender("delete", h)
    print(feature, "probed", leap[-1], "unprobed", plain[-1])
    assert same_bits(leap[:-1], plain[:-1])
    assert leap[-1][0] == plain[-1][0] > 0
    assert plain[-1][1] == plain[-1][0]  # every visited sample fetched
    assert leap[-1][1] <= plain[-1][1]
    assert leap[-1][2:] == plain[-1][2:]  # (the isosurface's surface pixels)
