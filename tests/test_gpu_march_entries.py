"""GPU test of the host's march entry table (vr_launch.h MarchEntries, vr_frame.hip march_entries): every
(shading variant, depth lanes) the host can ask for goes through each entry of the object that serves it
-- launch and blocks (render, fused stereo pair), launch_views (the fused pair of renderChannels) and
launch_slab (a two-slab sort-last chain) -- and gives the bits of the same variant at one depth lane.
The 40 x 24 image is ragged against the 16 x 16 block of every K, so a wrong tile shape or block count
in a row of the table shows."""
import gc

import numpy as np
import pytest

import oracle as O
import test_gpu_parity as parity

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("volume_renderer_amd")

W, H = 40, 24
LIGHTS = ([500, 1000, 550], [0, 1, 1]), ([0, 550, 90], [1, 0.5, 1])
_results = {}  # (shade, lanes) -> the images below, rendered once


def _render_all(shade, lanes):
    """render, the fused stereo pair (vr_render_stereo and renderChannels) and a two-slab chain of the
    24^3 shell with two lights and an HG LUT of 16, under VR_EXACT_SHADE / VR_DEPTH_LANES."""
    from volume_renderer_amd import mex
    key = (shade, lanes)
    if key in _results:
        return _results[key]
    gc.collect()
    with pytest.MonkeyPatch.context() as mp:
        mp.setenv("VR_DEPTH_LANES", str(lanes))
        if shade == "exact":
            mp.setenv("VR_EXACT_SHADE", "1")
        else:
            mp.delenv("VR_EXACT_SHADE", raising=False)
        data = O.shell_volume(24)
        lut = vr.Volume(vr.HenyeyGreenstein(16))
        r = parity.ex1_renderer(vr.Volume(data), res=(W, H))
        r.VolumeIllumination = lut
        out = {"render": np.asarray(r.render(), np.float32), "kernel": mex.last_march_kernel()}
        r.CameraXOffset = 0.5
        out["stereo"] = np.asarray(r.render(), np.float32)
        out["views"] = np.asarray(vr.VolumeRender.renderChannels([r])[0], np.float32)
        r.CameraXOffset = 0
        lights = [vr.LightSource(*l) for l in LIGHTS]
        ra_args = (np.float32([1.0, 0.4, 0.6]), np.float32([1, 1, 1]), np.uint64([H, W]),
                   np.flip(r.RotationMatrix, 0).astype(np.float32), np.float32([0, 3.0, 6.0]), np.float32(0.9),
                   np.float32([1, 1, 0]))
        out["slabs"], st = parity._slab_chain(data, [1, 1, 1], [-np.inf, 11, np.inf], lights, lut, ra_args, W, H)
        out["unfinished"] = bool(st[4].any())
        r.delete()
    gc.collect()
    _results[key] = out
    return out


@pytest.mark.parametrize("lanes", [1, 2, 4])
@pytest.mark.parametrize("shade", ["fast", "exact"])
def test_every_march_entry_gives_the_one_lane_image(counter_clock, shade, lanes):
    ref = _render_all(shade, 1)
    got = _render_all(shade, lanes)
    # the object that served the render: the exact variant is built for K = 1, 2 only (exact_lanes)
    k = lanes if shade == "fast" else min(lanes, 2)
    assert got["kernel"].startswith(f"vr::{shade}::march_kernel<{k}, "), got["kernel"]
    assert not got["unfinished"]  # every ray of the chain finished
    for what in ("render", "stereo", "views", "slabs"):
        assert ref[what].max() > 0, what
        assert got[what].shape == ref[what].shape, what
        assert np.array_equal(got[what].view(np.uint32), ref[what].view(np.uint32)), (what, shade, lanes)
