#!/usr/bin/env python3
"""tools/isosurface_bench.py [OUT.json] [--n N] [--res W H] [--level L] [--frames F] [--repeats R] --
time of the first-hit isosurface render (vr_render_isosurface_device, vr_isosurface.hip) on the metric
frame: V_shell(1024), 1920 x 1080, the ex1 camera (rotate(125,25,0), f 3, dist 6), the two ex1 lights
through HenyeyGreenstein(64), level 0.3.

Timed, each over windows of F serial frames between two HIP events, R windows per variant, the
variants taken in turn within a repeat (so that a drift of the machine hits all alike):
  iso          -- the default launch (empty-space leap through the occupancy map), all planes written;
  iso_noprobe  -- VR_ISO_NO_PROBE=1: every search sample fetched;
  render, mip  -- for scale: the existing 'render' (the same lights, Fa 0.6, threshold 0.9) and the
                  maximum-intensity projection of the same frame.
Per variant the median / min / max ms per frame, and once the counters.  The planes with and without
the probe are compared bit for bit.  A library built with another VR_ISO_BATCH (VR_LIB_PATH, an A/B
build) gives that batch size's times from the same script (--label names it in the output)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import volume_renderer_amd as vr  # noqa: E402
from volume_renderer_amd import mex  # noqa: E402
import oracle as O  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--res", type=int, nargs=2, default=[1920, 1080], metavar=("W", "H"))
    ap.add_argument("--level", type=float, default=0.3)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="")
    ap.add_argument("--only-iso", action="store_true", help="skip render and mip (an A/B build's run)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "isosurface_bench needs a GPU"
    mex.enable_test_switches()  # (VR_ISO_NO_PROBE)
    n, (W, H) = a.n, a.res
    t = torch.empty(n ** 3, dtype=torch.float32, device="cuda")
    mex.synth_shell_device(t.data_ptr(), n)
    torch.cuda.synchronize()
    em = mex.DeviceVolume(t.data_ptr(), (n, n, n), last_update=20, owner=t)
    refl = vr.Volume(1)
    refl.TimeLastUpdate = np.uint64(5)
    h = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", h, np.uint64(0), em, refl, em)
    del t
    R = np.flip(O.rotation(125, 25, 0), 0).astype(np.float32)
    lut = vr.Volume(vr.HenyeyGreenstein(64))
    lights = [vr.LightSource([500, 1000, 550], [0, 1, 1]), vr.LightSource([0, 550, 90], [1, 0.5, 1])]
    rest = [np.float32([1, 0.4, 0.6]), np.float32([1, 1, 1]), np.uint64([H, W]), R, np.float32([0, 3, 6]),
            np.float32(0.9), np.float32([1, 1, 0])]
    ra, keep = mex.render_args(lights, lut, *rest)
    out = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    depth = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    normal = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    steps = torch.zeros(48, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def run(variant, d_steps=0):
        if variant == "render":
            mex.render_device(h, ra, out.data_ptr(), None, d_steps, s)
        elif variant == "mip":
            mex.render_projection_device(h, ra, "mip", out.data_ptr(), depth.data_ptr(), None, d_steps, s)
        else:
            if variant == "iso_noprobe":
                os.environ["VR_ISO_NO_PROBE"] = "1"
            try:
                mex.render_isosurface_device(h, ra, a.level, out.data_ptr(), depth.data_ptr(), normal.data_ptr(), None,
                                             d_steps, s)
            finally:
                os.environ.pop("VR_ISO_NO_PROBE", None)

    variants = ["iso", "iso_noprobe"] + ([] if a.only_iso else ["render", "mip"])
    res = {"config": "V_shell(%d), %dx%d, rotate(125,25,0) f=3 dist=6, Fe 1 Fr 0.4, 2 lights HG(64), level %g; "
                     "%d frames per window, %d windows" % (n, W, H, a.level, a.frames, a.repeats),
           "label": a.label, "lib": os.path.basename(vr._lib.LIB_PATH)}
    planes, ms = {}, {v: [] for v in variants}
    for v in variants:  # warm-up, the planes and the counters
        for _ in range(2):
            run(v)
        torch.cuda.synchronize()
        planes[v] = (out.cpu().numpy().copy(), depth.cpu().numpy().copy(), normal.cpu().numpy().copy())
        steps.zero_()
        run(v, steps.data_ptr())
        torch.cuda.synchronize()
        c = steps.cpu().numpy()
        res[v] = {"samples_visited": int(c[0]), "samples_fetched_or_shaded": int(c[1])}
        if v.startswith("iso"):
            res[v]["surface_pixels"] = int(c[2])
    for _ in range(a.repeats):
        for v in variants:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.frames):
                run(v)
            e1.record()
            torch.cuda.synchronize()
            ms[v].append(e0.elapsed_time(e1) / a.frames)
    for v in variants:
        res[v].update(ms_median=round(float(np.median(ms[v])), 3), ms_min=round(min(ms[v]), 3),
                      ms_max=round(max(ms[v]), 3))
        print(v, json.dumps(res[v]), flush=True)
    res["probe_bit_identical"] = bool(all(np.array_equal(x.view(np.uint32), y.view(np.uint32))
                                          for x, y in zip(planes["iso"], planes["iso_noprobe"])))
    res["probe_speedup"] = round(res["iso_noprobe"]["ms_median"] / res["iso"]["ms_median"], 3)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    vr.volumeRender("delete", h)
    del keep


if __name__ == "__main__":
    main()
