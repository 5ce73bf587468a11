#!/usr/bin/env python3
"""tools/projection_bench.py [OUT.json] [--n N] [--res W H] [--frames F] [--repeats R] -- time of the
projection renders (vr_render_projection_device, vr_project.hip) on the metric frame: V_shell(1024),
1920 x 1080, the ex1 camera (rotate(125,25,0), f 3, dist 6).

Timed, each over windows of F serial frames between two HIP events, R windows per variant, the
variants taken in turn within a repeat (so that a drift of the machine hits all alike):
  mip, sum             -- the default launch (empty-space leap through the occupancy map);
  mip_noprobe, sum_... -- VR_PROJ_NO_PROBE=1: every sample fetched;
  render_ea            -- for scale, the existing 'render' of the same frame with no lights, Fa 0.6 and
                          an opacity threshold of 1 (never reached: the same samples).
Per variant the median / min / max ms per frame, and once the counters (samples visited, fetched).
The images with and without the probe are compared bit for bit.  A library built with another
VR_PROJ_BATCH (VR_LIB_PATH, an A/B build) gives the unbatched loop's times from the same script."""
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
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "projection_bench needs a GPU"
    mex.enable_test_switches()  # (VR_PROJ_NO_PROBE)
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
    ra, keep = mex.render_args(False, False, np.float32([1, 0.4, 0.6]), np.float32([1, 1, 1]), np.uint64([H, W]), R,
                               np.float32([0, 3, 6]), np.float32(1.0), np.float32([1, 1, 0]))
    out = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    aux = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    steps = torch.zeros(48, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def run(variant, d_steps=0):
        if variant == "render_ea":
            mex.render_device(h, ra, out.data_ptr(), None, d_steps, s)
            return
        mode, _, np_ = variant.partition("_")
        if np_:
            os.environ["VR_PROJ_NO_PROBE"] = "1"
        try:
            mex.render_projection_device(h, ra, mode, out.data_ptr(), aux.data_ptr(), None, d_steps, s)
        finally:
            os.environ.pop("VR_PROJ_NO_PROBE", None)

    variants = ["mip", "mip_noprobe", "sum", "sum_noprobe", "render_ea"]
    res = {"config": "V_shell(%d), %dx%d, rotate(125,25,0) f=3 dist=6, Fe 1, no lights; %d frames per window, %d windows"
                     % (n, W, H, a.frames, a.repeats), "label": a.label, "lib": os.path.basename(vr._lib.LIB_PATH)}
    planes, ms = {}, {v: [] for v in variants}
    for v in variants:  # warm-up, the planes and the counters
        for _ in range(2):
            run(v)
        torch.cuda.synchronize()
        planes[v] = (out.cpu().numpy().copy(), aux.cpu().numpy().copy())
        steps.zero_()
        run(v, steps.data_ptr())
        torch.cuda.synchronize()
        c = steps.cpu().numpy()
        res[v] = {"samples_visited": int(c[0]), "samples_fetched_or_shaded": int(c[1])}
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

    def same(p, q):
        return bool(all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(p, q)))

    res["probe_bit_identical"] = {m: same(planes[m], planes[m + "_noprobe"]) for m in ("mip", "sum")}
    res["probe_speedup"] = {m: round(res[m + "_noprobe"]["ms_median"] / res[m]["ms_median"], 3) for m in ("mip", "sum")}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    vr.volumeRender("delete", h)
    del keep


if __name__ == "__main__":
    main()
