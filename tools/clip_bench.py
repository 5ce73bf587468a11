#!/usr/bin/env python3
"""tools/clip_bench.py [OUT.json] [--n N] [--res W H] [--frames F] [--repeats R] -- what clip planes
(vr_set_clip, csrc/vr_clip.h) cost and save on the metric frame: V_shell(1024), 1920 x 1080, the ex1
camera (rotate(125,25,0), f 3, dist 6) and its two lights.

Timed, each over windows of F serial frames between two HIP events, R windows per variant, the
variants taken in turn within a repeat (so that a drift of the machine hits all alike):
  render               -- no planes: the LDS-staged march, as every frame before this feature;
  render_nolds         -- no planes, VR_NO_LDS=1: the general one-lane kernel the clipped render is built from;
  render_keepall       -- one plane that contains the whole box: the clipped general kernel doing the
                          unclipped frame's work (should sit within run-to-run spread of render_nolds);
  render_plane1        -- one oblique plane through the centre (normal 0.6, -0.3, 0.74);
  render_crop6         -- six planes, the crop box 0.25 <= q <= 0.75 on every axis (the central half);
  mip / iso / tf       -- the maximum-intensity projection, the isosurface (level 0.3, lit) and the unlit
                          transfer render (256-entry colormap), each with no planes, _keepall, _plane1
                          and _crop6.
Per variant the median / min / max ms per frame and once the counters: samples visited (d_steps[0])
and d_steps[1] (render: samples shaded; the others: samples fetched, i.e. not leaped).
Nothing is asserted: the numbers go to OUT.json (profiles/round14/clip.json) and DESIGN.md."""
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
from transfer_bench import parula_like  # noqa: E402

PLANE_SETS = {
    "": None,
    "_keepall": np.float32([[0.6, -0.3, 0.74, 100.0]]),
    "_plane1": np.float32([[0.6, -0.3, 0.74, -0.52]]),
    "_crop6": np.float32([[1, 0, 0, -0.25], [-1, 0, 0, 0.75], [0, 1, 0, -0.25], [0, -1, 0, 0.75], [0, 0, 1, -0.25],
                          [0, 0, -1, 0.75]]),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--res", type=int, nargs=2, default=[1920, 1080], metavar=("W", "H"))
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "clip_bench needs a GPU"
    mex.enable_test_switches()  # (VR_NO_LDS)
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
    lights = [vr.LightSource([500, 1000, 550], [0, 1, 1]), vr.LightSource([0, 550, 90], [1, 0.5, 1])]
    lut = vr.Volume(vr.HenyeyGreenstein(64))
    lut.TimeLastUpdate = np.uint64(7)
    frame = [np.float32([1, 0.4, 0.6]), np.float32([1, 1, 1]), np.uint64([H, W]), R, np.float32([0, 3, 6]),
             np.float32(0.9), np.float32([1, 1, 0])]
    ra_lit, keep1 = mex.render_args(lights, lut, *frame)
    # (an empty light list, not the logical false: false keeps the lights of the last lit call, as 'render' does)
    ra_unlit, keep2 = mex.render_args([], lut, *frame)
    tf, keep3 = mex.transfer(parula_like(256), (0, 1))
    out = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    aux = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    steps = torch.zeros(48, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def run(variant, d_steps=0):
        kind = variant.split("_")[0]
        env = {"VR_NO_LDS": "1"} if variant == "render_nolds" else {}
        os.environ.update(env)
        try:
            if kind == "render":
                mex.render_device(h, ra_lit, out.data_ptr(), None, d_steps, s)
            elif kind == "mip":
                mex.render_projection_device(h, ra_unlit, "mip", out.data_ptr(), aux.data_ptr(), None, d_steps, s)
            elif kind == "iso":
                mex.render_isosurface_device(h, ra_lit, 0.3, out.data_ptr(), aux.data_ptr(), 0, None, d_steps, s)
            else:
                mex.render_transfer_device(h, ra_unlit, tf, out.data_ptr(), aux.data_ptr(), None, d_steps, s)
        finally:
            for k in env:
                os.environ.pop(k, None)

    def planes_of(variant):
        suffix = variant[variant.index("_"):] if "_" in variant else ""
        return PLANE_SETS.get(suffix)  # (render_nolds: none)

    variants = ["render", "render_nolds", "render_keepall", "render_plane1", "render_crop6"]
    variants += [k + sfx for k in ("mip", "iso", "tf") for sfx in ("", "_keepall", "_plane1", "_crop6")]
    res = {"config": "V_shell(%d), %dx%d, rotate(125,25,0) f=3 dist=6, factors 1/0.4/0.6, thr 0.9, 2 lights + HG(64); "
                     "%d frames per window, %d windows" % (n, W, H, a.frames, a.repeats),
           "lib": os.path.basename(vr._lib.LIB_PATH),
           "planes": {k.lstrip("_"): v.tolist() for k, v in PLANE_SETS.items() if v is not None}}
    ms = {v: [] for v in variants}
    for v in variants:  # warm-up and the counters
        mex.set_clip(h, planes_of(v))
        for _ in range(2):
            run(v)
        steps.zero_()
        run(v, steps.data_ptr())
        torch.cuda.synchronize()
        c = steps.cpu().numpy()
        res[v] = {"samples_visited": int(c[0]), "samples_fetched_or_shaded": int(c[1])}
    for _ in range(a.repeats):
        for v in variants:
            mex.set_clip(h, planes_of(v))
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
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    mex.set_clip(h, None)
    vr.volumeRender("delete", h)
    del keep1, keep2, keep3


if __name__ == "__main__":
    main()
