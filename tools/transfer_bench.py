#!/usr/bin/env python3
"""tools/transfer_bench.py [OUT.json] [--n N] [--res W H] [--frames F] [--repeats R] [--label L] -- time
of the transfer-function render (vr_render_transfer_device, vr_transfer.hip) on the metric frame:
V_shell(1024), 1920 x 1080, the ex1 camera (rotate(125,25,0), f 3, dist 6) and its two lights, a
parula-like colormap of 256 entries over [0, 1].

Timed, each over windows of F serial frames between two HIP events, R windows per variant, the
variants taken in turn within a repeat (so that a drift of the machine hits all alike):
  tf_lit, tf_unlit     -- value-coded colour, with the two lights and the HG LUT / without;
  tf_alpha             -- lit, with an alphamap of 256 entries, A(0) = 0 (so the leap stays legal);
  ..._noprobe          -- VR_TF_NO_PROBE=1: every sample fetched, no empty-space leap;
  render, render_exact -- for scale, 'render' of the same lit frame with the default fast shading
                          and with VR_EXACT_SHADE=1 (the arithmetic the transfer render uses);
  mip                  -- for scale, the maximum-intensity projection.
Per variant the median / min / max ms per frame, and once the counters (samples visited, fetched).
The planes with and without the leap are compared bit for bit.  A library built with another
VR_TF_BATCH or with VR_TF_TABLE_GLOBAL=1 (VR_LIB_PATH, an A/B build) gives that build's times from
the same script; --append merges the result into OUT.json under its label."""
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


def parula_like(n):
    """A smooth blue -> teal -> yellow map of n entries (not MATLAB's table)."""
    x = np.linspace(0.0, 1.0, n)
    r = np.clip(1.6 * x - 0.45, 0.05, 1.0) * (0.6 + 0.4 * x)
    g = np.clip(0.15 + 0.85 * x, 0.0, 1.0) ** 0.9
    b = np.clip(0.55 + 0.9 * x * (1 - 2.2 * x), 0.05, 1.0)
    return np.asfortranarray(np.stack([r, g, b], 1).astype(np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--res", type=int, nargs=2, default=[1920, 1080], metavar=("W", "H"))
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="default")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--no-scale", action="store_true", help="skip render / render_exact / mip")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "transfer_bench needs a GPU"
    mex.enable_test_switches()  # (VR_TF_NO_PROBE)
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
    cmap = parula_like(256)
    amap = np.linspace(0.0, 1.2, 256).astype(np.float32)
    tf_plain, keep3 = mex.transfer(cmap, (0, 1))
    tf_alpha, keep4 = mex.transfer(cmap, (0, 1), amap, (0, 1))
    out = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    aux = torch.zeros(W * H, dtype=torch.float32, device="cuda")
    steps = torch.zeros(48, dtype=torch.int64, device="cuda")
    s = torch.cuda.current_stream().cuda_stream

    def run(variant, d_steps=0):
        env = {}
        if variant.endswith("_noprobe"):
            env["VR_TF_NO_PROBE"] = "1"
        if variant == "render_exact":
            env["VR_EXACT_SHADE"] = "1"
        os.environ.update(env)
        try:
            if variant.startswith("render"):
                mex.render_device(h, ra_lit, out.data_ptr(), None, d_steps, s)
            elif variant == "mip":
                mex.render_projection_device(h, ra_unlit, "mip", out.data_ptr(), aux.data_ptr(), None, d_steps, s)
            else:
                base = variant.replace("_noprobe", "")
                ra = ra_unlit if base == "tf_unlit" else ra_lit
                mex.render_transfer_device(h, ra, tf_alpha if base == "tf_alpha" else tf_plain, out.data_ptr(),
                                           aux.data_ptr(), None, d_steps, s)
        finally:
            for k in env:
                os.environ.pop(k, None)

    tfv = ["tf_lit", "tf_unlit", "tf_alpha"]
    variants = tfv + [v + "_noprobe" for v in tfv] + ([] if a.no_scale else ["render", "render_exact", "mip"])
    res = {"config": "V_shell(%d), %dx%d, rotate(125,25,0) f=3 dist=6, factors 1/0.4/0.6, thr 0.9, 2 lights + HG(64), "
                     "256-entry colormap over [0, 1]; %d frames per window, %d windows" % (n, W, H, a.frames, a.repeats),
           "label": a.label, "lib": os.path.basename(vr._lib.LIB_PATH)}
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

    res["leap_bit_identical"] = {v: same(planes[v], planes[v + "_noprobe"]) for v in tfv}
    res["leap_speedup"] = {v: round(res[v + "_noprobe"]["ms_median"] / res[v]["ms_median"], 3) for v in tfv}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        allres = {}
        if a.append and os.path.exists(a.out):
            with open(a.out) as fh:
                allres = json.load(fh)
        if a.append:
            allres[a.label] = res
        else:
            allres = res
        with open(a.out, "w") as fh:
            json.dump(allres, fh, indent=1)
    vr.volumeRender("delete", h)
    del keep1, keep2, keep3, keep4


if __name__ == "__main__":
    main()
