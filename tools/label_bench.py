#!/usr/bin/env python3
"""Label-gain timing (include/vrhip.h vr_set_label_gains), run once on the GPU box.

Frame: the metric frame (V_shell(1024), 1920 x 1080, two lights); labels = the half-space mask of
examples/example4.m (label 1 where i1 >= d1 / 2); the gain of label 1 is swept per frame.  One handle,
the variants interleaved in one process: windows of --frames frames, --windows windows per variant, each
figure ms per frame as median (min-max) over the windows:

  (i)   gains        vr_set_label_gains alone (the label pass, its statistics, the occupancy rebuild);
  (ii)  gains+render vr_set_label_gains, then 'render' into device memory;
  (iii) sync+render  the way without the feature: 'sync_volumes' of a host-rewritten volume (two
                     prepared host volumes alternate, as tools/upload_bench.py's movie), then 'render';
                     in fp32 and in uint8;
  (iv)  render       'render' alone.

Also recorded: the bytes the label pass and the occupancy rebuild move, and their share of an 8 TB/s roof
at the median of (i).
usage: python tools/label_bench.py [--n 1024 --width 1920 --height 1080 --frames 5 --windows 7 --out profiles/round16/labels.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def stat(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round16", "labels.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    import volume_renderer_amd as vr
    from volume_renderer_amd import mex
    from bench import rotation

    n, W, H = args.n, args.width, args.height
    t = torch.empty(n * n * n, dtype=torch.float32, device="cuda")
    mex.synth_shell_device(t.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    shape = (n, n, n)
    base = t.cpu().numpy().reshape(shape, order="F")
    base_u8 = (t * 255).round().to(torch.uint8).cpu().numpy().reshape(shape, order="F")
    del t
    labels = np.zeros(shape, np.uint8, order="F")
    labels[:, n // 2:, :] = 1
    # the host-rewritten volumes of variant (iii): the mask times two factors, alternating per frame
    rewritten = []
    rewritten_u8 = []
    for f in (0.75, 0.5):
        a = np.array(base, order="F")
        a[:, n // 2:, :] *= np.float32(f)
        rewritten.append(vr.Volume(a))
        b = np.array(base_u8, order="F")
        b[:, n // 2:, :] = (b[:, n // 2:, :] * f).astype(np.uint8)
        rewritten_u8.append(vr.RawVolume(b))
    em = vr.Volume(base)
    refl = vr.Volume(1)
    lut = vr.Volume(vr.HenyeyGreenstein(64))
    lights = [vr.LightSource([500, 1000, 550], [0, 1, 1]), vr.LightSource([0, 550, 90], [1, 0.5, 1])]
    R = rotation(125, 25, 0)

    def argv(scale):
        return (lights, lut, np.float32([1.0 * scale, 0.4, 0.6 * scale]), np.float32([1, 1, 1]), np.uint64([H, W]),
                np.flip(R, 0).astype(np.float32), np.float32([0, 3.0, 6.0]), np.float32(0.9), np.float32([1, 1, 0]))

    ra, keep = mex.render_args(*argv(1.0))
    ra8, keep8 = mex.render_args(*argv(1.0 / 255.0))
    out = torch.empty(3 * W * H, dtype=torch.float32, device="cuda")
    stream = torch.cuda.Stream()
    h = vr.volumeRender("new")
    sweep = [0.9, 0.7, 0.5, 0.3, 0.1, 0.0, 0.2, 0.4, 0.6, 0.8]
    state = {"k": 0}

    def next_gain():
        state["k"] += 1
        return np.float32([1.0, sweep[state["k"] % len(sweep)]])

    def labelled():  # the handle holds the unmodified volume and the labels
        mex.set_label_gains(h, None)
        em.touch()
        vr.volumeRender("sync_volumes", h, np.uint64(1), em, refl, em)
        mex.sync_labels(h, labels)
        mex.set_label_gains(h, next_gain())

    def render(r=ra):
        mex.render_device(h, r, out.data_ptr(), None, 0, stream.cuda_stream)

    def resync(vols, r):
        def frame(k):
            v = vols[k % 2]
            v.touch()
            vr.volumeRender("sync_volumes", h, np.uint64(1), v, refl, v)
            render(r)
        return frame

    variants = {
        "gains": (labelled, lambda k: mex.set_label_gains(h, next_gain())),
        "gains+render": (labelled, lambda k: (mex.set_label_gains(h, next_gain()), render())),
        "sync+render fp32": (lambda: mex.set_label_gains(h, None), resync(rewritten, ra)),
        "sync+render uint8": (lambda: mex.set_label_gains(h, None), resync(rewritten_u8, ra8)),
        "render": (labelled, lambda k: render()),
    }
    times = {k: [] for k in variants}
    for w in range(args.windows + 1):  # window 0 warms up (allocations, schedules)
        for name, (prepare, frame) in variants.items():
            prepare()
            frame(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for k in range(1, args.frames + 1):
                frame(k)
            torch.cuda.synchronize()
            if w:
                times[name].append((time.perf_counter() - t0) * 1e3 / args.frames)
    vr.volumeRender("delete", h)
    del keep, keep8

    padded = (n + 2) ** 3
    pass_bytes = padded * 8 + n ** 3  # the unmodified row read, the modulated row written, one label byte per voxel
    occ_bytes = padded * 4            # the occupancy rebuild reads the modulated buffer again
    res = {"volume": n, "image": [W, H], "frames_per_window": args.frames, "windows": args.windows,
           "ms_per_frame": {k: stat(v) for k, v in times.items()},
           "label_pass_bytes": pass_bytes, "occupancy_rebuild_bytes": occ_bytes}
    med = res["ms_per_frame"]["gains"]["median"] * 1e-3
    res["gains_GBps"] = round((pass_bytes + occ_bytes) / med / 1e9, 1)
    res["gains_share_of_8TBps"] = round((pass_bytes + occ_bytes) / med / 8e12, 3)
    a, b = res["ms_per_frame"]["gains+render"], res["ms_per_frame"]
    res["gains+render_below_sync+render_disjoint"] = {k: bool(a["max"] < b[k]["min"])
                                                      for k in ("sync+render fp32", "sync+render uint8")}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
