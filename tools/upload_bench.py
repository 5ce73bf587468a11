#!/usr/bin/env python3
"""Typed-volume upload timing (include/vrhip.h vr_dtype), run once on the GPU box:

  * 'sync_volumes' of a changed 1024^3 HOST volume of each element type (fp32 included): the call's
    wall time, and its copy and pad parts as the library reports them with VR_UPLOAD_TIMING=1
    ("copies": when the last H2D copy had landed, "total": when the last pad had ended; pad = total -
    copies, the whole volume crosses in one copy).  Each typed copy part is put next to
    bytes / (the fp32 link rate of the same run);
  * the changing-data movie of tools/e2e_bench.py (1920 x 1080, each frame's upload overlapping the
    previous frame's render) in fp32 and in uint8: ms per frame by the host clock and by a pair of
    HIP events on the render stream.

Every figure is per upload (per frame), the median of --reps (at least 5) with min and max.
usage: python tools/upload_bench.py [--n 1024 --width 1920 --height 1080 --reps 7 --out profiles/round7/typed_upload.json]"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

LINE = re.compile(r"VR_UPLOAD_TIMING bytes (\d+) copies ([0-9.]+) ms total ([0-9.]+) ms")


class StderrCapture:
    """The library prints its VR_UPLOAD_TIMING line to the C stderr: fd 2 into a file meanwhile."""

    def __enter__(self):
        self.tmp = tempfile.TemporaryFile(mode="w+b")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.tmp.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.tmp.seek(0)
        self.text = self.tmp.read().decode(errors="replace")
        self.tmp.close()


def stat(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def typed_hosts(n):
    """V_shell(n) (values in [0, 1]) on the host as fp32 and quantised to each narrow type."""
    from volume_renderer_amd import mex
    t = torch.empty(n * n * n, dtype=torch.float32, device="cuda")
    mex.synth_shell_device(t.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    shape = (n, n, n)
    hosts = {"float32": t.cpu().numpy().reshape(shape, order="F")}
    hosts["uint8"] = (t * 255).round().to(torch.uint8).cpu().numpy().reshape(shape, order="F")
    q16 = (t * 32767).round().to(torch.int16)
    hosts["int16"] = q16.cpu().numpy().reshape(shape, order="F")
    hosts["uint16"] = (q16.cpu().numpy().astype(np.uint16) * np.uint16(2)).reshape(shape, order="F")
    hosts["float16"] = t.to(torch.float16).cpu().numpy().reshape(shape, order="F")
    del t, q16
    torch.cuda.synchronize()
    return hosts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round7", "typed_upload.json"))
    args = ap.parse_args()
    assert args.reps >= 5
    torch.cuda.set_device(0)
    import volume_renderer_amd as vr
    from volume_renderer_amd import mex
    mex.enable_test_switches()
    from bench import rotation

    n, W, H = args.n, args.width, args.height
    hosts = typed_hosts(n)
    refl = vr.Volume(1)
    out = {"volume": n, "image": [W, H], "reps": args.reps, "uploads": {}, "movie": {}}

    def volume_of(name, unorm=False):
        return vr.Volume(hosts[name]) if name == "float32" else vr.RawVolume(hosts[name], unorm)

    # ---- the upload of each element type ---------------------------------------------------------
    forms = [("float32", False), ("uint8", False), ("uint8", True), ("uint16", False), ("uint16", True),
             ("int16", False), ("float16", False)]
    os.environ["VR_UPLOAD_TIMING"] = "1"  # (read per upload)
    for name, unorm in forms:
        v = volume_of(name, unorm)
        h = vr.volumeRender("new")
        wall, copy, pad, nbytes = [], [], [], 0
        for rep in range(args.reps + 1):
            v.touch()
            with StderrCapture() as cap:
                t0 = time.perf_counter()
                vr.volumeRender("sync_volumes", h, np.uint64(1), v, refl, v)
                t1 = time.perf_counter()
            lines = LINE.findall(cap.text)  # one per uploaded volume: the emission volume is the large one
            assert lines, cap.text
            if rep == 0:
                continue  # warm-up: allocations
            m = max(lines, key=lambda g: int(g[0]))
            nbytes = int(m[0])
            wall.append((t1 - t0) * 1e3)
            copy.append(float(m[1]))
            pad.append(float(m[2]) - float(m[1]))
        vr.volumeRender("delete", h)
        key = name + ("_unorm" if unorm else "")
        out["uploads"][key] = {"bytes": nbytes, "sync_ms": stat(wall), "copy_ms": stat(copy), "pad_ms": stat(pad)}
        print(key, json.dumps(out["uploads"][key]), flush=True)
        del v
    os.environ["VR_UPLOAD_TIMING"] = "0"
    f = out["uploads"]["float32"]
    rate = f["bytes"] / (f["copy_ms"]["median"] * 1e-3)  # the link rate of this run, B/s
    out["fp32_link_GBps"] = round(rate / 1e9, 2)
    for key, u in out["uploads"].items():
        u["copy_ms_at_fp32_link_rate"] = round(u["bytes"] / rate * 1e3, 3)
        u["pad_not_longer_than_fp32"] = bool(u["pad_ms"]["median"] <= f["pad_ms"]["median"])

    # ---- the changing-data movie, fp32 and uint8 -------------------------------------------------
    lut = vr.Volume(vr.HenyeyGreenstein(64))
    lights = [vr.LightSource([500, 1000, 550], [0, 1, 1]), vr.LightSource([0, 550, 90], [1, 0.5, 1])]
    R = rotation(125, 25, 0)
    for name in ("float32", "uint8"):
        scale = 1.0 if name == "float32" else 1.0 / 255.0
        argv = (lights, lut, np.float32([1.0 * scale, 0.4, 0.6 * scale]), np.float32([1, 1, 1]), np.uint64([H, W]),
                np.flip(R, 0).astype(np.float32), np.float32([0, 3.0, 6.0]), np.float32(0.9), np.float32([1, 1, 0]))
        second = hosts[name] * np.float32(0.9) if name == "float32" else (hosts[name] // 10 * 9).astype(np.uint8)
        vols = [volume_of(name), vr.Volume(second) if name == "float32" else vr.RawVolume(second)]
        h = vr.volumeRender("new")
        ra, keep = mex.render_args(*argv)
        outs = [torch.empty(3 * W * H, dtype=torch.float32, device="cuda") for _ in range(2)]
        stream = torch.cuda.Stream()

        def frame(k):
            v = vols[k % 2]
            v.touch()
            vr.volumeRender("sync_volumes", h, np.uint64(1), v, refl, v)
            mex.render_device(h, ra, outs[k % 2].data_ptr(), None, 0, stream.cuda_stream)

        wall, evms = [], []
        for rep in range(args.reps + 1):
            frame(0)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            t0 = time.perf_counter()
            for k in range(1, args.frames + 1):
                frame(k)
            e1.record(stream)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            if rep:
                wall.append((t1 - t0) * 1e3 / args.frames)
                evms.append(e0.elapsed_time(e1) / args.frames)
        # a render alone (no upload beside it): what bounds the movie once the link does not
        alone = []
        for rep in range(args.reps + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mex.render_device(h, ra, outs[0].data_ptr(), None, 0, stream.cuda_stream)
            torch.cuda.synchronize()
            if rep:
                alone.append((time.perf_counter() - t0) * 1e3)
        vr.volumeRender("delete", h)
        out["movie"][name] = {"frames": args.frames, "ms_per_frame": stat(wall), "ms_per_frame_hip_events": stat(evms),
                              "render_alone_ms": stat(alone), "upload_bytes_per_frame": int(hosts[name].nbytes)}
        print("movie", name, json.dumps(out["movie"][name]), flush=True)
        del vols, keep

    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
