#!/usr/bin/env python3
"""Volume histogram timing (include/vrhip.h vr_volume_histogram_device), run once on the GPU box.

Two resident volumes of n^3 voxels -- V_shell(n), which is mostly exact zeros, and a uniform-random one in
[0, 1), which has no coherence -- each in three configurations:

  plain     256 bins over [0, 1];
  by_label  16 labels x 256 bins (17 rows), the labels a mask split into 16 slabs along dimension 1;
  clip      plain with one oblique clip plane.

Every configuration is run with the kernel's wave-uniform shortcut (VR_HIST_UNIFORM=1) and with plain LDS
atomics (VR_HIST_UNIFORM=0): the contention A/B of DESIGN.md s18.  For scale, torch.histc (256 bins, the
same limits) on the same device tensor: the yardstick, not the code under test.  All variants of a volume
are interleaved, --repeats times (the library's default is plain LDS atomics); each figure is the ms of one call (device events around --calls calls on
one stream, counts only -- no finalize launch) as median (min-max) over the repeats.  Also recorded: the
bytes a call reads and their share of an 8 TB/s roof at the median.
usage: python tools/histogram_bench.py [--n 1024 --calls 5 --repeats 9 --out profiles/round21/histogram.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def stat(xs):
    return {"median": round(float(np.median(xs)), 4), "min": round(float(min(xs)), 4), "max": round(float(max(xs)), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round21", "histogram.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    import volume_renderer_amd as vr
    from volume_renderer_amd import _lib, mex
    mex.enable_test_switches()

    n = args.n
    stream = torch.cuda.Stream()
    shell = torch.empty(n * n * n, dtype=torch.float32, device="cuda")
    mex.synth_shell_device(shell.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
    rand = torch.rand(n * n * n, dtype=torch.float32, device="cuda", generator=torch.Generator("cuda").manual_seed(21))
    # labels[i0, i1, i2] = i1 * 16 // n (column-major: i1 is the middle index of the (i2, i1, i0) tensor)
    lab = (torch.arange(n, device="cuda") * 16 // n).to(torch.uint8).view(1, n, 1).expand(n, n, n).contiguous()
    torch.cuda.synchronize()
    zero_share = float((shell == 0).float().mean())
    h = vr.volumeRender("new")
    mex.sync_labels(h, mex.DeviceVolume(lab.data_ptr(), (n, n, n), owner=lab, dtype=_lib.VR_U8))
    refl = vr.Volume(1)
    d_counts = torch.zeros(17 * 256, dtype=torch.int64, device="cuda")
    lim = np.float32([0, 1])
    queries = {"plain": mex.make_histogram("emission", 256, lim),
               "by_label": mex.make_histogram("emission", 256, lim, np.int32([0, 16])),
               "clip": mex.make_histogram("emission", 256, lim, None, 1)}
    mex.set_clip(h, np.float32([[0.6, -0.3, 0.8, -0.35]]))
    voxels = n ** 3
    bytes_read = {"plain": 4 * voxels, "by_label": 5 * voxels, "clip": 4 * voxels}

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            fn()  # warm
            a.record(stream)
            for _ in range(args.calls):
                fn()
            b.record(stream)
        b.synchronize()
        return a.elapsed_time(b) / args.calls

    def hist(q, uniform):
        def fn():
            os.environ["VR_HIST_UNIFORM"] = "1" if uniform else "0"
            mex.volume_histogram_device(h, q, d_counts.data_ptr(), 0, stream.cuda_stream)
        return fn

    res = {"volume": n, "calls_per_figure": args.calls, "repeats": args.repeats, "bins": 256,
           "shell_zero_share": round(zero_share, 4), "bytes_read": bytes_read, "volumes": {}}
    for vname, t in (("shell", shell), ("uniform_random", rand)):
        em = mex.DeviceVolume(t.data_ptr(), (n, n, n), owner=t)
        vr.volumeRender("sync_volumes", h, np.uint64(0), em, refl, em)
        variants = {f"{c} {'uniform' if u else 'atomics'}": hist(q, u) for c, q in queries.items() for u in (True, False)}
        variants["torch.histc"] = lambda: torch.histc(t, bins=256, min=0.0, max=1.0)
        times = {k: [] for k in variants}
        for r in range(args.repeats + 1):  # repeat 0 warms up
            for k, fn in variants.items():
                ms = timed(fn)
                if r:
                    times[k].append(ms)
        os.environ.pop("VR_HIST_UNIFORM", None)
        # the counts of the last call of each kind agree with torch's where they are comparable
        mex.volume_histogram_device(h, queries["plain"], d_counts.data_ptr(), 0, stream.cuda_stream)
        stream.synchronize()
        ours = d_counts[:256].cpu().numpy()
        theirs = torch.histc(t, bins=256, min=0.0, max=1.0).cpu().numpy().astype(np.int64)
        out = {"ms": {k: stat(v) for k, v in times.items()},
               "counts_total": int(ours.sum()), "bins_differing_from_torch_histc": int((ours != theirs).sum())}
        for c in queries:
            for side in ("uniform", "atomics"):
                med = out["ms"][f"{c} {side}"]["median"] * 1e-3
                out.setdefault("GBps", {})[f"{c} {side}"] = round(bytes_read[c] / med / 1e9, 1)
                out.setdefault("share_of_8TBps", {})[f"{c} {side}"] = round(bytes_read[c] / med / 8e12, 3)
        res["volumes"][vname] = out
    vr.volumeRender("delete", h)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
