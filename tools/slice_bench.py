#!/usr/bin/env python3
"""tools/slice_bench.py [OUT.json] [--n N] [--res R] [--frames F] [--repeats R] [--label L] -- time of the
slice views (vr_render_slice_device, vr_slice.hip) on V_shell(1024): R x R slices (default 1024) along
each axis (axis2t: the axis-2 slice transposed, its columns along dims[0]) and an oblique plane through
the centre, thickness 1 (max) and 32 (max and sum), each with
VR_SLICE_LANES=x, =y and unset (the host's rule).

Timed as tools/projection_bench.py does: windows of F serial calls between two HIP events, R windows per
variant, the variants taken in turn within a repeat (a drift of the machine hits all alike).  Per variant
the median / min / max ms per call; the cache lines (128 B) a wave touches per row load, counted on the
host from the addresses of a sample of waves (the honest unit of a gather's cost), and the line requests
they add up to (lines x 128 B x 4 row loads x samples x waves; neighbouring waves ask for the same lines
again, so most are served by the caches); the bytes the slice needs -- its distinct lines, counted on a
128 x 128 block, plus the planes stored -- and that traffic as a fraction of the 8 TB/s roof.
For scale, the MIP of the metric frame (1920 x 1080, the ex1 camera) from the same run.  A library built
with another VR_SLICE_BATCH (VR_LIB_PATH, an A/B build) gives the unbatched loop's times from the same
script; both sides of a lane axis are compared bit for bit."""
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

ROOF = 8.0e12  # bytes / s


def geometry(s):
    return [np.array(list(v), np.float64) for v in (s.origin, s.du, s.dv, s.dw)]


def lines_per_wave(s, dims, lanes_x, waves=192):
    """Mean number of distinct 128-byte lines one row load of a wave touches (8 bytes per lane), over a
    sample of waves and the slab's samples, from the kernel's address computation in double."""
    o, du, dv, dw = geometry(s)
    H, W, n = int(s.resolution[0]), int(s.resolution[1]), int(s.samples)
    d = np.array(dims, np.float64)
    px, pxy = dims[0] + 2, (dims[0] + 2) * (dims[1] + 2)
    la, lo = (W, H) if lanes_x else (H, W)
    nla = (la + 63) // 64
    total = nla * lo
    rng = np.random.default_rng(1)
    counts = []
    for wv in rng.choice(total, size=min(waves, total), replace=False):
        a = (wv % nla) * 64 + np.arange(64)
        b = np.full(64, wv // nla)
        x, y = (a, b) if lanes_x else (b, a)
        ok = (x < W) & (y < H)
        for k in sorted({0, n // 2, n - 1}):
            q = o[None, :] + du[None, :] * x[:, None] + dv[None, :] * y[:, None] + dw[None, :] * k
            ins = ok & np.all((q >= 0) & (q <= 1), axis=1)
            if not ins.any():
                continue
            i = np.clip(np.floor(q * d[None, :] - 0.5), -1, d[None, :] - 1).astype(np.int64) + 1
            base = i[:, 2] * pxy + i[:, 1] * px + i[:, 0]
            for off in (0, px, pxy, pxy + px):
                f = (base + off)[ins]
                counts.append(len(set((f * 4) // 128) | set((f * 4 + 4) // 128)))
    return float(np.mean(counts)) if counts else 0.0


def rule_lanes_x(s, dims, planes):
    """The host's lane-axis rule (vr_features.hip slice_lanes_x), restated."""
    _, du, dv, _ = geometry(s)
    d = np.array(dims, np.float64)

    def lines(step):
        a = np.abs(step * d)
        return min(64.0, 1.0 + 63.0 * min(1.0, a[1] + a[2]) + 63.0 * a[0] / 32.0)

    loads = 4.0 * s.samples
    return loads * lines(du) + 4.0 * 64.0 * planes < loads * lines(dv) + 4.0 * 2.0 * planes


def footprint_lines(s, dims, block=128):
    """Distinct 128-byte lines the whole slice reads -- the traffic it needs from HBM at least -- counted
    on a block x block corner of the image over every slab sample and scaled to the image."""
    o, du, dv, dw = geometry(s)
    H, W, n = int(s.resolution[0]), int(s.resolution[1]), int(s.samples)
    d = np.array(dims, np.float64)
    px, pxy = dims[0] + 2, (dims[0] + 2) * (dims[1] + 2)
    bh, bw = min(block, H), min(block, W)
    y, x = np.meshgrid(np.arange(bh) + (H - bh) // 2, np.arange(bw) + (W - bw) // 2, indexing="ij")
    seen = []
    for k in range(n):
        q = (o[None, None, :] + du[None, None, :] * x[:, :, None] + dv[None, None, :] * y[:, :, None] + dw[None, None, :] * k)
        ins = np.all((q >= 0) & (q <= 1), axis=2)
        i = np.clip(np.floor(q * d - 0.5), -1, d - 1).astype(np.int64) + 1
        base = (i[:, :, 2] * pxy + i[:, :, 1] * px + i[:, :, 0])[ins]
        for off in (0, px, pxy, pxy + px):
            seen.append(np.unique(np.concatenate([(base + off) * 4 // 128, ((base + off) * 4 + 4) // 128])))
    if not seen:
        return 0.0
    return float(np.unique(np.concatenate(seen)).size) * (H * W) / (bh * bw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "slice_bench needs a GPU"
    mex.enable_test_switches()  # (VR_SLICE_LANES)
    n, R = a.n, a.res
    t = torch.empty(n ** 3, dtype=torch.float32, device="cuda")
    mex.synth_shell_device(t.data_ptr(), n)
    torch.cuda.synchronize()
    em = mex.DeviceVolume(t.data_ptr(), (n, n, n), last_update=20, owner=t)
    refl = vr.Volume(1)
    refl.TimeLastUpdate = np.uint64(5)
    h = vr.volumeRender("new")
    vr.volumeRender("sync_volumes", h, np.uint64(0), em, refl, em)
    del t
    dims = (n, n, n)
    out = torch.zeros(2 * R * R, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def slice_of(geom, thick, mode):
        if geom.startswith("axis"):
            s = mex.slice_axis(dims, int(geom[4]), (n - 1) / 2, thick)
            # R x R pixels over the same plane (R = n: one pixel per voxel, the helper's own geometry)
            for j in range(3):
                s.origin[j] = s.origin[j] if s.du[j] == 0 and s.dv[j] == 0 else 0.5 / R
                s.du[j] *= n / R
                s.dv[j] *= n / R
            s.resolution[0] = s.resolution[1] = R
        else:
            s = mex.slice_oblique(dims, [1, 1, 1], [0.5, 0.5, 0.5], [1, 0.7, 0.4], [0, 0, 1], n / R, R, R, thick)
        if geom.endswith("t"):  # transposed: columns along the slice's first dimension, rows along the second
            for j in range(3):
                s.du[j], s.dv[j] = s.dv[j], s.du[j]
        s.mode = mex.slice_mode(mode)
        return s

    variants = {}
    for geom in ("axis0", "axis1", "axis2", "axis2t", "oblique"):
        for thick, mode in ((1, "max"), (32, "max"), (32, "sum")):
            for lanes in ("x", "y", "auto"):
                variants[f"{geom}_n{thick}_{mode}_{lanes}"] = (slice_of(geom, thick, mode), lanes)

    def run(name):
        s, lanes = variants[name]
        if lanes != "auto":
            os.environ["VR_SLICE_LANES"] = lanes
        try:
            mex.render_slice_device(h, s, out.data_ptr(), out.data_ptr() + 4 * R * R, 0, st)
        finally:
            os.environ.pop("VR_SLICE_LANES", None)

    Rm = np.flip(O.rotation(125, 25, 0), 0).astype(np.float32)
    ra, keep = mex.render_args(False, False, np.float32([1, 0.4, 0.6]), np.float32([1, 1, 1]), np.uint64([1080, 1920]), Rm,
                               np.float32([0, 3, 6]), np.float32(1.0), np.float32([1, 1, 0]))
    mip_out = torch.zeros(4 * 1920 * 1080, dtype=torch.float32, device="cuda")

    def run_mip():
        mex.render_projection_device(h, ra, "mip", mip_out.data_ptr(), mip_out.data_ptr() + 12 * 1920 * 1080, None, 0, st)

    res = {"config": "V_shell(%d), %d x %d slices, image + aux planes; %d calls per window, %d windows"
                     % (n, R, R, a.frames, a.repeats), "label": a.label, "lib": os.path.basename(vr._lib.LIB_PATH)}
    planes, ms = {}, {v: [] for v in list(variants) + ["mip_metric_frame"]}
    for v in variants:  # warm-up and the planes
        run(v)
        run(v)
        torch.cuda.synchronize()
        planes[v] = out.cpu().numpy().copy()
    run_mip()
    torch.cuda.synchronize()
    for _ in range(a.repeats):
        for v in ms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.frames):
                run(v) if v in variants else run_mip()
            e1.record()
            torch.cuda.synchronize()
            ms[v].append(e0.elapsed_time(e1) / a.frames)
    same, foot = {}, {}
    for v, (s, lanes) in variants.items():
        lx = rule_lanes_x(s, dims, 2) if lanes == "auto" else lanes == "x"
        lpw = lines_per_wave(s, dims, lx)
        waves = ((R + 63) // 64) * R
        requested = lpw * 128 * 4 * s.samples * waves  # line requests of the loads, however they are served
        base = v.rsplit("_", 1)[0]
        if base not in foot:
            foot[base] = footprint_lines(s, dims) * 128 + 2 * R * R * 4
        med = float(np.median(ms[v]))
        res[v] = {"lanes": "x" if lx else "y", "ms_median": round(med, 4), "ms_min": round(min(ms[v]), 4),
                  "ms_max": round(max(ms[v]), 4), "lines_per_wave_per_row_load": round(lpw, 2),
                  "mbytes_requested_in_lines": round(requested / 1e6, 2),
                  "mbytes_needed": round(foot[base] / 1e6, 2),
                  "fraction_of_roof": round(foot[base] / (med * 1e-3) / ROOF, 4)}
        print(v, json.dumps(res[v]), flush=True)
        same[base] = same.get(base, True) and bool(np.array_equal(planes[v].view(np.uint32), planes[base + "_x"].view(np.uint32)))
    v = "mip_metric_frame"
    res[v] = {"ms_median": round(float(np.median(ms[v])), 3), "ms_min": round(min(ms[v]), 3), "ms_max": round(max(ms[v]), 3)}
    print(v, json.dumps(res[v]), flush=True)
    res["lanes_bit_identical"] = same
    # the rule's verdict per geometry: is the forced other side's range wholly above the chosen side's?
    verdict = {}
    for base in same:
        chosen = res[base + "_auto"]["lanes"]
        other = "y" if chosen == "x" else "x"
        verdict[base] = {"chosen": chosen, "chosen_range": [res[f"{base}_{chosen}"]["ms_min"], res[f"{base}_{chosen}"]["ms_max"]],
                         "other_range": [res[f"{base}_{other}"]["ms_min"], res[f"{base}_{other}"]["ms_max"]],
                         "other_wholly_above": res[f"{base}_{other}"]["ms_min"] > res[f"{base}_{chosen}"]["ms_max"]}
    res["lane_rule"] = verdict
    print(json.dumps({"lanes_bit_identical": same, "lane_rule": verdict}))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
    vr.volumeRender("delete", h)
    del keep


if __name__ == "__main__":
    main()
