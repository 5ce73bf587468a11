#!/usr/bin/env python3
"""Gaussian smoothing timing and a correctness check at size (include/vrhip.h vr_set_smoothing; DESIGN.md
s19), run once on the GPU box.

Volumes: V_shell(n) and a uniform-random n^3 volume, n = 1024.  Sigmas: isotropic 1, 2 and 6, and (1, 1, 0).
Two kernel forms: `passes` (one launch per axis) and `fused` (one launch, a z march with a ring of planes in
LDS; three active axes only).  One handle per volume, everything -- both forms included -- interleaved in
one process, each figure ms as median (min-max) over --repeats repeats after one warm-up:

  set_smoothing   one vr_set_smoothing with the form forced (VR_SMOOTH_FORM): device events on the null
                  stream around the synchronous call, and of that call the library's own host-clock
                  times of its two synchronised parts: the filter launches with the statistics read-back,
                  and the occupancy rebuild;
  launches        the same kernels alone between two padded device buffers (device events), without and
                  with the statistics folded in -- their difference is the statistics' cost, reported as
                  below resolution when it is inside the spread; the passes also per axis.

Yardsticks, measured in the same run:
  label gains     vr_set_label_gains on the same handle: a one-read one-write stream of the same buffer
                  plus the same statistics and occupancy rebuild;
  sync            'sync_volumes' of the host-filtered volume, the way without the feature;
  conv3d          (--conv3d-only, a run of its own) a separable torch.nn.functional.conv3d.

Bytes are computed from shapes: a pass reads and writes the padded volume once; the fused launch reads
each input plane's tile with its x and y halo ((FY + 2Ry)(FX + 2Rx) / (FY FX) of the volume, part of it
from the caches) and re-reads 2Rz planes per z chunk, and writes the volume once.  Shares are of an
8 TB/s roof; that HBM bandwidth is the bound is an assumption the small shares do not show.

Correctness at size: 32^3 blocks of the handle's resident buffer (read back after vr_set_smoothing, under
each form) at corners, faces, the centre and across the plane where the padded buffer passes 2^31 bytes (a
padded 1026^3 volume has fewer than 2^31 elements; 2^32 bytes fall inside the last corner blocks) against
tests/smooth_ref.py of the input block plus its halo, bit for bit.
usage: python tools/smooth_bench.py [--n 1024 --repeats 5 --out profiles/round22/smooth.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

F = np.float32
SIGMAS = {"1": (1, 1, 1), "2": (2, 2, 2), "6": (6, 6, 6), "1,1,0": (1, 1, 0)}
FX, FY, FZ = 64, 16, 256  # csrc/vr_smooth.hip


def stat(xs):
    return {"median": round(float(np.median(xs)), 3), "min": round(float(min(xs)), 3), "max": round(float(max(xs)), 3)}


def difference(with_, without):
    """Median difference, or 'below resolution' when it lies inside either spread."""
    d = float(np.median(with_) - np.median(without))
    spread = max(max(with_) - min(with_), max(without) - min(without))
    return round(d, 3) if abs(d) > spread else f"below resolution ({d:.3f} ms inside a spread of {spread:.3f} ms)"


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def block_origins(n, b):
    lo, mid, hi = 0, (n - b) // 2, n - b
    o = [(x, y, z) for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)]
    o += [(lo, mid, mid), (hi, mid, mid), (mid, lo, mid), (mid, hi, mid), (mid, mid, lo), (mid, mid, hi), (mid, mid, mid)]
    k = 2 ** 31 // ((n + 2) * (n + 2) * 4) - 1  # interior plane whose padded plane holds byte 2^31
    if b // 2 <= k < n - b // 2:
        o.append((mid, mid, min(max(k - b // 2, 0), hi)))
    return o


def check_blocks(mex, SR, h, base, sigma, n, b=32):
    """Blocks of the handle's resident buffer against smooth_ref of the input block plus its halo."""
    R = [int(np.ceil(2 * s)) if s > 0 else 0 for s in sigma]
    px = n + 2
    bad, blocks = 0, []
    for (x, y, z) in block_origins(n, b):
        lo = [max(c - r, 0) for c, r in zip((x, y, z), R)]
        hi = [min(c + b + r, n) for c, r in zip((x, y, z), R)]
        ref = SR.smooth(base[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], sigma, weights_of=mex.smooth_weights_host)
        ref = ref[x - lo[0]:x - lo[0] + b, y - lo[1]:y - lo[1] + b, z - lo[2]:z - lo[2] + b]
        got = np.empty((b, b, b), F)
        for k in range(b):  # the b padded rows y+1 .. y+b of padded plane z+k+1, in one read
            rows = mex.read_emission(h, ((z + k + 1) * px + (y + 1)) * px, b * px).reshape(b, px)
            got[:, :, k] = rows[:, x + 1:x + 1 + b].T
        same = np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
        bad += not same
        blocks.append({"origin": [x, y, z], "equal": bool(same)})
    return {"blocks": len(blocks), "differing": int(bad), "detail": blocks}


def conv3d_only(args, res, save, mex):
    n = args.n
    for vname in ("shell", "random"):
        t = torch.empty(n * n * n, dtype=torch.float32, device="cuda")
        if vname == "shell":
            mex.synth_shell_device(t.data_ptr(), n, torch.cuda.current_stream().cuda_stream)
        else:
            t.copy_(torch.rand(n * n * n, generator=torch.Generator(device="cuda").manual_seed(22), device="cuda"))
        vol = t.view(1, 1, n, n, n)
        out = res["volumes"].setdefault(vname, {})
        out["conv3d_ms"] = {}
        for k in ("1", "6"):
            try:
                ws = []
                for j in range(3):
                    Rj, w = mex.smooth_weights_host(SIGMAS[k][j])
                    kshape = [1, 1, 1, 1, 1]
                    kshape[4 - j] = 2 * Rj + 1  # tensor dims [N, C, z, y, x]: dims[j] of Data is tensor dim 4 - j
                    ws.append((Rj, j, torch.from_numpy(w).cuda().view(kshape)))

                def conv():
                    x = vol
                    for Rj, j, w in ws:
                        p = [0] * 6
                        p[2 * j], p[2 * j + 1] = Rj, Rj  # F.pad counts from the last dim: x, y, z
                        x = torch.nn.functional.conv3d(torch.nn.functional.pad(x, p, mode="replicate"), w)
                    return x

                conv()
                out["conv3d_ms"][k] = stat([timed(conv) for _ in range(3)])
            except Exception as e:  # noqa: BLE001  (recorded: the yardstick could not be taken)
                out["conv3d_ms"][k] = "not measured: " + str(e)[:200]
            save()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--conv3d-only", action="store_true", help="add the conv3d yardstick to an existing --out file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round22", "smooth.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    import volume_renderer_amd as vr
    from volume_renderer_amd import mex
    import smooth_ref as SR

    n = args.n
    shape = (n, n, n)
    padded = (n + 2) ** 3
    res = {"volume": n, "repeats": args.repeats, "padded_bytes": padded * 4, "volumes": {}}
    if args.conv3d_only and os.path.exists(args.out):
        with open(args.out) as fh:
            res = json.load(fh)

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    if args.conv3d_only:
        conv3d_only(args, res, save, mex)
        print(json.dumps(res), flush=True)
        return

    mex.enable_test_switches()
    refl = vr.Volume(1)
    stream = torch.cuda.current_stream().cuda_stream
    for vname in ("shell", "random"):
        t = torch.empty(n * n * n, dtype=torch.float32, device="cuda")
        if vname == "shell":
            mex.synth_shell_device(t.data_ptr(), n, stream)
        else:
            t.copy_(torch.rand(n * n * n, generator=torch.Generator(device="cuda").manual_seed(22), device="cuda"))
        torch.cuda.synchronize()
        base = t.cpu().numpy().reshape(shape, order="F")
        # the padded twin for the launches alone: [z][y][x] with x fastest, edge-replicated; only read
        pad = torch.nn.functional.pad(t.view(1, 1, n, n, n), (1, 1, 1, 1, 1, 1), mode="replicate").contiguous().view(-1)
        del t
        other, third = torch.empty_like(pad), torch.empty_like(pad)
        d_stats = torch.zeros(2, dtype=torch.int32, device="cuda")
        out = res["volumes"].setdefault(vname, {})
        out["sigma"] = {}
        wts = {}
        for k, sg in SIGMAS.items():
            buf = np.zeros(75, F)
            radius = []
            for j in range(3):
                Rj, w = mex.smooth_weights_host(sg[j])
                buf[25 * j:25 * j + w.size] = w
                radius.append(Rj)
            wts[k] = (radius, torch.from_numpy(buf).cuda())

        def run_passes(k, with_stats, only=None):
            radius, w = wts[k]
            active = [j for j in range(3) if radius[j]]
            a, b2 = pad, other
            for j in (active if only is None else [only]):
                st = d_stats.data_ptr() if (with_stats and j == active[-1]) else 0
                mex.smooth_axis_device(a.data_ptr(), b2.data_ptr(), shape, j, w.data_ptr() + 100 * j, radius[j], st, stream)
                a, b2 = b2, (third if a is pad else a)

        def run_fused(k, with_stats):
            radius, w = wts[k]
            mex.smooth_fused_device(pad.data_ptr(), other.data_ptr(), shape, w.data_ptr(), radius,
                                    d_stats.data_ptr() if with_stats else 0, stream)

        em = vr.Volume(base)
        h = vr.volumeRender("new")
        vr.volumeRender("sync_volumes", h, np.uint64(0), em, refl, em)
        labels = np.zeros(shape, np.uint8, order="F")
        labels[:, n // 2:, :] = 1
        mex.sync_labels(h, labels)
        del labels

        forms_of = {k: (("passes", "fused") if all(s > 0 for s in sg) else ("passes",)) for k, sg in SIGMAS.items()}
        T = {k: {f: {"call": [], "filter_host": [], "occupancy_host": [], "launch": [], "launch_stats": []}
                 for f in forms_of[k]} for k in SIGMAS}
        per_axis = {k: {0: [], 1: [], 2: []} for k in SIGMAS}
        gains_ms = []
        for rep in range(args.repeats + 1):  # repeat 0 warms up
            for k, sg in SIGMAS.items():
                for form in forms_of[k]:
                    os.environ["VR_SMOOTH_FORM"] = form
                    mex.set_smoothing(h, None)
                    call = timed(lambda: mex.set_smoothing(h, F(sg)))
                    parts = mex.derive_times(h)
                    run = (lambda s: run_fused(k, s)) if form == "fused" else (lambda s: run_passes(k, s))
                    l0, l1 = timed(lambda: run(False)), timed(lambda: run(True))
                    if rep:
                        for key, v in (("call", call), ("filter_host", parts[0]), ("occupancy_host", parts[1]),
                                       ("launch", l0), ("launch_stats", l1)):
                            T[k][form][key].append(v)
                for j in range(3):
                    if wts[k][0][j]:
                        v = timed(lambda: run_passes(k, False, only=j))
                        if rep:
                            per_axis[k][j].append(v)
            os.environ.pop("VR_SMOOTH_FORM", None)
            mex.set_smoothing(h, None)
            mex.set_label_gains(h, None)
            gv = timed(lambda: mex.set_label_gains(h, F([1, 0.5 + 0.01 * rep])))
            mex.set_label_gains(h, None)
            if rep:
                gains_ms.append(gv)
        for k, sg in SIGMAS.items():
            radius = wts[k][0]
            npass = sum(1 for s in sg if s > 0)
            o = {"pass_ms_by_axis": {str(j): stat(v) for j, v in per_axis[k].items() if v}, "forms": {}}
            for form in forms_of[k]:
                tf = T[k][form]
                if form == "passes":
                    byts = npass * padded * 8
                else:
                    amp = (FY + 2 * radius[1]) * (FX + 2 * radius[0]) / (FY * FX) * (FZ + 2 * radius[2]) / FZ
                    byts = int(padded * 4 * (amp + 1))
                med = float(np.median(tf["launch_stats"])) * 1e-3
                o["forms"][form] = {
                    "set_smoothing_ms": stat(tf["call"]), "of_it_filter_and_statistics_read_back_ms_host": stat(tf["filter_host"]),
                    "of_it_occupancy_rebuild_ms_host": stat(tf["occupancy_host"]),
                    "launches_ms": stat(tf["launch"]), "launches_with_statistics_ms": stat(tf["launch_stats"]),
                    "statistics_ms": difference(tf["launch_stats"], tf["launch"]),
                    "bytes_from_shapes": byts, "GBps": round(byts / med / 1e9, 1),
                    "share_of_8TBps": round(byts / med / 8e12, 3),
                    "share_of_8TBps_at_floor_bytes": round(padded * 8 / med / 8e12, 3),
                    "bound": "HBM bandwidth (assumed, not shown by these shares)"}
            if len(forms_of[k]) == 2:
                a, b2 = T[k]["passes"]["call"], T[k]["fused"]["call"]
                o["fused_over_passes_call"] = round(float(np.median(b2) / np.median(a)), 3)
                o["disjoint"] = bool(max(a) < min(b2) or max(b2) < min(a))
            out["sigma"][k] = o
        out["label_gains_ms"] = stat(gains_ms)
        out["label_gain_pass_bytes"] = padded * 8 + n ** 3
        out["floor_bytes_one_read_one_write"] = padded * 8
        save()

        out["correctness"] = {}
        for k in ("6", "1"):
            for form in ("fused", "passes"):
                os.environ["VR_SMOOTH_FORM"] = form
                mex.set_smoothing(h, None)
                mex.set_smoothing(h, F(SIGMAS[k]))
                out["correctness"][k + " " + form] = c = check_blocks(mex, SR, h, base, SIGMAS[k], n)
                print(vname, "sigma", k, form, "blocks differing:", c["differing"], "of", c["blocks"], flush=True)
        os.environ.pop("VR_SMOOTH_FORM", None)
        save()
        # the host-filtered volume (sigma 1) for the sync yardstick: the resident buffer, read back
        px = n + 2
        filt = np.empty(shape, F, order="F")
        for z in range(n):
            filt[:, :, z] = mex.read_emission(h, (z + 1) * px * px, px * px).reshape(px, px)[1:-1, 1:-1].T
        mex.set_smoothing(h, None)
        fv = [vr.Volume(filt), vr.Volume(np.array(filt, order="F"))]
        sync_ms = []
        for rep in range(args.repeats + 1):
            v = fv[rep % 2]
            v.touch()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vr.volumeRender("sync_volumes", h, np.uint64(1), v, refl, v)
            torch.cuda.synchronize()
            if rep:
                sync_ms.append((time.perf_counter() - t0) * 1e3)
        out["sync_of_host_filtered_ms_host"] = stat(sync_ms)
        del fv, filt, pad, other, third, base, em
        vr.volumeRender("delete", h)
        torch.cuda.empty_cache()
        save()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
