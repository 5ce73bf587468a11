#!/usr/bin/env python3
"""Richardson-Lucy deconvolution timing and a correctness check at size (include/vrhip.h
vr_set_deconvolution), run once on the GPU box.

Volumes: V_shell(n) and a uniform-random n^3 volume, n = 1024.  PSF sigmas (1, 1, 2) and (2, 2, 5).  One
handle per volume, everything interleaved in one process, each figure ms as median (min-max) over --repeats
repeats after one warm-up:

  set_deconvolution  one vr_set_deconvolution at 1, 10 and 50 iterations (device events on the null stream
                     around the synchronous call; it includes the statistics read-back and the occupancy
                     rebuild, once per call), and the time per iteration from the slope between 10 and 50;
  fused iteration    one iteration k > 0 as the derivation launches it, between caller-owned padded
                     buffers: six filter passes, the third storing the ratio and the sixth the update
                     (vr_deconv_axis_device), the update writing the buffer it reads;
  unfused iteration  the same iteration from six plain passes (vr_smooth_axis_device) and the two
                     elementwise launches (vr_deconv_pointwise_device): what the epilogues are measured
                     against;
  smoothing          the yardstick: vr_set_smoothing of the same sigma on the same handle, the library's
                     host-clock time of its filter part, and its three passes alone (device events).

Reported: the time per iteration over two smoothing filter times (the three passes alone, twice), the
fused-over-unfused ratio, and the bytes moved, computed from shapes: a pass reads and writes the padded
volume once (8 bytes per padded voxel), an epilogue reads one more (4), an elementwise launch reads two and
writes one (12) -- 56 bytes per padded voxel and fused iteration, 72 unfused.  Shares are of an 8 TB/s
roof; that HBM bandwidth is the bound is an assumption the shares do not show.

Correctness at size: after 2 iterations at sigma (1, 1, 1), the 16 blocks of 32^3 voxels of the resident
buffer that tools/smooth_bench.py names (corners, faces, the centre and the plane where the padded buffer
passes 2^31 bytes) against tests/deconv_ref.py of the input block plus a halo of 2 * 2 * R = 8 voxels,
bit for bit.
usage: python tools/deconv_bench.py [--n 1024 --repeats 5 --out profiles/round23/deconv.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from smooth_bench import block_origins, stat, timed  # noqa: E402

F = np.float32
SIGMAS = {"1,1,2": (1, 1, 2), "2,2,5": (2, 2, 5)}
COUNTS = (1, 10, 50)
CHECK_SIGMA, CHECK_ITERATIONS = (1, 1, 1), 2


def check_blocks(mex, DR, h, base, n, b=32):
    """Blocks of the handle's resident buffer against deconv_ref of the input block plus its halo."""
    halo = 2 * CHECK_ITERATIONS * 2  # two blurs of radius R = 2 per iteration
    px = n + 2
    bad, blocks = 0, []
    for (x, y, z) in block_origins(n, b):
        lo = [max(c - halo, 0) for c in (x, y, z)]
        hi = [min(c + b + halo, n) for c in (x, y, z)]
        ref = DR.deconvolve(base[lo[0]:hi[0], lo[1]:hi[1], lo[2]:hi[2]], CHECK_SIGMA, CHECK_ITERATIONS,
                            weights_of=mex.smooth_weights_host)
        ref = ref[x - lo[0]:x - lo[0] + b, y - lo[1]:y - lo[1] + b, z - lo[2]:z - lo[2] + b]
        got = np.empty((b, b, b), F)
        for k in range(b):  # the b padded rows y+1 .. y+b of padded plane z+k+1, in one read
            rows = mex.read_emission(h, ((z + k + 1) * px + (y + 1)) * px, b * px).reshape(b, px)
            got[:, :, k] = rows[:, x + 1:x + 1 + b].T
        same = np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(ref).view(np.uint32))
        bad += not same
        blocks.append({"origin": [x, y, z], "equal": bool(same), "last_padded_byte": int((((z + b) * px + y + b) * px + x + b) * 4)})
    return {"blocks": len(blocks), "differing": int(bad), "detail": blocks}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "round23", "deconv.json"))
    args = ap.parse_args()
    torch.cuda.set_device(0)
    import volume_renderer_amd as vr
    from volume_renderer_amd import _lib, mex
    import deconv_ref as DR

    n = args.n
    shape = (n, n, n)
    padded = (n + 2) ** 3
    res = {"volume": n, "repeats": args.repeats, "padded_bytes": padded * 4, "floor": float(mex.DECONV_FLOOR),
           "bytes_per_padded_voxel": {"fused_iteration": 56, "unfused_iteration": 72, "smoothing": 24}, "volumes": {}}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    refl = vr.Volume(1)
    stream = torch.cuda.current_stream().cuda_stream
    for vname in ("shell", "random"):
        t = torch.empty(n * n * n, dtype=torch.float32, device="cuda")
        if vname == "shell":
            mex.synth_shell_device(t.data_ptr(), n, stream)
        else:
            t.copy_(torch.rand(n * n * n, generator=torch.Generator(device="cuda").manual_seed(23), device="cuda"))
        torch.cuda.synchronize()
        base = t.cpu().numpy().reshape(shape, order="F")
        # the padded twin for the launches alone: [z][y][x] with x fastest, edge-replicated; only read
        y = torch.nn.functional.pad(t.view(1, 1, n, n, n), (1, 1, 1, 1, 1, 1), mode="replicate").contiguous().view(-1)
        del t
        u, t1, t2 = torch.empty_like(y), torch.empty_like(y), torch.empty_like(y)
        out = res["volumes"].setdefault(vname, {"sigma": {}})
        wts = {}
        for k, sg in SIGMAS.items():
            buf = np.zeros(75, F)
            radius = []
            for j in range(3):
                Rj, w = mex.smooth_weights_host(sg[j])
                buf[25 * j:25 * j + w.size] = w
                radius.append(Rj)
            wts[k] = (radius, torch.from_numpy(buf).cuda())

        def plain(k, a, b, j):
            radius, w = wts[k]
            mex.smooth_axis_device(a.data_ptr(), b.data_ptr(), shape, j, w.data_ptr() + 100 * j, radius[j], 0, stream)

        def epilogue(k, a, b, j, epi, aux):
            radius, w = wts[k]
            mex.deconv_axis_device(a.data_ptr(), b.data_ptr(), shape, j, w.data_ptr() + 100 * j, radius[j], epi,
                                   aux.data_ptr(), mex.DECONV_FLOOR, 0, 0, stream)

        def fused_iteration(k):
            plain(k, u, t1, 0)
            plain(k, t1, t2, 1)
            epilogue(k, t2, t1, 2, _lib.VR_EPI_RATIO, y)
            plain(k, t1, t2, 0)
            plain(k, t2, t1, 1)
            epilogue(k, t1, u, 2, _lib.VR_EPI_UPDATE, u)

        def unfused_iteration(k):
            plain(k, u, t1, 0)
            plain(k, t1, t2, 1)
            plain(k, t2, t1, 2)
            mex.deconv_pointwise_device(t1.data_ptr(), t1.data_ptr(), shape, _lib.VR_EPI_RATIO, y.data_ptr(),
                                        mex.DECONV_FLOOR, 0, stream)
            plain(k, t1, t2, 0)
            plain(k, t2, t1, 1)
            plain(k, t1, t2, 2)
            mex.deconv_pointwise_device(t2.data_ptr(), u.data_ptr(), shape, _lib.VR_EPI_UPDATE, u.data_ptr(),
                                        mex.DECONV_FLOOR, 0, stream)

        def smoothing_passes(k):
            plain(k, y, t1, 0)
            plain(k, t1, t2, 1)
            plain(k, t2, t1, 2)

        em = vr.Volume(base)
        h = vr.volumeRender("new")
        vr.volumeRender("sync_volumes", h, np.uint64(0), em, refl, em)

        T = {k: {"call": {c: [] for c in COUNTS}, "fused": [], "unfused": [], "smooth_call": [], "smooth_filter_host": [],
                 "smooth_passes": []} for k in SIGMAS}
        for rep in range(args.repeats + 1):  # repeat 0 warms up
            for k, sg in SIGMAS.items():
                row = {}
                for c in COUNTS:
                    mex.set_deconvolution(h, None)
                    row[c] = timed(lambda: mex.set_deconvolution(h, F(sg), c))
                mex.set_deconvolution(h, None)
                sc = timed(lambda: mex.set_smoothing(h, F(sg)))
                sf = mex.derive_times(h)[0]
                mex.set_smoothing(h, None)
                u.copy_(y)
                a = timed(lambda: fused_iteration(k))
                u.copy_(y)
                b = timed(lambda: unfused_iteration(k))
                p = timed(lambda: smoothing_passes(k))
                if rep:
                    for c in COUNTS:
                        T[k]["call"][c].append(row[c])
                    for key, v in (("fused", a), ("unfused", b), ("smooth_call", sc), ("smooth_filter_host", sf), ("smooth_passes", p)):
                        T[k][key].append(v)
                print(vname, k, "repeat", rep, {c: round(v, 1) for c, v in row.items()}, "fused", round(a, 2), "unfused",
                      round(b, 2), "smoothing passes", round(p, 2), flush=True)
        for k in SIGMAS:
            tk = T[k]
            slope = [(hi - lo) / (COUNTS[2] - COUNTS[1]) for lo, hi in zip(tk["call"][COUNTS[1]], tk["call"][COUNTS[2]])]
            two = 2.0 * float(np.median(tk["smooth_passes"]))
            it, fu, un = float(np.median(slope)), float(np.median(tk["fused"])), float(np.median(tk["unfused"]))
            out["sigma"][k] = {
                "set_deconvolution_ms": {str(c): stat(tk["call"][c]) for c in COUNTS},
                "ms_per_iteration_from_slope_10_to_50": stat(slope),
                "fused_iteration_launches_ms": stat(tk["fused"]), "unfused_iteration_launches_ms": stat(tk["unfused"]),
                "set_smoothing_ms": stat(tk["smooth_call"]), "of_it_filter_and_statistics_read_back_ms_host": stat(tk["smooth_filter_host"]),
                "smoothing_passes_alone_ms": stat(tk["smooth_passes"]),
                "iteration_over_two_smoothing_filter_times": round(it / two, 3),
                "fused_over_unfused": round(fu / un, 3),
                "disjoint": bool(max(tk["fused"]) < min(tk["unfused"]) or max(tk["unfused"]) < min(tk["fused"])),
                "fused_iteration_bytes": padded * 56, "unfused_iteration_bytes": padded * 72,
                "fused_GBps_from_slope": round(padded * 56 / (it * 1e-3) / 1e9, 1),
                "fused_share_of_8TBps_from_slope": round(padded * 56 / (it * 1e-3) / 8e12, 3),
                "unfused_share_of_8TBps": round(padded * 72 / (un * 1e-3) / 8e12, 3),
                "bound": "HBM bandwidth (assumed, not shown by these shares)"}
        save()

        mex.set_deconvolution(h, F(CHECK_SIGMA), CHECK_ITERATIONS)
        out["correctness"] = c = check_blocks(mex, DR, h, base, n)
        print(vname, "blocks differing:", c["differing"], "of", c["blocks"], flush=True)
        mex.set_deconvolution(h, None)
        del y, u, t1, t2, base, em
        vr.volumeRender("delete", h)
        torch.cuda.empty_cache()
        save()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
