#!/usr/bin/env python3
"""tools/record_march_golden.py --commit HASH [--out FILE] -- record tests/golden/march_fast_k2.npz.

Renders the cases of tests/lit_sample_cases.py on the GPU with the library in use (VR_LIB_PATH
selects another build) and stores each frame's uint32 bits, the march kernel it launched and HASH,
the commit that library was built from.  tests/test_gpu_lit_sample_pinned.py compares later trees
against the file bit for bit, so it is recorded once, from the parent of a change to the lit
sample's arithmetic, and not from the tree under test."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="commit the library in use was built from")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import volume_renderer_amd as vr
    from volume_renderer_amd import mex
    import lit_sample_cases as cases
    mex.enable_test_switches()
    out = {"commit": np.array(args.commit)}
    for name in cases.CASES:
        img, kernel = cases.render_case(vr, name, os.environ.__setitem__)
        assert np.isfinite(img).all() and img.max() > 0, name
        out[name] = img.view(np.uint32)
        out[name + "__kernel"] = np.array(kernel)
        print(f"{name}: {img.shape} max {img.max():.6f} lit {(img > 0).mean():.3f} {kernel}")
    path = args.out or cases.GOLDEN
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    print(f"wrote {path} ({os.path.getsize(path)} bytes)")


if __name__ == "__main__":
    main()
