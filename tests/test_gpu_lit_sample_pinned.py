"""The lit sample of the fast depth-lane march, pinned bit for bit to the commit before its
arithmetic was re-expressed (8-bit filter weights without v_rndne, ...): the frames of
tests/lit_sample_cases.py against tests/golden/march_fast_k2.npz, which was recorded with that
commit's library (tools/record_march_golden.py; the hash is in the file) -- not with the tree under
test, so a change that moves every kernel variant alike cannot pass unnoticed."""
import gc

import numpy as np
import pytest

import lit_sample_cases as cases

pytestmark = pytest.mark.gpu

vr = pytest.importorskip("volume_renderer_amd")


@pytest.fixture(scope="module")
def golden():
    with np.load(cases.GOLDEN) as z:
        return {k: z[k] for k in z.files}


@pytest.mark.parametrize("name", list(cases.CASES))
def test_lit_sample_equals_recorded_parent(monkeypatch, counter_clock, golden, name):
    gc.collect()
    img, kernel = cases.render_case(vr, name, monkeypatch.setenv)
    _, _, _, lanes, nl = cases.CASES[name]
    # the pinned path is the one launched: fast shading, K depth lanes, on-the-fly gradient (MODE 1),
    # specialised on the light count (the box's general launch on none), and the parent's own launch
    assert kernel.startswith(f"vr::fast::march_kernel<{lanes}, 1, ") and kernel.endswith(f", {nl}>"), kernel
    assert kernel == str(golden[name + "__kernel"]), (kernel, str(golden[name + "__kernel"]))
    want = golden[name]
    assert want.dtype == np.uint32 and img.shape == want.shape
    assert img.max() > 0
    got = img.view(np.uint32)
    diff = got != want
    assert not diff.any(), f"{name}: {int(diff.sum())} of {diff.size} words differ from commit {golden['commit']}"
