"""Round-24 GPU tests of the march's chunk set-up: the staging copy that moves up to four floats of a row
per lane (vr_stage.h stage_box, vr_stage_map.h, VR_STAGE_VEC).  It must copy the same voxels of the same
boxes and find the same boxes empty, so every frame and every chunk counter is what the one-float copy
gives.

For every case (volume x image size x camera) at 1, 2 and 4 depth lanes:
  (a) the frame equals, bit for bit, the frame of the library built with the items off
      (build_ab/libvrhip_off.so: tools/ablate_build.sh off "-DVR_STAGE_VEC=1 -DVR_UDIV_MAGIC=0
      -DVR_JOINT_MIN=0" -- with the last two it also serves tests/test_gpu_setup_trim.py),
      rendered by a child process that loads that library -- skipped with a message where it is absent;
  (b) the frame meets the oracle's fp32 / fp64 renders within the tolerance of tests/test_gpu_golden.py
      (conftest.assert_parity), and equals the unstaged render (VR_NO_LDS=1, which plans no box and
      copies nothing) bit for bit -- always;
  (c) the counted launch's chunk counters (staged / leaped / global, wave iterations, probe runs and
      failures, staged by S, floats staged, chunks leaped unstaged, the box-volume histogram of partial
      chunks) equal the switched-off library's -- skipped with (a).  They pin the boxes and the empty
      test.
The counters of the tree's own launches must show that the paths occurred: staged rows of every length
mod 4 (d_steps[47], the set of ex mod 4 over the staged boxes), a chunk staged at S = 16, a leap on an
all-zero staged box and a leap on the occupancy map's word."""
import gc
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF_LIB = os.path.join(ROOT, "build_ab", "libvrhip_off.so")

pytestmark = pytest.mark.gpu

KEYS = ("VR_NO_LDS", "VR_NO_EMPTY_SKIP", "VR_NO_BRICK_TEST", "VR_DEPTH_LANES", "VR_NO_PROBE", "VR_MAX_STEPS")
IMAGES = [(64, 48), (96, 64)]
# the three axis views (one looks down x: rows of a few floats, so the narrow widths and many rows per
# pass; one down z: on the permuted non-cube its 72-voxel axis is x), the metric frame's oblique view
# and a grazing one, which parks rays and stages partial boxes
CAMERAS = [(0, 0, 0), (90, 0, 0), (0, 90, 0), (125, 25, 0), (30, 10, 0)]
# shell64c: the 64^3 shell with its high corner filled -- data in the last voxel along x, y and z, so
# a box holds the padded volume's last row and a lane's group ends on the last float of the volume
VOLUMES = ["shell32", "shell64", "shell64c", "box24x40x72", "box72x40x24"]
LIGHTS = [([500, 1000, 550], [0, 1, 1]), ([0, 550, 90], [1, 0.5, 1])]
# counters compared between the builds (include/vrhip.h vr_render_device): [2] staged, [3] leaped, [4]
# global (partial or unstaged), [5] wave iterations, [6] lit ones, [7] probe runs leaped, [8:40] box
# volumes of the global chunks, [40:44] staged by S = 32, 16, 8, less, [44] probes that found data, [45]
# floats staged, [46] leaped unstaged
COUNTERS = list(range(2, 47))


def volume_data(name):
    import oracle as O
    if name.startswith("shell"):
        n = int(name[5:7])
        data = O.shell_volume(n)  # a power-of-two cube: the half-texel production path
        if name.endswith("c"):
            data = np.array(data, np.float32, order="F")
            data[n - 6:, n - 6:, n - 6:] = 0.8
            assert data[n - 1, n - 1, n - 1] != 0
        return data
    dims = tuple(int(x) for x in name[3:].split("x"))
    cut = O.shell_volume(72)[:24, :40, :72]  # the shell's wall crosses the faces of the non-cube
    if dims != (24, 40, 72):
        cut = cut.transpose(2, 1, 0)  # z becomes x
    assert cut.shape == dims
    return np.asfortranarray(cut)


def renderer(vr, vol, res, rot):
    """examples/example1.m:32-58 on synthetic data: two lights, on-the-fly gradient."""
    r = vr.VolumeRender()
    r.VolumeIllumination = vr.Volume(vr.HenyeyGreenstein(64))
    r.LightSources = [vr.LightSource(p, c) for p, c in LIGHTS]
    r.ElementSizeUm = [1, 1, 1]
    r.FocalLength = 3.0
    r.DistanceToObject = 6
    r.rotate(*rot)
    r.OpacityThreshold = 0.9
    r.ImageResolution = list(res)
    r.VolumeEmission = vol
    r.VolumeAbsorption = vol
    r.FactorAbsorption = 0.6
    r.FactorReflection = 0.4
    r.Color = [1, 1, 0]
    return r


def render_env(r, env):
    saved = {k: os.environ.pop(k, None) for k in KEYS}
    os.environ.update(env)
    try:
        return np.asarray(r.render(), np.float32)
    finally:
        for k in KEYS:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def counted(r, res):
    """The counter variant's launch of the renderer's current frame: its 48 counters."""
    import torch
    from volume_renderer_amd import mex
    W, H = res
    ra, keep = mex.render_args(r.LightSources, r.VolumeIllumination,
                               np.float32([r.FactorEmission, r.FactorReflection, r.FactorAbsorption]),
                               np.float32(r.ElementSizeUm), np.uint64([H, W]),
                               np.flip(r.RotationMatrix, 0).astype(np.float32),
                               np.float32([0, r.FocalLength, r.DistanceToObject]), np.float32(r.OpacityThreshold),
                               np.float32(r.Color))
    out = torch.zeros(3 * W * H, dtype=torch.float32, device="cuda")
    steps = torch.zeros(48, dtype=torch.int64, device="cuda")
    mex.render_device(r.objectHandle, ra, out.data_ptr(), None, steps.data_ptr())
    torch.cuda.synchronize()
    return steps.cpu().numpy(), out.cpu().numpy()


def render_volume(vr, name):
    """Every frame and counted launch of one volume: {key: array}."""
    got = {}
    ticks = iter(range(1000, 1 << 30))
    vr.set_clock(lambda: next(ticks))  # (strictly increasing stamps, as conftest's counter_clock)
    try:
        return _render_volume(vr, name, got)
    finally:
        vr.set_clock(None)


def _render_volume(vr, name, got):
    vol = vr.Volume(volume_data(name))
    for res in IMAGES:
        for rot in CAMERAS:
            r = renderer(vr, vol, res, rot)
            tag = f"{res[0]}x{res[1]}_{rot[0]}_{rot[1]}"
            for k in ("1", "2", "4"):
                got[f"img_{tag}_k{k}"] = render_env(r, {"VR_DEPTH_LANES": k})
            got[f"plain_{tag}"] = render_env(r, {"VR_NO_LDS": "1"})
            st, out = counted(r, res)
            got[f"steps_{tag}"] = st
            got[f"cimg_{tag}"] = out
            r.delete()
    return got


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.fixture(autouse=True)
def _clean():
    gc.collect()
    yield
    gc.collect()


@pytest.fixture(scope="module")
def tree_frames():
    import volume_renderer_amd as vr
    return {name: render_volume(vr, name) for name in VOLUMES}


@pytest.fixture(scope="module")
def off_frames(tmp_path_factory):
    """The same frames and counters from the switched-off library, rendered once by a child process
    (a process loads one libvrhip); None where that library was not built."""
    if not os.path.exists(OFF_LIB):
        return None
    out = str(tmp_path_factory.mktemp("stage_vec") / "off")
    env = dict(os.environ, VR_LIB_PATH=OFF_LIB)
    for k in KEYS:
        env.pop(k, None)
    subprocess.run([sys.executable, os.path.abspath(__file__), out], check=True, env=env, cwd=ROOT, timeout=300)
    return {name: dict(np.load(f"{out}_{name}.npz")) for name in VOLUMES}


def oracle_pair(name, res, rotation_flipped, lut, refl):
    import oracle as O
    S = O.OracleSession()
    h = S.new()
    ov = O.OVolume(volume_data(name), 1)
    S.sync_volumes(h, 0, ov, O.OVolume(refl, 2), ov)
    lights = np.array([p + c for p, c in LIGHTS], np.float32)
    args = (lights, O.OVolume(lut, 3), [1, 0.4, 0.6], [1, 1, 1], [res[1], res[0]], rotation_flipped, [0, 3, 6], 0.9,
            [1, 1, 0])
    ref32, _ = S.render(h, *args)
    ref64, _ = S.render(h, *args, double=True)
    return ref32, ref64


@pytest.mark.parametrize("name", VOLUMES)
def test_frames_meet_oracle_and_unstaged_render(tree_frames, name):
    """(b): every frame of the volume against the oracle (SURVEY.md 8c tolerance) and, bit for bit,
    against the unstaged render and the other depth-lane counts."""
    import volume_renderer_amd as vr
    from conftest import assert_parity
    got = tree_frames[name]
    lut = vr.Volume(vr.HenyeyGreenstein(64)).Data
    for res in IMAGES:
        for rot in CAMERAS:
            tag = f"{res[0]}x{res[1]}_{rot[0]}_{rot[1]}"
            r = vr.VolumeRender()
            r.rotate(*rot)
            flipped = np.flip(r.RotationMatrix, 0).astype(np.float32)
            refl = r.VolumeReflection.Data
            r.delete()
            ref32, ref64 = oracle_pair(name, res, flipped, lut, refl)
            plain = got[f"plain_{tag}"]
            assert plain.max() > 0, (name, tag)
            for k in ("1", "2", "4"):
                img = got[f"img_{tag}_k{k}"]
                assert np.array_equal(bits(img), bits(plain)), (name, tag, k, "staged against unstaged")
                stats = assert_parity(img, ref32, ref64, f"{name} {tag} K={k}")
            print(name, tag, stats)
            assert np.array_equal(bits(got[f"cimg_{tag}"]), bits(plain.reshape(-1, order="F"))), (name, tag, "counted")


@pytest.mark.parametrize("name", VOLUMES)
def test_frames_and_counters_equal_switched_off_build(tree_frames, off_frames, name):
    """(a) and (c): against the library built with VR_STAGE_VEC=1."""
    if off_frames is None:
        pytest.skip("build_ab/libvrhip_off.so is not built (tools/ablate_build.sh off \"-DVR_STAGE_VEC=1 "
                    "-DVR_UDIV_MAGIC=0 -DVR_JOINT_MIN=0\"): (a) and (c) need it; (b) ran in "
                    "test_frames_meet_oracle_and_unstaged_render")
    got, off = tree_frames[name], off_frames[name]
    assert sorted(got) == sorted(off)
    for key in sorted(got):
        if key.startswith("steps_"):
            a, b = got[key][COUNTERS], off[key][COUNTERS]
            assert np.array_equal(a, b), (name, key, a.tolist(), b.tolist())
        else:
            assert np.array_equal(bits(got[key]), bits(off[key])), (name, key)


def test_paths_occurred(tree_frames):
    """From the counters of the tree's counted launches: staged boxes with ex mod 4 = 0, 1, 2 and 3 (a
    whole number of four-float groups, and the overlapping last group at every offset), a chunk staged
    at S = 16, a leap on an all-zero staged box, a leap on the occupancy map's word -- and staged chunks
    in every frame."""
    residues = at16 = staged_leaps = unstaged_leaps = 0
    for name in VOLUMES:
        for key, st in tree_frames[name].items():
            if not key.startswith("steps_"):
                continue
            print(name, key, "staged", st[2], "leaped", st[3], "global", st[4], "by S", st[40:44].tolist(),
                  "floats", st[45], "leaped unstaged", st[46], "ex mod 4 seen", bin(int(st[47])))
            assert st[2] > 0, (name, key)
            residues |= int(st[47])
            at16 += int(st[41])
            staged_leaps += int(st[3]) - int(st[46])  # ([3] counts the leaps on the map's word too)
            unstaged_leaps += int(st[46])
    assert residues == 0b1111, f"ex mod 4 over the staged boxes: {bin(residues)}"
    assert at16 > 0, "no chunk was staged at S = 16"
    assert staged_leaps > 0, "no chunk was leaped on an all-zero staged box"
    assert unstaged_leaps > 0, "no chunk was leaped on the occupancy map's word"


if __name__ == "__main__":  # the child of off_frames: VR_LIB_PATH names the library
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import volume_renderer_amd as vr_child
    from volume_renderer_amd import mex as mex_child
    mex_child.enable_test_switches()
    for vol_name in VOLUMES:
        np.savez(f"{sys.argv[1]}_{vol_name}.npz", **render_volume(vr_child, vol_name))
    print(json.dumps({"library": os.environ.get("VR_LIB_PATH"), "volumes": VOLUMES}))
