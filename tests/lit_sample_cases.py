"""The renders pinned by tests/golden/march_fast_k2.npz: small frames through the fast two-light (and
one-light) depth-lane march, recorded once with the library of the commit named in the file
(tools/record_march_golden.py) and compared bit for bit by tests/test_gpu_lit_sample_pinned.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "march_fast_k2.npz")

LIGHTS = (([500, 1000, 550], [0, 1, 1]), ([0, 550, 90], [1, 0.5, 1]))

# name -> (volume, rotation, lights, VR_DEPTH_LANES, NL); every frame is 96 x 64.  NL: the light count the
# kernel launched is specialised on (its last template argument) -- the cube's launches on their
# count, the general on-the-fly gradient launch of the box on none (0)
CASES = {
    "cube64_k2": ("cube64", (125, 25, 0), 2, "2", 2),       # V_shell(64) in [-1, 1]^3: the half-texel tap launch
    "cube64_grazing_k2": ("cube64", (30, 10, 0), 2, "2", 2),  # partial and edge chunks: the non-whole loop
    "cube64_one_light_k2": ("cube64", (125, 25, 0), 1, "2", 1),
    "cube64_k4": ("cube64", (125, 25, 0), 2, "4", 2),
    "box32x48x64_k2": ("box", (125, 25, 0), 2, "2", 0),     # not a cube: axis_raw_s and global-memory taps
}
RES = (96, 64)


def volume(kind):
    import oracle as O
    v = O.shell_volume(64)
    if kind == "box":
        v = np.asfortranarray(v[:32, :48, :])
    return v


def render_case(vr, name, setenv):
    """Render case `name`; setenv(key, value) sets an environment variable for the render (the
    caller restores it).  Returns (image, name of the march kernel launched)."""
    from volume_renderer_amd import mex
    kind, rot, nl, lanes, _ = CASES[name]
    setenv("VR_DEPTH_LANES", lanes)
    r = vr.VolumeRender()
    r.VolumeIllumination = vr.Volume(vr.HenyeyGreenstein(64))
    r.LightSources = [vr.LightSource(p, c) for p, c in LIGHTS[:nl]]
    r.ElementSizeUm = [1, 1, 1]
    r.FocalLength = 3.0
    r.DistanceToObject = 6
    r.rotate(*rot)
    r.OpacityThreshold = 0.9
    r.ImageResolution = list(RES)
    v = vr.Volume(volume(kind))
    r.VolumeEmission = v
    r.VolumeAbsorption = v
    r.FactorAbsorption = 0.6
    r.FactorReflection = 0.4
    r.Color = [1, 1, 0]
    img = np.asarray(r.render(), np.float32)
    kernel = mex.last_march_kernel()
    r.delete()
    return img, kernel
