"""TEST INFRASTRUCTURE ONLY: the CPU reference of the clip planes (include/vrhip.h vr_set_clip).

Clipping is a per-ray interval intersection after the ray set-up, so the reference wraps the ray
set-ups of the existing references without editing them: inside `with clipped(planes):` the functions
projection_ref.rays (which project_params and isosurface_ref.isosurface_params call) and
transfer_ref.rays (its float64 branch; its float32 branch is projection_ref.rays) return tnear, tfar
and hit with the plane rule of the header applied.  Everything after the set-up -- the samples, the
recurrences, the exits, the reductions -- is the unclipped references' own code.

The rule, restated in numpy float32 (fma: projection_ref.fma, singly rounded), per plane in order:
    N_k = n_k * bscale_k;   D = fma(-N_2, bmin_2, fma(-N_1, bmin_1, fma(-N_0, bmin_0, offset)))
    s0 = fma(N_2, o_2, fma(N_1, o_1, fma(N_0, o_0, D)));   sd = fma(N_2, d_2, fma(N_1, d_1, N_0 * d_0))
    tc = (-s0) / sd;   sd > 0: tnear = max-by-(tc > tnear);   sd < 0: tfar = min-by-(tc < tfar)
    sd == +-0 or NaN: a miss unless s0 >= 0
and after the last plane hit &= tnear <= tfar.  The float64 envelope runs the same rule in float64
from the fp32 constants N and D.

The reference of a clipped 'render' is transfer_ref.transfer with constant_colormap(color), which
tests/test_transfer_ref.py pins bit for bit to the C oracle's render."""
from __future__ import annotations

import contextlib

import numpy as np

import isosurface_ref as IR
import projection_ref as PR
import transfer_ref as TR
from projection_ref import F, fma

CLIP_MAX = 6  # VR_CLIP_MAX

# The plane sets the GPU tests use on the scenes of projection_ref.FRAMES, rows [n0 n1 n2 offset] in
# the normalized volume coordinate q (dimension order of Data).  OBLIQUE: one plane through the centre.
# WEDGE: three planes through the centre whose kept region is a wedge.  tests/test_clip_ref.py checks
# that neither is vacuous on any scene (rays shortened and rays lost, at least 50 each).
OBLIQUE = F([[0.6, -0.3, 0.74, -0.52]])
WEDGE = F([[0.6, -0.3, 0.74, -0.52], [-0.7, 0.5, 0.4, -0.1], [0.2, 0.9, -0.5, -0.3]])
PLANE_SETS = {"oblique": OBLIQUE, "wedge": WEDGE}
KEEP_ALL = F([[0.6, -0.3, 0.74, 100.0]])  # contains the whole box: every output stays bit-identical


def convert(planes, bmin, bscale):
    """The host conversion of the header in fp32: rows [N_0 N_1 N_2 D] for the box (bmin, bscale)."""
    planes = np.asarray(planes, F).reshape(-1, 4)
    out = np.zeros((planes.shape[0], 4), F)
    with np.errstate(all="ignore"):
        for i, p in enumerate(planes):
            N = [F(p[k] * F(bscale[k])) for k in range(3)]
            D = fma(-N[2], bmin[2], fma(-N[1], bmin[1], fma(-N[0], bmin[0], p[3])))
            out[i] = [N[0], N[1], N[2], F(D)]
    return out


def apply(R, planes, A=IR._A32):
    """The ray set-up R (a dict as projection_ref.rays returns) with the planes applied, in the
    arithmetic A: a copy of R with tnear, tfar, hit replaced, plus the unclipped ones as tnear0, tfar0,
    hit0."""
    T = A.T
    C = convert(planes, [F(b) for b in R["bmin"]], [F(b) for b in R["bscale"]]).astype(T)
    with np.errstate(all="ignore"):
        tnear, tfar, hit = np.array(R["tnear"], T), np.array(R["tfar"], T), np.array(R["hit"], bool)
        o = [np.asarray(c, T) for c in R["o"]]
        d = [np.asarray(c, T) for c in R["d"]]
        for N0, N1, N2, D in C:
            s0 = np.asarray(A.fma(N2, o[2], A.fma(N1, o[1], A.fma(N0, o[0], D))), T)
            sd = np.asarray(A.fma(N2, d[2], A.fma(N1, d[1], (N0 * d[0]).astype(T))), T)
            tc = ((-s0) / sd).astype(T)
            pos, neg = sd > 0, sd < 0
            tnear = np.where(pos & (tc > tnear), tc, tnear).astype(T)
            tfar = np.where(neg & (tc < tfar), tc, tfar).astype(T)
            hit = hit & ~(~pos & ~neg & ~(s0 >= 0))
        hit = hit & (tnear <= tfar)  # (a NaN fails)
    out = dict(R)
    out.update(tnear=tnear, tfar=tfar, hit=hit, tnear0=R["tnear"], tfar0=R["tfar"], hit0=R["hit"])
    return out


@contextlib.contextmanager
def clipped(planes):
    """Inside the block every reference's ray set-up applies `planes` (n x 4; empty: none)."""
    planes = np.asarray(planes, F).reshape(-1, 4)
    assert planes.shape[0] <= CLIP_MAX
    if planes.shape[0] == 0:  # no planes: the references as they are (not even the tnear <= tfar test)
        yield
        return
    pr_rays, tr_rays = PR.rays, TR.rays

    def rays32(P):
        return apply(pr_rays(P), planes, IR._A32)

    def rays_any(P, A=IR._A32):
        if A.T is F:
            return PR.rays(P)  # (the wrapped one: applied once)
        return apply(tr_rays(P, A), planes, A)

    PR.rays, TR.rays = rays32, rays_any
    try:
        yield
    finally:
        PR.rays, TR.rays = pr_rays, tr_rays


# ---- the references the tests share, computed once per (scene, plane set) ----------------------------

_cache = {}


def _key(planes):
    return np.asarray(planes, F).reshape(-1, 4).tobytes()


def scene(name, lit=False):
    """The scene `name` of projection_ref.FRAMES: dict(S, h, sc, em, args -- the seven arguments after
    the LUT at the frame of FRAMES, lights -- the scene's (n, 6) array, lut -- an OVolume).  lit: the
    oracle session of the lit references, a different one (a session that has rendered lit keeps its
    lights, as a handle does, and would light the unlit references too)."""
    import oracle as O
    from golden_cases import STAMP_LUT
    k = ("scene", name, bool(lit))
    if k not in _cache:
        S, h, sc, em = PR.scene_session(name)
        _cache[k] = dict(S=S, h=h, sc=sc, em=em, args=PR.frame_args(sc, PR.FRAMES[name]), lights=sc["lights"],
                         lut=O.OVolume(O.hg_lut(sc["lut"]), STAMP_LUT))
    return _cache[k]


def projections(name, planes):
    """projection_ref.project_both of scene `name` under `planes`: ({MIP: (image, aux), SUM: ...}, n)."""
    k = ("proj", name, _key(planes))
    if k not in _cache:
        s = scene(name)
        with clipped(planes):
            _cache[k] = PR.project_both(s["S"], s["h"], *s["args"])
    return _cache[k]


def rays_of(name, planes):
    """The clipped ray set-up of scene `name` (apply()'s dict, [H, W] planes)."""
    k = ("rays", name, _key(planes))
    if k not in _cache:
        s = scene(name)
        P, keep, _ = s["S"].params(s["h"], None, None, *s["args"])
        with clipped(planes):
            _cache[k] = PR.rays(P)
        del keep
    return _cache[k]


def isosurface(name, planes, level=0.3, lights=True):
    """isosurface_ref.isosurface of scene `name` under `planes` (lit by the scene's lights)."""
    k = ("iso", name, _key(planes), float(level), bool(lights))
    if k not in _cache:
        s = scene(name, lights)
        with clipped(planes):
            _cache[k] = IR.isosurface(s["S"], s["h"], level, s["lights"] if lights else None,
                                      s["lut"] if lights else None, *s["args"])
    return _cache[k]


def transfer(name, planes, tf, tag, lights=True, double=True, exp="glibc"):
    """transfer_ref.transfer of scene `name` under `planes` with tf (transfer_ref.make_tf); `tag` names
    tf in the cache."""
    k = ("tf", name, _key(planes), tag, bool(lights), bool(double), exp)
    if k not in _cache:
        s = scene(name, lights)
        with clipped(planes):
            _cache[k] = TR.transfer(s["S"], s["h"], tf, s["lights"] if lights else None, s["lut"] if lights else None,
                                    *s["args"], double=double, exp=exp)
    return _cache[k]


def render(name, planes, lights=True, double=True, exp="glibc"):
    """The reference of a clipped 'render': the transfer reference with the constant colormap `color`."""
    s = scene(name)
    return transfer(name, planes, TR.make_tf(TR.constant_colormap(s["args"][6])), "render", lights, double, exp)


def effect(name, planes):
    """(hit rays unclipped, hit rays clipped, rays still hit with fewer samples, rays hit -> miss)."""
    n0 = projections(name, np.zeros((0, 4), F))[1]
    n1 = projections(name, planes)[1]
    R = rays_of(name, planes)
    before, after = np.asarray(R["hit0"], bool), np.asarray(R["hit"], bool)
    return int(before.sum()), int(after.sum()), int((after & (n1 < n0)).sum()), int((before & ~after).sum())
