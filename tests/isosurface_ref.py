"""TEST INFRASTRUCTURE ONLY: the CPU reference of the first-hit isosurface render (include/vrhip.h
vr_render_isosurface).

A numpy float32 restatement of the contract, vectorised over the pixels of a frame.  The ray set-up,
fma (singly rounded) and the plane comparisons are those of tests/projection_ref.py; every fetch,
the LUT included, is the oracle's sampler (or_tex3d_f32); square root and division are numpy
float32 (correctly rounded, as the oracle's sqrtf and '/'); acosf is glibc's through ctypes, the
oracle's own.  The gradient and the shading follow oracle/vr_oracle.c shade() op for op
(tests/test_isosurface_ref.py pins them to the oracle's one-sample render bit for bit).

The shading also runs in float64 from the fp32 surface point (key "img64"): the envelope
|fp32 - fp64| that the GPU test reports next to its differences."""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O
import projection_ref as PR
from projection_ref import F, assert_plane, fma, frame_args, same_bits, scene_session  # noqa: F401

REFINE = 6  # VR_ISO_REFINE
D = np.float64
_libm = ctypes.CDLL("libm.so.6")
_libm.acosf.restype = ctypes.c_float
_libm.acosf.argtypes = [ctypes.c_float]
_libm.expf.restype = ctypes.c_float
_libm.expf.argtypes = [ctypes.c_float]
PI32 = F(3.14159265358979323846)


def acosf(x):
    return np.array([_libm.acosf(ctypes.c_float(float(v))) for v in np.asarray(x, F).reshape(-1)], F)


def expf(x):
    return np.array([_libm.expf(ctypes.c_float(float(v))) for v in np.asarray(x, F).reshape(-1)], F)


def tex32(t, x, y, z):
    """or_tex3d_f32 of the OrTex t at the coordinate arrays (an unbound texture reads 0)."""
    x = np.asarray(x, F).reshape(-1)
    if not t.data:
        return np.zeros(x.size, F)
    f, cf = O.lib().or_tex3d_f32, ctypes.c_float
    nx, ny, nz = int(t.nx), int(t.ny), int(t.nz)
    return np.array([f(t.data, nx, ny, nz, cf(a), cf(b), cf(c))
                     for a, b, c in zip(x, np.asarray(y, F).reshape(-1), np.asarray(z, F).reshape(-1))], F)


def tex64(t, x, y, z):
    """The same sampler (clamp addressing, 8-bit weights) in float64 arithmetic."""
    x = np.asarray(x, D).reshape(-1)
    if not t.data:
        return np.zeros(x.size, D)
    n = (int(t.nx), int(t.ny), int(t.nz))
    vol = np.ctypeslib.as_array(ctypes.cast(t.data, ctypes.POINTER(ctypes.c_float)), shape=(n[0] * n[1] * n[2],))
    vol = vol.reshape(n, order="F").astype(D)
    i0, i1, w = [], [], []
    with np.errstate(all="ignore"):
        for c, m in zip((x, np.asarray(y, D).reshape(-1), np.asarray(z, D).reshape(-1)), n):
            c = np.where(np.isnan(c), 0.0, c)
            xb = c * m - 0.5
            fl = np.floor(xb)
            w.append(np.rint((xb - fl) * 256.0) / 256.0)
            i = np.clip(fl, -2, m + 1).astype(np.int64)
            i0.append(np.clip(i, 0, m - 1))
            i1.append(np.clip(i + 1, 0, m - 1))

        def lerp(a, b, ww):
            return ww * (b - a) + a
        c00 = lerp(vol[i0[0], i0[1], i0[2]], vol[i1[0], i0[1], i0[2]], w[0])
        c10 = lerp(vol[i0[0], i1[1], i0[2]], vol[i1[0], i1[1], i0[2]], w[0])
        c01 = lerp(vol[i0[0], i0[1], i1[2]], vol[i1[0], i0[1], i1[2]], w[0])
        c11 = lerp(vol[i0[0], i1[1], i1[2]], vol[i1[0], i1[1], i1[2]], w[0])
        return lerp(lerp(c00, c10, w[1]), lerp(c01, c11, w[1]), w[2])


class _A32:
    T = F
    fma = staticmethod(fma)
    tex = staticmethod(tex32)
    acos = staticmethod(acosf)
    pi = PI32


class _A64:
    T = D
    fma = staticmethod(lambda a, b, c: np.asarray(a, D) * np.asarray(b, D) + np.asarray(c, D))
    tex = staticmethod(tex64)
    acos = staticmethod(lambda x: np.arccos(np.asarray(x, D)))
    pi = D(PI32)


def lit(P):
    """Whether the frame has an illumination term: lights and a LUT."""
    return int(P.num_lights) > 0 and bool(P.lut.data)


def surface_sample(P, p, A=_A32):
    """The surface sample of the contract at the world positions p (three arrays) of frame P, in the
    arithmetic A: (v* -- the emission sample, g -- the gradient, n -- the unit normal, ill -- the
    illumination term, three arrays each)."""
    T = A.T
    with np.errstate(all="ignore"):
        p = [np.asarray(c, T).reshape(-1) for c in p]
        bmin = [T(P.boxmin[i]) for i in range(3)]
        bsc = [T(F(1) / (F(P.boxmax[i]) - F(P.boxmin[i]))) for i in range(3)]  # (the frame's fp32 constant)
        ps = [((p[i] - bmin[i]) * bsc[i]).astype(T) for i in range(3)]
        vs = A.tex(P.em, *ps).astype(T)
        if int(P.grad_method) == 0:  # computeGradient: world offsets +-gradStep on the emission binding
            g = []
            for i in range(3):
                s = T(P.grad_step[i])
                cp, cm = list(ps), list(ps)
                cp[i] = (((p[i] + s) - bmin[i]) * bsc[i]).astype(T)
                cm[i] = (((p[i] - s) - bmin[i]) * bsc[i]).astype(T)
                g.append(((A.tex(P.grad_em, *cp).astype(T) - A.tex(P.grad_em, *cm).astype(T)) * T(0.5)).astype(T))
        else:  # lookupGradient
            g = [A.tex(t, *ps).astype(T) for t in (P.gx, P.gy, P.gz)]

        def dot3(a, b):
            return A.fma(a[2], b[2], A.fma(a[1], b[1], a[0] * b[0]))

        def len3(a):
            return np.sqrt(dot3(a, a))

        def angle(a, b):
            return A.acos(dot3(a, b) / (len3(a) * len3(b))).astype(T) / A.pi
        inv = T(1) / np.sqrt(dot3(g, g))
        n = [-(g[i] * inv) for i in range(3)]
        ill = [np.zeros(p[0].size, T) for _ in range(3)]
        if lit(P):
            L = np.ctypeslib.as_array(ctypes.cast(P.lights, ctypes.POINTER(ctypes.c_float)),
                                      shape=(int(P.num_lights), 6)).astype(T)
            X, Z = ([T(P.rot[j][i]) for i in range(3)] for j in (0, 2))
            xoff, dist = T(P.rot[3][0]), T(P.rot[3][2])
            eye = [A.fma(-dist, Z[i], xoff * X[i]) for i in range(3)]
            col = [T(P.color[i]) for i in range(3)]
            refl = T(P.factor_reflection) * A.tex(P.re, *ps).astype(T)
            li = [eye[i] - p[i] for i in range(3)]
            alpha = angle(n, li)
            dli = dot3(li, n)
            lip = [A.fma(-dli, n[i], li[i]) for i in range(3)]
            for l in range(int(P.num_lights)):
                lo = [L[l, i] - p[i] for i in range(3)]
                beta = angle(n, lo)
                dlo = dot3(lo, n)
                lop = [A.fma(-dlo, n[i], lo[i]) for i in range(3)]
                gamma = angle(lip, lop)
                light = A.tex(P.lut, alpha, beta, gamma).astype(T)
                rl = refl * light
                ill = [A.fma(rl * L[l, 3 + c], col[c], ill[c]) for c in range(3)]
    return vs, g, n, ill


def isosurface_params(P, level):
    """The isosurface render of the frame OrParams P: dict of column-major arrays --
    img [H, W, 3], depth [H, W], normal [H, W, 3] (the three planes of the contract), img64 (the image
    with gradient and shading in float64 from the fp32 surface point), k [H, W] (the hit's sample
    index, -1: no surface), hi [H, W], tprev / tk [H, W] (t of samples k - 1 and k), tnear, vstar,
    n [H, W] (search samples visited)."""
    Wn, Hn = int(P.width), int(P.height)
    level = F(level)
    R = PR.rays(P)
    tstep, Fe = F(P.tstep), F(P.factor_emission)
    cap = int(P.max_steps)
    N = Wn * Hn
    with np.errstate(all="ignore"):
        hit = R["hit"].reshape(-1)
        tfar = R["tfar"].reshape(-1)
        t = R["tnear"].reshape(-1).copy()
        d = [c.reshape(-1) for c in R["d"]]
        pos = [fma(d[i], t, R["o"][i]) for i in range(3)]
        step = [(d[i] * tstep).astype(F) for i in range(3)]
        n = np.zeros(N, np.int64)
        k = np.full(N, -1, np.int64)
        bpos = [np.zeros(N, F) for _ in range(3)]  # pos_{k-1} (pos_0 when k = 0)
        bt = np.zeros(N, F)
        tk = np.full(N, np.nan, F)
        alive = hit.copy()

        def sample(q):
            return tex32(P.em, *[((q[i] - R["bmin"][i]) * R["bscale"][i]).astype(F) for i in range(3)])
        while alive.any():
            idx = np.nonzero(alive)[0]
            v = sample([pos[i][idx] for i in range(3)])
            got = v >= level  # a NaN sample is never >=
            h = idx[got]
            k[h] = n[h]
            tk[h] = t[h]
            first = h[n[h] == 0]
            for i in range(3):
                bpos[i][first] = pos[i][first]
            bt[first] = t[first]
            n[idx] += 1
            alive[h] = False
            m = idx[~got]  # below the level: this sample is the next one's k - 1
            for i in range(3):
                bpos[i][m] = pos[i][m]
            bt[m] = t[m]
            go = n[m] < cap
            t[m[go]] = t[m[go]] + tstep
            go &= ~(t[m] > tfar[m])
            for i in range(3):
                pos[i][m[go]] = pos[i][m[go]] + step[i][m[go]]
            alive[m] = go
        surf = np.nonzero(k >= 0)[0]
        deep = surf[k[surf] > 0]
        lo, hi = np.zeros(N, F), np.ones(N, F)
        for _ in range(REFINE):
            c = ((lo[deep] + hi[deep]) * F(0.5)).astype(F)
            v = sample([fma(step[i][deep], c, bpos[i][deep]) for i in range(3)])
            up = v >= level
            hi[deep[up]] = c[up]
            lo[deep[~up]] = c[~up]
        ps = [bpos[i].copy() for i in range(3)]
        ts = bt.copy()
        for i in range(3):
            ps[i][deep] = fma(step[i][deep], hi[deep], bpos[i][deep])
        ts[deep] = fma(tstep, hi[deep], bt[deep])
        color = [F(P.color[i]) for i in range(3)]
        img = np.zeros((Hn, Wn, 3), F, order="F")
        img64 = np.zeros((Hn, Wn, 3), D, order="F")
        normal = np.full((Hn, Wn, 3), np.nan, F, order="F")
        depth = np.full(N, np.nan, F)
        vstar = np.full(N, np.nan, F)
        depth[surf] = ts[surf]
        if surf.size:
            p = [ps[i][surf] for i in range(3)]
            vs, g, nn, ill = surface_sample(P, p, _A32)
            vs64, _, _, ill64 = surface_sample(P, p, _A64)
            vstar[surf] = vs
            for c in range(3):
                plane = np.zeros(N, F)
                plane[surf] = fma(Fe * vs, color[c], ill[c])
                img[:, :, c] = plane.reshape(Hn, Wn)
                plane = np.zeros(N, D)
                plane[surf] = D(Fe) * vs64 * D(color[c]) + ill64[c]
                img64[:, :, c] = plane.reshape(Hn, Wn)
                plane = np.full(N, np.nan, F)
                plane[surf] = nn[c]
                normal[:, :, c] = plane.reshape(Hn, Wn)

    def pl(a):
        return np.asfortranarray(a.reshape(Hn, Wn))
    return dict(img=img, img64=img64, depth=pl(depth), normal=normal, k=pl(k), hi=pl(hi), tprev=pl(bt), tk=pl(tk),
                tnear=pl(R["tnear"].reshape(-1)), hit=pl(hit), vstar=pl(vstar), n=pl(n), tstep=tstep,
                pos_prev=[pl(b) for b in bpos], step=[pl(s) for s in step])


def isosurface(S, h, level, lights, illum, factors, element_size_um, resolution, rot_flipped, props, thr, color):
    """The isosurface render of a frame of oracle session S / handle h, described by the nine
    positional 'render' arguments (lights: None or an (n, 6) array; illum: None or an OVolume)."""
    P, keep, degenerate = S.params(h, lights, illum, factors, element_size_um, resolution, rot_flipped, props, thr,
                                   color)
    H, W = int(P.height), int(P.width)
    if degenerate or W * H == 0:
        nan2 = np.full((H, W), np.nan, F, order="F")
        return dict(img=np.zeros((H, W, 3), F, order="F"), img64=np.zeros((H, W, 3), D, order="F"), depth=nan2,
                    normal=np.full((H, W, 3), np.nan, F, order="F"), k=np.full((H, W), -1, np.int64),
                    n=np.zeros((H, W), np.int64), hi=np.ones((H, W), F), vstar=nan2.copy())
    out = isosurface_params(P, level)
    del keep
    return out


# ---- the scenes the isosurface tests share -------------------------------------------------------

RAND = "rand12_re8"  # rand_volume(12), reflection rand_volume(8), the lights and the frame of example 1
# scene -> ([H W] of the GPU parity frame, level); the CPU tests use projection_ref.FRAMES
SCENES = {"hg2_compute_32": ([80, 96], 0.3), "stereo_right_24": ([64, 82], 0.3), "hg1_lookup_24": ([80, 72], 0.3),
          RAND: ([48, 40], 0.5)}
_cache = {}


def _declared(name):
    from golden_cases import EX1_LIGHTS, EX1_R, SCENES as GOLD
    if name in GOLD:
        return GOLD[name]
    assert name == RAND
    return dict(em=lambda: O.rand_volume(12), re=lambda: O.rand_volume(8), grads=False, lights=EX1_LIGHTS, lut=64,
                factors=[1, 0.4, 0.6], es=[1, 1, 1], res=SCENES[RAND][0], R=EX1_R, props=[0, 3, 6], thr=0.9,
                color=[1, 1, 0])


def scene(name, res=None, level=None, lights=True, grads=None, color=None, factors=None):
    """A scene of SCENES at [H W] = res (default: its GPU parity frame) and `level` (default: the
    scene's), computed once and shared: dict(sc, em, re, grads (the gradient volumes or None),
    lights ((n, 6) array or None), lut (array or None), args (the seven arguments after the LUT),
    level, ref (isosurface()), S, h).  lights=False: the logical false for the lights and the LUT;
    grads: override the scene's gradient method; color / factors: override those arguments."""
    from golden_cases import STAMP_EM, STAMP_GRAD, STAMP_LUT, STAMP_RE
    sc = _declared(name)
    res = list(SCENES[name][0] if res is None else res)
    level = SCENES[name][1] if level is None else level
    grads = sc["grads"] if grads is None else grads
    key = (name, tuple(res), float(level), bool(lights), bool(grads), None if color is None else tuple(color),
           None if factors is None else tuple(factors))
    if key in _cache:
        return _cache[key]
    em = sc["em"]()
    re = sc["re"]() if sc["re"] else None
    S = O.OracleSession()
    h = S.new()
    v = O.OVolume(em, STAMP_EM)
    r = O.OVolume(re if re is not None else np.ones((1, 1), F), STAMP_RE)
    gv = O.matlab_gradient(em) if grads else None
    if gv:
        S.sync_volumes(h, 0, v, r, v, *(O.OVolume(g, STAMP_GRAD) for g in gv))
    else:
        S.sync_volumes(h, 0, v, r, v)
    args = frame_args(sc, res, factors=factors)
    if color is not None:
        args[6] = F(color)
    lut = O.hg_lut(sc["lut"]) if lights else None
    ref = isosurface(S, h, level, sc["lights"] if lights else None, O.OVolume(lut, STAMP_LUT) if lights else None,
                     *args)
    d = dict(sc=sc, em=em, re=re, grads=gv, lights=sc["lights"] if lights else None, lut=lut, args=args, level=level,
             ref=ref, S=S, h=h, res=res)
    _cache[key] = d
    return d
