"""TEST INFRASTRUCTURE ONLY: the CPU reference of the transfer-function render (include/vrhip.h
vr_render_transfer).

A numpy restatement of the contract, vectorised over the pixels of a frame, on top of
tests/projection_ref.py (the rays and the singly rounded fma) and tests/isosurface_ref.py
(surface_sample: the gradient and the oracle-order shading at a position; expf / acosf through glibc;
the arithmetic pair _A32 / _A64).  It runs in float32 (ref32: every operation rounded once, as the
kernel's) and in float64 from the same fp32 inputs (ref64: the envelope of conftest.assert_parity).

The sample loop is oracle/vr_oracle.c render_pixel op for op with the contract's two substitutions:
C_c = L(colormap) where the oracle has color[c] in the emission term, A = L(alphamap, ab_s) where it
has ab_s in the opacity.  With a constant colormap equal to `color` and no alphamap it is the
oracle's render (tests/test_transfer_ref.py pins that bit for bit, sample counts included).

The fp32 opacity's exponential is selectable (EXPONENTIALS): "glibc", expf as the oracle calls it --
the reference of the parity checks -- or "kernel", a restatement of the product's exp_neg_rn
(csrc/vr_sampling.h: the Taylor form for |x| < 2^-7, exp in double rounded otherwise), which differs
from glibc's by one ulp on a small share of arguments.  With "kernel" nothing is left between this
reference and the product in the alpha plane (no shading enters it) and in an unlit image, so the GPU
tests compare those bit for bit.

The illumination term is evaluated only where alpha != 0 or eds is not finite: elsewhere the sample
adds fma(eds, C, ill) * 0, which is exactly 0 for a finite ill -- and ill is finite for finite
inputs, because the sampler reads a NaN LUT coordinate (a zero gradient's) as 0."""
from __future__ import annotations

import numpy as np

import isosurface_ref as IR
import projection_ref as PR
from projection_ref import F, fma  # noqa: F401

D = np.float64
VALUE, DEPTH = 0, 1
COORDS = {"value": VALUE, "depth": DEPTH}


def exp_neg_glibc(x):
    """exp(-x) in fp32 as the oracle forms it: expf of the (exact) negation."""
    return IR.expf(-np.asarray(x, F))


def exp_neg_kernel(x):
    """exp(-x) in fp32 as the product's exp_neg_rn: 1 + fma(x^2, q, -x) with q = fma(x, x / 24 - 1 / 6,
    1 / 2) for |x| < 2^-7, every operation rounded once; other x (NaN included): exp in double, rounded."""
    x = np.asarray(x, F).reshape(-1)
    with np.errstate(all="ignore"):
        x2 = (x * x).astype(F)
        q = fma(x, (x * (F(1) / F(24)) + (-(F(1) / F(6)))).astype(F), F(0.5))
        e = (F(1) + fma(x2, q, -x)).astype(F)
        big = ~(np.abs(x) < F(2.0 ** -7))
        e[big] = np.exp(-x[big].astype(D)).astype(F)
    return e


EXPONENTIALS = {"glibc": exp_neg_glibc, "kernel": exp_neg_kernel}


def lookup(table, lim, c, A=IR._A32):
    """L(T, n, lo, hi, c) of the contract in the arithmetic A: table [n] (fp32 values), lim = (lo, hi),
    c an array of coordinates."""
    T = A.T
    tab = np.asarray(table, F).reshape(-1).astype(T)
    n = tab.size
    with np.errstate(all="ignore"):
        lo, hi = T(F(lim[0])), T(F(lim[1]))
        inv = T(1) / (hi - lo)
        top = T(n - 1)
        c = np.asarray(c, T).reshape(-1)
        x = (((c - lo).astype(T) * inv).astype(T) * top).astype(T)
        x = np.where(x > 0, x, T(0)).astype(T)  # NaN and -0 -> +0
        x = np.where(x < top, x, top).astype(T)
        i = np.minimum(x.astype(np.int64), n - 2)
        w = (x - i.astype(T)).astype(T)
        slope = (tab[i + 1] - tab[i]).astype(T)
        return A.fma(w, slope, tab[i]).astype(T)


def rays(P, A=IR._A32):
    """projection_ref.rays in the arithmetic A (float32: that function itself)."""
    if A.T is F:
        return PR.rays(P)
    T = A.T
    Wn, Hn = int(P.width), int(P.height)
    with np.errstate(all="ignore"):
        W, H = T(Wn), T(Hn)
        x, y = np.meshgrid(np.arange(Wn, dtype=T), np.arange(Hn, dtype=T))
        u = (x / W) * T(2) + T(-1)
        ratio = H / W
        v = ((y / H) * T(2)) * ratio - ratio
        bmin = [T(P.boxmin[i]) for i in range(3)]
        bmax = [T(P.boxmax[i]) for i in range(3)]
        bscale = [T(1) / (bmax[i] - bmin[i]) for i in range(3)]
        X, Y, Z = ([T(P.rot[j][i]) for i in range(3)] for j in range(3))
        xoff, f, dist = T(P.rot[3][0]), T(P.rot[3][1]), T(P.rot[3][2])
        o = [-dist * Z[i] + xoff * X[i] for i in range(3)]
        nX = [X[i] / np.sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]) for i in range(3)]
        du = [f * Z[i] + (v * Y[i] + u * nX[i]) for i in range(3)]
        ln = np.sqrt(du[0] * du[0] + du[1] * du[1] + du[2] * du[2])
        d = [du[i] / ln for i in range(3)]
        inv = [T(1) / d[i] for i in range(3)]
        lo = [(np.where(inv[i] < 0, bmax[i], bmin[i]) - o[i]) * inv[i] for i in range(3)]
        hi = [(np.where(inv[i] < 0, bmin[i], bmax[i]) - o[i]) * inv[i] for i in range(3)]
        tmin, tmax = lo[0], hi[0]
        hit = ~((tmin > hi[1]) | (lo[1] > tmax))
        tmin = np.where(lo[1] > tmin, lo[1], tmin)
        tmax = np.where(hi[1] < tmax, hi[1], tmax)
        hit &= ~((tmin > hi[2]) | (lo[2] > tmax))
        tmin = np.where(lo[2] > tmin, lo[2], tmin)
        tmax = np.where(hi[2] < tmax, hi[2], tmax)
        tnear = np.where(tmin < 0, T(0), tmin)
    return dict(o=o, d=d, tnear=tnear, tfar=tmax, hit=hit, bmin=bmin, bscale=bscale)


def _same_tex(a, b):
    return a.data == b.data and int(a.nx) == int(b.nx) and int(a.ny) == int(b.ny) and int(a.nz) == int(b.nz)


def transfer_params(P, tf, A=IR._A32, exp="glibc"):
    """The transfer render of the frame OrParams P in the arithmetic A (exp: the fp32 opacity's
    exponential, a key of EXPONENTIALS; float64 takes numpy's).  tf: dict(colormap [N, 3],
    clim, alphamap ([M] or None), alim, coord (VALUE / DEPTH)).  Returns (image [H, W, 3], alpha
    [H, W], samples per ray [H, W] int64, rays) -- column-major, of A's type."""
    T = A.T
    Wn, Hn = int(P.width), int(P.height)
    R = rays(P, A)
    tstep, Fe, Fa = T(P.tstep), T(P.factor_emission), T(P.factor_absorption)
    thr = T(P.opacity_threshold)
    cap = int(P.max_steps)
    cm = np.asarray(tf["colormap"], F)
    am = None if tf.get("alphamap") is None else np.asarray(tf["alphamap"], F).reshape(-1)
    lit = IR.lit(P)
    alias = _same_tex(P.ab, P.em)
    exp_neg = EXPONENTIALS[exp] if T is F else (lambda x: np.exp(-x))
    with np.errstate(all="ignore"):
        hit = R["hit"].reshape(-1)
        tfar = R["tfar"].reshape(-1).astype(T)
        t = R["tnear"].reshape(-1).astype(T).copy()
        d = [np.asarray(c, T).reshape(-1) for c in R["d"]]
        pos = [A.fma(d[i], t, R["o"][i]).astype(T) for i in range(3)]
        step = [(d[i] * tstep).astype(T) for i in range(3)]
        N = hit.size
        n = np.zeros(N, np.int64)
        acc = [np.zeros(N, T) for _ in range(4)]  # sr, sg, sb, sa
        alive = hit.copy()
        while alive.any():
            idx = np.nonzero(alive)[0]
            p = [pos[i][idx] for i in range(3)]
            ps = [((p[i] - R["bmin"][i]) * R["bscale"][i]).astype(T) for i in range(3)]
            em_s = A.tex(P.em, *ps).astype(T)
            ab_s = em_s if alias else A.tex(P.ab, *ps).astype(T)
            cc = em_s if tf["coord"] == VALUE else t[idx]
            C = [lookup(cm[:, c], tf["clim"], cc, A) for c in range(3)]
            Aa = ab_s if am is None else lookup(am, tf["alim"], ab_s, A)
            e = (Fe * em_s).astype(T)
            a = (Fa * Aa).astype(T)
            alpha = (T(1) - np.asarray(exp_neg((a * tstep).astype(T)), T)).astype(T)
            eds = (e * tstep).astype(T)
            ill = [np.zeros(idx.size, T) for _ in range(3)]
            if lit:
                need = ~((alpha == 0) & np.isfinite(eds))
                if need.any():
                    _, _, _, il = IR.surface_sample(P, [c[need] for c in p], A)
                    for c in range(3):
                        ill[c][need] = il[c]
            om = (T(1) - acc[3][idx]).astype(T)
            for c in range(3):
                r = (A.fma(eds, C[c], ill[c]).astype(T) * alpha).astype(T)
                acc[c][idx] = A.fma(om, r, acc[c][idx])
            acc[3][idx] = A.fma(om, alpha, acc[3][idx])
            n[idx] += 1
            go = ~(acc[3][idx] > thr) & (n[idx] < cap)
            t[idx[go]] = t[idx[go]] + tstep
            go &= ~(t[idx] > tfar[idx])
            for i in range(3):
                pos[i][idx[go]] = pos[i][idx[go]] + step[i][idx[go]]
            alive[idx] = go
        img = np.zeros((Hn, Wn, 3), T, order="F")
        for c in range(3):
            img[:, :, c] = acc[c].reshape(Hn, Wn)
    return img, np.asfortranarray(acc[3].reshape(Hn, Wn)), n.reshape(Hn, Wn), R


def make_tf(colormap, clim=(0, 1), alphamap=None, alim=(0, 1), coord="value"):
    return dict(colormap=np.asarray(colormap, F), clim=(F(clim[0]), F(clim[1])),
                alphamap=None if alphamap is None else np.asarray(alphamap, F).reshape(-1),
                alim=(F(alim[0]), F(alim[1])), coord=COORDS[coord] if isinstance(coord, str) else int(coord))


def transfer(S, h, tf, lights, illum, factors, element_size_um, resolution, rot_flipped, props, thr, color,
             double=True, exp="glibc"):
    """The transfer render of a frame of oracle session S / handle h, described by tf (make_tf) and the
    nine positional 'render' arguments (lights: None or an (n, 6) array; illum: None or an OVolume):
    dict(img, alpha, n -- the ref32 planes (exp: its exponential) and the samples per ray; img64, alpha64 --
    ref64 (double=True);
    tnear, tfar, hit -- the fp32 rays' [H, W] planes)."""
    P, keep, degenerate = S.params(h, lights, illum, factors, element_size_um, resolution, rot_flipped, props, thr,
                                   color)
    H, W = int(P.height), int(P.width)
    if degenerate or W * H == 0:
        z3, z = np.zeros((H, W, 3), F, order="F"), np.zeros((H, W), F, order="F")
        return dict(img=z3, alpha=z, n=np.zeros((H, W), np.int64), img64=z3.astype(D), alpha64=z.astype(D))
    img, alpha, n, R = transfer_params(P, tf, IR._A32, exp)
    out = dict(img=img, alpha=alpha, n=n, tnear=np.asfortranarray(R["tnear"]), tfar=np.asfortranarray(R["tfar"]),
               hit=np.asfortranarray(R["hit"]))
    if double:
        out["img64"], out["alpha64"], _, _ = transfer_params(P, tf, IR._A64)
    del keep
    return out


def constant_colormap(color, n=2):
    """An [n, 3] colormap whose every row is `color`."""
    return np.asfortranarray(np.tile(np.asarray(color, F).reshape(1, 3), (n, 1)))
