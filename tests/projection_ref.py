"""TEST INFRASTRUCTURE ONLY: the CPU reference of the projection renders (include/vrhip.h
vr_render_projection).

A numpy float32 restatement of the oracle's ray set-up and march recurrences (oracle/vr_oracle.c
render_pixel / intersect_box, op for op), vectorised over the pixels of a frame.  The box, tstep and
the sample cap come from the oracle's own host model (OracleSession.params -> or_init_render), every
sample from the oracle's sampler (or_tex3d_f32); the reduction rules are those of the header:
  mip  m = -inf; v_k > m (strictly) -> m = v_k, t* = t;  pixel (Fe * (m + 0)) * color, aux t*
       (a miss or no winning sample: pixel 0, aux NaN)
  sum  s = s + v_k in sample order;  pixel ((Fe * s) * tstep) * color, aux n  (a miss: 0, 0)
The per-ray sample counts equal the oracle's render(pixels=...) step counts with an opacity
threshold that is never reached (tests/test_projection_ref.py pins that).

fma(a, b, c) is float32(float64(a) * float64(b) + float64(c)) with the double sum rounded to odd
(Knuth's two-sum gives the sum's error): the product of two floats is exact in double, and a sum
rounded to odd at 53 bits rounds to float32 as the exact value does, so this is the single rounding
of fmaf -- the plain double sum would round twice."""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O

F = np.float32
MIP, SUM = 0, 1


def fma(a, b, c):
    a, b, c = (np.asarray(v, F).astype(np.float64) for v in (a, b, c))
    with np.errstate(all="ignore"):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        even = (np.asarray(s).view(np.int64) & 1) == 0
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & even
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(F)


def _dot3(a, b):
    return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]))


def _normalize3(a):
    inv = F(1) / np.sqrt(_dot3(a, a))
    return [a[0] * inv, a[1] * inv, a[2] * inv]


def rays(P):
    """Ray set-up of every pixel of the frame OrParams P: dict of [H, W] float32 arrays (o is a
    per-frame constant) and the hit mask, as render_pixel computes them up to its sample loop."""
    Wn, Hn = int(P.width), int(P.height)
    with np.errstate(all="ignore"):
        W, H = F(Wn), F(Hn)
        x, y = np.meshgrid(np.arange(Wn, dtype=F), np.arange(Hn, dtype=F))  # [H, W]
        u = fma(x / W, F(2), F(-1))
        ratio = H / W
        v = fma((y / H) * F(2), ratio, -ratio)
        bmin = [F(P.boxmin[i]) for i in range(3)]
        bmax = [F(P.boxmax[i]) for i in range(3)]
        bscale = [F(1) / (bmax[i] - bmin[i]) for i in range(3)]
        X, Y, Z = ([F(P.rot[j][i]) for i in range(3)] for j in range(3))
        xoff, f, dist = F(P.rot[3][0]), F(P.rot[3][1]), F(P.rot[3][2])
        o = [fma(-dist, Z[i], xoff * X[i]) for i in range(3)]
        nX = _normalize3(X)
        du = [fma(f, Z[i], fma(v, Y[i], u * nX[i])) for i in range(3)]
        d = _normalize3(du)
        # intersect_box (slab test); a miss returns early there, so its later values do not matter
        inv = [F(1) / d[i] for i in range(3)]
        lo = [(np.where(inv[i] < 0, bmax[i], bmin[i]) - o[i]) * inv[i] for i in range(3)]
        hi = [(np.where(inv[i] < 0, bmin[i], bmax[i]) - o[i]) * inv[i] for i in range(3)]
        tmin, tmax = lo[0], hi[0]
        hit = ~((tmin > hi[1]) | (lo[1] > tmax))
        tmin = np.where(lo[1] > tmin, lo[1], tmin)
        tmax = np.where(hi[1] < tmax, hi[1], tmax)
        hit &= ~((tmin > hi[2]) | (lo[2] > tmax))
        tmin = np.where(lo[2] > tmin, lo[2], tmin)
        tmax = np.where(hi[2] < tmax, hi[2], tmax)
        tnear = np.where(tmin < 0, F(0), tmin).astype(F)
    return dict(o=o, d=d, tnear=tnear, tfar=tmax.astype(F), hit=hit, bmin=bmin, bscale=bscale)


def project_params(P):
    """Both projections of the frame OrParams P describes, from one march (the samples are the
    same): ({MIP: (image [H, W, 3], aux [H, W]), SUM: (image, aux)}, samples per ray [H, W] int64),
    column-major float32 like the product's."""
    Wn, Hn = int(P.width), int(P.height)
    R = rays(P)
    tstep, Fe = F(P.tstep), F(P.factor_emission)
    cap = int(P.max_steps)
    tex = O.lib().or_tex3d_f32
    data, nx, ny, nz = P.em.data, int(P.em.nx), int(P.em.ny), int(P.em.nz)
    cf = ctypes.c_float
    with np.errstate(all="ignore"):
        hit = R["hit"].reshape(-1)
        tfar = R["tfar"].reshape(-1)
        t = R["tnear"].reshape(-1).copy()
        d = [c.reshape(-1) for c in R["d"]]
        pos = [fma(d[i], t, R["o"][i]) for i in range(3)]
        step = [(d[i] * tstep).astype(F) for i in range(3)]
        n = np.zeros(hit.size, np.int64)
        m = np.full(hit.size, -np.inf, F)
        tm = np.full(hit.size, np.nan, F)
        s = np.zeros(hit.size, F)
        alive = hit.copy()
        while alive.any():
            idx = np.nonzero(alive)[0]
            ps = [((pos[i][idx] - R["bmin"][i]) * R["bscale"][i]).astype(F) for i in range(3)]
            if data:
                v = np.array([tex(data, nx, ny, nz, cf(a), cf(b), cf(c)) for a, b, c in zip(*ps)], F)
            else:
                v = np.zeros(idx.size, F)  # an unbound texture reads 0
            w = v > m[idx]  # strictly greater: the first maximum wins; NaN never does
            m[idx[w]] = v[w]
            tm[idx[w]] = t[idx[w]]
            s[idx] = s[idx] + v  # one fp32 addition per sample, in sample order
            n[idx] += 1
            go = n[idx] < cap
            t[idx[go]] = t[idx[go]] + tstep
            go &= ~(t[idx] > tfar[idx])
            for i in range(3):
                pos[i][idx[go]] = pos[i][idx[go]] + step[i][idx[go]]
            alive[idx] = go
        color = [F(P.color[i]) for i in range(3)]
        won = m > -np.inf
        planes = {MIP: (np.where(won, Fe * (m + F(0)), F(0)).astype(F), np.where(won, tm, F(np.nan)).astype(F), won),
                  SUM: (((Fe * s) * tstep).astype(F), n.astype(F), hit)}
        out = {}
        for mode, (p, aux, wr) in planes.items():
            img = np.zeros((Hn, Wn, 3), F, order="F")
            for c in range(3):
                img[:, :, c] = np.where(wr, p * color[c], F(0)).reshape(Hn, Wn)
            out[mode] = (img, np.asfortranarray(aux.reshape(Hn, Wn)))
    return out, n.reshape(Hn, Wn)


def project_both(S, h, factors, element_size_um, resolution, rot_flipped, props, thr, color):
    """Both projections of a frame of oracle session S / handle h, described by the positional
    'render' arguments after the lights and the LUT (which a projection ignores):
    ({MIP: (image, aux), SUM: (image, aux)}, samples per ray)."""
    P, keep, degenerate = S.params(h, None, None, factors, element_size_um, resolution, rot_flipped, props, thr, color)
    H, W = int(P.height), int(P.width)
    if degenerate or W * H == 0:
        z = np.zeros((H, W, 3), F, order="F")
        return ({MIP: (z, np.full((H, W), np.nan, F, order="F")), SUM: (z.copy(), np.zeros((H, W), F, order="F"))},
                np.zeros((H, W), np.int64))
    out = project_params(P)
    del keep
    return out


def project(S, h, mode, *args):
    """One projection: (image [H, W, 3], aux [H, W], samples per ray [H, W])."""
    out, n = project_both(S, h, *args)
    return out[mode][0], out[mode][1], n


def session(em, stamp=5):
    """An oracle session with `em` synced as emission and absorption and the class default
    reflection Volume(1): (S, h)."""
    S = O.OracleSession()
    h = S.new()
    v = O.OVolume(np.asfortranarray(em, dtype=F), stamp)
    S.sync_volumes(h, 0, v, O.OVolume(np.ones((1, 1), F), 3), v)
    return S, h


def same_bits(a, b):
    """Share of values with identical bits, NaN == NaN whatever the payload; NaN positions must agree."""
    a, b = np.ascontiguousarray(a, F).reshape(-1), np.ascontiguousarray(b, F).reshape(-1)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"NaN positions differ ({int(na.sum())} vs {int(nb.sum())})"
    eq = (a.view(np.uint32) == b.view(np.uint32)) | na
    return float(eq.mean()) if eq.size else 1.0


def assert_plane(got, ref, what=""):
    """The parity condition of a projection plane: NaN positions equal, at most 0.1 % of the values
    differ in bits (the share assert_parity allows) and none by more than 1e-2 x the plane's maximum
    (the same helper's cap).  Returns the share of identical values."""
    share = same_bits(got, ref)
    g = np.where(np.isnan(got), 0, got).astype(np.float64)
    r = np.where(np.isnan(ref), 0, ref).astype(np.float64)
    fin = np.isfinite(r) & np.isfinite(g)
    assert np.array_equal(np.isfinite(g), np.isfinite(r)) and np.array_equal(g[~fin], r[~fin]), f"{what}: infinities differ"
    scale = max(float(np.abs(r[fin]).max()) if fin.any() else 0.0, 1e-30)
    dmax = float(np.abs(g[fin] - r[fin]).max()) if fin.any() else 0.0
    print(f"{what}: identical {share:.6f}, max |d| {dmax:.3g} of scale {scale:.3g}")
    assert share >= 0.999, f"{what}: only {share:.6f} of the values bit-identical"
    assert dmax <= 1e-2 * scale, f"{what}: |d| {dmax} > 1e-2 * {scale}"
    return share


# ---- the scenes the projection tests share ------------------------------------------------------

# golden scene (tests/golden_cases.py) -> the [H W] its projections are checked at
FRAMES = {"hg2_compute_32": [40, 48], "stereo_right_24": [32, 41], "hg1_lookup_24": [40, 36]}


def scene_session(name):
    """A golden scene's volumes synced into a fresh oracle session: (S, h, scene, emission)."""
    from golden_cases import SCENES, STAMP_EM, STAMP_GRAD, STAMP_RE
    sc = SCENES[name]
    em = sc["em"]()
    S = O.OracleSession()
    h = S.new()
    v = O.OVolume(em, STAMP_EM)
    r = O.OVolume(sc["re"]() if sc["re"] else np.ones((1, 1), F), STAMP_RE)
    if sc["grads"]:
        S.sync_volumes(h, 0, v, r, v, *(O.OVolume(g, STAMP_GRAD) for g in O.matlab_gradient(em)))
    else:
        S.sync_volumes(h, 0, v, r, v)
    return S, h, sc, em


def frame_args(sc, res, factors=None, thr=None):
    """The positional 'render' arguments of scene sc after the lights and the LUT, at [H W] = res."""
    from golden_cases import render_argv
    a = list(render_argv(dict(sc, res=res), None, None)[2:])
    if factors is not None:
        a[0] = F(factors)
    if thr is not None:
        a[5] = F(thr)
    return a
