"""TEST INFRASTRUCTURE ONLY: the CPU reference of the slice views (include/vrhip.h vr_render_slice).

A numpy float32 restatement of the header's contract: sample k of pixel (y, x) at
  p_j = fma(dv_j, y, fma(du_j, x, origin_j)),  q_kj = fma(dw_j, k, p_j)
with projection_ref.fma (the single rounding of fmaf), inside iff 0 <= q_kj <= 1 on all three axes (a
NaN is outside), every inside sample from the oracle's sampler (or_tex3d_f32), reduced in the order of k:
  max  m = -inf; v_k > m (strictly) -> m = v_k, kk = k;  pixel m + 0, aux kk (no winner: NaN, NaN)
  min  the mirror image
  sum  s = s + v_k, c += 1;  pixel s if c > 0 else NaN, aux c
and the label plane at the centre sample kc = (n - 1) // 2 by the nearest rule
  i_j = min(int(q_j * D_j), D_j - 1), labels[i0, i1, i2], NaN when outside or without labels."""
from __future__ import annotations

import ctypes

import numpy as np

import oracle as O
from projection_ref import fma

F = np.float32
MAX, MIN, SUM = 0, 1, 2
MODES = (("max", MAX), ("min", MIN), ("sum", SUM))


class Slice:
    """origin, du, dv, dw (float32 [3]), H, W, n -- a vr_slice's geometry."""

    def __init__(self, origin, du, dv, dw, H, W, n=1):
        self.origin, self.du, self.dv, self.dw = (np.asarray(v, F).reshape(3).copy() for v in (origin, du, dv, dw))
        self.H, self.W, self.n = int(H), int(W), int(n)

    @classmethod
    def of(cls, s):
        """From a ctypes VrSlice (the host helpers fill one in)."""
        return cls(list(s.origin), list(s.du), list(s.dv), list(s.dw), s.resolution[0], s.resolution[1], s.samples)

    def geom(self):
        """The mex command's geom: 3 x 4 single [origin du dv dw]."""
        return np.asfortranarray(np.stack([self.origin, self.du, self.dv, self.dw], axis=1).astype(F))


def axis_slice(dims, axis, index, thickness=1):
    """The numpy double-then-round restatement of vr_slice_axis."""
    d = [int(x) for x in dims] + [1] * (3 - len(dims))
    a, b = [j for j in range(3) if j != axis]
    origin, du, dv, dw = (np.zeros(3, F) for _ in range(4))
    first = np.float64(index) - np.float64(thickness - 1) / np.float64(2)
    origin[axis] = F((first + np.float64(0.5)) / np.float64(d[axis]))
    dw[axis] = F(np.float64(1) / np.float64(d[axis]))
    origin[a] = F(np.float64(0.5) / np.float64(d[a]))
    dv[a] = F(np.float64(1) / np.float64(d[a]))
    origin[b] = F(np.float64(0.5) / np.float64(d[b]))
    du[b] = F(np.float64(1) / np.float64(d[b]))
    return Slice(origin, du, dv, dw, d[a], d[b], thickness)


def coords(s, k):
    """q of sample k of every pixel: three [H, W] float32 arrays."""
    x, y = np.meshgrid(np.arange(s.W, dtype=F), np.arange(s.H, dtype=F))  # [H, W]
    p = [fma(s.dv[j], y, fma(s.du[j], x, s.origin[j])) for j in range(3)]
    return [fma(s.dw[j], F(k), p[j]) for j in range(3)]


def inside(q):
    with np.errstate(invalid="ignore"):
        m = np.ones(q[0].shape, bool)
        for c in q:
            m &= (c >= 0) & (c <= 1)
    return m


def sample(vol, q, mask):
    """or_tex3d_f32 of `vol` (None: an unbound texture, reads 0) at the masked coordinates."""
    v = np.zeros(mask.shape, F)
    if vol is None:
        return v
    a = np.asfortranarray(vol, dtype=F)
    d = a.shape + (1,) * (3 - a.ndim) if a.ndim else (1, 1, 1)
    tex, cf = O.lib().or_tex3d_f32, ctypes.c_float
    idx = np.nonzero(mask)
    v[idx] = [tex(a.ctypes.data, d[0], d[1], d[2], cf(q[0][i, j]), cf(q[1][i, j]), cf(q[2][i, j])) for i, j in zip(*idx)]
    return v


def source_volume(S, source):
    """The array a 'render' of oracle session S would sample as `source` (0 emission, 1 absorption, 2
    reflection): the binding behind the slot index of the reference's host model (the alias rule, the
    module-global indices), MATLAB-shaped; None when that texture is unbound."""
    arr = S.bind[S.idx[(O.EM, O.AB, O.RE)[source]]]
    if arr is None or not arr.data.size:
        return None
    return arr.data.reshape(arr.dims, order="F")


def render_all(vol, s, labels=None):
    """{mode: (image, aux, label plane)} for the three modes from one pass over the samples; each
    plane [H, W] float32 column-major."""
    H, W = s.H, s.W
    with np.errstate(all="ignore"):
        m = {MAX: np.full((H, W), -np.inf, F), MIN: np.full((H, W), np.inf, F)}
        kk = {MAX: np.full((H, W), -1, np.int64), MIN: np.full((H, W), -1, np.int64)}
        acc = np.zeros((H, W), F)
        cnt = np.zeros((H, W), np.int64)
        for k in range(s.n):
            q = coords(s, k)
            ins = inside(q)
            v = sample(vol, q, ins)
            acc = np.where(ins, acc + v, acc).astype(F)  # one fp32 addition per inside sample, in order
            cnt += ins
            for mode in (MAX, MIN):
                w = ins & ((v > m[mode]) if mode == MAX else (v < m[mode]))  # strict; a NaN never wins
                m[mode] = np.where(w, v, m[mode]).astype(F)
                kk[mode] = np.where(w, k, kk[mode])
        lab = np.full((H, W), np.nan, F)
        if labels is not None and H * W:
            L = np.asarray(labels)
            D = L.shape + (1,) * (3 - L.ndim)
            L = L.reshape(D)
            q = coords(s, (s.n - 1) // 2)
            ins = inside(q)
            i = [np.minimum((np.where(ins, q[j], F(0)) * F(D[j])).astype(F).astype(np.int64), D[j] - 1) for j in range(3)]
            lab = np.where(ins, L[i[0], i[1], i[2]].astype(F), F(np.nan)).astype(F)
        lab = np.asfortranarray(lab)
        out = {SUM: (np.asfortranarray(np.where(cnt > 0, acc, F(np.nan)).astype(F)), np.asfortranarray(cnt.astype(F)), lab)}
        for mode in (MAX, MIN):
            won = kk[mode] >= 0
            out[mode] = (np.asfortranarray(np.where(won, m[mode] + F(0), F(np.nan)).astype(F)),
                         np.asfortranarray(np.where(won, kk[mode].astype(F), F(np.nan)).astype(F)), lab)
    return out


def render(vol, s, mode, labels=None):
    """(image, aux, label plane), each [H, W] float32 column-major, of the slice s of `vol`."""
    return render_all(vol, s, labels)[mode]
