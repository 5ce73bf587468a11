"""TEST-ONLY numpy restatement of the volume histogram's contract (include/vrhip.h vr_volume_histogram):
the class of a voxel in float32 operations rounded once each, the rows by label, the clip rule per voxel
centre, the extrema in IEEE totalOrder through integer keys, the sum by math.fsum.  Nothing here looks at
how the kernel walks the volume."""
import math

import numpy as np

from projection_ref import fma

F = np.float32
BELOW, ABOVE, NAN = -1, -2, -3
SUMMARY = ("total", "below", "above", "nan", "ninf", "min", "max", "sum")


def bins(v, nbins, lim):
    """Per value its bin 0 .. nbins-1, or BELOW / ABOVE / NAN: inv = 1 / (hi - lo) once;
    x = ((v - lo) * inv) * nbins; b = min((int)x, nbins - 1)."""
    v = np.ascontiguousarray(v, F).reshape(-1)
    lo, hi = F(lim[0]), F(lim[1])
    with np.errstate(all="ignore"):
        inv = F(F(1) / F(hi - lo))
        inside = ~np.isnan(v) & ~(v < lo) & ~(v > hi)
        x = (((np.where(inside, v, lo) - lo).astype(F) * inv).astype(F) * F(nbins)).astype(F)
        b = np.minimum(x.astype(np.int64), nbins - 1)
    return np.where(np.isnan(v), NAN, np.where(v < lo, BELOW, np.where(v > hi, ABOVE, b))).astype(np.int32)


def keys(v):
    """totalOrder of non-NaN floats as uint32: -inf < ... < -0 < +0 < ... < +inf."""
    bits = np.ascontiguousarray(v, F).reshape(-1).view(np.uint32)
    return np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)


def unkey(k):
    k = np.uint32(k)
    bits = np.uint32(k ^ np.uint32(0x80000000)) if k & np.uint32(0x80000000) else np.uint32(~k)
    return np.array([bits], np.uint32).view(F)[0]


def rows_of(labels, first, count):
    """The row of every voxel: (uint8)(l - first) < count ? l - first : count; all 0 for count = 0."""
    l = np.ascontiguousarray(labels, np.uint8).reshape(-1)
    if count == 0:
        return np.zeros(l.size, np.int64)
    d = (l.astype(np.int64) - first) & 0xFF
    return np.where(d < count, d, count)


def clip_keep(dims, planes):
    """Per voxel (flattened in MATLAB order, dimension 0 fastest) whether every plane [n0 n1 n2 offset] keeps
    its centre q_j = ((float)i_j + 0.5f) / (float)d_j: fmaf(n2, q2, fmaf(n1, q1, fmaf(n0, q0, offset))) >= 0."""
    d = list(dims) + [1] * (3 - len(dims))
    q = [((np.arange(n, dtype=F) + F(0.5)).astype(F) / F(n)).astype(F) for n in d]
    q0, q1, q2 = np.meshgrid(*q, indexing="ij")
    keep = np.ones(d, bool)
    for p in np.asarray(planes, F).reshape(-1, 4):
        s = fma(p[2], q2, fma(p[1], q1, fma(p[0], q0, p[3])))
        keep &= s >= 0  # a NaN is not kept
    return keep.reshape(-1, order="F")


def histogram(vol, nbins, lim, labels=None, first=0, count=0, planes=None):
    """(counts uint64 [rows, nbins], summary dict of per-row arrays) of `vol` (None: an unbound texture).
    labels: uint8 of vol's shape, read when count > 0; planes: the clip planes in use, or None."""
    nrows = count + 1 if count > 0 else 1
    counts = np.zeros((nrows, nbins), np.uint64)
    s = {k: np.zeros(nrows, np.uint64) for k in SUMMARY[:5]}
    s["min"], s["max"], s["sum"] = np.full(nrows, np.nan, F), np.full(nrows, np.nan, F), np.zeros(nrows, np.float64)
    s["abs_sum"], s["finite"] = np.zeros(nrows, np.float64), np.zeros(nrows, np.uint64)  # for the sum's bound
    if vol is None:
        return counts, s
    v = np.asarray(vol, F).reshape(-1, order="F")
    row = rows_of(labels.reshape(-1, order="F"), first, count) if count > 0 else np.zeros(v.size, np.int64)
    if planes is not None and len(planes):
        keep = clip_keep(np.asarray(vol).shape, planes)
        v, row = v[keep], row[keep]
    b = bins(v, nbins, lim)
    for r in range(nrows):
        vr_, br = v[row == r], b[row == r]
        counts[r] = np.bincount(br[br >= 0], minlength=nbins).astype(np.uint64)
        s["below"][r], s["above"][r], s["nan"][r] = (br == BELOW).sum(), (br == ABOVE).sum(), (br == NAN).sum()
        s["ninf"][r] = np.isinf(vr_).sum()
        s["total"][r] = vr_.size
        assert s["total"][r] == s["nan"][r] + s["below"][r] + s["above"][r] + counts[r].sum()
        real = vr_[~np.isnan(vr_)]
        if real.size:
            k = keys(real)
            s["min"][r], s["max"][r] = unkey(k.min()), unkey(k.max())
        fin = vr_[np.isfinite(vr_)].astype(np.float64)
        s["sum"][r] = math.fsum(fin)
        s["abs_sum"][r] = math.fsum(np.abs(fin))
        s["finite"][r] = fin.size
    return counts, s
