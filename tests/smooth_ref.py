"""The Gaussian smoothing's value rule (include/vrhip.h vr_set_smoothing) restated in numpy, the
reference of tests/test_smooth_host.py: weights in double, and per axis the chain
acc = w[0] * x[c(i-R)], acc = fma(w[k], x[c(i-R+k)], acc), every operation rounded once to fp32
(projection_ref.fma is the single-rounded fused multiply-add)."""
import math

import numpy as np

from projection_ref import fma

F = np.float32


def weights(sigma):
    """(R, the 2R+1 fp32 weights) of one axis for an fp32 sigma > 0, formed in double."""
    s = float(F(sigma))
    R = int(math.ceil(2.0 * s))
    g = [math.exp(-float(i * i) / (2.0 * s * s)) for i in range(-R, R + 1)]
    S = 0.0
    for v in g:  # ascending i
        S += v
    return R, np.array([v / S for v in g], np.float64).astype(F)


def smooth_axis(x, axis, R, w):
    """One axis pass over the fp32 array x with the weights w[0..2R] (any provenance), clamped borders."""
    x = np.asarray(x, F)
    n = x.shape[axis]
    idx = np.arange(n)

    def tap(k):
        return np.take(x, np.clip(idx - R + k, 0, n - 1), axis=axis)

    with np.errstate(all="ignore"):
        acc = (F(w[0]) * tap(0)).astype(F)
        for k in range(1, 2 * R + 1):
            acc = fma(F(w[k]), tap(k), acc)
    return acc


def smooth(x, sigma, weights_of=weights):
    """x (at most 3-D, axis j = dims[j]) under sigma[0..2]: passes along axis 0, 1, 2; an axis with
    sigma 0 or one voxel is skipped.  weights_of(sigma) -> (R, w): where the weights come from."""
    x = np.asarray(x, F)
    out = x.reshape(x.shape + (1,) * (3 - x.ndim))
    for j in range(3):
        if F(sigma[j]) > 0 and out.shape[j] > 1:
            R, w = weights_of(sigma[j])
            out = smooth_axis(out, j, R, w)
    return np.asfortranarray(out.reshape(x.shape))
