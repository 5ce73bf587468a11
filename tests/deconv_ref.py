"""The Richardson-Lucy deconvolution's value rule (include/vrhip.h vr_set_deconvolution) restated in numpy,
the reference of tests/test_deconv_host.py: the blur B is smooth_ref.smooth, the division and the
multiplication are numpy's fp32 `/` and `*` (each rounded once), the two comparisons are written out."""
import numpy as np

import smooth_ref as SR

F = np.float32


def data(y):
    """d = (y < 0) ? 0 : y -- NaN and -0 pass through."""
    y = np.asarray(y, F)
    with np.errstate(invalid="ignore"):
        return np.where(y < F(0), F(0), y).astype(F)


def deconvolve(y, sigma, iterations, floor=F(1e-6), weights_of=SR.weights):
    """u_n of y (at most 3-D, axis j = dims[j]); iterations = 0 or every sigma zero: y itself."""
    y = np.asarray(y, F)
    sigma = [F(s) for s in sigma]
    floor = F(floor)
    if iterations == 0 or not any(s != 0 for s in sigma):
        return np.asfortranarray(y.copy())
    d = data(y)
    u = d
    with np.errstate(all="ignore"):
        for _ in range(iterations):
            c = SR.smooth(u, sigma, weights_of)
            g = np.where(c > floor, c, floor).astype(F)  # a NaN in c compares false: floor
            r = (d / g).astype(F)
            m = SR.smooth(r, sigma, weights_of)
            u = (u * m).astype(F)
    return np.asfortranarray(u)
