"""numpy restatement of what mcalf_model_band_batch computes from the model matrix M[batch, npix]: per pixel, over the rows
that are not NaN there, the count, the mean and the population variance (both evaluated in np.longdouble, two passes) and
np.nanquantile under numpy's default "linear" rule -- and the bars tests/test_gpu_band.py holds the kernels to."""
import warnings

import numpy as np

EPS = 2.0 ** -52


def sorted_columns(M):
    """Per pixel, the sorted valid (non-NaN) values of the column: a list of npix 1-d arrays."""
    M = np.asarray(M, dtype=float)
    return [np.sort(col[~np.isnan(col)]) for col in M.T]


def moments(M):
    """(nvalid[npix] int64, mean[npix], var[npix]) with the sums in np.longdouble; NaN where a pixel has no valid row."""
    M = np.asarray(M, dtype=float)
    npix = M.shape[1]
    nvalid = np.zeros(npix, dtype=np.int64)
    mean, var = np.full(npix, np.nan), np.full(npix, np.nan)
    for k, x in enumerate(sorted_columns(M)):
        nvalid[k] = x.size
        if x.size:
            xl = x.astype(np.longdouble)
            mu = xl.sum() / x.size
            mean[k] = float(mu)
            var[k] = float(((xl - mu) ** 2).sum() / x.size)
    return nvalid, mean, var


def quantiles(M, q):
    """np.nanquantile(M, q, axis=0, method="linear"), shape [len(q), npix]; all-NaN columns give NaN without the warning."""
    M = np.asarray(M, dtype=float)
    q = np.asarray(q, dtype=float).reshape(-1)
    if q.size == 0:
        return np.empty((0, M.shape[1]))
    if M.shape[0] == 0:
        return np.full((q.size, M.shape[1]), np.nan)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return np.nanquantile(M, q, axis=0, method="linear")


def neighbours(M, q):
    """(lo, hi)[len(q), npix]: the two order statistics the linear rule interpolates between (NaN for an empty column)."""
    q = np.asarray(q, dtype=float).reshape(-1)
    cols = sorted_columns(M)
    lo, hi = np.full((q.size, len(cols)), np.nan), np.full((q.size, len(cols)), np.nan)
    for k, x in enumerate(cols):
        if x.size:
            h = (x.size - 1) * q
            f = np.floor(h).astype(int)
            lo[:, k], hi[:, k] = x[f], x[np.minimum(f + 1, x.size - 1)]
    return lo, hi


def quantile_bar(M, q):
    """4 ulp of max(|lo|, |hi|): numpy's two forms of the lerp and the plain lo + (hi - lo) t each make at most three roundings
    of at most half an ulp of that magnitude, so any two of them differ by at most 3 ulp."""
    lo, hi = neighbours(M, q)
    return 4.0 * EPS * np.maximum(np.abs(lo), np.abs(hi))


def mean_bar(M):
    """n eps max|x| per pixel: the forward error of any order of summation of n terms, and of the division."""
    n = np.array([x.size for x in sorted_columns(M)], dtype=float)
    amax = np.array([np.abs(x).max() if x.size else 0.0 for x in sorted_columns(M)])
    return n * EPS * amax


def var_bar(M):
    """2 (n + 3) eps max|x - mu|^2 + (n eps max|x|)^2 per pixel: the forward error of a two-pass variance (the centred squares
    summed in any order, plus the square of the error of the mean they are centred on).  A one-pass E[x^2] - mu^2 misses it
    wherever the spread is small against the level: every continuum pixel."""
    _, mean, _ = moments(M)
    out = np.zeros(len(mean))
    for k, x in enumerate(sorted_columns(M)):
        if x.size:
            out[k] = 2.0 * (x.size + 3) * EPS * np.abs(x - mean[k]).max() ** 2 + (x.size * EPS * np.abs(x).max()) ** 2
    return out


def same_nan(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b))


def within(got, want, bar):
    """NaNs coincide and every other entry is within its bar."""
    got, want = np.asarray(got), np.asarray(want)
    ok = ~np.isnan(want)
    return same_nan(got, want) and bool(np.all(np.abs(got[ok] - want[ok]) <= np.broadcast_to(bar, want.shape)[ok]))


def worst(got, want, bar):
    """max |got - want| / bar over the finite entries (0 / 0 counts as 0)."""
    got, want = np.asarray(got), np.asarray(want)
    ok = ~np.isnan(want) & ~np.isnan(got)
    if not ok.any():
        return 0.0
    d, b = np.abs(got[ok] - want[ok]), np.broadcast_to(bar, want.shape)[ok]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0.0, 0.0, d / b)
    return float(r.max())
