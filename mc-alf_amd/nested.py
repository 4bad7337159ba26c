"""Nested sampling on top of a batched replacement step: the book-keeping of the run in numpy on the host (O(nlive log nlive)
per round, not the hot path), the likelihood work behind two callables.

    loglike_cube(U) -> (theta, logL)                       rows of the unit cube in, transformed rows and logL out
    replace(U0, Lmin, dirs, nmoves, seed, stream_ids)
        -> (U, theta, logL, status, nevals, moves)         every start moved `nmoves` times under logL > Lmin

`als_fitter.nested_sample` passes its own `loglike_cube_batch` and `slice_replace_batch` (HIP kernels); the tests drive the
same loop with the numpy restatement of the replacement step.  This module imports nothing of the package: it is pure numpy.

A round: the K = `batch` live points of lowest logL die in order -- point j at live count nlive - j, ln X dropping by
1 / (nlive - j), weight (X_prev - X_new) L -- and K chains started from surviving points replace them under the K-th dead
point's logL.  Killing K points without replacement and then drawing K new ones above the K-th threshold is the sequential
scheme with the replacements postponed: the shrinkage factors are those of live counts nlive, nlive - 1, ..., nlive - K + 1."""
from __future__ import annotations

import numpy as np


class NestedResult:
    """What `nested_sample` returns.

    logZ, logZ_err, H     evidence, sqrt(H / nlive), information (nats)
    cube, theta, logL     the dead points in the order they died (the last live points included), [n, ndim] / [n]
    logw                  their log posterior weights, normalised: sum(exp(logw)) == 1
    rounds, nevals        replacement rounds; likelihood evaluations (the initial points and every trial of every chain)
    unfinished            rows a replacement call returned with status 0 (kept: they satisfy their constraint)
    rows_launched         rows handed to likelihood launches, carried finished rows included (None: the `replace` callable does
                          not say; `als_fitter.nested_sample` fills it in from `slice_stats()`)
    lnprior               lnprior of the dead points [n] under a Gaussian prior (None: the callables do not say;
                          `als_fitter.nested_sample` fills it in when one is set -- its callables then return logL + lnprior,
                          so `logL` holds that sum and logZ is ln of the integral of L g over the cube)
    nlive"""

    rows_launched = None
    lnprior = None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def equal_weight_samples(self, rng=None):
        """(logL, theta) of an equally weighted subset: every dead point is kept with probability w / max(w).  The pair goes
        straight into `write_equal_weights(path, logL, theta)`."""
        rng = np.random.default_rng(rng)
        keep = rng.random(self.logw.size) < np.exp(self.logw - self.logw.max())
        return self.logL[keep], self.theta[keep]


def _key(logL):
    """The sort key of a logL: NaN (and -inf) first."""
    return np.where(np.isnan(logL), -np.inf, logL)


def directions(cube):
    """Direction rows for chains among the points `cube` [n, ndim]: the columns of the Cholesky factor of their covariance
    (a small relative jitter added), diag(std) if the factorisation fails."""
    cube = np.asarray(cube, dtype=float)
    ndim = cube.shape[1]
    cov = np.atleast_2d(np.cov(cube, rowvar=False)) if cube.shape[0] > 1 else np.zeros((ndim, ndim))
    var = np.diag(cov).copy()
    try:
        if not np.isfinite(cov).all():
            raise np.linalg.LinAlgError("covariance is not finite")
        chol = np.linalg.cholesky(cov + 1e-9 * max(var.mean(), 1e-300) * np.eye(ndim))
        return np.ascontiguousarray(chol.T)
    except np.linalg.LinAlgError:
        std = np.sqrt(np.where(np.isfinite(var) & (var > 0.0), var, 0.0))
        return np.diag(np.where(std > 0.0, std, 1.0))


def nested_sample(loglike_cube, replace, ndim, nlive, batch=None, nmoves=None, dlogz=1e-3, max_rounds=100000, seed=0):
    """Run nested sampling until max(L_live) X < dlogz Z (or `max_rounds`), then add the remaining live points with the live
    count decreasing from nlive to 1.  `batch`: points replaced per round (None: nlive // 4); `nmoves`: slice moves per chain
    (None: 2 ndim).  `seed` seeds the host generator (initial points, chain starts) and is handed to `replace`; stream ids
    come from a running counter, so none repeats within a run."""
    nlive, ndim = int(nlive), int(ndim)
    K = max(1, nlive // 4) if batch is None else int(batch)
    if not 1 <= K < nlive:
        raise ValueError(f"batch must be in [1, nlive), got {K} with nlive {nlive}")
    nmoves = 2 * ndim if nmoves is None else int(nmoves)
    rng = np.random.default_rng(seed)
    U = rng.random((nlive, ndim))
    theta, L = loglike_cube(U)
    theta, L = np.array(theta, dtype=float).reshape(nlive, -1), np.array(L, dtype=float).reshape(nlive)
    nevals, unfinished, rounds, next_id = nlive, 0, 0, 0
    logX, logZ = 0.0, -np.inf
    dead_u, dead_t, dead_l, dead_w = [], [], [], []

    def die(idx, n_first):
        """Points `idx` (sorted by logL) die at live counts n_first, n_first - 1, ...: their unnormalised log weights."""
        nonlocal logX, logZ
        n = n_first - np.arange(idx.size, dtype=float)
        lx = logX + np.concatenate([[0.0], np.cumsum(-1.0 / n)])
        lw = lx[:-1] + np.log(-np.expm1(-1.0 / n)) + _key(L[idx])      # ln(X_prev - X_new) + ln L
        logX = float(lx[-1])
        logZ = float(np.logaddexp(logZ, np.logaddexp.reduce(lw)))
        dead_u.append(U[idx].copy()); dead_t.append(theta[idx].copy()); dead_l.append(L[idx].copy()); dead_w.append(lw)

    while rounds < max_rounds:
        key = _key(L)
        if logZ > -np.inf and key.max() + logX < np.log(dlogz) + logZ:
            break
        order = np.argsort(key, kind="stable")
        dying, alive = order[:K], order[K:]
        lmin = float(key[dying[-1]])
        starts = alive[key[alive] > lmin]                   # a start must satisfy the constraint strictly
        if starts.size == 0:
            break                                           # a plateau at the top: nothing above the threshold to start from
        die(dying, nlive)
        D = directions(U[alive])
        pick = starts[rng.integers(0, starts.size, K)]
        ids = np.arange(next_id, next_id + K, dtype=np.uint64)
        next_id += K
        Un, tn, Ln, status, ne, _ = replace(np.ascontiguousarray(U[pick]), np.full(K, lmin), D, nmoves, seed, ids)
        Ln = np.asarray(Ln, dtype=float)
        status = np.asarray(status)
        if (status < 0).any() or not (Ln > lmin).all():     # (NaN fails the comparison: it is never accepted as a replacement)
            raise RuntimeError("a replacement came back outside its constraint: rows %s" % np.flatnonzero((status < 0) | ~(Ln > lmin))[:8])
        U[dying], theta[dying], L[dying] = Un, np.asarray(tn, dtype=float).reshape(K, -1), Ln
        unfinished += int((status == 0).sum())
        nevals += int(np.asarray(ne).sum())
        rounds += 1
    die(np.argsort(_key(L), kind="stable"), nlive)
    cube, th, ll, lw = (np.concatenate(a) for a in (dead_u, dead_t, dead_l, dead_w))
    logZ = float(np.logaddexp.reduce(lw))                   # (one sum over all weights: the running value only steers the stop)
    logw = lw - logZ
    p = np.exp(logw)
    pos = p > 0.0
    H = float(np.sum(p[pos] * (_key(ll)[pos] - logZ)))
    return NestedResult(logZ=logZ, logZ_err=float(np.sqrt(max(H, 0.0) / nlive)), H=H, cube=cube, theta=th, logL=ll, logw=logw,
                        rounds=rounds, nevals=nevals, unfinished=unfinished, nlive=nlive)
