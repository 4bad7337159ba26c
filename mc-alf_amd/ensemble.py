"""Ensemble MCMC on top of a batched walker step: the book-keeping of a run in numpy on the host, the likelihood work behind
two callables.

    loglike_cube(U) -> (theta, logL[, lnprior])            rows of the unit cube in, transformed rows and logL out (and lnprior of
                                                           the rows, where the target has a prior beyond the flat cube)
    advance(U0, nsteps, thin, seed, first_iter, chain)
        -> (U, theta, logL, status, naccept, chainU, chainL)
                                                           the walkers U0 [n, ndim] moved by `nsteps` iterations; with `chain`
                                                           the state after every thin-th one, [nsteps // thin, n, ndim] and
                                                           [nsteps // thin, n] (else None, None)

`als_fitter.ensemble_sample` passes its own `loglike_cube_batch` and `ensemble_batch` (HIP kernels; the move and its scale are
bound there); the tests drive the same loop with the numpy restatement of the step.  This module imports nothing of the
package: it is pure numpy.

A run: the walkers are drawn uniformly in the cube, or in a ball of half-width `ball` around the cube point `start`, clipped to
the cube; `burn` iterations are made and forgotten; `nsteps` more are made with every thin-th state kept.  The second call
continues the first (`first_iter = burn`), so the run is the one call of burn + nsteps iterations, bit for bit.  The kept cube
rows go through `loglike_cube` once for their transformed rows: nsteps // thin x nwalkers more rows, 1 / thin of the run's."""
from __future__ import annotations

import numpy as np


def batch_means_se(x, nbatch=20):
    """Standard error of the mean of the correlated series `x` [T] or [T, d] by batch means: the first nbatch (T // nbatch)
    entries are cut into `nbatch` consecutive batches, and the error is the standard deviation of the batch means (ddof 1)
    over sqrt(nbatch).  Sound when a batch is long against the autocorrelation time."""
    x = np.asarray(x, dtype=float)
    nbatch = int(nbatch)
    size = x.shape[0] // nbatch
    if nbatch < 2 or size < 1:
        raise ValueError(f"{x.shape[0]} entries cannot be cut into {nbatch} batches")
    means = x[:nbatch * size].reshape((nbatch, size) + x.shape[1:]).mean(axis=1)
    return means.std(axis=0, ddof=1) / np.sqrt(nbatch)


def _autocorr(x):
    """Normalised autocorrelation function of the series x [T] (FFT, zero padded)."""
    x = np.asarray(x, dtype=float) - np.mean(x)
    n = 1 << int(2 * x.size - 1).bit_length()
    f = np.fft.rfft(x, n)
    acf = np.fft.irfft(f * np.conjugate(f), n)[:x.size]
    return acf / acf[0] if acf[0] > 0.0 else np.zeros(x.size)


def sokal_tau(x, c=5.0):
    """Integrated autocorrelation time of the series x [T] with Sokal's automatic window: tau(M) = 1 + 2 sum_{t <= M} rho(t) at
    the smallest M with M >= c tau(M) (the last M if none)."""
    tau = 2.0 * np.cumsum(_autocorr(x)) - 1.0
    ok = np.arange(tau.size) >= c * tau
    return float(tau[np.argmax(ok)] if ok.any() else tau[-1])


class EnsembleResult:
    """What `ensemble_sample` returns.

    cube, theta, logL     the kept chain, [nkeep, nwalkers, ndim] twice and [nkeep, nwalkers]
    lnprior               lnprior of the kept rows [nkeep, nwalkers] where `loglike_cube` returns it as a third array (one pass
                          over the rows already transformed), else None; logL is the likelihood's in either case
    accept_frac           accepted proposals per walker over the nsteps iterations after burn-in, / nsteps (one proposal per
                          walker and iteration) [nwalkers]
    status                0, or -1 for a walker whose start lay outside the cube or had a NaN (it never moved) [nwalkers]
    last                  the walkers after the last iteration [nwalkers, ndim] (continue with first_iter = burn + nsteps)
    nwalkers, nsteps, burn, thin, seed"""

    lnprior = None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def means(self):
        """The series of ensemble means of the cube coordinates [nkeep, ndim], over the walkers of status 0."""
        return self.cube[:, self.status == 0, :].mean(axis=1)

    def autocorr_time(self, c=5.0):
        """Integrated autocorrelation time per coordinate [ndim], in iterations (kept steps x thin): Sokal's window with
        c = 5 on the series of ensemble means."""
        mu = self.means()
        return np.array([sokal_tau(mu[:, k], c) for k in range(mu.shape[1])]) * self.thin

    def flat(self):
        """(logL, theta) of the kept chain with the walkers of status 0, flattened to [rows] and [rows, ndim]: ready for
        `write_equal_weights`, `model_band_batch` and `eqw_batch`."""
        ok = self.status == 0
        return np.ascontiguousarray(self.logL[:, ok].reshape(-1)), np.ascontiguousarray(self.theta[:, ok, :].reshape(-1, self.theta.shape[2]))


def _check_run(n, nsteps, burn, thin, swap_every=None):
    """The run arguments of `ensemble_sample`, and of `tempering.tempered_sample` (which has `swap_every` as well)."""
    if n < 4 or n % 2:
        raise ValueError(f"nwalkers must be even and >= 4, got {n}")
    if nsteps < 0 or burn < 0 or thin < 1 or (swap_every or 0) < 0:
        raise ValueError(f"nsteps and burn must be >= 0 and thin >= 1, got {nsteps}, {burn}, {thin}" if swap_every is None else
                         f"nsteps, burn and swap_every must be >= 0 and thin >= 1, got {nsteps}, {burn}, {swap_every}, {thin}")


def _draw_starts(seed, shape, start, ball):
    """The walkers' starts, `shape` = [..., ndim]: ONE uniform draw of that shape from `default_rng(seed)`, mapped into the
    ball of half-width `ball` around the cube point `start` and clipped to the cube where the two are given."""
    if (start is None) != (ball is None):
        raise ValueError("start and ball go together")
    U = np.random.default_rng(seed).random(shape)
    if start is not None:
        centre = np.asarray(start, dtype=float).reshape(shape[-1])
        U = np.clip(centre + float(ball) * (2.0 * U - 1.0), 0.0, 1.0)
    return U


def _kept_rows(loglike_cube, cube):
    """The kept cube rows [nkeep, n, ndim] through `loglike_cube` once: their transformed rows [nkeep, n, ...] and, as the
    keyword for an `EnsembleResult`, lnprior [nkeep, n] where a third array comes back."""
    nkeep, n, ndim = cube.shape
    out = loglike_cube(cube.reshape(-1, ndim)) if nkeep else (np.empty((0, n, ndim)),)
    theta = np.asarray(out[0], dtype=float).reshape(nkeep, n, -1 if nkeep else ndim)
    return theta, (dict(lnprior=np.asarray(out[2], dtype=float).reshape(nkeep, n)) if len(out) > 2 else {})


def ensemble_sample(loglike_cube, advance, ndim, nwalkers, nsteps, burn=0, thin=1, start=None, ball=None, seed=0):
    """`burn` + `nsteps` iterations of `nwalkers` walkers (even, >= 4); see the module's text.  `seed` seeds the host generator
    of the starts and is handed to `advance`."""
    ndim, n, nsteps, burn, thin = int(ndim), int(nwalkers), int(nsteps), int(burn), int(thin)
    _check_run(n, nsteps, burn, thin)
    U = _draw_starts(seed, (n, ndim), start, ball)
    if burn:
        U = advance(U, burn, thin=1, seed=seed, first_iter=0, chain=False)[0]
    U, _, _, status, naccept, CU, CL = advance(np.ascontiguousarray(U), nsteps, thin=thin, seed=seed, first_iter=burn, chain=True)
    nkeep = nsteps // thin
    CU, CL = np.asarray(CU, dtype=float).reshape(nkeep, n, ndim), np.asarray(CL, dtype=float).reshape(nkeep, n)
    theta, extra = _kept_rows(loglike_cube, CU)
    return EnsembleResult(cube=CU, theta=theta, logL=CL, **extra, accept_frac=np.asarray(naccept) / max(nsteps, 1), status=np.asarray(status),
                          last=np.asarray(U), nwalkers=n, nsteps=nsteps, burn=burn, thin=thin, seed=seed)
