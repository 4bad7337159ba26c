"""Parallel tempering on top of a batched tempered walker step: the book-keeping of a run and its evidence estimators in numpy
on the host, the likelihood work behind two callables.

    loglike_cube(U) -> (theta, logL)                       rows of the unit cube in, transformed rows and logL out
    advance(U0, nsteps, thin, swap_every, seed, first_iter, chain, chain_temps)
        -> (U, theta, logL, status, naccept, nswap, chainU, chainL)
                                                           the walkers U0 [T, n, ndim] of T temperatures moved by `nsteps`
                                                           iterations with a swap round after every swap_every-th; with `chain`
                                                           the state after every thin-th one, [nkeep, chain_temps, n, ndim] and
                                                           [nkeep, T, n] (else None, None); logL is always the untempered value

`als_fitter.tempered_sample` passes its own `loglike_cube_batch` and `tempered_batch` (HIP kernels; the ladder, the move and
its scale are bound there); the tests drive the same loop with the numpy restatement of the step.  This module imports nothing
of the package but `ensemble`, which is pure numpy as well.

A run: temperature t samples logL^beta[t] over the cube, beta[0] = 1 the posterior and the last rung, beta = 0, the prior.  The
walkers of every rung are drawn uniformly in the cube, or in a ball of half-width `ball` around the cube point `start`; `burn`
iterations are made and forgotten; `nsteps` more are made with every thin-th state kept: logL of every rung (the evidence needs
them) and the cube rows of the cold rung alone.  The second call continues the first (`first_iter = burn`), so the run is the
one call of burn + nsteps iterations, bit for bit."""
from __future__ import annotations

import numpy as np

from .ensemble import EnsembleResult


def default_ladder(ntemps, beta_min):
    """The inverse temperatures [ntemps] of a geometric ladder that ends at the prior: beta_t = beta_min^(t / (T - 2)) for
    t < T - 1 (from 1 down to beta_min) and beta_{T - 1} = 0.  T = 2 is (1, 0)."""
    T, beta_min = int(ntemps), float(beta_min)
    if T < 2 or not 0.0 < beta_min < 1.0:
        raise ValueError(f"ntemps must be >= 2 and beta_min in (0, 1), got {ntemps}, {beta_min}")
    beta = np.zeros(T)
    beta[:T - 1] = beta_min ** (np.arange(T - 1) / max(T - 2, 1))
    return beta


def ln_prior_mass(lo, hi, mu, sigma):
    """ln of the integral over the unit cube of the Gaussian prior factors g (not renormalised for the box): the sum over the
    coordinates with sigma[k] > 0 of ln((Phi((hi_k - mu_k) / sigma_k) - Phi((lo_k - mu_k) / sigma_k)) / (hi_k - lo_k)), Phi the
    standard normal distribution function by `math.erf`.  It is ln Z(beta = 0) of a ladder under such a prior; 0.0 with none."""
    import math                                             # (the standard library's erf: the module stays numpy and `ensemble`)
    total = 0.0
    for l, h, m, s in zip(np.asarray(lo, dtype=float), np.asarray(hi, dtype=float), np.asarray(mu, dtype=float), np.asarray(sigma, dtype=float)):
        if s > 0.0:
            a, b = (l - m) / (s * math.sqrt(2.0)), (h - m) / (s * math.sqrt(2.0))
            total += math.log(0.5 * (math.erf(b) - math.erf(a)) / (h - l))
    return total


class TemperedResult:
    """What `tempered_sample` returns.

    betas                 the ladder [T]
    logL                  the kept logL chain of every rung (untempered values) [nkeep, T, nwalkers]
    cube                  the kept chain of the cold rung (beta[0]) in cube coordinates [nkeep, nwalkers, ndim]
    accept_frac           accepted proposals per rung over the nsteps iterations after burn-in, / (nsteps x walkers) [T]
    swap_frac             accepted swaps of the pair (t, t + 1) / swaps drawn for it after burn-in [T - 1] (NaN: none drawn)
    naccept, nswap        the counts behind them, per position [T, nwalkers] and [T - 1, nwalkers]
    status                0, or -1 for a position whose start lay outside the cube or had a NaN (it never moved nor swapped)
                          [T, nwalkers]
    last                  the walkers after the last iteration [T, nwalkers, ndim] (continue with first_iter = burn + nsteps)
    ln_prior_mass         None, or under a Gaussian prior ln of the integral of its factors over the cube (`ln_prior_mass`):
                          the ladder then measures Z(1) / Z(0) with Z(0) this mass, and both evidence routes add it, so that
                          they report ln of the integral of L g over the cube, as nested sampling of L g does
    nwalkers, nsteps, burn, thin, swap_every, seed"""

    ln_prior_mass = None

    def __init__(self, loglike_cube, **kw):
        self._loglike_cube = loglike_cube
        self.__dict__.update(kw)

    def cold(self):
        """The beta[0] rung as an `ensemble.EnsembleResult`; its theta comes from one `loglike_cube` pass over the kept cold
        rows alone.  Its `flat()` goes into `write_equal_weights`, `model_band_batch` and `eqw_batch`."""
        from .ensemble import _kept_rows                    # (the book-keeping the two drivers share lives in `ensemble`)
        n = self.cube.shape[1]
        theta, extra = _kept_rows(self._loglike_cube, self.cube)
        return EnsembleResult(cube=self.cube, theta=theta, **extra, logL=np.ascontiguousarray(self.logL[:, 0, :]), accept_frac=self.naccept[0] / max(self.nsteps, 1),
                              status=self.status[0], last=self.last[0], nwalkers=n, nsteps=self.nsteps, burn=self.burn, thin=self.thin, seed=self.seed)

    def _rung(self, t, lo=0, hi=None):
        """The kept logL of rung t over the slots [lo, hi) and the positions of status 0, flattened."""
        return self.logL[lo:hi, t, self.status[t] == 0].reshape(-1)

    def _plus_prior_mass(self, lnZ):
        """ln Z of the ladder plus ln Z(0): under a Gaussian prior Z(0) is its mass over the cube, a constant; None adds
        nothing (the value goes through untouched, not as lnZ + 0.0)."""
        return lnZ if self.ln_prior_mass is None else lnZ + self.ln_prior_mass

    def _stepping_stone(self, lo=0, hi=None):
        total = 0.0
        for t in range(self.betas.size - 1):
            L = self._rung(t + 1, lo, hi)
            total += np.logaddexp.reduce((self.betas[t] - self.betas[t + 1]) * L) - np.log(L.size)      # (logL -inf: a weight of 0)
        return float(total)

    def logZ_stepping_stone(self, nbatch=20):
        """(ln Z, standard error) by stepping stones: ln Z = sum_t ln < exp((beta_t - beta_{t+1}) logL) > over the kept samples
        of rung t + 1 (every ratio Z(beta_t) / Z(beta_{t+1}) by importance sampling from the hotter rung).  The error is the
        standard deviation (ddof 1) of the same estimator over `nbatch` consecutive batches of the chain, / sqrt(nbatch).  Z is
        the evidence under the flat prior of the cube, so the ladder has to end at beta = 0."""
        if self.betas[-1] != 0.0:
            raise ValueError(f"the stepping stones need a ladder that ends at beta = 0 (the prior), got {self.betas[-1]}")
        nbatch = int(nbatch)
        size = self.logL.shape[0] // nbatch
        if nbatch < 2 or size < 1:
            raise ValueError(f"{self.logL.shape[0]} kept iterations cannot be cut into {nbatch} batches")
        parts = np.array([self._stepping_stone(b * size, (b + 1) * size) for b in range(nbatch)])
        return self._plus_prior_mass(self._stepping_stone()), float(parts.std(ddof=1) / np.sqrt(nbatch))

    def logZ_ti(self):
        """ln Z by thermodynamic integration: the trapezoid rule over < logL >_beta on the ladder's nodes.  Its bias is the
        rule's: large where < logL > bends between two rungs, as it does towards beta = 0."""
        if self.betas[-1] != 0.0:
            raise ValueError(f"thermodynamic integration needs a ladder that ends at beta = 0 (the prior), got {self.betas[-1]}")
        mean = np.array([self._rung(t).mean() for t in range(self.betas.size)])
        return self._plus_prior_mass(float((0.5 * (mean[:-1] + mean[1:]) * (self.betas[:-1] - self.betas[1:])).sum()))


def swap_rounds(first_iter, nsteps, swap_every, ntemps):
    """How many of the swap rounds of the iterations [first_iter, first_iter + nsteps) draw the pair (t, t + 1) [ntemps - 1]:
    round r = (g + 1) / swap_every - 1 follows every global iteration g with (g + 1) mod swap_every == 0 and draws the pairs
    with t = r mod 2."""
    drawn = np.zeros(max(ntemps - 1, 0), dtype=np.int64)
    if swap_every > 0 and ntemps > 1:
        r0, r1 = first_iter // swap_every, (first_iter + nsteps) // swap_every      # the rounds [r0, r1)
        even = (r1 + 1) // 2 - (r0 + 1) // 2
        drawn[0::2], drawn[1::2] = even, (r1 - r0) - even
    return drawn


def tempered_sample(loglike_cube, advance, ndim, nwalkers, nsteps, betas, burn=0, thin=1, swap_every=1, start=None, ball=None, seed=0):
    """`burn` + `nsteps` iterations of len(betas) temperatures of `nwalkers` walkers each (even, >= 4); see the module's text.
    `seed` seeds the host generator of the starts and is handed to `advance`."""
    ndim, n, nsteps, burn, thin, swap_every = int(ndim), int(nwalkers), int(nsteps), int(burn), int(thin), int(swap_every)
    betas = np.array(betas, dtype=float).reshape(-1)
    T = betas.size
    from .ensemble import _check_run, _draw_starts
    _check_run(n, nsteps, burn, thin, swap_every)
    if T < 1 or not np.isfinite(betas).all() or (betas < 0.0).any() or (np.diff(betas) >= 0.0).any():
        raise ValueError(f"betas must be finite, >= 0 and strictly decreasing, got {betas}")
    U = _draw_starts(seed, (T, n, ndim), start, ball)
    if burn:
        U = advance(U, burn, thin=1, swap_every=swap_every, seed=seed, first_iter=0, chain=False, chain_temps=0)[0]
    U, _, _, status, naccept, nswap, CU, CL = advance(np.ascontiguousarray(U), nsteps, thin=thin, swap_every=swap_every, seed=seed, first_iter=burn,
                                                      chain=True, chain_temps=1)
    nkeep = nsteps // thin
    naccept, nswap = np.asarray(naccept).reshape(T, n), np.asarray(nswap).reshape(max(T - 1, 0), n)
    drawn = swap_rounds(burn, nsteps, swap_every, T) * n
    with np.errstate(invalid="ignore", divide="ignore"):
        swap_frac = nswap.sum(axis=1) / drawn
    return TemperedResult(loglike_cube, betas=betas, logL=np.asarray(CL, dtype=float).reshape(nkeep, T, n),
                          cube=np.asarray(CU, dtype=float).reshape(nkeep, n, ndim), accept_frac=naccept.sum(axis=1) / (max(nsteps, 1) * n),
                          swap_frac=swap_frac, naccept=naccept, nswap=nswap, status=np.asarray(status).reshape(T, n),
                          last=np.asarray(U).reshape(T, n, ndim), nwalkers=n, nsteps=nsteps, burn=burn, thin=thin, swap_every=swap_every, seed=seed)
