"""Chain diagnostics on the device, and an ensemble run that stops on them: `mcalf_chain_stats` and `mcalf_ensemble_converge`
(include/mcalf_hip.h; HIP kernels) for an `als_fitter`.  Functions of a fitter, not methods: the surface of
`als_fitter` is the reference's plus what tests/golden/python_api.json records.

    from mcalf_amd import convergence
    st = convergence.chain_stats(fit, res.cube, status=res.status)        # ChainStats(mean, var, tau, tau_mean, rhat, ess, ...)
    res = convergence.ensemble_sample_until(fit, nwalkers=256, max_steps=20000, burn=500, start=u_best, ball=0.05)
    res.converged, res.nsteps, res.tau, res.rhat, res.ess                 # an ensemble.EnsembleResult with these on top
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from .ensemble import EnsembleResult, _check_run, _draw_starts, _kept_rows

# what chain_stats returns, per coordinate [d]: the pooled mean and variance, the walker-averaged and the ensemble-mean
# autocorrelation times (kept steps), split R-hat, the effective sample size, the two windows M, the walkers that are not constant,
# whether the two windows were reached [d, 2] (bool), and the walker-averaged ACF [d, L + 1] (None unless asked for)
ChainStats = collections.namedtuple("ChainStats", "mean var tau tau_mean rhat ess window window_mean nused reached acf")


def _stats(stats, info, acf=None):
    stats, info = stats.reshape(-1, 6), info.reshape(-1, 4)
    reached = np.stack([(info[:, 3] & 1) != 0, (info[:, 3] & 2) != 0], axis=1)
    return ChainStats(*(stats[:, j] for j in range(6)), info[:, 0], info[:, 1], info[:, 2], reached, acf)


def chain_stats(fit, chain, status=None, c=5.0, max_lag=None, acf=False):
    """Convergence diagnostics of `chain` [T, n, d] (T kept steps of n walkers; d is the chain's own width: cube rows, theta rows
    or derived quantities) per coordinate, on the device (`mcalf_chain_stats`; HIP kernels): `ChainStats(mean, var, tau,
    tau_mean, rhat, ess, window, window_mean, nused, reached, acf)`.

    `tau` is the integrated autocorrelation time of the walker-averaged autocorrelation function -- every walker's own
    normalised ACF (biased sums about the walker's mean, lags 0 .. L), averaged over the walkers that are not constant in the
    coordinate (`nused` of them) -- under Sokal's window: the smallest M with M >= c tau(M) (`window`; `reached[:, 0]` False and
    M = L where there is none).  `tau_mean` is the same rule on the one series of ensemble means, what
    `EnsembleResult.autocorr_time()` computes on the host; both are in kept steps (multiply by `thin`).  `rhat` is split R-hat
    over the 2 n half chains, `ess` = n T / tau, `mean` and `var` are pooled over all T n values.  Walkers whose `status` is not
    0 take no part (None: all do).  `max_lag` (None: T - 1) bounds the lags; `acf=True` returns the ACF too.  A coordinate in
    which every walker is constant has tau, tau_mean, rhat and ess NaN and nused 0; a NaN in a coordinate makes that
    coordinate NaN and no other.  T >= 4."""
    X = np.ascontiguousarray(chain, dtype=float)
    if X.ndim != 3:
        raise ValueError(f"chain must be [T, nwalkers, d], got shape {X.shape}")
    T, n, d = X.shape
    st = None if status is None else np.ascontiguousarray(status, dtype=np.int32).reshape(-1)
    if st is not None and st.size != n:
        raise ValueError(f"status must have one entry per walker ({n}), got {st.size}")
    opts = _lib.mcalf_chain_opts(float(c), 0 if max_lag is None else int(max_lag))
    L = T - 1 if max_lag is None else int(max_lag)
    stats, info = np.empty((d, 6)), np.empty((d, 4), dtype=np.int32)
    rho = np.empty((d, max(L, 0) + 1)) if acf else None
    fit._call(fit._lib.mcalf_chain_stats, fit._ptr(X), T, n, d, fit._optr(st), C.addressof(opts), fit._ptr(stats), fit._ptr(info), fit._optr(rho))
    return _stats(stats, info, rho)


def _ensemble_converge(fit, U0, max_steps, thin=1, check_every=600, factor=50.0, rtol=0.01, c=5.0, move="stretch", scale=None, seed=0,
                      first_iter=0):
    """(U, theta, logL, status, naccept, chainU, chainL, nkept, converged, tau_history, ChainStats): `ensemble_batch` from the
    walkers U0 in blocks of `check_every` kept steps, with a convergence check on the device chain behind each, for at most
    `max_steps` iterations (`mcalf_ensemble_converge`).  The arrays are `ensemble_batch(U0, nkept * thin, ...)`'s bit for bit,
    the chain cut to its `nkept` slots; tau_history [nchecks, ndim] holds the tau of every check, in kept steps."""
    U0 = fit._rows(U0, fit.ndim)
    n = U0.shape[0]
    opts = _lib.mcalf_ens_opts()
    U, theta, logL, status, naccept, CU, CL = fit._walker_setup(opts, U0, max_steps, thin, move, scale, seed, first_iter, True)
    conv = _lib.mcalf_converge_opts(int(check_every), 0, float(factor), float(rtol), float(c))
    nkeep = CU.shape[0]
    hist = np.full((-(-nkeep // max(int(check_every), 1)), fit.ndim), np.nan)
    stats, info = np.zeros((fit.ndim, 6)), np.zeros((fit.ndim, 4), dtype=np.int32)
    nkept, converged, nchecks = C.c_int64(0), C.c_int32(0), C.c_int32(0)
    p = fit._ptr
    fit._call(fit._lib.mcalf_ensemble_converge, p(U0), n, C.addressof(opts), C.addressof(conv), p(U), p(theta), p(logL), p(status), p(naccept),
              p(CU), p(CL), C.addressof(nkept), C.addressof(converged), C.addressof(nchecks), p(hist), p(stats), p(info))
    k = int(nkept.value)
    return U, theta, logL, status, naccept, CU[:k], CL[:k], k, bool(converged.value), hist[:nchecks.value], _stats(stats, info)


def ensemble_sample_until(fit, nwalkers, max_steps, burn=0, thin=1, check_every=600, factor=50.0, rtol=0.01, c=5.0, start=None, ball=None,
                          seed=0, move="stretch", scale=None):
    """`fit.ensemble_sample` that stops when its chain has converged: the starts and the burn-in are `ensemble_sample`'s, then
    ONE `mcalf_ensemble_converge` call runs blocks of `check_every` kept steps and checks the chain so far on the device after
    each, for `max_steps` iterations at the most.  A check converges when, in every coordinate that is not frozen, the
    walker-averaged autocorrelation time tau has its Sokal window (constant `c`), the chain holds T >= `factor` tau kept
    steps, and tau moved by at most `rtol` tau since the check before.  A check reads the whole chain so far, so its cost grows
    with the chain: at 4096 walkers x 47 coordinates it reaches that of 100 iterations when the chain fills its 4 GiB, and
    `check_every=600` is what keeps all the checks of such a run under a tenth of it; a small problem can check
    far more often.

    Blocks end on kept steps: the `max_steps % thin` iterations behind the last kept one are never made, so a run that does not stop
    is `ensemble_sample(nwalkers, (max_steps // thin) * thin, ...)`, and its `last` continues from `first_iter = burn + nsteps`.

    Returns an `ensemble.EnsembleResult` whose chain is cut to the `nkept` steps made -- bit for bit the chain of
    `ensemble_sample(nwalkers, nkept * thin, ...)` -- with, on top: `converged`, `nsteps` (= nkept thin), `nchecks`, `tau` [ndim] (the last
    check's, in ITERATIONS: kept steps x thin), `tau_history` [nchecks, ndim] (likewise), `rhat`, `ess` and `stats` (the last
    check's `ChainStats`, in kept steps)."""
    n, max_steps, burn, thin = int(nwalkers), int(max_steps), int(burn), int(thin)
    _check_run(n, max_steps, burn, thin)
    U = _draw_starts(seed, (n, fit.ndim), start, ball)
    if burn:
        U = fit.ensemble_batch(U, burn, thin=1, move=move, scale=scale, seed=seed, first_iter=0, chain=False)[0]
    U, _, _, status, naccept, CU, CL, nkept, converged, hist, st = _ensemble_converge(
        fit, np.ascontiguousarray(U), max_steps, thin=thin, check_every=check_every, factor=factor, rtol=rtol, c=c, move=move, scale=scale,
        seed=seed, first_iter=burn)
    CU, CL = np.ascontiguousarray(CU), np.ascontiguousarray(CL)
    theta, extra = _kept_rows(fit._cube_with_prior if fit._has_gauss() else (lambda V: fit.loglike_cube_batch(V)), CU)
    nsteps = nkept * thin
    return EnsembleResult(cube=CU, theta=theta, logL=CL, **extra, accept_frac=np.asarray(naccept) / max(nsteps, 1), status=np.asarray(status),
                          last=np.asarray(U), nwalkers=n, nsteps=nsteps, burn=burn, thin=thin, seed=seed, converged=converged,
                          nchecks=hist.shape[0], tau=st.tau * thin, tau_history=hist * thin, rhat=st.rhat, ess=st.ess, stats=st)
