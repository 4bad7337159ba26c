"""Hamiltonian Monte Carlo for an `als_fitter`, driven by the analytic gradient of logL on the device: the batched walker step
`mcalf_hmc_batch` (include/mcalf_hip.h; HIP kernels) and a host driver that adapts its step size and its
per-coordinate scales during burn-in.  Functions of a fitter, not methods: the surface of `als_fitter` is the reference's plus
what tests/golden/python_api.json records.

    from mcalf_amd import hmc
    res = hmc.hmc_sample(fit, nwalkers=256, nsteps=2000, burn=500, start=u_best, ball=0.05)   # an ensemble.EnsembleResult
    U, theta, logL, status, naccept, ndead, CU, CL = hmc.hmc_batch(fit, U0, 100, eps=0.2, nleap=8, scale=s)

The walkers are independent chains; a walker keeps its component count (the ncomp slot is frozen: moves that change the count
belong to the ensemble and the nested samplers), and different walkers may hold different counts.

`sample_with` keeps the books of a run in numpy, the likelihood work behind two callables:

    loglike_cube(U) -> (theta, logL[, lnprior])            as `ensemble.ensemble_sample` takes it
    advance(U0, nsteps, eps, scale, thin, seed, first_iter, chain)
        -> (U, theta, logL, status, naccept, ndead, chainU, chainL)

`hmc_sample` passes the fitter's own entries; the tests drive the same loop with the numpy restatement of the step.  This module
imports nothing of the package but `ensemble`, which is pure numpy as well."""
from __future__ import annotations

import numpy as np

from .ensemble import EnsembleResult, _draw_starts, _kept_rows


def hmc_batch(fit, U0, nsteps, eps, nleap, scale=None, jitter=0.1, thin=1, seed=0, first_iter=0, walker_ids=None, chain=True):
    """(U, theta, logL, status, naccept, ndead, chainU, chainL): `nsteps` iterations of Hamiltonian Monte Carlo on the device
    (`mcalf_hmc_batch`; HIP kernels) for the independent walkers U0 (unit cube, [nwalkers, ndim]).  An iteration draws a
    momentum per coordinate, makes `nleap` leapfrog steps of size eps (1 + jitter (2 xi - 1)) scale[k] in coordinate k --
    reflected at the cube's walls, one gradient launch over all walkers per step -- and accepts or rejects the end point.
    `scale` [ndim] is a length per coordinate in cube units (None: 1 everywhere); scale[k] == 0 freezes coordinate k.  The
    ncomp slot and coordinates whose prior has no width are always frozen: HMC samples WITHIN a walker's component count, and
    different walkers may hold different counts.  The target is `loglike_cube_batch`'s logL, plus lnprior under a Gaussian
    prior (`Gpriors`, `set_gauss_prior`), whose gradient joins the likelihood's; logL and chainL stay the likelihood's.

    theta holds the transformed rows of U and logL[i] is `loglike_cube_batch(U)[i]` bit for bit.  status: 0, or -1 for a walker
    whose start lies outside the cube or has a NaN, whose logL is not finite (the asymmetric veto) or whose gradient is not (it
    never moves and comes back as given).  naccept: accepted trajectories per walker.  ndead: trajectories that left the cube
    after their one reflection or met a logL or gradient that is not finite; they are rejected.  chainU [nsteps // thin,
    nwalkers, ndim] and chainL [nsteps // thin, nwalkers] hold the state after every thin-th iteration (`chain=False`: None,
    None).  The random words are Philox4x64-10 of (iteration, coordinate, walker id, seed), the ids `walker_ids` (None:
    arange; distinct): a walker's results depend on its start, its id and the options alone, and calling again with the
    returned U and `first_iter` advanced by `nsteps` is, bit for bit, the longer call."""
    import ctypes as C

    from . import _lib
    U0 = fit._rows(U0, fit.ndim)
    n = U0.shape[0]
    scale = np.ones(fit.ndim) if scale is None else np.ascontiguousarray(scale, dtype=float).reshape(-1)
    if scale.size != fit.ndim:
        raise ValueError(f"scale must have ndim = {fit.ndim} entries, got {scale.size}")
    wid = None if walker_ids is None else np.ascontiguousarray(walker_ids, dtype=np.uint64).reshape(-1)
    if wid is not None and wid.size != n:
        raise ValueError(f"walker_ids must have one entry per walker ({n}), got {wid.size}")
    nsteps, thin = int(nsteps), int(thin)
    fit._ensure_prior()
    mask = 0xFFFFFFFFFFFFFFFF
    opts = _lib.mcalf_hmc_opts(nsteps, thin, int(nleap), 0, float(eps), float(jitter), int(seed) & mask, int(first_iter) & mask)
    U, theta, logL = np.empty_like(U0), np.empty_like(U0), np.empty(n)
    status, naccept, ndead = (np.empty(n, dtype=np.int32) for _ in range(3))
    nkeep = nsteps // thin if nsteps >= 0 and thin >= 1 else 0
    CU, CL = (np.empty((nkeep, n, fit.ndim)), np.empty((nkeep, n))) if chain else (None, None)
    p, o = fit._ptr, fit._optr
    fit._call(fit._lib.mcalf_hmc_batch, p(U0), n, p(scale), o(wid), C.addressof(opts), p(U), p(theta), p(logL), p(status), p(naccept),
              p(ndead), o(CU), o(CL))
    return U, theta, logL, status, naccept, ndead, CU, CL


def _windows(burn, windows):
    """The burn-in cut into at most `windows` windows of equal length, the last one taking the remainder."""
    k = max(1, min(int(windows), burn))
    size = burn // k
    return [size] * (k - 1) + [burn - size * (k - 1)]


def sample_with(loglike_cube, advance, ndim, nwalkers, nsteps, burn=0, thin=1, start=None, ball=None, seed=0, eps=0.1, scale=None,
                target=0.8, windows=5, gain=1.5):
    """`burn` + `nsteps` iterations of `nwalkers` independent HMC walkers; see the module's text for the two callables.

    The walkers start as `ensemble.ensemble_sample`'s do: uniformly in the cube, or in a ball of half-width `ball` around the
    cube point `start`.  The burn-in is cut into `windows` windows.  `scale` (None: the spread of the starts) and `eps` are
    what the first window runs under; after every window
        eps   <- eps exp(gain / (1 + w) * d), w = 0, 1, ... the window, d = (a - target) / (1 - target) for an accepted fraction
                 a (over the walkers of status 0) above the target and (a - target) / target below it: d is in [-1, 1], the
                 first window may change eps by e^gain either way, and the later ones settle, and
        scale <- the standard deviation of those walkers per coordinate (a coordinate whose spread is 0 or not finite keeps
                 its scale),
    so that eps ends as a step in units of the posterior's width.  Both are frozen before the kept run, which is ONE call:
    the chain it keeps is a chain of one kernel.  Every call continues the one before (`first_iter`), all of it deterministic
    numpy: the same arguments give the same bytes.  Returns an `ensemble.EnsembleResult` that also carries `eps`, `scale`,
    `window_accept` (the accepted fraction of every burn-in window), `window_eps` (the step each ran under) and `ndead`
    (dead trajectories per walker in the kept run)."""
    ndim, n, nsteps, burn, thin = int(ndim), int(nwalkers), int(nsteps), int(burn), int(thin)
    if n < 2:
        raise ValueError(f"nwalkers must be >= 2 (the scales come from the walkers' spread), got {n}")
    if nsteps < 0 or burn < 0 or thin < 1:
        raise ValueError(f"nsteps and burn must be >= 0 and thin >= 1, got {nsteps}, {burn}, {thin}")
    if not (0.0 < target < 1.0) or not eps > 0.0:
        raise ValueError(f"target must be in (0, 1) and eps > 0, got {target}, {eps}")
    U = _draw_starts(seed, (n, ndim), start, ball)
    eps = float(eps)

    def spread(U, ok, old):
        sd = U[ok].std(axis=0) if ok.sum() >= 2 else np.zeros(ndim)
        return np.where(np.isfinite(sd) & (sd > 0.0), sd, old)

    scale = spread(U, np.isfinite(U).all(axis=1), np.ones(ndim)) if scale is None else np.array(scale, dtype=float).reshape(ndim)
    window_accept, window_eps, done = [], [], 0
    for length in (_windows(burn, windows) if burn else []):
        U, _, _, status, naccept, _, _, _ = advance(np.ascontiguousarray(U), length, eps, scale, thin=1, seed=seed, first_iter=done, chain=False)
        done += length
        ok = np.asarray(status) == 0
        frac = float(np.asarray(naccept)[ok].sum()) / max(int(ok.sum()) * length, 1)
        window_accept.append(frac)
        window_eps.append(eps)
        miss = (frac - target) / (1.0 - target if frac > target else target)
        eps = eps * float(np.exp(gain / len(window_eps) * miss))            # (len(window_eps) is 1 + w here)
        scale = spread(np.asarray(U), ok, scale)
    U, _, _, status, naccept, ndead, CU, CL = advance(np.ascontiguousarray(U), nsteps, eps, scale, thin=thin, seed=seed, first_iter=burn, chain=True)
    nkeep = nsteps // thin
    CU, CL = np.asarray(CU, dtype=float).reshape(nkeep, n, ndim), np.asarray(CL, dtype=float).reshape(nkeep, n)
    theta, extra = _kept_rows(loglike_cube, CU)
    return EnsembleResult(cube=CU, theta=theta, logL=CL, **extra, accept_frac=np.asarray(naccept) / max(nsteps, 1), status=np.asarray(status),
                          last=np.asarray(U), nwalkers=n, nsteps=nsteps, burn=burn, thin=thin, seed=seed, eps=eps, scale=scale,
                          window_accept=np.array(window_accept), window_eps=np.array(window_eps), ndead=np.asarray(ndead))


def hmc_sample(fit, nwalkers, nsteps, burn=0, thin=1, start=None, ball=None, seed=0, eps=0.1, nleap=8, jitter=0.1, scale=None, target=0.8,
               windows=5):
    """Hamiltonian Monte Carlo of this problem's posterior with the device's own entries: `hmc_batch` for every burn-in window
    and for the kept run, `loglike_cube_batch` for the transformed rows of the kept chain (`sample_with` keeps the books and
    adapts `eps` and `scale` during burn-in).  The walkers start uniformly in the cube, or in a ball of half-width `ball`
    around the cube point `start` (e.g. a `maximize_batch` optimum mapped into the cube); each keeps the component count it
    starts with.  Returns an `ensemble.EnsembleResult` with `eps`, `scale`, `window_accept`, `window_eps` and `ndead` on top."""
    def advance(U0, nsteps, eps, scale, thin=1, seed=0, first_iter=0, chain=True):
        return hmc_batch(fit, U0, nsteps, eps, nleap, scale=scale, jitter=jitter, thin=thin, seed=seed, first_iter=first_iter, chain=chain)

    return sample_with(fit._cube_with_prior if fit._has_gauss() else (lambda U: fit.loglike_cube_batch(U)), advance, fit.ndim, nwalkers, nsteps,
                       burn=burn, thin=thin, start=start, ball=ball, seed=seed, eps=eps, scale=scale, target=target, windows=windows)
