"""The prior and sampler entries of `als_fitter`, as the one mixin it inherits: everything here needs the prior box on the
device (`_ensure_prior`) -- the Gaussian prior, lnprior, nested sampling's replacement step, the ensemble and the tempered
walker steps, and the host drivers built on them.  The mixin uses the fitter's `_call`, `_ptr`, `_optr` and `_rows`."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .. import _lib

_MOVES = {"stretch": _lib.MCALF_ENS_STRETCH, "de": _lib.MCALF_ENS_DE}       # the `move=` names of the two walker entries


def _u64(v):
    """A Python integer as the uint64 a Philox seed or iteration counter is: reduced mod 2^64, so negative values wrap."""
    return int(v) & 0xFFFFFFFFFFFFFFFF


class SamplingMixin:
    def _ensure_prior(self, int_ncomp=None):
        """The prior box on the device (`mcalf_set_prior`), sent once per ncomp flavour.  `int_ncomp=None`: any flavour
        that is already there will do (the box is the same), the PolyChord one if none is."""
        have = self._prior_key
        key = (True if have is None else have) if int_ncomp is None else bool(int_ncomp)
        if have != key:
            self._call(self._lib.mcalf_set_prior, self._ptr(self._lo), self._ptr(self._hi), int(key))
            self._prior_key = key
        if self._gauss is not None and not self._gauss_sent:
            mu, sigma = self._gauss
            self._call(self._lib.mcalf_set_gauss_prior, self._ptr(mu), self._ptr(sigma))
            self._gauss_sent = True

    def set_gauss_prior(self, mu, sigma):
        """Gaussian prior factors on top of the box (`mcalf_set_gauss_prior`): parameter k carries
        exp(-0.5 ((theta_k - mu[k]) / sigma[k])^2) / sqrt(2 pi sigma[k]^2) where sigma[k] > 0 and none where sigma[k] == 0, not
        renormalised for the truncation by the box (hires_fitter.py:230).  `lnprior_batch`, `slice_replace_batch` /
        `nested_sample`, `ensemble_batch` / `ensemble_sample` and `tempered_batch` / `tempered_sample` honour it;
        `maximize_batch` does not.  The ncomp slot cannot carry one."""
        mu = np.ascontiguousarray(mu, dtype=float).reshape(-1)
        sigma = np.ascontiguousarray(sigma, dtype=float).reshape(-1)
        if mu.size != self.ndim or sigma.size != self.ndim:
            raise ValueError(f"mu and sigma must have ndim = {self.ndim} entries, got {mu.size} and {sigma.size}")
        self._gauss = None                                   # (what the constructor parsed is superseded)
        self._ensure_prior()
        self._call(self._lib.mcalf_set_gauss_prior, self._ptr(mu), self._ptr(sigma))

    def clear_gauss_prior(self):
        """Back to the flat box: every entry runs the code path, and returns the bits, of a fitter that never had a Gaussian."""
        self._gauss = None
        self._ensure_prior()
        self._call(self._lib.mcalf_set_gauss_prior, None, None)

    @property
    def gauss_prior(self):
        """(mu, sigma, c) [ndim] as the library holds them (`mcalf_get_gauss_prior`), c[k] = ln(2 pi sigma[k]^2) as the kernels
        add it; None when no Gaussian is set."""
        self._ensure_prior()
        mu, sigma, c = (np.empty(self.ndim) for _ in range(3))
        n = C.c_int32(0)
        self._call(self._lib.mcalf_get_gauss_prior, self._ptr(mu), self._ptr(sigma), self._ptr(c), C.byref(n))
        return (mu, sigma, c) if n.value > 0 else None

    def lnprior_batch(self, rows, cube=False):
        """lnprior[i] of every row on the device (`mcalf_lnprior_batch`; a HIP kernel): -inf for a row with a NaN or an entry
        outside the box, else the sum of the Gaussian factors' logarithms (hires_fitter.py:218-234), an exact 0 without any.
        `cube=True`: the rows are unit-cube rows, mapped through the box as `loglike_cube_batch` maps them."""
        rows = self._rows(rows, self.ndim)
        self._ensure_prior()
        out = np.empty(rows.shape[0])
        self._call(self._lib.mcalf_lnprior_batch, self._ptr(rows), rows.shape[0], int(bool(cube)), self._ptr(out))
        return out

    def lnprior(self, p):
        """hires_fitter.py:218-234."""
        return float(self.lnprior_batch(np.asarray(p, dtype=float))[0])

    def _cube_posterior(self, U):
        """(theta, logL + lnprior) of unit-cube rows: the callable the host drivers start from."""
        theta, logL = self.loglike_cube_batch(U)
        return (theta, logL + self.lnprior_batch(U, cube=True)) if self._has_gauss() else (theta, logL)

    def _cube_with_prior(self, U):
        """(theta, logL, lnprior) of unit-cube rows, lnprior by one pass over the rows already transformed."""
        theta, logL = self.loglike_cube_batch(U)
        return theta, logL, self.lnprior_batch(theta)

    def _has_gauss(self):
        return self.gauss_prior is not None

    def slice_replace_batch(self, U0, Lmin, dirs, nmoves=None, max_steps=None, seed=0, stream_ids=None):
        """(U, theta, logL, status, nevals, moves): nested sampling's replacement step on the device
        (`mcalf_slice_replace_batch`; HIP kernels).  Every row of U0 (unit cube, [batch, ndim]) is a chain that makes
        `nmoves` (None: 2 ndim) slice-sampling moves along rows of `dirs` ([ndirs, ndim], shared by all rows) under the
        hard constraint logL > Lmin[row] (`Lmin`: a scalar or one value per row), in lock step for at most `max_steps`
        (None: 50 nmoves) steps of one trial per row.

        theta holds the transformed rows of U and logL[i] is `loglike_cube_batch(U)[i]` bit for bit.  status: 1 the row
        made its moves, 0 `max_steps` reached (the row holds its last accepted point, which satisfies the constraint),
        -1 the start lies outside the cube, has a NaN or does not satisfy the constraint (the row comes back as given).
        nevals: trials the row evaluated; moves: accepted ones.  The random words of a row are Philox4x64-10 of (step,
        stream_ids[row], seed) -- `stream_ids` (None: arange) must be distinct -- so a row's result does not depend on its
        batch or its position.

        Under a Gaussian prior (`Gpriors`, `set_gauss_prior`) the constrained quantity is logL + lnprior, evaluated inside the
        step's own kernels: `Lmin` bounds that sum and logL[i] is `loglike_cube_batch(U)[i] + lnprior_batch(U, cube=True)[i]`
        bit for bit."""
        U0 = self._rows(U0, self.ndim)
        n = U0.shape[0]
        dirs = self._rows(dirs, self.ndim)
        Lmin = np.ascontiguousarray(np.broadcast_to(np.asarray(Lmin, dtype=float), (n,)))
        sid = np.arange(n, dtype=np.uint64) if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.uint64).reshape(-1)
        if sid.size != n:
            raise ValueError(f"stream_ids must have one entry per row ({n}), got {sid.size}")
        nmoves = 2 * self.ndim if nmoves is None else int(nmoves)
        max_steps = 50 * nmoves if max_steps is None else int(max_steps)
        self._ensure_prior()
        opts = _lib.mcalf_slice_opts(nmoves, max_steps, dirs.shape[0], 0, _u64(seed))
        U, theta, logL = np.empty_like(U0), np.empty_like(U0), np.empty(n)
        status, nevals, moves = (np.empty(n, dtype=np.int32) for _ in range(3))
        p = self._ptr
        self._call(self._lib.mcalf_slice_replace_batch, p(U0), p(Lmin), p(dirs), p(sid), n, C.addressof(opts), p(U), p(theta), p(logL),
                   p(status), p(nevals), p(moves))
        return U, theta, logL, status, nevals, moves

    def set_slice_compact(self, on):
        """Packing of the live rows in `slice_replace_batch` (`mcalf_set_slice_compact`; off by default, MCALF_NS_COMPACT gives
        the initial value).  On: every lock step launches the likelihood over the rows that proposed a trial only, instead of
        over all rows of the call.  Results never depend on it, bit for bit; `slice_stats()` shows what it saves."""
        self._call(self._lib.mcalf_set_slice_compact, int(bool(on)))

    def slice_stats(self):
        """What the last `slice_replace_batch` call launched (`mcalf_slice_last_stats`), as a dict: `batch` its rows,
        `rows_launched` the rows handed to likelihood launches (the start launch included), `trials` the trials its rows
        proposed (the sum of nevals), `steps` the lock steps issued, `compact` whether the call packed its trial rows.
        All 0 before the first call."""
        st = _lib.mcalf_slice_stats_t()
        self._call(self._lib.mcalf_slice_last_stats, C.byref(st))
        return {name: int(getattr(st, name)) for name, _ in st._fields_}

    def nested_sample(self, nlive, batch=None, nmoves=None, dlogz=1e-3, max_rounds=100000, seed=0, max_steps=None):
        """Nested sampling of this problem's posterior with the device's own two entries: `loglike_cube_batch` for the
        initial live points and `slice_replace_batch` for every replacement round (`nested.nested_sample` keeps the books).
        Returns a `nested.NestedResult`: logZ, logZ_err, H, the dead points with their log weights, and
        `equal_weight_samples(rng)`, whose output goes into `write_equal_weights`.  Its `rows_launched` counts the rows
        handed to likelihood launches: nlive for the initial points and `slice_stats()["rows_launched"]` of every round
        (`set_slice_compact(True)` lowers it; nothing else of the result depends on that setting).  Under a Gaussian prior
        (`Gpriors`, `set_gauss_prior`) both entries work on logL + lnprior: nested sampling of L g under the box measure, so
        `logL` holds that sum, `lnprior` the prior's part, and logZ is ln of the integral of L g over the cube."""
        from .. import nested
        launched = [int(nlive)]

        def replace(U0, Lmin, dirs, nmoves, seed, stream_ids):
            out = self.slice_replace_batch(U0, Lmin, dirs, nmoves=nmoves, max_steps=max_steps, seed=seed, stream_ids=stream_ids)
            launched[0] += self.slice_stats()["rows_launched"]
            return out

        gauss = self._has_gauss()
        res = nested.nested_sample(self._cube_posterior if gauss else (lambda U: self.loglike_cube_batch(U)), replace, self.ndim, nlive, batch=batch,
                                   nmoves=nmoves, dlogz=dlogz, max_rounds=max_rounds, seed=seed)
        res.rows_launched = launched[0]
        if gauss:
            res.lnprior = self.lnprior_batch(res.cube, cube=True)
        return res

    def _walker_setup(self, opts, U0, nsteps, thin, move, scale, seed, first_iter, chain, chain_lead=None):
        """What `ensemble_batch` and `tempered_batch` share: fills the fields their option structs have in common into `opts`, sends
        the prior box, and allocates the outputs for the walkers U0 ([n, ndim] or [T, n, ndim]): (U, theta, logL, status, naccept,
        chainU, chainL).  chainL keeps a slot per walker position, chainU the positions `chain_lead` (None: all of them)."""
        if move not in _MOVES:
            raise ValueError(f"move must be 'stretch' or 'de', got {move!r}")
        if scale is None:
            scale = 2.0 if move == "stretch" else 2.38 / np.sqrt(2.0 * self.ndim)
        nsteps, thin = int(nsteps), int(thin)
        self._ensure_prior()
        opts.nsteps, opts.thin, opts.move, opts.scale, opts.seed, opts.first_iter = nsteps, thin, _MOVES[move], float(scale), _u64(seed), _u64(first_iter)
        lead = U0.shape[:-1]
        U, theta, logL = np.empty_like(U0), np.empty_like(U0), np.empty(lead)
        status, naccept = (np.empty(lead, dtype=np.int32) for _ in range(2))
        nkeep = nsteps // thin if nsteps >= 0 and thin >= 1 else 0
        CU = np.empty((nkeep,) + (lead if chain_lead is None else chain_lead) + (self.ndim,)) if chain else None
        return U, theta, logL, status, naccept, CU, (np.empty((nkeep,) + lead) if chain else None)

    def ensemble_batch(self, U0, nsteps, thin=1, move="stretch", scale=None, seed=0, first_iter=0, chain=True):
        """(U, theta, logL, status, naccept, chainU, chainL): `nsteps` iterations of an affine-invariant ensemble sampler on
        the device (`mcalf_ensemble_batch`; HIP kernels).  The rows of U0 (unit cube, [nwalkers, ndim]; nwalkers even, >= 4)
        are the walkers; the halves [0, n / 2) and [n / 2, n) move in turn, each with partners from the other.  `move`:
        "stretch" (Goodman & Weare; `scale` = a > 1, None: 2.0) or "de" (differential evolution; `scale` = g > 0, None:
        2.38 / sqrt(2 ndim)).  The target is `loglike_cube_batch`'s logL with a flat prior over the cube; the integer `ncomp`
        slot is sampled with it, since the cube transform truncates it.

        theta holds the transformed rows of U and logL[i] is `loglike_cube_batch(U)[i]` bit for bit.  status: 0, or -1 for a
        walker whose start lies outside the cube or has a NaN (it never moves and comes back as given).  naccept: accepted
        proposals per walker.  chainU [nsteps // thin, nwalkers, ndim] and chainL [nsteps // thin, nwalkers] hold the state
        after every thin-th iteration, kept on the device until the call ends (`chain=False`: None, None).  The random words
        are Philox4x64-10 of (half-step, walker, seed): calling again with the returned U and `first_iter` advanced by
        `nsteps` is, bit for bit, the longer call.

        Under a Gaussian prior (`Gpriors`, `set_gauss_prior`) the target is logL + lnprior: the accept rule gains
        lnprior(trial) - lnprior(walker), evaluated inside the step's own kernels, while logL and chainL stay the likelihood's
        (`lnprior_batch(U, cube=True)` gives the prior's part)."""
        U0 = self._rows(U0, self.ndim)
        opts = _lib.mcalf_ens_opts()
        U, theta, logL, status, naccept, CU, CL = self._walker_setup(opts, U0, nsteps, thin, move, scale, seed, first_iter, chain)
        p, o = self._ptr, self._optr
        self._call(self._lib.mcalf_ensemble_batch, p(U0), U0.shape[0], C.addressof(opts), p(U), p(theta), p(logL), p(status), p(naccept),
                   o(CU), o(CL))
        return U, theta, logL, status, naccept, CU, CL

    def ensemble_sample(self, nwalkers, nsteps, burn=0, thin=1, start=None, ball=None, seed=0, move="stretch", scale=None):
        """Ensemble MCMC of this problem's posterior with the device's own two entries: `ensemble_batch` for the burn-in and
        for the kept run (two calls, whatever their length) and `loglike_cube_batch` for the transformed rows of the kept
        chain (`ensemble.ensemble_sample` keeps the books).  The walkers start uniformly in the cube, or in a ball of
        half-width `ball` around the cube point `start` (e.g. a `maximize_batch` optimum mapped into the cube).  Returns an
        `ensemble.EnsembleResult`: the chain in cube and theta coordinates, logL, the acceptance fractions,
        `autocorr_time()`, and `flat()`, whose output goes into `write_equal_weights`, `model_band_batch` and `eqw_batch`."""
        from .. import ensemble

        def advance(U0, nsteps, thin=1, seed=0, first_iter=0, chain=True):
            return self.ensemble_batch(U0, nsteps, thin=thin, move=move, scale=scale, seed=seed, first_iter=first_iter, chain=chain)

        return ensemble.ensemble_sample(self._cube_with_prior if self._has_gauss() else (lambda U: self.loglike_cube_batch(U)), advance, self.ndim, nwalkers, nsteps, burn=burn, thin=thin,
                                        start=start, ball=ball, seed=seed)

    def tempered_batch(self, U0, betas, nsteps, thin=1, swap_every=1, move="stretch", scale=None, seed=0, first_iter=0, chain=True, chain_temps=1):
        """(U, theta, logL, status, naccept, nswap, chainU, chainL): `nsteps` iterations of the ensemble sampler of
        `ensemble_batch` at T = len(betas) temperatures at once, with swaps between neighbouring temperatures
        (`mcalf_tempered_batch`; HIP kernels).  U0 [T, nwalkers, ndim] holds the starts of every rung (unit cube; nwalkers even,
        >= 4); rung t samples logL^betas[t] (betas finite, >= 0, strictly decreasing; 1 <= T <= 64).  A half-step moves one half
        of every rung, T x nwalkers / 2 trial rows through one likelihood launch; after every global iteration g with
        (g + 1) % swap_every == 0 (0: never) every other pair of neighbouring rungs, alternating from round to round, exchanges
        walkers along a random shift, a swap costing no likelihood evaluation.

        U, theta [T, nwalkers, ndim], logL, status, naccept [T, nwalkers]: as `ensemble_batch`'s, per position; logL is always
        the untempered `loglike_cube_batch` value.  nswap [T - 1, nwalkers]: accepted swaps of position (t, w) with rung t + 1.
        chainL [nsteps // thin, T, nwalkers] keeps logL of every rung (the evidence needs them), chainU
        [nsteps // thin, chain_temps, nwalkers, ndim] the rows of the first `chain_temps` rungs (`chain=False`: None, None).
        The random words are Philox4x64-10 of (half-step or swap round, position, seed): calling again with the returned U and
        `first_iter` advanced by `nsteps` is, bit for bit, the longer call, and one rung at beta = 1 is `ensemble_batch`.

        Under a Gaussian prior (`Gpriors`, `set_gauss_prior`) rung t samples logL^betas[t] times the prior's Gaussian factors:
        the temperature acts on logL alone, the swap rule is unchanged (the prior cancels between rungs), and the rung at
        beta = 0 samples the Gaussian factors over the cube; logL and chainL stay the likelihood's."""
        U0 = np.ascontiguousarray(U0, dtype=float)
        betas = np.ascontiguousarray(betas, dtype=float).reshape(-1)
        T = betas.size
        if U0.ndim != 3 or U0.shape[0] != T or U0.shape[2] != self.ndim:
            raise ValueError(f"U0 must be [len(betas) = {T}, nwalkers, ndim = {self.ndim}], got {U0.shape}")
        n = U0.shape[1]
        chain_temps = int(chain_temps)
        opts = _lib.mcalf_pt_opts(ntemps=T, swap_every=int(swap_every), chain_temps=chain_temps)
        U, theta, logL, status, naccept, CU, CL = self._walker_setup(opts, U0, nsteps, thin, move, scale, seed, first_iter, chain,
                                                                     chain_lead=(min(max(chain_temps, 0), T), n))
        nswap = np.zeros((max(T - 1, 0), n), dtype=np.int32)
        p, o = self._ptr, self._optr
        self._call(self._lib.mcalf_tempered_batch, p(U0), n, p(betas), C.addressof(opts), p(U), p(theta), p(logL), p(status), p(naccept),
                   p(nswap), o(CU), o(CL))
        return U, theta, logL, status, naccept, nswap, CU, CL

    def tempered_sample(self, nwalkers, nsteps, ntemps=8, betas=None, burn=0, thin=1, swap_every=1, start=None, ball=None, seed=0, move="stretch",
                        scale=None):
        """Parallel tempering of this problem's posterior with the device's own two entries: `tempered_batch` for the burn-in
        and for the kept run (two calls, whatever their length) and `loglike_cube_batch` for the transformed rows of the cold
        rung (`tempering.tempered_sample` keeps the books).  `betas` (None: `tempering.default_ladder(ntemps, 1e-4)`, which
        ends at the prior) is the ladder; every rung holds `nwalkers` walkers, started uniformly in the cube or in a ball of
        half-width `ball` around the cube point `start`.  Returns a `tempering.TemperedResult`: logL of every rung, the
        acceptance and swap fractions per rung, `cold()` -- the beta[0] rung as an `ensemble.EnsembleResult` -- and the
        evidence by `logZ_stepping_stone()` and `logZ_ti()`.  Under a Gaussian prior the result carries `ln_prior_mass`, the
        ladder's Z at beta = 0, which both evidence routes add: they then report ln of the integral of L g over the cube, as
        `nested_sample` does."""
        from .. import tempering
        betas = tempering.default_ladder(ntemps, 1e-4) if betas is None else betas

        def advance(U0, nsteps, thin=1, swap_every=1, seed=0, first_iter=0, chain=True, chain_temps=1):
            return self.tempered_batch(U0, betas, nsteps, thin=thin, swap_every=swap_every, move=move, scale=scale, seed=seed, first_iter=first_iter,
                                       chain=chain, chain_temps=chain_temps)

        gauss = self._has_gauss()
        res = tempering.tempered_sample(self._cube_with_prior if gauss else (lambda U: self.loglike_cube_batch(U)), advance, self.ndim, nwalkers, nsteps, betas,
                                        burn=burn, thin=thin, swap_every=swap_every, start=start, ball=ball, seed=seed)
        if gauss:
            res.ln_prior_mass = tempering.ln_prior_mass(self._lo, self._hi, *self.gauss_prior[:2])
        return res
