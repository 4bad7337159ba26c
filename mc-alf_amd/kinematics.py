"""Where in wavelength a chain's absorption sits, on the MODEL's optical depth: the batched kinematics of
`mcalf_kinematics_batch` (include/mcalf_hip.h; HIP kernels) for an `als_fitter`, next to its `eqw_batch` and
`model_band_batch` in the analysis pass.  Functions of a fitter, not methods: the surface of `als_fitter` is the reference's plus
what tests/golden/python_api.json records.

    from mcalf_amd import kinematics
    kin = kinematics.kinematics_batch(fit, chain)            # Kinematics(tau_int, lam_mean, lam_rms, lam_q)
    dv90 = kinematics.dv90_batch(fit, chain)                 # km/s, Prochaska & Wolfe 1997
    zabs = kinematics.zabs_batch(fit, chain)                 # the zero point of a velocity plot
"""
from __future__ import annotations

import collections

import numpy as np

CLIGHT_KMS = 2.9979245e5                  # as the reference has it
# what kinematics_batch returns: per row and line the integral of tau dlambda, its centroid and width, and lam_q [.., len(q)]
Kinematics = collections.namedtuple("Kinematics", "tau_int lam_mean lam_rms lam_q")


def kinematics_batch(fit, P, q=(0.05, 0.5, 0.95), out=None):
    """Where in wavelength the model's absorption sits, per row and target line, on the device (HIP kernels; no spectrum
    is written to memory): `Kinematics(tau_int[batch, nlines], lam_mean[batch, nlines], lam_rms[batch, nlines],
    lam_q[batch, nlines, len(q)])`, all in Angstrom, observed frame.  `fit` is an `als_fitter`.

    With tau[k] the summed optical depth of line `l` of the row's active slots at pixel k (the slots `fit.eqw_batch` reads
    under `reference_indexing=False`; nothing convolved, no continuum, no fillers), t = tau * dlambda and S its running
    sum: `tau_int` = S[-1]; `lam_mean` the t-weighted mean wavelength; `lam_rms` the square root of the t-weighted
    variance about that mean; `lam_q[..., j]` the wavelength below which the fraction q[j] of `tau_int` lies, linear
    inside the crossing pixel's cell (q = 0.05, 0.95 bound the Delta v90 interval; `dv90_batch`).  Taken on tau, not on
    flux: a saturated core does not spoil them.  Where `tau_int` is 0 (no active slot) or not finite the other three are
    NaN; a NaN in an active slot makes that row NaN and touches no other.  A spectrum of several fit ranges has one wide
    dlambda at each gap, as `calc_w` has: the pixel after a gap weighs its tau with the gap's width.

    `q=()` leaves the quantiles out (shape [batch, nlines, 0]).  `out=(mom, lam_q)` (float64, C-contiguous, mom of shape
    [batch, nlines, 3] = tau_int, lam_mean, lam_rms; an entry may be None, not both) is filled in place and the result's
    fields are views of it (None for what was left out).  A row's bits depend on nothing but the row."""
    P = fit._rows(P, fit.ndim)
    n, nl = P.shape[0], fit.numlines
    qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=float)).reshape(-1))
    if out is None:
        mom, lamq = np.empty((n, nl, 3)), (np.empty((n, nl, qs.size)) if qs.size else None)
    else:
        mom = None if out[0] is None else fit._out(out[0], (n, nl, 3), "out[0]")
        lamq = None if out[1] is None else fit._out(out[1], (n, nl, qs.size), "out[1]")
    fit._call(fit._lib.mcalf_kinematics_batch, fit._ptr(P), n, fit._ptr(qs) if qs.size else None, qs.size,
              fit._optr(mom), fit._optr(lamq))
    if out is None and lamq is None:
        lamq = np.empty((n, nl, 0))
    m = None if mom is None else mom.reshape(n, nl, 3)
    return Kinematics(*((None,) * 3 if m is None else (m[:, :, 0], m[:, :, 1], m[:, :, 2])),
                      lamq if lamq is None or lamq.shape == (n, nl, qs.size) else lamq.reshape(n, nl, qs.size))


def _line(fit, lineid):
    lineid = int(lineid)
    if not 0 <= lineid < fit.numlines:
        raise ValueError(f"lineid must be in [0, {fit.numlines}), got {lineid}")
    return lineid


def dv90_batch(fit, P, lineid=0):
    """Delta v90 of line `lineid` for every row ([batch], km/s): c (lam_0.95 - lam_0.05) / lam_0.5 from one
    `kinematics_batch` call -- the velocity interval that holds 90 % of the line's optical depth (Prochaska & Wolfe
    1997), on the model's tau.  NaN where the row has no absorption.  `lineid` is checked as `calc_w_batch` checks it."""
    lineid = _line(fit, lineid)
    lam = kinematics_batch(fit, P, q=(0.05, 0.5, 0.95)).lam_q[:, lineid, :]
    return CLIGHT_KMS * (lam[:, 2] - lam[:, 0]) / lam[:, 1]


def zabs_batch(fit, P, lineid=0):
    """The optical-depth-weighted redshift of line `lineid` for every row ([batch]): lam_mean / wrest - 1 from one
    `kinematics_batch` call -- the zero point of a velocity plot.  NaN where the row has no absorption."""
    lineid = _line(fit, lineid)
    return kinematics_batch(fit, P, q=()).lam_mean[:, lineid] / fit.linepars[lineid]["wrest"] - 1.0
