"""The yardstick of mcalf_eqw_batch: equivalent widths of ONE parameter vector restated in numpy from nothing but the
oracle's `voigt_tau`, `voigt_model` and `decode` (oracle/numpy_oracle.py; hires_fitter.py:331-377, :412-428, :467-491).

    Wcomp[c, l] = ( sum_pix (1 - exp(-tau_cl)) dlambda ) / (1 + z_c)        rest frame, per slot and line
    Wblend[l]   =   sum_pix (1 - exp(-sum_c tau_cl)) dlambda                observed frame, the slots together

with dlambda = insert(diff(wl), 0, diff(wl)[0]) (:485-486).  `reference_indexing=False`: slot c reads (N, z, b) at
startind + 1 + 3c for c below the active count (int() of the ncomp slot, floor with `jax`; clamped to [0, ncompmax]; a slot
that is not finite counts as 0, where the single-point callables raise); the other cells are 0.  `reference_indexing=True`:
all ncompmax slots from startind + 3c, the reference as written (:481-482).  The continuum is left out: the reference's
(cont v) / cont is v to within one rounding."""
import math

import numpy as np

from oracle import numpy_oracle as o

TOL_ABS, TOL_REL = 1e-11, 1e-9            # the bar tests/test_gpu_parity.py applies to calc_w


def active_count(prob, p, jax=False):
    slot = float(p[prob.startind])
    if not math.isfinite(slot):
        return 0
    nc = math.floor(slot) if jax else o.decode(prob, p)[2]
    return min(max(int(nc), 0), prob.ncompmax)


def dlambda(prob):
    dl = np.diff(prob.wl)
    return np.insert(dl, 0, dl[0])


def eqw(prob, p, reference_indexing=False, jax=False):
    """(Wcomp[ncompmax, nlines], Wblend[nlines]) of one row."""
    p = np.asarray(p, dtype=float)
    if reference_indexing:
        nc, first = prob.ncompmax, prob.startind
    else:
        nc, first = active_count(prob, p, jax), prob.startind + 1
    dl = dlambda(prob)
    wcomp = np.zeros((prob.ncompmax, prob.numlines))
    tau = np.zeros((prob.numlines, prob.wl.size))
    with np.errstate(all="ignore"):
        for c in range(nc):
            N, z, b = p[first + 3 * c: first + 3 * c + 3]
            for l, (wrest, f, gam) in enumerate(prob.lines):
                wcomp[c, l] = np.sum((1 - o.voigt_model(prob.wl, N, b, z, wrest, f, gam)) * dl) / (1 + z)
                tau[l] += o.voigt_tau(prob.wl / 1e8, N, z, b * 1e5, wrest / 1e8, f, gam)
        wblend = np.sum((1 - np.exp(-tau)) * dl, axis=1)
    return wcomp, wblend


def eqw_rows(prob, P, reference_indexing=False, jax=False):
    both = [eqw(prob, p, reference_indexing, jax) for p in np.atleast_2d(P)]
    return np.array([w for w, _ in both]), np.array([w for _, w in both])


def close(got, want):
    """Every cell within the bar; NaN and infinities must sit in the same cells with the same sign."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    fin = np.isfinite(want)
    if not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    if not np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]):
        return False
    return bool(np.all(np.abs(got[fin] - want[fin]) <= TOL_ABS + TOL_REL * np.abs(want[fin])))


def worst(got, want):
    """Largest |got - want| / bar over the finite cells (for the figures a test prints)."""
    fin = np.isfinite(want) & np.isfinite(got)
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(got[fin] - want[fin]) / (TOL_ABS + TOL_REL * np.abs(want[fin]))))
