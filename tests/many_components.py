"""A problem family with an exact ndim, for the kernels in which ONE wave64 owns a row and lane k owns the coordinates
k, k + 64, k + 128, ... (the fit: fit_kernels.hip; the slice sampler: ns_kernels.hip): ndim = startind + 1 + 3 ncompmax +
3 nfill, with startind 0 (resolution and continuum fixed), 1 (resolution free) or 2 (both free), so that every ndim is
reachable and the boundaries 63 / 64 / 65 and 127 / 128 / 129 of the lane ownership can be placed exactly.

`many(ndim)`: one line (CIV 1548), ncompmax components 0.0013 apart in z from z = 3 (about 97 km/s), logN uniform in
13.2 .. 13.6 and b uniform in 14 .. 26 km/s, box N [12.5, 14.5], b [8, 40], one z box that spans all components; a
logarithmic pixel grid of 4 km/s per pixel (so the LSF of 6 .. 9 km/s FWHM applies and a free resolution has a live
column), 100 km/s of continuum at either end; sigma 0.02; the data are the oracle's model of the truth plus seeded noise.
A filler (nfill = 1) is one more absorber of the filler line (250 A) at the next position of the same ladder, with
logN 14.1 (the filler's tau per column density is 6.2 times weaker).  At most 43 positions: 1068 pixels."""
import numpy as np

import fit_reference as fr
from cases import oracle_synth, problem_from_kwargs

CKMS = 2.99792458e5
WREST = fr.CIV[0][0]
Z0, DZ = 3.0, 0.0013
STEP_KMS, MARGIN_KMS = 4.0, 100.0
START_SCALE = (0.1, 5e-5, 2.0)                       # starts: truth +- (0.1 dex, 5e-5, 2 km/s), uniform
NDIMS = (63, 64, 65, 127, 128, 129, 130)


def layout(ndim, nfill=0):
    """(startind, ncompmax) of the family's problem with `ndim` parameters and `nfill` fillers."""
    rem = ndim - 1 - 3 * nfill
    assert rem >= 3
    return rem % 3, rem // 3


def many(ndim, nfill=0, seed=0, brange=(8.0, 40.0), b_truth=None):
    """(kwargs, truth).  `b_truth` {component: b} overrides the Doppler parameter the DATA are made with (it may lie
    outside `brange`: the truth vector then holds a b the box excludes)."""
    startind, ncompmax = layout(ndim, nfill)
    rng = np.random.default_rng(seed)
    npos = ncompmax + nfill
    zpos = Z0 + DZ * np.arange(npos)
    first = WREST * (1.0 + zpos[0]) * np.exp(-MARGIN_KMS / CKMS)
    last = WREST * (1.0 + zpos[-1]) * np.exp(MARGIN_KMS / CKMS)
    npix = int(np.ceil(np.log(last / first) * CKMS / STEP_KMS)) + 1
    wl = first * np.exp(np.arange(npix) * STEP_KMS / CKMS)
    err = np.full(npix, 0.02)
    kw = dict(fitrange=[[wl[0] - 0.01, wl[-1] + 0.01]], fitlines=["CIV 1548"], linepars=fr.CIV[:1], ncomp=[1, ncompmax], nfill=nfill,
              specres=[6.0, 9.0] if startind >= 1 else [8.0], contval=[0.9, 1.1] if startind == 2 else [1.0],
              Nrange=[12.5, 14.5], brange=list(brange), zrange=[Z0 - 0.5 * DZ, zpos[ncompmax - 1] + 0.5 * DZ],
              Nrangefill=[12.5, 14.5], brangefill=[8.0, 40.0], velstep=STEP_KMS, spectrum=(wl, np.ones(npix), err))
    truth = np.zeros(ndim)
    if startind >= 1:
        truth[0] = 7.5
    if startind == 2:
        truth[1] = 1.0
    truth[startind] = float(ncompmax)
    comps = np.column_stack([rng.uniform(13.2, 13.6, ncompmax), zpos[:ncompmax], rng.uniform(14.0, 26.0, ncompmax)])
    for c, b in (b_truth or {}).items():
        comps[c, 2] = b
    truth[startind + 1:startind + 1 + 3 * ncompmax] = comps.ravel()
    if nfill:
        zf = WREST * (1.0 + zpos[ncompmax:]) / 250.0 - 1.0
        truth[startind + 1 + 3 * ncompmax:] = np.column_stack([np.full(nfill, 14.1), zf, np.full(nfill, 20.0)]).ravel()
    flux = oracle_synth(kw, truth) + rng.normal(0.0, 0.02, npix)
    kw = dict(kw, spectrum=(wl, flux, err))
    prob = problem_from_kwargs(kw)
    assert (prob.ndim, prob.startind, prob.ncompmax) == (ndim, startind, ncompmax) and prob.wl.size == npix <= 1100
    return kw, truth


def start_scales(kw, truth):
    """The half-widths of the starts per coordinate: (0.1 dex, 5e-5, 2 km/s) per absorber (a filler's z scaled to the same
    velocity), 0.3 km/s on a free resolution, 0.01 on a free continuum, 0 on the ncomp slot."""
    prob = problem_from_kwargs(kw)
    w = np.zeros(prob.ndim)
    if prob.startind >= 1:
        w[0] = 0.3
    if prob.startind == 2:
        w[1] = 0.01
    w[prob.startind + 1:] = np.tile(START_SCALE, prob.ncompmax + prob.nfill)
    zf = np.arange(prob.endind + 1, prob.ndim, 3)
    w[zf] *= (1.0 + truth[zf]) / (1.0 + Z0)
    return w


def starts(kw, truth, n, seed):
    """`n` rows: the truth plus uniform offsets within `start_scales`."""
    return truth + np.random.default_rng(seed).uniform(-1.0, 1.0, (n, truth.size)) * start_scales(kw, truth)


def cg_iters(ndim):
    """CG iterations per outer iteration of the convergence cases.  With the resolution fixed the default (None: ndim) is
    enough.  With it free, R and the b of every component are nearly degenerate at 4 km/s pixels (both widen the lines): the
    system is too ill-conditioned for ndim iterations of CG, the numpy restatement then gains ~1e-2 of logL per outer
    iteration for as long as it runs (status 0 after 15), while with 4 ndim iterations it converges in 6 or 7
    (tests/test_many_components_reference.py)."""
    return 4 * ndim if layout(ndim)[0] >= 1 else None


# ---- the sampler's hand-built chords ---------------------------------------------------------------------------------------

def few_pixels(ndim, npix=64, seed=0):
    """kwargs of the same layout as `many(ndim)` on a 64-pixel spectrum of noise: what the sampler's long unconstrained
    chains need of a likelihood is that it is finite."""
    startind, ncompmax = layout(ndim)
    rng = np.random.default_rng(seed)
    wl = WREST * (1.0 + Z0) * np.exp(np.arange(npix) * STEP_KMS / CKMS)
    z0 = wl[npix // 2] / WREST - 1.0
    return dict(fitrange=[[wl[0] - 0.01, wl[-1] + 0.01]], fitlines=["CIV 1548"], linepars=fr.CIV[:1], ncomp=[1, ncompmax], nfill=0,
                specres=[6.0, 9.0] if startind >= 1 else [8.0], contval=[0.9, 1.1] if startind == 2 else [1.0], Nrange=[12.5, 14.5],
                brange=[8.0, 40.0], zrange=[z0 - 1e-3, z0 + 1e-3], velstep=STEP_KMS,
                spectrum=(wl, 1.0 + rng.normal(0.0, 0.03, npix), rng.uniform(0.01, 0.05, npix)))


def binding(x, d):
    """(index that sets tl, index that sets tr) of the chord of x + t d through the unit cube, by the rule of
    ns_reference.chord: the argmax of min(a, b) and the argmin of max(a, b) over the coordinates with d != 0."""
    nz = d != 0.0
    safe = np.where(nz, d, 1.0)
    a, b = (0.0 - x) / safe, (1.0 - x) / safe
    return int(np.argmax(np.where(nz, np.minimum(a, b), -np.inf))), int(np.argmin(np.where(nz, np.maximum(a, b), np.inf)))


def chord_cases(ndim, seed=5):
    """Hand-built (name, start x, direction d, index setting tl, index setting tr) whose chord is set by a coordinate >= 64;
    an index is None where the case does not fix it.  tests/test_many_components_reference.py asserts the indices with
    `binding` and ns_reference.chord on the CPU."""
    assert ndim >= 65
    rng = np.random.default_rng(seed)
    late = [64] + ([127, 128] if ndim >= 129 else [ndim - 1] if ndim > 65 else [])
    cases = []
    x = rng.uniform(0.2, 0.8, ndim)
    d = np.zeros(ndim)
    d[64:] = rng.uniform(0.5, 1.0, ndim - 64) * rng.choice([-1.0, 1.0], ndim - 64)
    cases.append(("only_late_entries", x, d, "late", "late"))
    for k in late:                                                     # a unit vector of a late coordinate
        cases.append((f"unit_{k}", rng.uniform(0.2, 0.8, ndim), np.eye(ndim)[k], k, k))
    dense = rng.uniform(0.5, 1.0, ndim)                                # all positive: tr from a coordinate near 1, tl from one near 0
    for k in late:
        k2 = late[(late.index(k) + 1) % len(late)] if len(late) > 1 else None
        x = np.full(ndim, 0.5)
        x[k] = 0.999
        if k2 is not None:
            x[k2] = 0.001
        cases.append((f"dense_hi_{k}", x, dense, k2, k))
        x = np.full(ndim, 0.5)                                         # on the face itself, the direction pointing outward
        x[k] = 1.0
        cases.append((f"on_face_1_of_{k}", x, dense, None, k))
        x = np.full(ndim, 0.5)
        x[k] = 0.0
        cases.append((f"on_face_0_of_{k}", x, -dense, None, k))
    return cases
