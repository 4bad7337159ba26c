"""Shared helpers for the parity tests: build the oracle Problem that corresponds to a set
of als_fitter kwargs, and synthesise config spectra with the oracle."""
import numpy as np

from oracle import numpy_oracle as oracle


def problem_from_kwargs(kw):
    wl, flux, err = (np.asarray(a, dtype=float) for a in kw["spectrum"])
    if kw.get("fitrange") is not None:                 # range selection, hires_fitter.py:75-82
        ok = np.zeros(wl.size, dtype=bool)
        for lo, hi in kw["fitrange"]:
            ok |= (wl > lo) & (wl < hi)
        wl, flux, err = wl[ok], flux[ok], err[ok]
    return oracle.Problem(
        wl, flux, err, kw["linepars"], tuple(kw["ncomp"]), nfill=kw.get("nfill", 0),
        specres=kw.get("specres", [7.0]), contval=kw.get("contval", [1.0]),
        Nrange=kw.get("Nrange", [11.5, 16]), brange=kw.get("brange", [1, 30]), zrange=kw.get("zrange"),
        Nrangefill=kw.get("Nrangefill", [11.5, 16]), brangefill=kw.get("brangefill", [1, 30]),
        fitrange=kw.get("fitrange"), velstep=kw.get("velstep"))


BAD_KINDS = ("flux_nan", "err_nan", "err_zero")      # each drops the pixel's term from np.nansum (hires_fitter.py:292-294)


def with_bad_pixels(kw, idx, kind):
    """The kwargs `kw` of a finite problem with the FITTED pixels `idx` (indices after the fitrange selection, the
    library's own pixel numbering) made bad: `kind` is one of 'flux_nan', 'err_nan', 'err_zero' (the term is NaN and
    nansum drops it), 'err_neg' (squared away: a control, nothing is dropped), 'err_inf' / 'flux_inf' (term +inf,
    logL = -inf), or one such name per index."""
    wl, flux, err = (np.array(a, dtype=float) for a in kw["spectrum"])
    ok = np.zeros(wl.size, dtype=bool)
    for lo, hi in kw["fitrange"]:
        ok |= (wl > lo) & (wl < hi)
    at = np.flatnonzero(ok)[np.asarray(idx, dtype=int)]
    kinds = [kind] * at.size if isinstance(kind, str) else list(kind)
    assert len(kinds) == at.size
    for i, k in zip(at, kinds):
        if k == "flux_nan":
            flux[i] = np.nan
        elif k == "err_nan":
            err[i] = np.nan
        elif k == "err_zero":
            err[i] = 0.0
        elif k == "err_neg":
            err[i] = -err[i]
        elif k == "err_inf":
            err[i] = np.inf
        elif k == "flux_inf":
            flux[i] = np.inf
        else:
            raise ValueError(k)
    return dict(kw, spectrum=(wl, flux, err))


HI_1215 = (1215.67, 0.4164, 6.265e8)
ASYM_BRACKETS = (64.0, 225.0, 900.0, 1e4, 1e6, np.inf)      # |z|^2 edges of voigt_grad.h: asym_terms (24, 14, 9, 6, 4 terms)


def wing_only_problem(npix=3000, seed=5):
    """(kwargs, rows) of a damped HI 1215 component at z = 0 seen ONLY in its red wing: a logarithmic grid from +300 to
    +12000 km/s of the line centre, no filler.  Every pixel of every row has |u| >= 8.5, so the gradient's Voigt
    evaluations all come from the asymptotic series and the b column is e = H + u H_u + a H_a alone, without a line core
    to dominate its scale S_b; the (logN, b) of the rows spread the pixels over all five truncation brackets of that
    series (`bracket_counts`).  The data are the model of (logN, b) = (20.5, 25) plus noise: no row fits them, so q is not
    noise alone and S_b is 2 .. 8 on every row."""
    step = (12000.0 - 300.0) / (npix - 1)
    wl = HI_1215[0] * np.exp((300.0 + step * np.arange(npix)) / 2.9979245e5)
    err = np.full(npix, 0.02)
    kw = dict(fitrange=[[wl[0] - 1e-3, wl[-1] + 1e-3]], fitlines=["HI 1215"], linepars=[HI_1215], ncomp=[1, 1], nfill=0,
              specres=[8.0], Nrange=[12.0, 21.0], brange=[5.0, 100.0], zrange=[-1e-4, 1e-4], velstep=float(step),
              spectrum=(wl, np.ones(npix), err))
    P = np.array([[1.0, 20.3, 0.0, 30.0], [1.0, 19.5, 2e-5, 12.0], [1.0, 20.8, -3e-5, 35.0], [1.0, 20.0, 1e-5, 6.0]])
    flux = oracle_synth(kw, np.array([1.0, 20.5, 0.0, 25.0])) + np.random.default_rng(seed).normal(0, 0.02, npix)
    return dict(kw, spectrum=(wl, flux, err)), P


def bracket_counts(prob, p):
    """(min |u|, pixels per `ASYM_BRACKETS` bracket of |z|^2) of the single component of row `p`, from the reference's own
    u = (nu (1 + z) - nu0) / dnu and a (hires_fitter.py:357-362)."""
    s = prob.startind
    logN, z, b = p[s + 1:s + 4]
    wrest, f, gam = prob.lines[0]
    dnu = b * 1e5 / (wrest / 1e8)
    u = (oracle.CCGS / (prob.wl / 1e8) * (z + 1.0) - oracle.CCGS / (wrest / 1e8)) / dnu
    a = gam / (4 * np.pi * dnu)
    return np.abs(u).min(), np.histogram(u * u + a * a, bins=ASYM_BRACKETS)[0]


def oracle_synth(kw, p):
    return oracle.reconstruct_spec(problem_from_kwargs(kw), p)


def seeded_noise():
    """The noise realisation of testdata/generate_from_model.py:52-54."""
    np.random.seed(42)
    return np.random.normal(0, 0.02, size=1998)


def require_streaming_shape(fit):
    """Skip a test that asserts the STREAMING launch of the host-pointer entries when the context's stream does not reach
    exactly the eight XCDs of an unpartitioned MI355X (a DPX / QPX / CPX partition): there the library takes the row-block
    pipeline by design (tests/test_gpu_stream_shape.py covers that decision), and only the path assertions would fail."""
    import pytest
    mask = fit.last_launch().xcd_mask
    if mask != 0xFF:
        pytest.skip(f"this device's stream reaches XCDs {mask:#x}, not 0xff: the streaming launch is not taken here")


def tiny_problem(npix, seed=0):
    """One line, one component on a logarithmic grid of `npix` pixels at 2 km/s per pixel, fixed resolution and continuum
    (ndim 4): the smallest problem that still goes through every kernel -- one pixel tile up to ~4000 pixels, two beyond."""
    rng = np.random.default_rng(seed)
    wl = 6190.0 * np.exp(np.arange(npix) * 2.0 / 2.99792458e5)
    z0 = wl[npix // 2] / 1548.204 - 1.0
    return dict(fitrange=[[wl[0] - 0.01, wl[-1] + 0.01]], fitlines=["CIV 1548"], linepars=[(1548.204, 0.1899, 2.643e8)], ncomp=[1, 1],
                nfill=0, specres=[8.0], contval=[1.0], Nrange=[12.0, 14.5], brange=[5.0, 40.0], zrange=[z0 - 2e-4, z0 + 2e-4],
                spectrum=(wl, 1 + rng.normal(0, 0.03, npix), rng.uniform(0.01, 0.05, npix)), velstep=2.0)
