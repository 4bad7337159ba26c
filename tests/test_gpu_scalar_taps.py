"""GPU: the batch kernels' LSF convolution, whose weights are scalar operands read from the set-up kernel's tap rows, against
the one-launch variant, which reads the same weights from their copy in LDS.

The two run the same FMAs on the same operands in the same order, so the same rows must come out BIT FOR BIT through

  * the batch kernels (a context created under MCALF_INLINE_MAX=0: set-up kernel + fused kernel for every batch) --
    device-pointer entries, one launch per batch;
  * the one-launch variant (a default context: batches of at most 512 work items) -- device-pointer entries;
  * the host-pointer entries of the first context, in one row block and in two (`set_chunks`).

Every row whose reference value is finite is also held to oracle/numpy_oracle.py at the bars of tests/test_gpu_parity.py.

What the convolution loop can get wrong is decided by the tap count 2 n + 1 of a row: whole groups of eight taps are taken
in pairs from two register sets (an odd count of groups leaves the remainder's weights in the other set), the last
1, 3, 5 or 7 taps come from one more group.  The half-width n of a row is ceil(3.0348 sigma) of its resolution, 0 at or
below the pixel step, and never 1 (a resolution above the 2 km/s step gives n >= 2).  `HALF_WIDTHS` below lists what a
context with a floated resolution sees in ONE batch, neighbours differing, with n_cap = 26; contexts of a fixed resolution
(one tap row for all live points) cover a few of them again.  Spectra: cases.tiny_problem at 600 pixels (one tile) and
4500 (two), with one filler line added so that `targonly` means something.

The persistent grid needs four work items per workgroup slot of the chip (2048 at least), which batches of this size
never reach and no knob forces: it is covered by tests/test_gpu_segment_masks.py (2048 rows) and by the benchmark.
"""
import contextlib
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import mcalf_amd
from mcalf_amd import _lib
from cases import problem_from_kwargs, tiny_problem
from oracle import numpy_oracle as o

pytestmark = pytest.mark.gpu

LOGL_ATOL = 1e-4            # tests/test_gpu_parity.py: check_batch
LOGL_RTOL = 1e-10
MODEL_ATOL = 1e-11
FLUX_RTOL = 1e-6

STEP = 2.0                  # km/s per pixel (cases.tiny_problem)
FWHM_TO_SIGMA, REACH = 2.354820, 3.0348      # hires_fitter.py:454, :458
N_CAP = 26
# taps:      1  5  7  9 11 13 15  17  25  27  33  41  49  53   55 (wider than provisioned: not computed)
HALF_WIDTHS = [0, 2, 3, 4, 5, 6, 7, 8, 12, 13, 16, 20, 24, 26, 27]
WFILL = 250.0               # rest wavelength of the filler line (hires_fitter.py:120-121)


def half_width(R):
    return int(np.ceil(REACH * (R / FWHM_TO_SIGMA) / STEP)) if R > STEP else 0


def res_for(n):
    """A resolution (km/s) whose LSF has half-width n: the middle of the interval that ceil() maps to n."""
    R = (n - 0.5) * STEP * FWHM_TO_SIGMA / REACH if n > 0 else 0.75 * STEP
    assert half_width(R) == n, (n, R)
    return R


def problem(npix, specres):
    kw = dict(tiny_problem(npix), nfill=1, Nrangefill=[11.5, 14.0], brangefill=[1.0, 30.0], specres=list(specres))
    return kw


def rows(kw, resolutions):
    """One row per entry of `resolutions` (None: a context of fixed resolution, rows without that column):
    [R,] ncomp = 1, (N, z, b), filler (N, z, b) -- lines of moderate depth at drawn places -- and behind them a saturated
    component that blots the spectrum out (chi2's all-zero-model test) and rows with a NaN N and a NaN z."""
    wl = kw["spectrum"][0]
    rng = np.random.default_rng(len(wl) + len(resolutions))
    zlo, zhi = kw["zrange"]
    out = []
    for R in resolutions:
        body = [1.0, rng.uniform(13.0, 14.3), rng.uniform(zlo, zhi), rng.uniform(8.0, 35.0),
                rng.uniform(12.0, 13.8), float(wl[rng.integers(20, len(wl) - 20)] / WFILL - 1.0), rng.uniform(2.0, 20.0)]
        out.append(([] if R is None else [R]) + body)
    P = np.array(out)
    first = 0 if resolutions[0] is None else 1
    special = P[[1, 2, 3]].copy()
    special[0, first + 1], special[0, first + 3] = 24.5, 40.0          # saturated: the model is 0 on every pixel of 600
    special[1, first + 1] = np.nan
    special[2, first + 2] = np.nan
    return np.vstack([P, special])


@contextlib.contextmanager
def batch_and_inline(kw, conv_mode):
    """(batch, inline): a context whose every batch goes through the set-up kernel and the batch fused kernel, and a
    default one, whose batches of at most 512 work items take the one-launch variant."""
    old = os.environ.get("MCALF_INLINE_MAX")
    os.environ["MCALF_INLINE_MAX"] = "0"
    try:
        batch = mcalf_amd.als_fitter(None, conv_mode=conv_mode, **kw)
    finally:
        if old is None:
            del os.environ["MCALF_INLINE_MAX"]
        else:
            os.environ["MCALF_INLINE_MAX"] = old
    try:
        inline = mcalf_amd.als_fitter(None, conv_mode=conv_mode, **kw)
        try:
            yield batch, inline
        finally:
            inline.close()
    finally:
        batch.close()


def device_logl(fit, P):
    dP = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    out = torch.empty(P.shape[0], dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(fit._lib.mcalf_loglike_batch_device(fit._ctx, dP.data_ptr(), P.shape[0], out.data_ptr(), st), fit._ctx)
    info = fit.last_launch()
    torch.cuda.synchronize()
    return out.cpu().numpy(), info


def device_models(fit, P, targonly):
    dP = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    dm = torch.empty((P.shape[0], fit.obj_wl.size), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(fit._lib.mcalf_model_batch_device(fit._ctx, dP.data_ptr(), P.shape[0], int(targonly), dm.data_ptr(), st), fit._ctx)
    info = fit.last_launch()
    torch.cuda.synchronize()
    return dm.cpu().numpy(), info


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def differ(a, b):
    return np.argwhere(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64))[:8]


def three_routes(kw, conv_mode, P, ntiles):
    """logL, chi2 and the models (targonly both ways) of the rows through every route; all asserted equal bit for bit.
    Returns the batch kernels' (logL, chi2, models, models of the components alone)."""
    with batch_and_inline(kw, conv_mode) as (batch, inline):
        assert batch.info.ntiles == ntiles and inline.info.ntiles == ntiles
        n_cap = batch.info.n_cap
        lb, ilb = device_logl(batch, P)
        li, ili = device_logl(inline, P)
        mb, imb = device_models(batch, P, False)
        mi, imi = device_models(inline, P, False)
        tb, itb = device_models(batch, P, True)
        ti, iti = device_models(inline, P, True)
        hb = batch.loglike_batch(P)
        hpath = batch.last_launch().path
        batch.set_chunks(2)
        hb2 = batch.loglike_batch(P)
        batch.set_chunks(0)
        hm, ht = batch.model_batch(P), batch.model_batch(P, targonly=True)
        cb = batch.chi2_batch(P)
        icb = batch.last_launch()
        ci = inline.chi2_batch(P)
        ici = inline.last_launch()
    print("host-pointer entry: path", hpath, "| chi2: batch context inline_setup", icb.inline_setup, "default context inline_setup",
          ici.inline_setup)
    for i in (ilb, imb, itb):                                # the set-up kernel and the batch fused kernel, not persistent
        assert i.inline_setup == 0 and i.persistent == 0 and i.selfhalo == (1 if ntiles == 1 else 0), (i.inline_setup, i.persistent)
    for i in (ili, imi, iti):                                # the one-launch variant
        assert i.inline_setup == 1
    assert icb.inline_setup == 0
    assert same_bits(lb, li), differ(lb, li)
    assert same_bits(hb, li), differ(hb, li)
    assert same_bits(hb2, li), differ(hb2, li)
    assert same_bits(mb, mi), differ(mb, mi)
    assert same_bits(hm, mi), differ(hm, mi)
    assert same_bits(tb, ti), differ(tb, ti)
    assert same_bits(ht, ti), differ(ht, ti)
    assert same_bits(cb, ci), differ(cb, ci)
    return n_cap, lb, cb, mb, tb


def check_against_oracle(kw, conv_mode, P, skip, logl, chi2, models, targ):
    """The bars of tests/test_gpu_parity.py (check_batch) for every row outside `skip` whose reference values are finite;
    chi2 (numpy semantics only: the oracle has no JAX chi2) at the relative bar of logL, and +inf where the oracle finds
    the model zero on every pixel."""
    prob = problem_from_kwargs(kw)
    checked = 0
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for k, p in enumerate(P):
            if k in skip:
                continue
            if conv_mode == "jax":
                want, ref, tref, wchi = o.jax_loglike_f64(prob, p), o.jax_reconstruct_spec_f64(prob, p), None, None
            else:
                want, ref, tref, wchi = o.lnlhood_worker(prob, p), o.reconstruct_spec(prob, p), o.reconstruct_spec(prob, p, True), o.chi2(prob, p)
            if not (np.isfinite(want) and np.all(np.isfinite(ref))):
                continue
            checked += 1
            g = logl[k]
            assert abs(g - want) < LOGL_ATOL and abs(g - want) / max(1.0, abs(want)) < LOGL_RTOL, (p, g, want)
            if wchi is not None:
                if isinstance(wchi, tuple):
                    assert chi2[k] == np.inf, (p, chi2[k])
                else:
                    assert abs(chi2[k] - wchi) / max(1.0, abs(wchi)) < LOGL_RTOL, (p, chi2[k], wchi)
            R = p[0] if len(kw["specres"]) > 1 else kw["specres"][0]
            if conv_mode != "jax" and R <= STEP:             # unconvolved: test_gpu_parity.py holds such a model to logL alone
                continue
            for m, r in ((models[k], ref), (targ[k], tref)):
                if r is None:
                    continue
                assert np.abs(m - r).max() < MODEL_ATOL, p
                ok = r > 1e-290
                assert not ok.any() or np.abs(m[ok] / r[ok] - 1).max() < FLUX_RTOL, p
    return checked


@pytest.mark.parametrize("conv_mode", ["numpy", "jax"])
@pytest.mark.parametrize("npix,ntiles", [(600, 1), (4500, 2)])
def test_floated_resolution_every_tap_count_in_one_batch(npix, ntiles, conv_mode):
    """Numpy semantics: the rows' half-widths are HALF_WIDTHS -- one tap; fewer than eight; every remainder 1, 3, 5, 7; one,
    two, three, four, five and six whole groups; exactly 2 n_cap + 1; and one LSF wider than provisioned, which must come out
    as logL = -inf, chi2 = +inf and a NaN model.  JAX semantics: the kernel grid is fixed (2 n_cap + 1 taps for every row,
    the edge reset on n_cap pixels either side) and the resolution only shapes the weights."""
    kw = problem(npix, [1.0, res_for(N_CAP)])
    res = [res_for(n) for n in HALF_WIDTHS]
    P = rows(kw, res)
    assert 3 <= P.shape[0] <= 40
    n_cap, logl, chi2, models, targ = three_routes(kw, conv_mode, P, ntiles)
    skip = set()
    if conv_mode == "numpy":
        assert n_cap == N_CAP
        wide = HALF_WIDTHS.index(N_CAP + 1)
        assert logl[wide] == -np.inf and chi2[wide] == np.inf and np.isnan(models[wide]).all() and np.isnan(targ[wide]).all()
        skip.add(wide)                                       # (the reference would build the longer kernel)
    sat = len(res)
    assert np.isfinite(logl[:sat]).sum() >= len(res) - 1
    if npix == 600:
        assert np.all(models[sat] == 0.0) and chi2[sat] == np.inf
    assert check_against_oracle(kw, conv_mode, P, skip, logl, chi2, models, targ) >= len(res) - 1


@pytest.mark.parametrize("conv_mode", ["numpy", "jax"])
@pytest.mark.parametrize("npix,ntiles,n", [(600, 1, 0), (600, 1, 3), (600, 1, 12), (600, 1, 24), (4500, 2, 8), (4500, 2, 13)])
def test_fixed_resolution_one_tap_row_for_all(npix, ntiles, n, conv_mode):
    """A fixed resolution: the set-up kernel writes ONE tap row and every live point reads it (`taps_shared`).  Half-widths
    0 (numpy semantics: no convolution; JAX: its smallest grid), 3 (seven taps, no whole group), 12 (three groups + 1),
    24 (the benchmark's 49 taps), and on two tiles 8 (two groups + 1) and 13 (three groups + 3); n = n_cap throughout."""
    kw = problem(npix, [res_for(n)])
    P = rows(kw, [None] * 9)
    n_cap, logl, chi2, models, targ = three_routes(kw, conv_mode, P, ntiles)
    if conv_mode == "numpy":
        assert n_cap == n
    assert np.isfinite(logl[:9]).all()
    assert check_against_oracle(kw, conv_mode, P, set(), logl, chi2, models, targ) >= 9
