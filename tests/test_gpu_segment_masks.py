"""GPU: the fused kernel's pre-classified path -- segment-mask words written by the set-up, interpolation nodes held on
adjacent segments -- against the one-launch variant, which still classifies every line's segments in the component loop.

A single-tile context sends a batch through the set-up kernel and the masked path once the batch has more work items than
MCALF_INLINE_MAX, and through the one-launch variant otherwise.  The variable is read once per context, so a context created
under MCALF_INLINE_MAX=0 (every batch masked) and a default one (batches of <= 512 rows in one launch) live side by side
here, and the two must agree BIT FOR BIT in logL (mcalf_loglike_batch_device) and in the model spectra
(mcalf_model_batch_device): the same operations on the same operands, whoever owns a node.  One segment classified
differently, or one node sum read from another wave's slot, changes bits.  Every row whose reference value is finite is
also held against oracle/numpy_oracle.py at the tolerances of tests/test_gpu_parity.py.

Spectra: a CIV doublet on a logarithmic grid of 2 km/s pixels (a 64-pixel segment = 128 km/s, the doublet's lines lie
~250 pixels apart), up to 3 components and 2 fillers.  Rows are constructed (see `rows_for`), a few are drawn.

About "a spectrum with NaN pixels": mcalf_create decides which segments may be interpolated from the WAVELENGTH grid alone
(is nu reproduced by the 8-node interpolant, is it monotonic), and a pixel with a NaN wavelength never passes the fit-range
selection -- NaN flux or error values exclude no segment.  What does exclude segments is a grid with a jump, so the case
below has two fit ranges (the segment that holds the seam between them is never interpolated: the context's mask word
clears bits of every record's word) and NaN flux / error pixels on top, which np.nansum drops.
"""
import contextlib
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import mcalf_amd
from mcalf_amd import _lib, workloads
from cases import problem_from_kwargs
from oracle import numpy_oracle as o

pytestmark = pytest.mark.gpu

LOGL_ATOL = 1e-4            # tests/test_gpu_parity.py: check_batch
LOGL_RTOL = 1e-10
MODEL_ATOL = 1e-11
FLUX_RTOL = 1e-6

CIV = [(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8)]
WFILL = 250.0               # rest wavelength of the filler line (hires_fitter.py:120-121)
NCOMP, NFILL = 3, 2
CKMS = 2.99792458e5
STEP = 2.0                  # km/s per pixel


def grid(k):
    """Wavelength of pixel k of the logarithmic grid (any k: lines are also centred outside the spectrum)."""
    return 6190.0 * np.exp(np.asarray(k, dtype=float) * STEP / CKMS)


def problem(npix, nfill=NFILL, gap=False, specres=8.0, seed=0, ncomp=NCOMP):
    """Noise as in the configurations tests/test_gpu_parity.py runs (mcalf_amd.workloads: sigma = 0.02 on every pixel), so
    that its bars mean here what they mean there: its relative bar is 1e-10 of |logL|, and with errors drawn between 0.01
    and 0.05 the chi-square and the log(ispec2) terms of a good fit nearly cancel -- |logL| ~ 1, the bar then asks 1e-10
    ABSOLUTE of a sum whose terms the same check allows 1e-11 x ispec2 x |residual| each (seen: 1e-9 at 130 pixels)."""
    rng = np.random.default_rng(seed + npix)
    wl = grid(np.arange(npix))
    flux, err = 1 + rng.normal(0, 0.02, npix), np.full(npix, 0.02)
    fitrange = [[wl[0] - 0.01, wl[-1] + 0.01]]
    if gap:                                              # two fit ranges: pixels 300 .. 329 are not fitted, the grid jumps
        fitrange = [[wl[0] - 0.01, 0.5 * (wl[299] + wl[300])], [0.5 * (wl[329] + wl[330]), wl[-1] + 0.01]]
        flux[[5, 77, 500]] = np.nan
        err[[6, 640]] = np.nan
    z0 = float(wl[npix // 2] / CIV[0][0] - 1.0)
    return dict(fitrange=fitrange, fitlines=["CIV 1548", "CIV 1550"], linepars=CIV, ncomp=[1, ncomp], nfill=nfill,
                specres=[specres], contval=[1.0], Nrange=[12.0, 14.5], brange=[5.0, 40.0], zrange=[z0 - 2e-3, z0 + 2e-3],
                Nrangefill=[11.5, 14.0], brangefill=[1.0, 30.0], spectrum=(wl, flux, err), velstep=STEP)


def zc(k):
    """Redshift that puts CIV 1548 on pixel k."""
    return float(grid(k) / CIV[0][0] - 1.0)


def zf(k):
    """Redshift that puts the filler line on pixel k."""
    return float(grid(k) / WFILL - 1.0)


def rows_for(npix, nfill=NFILL, ncomp=NCOMP):
    """Constructed rows [ncomp, (N, z, b) x ncomp, (N, z, b) x nfill]; components and fillers a row does not name are weak
    lines in the middle of the spectrum (with more than three components the rows that name fewer switch all of them on)."""
    mid = npix // 2

    ncompmax = ncomp

    def row(ncomp, comps=(), fills=()):
        if ncompmax > NCOMP and ncomp > 0:
            ncomp = ncompmax
        c = list(comps) + [(12.5, zc(mid + 7), 15.0)] * (ncompmax - len(comps))
        f = (list(fills) + [(11.5, zf(mid - 9), 10.0)] * NFILL)[:nfill]
        return [float(ncomp)] + [v for t in c for v in t] + [v for t in f for v in t]

    seam = 64 * max(1, (npix // 64) // 2)                  # a segment boundary (the first one past the data at npix <= 64)
    rows = [
        row(1, [(13.6, zc(seam), 12.0)]),                  # centred exactly on a segment boundary ...
        row(2, [(13.9, zc(seam - 0.5), 9.0), (13.2, zc(seam + 64), 25.0)]),   # ... between its two pixels, and on the next one
        row(1, [(13.7, zc(0), 14.0)]),                     # centred on the first pixel
        row(1, [(13.7, zc(npix - 1), 14.0)]),              # centred on the last pixel
        row(2, [(14.2, zc(-6000), 20.0), (14.2, zc(12000), 20.0)]),   # well outside the tile on either side: all interpolated
        row(1, [(24.5, zc(mid), 40.0)]),                   # the whole tile inside |u| < uthr: every segment direct
        row(1, [(13.0, zc(mid), 20.0)], [(14.0, zf(npix // 3), 1.0), (13.5, zf(2 * npix // 3), 1.0)]),   # b = 1 fillers
        row(1, [(16.0, zc(mid), 20.0)]),                   # x2c at its cap
        row(3, [(13.5, zc(mid - 20), 0.05), (13.4, zc(mid + 30), 18.0), (13.8, zc(mid // 2), 11.0)]),   # a > 2^-8 among fast-path lines
        row(0, [], [(13.0, zf(mid), 5.0), (13.3, zf(mid // 3), 3.0)]),   # no component, fillers only
        row(1, [(13.5, 1e150, 15.0)]),                     # |1 + z| > 1e100
        row(2, [(13.5, zc(mid), 15.0), (13.5, -1e150, 15.0)]),
    ]
    for v in (np.nan, np.inf, -np.inf):                    # NaN / infinite N, z, b
        rows += [row(2, [(v, zc(mid), 15.0), (13.3, zc(mid + 40), 12.0)]),
                 row(2, [(13.5, v, 15.0), (13.3, zc(mid + 40), 12.0)]),
                 row(2, [(13.5, zc(mid), v), (13.3, zc(mid + 40), 12.0)])]
    P = np.array(rows)
    drawn = workloads.draw_P(problem(npix, nfill, ncomp=ncompmax), 8, np.random.default_rng(11 + npix))
    assert drawn.shape[1] == P.shape[1]
    return np.vstack([P, drawn])


@contextlib.contextmanager
def masked_and_inline(kw, conv_mode):
    """(masked, inline): a context whose every batch goes through the set-up kernel and the masked fused kernel, and a
    default one, whose batches of at most 512 rows take the one-launch variant."""
    old = os.environ.get("MCALF_INLINE_MAX")
    os.environ["MCALF_INLINE_MAX"] = "0"
    try:
        masked = mcalf_amd.als_fitter(None, conv_mode=conv_mode, **kw)
    finally:
        if old is None:
            del os.environ["MCALF_INLINE_MAX"]
        else:
            os.environ["MCALF_INLINE_MAX"] = old
    try:
        inline = mcalf_amd.als_fitter(None, conv_mode=conv_mode, **kw)
        try:
            yield masked, inline
        finally:
            inline.close()
    finally:
        masked.close()


def device_logl(fit, P, block=None):
    """logL of the rows through mcalf_loglike_batch_device, `block` rows per call (None: one call)."""
    dP = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    out = torch.empty(P.shape[0], dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    step = block or P.shape[0]
    info = []
    for i in range(0, P.shape[0], step):
        n = min(step, P.shape[0] - i)
        _lib.check(fit._lib.mcalf_loglike_batch_device(fit._ctx, dP[i:].data_ptr(), n, out[i:].data_ptr(), st), fit._ctx)
        info.append(fit.last_launch())
    torch.cuda.synchronize()
    return out.cpu().numpy(), info


def device_models(fit, P):
    dP = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    dm = torch.empty((P.shape[0], fit.obj_wl.size), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(fit._lib.mcalf_model_batch_device(fit._ctx, dP.data_ptr(), P.shape[0], 0, dm.data_ptr(), st), fit._ctx)
    info = fit.last_launch()
    torch.cuda.synchronize()
    return dm.cpu().numpy(), info


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_against_oracle(kw, conv_mode, P, logl, models):
    """tests/test_gpu_parity.py's bars: check_batch's for a convolved context; for one that skips the convolution (R <= the
    pixel step) the bar it holds such a context to (test_edge_cases (1): logL alone) -- unconvolved, a model pixel carries the
    cancellation noise of u = nu A - B on both sides (eps x |nu A| ~ 3e-11 in u for a b = 1 filler, times K H'(u): seen
    1.4e-11 in the flux of the b = 1 row at 4096 pixels, from the one-launch variant and the masked path alike), which is
    not what this file is about; those models are still held to the one-launch variant's bit for bit."""
    prob = problem_from_kwargs(kw)
    convolved = kw["specres"][0] > kw["velstep"]
    checked = 0
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for p, g, m in zip(P, logl, models):
            if conv_mode == "jax":
                want, ref = o.jax_loglike_f64(prob, p), o.jax_reconstruct_spec_f64(prob, p)
            else:
                want, ref = o.lnlhood_worker(prob, p), o.reconstruct_spec(prob, p)
            if not (np.isfinite(want) and np.all(np.isfinite(ref))):
                continue
            checked += 1
            assert abs(g - want) < LOGL_ATOL and abs(g - want) / max(1.0, abs(want)) < LOGL_RTOL, (p, g, want)
            if not convolved:
                continue
            assert np.abs(m - ref).max() < MODEL_ATOL, p
            ok = ref > 1e-290                            # (none where a saturated line blots the whole spectrum out)
            assert not ok.any() or np.abs(m[ok] / ref[ok] - 1).max() < FLUX_RTOL, p
    return checked


def differential(kw, conv_mode, P, lines_per_sync=4):
    with masked_and_inline(kw, conv_mode) as (masked, inline):
        assert masked.info.ntiles == 1 and inline.info.ntiles == 1
        lm, im = device_logl(masked, P)
        li, ii = device_logl(inline, P)
        mm, imm = device_models(masked, P)
        mi, imi = device_models(inline, P)
    assert all(i.inline_setup == 0 and i.selfhalo == 1 for i in im + [imm])      # the set-up kernel and the masked path
    assert all(i.lines_per_sync == lines_per_sync for i in im + [imm])
    assert all(i.inline_setup == 1 and i.selfhalo == 1 for i in ii + [imi])      # the one-launch variant
    assert same_bits(lm, li), np.flatnonzero(lm.view(np.uint64) != li.view(np.uint64))
    assert same_bits(mm, mi), np.argwhere(mm.view(np.uint64) != mi.view(np.uint64))[:8]
    return lm, mm


# 63: one partial segment; 64: one whole segment; 130: a partial third; 700: eleven segments -- node waves 0 and 1 both hold
# nodes and a line's run of direct segments crosses the boundary between them; 4000: the last segment partial, the grid
# continued virtually.  A full tile: the 4096 entries of a tile include the LSF's halo and tiles are multiples of 8 pixels, so
# with this LSF (6 pixels either side) the largest single-tile spectrum has 4080 pixels; a spectrum of 4096 pixels is a
# single tile only without a halo -- numpy semantics at a resolution below the pixel step (no convolution,
# hires_fitter.py:445; JAX semantics always convolve, on at least 3 taps).
SHAPES = [(n, m, 8.0) for n in (63, 64, 130, 700, 4000, 4080) for m in ("numpy", "jax")] + [(4096, "numpy", 1.5)]


@pytest.mark.parametrize("npix,conv_mode,specres", SHAPES)
def test_masked_path_equals_the_one_launch_variant_bit_for_bit(npix, conv_mode, specres):
    kw, P = problem(npix, specres=specres), rows_for(npix)
    logl, models = differential(kw, conv_mode, P)
    assert check_against_oracle(kw, conv_mode, P, logl, models) >= 16


@pytest.mark.parametrize("npix", [700, 4000])
@pytest.mark.parametrize("conv_mode", ["numpy", "jax"])
def test_five_lines_per_barrier(npix, conv_mode):
    """Four components and two fillers are ten lines a row: the context folds five lines per barrier (two groups where four a
    group make three), so the masked five-line instantiations run -- the benchmark's -- and the node sums cross waves through
    a table half of that layout.  The contexts above, with at most eight lines, fold four."""
    kw, P = problem(npix, ncomp=4), rows_for(npix, ncomp=4)
    logl, models = differential(kw, conv_mode, P, lines_per_sync=5)
    assert check_against_oracle(kw, conv_mode, P, logl, models) >= 16


@pytest.mark.parametrize("conv_mode", ["numpy", "jax"])
def test_no_fillers_and_a_grid_with_a_seam(conv_mode):
    kw, P = problem(700, nfill=0), rows_for(700, nfill=0)
    logl, models = differential(kw, conv_mode, P)
    assert check_against_oracle(kw, conv_mode, P, logl, models) >= 16
    kw = problem(700, gap=True)
    P = rows_for(700)
    P[0, 2] = zc(300)                                    # a line on the seam of the two fit ranges
    logl, models = differential(kw, conv_mode, P)
    assert models.shape[1] == 670
    assert check_against_oracle(kw, conv_mode, P, logl, models) >= 16


@pytest.mark.parametrize("conv_mode", ["numpy", "jax"])
def test_persistent_grid_and_streaming_launch_equal_the_one_launch_variant(conv_mode):
    """2048 rows at 700 pixels: one device call is the persistent grid with the ordered hand-out, the host-pointer entry the
    streaming launch -- asserted wherever the device streams (all eight XCDs visible, what tests/test_gpu_device_api.py
    asks of a device before it expects that path); elsewhere the row-block pipeline, which runs the same masked batch
    kernel.  Both must give every row the bits the one-launch variant gives it in blocks of 512."""
    kw = problem(700)
    base = rows_for(700)
    rng = np.random.default_rng(5)
    P = np.vstack([base, workloads.draw_P(kw, 2048 - base.shape[0], rng)])
    P = P[rng.permutation(2048)]
    with masked_and_inline(kw, conv_mode) as (masked, inline):
        want, iw = device_logl(inline, P, block=512)
        got, ig = device_logl(masked, P)
        host = masked.loglike_batch(P)
        path, streams = masked.last_launch().path, masked.last_launch().xcd_mask == 0xFF
        models, _ = device_models(inline, P[:64])
    assert all(i.inline_setup == 1 for i in iw)
    assert ig[0].inline_setup == 0 and ig[0].persistent == 1 and ig[0].ordered == 1 and ig[0].selfhalo == 1
    print("host-pointer entry: path", path, "streams", streams)
    assert path == (_lib.MCALF_PATH_HOST_STREAM if streams else _lib.MCALF_PATH_HOST_PIPELINED)
    assert same_bits(got, want), np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:8]
    assert same_bits(host, want), np.flatnonzero(host.view(np.uint64) != want.view(np.uint64))[:8]
    assert check_against_oracle(kw, conv_mode, P[:64], got[:64], models) >= 32
