"""GPU: the set-up's segment-mask words by boundary search (mc-alf_amd/csrc/kernel_args.h), and the hand-out order.

The method is tests/test_gpu_segment_masks.py's: a context created under MCALF_INLINE_MAX=0 sends every batch through the
set-up kernel -- whose lanes now each SEARCH the ends of the tile's segments for where their record's threshold run begins
and ends -- and the masked fused kernel; a default context takes the one-launch variant, which classifies every segment
in the component loop.  The two must agree BIT FOR BIT in logL and in the model spectra: one segment classified
differently changes bits.  Rows whose reference value is finite are also held to oracle/numpy_oracle.py at that file's
tolerances.

Rows (`edge_rows`) put a line's threshold run -- the pixels with |u| < uthr, evaluated directly -- where the search has its
boundaries: beginning or ending in segment 0, in the last real segment, inside the virtually continued part of the last
segment, nowhere (a line far outside the spectrum on either side: the predicate holds at both outer ends) and everywhere
(logN so small that the record's threshold is at its floor), and the degenerate records: z = -1 (A = 0), z < -1 (A < 0),
z = 1e200, NaN in logN, z and b, b = 0.  Every such row is there twice: with every component switched on (the full slot
count) and with ncomp = 0 (the fillers alone, which carry the same lines).

A wavelength array out of order: mcalf_create accepts one (nothing sorts the pixels of a fit range), so one context has two
64-pixel blocks of its grid exchanged.  Its segment ends are not monotone, create leaves the walk over all 64 segments in
force for it, and it must stay bit-equal like the others.
"""
import ctypes as C
import os
import warnings

import numpy as np
import pytest
import torch

import mcalf_amd
from mcalf_amd import _lib, workloads
import test_gpu_segment_masks as sm
from test_gpu_segment_masks import NCOMP, NFILL, zc, zf

pytestmark = pytest.mark.gpu


def edge_rows(npix):
    """Constructed rows [ncomp, (N, z, b) x 3, (N, z, b) x 2], each at ncomp = 3 and at ncomp = 0; component 0 and filler 0
    carry the line under test, the others are weak lines in the middle."""
    mid = npix // 2
    nreal = (npix + 63) // 64
    last0 = 64 * (nreal - 1)                                # first pixel of the last real segment
    virt = 0.5 * (npix + 64 * nreal)                        # inside the virtually continued part (npix itself on a whole grid)
    # b = 12 km/s is 6 pixels of Doppler width: uthr of 6 .. 8 puts the run's ends 36 .. 48 pixels from the centre
    centres = [-50, -44, -38, -20, 0, 20, 45,                                    # begins / ends in segment 0
               last0 - 45, last0 - 38, last0, last0 + 20, npix - 1,              # ... in the last real segment
               virt, npix + 30, 64 * nreal + 40, 64 * nreal - 1,                 # ... in its virtual part, or just behind it
               -6000, -300, npix + 300, npix + 12000]                            # nowhere
    cases = [((13.6, zc(k), 12.0), (13.2, zf(k), 12.0)) for k in centres]
    cases += [((lgn, zc(mid), 15.0), (lgn, zf(mid), 15.0)) for lgn in (2.0, -50.0, -400.0)]     # everywhere: uthr at its floor
    for z in (-1.0, -1.5, -3.0, 1e200):
        cases.append(((13.5, z, 15.0), (13.0, z, 15.0)))
    cases += [((np.nan, zc(mid), 15.0), (np.nan, zf(mid), 15.0)), ((13.5, np.nan, 15.0), (13.0, np.nan, 15.0)),
              ((13.5, zc(mid), np.nan), (13.0, zf(mid), np.nan)), ((13.5, zc(mid), 0.0), (13.0, zf(mid), 0.0))]
    weak_c, weak_f = (12.5, zc(mid + 7), 15.0), (11.5, zf(mid - 9), 10.0)
    rows = []
    for comp, fill in cases:
        body = list(comp) + list(weak_c) * (NCOMP - 1) + list(fill) + list(weak_f) * (NFILL - 1)
        rows += [[float(NCOMP)] + body, [0.0] + body]
    return np.array(rows)


def rows_for(kw, npix):
    return np.vstack([edge_rows(npix), workloads.draw_P(kw, 8, np.random.default_rng(23 + npix))])


def run_case(kw, conv_mode, P, npix_out=None):
    logl, models = sm.differential(kw, conv_mode, P)
    if npix_out is not None:
        assert models.shape[1] == npix_out
    checked = sm.check_against_oracle(kw, conv_mode, P, logl, models)
    print("rows", P.shape[0], "held to the oracle", checked)
    assert checked >= 16


# 64 / 128: whole segments, nothing virtual; 130: two pixels of a third; 700: eleven segments; 4080: the largest single-tile
# spectrum with this LSF, 64 real segments (the last one continued virtually), no wholly virtual one
@pytest.mark.parametrize("npix,conv_mode", [(n, "numpy") for n in (64, 130, 128, 700, 4080)] + [(130, "jax"), (4080, "jax")])
def test_searched_words_equal_the_one_launch_variant_bit_for_bit(npix, conv_mode):
    kw = sm.problem(npix)
    run_case(kw, conv_mode, rows_for(kw, npix))


def test_a_grid_with_a_gap():
    kw = sm.problem(700, gap=True)
    P = rows_for(kw, 670)
    P[0, 2], P[1, 1 + 3 * NCOMP + 1] = zc(300), zf(300)   # a line on the seam of the two fit ranges (component 0, filler 0)
    run_case(kw, "numpy", P, npix_out=670)


def test_a_wavelength_array_out_of_order_keeps_the_walk():
    """Two 64-pixel blocks of the grid exchanged (flux and errors with them): the ends of the segments are not monotone."""
    kw = sm.problem(700)
    wl, flux, err = (np.array(a) for a in kw["spectrum"])
    for a in (wl, flux, err):
        a[64:128], a[320:384] = a[320:384].copy(), a[64:128].copy()
    kw["spectrum"] = (wl, flux, err)
    run_case(kw, "numpy", rows_for(kw, 700), npix_out=700)


def test_streaming_host_entry():
    """2048 rows at 700 pixels through the host-pointer entry (the streaming launch where the device streams, whose set-up
    phase is the same code with its table of ends in the workgroup's LDS) and through one device call, against the
    one-launch variant in blocks of 512."""
    kw = sm.problem(700)
    base = rows_for(kw, 700)
    rng = np.random.default_rng(6)
    P = np.vstack([base, workloads.draw_P(kw, 2048 - base.shape[0], rng)])
    P = P[rng.permutation(2048)]
    with sm.masked_and_inline(kw, "numpy") as (masked, inline):
        want, iw = sm.device_logl(inline, P, block=512)
        got, ig = sm.device_logl(masked, P)
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            host = masked.loglike_batch(P)
        path, streams = masked.last_launch().path, masked.last_launch().xcd_mask == 0xFF
    assert all(i.inline_setup == 1 for i in iw)
    assert ig[0].inline_setup == 0 and ig[0].persistent == 1 and ig[0].selfhalo == 1
    print("host-pointer entry: path", path, "streams", streams)
    assert path == (_lib.MCALF_PATH_HOST_STREAM if streams else _lib.MCALF_PATH_HOST_PIPELINED)
    assert sm.same_bits(got, want), np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:8]
    assert sm.same_bits(host, want), np.flatnonzero(host.view(np.uint64) != want.view(np.uint64))[:8]


def _fitter_with_order(kw, order):
    old = os.environ.get("MCALF_ORDER")
    os.environ["MCALF_ORDER"] = order
    try:
        return mcalf_amd.als_fitter(None, conv_mode="numpy", **kw)
    finally:
        if old is None:
            del os.environ["MCALF_ORDER"]
        else:
            os.environ["MCALF_ORDER"] = old


def _logl_into_nan(fit, P):
    dP = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    out = torch.full((P.shape[0],), float("nan"), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(fit._lib.mcalf_loglike_batch_device(fit._ctx, dP.data_ptr(), P.shape[0], out.data_ptr(), st), fit._ctx)
    info = fit.last_launch()
    torch.cuda.synchronize()
    return out.cpu().numpy(), info


@pytest.mark.parametrize("equal_rows", [False, True])
def test_ordered_hand_out_reaches_every_row_once(equal_rows):
    """2560 rows at 130 pixels (4 .. 16 work items per workgroup slot of a 256-CU device: the ordered hand-out), component
    counts drawn from {0, 1, 2, 3} or all equal, into a buffer of NaN: MCALF_ORDER=1 against MCALF_ORDER=0, bit for bit.
    order[] must be a permutation: a lost ticket leaves a NaN behind, a doubled one leaves another row's NaN."""
    kw = sm.problem(130)
    rng = np.random.default_rng(9)
    P = workloads.draw_P(kw, 2560, rng)
    P[:, 0] = 2.0 if equal_rows else rng.integers(0, 4, 2560).astype(float)
    ordered, plain = _fitter_with_order(kw, "1"), _fitter_with_order(kw, "0")
    try:
        a, ia = _logl_into_nan(ordered, P)
        b, ib = _logl_into_nan(plain, P)
    finally:
        ordered.close()
        plain.close()
    print("ordered", ia.ordered, ib.ordered, "persistent", ia.persistent, "grid", ia.grid)
    assert ia.persistent == 1 and ia.ordered == 1 and ib.ordered == 0
    assert not np.isnan(a).any() and not np.isnan(b).any()
    assert sm.same_bits(a, b), np.flatnonzero(a.view(np.uint64) != b.view(np.uint64))[:8]
