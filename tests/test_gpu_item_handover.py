"""GPU: the hand-over from one work item to the next inside the persistent fused kernel -- the next item's loads, the
queue ticket taken ahead of the item's first barrier and looked up in the hand-out order behind the component loop, the
header's counts read back at the top of the item that uses them.

Every test runs the same rows through the persistent grid and through a context created under MCALF_PERSIST=0 (one
workgroup per item: no queue, no hand-over) and asks for the same bits.  The persistent call runs TWICE on one context, so
the second call starts from the queue word the first one left for the set-up kernel to reset, and `mcalf_last_launch` has
to say that the mode a test means to exercise (persistent, ordered or not, lines per barrier) is the one that ran.  No
oracle here: tests/test_gpu_segment_masks.py and tests/test_gpu_parity.py hold the non-persistent paths to it.

The slots of the persistent grid are two per compute unit (512 on an MI355X); the grid is used from four items a slot and
the ordered hand-out up to sixteen, so 2048 rows are exactly four items a slot (the last trip of every slot finds no
further item), 2049 and 2563 leave a ragged last round, and 8193 rows are past the ordered hand-out.
"""
import contextlib
import os

import numpy as np
import pytest
import torch

import mcalf_amd
from mcalf_amd import _lib, workloads
import test_gpu_segment_masks as sm

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def fitter(kw, conv_mode="numpy", **env):
    """A context created under the given MCALF_* variables (the library reads them once, in mcalf_create)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        fit = mcalf_amd.als_fitter(None, conv_mode=conv_mode, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        yield fit
    finally:
        fit.close()


def slots():
    return 2 * torch.cuda.get_device_properties(0).multi_processor_count


def rows(kw, npix, count, seed=3, **rows_kw):
    """`count` rows: the constructed ones of tests/test_gpu_segment_masks.py (one to three components and none at all,
    lines on segment boundaries and far outside the tile, NaN and infinite parameters) among drawn ones, shuffled."""
    base = sm.rows_for(npix, **rows_kw)
    rng = np.random.default_rng(seed + count)
    P = np.vstack([base, workloads.draw_P(kw, count - base.shape[0], rng)])
    return P[rng.permutation(count)]


def differential(kw, conv_mode, P, ordered, lines_per_sync=None, models=True, env=None):
    """logL (and the model spectra) of P from the persistent grid, twice, against MCALF_PERSIST=0; returns logL."""
    env = dict(env or {})
    with fitter(kw, conv_mode, MCALF_PERSIST=0, **env) as plain, fitter(kw, conv_mode, **env) as fit:
        ntiles = fit.info.ntiles
        want, iw = sm.device_logl(plain, P)
        first, i1 = sm.device_logl(fit, P)
        second, i2 = sm.device_logl(fit, P)
        if models:
            mwant, imw = sm.device_models(plain, P)
            mgot, img = sm.device_models(fit, P)
    assert iw[0].persistent == 0 and iw[0].grid == P.shape[0] * ntiles and iw[0].inline_setup == 0
    for i in (i1[0], i2[0]) + ((img,) if models else ()):
        assert i.persistent == 1 and i.grid == slots() and i.items == P.shape[0] * ntiles, (i.persistent, i.grid, i.items)
        assert i.ordered == (1 if ordered else 0)
        assert lines_per_sync is None or i.lines_per_sync == lines_per_sync
    assert sm.same_bits(first, want), np.flatnonzero(first.view(np.uint64) != want.view(np.uint64))[:8]
    assert sm.same_bits(second, want), np.flatnonzero(second.view(np.uint64) != want.view(np.uint64))[:8]
    if models:
        assert imw.persistent == 0
        assert sm.same_bits(mgot, mwant), np.argwhere(mgot.view(np.uint64) != mwant.view(np.uint64))[:8]
    assert np.isfinite(want).sum() > P.shape[0] // 2          # (the comparison is not one of NaN with NaN)
    return want


@pytest.mark.parametrize("npix", [200, 4080])
@pytest.mark.parametrize("conv_mode", ["numpy", "jax"])
def test_short_and_full_tile_with_an_lsf(npix, conv_mode):
    """200 pixels: most threads of the workgroup hold no pixel, and the record, tap and table slices of the threads past
    their ends are loads of a clamped index whose value is never stored.  4080 pixels: the largest single-tile spectrum
    with this LSF (tests/test_gpu_segment_masks.py)."""
    kw = sm.problem(npix)
    differential(kw, conv_mode, rows(kw, npix, 4 * slots()), ordered=True)


@pytest.mark.parametrize("extra", [0, 1, 515])
def test_row_counts_of_the_ordered_hand_out(extra):
    """2048, 2049 and 2563 rows on 512 slots: the last trip of a slot with and without a further item."""
    kw = sm.problem(700)
    differential(kw, "numpy", rows(kw, 700, 4 * slots() + extra), ordered=True, models=extra == 1)


def test_more_than_sixteen_items_a_slot_are_not_ordered():
    kw = sm.problem(700)
    differential(kw, "numpy", rows(kw, 700, 16 * slots() + 1), ordered=False, models=False)


@pytest.mark.parametrize("conv_mode", ["numpy", "jax"])
def test_hand_out_in_queue_order(conv_mode):
    """MCALF_ORDER=0: the ticket is the item, no look-up follows the atomic."""
    kw = sm.problem(700)
    differential(kw, conv_mode, rows(kw, 700, 4 * slots() + 1), ordered=False, env={"MCALF_ORDER": 0})


@pytest.mark.parametrize("lines_per_sync,ncomp", [(4, 4), (5, 4), (5, 3), (4, 3)])
def test_lines_per_barrier(lines_per_sync, ncomp):
    """Ten lines a row fold five a barrier by default and eight fold four: both widths on both, so that a row's component
    loop has one group, two or three -- the ticket's look-up stands behind the loop whatever its trip count."""
    kw = sm.problem(700, ncomp=ncomp)
    differential(kw, "numpy", rows(kw, 700, 4 * slots() + 1, ncomp=ncomp), ordered=True, lines_per_sync=lines_per_sync,
                 models=False, env={"MCALF_LINES_PER_SYNC": lines_per_sync})


def test_mixed_component_counts_and_rows_marked_bad():
    """Free resolution: a row's LSF half-width comes with the row, and a row that asks for a wider LSF than the context
    provisioned is marked bad by the set-up (logL = -inf, a NaN spectrum).  Component counts 0 .. 3 and no fillers switched on
    in some rows: the component loop of consecutive items of a slot runs zero, one or several groups of lines."""
    base = sm.problem(700)
    kw = dict(base, specres=[7.5, 9.0], ncomp=[0, sm.NCOMP])
    n = 4 * slots() + 1
    rng = np.random.default_rng(17)
    body = rows(base, 700, n)
    body[:, 0] = rng.integers(0, sm.NCOMP + 1, n)              # 0 .. 3 components, whatever the row was built for
    R = rng.uniform(7.5, 9.0, n)
    bad = rng.random(n) < 0.05
    R[bad] = rng.uniform(40.0, 80.0, bad.sum())                # half-width far beyond the provisioned halo
    R[rng.random(n) < 0.01] = np.nan
    bad = R > 9.0                                              # (a NaN resolution is not a wide one)
    assert bad.sum() > 50
    P = np.ascontiguousarray(np.column_stack([R, body]))
    with fitter(kw) as probe:
        assert probe.ndim == P.shape[1]
    want = differential(kw, "numpy", P, ordered=True)
    assert np.all(np.isneginf(want[bad & np.isfinite(body).all(axis=1)]))


@pytest.mark.parametrize("conv_mode", ["numpy", "jax"])
def test_two_tiles(conv_mode):
    """6000 pixels are two tiles: 1025 rows are 2050 items, the tiled instantiation, which publishes its ticket at once."""
    kw = sm.problem(6000)
    with fitter(kw, conv_mode) as probe:
        assert probe.info.ntiles == 2
    differential(kw, conv_mode, rows(kw, 6000, 2 * slots() + 1), ordered=False)


def test_chi2_through_the_persistent_grid():
    """chi2 has a host-pointer entry only: with the streaming launch off and one row block it is one launch of the batch
    kernels -- the persistent grid -- in chi2 mode (two sums a wave instead of one)."""
    kw = sm.problem(700)
    P = rows(kw, 700, 4 * slots() + 1)
    env = {"MCALF_STREAM": 0, "MCALF_CHUNKS": 1}
    with fitter(kw, MCALF_PERSIST=0, **env) as plain, fitter(kw, **env) as fit:
        want = plain.chi2_batch(P)
        assert plain.last_launch().persistent == 0 and plain.last_launch().row_blocks == 1
        for _ in range(2):
            got = fit.chi2_batch(P)
            info = fit.last_launch()
            assert info.persistent == 1 and info.ordered == 1 and info.row_blocks == 1 and info.items == P.shape[0]
            assert sm.same_bits(got, want), np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:8]
    assert np.isfinite(want).sum() > P.shape[0] // 2


def test_streaming_launch():
    """The host-pointer entry's single launch hands items out by the same code (per-XCD queues, the next row's stamp looked
    at with the ticket): same bits as one workgroup per item.  Asserted where the device streams -- all eight XCDs visible."""
    kw = sm.problem(700)
    P = rows(kw, 700, 5 * slots() + 3)
    with fitter(kw, MCALF_PERSIST=0) as plain, fitter(kw) as fit:
        want, _ = sm.device_logl(plain, P)
        for _ in range(2):
            got = fit.loglike_batch(P)
            info = fit.last_launch()
            if info.xcd_mask == 0xFF:
                assert info.path == _lib.MCALF_PATH_HOST_STREAM
            assert sm.same_bits(got, want), np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:8]
