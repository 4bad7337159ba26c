"""GPU: batched equivalent widths -- mcalf_eqw_batch[_device] and the Python entries on it (eqw_batch, calc_w_batch,
calc_N_batch) -- against the numpy restatement of tests/eqw_reference.py (itself checked against the oracle's calc_w by
tests/test_eqw_host.py).  Every cell must satisfy |got - want| <= 1e-11 + 1e-9 |want|, the bar tests/test_gpu_parity.py
applies to calc_w; NaN and infinite cells must coincide.  Every comparison prints its worst error / bar (pytest -s).

Shapes: the pixel kernel's tile is 2048 pixels (four waves of 64 lanes, 8 pixels per thread), so 2 and 257 pixels are
partial first tiles (one wave partly filled, then three empty ones) and 4500 pixels are two full tiles and one of 404."""
import ctypes as C

import numpy as np
import pytest
import torch

import eqw_reference as er
import mcalf_amd
from cases import oracle_synth, problem_from_kwargs
from mcalf_amd import _lib, workloads

pytestmark = pytest.mark.gpu

CIV3 = [(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8), (1549.5, 0.05, 2.6e8)]      # (the third is made up: a line between the two)


def _mode(jax):
    return "jax" if jax else "numpy"


def _compare(fit, prob, P, reference_indexing, what, jax=False):
    wc, wb = fit.eqw_batch(P, reference_indexing=reference_indexing)
    wantc, wantb = er.eqw_rows(prob, P, reference_indexing, jax)
    assert wc.shape == wantc.shape == (len(P), prob.ncompmax, prob.numlines) and wb.shape == wantb.shape == (len(P), prob.numlines)
    print(f"eqw {what}: worst error / bar: Wcomp {er.worst(wc, wantc):.3g}, Wblend {er.worst(wb, wantb):.3g}")
    assert er.close(wc, wantc), what
    assert er.close(wb, wantb), what
    return wc, wb, wantc, wantb


@pytest.fixture(scope="module")
def cfgC():
    return workloads.config("C", oracle_synth)


@pytest.mark.parametrize("reference_indexing", [False, True], ids=["layout", "as_written"])
def test_config_C(cfgC, reference_indexing):
    kw, _, seed = cfgC
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 6, np.random.default_rng(seed + 5))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        wc, wb, wantc, wantb = _compare(fit, prob, P, reference_indexing, f"config C, reference_indexing={reference_indexing}")
    if reference_indexing:
        assert np.isfinite(wantc).all() and np.isfinite(wantb).all()
        assert np.all(wantc.sum(axis=1) > 1.0)                    # (about 14 Angstrom: saturated slots, columns read off the b entries)
    else:
        for r, p in enumerate(P):
            nc = int(p[prob.startind])
            assert np.all(wc[r, nc:] == 0.0) and np.all(wc[r, :nc] > 0.0)


def test_config_E_damped():
    kw, _, seed = workloads.config("E", oracle_synth)
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 3, np.random.default_rng(seed), damped=2)
    P[0, prob.startind + 1] = 20.5                                # one saturated damped component for certain
    with mcalf_amd.als_fitter(None, **kw) as fit:
        wc, wb, _, _ = _compare(fit, prob, P, False, "config E, damped")
    z = P[:, prob.startind + 2::3][:, :prob.ncompmax]
    total = (wc[:, :, 0] * (1 + z)).sum(axis=1)
    # logN = 20.5 is a rest-frame width of ~9 Angstrom when the window holds the whole line, and damping wings overlap everything
    assert wc[0, 0, 0] > 2.0 and np.all(total >= wb[:, 0] - 1e-9) and np.all(wb[:, 0] < total)


def test_the_1998_pixel_fixture():
    kw, _, seed = workloads.config("A")
    prob = problem_from_kwargs(kw)
    assert prob.wl.size == 1998 and kw["ncomp"] == [2, 2]
    P = workloads.draw_P(kw, 5, np.random.default_rng(seed))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        for ri in (False, True):
            _compare(fit, prob, P, ri, f"fixture, reference_indexing={ri}")


def _edge_kw(npix, nlines, startind, ncompmax=3, nfill=1):
    wl = np.linspace(6180.0, 6220.0, npix + 2)[1:-1]
    rng = np.random.default_rng(npix)
    return dict(fitrange=[[6180.0, 6220.0]], fitlines=["CIV 1548", "CIV 1550", "made up"][:nlines], linepars=CIV3[:nlines],
                ncomp=[0, ncompmax], nfill=nfill, specres=[6.0, 9.0] if startind >= 1 else [8.0], contval=[0.9, 1.1] if startind == 2 else [1.0],
                Nrange=[12.5, 14.5], brange=[8.0, 40.0], zrange=[2.995, 3.012], velstep=float(np.median(np.diff(wl) / wl[1:]) * 2.9979245e5),
                spectrum=(wl, 1 + rng.normal(0, 0.03, npix), np.full(npix, 0.03)))


def _edge_rows(kw, s):
    """Active counts 0, 1 and ncompmax, a fractional and a negative slot, a component shifted off the spectrum, NaN in the
    inactive slots, NaN in an active slot."""
    P = workloads.draw_P(kw, 8, np.random.default_rng(3))
    P[:, s] = [0.0, 1.0, 3.0, 2.7, -1.0, 1.0, 1.0, 2.0]
    P[5, s + 2] = 3.2                                             # z = 3.2: CIV at 6502 Angstrom, off the window
    P[6, s + 4:s + 10] = np.nan                                   # slots 1 and 2 of a row with one active component
    P[7, s + 2] = np.nan                                          # z of the first of two active components
    return P


@pytest.mark.parametrize("npix,nlines,startind", [(2, 1, 0), (2, 3, 2), (257, 2, 1), (257, 3, 0), (4500, 3, 2), (4500, 1, 1), (4500, 2, 0)])
def test_edge_shapes(npix, nlines, startind):
    kw = _edge_kw(npix, nlines, startind)
    prob = problem_from_kwargs(kw)
    s = prob.startind
    assert s == startind and prob.wl.size == npix and prob.numlines == nlines
    P = _edge_rows(kw, s)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        wc, wb, _, _ = _compare(fit, prob, P, False, f"edge {npix} px, {nlines} lines, startind {startind}, layout")
        active = [0, 1, 3, 2, 0, 1, 1, 2]
        for r, nc in enumerate(active):
            assert np.all(wc[r, nc:] == 0.0)
        assert np.isfinite(wc[:7]).all() and np.isfinite(wb[:7]).all()          # NaN in inactive slots does not leak
        assert np.all(wc[0] == 0.0) and np.all(wb[0] == 0.0) and np.all(wb[4] == 0.0)
        assert np.isnan(wc[7, 0]).all() and np.isfinite(wc[7, 1]).all() and np.isnan(wb[7]).all()
        assert np.array_equal(fit.eqw_batch(P[:7])[0], wc[:7]) and np.array_equal(fit.eqw_batch(P[:7])[1], wb[:7])   # only that row
        if npix >= 257:
            assert np.all(wc[5, 0] < 1e-3 * wc[1, 0])                            # the shifted component: far wings only
        # the reference as written on the rows whose shifted triples are finite: b = z1 ~ 3 km/s, N = the b entries
        _compare(fit, prob, P[:6], True, f"edge {npix} px, {nlines} lines, startind {startind}, as written")


def test_jax_context_floors_the_slot():
    kw = _edge_kw(257, 2, 1)
    prob = problem_from_kwargs(kw)
    s = prob.startind
    P = _edge_rows(kw, s)[:4]
    P[:, s] = [-0.5, 2.7, 1.0, 3.9]
    with mcalf_amd.als_fitter(None, conv_mode="jax", **kw) as fit:
        wc, _, _, _ = _compare(fit, prob, P, False, "JAX context", jax=True)
        assert np.all(wc[0] == 0.0) and np.all(wc[1, 2] == 0.0) and np.all(wc[1, :2] > 0.0) and np.all(wc[3] > 0.0)


def test_a_negative_b_and_an_absurd_column_take_the_general_voigt_path():
    """What the shifted triples can produce, put into the layout's own slots: b < 0 (a < 0: scipy's reflection), logN = 30
    (exp(-x^2) matters far beyond |x| = 8), b = 0.001 km/s (a beyond the fast range)."""
    kw = _edge_kw(257, 2, 0, nfill=0)
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 3, np.random.default_rng(8))
    P[:, 0] = 3.0
    P[0, 3] = -12.0
    P[1, 1] = 30.0
    P[2, 3] = 0.001
    with mcalf_amd.als_fitter(None, **kw) as fit:
        _compare(fit, prob, P, False, "general Voigt path")


def test_a_spectrum_of_one_pixel_is_refused():
    lib = _lib.load()
    wl, one, err = np.array([6200.0]), np.ones(1), np.full(1, 0.02)
    pd = C.POINTER(C.c_double)
    lines = (_lib.mcalf_line * 1)(_lib.mcalf_line(1548.204, 0.1899, 2.643e8))
    sp = _lib.mcalf_spec(npix=1, wl=wl.ctypes.data_as(pd), flux=one.ctypes.data_as(pd), err=err.ctypes.data_as(pd), velstep=1.0, nlines=1,
                         lines=lines, fill=_lib.mcalf_line(250.0, 0.1899, 2.643e8), ncompmax=2, nfill=0, freespecres=0, freecont=0,
                         specres_fixed=0.5, specres_max=0.5, contval_fixed=1.0, conv_mode=0, device=-1, asymmlike=0, asymm_n4=0.0, asymm_n5=0.0)
    ctx = C.c_void_p()
    _lib.check(lib.mcalf_create(C.byref(sp), C.byref(ctx)))
    try:
        P, W = np.array([[1.0, 13.0, 3.0, 10.0, 13.0, 3.0, 10.0]]), np.zeros(2)
        assert lib.mcalf_eqw_batch(ctx, P.ctypes.data, 1, 0, W.ctypes.data, None) == _lib.MCALF_ERR_INVALID
        assert b"2 pixels" in lib.mcalf_last_error(ctx)
        assert lib.mcalf_eqw_batch_device(ctx, P.ctypes.data, 1, 0, W.ctypes.data, None, None) == _lib.MCALF_ERR_INVALID
        assert b"2 pixels" in lib.mcalf_last_error(ctx)
    finally:
        lib.mcalf_destroy(ctx)


@pytest.fixture(scope="module")
def full_C(cfgC):
    """Config C's 4096 rows through the host entry, both outputs, once for the tests below."""
    kw, batch, seed = cfgC
    P = workloads.draw_P(kw, batch, np.random.default_rng(seed))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        wc, wb = fit.eqw_batch(P)
    assert np.isfinite(wc).all() and np.isfinite(wb).all()
    return kw, P, wc, wb


def test_bits_do_not_depend_on_batch_position_or_outputs(full_C):
    kw, P, wc, wb = full_C
    with mcalf_amd.als_fitter(None, **kw) as fit:
        c, b = fit.eqw_batch(P[100:164])
        assert np.array_equal(c, wc[100:164]) and np.array_equal(b, wb[100:164])
        c, none = fit.eqw_batch(P, blend=False)
        assert none is None and np.array_equal(c, wc)
        none, b = fit.eqw_batch(P, comp=False)
        assert none is None and np.array_equal(b, wb)
        out = (np.full(wc.shape, -7.0), np.full(wb.shape, -7.0))
        got = fit.eqw_batch(P, out=out)
        assert got[0] is out[0] and got[1] is out[1] and np.array_equal(out[0], wc) and np.array_equal(out[1], wb)
        with pytest.raises(ValueError):
            fit.eqw_batch(P, comp=False, blend=False)
        with pytest.raises(ValueError):
            fit.eqw_batch(P, out=(np.zeros(3), None))
    # blending never adds absorption
    s = 1
    z = P[:, s + 2::3][:, :wc.shape[1]]
    assert np.all((wc * (1 + z)[:, :, None]).sum(axis=1) >= wb - 1e-9)


def test_the_device_entry_equals_the_host_entry(full_C):
    kw, P, wc, wb = full_C
    n = len(P)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        dP = torch.from_numpy(P).cuda()
        kept = dP.clone()
        dC = torch.full(wc.shape, -7.0, dtype=torch.float64, device="cuda")
        dB = torch.full(wb.shape, -7.0, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        for _ in range(2):                                               # (the second call allocates nothing)
            dC.fill_(-7.0)
            dB.fill_(-7.0)
            side.wait_stream(torch.cuda.current_stream())
            assert fit._lib.mcalf_eqw_batch_device(fit._ctx, dP.data_ptr(), n, 0, dC.data_ptr(), dB.data_ptr(), C.c_void_p(side.cuda_stream)) == 0
            side.synchronize()
            assert np.array_equal(dC.cpu().numpy(), wc) and np.array_equal(dB.cpu().numpy(), wb)
        assert torch.equal(dP.view(torch.int64), kept.view(torch.int64))
        dB.fill_(-7.0)
        stream = torch.cuda.current_stream().cuda_stream
        assert fit._lib.mcalf_eqw_batch_device(fit._ctx, dP.data_ptr(), n, 0, None, dB.data_ptr(), C.c_void_p(stream)) == 0
        torch.cuda.synchronize()
        assert np.array_equal(dB.cpu().numpy(), wb)
        assert fit._lib.mcalf_eqw_batch_device(fit._ctx, None, 0, 0, dC.data_ptr(), None, None) == 0           # batch == 0: nothing to do
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as fit:
        assert fit.info.ndevices == 2
        c, b = fit.eqw_batch(P)
        assert fit.last_launch().devices_used == 2
        assert np.array_equal(c, wc) and np.array_equal(b, wb)
        rc = fit._lib.mcalf_eqw_batch_device(fit._ctx, dP.data_ptr(), 8, 0, dC.data_ptr(), None, None)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in fit._lib.mcalf_last_error(fit._ctx)


def test_a_batch_of_several_passes_equals_its_halves():
    """A pass holds at most 65535 rows (the row is the pixel kernel's grid.y): 70000 rows of a 2-pixel spectrum are two."""
    kw = _edge_kw(2, 2, 0, nfill=0)
    P = workloads.draw_P(kw, 70000, np.random.default_rng(12))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        wc, wb = fit.eqw_batch(P)
        h = [fit.eqw_batch(P[:35000]), fit.eqw_batch(P[35000:])]
    assert np.array_equal(wc, np.concatenate([h[0][0], h[1][0]])) and np.array_equal(wb, np.concatenate([h[0][1], h[1][1]]))
    assert np.isfinite(wc).all() and (wc[65535:] != 0.0).any()


def test_calc_w_batch_and_calc_N_batch_agree_with_the_single_point_routines(cfgC):
    kw, _, seed = cfgC
    P = workloads.draw_P(kw, 6, np.random.default_rng(seed + 5))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        for ri in (True, False):
            for k in range(2):
                got = fit.calc_w_batch(P, lineid=k, reference_indexing=ri)
                want = np.array([fit.calc_w(p, lineid=k, reference_indexing=ri) for p in P])
                print(f"calc_w_batch line {k}, reference_indexing={ri}: worst error / bar {er.worst(got, want):.3g}")
                assert got.shape == (6,) and er.close(got, want)
        assert np.array_equal(fit.calc_w_batch(P), fit.calc_w_batch(P, lineid=0, reference_indexing=True))
        with pytest.raises(ValueError):
            fit.calc_w_batch(P, lineid=2)
        with np.errstate(divide="ignore"):
            assert np.array_equal(fit.calc_N_batch(P), np.array([fit.calc_N(p, reference_indexing=False) for p in P]))
    kwc = dict(kw, contval=[0.5, 2.0])                                   # free continuum: slot 1
    Pc = workloads.draw_P(kwc, 4, np.random.default_rng(seed + 6))
    Pc[1, 1] = 0.0
    Pc[2, 1] = np.inf
    Pc[3, 2] = 0.0                                                       # no active slot: calc_w returns 0 before it divides
    Pc[3, 1] = 0.0
    with mcalf_amd.als_fitter(None, **kwc) as fit:
        for ri in (True, False):
            got = fit.calc_w_batch(Pc, lineid=1, reference_indexing=ri)
            with np.errstate(all="ignore"):
                want = np.array([fit.calc_w(p, lineid=1, reference_indexing=ri) for p in Pc])
            assert np.isfinite(got[0]) and np.isnan(got[1]) and np.isnan(got[2]) and er.close(got, want), (ri, got, want)
        assert fit.calc_w_batch(Pc, lineid=1, reference_indexing=False)[3] == 0.0
