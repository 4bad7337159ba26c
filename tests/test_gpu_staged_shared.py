"""GPU: the host-pointer analysis entries share ONE staging arena per context (host_staged.cpp: run_staged, `stage_dev`), carved
per call in column order with every column on a 256-byte boundary.  Issued back to back on one context, in an order that makes
the arena grow, need less and grow again, every output of every entry equals by bytes the same call on a fresh context of its own
-- with every optional output given, and with every one of them NULL.  The row counts are odd on purpose: with ndim 4 they put
the int32 columns (status, nevals, moves, naccept, niter) and the bands' int64 nvalid behind double columns of odd length, where a
carve without alignment would show.  Every call reports MCALF_PATH_HOST_STAGED and the page-lockedness of the arrays its entry
has always reported.  One problem: cases.tiny_problem(64), prior set."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcalf_amd
from cases import tiny_problem
from mcalf_amd import _lib

pytestmark = pytest.mark.gpu

NPIX = 64


def _fit():
    fit = mcalf_amd.als_fitter(None, **tiny_problem(NPIX))
    fit._ensure_prior()
    return fit


def _rows(fit, n, seed):
    """`n` parameter rows inside the prior box."""
    return fit._lo + (fit._hi - fit._lo) * np.random.default_rng(seed).random((n, fit.ndim))


def _ptr(a):
    return None if a is None else a.ctypes.data


def _f64(*shape):
    return np.full(shape, -7.0)


def _i32(n):
    return np.full(n, -7, dtype=np.int32)


# Every call: (fit, opt) -> its outputs in the entry's order; opt False: every optional output is NULL (and missing below).

def grad(fit, opt, P=None, G=None):
    P = _rows(fit, 3, 1) if P is None else P
    L, G = (_f64(3) if opt else None), (_f64(3, fit.ndim) if G is None else G)
    assert fit._lib.mcalf_loglike_grad_batch(fit._ctx, _ptr(P), 3, _ptr(L), _ptr(G)) == 0
    return L, G


def ensemble(fit, opt):
    n, nsteps = 8, 2
    U0 = np.random.default_rng(2).random((n, fit.ndim))
    opts = _lib.mcalf_ens_opts(nsteps, 1, _lib.MCALF_ENS_STRETCH, 0, 2.0, 5, 0)
    U, theta, L, status, naccept = _f64(n, fit.ndim), (_f64(n, fit.ndim) if opt else None), _f64(n), _i32(n), _i32(n)
    CU, CL = (_f64(nsteps, n, fit.ndim), _f64(nsteps, n)) if opt else (None, None)
    assert fit._lib.mcalf_ensemble_batch(fit._ctx, _ptr(U0), n, C.addressof(opts), _ptr(U), _ptr(theta), _ptr(L), _ptr(status), _ptr(naccept),
                                         _ptr(CU), _ptr(CL)) == 0
    return U, theta, L, status, naccept, CU, CL


def eqw(fit, opt, Wcomp=None, Wblend=None, comp=True):
    P = _rows(fit, 5, 3)
    Wcomp = (_f64(5, int(fit.ncompmax), fit.numlines) if Wcomp is None else Wcomp) if opt and comp else None
    Wblend = _f64(5, fit.numlines) if Wblend is None else Wblend
    assert fit._lib.mcalf_eqw_batch(fit._ctx, _ptr(P), 5, _lib.MCALF_EQW_LAYOUT, _ptr(Wcomp), _ptr(Wblend)) == 0
    return Wcomp, Wblend


def slice_step(fit, opt):
    n = 3
    U0 = np.random.default_rng(4).random((n, fit.ndim))
    Lmin, D, sid = np.full(n, -1e300), np.eye(fit.ndim), np.arange(n, dtype=np.uint64) + 11
    opts = _lib.mcalf_slice_opts(2, 20, fit.ndim, 0, 9)
    U, theta, L = _f64(n, fit.ndim), (_f64(n, fit.ndim) if opt else None), _f64(n)
    status, nevals, moves = _i32(n), _i32(n), _i32(n)
    assert fit._lib.mcalf_slice_replace_batch(fit._ctx, _ptr(U0), _ptr(Lmin), _ptr(D), _ptr(sid), n, C.addressof(opts), _ptr(U), _ptr(theta),
                                              _ptr(L), _ptr(status), _ptr(nevals), _ptr(moves)) == 0
    return U, theta, L, status, nevals, moves


def band(fit, opt, mean=None):
    P = _rows(fit, 4, 5)
    q = np.array([0.25, 0.75]) if opt else None
    nq = 2 if opt else 0
    mean = _f64(NPIX) if mean is None else mean
    var, Q, nvalid = (_f64(NPIX) if opt else None), (_f64(nq, NPIX) if opt else None), np.full(NPIX, -7, dtype=np.int64)
    assert fit._lib.mcalf_model_band_batch(fit._ctx, _ptr(P), 4, 0, _ptr(q), nq, _ptr(mean), _ptr(var), _ptr(Q), _ptr(nvalid)) == 0
    return mean, var, Q, nvalid


def maximize(fit, opt):
    P0 = _rows(fit, 2, 6)
    opts = _lib.mcalf_fit_opts(2, 0, 0, 0, 1e-3, 1e-10)
    P, L, status, niter = _f64(2, fit.ndim), _f64(2), _i32(2), _i32(2)
    assert fit._lib.mcalf_maximize_batch(fit._ctx, _ptr(P0), 2, C.addressof(opts), _ptr(P), _ptr(L), _ptr(status), _ptr(niter)) == 0
    return P, L, status, niter


def fisher(fit, opt):
    P, V = _rows(fit, 3, 7), np.random.default_rng(8).standard_normal((3, fit.ndim))
    FV = _f64(3, fit.ndim)
    assert fit._lib.mcalf_fisher_matvec_batch(fit._ctx, _ptr(P), _ptr(V), 3, _ptr(FV)) == 0
    return (FV,)


# The arena's need: gradient 2 columns, ensemble 6, equivalent widths 3, slice step 10, bands 5 of 64 pixels, fit 5, Fisher 3,
# gradient again.
SEQUENCE = (grad, ensemble, eqw, slice_step, band, maximize, fisher, grad)


def _bytes(outs):
    """The outputs' bytes (None for one that was not asked for); no entry still holds the -7 the arrays were filled with."""
    assert all(a is None or not (a == -7).any() for a in outs)
    return tuple(None if a is None else a.tobytes() for a in outs)


# (call, index) of the outputs a call may leave out
OPTIONAL = {(grad, 0), (ensemble, 1), (ensemble, 5), (ensemble, 6), (eqw, 0), (slice_step, 1), (band, 1), (band, 2)}


@pytest.fixture(scope="module")
def alone():
    """{(call, opt): its outputs' bytes on a fresh context that makes no other call}."""
    ref = {}
    for opt in (True, False):
        for call in set(SEQUENCE):
            fit = _fit()
            try:
                ref[call, opt] = _bytes(call(fit, opt))
            finally:
                fit.close()
    return ref


@pytest.mark.parametrize("opt", [True, False], ids=["all-outputs", "optional-null"])
def test_back_to_back_on_one_context(alone, opt):
    fit = _fit()
    try:
        got = []
        for call in SEQUENCE:
            got.append(_bytes(call(fit, opt)))
            ll = fit.last_launch()
            assert (ll.path, ll.pinned_in, ll.pinned_out) == (_lib.MCALF_PATH_HOST_STAGED, 0, 0), call.__name__
    finally:
        fit.close()
    for call, outs in zip(SEQUENCE, got):
        assert len(outs) == len(alone[call, opt])
        for k, (a, b) in enumerate(zip(outs, alone[call, opt])):
            assert a == b, f"{call.__name__}: output {k} differs from the call on a fresh context"
            assert (a is None) == (not opt and (call, k) in OPTIONAL)
    assert got[-1] == got[0]


def _pinned(*shape):
    return torch.full(shape, -7.0, dtype=torch.float64).pin_memory().numpy()


def test_pinned_flags(alone):
    """What each entry has always recorded: the parameter rows in; the primary output out -- never for the bands, Wcomp if
    given else Wblend for the equivalent widths."""
    fit = _fit()
    try:
        def flags():
            ll = fit.last_launch()
            return ll.path, ll.pinned_in, ll.pinned_out

        staged = _lib.MCALF_PATH_HOST_STAGED
        Ppin = torch.from_numpy(_rows(fit, 3, 1)).pin_memory().numpy()
        assert _bytes(grad(fit, True, P=Ppin)) == alone[grad, True] and flags() == (staged, 1, 0)
        assert _bytes(grad(fit, True, P=Ppin, G=_pinned(3, fit.ndim))) == alone[grad, True] and flags() == (staged, 1, 1)
        assert _bytes(eqw(fit, True, Wblend=_pinned(5, fit.numlines))) == alone[eqw, True] and flags() == (staged, 0, 0)
        assert _bytes(eqw(fit, True, Wcomp=_pinned(5, int(fit.ncompmax), fit.numlines))) == alone[eqw, True] and flags() == (staged, 0, 1)
        assert _bytes(eqw(fit, True, Wblend=_pinned(5, fit.numlines), comp=False)) == alone[eqw, False] and flags() == (staged, 0, 1)
        assert _bytes(band(fit, True, mean=_pinned(NPIX))) == alone[band, True] and flags() == (staged, 0, 0)
    finally:
        fit.close()
