"""CPU: what of the batched equivalent widths can be checked without a device -- the numpy restatement the GPU tests
compare against (tests/eqw_reference.py) reproduces the oracle's calc_w, the two C entries refuse every bad argument before
they touch a device, the ABI number stands, and calc_N_batch's host arithmetic equals calc_N's bit for bit."""
import types

import numpy as np
import pytest

import eqw_reference as er
import mcalf_amd
from cases import oracle_synth, problem_from_kwargs
from mcalf_amd import _lib, workloads
from oracle import numpy_oracle as o


@pytest.fixture(scope="module")
def cfgC():
    return workloads.config("C", oracle_synth)


def test_the_restatement_reproduces_the_oracles_calc_w(cfgC):
    """Component sums of the restatement against o.calc_w_intended / o.calc_w_reference on config C draws.  The two differ
    only in (cont v) / cont against v -- one rounding of v <= 1 per pixel, 1.1e-16 sum(dlambda) = 4.4e-15 Angstrom per slot
    over the 40 Angstrom window -- and in the order the slots are added (a few ulp of W): bar 1e-12 + 1e-12 |W|."""
    kw, _, seed = cfgC
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 3, np.random.default_rng(seed + 5))
    for p in P:
        lay, _ = er.eqw(prob, p, reference_indexing=False)
        ref, _ = er.eqw(prob, p, reference_indexing=True)
        nc = int(p[prob.startind])
        assert np.all(lay[nc:] == 0.0) and np.all(lay[:nc] > 0.0)
        for k in range(prob.numlines):
            want = o.calc_w_intended(prob, p, lineid=k)
            assert abs(lay[:, k].sum() - want) <= 1e-12 + 1e-12 * abs(want)
            want = o.calc_w_reference(prob, p, lineid=k)
            assert np.isfinite(want) and abs(ref[:, k].sum() - want) <= 1e-12 + 1e-12 * abs(want)
        # blending never adds absorption
        z = p[prob.startind + 1 + 3 * np.arange(prob.ncompmax) + 1]
        _, blend = er.eqw(prob, p)
        assert np.all((lay * (1 + z)[:, None]).sum(axis=0) >= blend - 1e-9)


def test_the_restatement_counts_slots_as_the_likelihood_does():
    prob = types.SimpleNamespace(startind=1, ncompmax=3, freespecres=True, freecont=False, contval=[1.0])
    for slot, nc in [(2.7, 2), (-0.5, 0), (-1.5, 0), (0.0, 0), (0.9, 0), (3.0, 3), (9.0, 3), (np.nan, 0), (np.inf, 0), (-np.inf, 0)]:
        p = np.array([8.0, slot])
        assert er.active_count(prob, p) == nc and er.active_count(prob, p, jax=True) == nc


def _call(lib, name, ctx, P, batch, indexing, wc, wb):
    if name.endswith("_device"):
        return getattr(lib, name)(ctx, P, batch, indexing, wc, wb, None)
    return getattr(lib, name)(ctx, P, batch, indexing, wc, wb)


@pytest.mark.parametrize("name", ["mcalf_eqw_batch", "mcalf_eqw_batch_device"])
def test_argument_errors_are_refused_with_a_message(name):
    """Code -1 and a message that names the argument, before any device work: none of these needs a device (the spectrum
    of fewer than 2 pixels needs a context, tests/test_gpu_eqw.py)."""
    lib = _lib.load()
    buf = np.zeros(64)
    ptr = buf.ctypes.data
    for args, needle in [
        ((None, ptr, -1, 0, ptr, ptr), "batch"),
        ((None, None, 4, 0, ptr, ptr), "P is NULL"),
        ((None, ptr, 4, 0, None, None), "Wcomp and Wblend"),
        ((None, ptr, 4, 2, ptr, ptr), "indexing"),
        ((None, ptr, 4, -1, ptr, None), "indexing"),
        ((None, ptr, 4, 1, None, ptr), "ctx is NULL"),
        ((None, ptr, 0, 0, ptr, ptr), "ctx is NULL"),
    ]:
        assert _call(lib, name, *args) == _lib.MCALF_ERR_INVALID, args
        msg = lib.mcalf_last_error(None).decode()
        assert needle in msg and name + ":" in msg, (args, msg)


def test_abi_number_and_bindings():
    lib = _lib.load()
    assert b"abi 9" in lib.mcalf_version()
    assert "mcalf_eqw_batch" in _lib.SYMBOLS and "mcalf_eqw_batch_device" in _lib.SYMBOLS
    assert (_lib.MCALF_EQW_LAYOUT, _lib.MCALF_EQW_AS_WRITTEN) == (0, 1)
    for name in ("eqw_batch", "calc_w_batch", "calc_N_batch"):
        assert callable(getattr(mcalf_amd.als_fitter, name))


@pytest.mark.parametrize("startind,ncompmax,nfill", [(0, 1, 0), (1, 11, 4), (2, 16, 0), (2, 3, 2)])
def test_calc_N_batch_equals_calc_N_bit_for_bit(startind, ncompmax, nfill):
    """Host numpy only, so it runs here on a stand-in for `self`: random rows whose z straddle the z < 10 cut in every
    pattern (so rows keep different slots), fillers at z ~ 24, a row that keeps nothing (-inf)."""
    fit = types.SimpleNamespace(startind=startind, ndim=startind + 1 + 3 * (ncompmax + nfill))
    fit._rows = types.MethodType(mcalf_amd.als_fitter._rows, fit)
    rng = np.random.default_rng(startind + 10 * ncompmax)
    P = rng.uniform(11.0, 21.0, (200, fit.ndim))
    P[:, startind + 2::3] = np.where(rng.random((200, ncompmax + nfill)) < 0.3, 24.0, 3.0)
    P[:, startind + 2 + 3 * ncompmax::3] = 24.0
    P[7, startind + 2::3] = 24.0
    got = mcalf_amd.als_fitter.calc_N_batch(fit, P)
    with np.errstate(divide="ignore"):
        want = np.array([mcalf_amd.als_fitter.calc_N(fit, p, reference_indexing=False) for p in P])
    assert got[7] == -np.inf
    assert np.array_equal(got, want)
