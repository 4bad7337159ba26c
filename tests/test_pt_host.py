"""CPU: the argument checks of mcalf_tempered_batch[_device] that need no device (every refusal comes before any device work and
names the argument), the options struct and the Python signatures."""
import ctypes as C
import inspect

import numpy as np

import mcalf_amd
from mcalf_amd import _lib, tempering


def _opts(**over):
    kw = dict(nsteps=8, thin=2, move=0, ntemps=3, swap_every=1, chain_temps=1, scale=2.0, seed=1, first_iter=0)
    kw.update(over)
    return _lib.mcalf_pt_opts(**kw)


def test_the_options_struct_matches_the_header_layout():
    o = _lib.mcalf_pt_opts
    assert C.sizeof(o) == 48
    names = ("nsteps", "thin", "move", "ntemps", "swap_every", "chain_temps", "scale", "seed", "first_iter")
    assert [f for f, _ in o._fields_] == list(names)
    assert [getattr(o, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 32, 40]
    assert _lib.MCALF_PT_MAX_TEMPS == 64


def test_tempered_entries_refuse_invalid_arguments_without_a_device():
    lib = _lib.load()
    T, n, nd = 3, 4, 3
    U0, U, th = np.full((T, n, nd), 0.5), np.zeros((T, n, nd)), np.zeros((T, n, nd))
    L, CU, CL = np.zeros((T, n)), np.zeros((4, 1, n, nd)), np.zeros((4, T, n))
    st, na = (np.zeros((T, n), dtype=np.int32) for _ in range(2))
    ns = np.zeros((T - 1, n), dtype=np.int32)
    beta = np.array([1.0, 0.5, 0.0])
    host = lambda ctx, n_, b, o, *a: lib.mcalf_tempered_batch(ctx, a[0], n_, b, o, *a[1:])
    dev = lambda ctx, n_, b, o, *a: lib.mcalf_tempered_batch_device(ctx, a[0], n_, b, o, *a[1:], None)
    names = (b"U0", b"U", None, b"logL", b"status", b"naccept", b"nswap", None, None)       # (theta, CU and CL may be NULL)
    for call, name in ((host, b"mcalf_tempered_batch"), (dev, b"mcalf_tempered_batch_device")):
        arrs = tuple(a.ctypes.data for a in (U0, U, th, L, st, na, ns, CU, CL))
        ok = _opts()

        def refused(what, n_=n, b=beta, o=ok, a=arrs, code=_lib.MCALF_ERR_INVALID):
            assert call(None, n_, b.ctypes.data if b is not None else None, C.addressof(o) if o is not None else None, *a) == code, what
            assert name + b": " + what in lib.mcalf_last_error(None), (what, lib.mcalf_last_error(None))

        refused(b"ctx is NULL")                                                    # (all else is in order)
        refused(b"opts is NULL", o=None)
        for nw, what in ((-2, b"nwalkers must be >= 0"), (5, b"nwalkers must be even"), (2, b"nwalkers must be >= 4")):
            refused(what, n_=nw)
        for k, what in enumerate(names):
            a = list(arrs)
            a[k] = None
            refused(what + b" is NULL" if what else b"ctx is NULL", a=a)
        a = list(arrs)
        a[6] = None
        refused(b"ctx is NULL", b=np.array([1.0]), o=_opts(ntemps=1), a=a)          # (one rung has no nswap)
        refused(b"beta is NULL", b=None)
        for nt in (0, -1, 65):
            refused(b"ntemps must be in [1, 64]", o=_opts(ntemps=nt))
        refused(b"ctx is NULL", b=np.linspace(1.0, 0.0, 64), o=_opts(ntemps=64))
        inf, nan = float("inf"), float("nan")
        for b, what in (([1.0, nan, 0.0], b"beta[1] must be finite"), ([inf, 1.0, 0.0], b"beta[0] must be finite"), ([1.0, 0.5, -0.1], b"beta[2] must be >= 0"),
                        ([1.0, 1.0, 0.0], b"beta must be strictly decreasing"), ([0.5, 1.0, 0.0], b"beta must be strictly decreasing"),
                        ([1.0, 0.0, 0.0], b"beta must be strictly decreasing")):
            refused(what, b=np.array(b))
        refused(b"ctx is NULL", b=np.array([7.5, 1.0, 0.25]))                      # (a ladder need start at 1 or end at 0 no more than this)
        for over, what in ((dict(swap_every=-1), b"swap_every must be >= 0"), (dict(chain_temps=-1), b"chain_temps must be in [0, ntemps = 3]"),
                           (dict(chain_temps=4), b"chain_temps must be in [0, ntemps = 3]"),
                           (dict(nsteps=-1), b"nsteps must be"), (dict(thin=0), b"thin must be"), (dict(move=2), b"move must be"),
                           (dict(scale=nan), b"scale must be finite"), (dict(scale=1.0), b"scale must be > 1 for the stretch move"),
                           (dict(scale=0.0, move=1), b"scale must be > 0 for the DE move")):
            refused(what, o=_opts(**over))
        for over in (dict(swap_every=0), dict(chain_temps=0), dict(chain_temps=3), dict(swap_every=2 ** 31 - 1)):
            refused(b"ctx is NULL", o=_opts(**over))
        assert 3 * 715806036 <= 0x7fff0000 < 3 * 715806038
        refused(b"ntemps x nwalkers = 3 x 715806038 rows too large", n_=715806038, code=_lib.MCALF_ERR_RANGE)
        refused(b"ctx is NULL", n_=715806036)
        assert call(None, 0, beta.ctypes.data, C.addressof(ok), *([None] * 9)) == _lib.MCALF_ERR_INVALID
        assert b"ctx is NULL" in lib.mcalf_last_error(None)


def test_the_python_signatures():
    sig = inspect.signature(mcalf_amd.als_fitter.tempered_batch)
    assert list(sig.parameters)[1:4] == ["U0", "betas", "nsteps"]
    got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert got == dict(thin=1, swap_every=1, move="stretch", scale=None, seed=0, first_iter=0, chain=True, chain_temps=1)
    sig = inspect.signature(mcalf_amd.als_fitter.tempered_sample)
    assert list(sig.parameters)[1:] == ["nwalkers", "nsteps", "ntemps", "betas", "burn", "thin", "swap_every", "start", "ball", "seed", "move", "scale"]
    got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert got == dict(ntemps=8, betas=None, burn=0, thin=1, swap_every=1, start=None, ball=None, seed=0, move="stretch", scale=None)
    sig = inspect.signature(tempering.tempered_sample)
    assert list(sig.parameters) == ["loglike_cube", "advance", "ndim", "nwalkers", "nsteps", "betas", "burn", "thin", "swap_every", "start", "ball", "seed"]
    assert list(inspect.signature(tempering.default_ladder).parameters) == ["ntemps", "beta_min"]
    for name in ("cold", "logZ_stepping_stone", "logZ_ti"):
        assert callable(getattr(tempering.TemperedResult, name))
    assert inspect.signature(tempering.TemperedResult.logZ_stepping_stone).parameters["nbatch"].default == 20
    imports = [line.strip() for line in open(tempering.__file__) if line.startswith(("import ", "from "))]
    assert imports == ["from __future__ import annotations", "import numpy as np", "from .ensemble import EnsembleResult"]      # numpy over callables
