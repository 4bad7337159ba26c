"""CPU: the argument checks of mcalf_ensemble_batch[_device] that need no device (every refusal comes before any device work
and names the argument), the options struct, the Python signatures, and the host driver `ensemble.ensemble_sample` over the
numpy restatement of the step."""
import ctypes as C
import inspect

import numpy as np
import pytest

import ens_reference as er
import mcalf_amd
from mcalf_amd import _lib, ensemble


def _opts(**over):
    kw = dict(nsteps=8, thin=2, move=0, reserved=0, scale=2.0, seed=1, first_iter=0)
    kw.update(over)
    return _lib.mcalf_ens_opts(**kw)


def test_the_options_struct_matches_the_header_layout():
    o = _lib.mcalf_ens_opts
    assert C.sizeof(o) == 40
    assert [getattr(o, f).offset for f in ("nsteps", "thin", "move", "reserved", "scale", "seed", "first_iter")] == [0, 4, 8, 12, 16, 24, 32]
    assert (_lib.MCALF_ENS_STRETCH, _lib.MCALF_ENS_DE) == (0, 1) == (er.STRETCH, er.DE)


def test_ensemble_entries_refuse_invalid_arguments_without_a_device():
    lib = _lib.load()
    U0, U, th = np.full((4, 3), 0.5), np.zeros((4, 3)), np.zeros((4, 3))
    L, CU, CL = np.zeros(4), np.zeros((4, 4, 3)), np.zeros((4, 4))
    st, na = (np.zeros(4, dtype=np.int32) for _ in range(2))
    host = lambda ctx, n, o, *a: lib.mcalf_ensemble_batch(ctx, a[0], n, o, *a[1:])
    dev = lambda ctx, n, o, *a: lib.mcalf_ensemble_batch_device(ctx, a[0], n, o, *a[1:], None)
    names = (b"U0", b"U", None, b"logL", b"status", b"naccept", None, None)       # (theta, CU and CL may be NULL)
    for call, name in ((host, b"mcalf_ensemble_batch"), (dev, b"mcalf_ensemble_batch_device")):
        arrs = tuple(a.ctypes.data for a in (U0, U, th, L, st, na, CU, CL))
        ok = _opts()
        assert call(None, 4, C.addressof(ok), *arrs) == _lib.MCALF_ERR_INVALID
        assert name + b": ctx is NULL" in lib.mcalf_last_error(None)
        assert call(None, 4, None, *arrs) == _lib.MCALF_ERR_INVALID
        assert name + b": opts is NULL" in lib.mcalf_last_error(None)
        for n, what in ((-2, b"nwalkers must be >= 0"), (5, b"nwalkers must be even"), (7, b"nwalkers must be even"), (2, b"nwalkers must be >= 4")):
            assert call(None, n, C.addressof(ok), *arrs) == _lib.MCALF_ERR_INVALID
            assert name + b": " + what in lib.mcalf_last_error(None), (n, lib.mcalf_last_error(None))
        for k, what in enumerate(names):
            a = list(arrs)
            a[k] = None
            assert call(None, 4, C.addressof(ok), *a) == _lib.MCALF_ERR_INVALID
            assert (what + b" is NULL" if what else b"ctx is NULL") in lib.mcalf_last_error(None), (k, lib.mcalf_last_error(None))
        inf, nan = float("inf"), float("nan")
        for over, what in ((dict(nsteps=-1), b"nsteps must be"), (dict(thin=0), b"thin must be"), (dict(thin=-3), b"thin must be"),
                           (dict(move=2), b"move must be"), (dict(move=-1), b"move must be"),
                           (dict(scale=nan), b"scale must be finite"), (dict(scale=inf), b"scale must be finite"),
                           (dict(scale=-inf, move=1), b"scale must be finite"),
                           (dict(scale=1.0), b"scale must be > 1 for the stretch move"), (dict(scale=0.5), b"scale must be > 1 for the stretch move"),
                           (dict(scale=0.0, move=1), b"scale must be > 0 for the DE move"), (dict(scale=-0.3, move=1), b"scale must be > 0 for the DE move")):
            bad = _opts(**over)
            assert call(None, 4, C.addressof(bad), *arrs) == _lib.MCALF_ERR_INVALID
            assert name + b": " + what in lib.mcalf_last_error(None), (over, lib.mcalf_last_error(None))
        fine = _opts(scale=0.5, move=1)                                            # (a DE scale below 1 is a scale like any other)
        assert call(None, 4, C.addressof(fine), *arrs) == _lib.MCALF_ERR_INVALID and b"ctx is NULL" in lib.mcalf_last_error(None)
        assert call(None, 0, C.addressof(ok), *([None] * 8)) == _lib.MCALF_ERR_INVALID       # (ctx is NULL)
        assert b"ctx is NULL" in lib.mcalf_last_error(None)


def test_the_python_signatures():
    sig = inspect.signature(mcalf_amd.als_fitter.ensemble_batch)
    got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert got == dict(thin=1, move="stretch", scale=None, seed=0, first_iter=0, chain=True)
    assert list(sig.parameters)[1:3] == ["U0", "nsteps"]
    assert callable(mcalf_amd.als_fitter.ensemble_sample)
    sig = inspect.signature(mcalf_amd.ensemble.ensemble_sample)
    assert list(sig.parameters) == ["loglike_cube", "advance", "ndim", "nwalkers", "nsteps", "burn", "thin", "start", "ball", "seed"]
    assert sig.parameters["thin"].default == 1 and sig.parameters["burn"].default == 0 and sig.parameters["seed"].default == 0
    for name in ("autocorr_time", "flat", "means"):
        assert callable(getattr(ensemble.EnsembleResult, name))
    assert list(inspect.signature(ensemble.batch_means_se).parameters) == ["x", "nbatch"]
    imports = [line.strip() for line in open(ensemble.__file__) if line.startswith(("import ", "from "))]
    assert imports == ["from __future__ import annotations", "import numpy as np"]                # pure numpy, nothing of the package


def test_the_driver_over_the_reference_callables():
    logl = lambda U: -0.5 * (((U - 0.5) / 0.05) ** 2).sum(axis=1)
    lo, hi = np.array([1.0, -2.0, 10.0]), np.array([3.0, 2.0, 20.0])
    transform = lambda U: lo + U * (hi - lo)
    cube_ll = lambda U: (transform(U), logl(U))
    for move in (er.STRETCH, er.DE):
        adv = er.advance_with(logl, move, transform=transform)
        res = ensemble.ensemble_sample(cube_ll, adv, 3, 8, 40, burn=10, thin=4, start=[0.5, 0.5, 0.5], ball=0.05, seed=5)
        assert res.cube.shape == res.theta.shape == (10, 8, 3) and res.logL.shape == (10, 8)
        assert np.array_equal(res.theta, transform(res.cube)) and res.logL.tobytes() == logl(res.cube.reshape(-1, 3)).tobytes()
        assert res.accept_frac.shape == (8,) and (res.accept_frac > 0.0).all() and (res.accept_frac <= 1.0).all()
        # burn-in and kept run are one run of 50 iterations from the same starts
        U0 = np.clip(0.5 + 0.05 * (2.0 * np.random.default_rng(5).random((8, 3)) - 1.0), 0.0, 1.0)
        whole = er.ensemble(logl, U0, 50, 1, move, seed=5)
        assert res.last.tobytes() == whole[0].tobytes()
        assert res.cube.tobytes() == whole[4][10:][3::4].tobytes()
        ll, th = res.flat()
        assert ll.shape == (80,) and th.shape == (80, 3) and th.flags.c_contiguous
        assert res.autocorr_time().shape == (3,) and res.means().shape == (10, 3)
        uniform = ensemble.ensemble_sample(cube_ll, adv, 3, 8, 0, seed=5)         # no start: the whole cube; no step: an empty chain
        assert uniform.cube.shape == (0, 8, 3) and uniform.last.tobytes() == np.random.default_rng(5).random((8, 3)).tobytes()
    for bad in (dict(nwalkers=5), dict(nwalkers=2), dict(thin=0), dict(start=[0.5] * 3), dict(ball=0.1), dict(nsteps=-1)):
        kw = dict(nwalkers=8, nsteps=4, thin=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            ensemble.ensemble_sample(cube_ll, adv, 3, **kw)
