"""CPU: the argument checks of mcalf_maximize_batch[_device] and mcalf_fisher_matvec_batch[_device] that need no device
(every refusal comes before any device work and names the argument), and the Python methods."""
import ctypes as C

import numpy as np

from mcalf_amd import _lib

NAN = float("nan")


def _opts(**over):
    kw = dict(max_iter=5, cg_iters=0, rows_per_block=0, reserved=0, lambda0=1e-3, ftol=1e-10)
    kw.update(over)
    return _lib.mcalf_fit_opts(**kw)


def test_the_options_struct_matches_the_header_layout():
    assert C.sizeof(_lib.mcalf_fit_opts) == 4 * 4 + 2 * 8
    assert _lib.mcalf_fit_opts.lambda0.offset == 16 and _lib.mcalf_fit_opts.ftol.offset == 24


def test_fit_entries_refuse_invalid_arguments_without_a_device():
    lib = _lib.load()
    P0, P = np.zeros((2, 4)), np.zeros((2, 4))
    L = np.zeros(2)
    st, ni = np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int32)
    host = lambda ctx, p0, n, o, *outs: lib.mcalf_maximize_batch(ctx, p0, n, o, *outs)
    dev = lambda ctx, p0, n, o, *outs: lib.mcalf_maximize_batch_device(ctx, p0, n, o, *outs, None)
    for call, name in ((host, b"mcalf_maximize_batch"), (dev, b"mcalf_maximize_batch_device")):
        outs = (P.ctypes.data, L.ctypes.data, st.ctypes.data, ni.ctypes.data)
        ok = _opts()
        assert call(None, P0.ctypes.data, 2, C.addressof(ok), *outs) == _lib.MCALF_ERR_INVALID
        assert name + b": ctx is NULL" in lib.mcalf_last_error(None)
        assert call(None, P0.ctypes.data, 2, None, *outs) == _lib.MCALF_ERR_INVALID
        assert b"opts is NULL" in lib.mcalf_last_error(None)
        assert call(None, P0.ctypes.data, -1, C.addressof(ok), *outs) == _lib.MCALF_ERR_INVALID
        assert b"batch must be >= 0" in lib.mcalf_last_error(None)
        assert call(None, None, 2, C.addressof(ok), *outs) == _lib.MCALF_ERR_INVALID
        assert b"P0 is NULL" in lib.mcalf_last_error(None)
        for k, what in enumerate((b"P is NULL", b"logL is NULL", b"status is NULL", b"niter is NULL")):
            o = list(outs)
            o[k] = None
            assert call(None, P0.ctypes.data, 2, C.addressof(ok), *o) == _lib.MCALF_ERR_INVALID
            assert what in lib.mcalf_last_error(None)
        for over, what in ((dict(lambda0=0.0), b"lambda0"), (dict(lambda0=-1.0), b"lambda0"), (dict(lambda0=NAN), b"lambda0"),
                           (dict(lambda0=float("inf")), b"lambda0"), (dict(ftol=NAN), b"ftol"), (dict(ftol=-1e-3), b"ftol"),
                           (dict(max_iter=-1), b"max_iter"), (dict(cg_iters=-2), b"cg_iters"), (dict(rows_per_block=-1), b"rows_per_block")):
            bad = _opts(**over)
            assert call(None, P0.ctypes.data, 2, C.addressof(bad), *outs) == _lib.MCALF_ERR_INVALID
            assert what in lib.mcalf_last_error(None), (over, lib.mcalf_last_error(None))
        assert call(None, None, 0, C.addressof(ok), None, None, None, None) == _lib.MCALF_ERR_INVALID      # (ctx is NULL)


def test_fisher_entries_refuse_invalid_arguments_without_a_device():
    lib = _lib.load()
    P, V, FV = np.zeros((2, 4)), np.zeros((2, 4)), np.zeros((2, 4))
    host = lambda ctx, p, v, n, fv: lib.mcalf_fisher_matvec_batch(ctx, p, v, n, fv)
    dev = lambda ctx, p, v, n, fv: lib.mcalf_fisher_matvec_batch_device(ctx, p, v, n, fv, None)
    for call, name in ((host, b"mcalf_fisher_matvec_batch"), (dev, b"mcalf_fisher_matvec_batch_device")):
        assert call(None, P.ctypes.data, V.ctypes.data, 2, FV.ctypes.data) == _lib.MCALF_ERR_INVALID
        assert name + b": ctx is NULL" in lib.mcalf_last_error(None)
        assert call(None, P.ctypes.data, V.ctypes.data, -1, FV.ctypes.data) == _lib.MCALF_ERR_INVALID
        assert b"batch must be >= 0" in lib.mcalf_last_error(None)
        assert call(None, None, V.ctypes.data, 2, FV.ctypes.data) == _lib.MCALF_ERR_INVALID
        assert b"P is NULL" in lib.mcalf_last_error(None)
        assert call(None, P.ctypes.data, None, 2, FV.ctypes.data) == _lib.MCALF_ERR_INVALID
        assert b"V is NULL" in lib.mcalf_last_error(None)
        assert call(None, P.ctypes.data, V.ctypes.data, 2, None) == _lib.MCALF_ERR_INVALID
        assert b"FV is NULL" in lib.mcalf_last_error(None)
        assert call(None, None, None, 0, None) == _lib.MCALF_ERR_INVALID


def test_the_python_methods_exist():
    import inspect

    import mcalf_amd
    for name in ("maximize_batch", "maximize", "fisher_matvec_batch"):
        assert callable(getattr(mcalf_amd.als_fitter, name))
    sig = inspect.signature(mcalf_amd.als_fitter.maximize_batch)
    got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert got == dict(max_iter=50, cg_iters=None, lambda0=1e-3, ftol=1e-10, rows_per_block=0)
