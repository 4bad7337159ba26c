"""CPU: the argument checks of mcalf_slice_replace_batch[_device] that need no device (every refusal comes before any device
work and names the argument), the options struct and the Python methods."""
import ctypes as C
import inspect

import numpy as np

import mcalf_amd
from mcalf_amd import _lib


def _opts(**over):
    kw = dict(nmoves=8, max_steps=400, ndirs=4, reserved=0, seed=1)
    kw.update(over)
    return _lib.mcalf_slice_opts(**kw)


def test_the_options_struct_matches_the_header_layout():
    assert C.sizeof(_lib.mcalf_slice_opts) == 4 * 4 + 8
    assert _lib.mcalf_slice_opts.ndirs.offset == 8 and _lib.mcalf_slice_opts.seed.offset == 16
    assert (_lib.MCALF_SLICE_MAXSTEPS, _lib.MCALF_SLICE_DONE, _lib.MCALF_SLICE_BAD_START) == (0, 1, -1)


def test_slice_entries_refuse_invalid_arguments_without_a_device():
    lib = _lib.load()
    U0, U, th, D = np.full((2, 4), 0.5), np.zeros((2, 4)), np.zeros((2, 4)), np.eye(4)
    Lmin, L = np.zeros(2), np.zeros(2)
    sid = np.arange(2, dtype=np.uint64)
    st, ne, mv = (np.zeros(2, dtype=np.int32) for _ in range(3))
    host = lambda ctx, n, o, *a: lib.mcalf_slice_replace_batch(ctx, a[0], a[1], a[2], a[3], n, o, *a[4:])
    dev = lambda ctx, n, o, *a: lib.mcalf_slice_replace_batch_device(ctx, a[0], a[1], a[2], a[3], n, o, *a[4:], None)
    names = (b"U0", b"Lmin", b"D", b"sid", b"U", None, b"logL", b"status", b"nevals", b"moves")       # (theta may be NULL)
    for call, name in ((host, b"mcalf_slice_replace_batch"), (dev, b"mcalf_slice_replace_batch_device")):
        arrs = tuple(a.ctypes.data for a in (U0, Lmin, D, sid, U, th, L, st, ne, mv))
        ok = _opts()
        assert call(None, 2, C.addressof(ok), *arrs) == _lib.MCALF_ERR_INVALID
        assert name + b": ctx is NULL" in lib.mcalf_last_error(None)
        assert call(None, 2, None, *arrs) == _lib.MCALF_ERR_INVALID
        assert name + b": opts is NULL" in lib.mcalf_last_error(None)
        assert call(None, -1, C.addressof(ok), *arrs) == _lib.MCALF_ERR_INVALID
        assert b"batch must be >= 0" in lib.mcalf_last_error(None)
        for k, what in enumerate(names):
            a = list(arrs)
            a[k] = None
            assert call(None, 2, C.addressof(ok), *a) == _lib.MCALF_ERR_INVALID
            assert (what + b" is NULL" if what else b"ctx is NULL") in lib.mcalf_last_error(None), (k, lib.mcalf_last_error(None))
        for over, what in ((dict(nmoves=-1), b"nmoves"), (dict(max_steps=-3), b"max_steps"), (dict(ndirs=0), b"ndirs"), (dict(ndirs=-2), b"ndirs")):
            bad = _opts(**over)
            assert call(None, 2, C.addressof(bad), *arrs) == _lib.MCALF_ERR_INVALID
            assert name + b": " + what + b" must be" in lib.mcalf_last_error(None), (over, lib.mcalf_last_error(None))
        assert call(None, 0, C.addressof(ok), *([None] * 10)) == _lib.MCALF_ERR_INVALID       # (ctx is NULL)
        assert b"ctx is NULL" in lib.mcalf_last_error(None)


def test_the_python_methods_exist():
    sig = inspect.signature(mcalf_amd.als_fitter.slice_replace_batch)
    got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert got == dict(nmoves=None, max_steps=None, seed=0, stream_ids=None)
    assert list(sig.parameters)[1:4] == ["U0", "Lmin", "dirs"]
    assert callable(mcalf_amd.als_fitter.nested_sample)
    sig = inspect.signature(mcalf_amd.nested.nested_sample)
    assert list(sig.parameters)[:4] == ["loglike_cube", "replace", "ndim", "nlive"]
    assert sig.parameters["dlogz"].default == 1e-3 and sig.parameters["batch"].default is None and sig.parameters["seed"].default == 0
