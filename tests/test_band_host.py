"""CPU: the numpy restatement of the posterior-band statistics (tests/band_reference.py) on hand-made columns, and the
argument checks of mcalf_model_band_batch[_device] that need no device (every refusal comes before any device work)."""
import ctypes as C

import numpy as np

import band_reference as br
from mcalf_amd import _lib

NAN = np.nan


def test_reference_on_hand_made_columns():
    #              ties         a NaN   all NaN  n = 1 (the other rows NaN)
    M = np.array([[2.0,         1.0,    NAN,     NAN],
                  [1.0,         NAN,    NAN,     7.5],
                  [2.0,         4.0,    NAN,     NAN],
                  [1.0,         2.0,    NAN,     NAN],
                  [2.0,         3.0,    NAN,     NAN]])
    cols = br.sorted_columns(M)
    assert [c.tolist() for c in cols] == [[1.0, 1.0, 2.0, 2.0, 2.0], [1.0, 2.0, 3.0, 4.0], [], [7.5]]
    nvalid, mean, var = br.moments(M)
    assert nvalid.tolist() == [5, 4, 0, 1] and nvalid.dtype == np.int64
    assert mean[0] == 1.6 and mean[1] == 2.5 and np.isnan(mean[2]) and mean[3] == 7.5
    assert abs(var[0] - 0.24) < 1e-16 and var[1] == 1.25 and np.isnan(var[2]) and var[3] == 0.0
    q = [0.0, 0.25, 0.5, 0.9, 1.0]
    Q = br.quantiles(M, q)
    assert Q.shape == (5, 4)
    assert Q[:, 0].tolist() == [1.0, 1.0, 2.0, 2.0, 2.0]                       # h = 0, 1, 2, 3.6, 4: ties on both sides of 3.6
    assert np.allclose(Q[:, 1], [1.0, 1.75, 2.5, 3.7, 4.0], rtol=0, atol=1e-15)
    assert np.isnan(Q[:, 2]).all() and np.all(Q[:, 3] == 7.5)
    lo, hi = br.neighbours(M, q)
    assert lo[:, 1].tolist() == [1.0, 1.0, 2.0, 3.0, 4.0] and hi[:, 1].tolist() == [2.0, 2.0, 3.0, 4.0, 4.0]
    assert np.isnan(lo[:, 2]).all() and np.all(lo[:, 3] == 7.5) and np.all(hi[:, 3] == 7.5)
    # the plain formula the kernel uses is within the bar of numpy's
    h = 3 * np.asarray(q)
    plain = lo[:, 1] + (hi[:, 1] - lo[:, 1]) * (h - np.floor(h))
    assert br.within(plain, Q[:, 1], br.quantile_bar(M, q)[:, 1])
    assert br.quantiles(M, []).shape == (0, 4) and np.isnan(br.quantiles(M[:0], [0.5])).all()


def test_the_variance_bar_separates_two_passes_from_one():
    """A continuum pixel: level 1, spread 1e-10.  The two-pass variance in double meets the bar; E[x^2] - mean^2 does not."""
    rng = np.random.default_rng(0)
    x = 1.0 + 1e-10 * rng.standard_normal((300, 3))
    _, mean, var = br.moments(x)
    two = ((x - x.mean(axis=0)) ** 2).mean(axis=0)
    one = (x * x).mean(axis=0) - x.mean(axis=0) ** 2
    bar = br.var_bar(x)
    assert np.all(np.abs(two - var) <= bar)
    assert np.all(np.abs(one - var) > bar)
    assert np.all(np.abs(x.mean(axis=0) - mean) <= br.mean_bar(x))


def test_invalid_arguments_return_minus_one_without_a_device():
    lib = _lib.load()
    P, q = np.zeros((2, 4)), np.array([0.5])
    out = np.zeros(8)
    nv = np.zeros(8, dtype=np.int64)
    host = lambda ctx, P_, batch, targ, q_, nq, *outs: lib.mcalf_model_band_batch(ctx, P_, batch, targ, q_, nq, *outs)
    dev = lambda ctx, P_, batch, targ, q_, nq, *outs: lib.mcalf_model_band_batch_device(ctx, P_, batch, targ, q_, nq, out.ctypes.data, *outs, None)
    for call, name in ((host, b"mcalf_model_band_batch"), (dev, b"mcalf_model_band_batch_device")):
        o = (out.ctypes.data, out.ctypes.data, out.ctypes.data, nv.ctypes.data)
        assert call(None, P.ctypes.data, 2, 0, q.ctypes.data, 1, *o) == _lib.MCALF_ERR_INVALID
        assert name + b": ctx is NULL" in lib.mcalf_last_error(None)
        assert call(None, None, 0, 0, None, 0, None, None, None, None) == _lib.MCALF_ERR_INVALID
        assert b"all NULL" in lib.mcalf_last_error(None)
        assert call(None, P.ctypes.data, 2, 0, q.ctypes.data, 17, *o) == _lib.MCALF_ERR_INVALID
        assert b"nq must be in [0, 16], got 17" in lib.mcalf_last_error(None)
        assert call(None, P.ctypes.data, 2, 0, q.ctypes.data, -1, *o) == _lib.MCALF_ERR_INVALID
        assert call(None, P.ctypes.data, -1, 0, q.ctypes.data, 1, *o) == _lib.MCALF_ERR_INVALID
        assert b"batch must be >= 0" in lib.mcalf_last_error(None)
        assert call(None, None, 2, 0, q.ctypes.data, 1, *o) == _lib.MCALF_ERR_INVALID
        assert b"P is NULL" in lib.mcalf_last_error(None)
        assert call(None, P.ctypes.data, 2, 0, None, 1, *o) == _lib.MCALF_ERR_INVALID
        assert b"q is NULL" in lib.mcalf_last_error(None)
        assert call(None, P.ctypes.data, 2, 0, q.ctypes.data, 1, o[0], o[1], None, o[3]) == _lib.MCALF_ERR_INVALID
        assert b"Q is NULL" in lib.mcalf_last_error(None)
        assert call(None, P.ctypes.data, 2, 0, None, 0, *o) == _lib.MCALF_ERR_INVALID
        assert b"nq = 0" in lib.mcalf_last_error(None)
        for bad in (np.nan, np.inf, -0.1, 1.0000001):
            qq = np.array([0.5, bad])
            assert call(None, P.ctypes.data, 2, 0, qq.ctypes.data, 2, *o) == _lib.MCALF_ERR_INVALID
            assert b"q[1]" in lib.mcalf_last_error(None)
        assert call(None, P.ctypes.data, 2, 2, q.ctypes.data, 1, *o) == _lib.MCALF_ERR_INVALID
        assert b"targonly must be 0 or 1" in lib.mcalf_last_error(None)
    assert lib.mcalf_model_band_batch_device(None, P.ctypes.data, 2, 0, q.ctypes.data, 1, None, out.ctypes.data, None, out.ctypes.data, None,
                                             None) == _lib.MCALF_ERR_INVALID
    assert b"dM is NULL" in lib.mcalf_last_error(None)


def test_the_python_entry_exists():
    import mcalf_amd
    assert callable(mcalf_amd.als_fitter.model_band_batch)
    from importlib import import_module
    hf = import_module("mc-alf_amd.routines.hires_fitter")
    assert hf.ModelBand._fields == ("mean", "var", "quantiles", "nvalid")
