"""GPU: per-pixel posterior bands of the model -- mcalf_model_band_batch[_device] and als_fitter.model_band_batch -- against the
numpy restatement of tests/band_reference.py applied to M = fit.model_batch(P, targonly) of the SAME context, and against the
oracle's spectra.  Bars (band_reference.py; eps = 2^-52):
  quantiles  exact ranks: np.array_equal with the sorted column; interpolated: 4 ulp of max(|lo|, |hi|)
  mean       n eps max|x|
  variance   2 (n + 3) eps max|x - mu|^2 + (n eps max|x|)^2  (a two-pass variance meets it, a one-pass formula does not)
  oracle     1e-11 on quantiles and mean (the suite's model bar: both are 1-Lipschitz in max|M - M_o|)
Every comparison prints its worst error / bar (pytest -s).

Shapes: one lane owns one pixel and a strip is 64 pixels, so 1, 63, 64, 65 pixels are a partial, a nearly full, a full and a
full + partial strip, 4100 pixels are two pixel tiles of the model kernels; the moment passes cut the rows into blocks of 256
(four waves of 64 rows), so 64, 65, 257, 300 rows cross a wave and a block boundary; the select kernel's sixteen waves take the
rows modulo 16, sixteen at a time: 257 and 300 rows need a second, partly filled, turn."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import band_reference as br
import mcalf_amd
from cases import problem_from_kwargs, tiny_problem
from mcalf_amd import _lib, workloads
from oracle import numpy_oracle as o

pytestmark = pytest.mark.gpu

CIV = [(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8)]
Q5 = (0.025, 0.16, 0.5, 0.84, 0.975)
ROW_BLOCK = 256


def _two_line_kw(npix=300, seed=1):
    """Two lines, up to three components, a filler, floated resolution -- built like the parity tests' problems."""
    wl = np.linspace(6180.0, 6220.0, npix + 2)[1:-1]
    rng = np.random.default_rng(seed)
    return dict(fitrange=[[6180.0, 6220.0]], fitlines=["CIV 1548", "CIV 1550"], linepars=CIV, ncomp=[1, 3], nfill=1, specres=[6.0, 9.0],
                contval=[1.0], Nrange=[12.5, 14.5], brange=[8.0, 40.0], zrange=[2.995, 3.012],
                velstep=float(np.median(np.diff(wl) / wl[1:]) * 2.9979245e5), spectrum=(wl, 1 + rng.normal(0, 0.03, npix), np.full(npix, 0.03)))


def _wide_kw():
    """A context whose LSF is wider than a workgroup tile (tests/test_gpu_wide_lsf.py): free resolution and continuum, fillers."""
    npix, rng = 333, np.random.default_rng(333)
    wl = np.linspace(6180.0, 6220.0, npix + 2)[1:-1]
    return dict(fitrange=[[6180.0, 6220.0]], fitlines=["CIV 1548", "CIV 1550"], linepars=CIV, ncomp=[1, 3], nfill=2, specres=[6.0, 9.0],
                contval=[0.9, 1.1], Nrange=[12.0, 14.5], brange=[5.0, 40.0], zrange=[2.995, 3.012],
                spectrum=(wl, 1 + rng.normal(0, 0.03, npix), rng.uniform(0.01, 0.05, npix)), velstep=0.0031)


PROBLEMS = {"tiny": lambda: tiny_problem(200), "two_line": _two_line_kw}


@pytest.fixture(scope="module")
def fits():
    """One open context per problem, shared by the tests below, with 300 rows drawn from its prior box."""
    out = {}
    for k, (name, make) in enumerate(PROBLEMS.items()):
        kw = make()
        out[name] = (mcalf_amd.als_fitter(None, **kw), kw, workloads.draw_P(kw, 300, np.random.default_rng(20 + k)))
    yield out
    for fit, _, _ in out.values():
        fit.close()


def _check(fit, P, q, what, targonly=False, exact=None):
    """Every output of one call against the reference on the same context's model rows; `exact`: the sorted rows the
    quantiles must equal."""
    M = fit.model_batch(P, targonly)
    band = fit.model_band_batch(P, q=q, targonly=targonly)
    npix = M.shape[1]
    assert band.mean.shape == band.var.shape == band.nvalid.shape == (npix,) and band.quantiles.shape == (len(q), npix)
    assert band.nvalid.dtype == np.int64
    nvalid, mean, var = br.moments(M)
    want_q = br.quantiles(M, q)
    qbar, mbar, vbar = br.quantile_bar(M, q), br.mean_bar(M), br.var_bar(M)
    print(f"band {what}: worst error / bar: quantiles {br.worst(band.quantiles, want_q, qbar):.3g}, mean {br.worst(band.mean, mean, mbar):.3g}, "
          f"var {br.worst(band.var, var, vbar):.3g}")
    assert np.array_equal(band.nvalid, nvalid), what
    if exact is not None:
        assert np.array_equal(band.quantiles, np.sort(M, axis=0)[list(exact)]), what
    assert br.within(band.quantiles, want_q, qbar), what
    assert br.within(band.mean, mean, mbar), what
    assert br.within(band.var, var, vbar), what
    return M, band


# ---------------------------------------------------------------------------------------------------- 1. exact ranks
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_exact_ranks_are_the_sorted_column(fits, name):
    fit, _, P = fits[name]
    M = fit.model_batch(P[:5])
    got = fit.model_band_batch(P[:5], q=(0, 0.25, 0.5, 0.75, 1)).quantiles
    assert np.array_equal(got, np.sort(M, axis=0))
    assert np.array_equal(fit.model_band_batch(P[:2], q=(0, 1)).quantiles, np.sort(M[:2], axis=0))
    one = fit.model_band_batch(P[:1], q=(0, 0.3, 1))
    assert np.array_equal(one.quantiles, np.repeat(M[:1], 3, axis=0)) and np.array_equal(one.mean, M[0]) and np.all(one.var == 0.0)
    assert np.all(one.nvalid == 1)


# ---------------------------------------------------------------------------------- 2. interpolated ranks, 3. moments
@pytest.mark.parametrize("batch", [3, 64, 65, ROW_BLOCK + 1, 300])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_interpolated_ranks_against_nanquantile(fits, name, batch):
    fit, _, P = fits[name]
    M = fit.model_batch(P[:batch])
    got = fit.model_band_batch(P[:batch], q=Q5).quantiles
    want, bar = br.quantiles(M, Q5), br.quantile_bar(M, Q5)
    print(f"band quantiles {name}, {batch} rows: worst error / bar {br.worst(got, want, bar):.3g}")
    assert np.isfinite(want).all() and br.within(got, want, bar)


@pytest.mark.parametrize("batch", [3, 64, 65, ROW_BLOCK + 1, 300])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_mean_and_two_pass_variance_against_long_double(fits, name, batch):
    fit, _, P = fits[name]
    M = fit.model_batch(P[:batch])
    band = fit.model_band_batch(P[:batch], q=())
    assert band.quantiles.shape == (0, M.shape[1])
    nvalid, mean, var = br.moments(M)
    mbar, vbar = br.mean_bar(M), br.var_bar(M)
    print(f"band moments {name}, {batch} rows: worst error / bar: mean {br.worst(band.mean, mean, mbar):.3g}, var {br.worst(band.var, var, vbar):.3g}")
    assert np.array_equal(band.nvalid, nvalid) and np.all(nvalid == batch)
    assert br.within(band.mean, mean, mbar) and br.within(band.var, var, vbar)
    if name == "tiny" and batch >= 64:
        # the point of the bar: the one-pass formula misses it on the continuum pixels of this very matrix (the two-line
        # problem has none: its filler lines fall anywhere in the window)
        one_pass = (M * M).mean(axis=0) - M.mean(axis=0) ** 2
        assert np.any(np.abs(one_pass - var) > vbar)


# ------------------------------------------------------------------------------------------ 4. pixel-lane and tile edges
@pytest.mark.parametrize("npix", [1, 63, 64, 65, 4100])
def test_pixel_lane_and_tile_edges(npix):
    kw = tiny_problem(npix)
    P = workloads.draw_P(kw, 7, np.random.default_rng(npix))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.info.ntiles == (2 if npix == 4100 else 1) and fit.obj_wl.size == npix
        _check(fit, P, (0, 0.5, 1), f"{npix} px, exact", exact=(0, 3, 6))
        _check(fit, P, Q5, f"{npix} px, interpolated")
        _check(fit, P, Q5, f"{npix} px, targonly", targonly=True)


# --------------------------------------------------------------------------------------------------------------- 5. ties
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_ties(fits, name):
    fit, _, P = fits[name]
    same = np.repeat(P[:1], 9, axis=0)
    M, band = _check(fit, same, Q5, f"{name}, identical rows")
    assert np.array_equal(band.quantiles, np.repeat(M[:1], len(Q5), axis=0))
    assert np.all(band.var <= br.var_bar(M))
    half = np.concatenate([P[:6], P[:6]])[np.random.default_rng(4).permutation(12)]
    M, band = _check(fit, half, (0, 0.5, 1) + Q5, f"{name}, half the rows duplicated")
    s = np.sort(M, axis=0)
    assert np.array_equal(band.quantiles[0], s[0]) and np.array_equal(band.quantiles[2], s[-1])


# ----------------------------------------------------------------------------------------------------------- 6. NaN rows
def _poison(name, fit, P):
    """A copy of P whose row 2 gives an all-NaN model: a NaN column density, or a floated resolution beyond specres_max."""
    P = P.copy()
    if name == "tiny":
        P[2, fit.startind + 1] = np.nan
    else:
        P[2, 0] = 30.0
    return P


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_nan_rows_do_not_count(fits, name):
    fit, _, P0 = fits[name]
    P = _poison(name, fit, P0[:9])
    M = fit.model_batch(P)
    assert np.isnan(M[2]).all() and np.isfinite(np.delete(M, 2, axis=0)).all()       # (else the case tests nothing)
    q = (0, 0.5, 1) + Q5
    _, band = _check(fit, P, q, f"{name}, one NaN row")
    assert np.all(band.nvalid == 8)
    without = fit.model_band_batch(np.delete(P, 2, axis=0), q=q)
    for a, b in zip(band, without):
        assert np.array_equal(a, b)
    allnan = np.repeat(P[2:3], 5, axis=0)
    band = fit.model_band_batch(allnan, q=Q5)
    assert np.all(band.nvalid == 0) and np.isnan(band.mean).all() and np.isnan(band.var).all() and np.isnan(band.quantiles).all()


# ----------------------------------------------------------------------------------------------------- 7. the oracle
def _against_oracle(fit, P, M_o, targonly, what):
    band = fit.model_band_batch(P, q=Q5, targonly=targonly)
    dq = np.abs(band.quantiles - br.quantiles(M_o, Q5)).max()
    dm = np.abs(band.mean - M_o.mean(axis=0)).max()
    print(f"band vs oracle, {what}: max |dQ| {dq:.3g}, max |dmean| {dm:.3g} (bar 1e-11)")
    assert dq < 1e-11 and dm < 1e-11, what


@pytest.mark.parametrize("targonly", [False, True])
@pytest.mark.parametrize("name", list(PROBLEMS))
def test_against_the_oracle(fits, name, targonly):
    fit, kw, P = fits[name]
    prob = problem_from_kwargs(kw)
    M_o = np.array([o.reconstruct_spec(prob, p, targonly=targonly) for p in P[:16]])
    _against_oracle(fit, P[:16], M_o, targonly, f"{name}, targonly={targonly}")


def test_against_the_oracle_under_jax_semantics():
    kw = dict(_two_line_kw(), conv_mode="jax")
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 16, np.random.default_rng(31))
    M_o = np.array([o.jax_reconstruct_spec_f64(prob, p) for p in P])
    with mcalf_amd.als_fitter(None, **kw) as fit:
        _against_oracle(fit, P, M_o, False, "JAX semantics")
        _check(fit, P, Q5, "JAX semantics")


@pytest.mark.parametrize("targonly", [False, True])
def test_against_the_oracle_on_a_wide_lsf_context(targonly):
    kw = _wide_kw()
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 16, np.random.default_rng(32))
    M_o = np.array([o.reconstruct_spec(prob, p, targonly=targonly) for p in P])
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert 2 * fit.info.n_cap + 64 > 4096
        _against_oracle(fit, P, M_o, targonly, f"wide LSF, targonly={targonly}")
        _check(fit, P, Q5, "wide LSF", targonly=targonly)


# ------------------------------------------------------------------------------------------------------- 8. invariance
def _raw(fit, P, q, mean=True, var=True, quant=True, nvalid=True, targonly=0):
    """The C entry with any subset of the outputs."""
    npix, q = fit.obj_wl.size, np.asarray(q, dtype=float)
    out = dict(mean=np.full(npix, -7.0) if mean else None, var=np.full(npix, -7.0) if var else None,
               quant=np.full((q.size, npix), -7.0) if quant else None, nvalid=np.full(npix, -7, dtype=np.int64) if nvalid else None)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = fit._lib.mcalf_model_band_batch(fit._ctx, P.ctypes.data, len(P), targonly, q.ctypes.data if quant else None, q.size if quant else 0,
                                         ptr(out["mean"]), ptr(out["var"]), ptr(out["quant"]), ptr(out["nvalid"]))
    _lib.check(rc, fit._ctx)
    return out


@pytest.mark.parametrize("name", list(PROBLEMS))
def test_bits_do_not_depend_on_the_call_the_outputs_or_the_device_count(fits, name):
    fit, kw, P = fits[name]
    P = np.ascontiguousarray(P[:ROW_BLOCK + 44])
    a, b = fit.model_band_batch(P, q=Q5), fit.model_band_batch(P, q=Q5)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    full = _raw(fit, P, Q5)
    assert full["mean"].tobytes() == a.mean.tobytes() and full["quant"].tobytes() == a.quantiles.tobytes()
    only_q = _raw(fit, P, Q5, mean=False, var=False, nvalid=False)
    assert only_q["quant"].tobytes() == a.quantiles.tobytes()
    only_mean = _raw(fit, P, Q5, var=False, quant=False, nvalid=False)
    assert only_mean["mean"].tobytes() == a.mean.tobytes()
    only_var = _raw(fit, P, Q5, mean=False, quant=False, nvalid=False)
    assert only_var["var"].tobytes() == a.var.tobytes()
    only_n = _raw(fit, P, Q5, mean=False, var=False, quant=False)
    assert np.array_equal(only_n["nvalid"], a.nvalid)
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as two:
        assert two.info.ndevices == 2
        c = two.model_band_batch(P, q=Q5)
        for x, y in zip(a, c):
            assert x.tobytes() == y.tobytes()


# ---------------------------------------------------------------------------------------------------- 9. device entry
def test_the_device_entry_equals_the_host_entry(fits):
    fit, kw, P = fits["two_line"]
    n, npix, nq = 200, fit.obj_wl.size, len(Q5)
    P = np.ascontiguousarray(P[:n])
    want = fit.model_band_batch(P, q=Q5, targonly=True)
    M = fit.model_batch(P, targonly=True)
    q = np.asarray(Q5)
    dP = torch.from_numpy(P).cuda()
    f64 = dict(dtype=torch.float64, device="cuda")
    dM, dmean, dvar, dQ = torch.full((n, npix), -7.0, **f64), torch.full((npix,), -7.0, **f64), torch.full((npix,), -7.0, **f64), torch.full((nq, npix), -7.0, **f64)
    dn = torch.full((npix,), -7, dtype=torch.int64, device="cuda")

    def call(stream, qarr=q):
        return fit._lib.mcalf_model_band_batch_device(fit._ctx, dP.data_ptr(), n, 1, qarr.ctypes.data, nq, dM.data_ptr(), dmean.data_ptr(), dvar.data_ptr(),
                                                      dQ.data_ptr(), dn.data_ptr(), C.c_void_p(stream))

    def equal():
        return (np.array_equal(dmean.cpu().numpy(), want.mean) and np.array_equal(dvar.cpu().numpy(), want.var) and
                np.array_equal(dQ.cpu().numpy(), want.quantiles) and np.array_equal(dn.cpu().numpy(), want.nvalid) and np.array_equal(dM.cpu().numpy(), M))

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    qcopy = q.copy()
    _lib.check(call(side.cuda_stream, qcopy), fit._ctx)
    qcopy[:] = np.nan                                     # q travelled by value: nothing of the caller's is read after the call returns
    side.synchronize()
    assert equal()
    # the second call allocates and synchronises nothing: it can be captured into a hipGraph and replayed
    for t in (dM, dmean, dvar, dQ):
        t.fill_(-7.0)
    dn.fill_(-7)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _lib.check(call(torch.cuda.current_stream().cuda_stream), fit._ctx)
    g.replay()
    torch.cuda.synchronize()
    assert equal()
    # batch == 0: NaN and 0
    rc = fit._lib.mcalf_model_band_batch_device(fit._ctx, None, 0, 0, q.ctypes.data, nq, None, dmean.data_ptr(), dvar.data_ptr(), dQ.data_ptr(), dn.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.isnan(dmean).all() and torch.isnan(dvar).all() and torch.isnan(dQ).all() and (dn == 0).all()
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as two:
        rc = two._lib.mcalf_model_band_batch_device(two._ctx, dP.data_ptr(), n, 1, q.ctypes.data, nq, dM.data_ptr(), dmean.data_ptr(), None, dQ.data_ptr(), None, None)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in two._lib.mcalf_last_error(two._ctx)


# -------------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals(fits):
    fit, _, P = fits["tiny"]
    lib, ctx = fit._lib, fit._ctx
    npix = fit.obj_wl.size
    P = np.ascontiguousarray(P[:4])
    q, out, nv = np.array([0.5]), np.zeros(npix), np.zeros(npix, dtype=np.int64)
    p, qp, o_ = P.ctypes.data, q.ctypes.data, out.ctypes.data
    host = lambda *a: lib.mcalf_model_band_batch(ctx, *a)
    dev = lambda P_, batch, targ, q_, nq, *outs: lib.mcalf_model_band_batch_device(ctx, P_, batch, targ, q_, nq, o_, *outs, None)
    cases = [
        ((p, -1, 0, qp, 1, o_, o_, o_, nv.ctypes.data), b"batch must be >= 0, got -1"),
        ((None, 4, 0, qp, 1, o_, o_, o_, None), b"P is NULL"),
        ((p, 4, 0, None, 0, None, None, None, None), b"mean, var, Q and nvalid are all NULL"),
        ((p, 4, 0, qp, 17, o_, o_, o_, None), b"nq must be in [0, 16], got 17"),
        ((p, 4, 0, qp, -1, o_, o_, o_, None), b"nq must be in [0, 16], got -1"),
        ((p, 4, 0, None, 1, o_, o_, o_, None), b"q is NULL with nq = 1"),
        ((p, 4, 0, qp, 1, o_, o_, None, None), b"Q is NULL with nq = 1"),
        ((p, 4, 0, None, 0, o_, None, o_, None), b"Q is given with nq = 0"),
        ((p, 4, 2, qp, 1, o_, o_, o_, None), b"targonly must be 0 or 1, got 2"),
        ((p, 4, -1, qp, 1, o_, o_, o_, None), b"targonly must be 0 or 1, got -1"),
    ]
    for bad in (np.nan, np.inf, -1e-9, 1.5):
        qq = np.array([bad])
        cases.append(((p, 4, 0, qq.ctypes.data, 1, o_, o_, o_, None), b"q[0] = "))
        cases[-1] += (qq,)                                  # (kept alive)
    for entry in (host, dev):
        for case in cases:
            assert entry(*case[0]) == _lib.MCALF_ERR_INVALID, case[1]
            assert case[1] in lib.mcalf_last_error(ctx), (case[1], lib.mcalf_last_error(ctx))
    rc = lib.mcalf_model_band_batch_device(ctx, p, 4, 0, qp, 1, None, o_, o_, o_, None, None)
    assert rc == _lib.MCALF_ERR_INVALID and b"dM is NULL" in lib.mcalf_last_error(ctx)
    # the context still works
    assert np.isfinite(fit.model_band_batch(P).mean).all()


def test_the_matrix_cap_is_a_range_error_that_names_the_largest_batch():
    kw = tiny_problem(64)
    cap = (4 << 30) // (64 * 8)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        P = np.zeros((cap + 1, fit.ndim))                   # never read: the check comes before a single row of P is
        t0 = time.perf_counter()
        with pytest.raises(RuntimeError, match=f"MCALF_ERR_RANGE.*largest batch for this spectrum is {cap} "):
            fit.model_band_batch(P)
        assert time.perf_counter() - t0 < 1.0
        rc = fit._lib.mcalf_model_band_batch_device(fit._ctx, P.ctypes.data, cap + 1, 0, None, 0, P.ctypes.data, P.ctypes.data, None, None, None, None)
        assert rc == _lib.MCALF_ERR_RANGE and str(cap).encode() in fit._lib.mcalf_last_error(fit._ctx)
        # no row
        band = fit.model_band_batch(np.zeros((0, fit.ndim)), q=Q5)
        assert band.quantiles.shape == (5, 64) and np.isnan(band.quantiles).all() and np.isnan(band.mean).all() and np.isnan(band.var).all()
        assert np.all(band.nvalid == 0)
