"""GPU: mcalf_chain_stats against the numpy restatement (chain_reference.py) on AR(1) chains, within bounds derived from the
shapes; the edges (bad, constant and NaN walkers, optional arrays); the entries against one another by bytes."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import chain_reference as cr
import mcalf_amd
from cases import tiny_problem
from mcalf_amd import _lib, convergence

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FLOATS = ("mean", "var", "tau", "tau_mean", "rhat", "ess")


@pytest.fixture(scope="module")
def fit():
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as f:
        yield f


@functools.lru_cache(maxsize=None)
def chain(T, n, d, phi, seed=1):
    X = cr.ar1(T, n, d, phi, seed)
    X.setflags(write=False)
    return X


@functools.lru_cache(maxsize=None)
def reference(T, n, d, phi, seed=1, max_lag=None):
    return cr.chain_stats(chain(T, n, d, phi, seed), max_lag=max_lag)


def margins_hold(ref):
    """The condition on the INPUT: no comparison of the window rule stands closer than 1e-6 to its threshold, so the window
    cannot flip between device and reference."""
    live = ref["nused"] > 0
    print("margins", ref["margin"], ref["margin_mean"])
    assert (ref["margin"][live] > 1e-6).all() and (ref["margin_mean"][live & np.isfinite(ref["margin_mean"])] > 1e-6).all()


def compare(got, ref, T, nok, acf=True):
    """The integer outputs are equal; the floating-point ones lie within the bounds of the shapes: with u = 2^-53 and
    sum |terms| of c_w(tau) <= c_w(0) (Cauchy-Schwarz), |d rho| <= 8 (T + 3) u, |d tau| <= 16 (M + 1) (T + 3) u; mean, var and
    rhat within 4 N u relative to their own sum |terms| / N, N = T nok; ess = nok T / tau follows tau."""
    N = T * nok
    assert np.array_equal(got.window, ref["M"]) and np.array_equal(got.window_mean, ref["M_mean"])
    assert np.array_equal(got.nused, ref["nused"])
    assert np.array_equal(got.reached[:, 0].astype(int) | (got.reached[:, 1].astype(int) << 1), ref["flags"])
    for name in FLOATS:
        assert np.array_equal(np.isnan(getattr(got, name)), np.isnan(ref[name])), name
    ok = ~np.isnan(ref["tau"])
    tol_tau = 16.0 * (ref["M"] + 1.0) * (T + 3.0) * U
    tol_mean_tau = 16.0 * (ref["M_mean"] + 1.0) * (T + 3.0) * U
    err = {"mean": np.abs(got.mean - ref["mean"]) / (4.0 * N * U * np.abs(ref["mean"])),
           "var": np.abs(got.var - ref["var"]) / np.maximum(4.0 * N * U * ref["var"], 1e-300),
           "rhat": np.abs(got.rhat - ref["rhat"]) / (4.0 * N * U * ref["rhat"]),
           "tau": np.abs(got.tau - ref["tau"]) / tol_tau, "tau_mean": np.abs(got.tau_mean - ref["tau_mean"]) / tol_mean_tau,
           "ess": np.abs(got.ess - ref["ess"]) / (np.abs(ref["ess"]) * (tol_tau / np.abs(ref["tau"]) + 2.0 * U))}
    print({k: float(np.nanmax(v)) if np.isfinite(v).any() else None for k, v in err.items()}, "(errors in units of their bounds)")
    for name, e in err.items():
        assert (e[~np.isnan(e)] <= 1.0).all(), (name, e)
    if acf:
        e = np.abs(got.acf[ok] - ref["acf"][ok]) / (8.0 * (T + 3.0) * U)
        print("acf", float(e.max()) if e.size else None)
        assert (e <= 1.0).all()
        assert np.isnan(got.acf[~ok]).all()


# ---- the six cases of the issue, and one axis at a time around (65, 6, 5) -------------------------------------------------------

SIX = [(512, 16, 5, 0.5), (512, 16, 5, 0.8), (257, 6, 3, 0.3), (64, 4, 2, 0.2), (5, 4, 1, 0.0), (4, 1, 1, 0.0)]
# T: the small ones, a wave, the t-block of 192 steps and its neighbours
AXIS_T = [(T, 6, 5, 0.5) for T in (4, 5, 63, 64, 65, 129, 191, 192, 193, 257)]
# n: one walker, a walker block of 64 and its neighbours
AXIS_N = [(65, n, 5, 0.5) for n in (1, 2, 63, 64, 65, 129)]
# d: the coordinate tile of 8 and its neighbours, a wave, a lane that owns several coordinates
AXIS_D = [(65, 6, d, 0.5) for d in (1, 7, 8, 9, 64, 65, 129)]


@pytest.mark.parametrize("case", SIX + AXIS_T + AXIS_N + AXIS_D, ids=lambda c: "T%d-n%d-d%d-phi%g" % c)
def test_against_the_reference(fit, case):
    T, n, d, phi = case
    ref = reference(*case)
    margins_hold(ref)
    compare(convergence.chain_stats(fit, chain(*case), acf=True), ref, T, n)


# L: short, around a wave, T - 1; around the lag tile of 512 (T = 600: two lag tiles)
AXIS_L = [(129, L) for L in (1, 63, 64, 65, 128)] + [(600, L) for L in (511, 512, 513, 599)]


@pytest.mark.parametrize("T,L", AXIS_L)
def test_lags(fit, T, L):
    ref = reference(T, 6, 5, 0.5, 1, L)
    margins_hold(ref)
    got = convergence.chain_stats(fit, chain(T, 6, 5, 0.5), max_lag=L, acf=True)
    assert got.acf.shape == (5, L + 1)
    compare(got, ref, T, 6)


def test_a_lag_too_short_for_the_window_leaves_the_flag_clear(fit):
    ref = reference(257, 6, 5, 0.8, 1, 8)                  # tau is about 9: no m <= 8 has m >= 5 tau(m)
    margins_hold(ref)
    got = convergence.chain_stats(fit, chain(257, 6, 5, 0.8), max_lag=8, acf=True)
    assert (got.window == 8).all() and not got.reached[:, 0].any() and (ref["flags"] & 1 == 0).all()
    compare(got, ref, 257, 6)


# ---- edges ------------------------------------------------------------------------------------------------------------------------

def test_bad_walkers_are_left_out(fit):
    X = chain(65, 6, 5, 0.5)
    status = np.array([-1, 0, 0, -1, 0, -1], dtype=np.int32)          # the first, an interior one and the last
    ref = cr.chain_stats(X, status=status)
    margins_hold(ref)
    Y = X.copy()
    Y[:, status != 0, :] = np.nan                                     # whatever they hold
    got = convergence.chain_stats(fit, Y, status=status, acf=True)
    compare(got, ref, 65, 3)
    assert (got.nused == 3).all()


@pytest.mark.parametrize("stuck,frozen", [(0.25, 0.75), (0.3, 0.1), (0.7, 1.0 / 3.0)])
@pytest.mark.parametrize("T", [20, 65, 193, 1000])
def test_a_constant_walker_and_a_frozen_coordinate(fit, T, stuck, frozen):
    """Also at values that are no dyadic fractions: the float64 sum of T copies of 0.3, over T, is not 0.3 (at T = 65 it is
    0.3000000000000004), so a series is constant because x_t == x_0 for every t, not because a rounded c_w(0) comes out 0."""
    X = chain(T, 6, 5, 0.5).copy()
    base = convergence.chain_stats(fit, X, acf=True)
    X[:, 2, 1] = stuck                                                # walker 2 is stuck in coordinate 1
    X[:, :, 3] = frozen                                               # coordinate 3 is frozen for every walker
    ref = cr.chain_stats(X)
    margins_hold(ref)
    got = convergence.chain_stats(fit, X, acf=True)
    compare(got, ref, T, 6)
    assert list(got.nused) == [6, 5, 6, 0, 6]
    assert np.isnan(got.tau[3]) and np.isnan(got.ess[3]) and np.isnan(got.tau_mean[3]) and np.isnan(got.rhat[3])
    assert got.mean[3] == frozen and got.var[3] == 0.0 and got.window[3] == T - 1 and not got.reached[3].any()
    for k in (0, 2, 4):                                               # the other coordinates are unchanged, by bytes
        assert all(getattr(got, f)[k].tobytes() == getattr(base, f)[k].tobytes() for f in FLOATS) and got.acf[k].tobytes() == base.acf[k].tobytes()


def test_a_nan_spoils_its_coordinate_only(fit):
    X = chain(65, 6, 5, 0.5).copy()
    base = convergence.chain_stats(fit, X, acf=True)
    X[17, 4, 2] = np.nan
    got = convergence.chain_stats(fit, X, acf=True)
    assert all(np.isnan(getattr(got, f)[2]) for f in FLOATS) and np.isnan(got.acf[2]).all()
    assert got.window[2] == 64 and got.window_mean[2] == 64 and not got.reached[2].any() and got.nused[2] == 6
    for k in (0, 1, 3, 4):
        assert all(getattr(got, f)[k].tobytes() == getattr(base, f)[k].tobytes() for f in FLOATS) and got.acf[k].tobytes() == base.acf[k].tobytes()
        assert got.window[k] == base.window[k] and (got.reached[k] == base.reached[k]).all()


# ---- the entries ------------------------------------------------------------------------------------------------------------------

def _device_call(fit, X, status, c, max_lag, acf, stream):
    """mcalf_chain_stats_device on torch tensors: rc and (stats, info, acf) as numpy arrays."""
    T, n, d = X.shape
    L = T - 1 if not max_lag else max_lag
    opts = _lib.mcalf_chain_opts(c, max_lag or 0)
    dX = torch.from_numpy(np.array(X)).cuda()                    # (a writable copy: the cached chains are read-only)
    dS = None if status is None else torch.from_numpy(status).cuda()
    dstats = torch.full((d, 6), -7.0, dtype=torch.float64, device="cuda")
    dinfo = torch.full((d, 4), -7, dtype=torch.int32, device="cuda")
    dacf = torch.full((d, L + 1), -7.0, dtype=torch.float64, device="cuda")
    stream.wait_stream(torch.cuda.current_stream())
    rc = fit._lib.mcalf_chain_stats_device(fit._ctx, dX.data_ptr(), T, n, d, None if dS is None else dS.data_ptr(), C.addressof(opts),
                                           dstats.data_ptr(), dinfo.data_ptr(), dacf.data_ptr() if acf else None, C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, (dstats.cpu().numpy(), dinfo.cpu().numpy(), dacf.cpu().numpy())


def test_a_second_device_call_allocates_and_synchronises_nothing(fit):
    """After one call of the same size the device entry can be captured into a graph and replayed, as the band entry's is."""
    X = chain(193, 65, 9, 0.5)
    ref = convergence.chain_stats(fit, X, max_lag=40, acf=True)
    rc, first = _device_call(fit, X, None, 5.0, 40, True, torch.cuda.Stream())
    assert rc == 0
    opts = _lib.mcalf_chain_opts(5.0, 40)
    dX = torch.from_numpy(np.array(X)).cuda()
    dstats = torch.full((9, 6), -7.0, dtype=torch.float64, device="cuda")
    dinfo = torch.full((9, 4), -7, dtype=torch.int32, device="cuda")
    dacf = torch.full((9, 41), -7.0, dtype=torch.float64, device="cuda")
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with torch.cuda.graph(g, stream=s):
            _lib.check(fit._lib.mcalf_chain_stats_device(fit._ctx, dX.data_ptr(), 193, 65, 9, None, C.addressof(opts), dstats.data_ptr(), dinfo.data_ptr(),
                                                         dacf.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), fit._ctx)
    g.replay()
    torch.cuda.synchronize()
    got = convergence._stats(dstats.cpu().numpy(), dinfo.cpu().numpy(), dacf.cpu().numpy())
    assert _bytes(got) == _bytes(ref) and got.acf.tobytes() == ref.acf.tobytes()
    assert first[0].tobytes() == dstats.cpu().numpy().tobytes() and first[2].tobytes() == ref.acf.tobytes()


def _bytes(s):
    return b"".join(np.ascontiguousarray(getattr(s, f)).tobytes() for f in FLOATS + ("window", "window_mean", "nused", "reached"))


@pytest.mark.parametrize("case", [(65, 6, 5, 0.5), (193, 65, 9, 0.5)], ids=lambda c: "T%d-n%d-d%d-phi%g" % c)
def test_entries_streams_device_counts_and_repeats_agree_by_bytes(fit, case):
    X = chain(*case)
    status = np.zeros(case[1], dtype=np.int32)
    status[1] = -1
    ref = convergence.chain_stats(fit, X, status=status, max_lag=40, acf=True)
    again = convergence.chain_stats(fit, X, status=status, max_lag=40, acf=True)
    assert _bytes(ref) == _bytes(again) and ref.acf.tobytes() == again.acf.tobytes()
    # status NULL is a status of zeros; acf NULL changes nothing else
    zeros = convergence.chain_stats(fit, X, status=np.zeros(case[1], dtype=np.int32), max_lag=40, acf=True)
    none = convergence.chain_stats(fit, X, max_lag=40, acf=False)
    assert none.acf is None and _bytes(zeros) == _bytes(none)
    for acf in (True, False):
        rc, (stats, info, rho) = _device_call(fit, X, status, 5.0, 40, acf, torch.cuda.Stream())
        dev = convergence._stats(stats, info, rho)
        assert rc == 0 and _bytes(dev) == _bytes(ref)
        assert rho.tobytes() == ref.acf.tobytes() if acf else (rho == -7.0).all()
    with mcalf_amd.als_fitter(None, device=[0, 0], **tiny_problem(64)) as multi:
        got = convergence.chain_stats(multi, X, status=status, max_lag=40, acf=True)
        assert _bytes(got) == _bytes(ref) and got.acf.tobytes() == ref.acf.tobytes()
        rc, _ = _device_call(multi, X, status, 5.0, 40, True, torch.cuda.Stream())
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in multi._lib.mcalf_last_error(multi._ctx)
