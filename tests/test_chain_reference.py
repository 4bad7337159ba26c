"""CPU: the numpy restatement of the chain diagnostics (chain_reference.py) against the estimator the package already has, the
exact AR(1) value and a hand-made split R-hat; the converge rule on synthetic histories; the C entries' refusals with no
context; the binding's new names and struct sizes."""
import ctypes as C
import math

import numpy as np
import pytest

import chain_reference as cr
from mcalf_amd import _lib, ensemble

AR1_CASES = [(512, 16, 5, 0.5), (512, 16, 5, 0.8), (257, 6, 3, 0.3)]


@pytest.fixture(scope="module")
def ar1_stats():
    return {case: (cr.ar1(*case, seed=1), cr.chain_stats(cr.ar1(*case, seed=1))) for case in AR1_CASES}


@pytest.mark.parametrize("case", AR1_CASES)
def test_tau_mean_is_the_existing_estimator_on_the_ensemble_means(ar1_stats, case):
    X, ref = ar1_stats[case]
    want = [ensemble.sokal_tau(X.mean(axis=1)[:, k], 5.0) for k in range(X.shape[2])]
    print(ref["tau_mean"], want)
    assert np.abs(ref["tau_mean"] - want).max() <= 1e-9


@pytest.mark.parametrize("case", AR1_CASES)
def test_tau_is_within_five_standard_errors_of_the_exact_value(ar1_stats, case):
    T, n, d, phi = case
    _, ref = ar1_stats[case]
    exact = (1.0 + phi) / (1.0 - phi)
    se = ref["tau"] * np.sqrt(2.0 * (2.0 * ref["M"] + 1.0) / (n * T))
    print(ref["tau"], exact, se)
    assert (ref["flags"] & 1).all() and (np.abs(ref["tau"] - exact) <= 5.0 * se).all()
    assert np.allclose(ref["ess"], n * T / ref["tau"], rtol=1e-14) and (ref["nused"] == n).all()


def test_split_rhat_by_hand():
    # walker 0: 0 1 | 2 3, walker 1: 1 1 | 3 5.  h = 2: chain means 0.5 2.5 1 4, variances 0.5 0.5 0 2
    X = np.array([[0.0, 1.0], [1.0, 1.0], [2.0, 3.0], [3.0, 5.0]]).reshape(4, 2, 1)
    W = (0.5 + 0.5 + 0.0 + 2.0) / 4.0
    means = np.array([0.5, 2.5, 1.0, 4.0])
    B = 2.0 * ((means - 2.0) ** 2).sum() / 3.0
    want = math.sqrt((0.5 * W + B / 2.0) / W)
    ref = cr.chain_stats(X)
    assert abs(ref["rhat"][0] - want) <= 1e-15 * want
    assert ref["mean"][0] == 2.0 and abs(ref["var"][0] - X.var(ddof=1)) <= 1e-15


def test_split_rhat_tells_mixed_walkers_from_shifted_ones():
    X = np.random.default_rng(1).standard_normal((200, 64, 1))
    assert cr.chain_stats(X, max_lag=20)["rhat"][0] < 1.05
    X[:, :32, :] += 3.0
    assert cr.chain_stats(X, max_lag=20)["rhat"][0] > 1.5


def test_odd_T_drops_the_middle_state_and_constant_walkers_leave():
    X = cr.ar1(65, 6, 3, 0.4, seed=2)
    Y = X.copy()
    Y[32] += 100.0                                         # the middle state of T = 65 is in neither half
    a, b = cr.chain_stats(X, max_lag=8), cr.chain_stats(Y, max_lag=8)
    assert np.allclose(a["rhat"], b["rhat"], rtol=0, atol=0)
    X[:, 2, 1] = 0.3                                       # walker 2 is stuck in coordinate 1 (65 x 0.3 / 65 is not 0.3 in float64)
    X[:, :, 2] = 0.1                                       # coordinate 2 is frozen
    s = cr.chain_stats(X)
    assert list(s["nused"]) == [6, 5, 0] and np.isnan(s["tau"][2]) and np.isnan(s["ess"][2]) and np.isnan(s["tau_mean"][2])
    assert s["mean"][2] == 0.1 and s["var"][2] == 0.0 and np.isnan(s["rhat"][2]) and s["M"][2] == 64 and s["flags"][2] == 0


def test_the_converge_rule_on_synthetic_histories():
    d = 2
    Ts = [100, 200, 300, 400]
    yes, live = np.ones((4, d), dtype=bool), np.full((4, d), 8)
    hist = np.array([[3.0, 2.0], [3.5, 2.0], [3.51, 2.0], [3.51, 2.0]])
    # tau settles at the third check (|3.51 - 3.5| <= 0.01 x 3.51) and T = 300 >= 50 x 3.51
    assert cr.converge_rule(Ts, hist, yes, live, 50.0, 0.01)[0] == 2
    # never at the first check, whatever tau says
    assert cr.converge_rule(Ts[:1], hist[3:], yes[:1], live[:1], 50.0, 0.01)[0] is None
    # too short a chain: T >= factor tau fails until the last check
    assert cr.converge_rule(Ts, hist, yes, live, 110.0, 0.01)[0] == 3
    assert cr.converge_rule(Ts, hist, yes, live, 1000.0, 0.01)[0] is None
    # a window that is not reached blocks; a NaN on a live coordinate blocks; on a frozen one it is skipped
    no = yes.copy()
    no[2, 1] = False
    assert cr.converge_rule(Ts, hist, no, live, 50.0, 0.01)[0] == 3
    nan = hist.copy()
    nan[:, 1] = np.nan
    assert cr.converge_rule(Ts, nan, yes, live, 50.0, 0.01)[0] is None
    frozen = live.copy()
    frozen[:, 1] = 0
    assert cr.converge_rule(Ts, nan, yes, frozen, 50.0, 0.01)[0] == 2
    assert cr.check_lag(1000, 5.0, 50.0) == 101 and cr.check_lag(10, 5.0, 1.0) == 9


def test_the_binding_has_the_new_names_and_struct_sizes():
    for name in ("mcalf_chain_stats", "mcalf_chain_stats_device", "mcalf_ensemble_converge", "mcalf_ensemble_converge_device"):
        assert name in _lib.SYMBOLS
    assert C.sizeof(_lib.mcalf_chain_opts) == 16 and C.sizeof(_lib.mcalf_converge_opts) == 32


def _stats_call(lib, device, X=True, T=8, n=2, d=3, c=5.0, max_lag=0, opts=True, stats=True, info=True):
    buf = np.zeros(8 * 2 * 3)
    st, inf = np.zeros(64), np.zeros(64, dtype=np.int32)
    o = _lib.mcalf_chain_opts(c, max_lag)
    args = [None, buf.ctypes.data if X else None, T, n, d, None, C.addressof(o) if opts else None, st.ctypes.data if stats else None,
            inf.ctypes.data if info else None, None]
    return (lib.mcalf_chain_stats_device(*args, None) if device else lib.mcalf_chain_stats(*args)), lib.mcalf_last_error(None).decode()


@pytest.mark.parametrize("device", [False, True])
def test_chain_stats_refuses_bad_arguments_without_a_context(device):
    lib = _lib.load()
    for kw, needle in [(dict(X=False), "X is NULL"), (dict(opts=False), "opts is NULL"), (dict(stats=False), "stats is NULL"),
                       (dict(info=False), "info is NULL"), (dict(T=3), "nkeep"), (dict(n=0), "nwalkers"), (dict(d=0), "ndim"),
                       (dict(c=0.0), "c must"), (dict(c=-1.0), "c must"), (dict(c=float("nan")), "c must"), (dict(c=float("inf")), "c must"),
                       (dict(max_lag=-1), "max_lag"), (dict(max_lag=8), "max_lag"), (dict(T=2 ** 31 - 1, n=2 ** 40, d=2 ** 20), "overflows"),
                       (dict(), "ctx is NULL")]:
        rc, msg = _stats_call(lib, device, **kw)
        assert rc == _lib.MCALF_ERR_INVALID and needle in msg, (kw, rc, msg)
    # the partial sums' byte limit names the largest lag that fits: 2^20 walkers are 16384 blocks, x 64 coordinates x 8 bytes
    rc, msg = _stats_call(lib, device, T=4096, n=2 ** 20, d=64)
    assert rc == _lib.MCALF_ERR_RANGE and "largest max_lag that fits is 127" in msg, msg


@pytest.mark.parametrize("device", [False, True])
def test_ensemble_converge_refuses_bad_arguments_without_a_context(device):
    lib = _lib.load()
    n, ndim = 4, 4
    buf, ibuf = np.zeros(4096), np.zeros(4096, dtype=np.int32)
    nkept, conv, nchk = C.c_int64(), C.c_int32(), C.c_int32()

    def call(opts=(40, 1, 0, 0, 2.0, 0, 0), cv=(10, 0, 50.0, 0.01, 5.0), CU=True, hist=True, nwalkers=n, have_cv=True, have_opts=True):
        o, c = _lib.mcalf_ens_opts(*opts), _lib.mcalf_converge_opts(*cv)
        p = buf.ctypes.data
        args = [None, p, nwalkers, C.addressof(o) if have_opts else None, C.addressof(c) if have_cv else None, p, p, p, ibuf.ctypes.data,
                ibuf.ctypes.data, p if CU else None, p, C.addressof(nkept), C.addressof(conv), C.addressof(nchk), p if hist else None, p,
                ibuf.ctypes.data]
        rc = lib.mcalf_ensemble_converge_device(*args, None) if device else lib.mcalf_ensemble_converge(*args)
        return rc, lib.mcalf_last_error(None).decode()

    for kw, needle in [(dict(have_cv=False), "conv is NULL"), (dict(CU=False), "CU is NULL"), (dict(hist=False), "tau_hist is NULL"),
                       (dict(cv=(0, 0, 50.0, 0.01, 5.0)), "check_every"), (dict(cv=(10, 0, 0.0, 0.01, 5.0)), "factor"),
                       (dict(cv=(10, 0, float("nan"), 0.01, 5.0)), "factor"), (dict(cv=(10, 0, 50.0, -0.1, 5.0)), "rtol"),
                       (dict(cv=(10, 0, 50.0, 0.01, 0.0)), "c must"), (dict(have_opts=False), "opts is NULL"), (dict(nwalkers=0), "nwalkers"),
                       (dict(nwalkers=5), "nwalkers"), (dict(opts=(40, 0, 0, 0, 2.0, 0, 0)), "thin"), (dict(opts=(40, 1, 0, 0, 1.0, 0, 0)), "scale"),
                       (dict(), "ctx is NULL")]:
        rc, msg = call(**kw)
        assert rc == _lib.MCALF_ERR_INVALID and needle in msg, (kw, rc, msg)
