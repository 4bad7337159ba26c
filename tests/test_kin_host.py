"""CPU: what of the batched optical-depth kinematics can be checked without a device -- the numpy restatement the GPU tests
compare against (tests/kin_reference.py) is anchored on closed forms of a single Gaussian-cored line, so that it is not its
own yardstick; the two C entries refuse every bad argument before they touch a device; the ABI number stands and the bindings
and the three Python entries of mcalf_amd.kinematics exist; dv90_batch / zabs_batch are host arithmetic on one kinematics_batch call."""
import math
import types

import numpy as np
import pytest
from scipy.special import erfinv

import kin_reference as kr
import mcalf_amd
from cases import problem_from_kwargs
from mcalf_amd import _lib, kinematics as kn
from oracle import numpy_oracle as o

CIV1548 = kr.CIV1548
K_TAU = 0.014971475                       # the oracle's (and the kernels') pi e^2 / (m_e c) in cgs
seam_kw, seam_lam0, seam_row = kr.seam_kw, kr.seam_lam0, kr.seam_row


@pytest.mark.parametrize("N,b", [(13.0, 12.0), (15.5, 6.0)])
def test_the_integral_is_the_closed_form(N, b):
    """Integral of tau dlambda of one line = kTauConst sqrt(pi) f 10^N wrest^2 (1 + z) / c (the integral of H over u is
    sqrt(pi)), here in Angstrom.  The 40 Angstrom window cuts the damping wings: measured 2.2e-6 below."""
    kw = seam_kw()
    prob = problem_from_kwargs(kw)
    p = seam_row(kw, N, b)
    row = kr.Row(prob, p)
    wrest_cm = CIV1548[0] * 1e-8
    closed = K_TAU * math.sqrt(math.pi) * CIV1548[1] * 10.0 ** N * wrest_cm ** 2 * (1.0 + p[2]) / o.CCGS * 1e8
    rel = row.I[0] / closed - 1.0
    print(f"I / closed form - 1 at (N, b) = ({N}, {b}): {rel:.3g}")
    assert abs(rel) <= 1e-4


def test_centroid_median_and_dv90_of_a_gaussian_core():
    """(N, b) = (13, 12): the line is symmetric about LAM0, so the median and the mean sit on it; the core is a Gaussian of
    sigma = b / sqrt(2) in velocity, so dv90 / b = 2 erfinv(0.9) = 2.32617 up to the damping wings' share."""
    kw = seam_kw()
    prob = problem_from_kwargs(kw)
    row = kr.Row(prob, seam_row(kw, 13.0, 12.0), q=(0.05, 0.5, 0.95))
    lam0 = seam_lam0(kw)
    lo, med, hi = row.lam_q[0]
    ratio = o.CLIGHT_KMS * (hi - lo) / med / 12.0
    print(f"|lam_0.5 - lam0| {abs(med - lam0):.3g}, |lam_mean - lam0| {abs(row.lam_mean[0] - lam0):.3g}, dv90 / b {ratio:.6g}")
    assert abs(med - lam0) <= 1e-4 and abs(row.lam_mean[0] - lam0) <= 1e-4
    assert abs(ratio - 2.0 * erfinv(0.9)) <= 2e-3
    # the width: sigma_lambda = lam0 (b / sqrt 2) / c for the Gaussian core; the Lorentzian wings inside the window add to it
    assert row.lam_rms[0] >= lam0 * 12.0 / math.sqrt(2.0) / o.CLIGHT_KMS * (1 - 1e-3)


@pytest.mark.parametrize("N,b", [(13.0, 12.0), (15.5, 6.0)])
def test_the_restatements_quantiles_invert_its_own_cumulative(N, b):
    """C(lam_q) = q I to rounding: the margin the GPU bar (1e-11 + 1e-9 |I|) has over the reference alone."""
    kw = seam_kw()
    prob = problem_from_kwargs(kw)
    q = np.linspace(0.0, 1.0, 16)
    row = kr.Row(prob, seam_row(kw, N, b), q=q)
    worst = max(abs(row.C(0, row.lam_q[0, j]) - q[j] * row.I[0]) for j in range(q.size))
    print(f"worst |C(lam_q) - q I| / I at (N, b) = ({N}, {b}): {worst / row.I[0]:.3g}")
    assert worst <= 1e-11 + 1e-9 * row.I[0]
    assert row.e[0] <= row.lam_q[0, 0] and row.lam_q[0, -1] <= row.e[-1] and np.all(np.diff(row.lam_q[0]) >= 0)


def test_degenerate_rows_of_the_restatement():
    kw = seam_kw(ncompmax=2)
    prob = problem_from_kwargs(kw)
    p = np.array([0.0, 13.0, 3.0, 12.0, np.nan, np.nan, np.nan])
    row = kr.Row(prob, p, q=(0.5,))
    assert row.I[0] == 0.0 and np.isnan(row.lam_mean[0]) and np.isnan(row.lam_rms[0]) and np.isnan(row.lam_q).all()
    p[0] = 1.0                                                     # the NaN slot stays inactive
    assert np.isfinite(kr.Row(prob, p, q=(0.5,)).lam_q).all()
    p[0] = 2.0
    row = kr.Row(prob, p, q=(0.5,))
    assert np.isnan(row.I[0]) and np.isnan(row.lam_mean[0]) and np.isnan(row.lam_q).all()
    e = kr.edges(prob.wl)
    assert e.size == prob.wl.size + 1 and np.all(np.diff(e) > 0) and e[0] < prob.wl[0] and e[-1] > prob.wl[-1]


def _call(lib, name, ctx, P, batch, q, nq, mom, lamq):
    if name.endswith("_device"):
        return getattr(lib, name)(ctx, P, batch, q, nq, mom, lamq, None)
    return getattr(lib, name)(ctx, P, batch, q, nq, mom, lamq)


@pytest.mark.parametrize("name", ["mcalf_kinematics_batch", "mcalf_kinematics_batch_device"])
def test_argument_errors_are_refused_with_a_message(name):
    """Code -1 and a message that names the entry and the argument, before any device work: none of these needs a device (the
    spectrum of fewer than 2 pixels needs a context, tests/test_gpu_kin.py)."""
    lib = _lib.load()
    buf = np.zeros(64)
    ptr = buf.ctypes.data
    q = np.array([0.05, 0.5, 0.95])
    qp = q.ctypes.data

    def bad(v):
        a = np.array([0.5, v, 0.7])
        return a

    keep = [bad(np.nan), bad(np.inf), bad(-0.01), bad(1.5)]
    cases = [
        ((None, ptr, -1, qp, 3, ptr, ptr), "batch"),
        ((None, None, 4, qp, 3, ptr, ptr), "P is NULL"),
        ((None, ptr, 4, qp, -1, ptr, ptr), "nq"),
        ((None, ptr, 4, qp, 17, ptr, ptr), "nq"),
        ((None, ptr, 4, None, 3, ptr, ptr), "q is NULL"),
        ((None, ptr, 4, qp, 3, ptr, None), "lamq is NULL"),
        ((None, ptr, 4, None, 0, ptr, ptr), "lamq is given with nq = 0"),
        ((None, ptr, 4, None, 0, None, None), "mom and lamq"),
        ((None, ptr, 4, qp, 3, ptr, ptr), "ctx is NULL"),
        ((None, ptr, 0, qp, 3, ptr, ptr), "ctx is NULL"),
        ((None, ptr, 4, None, 0, ptr, None), "ctx is NULL"),
    ] + [((None, ptr, 4, a.ctypes.data, 3, ptr, ptr), "q[1]") for a in keep]
    for args, needle in cases:
        assert _call(lib, name, *args) == _lib.MCALF_ERR_INVALID, args
        msg = lib.mcalf_last_error(None).decode()
        assert needle in msg and name + ":" in msg, (args, msg)


def test_abi_number_and_bindings():
    lib = _lib.load()
    assert b"abi 9" in lib.mcalf_version()
    assert "mcalf_kinematics_batch" in _lib.SYMBOLS and "mcalf_kinematics_batch_device" in _lib.SYMBOLS
    assert hasattr(lib, "mcalf_kinematics_batch") and hasattr(lib, "mcalf_kinematics_batch_device")
    for name in ("kinematics_batch", "dv90_batch", "zabs_batch"):
        assert callable(getattr(mcalf_amd.kinematics, name))
    assert kn.Kinematics._fields == ("tau_int", "lam_mean", "lam_rms", "lam_q")


def test_dv90_and_zabs_are_host_arithmetic_on_one_kinematics_call(monkeypatch):
    """On a stand-in for the fitter, with kinematics_batch replaced by one that returns known numbers."""
    calls = []
    lam_q = np.array([[[6190.0, 6200.0, 6205.0], [6200.0, 6210.0, 6230.0]],
                      [[np.nan, np.nan, np.nan], [6201.0, 6202.0, 6204.0]]])
    lam_mean = np.array([[6199.0, 6211.0], [np.nan, 6202.5]])

    def kinematics_batch(fit, P, q=(0.05, 0.5, 0.95), out=None):
        calls.append(tuple(q))
        return kn.Kinematics(None, lam_mean, None, lam_q if len(q) else np.empty((2, 2, 0)))

    monkeypatch.setattr(kn, "kinematics_batch", kinematics_batch)
    fit = types.SimpleNamespace(numlines=2, linepars=[dict(wrest=1548.204), dict(wrest=1550.781)])
    P = np.zeros((2, 4))
    for k in range(2):
        got = kn.dv90_batch(fit, P, lineid=k)
        want = 2.9979245e5 * (lam_q[:, k, 2] - lam_q[:, k, 0]) / lam_q[:, k, 1]
        assert np.array_equal(got, want, equal_nan=True) and got.shape == (2,)
        got = kn.zabs_batch(fit, P, lineid=k)
        assert np.array_equal(got, lam_mean[:, k] / fit.linepars[k]["wrest"] - 1.0, equal_nan=True)
    assert calls == [(0.05, 0.5, 0.95), (), (0.05, 0.5, 0.95), ()]
    assert np.isnan(kn.dv90_batch(fit, P)[1]) and np.isnan(kn.zabs_batch(fit, P)[1])
    for bad in (2, -1):
        with pytest.raises(ValueError):
            kn.dv90_batch(fit, P, lineid=bad)
        with pytest.raises(ValueError):
            kn.zabs_batch(fit, P, lineid=bad)
    assert len(calls) == 6                                        # a bad lineid is refused before any call
