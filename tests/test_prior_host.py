"""CPU: the Gaussian prior's surface that needs no device -- the refusals of the four C entries that come before any device
work, the checks and constants of mcalf_set_gauss_prior as a stand-alone program under AddressSanitizer and UBSan
(tests/stubs/prior_check_main.cpp over mc-alf_amd/csrc/prior_args.h: nothing loaded into Python runs under a sanitizer), the
parsing of the reference's `Gpriors` keyword, the Python signatures, and `tempering.ln_prior_mass` against a midpoint sum."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import mcalf_amd
from mcalf_amd import _lib, ensemble, nested, tempering
from mcalf_amd.routines.hires_fitter import parse_gpriors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entries_refuse_invalid_arguments_without_a_device():
    lib = _lib.load()
    rows, out = np.full((4, 3), 0.5), np.zeros(4)
    mu, sigma = np.zeros(3), np.ones(3)
    n = C.c_int32(-7)
    assert lib.mcalf_set_gauss_prior(None, mu.ctypes.data, sigma.ctypes.data) == _lib.MCALF_ERR_INVALID
    assert b"mcalf_set_gauss_prior: ctx is NULL" in lib.mcalf_last_error(None)
    assert lib.mcalf_set_gauss_prior(None, None, None) == _lib.MCALF_ERR_INVALID
    assert lib.mcalf_get_gauss_prior(None, None, None, None, C.byref(n)) == _lib.MCALF_ERR_INVALID and n.value == -7
    assert b"mcalf_get_gauss_prior: ctx is NULL" in lib.mcalf_last_error(None)
    host = lambda ctx, r, b, cube, o: lib.mcalf_lnprior_batch(ctx, r, b, cube, o)
    dev = lambda ctx, r, b, cube, o: lib.mcalf_lnprior_batch_device(ctx, r, b, cube, o, None)
    for call, name in ((host, b"mcalf_lnprior_batch"), (dev, b"mcalf_lnprior_batch_device")):
        for args, what in (((rows.ctypes.data, 4, 0, out.ctypes.data), b"ctx is NULL"),
                           ((rows.ctypes.data, -1, 0, out.ctypes.data), b"batch must be >= 0"),
                           ((None, 4, 0, out.ctypes.data), b"rows is NULL"),
                           ((rows.ctypes.data, 4, 1, None), b"lnprior is NULL"),
                           ((rows.ctypes.data, 4, 2, out.ctypes.data), b"from_cube must be 0 or 1"),
                           ((rows.ctypes.data, 4, -1, out.ctypes.data), b"from_cube must be 0 or 1"),
                           ((rows.ctypes.data, 2 ** 31, 1, out.ctypes.data), b"batch 2147483648 too large"),
                           ((None, 0, 1, None), b"ctx is NULL")):
            rc = call(None, *args)
            assert rc == (_lib.MCALF_ERR_RANGE if b"too large" in what else _lib.MCALF_ERR_INVALID), (args, rc)
            assert name + b": " + what in lib.mcalf_last_error(None), (args, lib.mcalf_last_error(None))
    assert not out.any()


def test_the_checks_and_constants_of_set_gauss_prior_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "prior_check_main")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I",
                    os.path.join(ROOT, "mc-alf_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stubs", "prior_check_main.cpp")], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-4000:]
    checks = {}
    for line in res.stdout.splitlines():
        if line.startswith("check "):
            _, label, rc, *msg = line.split(" ")
            checks[label] = (int(rc), " ".join(msg))
    assert checks["fine"] == (0, "") and checks["all-zero"] == (0, "")
    for label, needle in (("sigma-negative", "sigma[2] must be finite and >= 0"), ("sigma-nan", "sigma[3] must be finite and >= 0"),
                          ("sigma-inf", "sigma[0] must be finite and >= 0"), ("mu-nan", "mu[2] must be finite"), ("mu-inf", "mu[3] must be finite"),
                          ("ncomp-slot", "sigma[1] > 0 puts a Gaussian on the ncomp slot"), ("first-wins", "sigma[0] must be finite and >= 0")):
        assert checks[label][0] == -1 and needle in checks[label][1], (label, checks[label])
    rows = [line.split(" ") for line in res.stdout.splitlines() if line.startswith("c ")]
    sigma = np.array([float.fromhex(r[2]) for r in rows])
    c = np.array([float.fromhex(r[3]) for r in rows])
    on = sigma > 0.0
    assert sigma.size == 131 and f"ngauss {on.sum()}" in res.stdout and not c[~on].any()
    want = np.log(2.0 * np.pi * sigma[on] ** 2)
    assert (np.abs(c[on] - want) <= np.spacing(np.abs(want))).all()          # within 1 ulp of numpy's


def test_gpriors_parsing():
    assert parse_gpriors(None, 4) is None
    mu, sigma = parse_gpriors(['none', 'none', 1, 'none', 'none', 0.2, '13.5', '0.25'], 4)
    assert mu.tolist() == [0.0, 0.0, 0.0, 13.5] and sigma.tolist() == [0.0, 0.0, 0.0, 0.25]      # 'none' in either place: no Gaussian
    mu, sigma = parse_gpriors((8.0, 0.5, 'none', 'none'), 2)
    assert mu.tolist() == [8.0, 0.0] and sigma.tolist() == [0.5, 0.0]
    mu, sigma = parse_gpriors(np.array([8.0, 0.5, 1.0, 2.0]), 2)
    assert mu.tolist() == [8.0, 1.0] and sigma.tolist() == [0.5, 2.0]
    for bad in ([1.0, 0.5], [1.0, 0.5, 'none'], [1.0] * 10, []):
        with pytest.raises(ValueError, match="2 \\* ndim = 8 entries"):
            parse_gpriors(bad, 4)
    for bad in ([1.0, 0.0], [1.0, -0.5], [1.0, float("nan")]):
        with pytest.raises(ValueError, match="width of parameter 0"):
            parse_gpriors(bad, 1)
    with pytest.raises(ValueError):
        parse_gpriors(['None', 1.0], 1)                            # (only the reference's spelling)


def test_the_python_surface():
    fit = mcalf_amd.als_fitter
    assert list(inspect.signature(fit.set_gauss_prior).parameters) == ["self", "mu", "sigma"]
    assert list(inspect.signature(fit.clear_gauss_prior).parameters) == ["self"]
    assert isinstance(fit.gauss_prior, property)
    sig = inspect.signature(fit.lnprior_batch)
    assert list(sig.parameters) == ["self", "rows", "cube"] and sig.parameters["cube"].default is False
    assert list(inspect.signature(fit.lnprior).parameters) == ["self", "p"] and list(inspect.signature(fit.__call__).parameters) == ["self", "p"]
    assert inspect.signature(fit.__init__).parameters["Gpriors"].default is None
    assert nested.NestedResult.lnprior is None and ensemble.EnsembleResult.lnprior is None and tempering.TemperedResult.ln_prior_mass is None
    assert "does not enter" in fit.maximize_batch.__doc__


def test_the_drivers_carry_lnprior_through():
    """A `loglike_cube` that returns a third array: the ensemble result and the ladder's cold rung keep it; the ladder's
    evidence routes add ln_prior_mass when it is set and are untouched when it is not."""
    import ens_reference as er
    import pt_reference as pt
    logl = lambda U: -0.5 * (((U - 0.5) / 0.1) ** 2).sum(axis=1)
    lnp = lambda U: -3.0 * U[:, 0]
    three = lambda U: (U.copy(), logl(U), lnp(U))
    two = lambda U: (U.copy(), logl(U))
    res = ensemble.ensemble_sample(three, er.advance_with(logl), 3, 8, 12, thin=2, seed=1)
    assert res.lnprior.shape == (6, 8) and res.lnprior.tobytes() == lnp(res.cube.reshape(-1, 3)).tobytes()
    assert ensemble.ensemble_sample(two, er.advance_with(logl), 3, 8, 12, thin=2, seed=1).lnprior is None
    betas = [1.0, 0.2, 0.0]
    a = tempering.tempered_sample(two, pt.advance_with(logl, betas), 3, 8, 40, betas, seed=1)
    b = tempering.tempered_sample(three, pt.advance_with(logl, betas), 3, 8, 40, betas, seed=1)
    assert a.cold().lnprior is None and b.cold().lnprior.tobytes() == lnp(b.cube.reshape(-1, 3)).tobytes()
    za, zb = a.logZ_stepping_stone(), b.logZ_stepping_stone()
    assert za == zb and a.logZ_ti() == b.logZ_ti()
    b.ln_prior_mass = -1.25
    assert b.logZ_stepping_stone() == (za[0] + -1.25, za[1]) and b.logZ_ti() == a.logZ_ti() + -1.25


def test_ln_prior_mass_against_a_midpoint_sum():
    lo, hi = np.array([11.5, 0.0, -2.0, 1.0]), np.array([16.0, 1.0, 3.0, 30.0])
    mu, sigma = np.array([13.0, 0.4, 7.0, 0.0]), np.array([0.8, 0.15, 2.5, 0.0])      # inside, cut on both sides, centre outside, none
    assert tempering.ln_prior_mass(lo, hi, np.zeros(4), np.zeros(4)) == 0.0
    got = tempering.ln_prior_mass(lo, hi, mu, sigma)
    u = (np.arange(10 ** 6) + 0.5) / 10 ** 6
    want = 0.0
    for k in range(3):
        theta = lo[k] + u * (hi[k] - lo[k])
        want += np.log(np.mean(np.exp(-0.5 * (((theta - mu[k]) / sigma[k]) ** 2 + np.log(2.0 * np.pi * sigma[k] ** 2)))))
    print(f"ln_prior_mass {got!r}, midpoint sum {want!r}")
    assert abs(got - want) < 1e-9                                  # (the midpoint rule's error at 1e6 nodes is ~1e-12 here)
