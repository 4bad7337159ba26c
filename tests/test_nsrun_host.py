"""CPU: what the device-resident nested-sampling run (mcalf_nested_*) decides without a device -- the struct layouts, every
refusal that needs no context, the Python function's signature -- and its evidence arithmetic, mc-alf_amd/csrc/ns_evidence.h,
driven from a stand-alone program under AddressSanitizer and UBSan (tests/stubs/ns_evidence_check.cpp; nothing loaded into
Python runs under a sanitizer) against the numpy restatement tests/nsrun_reference.py.

The bar on ln Z, H and the log weights is 1e-9 absolute: ndead eps |ln Z| with ndead <= 2e4 and |ln Z| ~ 1e2 is 4e-10 at most
for the two left folds, and the rest is libm against numpy, an ulp or two per weight."""
import ctypes as C
import inspect
import os
import shutil
import subprocess

import numpy as np
import pytest

import nsrun_reference as ref
from mcalf_amd import _lib, nested_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _opts(**over):
    kw = dict(batch=4, nmoves=8, max_steps=400, reserved=0, seed=1, dlogz=1e-3, max_dead=1000)
    kw.update(over)
    return _lib.mcalf_nested_opts(**kw)


def test_the_structs_match_the_header_layout():
    o, s = _lib.mcalf_nested_opts, _lib.mcalf_nested_state_t
    assert C.sizeof(o) == 40 and (o.batch.offset, o.nmoves.offset, o.max_steps.offset, o.seed.offset, o.dlogz.offset, o.max_dead.offset) == (0, 4, 8, 16, 24, 32)
    assert C.sizeof(s) == 80
    assert [getattr(s, f).offset for f, _ in s._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76]
    assert (_lib.MCALF_NESTED_BUDGET, _lib.MCALF_NESTED_CONVERGED, _lib.MCALF_NESTED_PLATEAU, _lib.MCALF_NESTED_FULL) == (0, 1, 2, 3)


def test_open_refuses_invalid_arguments_without_a_device():
    lib = _lib.load()
    U0 = np.full((16, 4), 0.5)
    ok = _opts()
    err = lambda: lib.mcalf_last_error(None)
    assert lib.mcalf_nested_open(None, None, 16, C.addressof(ok)) == _lib.MCALF_ERR_INVALID and b"mcalf_nested_open: U0 is NULL" in err()
    assert lib.mcalf_nested_open(None, U0.ctypes.data, 16, None) == _lib.MCALF_ERR_INVALID and b"mcalf_nested_open: opts is NULL" in err()
    for over, what in ((dict(batch=0), b"batch must be in [1, nlive)"), (dict(batch=16), b"batch must be in [1, nlive)"), (dict(batch=-3), b"batch"),
                       (dict(nmoves=-1), b"nmoves must be >= 0"), (dict(max_steps=-2), b"max_steps must be >= 0"), (dict(dlogz=-1e-3), b"dlogz must be >= 0"),
                       (dict(dlogz=float("nan")), b"dlogz must be >= 0"), (dict(max_dead=19), b"max_dead must be >= nlive + batch = 20")):
        bad = _opts(**over)
        assert lib.mcalf_nested_open(None, U0.ctypes.data, 16, C.addressof(bad)) == _lib.MCALF_ERR_INVALID, over
        assert b"mcalf_nested_open: " in err() and what in err(), (over, err())
    big = _opts(batch=1024, max_dead=10 ** 7)
    assert lib.mcalf_nested_open(None, U0.ctypes.data, 262145, C.addressof(big)) == _lib.MCALF_ERR_RANGE and b"cap of 262144" in err()
    assert lib.mcalf_nested_open(None, U0.ctypes.data, 16, C.addressof(ok)) == _lib.MCALF_ERR_INVALID and b"mcalf_nested_open: ctx is NULL" in err()
    zero = _opts(dlogz=0.0, max_dead=20)                                   # (valid: refused for the context alone)
    assert lib.mcalf_nested_open(None, U0.ctypes.data, 16, C.addressof(zero)) == _lib.MCALF_ERR_INVALID and b"ctx is NULL" in err()


def test_the_other_entries_refuse_a_null_context():
    lib = _lib.load()
    err = lambda: lib.mcalf_last_error(None)
    st = _lib.mcalf_nested_state_t()
    ms = np.zeros(7)
    assert lib.mcalf_nested_advance(None, -1, C.addressof(st)) == _lib.MCALF_ERR_INVALID and b"mcalf_nested_advance: max_rounds must be >= 0" in err()
    for name, call in (("advance", lambda: lib.mcalf_nested_advance(None, 1, C.addressof(st))), ("finish", lambda: lib.mcalf_nested_finish(None, None, None, None)),
                       ("read", lambda: lib.mcalf_nested_read(None, 0, 0, None, None, None, None)),
                       ("last_round", lambda: lib.mcalf_nested_last_round(None, None, None, None, None)), ("close", lambda: lib.mcalf_nested_close(None)),
                       ("set_timing", lambda: lib.mcalf_nested_set_timing(None, 1)),
                       ("footprint", lambda: lib.mcalf_nested_footprint(None, C.byref(C.c_int64()))), ("last_times", lambda: lib.mcalf_nested_last_times(None, ms.ctypes.data))):
        assert call() == _lib.MCALF_ERR_INVALID, name
        assert b"mcalf_nested_" + name.encode() + b": ctx is NULL" in err(), (name, err())


def test_the_python_function_is_a_module_level_one_with_the_host_drivers_defaults():
    import mcalf_amd
    sig = inspect.signature(nested_device.nested_sample_device)
    assert list(sig.parameters) == ["fit", "nlive", "batch", "nmoves", "max_steps", "dlogz", "max_rounds", "seed", "max_dead", "rounds_per_call"]
    got = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert got == dict(batch=None, nmoves=None, max_steps=None, dlogz=1e-3, max_rounds=100000, seed=0, max_dead=None, rounds_per_call=64)
    host = inspect.signature(mcalf_amd.als_fitter.nested_sample).parameters
    assert all(host[k].default == got[k] for k in ("batch", "nmoves", "dlogz", "max_rounds", "seed", "max_steps"))
    assert not hasattr(mcalf_amd.als_fitter, "nested_sample_device") and mcalf_amd.nested_device is nested_device


# ---- ns_evidence.h ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def evidence_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ns_evidence") / "ns_evidence_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I",
                    os.path.join(ROOT, "mc-alf_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stubs", "ns_evidence_check.cpp")], check=True)
    return exe


def _run(exe, tmp_path, logL, nlive, K):
    src, dst = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    np.ascontiguousarray(logL, dtype=float).tofile(src)
    res = subprocess.run([exe, src, dst, str(nlive), str(K)], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-4000:]
    out = np.fromfile(dst)
    return out[:5], out[5:]


def _dead(rng, nlive, K, rounds, scale=100.0):
    """An ascending dead sequence of a run's shape: logL ~ scale minus a shrinking exponential tail."""
    x = np.sort(rng.exponential(1.0, rounds * K + nlive))[::-1]
    return scale - 40.0 * x


@pytest.mark.parametrize("nlive,K,rounds", [(8, 1, 30), (8, 7, 5), (200, 16, 40), (256, 64, 60), (1000, 250, 76), (5, 4, 0)])
def test_the_evidence_is_the_numpy_restatements(evidence_exe, tmp_path, nlive, K, rounds):
    logL = _dead(np.random.default_rng(nlive + K), nlive, K, rounds)
    assert logL.size <= 20000
    head, logw = _run(evidence_exe, tmp_path, logL, nlive, K)
    logZ, H, want = ref.finish(logL, nlive, K)
    print(f"nlive {nlive} K {K} rounds {rounds}: ln Z {head[0]:.6f} off by {abs(head[0] - logZ):.2e}, H off by {abs(head[1] - H):.2e}, "
          f"logw off by {np.abs(logw - want).max():.2e}")
    assert abs(head[0] - logZ) <= 1e-9 and abs(head[1] - H) <= 1e-9 and np.abs(logw - want).max() <= 1e-9
    assert abs(np.exp(logw).sum() - 1.0) <= 1e-12
    ev = ref.Evidence()                                                    # the running value that steers the stop
    for r in range(rounds):
        ev.die(logL[r * K:(r + 1) * K], nlive)
    if rounds:
        assert abs(head[2] - ev.logZ) <= 1e-9 and abs(head[3] - ev.logX) <= 1e-12
    else:
        assert head[2] == -np.inf and head[3] == 0.0
    assert bool(head[4]) == bool(ev.converged(logL[-1], 1e-3))


def test_weightless_points_come_first_and_stay_weightless(evidence_exe, tmp_path):
    logL = _dead(np.random.default_rng(0), 50, 10, 20)
    logL[:7] = [np.nan, -np.inf, np.nan, -np.inf, -np.inf, np.nan, -np.inf]
    head, logw = _run(evidence_exe, tmp_path, logL, 50, 10)
    logZ, H, want = ref.finish(logL, 50, 10)
    assert np.isneginf(logw[:7]).all() and np.isfinite(logw[7:]).all() and np.isneginf(want[:7]).all()
    assert abs(head[0] - logZ) <= 1e-9 and abs(head[1] - H) <= 1e-9 and np.abs(logw[7:] - want[7:]).max() <= 1e-9
    assert abs(np.exp(logw).sum() - 1.0) <= 1e-12
    # a run of weightless points only: ln Z = -inf, no NaN weight arithmetic in H
    head, logw = _run(evidence_exe, tmp_path, np.full(12, -np.inf), 4, 2)
    assert head[0] == -np.inf and head[1] == 0.0 and head[2] == -np.inf and head[4] == 0.0
