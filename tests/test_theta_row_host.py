"""CPU: the rules by which a parameter row is read -- mc-alf_amd/csrc/theta_row.h, the header the derivative, equivalent-width
and fit kernels decode their rows with -- run in a stand-alone program under AddressSanitizer and UBSan
(tests/stubs/theta_row_check.cpp; nothing loaded into Python runs under a sanitizer).  Every expectation is computed here:
the layout against the planner's indices and against the slices oracle/numpy_oracle.py: reconstruct_spec takes, the count rule
against int() / math.floor, the record arithmetic bit for bit against numpy float64 in the same order, the LSF half-width
against the reference's expressions.  Built with -ffp-contract=off (the chains are products only: nothing would fuse anyway)."""
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import numpy_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FWHM_TO_SIGMA, KERNEL_REACH, TAU_CONST = 2.354820, 3.0348, 0.014971475          # hires_fitter.py:454, :458, :364


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("theta_row") / "theta_row_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I",
                    os.path.join(ROOT, "mc-alf_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stubs", "theta_row_check.cpp")], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-4000:]
    recs = [json.loads(line) for line in res.stdout.splitlines()]
    return {kind: [r for r in recs if r["kind"] == kind] for kind in ("layout", "count", "line_scale", "half_width")}


def oracle_columns(monkeypatch, r):
    """The columns reconstruct_spec reads for a row that carries its own column numbers: (targets, fillers, R, cont)."""
    wl = 6190.0 * np.exp(np.arange(96) * 2.0 / 2.99792458e5)
    prob = oracle.Problem(wl=wl, flux=np.ones(96), err=np.full(96, 0.05), lines=[(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8)],
                          ncomp=(0, r["ncompmax"]), nfill=r["nfill"], specres=[6.0, 8.0] if r["freespecres"] else [7.0],
                          contval=[0.9, 1.1] if r["freecont"] else [0.97], velstep=2.0)
    seen, conv = [], []
    monkeypatch.setattr(oracle, "voigt_model", lambda wl_, N, b, z, wrest, f, gam: seen.append((N, z, b, wrest)) or np.ones_like(wl_))
    monkeypatch.setattr(oracle, "convolve_model", lambda spec, fwhm, velstep: conv.append(fwhm) or spec)
    p = 100.0 + np.arange(prob.ndim)
    p[prob.startind] = r["ncompmax"]
    model = oracle.reconstruct_spec(prob, p)
    assert all(z == N + 1 and b == N + 2 for N, z, b, _ in seen)                      # three consecutive columns, in the order (N, z, b)
    first = lambda lines: sorted({int(N) - 100 for N, _, _, w in seen if (w == 250.0) == (lines == "fill")})
    return prob, first("target"), first("fill"), conv[0], float(model[0])


def test_layouts_are_the_planners_and_the_oracles(records, monkeypatch):
    recs = records["layout"]
    assert sorted((r["freespecres"], r["freecont"], r["nfill"], r["ncompmax"]) for r in recs) == sorted(
        (fs, fc, nf, nc) for fs in (0, 1) for fc in (0, 1) for nf in (0, 2) for nc in (1, 3))
    for r in recs:
        tag = (r["freespecres"], r["freecont"], r["nfill"], r["ncompmax"])
        prob, targets, fillers, R, cont = oracle_columns(monkeypatch, r)
        for f in ("ndim", "startind", "endind"):
            assert r[f] == r["plan"][f] == getattr(prob, f), (tag, f)
        assert r["target_col"] == targets == [1 + 3 * c + prob.startind for c in range(r["ncompmax"])], tag
        assert r["filler_col"] == fillers == [3 * k + prob.endind for k in range(r["nfill"])], tag
        # R and the continuum: their columns where they are free (the row holds 100 + column), the fixed values otherwise
        assert float.fromhex(r["R"]) == R == (100.0 if r["freespecres"] else 7.0), tag
        assert float.fromhex(r["cont"]) == cont == (100.0 + r["cont_col"] if r["freecont"] else 0.97), tag
        assert r["cont_col"] == r["freespecres"], tag
        # movable: every column but the count slot and the (N, z, b) of the slots at or beyond the count
        assert len(r["movable"]) == r["ncompmax"] + 1
        for nc, got in enumerate(r["movable"]):
            dead = {prob.startind} | {col + j for col in targets[nc:] for j in range(3)}
            assert got == [0 if k in dead else 1 for k in range(prob.ndim)], (tag, nc)


def test_count_rule_in_both_modes(records):
    recs = records["count"]
    for jax in (0, 1):
        for ncompmax in (1, 3):
            vals = [float.fromhex(r["value"]) for r in recs if r["jax"] == jax and r["ncompmax"] == ncompmax]
            want = [-math.inf, -1.5, -0.0, 0.0, math.nextafter(1.0, 0.0), 1.0, 1.5, ncompmax - 0.5, float(ncompmax), ncompmax + 0.5, 1e300, math.inf]
            assert all(any(v == w and math.copysign(1, v) == math.copysign(1, w) for v in vals) for w in want), (jax, ncompmax)
            assert sum(math.isnan(v) for v in vals) == 1
            assert any(math.isfinite(v) and v < 0 and int(v) != math.floor(v) for v in vals)  # int() and floor differ there
    for r in recs:
        v, m = float.fromhex(r["value"]), r["ncompmax"]
        if math.isnan(v) or v == -math.inf:
            want = 0
        elif v == math.inf:
            want = m
        else:
            want = min(max(math.floor(v) if r["jax"] else int(v), 0), m)
        assert r["count"] == want, r


def as_f64(hexbits):
    return np.array([int(hexbits, 16)], dtype=np.uint64).view(np.float64)[0]


def test_line_scale_bit_for_bit(records):
    recs = records["line_scale"]
    assert len(recs) >= 12
    kinds = set()
    with np.errstate(all="ignore"):
        for r in recs:
            z, b, cold, wrest, f, g4, nujk = (as_f64(r[k]) for k in ("z", "b", "cold", "wrest_cm", "f", "gamma4pi", "nujk"))
            zp1 = z + np.float64(1.0)
            rdnu = wrest / (b * np.float64(1e5))
            want = {"zp1": zp1, "rdnu": rdnu, "A": zp1 * rdnu, "B": nujk * rdnu, "a": g4 * rdnu, "K": np.float64(TAU_CONST) * cold * f * rdnu}
            for k, v in want.items():
                assert int(r[k], 16) == int(np.array([v]).view(np.uint64)[0]), (k, r, float(v))
            a, K = want["a"], want["K"]
            kind = 1                                                                     # fast
            if not (a <= 2.0 ** -8) or not (a >= 0.0):
                kind = 2                                                                 # general
            elif K * 1.6e-28 > 2e-17:
                kind = 2
            if not (abs(zp1) < 1e100) and zp1 == zp1 and abs(K) < 1e100 and abs(a) < 1e100:
                kind = 3                                                                 # exact zero
            assert r["record_kind"] == kind, r
            kinds.add(kind)
    assert kinds == {1, 2, 3}
    # the cases the list is there for
    vals = [(as_f64(r["z"]), as_f64(r["b"])) for r in recs]
    assert any(b < 0 for _, b in vals) and any(b == 0 for _, b in vals) and any(z == -1 for z, _ in vals)
    assert any(abs(1 + z) > 1e100 and np.isfinite(z) for z, _ in vals)
    for k in ("z", "b", "cold", "wrest_cm"):
        assert any(np.isnan(as_f64(r[k])) for r in recs), k


def test_lsf_half_width(records):
    """numpy path: no taps when R <= velstep -- a NaN R fails that comparison too, as it does in the reference (`if R > velstep`,
    hires_fitter.py:445) and in every kernel; beyond it astropy's ceil(kKernelReach sigma), `bad` when that exceeds n_cap (+inf
    included).  JAX path: the context's fixed half-width whatever R is."""
    recs = records["half_width"]
    seen = set()
    for r in recs:
        R, velstep = float.fromhex(r["R"]), float.fromhex(r["velstep"])
        if r["jax"]:
            assert (r["n"], r["bad"]) == (r["jax_half"], 0), r
            continue
        if not (R > velstep):
            want = (0, 0)
            seen.add("nan" if math.isnan(R) else "none")
        else:
            nd = np.ceil(np.float64(KERNEL_REACH) * ((np.float64(R) / np.float64(FWHM_TO_SIGMA)) / np.float64(velstep)))
            want = (int(nd), 0) if nd <= r["n_cap"] else (0, 1)
            seen.add(int(nd) - r["n_cap"] if np.isfinite(nd) and abs(nd - r["n_cap"]) <= 1 else ("inf" if np.isinf(nd) else "far"))
        assert (r["n"], r["bad"]) == want, r
    assert {"none", "nan", -1, 0, 1, "inf"} <= seen
    assert any(r["jax"] and math.isnan(float.fromhex(r["R"])) for r in recs)
