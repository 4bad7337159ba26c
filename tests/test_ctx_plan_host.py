"""CPU: what mcalf_create decides from a spec before it touches a device -- the checks, the launch geometry, the host tables --
planned by mc-alf_amd/csrc/ctx_plan.h (the header host_abi.cpp: create_impl plans with) in a stand-alone program under
AddressSanitizer and UBSan (tests/stubs/ctx_plan_check.cpp; nothing loaded into Python runs under a sanitizer), against
tests/golden/ctx_plan.json, which was recorded from the arithmetic of create_impl before the planner existed (tests/golden/README.md).
Field by field and without a tolerance: integers by value, doubles (hex floats) and the tables' FNV-1a digests by bits.
Built with -ffp-contract=off: the library's host build targets plain x86-64, where nothing is fused either.

The list of specs is there for the planner's branches; the last test holds the golden file to taking every one of them."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ctx_plan.json")


def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def records(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("ctx_plan") / "ctx_plan_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off", "-I",
                    os.path.join(ROOT, "mc-alf_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "stubs", "ctx_plan_check.cpp")], check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and not res.stderr, res.stderr[-4000:]
    return [json.loads(line) for line in res.stdout.splitlines()]


def test_the_planner_decides_what_create_decided(records):
    want = golden()
    assert [r["name"] for r in records] == [w["name"] for w in want]
    for got, ref in zip(records, want):
        assert sorted(got) == sorted(ref), got["name"]
        for key in ref:
            if isinstance(ref[key], dict):
                assert sorted(got[key]) == sorted(ref[key]), (got["name"], key)
                for f in ref[key]:
                    assert got[key][f] == ref[key][f], (got["name"], key, f, got[key][f], ref[key][f])
            else:
                assert got[key] == ref[key], (got["name"], key, got[key], ref[key])


def test_doubles_and_digests_are_kept_as_bits():
    """What compares by bits is a string in the golden file (a hex float or 16 hex digits), never a JSON number."""
    for r in golden():
        if r["rc"] == 0:
            for f in ("specres_fixed", "specres_max", "contval_fixed", "velstep", "veto4", "veto5", "dnu_seg"):
                assert isinstance(r["shape"][f], str) and float.fromhex(r["shape"][f]) == float.fromhex(r["shape"][f]), (r["name"], f)
            assert all(isinstance(v, str) and len(v) == 16 for v in list(r["fnv"].values()) + r["segok"]), r["name"]
            assert len(r["segok"]) == r["shape"]["ntiles"]


def test_every_branch_is_taken_by_a_case():
    recs = golden()
    ok = [r for r in recs if r["rc"] == 0]
    shapes = [dict(r["shape"], lps_env=r["spec"]["lps_env"], name=r["name"]) for r in ok]
    by = {r["name"]: r for r in recs}

    def some(pred):
        return any(pred(s) for s in shapes)
    # the geometry
    assert some(lambda s: s["wide"] == 1 and s["n_cap"] == 0 and s["wide_n_cap"] > 0) and some(lambda s: s["wide"] == 0 and s["n_cap"] > 0)
    assert some(lambda s: s["wide"] == 1 and s["conv_mode"] == 1 and s["jax_half"] == s["wide_n_cap"])
    assert some(lambda s: s["wide"] == 1 and s["selfhalo"] == 1) and some(lambda s: s["wide"] == 1 and s["ntiles"] > 1)
    assert some(lambda s: s["wide"] == 0 and s["n_cap"] == 0 and s["conv_mode"] == 0) and some(lambda s: s["conv_mode"] == 1 and s["wide"] == 0)
    assert some(lambda s: s["lps"] == 4 and s["lps_env"] == -1) and some(lambda s: s["lps"] == 5 and s["lps_env"] == -1)
    assert some(lambda s: s["lps"] == 4 and s["lps_env"] == 4 and s["ncl_cap"] == 5)           # forced over an automatic 5
    assert some(lambda s: s["lps"] == 5 and s["lps_env"] == 5 and s["ncl_cap"] == 4)           # honoured over an automatic 4
    assert some(lambda s: s["lps"] == 4 and s["lps_env"] == 5)                                 # refused by the fit test
    assert some(lambda s: s["lps"] == 5 and s["lps_env"] == 7)                                 # not a value: ignored
    assert some(lambda s: s["selfhalo"] == 1) and some(lambda s: s["selfhalo"] == 0 and s["ntiles"] == 1)
    assert {1, 2, 3} <= {s["ntiles"] for s in shapes}
    assert some(lambda s: s["seg_search"] == 1) and some(lambda s: s["selfhalo"] == 1 and s["seg_search"] == 0)
    fixed, free = by["reach-fixed"], by["reach-free"]        # the same spec but for freespecres: specres_fixed 30 over specres_max 8
    hexf = float.fromhex
    assert hexf(fixed["spec"]["specres_max"]) == hexf(free["spec"]["specres_max"]) == 8.0 and fixed["spec"]["freespecres"] == 0 and free["spec"]["freespecres"] == 1
    assert hexf(fixed["shape"]["specres_max"]) == 30.0 and fixed["shape"]["n_cap"] == 20 and hexf(free["shape"]["specres_max"]) == 8.0
    # the thresholds, from either side
    assert (by["tile4080"]["shape"]["ntiles"], by["tile4080"]["shape"]["selfhalo"]) == (1, 1)
    t = by["tile4081"]["shape"]
    assert (t["ntiles"], t["selfhalo"], t["tile"]) == (2, 0, 2048)
    assert (by["fit971"]["shape"]["wide"], by["fit971"]["shape"]["n_cap"]) == (0, 971)
    assert (by["wide972"]["shape"]["wide"], by["wide972"]["shape"]["wide_n_cap"]) == (1, 972)
    assert by["lps-137"]["shape"]["lps"] == 5 and by["lps-138"]["shape"]["lps"] == 4
    assert by["ncl242"]["shape"]["wide"] == 0 and by["ncl243"]["shape"]["wide"] == 1 and by["ncl244"]["rc"] == -4
    assert by["jax32"]["shape"]["jax_half"] == 32 and by["jax33"]["rc"] == -1
    assert by["jax-f32"]["shape"]["n_cap"] == 6 and by["numpy-f64"]["shape"]["n_cap"] == 7     # the float32 ceiling against the double one
    # the virtual pixels: a recognised grid completes the last partial segment, an unrecognised one does not
    last = lambda name: (int(by[name]["segok"][0], 16) >> (by[name]["shape"]["seg_nreal"] - 1)) & 1
    assert last("log130") == 1 and last("linear130") == 1 and last("log66") == 1 and last("log65") == 0 and last("log63") == 0
    assert int(by["gap700"]["segok"][0], 16) == 2 ** 64 - 1 - (1 << 4)                         # pixel 299 / 300 lies in segment 4
    assert by["tile4096"]["nu_len"] == 4096 and by["tile4081"]["nu_len"] == 4081 and by["log7"]["nu_len"] == 4096
    # every refusal, with its message
    refusals = {(r["refused_by"], r["rc"], r["msg"].split(" (")[0]) for r in recs if r["rc"] != 0}
    assert refusals == {
        ("check_spec", -1, "spec is NULL"), ("check_spec", -1, "npix must be > 0 and wl/flux/err non-NULL"), ("check_spec", -4, "npix too large"),
        ("check_spec", -1, "need at least one line"), ("check_spec", -1, "negative component counts"), ("check_spec", -1, "velstep must be > 0"),
        ("check_spec", -1, "unknown conv_mode 2"), ("check_spec", -1, "specres_max must be finite and > 0"),
        ("plan_shape", -1, "JAX-path LSF kernel"), ("plan_shape", -4, "LSF half-width 31000000 px"),
        ("plan_shape", -4, "244 component-lines do not fit the 79872-byte LDS budget")}
    for name in ("bad-npix0", "bad-null-wl", "bad-nlines0", "bad-null-lines", "bad-ncompmax", "bad-nfill", "bad-specres0", "bad-specres-inf"):
        assert by[name]["refused_by"] == "check_spec", name
    assert by["jax33"]["msg"] == ("JAX-path LSF kernel (67 taps) is longer than the spectrum (65 px): the reference's jnp.convolve(..., 'same') / "
                                  "jnp.where (hires_fitter.py:674-681) cannot broadcast either")
    assert by["wide-6e7"]["msg"] == ("LSF half-width 31000000 px (specres_max 2.41e+04 km/s at 0.001 km/s/px) with 1 component-lines does not fit a "
                                     "4096-pixel workgroup tile / the 79872-byte LDS budget")
