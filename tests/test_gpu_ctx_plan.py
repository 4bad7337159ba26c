"""GPU: mcalf_create decides what the planner of mc-alf_amd/csrc/ctx_plan.h decides on the CPU.  Every case of
tests/golden/ctx_plan.json (tests/stubs/ctx_plan_check.cpp lists them, tests/test_ctx_plan_host.py holds the planner to them bit for bit)
of at most 8192 pixels goes through mcalf_create as a raw spec: mcalf_info must show the golden record's ndim, startind, endind,
n_cap, tile, ntiles and npix, a refused spec its code and the text of mcalf_last_error.  A two-device context must report what
its sub-context 0 -- a single-device context of the same spec -- reports.  No kernel runs but what mcalf_create launches itself."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from mcalf_amd import _lib

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "ctx_plan.json")) as _fh:
    CASES = [r for r in json.load(_fh) if r["spec"]["npix"] <= 8192]
NULL_SPEC, NULL_WL, NULL_LINES = 1, 2, 3                  # `defect` of tests/stubs/ctx_plan_check.cpp
PD = C.POINTER(C.c_double)


def _wavelengths(grid, n):
    """The grids of tests/stubs/ctx_plan_check.cpp: make_wl (the geometry does not depend on their last bits)."""
    i = np.arange(n, dtype=np.float64)
    if grid == "linear":
        return 6190.0 + 0.04 * i
    k = {"gap": np.where(i >= 300, i + 30, i), "descending": -i}.get(grid, i)
    wl = 6190.0 * np.exp(k * 2.0 / 2.99792458e5)
    return np.random.default_rng(20240611).permutation(wl) if grid == "shuffled" else wl


def _spec(s):
    """(spec, the arrays it borrows) of a golden record's `spec`."""
    n = max(int(s["npix"]), 1)
    wl, flux = np.ascontiguousarray(_wavelengths(s["grid"], n)), np.ones(n)
    err = 0.02 + 0.001 * ((np.arange(n) * 37) % 11)
    nl = max(s["nlines"], 1)
    lines = (_lib.mcalf_line * nl)(*[_lib.mcalf_line(1548.204 + 2.577 * l, 0.1899 / (l + 1), 2.643e8) for l in range(nl)])
    sp = _lib.mcalf_spec(npix=s["npix"], wl=None if s["defect"] == NULL_WL else wl.ctypes.data_as(PD), flux=flux.ctypes.data_as(PD),
                         err=err.ctypes.data_as(PD), velstep=float.fromhex(s["velstep"]), nlines=s["nlines"],
                         lines=None if s["defect"] == NULL_LINES else lines, fill=_lib.mcalf_line(250.0, 0.1899, 2.643e8),
                         ncompmax=s["ncompmax"], nfill=s["nfill"], freespecres=s["freespecres"], freecont=0,
                         specres_fixed=float.fromhex(s["specres_fixed"]), specres_max=float.fromhex(s["specres_max"]), contval_fixed=1.0,
                         conv_mode=s["conv_mode"], device=-1, asymmlike=1, asymm_n4=0.3, asymm_n5=0.1)
    return sp, (wl, flux, err, lines)


def _info(lib, ctx):
    info = _lib.mcalf_info_t()
    _lib.check(lib.mcalf_info(ctx, C.byref(info)))
    return info


def _geometry(info):
    return {f: getattr(info, f) for f in ("ndim", "startind", "endind", "n_cap", "tile", "ntiles", "npix")}


def _golden_geometry(shape):
    want = {f: shape[f] for f in ("ndim", "startind", "endind", "tile", "ntiles", "npix")}
    want["n_cap"] = shape["wide_n_cap"] if shape["wide"] else shape["n_cap"]       # (what specres_max provisions: mcalf_info)
    return want


@pytest.mark.parametrize("case", CASES, ids=[r["name"] for r in CASES])
def test_create_decides_what_the_planner_decides(case, monkeypatch):
    lib = _lib.load()
    if case["spec"]["lps_env"] >= 0:
        monkeypatch.setenv("MCALF_LINES_PER_SYNC", str(case["spec"]["lps_env"]))
    else:
        monkeypatch.delenv("MCALF_LINES_PER_SYNC", raising=False)
    sp, keep = _spec(case["spec"])
    ctx = C.c_void_p()
    rc = lib.mcalf_create(None if case["spec"]["defect"] == NULL_SPEC else C.byref(sp), C.byref(ctx))
    try:
        assert rc == case["rc"], (rc, lib.mcalf_last_error(None))
        if rc != _lib.MCALF_OK:
            assert not ctx.value and lib.mcalf_last_error(None).decode() == case["msg"]
            return
        info = _info(lib, ctx)
        assert _geometry(info) == _golden_geometry(case["shape"])
        assert info.ndevices == 1 and info.arch.startswith(b"gfx950")
    finally:
        if ctx.value:
            lib.mcalf_destroy(ctx)


@pytest.mark.parametrize("name", ["log4000", "wide972"])
def test_a_two_device_parent_reports_its_first_sub_context(name, monkeypatch):
    lib = _lib.load()
    monkeypatch.delenv("MCALF_LINES_PER_SYNC", raising=False)
    case = next(r for r in CASES if r["name"] == name)
    sp, keep = _spec(case["spec"])
    sp.device = 0                                          # (sub-context 0 of the parent below is exactly this context)
    one, two = C.c_void_p(), C.c_void_p()
    try:
        _lib.check(lib.mcalf_create(C.byref(sp), C.byref(one)))
        _lib.check(lib.mcalf_create_multi(C.byref(sp), (C.c_int32 * 2)(0, 0), 2, C.byref(two)))
        single, parent = _info(lib, one), _info(lib, two)
        assert _geometry(parent) == _geometry(single) == _golden_geometry(case["shape"])
        assert (parent.device, parent.arch) == (single.device, single.arch)
        assert parent.ndevices == 2 and list(parent.devices[:2]) == [0, 0] and single.ndevices == 1
    finally:
        for ctx in (two, one):
            if ctx.value:
                lib.mcalf_destroy(ctx)
