"""What the tests of voigt_grad.h share: the mpmath fixture (tests/golden/voigt_grad_reference.npz), the device probe
(tests/stubs/voigt_grad_probe.hip) compiled with the flags of grad_kernels.o, and the bars of tests/test_gpu_voigt_grad.py."""
import ctypes as C
import importlib
import importlib.util
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PROBE_SRC = os.path.join(HERE, "stubs", "voigt_grad_probe.hip")
PROBE_NAMES = ("wr", "wi", "dr", "di", "e", "wr2", "dr2", "e_2", "d2", "e2", "e3")     # the probe's eleven columns
REF_NAMES = ("wr", "wi", "dr", "di", "e", "d2", "e2", "e3", "ei", "e2i", "e3i")       # the fixture's columns (VG_NAMES)
EPS = 2.0 ** -53
R2_SEAM = 64.0                                                                         # kAsymR2

_built = {}


def generator():
    """tests/golden/make_derived_goldens.py as a module (its __main__ part does not run)."""
    spec = importlib.util.spec_from_file_location("make_derived_goldens", os.path.join(HERE, "golden", "make_derived_goldens.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Fixture:
    """x, y and the exact values per point (ref, by the names of REF_NAMES; read-only), the region of each point and, for the core, the magnitudes M_q
    of the terms that the algebraic identities add up, from the REFERENCE values:
        M_w' = 2|z||w| + 2/sqrt(pi),  M_e = |w| + |z| M_w',  M_d2 = 2 M_e,  M_e2 = 2 M_w' + |z| M_d2,  M_e3 = 2 M_e + |z| M_e2."""

    def __init__(self):
        with np.load(os.path.join(HERE, "golden", "voigt_grad_reference.npz")) as f:
            self.x, self.y, ref, self.dps = f["x"], f["y"], f["ref"], f["dps"]
        self.n = self.x.size
        self.ref = dict(zip(REF_NAMES, ref.T))
        # (the generator made sure that no point's side of the seam depends on how x*x + y*y is contracted)
        self.series = self.x * self.x + self.y * self.y >= R2_SEAM
        self.core = ~self.series
        az = np.hypot(self.x, self.y)
        self.absw = np.hypot(self.ref["wr"], self.ref["wi"])
        self.absdw = np.hypot(self.ref["dr"], self.ref["di"])
        m_dw = 2.0 * az * self.absw + 2.0 / np.sqrt(np.pi)
        m_e = self.absw + az * m_dw
        m_e2 = 2.0 * m_dw + az * 2.0 * m_e
        self.M = {"e": m_e, "d2": 2.0 * m_e, "e2": m_e2, "e3": 2.0 * m_e + az * m_e2}
        # |q| of the COMPLEX quantity that each returned real (or imaginary) part belongs to
        abse = np.hypot(self.ref["e"], self.ref["ei"])
        self.cabs = {"wr": self.absw, "wi": self.absw, "dr": self.absdw, "di": self.absdw, "e": abse, "d2": 2.0 * abse,
                     "e2": np.hypot(self.ref["e2"], self.ref["e2i"]), "e3": np.hypot(self.ref["e3"], self.ref["e3i"])}
        for a in (self.x, self.y, self.series, self.core, *self.ref.values(), *self.M.values(), *self.cabs.values()):
            a.setflags(write=False)


def compile_probe(outdir, compile_only=False):
    """hipcc for gfx950 with build.KERNEL_FLAGS (what grad_kernels.o is built with: same contraction, same optimisation
    level); one build per session.  compile_only stops at the object file."""
    bld = importlib.import_module("mc-alf_amd.build")
    key = "obj" if compile_only else "lib"
    if key not in _built:
        out = os.path.join(str(outdir), "voigt_grad_probe.o" if compile_only else "libvoigt_grad_probe.so")
        cmd = [bld._hipcc()] + bld.KERNEL_FLAGS + ["-I" + bld.CSRC] + (["-c"] if compile_only else ["-shared"]) + [PROBE_SRC, "-o", out]
        res = subprocess.run(cmd, capture_output=True, text=True)
        assert res.returncode == 0, "hipcc failed (%s):\n%s%s" % (" ".join(cmd), res.stdout, res.stderr)
        _built[key] = out
    return _built[key]


def load_probe(outdir):
    lib = C.CDLL(compile_probe(outdir))
    pd = C.POINTER(C.c_double)
    lib.voigt_grad_probe.restype = C.c_int
    lib.voigt_grad_probe.argtypes = [pd, pd, C.c_long, pd]
    return lib


def run_probe(lib, x, y):
    """The probe's eleven columns at the points (x, y), by name."""
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    out = np.full((x.size, len(PROBE_NAMES)), np.nan)
    pd = C.POINTER(C.c_double)
    rc = lib.voigt_grad_probe(x.ctypes.data_as(pd), y.ctypes.data_as(pd), x.size, out.ctypes.data_as(pd))
    assert rc == 0, "HIP error %d" % rc
    return dict(zip(PROBE_NAMES, np.ascontiguousarray(out.T)))


def worst(err, bar, mask, fx, what):
    """max err/bar over mask, printed (pytest -s) with the point it is at."""
    ratio = np.where(mask, err / bar, 0.0)
    bad = mask & ~(err <= bar)                                     # a NaN error is bad
    i = int(np.argmax(np.where(bad, np.inf, ratio)))
    print("%-34s worst err/bar %.3g at x = %r, y = %r" % (what, ratio[i] if not bad[i] else np.inf, fx.x[i], fx.y[i]))
    return bad
