"""faddeeva_dw and faddeeva_d2w (mc-alf_amd/csrc/voigt_grad.h) ON THE DEVICE against mpmath: every output of both functions at
the points of tests/golden/voigt_grad_reference.npz (Gaussian core, Lorentzian wing, both sides of the |z| = 8 seam and of
every truncation bracket of asym_terms, each at small and large a), through the probe tests/stubs/voigt_grad_probe.hip, which
is compiled with the flags of grad_kernels.o.  One launch serves the module.

Bars (none comes from the code under test), eps = 2^-53:
  series region, r^2 >= 64   |dq| <= 1e-14 |q| + 1e-22 for every output.  1e-14: at most 26 complex multiply-adds and the
                             prefactor, about a hundred roundings of 1.1e-16.  1e-22: the series drops exp(-x^2) <= 1.6e-28
                             times its polynomial factors, which shows at y <= 1e-9 only.  At y = 0 the real parts ARE that
                             dropped term (the device returns 0 for wr, dr, e, d2, e2, e3), so there only the floor judges
                             them and the relative bar judges wi and di.
  core, r^2 < 64             |dw| <= 5e-15 |w| and |dw'| <= 2e-13 |w'| as complex numbers (the header's claims);
                             |dq| <= 16 eps M_q for e, d2, e2, e3, M_q the sum of the magnitudes that the algebraic identity of
                             q adds up (voigt_grad_probe.Fixture), from the reference values.
"""
import numpy as np
import pytest

import voigt_grad_probe as vgp

pytestmark = pytest.mark.gpu

REF_OF = {"wr": "wr", "wi": "wi", "dr": "dr", "di": "di", "e": "e", "wr2": "wr", "dr2": "dr", "e_2": "e", "d2": "d2", "e2": "e2",
          "e3": "e3"}
SEAM_A = (1e-4, 3e-4, 1e-3, 2.0 ** -8)


@pytest.fixture(scope="module")
def fx():
    return vgp.Fixture()


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    return vgp.load_probe(tmp_path_factory.mktemp("voigt_grad_probe"))


@pytest.fixture(scope="module")
def dev(probe, fx):
    out = vgp.run_probe(probe, fx.x, fx.y)
    for a in out.values():
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name", list(REF_OF))
def test_series_region_to_1e14_of_the_value(fx, dev, name):
    """|dq| <= 1e-14 |q| + 1e-22, q the returned real (or imaginary) part itself.

    The hard points are the zeros of a real part: Re (z w)' and Re w'' ~ Im z^3 vanish on x = y/sqrt 3 (5.77 at y = 10),
    Re (z^2 w)'' a little further out, and the fixture's x grid has points within 2 % of them, where the value is several
    hundred times smaller than the complex magnitude.  With the leading term i/(sqrt(pi) z^3) summed as a complex term the
    device missed this bar there (e 5.8e-14 and 2.3e-14 at x = 5.847 and 5.899, d2 1.6e-14, e3 2.3e-14 and 1.3e-14 at x = 6.050
    and 6.099); voigt_grad.h: asym_lead forms it in real arithmetic for that reason."""
    assert np.count_nonzero(fx.series) > 1500
    q = REF_OF[name]
    err = np.abs(dev[name] - fx.ref[q])
    bad = vgp.worst(err, 1e-14 * np.abs(fx.ref[q]) + 1e-22, fx.series, fx, "series %s / value" % name)
    for i in np.flatnonzero(bad):
        print("   miss: x = %r, y = %r: |dq|/|q| = %.3g, |dq|/|Q| = %.3g" % (fx.x[i], fx.y[i], err[i] / abs(fx.ref[q][i]),
                                                                               err[i] / fx.cabs[q][i]))
    assert not bad.any(), (name, int(bad.sum()))
    if name not in ("wi", "di"):                                    # y = 0: what the floor alone judged is exactly 0
        assert np.all(dev[name][fx.series & (fx.y == 0.0)] == 0.0)


def test_series_region_to_1e14_of_the_complex_magnitude(fx, dev):
    """The same hundred roundings, measured against |Q| of the complex quantity whose real (or imaginary) part is returned:
    |dq| <= 1e-14 |Q| + 1e-22.  The test above implies it (|q| <= |Q|); it is kept because it tells the two kinds of failure
    apart: a lost or wrong term fails here too, roundings next to a zero of a real part fail only above."""
    bad = {}
    for name, q in REF_OF.items():
        err = np.abs(dev[name] - fx.ref[q])
        b = vgp.worst(err, 1e-14 * fx.cabs[q] + 1e-22, fx.series, fx, "series %s / complex magnitude" % name)
        if b.any():
            bad[name] = int(b.sum())
    assert not bad, bad


def test_core_against_the_conditioned_bars(fx, dev):
    assert np.count_nonzero(fx.core) > 1500
    bad = {}
    dw = np.hypot(dev["wr"] - fx.ref["wr"], dev["wi"] - fx.ref["wi"])
    ddw = np.hypot(dev["dr"] - fx.ref["dr"], dev["di"] - fx.ref["di"])
    checks = [("w", dw, 5e-15 * fx.absw), ("w'", ddw, 2e-13 * fx.absdw)]
    for name in ("e", "e_2", "d2", "e2", "e3"):
        q = REF_OF[name]
        checks.append((name, np.abs(dev[name] - fx.ref[q]), 16 * vgp.EPS * fx.M[q]))
    for name, err, bar in checks:
        b = vgp.worst(err, bar, fx.core, fx, "core %s" % name)
        if b.any():
            bad[name] = int(b.sum())
    assert not bad, bad


def test_the_two_functions_agree(fx, dev):
    for a, b in (("wr", "wr2"), ("dr", "dr2"), ("e", "e_2")):
        # core: faddeeva_d2w calls faddeeva_dw
        assert np.array_equal(dev[a][fx.core], dev[b][fx.core]), a
        # series: the same sums, two terms longer
        assert np.all(np.abs(dev[a] - dev[b])[fx.series] <= 1e-14 * np.abs(dev[a][fx.series])), a


def test_symmetry_in_x_is_exact(fx, dev):
    index = {p: i for i, p in enumerate(zip(fx.x.tolist(), fx.y.tolist()))}
    neg = np.flatnonzero(fx.x < 0)
    pos = np.array([index[(-fx.x[i], fx.y[i])] for i in neg])
    assert neg.size >= 300 and fx.core[neg].any() and fx.series[neg].any()
    for name in ("wr", "e", "d2", "e3", "di", "wr2", "e_2"):         # even
        assert np.array_equal(dev[name][neg], dev[name][pos]), name
    for name in ("dr", "e2", "wi", "dr2"):                           # odd
        assert np.array_equal(dev[name][neg], -dev[name][pos]), name


def test_limits_and_nan(fx, dev, probe):
    x0 = fx.x == 0.0
    assert np.count_nonzero(x0) >= 13 and fx.series[x0].any() and fx.core[x0].any()
    for name in ("wi", "dr", "dr2"):
        assert np.all(dev[name][x0] == 0.0), name
    o = np.flatnonzero(x0 & (fx.y == 0.0))
    assert o.size == 1 and abs(dev["wr"][o[0]] - 1.0) <= 5e-15 and abs(dev["wr2"][o[0]] - 1.0) <= 5e-15
    nan = np.nan
    xs = np.array([nan, 1.0, nan, 100.0, nan, nan, 7.9999])
    ys = np.array([0.5, nan, nan, nan, 100.0, 0.0, nan])
    out = vgp.run_probe(probe, xs, ys)
    for name, v in out.items():
        assert np.all(np.isnan(v)), name


def test_what_a_pixel_sees_just_inside_the_seam(fx, dev):
    """PURE relative errors on the core points with 6 <= |x| < 8 at the a of Ly-alpha and CIV lines.  The algebraic forms
    cancel there: e, d2, e2 and e3 inherit 2|z|^2 d(Re w) and its multiples, with d(Re w) ~ 1e-17 absolute from the rational
    expansion, while the quantities themselves fall like a/|z|^2.  The first-order three are held to the project's derivative
    bar, 1e-7; the second-order three are printed and not asserted against it (as documented the algorithm cannot meet it just
    below |z| = 8 at a = 1e-4; DESIGN section 3.8 carries the table) -- the conditioned bars of the core test hold for them."""
    worst = {}
    for a in SEAM_A:
        m = fx.core & (fx.y == a) & (np.abs(fx.x) >= 6.0) & (np.abs(fx.x) < 8.0)
        assert np.count_nonzero(m) >= 80
        for name in ("wr", "dr", "e", "d2", "e2", "e3"):
            rel = np.abs(dev[name][m] - fx.ref[name][m]) / np.abs(fx.ref[name][m])
            worst[(name, a)] = float(rel.max())
    print("\nworst pure relative error, core points with 6 <= |x| < 8")
    print("%-10s" % "a" + "".join("%11s" % n for n in ("wr", "dr", "e", "d2", "e2", "e3")))
    for a in SEAM_A:
        print("%-10.4g" % a + "".join("%11.2e" % worst[(n, a)] for n in ("wr", "dr", "e", "d2", "e2", "e3")))
    for name in ("wr", "dr", "e"):
        for a in SEAM_A:
            assert worst[(name, a)] <= 1e-7, (name, a, worst[(name, a)])
