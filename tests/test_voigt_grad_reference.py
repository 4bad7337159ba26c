"""The mpmath fixture of the Voigt derivatives (tests/golden/voigt_grad_reference.npz) is what its generator says it is, and
the device probe of voigt_grad.h compiles for gfx950 (no GPU needed: a header edit that breaks it shows up here)."""
import numpy as np

import voigt_grad_probe as vgp


def test_fixture_round_trips_through_mpmath():
    gen = vgp.generator()
    fx = vgp.Fixture()
    assert int(fx.dps[0]) == gen.VG_DPS >= 80 and tuple(gen.VG_NAMES) == vgp.REF_NAMES
    X, Y = gen.voigt_grad_points()
    assert np.array_equal(X, fx.x) and np.array_equal(Y, fx.y)
    assert np.array_equal(np.signbit(X), np.signbit(fx.x))
    for i in np.random.default_rng(20240611).choice(fx.n, 200, replace=False):
        got = gen.voigt_grad_reference(float(fx.x[i]), float(fx.y[i]))
        want = [float(fx.ref[k][i]) for k in gen.VG_NAMES]
        assert got == want, (fx.x[i], fx.y[i], got, want)


def test_fixture_covers_what_it_names():
    fx = vgp.Fixture()
    r2 = fx.x * fx.x + fx.y * fx.y
    assert 3500 <= fx.n <= 7000
    assert set(np.unique(fx.y)) >= {0.0, 1e-9, 1e-6, 1e-4, 3e-4, 1e-3, 2.0 ** -8, 0.05, 0.5, 3.0, 10.0, 30.0, 8.0}
    for T in (64.0, 225.0, 900.0, 1e4, 1e6):                       # both sides of every bracket edge, at small and large a
        for sel in (fx.y <= 1e-3, fx.y >= 0.5):
            assert np.any(sel & (r2 < T) & (r2 >= T * (1 - 1e-14))) and np.any(sel & (r2 >= T) & (r2 <= T * (1 + 1e-14)))
    assert np.any(r2 == 64.0) and np.abs(fx.x).max() == 1e8
    assert np.any((fx.x == 7.9999) & fx.core) and np.any((fx.x == 0.0) & (fx.y == 0.0))
    assert np.count_nonzero(fx.x < 0) >= 300
    pts = set(zip(fx.x.tolist(), fx.y.tolist()))
    assert all((-x, y) in pts for x, y in pts if x < 0)            # every negative x has its mirror


def test_probe_compiles_for_gfx950(tmp_path):
    obj = vgp.compile_probe(tmp_path, compile_only=True)
    with open(obj, "rb") as fh:
        assert fh.read(4) == b"\x7fELF"
