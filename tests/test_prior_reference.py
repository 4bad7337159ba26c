"""CPU: the numpy restatement of the Gaussian prior (tests/prior_reference.py) against the plain formula of hires_fitter.py:230,
and the restated ensemble sampler on a flat target under a Gaussian on one coordinate, which must end truncated-normal in
that coordinate and uniform in the others -- checked here for the reference alone, before the device relies on it
(tests/test_gpu_prior.py).

The restatement reorders a sum of at most 129 terms (lane partial sums, then a butterfly), each term computed as the formula
writes it: the bar is 1e-12 relative.

Flat target: test_ens_reference.py's ball, iteration count, seed and bar (2048 walkers, ndim 4, 250 iterations, KS_BAR = 2.8 /
sqrt(2048) ~ 0.0619), the Gaussian N(0.4, 0.15^2) on coordinate 1 of the unit cube, where both faces cut it (2.7 sigma below,
4 sigma above: 0.4 % of the mass lies outside).  Distances per coordinate at that count (seed 3), coordinate 1 against the
truncated normal by math.erf, the others against U(0, 1):
    stretch 0.0134 0.0198 0.0239 0.0203 (acceptance 0.44)      DE 0.0176 0.0147 0.0181 0.0131 (acceptance 0.25)"""
import numpy as np
import pytest

import prior_reference as pr
from test_ens_reference import FLAT_ITERS, FLAT_SEED, KS_BAR, flat_start, ks_distances

MU, SIGMA = 0.4, 0.15


def _problem(ndim, which, rng):
    lo = rng.uniform(-3.0, 3.0, ndim)
    hi = lo + rng.uniform(0.5, 4.0, ndim)
    mu = rng.uniform(lo, hi)
    sigma = np.zeros(ndim)
    sigma[which] = rng.uniform(0.05, 2.0, len(which))
    return lo, hi, mu, sigma, np.log(2.0 * np.pi * sigma ** 2, where=sigma > 0.0, out=np.zeros(ndim))


@pytest.mark.parametrize("ndim", [4, 65, 129])
def test_the_restatement_is_the_plain_formula_reordered(ndim):
    rng = np.random.default_rng(ndim)
    for which in ([1], [ndim - 1], [k for k in (63, 64) if k < ndim], [k for k in range(ndim) if k != 2], []):
        lo, hi, mu, sigma, c = _problem(ndim, which, rng)
        U = rng.random((65, ndim))
        U[3, ndim - 1], U[5, 0], U[7, ndim // 2], U[9, 1], U[11, 0] = 1.0, 0.0, np.nan, 1.0 + 2.0 ** -52, -1e-300
        theta = U * (hi - lo) + lo
        want = pr.plain(theta, lo, hi, mu, sigma)
        want[[7, 9, 11]] = -np.inf                               # (the cube test: NaN, just above 1, just below 0)
        got = pr.lnprior(U, lo, hi, mu, sigma, c, True, int_slot=2)
        assert np.isneginf(got[[7, 9, 11]]).all() and np.isfinite(np.delete(got, [7, 9, 11])).all()
        fin = np.isfinite(want)
        assert (np.isfinite(got) == fin).all()
        assert (np.abs(got[fin] - want[fin]) <= 1e-12 * np.maximum(np.abs(want[fin]), 1.0)).all()
        if not which:
            assert not got[fin].any() and not np.signbit(got[fin]).any()     # an exact +0
            assert pr.lnprior(U, lo, hi, None, None, None, True).tobytes() == got.tobytes()
        # parameter rows: the same terms, the box test on theta itself
        inside = theta[fin]
        assert pr.lnprior(inside, lo, hi, mu, sigma, c, False).tobytes() == got[fin].tobytes()
        out = inside.copy()
        out[0, 0], out[1, ndim - 1], out[2, 1] = np.nextafter(lo[0], -np.inf), np.nextafter(hi[-1], np.inf), np.nan
        face = inside.copy()
        face[0, 0], face[1, ndim - 1] = lo[0], hi[-1]
        assert np.isneginf(pr.lnprior(out, lo, hi, mu, sigma, c, False)[:3]).all()
        assert np.isfinite(pr.lnprior(face, lo, hi, mu, sigma, c, False)).all()


def test_a_lane_adds_in_index_order_and_the_butterfly_folds_the_lanes():
    """Three terms of very different size on coordinates 0, 64 and 128 (one lane) and one on 1 (its neighbour): the sum is
    ((t0 + t64) + t128) + t1, not another order."""
    ndim = 129
    lo, hi = np.zeros(ndim), np.ones(ndim)
    sigma, mu = np.zeros(ndim), np.zeros(ndim)
    sigma[[0, 64, 128, 1]] = [1e-8, 1.0, 1e-3, 0.5]
    c = np.zeros(ndim)                                           # (any stored constants will do)
    U = np.full((1, ndim), 0.3)
    t = [-0.5 * ((0.3 / s) * (0.3 / s) + 0.0) for s in sigma[[0, 64, 128, 1]]]
    assert pr.lnprior(U, lo, hi, mu, sigma, c, False)[0] == ((0.0 + t[0]) + t[1] + t[2]) + t[3]


@pytest.mark.parametrize("move", [pr.STRETCH, pr.DE])
def test_a_flat_target_under_a_gaussian_ends_truncated_normal(move):
    ndim = 4
    lo, hi = np.zeros(ndim), np.ones(ndim)
    mu, sigma = np.zeros(ndim), np.zeros(ndim)
    mu[1], sigma[1] = MU, SIGMA
    c = np.log(2.0 * np.pi * sigma ** 2, where=sigma > 0.0, out=np.zeros(ndim))
    lnp = lambda U: pr.lnprior(U, lo, hi, mu, sigma, c, True)
    U, L, status, naccept, CU, CL, PR = pr.ensemble(lambda Y: np.zeros(Y.shape[0]), lnp, flat_start(ndim), FLAT_ITERS[ndim], FLAT_ITERS[ndim], move,
                                                    seed=FLAT_SEED)
    assert (status == 0).all() and ((U >= 0.0) & (U <= 1.0)).all() and not L.any()
    assert PR.tobytes() == lnp(U).tobytes() and np.array_equal(CU[0], U)
    d = ks_distances(U)
    d[1] = pr.ks_against(U[:, 1], lambda x: pr.truncated_normal_cdf(x, MU, SIGMA))
    print(f"move {move}: KS distances {np.round(d, 4)} (bar {KS_BAR:.4f}), acceptance {naccept.mean() / FLAT_ITERS[ndim]:.3f}")
    assert ks_distances(U)[1] > 2.0 * KS_BAR                     # coordinate 1 is not uniform any more
    assert (d < KS_BAR).all()


def test_without_a_gaussian_the_restated_drivers_are_the_originals():
    """lnprior 0 everywhere: q + (0 - 0) is q, so the runs are ens_reference's and pt_reference's bit for bit."""
    import ens_reference as er
    import pt_reference as pt
    rng = np.random.default_rng(5)
    logl = lambda U: -0.5 * (((U - 0.5) / 0.1) ** 2).sum(axis=1)
    zero = lambda U: np.zeros(U.shape[0])
    for move in (pr.STRETCH, pr.DE):
        U0 = 0.5 + 0.1 * (2.0 * rng.random((3, 6, 5)) - 1.0)
        a = er.ensemble(logl, U0[0], 9, 2, move, seed=3, first_iter=4)
        b = pr.ensemble(logl, zero, U0[0], 9, 2, move, seed=3, first_iter=4)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b[:6]))
        a = pt.tempered(logl, U0, [1.0, 0.3, 0.0], 9, 2, 1, move, seed=3, first_iter=4, chain_temps=2)
        b = pr.tempered(logl, zero, U0, [1.0, 0.3, 0.0], 9, 2, 1, move, seed=3, first_iter=4, chain_temps=2)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b[:7])) and a[4].sum() > 0
