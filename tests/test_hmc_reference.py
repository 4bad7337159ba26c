"""CPU: the numpy restatement of Hamiltonian Monte Carlo (tests/hmc_reference.py) and the host driver `hmc.sample_with` -- the
polar normals' distribution, the integrator's reversibility with reflections in play, the moments of a correlated Gaussian
truncated to the cube with one frozen coordinate, and the driver's adaptation, its frozen kept run and its determinism."""
import math

import numpy as np
import pytest

import hmc_reference as hr
from mcalf_amd import ensemble, hmc

# The bar of test_ens_reference.KS_BAR, 2.8 / sqrt(n), at this file's sample count.
NDRAWS = 200000
KS_BAR = 2.8 / np.sqrt(NDRAWS)


def test_the_polar_normals_are_standard_normal():
    """2e5 draws (400 walkers x 500 coordinates of one iteration): mean within 4 / sqrt(n), variance within 4 sqrt(2 / n),
    Kolmogorov-Smirnov distance to the normal distribution function under 2.8 / sqrt(n)."""
    r = hr.normals(7, np.arange(400) + 2 ** 40, np.arange(500), seed=2 ** 63 + 5).reshape(-1)
    assert r.size == NDRAWS and np.isfinite(r).all() and (r != 0.0).all()
    x = np.sort(r)
    F = np.array([0.5 * (1.0 + math.erf(v / math.sqrt(2.0))) for v in x])
    grid = np.arange(1, NDRAWS + 1) / NDRAWS
    d = max((grid - F).max(), (F - (grid - 1.0 / NDRAWS)).max())
    print(f"mean {r.mean():.5f}, variance {r.var():.5f}, KS distance {d:.5f} (bar {KS_BAR:.5f})")
    assert abs(r.mean()) < 4.0 / np.sqrt(NDRAWS) and abs(r.var() - 1.0) < 4.0 * np.sqrt(2.0 / NDRAWS)
    assert d < KS_BAR
    # other ids, another iteration, another seed: other draws; the same arguments: the same bytes
    a = hr.normals(7, [3, 4], [0, 1, 2], seed=1)
    assert a.tobytes() == hr.normals(7, [3, 4], [0, 1, 2], seed=1).tobytes()
    assert a[0].tolist() != a[1].tolist() and a.tolist() != hr.normals(8, [3, 4], [0, 1, 2], seed=1).tolist()
    assert a.tolist() != hr.normals(7, [3, 4], [0, 1, 2], seed=2).tolist()
    assert a[:, 1:].tobytes() == hr.normals(7, [3, 4], [1, 2], seed=1).tobytes()          # a coordinate's draw is its own


# ---- a correlated Gaussian truncated to the cube ----------------------------------------------------------------------------------

MU = np.array([0.08, 0.5, 0.5, 0.93, 0.4, 0.5])
SD = np.array([0.10, 0.08, 0.06, 0.10, 0.05, 1.0])
BLOCKS = (((0, 1), 0.6), ((2, 3), -0.5), ((4,), 0.0))          # correlated pairs, so that the quadrature factorises
SLOT = 5                                                        # the frozen coordinate (the ncomp slot of the problem)


def _target():
    """(Problem, grad) of the six-dimensional target: coordinates 0 and 3 have their means 0.8 and 0.7 standard deviations from
    a wall, so the truncation carries a fifth of their untruncated mass and trajectories reflect; coordinate 5 is the frozen
    slot and does not enter the density."""
    cov = np.zeros((6, 6))
    for idx, rho in BLOCKS:
        for i in idx:
            for j in idx:
                cov[i, j] = (1.0 if i == j else rho) * SD[i] * SD[j]
    prec = np.zeros((6, 6))
    prec[:5, :5] = np.linalg.inv(cov[:5, :5])

    def grad(theta):
        d = theta - MU
        Pd = d @ prec
        return -0.5 * np.einsum("ij,ij->i", d, Pd), -Pd
    return hr.Problem(np.zeros(6), np.ones(6), SLOT, int_ncomp=False), grad, cov


def _quadrature(cov, m=1200):
    """Means and variances of coordinates 0 .. 4 of the truncated target by the midpoint rule, block by block."""
    mean, var = np.zeros(5), np.zeros(5)
    x = (np.arange(m) + 0.5) / m
    for idx, _ in BLOCKS:
        idx = list(idx)
        pts = np.stack(np.meshgrid(*([x] * len(idx)), indexing="ij"), axis=-1).reshape(-1, len(idx))
        d = pts - MU[idx]
        w = np.exp(-0.5 * np.einsum("ij,jk,ik->i", d, np.linalg.inv(cov[np.ix_(idx, idx)]), d))
        w /= w.sum()
        mean[idx] = w @ pts
        var[idx] = w @ (pts - mean[idx]) ** 2
    return mean, var


def test_the_integrator_is_reversible_with_reflections_in_play():
    """nleap steps, the momentum negated, nleap steps again: back at the start within 1e-12, position and momentum, for 64
    walkers of which some reflect (asserted on the trace) and none dies."""
    prob, grad, _ = _target()
    rng = np.random.default_rng(0)
    x = np.clip(MU + SD * rng.standard_normal((64, 6)) * 0.5, 0.01, 0.99)
    free = np.arange(5)
    r = np.zeros((64, 6))
    r[:, free] = hr.normals(0, np.arange(64), free, seed=1)
    a = 0.25 * np.where(np.arange(6) == SLOT, 0.0, SD) * np.ones((64, 1))
    th = prob.theta(x)
    gx = prob.cube_grad(grad(th)[1], th)
    trace = []
    none = np.zeros(64, dtype=bool)
    y, r1, gy, _, parked = hr.leapfrog(prob, grad, x, gx, r, a, 10, free, none, trace)
    assert sum(t[3] for t in trace if t[0] == "reflect") >= 5 and not parked.any()
    assert np.abs(y - x)[:, free].min(axis=0).min() > 0.0 and (y[:, SLOT] == x[:, SLOT]).all()
    back, r2, _, _, parked = hr.leapfrog(prob, grad, y, gy, -r1, a, 10, free, none)
    assert not parked.any()
    print(f"largest return error: position {np.abs(back - x).max():.2e}, momentum {np.abs(-r2 - r).max():.2e}")
    assert np.abs(back - x).max() < 1e-12 and np.abs(-r2 - r).max() < 1e-12


SAMPLER_SEED = 5
BURN, KEPT, NBATCH = 200, 1500, 20


def test_a_truncated_correlated_gaussian_has_its_means_and_variances():
    """64 walkers from the cube's centre, 200 iterations forgotten, 1500 kept, 20 batches of 75 iterations (a trajectory of 6
    steps of 0.4 standard deviations decorrelates a walker within a few iterations).  Every mean and variance of the five
    moving coordinates within 4 batch-means standard errors of the quadrature; the frozen coordinate keeps its bytes."""
    prob, grad, cov = _target()
    qmean, qvar = _quadrature(cov)
    assert qmean[0] > MU[0] + 0.02 and qmean[3] < MU[3] - 0.02        # the walls matter
    U0 = np.clip(0.5 + 0.1 * (2.0 * np.random.default_rng(SAMPLER_SEED).random((64, 6)) - 1.0), 0.0, 1.0)
    trace = []
    U, L, status, naccept, ndead, CU, CL = hr.hmc(prob, grad, U0, BURN + KEPT, 0.4, 6, scale=SD, seed=SAMPLER_SEED, trace=trace)
    assert (status == 0).all() and ((CU >= 0.0) & (CU <= 1.0)).all()
    assert (CU[:, :, SLOT] == U0[:, SLOT]).all()
    assert any(t[0] == "reflect" for t in trace)
    x = CU[BURN:, :, :5]
    print(f"acceptance {naccept.mean() / (BURN + KEPT):.3f}, dead trajectories {ndead.sum()}")
    for name, series, want in (("mean", x.mean(axis=1), qmean), ("variance", ((x - qmean) ** 2).mean(axis=1), qvar)):
        se = ensemble.batch_means_se(series, NBATCH)
        dev = (series.mean(axis=0) - want) / se
        print(f"{name} {series.mean(axis=0)}, quadrature {want}: deviations {np.round(dev, 2)} standard errors")
        assert (np.abs(dev) <= 4.0).all()


def test_ten_iterations_are_four_and_then_six_and_a_walker_is_its_own():
    prob, grad, _ = _target()
    U0 = np.clip(MU + 0.3 * SD * np.random.default_rng(2).standard_normal((7, 6)), 0.0, 1.0)
    U0[3, 1] = 1.5                                                 # a refused start among them
    whole = hr.hmc(prob, grad, U0, 10, 0.5, 3, scale=SD, thin=2, seed=9)
    assert whole[2].tolist() == [0, 0, 0, -1, 0, 0, 0] and whole[0][3].tobytes() == U0[3].tobytes() and whole[3][3] == 0
    a = hr.hmc(prob, grad, U0, 4, 0.5, 3, scale=SD, thin=2, seed=9)
    b = hr.hmc(prob, grad, a[0], 6, 0.5, 3, scale=SD, thin=2, seed=9, first_iter=4)
    assert whole[0].tobytes() == b[0].tobytes() and whole[1].tobytes() == b[1].tobytes()
    assert np.array_equal(whole[3], a[3] + b[3]) and whole[5].tobytes() == np.concatenate([a[5], b[5]]).tobytes()
    pick = np.array([5, 0, 2])
    part = hr.hmc(prob, grad, U0[pick], 10, 0.5, 3, scale=SD, thin=2, seed=9, wid=pick)
    assert part[0].tobytes() == whole[0][pick].tobytes() and np.array_equal(part[3], whole[3][pick])
    assert 0 < whole[3].sum() < 60


# ---- the driver -------------------------------------------------------------------------------------------------------------------

def _driver(eps, seed=3, record=None):
    prob, grad, _ = _target()
    inner = hr.advance_with(prob, grad, nleap=4)

    def advance(U0, nsteps, eps, scale, **kw):
        if record is not None:
            record.append((nsteps, eps, np.array(scale), kw["first_iter"], kw["chain"]))
        return inner(U0, nsteps, eps, scale, **kw)
    return hmc.sample_with(lambda U: (prob.theta(U), grad(prob.theta(U))[0]), advance, 6, 32, 60, burn=150, thin=2, start=np.clip(MU, 0.1, 0.9),
                           ball=0.05, seed=seed, eps=eps, target=0.8, windows=5)


@pytest.mark.parametrize("eps0", [4.0, 0.02])
def test_the_driver_adapts_eps_freezes_it_and_is_deterministic(eps0):
    """From a step far too long (acceptance near 0) and from one far too short (acceptance near 1): eps moves in the right
    direction in every window, the last window's acceptance is closer to the target than the first one's, the kept run is one
    call under the eps and the scale the burn-in ended with, and a second run gives the same bytes."""
    calls = []
    res = _driver(eps0, record=calls)
    assert [c[0] for c in calls] == [30] * 5 + [60] and [c[3] for c in calls] == [0, 30, 60, 90, 120, 150]
    assert [c[4] for c in calls] == [False] * 5 + [True]
    acc, eps = res.window_accept, [c[1] for c in calls]
    print(f"eps0 {eps0}: window acceptance {np.round(acc, 3)}, eps {np.round(eps, 4)}")
    assert eps[0] == eps0 and res.window_eps.tolist() == eps[:5]
    for k in range(5):                                             # towards the target: down when too few are accepted, up when too many
        assert (eps[k + 1] < eps[k]) == (acc[k] < 0.8)
    assert abs(acc[-1] - 0.8) < abs(acc[0] - 0.8)
    assert (eps[-1] < eps0) if eps0 > 1.0 else (eps[-1] > eps0)
    assert res.eps == eps[-1] and res.scale.tobytes() == calls[-1][2].tobytes()      # frozen: what the kept run ran under
    assert res.scale[SLOT] == calls[0][2][SLOT] or res.scale[SLOT] > 0.0
    assert res.cube.shape == (30, 32, 6) and res.logL.shape == (30, 32) and res.ndead.shape == (32,)
    assert (res.cube[:, :, SLOT] == res.last[:, SLOT]).all() and np.array_equal(res.last, res.cube[-1])
    again = _driver(eps0)
    for name in ("cube", "theta", "logL", "accept_frac", "last", "scale", "window_accept", "window_eps", "ndead"):
        assert getattr(res, name).tobytes() == getattr(again, name).tobytes(), name
    assert res.eps == again.eps
    assert _driver(eps0, seed=4).cube.tobytes() != res.cube.tobytes()
