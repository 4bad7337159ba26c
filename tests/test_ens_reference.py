"""CPU: the numpy restatement of the ensemble sampler (tests/ens_reference.py) -- its logarithm against numpy's, its random
words against numpy's own Philox bit generator, the uniformity of a flat target's walkers, the moments of a correlated
Gaussian, which walkers a half-step reads, and the continuation.

Flat target (logL = 0, 2048 walkers from the ball of half-width FLAT_BALL = 0.25 around the cube's centre, whose own
Kolmogorov-Smirnov distance from U(0, 1) is 0.25): the iteration counts FLAT_ITERS were chosen from runs of this file's
reference in steps of 250 (ndim 4) and 500 (ndim 65) iterations up to 3000, as a count from which every later one stayed below
the bar 2.8 / sqrt(2048) ~ 0.0619 with some room.  Largest distance over the coordinates at that count (seed 3):
    ndim 4,  250 iterations:   stretch 0.0220, DE 0.0271   (250 .. 3000 iterations: 0.015 .. 0.034, no trend)
    ndim 65, 2500 iterations:  stretch 0.0559, DE 0.0330   (stretch: 0.0651, 0.0632, 0.0602, 0.0571, 0.0559, 0.0537 after
                               500, 1000, ..., 3000 iterations; DE: 0.0473, 0.0436, 0.0418, 0.0379, 0.0330, 0.0317.  Acceptance
                               in the full cube is 2 % to 3 %: every one of the 65 coordinates of a proposal has to stay inside)
tests/test_gpu_ens.py runs the same counts on the device."""
import numpy as np
import pytest

import ens_reference as er
from mcalf_amd import ensemble

FLAT_BALL = 0.25
FLAT_ITERS = {4: 250, 65: 2500}
FLAT_SEED = 3
KS_BAR = 2.8 / np.sqrt(2048)


def ks_distances(U):
    """Each coordinate's Kolmogorov-Smirnov distance of the rows of U from U(0, 1)."""
    n = U.shape[0]
    grid = np.arange(1, n + 1) / n
    x = np.sort(U, axis=0)
    return np.maximum((grid[:, None] - x).max(axis=0), (x - (grid[:, None] - 1.0 / n)).max(axis=0))


def flat_start(ndim, n=2048):
    return np.clip(0.5 + FLAT_BALL * (2.0 * np.random.default_rng(ndim).random((n, ndim)) - 1.0), 0.0, 1.0)


def test_the_logarithm_is_within_1e_13_of_numpys():
    rng = np.random.default_rng(0)
    edge = [2.0 ** -53, 1.0, 0.25, 4.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0), er.SQRT2, np.nextafter(er.SQRT2, 2.0), 0.5, 2.0]
    x = np.concatenate([np.exp(rng.uniform(np.log(2.0 ** -53), 0.0, 500000)), np.exp(rng.uniform(np.log(0.25), np.log(4.0), 500000)), edge])
    x = x[(x >= 2.0 ** -53) & (x <= 4.0)]
    assert x.size >= 1000000
    got, want = er.ln(x), np.log(x)
    assert got[x == 1.0].tolist() == [0.0] * int((x == 1.0).sum())
    rel = np.abs(got - want)[want != 0.0] / np.abs(want[want != 0.0])
    print(f"largest relative error of ln against np.log over {x.size} arguments: {rel.max():.3e}")
    assert rel.max() <= 1e-13


@pytest.mark.parametrize("seed,w,s", [(0, 0, 0), (5, 3, 7), (2 ** 64 - 1, 2 ** 63 + 12345, 2 ** 40 + 1), (2 ** 63 + 9, 129, 23)])
def test_the_words_are_numpys_philox(seed, w, s):
    # (uint64 arrays: numpy takes a list holding an integer >= 2^63 through float64 and drops its low bits)
    raw = np.random.Philox(counter=np.array([s, 0, w, 0], dtype=np.uint64), key=np.array([seed, 1], dtype=np.uint64)).random_raw(4)
    blk = er.words(s, [w, w + 1 if w < 2 ** 63 else 1], seed)
    assert blk[0].tolist() == raw.tolist()
    assert blk[1].tolist() != raw.tolist()
    other = np.random.Philox(counter=np.array([s, 0, w, 0], dtype=np.uint64), key=np.array([seed, 0], dtype=np.uint64)).random_raw(4)
    assert other.tolist() != raw.tolist()                      # key word 1 keeps the streams apart from nested sampling's


@pytest.mark.parametrize("move", [er.STRETCH, er.DE])
@pytest.mark.parametrize("ndim", [4, 65])
def test_a_flat_target_ends_uniform_in_every_coordinate(ndim, move):
    U, L, status, naccept, _, _ = er.ensemble(lambda Y: np.zeros(Y.shape[0]), flat_start(ndim), FLAT_ITERS[ndim], FLAT_ITERS[ndim], move,
                                              seed=FLAT_SEED)
    assert (status == 0).all() and ((U >= 0.0) & (U <= 1.0)).all() and not L.any()
    d = ks_distances(U)
    print(f"ndim {ndim}, move {move}, {FLAT_ITERS[ndim]} iterations: largest KS distance {d.max():.4f} (coordinate {d.argmax()}; bar "
          f"{KS_BAR:.4f}), acceptance {naccept.mean() / FLAT_ITERS[ndim]:.3f}")
    assert ks_distances(flat_start(ndim)).min() > 0.2           # the start is far from uniform
    assert (d < KS_BAR).all()


# ---- a correlated Gaussian well inside the cube ----------------------------------------------------------------------------------

def _gaussian():
    sd = np.array([0.02, 0.03, 0.025, 0.015, 0.035])
    corr = 0.6 ** np.abs(np.subtract.outer(np.arange(5), np.arange(5)))
    cov = corr * np.outer(sd, sd)
    mu = np.array([0.5, 0.45, 0.55, 0.5, 0.4])
    prec = np.linalg.inv(cov)

    def logl(U):
        d = U - mu
        return -0.5 * np.einsum("ij,jk,ik->i", d, prec, d)
    return mu, cov, logl


@pytest.mark.parametrize("move", [er.STRETCH, er.DE])
def test_a_correlated_gaussian_has_its_means_and_variances(move):
    """64 walkers, 500 iterations of burn-in, 6000 kept; 24 batches of 250 iterations (the autocorrelation time of the ensemble
    means: 31 .. 67 iterations for the stretch move, 14 .. 18 for DE).  Ten comparisons per move at 5 standard errors.
    Measured deviations in standard errors (seed 11): stretch, means 0.57, 1.92, 1.98, -0.05, -0.49 and variances -1.90, 0.25,
    2.07, 1.70, -1.86; DE, means -2.17, -3.78, -3.27, -1.79, -0.31 (neighbouring coordinates correlate at 0.6, so one excursion
    shows in several) and variances -0.32, 0.03, -0.19, 0.21, -0.71.  Seeds 12 .. 14 stay within 2.7 for both moves."""
    mu, cov, logl = _gaussian()
    res = ensemble.ensemble_sample(lambda U: (U.copy(), logl(U)), er.advance_with(logl, move), 5, 64, 6000, burn=500, thin=1,
                                   start=mu, ball=0.02, seed=11)
    assert res.cube.shape == (6000, 64, 5) and (res.status == 0).all()
    assert ((res.cube > 0.1) & (res.cube < 0.9)).all()         # well inside: the cube's faces play no part
    means = res.means()
    second = ((res.cube - mu) ** 2).mean(axis=1)               # E = the variance, whatever the ensemble mean does
    tau = res.autocorr_time()
    print(f"move {move}: acceptance {res.accept_frac.mean():.3f}, autocorrelation times {np.round(tau, 1)}")
    assert (tau > 1.0).all() and (tau < 250.0 / 2).all()        # a batch is long against it
    for name, series, truth in (("mean", means, mu), ("variance", second, np.diag(cov))):
        se = ensemble.batch_means_se(series, 24)
        dev = (series.mean(axis=0) - truth) / se
        print(f"move {move}: {name} deviations in standard errors {np.round(dev, 2)}")
        assert (np.abs(dev) <= 5.0).all()


# ---- the state machine -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", [er.STRETCH, er.DE])
@pytest.mark.parametrize("n", [4, 6, 130])
def test_no_walker_of_the_moving_half_is_read_as_a_partner(n, move):
    mu, cov, logl = _gaussian()
    U0 = 0.5 + 0.05 * (2.0 * np.random.default_rng(n).random((n, 5)) - 1.0)
    trace = []
    er.ensemble(logl, U0, 20, 1, move, seed=n, trace=trace)
    assert len(trace) == 40
    m = n // 2
    seen = set()
    for h, mov, partners in trace:
        assert mov.tolist() == list(range(h * m, (h + 1) * m))
        lo = (1 - h) * m
        assert ((partners >= lo) & (partners < lo + m)).all()
        if move == er.DE:
            assert (partners[:, 0] != partners[:, 1]).all()
        seen |= set(partners.reshape(-1).tolist())
    assert seen == set(range(n))                               # every walker serves as a partner at some point


@pytest.mark.parametrize("move", [er.STRETCH, er.DE])
def test_ten_iterations_are_four_and_then_six(move):
    mu, cov, logl = _gaussian()
    U0 = 0.5 + 0.05 * (2.0 * np.random.default_rng(1).random((16, 5)) - 1.0)
    U0[3, 2] = np.nan                                          # a bad start stays as given in both
    whole = er.ensemble(logl, U0, 10, 2, move, seed=9)
    a = er.ensemble(logl, U0, 4, 2, move, seed=9)
    b = er.ensemble(logl, a[0], 6, 2, move, seed=9, first_iter=4)
    assert whole[2][3] == -1 and whole[3][3] == 0 and np.isnan(whole[0][3, 2])
    assert whole[0].tobytes() == b[0].tobytes() and whole[1].tobytes() == b[1].tobytes()
    assert np.array_equal(whole[3], a[3] + b[3]) and 0 < whole[3].sum() < 10 * 16
    assert whole[4].tobytes() == np.concatenate([a[4], b[4]]).tobytes() and whole[5].tobytes() == np.concatenate([a[5], b[5]]).tobytes()
    assert whole[4][-1].tobytes() == whole[0].tobytes() and whole[5][-1].tobytes() == whole[1].tobytes()
    assert er.ensemble(logl, U0, 10, 2, move, seed=10)[0].tobytes() != whole[0].tobytes()


def test_batch_means_and_the_autocorrelation_window():
    rng = np.random.default_rng(0)
    x = rng.normal(size=(40000, 2))
    se = ensemble.batch_means_se(x, 40)
    assert se.shape == (2,) and np.all(np.abs(se * np.sqrt(40000) - 1.0) < 0.35)
    assert abs(ensemble.sokal_tau(x[:, 0]) - 1.0) < 0.2
    ar = np.zeros(40000)                                       # AR(1) with phi = 0.9: tau = (1 + phi) / (1 - phi) = 19
    for i in range(1, ar.size):
        ar[i] = 0.9 * ar[i - 1] + x[i, 1]
    assert abs(ensemble.sokal_tau(ar) - 19.0) < 4.0
    with pytest.raises(ValueError):
        ensemble.batch_means_se(x[:10], 20)
