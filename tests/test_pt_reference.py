"""CPU: the numpy restatement of the tempered ensemble sampler (tests/pt_reference.py) -- one rung at beta = 1 against
ens_reference.py, the swap words against numpy's own Philox bit generator, the partner map and the pairs of a round, what a
swap round preserves, the continuation, a flat target -- and the driver `tempering.tempered_sample` over it: the stepping-stone
evidence of a Gaussian against its closed form, and a two-mode target that the plain ensemble does not cross."""
import math

import numpy as np
import pytest

import ens_reference as er
import pt_reference as pr
from mcalf_amd import ensemble, tempering


def _gauss(mu, sd):
    mu, sd = np.asarray(mu, dtype=float), np.asarray(sd, dtype=float)
    return lambda U: -0.5 * (((U - mu) / sd) ** 2).sum(axis=1)


def _starts(T, n, ndim, seed, centre=0.5, half=0.05):
    return np.clip(centre + half * (2.0 * np.random.default_rng(seed).random((T, n, ndim)) - 1.0), 0.0, 1.0)


# ---- the state machine -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", [er.STRETCH, er.DE])
@pytest.mark.parametrize("swap_every", [0, 1])
def test_one_rung_at_beta_one_is_the_ensemble_sampler(move, swap_every):
    logl = _gauss([0.5, 0.45, 0.55], [0.03, 0.02, 0.04])
    U0 = _starts(1, 10, 3, 1)
    U0[0, 3, 1] = np.nan
    want = er.ensemble(logl, U0[0], 12, 5, move, seed=7, first_iter=3)
    U, L, status, naccept, nswap, CU, CL = pr.tempered(logl, U0, [1.0], 12, 5, swap_every, move, seed=7, first_iter=3)
    assert nswap.shape == (0, 10) and CU.shape == (2, 1, 10, 3) and CL.shape == (2, 1, 10)
    for got, ref in zip((U[0], L[0], status[0], naccept[0], CU[:, 0], CL[:, 0]), want):
        assert got.dtype == ref.dtype and np.ascontiguousarray(got).tobytes() == ref.tobytes()
    assert 0 < naccept.sum() < 12 * 9


@pytest.mark.parametrize("seed,r,t,n", [(0, 0, 0, 4), (5, 3, 2, 130), (2 ** 64 - 1, 2 ** 40 + 1, 62, 6), (2 ** 63 + 9, 23, 1, 128)])
def test_the_swap_words_are_numpys_philox(seed, r, t, n):
    key = np.array([seed, 2], dtype=np.uint64)
    shift = np.random.Philox(counter=np.array([r, 1, t, 0], dtype=np.uint64), key=key).random_raw(4)
    assert pr.swap_shift(r, t, n, seed) == int(shift[0]) % n
    zeta = pr.swap_zeta(r, t, n, seed)
    for w in (0, n - 1):
        raw = np.random.Philox(counter=np.array([r, 0, t * n + w, 0], dtype=np.uint64), key=key).random_raw(4)
        assert zeta[w] == ((int(raw[2]) >> 11) + 1) * 2.0 ** -53 and 0.0 < zeta[w] <= 1.0
    moves = np.random.Philox(counter=np.array([r, 0, t * n, 0], dtype=np.uint64), key=np.array([seed, 1], dtype=np.uint64)).random_raw(4)
    assert ((int(moves[2]) >> 11) + 1) * 2.0 ** -53 != zeta[0]                    # key word 1 keeps the swaps apart from the moves


@pytest.mark.parametrize("T", [2, 3, 4])
def test_the_partner_map_is_a_bijection_and_a_rounds_pairs_are_disjoint(T):
    shifts = set()
    for r in range(12):
        pairs = pr.swap_pairs(r, T)
        assert all(t % 2 == r % 2 and t + 1 < T for t in pairs)
        rungs = [t for p in pairs for t in (p, p + 1)]
        assert len(set(rungs)) == len(rungs)                                      # no rung is in two pairs
        assert pairs == [t for t in range(T - 1) if t % 2 == r % 2]               # and none that could swap is left out
        for t in pairs:
            for n in (4, 6, 130):
                j = pr.swap_partners(r, t, n, seed=3)
                assert np.array_equal(np.sort(j), np.arange(n))
                assert np.array_equal((j - np.arange(n)) % n, np.full(n, pr.swap_shift(r, t, n, 3)))
                shifts.add((n, int(j[0])))
    assert len(shifts) > 6                                                        # the shift varies
    assert pr.swap_pairs(1, 2) == [] and pr.swap_pairs(0, 3) == [0] and pr.swap_pairs(1, 3) == [1]      # T = 3: one rung sits out


def test_a_swap_round_preserves_the_multiset_of_rows_and_logl():
    rng = np.random.default_rng(0)
    T, n, ndim = 4, 6, 3
    beta = np.array([1.0, 0.5, 0.1, 0.0])
    for r in range(6):
        U, L = rng.random((T, n, ndim)), rng.normal(0.0, 3.0, (T, n))
        status = np.zeros((T, n), dtype=np.int32)
        status[1, 2] = -1
        nswap = np.zeros((T - 1, n), dtype=np.int32)
        before = np.concatenate([U.reshape(-1, ndim), L.reshape(-1, 1)], axis=1)
        U1, L1, trace = U.copy(), L.copy(), []
        pr.swap_round(U1, L1, status, nswap, beta, r, seed=r, trace=trace)
        after = np.concatenate([U1.reshape(-1, ndim), L1.reshape(-1, 1)], axis=1)
        assert np.array_equal(before[np.lexsort(before.T)], after[np.lexsort(after.T)])
        assert U1[1, 2].tobytes() == U[1, 2].tobytes() and L1[1, 2] == L[1, 2]     # a bad position keeps its state
        moved = (L1 != L)
        assert 0 < nswap.sum() < n * len(trace) and moved.sum() == 2 * nswap.sum()
        for t, j, zeta, acc in trace:
            assert np.array_equal(nswap[t], acc.astype(np.int32))
            assert np.array_equal(L1[t][acc], L[t + 1][j][acc]) and np.array_equal(U1[t + 1][j][acc], U[t][acc])
        untouched = [t for t in range(T) if t not in {p for e in trace for p in (e[0], e[0] + 1)}]
        assert all(np.array_equal(L1[t], L[t]) for t in untouched)


@pytest.mark.parametrize("move", [er.STRETCH, er.DE])
def test_ten_iterations_are_four_and_then_six_with_a_swap_round_every_third(move):
    logl = _gauss([0.5, 0.5, 0.5], [0.05, 0.04, 0.03])
    beta = [1.0, 0.3, 0.0]
    U0 = _starts(3, 8, 3, 2)
    U0[1, 5, 0] = 1.5
    whole = pr.tempered(logl, U0, beta, 10, 2, 3, move, seed=9, chain_temps=2)
    a = pr.tempered(logl, U0, beta, 4, 2, 3, move, seed=9, chain_temps=2)
    b = pr.tempered(logl, a[0], beta, 6, 2, 3, move, seed=9, first_iter=4, chain_temps=2)
    assert whole[2][1, 5] == -1 and whole[3][1, 5] == 0 and whole[0][1, 5, 0] == 1.5 and not whole[4][:, 5].all()
    assert whole[0].tobytes() == b[0].tobytes() and whole[1].tobytes() == b[1].tobytes()
    assert np.array_equal(whole[3], a[3] + b[3]) and np.array_equal(whole[4], a[4] + b[4])
    assert 0 < whole[4].sum() < 2 * 8 * 2                                          # rounds 0, 1, 2: pairs 0, 1, 0
    assert whole[5].tobytes() == np.concatenate([a[5], b[5]]).tobytes() and whole[6].tobytes() == np.concatenate([a[6], b[6]]).tobytes()
    assert whole[5].shape == (5, 2, 8, 3) and whole[6].shape == (5, 3, 8)
    assert whole[5][-1].tobytes() == whole[0][:2].tobytes() and whole[6][-1].tobytes() == whole[1].tobytes()
    assert pr.tempered(logl, U0, beta, 10, 2, 3, move, seed=9, first_iter=1)[0].tobytes() != whole[0].tobytes()
    never = pr.tempered(logl, U0, beta, 10, 2, 0, move, seed=9)
    assert not never[4].any() and never[0].tobytes() != whole[0].tobytes()


def test_a_flat_target_accepts_every_swap():
    """logL is one constant, so q = 0 and ln zeta < 0 for every zeta < 1: every drawn swap of good positions is accepted."""
    T, n = 4, 6
    U0 = np.random.default_rng(0).random((T, n, 2))
    U0[2, 1, 0] = np.nan
    trace = []
    out = pr.tempered(lambda U: np.full(U.shape[0], 3.5), U0, [1.0, 0.5, 0.25, 0.0], 9, 1, 2, seed=1, trace=trace)
    rounds = [e[1] for e in trace if e[0] == "round"]
    assert rounds == [0, 1, 2, 3] and tempering.swap_rounds(0, 9, 2, T).tolist() == [2, 2, 2]
    good = (out[2][:-1] == 0)
    for t, j, zeta, acc in (e for e in trace if e[0] != "round"):
        assert (zeta < 1.0).all() and np.array_equal(acc, good[t] & (out[2][t + 1][j] == 0))
    assert out[4].sum(axis=1).tolist() == [2 * n, 2 * (n - 1), 2 * (n - 1)]       # two rounds each; the bad position is in pairs 1 and 2
    assert not out[4][2, 1] and (out[0][2, 1, 1] == U0[2, 1, 1])
    assert tempering.swap_rounds(4, 6, 3, 3).tolist() == [1, 1] and tempering.swap_rounds(0, 10, 3, 3).tolist() == [2, 1]
    assert tempering.swap_rounds(5, 0, 1, 3).tolist() == [0, 0] and tempering.swap_rounds(0, 5, 0, 3).tolist() == [0, 0]


# ---- the driver ------------------------------------------------------------------------------------------------------------------

def test_the_default_ladder():
    b = tempering.default_ladder(16, 1e-4)
    assert b.shape == (16,) and b[0] == 1.0 and b[-1] == 0.0 and abs(b[14] - 1e-4) < 1e-18 and (np.diff(b) < 0.0).all()
    assert np.allclose(b[1:15] / b[:14], 1e-4 ** (1.0 / 14.0), rtol=1e-12)
    assert tempering.default_ladder(2, 0.1).tolist() == [1.0, 0.0] and tempering.default_ladder(3, 0.1).tolist() == [1.0, 0.1, 0.0]
    for bad in ((1, 0.1), (4, 0.0), (4, 1.0)):
        with pytest.raises(ValueError):
            tempering.default_ladder(*bad)


def test_the_driver_over_the_reference_callables():
    logl = _gauss([0.5, 0.5, 0.5], [0.05, 0.05, 0.05])
    lo, hi = np.array([1.0, -2.0, 10.0]), np.array([3.0, 2.0, 20.0])
    transform = lambda U: lo + U * (hi - lo)
    seen = []

    def cube_ll(U):
        seen.append(U.shape[0])
        return transform(U), logl(U)
    beta = [1.0, 0.2, 0.0]
    res = tempering.tempered_sample(cube_ll, pr.advance_with(logl, beta, transform=transform), 3, 8, 40, beta, burn=10, thin=4, swap_every=3, seed=5)
    assert res.logL.shape == (10, 3, 8) and res.cube.shape == (10, 8, 3) and res.last.shape == (3, 8, 3) and not seen
    U0 = np.random.default_rng(5).random((3, 8, 3))
    whole = pr.tempered(logl, U0, beta, 50, 1, 3, seed=5)
    assert res.last.tobytes() == whole[0].tobytes()                                # burn-in and kept run are one run of 50 iterations
    assert res.cube.tobytes() == np.ascontiguousarray(whole[5][10:][3::4, 0]).tobytes() and res.logL.tobytes() == np.ascontiguousarray(whole[6][10:][3::4]).tobytes()
    assert res.accept_frac.shape == (3,) and (res.accept_frac > 0.0).all() and (res.accept_frac <= 1.0).all()
    assert res.swap_frac.shape == (2,) and (res.swap_frac > 0.0).all() and (res.swap_frac <= 1.0).all()
    cold = res.cold()
    assert seen == [80] and isinstance(cold, ensemble.EnsembleResult)              # one pass over the cold rows alone
    assert np.array_equal(cold.theta, transform(res.cube)) and cold.logL.tobytes() == logl(res.cube.reshape(-1, 3)).tobytes()
    ll, th = cold.flat()
    assert ll.shape == (80,) and th.shape == (80, 3) and th.flags.c_contiguous and cold.autocorr_time().shape == (3,)
    lnz, err = res.logZ_stepping_stone(5)
    assert np.isfinite(lnz) and err > 0.0 and np.isfinite(res.logZ_ti())
    open_ladder = tempering.tempered_sample(cube_ll, pr.advance_with(logl, [1.0, 0.5]), 3, 8, 20, [1.0, 0.5], seed=5)
    with pytest.raises(ValueError, match="beta = 0"):
        open_ladder.logZ_stepping_stone(5)
    with pytest.raises(ValueError, match="beta = 0"):
        open_ladder.logZ_ti()
    with pytest.raises(ValueError):
        res.logZ_stepping_stone(11)                                                # 10 kept iterations
    for bad in (dict(nwalkers=5), dict(nwalkers=2), dict(thin=0), dict(start=[0.5] * 3), dict(ball=0.1), dict(nsteps=-1), dict(swap_every=-1),
                dict(betas=[0.5, 1.0]), dict(betas=[1.0, 1.0]), dict(betas=[1.0, -0.1]), dict(betas=[np.inf, 1.0])):
        kw = dict(nwalkers=8, nsteps=4, thin=1, betas=beta)
        kw.update(bad)
        betas = kw.pop("betas")
        with pytest.raises(ValueError):
            tempering.tempered_sample(cube_ll, pr.advance_with(logl, betas), 3, betas=betas, **kw)


# ---- the evidence of a Gaussian ----------------------------------------------------------------------------------------------------

GAUSS_MU, GAUSS_SD = np.array([0.5, 0.45, 0.6]), np.array([0.05, 0.03, 0.04])


def _gauss_lnz():
    """ln of the integral of exp(logL) over the cube: per coordinate sd sqrt(2 pi) times the normal mass inside [0, 1]."""
    mass = [0.5 * (math.erf((1.0 - m) / (s * math.sqrt(2.0))) - math.erf((0.0 - m) / (s * math.sqrt(2.0)))) for m, s in zip(GAUSS_MU, GAUSS_SD)]
    return float(np.sum(np.log(GAUSS_SD * np.sqrt(2.0 * np.pi) * np.array(mass))))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_stepping_stones_find_the_evidence_of_a_gaussian(seed):
    """12 rungs down to beta 1e-3 and the prior (logL ranges over -260 .. 0 across the cube), 32 walkers each from uniform
    starts, 200 iterations of burn-in, 1000 kept, 20 batches of 50.  Measured deviations from the closed form in standard errors
    (about 0.02 each): see the printed line; the bar is 5."""
    logl = _gauss(GAUSS_MU, GAUSS_SD)
    beta = tempering.default_ladder(12, 1e-3)
    res = tempering.tempered_sample(lambda U: (U.copy(), logl(U)), pr.advance_with(logl, beta), 3, 32, 1000, beta, burn=200, seed=seed)
    lnz, err = res.logZ_stepping_stone(20)
    want = _gauss_lnz()
    print(f"seed {seed}: ln Z {lnz:.4f} +- {err:.4f}, closed form {want:.4f}: {(lnz - want) / err:+.2f} standard errors; thermodynamic "
          f"integration {res.logZ_ti():.4f}; acceptance {np.round(res.accept_frac, 2)}, swaps {np.round(res.swap_frac, 2)}")
    assert (res.status == 0).all() and 0.0 < err < 0.1
    assert abs(lnz - want) <= 5.0 * err


# ---- two modes -------------------------------------------------------------------------------------------------------------------

MODES, MODE_SD, MODE_WEIGHTS = np.array([[0.25, 0.3], [0.75, 0.7]]), 0.02, np.array([0.7, 0.3])


def _two_modes(U):
    parts = [np.log(w) - 0.5 * (((U - mu) / MODE_SD) ** 2).sum(axis=1) for mu, w in zip(MODES, MODE_WEIGHTS)]
    return np.logaddexp(parts[0], parts[1])


def _in_second_mode(cube):
    return np.abs(cube - MODES[1]).max(axis=-1) < 10.0 * MODE_SD


@pytest.mark.parametrize("seed", [0, 1])
def test_tempering_crosses_between_two_modes_and_the_plain_ensemble_does_not(seed):
    """Two Gaussians of width 0.02, 35 widths apart, holding 0.7 and 0.3 of the mass; every walker of every rung starts in a ball
    of half-width 0.02 around the first.  8 rungs down to beta 1e-3 and the prior, 32 walkers each, 300 iterations of burn-in,
    2000 kept, 20 batches of 100: the cold rung's share of walkers in the second mode is 0.3 within 5 batch-means standard
    errors.  The plain ensemble (one rung, same start, same length) has no walker there at any kept iteration."""
    beta = tempering.default_ladder(8, 1e-3)
    cube_ll = lambda U: (U.copy(), _two_modes(U))
    res = tempering.tempered_sample(cube_ll, pr.advance_with(_two_modes, beta), 2, 32, 2000, beta, burn=300, start=MODES[0], ball=0.02, seed=seed)
    share = _in_second_mode(res.cube).mean(axis=1)
    near = (np.abs(res.cube[:, :, None, :] - MODES).max(axis=-1) < 10.0 * MODE_SD).any(axis=2)
    se = ensemble.batch_means_se(share, 20)
    dev = (share.mean() - MODE_WEIGHTS[1]) / se
    print(f"seed {seed}: share of the cold rung in the second mode {share.mean():.4f} +- {se:.4f} ({dev:+.2f} standard errors from "
          f"{MODE_WEIGHTS[1]}); acceptance {np.round(res.accept_frac, 2)}, swaps {np.round(res.swap_frac, 2)}")
    assert near.all()                                                              # every cold walker sits in one of the two
    assert share.min() < share.max() and abs(dev) <= 5.0
    plain = ensemble.ensemble_sample(cube_ll, er.advance_with(_two_modes), 2, 32, 2000, burn=300, start=MODES[0], ball=0.02, seed=seed)
    assert not _in_second_mode(plain.cube).any() and plain.accept_frac.mean() > 0.2
