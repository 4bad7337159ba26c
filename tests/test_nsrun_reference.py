"""CPU: the numpy restatement of the device-resident nested-sampling run (tests/nsrun_reference.py) -- its evidence against
nested.py's own arithmetic, its picks against numpy's Philox, and the run itself on a Gaussian whose evidence is known in
closed form (`_gauss`, sigma 0.02: the fixture tests/test_ns_reference.py holds the host driver to)."""
import numpy as np
import pytest

import ns_reference as nr
import nsrun_reference as ref
from mcalf_amd import nested

SIGMA = 0.02


def _gauss(U):
    return -0.5 * (((np.asarray(U) - 0.5) / SIGMA) ** 2).sum(axis=1)


def test_the_evidence_is_nested_pys():
    """The dead sequence of a `nested.nested_sample` run (a vetoed and a NaN initial point in it), put through `finish`."""
    def logl(U):
        L = _gauss(U)
        L[(U[:, 0] > 0.97)] = -np.inf
        L[(U[:, 1] > 0.98)] = np.nan
        return L
    res = nested.nested_sample(lambda U: (U.copy(), logl(U)), nr.replace_with(logl), 4, 120, batch=30, nmoves=4, seed=5, max_rounds=25)
    assert np.isnan(res.logL).any() and np.isneginf(res.logL).any()
    logZ, H, logw = ref.finish(res.logL, 120, 30)
    assert abs(logZ - res.logZ) <= 1e-12 and abs(H - res.H) <= 1e-12
    assert np.array_equal(np.isneginf(logw), np.isneginf(res.logw))
    ok = np.isfinite(logw)
    assert np.abs(logw[ok] - res.logw[ok]).max() <= 1e-12
    # the running value, block by block
    ev = ref.Evidence()
    for r in range(res.rounds):
        ev.die(ref.key(res.logL[r * 30:(r + 1) * 30]), 120)
    assert ev.logX == pytest.approx(res.rounds * sum(-1.0 / (120 - j) for j in range(30)), abs=1e-12)


@pytest.mark.parametrize("seed,rnd", [(0, 0), (7, 3), (2 ** 63 + 5, 2 ** 33), (2 ** 64 - 1, 12)])
def test_the_picks_are_numpys_philox(seed, rnd):
    """numpy increments word 0 of the counter before its first block: counter [rnd, 0, j, 0] yields the block at rnd + 1."""
    K, nstarts = 9, 1000003
    got = ref.picks(seed, rnd, K, nstarts)
    for j in range(K):
        gen = np.random.Philox(counter=np.array([rnd, 0, j, 0], dtype=np.uint64), key=np.array([seed, 3], dtype=np.uint64))
        assert int(got[j]) == int(gen.random_raw(1)[0]) % nstarts, (seed, rnd, j)


def test_select_is_the_host_drivers():
    L = np.array([3.0, -np.inf, 1.0, np.nan, 1.0, 0.0, -0.0, 5.0, 1.0])
    order, dying, lmin, r0, pick = ref.select(L, 5, seed=1, rnd=0)
    assert order.tolist() == [1, 3, 5, 6, 2, 4, 8, 0, 7] and dying.tolist() == [1, 3, 5, 6, 2]
    assert lmin == 1.0 and r0 == 7 and set(pick) <= {0, 7}                 # the survivors equal to lmin are not starts
    assert ref.select(np.ones(6), 2, seed=1, rnd=0)[4] is None             # a plateau
    assert ref.select(L, 8, seed=1, rnd=0)[4].tolist() == [7] * 8                                  # one start left


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_run_finds_the_gaussian_evidence(seed):
    """4-D Gaussian in the cube (sigma 0.02, centre 0.5, unnormalised): Z = (2 pi sigma^2)^2, within 4 sqrt(H / nlive)."""
    U0 = np.random.default_rng(seed).random((400, 4))
    run = ref.Run(_gauss, U0, 100, 8, 400, seed=seed)
    assert run.advance(10 ** 6) == ref.CONVERGED
    logZ, H, logw, cube, logL = run.finish()
    want = 2.0 * np.log(2.0 * np.pi * SIGMA ** 2)
    err = np.sqrt(H / 400)
    print(f"seed {seed}: logZ {logZ:.4f} want {want:.4f}, {abs(logZ - want) / err:.2f} standard errors of {err:.4f}; H {H:.3f}, {run.rounds} rounds")
    assert abs(logZ - want) <= 4.0 * err
    assert abs(np.exp(logw).sum() - 1.0) <= 1e-12 and (np.diff(logL) >= 0.0).all()
    assert logL.size == run.rounds * 100 + 400 == run.ndead + 400 and run.unfinished == 0
    assert logL.tobytes() == _gauss(cube).tobytes()


def test_the_cut_into_calls_changes_nothing_and_a_full_buffer_stops():
    U0 = np.random.default_rng(3).random((40, 4))
    a = ref.Run(_gauss, U0, 10, 4, 200, seed=3, dlogz=0.0)
    b = ref.Run(_gauss, U0, 10, 4, 200, seed=3, dlogz=0.0)
    assert a.advance(6) == ref.BUDGET
    assert [b.advance(n) for n in (2, 0, 4)] == [ref.BUDGET] * 3
    fa, fb = a.finish(), b.finish()
    assert fa[:2] == fb[:2] and all(x.tobytes() == y.tobytes() for x, y in zip(fa[2:], fb[2:]))
    c = ref.Run(_gauss, U0, 10, 4, 200, seed=3, dlogz=0.0, max_dead=40 + 3 * 10)
    assert c.advance(100) == ref.FULL and c.rounds == 3
