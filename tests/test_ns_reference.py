"""CPU: the numpy restatement of nested sampling's replacement step (tests/ns_reference.py) -- its Philox4x64-10 against
numpy's own bit generator, its state machine's invariants -- and the host driver `nested.nested_sample` on a Gaussian whose
evidence is known in closed form."""
import numpy as np
import pytest

import ns_reference as nr
from mcalf_amd import nested

SIGMA = 0.02


def _gauss(U):
    return -0.5 * (((np.asarray(U) - 0.5) / SIGMA) ** 2).sum(axis=1)


@pytest.mark.parametrize("seed,sid", [(0, 0), (1, 7), (12345, 2 ** 32), (2 ** 63 + 5, 2 ** 40 + 3), (2 ** 64 - 1, 2 ** 64 - 1)])
def test_philox_is_numpys(seed, sid):
    """numpy increments word 0 of the counter before its first block: counter [0, 0, sid, 0] yields blocks it = 1, 2, ..."""
    n = 6
    # (uint64 arrays: numpy takes a list holding an integer >= 2^63 through float64 and drops its low bits)
    counter, key = np.array([0, 0, sid, 0], dtype=np.uint64), np.array([seed, 0], dtype=np.uint64)
    raw = np.random.Philox(counter=counter, key=key).random_raw(4 * n).reshape(n, 4)
    for it in (1, 2, n):
        blk = nr.philox4x64(np.array([it, 0, sid, 0], dtype=np.uint64), np.array([seed, 0], dtype=np.uint64))
        assert blk.tolist() == raw[it - 1].tolist(), (seed, sid, it)
    w0, w1 = nr.words(3, [sid, 5, sid], seed)
    assert (int(w0[0]), int(w1[0])) == (int(raw[2, 0]), int(raw[2, 1])) and w0[2] == w0[0] and w0[1] != w0[0]
    # Generator.random() is (w >> 11) 2^-53
    u = np.random.Generator(np.random.Philox(counter=counter, key=key)).random(4)
    assert u.tolist() == ((raw[0] >> np.uint64(11)).astype(float) * 2.0 ** -53).tolist()


def test_state_machine_invariants():
    rng = np.random.default_rng(4)
    U0 = 0.5 + rng.normal(0.0, SIGMA, (40, 4))
    lmin = np.sort(_gauss(U0))[10]
    U0[0, 1] = 1.5                     # outside the cube
    U0[1, 2] = np.nan
    D = np.vstack([np.eye(4) * SIGMA, np.zeros((1, 4))])             # (an all-zero direction: the trial is the point itself)
    U, L, status, nevals, moves = nr.slice_replace(_gauss, U0, lmin, D, np.arange(40), 8, 400, seed=3)
    bad = ~(_gauss(U0) > lmin)
    bad[:2] = True
    assert (status[bad] == -1).all() and (status[~bad] == 1).all()
    assert np.array_equal(U[bad], U0[bad], equal_nan=True) and (nevals[bad] == 0).all()
    assert (moves[~bad] == 8).all() and (nevals[~bad] >= 8).all() and (L[~bad] > lmin).all()
    assert L[~bad].tobytes() == _gauss(U[~bad]).tobytes()
    assert ((U[~bad] >= 0) & (U[~bad] <= 1)).all() and (np.abs(U[~bad] - U0[~bad]).max(axis=1) > 0).all()
    # a row's result depends on its own inputs alone
    one = nr.slice_replace(_gauss, U0[7:8], lmin, D, [7], 8, 400, seed=3)
    assert all(a[7:8].tobytes() == b.tobytes() for a, b in zip((U, L, status, nevals, moves), one))
    # out of steps: status 0, the last accepted point, still under the constraint
    Us, Ls, ss, ns, ms = nr.slice_replace(_gauss, U0, lmin, D, np.arange(40), 8, 3, seed=3)
    assert (ss[~bad] == 0).all() and (ns[~bad] == 3).all() and (ms <= 3).all() and (Ls[~bad] > lmin).all()
    # nmoves 0: the checked start
    Uz, Lz, sz, nz, mz = nr.slice_replace(_gauss, U0, lmin, D, np.arange(40), 0, 50, seed=3)
    assert np.array_equal(Uz, U0, equal_nan=True) and (sz[~bad] == 1).all() and (sz[bad] == -1).all() and not nz.any()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_nested_sampling_finds_the_gaussian_evidence(seed):
    """4-D Gaussian in the cube (sigma 0.02, centre 0.5, unnormalised): Z = (2 pi sigma^2)^2.  The bar is 4 standard errors
    sqrt(H / nlive) of the nested-sampling estimator."""
    res = nested.nested_sample(lambda U: (U.copy(), _gauss(U)), nr.replace_with(_gauss), 4, 400, batch=100, nmoves=8, seed=seed)
    want = 2.0 * np.log(2.0 * np.pi * SIGMA ** 2)
    err = np.sqrt(res.H / 400)
    print(f"seed {seed}: logZ {res.logZ:.4f} want {want:.4f}, {abs(res.logZ - want) / err:.2f} standard errors of {err:.4f}; H {res.H:.3f}, "
          f"{res.rounds} rounds, {res.nevals} evaluations, {res.unfinished} unfinished")
    assert abs(res.logZ - want) <= 4.0 * err
    assert res.logZ_err == pytest.approx(err)
    assert abs(np.exp(res.logw).sum() - 1.0) <= 1e-12
    assert (np.diff(res.logL) >= 0.0).all()
    assert res.cube.shape == res.theta.shape == (res.logL.size, 4) and res.logL.size == res.rounds * 100 + 400
    assert res.unfinished == 0
    ll, th = res.equal_weight_samples(np.random.default_rng(seed))
    assert 50 < ll.size < res.logL.size and th.shape == (ll.size, 4)
    assert abs(th.mean() - 0.5) < 0.01 and abs(th.std() - SIGMA) < 0.005


def test_driver_handles_vetoed_and_nan_initial_points():
    """-inf and NaN logL among the initial points sort first, carry no weight and are never started from."""
    def logl(U):
        L = _gauss(U)
        L[U[:, 0] < 0.2] = -np.inf
        L[(U[:, 0] >= 0.2) & (U[:, 0] < 0.3)] = np.nan
        return L
    res = nested.nested_sample(lambda U: (U.copy(), logl(U)), nr.replace_with(logl), 4, 60, batch=15, nmoves=4, dlogz=0.1, seed=5)
    first = res.logL[:15]
    assert (np.isnan(first) | np.isneginf(first)).all() and np.isnan(res.logL).any() and np.isneginf(res.logL).any()
    assert np.isfinite(res.logZ) and abs(np.exp(res.logw).sum() - 1.0) <= 1e-12
    assert (np.exp(res.logw[~np.isfinite(res.logL)]) == 0.0).all()
    with pytest.raises(ValueError, match="batch"):
        nested.nested_sample(lambda U: (U, _gauss(U)), nr.replace_with(_gauss), 4, 8, batch=8)


def test_directions_fall_back_to_the_diagonal():
    pts = np.random.default_rng(0).random((50, 3))
    D = nested.directions(pts)
    assert np.allclose(D.T @ D, np.cov(pts, rowvar=False), rtol=1e-6)            # rows are the columns of the factor
    pts[:, 1] = np.nan
    D = nested.directions(pts)
    assert np.array_equal(D != 0.0, np.eye(3, dtype=bool)) and D[1, 1] == 1.0
