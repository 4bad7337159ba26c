"""GPU: the tempered ensemble sampler (mcalf_tempered_batch[_device]) against the numpy restatement tests/pt_reference.py with
logL = als_fitter.loglike_cube_batch (the existing entry: every decision sees the same bits): U by value (the sign of a zero
may differ), logL and the chain's logL by bytes, naccept, nswap and status equal -- no tolerance.  Then one rung at beta = 1
against `ensemble_batch`, its invariance under entry, stream, device count and continuation, and the evidence and the posterior
moments of a three-parameter problem end to end against a quadrature of the C oracle.  Every case is at most 2048 rows per
launch and 300 pixels."""
import ctypes as C

import numpy as np
import pytest
import torch

import ens_reference as er
import many_components as mc
import mcalf_amd
import pt_reference as pr
from cases import problem_from_kwargs, tiny_problem
from mcalf_amd import _lib, ensemble, tempering, workloads
from mcalf_amd.routines.hires_fitter import write_equal_weights
from test_gpu_ns import _evidence_problem

pytestmark = pytest.mark.gpu

MOVES = {"stretch": er.STRETCH, "de": er.DE}
LADDERS = {1: [1.0], 2: [1.0, 0.2], 3: [1.0, 0.3, 0.0]}


def _logl(fit):
    return lambda U: fit.loglike_cube_batch(U, return_theta=False)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _ball(centre, half, shape, rng):
    return np.clip(centre + half * (2.0 * rng.random(tuple(shape) + (centre.size,)) - 1.0), 0.0, 1.0)


def _drawn(nsteps, swap_every, T, n, first_iter=0):
    """Swaps drawn for the pairs (t, t + 1) over a call [T - 1]."""
    return tempering.swap_rounds(first_iter, nsteps, swap_every, T) * n


def _device_call(fit, U0, betas, nsteps, thin, swap_every, move, seed=0, first_iter=0, chain_temps=1, stream=None, theta=True, chain=True):
    """mcalf_tempered_batch_device on torch tensors: rc and (U, theta, logL, status, naccept, nswap, CU, CL) as numpy arrays."""
    T, n, ndim = U0.shape
    betas = np.ascontiguousarray(betas, dtype=float)
    opts = _lib.mcalf_pt_opts(nsteps, thin, MOVES[move], T, swap_every, chain_temps, er.default_scale(MOVES[move], ndim), seed, first_iter)
    nkeep = nsteps // thin
    dU0 = torch.from_numpy(np.ascontiguousarray(U0)).cuda()
    dU, dT = (torch.full(U0.shape, -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    dL = torch.full((T, n), -7.0, dtype=torch.float64, device="cuda")
    dS, dN = (torch.full((T, n), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    dW = torch.full((max(T - 1, 0), n), -7, dtype=torch.int32, device="cuda")
    dCU = torch.full((nkeep, chain_temps, n, ndim), -7.0, dtype=torch.float64, device="cuda")
    dCL = torch.full((nkeep, T, n), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream() if stream is None else stream
    stream.wait_stream(torch.cuda.current_stream())
    rc = fit._lib.mcalf_tempered_batch_device(fit._ctx, dU0.data_ptr(), n, betas.ctypes.data, C.addressof(opts), dU.data_ptr(),
                                              dT.data_ptr() if theta else None, dL.data_ptr(), dS.data_ptr(), dN.data_ptr(), dW.data_ptr(),
                                              dCU.data_ptr() if chain else None, dCL.data_ptr() if chain else None, C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, tuple(t.cpu().numpy() for t in (dU, dT, dL, dS, dN, dW, dCU, dCL))


def _against_reference(fit, U0, betas, nsteps, thin, swap_every, move, seed, first_iter=0, chain_temps=1, logl=None):
    """The host entry against pt_reference; theta is the prior transform of U, logL the cube entry's value of U and the last
    chain slot the final state when thin divides nsteps."""
    T, n, ndim = U0.shape
    got = fit.tempered_batch(U0, betas, nsteps, thin=thin, swap_every=swap_every, move=move, seed=seed, first_iter=first_iter, chain_temps=chain_temps)
    U, theta, L, status, naccept, nswap, CU, CL = got
    rU, rL, rs, rn, rw, rCU, rCL = pr.tempered(logl or _logl(fit), U0, betas, nsteps, thin, swap_every, MOVES[move], None, seed, first_iter, chain_temps)
    assert np.array_equal(status, rs) and np.array_equal(naccept, rn) and nswap.shape == rw.shape and np.array_equal(nswap, rw)
    assert np.array_equal(U, rU, equal_nan=True)
    assert L.tobytes() == rL.tobytes()
    assert CU.shape == rCU.shape and np.array_equal(CU, rCU, equal_nan=True)
    assert CL.shape == rCL.shape and CL.tobytes() == rCL.tobytes()
    assert L.tobytes() == _logl(fit)(U.reshape(T * n, ndim)).tobytes()
    assert np.array_equal(theta.reshape(T * n, ndim), fit.scale_cube_batch(U.reshape(T * n, ndim)), equal_nan=True)
    if nsteps >= thin and nsteps % thin == 0:
        assert np.array_equal(CU[-1], U[:chain_temps], equal_nan=True) and CL[-1].tobytes() == L.tobytes()
    assert (naccept[status == -1] == 0).all() and (naccept <= nsteps).all() and (naccept >= 0).all()
    assert (nswap >= 0).all() and (nswap.sum(axis=1) <= _drawn(nsteps, swap_every, T, n, first_iter)).all()
    return got


# ---- the ndim-4 problem ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    """(fit, the best of 256 uniform points of the cube) of cases.tiny_problem(64)."""
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        draws = np.random.default_rng(1).random((256, fit.ndim))
        yield fit, draws[np.nanargmax(_logl(fit)(draws))]


@pytest.mark.parametrize("thin", [1, 5])
@pytest.mark.parametrize("swap_every", [1, 3])
@pytest.mark.parametrize("move", ["stretch", "de"])
@pytest.mark.parametrize("T", [1, 2, 3])
@pytest.mark.parametrize("n", [4, 6, 128, 130])
def test_trajectories(tiny, n, T, move, swap_every, thin):
    """Halves of 2, 3, 64 and 65 walkers; with three rungs one sits out every round, with two the odd rounds have no pair (and
    the chain slot of such an iteration is the decide kernel's); kept iterations with and without a swap round."""
    fit, best = tiny
    U0 = _ball(best, 0.1, (T, n), np.random.default_rng(100 * T + n))
    U, theta, L, status, naccept, nswap, CU, CL = _against_reference(fit, U0, LADDERS[T], 12, thin, swap_every, move, seed=n + thin + 7 * T)
    assert CU.shape == (12 // thin, 1, n, fit.ndim) and CL.shape == (12 // thin, T, n) and (status == 0).all()
    assert 0 < naccept.sum() < 12 * n * T                   # moves are both accepted and rejected
    assert ((U >= 0.0) & (U <= 1.0)).all()
    if T > 1:
        drawn = _drawn(12, swap_every, T, n)
        assert drawn.sum() > 0 and 0 < nswap.sum() < drawn.sum()      # and so are swaps


@pytest.mark.parametrize("move", ["stretch", "de"])
def test_one_rung_at_beta_one_is_the_ensemble_entry_byte_for_byte(tiny, move):
    fit, best = tiny
    U0 = _ball(best, 0.1, (130,), np.random.default_rng(3))
    U0[9, 1] = np.nan
    want = fit.ensemble_batch(U0, 11, thin=2, move=move, seed=5, first_iter=2)
    for swap_every in (0, 1):
        got = fit.tempered_batch(U0[None], [1.0], 11, thin=2, swap_every=swap_every, move=move, seed=5, first_iter=2)
        assert got[5].shape == (0, 130) and got[6].shape == (5, 1, 130, fit.ndim) and got[7].shape == (5, 1, 130)
        assert _same([got[k] for k in (0, 1, 2, 3, 4, 6, 7)], want)
    assert want[3][9] == -1 and 0 < want[4].sum() < 11 * 129
    rc, dev = _device_call(fit, U0[None], [1.0], 11, 2, 1, move, seed=5, first_iter=2)
    assert rc == 0 and _same([dev[k] for k in (0, 1, 2, 3, 4, 6, 7)], want)


def test_no_step_no_chain_and_no_walker(tiny):
    fit, best = tiny
    U0 = _ball(best, 0.1, (3, 6), np.random.default_rng(0))
    got = _against_reference(fit, U0, LADDERS[3], 0, 1, 1, "stretch", seed=1)
    assert got[0].tobytes() == U0.tobytes() and got[6].shape == (0, 1, 6, fit.ndim) and not got[4].any() and not got[5].any()
    none = fit.tempered_batch(U0, LADDERS[3], 7, thin=2, chain=False, seed=1)
    kept = fit.tempered_batch(U0, LADDERS[3], 7, thin=2, seed=1)
    assert none[6] is None and none[7] is None and _same(none[:6], kept[:6]) and kept[7].shape == (3, 3, 6)
    opts = _lib.mcalf_pt_opts(1, 1, 0, 3, 1, 1, 2.0, 0, 0)
    beta = np.array(LADDERS[3])
    assert fit._lib.mcalf_tempered_batch(fit._ctx, None, 0, beta.ctypes.data, C.addressof(opts), *([None] * 8)) == 0
    with pytest.raises(RuntimeError, match="beta must be strictly decreasing"):
        fit.tempered_batch(U0, [1.0, 1.0, 0.0], 1)
    with pytest.raises(ValueError):
        fit.tempered_batch(U0, [1.0, 0.0], 1)                                      # two rungs of starts for three betas
    big = _lib.mcalf_pt_opts(2 ** 31 - 1, 1, 0, 3, 1, 1, 2.0, 0, 0)               # 2^31 slots: far above 4 GiB
    one = np.zeros(1)
    rc = fit._lib.mcalf_tempered_batch(fit._ctx, U0.ctypes.data, 6, beta.ctypes.data, C.addressof(big), got[0].ctypes.data, None, got[2].ctypes.data,
                                       got[3].ctypes.data, got[4].ctypes.data, got[5].ctypes.data, one.ctypes.data, one.ctypes.data)
    assert rc == _lib.MCALF_ERR_RANGE
    assert f"the largest nkeep for this ensemble is {(4 << 30) // (6 * (fit.ndim + 3) * 8)}".encode() in fit._lib.mcalf_last_error(fit._ctx)


# ---- a lane owns several coordinates -------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def many():
    made = {}

    def get(ndim):
        if ndim not in made:
            fit = mcalf_amd.als_fitter(None, **mc.many(ndim)[0])
            fit.__enter__()
            assert fit.ndim == ndim
            draws = np.random.default_rng(ndim).random((4 * ndim, ndim))
            made[ndim] = (fit, draws[np.nanargmax(_logl(fit)(draws))])
        return made[ndim]
    yield get
    for fit, _ in made.values():
        fit.__exit__(None, None, None)


@pytest.mark.parametrize("move", ["stretch", "de"])
@pytest.mark.parametrize("ndim", [65, 129])
def test_a_swap_exchanges_the_coordinates_a_lane_reaches_in_its_later_turns(many, ndim, move):
    """Two rungs of 8 walkers.  One iteration with its swap round against the same iteration without (the moves' words do not
    depend on the swaps): a position that swapped holds its partner's whole row, the coordinates from index 64 on among them,
    and these differ from what it held.  A swap kernel that moved the first 64 coordinates only would fail here."""
    fit, best = many(ndim)
    betas = [1.0, 0.5]
    U0 = _ball(best, 0.02, (2, 8), np.random.default_rng(ndim))
    _against_reference(fit, U0, betas, 12, 5, 1, move, seed=ndim)
    _against_reference(fit, U0, betas, 12, 1, 3, move, seed=ndim)
    with_swap = fit.tempered_batch(U0, betas, 1, swap_every=1, move=move, seed=ndim)
    without = fit.tempered_batch(U0, betas, 1, swap_every=0, move=move, seed=ndim)
    j = pr.swap_partners(0, 0, 8, ndim)
    w = np.flatnonzero(with_swap[5][0])
    assert w.size > 0 and not without[5].any()
    assert with_swap[0][0, w].tobytes() == without[0][1, j[w]].tobytes() and with_swap[0][1, j[w]].tobytes() == without[0][0, w].tobytes()
    assert with_swap[2][0, w].tobytes() == without[2][1, j[w]].tobytes() and with_swap[2][1, j[w]].tobytes() == without[2][0, w].tobytes()
    assert (with_swap[0][0, w][:, 64:] != without[0][0, w][:, 64:]).all()          # every late coordinate changed hands
    rest = np.setdiff1d(np.arange(8), w)
    assert with_swap[0][0, rest].tobytes() == without[0][0, rest].tobytes() and with_swap[0][1, j[rest]].tobytes() == without[0][1, j[rest]].tobytes()


@pytest.mark.parametrize("move", ["stretch", "de"])
def test_bad_starts(many, move):
    """NaN, -0.1 and 1.5 in single coordinates, index 64 among them, in all three rungs: status -1, the row as given, no swap --
    though the reference draws the bad positions as partners of moves and of swaps too, and the others match it."""
    fit, best = many(65)
    U0 = _ball(best, 0.02, (3, 16), np.random.default_rng(8))
    defects = {(0, 1): (64, np.nan), (0, 2): (3, -0.1), (1, 5): (64, 1.5), (1, 9): (64, -0.1), (2, 10): (0, np.nan), (2, 12): (30, 1.5)}
    for (t, w), (k, v) in defects.items():
        U0[t, w, k] = v
    start_logl = _logl(fit)(U0.reshape(48, 65)).reshape(3, 16)
    U, theta, L, status, naccept, nswap, CU, CL = _against_reference(fit, U0, LADDERS[3], 12, 1, 1, move, seed=21, chain_temps=3)
    bad = np.zeros((3, 16), dtype=bool)
    for t, w in defects:
        bad[t, w] = True
    assert (status[bad] == -1).all() and (status[~bad] == 0).all() and not naccept[bad].any() and naccept[~bad].sum() > 0
    assert not nswap[bad[:2]].any() and nswap[~bad[:2]].sum() > 0
    assert np.array_equal(U[bad], U0[bad], equal_nan=True) and L[bad].tobytes() == start_logl[bad].tobytes()
    assert np.array_equal(CU[:, bad], np.broadcast_to(U0[bad], (12, 6, 65)), equal_nan=True)
    assert CL[:, bad].tobytes() == np.broadcast_to(start_logl[bad], (12, 6)).tobytes()


# ---- values as values ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", ["stretch", "de"])
def test_a_vetoed_trial_is_never_accepted_at_any_rung(move):
    """The veto fitter of test_gpu_ens.py (two thirds of uniform draws have logL = -inf) under a ladder that ends at beta = 0,
    where 0 (-inf) is NaN: no -inf trial is accepted at any rung, and no swap brings one in."""
    with mcalf_amd.als_fitter(None, Asymmlike=True, gauss_cdf=[50, 10, 5], **tiny_problem(64)) as fit:
        draws = np.random.default_rng(3).random((1024, fit.ndim))
        L0 = _logl(fit)(draws)
        assert np.isneginf(L0).any() and np.isfinite(L0).sum() >= 192
        U0 = draws[np.flatnonzero(np.isfinite(L0))[:192]].reshape(3, 64, fit.ndim).copy()
        seen = []

        def logl(U):
            out = _logl(fit)(U)
            seen.append(out)
            return out
        U, theta, L, status, naccept, nswap, CU, CL = _against_reference(fit, U0, LADDERS[3], 12, 1, 1, move, seed=4, logl=logl)
        trials = np.stack(seen[1:]).reshape(24, 3, 32)
        for t in range(3):
            assert np.isneginf(trials[:, t]).any() and np.isfinite(trials[:, t]).any()      # some trial rows of every rung are vetoed
        assert np.isfinite(L).all() and np.isfinite(CL).all() and (naccept.sum(axis=1) > 0).all() and nswap.sum() > 0


# ---- invariance ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", ["stretch", "de"])
def test_results_do_not_depend_on_entry_stream_device_count_or_continuation(tiny, move):
    fit, best = tiny
    T, betas = 3, LADDERS[3]
    U0 = _ball(best, 0.1, (T, 130), np.random.default_rng(6))
    U0[1, 7, 2] = 2.0                                                            # a bad start among them
    kw = dict(thin=2, swap_every=3, move=move, seed=4)
    ref = fit.tempered_batch(U0, betas, 10, **kw)
    assert ref[3][1, 7] == -1 and 0 < ref[4].sum() < 10 * 130 * T and 0 < ref[5].sum() < _drawn(10, 3, T, 130).sum()
    assert ref[2].tobytes() == _logl(fit)(ref[0].reshape(-1, fit.ndim)).tobytes()
    assert ref[6].shape == (5, 1, 130, fit.ndim) and ref[7].shape == (5, T, 130)
    assert ref[6][-1, 0].tobytes() == ref[0][0].tobytes() and ref[7][-1].tobytes() == ref[2].tobytes()
    assert _same(ref, fit.tempered_batch(U0, betas, 10, **kw))                    # two calls
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    for stream, theta, chain in ((None, True, True), (side, True, True), (side, False, False)):
        rc, dev = _device_call(fit, U0, betas, 10, 2, 3, move, seed=4, stream=stream, theta=theta, chain=chain)
        keep = [k for k in range(8) if (theta or k != 1) and (chain or k < 6)]
        assert rc == 0 and _same([dev[k] for k in keep], [ref[k] for k in keep])
    # the chain keeps what it is asked for: no rung's rows, the cold rung's, every rung's; logL of every rung always
    for chain_temps in (0, 1, T):
        got = fit.tempered_batch(U0, betas, 10, chain_temps=chain_temps, **kw)
        assert got[6].shape == (5, chain_temps, 130, fit.ndim) and _same(got[:6] + got[7:], ref[:6] + ref[7:])
        assert np.ascontiguousarray(got[6][:, :min(chain_temps, 1)]).tobytes() == (ref[6].tobytes() if chain_temps else b"")
        rc, dev = _device_call(fit, U0, betas, 10, 2, 3, move, seed=4, chain_temps=chain_temps, stream=side)
        assert rc == 0 and _same(dev, got)
    everything = fit.tempered_batch(U0, betas, 10, chain_temps=T, **kw)
    assert everything[6][-1].tobytes() == ref[0].tobytes()
    # continuation: 4 iterations, then 6 more from the returned walkers (rounds 0, 1, 2 follow iterations 2, 5 and 8)
    a = fit.tempered_batch(U0, betas, 4, **kw)
    b = fit.tempered_batch(a[0], betas, 6, first_iter=4, **kw)
    assert _same(ref[:3], b[:3]) and np.array_equal(ref[4], a[4] + b[4]) and np.array_equal(ref[5], a[5] + b[5]) and a[5].any() and b[5].any()
    assert ref[6].tobytes() == np.concatenate([a[6], b[6]]).tobytes() and ref[7].tobytes() == np.concatenate([a[7], b[7]]).tobytes()
    # another seed, another first iteration or another swap period is another run
    assert not _same(ref[:1], fit.tempered_batch(U0, betas, 10, **dict(kw, seed=5))[:1])
    assert not _same(ref[:1], fit.tempered_batch(U0, betas, 10, first_iter=1, **kw)[:1])
    assert not _same(ref[:1], fit.tempered_batch(U0, betas, 10, **dict(kw, swap_every=1))[:1])
    with mcalf_amd.als_fitter(None, device=[0, 0], **tiny_problem(64)) as multi:
        assert _same(ref, multi.tempered_batch(U0, betas, 10, **kw))
        rc, _ = _device_call(multi, U0, betas, 2, 1, 1, move)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in multi._lib.mcalf_last_error(multi._ctx)


# ---- the evidence and the posterior end to end -----------------------------------------------------------------------------------

NTEMPS, BETA_MIN, WALKERS, BURN, KEPT, NBATCH = 16, 1e-4, 64, 300, 1500, 20


@pytest.fixture(scope="module")
def quadrature():
    """(kwargs, [ln Z, mean and variance of the three continuous cube coordinates] by the midpoint rule with 96^3 nodes, the
    same with 64^3 nodes), evaluated with the C oracle once per module.  As in test_gpu_ens.py's fixture the nodes cover the box
    of +- 10 standard deviations around the posterior mean (both from a first 64^3 pass over the whole cube, whose nodes outside
    the box must hold less than 1e-12 of the mass); Z is the integral over the cube under its flat prior."""
    from oracle.c_oracle import COracle
    kw = _evidence_problem()
    orc = COracle(problem_from_kwargs(kw), threads=8)
    b = workloads.bounds_of(kw)
    lo, hi = b.min(axis=1), b.max(axis=1)

    def grid(m, a, c):
        axes = [a[k] + (np.arange(m) + 0.5) / m * (c[k] - a[k]) for k in range(3)]
        g = np.stack(np.meshgrid(*axes, indexing="ij"), axis=-1).reshape(-1, 3)
        P = np.empty((g.shape[0], 4))
        P[:, 0] = 1.0
        P[:, 1:] = g * (hi[1:] - lo[1:]) + lo[1:]
        return g, orc.loglike_batch(P)

    def moments(g, ll):
        w = np.exp(ll - ll.max())
        w /= w.sum()
        mean = (w[:, None] * g).sum(axis=0)
        return mean, (w[:, None] * (g - mean) ** 2).sum(axis=0), w

    def summary(m, a, c):
        g, ll = grid(m, a, c)
        return (float(np.logaddexp.reduce(ll) - 3.0 * np.log(m) + np.log(c - a).sum()),) + moments(g, ll)[:2]

    g, ll = grid(64, np.zeros(3), np.ones(3))
    mean, var, w = moments(g, ll)
    a, c = np.clip(mean - 10.0 * np.sqrt(var), 0.0, 1.0), np.clip(mean + 10.0 * np.sqrt(var), 0.0, 1.0)
    assert w[((g < a) | (g > c)).any(axis=1)].sum() < 1e-12
    return kw, summary(96, a, c), summary(64, a, c)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_tempering_finds_the_evidence_and_the_posterior_moments(quadrature, seed, tmp_path):
    """`default_ladder(16, 1e-4)` (across the prior logL ranges over -5306 .. 112, so the last real rung has to be that hot), 64
    walkers per rung from uniform starts, 300 iterations of burn-in, 1500 kept, a swap round after every iteration, the stretch
    move; `logZ_stepping_stone(20)`.
    ln Z within 5 of its own standard errors (about 0.02) of the 96^3 quadrature, 102.8768, whose 64^3 value must agree to a
    fifth of a standard error; every mean and variance of the three continuous cube coordinates of the cold rung within 5
    batch-means standard errors of the quadrature, whose two values must agree likewise.  The thermodynamic-integration value
    is printed and not asserted: its trapezoid bias over this ladder is about -0.5.
    A numpy tempering of the same structure (other words, independent proposal streams per rung) over the C oracle, this
    configuration, seeds 0, 1, 2: stepping-stone deviations +0.37, -1.53, +1.05 standard errors, cold acceptance 0.55, swap
    fractions 0.56 .. 0.97.  pt_reference alone over the C oracle (these words, burn-in, length, walkers and seeds), deviations
    in standard errors (ln Z | means | variances; the 96^3 and 64^3 quadratures differ by 1.5e-11 in ln Z):
        seed 0   +2.00 |  0.06 -0.01 -0.47 |  1.41 -1.80 -1.23
        seed 1   -0.46 | -2.08 -0.64 -0.89 |  0.32 -0.69  1.39
        seed 2   -0.32 |  0.75  1.22 -0.36 | -0.40  1.96 -1.26
    Measured on an MI355X (this test): the same figures to the digits shown (the device's logL differs from the oracle's in
    the last bits, and no decision of these runs fell between the two); ln Z 102.9190 +- 0.0211, 102.8675 +- 0.0201 and
    102.8682 +- 0.0268 against 102.8768; thermodynamic integration -0.493, -0.549, -0.561 off; acceptance 0.55 in the cold rungs
    falling to 0.37 at the prior, swap fractions 0.56 .. 0.97."""
    kw, (qz, qmean, qvar), (cz, cmean, cvar) = quadrature
    with mcalf_amd.als_fitter(None, **kw) as fit:
        res = fit.tempered_sample(WALKERS, KEPT, betas=tempering.default_ladder(NTEMPS, BETA_MIN), burn=BURN, seed=seed)
        assert res.logL.shape == (KEPT, NTEMPS, WALKERS) and res.cube.shape == (KEPT, WALKERS, 4) and (res.status == 0).all()
        lnz, err = res.logZ_stepping_stone(NBATCH)
        print(f"seed {seed}: ln Z {lnz:.4f} +- {err:.4f}, quadrature {qz:.4f}: {(lnz - qz) / err:+.2f} standard errors; quadrature 96^3 - 64^3 "
              f"{qz - cz:+.5f} ({abs(qz - cz) / err:.3f} standard errors); thermodynamic integration {res.logZ_ti():.4f} ({res.logZ_ti() - qz:+.3f})")
        print(f"acceptance per rung {np.round(res.accept_frac, 3)}, swap fractions {np.round(res.swap_frac, 3)}")
        assert abs(qz - cz) < 0.2 * err
        assert abs(lnz - qz) <= 5.0 * err
        cold = res.cold()
        assert np.array_equal(cold.theta[-1], fit.scale_cube_batch(cold.cube[-1])) and np.array_equal(cold.last, res.last[0])
        assert cold.logL.tobytes() == _logl(fit)(cold.cube.reshape(-1, 4)).tobytes()
        x = cold.cube[:, :, 1:]
        for name, series, want, coarse in (("mean", x.mean(axis=1), qmean, cmean), ("variance", ((x - qmean) ** 2).mean(axis=1), qvar, cvar)):
            se = ensemble.batch_means_se(series, NBATCH)
            dev = (series.mean(axis=0) - want) / se
            print(f"seed {seed}: {name} {series.mean(axis=0)}, quadrature {want}: deviations {np.round(dev, 2)} standard errors; "
                  f"quadrature 96^3 - 64^3 over a standard error {np.round(np.abs(want - coarse) / se, 4)}")
            assert (np.abs(want - coarse) < 0.2 * se).all()
            assert (np.abs(dev) <= 5.0).all()
        ll, th = cold.flat()
        assert ll.shape == (KEPT * WALKERS,) and th.shape == (KEPT * WALKERS, 4)
        ll, th = ll[::256], np.ascontiguousarray(th[::256])
        path = str(tmp_path / "run_equal_weights.txt")
        write_equal_weights(path, ll, th)
        assert np.loadtxt(path, ndmin=2).shape == (ll.size, 2 + fit.ndim)
        mean, var, Q, nvalid = fit.model_band_batch(th)[:4]
        assert np.isfinite(mean).all() and (nvalid == ll.size).all()
        assert np.isfinite(np.asarray(fit.eqw_batch(th)[0])).all()
