"""GPU: the ensemble sampler (mcalf_ensemble_batch[_device]) against the numpy restatement tests/ens_reference.py with
logL = als_fitter.loglike_cube_batch (the existing entry: every decision sees the same bits): U by value (the sign of a zero
may differ), logL and the chain's logL by bytes, naccept and status equal -- no tolerance.  Then its invariance under entry,
stream, device count and continuation, the uniformity of a flat target's walkers, and the posterior moments of a
three-parameter problem end to end against a quadrature of the C oracle.  Every case is at most 2048 walkers and 300 pixels."""
import ctypes as C

import numpy as np
import pytest
import torch

import ens_reference as er
import many_components as mc
import mcalf_amd
from cases import problem_from_kwargs, tiny_problem
from mcalf_amd import _lib, ensemble, workloads
from mcalf_amd.routines.hires_fitter import write_equal_weights
from test_ens_reference import FLAT_ITERS, FLAT_SEED, KS_BAR, flat_start, ks_distances
from test_gpu_fit import _civ
from test_gpu_ns import _evidence_problem

pytestmark = pytest.mark.gpu

MOVES = {"stretch": er.STRETCH, "de": er.DE}


def _logl(fit):
    return lambda U: fit.loglike_cube_batch(U, return_theta=False)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _device_call(fit, U0, nsteps, thin, move, seed=0, first_iter=0, scale=None, stream=None, theta=True, chain=True):
    """mcalf_ensemble_batch_device on torch tensors: rc and (U, theta, logL, status, naccept, CU, CL) as numpy arrays."""
    n, ndim = U0.shape
    scale = er.default_scale(MOVES[move], ndim) if scale is None else scale
    opts = _lib.mcalf_ens_opts(nsteps, thin, MOVES[move], 0, scale, seed, first_iter)
    nkeep = nsteps // thin
    dU0 = torch.from_numpy(np.ascontiguousarray(U0)).cuda()
    dU, dT = (torch.full(U0.shape, -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    dL = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    dS, dN = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(2))
    dCU = torch.full((nkeep, n, ndim), -7.0, dtype=torch.float64, device="cuda")
    dCL = torch.full((nkeep, n), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream() if stream is None else stream
    stream.wait_stream(torch.cuda.current_stream())
    rc = fit._lib.mcalf_ensemble_batch_device(fit._ctx, dU0.data_ptr(), n, C.addressof(opts), dU.data_ptr(), dT.data_ptr() if theta else None,
                                              dL.data_ptr(), dS.data_ptr(), dN.data_ptr(), dCU.data_ptr() if chain else None,
                                              dCL.data_ptr() if chain else None, C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, tuple(t.cpu().numpy() for t in (dU, dT, dL, dS, dN, dCU, dCL))


def _against_reference(fit, U0, nsteps, thin, move, seed, first_iter=0, scale=None, logl=None):
    """The host entry against ens_reference; theta is the prior transform of U, logL the cube entry's value of U and the last
    chain slot the final state when thin divides nsteps."""
    got = fit.ensemble_batch(U0, nsteps, thin=thin, move=move, scale=scale, seed=seed, first_iter=first_iter)
    U, theta, L, status, naccept, CU, CL = got
    rU, rL, rs, rn, rCU, rCL = er.ensemble(logl or _logl(fit), U0, nsteps, thin, MOVES[move], scale, seed, first_iter)
    assert np.array_equal(status, rs) and np.array_equal(naccept, rn)
    assert np.array_equal(U, rU, equal_nan=True)
    assert L.tobytes() == rL.tobytes()
    assert CU.shape == rCU.shape and np.array_equal(CU, rCU, equal_nan=True)
    assert CL.tobytes() == rCL.tobytes()
    assert L.tobytes() == _logl(fit)(U).tobytes()
    assert np.array_equal(theta, fit.scale_cube_batch(U), equal_nan=True)
    if nsteps >= thin and nsteps % thin == 0:
        assert np.array_equal(CU[-1], U, equal_nan=True) and CL[-1].tobytes() == L.tobytes()
    assert (naccept[status == -1] == 0).all() and (naccept <= nsteps).all() and (naccept >= 0).all()
    return got


def _ball(centre, half, n, rng):
    return np.clip(centre + half * (2.0 * rng.random((n, centre.size)) - 1.0), 0.0, 1.0)


# ---- the ndim-4 problem ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    """(fit, the best of 256 uniform points of the cube) of cases.tiny_problem(64)."""
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        draws = np.random.default_rng(1).random((256, fit.ndim))
        yield fit, draws[np.nanargmax(_logl(fit)(draws))]


@pytest.mark.parametrize("thin", [1, 5])
@pytest.mark.parametrize("move", ["stretch", "de"])
@pytest.mark.parametrize("n", [4, 6, 128, 130])
def test_trajectories(tiny, n, move, thin):
    """Halves of 2, 3, 64 and 65 walkers: the smallest DE partner arithmetic, and a half that crosses one wave."""
    fit, best = tiny
    U0 = _ball(best, 0.1, n, np.random.default_rng(n))
    U, theta, L, status, naccept, CU, CL = _against_reference(fit, U0, 12, thin, move, seed=n + thin)
    assert CU.shape == (12 // thin, n, fit.ndim) and (status == 0).all()
    assert 0 < naccept.sum() < 12 * n                       # moves are both accepted and rejected
    assert ((U >= 0.0) & (U <= 1.0)).all()


def test_no_step_no_chain_and_no_walker(tiny):
    fit, best = tiny
    U0 = _ball(best, 0.1, 6, np.random.default_rng(0))
    U, theta, L, status, naccept, CU, CL = _against_reference(fit, U0, 0, 1, "stretch", seed=1)
    assert U.tobytes() == U0.tobytes() and CU.shape == (0, 6, fit.ndim) and not naccept.any()
    short = _against_reference(fit, U0, 3, 5, "de", seed=1)                       # thin above nsteps: an empty chain
    assert short[5].shape == (0, 6, fit.ndim)
    none = fit.ensemble_batch(U0, 7, thin=2, chain=False, seed=1)
    kept = fit.ensemble_batch(U0, 7, thin=2, seed=1)
    assert none[5] is None and none[6] is None and _same(none[:5], kept[:5]) and kept[5].shape[0] == 3
    opts = _lib.mcalf_ens_opts(1, 1, 0, 0, 2.0, 0, 0)
    assert fit._lib.mcalf_ensemble_batch(fit._ctx, None, 0, C.addressof(opts), None, None, None, None, None, None, None) == 0
    with pytest.raises(RuntimeError, match="nwalkers must be even"):
        fit.ensemble_batch(U0[:5], 1)
    with pytest.raises(ValueError):
        fit.ensemble_batch(U0, 1, move="walk")
    big = _lib.mcalf_ens_opts(2 ** 31 - 1, 1, 0, 0, 2.0, 0, 0)                    # 2^31 slots of 6 walkers: far above 4 GiB
    one = np.zeros(1)
    rc = fit._lib.mcalf_ensemble_batch(fit._ctx, U0.ctypes.data, 6, C.addressof(big), U.ctypes.data, None, L.ctypes.data, status.ctypes.data,
                                       naccept.ctypes.data, one.ctypes.data, one.ctypes.data)
    assert rc == _lib.MCALF_ERR_RANGE
    assert f"the largest nkeep for this ensemble is {(4 << 30) // (6 * (fit.ndim + 1) * 8)}".encode() in fit._lib.mcalf_last_error(fit._ctx)


# ---- the ndim-15 problem -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", ["stretch", "de"])
def test_trajectories_two_lines_floated_resolution_and_continuum(move):
    kw, _ = _civ(npix=300, specres=(6.0, 9.0), contval=(0.9, 1.1))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.ndim == 15
        draws = np.random.default_rng(2).random((128, 15))
        best = draws[np.nanargmax(_logl(fit)(draws))]
        U0 = _ball(best, 0.05, 64, np.random.default_rng(4))
        got = _against_reference(fit, U0, 12, 5, move, seed=2 ** 63 + 9, first_iter=2 ** 40)
        assert 0 < got[4].sum() < 12 * 64
        rc, dev = _device_call(fit, U0, 12, 5, move, seed=2 ** 63 + 9, first_iter=2 ** 40)
        assert rc == 0 and _same(dev, got)


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
def test_trajectories_where_a_lane_owns_several_coordinates(many, ndim, move):
    fit, best = many(ndim)
    U0 = _ball(best, 0.02, 8, np.random.default_rng(ndim))
    got = _against_reference(fit, U0, 12, 1, move, seed=ndim)
    assert got[4].sum() > 0 and (np.abs(got[0] - U0)[:, 64:].max(axis=0) > 0.0).all()      # every late coordinate moved in some walker


@pytest.mark.parametrize("move", ["stretch", "de"])
@pytest.mark.parametrize("ndim", [65, 129])
def test_a_proposal_that_leaves_the_cube_in_a_late_coordinate_only(many, ndim, move):
    """Walker 0's first proposal is outside the cube in the last coordinate alone (index 64 or 128, asserted on the reference's
    raw proposal), so it is rejected whatever its logL; the control differs in that coordinate of walker 0 and of its partners
    alone, and there the proposal is inside.  A kernel that tested the first 64 coordinates only would evaluate the outside
    point and decide on its logL."""
    fit, best = many(ndim)
    k, mv = ndim - 1, MOVES[move]
    scale = er.default_scale(mv, ndim)
    U0 = _ball(np.clip(best, 0.1, 0.9), 0.005, 8, np.random.default_rng(5))       # (away from the faces: nothing else leaves the cube)
    # a half-step number whose draw suits the construction: z > 1.05 for the stretch move (any for DE)
    first = next(i for i in range(64) if mv == er.DE or (((scale - 1.0) * _xi(2 * i, 0, 7) + 1.0) ** 2) / scale > 1.05)
    partners = er.propose(U0, 0, 2 * first, mv, scale, 7)[4][0]
    ctrl = U0.copy()
    ctrl[:, k] = 0.5
    late = ctrl.copy()
    if mv == er.STRETCH:                                     # y = x_j + z (x - x_j) with z > 1.05: beyond 1
        late[0, k], late[partners[0], k] = 0.99, 0.01
    else:                                                    # y = x + gamma (x_j1 - x_j2)
        late[0, k], late[partners[0], k], late[partners[1], k] = 0.99, 0.99, 0.01
    for U, outside in ((late, True), (ctrl, False)):
        Y, _, _, inside, _, raw = er.propose(U, 0, 2 * first, mv, scale, 7)
        bad = np.flatnonzero(~((raw[0] >= 0.0) & (raw[0] <= 1.0)))
        assert bad.tolist() == ([k] if outside else []) and k >= 64 and inside[0] == (not outside)
        got = _against_reference(fit, U, 1, 1, move, seed=7, first_iter=first)
        if outside:
            assert got[4][0] == 0 and got[0][0].tobytes() == U[0].tobytes()
        _against_reference(fit, U, 12, 5, move, seed=7, first_iter=first)


def _xi(s, w, seed):
    return float((er.words(s, [w], seed)[0, 1] >> np.uint64(11)).astype(np.float64) * 2.0 ** -53)


@pytest.mark.parametrize("move", ["stretch", "de"])
def test_bad_starts(many, move):
    """NaN, -0.1 and 1.5 in single coordinates, index 64 among them: status -1, the row as given; the others match the
    reference, which draws the bad walkers as partners too."""
    fit, best = many(65)
    U0 = _ball(best, 0.02, 16, np.random.default_rng(8))
    defects = {1: (64, np.nan), 2: (3, -0.1), 5: (64, 1.5), 9: (64, -0.1), 10: (0, np.nan), 12: (30, 1.5)}
    for w, (k, v) in defects.items():
        U0[w, k] = v
    start_logl = _logl(fit)(U0)
    U, theta, L, status, naccept, CU, CL = _against_reference(fit, U0, 12, 1, move, seed=21)
    bad = np.array(sorted(defects))
    good = np.setdiff1d(np.arange(16), bad)
    assert (status[bad] == -1).all() and (status[good] == 0).all() and not naccept[bad].any() and naccept[good].sum() > 0
    assert np.array_equal(U[bad], U0[bad], equal_nan=True) and L[bad].tobytes() == start_logl[bad].tobytes()
    assert np.array_equal(CU[:, bad], np.broadcast_to(U0[bad], (12, bad.size, 65)), equal_nan=True)


# ---- values as values ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", ["stretch", "de"])
def test_a_vetoed_trial_is_never_accepted_from_a_finite_point(move):
    """Veto thresholds of 10 pixels above 4 sigma and 5 above 5 sigma: by the numpy oracle two thirds of these 512 uniform
    draws are vetoed (logL = -inf) and a third is finite."""
    with mcalf_amd.als_fitter(None, Asymmlike=True, gauss_cdf=[50, 10, 5], **tiny_problem(64)) as fit:
        draws = np.random.default_rng(3).random((512, fit.ndim))
        L0 = _logl(fit)(draws)
        assert np.isneginf(L0).any() and np.isfinite(L0).sum() >= 64
        U0 = draws[np.flatnonzero(np.isfinite(L0))[:64]].copy()
        seen = []

        def logl(U):
            out = _logl(fit)(U)
            seen.append(out)
            return out
        U, theta, L, status, naccept, CU, CL = _against_reference(fit, U0, 12, 1, move, seed=4, logl=logl)
        trials = np.concatenate(seen[1:])
        assert np.isneginf(trials).any() and np.isfinite(trials).any()         # some trial rows are vetoed
        assert np.isfinite(L).all() and np.isfinite(CL).all() and naccept.sum() > 0


# ---- invariance ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", ["stretch", "de"])
def test_results_do_not_depend_on_entry_stream_device_count_or_continuation(tiny, move):
    fit, best = tiny
    U0 = _ball(best, 0.1, 130, np.random.default_rng(6))
    U0[7, 2] = 2.0                                                               # a bad start among them
    ref = fit.ensemble_batch(U0, 10, thin=2, move=move, seed=4)
    assert ref[3][7] == -1 and 0 < ref[4].sum() < 10 * 130
    assert np.array_equal(ref[1], fit.scale_cube_batch(ref[0])) and ref[2].tobytes() == _logl(fit)(ref[0]).tobytes()
    assert ref[5][-1].tobytes() == ref[0].tobytes() and ref[6][-1].tobytes() == ref[2].tobytes()
    assert _same(ref, fit.ensemble_batch(U0, 10, thin=2, move=move, seed=4))     # two calls
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    for stream, theta, chain in ((None, True, True), (side, True, True), (side, False, False)):
        rc, dev = _device_call(fit, U0, 10, 2, move, seed=4, stream=stream, theta=theta, chain=chain)
        keep = [k for k in range(7) if (theta or k != 1) and (chain or k < 5)]
        assert rc == 0 and _same([dev[k] for k in keep], [ref[k] for k in keep])
    # continuation: 4 iterations, then 6 more from the returned walkers
    a = fit.ensemble_batch(U0, 4, thin=2, move=move, seed=4)
    b = fit.ensemble_batch(a[0], 6, thin=2, move=move, seed=4, first_iter=4)
    assert _same(ref[:3], b[:3]) and np.array_equal(ref[4], a[4] + b[4])
    assert ref[5].tobytes() == np.concatenate([a[5], b[5]]).tobytes() and ref[6].tobytes() == np.concatenate([a[6], b[6]]).tobytes()
    # another seed or another first iteration is another run
    assert not _same(ref[:1], fit.ensemble_batch(U0, 10, thin=2, move=move, seed=5)[:1])
    assert not _same(ref[:1], fit.ensemble_batch(U0, 10, thin=2, move=move, seed=4, first_iter=1)[:1])
    with mcalf_amd.als_fitter(None, device=[0, 0], **tiny_problem(64)) as multi:
        assert _same(ref, multi.ensemble_batch(U0, 10, thin=2, move=move, seed=4))
        rc, _ = _device_call(multi, U0, 2, 1, move)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in multi._lib.mcalf_last_error(multi._ctx)


# ---- a flat target ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", ["stretch", "de"])
def test_a_flat_target_ends_uniform_and_equals_the_reference(move):
    """Errors of 1e30 make logL one constant (asserted), so the reference needs no likelihood call: 2048 walkers from
    test_ens_reference.py's ball, its iteration count and seed; the final positions are the reference's exactly."""
    kw = tiny_problem(64)
    wl, flux, _ = kw["spectrum"]
    with mcalf_amd.als_fitter(None, **dict(kw, spectrum=(wl, flux, np.full(64, 1e30)))) as fit:
        nd = fit.ndim
        U0 = flat_start(nd)
        const = _logl(fit)(np.random.default_rng(0).random((512, nd)))
        assert np.isfinite(const[0]) and (const == const[0]).all()
        U, theta, L, status, naccept, CU, CL = fit.ensemble_batch(U0, FLAT_ITERS[nd], thin=FLAT_ITERS[nd], move=move, seed=FLAT_SEED)
        assert (L == const[0]).all() and (CL == const[0]).all() and (status == 0).all()
    ref = er.ensemble(lambda Y: np.full(Y.shape[0], const[0]), U0, FLAT_ITERS[nd], FLAT_ITERS[nd], MOVES[move], seed=FLAT_SEED)
    assert np.array_equal(U, ref[0]) and np.array_equal(naccept, ref[3]) and np.array_equal(CU[0], U)
    d = ks_distances(U)
    print(f"move {move}: largest KS distance {d.max():.4f} (bar {KS_BAR:.4f}), acceptance {naccept.mean() / FLAT_ITERS[nd]:.3f}")
    assert (d < KS_BAR).all()


# ---- the posterior end to end ------------------------------------------------------------------------------------------------------

BURN, KEPT, NBATCH = 500, 4000, 20


@pytest.fixture(scope="module")
def posterior():
    """(kwargs, mean and variance of the three continuous cube coordinates by the midpoint rule with 96^3 nodes, the same with
    64^3 nodes), evaluated with the C oracle once per module.  The nodes cover the box of +- 10 standard deviations around the
    posterior mean (both from a first 64^3 pass over the whole cube, whose nodes outside the box must hold less than 1e-12 of
    the mass): the posterior's standard deviation in the column density is 0.008 of the cube, below the spacing of 96 nodes
    over the whole of it, which would leave the quadrature 1e-5 off in that variance -- many standard errors of the run."""
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

    g, ll = grid(64, np.zeros(3), np.ones(3))
    mean, var, w = moments(g, ll)
    a, c = np.clip(mean - 10.0 * np.sqrt(var), 0.0, 1.0), np.clip(mean + 10.0 * np.sqrt(var), 0.0, 1.0)
    assert w[((g < a) | (g > c)).any(axis=1)].sum() < 1e-12
    return kw, moments(*grid(96, a, c))[:2], moments(*grid(64, a, c))[:2]


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("move", ["stretch", "de"])
def test_the_sampler_finds_the_posterior_moments(posterior, move, seed, tmp_path):
    """256 walkers from a ball of half-width 0.05 around the `maximize_batch` optimum, 500 iterations of burn-in, 4000 kept, 20
    batches of 200 iterations (the autocorrelation times of the ensemble means are 30 .. 90 iterations for the stretch move, 10 .. 20 for DE).
    Every mean and variance of the three continuous cube coordinates within 5 batch-means standard errors of the quadrature,
    whose 96^3 and 64^3 values must agree to a fifth of each standard error (they agree to 1e-13).
    The reference alone over the C oracle, same burn-in, length, walkers and seeds, started at the quadrature's best node,
    deviations in standard errors (means | variances):
        stretch  seed 0  -0.46  0.12 -0.64 |  0.10 -0.57 -0.60      DE  seed 0   2.00  0.34  2.00 |  0.89  1.57 -0.91
                 seed 1   0.93  0.47  0.27 |  0.54  0.51 -1.04          seed 1   1.51 -0.77 -2.89 |  0.39 -1.28 -1.90
                 seed 2  -0.36 -0.11  2.98 | -0.16  0.36  0.59          seed 2   0.36 -0.68  1.01 | -0.05 -1.05 -0.06
    Measured on an MI355X (this test): the largest of the 36 deviations is 2.35 standard errors; acceptance 0.55 (stretch) and
    0.27 (DE)."""
    kw, (qmean, qvar), (cmean, cvar) = posterior
    b = workloads.bounds_of(kw)
    lo, hi = b.min(axis=1), b.max(axis=1)
    wl = kw["spectrum"][0]
    p0 = np.array([[1.0, 13.3, wl[32] / 1548.204 - 1.0 + 3e-5, 15.0]])
    with mcalf_amd.als_fitter(None, **kw) as fit:
        P, _, status, _ = fit.maximize_batch(p0)
        assert status[0] >= 0
        start = np.full(4, 0.5)
        start[1:] = (P[0, 1:] - lo[1:]) / (hi[1:] - lo[1:])
        assert ((start > 0.1) & (start < 0.9)).all()
        res = fit.ensemble_sample(256, KEPT, burn=BURN, thin=1, start=start, ball=0.05, seed=seed, move=move)
        assert res.cube.shape == (KEPT, 256, 4) and (res.status == 0).all()
        assert np.array_equal(res.theta[-1], fit.scale_cube_batch(res.cube[-1])) and np.array_equal(res.last, res.cube[-1])
        x = res.cube[:, :, 1:]
        for name, series, want, coarse in (("mean", x.mean(axis=1), qmean, cmean), ("variance", ((x - qmean) ** 2).mean(axis=1), qvar, cvar)):
            se = ensemble.batch_means_se(series, NBATCH)
            dev = (series.mean(axis=0) - want) / se
            print(f"move {move}, seed {seed}: {name} {series.mean(axis=0)}, quadrature {want}: deviations {np.round(dev, 2)} standard errors; "
                  f"quadrature 96^3 - 64^3 over a standard error {np.round(np.abs(want - coarse) / se, 4)}")
            assert (np.abs(want - coarse) < 0.2 * se).all()
            assert (np.abs(dev) <= 5.0).all()
        print(f"acceptance {res.accept_frac.mean():.3f}, autocorrelation times {np.round(res.autocorr_time(), 1)}")
        ll, th = res.flat()
        assert ll.shape == (KEPT * 256,) and th.shape == (KEPT * 256, 4)
        ll, th = ll[::1024], np.ascontiguousarray(th[::1024])
        path = str(tmp_path / "run_equal_weights.txt")
        write_equal_weights(path, ll, th)
        assert np.loadtxt(path, ndmin=2).shape == (ll.size, 2 + fit.ndim)
        mean, var, Q, nvalid = fit.model_band_batch(th)[:4]
        assert np.isfinite(mean).all() and (nvalid == ll.size).all()
