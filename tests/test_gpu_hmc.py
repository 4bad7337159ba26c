"""GPU: Hamiltonian Monte Carlo (mcalf_hmc_batch[_device], mcalf_amd.hmc) against the numpy restatement tests/hmc_reference.py
with grad = als_fitter.loglike_grad_batch on als_fitter.scale_cube_batch(U) (the existing entries: every kernel decision sees
the same bits): U by value (the sign of a zero may differ), logL and the chain's logL by bytes, status, naccept and ndead
equal -- no tolerance.  Then the walls and the dead trajectories, the Gaussian prior's gradient, the frozen coordinates, the
invariances, the refused starts and arguments, and the posterior moments of a three-parameter problem end to end against the
quadrature of the C oracle that test_gpu_ens.py applies to the ensemble.  Every case is at most 130 walkers and 300 pixels."""
import ctypes as C

import numpy as np
import pytest
import torch

import hmc_reference as hr
import many_components as mc
import mcalf_amd
from cases import tiny_problem
from mcalf_amd import _lib, ensemble, hmc, workloads
from test_gpu_ens import posterior  # noqa: F401  (the quadrature fixture of the ensemble's end-to-end test)
from test_gpu_fit import _civ

pytestmark = pytest.mark.gpu


def _logl(fit):
    return lambda U: fit.loglike_cube_batch(U, return_theta=False)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _ball(centre, half, n, rng):
    return np.clip(centre + half * (2.0 * rng.random((n, centre.size)) - 1.0), 0.0, 1.0)


def _problem(fit):
    """The restatement's view of the fitter: its box and slot, the library's own mu, sigma, c, its cube transform."""
    return hr.Problem(fit._lo, fit._hi, fit.startind, True, fit.gauss_prior, transform=fit.scale_cube_batch)


def _grad(fit, seen=None):
    def grad(theta):
        out = fit.loglike_grad_batch(theta)
        if seen is not None:
            seen.append(out[0].copy())
        return out
    return grad


def _device_call(fit, U0, nsteps, eps, nleap, scale, thin=1, jitter=0.1, seed=0, first_iter=0, wid=None, stream=None, theta=True, chain=True):
    """mcalf_hmc_batch_device on torch tensors: rc and (U, theta, logL, status, naccept, ndead, CU, CL) as numpy arrays."""
    n, ndim = U0.shape
    opts = _lib.mcalf_hmc_opts(nsteps, thin, nleap, 0, eps, jitter, seed, first_iter)
    nkeep = nsteps // thin
    scale = np.ascontiguousarray(scale, dtype=float)
    dU0 = torch.from_numpy(np.ascontiguousarray(U0)).cuda()
    dU, dT = (torch.full(U0.shape, -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    dL = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    dS, dN, dD = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    dCU = torch.full((nkeep, n, ndim), -7.0, dtype=torch.float64, device="cuda")
    dCL = torch.full((nkeep, n), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream() if stream is None else stream
    stream.wait_stream(torch.cuda.current_stream())
    rc = fit._lib.mcalf_hmc_batch_device(fit._ctx, dU0.data_ptr(), n, scale.ctypes.data, None if wid is None else wid.ctypes.data, C.addressof(opts),
                                         dU.data_ptr(), dT.data_ptr() if theta else None, dL.data_ptr(), dS.data_ptr(), dN.data_ptr(), dD.data_ptr(),
                                         dCU.data_ptr() if chain else None, dCL.data_ptr() if chain else None, C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, tuple(t.cpu().numpy() for t in (dU, dT, dL, dS, dN, dD, dCU, dCL))


def _against_reference(fit, U0, nsteps, eps, nleap, scale, thin=1, jitter=0.1, seed=0, first_iter=0, wid=None, trace=None, seen=None):
    """The host entry against hmc_reference; theta is the prior transform of U, logL the cube entry's value of U and the last
    chain slot the final state when thin divides nsteps."""
    got = hmc.hmc_batch(fit, U0, nsteps, eps, nleap, scale=scale, jitter=jitter, thin=thin, seed=seed, first_iter=first_iter, walker_ids=wid)
    U, theta, L, status, naccept, ndead, CU, CL = got
    rU, rL, rs, rn, rd, rCU, rCL = hr.hmc(_problem(fit), _grad(fit, seen), U0, nsteps, eps, nleap, scale, jitter, thin, seed, first_iter, wid, trace)
    assert np.array_equal(status, rs) and np.array_equal(naccept, rn) and np.array_equal(ndead, rd)
    assert np.array_equal(U, rU, equal_nan=True)
    assert L.tobytes() == rL.tobytes()
    assert CU.shape == rCU.shape and np.array_equal(CU, rCU, equal_nan=True)
    assert CL.tobytes() == rCL.tobytes()
    assert L.tobytes() == _logl(fit)(U).tobytes()
    assert np.array_equal(theta, fit.scale_cube_batch(U), equal_nan=True)
    if nsteps >= thin and nsteps % thin == 0:
        assert np.array_equal(CU[-1], U, equal_nan=True) and CL[-1].tobytes() == L.tobytes()
    assert (naccept[status == -1] == 0).all() and (ndead[status == -1] == 0).all()
    assert (naccept >= 0).all() and (ndead >= 0).all() and (naccept + ndead <= nsteps).all()
    return got


# ---- the ndim-4 problem ------------------------------------------------------------------------------------------------------

TINY_SCALE = np.array([1.0, 0.1, 0.1, 0.1])           # (the ncomp slot is frozen whatever its scale)
TINY_EPS = {1: 0.3, 3: 0.2}                            # by nleap: steps at which these 12 iterations both accept and reject


@pytest.fixture(scope="module")
def tiny():
    """(fit, the best of 256 uniform points of the cube) of cases.tiny_problem(64)."""
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        draws = np.random.default_rng(1).random((256, fit.ndim))
        yield fit, draws[np.nanargmax(_logl(fit)(draws))]


@pytest.mark.parametrize("thin", [1, 5])
@pytest.mark.parametrize("nleap", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 65])
def test_trajectories(tiny, n, nleap, thin):
    fit, best = tiny
    U0 = _ball(np.clip(best, 0.2, 0.8), 0.1, n, np.random.default_rng(n))
    U, theta, L, status, naccept, ndead, CU, CL = _against_reference(fit, U0, 12, TINY_EPS[nleap], nleap, TINY_SCALE, thin=thin, seed=n + thin)
    assert CU.shape == (12 // thin, n, fit.ndim) and (status == 0).all()
    print(f"n {n}, nleap {nleap}: accepted {naccept.sum()} of {12 * n}, dead {ndead.sum()}")
    assert 0 < naccept.sum() < 12 * n                       # trajectories are both accepted and rejected
    assert ((U >= 0.0) & (U <= 1.0)).all()


def test_no_step_no_chain_and_no_walker(tiny):
    fit, best = tiny
    U0 = _ball(best, 0.1, 6, np.random.default_rng(0))
    U, theta, L, status, naccept, ndead, CU, CL = _against_reference(fit, U0, 0, 0.2, 2, TINY_SCALE, seed=1)
    assert U.tobytes() == U0.tobytes() and CU.shape == (0, 6, fit.ndim) and not naccept.any() and not ndead.any() and (status == 0).all()
    short = _against_reference(fit, U0, 3, 0.2, 2, TINY_SCALE, thin=5, seed=1)            # thin above nsteps: an empty chain
    assert short[6].shape == (0, 6, fit.ndim)
    none = hmc.hmc_batch(fit, U0, 7, 0.2, 2, scale=TINY_SCALE, thin=2, chain=False, seed=1)
    kept = hmc.hmc_batch(fit, U0, 7, 0.2, 2, scale=TINY_SCALE, thin=2, seed=1)
    assert none[6] is None and none[7] is None and _same(none[:6], kept[:6]) and kept[6].shape[0] == 3
    opts = _lib.mcalf_hmc_opts(1, 1, 1, 0, 0.1, 0.0, 0, 0)
    assert fit._lib.mcalf_hmc_batch(fit._ctx, None, 0, None, None, C.addressof(opts), None, None, None, None, None, None, None, None) == 0
    big = _lib.mcalf_hmc_opts(2 ** 31 - 1, 1, 1, 0, 0.1, 0.0, 0, 0)                       # 2^31 slots of 6 walkers: far above 4 GiB
    one = np.zeros(1)
    rc = fit._lib.mcalf_hmc_batch(fit._ctx, U0.ctypes.data, 6, TINY_SCALE.ctypes.data, None, C.addressof(big), U.ctypes.data, None, L.ctypes.data,
                                  status.ctypes.data, naccept.ctypes.data, ndead.ctypes.data, one.ctypes.data, one.ctypes.data)
    assert rc == _lib.MCALF_ERR_RANGE
    assert f"the largest nkeep for this ensemble is {(4 << 30) // (6 * (fit.ndim + 1) * 8)}".encode() in fit._lib.mcalf_last_error(fit._ctx)


def test_every_argument_check_names_its_argument(tiny):
    """Each refusal comes back as MCALF_ERR_INVALID with the argument's name, and leaves the outputs as they were."""
    fit, best = tiny
    U0 = _ball(best, 0.1, 4, np.random.default_rng(0))
    outs = dict(U=np.full((4, 4), -7.0), logL=np.full(4, -7.0), status=np.full(4, -7, dtype=np.int32), naccept=np.full(4, -7, dtype=np.int32),
                ndead=np.full(4, -7, dtype=np.int32))
    before = {k: v.copy() for k, v in outs.items()}

    def call(n=4, opts=(1, 1, 1, 0, 0.1, 0.1, 0, 0), scale=TINY_SCALE, null=(), has_opts=True, ctx=None):
        o = _lib.mcalf_hmc_opts(*opts)
        arrays = dict(outs, U0=U0, scale=np.ascontiguousarray(scale, dtype=float))       # (alive until the call has returned)
        ptr = {k: (None if k in null else v.ctypes.data) for k, v in arrays.items()}
        ctx = fit if ctx is None else ctx
        rc = ctx._lib.mcalf_hmc_batch(ctx._ctx, ptr["U0"], n, ptr["scale"], None, C.addressof(o) if has_opts else None, ptr["U"], None, ptr["logL"],
                                      ptr["status"], ptr["naccept"], ptr["ndead"], None, None)
        return rc, ctx._lib.mcalf_last_error(ctx._ctx).decode()

    cases = [(dict(has_opts=False), "opts is NULL"), (dict(n=-1), "nwalkers must be >= 0"),
             (dict(opts=(-1, 1, 1, 0, 0.1, 0.1, 0, 0)), "nsteps must be >= 0"), (dict(opts=(1, 0, 1, 0, 0.1, 0.1, 0, 0)), "thin must be >= 1"),
             (dict(opts=(1, 1, 0, 0, 0.1, 0.1, 0, 0)), "nleap must be >= 1"), (dict(opts=(1, 1, 1, 0, 0.0, 0.1, 0, 0)), "eps must be finite and > 0"),
             (dict(opts=(1, 1, 1, 0, -0.1, 0.1, 0, 0)), "eps must be finite and > 0"), (dict(opts=(1, 1, 1, 0, np.inf, 0.1, 0, 0)), "eps must be finite and > 0"),
             (dict(opts=(1, 1, 1, 0, np.nan, 0.1, 0, 0)), "eps must be finite and > 0"), (dict(opts=(1, 1, 1, 0, 0.1, -0.01, 0, 0)), "jitter must be in [0, 1)"),
             (dict(opts=(1, 1, 1, 0, 0.1, 1.0, 0, 0)), "jitter must be in [0, 1)"), (dict(opts=(1, 1, 1, 0, 0.1, np.nan, 0, 0)), "jitter must be in [0, 1)"),
             (dict(scale=[1.0, 0.1, -0.1, 0.1]), "scale[2] must be finite and >= 0"), (dict(scale=[1.0, 0.1, 0.1, np.inf]), "scale[3] must be finite and >= 0"),
             (dict(scale=[np.nan, 0.1, 0.1, 0.1]), "scale[0] must be finite and >= 0")]
    cases += [(dict(null=(name,)), f"{name} is NULL") for name in ("U0", "scale", "U", "logL", "status", "naccept", "ndead")]
    for kw, needle in cases:
        rc, msg = call(**kw)
        assert rc == _lib.MCALF_ERR_INVALID and needle in msg and "mcalf_hmc_batch:" in msg, (kw, msg)
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fresh:                          # no prior box on the device yet
        rc, msg = call(ctx=fresh)
        assert rc == _lib.MCALF_ERR_INVALID and "mcalf_set_prior has not been called" in msg
    assert all(outs[k].tobytes() == before[k].tobytes() for k in outs)
    rc, _ = _device_call(fit, U0, 1, 0.1, 0, TINY_SCALE)
    assert rc == _lib.MCALF_ERR_INVALID and b"mcalf_hmc_batch_device: nleap must be >= 1" in fit._lib.mcalf_last_error(fit._ctx)
    with pytest.raises(ValueError, match="scale must have ndim"):
        hmc.hmc_batch(fit, U0, 1, 0.1, 1, scale=[1.0, 2.0])
    with pytest.raises(ValueError, match="walker_ids must have one entry per walker"):
        hmc.hmc_batch(fit, U0, 1, 0.1, 1, walker_ids=[1, 2])


# ---- walls and deaths ----------------------------------------------------------------------------------------------------------

def test_reflections_and_dead_trajectories(tiny):
    """Starts within 0.02 of a wall in every moving coordinate and a step half as long again as the longest that the interior
    starts of test_trajectories take: the restatement's trace must hold reflections and dead trajectories (a drift that is still
    outside the cube after its one reflection), and the device agrees on all of it."""
    fit, best = tiny
    rng = np.random.default_rng(12)
    U0 = np.where(rng.random((33, 4)) < 0.5, 0.02 * rng.random((33, 4)), 1.0 - 0.02 * rng.random((33, 4)))
    U0[:, 0] = 0.5
    trace = []
    got = _against_reference(fit, U0, 12, 0.3, 3, TINY_SCALE, seed=77, trace=trace)
    reflected = sum(t[3] for t in trace if t[0] == "reflect")
    died = sum(len(t[3]) for t in trace if t[0] == "dead")
    print(f"{reflected} reflections, {died} dead trajectories, accepted {got[4].sum()} of {12 * 33}")
    assert reflected >= 1 and died >= 1 and got[5].sum() == died
    assert ((got[0] >= 0.0) & (got[0] <= 1.0)).all() and (got[3] == 0).all()


# ---- the ndim-15 problem -------------------------------------------------------------------------------------------------------

def test_trajectories_two_lines_floated_resolution_and_continuum():
    kw, _ = _civ(npix=300, specres=(6.0, 9.0), contval=(0.9, 1.1))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.ndim == 15
        draws = np.random.default_rng(2).random((128, 15))
        best = draws[np.nanargmax(_logl(fit)(draws))]
        U0 = _ball(np.clip(best, 0.1, 0.9), 0.05, 64, np.random.default_rng(4))
        scale = np.full(15, 0.05)
        got = _against_reference(fit, U0, 12, 0.02, 3, scale, thin=5, seed=2 ** 63 + 9, first_iter=2 ** 40)
        print(f"accepted {got[4].sum()} of {12 * 64}, dead {got[5].sum()}")
        assert 0 < got[4].sum() < 12 * 64
        side = torch.cuda.Stream()
        assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
        rc, dev = _device_call(fit, U0, 12, 0.02, 3, scale, thin=5, seed=2 ** 63 + 9, first_iter=2 ** 40, stream=side)
        assert rc == 0 and _same(dev, got)


# ---- a lane owns two coordinates -----------------------------------------------------------------------------------------------

def test_trajectories_where_a_lane_owns_two_coordinates():
    kw, truth = mc.many(65)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.ndim == 65
        centre = (truth - fit._lo) / (fit._hi - fit._lo)
        U0 = _ball(centre, 0.01, 4, np.random.default_rng(65))
        scale = np.full(65, 0.01)
        got = _against_reference(fit, U0, 3, 0.02, 2, scale, seed=65)
        print(f"accepted {got[4].sum()} of 12, dead {got[5].sum()}")
        assert got[4].sum() > 0 and (np.abs(got[0] - U0)[:, 64] > 0.0).any()               # the late coordinate moved
        assert (got[0][:, fit.startind] == U0[:, fit.startind]).all()


# ---- the Gaussian prior ----------------------------------------------------------------------------------------------------------

def test_trajectories_under_a_gaussian_prior_and_after_it_is_cleared(tiny):
    fit, best = tiny
    U0 = _ball(np.clip(best, 0.2, 0.8), 0.1, 65, np.random.default_rng(3))
    flat = _against_reference(fit, U0, 12, TINY_EPS[3], 3, TINY_SCALE, thin=5, seed=8)
    mu, sigma = np.zeros(4), np.zeros(4)
    span = fit._hi - fit._lo
    for k in (1, 3):                                             # narrow Gaussians half a width beside the ball's centre
        sigma[k] = 0.05 * span[k]
        mu[k] = fit._lo[k] + best[k] * span[k] + 0.5 * sigma[k]
    fit.set_gauss_prior(mu, sigma)
    try:
        assert _problem(fit).gauss is not None
        under = _against_reference(fit, U0, 12, TINY_EPS[3], 3, TINY_SCALE, thin=5, seed=8)
        assert 0 < under[4].sum() < 12 * 65 and not _same(under[:1], flat[:1])           # the prior's gradient and ratio change the run
    finally:
        fit.clear_gauss_prior()
    assert _same(flat, hmc.hmc_batch(fit, U0, 12, TINY_EPS[3], 3, scale=TINY_SCALE, thin=5, seed=8))


# ---- frozen coordinates ----------------------------------------------------------------------------------------------------------

def test_frozen_coordinates_keep_their_bytes():
    kw, _ = _civ(npix=300, specres=(6.0, 9.0), contval=(0.9, 1.1))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        draws = np.random.default_rng(2).random((128, 15))
        best = draws[np.nanargmax(_logl(fit)(draws))]
        U0 = _ball(np.clip(best, 0.1, 0.9), 0.05, 16, np.random.default_rng(5))
        U0[:, fit.startind] = np.random.default_rng(6).random(16)                         # walkers of different component counts
        scale = np.full(15, 0.05)
        scale[[0, 7]] = 0.0
        U, theta, L, status, naccept, ndead, CU, CL = _against_reference(fit, U0, 8, 0.02, 2, scale, seed=3)
        assert naccept.sum() > 0 and (status == 0).all()
        for k in (0, 7, fit.startind):
            assert U[:, k].tobytes() == U0[:, k].tobytes()
            assert CU[:, :, k].tobytes() == np.broadcast_to(U0[:, k], (8, 16)).tobytes()
        moving = [k for k in range(15) if k not in (0, 7, fit.startind)]
        assert (np.abs(U - U0)[:, moving].max(axis=0) > 0.0).all()


def test_a_coordinate_whose_box_has_no_width_is_frozen():
    """brange = [20, 20]: hi == lo in the last coordinate, whose scale is not 0 -- it keeps its bytes while the others move, and
    the run is the restatement's."""
    with mcalf_amd.als_fitter(None, **dict(tiny_problem(64), brange=[20.0, 20.0])) as fit:
        assert fit._hi[3] == fit._lo[3] and fit._hi[1] > fit._lo[1]
        draws = np.random.default_rng(1).random((256, fit.ndim))
        best = draws[np.nanargmax(_logl(fit)(draws))]
        U0 = _ball(np.clip(best, 0.2, 0.8), 0.1, 16, np.random.default_rng(7))
        U, theta, L, status, naccept, ndead, CU, CL = _against_reference(fit, U0, 8, 0.2, 2, TINY_SCALE, seed=5)
        assert (status == 0).all() and naccept.sum() > 0
        for k in (0, 3):
            assert U[:, k].tobytes() == U0[:, k].tobytes() and CU[:, :, k].tobytes() == np.broadcast_to(U0[:, k], (8, 16)).tobytes()
        assert (np.abs(U - U0)[:, 1:3].max(axis=0) > 0.0).all()
        assert (theta[:, 3] == 20.0).all()


def test_the_driver_under_a_gaussian_prior_carries_lnprior(tiny):
    """`hmc_sample` with a Gaussian set: the kept rows come back with their lnprior (one pass over the transformed rows), logL
    stays the likelihood's, and the walkers gather around the prior's centre in the coordinate that carries it."""
    fit, best = tiny
    span = fit._hi - fit._lo
    mu, sigma = np.zeros(4), np.zeros(4)
    sigma[3], mu[3] = 0.02 * span[3], fit._lo[3] + 0.6 * span[3]
    fit.set_gauss_prior(mu, sigma)
    try:
        start = np.clip(best, 0.2, 0.8)
        start[3] = 0.6
        res = hmc.hmc_sample(fit, 32, 40, burn=40, thin=2, start=start, ball=0.02, seed=1, eps=0.2, nleap=3)
        assert res.cube.shape == (20, 32, 4) and (res.status == 0).all() and res.accept_frac.mean() > 0.0
        flat = res.cube.reshape(-1, 4)
        assert res.lnprior is not None and res.lnprior.reshape(-1).tobytes() == fit.lnprior_batch(res.theta.reshape(-1, 4)).tobytes()
        assert res.logL.reshape(-1).tobytes() == _logl(fit)(flat).tobytes()
        assert np.isfinite(res.lnprior).all() and np.abs(res.cube[:, :, 3] - 0.6).max() < 0.2        # within 10 sigma of the centre
    finally:
        fit.clear_gauss_prior()


# ---- invariances ---------------------------------------------------------------------------------------------------------------

def test_results_do_not_depend_on_entry_stream_batch_order_device_count_or_continuation(tiny):
    fit, best = tiny
    U0 = _ball(np.clip(best, 0.2, 0.8), 0.1, 130, np.random.default_rng(6))
    U0[7, 2] = 2.0                                                               # a refused start among them
    kw = dict(scale=TINY_SCALE, thin=2, seed=4)
    ref = hmc.hmc_batch(fit, U0, 10, TINY_EPS[3], 3, **kw)
    assert ref[3][7] == -1 and 0 < ref[4].sum() < 10 * 130
    assert np.array_equal(ref[1], fit.scale_cube_batch(ref[0])) and ref[2].tobytes() == _logl(fit)(ref[0]).tobytes()
    assert ref[6][-1].tobytes() == ref[0].tobytes() and ref[7][-1].tobytes() == ref[2].tobytes()
    assert _same(ref, hmc.hmc_batch(fit, U0, 10, TINY_EPS[3], 3, **kw))           # two calls
    none = hmc.hmc_batch(fit, U0, 10, TINY_EPS[3], 3, chain=False, **kw)
    assert none[6] is None and none[7] is None and _same(none[:6], ref[:6])
    side = torch.cuda.Stream()
    for stream, theta, chain in ((None, True, True), (side, True, True), (side, False, False)):
        rc, dev = _device_call(fit, U0, 10, TINY_EPS[3], 3, TINY_SCALE, thin=2, seed=4, stream=stream, theta=theta, chain=chain)
        keep = [k for k in range(8) if (theta or k != 1) and (chain or k < 6)]
        assert rc == 0 and _same([dev[k] for k in keep], [ref[k] for k in keep])
    # continuation: 4 iterations, then 6 more from the returned walkers
    a = hmc.hmc_batch(fit, U0, 4, TINY_EPS[3], 3, **kw)
    b = hmc.hmc_batch(fit, a[0], 6, TINY_EPS[3], 3, first_iter=4, **kw)
    assert _same(ref[:3], b[:3]) and np.array_equal(ref[4], a[4] + b[4]) and np.array_equal(ref[5], a[5] + b[5])
    assert ref[6].tobytes() == np.concatenate([a[6], b[6]]).tobytes() and ref[7].tobytes() == np.concatenate([a[7], b[7]]).tobytes()
    # rows shuffled with their ids, and a part of the batch on its own: a walker's results are its own
    perm = np.random.default_rng(9).permutation(130)
    shuffled = hmc.hmc_batch(fit, U0[perm], 10, TINY_EPS[3], 3, walker_ids=perm, **kw)
    assert _same(shuffled[:6], [v[perm] for v in ref[:6]]) and _same(shuffled[6:], [v[:, perm] for v in ref[6:]])
    rc, dev = _device_call(fit, U0[perm[:5]], 10, TINY_EPS[3], 3, TINY_SCALE, thin=2, seed=4, wid=perm[:5].astype(np.uint64))
    assert rc == 0 and _same(dev[:6], [v[perm[:5]] for v in ref[:6]])
    # another seed or another first iteration is another run
    assert not _same(ref[:1], hmc.hmc_batch(fit, U0, 10, TINY_EPS[3], 3, scale=TINY_SCALE, thin=2, seed=5)[:1])
    assert not _same(ref[:1], hmc.hmc_batch(fit, U0, 10, TINY_EPS[3], 3, first_iter=1, **kw)[:1])
    with mcalf_amd.als_fitter(None, device=[0, 0], **tiny_problem(64)) as multi:
        assert _same(ref, hmc.hmc_batch(multi, U0, 10, TINY_EPS[3], 3, **kw))
        rc, _ = _device_call(multi, U0, 2, 0.5, 1, TINY_SCALE)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in multi._lib.mcalf_last_error(multi._ctx)


# ---- refused starts --------------------------------------------------------------------------------------------------------------

def test_refused_starts_come_back_as_given():
    """A start outside the cube, one with a NaN and one in the asymmetric-veto region (logL = -inf: veto thresholds of 10 pixels
    above 4 sigma and 5 above 5 sigma) have status -1 and come back as given; the others match the restatement, whose
    launches carry the refused rows along."""
    with mcalf_amd.als_fitter(None, Asymmlike=True, gauss_cdf=[50, 10, 5], **tiny_problem(64)) as fit:
        draws = np.random.default_rng(3).random((512, fit.ndim))
        L0 = _logl(fit)(draws)
        vetoed, fine = np.flatnonzero(np.isneginf(L0)), np.flatnonzero(np.isfinite(L0))
        assert vetoed.size > 0 and fine.size >= 9
        U0 = draws[fine[:9]].copy()
        U0[2, 1], U0[4, 3], U0[6] = 1.5, np.nan, draws[vetoed[0]]
        seen = []
        U, theta, L, status, naccept, ndead, CU, CL = _against_reference(fit, U0, 12, 0.2, 2, TINY_SCALE, seed=21, seen=seen)
        bad = np.array([2, 4, 6])
        good = np.setdiff1d(np.arange(9), bad)
        assert (status[bad] == -1).all() and (status[good] == 0).all() and not naccept[bad].any() and not ndead[bad].any()
        assert np.array_equal(U[bad], U0[bad], equal_nan=True) and np.isneginf(L[6])
        assert np.array_equal(CU[:, bad], np.broadcast_to(U0[bad], (12, 3, 4)), equal_nan=True)
        assert naccept[good].sum() > 0 and np.isfinite(L[good]).all() and np.isfinite(CL[:, good]).all()
        print(f"accepted {naccept.sum()}, dead {ndead.sum()}; vetoed trial rows among the launches: {sum(int(np.isneginf(s[good]).sum()) for s in seen[1:])}")


# ---- the posterior end to end --------------------------------------------------------------------------------------------------------

BURN, KEPT, NBATCH, WALKERS = 300, 1000, 20, 128


def test_the_sampler_finds_the_posterior_moments(posterior):  # noqa: F811
    """128 walkers from a ball of half-width 0.05 around the `maximize_batch` optimum, 300 iterations of burn-in in 5 windows
    that adapt the step and the scales, 1000 kept, 20 batches of 50 iterations, trajectories of 4 steps.  The bars are the
    ensemble test's: every mean and variance of the three continuous cube coordinates within 5 batch-means standard errors of
    the quadrature, whose 96^3 and 64^3 values must agree to a fifth of each standard error.
    Measured on an MI355X (this test): deviations 1.28, -0.98, -0.79 (means) and 0.27, 0.78, 0.09 (variances) standard errors;
    window acceptances 0.88, 0.97, 0.86, 0.76, 0.82 with eps from 0.3 to 1.19, acceptance 0.82 in the kept run, no dead
    trajectory, autocorrelation times of the ensemble means 3 .. 9 iterations."""
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
        res = hmc.hmc_sample(fit, WALKERS, KEPT, burn=BURN, start=start, ball=0.05, seed=0, eps=0.3, nleap=4)
        assert res.cube.shape == (KEPT, WALKERS, 4) and (res.status == 0).all()
        assert np.array_equal(res.theta[-1], fit.scale_cube_batch(res.cube[-1])) and np.array_equal(res.last, res.cube[-1])
        print(f"window acceptance {np.round(res.window_accept, 3)}, window eps {np.round(res.window_eps, 3)}, eps {res.eps:.3f}, scale {res.scale}, "
              f"acceptance {res.accept_frac.mean():.3f}, dead {res.ndead.sum()}, autocorrelation times {np.round(res.autocorr_time(), 1)}")
        x = res.cube[:, :, 1:]
        for name, series, want, coarse in (("mean", x.mean(axis=1), qmean, cmean), ("variance", ((x - qmean) ** 2).mean(axis=1), qvar, cvar)):
            se = ensemble.batch_means_se(series, NBATCH)
            dev = (series.mean(axis=0) - want) / se
            print(f"{name} {series.mean(axis=0)}, quadrature {want}: deviations {np.round(dev, 2)} standard errors; "
                  f"quadrature 96^3 - 64^3 over a standard error {np.round(np.abs(want - coarse) / se, 4)}")
            assert (np.abs(want - coarse) < 0.2 * se).all()
            assert (np.abs(dev) <= 5.0).all()
