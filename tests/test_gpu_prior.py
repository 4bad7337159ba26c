"""GPU: the Gaussian prior (mcalf_set_gauss_prior, mcalf_lnprior_batch[_device]) and the three samplers under it, against the
numpy restatement tests/prior_reference.py with logL = als_fitter.loglike_cube_batch and the constants c the library holds.
lnprior by bytes; the samplers' U by value (the sign of a zero may differ), logL and the chain's logL by bytes, the counters
equal -- no tolerance.  Then a flat target, which must end truncated-normal in the coordinate that carries the Gaussian, and
the posterior moments and the evidence of the three-parameter problem of test_gpu_ns.py end to end against a quadrature of
the C oracle whose weights are multiplied by the prior's density.

many_components.many(65) has its ncomp slot at coordinate 1 (startind 1), which may carry no Gaussian: the case "coordinate 1
alone" is, at that ndim, the refusal, and is asserted as one; at ndim 4 and 129 it is a Gaussian like any other.

Posterior and evidence: the figures measured on an MI355X are in the docstrings of the two tests."""
import ctypes as C

import numpy as np
import pytest
import torch

import many_components as mc
import mcalf_amd
import prior_reference as pr
from cases import problem_from_kwargs, tiny_problem
from mcalf_amd import _lib, ensemble, nested, tempering, workloads
from test_ens_reference import FLAT_ITERS, FLAT_SEED, KS_BAR, flat_start, ks_distances
from test_gpu_fit import _civ
from test_gpu_ns import _evidence_problem

pytestmark = pytest.mark.gpu

MOVES = {"stretch": pr.STRETCH, "de": pr.DE}
INF = float("inf")


def _logl(fit):
    return lambda U: fit.loglike_cube_batch(U, return_theta=False)


def _lnp(fit):
    """The restatement over the library's own mu, sigma, c and the fitter's box, for cube rows."""
    g = fit.gauss_prior
    mu, sigma, c = g if g is not None else (None, None, None)
    return lambda U, cube=True: pr.lnprior(U, fit._lo, fit._hi, mu, sigma, c, cube, int_slot=fit.startind)


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _ball(centre, half, shape, rng):
    return np.clip(centre + half * (2.0 * rng.random(tuple(shape) + (centre.size,)) - 1.0), 0.0, 1.0)


def _gauss_at(fit, centre_cube, which, shift=0.5, width=0.1):
    """mu, sigma [ndim]: on the coordinates `which` a Gaussian `shift` widths beside the cube point `centre_cube`, `width` of the
    box wide; none elsewhere."""
    mu, sigma = np.zeros(fit.ndim), np.zeros(fit.ndim)
    span = fit._hi - fit._lo
    for k in which:
        sigma[k] = width * span[k]
        mu[k] = fit._lo[k] + centre_cube[k] * span[k] + shift * sigma[k]
    return mu, sigma


def _device_lnprior(fit, rows, cube, stream=None):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    out = torch.full((rows.shape[0],), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream() if stream is None else stream
    stream.wait_stream(torch.cuda.current_stream())
    rc = fit._lib.mcalf_lnprior_batch_device(fit._ctx, d.data_ptr(), rows.shape[0], int(cube), out.data_ptr(), C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, out.cpu().numpy()


# ---- the problems ------------------------------------------------------------------------------------------------------------------

def _kwargs(ndim):
    return tiny_problem(64) if ndim == 4 else mc.many(ndim)[0]


@pytest.fixture(scope="module")
def problems():
    """ndim -> (fit, multi-device fit on [0, 0], the best of some uniform points of the cube), made once."""
    made = {}

    def get(ndim):
        if ndim not in made:
            fit = mcalf_amd.als_fitter(None, **_kwargs(ndim))
            multi = mcalf_amd.als_fitter(None, device=[0, 0], **_kwargs(ndim))
            assert fit.ndim == ndim
            draws = np.random.default_rng(ndim).random((max(4 * ndim, 256), ndim))
            made[ndim] = (fit, multi, draws[np.nanargmax(_logl(fit)(draws))])
        made[ndim][0].clear_gauss_prior()
        made[ndim][1].clear_gauss_prior()
        return made[ndim]
    yield get
    for fit, multi, _ in made.values():
        fit.close()
        multi.close()


def _sets(ndim, slot):
    allowed = [k for k in range(ndim) if k != slot]
    return {"one": [1], "63_64": [k for k in (63, 64) if k < ndim] or [2, 3], "last": [ndim - 1], "all": allowed, "none": []}


# ---- lnprior_batch against the restatement, by bytes ---------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["one", "63_64", "last", "all", "none"])
@pytest.mark.parametrize("ndim", [4, 65, 129])
def test_lnprior_batch_is_the_restatement_by_bytes(problems, ndim, which):
    fit, multi, best = problems(ndim)
    rng = np.random.default_rng(ndim + len(which))
    coords = _sets(ndim, fit.startind)[which]
    mu, sigma = _gauss_at(fit, rng.random(ndim), coords, shift=0.7, width=0.2)
    if fit.startind in coords:                                  # (ndim 65: coordinate 1 is the ncomp slot)
        assert ndim == 65 and coords == [1]
        with pytest.raises(RuntimeError, match=r"mcalf_set_gauss_prior: sigma\[1\] > 0 puts a Gaussian on the ncomp slot"):
            fit.set_gauss_prior(mu, sigma)
        assert fit.gauss_prior is None
        coords = [0]                                            # the first coordinate alone takes its place in what follows
        mu, sigma = _gauss_at(fit, rng.random(ndim), coords, shift=0.7, width=0.2)
    for f in (fit, multi):
        f.set_gauss_prior(mu, sigma)
    if coords:
        gm, gs, gc = fit.gauss_prior
        assert gm.tobytes() == mu.tobytes() and gs.tobytes() == sigma.tobytes() and not gc[sigma == 0.0].any()
        want = np.log(2.0 * np.pi * sigma[sigma > 0.0] ** 2)
        assert (np.abs(gc[sigma > 0.0] - want) <= np.spacing(np.abs(want))).all()
        assert _same(fit.gauss_prior, multi.gauss_prior)
    else:
        assert fit.gauss_prior is None and multi.gauss_prior is None
    lnp = _lnp(fit)
    side = torch.cuda.Stream()
    for batch in (1, 64, 65):
        U = rng.random((batch, ndim))
        k = ndim - 1
        if batch >= 64:                                         # on a face, just outside it, NaN -- early and late coordinates
            U[1, 0], U[2, k], U[3, 0], U[4, k] = 0.0, 1.0, np.nextafter(0.0, -1.0), np.nextafter(1.0, 2.0)
            U[5, k], U[6, 1], U[7, k // 2] = np.nan, np.nan, 1.0
        for cube in (True, False):
            rows = U.copy()
            if not cube:
                rows = rows * (fit._hi - fit._lo) + fit._lo
                if batch >= 64:
                    rows[1, 0], rows[2, k], rows[7, k // 2] = fit._lo[0], fit._hi[k], fit._hi[k // 2]
                    rows[3, 0], rows[4, k] = np.nextafter(fit._lo[0], -INF), np.nextafter(fit._hi[k], INF)
            want = lnp(rows, cube)
            got = fit.lnprior_batch(rows, cube=cube)
            assert got.tobytes() == want.tobytes(), (batch, cube, np.flatnonzero(got != want)[:8])
            if batch >= 64:
                assert np.isneginf(got[3:7]).all() and np.isfinite(got[[0, 1, 2, 7]]).all() and np.isfinite(got[8:]).all()
            if not coords:
                assert not got[np.isfinite(got)].any()
            rc, dev = _device_lnprior(fit, rows, cube, side)
            assert rc == 0 and dev.tobytes() == got.tobytes()
            assert multi.lnprior_batch(rows, cube=cube).tobytes() == got.tobytes()
    # cube rows and their transformed rows agree wherever both are inside
    U = rng.random((65, ndim))
    assert fit.lnprior_batch(U, cube=True).tobytes() == fit.lnprior_batch(fit.loglike_cube_batch(U)[0], cube=False).tobytes()
    rc, _ = _device_lnprior(multi, U, True)
    assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in multi._lib.mcalf_last_error(multi._ctx)
    assert fit._lib.mcalf_lnprior_batch(fit._ctx, None, 0, 1, None) == 0
    p = fit.loglike_cube_batch(U[:1])[0][0]
    assert fit.lnprior(p) == fit.lnprior_batch(p)[0] and fit(p) == fit.lnprior(p) + fit.lnlhood_worker(p)
    p[ndim - 1] = np.nextafter(fit._hi[-1], INF)
    assert fit(p) == -INF


def test_refusals_that_need_a_context_and_a_later_box(problems):
    fit, multi, best = problems(4)
    for mu, sigma, what in (([0, 13.0, 3.0, 20.0], [0, -1.0, 0, 0], r"sigma\[1\] must be finite and >= 0"),
                            ([0, 13.0, 3.0, 20.0], [0, 0, np.nan, 0], r"sigma\[2\] must be finite and >= 0"),
                            ([0, 13.0, 3.0, 20.0], [0, 0, 0, INF], r"sigma\[3\] must be finite and >= 0"),
                            ([0, np.nan, 3.0, 20.0], [0, 0.5, 0, 0], r"mu\[1\] must be finite"),
                            ([1.0, 13.0, 3.0, 20.0], [0.5, 0, 0, 0], r"sigma\[0\] > 0 puts a Gaussian on the ncomp slot")):
        for f in (fit, multi):
            with pytest.raises(RuntimeError, match=what):
                f.set_gauss_prior(mu, sigma)
            assert f.gauss_prior is None
    with pytest.raises(ValueError):
        fit.set_gauss_prior([0.0] * 3, [0.0] * 3)
    mu, sigma = _gauss_at(fit, best, [1, 3])
    fit.set_gauss_prior(mu, sigma)
    U = np.random.default_rng(0).random((8, 4))
    before = fit.lnprior_batch(U, cube=True)
    fit._prior_key = None
    fit._ensure_prior(False)                                    # the box again, the other ncomp flavour: the Gaussian stays
    assert _same(fit.gauss_prior, (mu, sigma, fit.gauss_prior[2])) and fit.lnprior_batch(U, cube=True).tobytes() == before.tobytes()
    fit._prior_key = None
    fit._ensure_prior(True)
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fresh:      # no box yet
        assert fresh._lib.mcalf_set_gauss_prior(fresh._ctx, mu.ctypes.data, sigma.ctypes.data) == _lib.MCALF_ERR_INVALID
        assert b"mcalf_set_prior has not been called" in fresh._lib.mcalf_last_error(fresh._ctx)
        out = np.zeros(8)
        assert fresh._lib.mcalf_lnprior_batch(fresh._ctx, U.ctypes.data, 8, 1, out.ctypes.data) == _lib.MCALF_ERR_INVALID
    g = ['none'] * 8
    g[2], g[3], g[6], g[7] = mu[1], sigma[1], str(mu[3]), str(sigma[3])
    with mcalf_amd.als_fitter(None, Gpriors=g, **tiny_problem(64)) as viakw:
        assert _same(viakw.gauss_prior, fit.gauss_prior) and viakw.lnprior_batch(U, cube=True).tobytes() == before.tobytes()


# ---- the samplers under the prior, against the restatement ---------------------------------------------------------------------------

def _check_slice(fit, U0, Lmin, D, sid, nmoves, max_steps, seed):
    got = fit.slice_replace_batch(U0, Lmin, D, nmoves=nmoves, max_steps=max_steps, seed=seed, stream_ids=sid)
    U, theta, L, status, nevals, moves = got
    rU, rL, rs, rn, rm = pr.slice_replace(_logl(fit), _lnp(fit), U0, Lmin, D, sid, nmoves, max_steps, seed)
    assert np.array_equal(status, rs) and np.array_equal(nevals, rn) and np.array_equal(moves, rm)
    assert np.array_equal(U, rU, equal_nan=True) and L.tobytes() == rL.tobytes()
    assert L.tobytes() == (_logl(fit)(U) + fit.lnprior_batch(U, cube=True)).tobytes()
    assert np.array_equal(theta, fit.scale_cube_batch(U), equal_nan=True)
    return got


def _check_ens(fit, U0, nsteps, thin, move, seed, first_iter=0):
    got = fit.ensemble_batch(U0, nsteps, thin=thin, move=move, seed=seed, first_iter=first_iter)
    U, theta, L, status, naccept, CU, CL = got
    rU, rL, rs, rn, rCU, rCL, rPR = pr.ensemble(_logl(fit), _lnp(fit), U0, nsteps, thin, MOVES[move], None, seed, first_iter)
    assert np.array_equal(status, rs) and np.array_equal(naccept, rn)
    assert np.array_equal(U, rU, equal_nan=True) and L.tobytes() == rL.tobytes()
    assert CU.shape == rCU.shape and np.array_equal(CU, rCU, equal_nan=True) and CL.tobytes() == rCL.tobytes()
    assert L.tobytes() == _logl(fit)(U).tobytes() and rPR.tobytes() == fit.lnprior_batch(U, cube=True).tobytes()
    return got


def _check_pt(fit, U0, betas, nsteps, thin, swap_every, move, seed, first_iter=0):
    T, n, ndim = U0.shape
    got = fit.tempered_batch(U0, betas, nsteps, thin=thin, swap_every=swap_every, move=move, seed=seed, first_iter=first_iter)
    U, theta, L, status, naccept, nswap, CU, CL = got
    rU, rL, rs, rn, rw, rCU, rCL, rPR = pr.tempered(_logl(fit), _lnp(fit), U0, betas, nsteps, thin, swap_every, MOVES[move], None, seed, first_iter, 1)
    assert np.array_equal(status, rs) and np.array_equal(naccept, rn) and np.array_equal(nswap, rw)
    assert np.array_equal(U, rU, equal_nan=True) and L.tobytes() == rL.tobytes()
    assert CU.shape == rCU.shape and np.array_equal(CU, rCU, equal_nan=True) and CL.tobytes() == rCL.tobytes()
    assert L.tobytes() == _logl(fit)(U.reshape(T * n, ndim)).tobytes()
    assert rPR.tobytes() == fit.lnprior_batch(U.reshape(T * n, ndim), cube=True).tobytes()
    return got


def _slice_setup(fit, n, rng, nlive=256):
    live = rng.random((nlive, fit.ndim))
    L = _logl(fit)(live) + fit.lnprior_batch(live, cube=True)
    lmin = float(np.median(L))
    ok = np.flatnonzero(L > lmin)
    return live[ok[rng.integers(0, ok.size, n)]].copy(), lmin, nested.directions(live[L > lmin])


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("batch", [1, 65])
def test_slice_trajectories_under_the_prior(problems, batch, compact):
    fit, multi, best = problems(4)
    fit.set_gauss_prior(*_gauss_at(fit, best, [1, 3]))
    U0, lmin, D = _slice_setup(fit, batch, np.random.default_rng(batch))
    sid = np.arange(batch, dtype=np.uint64) + np.uint64(77)
    fit.set_slice_compact(compact)
    try:
        got = _check_slice(fit, U0, lmin, D, sid, 8, 400, seed=batch)
        assert (got[3] == 1).all() and fit.slice_stats()["compact"] == int(compact)
        if batch == 65:
            bad = U0.copy()
            bad[3, 1] = 1.5                                     # outside the cube: -1, as given, logL + (-inf)
            lm = np.full(65, lmin)
            lm[5] = INF
            got = _check_slice(fit, bad, lm, D, sid, 8, 400, seed=2)
            assert got[3][3] == -1 and got[3][5] == -1 and np.isneginf(got[2][3]) and (np.delete(got[3], [3, 5]) == 1).all()
    finally:
        fit.set_slice_compact(False)
    if batch == 65:                                             # the prior changes the walk: without it the same call ends elsewhere
        fit.clear_gauss_prior()
        assert not _same(got[:1], fit.slice_replace_batch(bad, lm, D, nmoves=8, max_steps=400, seed=2, stream_ids=sid)[:1])


@pytest.mark.parametrize("move", ["stretch", "de"])
@pytest.mark.parametrize("n", [4, 6, 130])
def test_ensemble_and_ladder_trajectories_under_the_prior(problems, n, move):
    """Halves of 2, 3 and 65 walkers; one rung, and three rungs with a swap round after every iteration (the hottest at
    beta = 0, which samples the prior's Gaussian factors); continuation equal to the long call."""
    fit, multi, best = problems(4)
    fit.set_gauss_prior(*_gauss_at(fit, best, [1, 3]))
    U0 = _ball(best, 0.1, (3, n), np.random.default_rng(n))
    U0[2, 1, 2] = 1.0 + 2.0 ** -52                             # a bad start in the hot rung: lnprior -inf, never read
    got = _check_ens(fit, U0[0], 12, 5, move, seed=n)
    assert 0 < got[4].sum() < 12 * n
    a = fit.ensemble_batch(U0[0], 5, thin=5, move=move, seed=n)
    b = fit.ensemble_batch(a[0], 7, thin=5, move=move, seed=n, first_iter=5)
    assert _same(got[:3], b[:3]) and np.array_equal(got[4], a[4] + b[4]) and got[5].tobytes() == np.concatenate([a[5], b[5]]).tobytes()
    betas = [1.0, 0.3, 0.0]
    pt = _check_pt(fit, U0, betas, 12, 5, 1, move, seed=n + 1)
    assert pt[3][2, 1] == -1 and pt[5].sum() > 0 and 0 < pt[4].sum() < 12 * n * 3
    a = fit.tempered_batch(U0, betas, 4, thin=2, swap_every=1, move=move, seed=n + 1)
    b = fit.tempered_batch(a[0], betas, 8, thin=2, swap_every=1, move=move, seed=n + 1, first_iter=4)
    whole = fit.tempered_batch(U0, betas, 12, thin=2, swap_every=1, move=move, seed=n + 1)
    assert _same(whole[:3], b[:3]) and np.array_equal(whole[4], a[4] + b[4]) and np.array_equal(whole[5], a[5] + b[5])
    assert whole[7].tobytes() == np.concatenate([a[7], b[7]]).tobytes()
    assert _same(whole, multi_call(multi, fit, U0, betas, move, n))
    if n == 130:                                                # the prior changed the walk (a handful of walkers may meet no decision it flips)
        fit.clear_gauss_prior()
        assert not _same(got[:1], fit.ensemble_batch(U0[0], 12, thin=5, move=move, seed=n)[:1])


def multi_call(multi, fit, U0, betas, move, n):
    g = fit.gauss_prior
    multi.set_gauss_prior(g[0], g[1])
    return multi.tempered_batch(U0, betas, 12, thin=2, swap_every=1, move=move, seed=n + 1)


def test_trajectories_two_lines_with_a_gaussian_on_the_resolution_and_on_one_redshift():
    kw, _ = _civ(npix=300, specres=(6.0, 9.0), contval=(0.9, 1.1))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.ndim == 15 and fit.startind == 2
        draws = np.random.default_rng(2).random((128, 15))
        best = draws[np.nanargmax(_logl(fit)(draws))]
        fit.set_gauss_prior(*_gauss_at(fit, best, [0, 4]))
        for move in ("stretch", "de"):
            got = _check_ens(fit, _ball(best, 0.05, (64,), np.random.default_rng(4)), 12, 5, move, seed=2 ** 63 + 9, first_iter=2 ** 40)
            assert 0 < got[4].sum() < 12 * 64
        _check_pt(fit, _ball(best, 0.05, (3, 6), np.random.default_rng(5)), [1.0, 0.3, 0.0], 12, 5, 1, "stretch", seed=3)
        U0, lmin, D = _slice_setup(fit, 33, np.random.default_rng(6), nlive=128)
        got = _check_slice(fit, U0, lmin, D, np.arange(33, dtype=np.uint64) * np.uint64(2 ** 33 + 1), 8, 400, seed=2 ** 63 + 9)
        assert (got[3] == 1).all()


def test_trajectories_with_the_gaussian_on_the_last_of_65_coordinates(problems):
    fit, multi, best = problems(65)
    fit.set_gauss_prior(*_gauss_at(fit, best, [64], shift=1.0, width=0.05))
    for move in ("stretch", "de"):
        got = _check_ens(fit, _ball(best, 0.02, (8,), np.random.default_rng(65)), 12, 1, move, seed=65)
        assert got[4].sum() > 0
    _check_pt(fit, _ball(best, 0.02, (3, 4), np.random.default_rng(66)), [1.0, 0.3, 0.0], 12, 5, 1, "de", seed=66)
    fit.set_slice_compact(True)
    try:
        U0, lmin, D = _slice_setup(fit, 65, np.random.default_rng(67), nlive=260)
        got = _check_slice(fit, U0, lmin, D, np.arange(65, dtype=np.uint64), 4, 200, seed=67)
        assert (got[3] >= 0).all() and got[5].sum() > 0
    finally:
        fit.set_slice_compact(False)


def test_set_then_cleared_is_a_context_that_never_had_a_prior(problems):
    fit, multi, best = problems(4)
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as never:
        rng = np.random.default_rng(9)
        U0 = _ball(best, 0.1, (3, 130), rng)
        live = rng.random((256, 4))
        L = _logl(never)(live)
        lmin = float(np.median(L))
        D = nested.directions(live[L > lmin])
        S0 = live[L > lmin][:65].copy()
        calls = (lambda f: f.ensemble_batch(U0[0], 10, thin=2, move="de", seed=4),
                 lambda f: f.tempered_batch(U0, [1.0, 0.3, 0.0], 10, thin=2, swap_every=1, seed=4),
                 lambda f: f.slice_replace_batch(S0, lmin, D, nmoves=8, max_steps=400, seed=4))
        want = [call(never) for call in calls]
        fit.set_gauss_prior(*_gauss_at(fit, best, [1, 3]))
        under = [call(fit) for call in calls]
        assert not any(_same(a[:1], b[:1]) for a, b in zip(want, under))
        fit.clear_gauss_prior()
        assert fit.gauss_prior is None
        assert all(_same(a, call(fit)) for a, call in zip(want, calls))
        assert not fit.lnprior_batch(live, cube=True).any()


# ---- a flat target -------------------------------------------------------------------------------------------------------------------

MU, SIGMA = 0.4, 0.15


@pytest.mark.parametrize("move", ["stretch", "de"])
def test_a_flat_target_ends_truncated_normal_and_equals_the_reference(move):
    """Errors of 1e30 make logL one constant (asserted), as in test_gpu_ens.py; N(0.4, 0.15^2) in cube units on coordinate 1."""
    kw = tiny_problem(64)
    wl, flux, _ = kw["spectrum"]
    with mcalf_amd.als_fitter(None, **dict(kw, spectrum=(wl, flux, np.full(64, 1e30)))) as fit:
        nd = fit.ndim
        U0 = flat_start(nd)
        const = _logl(fit)(np.random.default_rng(0).random((512, nd)))
        assert np.isfinite(const[0]) and (const == const[0]).all()
        mu, sigma = np.zeros(nd), np.zeros(nd)
        mu[1], sigma[1] = fit._lo[1] + MU * (fit._hi[1] - fit._lo[1]), SIGMA * (fit._hi[1] - fit._lo[1])
        fit.set_gauss_prior(mu, sigma)
        lnp = _lnp(fit)
        U, theta, L, status, naccept, CU, CL = fit.ensemble_batch(U0, FLAT_ITERS[nd], thin=FLAT_ITERS[nd], move=move, seed=FLAT_SEED)
        assert (L == const[0]).all() and (CL == const[0]).all() and (status == 0).all()
    ref = pr.ensemble(lambda Y: np.full(Y.shape[0], const[0]), lnp, U0, FLAT_ITERS[nd], FLAT_ITERS[nd], MOVES[move], seed=FLAT_SEED)
    assert np.array_equal(U, ref[0]) and np.array_equal(naccept, ref[3]) and np.array_equal(CU[0], U)
    d = ks_distances(U)
    d[1] = pr.ks_against(U[:, 1], lambda x: pr.truncated_normal_cdf(x, MU, SIGMA))
    print(f"move {move}: KS distances {np.round(d, 4)} (bar {KS_BAR:.4f}), acceptance {naccept.mean() / FLAT_ITERS[nd]:.3f}")
    assert ks_distances(U)[1] > 2.0 * KS_BAR and (d < KS_BAR).all()


# ---- the posterior and the evidence end to end ---------------------------------------------------------------------------------------

BURN, KEPT, NBATCH = 500, 4000, 20
NTEMPS, BETA_MIN, PT_WALKERS, PT_BURN, PT_KEPT = 16, 1e-4, 64, 300, 1500


@pytest.fixture(scope="module")
def quadrature():
    """test_gpu_ens.py's evidence problem and quadrature construction over the C oracle (midpoint rule, 96^3 and 64^3 nodes over
    the box of +- 10 standard deviations around the no-prior posterior mean, extended by the prior's shift), once without and
    once with the weights multiplied by g.  The prior comes from the no-prior quadrature's own moments (m, s) of the column
    density: mu = m + 2 s, sigma = s, in theta units.  Returns (kwargs, mu, sigma [ndim], {nodes: (ln Z, mean, var)} with the
    prior, the no-prior mean and standard deviation)."""
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
        return g, P, orc.loglike_batch(P)

    def moments(g, ll):
        w = np.exp(ll - ll.max())
        w /= w.sum()
        mean = (w[:, None] * g).sum(axis=0)
        return mean, (w[:, None] * (g - mean) ** 2).sum(axis=0), w

    g, P, ll = grid(64, np.zeros(3), np.ones(3))
    mean, var, w = moments(g, ll)
    sd = np.sqrt(var)
    mu, sigma = np.zeros(4), np.zeros(4)
    mu[1] = lo[1] + (mean[0] + 2.0 * sd[0]) * (hi[1] - lo[1])
    sigma[1] = sd[0] * (hi[1] - lo[1])
    lng = lambda P: -0.5 * (((P[:, 1] - mu[1]) / sigma[1]) ** 2 + np.log(2.0 * np.pi * sigma[1] ** 2))
    a, c = np.clip(mean - 10.0 * sd, 0.0, 1.0), np.clip(mean + 12.0 * sd, 0.0, 1.0)
    out = ((g < a) | (g > c)).any(axis=1)
    assert w[out].sum() < 1e-12 and moments(g, ll + lng(P))[2][out].sum() < 1e-12
    with_prior = {}
    for m in (96, 64):
        g, P, ll = grid(m, a, c)
        lp = ll + lng(P)
        with_prior[m] = (float(np.logaddexp.reduce(lp) - 3.0 * np.log(m) + np.log(c - a).sum()),) + moments(g, lp)[:2]
    return kw, mu, sigma, with_prior, mean, sd


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_ensemble_finds_the_posterior_under_the_prior(quadrature, seed):
    """test_gpu_ens.py's run (256 walkers, 500 iterations of burn-in, 4000 kept, 20 batches, the stretch move) under the prior
    N(m + 2 s, s^2) on the column density.  Precondition: the with-prior quadrature mean of that coordinate lies at least 0.5 s
    from the no-prior one (for two Gaussians of equal width it lies 1 s away) while the sampler's standard error is about a
    hundredth of s, so a sampler that ignores the prior cannot pass.  Every mean and variance of the three continuous cube
    coordinates within 5 batch-means standard errors of the quadrature, whose 96^3 and 64^3 values must agree to a fifth of
    each standard error.
    Measured on an MI355X (this test), deviations in standard errors (means | variances); prior_reference.ensemble alone over
    the C oracle (c by np.log) gives the same figures to the digits shown:
        seed 0   0.44  1.38  0.20 |  0.68  1.65 -0.23      (the no-prior mean lies 229 standard errors away)
        seed 1  -0.02  0.07  0.10 |  0.12 -0.76 -0.22      (205)
        seed 2  -1.12  0.54 -0.16 |  2.80 -1.90  0.15      (168)"""
    kw, mu, sigma, q, mean0, sd0 = quadrature
    (_, qmean, qvar), (_, cmean, cvar) = q[96], q[64]
    assert abs(qmean[0] - mean0[0]) >= 0.5 * sd0[0]
    b = workloads.bounds_of(kw)
    lo, hi = b.min(axis=1), b.max(axis=1)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        fit.set_gauss_prior(mu, sigma)
        start = np.full(4, 0.5)
        start[1:] = qmean
        res = fit.ensemble_sample(256, KEPT, burn=BURN, thin=1, start=start, ball=0.05, seed=seed, move="stretch")
        assert res.cube.shape == (KEPT, 256, 4) and (res.status == 0).all() and res.lnprior.shape == (KEPT, 256)
        assert res.lnprior[-1].tobytes() == fit.lnprior_batch(res.cube[-1], cube=True).tobytes()
        x = res.cube[:, :, 1:]
        for name, series, want, coarse in (("mean", x.mean(axis=1), qmean, cmean), ("variance", ((x - qmean) ** 2).mean(axis=1), qvar, cvar)):
            se = ensemble.batch_means_se(series, NBATCH)
            dev = (series.mean(axis=0) - want) / se
            print(f"seed {seed}: {name} {series.mean(axis=0)}, quadrature {want}: deviations {np.round(dev, 2)} standard errors; no-prior mean "
                  f"{(mean0[0] - qmean[0]) / se[0] if name == 'mean' else 0.0:+.0f} standard errors away; 96^3 - 64^3 over a standard error "
                  f"{np.round(np.abs(want - coarse) / se, 4)}")
            assert (np.abs(want - coarse) < 0.2 * se).all()
            assert (np.abs(dev) <= 5.0).all()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_both_evidence_routes_find_the_integral_of_likelihood_times_prior(quadrature, seed):
    """`nested_sample` (256 live points, as test_gpu_ns.py runs it) within 4 sqrt(H / nlive), and
    `tempered_sample(...).logZ_stepping_stone()` (test_gpu_pt.py's ladder and run) within 5 of its own standard errors, of the
    quadrature's ln of the integral of L g over the cube.  The deviations are printed in standard errors.
    Measured on an MI355X (this test) against the quadrature's 104.4349 (96^3 and 64^3 nodes agree to 1e-4); the numpy
    restatements alone over the C oracle give the same figures to the digits shown:
        seed 0   nested 104.4227, -0.07 of 0.1832      stepping stones 104.4488 +- 0.0131, +1.06      TI 104.1136
        seed 1   nested 104.2668, -0.91 of 0.1842      stepping stones 104.4440 +- 0.0237, +0.38      TI 104.1060
        seed 2   nested 104.4320, -0.02 of 0.1827      stepping stones 104.4234 +- 0.0194, -0.59      TI 104.0841
    ln of the prior's mass over the cube (Z at beta = 0) is -0.9163."""
    kw, mu, sigma, q, _, _ = quadrature
    want, coarse = q[96][0], q[64][0]
    with mcalf_amd.als_fitter(None, **kw) as fit:
        fit.set_gauss_prior(mu, sigma)
        res = fit.nested_sample(nlive=256, batch=64, nmoves=8, seed=seed, max_steps=200)
        err = np.sqrt(res.H / 256)
        print(f"seed {seed}: nested ln Z {res.logZ:.4f}, quadrature {want:.4f} (64^3: {coarse:.4f}): {(res.logZ - want) / err:+.2f} standard errors of {err:.4f}")
        assert abs(want - coarse) < 0.2 * err and res.unfinished == 0
        assert res.lnprior.tobytes() == fit.lnprior_batch(res.cube, cube=True).tobytes()
        assert res.logL.tobytes() == (_logl(fit)(res.cube) + res.lnprior).tobytes()
        assert abs(res.logZ - want) <= 4.0 * err
        pt = fit.tempered_sample(PT_WALKERS, PT_KEPT, betas=tempering.default_ladder(NTEMPS, BETA_MIN), burn=PT_BURN, seed=seed)
        lnz, perr = pt.logZ_stepping_stone(NBATCH)
        mass = tempering.ln_prior_mass(fit._lo, fit._hi, mu, sigma)
        print(f"seed {seed}: stepping stones ln Z {lnz:.4f} +- {perr:.4f} (ln of the prior's mass over the cube {mass:.4f}): {(lnz - want) / perr:+.2f} "
              f"standard errors; thermodynamic integration {pt.logZ_ti():.4f}")
        assert pt.ln_prior_mass == mass and abs(want - coarse) < 0.2 * perr
        assert abs(lnz - want) <= 5.0 * perr
