"""GPU: the device-resident nested-sampling run (mcalf_nested_*) against its numpy restatement tests/nsrun_reference.py with
logL = als_fitter.loglike_cube_batch (every decision sees the same bits) and the device's own direction rows of each round fed
to the reference: the selections exactly, the dead points by value, their logL by bytes; the direction rows against numpy's
covariance within the derived bound; ties, bad initial points, plateaus; invariance under the cut into calls, the packing, the
device count and the prior; the stop, the full buffer, and the evidence end to end.  Every case is at most 2048 rows and 300
pixels."""
import ctypes as C

import numpy as np
import pytest

import many_components as mc
import mcalf_amd
import nsrun_reference as ref
from cases import tiny_problem
from mcalf_amd import _lib, nested_device
from mcalf_amd.routines.hires_fitter import write_equal_weights
from test_gpu_fit import _civ
from test_gpu_ns import _evidence_problem

pytestmark = pytest.mark.gpu

EPS = np.finfo(float).eps
QUADRATURE = 102.8768        # ln Z of _evidence_problem() by the 96^3 midpoint rule (test_gpu_ns.py computes it with the C oracle)


def _logl(fit):
    return lambda U: fit.loglike_cube_batch(U, return_theta=False)


def _init_of(logl):
    """The initial points' values: a row with a NaN or outside the cube takes -inf unless its logL is NaN."""
    def init(U):
        L = np.array(logl(U), dtype=float)
        with np.errstate(invalid="ignore"):
            out = ~((U >= 0.0) & (U <= 1.0)).all(axis=1)
            L[out & (L > -np.inf)] = -np.inf
        return L
    return init


class Dev:
    """One run through the C ABI."""

    def __init__(self, fit, U0, K, nmoves, max_steps, seed=0, dlogz=0.0, max_dead=None):
        self.fit, self.lib, self.ctx = fit, fit._lib, fit._ctx
        self.U0 = np.ascontiguousarray(U0, dtype=float)
        self.nlive, self.ndim, self.K = self.U0.shape[0], self.U0.shape[1], K
        fit._ensure_prior()
        self.opts = _lib.mcalf_nested_opts(K, nmoves, max_steps, 0, seed, dlogz, self.nlive + 64 * K if max_dead is None else max_dead)
        self.st = _lib.mcalf_nested_state_t()
        fit._call(self.lib.mcalf_nested_close)                    # (a run an earlier, failed test left open)
        fit._call(self.lib.mcalf_nested_open, self.U0.ctypes.data, self.nlive, C.addressof(self.opts))

    def advance(self, n):
        self.fit._call(self.lib.mcalf_nested_advance, n, C.addressof(self.st))
        return self.st.reason

    def last(self):
        dying, pick = np.empty(self.K, dtype=np.int32), np.empty(self.K, dtype=np.int32)
        D, lmin = np.empty((self.ndim, self.ndim)), np.empty(1)
        self.fit._call(self.lib.mcalf_nested_last_round, dying.ctypes.data, pick.ctypes.data, D.ctypes.data, lmin.ctypes.data)
        return dying, pick, D, float(lmin[0])

    def finish(self):
        z, e, h = C.c_double(), C.c_double(), C.c_double()
        self.fit._call(self.lib.mcalf_nested_finish, C.addressof(z), C.addressof(e), C.addressof(h))
        return z.value, e.value, h.value

    def read(self, logw=True):
        n = self.st.ndead if logw is False else self.st.ndead + self.nlive
        cube, theta, logL, lw = np.empty((n, self.ndim)), np.empty((n, self.ndim)), np.empty(n), np.empty(n)
        self.fit._call(self.lib.mcalf_nested_read, 0, n, cube.ctypes.data, theta.ctypes.data, logL.ctypes.data, lw.ctypes.data if logw else None)
        return cube, theta, logL, lw

    def close(self):
        self.fit._call(self.lib.mcalf_nested_close)


def _lockstep(fit, U0, K, nmoves, max_steps, seed, rounds, logl=None, dlogz=0.0, check_dirs=True):
    """The device and the reference round by round, the reference on the device's D: the selections must agree exactly and D
    must be the Cholesky factor of the survivors' covariance within the bound.  Returns (dev, run) with the device run open."""
    logl = logl or _logl(fit)
    dev = Dev(fit, U0, K, nmoves, max_steps, seed=seed, dlogz=dlogz)
    run = ref.Run(logl, U0, K, nmoves, max_steps, seed=seed, dlogz=dlogz, init=_init_of(logl))
    dev.lmins = []
    for r in range(rounds):
        alive = run.U[np.argsort(ref.key(run.L), kind="stable")[K:]]
        before = ref.key(run.L)
        got = dev.advance(1)
        dying, pick, D, lmin = dev.last()
        want = run.advance(1, D_of_round=lambda _: D)
        assert got == want, (r, got, want)
        if want != ref.BUDGET:
            break
        wd, wp, _, wl = run.last
        assert np.array_equal(dying, wd) and np.array_equal(pick, wp) and lmin == wl, r
        assert (before[pick] > lmin).all() and (before[dying] <= lmin).all(), r       # every start is strictly above the threshold
        dev.lmins.append(lmin)
        if check_dirs:
            _check_directions(D, alive)
        assert dev.st.rounds == run.rounds and dev.st.nevals == run.nevals and dev.st.unfinished == run.unfinished and dev.st.ndead == run.ndead
        assert dev.st.max_key == ref.key(run.L).max() and abs(dev.st.logX - run.ev.logX) <= 1e-12
        assert dev.st.logZ == run.ev.logZ or abs(dev.st.logZ - run.ev.logZ) <= 1e-9      # (-inf while only weightless points have died)
    return dev, run


def _check_directions(D, alive):
    """D is upper triangular as rows and D^T D is the survivors' covariance plus the jitter within
    4 (n_alive + ndim) eps max diag(cov): twice the sum of the Cholesky backward-error bound (ndim + 1) eps sqrt(a_ii a_jj) and
    a sequential-sum bound n_alive eps sqrt(a_ii a_jj) for the covariance (derived, not measured).  A non-finite covariance:
    the fallback, exactly."""
    n, ndim = alive.shape
    cov = np.atleast_2d(np.cov(alive, rowvar=False)) if n > 1 else np.zeros((ndim, ndim))
    var = np.diag(cov)
    if not np.isfinite(cov).all():
        std = np.sqrt(np.where(np.isfinite(var) & (var > 0.0), var, 0.0))
        assert np.array_equal(D, np.diag(np.where(std > 0.0, std, 1.0)))
        return
    assert not np.tril(D, -1).any()
    err = np.abs(D.T @ D - (cov + 1e-9 * max(var.mean(), 1e-300) * np.eye(ndim))).max()
    bar = 4.0 * (n + ndim) * EPS * var.max()
    print(f"ndim {ndim}, {n} survivors: max |D^T D - cov| = {err:.3e}, bar {bar:.3e}")
    if var.max() > 0.0:
        assert err <= bar


def _end_matches(dev, run, logl, fit):
    """Both finished: the dead cube by value, the dead logL by bytes, the counters, theta and logL against the entries."""
    st = dev.st
    assert (st.nevals, st.unfinished, st.rounds) == (run.nevals, run.unfinished, run.rounds)
    z, e, h = dev.finish()
    cube, theta, L, lw = dev.read()
    rz, rh, rlw, rcube, rL = run.finish()
    assert cube.shape == rcube.shape and np.array_equal(cube, rcube, equal_nan=True) and L.tobytes() == rL.tobytes()
    assert np.array_equal(theta, fit.scale_cube_batch(cube), equal_nan=True)
    inside = ((cube >= 0.0) & (cube <= 1.0)).all(axis=1)
    assert L[inside].tobytes() == np.asarray(logl(cube))[inside].tobytes()
    ok = np.isfinite(rlw)
    assert abs(z - rz) <= 1e-9 and abs(h - rh) <= 1e-9 and np.abs(lw[ok] - rlw[ok]).max() <= 1e-9 and np.isneginf(lw[~ok]).all()
    assert e == np.sqrt(max(h, 0.0) / dev.nlive) and abs(np.exp(lw).sum() - 1.0) <= 1e-12
    return cube, L, lw


@pytest.fixture(scope="module")
def tiny():
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        yield fit


# ---- a round, exactly ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nlive,K,rounds", [(8, 1, 6), (8, 2, 6), (8, 7, 4), (64, 16, 5), (65, 16, 5), (200, 16, 4), (200, 199, 3)])
def test_rounds_are_the_restatements(tiny, nlive, K, rounds):
    U0 = np.random.default_rng(nlive + K).random((nlive, 4))
    dev, run = _lockstep(tiny, U0, K, 4, 200, seed=nlive, rounds=rounds)
    try:
        assert dev.st.rounds == rounds and dev.st.reason == ref.BUDGET
        _end_matches(dev, run, _logl(tiny), tiny)
    finally:
        dev.close()


# ---- the direction rows ------------------------------------------------------------------------------------------------------------

def _one_round_directions(fit, nlive, K, seed):
    """One round without moves (nmoves = 0: the replacements are the starts themselves): the device's dying rows and D against
    the host's order and covariance of the same points."""
    U0 = np.random.default_rng(seed).random((nlive, fit.ndim))
    dev = Dev(fit, U0, K, 0, 0, seed=seed)
    try:
        assert dev.advance(1) == ref.BUDGET and dev.st.rounds == 1
        dying, pick, D, lmin = dev.last()
        order, wd, wl, r0, wp = ref.select(_logl(fit)(U0), K, seed, 0)
        assert np.array_equal(dying, wd) and np.array_equal(pick, wp) and lmin == wl
        _check_directions(D, U0[order[K:]])
    finally:
        dev.close()


def test_directions_two_lines_floated_resolution_and_continuum():
    kw, _ = _civ(npix=300, specres=(6.0, 9.0), contval=(0.9, 1.1))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.ndim == 15
        _one_round_directions(fit, 60, 15, seed=2)


@pytest.mark.parametrize("ndim", [65, 129])
def test_directions_where_a_lane_owns_several_coordinates(ndim):
    """ndim 65 and 129: a lane of the row kernels owns 2 and 3 coordinates; at 129 the packed triangle (67 080 bytes) is factored
    in HBM, at 65 in LDS."""
    with mcalf_amd.als_fitter(None, **mc.many(ndim)[0]) as fit:
        assert fit.ndim == ndim
        _one_round_directions(fit, 4 * ndim, ndim, seed=ndim)


# ---- ties and bad points -----------------------------------------------------------------------------------------------------------

def test_survivors_equal_to_the_threshold_are_not_starts(tiny):
    U0 = np.random.default_rng(5).random((16, 4))
    order = np.argsort(_logl(tiny)(U0), kind="stable")
    U0[order[4]] = U0[order[5]] = U0[order[3]]                    # the K-th point twice more: two survivors sit on lmin
    dev, run = _lockstep(tiny, U0, 4, 4, 200, seed=1, rounds=1)
    try:
        dying, pick, D, lmin = dev.last()
        L0 = _logl(tiny)(U0)
        assert (L0 == lmin).sum() == 3 and (L0[dying] == lmin).sum() == 1
        assert (L0[pick] > lmin).all() and not np.isin(pick, np.flatnonzero(L0 == lmin)).any()
        for _ in range(3):
            assert dev.advance(1) == run.advance(1, D_of_round=lambda _: dev.last()[2]) == ref.BUDGET
        _end_matches(dev, run, _logl(tiny), tiny)
    finally:
        dev.close()


def test_a_live_set_of_equal_rows_is_a_plateau(tiny):
    U0 = np.tile(np.random.default_rng(6).random((1, 4)), (12, 1))
    dev = Dev(tiny, U0, 3, 4, 200)
    try:
        assert dev.advance(5) == ref.PLATEAU and dev.st.ndead == 0 and dev.st.rounds == 0 and dev.st.nevals == 12
        z, e, h = dev.finish()
        cube, theta, L, lw = dev.read()
        assert cube.shape == (12, 4) and np.array_equal(cube, U0) and abs(np.exp(lw).sum() - 1.0) <= 1e-12
        rz, rh, rlw = ref.finish(L, 12, 3)
        assert abs(z - rz) <= 1e-9 and abs(h - rh) <= 1e-9
    finally:
        dev.close()


def test_bad_initial_points_die_first_without_weight(tiny):
    """A NaN row, a row of NaN in one coordinate and two rows outside the cube among 16: they sort first (logL NaN or -inf), die
    in the first round and carry no weight."""
    U0 = np.random.default_rng(7).random((16, 4))
    U0[2] = np.nan
    U0[5, 1] = np.nan
    U0[9, 2] = 1.5
    U0[11, 3] = -1e-300
    bad = [2, 5, 9, 11]
    dev, run = _lockstep(tiny, U0, 4, 4, 200, seed=2, rounds=3, check_dirs=False)
    try:
        cube, L, lw = _end_matches(dev, run, _logl(tiny), tiny)
        assert np.array_equal(cube[:4], U0[bad], equal_nan=True)
        assert (np.isnan(L[:4]) | np.isneginf(L[:4])).all() and np.isneginf(lw[:4]).all() and np.isfinite(lw[4:]).all()
    finally:
        dev.close()


@pytest.fixture(scope="module")
def vetoing():
    """(fit, vetoed cube rows, finite cube rows): veto thresholds of 10 pixels above 4 sigma and 5 above 5 sigma, under which two
    thirds of uniform draws have logL = -inf from the likelihood itself (the fitter of tests/test_gpu_ens.py)."""
    with mcalf_amd.als_fitter(None, Asymmlike=True, gauss_cdf=[50, 10, 5], **tiny_problem(64)) as fit:
        draws = np.random.default_rng(3).random((512, fit.ndim))
        L0 = _logl(fit)(draws)
        assert np.isneginf(L0).sum() >= 64 and np.isfinite(L0).sum() >= 64
        yield fit, draws[np.isneginf(L0)], draws[np.isfinite(L0)]


@pytest.mark.parametrize("nveto,nfinite,K,rounds", [(3, 29, 8, 3), (21, 11, 8, 4), (13, 3, 4, 5)])
def test_vetoed_initial_rows_die_first_without_weight(vetoing, nveto, nfinite, K, rounds):
    """In-cube rows whose likelihood is -inf (the replacement call refuses them as starts, nothing rewrites their logL), mixed
    with finite rows: fewer than K, and more than K so that lmin = -inf for several rounds with -inf survivors that are not
    starts.  They die first, in index order, with logw = -inf; every pick is above lmin (asserted round by round in _lockstep);
    trials of the chains are vetoed too and never accepted."""
    fit, vetoed, finite = vetoing
    rows = np.concatenate([vetoed[:nveto], finite[:nfinite]])
    U0 = rows[np.random.default_rng(nveto).permutation(nveto + nfinite)]
    L0 = _logl(fit)(U0)
    assert np.isneginf(L0).sum() == nveto and ((U0 >= 0.0) & (U0 <= 1.0)).all()
    dev, run = _lockstep(fit, U0, K, 4, 200, seed=nveto, rounds=rounds)
    try:
        assert dev.st.rounds == rounds and sum(l == -np.inf for l in dev.lmins) == nveto // K
        cube, L, lw = _end_matches(dev, run, _logl(fit), fit)
        assert np.array_equal(cube[:nveto], U0[np.isneginf(L0)]) and np.isneginf(L[:nveto]).all() and np.isneginf(lw[:nveto]).all()
        assert np.isfinite(L[nveto:]).all() and np.isfinite(lw[nveto:]).all()
    finally:
        dev.close()


def test_more_nan_rows_than_a_round_retires(tiny):
    """5 NaN rows, K = 2: the survivors hold a NaN in rounds 0 and 1 and D is the identity; from round 2 on it is the factor."""
    U0 = np.random.default_rng(8).random((16, 4))
    U0[[1, 4, 6, 10, 13]] = np.nan
    dev, run = _lockstep(tiny, U0, 2, 4, 200, seed=3, rounds=2, check_dirs=True)
    try:
        assert np.array_equal(dev.last()[2], np.eye(4))
        got = dev.advance(1)
        D = dev.last()[2]
        assert got == run.advance(1, D_of_round=lambda _: D) == ref.BUDGET
        assert not np.array_equal(D, np.eye(4)) and np.isfinite(D).all() and not np.tril(D, -1).any()
        _end_matches(dev, run, _logl(tiny), tiny)
    finally:
        dev.close()


# ---- invariance, by bytes ------------------------------------------------------------------------------------------------------------

def _whole_run(fit, U0, cuts, K=16, seed=4):
    dev = Dev(fit, U0, K, 4, 200, seed=seed)
    try:
        for n in cuts:
            assert dev.advance(n) == ref.BUDGET
        out = (dev.st.rounds, dev.st.nevals, dev.st.unfinished, dev.st.ndead) + dev.finish() + dev.read()
    finally:
        dev.close()
    return out


def _footprint(fit):
    n = C.c_int64(-1)
    fit._call(fit._lib.mcalf_nested_footprint, C.byref(n))
    return n.value


def _same_run(a, b):
    return a[:7] == b[:7] and all(x.tobytes() == y.tobytes() for x, y in zip(a[7:], b[7:]))


def test_a_run_does_not_depend_on_the_cut_the_packing_or_the_device_count(tiny):
    U0 = np.random.default_rng(9).random((64, 4))
    whole = _whole_run(tiny, U0, [12, 0])
    assert whole[0] == 12 and whole[3] == 12 * 16
    held = _footprint(tiny)
    assert held >= (64 + 64 * 16 + 64) * 5 * 8                             # (the live and the dead rows at least)
    assert _same_run(whole, _whole_run(tiny, U0, [5, 7]))                  # the second run of the context ...
    assert _footprint(tiny) == held                                        # ... allocates nothing: its buffers are the first's
    assert _same_run(whole, _whole_run(tiny, U0, [1] * 12))
    tiny.set_slice_compact(True)
    try:
        assert _same_run(whole, _whole_run(tiny, U0, [12]))
    finally:
        tiny.set_slice_compact(False)
    assert not _same_run(whole, _whole_run(tiny, U0, [12], seed=5))
    assert _footprint(tiny) == held
    with mcalf_amd.als_fitter(None, device=[0, 0], **tiny_problem(64)) as multi:
        assert _footprint(multi) == 0
        assert _same_run(whole, _whole_run(multi, U0, [5, 7]))
        first = _footprint(multi)
        assert first > 0 and _same_run(whole, _whole_run(multi, U0, [12])) and _footprint(multi) == first


def test_a_run_under_a_gaussian_prior_works_on_the_sum(tiny):
    """dead logL = logL + lnprior, against the reference with that sum as its callable (tests/test_gpu_prior.py does the same for
    the host driver)."""
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        span = fit._hi - fit._lo
        mu, sigma = np.zeros(4), np.zeros(4)
        for k in (1, 3):
            sigma[k] = 0.1 * span[k]
            mu[k] = fit._lo[k] + 0.5 * span[k] + 0.5 * sigma[k]
        fit.set_gauss_prior(mu, sigma)
        post = lambda U: _logl(fit)(U) + fit.lnprior_batch(U, cube=True)
        U0 = np.random.default_rng(10).random((32, 4))
        dev, run = _lockstep(fit, U0, 8, 4, 200, seed=6, rounds=4, logl=post)
        try:
            cube, L, lw = _end_matches(dev, run, post, fit)
            assert not L.tobytes() == _logl(fit)(cube).tobytes()
        finally:
            dev.close()


# ---- refusals that need a context ----------------------------------------------------------------------------------------------------

def test_refusals_with_a_context():
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        lib, ctx = fit._lib, fit._ctx
        err = lambda: lib.mcalf_last_error(ctx)
        U0 = np.random.default_rng(11).random((16, 4))
        opts = _lib.mcalf_nested_opts(4, 4, 200, 0, 0, 0.0, 64)
        st = _lib.mcalf_nested_state_t()
        assert fit._prior_key is None                                      # (the fitter sends its box on first use: none is set yet)
        assert lib.mcalf_nested_open(ctx, U0.ctypes.data, 16, C.addressof(opts)) == _lib.MCALF_ERR_INVALID and b"mcalf_set_prior has not been called" in err()
        fit._ensure_prior()
        for name, call in (("advance", lambda: lib.mcalf_nested_advance(ctx, 1, C.addressof(st))), ("finish", lambda: lib.mcalf_nested_finish(ctx, None, None, None)),
                           ("read", lambda: lib.mcalf_nested_read(ctx, 0, 0, None, None, None, None)),
                           ("last_round", lambda: lib.mcalf_nested_last_round(ctx, None, None, None, None))):
            assert call() == _lib.MCALF_ERR_INVALID and b"mcalf_nested_" + name.encode() + b": no run is open" in err(), name
        assert lib.mcalf_nested_close(ctx) == 0
        huge = _lib.mcalf_nested_opts(4, 4, 200, 0, 0, 0.0, (4 << 30) // 40)
        assert lib.mcalf_nested_open(ctx, U0.ctypes.data, 16, C.addressof(huge)) == _lib.MCALF_ERR_RANGE
        assert b"the largest max_dead for this run is %d" % ((4 << 30) // 40 - 16) in err()
        assert lib.mcalf_nested_open(ctx, U0.ctypes.data, 16, C.addressof(opts)) == 0
        assert lib.mcalf_nested_open(ctx, U0.ctypes.data, 16, C.addressof(opts)) == _lib.MCALF_ERR_INVALID and b"a run is already open" in err()
        assert lib.mcalf_nested_last_round(ctx, None, None, None, None) == _lib.MCALF_ERR_INVALID and b"has not selected a round yet" in err()
        lw = np.empty(4)
        assert lib.mcalf_nested_advance(ctx, 1, C.addressof(st)) == 0 and st.ndead == 4
        assert lib.mcalf_nested_read(ctx, 0, 4, None, None, None, lw.ctypes.data) == _lib.MCALF_ERR_INVALID and b"logw exists only after" in err()
        assert lib.mcalf_nested_read(ctx, 2, 3, None, None, None, None) == _lib.MCALF_ERR_INVALID and b"outside the 4 dead rows" in err()
        assert lib.mcalf_nested_finish(ctx, None, None, None) == 0
        assert lib.mcalf_nested_advance(ctx, 1, None) == _lib.MCALF_ERR_INVALID and b"the run is finished" in err()
        assert lib.mcalf_nested_finish(ctx, None, None, None) == _lib.MCALF_ERR_INVALID
        lw = np.empty(20)
        assert lib.mcalf_nested_read(ctx, 0, 20, None, None, None, lw.ctypes.data) == 0 and abs(np.exp(lw).sum() - 1.0) <= 1e-12
        assert lib.mcalf_nested_close(ctx) == 0 and lib.mcalf_nested_close(ctx) == 0


# ---- the stop and the full buffer ----------------------------------------------------------------------------------------------------

def test_the_run_stops_where_the_restatement_stops(tiny):
    U0 = np.random.default_rng(12).random((32, 4))
    dev, run = _lockstep(tiny, U0, 8, 4, 200, seed=7, rounds=400, dlogz=1e-3, check_dirs=False)
    try:
        assert dev.st.reason == ref.CONVERGED and dev.st.rounds == run.rounds and 3 < run.rounds < 400
        print(f"{run.rounds} rounds; the smallest stop margin was {min(run.margins):.3e}")
        assert min(run.margins) > 1e-9
        _end_matches(dev, run, _logl(tiny), tiny)
    finally:
        dev.close()


def test_a_full_dead_buffer_ends_the_run_and_finish_still_works(tiny):
    U0 = np.random.default_rng(13).random((32, 4))
    dev = Dev(tiny, U0, 8, 4, 200, seed=8, max_dead=32 + 3 * 8)             # a fourth round would not leave room for the last 32
    try:
        assert dev.advance(4) == ref.FULL and dev.st.rounds == 3 and dev.st.ndead == 24
        z, e, h = dev.finish()
        cube, theta, L, lw = dev.read()
        assert L.size == 56 and (np.diff(L) >= 0.0).all() and abs(np.exp(lw).sum() - 1.0) <= 1e-12
        rz, rh, rlw = ref.finish(L, 32, 8)
        assert abs(z - rz) <= 1e-9 and abs(h - rh) <= 1e-9 and np.abs(lw - rlw).max() <= 1e-9
    finally:
        dev.close()


def test_the_python_function_warns_when_the_dead_rows_fill_up(tiny):
    with pytest.warns(RuntimeWarning, match="dead rows were full after 2 rounds"):
        res = nested_device.nested_sample_device(tiny, nlive=32, batch=8, nmoves=4, max_steps=200, seed=1, max_dead=32 + 2 * 8)
    assert res.stop_reason == 3 and res.rounds == 2 and res.logL.size == 48 and abs(np.exp(res.logw).sum() - 1.0) <= 1e-12


# ---- evidence end to end -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", [0, 1, 2])
def test_the_python_function_finds_the_evidence(seed, tmp_path):
    """|ln Z - quadrature| <= 4 sqrt(H / nlive), 4 standard errors of the nested-sampling estimator; ln Z, H and the weights are
    the numpy restatement's over the same dead logL.  Measured on one MI355X: seeds 0, 1, 2 lie 0.40, 0.41 and 0.33 standard errors
    (0.179 each) from the quadrature, after 58, 59 and 58 rounds."""
    with mcalf_amd.als_fitter(None, **_evidence_problem()) as fit:
        res = nested_device.nested_sample_device(fit, nlive=256, batch=64, nmoves=8, max_steps=200, seed=seed)
        err = np.sqrt(res.H / 256)
        print(f"seed {seed}: ln Z {res.logZ:.4f}, quadrature {QUADRATURE:.4f}: {abs(res.logZ - QUADRATURE) / err:.2f} standard errors of {err:.4f}; "
              f"H {res.H:.3f}, {res.rounds} rounds, {res.nevals} evaluations, {res.unfinished} unfinished, {res.rows_launched} rows launched")
        assert abs(res.logZ - QUADRATURE) <= 4.0 * err
        assert res.stop_reason == 1 and res.logL.size == res.rounds * 64 + 256 and res.lnprior is None and res.rows_launched >= res.nevals
        rz, rh, rlw = ref.finish(res.logL, 256, 64)
        assert abs(res.logZ - rz) <= 1e-9 and abs(res.H - rh) <= 1e-9 and np.abs(res.logw - rlw).max() <= 1e-9
        assert res.logZ_err == err and abs(np.exp(res.logw).sum() - 1.0) <= 1e-12 and (np.diff(res.logL) >= 0.0).all()
        assert np.array_equal(res.theta, fit.scale_cube_batch(res.cube))
        assert res.logL.tobytes() == _logl(fit)(res.cube).tobytes()
        ll, th = res.equal_weight_samples(np.random.default_rng(seed))
        path = str(tmp_path / "run_equal_weights.txt")
        write_equal_weights(path, ll, th)
        chain = np.loadtxt(path, ndmin=2)
        assert chain.shape == (ll.size, 2 + fit.ndim) and ll.size > 20
        assert np.isin(chain[:, 1], -2.0 * res.logL).all() and (chain[:, 0] == 1.0).all()
