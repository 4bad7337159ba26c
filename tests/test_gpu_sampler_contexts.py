"""GPU: the samplers and the fitter on every route `launch()` can take.  The ensemble sampler, parallel tempering, nested
sampling's slice moves, the device-resident nested run, HMC, the run to convergence and the Levenberg-Marquardt fit are tested
elsewhere on one kind of context only (one tile, a narrow LSF, numpy convolution, clean pixels, one row block, launches below
the persistent grid).  Here the same harnesses -- imported from those modules, with their comparisons by bytes -- run on the
contexts of tests/hard_contexts.py: two tiles (the finalize kernel behind every fused launch), a wide LSF (launch_wide: four
kernels per pass), both, JAX convolution semantics, bad pixels, the asymmetric veto, three row blocks on the auxiliary streams,
and a half-ensemble large enough for the persistent grid with its ordered hand-out.  tests/test_sampler_contexts_host.py checks
on the CPU that these inputs do what the tests below rely on.

A restatement driven by the public cube entry shares that entry's launch with the sampler, so once per context the sampler's
last state is also compared with the numpy oracle at the bar of tests/test_gpu_wide_lsf.py; and after each run `last_launch()`
must show the path the context is here for.  Sizes: 64 walkers or rows, 6 iterations kept every second one, start balls of
half-width 0.05 round the best of 128 uniform draws, unless a test says otherwise."""
import contextlib
import types

import numpy as np
import pytest
import torch

import fit_reference as fr
import hard_contexts as hc
import mcalf_amd
import nsrun_reference as nsr
import test_gpu_converge as tcv
import test_gpu_ens as tens
import test_gpu_fit as tfit
import test_gpu_hmc as thm
import test_gpu_ns as tns
import test_gpu_nsrun as tnr
import test_gpu_pt as tpt
from cases import problem_from_kwargs
from mcalf_amd import convergence, ensemble, nested

pytestmark = pytest.mark.gpu

N, NSTEPS, THIN = 64, 6, 2
MOVES = ["stretch", "de"]


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _config(fit):
    """The knobs the context runs under (`get_config`), as a dict of strings."""
    text = fit.get_config().split(" [env:")[0]
    return dict(word.split("=", 1) for word in text.split() if "=" in word)


def _open(name):
    """The context `name` with what the tests need of it; what the table of hard_contexts.py says of it is asserted here."""
    kw = hc.kwargs(name)
    fit = mcalf_amd.als_fitter(None, **kw)
    try:
        c = types.SimpleNamespace(name=name, kw=kw, fit=fit, prob=problem_from_kwargs(kw), wide=hc.is_wide(kw),
                                  cus=torch.cuda.get_device_properties(0).multi_processor_count, config=_config(fit))
        c.logl = lambda U: fit.loglike_cube_batch(U, return_theta=False)
        assert fit.ndim == c.prob.ndim
        assert (2 * fit.info.n_cap + 64 > hc.TILE) == c.wide == (name in ("wide", "wide_two_tile")) == (c.config["wide_lsf"] != "0")
        assert fit.info.ntiles == (2 if name in ("two_tile", "wide_two_tile") else 1)
        if c.wide:
            assert fit.info.n_cap == hc.n_cap(kw)
        if name == "chunked":
            fit.set_chunks(hc.CHUNKS)
        if name == "bad_pixels":
            rows = np.random.default_rng(7).random((32, fit.ndim))
            with mcalf_amd.als_fitter(None, **hc.bad_pixels_clean()) as clean:
                got, want = c.logl(rows), clean.loglike_cube_batch(rows, return_theta=False)
            assert np.isfinite(got).all() and np.isfinite(want).all() and (got != want).all()
        if name == "veto":
            c.best = hc.VETO_CENTRE
        else:
            draws = hc.draws(fit.ndim)
            c.best = draws[np.nanargmax(c.logl(draws))]
        assert np.isfinite(c.logl(c.best[None])[0])
        return c
    except BaseException:
        fit.close()
        raise


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(name):
        if name not in made:
            made[name] = _open(name)
        return made[name]
    yield get
    for c in made.values():
        c.fit.close()


def _starts(c, n, seed=hc.BALL_SEED):
    """`n` rows of the context's start ball; on `veto` the first n rows of its ball that are not vetoed."""
    if c.name != "veto":
        return hc.ball(c.best, hc.BALL, n, seed)
    rows = hc.veto_ball(8 * n, seed)
    L = c.logl(rows)
    assert 0.1 <= np.isneginf(L).mean() <= 0.9 and np.isfinite(L).sum() >= n
    return np.ascontiguousarray(rows[np.isfinite(L)][:n])


def _check_path(c, info, rows):
    """`info`: `last_launch()` right behind a sampler call whose last likelihood launch had `rows` rows.  The row blocks or passes,
    the work items of the last of them, and whether that launch took the persistent grid, the ordered hand-out and the
    one-launch variant, each as host_launch.cpp decides it under the context's own knobs."""
    fit, slots = c.fit, 2 * c.cus
    if c.wide:
        per = hc.wide_rows_per_pass(fit.info.npix, fit.info.n_cap, rows)
        blocks = -(-rows // per)
        last = rows - (blocks - 1) * per
    elif c.name == "chunked":
        blocks = hc.CHUNKS
        last = rows - rows * (blocks - 1) // blocks
    else:
        blocks, last = 1, rows
    items = last * fit.info.ntiles
    assert info.row_blocks == blocks and info.items == items, (info.row_blocks, blocks, info.items, items)
    persistent = c.config["persist"] != "0" and items >= 4 * slots
    ordered = persistent and c.config["order"] != "0" and info.selfhalo != 0 and items <= 16 * slots
    inline = not persistent and items <= int(c.config["inline_max"])
    assert (info.persistent, info.ordered, info.inline_setup) == (int(persistent), int(ordered), int(inline))
    assert info.grid == (slots if persistent else items)
    if c.name == "persistent":
        assert info.persistent == 1 and info.ordered == 1
    return info


def _anchor(c, U, L=None):
    """The public cube entry's logL of the rows U (or `L`, its bits) against the numpy oracle, under the context's own semantics,
    at the bar of tests/test_gpu_wide_lsf.py."""
    theta, got = c.fit.loglike_cube_batch(U)
    assert L is None or np.asarray(L).tobytes() == got.tobytes()
    want = hc.oracle_loglike(c.kw, theta)
    assert np.isfinite(want).all() and np.isfinite(got).all()
    err = np.abs(got - want)
    print(f"{c.name}: {len(want)} rows, largest |logL - oracle| {err.max():.3e}, smallest bar {(1e-10 * np.abs(want) + 1e-9).min():.3e}")
    assert np.all(err < 1e-10 * np.abs(want) + 1e-9)


# ---- the ensemble sampler ----------------------------------------------------------------------------------------------------

ENS = [(name, N) for name in hc.NAMES if name != "persistent"] + [("two_tile", 130), ("wide", 130), ("persistent", None)]


def _ens_sizes(c, n):
    """(walkers, iterations, thin): 64 x 6 kept every second; on `persistent` the smallest ensemble whose half takes the
    persistent grid (4096 walkers on 256 compute units) for 3 iterations."""
    return (hc.persistent_walkers(c.cus), 3, 1) if n is None else (n, NSTEPS, THIN)


@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("name,n", ENS)
def test_ensemble_trajectories(contexts, name, n, move):
    """A half of 32 walkers, of 65 (it crosses a wave) and of 2048.  On `veto` trial rows are vetoed and no walker ends on one; on
    `chunked` the run is also the run of a context that never heard of row blocks."""
    c = contexts(name)
    fit = c.fit
    n, nsteps, thin = _ens_sizes(c, n)
    U0 = _starts(c, n)
    seen = []

    def logl(U):
        out = c.logl(U)
        seen.append(out)
        return out
    got = tens._against_reference(fit, U0, nsteps, thin, move, seed=11, logl=logl)
    U, theta, L, status, naccept, CU, CL = got
    assert CU.shape == (nsteps // thin, n, fit.ndim) and (status == 0).all()
    print(f"{name}, {n} walkers, {move}: accepted {naccept.sum()} of {nsteps * n}")
    assert 0 < naccept.sum() < nsteps * n
    again = fit.ensemble_batch(U0, nsteps, thin=thin, move=move, seed=11)
    info = fit.last_launch()
    assert _same(again, got)
    _check_path(c, info, n // 2)
    if name == "veto":
        trials = np.concatenate(seen[1:])
        assert np.isneginf(trials).any() and np.isfinite(trials).any()
        assert np.isfinite(L).all() and np.isfinite(CL).all()
    if name == "chunked":
        with mcalf_amd.als_fitter(None, **c.kw) as plain:
            want = plain.ensemble_batch(U0, nsteps, thin=thin, move=move, seed=11)
            assert plain.last_launch().row_blocks == 1 and _same(want, got)


def test_ensemble_on_a_wide_batch_of_several_passes(contexts):
    """One more walker per half than a pass of the wide launch holds: the start launch makes three passes, every half-step two
    (the second of one row), each into its own rows of the trial logL.  The walkers at the passes' edges against the oracle."""
    c = contexts("wide")
    fit = c.fit
    per = hc.wide_rows_per_pass(fit.info.npix, fit.info.n_cap, 1 << 30)
    n = 2 * (per + 1)
    U0 = hc.ball(c.best, hc.BALL, n)
    got = tens._against_reference(fit, U0, 2, 1, "stretch", seed=5)
    again = fit.ensemble_batch(U0, 2, move="stretch", seed=5)
    info = fit.last_launch()
    assert _same(again, got) and info.row_blocks == 2
    _check_path(c, info, per + 1)
    print(f"{n} walkers, {per} rows per pass: accepted {got[4].sum()} of {2 * n}")
    assert 0 < got[4].sum() < 2 * n
    edges = [0, 1, per - 1, per, per + 1, 2 * per - 1, 2 * per, n - 1]
    want = hc.oracle_cube_loglike(c.kw, got[0][edges])
    assert np.all(np.abs(got[2][edges] - want) < 1e-10 * np.abs(want) + 1e-9)


@pytest.mark.parametrize("name", hc.NAMES)
def test_the_samplers_last_state_against_the_oracle(contexts, name):
    """Same bits as the public entry is not yet the right value: a defect that the sampler's inner launch shares with that
    entry would pass every comparison with a restatement."""
    c = contexts(name)
    n, nsteps, thin = _ens_sizes(c, None if name == "persistent" else N)
    U, _, L = c.fit.ensemble_batch(_starts(c, n), nsteps, thin=thin, seed=11, chain=False)[:3]
    _anchor(c, U, L)


# ---- parallel tempering --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("move", MOVES)
@pytest.mark.parametrize("name", ["two_tile", "wide", "jax", "veto", "chunked"])
def test_tempered_trajectories(contexts, name, move):
    """Three rungs down to beta = 0, a swap round after every second iteration: 96 trial rows per launch."""
    c = contexts(name)
    fit = c.fit
    T, betas = 3, tpt.LADDERS[3]
    U0 = _starts(c, T * N).reshape(T, N, fit.ndim)
    got = tpt._against_reference(fit, U0, betas, NSTEPS, THIN, 2, move, seed=13)
    U, theta, L, status, naccept, nswap, CU, CL = got
    print(f"{name}, {move}: accepted {naccept.sum(axis=1)} of {NSTEPS * N} per rung, swaps {nswap.sum(axis=1)} of {tpt._drawn(NSTEPS, 2, T, N)}")
    assert (status == 0).all() and 0 < naccept.sum() < NSTEPS * N * T and tpt._drawn(NSTEPS, 2, T, N).sum() > 0
    assert CU.shape == (NSTEPS // THIN, 1, N, fit.ndim) and CL.shape == (NSTEPS // THIN, T, N)
    again = fit.tempered_batch(U0, betas, NSTEPS, thin=THIN, swap_every=2, move=move, seed=13)
    info = fit.last_launch()
    assert _same(again, got)
    _check_path(c, info, T * N // 2)
    if name == "veto":
        assert np.isfinite(L).all() and np.isfinite(CL).all()


# ---- nested sampling's slice moves ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_tile", "wide", "jax", "bad_pixels", "veto", "chunked"])
def test_slice_moves_under_the_median_constraint(contexts, name):
    """64 chains of 3 moves from live points above the median of 128.  On `veto` the live points are the veto ball's, the median
    is that of the rows that are not vetoed, and 12 of the starts are vetoed themselves -- 8 under the constraint and 4 under
    none, where -inf is still not above -inf: status -1, the row as given, no trial (the conventions of
    test_gpu_ns.py::test_bad_starts_faces_and_direction_sets)."""
    c = contexts(name)
    fit = c.fit
    live = hc.veto_ball(128) if name == "veto" else hc.draws(fit.ndim)
    L = c.logl(live)
    lmin = float(np.median(L[np.isfinite(L)]))
    U0 = tns._starts(live, L, lmin, N, np.random.default_rng(4))
    D = nested.directions(live[L > lmin])
    Lmin = np.full(N, lmin)
    nbad = 0
    if name == "veto":
        vetoed = live[np.isneginf(L)]
        assert vetoed.shape[0] >= 12
        nbad = 12
        U0[:12] = vetoed[:12]
        Lmin[8:12] = -np.inf
    sid = np.arange(N, dtype=np.uint64) + np.uint64(7)
    got = tns._against_reference(fit, U0, Lmin, D, sid, 3, 150, seed=17)
    U, theta, Lg, status, nevals, moves = got
    print(f"{name}: status {np.bincount(status + 1, minlength=3)} (-1, 0, 1), trials {nevals.sum()}, moves {moves.sum()}")
    assert (status[:nbad] == -1).all() and np.array_equal(U[:nbad], U0[:nbad]) and not nevals[:nbad].any() and np.isneginf(Lg[:nbad]).all()
    assert (status[nbad:] >= 0).all() and (Lg[nbad:] > lmin).all() and moves[nbad:].sum() > 0 and (nevals[nbad:] > 0).all()
    # the device entry issues its 150 steps in one go, nothing is read back between them
    rc, dev = tns._device_call(fit, U0, Lmin, D, sid, 3, 150, seed=17)
    info = fit.last_launch()
    assert rc == 0 and _same(dev, got)
    _check_path(c, info, N)


# ---- the device-resident nested run ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["two_tile", "wide", "bad_pixels", "chunked"])
def test_nested_run_rounds(contexts, name):
    """64 live points, 16 replaced per round, three rounds in lock step with the restatement and a fourth for the path."""
    c = contexts(name)
    fit = c.fit
    U0 = np.random.default_rng(21).random((N, fit.ndim))
    dev, run = tnr._lockstep(fit, U0, 16, 4, 200, seed=3, rounds=3)
    try:
        assert dev.st.rounds == 3 and dev.st.reason == nsr.BUDGET and dev.st.ndead == 48
        got = dev.advance(1)
        info = fit.last_launch()
        D = dev.last()[2]
        assert got == run.advance(1, D_of_round=lambda _: D) == nsr.BUDGET
        assert info.row_blocks == (hc.CHUNKS if name == "chunked" else 1) and info.persistent == 0
        tnr._end_matches(dev, run, c.logl, fit)
    finally:
        dev.close()


def test_a_whole_short_nested_run_on_two_tiles(contexts):
    c = contexts("two_tile")
    fit = c.fit
    U0 = np.random.default_rng(22).random((N, fit.ndim))
    whole = tnr._whole_run(fit, U0, [3, 0])
    assert whole[0] == 3 and whole[3] == 3 * 16
    assert tnr._same_run(whole, tnr._whole_run(fit, U0, [1, 2]))
    fit.set_slice_compact(True)
    try:
        assert tnr._same_run(whole, tnr._whole_run(fit, U0, [3]))
    finally:
        fit.set_slice_compact(False)
    cube, theta, L, lw = whole[7:]
    assert cube.shape == (3 * 16 + N, fit.ndim) and np.array_equal(theta, fit.scale_cube_batch(cube))
    assert L.tobytes() == c.logl(cube).tobytes() and (np.diff(L) >= 0.0).all() and abs(np.exp(lw).sum() - 1.0) <= 1e-12
    _anchor(c, cube[-16:], L[-16:])


# ---- Hamiltonian Monte Carlo -------------------------------------------------------------------------------------------------------

# Steps (scale 0.05 per coordinate) at which the restatement over the numpy gradient of tests/grad_reference.py, from these
# starts, accepts 154, 126 and 126 of its 256 trajectories on `two_tile`, `jax` and `bad_pixels` (15 times the pixels make
# `two_tile`'s logL that much steeper: at 0.02 it accepts none), and all of them on `wide`, whose model is flat under its LSF.
HMC_EPS = {"two_tile": 0.005, "wide": 0.02, "jax": 0.02, "bad_pixels": 0.02}


@pytest.mark.parametrize("name", ["two_tile", "wide", "jax", "bad_pixels", "veto"])
def test_hmc_trajectories(contexts, name):
    """Trajectories of 3 steps, 4 iterations, driven by the device's `loglike_grad_batch` as in test_gpu_hmc.py.  On `veto` the
    walkers start all over the veto ball: those that start vetoed are refused, and trajectories of the others run into the
    veto and die."""
    c = contexts(name)
    fit = c.fit
    if name == "veto":
        U0, scale, eps = hc.veto_ball(N), thm.TINY_SCALE, 0.2
    else:
        U0, scale, eps = hc.ball(np.clip(c.best, 0.1, 0.9), hc.BALL, N), np.full(fit.ndim, 0.05), HMC_EPS[name]
    trace = []
    got = thm._against_reference(fit, U0, 4, eps, 3, scale, thin=2, seed=19, trace=trace)
    U, theta, L, status, naccept, ndead, CU, CL = got
    died = sum(len(t[3]) for t in trace if t[0] == "dead")
    print(f"{name}: refused {(status == -1).sum()}, accepted {naccept.sum()} of {4 * (status == 0).sum()}, dead {ndead.sum()}")
    assert CU.shape == (2, N, fit.ndim) and ndead.sum() == died
    if name == "veto":
        L0 = c.logl(U0)
        assert 0.1 * N <= np.isneginf(L0).sum() <= 0.9 * N and (status[np.isneginf(L0)] == -1).all()
        assert (status == 0).sum() >= 16 and ndead.sum() > 0 and naccept.sum() > 0
        assert np.isfinite(L[status == 0]).all() and np.isfinite(CL[:, status == 0]).all()
    else:
        assert (status == 0).all() and np.isfinite(L).all()
        assert naccept.sum() > 0 and (name == "wide" or naccept.sum() < 4 * N)


# ---- the run to convergence --------------------------------------------------------------------------------------------------------

def _short_run(c):
    """12 iterations checked every 4 with factor 1000: three checks, none of which can stop the run."""
    res = convergence.ensemble_sample_until(c.fit, N, 12, check_every=4, factor=1000.0, start=c.best, ball=hc.BALL, seed=tcv.SEED)
    assert not res.converged and res.nsteps == 12 and res.cube.shape[0] == 12 and res.nchecks == 3
    assert res.tau_history.shape == (3, c.fit.ndim)
    return res


@pytest.mark.parametrize("name", ["two_tile", "wide"])
def test_a_run_that_cannot_converge_is_the_plain_sampler(contexts, name):
    """By bytes the run of `ensemble_batch`, and the stopping rule replayed on its chain stops it nowhere."""
    c = contexts(name)
    res = _short_run(c)
    tcv._same_as_the_plain_sampler(c.fit, res, ensemble._draw_starts(tcv.SEED, (N, c.fit.ndim), c.best, hc.BALL))
    stop, hist, Ts, refs = tcv._replay(res, 4, 1000.0, 0.01)
    assert stop is None and Ts == [4, 8, 12]


@pytest.mark.parametrize("name", ["two_tile", "wide"])
def test_the_tau_history_of_a_short_run_within_the_bound_of_test_gpu_converge(contexts, name):
    """tau of the three checks against chain_reference within test_gpu_converge.py's bound 16 (M + 1) (T + 3) 2^-53, which
    counts the rounding of the sums c_w(tau) and takes the centred values as exact to their own rounding.  After 4 or 8 steps
    a walker whose only accepted stretch had z close to 1 has hardly moved (on either context one walker's rms excursion in one
    coordinate is 9e-6, at x = 0.36 and x = 0.88), and centred as x_t - S_w / T it lost five digits: tau came out 3.87e-14
    (bound 3.73e-14; two_tile, T = 4, coordinate 0) and 1.84e-13 (bound 5.86e-14; wide, T = 8, coordinate 4) from the
    restatement.  The kernels centre through x_t - x_0 since, which is exact for close values: float64 numpy in the header's
    order gives 2e-16 on both."""
    c = contexts(name)
    res = _short_run(c)
    stop, hist, Ts, refs = tcv._replay(res, 4, 1000.0, 0.01)
    tcv._tau_close(res.tau_history, refs, Ts)


# ---- Levenberg-Marquardt -----------------------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _box(fit, lo, hi):
    """The fitter's prior box narrowed to [lo, hi] (sent to the device with the next call that needs it), and put back."""
    keep = fit._lo.copy(), fit._hi.copy()
    fit._lo[:], fit._hi[:], fit._prior_key = lo, hi, None
    try:
        yield
    finally:
        fit._lo[:], fit._hi[:] = keep
        fit._prior_key = None


@pytest.mark.parametrize("name", ["two_tile", "wide", "jax", "bad_pixels"])
def test_levenberg_marquardt_against_the_restatement(contexts, name):
    """Eight starts of `hc.fit_case` (why these: its docstring; tests/test_sampler_contexts_host.py checks what it says) against
    fit_reference.maximize_batch at the bars of test_gpu_fit.py::test_rejected_steps_follow_the_reference: the same status, as
    many iterations give or take one, logL within the stopping rule's ftol (1 + |logL|), theta within THETA_BAR in cube units.
    Then everything free for six iterations: test_gpu_fit.py's invariants hold along the flat valleys too."""
    c = contexts(name)
    fit, prob = c.fit, c.prob
    jax = c.kw.get("conv_mode") == "jax"
    centre, free, max_iter = hc.fit_case(name)
    lo, hi = fr.box(prob)
    assert np.array_equal(fit._lo, lo) and np.array_equal(fit._hi, hi)
    nlo, nhi = centre.copy(), centre.copy()
    move = free + [prob.startind]
    nlo[move], nhi[move] = lo[move], hi[move]
    P0 = tfit._starts(c.kw, centre, 8, 31)
    with np.errstate(all="ignore"):
        rP, rL, rs, rn = fr.maximize_batch(prob, P0, nlo, nhi, max_iter=max_iter, ftol=tfit.FTOL, jax=jax)
    with _box(fit, nlo, nhi):
        got = fit.maximize_batch(P0, max_iter=max_iter, ftol=tfit.FTOL)
        tfit._check_invariants(fit, prob, P0, got, jax)
    P, L, status, niter = got
    span = np.where(hi > lo, hi - lo, 1.0)
    for r in range(8):
        print(f"{name} start {r}: status {status[r]} ({rs[r]}), niter {niter[r]} ({rn[r]}), logL - restatement's {L[r] - rL[r]:.3e}, "
              f"bar {tfit.FTOL * (1 + abs(rL[r])):.3e}, cube distance {np.abs((P[r] - rP[r]) / span).max():.3e}, bar {fr.THETA_BAR:.3e}")
    assert np.array_equal(status, rs) and (status == (0 if name == "wide" else 1)).all()
    assert (np.abs(niter.astype(int) - rn) <= 1).all()
    assert (np.abs(L - rL) <= tfit.FTOL * (1.0 + np.abs(rL))).all()
    assert (np.abs((P - rP) / span).max(axis=1) <= fr.THETA_BAR).all()
    tfit._check_invariants(fit, prob, P0, fit.maximize_batch(P0, max_iter=6, ftol=tfit.FTOL), jax)
