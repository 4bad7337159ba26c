"""CPU: the inputs of tests/test_gpu_sampler_contexts.py do what its tests rely on, by the numpy oracle alone -- the wide
contexts are wide, the bad pixels lie in the fit range and change logL, the veto's start ball straddles the veto's edge, every
start ball has a finite centre, the Levenberg-Marquardt cases end where the comparison's bars mean something -- so that a green
GPU test cannot be vacuous."""
import numpy as np
import pytest

import fit_reference as fr
import hard_contexts as hc
from cases import problem_from_kwargs
from test_gpu_fit import FTOL, _starts


@pytest.fixture(scope="module")
def centres():
    """name -> the centre of the GPU tests' start ball: the best of the NDRAW uniform draws, here by the oracle (the GPU module
    takes the device's logL, asserts that it is finite there and holds it to the oracle's at 1e-10), VETO_CENTRE on `veto`."""
    made = {}

    def get(name):
        if name not in made:
            kw = hc.kwargs(name)
            if name == "veto":
                made[name] = hc.VETO_CENTRE
            else:
                d = hc.draws(problem_from_kwargs(kw).ndim)
                made[name] = d[np.nanargmax(hc.oracle_cube_loglike(kw, d))]
        return made[name]
    return get


@pytest.mark.parametrize("name", ["wide", "wide_two_tile"])
def test_the_wide_contexts_are_wide(name):
    kw = hc.kwargs(name)
    n = int(np.ceil(3.0348 * (max(kw["specres"]) / 2.354820) / kw["velstep"]))
    assert n == hc.n_cap(kw) and 2 * n + 64 > 4096 and hc.is_wide(kw)
    npix = problem_from_kwargs(kw).wl.size
    assert (npix > hc.TILE) == (name == "wide_two_tile")
    # a batch of one pass at the sizes of the GPU tests, and the walkers whose half-ensemble needs a second one
    per = hc.wide_rows_per_pass(npix, n, 1 << 30)
    assert per >= 130 and (per + 1) * 8 * (2 * n + 1) > 512 << 20 >= per * 8 * (2 * n + 1)


@pytest.mark.parametrize("name", ["two_tile", "jax", "bad_pixels", "veto", "chunked", "persistent"])
def test_the_other_contexts_are_narrow(name):
    kw = hc.kwargs(name)
    prob = problem_from_kwargs(kw)
    assert not hc.is_wide(kw)
    assert 2 * int(np.ceil(3.0348 * (max(kw["specres"]) / 2.354820) / prob.velstep)) + 64 <= 4096
    assert (prob.wl.size > hc.TILE) == (name == "two_tile")


def test_the_bad_pixels_are_fitted_pixels_and_change_logl():
    kw, clean = hc.bad_pixels(), hc.bad_pixels_clean()
    prob = problem_from_kwargs(kw)
    assert prob.wl.size == 300 and hc.BAD_AT == (0, 150, prob.wl.size - 1)       # the indices are those of the fitted pixels
    lo, hi = kw["fitrange"][0]
    assert ((prob.wl[list(hc.BAD_AT)] > lo) & (prob.wl[list(hc.BAD_AT)] < hi)).all()
    pc = problem_from_kwargs(clean)
    bad = ~(np.isfinite(prob.flux) & np.isfinite(prob.err) & (prob.err > 0.0))
    assert np.flatnonzero(bad).tolist() == list(hc.BAD_AT)
    assert np.isnan(prob.flux[0]) and np.isnan(prob.err[150]) and prob.err[299] == 0.0
    keep = ~bad
    assert np.array_equal(prob.flux[keep], pc.flux[keep]) and np.array_equal(prob.err[keep], pc.err[keep])
    U = np.random.default_rng(7).random((32, prob.ndim))
    got, want = hc.oracle_cube_loglike(kw, U), hc.oracle_cube_loglike(clean, U)
    assert np.isfinite(got).all() and np.isfinite(want).all() and (got != want).all()


def test_the_veto_ball_straddles_the_vetos_edge():
    kw = hc.veto()
    L = hc.oracle_cube_loglike(kw, hc.veto_ball(512))
    assert (np.isneginf(L) | np.isfinite(L)).all()
    frac = np.isneginf(L).mean()
    print(f"vetoed: {frac:.3f} of the 512 draws of the ball")
    assert 0.1 <= frac <= 0.9
    # what the GPU tests draw from it: 64 finite starts for the ensemble, 192 for three rungs, vetoed rows for the refusals
    assert np.isfinite(L).sum() >= 64 and np.isfinite(hc.oracle_cube_loglike(kw, hc.veto_ball(1024))).sum() >= 192
    assert np.isneginf(hc.oracle_cube_loglike(kw, hc.veto_ball(64))).sum() >= 8
    live = hc.oracle_cube_loglike(kw, hc.veto_ball(128))
    # the slice moves: the constraint is the median of the live rows that are not vetoed; vetoed rows to start from
    assert np.isfinite(live).sum() >= 32 and np.isneginf(live).sum() >= 12
    # without the veto the same rows are all finite: the -inf is the veto's
    assert np.isfinite(hc.oracle_cube_loglike(hc.chunked(), hc.veto_ball(512))).all()


@pytest.mark.parametrize("name", hc.NAMES)
def test_logl_is_finite_at_the_centre_of_every_start_ball(centres, name):
    kw = hc.kwargs(name)
    centre = centres(name)
    assert ((centre >= 0.0) & (centre <= 1.0)).all()
    assert np.isfinite(hc.oracle_cube_loglike(kw, centre[None])[0])
    U0 = hc.veto_ball(64) if name == "veto" else hc.ball(centre, hc.BALL, 64)
    assert U0.shape == (64, centre.size) and ((U0 >= 0.0) & (U0 <= 1.0)).all() and np.unique(U0, axis=0).shape[0] == 64


def test_the_persistent_launch_is_the_smallest_one():
    """4 x 2 x (compute units) items in a half-ensemble: 4096 walkers on the 256 compute units of an MI355X."""
    assert hc.persistent_walkers(256) == 4096 and hc.persistent_walkers(256) // 2 == 4 * 2 * 256
    assert hc.persistent_walkers(64) // 2 <= 16 * 2 * 64                          # (within the ordered hand-out's range)


@pytest.mark.parametrize("name", ["two_tile", "wide", "jax", "bad_pixels"])
def test_the_fit_cases_end_where_the_bars_mean_something(name):
    """The restatement alone on the cases of `hc.fit_case`: every start of the two-line problems converges (status 1) without a
    rejected step; the one step on `wide` is accepted with a gain far above the stopping rule's bar (status 0)."""
    kw = hc.kwargs(name)
    prob = problem_from_kwargs(kw)
    centre, free, max_iter = hc.fit_case(name)
    lo, hi = fr.box(prob)
    assert ((centre >= lo) & (centre <= hi)).all()
    nlo, nhi = centre.copy(), centre.copy()
    move = free + [prob.startind]
    nlo[move], nhi[move] = lo[move], hi[move]
    P0 = _starts(kw, centre, 8, 31)[:3]                  # (three of the eight starts: the GPU test runs the restatement on all)
    with np.errstate(all="ignore"):
        for p0 in P0:
            trace = []
            p, logl, status, niter = fr.maximize_row(prob, p0, nlo, nhi, max_iter=max_iter, ftol=FTOL, jax=kw.get("conv_mode") == "jax", trace=trace)
            assert all(rec["accepted"] for rec in trace) and niter == len(trace)
            if name == "wide":
                assert status == 0 and niter == 1 and trace[0]["logL_T"] - trace[0]["logL"] > 1e3 * FTOL * (1.0 + abs(logl))
            else:
                assert status == 1 and 3 <= niter <= 10
            fixed = np.setdiff1d(np.flatnonzero(fr.movable(prob, p0, kw.get("conv_mode") == "jax")), move)
            assert fixed.size > 0 and np.array_equal(p[fixed], centre[fixed])          # (clamped into a box of no width)
