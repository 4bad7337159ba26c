"""GPU: mcalf_ensemble_converge through convergence.ensemble_sample_until on the one-line problem of cases.tiny_problem, 64 walkers,
the stretch move: the run is the plain sampler's by bytes, and it stops where the rule, replayed on the host chain with
chain_reference.py, says it stops."""
import numpy as np
import pytest

import chain_reference as cr
import mcalf_amd
from cases import tiny_problem
from mcalf_amd import convergence, ensemble

pytestmark = pytest.mark.gpu

N = 64
U = 2.0 ** -53
SEED = 3            # (the seed of the runs below; the replay asserts that no decision of theirs stands within 1e-6 of its threshold)


@pytest.fixture(scope="module")
def tiny():
    """(fit, the best of 256 uniform points of the cube) of cases.tiny_problem(64)."""
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        draws = np.random.default_rng(1).random((256, fit.ndim))
        yield fit, draws[np.nanargmax(fit.loglike_cube_batch(draws, return_theta=False))]


def _same_as_the_plain_sampler(fit, res, U0):
    U, theta, logL, status, naccept, CU, CL = fit.ensemble_batch(U0, res.nsteps, thin=res.thin, seed=res.seed, first_iter=res.burn)
    assert res.cube.shape == CU.shape and res.cube.tobytes() == CU.tobytes() and res.logL.tobytes() == CL.tobytes()
    assert res.last.tobytes() == U.tobytes() and np.array_equal(res.status, status)
    assert np.array_equal(np.rint(res.accept_frac * max(res.nsteps, 1)).astype(np.int64), naccept)
    return logL


def _replay(res, check_every, factor, rtol, c=5.0):
    """Every check of the run on the host chain: (index of the stopping check or None, the reference's tau history)."""
    nkeep = res.cube.shape[0]
    Ts = list(range(check_every, nkeep + 1, check_every)) + ([nkeep] if nkeep % check_every else [])
    Ts = [T for T in Ts if T >= 4]
    refs = [cr.chain_stats(res.cube[:T], status=res.status, c=c, max_lag=cr.check_lag(T, c, factor), full_acf=False) for T in Ts]
    for T, r in zip(Ts, refs):
        assert (r["margin"][r["nused"] > 0] > 1e-6).all(), (T, r["margin"])
    hist = np.array([r["tau"] for r in refs])
    stop, margin = cr.converge_rule(Ts, hist, [r["flags"] & 1 for r in refs], [r["nused"] for r in refs], factor, rtol)
    print("replay: stop", stop, "of", len(Ts), "margin", margin)
    assert margin > 1e-6
    return stop, hist, Ts, refs


def _tau_close(got, refs, Ts):
    for j, (T, r) in enumerate(zip(Ts, refs)):
        tol = 16.0 * (r["M"] + 1.0) * (T + 3.0) * U
        live = r["nused"] > 0
        print("check", j, "T", T, "tau", got[j], "err/tol", np.abs(got[j] - r["tau"])[live] / tol[live])
        assert (np.abs(got[j] - r["tau"])[live] <= tol[live]).all()
        assert np.isnan(got[j][~live]).all()


def test_a_run_that_converges_is_the_plain_sampler_and_stops_where_the_rule_says(tiny):
    """tau of this problem under the stretch move is 60 to 110 iterations, so the chain is thinned by 5: the statistics see a
    tau of 12 to 22 kept steps, the run stops after a few hundred of them, and the replay of every check in np.longdouble
    stays quick."""
    fit, best = tiny
    res = convergence.ensemble_sample_until(fit, N, 6000, thin=5, check_every=50, factor=10.0, start=best, ball=0.05, seed=SEED)
    print("nsteps", res.nsteps, "nchecks", res.nchecks, "tau", res.tau, "rhat", res.rhat, "ess", res.ess)
    assert res.converged and 500 <= res.nsteps < 6000 and res.nsteps % 250 == 0 and res.nchecks == res.nsteps // 250
    assert res.tau_history.shape == (res.nchecks, fit.ndim) and np.array_equal(res.tau_history[-1], res.tau, equal_nan=True)
    U0 = ensemble._draw_starts(SEED, (N, fit.ndim), best, 0.05)
    logL = _same_as_the_plain_sampler(fit, res, U0)
    assert res.theta.shape == res.cube.shape and logL.tobytes() == fit.loglike_cube_batch(res.last, return_theta=False).tobytes()
    # the same run left to go on: its checks up to the stop are this run's, and none before the last one stops it
    longer = fit.ensemble_batch(U0, res.nsteps + 500, thin=5, seed=SEED)
    full = ensemble.EnsembleResult(cube=longer[5], status=longer[3])
    stop, hist, Ts, refs = _replay(full, 50, 10.0, 0.01)
    assert stop == res.nchecks - 1
    _tau_close(res.tau_history / 5, refs[:res.nchecks], Ts[:res.nchecks])           # (the result's tau is in iterations)
    live = refs[stop]["nused"] > 0
    assert (res.rhat[live] < 1.2).all() and (res.ess[live] > N).all()


def test_a_run_that_cannot_converge_uses_all_its_steps(tiny):
    fit, best = tiny
    res = convergence.ensemble_sample_until(fit, N, 150, check_every=50, factor=1000.0, start=best, ball=0.05, seed=SEED)
    assert not res.converged and res.nsteps == 150 and res.cube.shape[0] == 150 and res.nchecks == 3
    assert res.tau_history.shape == (3, fit.ndim)
    _same_as_the_plain_sampler(fit, res, ensemble._draw_starts(SEED, (N, fit.ndim), best, 0.05))
    stop, hist, Ts, refs = _replay(res, 50, 1000.0, 0.01)
    assert stop is None and Ts == [50, 100, 150]
    _tau_close(res.tau_history, refs, Ts)


def test_thinning_burn_in_and_a_last_short_block(tiny):
    fit, best = tiny
    # 3 x 20 = 60 iterations per block: 200 = 3 blocks and one of 20 iterations (6 kept steps), 2 iterations left unmade
    res = convergence.ensemble_sample_until(fit, N, 200, burn=30, thin=3, check_every=20, factor=1000.0, start=best, ball=0.05, seed=SEED)
    assert not res.converged and res.cube.shape[0] == 66 and res.nsteps == 198 and res.nchecks == 4 and res.thin == 3
    U0 = fit.ensemble_batch(ensemble._draw_starts(SEED, (N, fit.ndim), best, 0.05), 30, seed=SEED, chain=False)[0]
    _same_as_the_plain_sampler(fit, res, U0)
    stop, hist, Ts, refs = _replay(res, 20, 1000.0, 0.01)
    assert stop is None and Ts == [20, 40, 60, 66]
    _tau_close(res.tau_history / 3, refs, Ts)               # (the result's tau is in iterations)
    assert np.array_equal(res.tau, res.stats.tau * 3, equal_nan=True)


def test_a_bad_start_is_reported_and_left_out_of_the_statistics(tiny):
    fit, best = tiny
    U0 = ensemble._draw_starts(SEED, (N, fit.ndim), best, 0.05)
    U0[5, 1] = 1.5                                          # outside the cube: status -1, it never moves
    out = convergence._ensemble_converge(fit, U0, 150, check_every=50, factor=1000.0, seed=SEED)
    last, theta, logL, status, naccept, CU, CL, nkept, converged, hist, st = out
    assert status[5] == -1 and (np.delete(status, 5) == 0).all() and naccept[5] == 0 and nkept == 150 and not converged
    assert (CU[:, 5, :] == U0[5]).all()                     # a constant walker at a point that would wreck the means
    plain = fit.ensemble_batch(U0, 150, seed=SEED)
    assert CU.tobytes() == plain[5].tobytes() and CL.tobytes() == plain[6].tobytes() and last.tobytes() == plain[0].tobytes()
    assert theta.tobytes() == plain[1].tobytes() and logL.tobytes() == plain[2].tobytes()
    assert np.array_equal(status, plain[3]) and np.array_equal(naccept, plain[4])
    ref = cr.chain_stats(CU, status=status, max_lag=cr.check_lag(150, 5.0, 1000.0))
    assert (ref["margin"][ref["nused"] > 0] > 1e-6).all()
    live = ref["nused"] > 0
    assert np.array_equal(st.nused, ref["nused"]) and (st.nused[live] == N - 1).all()
    assert (np.abs(st.mean - ref["mean"]) <= 4.0 * 150 * (N - 1) * U * np.abs(ref["mean"])).all() and (st.mean <= 1.0).all()
    assert (np.abs(hist[-1] - ref["tau"])[live] <= (16.0 * (ref["M"] + 1.0) * 153.0 * U)[live]).all()


def test_a_coordinate_frozen_at_a_value_that_is_no_dyadic_fraction_does_not_keep_the_run_from_stopping(tiny):
    """Every start shares coordinate 0 = 0.3, and the stretch move keeps it there (x_j + z (x_k - x_j) with x_k == x_j).  A sum of
    T copies of 0.3 over T is not 0.3, so constancy has to be decided exactly for this coordinate to count as frozen."""
    fit, best = tiny
    U0 = ensemble._draw_starts(SEED, (N, fit.ndim), best, 0.05)
    U0[:, 0] = 0.3
    out = convergence._ensemble_converge(fit, U0, 8000, thin=5, check_every=50, factor=10.0, seed=SEED)
    last, theta, logL, status, naccept, CU, CL, nkept, converged, hist, st = out
    print("nkept", nkept, "tau", st.tau, "nused", st.nused)
    assert (CU[:, :, 0] == 0.3).all() and (status == 0).all()
    assert st.nused[0] == 0 and (st.nused[1:] == N).all() and np.isnan(st.tau[0]) and np.isnan(st.tau_mean[0]) and np.isnan(st.rhat[0])
    assert st.mean[0] == 0.3 and st.var[0] == 0.0 and np.isnan(hist[:, 0]).all() and np.isfinite(hist[:, 1:]).all()
    assert converged and nkept < 1600
    plain = fit.ensemble_batch(U0, nkept * 5, thin=5, seed=SEED)
    assert CU.tobytes() == plain[5].tobytes() and logL.tobytes() == plain[2].tobytes() and np.array_equal(naccept, plain[4])
