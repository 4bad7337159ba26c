"""CPU, no device: the numpy restatement of the batched Levenberg-Marquardt fit (tests/fit_reference.py) against
scipy.optimize.least_squares, and its invariants by hand-checkable construction.

The problem (fit_reference.convergence_kwargs / convergence_starts): 300 pixels of 6188-6212 A, CIV 1548 / 1550,
ncomp [2, 3], R = 8 fixed, sigma 0.02, the oracle's model of three components plus default_rng(1) noise, six starts at the
truth +- (0.2 dex, 1e-4, 4 km/s).  Measured here, ftol 1e-10: status 1 on all six starts after 6 outer iterations each, no
rejected step; scipy's logL (770.58717321...) exceeds the reference's by 4.3e-11 .. 4.8e-10, the bar ftol (1 + |logL|) is
7.7e-8; the largest cube-unit distance between the two optima is 8.63e-7, so the theta bar of the GPU test
(fit_reference.THETA_BAR) is 8.63e-6."""
import numpy as np
import pytest

import cases
import fit_reference as fr

FTOL = 1e-10


@pytest.fixture(scope="module")
def setup():
    prob = cases.problem_from_kwargs(fr.convergence_kwargs())
    lo, hi = fr.box(prob)
    return prob, lo, hi, fr.convergence_starts()


def test_every_start_converges_to_scipys_optimum(setup):
    prob, lo, hi, P0 = setup
    worst = 0.0
    for i, p0 in enumerate(P0):                                       # every start: none is left out
        trace = []
        p, logl, status, niter = fr.maximize_row(prob, p0, lo, hi, max_iter=50, ftol=FTOL, trace=trace)
        ps, ls = fr.scipy_optimum(prob, p0, lo, hi)
        dist = np.abs((p - ps) / (hi - lo)).max()
        print(f"start {i}: status {status}, niter {niter}, logL {logl!r}, scipy - ours {ls - logl:.3e}, bar {FTOL * (1 + abs(logl)):.3e}, "
              f"cube distance {dist:.3e}")
        assert status == 1
        assert niter <= 8 and niter == len(trace)
        assert logl >= ls - FTOL * (1.0 + abs(logl))
        assert logl == fr.point(prob, p)[0]
        worst = max(worst, dist)
    assert worst <= fr.THETA_BAR / 10 * 1.0000001, worst             # THETA_BAR is 10 x what is measured here


def test_a_pinned_coordinate_never_moves_and_logl_never_decreases(setup):
    """The data want the first component narrower than the box allows: its b ends on lo and stays pinned there; a coordinate
    with lo == hi, the ncomp slot (2.7: two active components) and the inactive third slot keep their bits."""
    prob, lo, hi, P0 = setup
    lo, hi = lo.copy(), hi.copy()
    lo[3] = 18.0                                                      # b of component 0: the data were made with 15
    lo[5] = hi[5] = 3.0012                                            # z of component 1 fixed
    p0 = P0[0].copy()
    p0[0] = 2.7
    p0[5] = 3.0012
    p0[7:10] = (13.3, 3.1, 55.0)                                      # inactive, outside the box: not clamped, not changed
    trace = []
    p, logl, status, niter = fr.maximize_row(prob, p0, lo, hi, max_iter=30, ftol=FTOL, trace=trace)
    assert status == 1 and p[3] == lo[3]
    assert p[0].tobytes() == p0[0].tobytes() and p[5] == 3.0012 and p[7:10].tobytes() == p0[7:10].tobytes()
    assert np.all(p[1:7] >= lo[1:7]) and np.all(p[1:7] <= hi[1:7])
    last = trace[0]["logL"]
    for rec in trace:
        assert rec["pin"][[0, 5, 7, 8, 9]].all()
        assert np.array_equal(rec["T"][rec["pin"]], rec["theta"][rec["pin"]])          # pinned: the trial does not move it
        assert np.array_equal(rec["x"][rec["pin"]], np.zeros(rec["pin"].sum()))
        if not rec["accepted"]:
            assert rec["after"].tobytes() == rec["theta"].tobytes()                    # rejected: theta unchanged
        assert rec["logL"] >= last
        last = rec["logL"]
    assert logl >= last
    assert any(rec["pin"][3] for rec in trace)


def test_a_rejected_step_leaves_theta_unchanged(setup):
    """lambda0 = 1e-15 from a far start: the undamped Gauss-Newton step overshoots, is rejected, and lambda grows tenfold."""
    prob, lo, hi, P0 = setup
    p0 = fr.TRUTH.copy()
    p0[1:] += np.tile([0.6, 4e-4, 12.0], 3) * np.array([1, -1, 1, -1, 1, -1, 1, 1, -1])
    trace = []
    p, logl, status, niter = fr.maximize_row(prob, p0, lo, hi, max_iter=40, lambda0=1e-15, ftol=FTOL, trace=trace)
    rejected = [rec for rec in trace if not rec["accepted"]]
    assert rejected, "the construction is meant to reject at least one step"
    lam = 1e-15
    for rec in trace:
        if rec["accepted"]:
            assert rec["logL_T"] > rec["logL"]
            lam = max(lam / 10, 1e-15)
        else:
            assert rec["after"].tobytes() == rec["theta"].tobytes()
            lam = lam * 10
        assert rec["lam"] == lam
    logs = [rec["logL"] for rec in trace] + [logl]
    assert all(b >= a for a, b in zip(logs, logs[1:]))


def test_bad_starts_and_zero_iterations(setup):
    prob, lo, hi, P0 = setup
    bad = P0[1].copy()
    bad[2] = np.nan
    p, logl, status, niter = fr.maximize_row(prob, bad, lo, hi)
    assert status == -1 and niter == 0 and p.tobytes() == bad.tobytes()
    out = P0[2].copy()
    out[1] = 99.0                                                     # clamped to hi
    p, logl, status, niter = fr.maximize_row(prob, out, lo, hi, max_iter=0)
    assert status == 0 and niter == 0 and p[1] == hi[1] and np.array_equal(p[2:], out[2:])
    assert logl == fr.point(prob, p)[0]


def test_cg_solves_the_damped_system():
    rng = np.random.default_rng(0)
    B = rng.standard_normal((12, 7))
    A = B.T @ B
    g = rng.standard_normal(7)
    x, n = fr.cg(A, g, 1e-2, 7)
    assert n <= 7 and np.abs((A + 1e-2 * np.eye(7)) @ x - g).max() <= 1e-9 * np.abs(g).max()
    x1, n1 = fr.cg(A, g, 1.0, 1)
    assert n1 == 1 and np.allclose(x1, (g @ g) / (g @ (A @ g + g)) * g, rtol=1e-15, atol=0)
