"""GPU: every kernel family reads a parameter row by the rules of mc-alf_amd/csrc/theta_row.h (tests/test_theta_row_host.py
checks the header itself on the CPU).  The fused likelihood kernel keeps its own text of the rules (sample_setup.h); this test
is what ties that copy to the header: the count, the columns and the slots that are never read must be the header's.

One small problem -- 96 pixels, two lines, ncompmax 3, one filler, free R and continuum -- under both convolution modes,
and 16 rows whose count slot runs over the values at which the rule has an edge, NaN and +inf included.  Every comparison is
exact: bits against bits, or exactly 0."""
import math

import numpy as np
import pytest

import mcalf_amd
from mcalf_amd import workloads

pytestmark = pytest.mark.gpu

NCOMPMAX, NPIX = 3, 96
COUNT_SLOTS = [-1.5, -0.5, -0.0, 0.0, 0.5, math.nextafter(1.0, 0.0), 1.0, 1.5, 2.0, NCOMPMAX - 0.5, math.nextafter(3.0, 0.0), float(NCOMPMAX),
               NCOMPMAX + 0.5, 1e300, math.nan, math.inf]


def expected_count(v, jax):
    """theta_row.h: active_components."""
    if math.isnan(v):
        return 0
    if math.isinf(v):
        return NCOMPMAX if v > 0 else 0
    return min(max(math.floor(v) if jax else int(v), 0), NCOMPMAX)


def problem():
    rng = np.random.default_rng(96)
    wl = np.linspace(6190.0, 6206.0, NPIX + 2)[1:-1]                  # 8 km/s pixels: R in [20, 30] km/s convolves on both paths
    kw = dict(fitrange=[[6190.0, 6206.0]], fitlines=["CIV 1548", "CIV 1550"], linepars=[(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8)],
              ncomp=[0, NCOMPMAX], nfill=1, specres=[20.0, 30.0], contval=[0.9, 1.1], Nrange=[13.0, 14.5], brange=[8.0, 40.0],
              zrange=[2.9995, 3.0015], spectrum=(wl, 1.0 + rng.normal(0.0, 0.03, NPIX), np.full(NPIX, 0.03)))
    P = workloads.draw_P(kw, len(COUNT_SLOTS), rng)
    return kw, P


@pytest.fixture(scope="module", params=["numpy", "jax"])
def case(request):
    kw, P = problem()
    jax = request.param == "jax"
    with mcalf_amd.als_fitter(None, conv_mode=request.param, **kw) as fit:
        s = fit.startind
        assert (s, fit.ndim, int(fit.ncompmax)) == (2, 2 + 1 + 3 * NCOMPMAX + 3, NCOMPMAX)
        P[:, s] = COUNT_SLOTS
        counts = [expected_count(v, jax) for v in COUNT_SLOTS]
        assert set(counts) == set(range(NCOMPMAX + 1))
        # per row: the columns of the slots at or beyond the count
        dead = [np.arange(s + 1 + 3 * nc, s + 1 + 3 * NCOMPMAX) for nc in counts]
        yield fit, P, counts, dead


def test_fused_kernel_reads_the_count_and_nothing_beyond_it(case):
    fit, P, counts, dead = case
    Q = P.copy()
    for r, nc in enumerate(counts):
        Q[r, fit.startind] = float(nc)
        Q[r, dead[r]] = np.nan
    got, want = fit.model_batch(P), fit.model_batch(Q)
    assert np.isfinite(want).all()
    assert got.tobytes() == want.tobytes()
    assert fit.loglike_batch(P).tobytes() == fit.loglike_batch(Q).tobytes()


def test_gradient_is_zero_exactly_on_the_unread_columns(case):
    fit, P, counts, dead = case
    logL, G = fit.loglike_grad_batch(P)
    assert np.isfinite(logL).all()
    for r in range(P.shape[0]):
        zero = np.zeros(fit.ndim, dtype=bool)
        zero[dead[r]] = True
        zero[fit.startind] = True
        assert np.all(G[r, zero] == 0.0), (r, COUNT_SLOTS[r])
        assert np.all(np.isfinite(G[r, ~zero]) & (G[r, ~zero] != 0.0)), (r, COUNT_SLOTS[r])


def test_equivalent_widths_are_zero_exactly_beyond_the_count(case):
    fit, P, counts, dead = case
    wcomp, _ = fit.eqw_batch(P)
    for r, nc in enumerate(counts):
        assert np.all(wcomp[r, nc:] == 0.0), (r, COUNT_SLOTS[r])
        assert np.all(wcomp[r, :nc] > 0.0), (r, COUNT_SLOTS[r])


def test_the_fit_returns_the_unread_coordinates_bit_for_bit(case):
    fit, P, counts, dead = case
    out, logL, status, niter = fit.maximize_batch(P, max_iter=2, cg_iters=3)
    assert np.all(status >= 0) and np.all(niter >= 1)                  # every row started and moved
    for r in range(P.shape[0]):
        keep = np.append(dead[r], fit.startind)
        assert out[r, keep].tobytes() == P[r, keep].tobytes(), (r, COUNT_SLOTS[r])
