"""GPU: nested sampling's replacement step (mcalf_slice_replace_batch[_device]) where a lane of the row's wave owns MORE than
one coordinate: ndim 63 .. 130 on the problems of tests/many_components.py, against the numpy restatement
tests/ns_reference.py with logL = als_fitter.loglike_cube_batch, by `_against_reference` of tests/test_gpu_ns.py: U by value,
logL by bytes, the counters equal -- no tolerance.  At ndim 64 every lane owns one coordinate, at 65 lane 0 alone owns two, at
129 three: the chord's max / min, the outside-the-cube test and the any-non-zero-direction test must fold every turn.

Every "late coordinate" case either asserts that the binding or defective index is >= 64 (the chords: with
`many_components.binding`, restated on the CPU in tests/test_many_components_reference.py) or has a control row that differs
in the index alone.

Uniformity (ndim 65, 2048 chains, 650 moves along unit vectors): the share of rows in which a coordinate never moved is
(64 / 65)^650 ~ 4.2e-5; the bar on each coordinate's Kolmogorov-Smirnov distance is test_gpu_ns.py's 2.8 / sqrt(2048) ~
0.062.  Measured on an MI355X: the largest distance over the 65 coordinates 0.0363, coordinate 64's 0.0252.

With the outside-the-cube test and the chord cut to the first 64 coordinates (a library built that way, not committed) the
chords, the bad starts, the invariance, the uniformity and every trajectory at ndim >= 128 fail."""
import numpy as np
import pytest
import torch

import many_components as mc
import mcalf_amd
import ns_reference as nr
from mcalf_amd import _lib, nested
from test_gpu_ns import INF, _against_reference, _device_call, _logl, _same, _starts

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def problems():
    """ndim -> (fit, live points, their logL) of many_components.many(ndim): 4 ndim uniform points of the cube, evaluated
    once per module."""
    made = {}

    def get(ndim):
        if ndim not in made:
            fit = mcalf_amd.als_fitter(None, **mc.many(ndim)[0])
            fit.__enter__()
            assert fit.ndim == ndim
            live = np.random.default_rng(ndim).random((4 * ndim, ndim))
            made[ndim] = (fit, live, _logl(fit)(live))
        return made[ndim]
    yield get
    for fit, _, _ in made.values():
        fit.__exit__(None, None, None)


# ---- trajectories ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [63, 64, 65, 128, 129, 130])
@pytest.mark.parametrize("batch", [1, 65])
@pytest.mark.parametrize("nmoves", [1, 8])
def test_trajectories_under_the_median_constraint(problems, ndim, batch, nmoves):
    fit, live, L = problems(ndim)
    assert np.isfinite(L).all()
    lmin = float(np.median(L))
    U0 = _starts(live, L, lmin, batch, np.random.default_rng(batch + nmoves))
    D = nested.directions(live[L > lmin])                                  # 2 ndim points: dense Cholesky rows
    assert D.shape == (ndim, ndim) and np.count_nonzero(np.triu(D, 1)) == ndim * (ndim - 1) // 2
    sid = np.arange(batch, dtype=np.uint64) + np.uint64(2 ** 32 * nmoves)
    for dirs in (D, np.eye(ndim)):
        U, theta, Lg, status, nevals, moves = _against_reference(fit, U0, lmin, dirs, sid, nmoves, 50 * nmoves, seed=batch)
        moved = moves >= 1
        assert (status >= 0).all() and (status == 1).any() and (nevals >= moves).all()
        assert (np.abs(U - U0).max(axis=1)[moved] > 0.0).all()
        if dirs is D and ndim > 64 and batch > 1:
            assert (np.abs(U - U0)[:, 64:].max(axis=0) > 0.0).all()        # every late coordinate moved in some row


# ---- the chord is set by a late coordinate ---------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [65, 129, 130])
def test_the_chord_is_set_by_a_late_coordinate(problems, ndim):
    """Hand-built directions, no constraint (every finite logL passes: one trial per move).  Each case alone with its one
    direction and one move, so that the first chord is the one the case is about; then all of them together with an all-zero
    direction row among the others, eight moves."""
    fit, _, _ = problems(ndim)
    cases = mc.chord_cases(ndim)
    for i, (name, x, d, klo, khi) in enumerate(cases):
        ilo, ihi = mc.binding(x, d)
        assert ihi >= 64 and (ilo >= 64 or klo is None), name              # else the case tests nothing
        assert klo in (None, "late", ilo) and khi in ("late", ihi), name
        tl, tr = nr.chord(x[None, :], d[None, :])
        U, theta, L, status, nevals, moves = _against_reference(fit, x[None, :], -INF, d[None, :], np.array([i], dtype=np.uint64), 1, 50, seed=3)
        assert status[0] == 1 and nevals[0] == 1, name
        t = (U[0] - x)[ihi] / d[ihi]
        assert tl[0] <= t <= tr[0] and t != 0.0, (name, t)
        assert np.array_equal(U[0][d == 0.0], x[d == 0.0]) and ((U[0] >= 0.0) & (U[0] <= 1.0)).all()
    rows = np.array([c[1] for c in cases])
    dirs = np.unique(np.array([c[2] for c in cases]), axis=0)
    dirs = np.vstack([dirs[:2], np.zeros((1, ndim)), dirs[2:]])
    got = _against_reference(fit, rows, -INF, dirs, np.arange(len(cases), dtype=np.uint64) + np.uint64(7), 8, 400, seed=5)
    assert (got[3] == 1).all() and ((got[0] >= 0.0) & (got[0] <= 1.0)).all()
    only_zero = _against_reference(fit, rows, -INF, np.zeros((2, ndim)), np.arange(len(cases), dtype=np.uint64), 3, 400, seed=5)
    assert (only_zero[3] == 1).all() and only_zero[0].tobytes() == rows.tobytes()      # nowhere to go: the moves are made in place


# ---- bad starts decided by a late coordinate -------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [65, 129])
def test_bad_starts_decided_by_a_late_coordinate(problems, ndim):
    """1.5, -1e-300 and NaN, each at index 64 (and 128) in a row of its own and at the control index 7 (and 40) in another:
    status -1, the row as given, no evaluation.  Without a constraint and with a finite logL of the start, the entry itself
    is all that makes the rows of 1.5 and -1e-300 bad.  The good rows have the bits they have without the bad ones."""
    fit, live, L = problems(ndim)
    where = ([64, 128] if ndim >= 129 else [64]) + ([7, 40] if ndim >= 129 else [7])
    defects = [(v, k) for k in where for v in (1.5, -1e-300, np.nan)]
    n = 2 * len(defects) + 1
    U0 = live[:n].copy()
    bad = np.arange(len(defects)) * 2 + 1
    for r, (v, k) in zip(bad, defects):
        U0[r, k] = v
    good = np.setdiff1d(np.arange(n), bad)
    start_logl = _logl(fit)(U0)
    assert all(np.isfinite(start_logl[r]) for r, (v, k) in zip(bad, defects) if not np.isnan(v))
    sid = np.arange(n, dtype=np.uint64) + np.uint64(11)
    for dirs in (np.eye(ndim), nested.directions(live)):
        U, theta, Lg, status, nevals, moves = _against_reference(fit, U0, -INF, dirs, sid, 8, 400, seed=13)
        assert (status[bad] == -1).all() and (status[good] == 1).all()
        assert np.array_equal(U[bad], U0[bad], equal_nan=True) and not nevals[bad].any() and not moves[bad].any()
        assert Lg[bad].tobytes() == start_logl[bad].tobytes()
        alone = fit.slice_replace_batch(U0[good], -INF, dirs, nmoves=8, max_steps=400, seed=13, stream_ids=sid[good])
        assert _same([a[good] for a in (U, theta, Lg, status, nevals, moves)], alone)


# ---- invariance ------------------------------------------------------------------------------------------------------------

def test_results_do_not_depend_on_entry_batch_position_or_device_count(problems):
    fit, live, L = problems(129)
    lmin = float(np.median(L))
    U0 = _starts(live, L, lmin, 65, np.random.default_rng(6))
    U0[7, 128] = 2.0                                                        # a bad start among them, by the last coordinate
    D = nested.directions(live[L > lmin])
    sid = np.arange(65, dtype=np.uint64) + np.uint64(100)
    ref = fit.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid)
    assert set(ref[3]) <= {1, 0, -1} and ref[3][7] == -1 and (np.delete(ref[3], 7) >= 0).all() and (ref[3] == 1).any()
    assert ref[2].tobytes() == _logl(fit)(ref[0]).tobytes()
    assert _same(ref, fit.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid))      # two calls
    side = torch.cuda.Stream()
    assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
    for stream, theta in ((None, True), (side, True), (side, False)):
        rc, dev = _device_call(fit, U0, lmin, D, sid, 8, 400, seed=4, stream=stream, theta=theta)
        assert rc == 0 and _same([a for k, a in enumerate(dev) if theta or k != 1], [a for k, a in enumerate(ref) if theta or k != 1])
    for i in (0, 7, 64):                                                    # a row alone
        one = fit.slice_replace_batch(U0[i:i + 1], lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid[i:i + 1])
        assert _same([a[i:i + 1] for a in ref], one), i
    perm = np.random.default_rng(0).permutation(65)                         # the rows in another order
    assert _same([a[perm] for a in ref], fit.slice_replace_batch(U0[perm], lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid[perm]))
    short = fit.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=3, seed=4, stream_ids=sid)                   # out of steps
    rc, dev = _device_call(fit, U0, lmin, D, sid, 8, 3, seed=4)
    assert rc == 0 and _same(dev, short) and (short[3] == 0).any() and (short[4][short[3] == 0] == 3).all()
    with mcalf_amd.als_fitter(None, device=[0, 0, 0], **mc.many(129)[0]) as multi:
        assert _same(ref, multi.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid))
        rc, _ = _device_call(multi, U0, lmin, D, sid, 8, 3)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in multi._lib.mcalf_last_error(multi._ctx)


# ---- uniformity ------------------------------------------------------------------------------------------------------------

def test_unconstrained_chains_end_uniform_in_every_coordinate():
    """2048 chains from the centre, identity directions, 10 ndim = 650 moves, no constraint, on a 64-pixel spectrum: each of the
    65 coordinates, index 64 among them, must end within 2.8 / sqrt(2048) of U(0, 1) in Kolmogorov-Smirnov distance."""
    n, nd = 2048, 65
    with mcalf_amd.als_fitter(None, **mc.few_pixels(nd)) as fit:
        assert fit.ndim == nd
        U, theta, L, status, nevals, moves = fit.slice_replace_batch(np.full((n, nd), 0.5), -INF, np.eye(nd), nmoves=10 * nd, seed=7)
    assert (status == 1).all() and (moves == 10 * nd).all()
    grid = np.arange(1, n + 1) / n
    worst = 0.0
    for k in range(nd):
        x = np.sort(U[:, k])
        ks = max((grid - x).max(), (x - (grid - 1.0 / n)).max())
        worst = max(worst, ks)
        if k in (0, 1, 63, 64) or ks > 0.05:
            print(f"coordinate {k}: KS distance {ks:.4f} (bar {2.8 / np.sqrt(n):.4f})")
        assert ks < 2.8 / np.sqrt(n), k
    print(f"largest KS distance over the {nd} coordinates {worst:.4f} (bar {2.8 / np.sqrt(n):.4f})")
