"""GPU: nested sampling's replacement step (mcalf_slice_replace_batch[_device]) against the numpy restatement
tests/ns_reference.py with logL = als_fitter.loglike_cube_batch (the existing entry: every decision sees the same bits), its
invariance under batch, position, entry and device count, the uniformity of unconstrained chains, and the evidence of a
three-parameter problem end to end against a quadrature of the C oracle.  Every case is at most 2048 rows and 300 pixels."""
import ctypes as C

import numpy as np
import pytest
import torch

import mcalf_amd
import ns_reference as nr
from cases import oracle_synth, problem_from_kwargs, tiny_problem
from mcalf_amd import _lib, nested
from mcalf_amd.routines.hires_fitter import write_equal_weights
from test_gpu_fit import _civ

pytestmark = pytest.mark.gpu

INF = float("inf")


def _logl(fit):
    return lambda U: fit.loglike_cube_batch(U, return_theta=False)


def _device_call(fit, U0, Lmin, D, sid, nmoves, max_steps, seed=0, stream=None, theta=True):
    """mcalf_slice_replace_batch_device on torch tensors: rc and (U, theta, logL, status, nevals, moves) as numpy arrays."""
    n = U0.shape[0]
    opts = _lib.mcalf_slice_opts(nmoves, max_steps, D.shape[0], 0, seed)
    dU0, dD = torch.from_numpy(np.ascontiguousarray(U0)).cuda(), torch.from_numpy(np.ascontiguousarray(D)).cuda()
    dLmin = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(np.asarray(Lmin, dtype=float), (n,)))).cuda()
    dsid = torch.from_numpy(np.ascontiguousarray(sid, dtype=np.uint64).view(np.int64)).cuda()
    dU, dT = (torch.full(U0.shape, -7.0, dtype=torch.float64, device="cuda") for _ in range(2))
    dL = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    dS, dN, dM = (torch.full((n,), -7, dtype=torch.int32, device="cuda") for _ in range(3))
    stream = torch.cuda.current_stream() if stream is None else stream
    stream.wait_stream(torch.cuda.current_stream())
    rc = fit._lib.mcalf_slice_replace_batch_device(fit._ctx, dU0.data_ptr(), dLmin.data_ptr(), dD.data_ptr(), dsid.data_ptr(), n,
                                                   C.addressof(opts), dU.data_ptr(), dT.data_ptr() if theta else None, dL.data_ptr(),
                                                   dS.data_ptr(), dN.data_ptr(), dM.data_ptr(), C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, tuple(t.cpu().numpy() for t in (dU, dT, dL, dS, dN, dM))


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def _against_reference(fit, U0, Lmin, D, sid, nmoves, max_steps, seed):
    """The host entry against ns_reference: U by value (the sign of a zero may differ), logL by bytes, the counters equal;
    theta is the prior transform of U and logL the cube entry's value of U."""
    got = fit.slice_replace_batch(U0, Lmin, D, nmoves=nmoves, max_steps=max_steps, seed=seed, stream_ids=sid)
    U, theta, L, status, nevals, moves = got
    rU, rL, rs, rn, rm = nr.slice_replace(_logl(fit), U0, Lmin, D, sid, nmoves, max_steps, seed)
    assert np.array_equal(status, rs) and np.array_equal(nevals, rn) and np.array_equal(moves, rm)
    assert np.array_equal(U, rU, equal_nan=True)
    assert L.tobytes() == rL.tobytes()
    assert L.tobytes() == _logl(fit)(U).tobytes()
    assert np.array_equal(theta, fit.scale_cube_batch(U), equal_nan=True)
    lmin = np.broadcast_to(np.asarray(Lmin, dtype=float), L.shape)
    assert (L[status >= 0] > lmin[status >= 0]).all()
    assert (moves[status == 1] == nmoves).all() and (moves[status == 0] < max(nmoves, 1)).all() and (moves[status == -1] == 0).all()
    return got


# ---- the ndim-4 problem ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def tiny():
    """(fit, live points, their logL) of cases.tiny_problem(64): 256 uniform points of the cube, evaluated once."""
    with mcalf_amd.als_fitter(None, **tiny_problem(64)) as fit:
        live = np.random.default_rng(1).random((256, fit.ndim))
        yield fit, live, _logl(fit)(live)


def _starts(live, L, lmin, n, rng):
    ok = np.flatnonzero(L > lmin)
    return live[ok[rng.integers(0, ok.size, n)]].copy()


@pytest.mark.parametrize("batch", [1, 64, 65, 200])
@pytest.mark.parametrize("nmoves", [1, 8])
def test_trajectories_under_the_median_constraint(tiny, batch, nmoves):
    fit, live, L = tiny
    lmin = float(np.median(L))
    rng = np.random.default_rng(batch + nmoves)
    U0 = _starts(live, L, lmin, batch, rng)
    D = nested.directions(live[L > lmin])
    sid = np.arange(batch, dtype=np.uint64) + np.uint64(2 ** 32 * nmoves)
    U, theta, Lg, status, nevals, moves = _against_reference(fit, U0, lmin, D, sid, nmoves, 50 * nmoves, seed=batch)
    assert (status == 1).all() and (nevals >= nmoves).all()
    assert (np.abs(U - U0).max(axis=1) > 0.0).all()


def test_trajectories_without_a_constraint_and_with_one_per_row(tiny):
    fit, live, L = tiny
    rng = np.random.default_rng(9)
    D = nested.directions(live)
    free = _against_reference(fit, live[:65].copy(), -INF, D, np.arange(65, dtype=np.uint64), 8, 400, seed=2)
    assert (free[3] == 1).all() and (free[4] == 8).all()                 # every finite logL passes: one trial per move
    lmin = L[:200] - rng.uniform(0.1, 5.0, 200)
    lmin[::7] = L[:200:7]                                                # not above its own logL: L > Lmin is false
    lmin[3::7] = L[3:200:7] + 1.0
    got = _against_reference(fit, live[:200].copy(), lmin, D, np.arange(200, dtype=np.uint64) + np.uint64(5), 8, 400, seed=3)
    bad = np.zeros(200, dtype=bool)
    bad[::7] = bad[3::7] = True
    assert (got[3][bad] == -1).all() and (got[3][~bad] == 1).all()
    assert got[0][bad].tobytes() == live[:200][bad].tobytes() and got[2][bad].tobytes() == L[:200][bad].tobytes()
    assert not got[4][bad].any()


def test_out_of_steps_rows_keep_a_valid_point(tiny):
    fit, live, L = tiny
    lmin = float(np.median(L))
    U0 = _starts(live, L, lmin, 64, np.random.default_rng(3))
    U, theta, Lg, status, nevals, moves = _against_reference(fit, U0, lmin, nested.directions(live[L > lmin]),
                                                             np.arange(64, dtype=np.uint64), 8, 3, seed=1)
    assert (status == 0).any() and (nevals[status == 0] == 3).all()
    assert (Lg[status == 0] > lmin).all()
    zero = _against_reference(fit, U0, lmin, np.eye(fit.ndim), np.arange(64, dtype=np.uint64), 8, 0, seed=1)      # no step at all
    assert (zero[3] == 0).all() and zero[0].tobytes() == U0.tobytes() and not zero[4].any()
    none = _against_reference(fit, U0, lmin, np.eye(fit.ndim), np.arange(64, dtype=np.uint64), 0, 50, seed=1)     # nmoves 0: the checked start
    assert (none[3] == 1).all() and none[0].tobytes() == U0.tobytes() and not none[4].any()


def test_bad_starts_faces_and_direction_sets(tiny):
    fit, live, L = tiny
    nd = fit.ndim
    lmin = np.full(64, float(np.median(L)))
    U0 = _starts(live, L, lmin[0], 64, np.random.default_rng(5))
    U0[0, 1] = 1.5                                     # outside the cube
    U0[1, 2] = -1e-300
    U0[2, 3] = np.nan
    U0[3, 0] = np.nan                                  # (the ncomp slot)
    lmin[4:12] = -INF                                  # starts exactly on the faces 0 and 1
    U0[4, 1], U0[5, 1], U0[6, 2], U0[7, 3] = 0.0, 1.0, 0.0, 1.0
    U0[8, 1:] = 0.0
    U0[9, 1:] = 1.0
    U0[10] = 0.0
    U0[11] = 1.0
    sid = np.arange(64, dtype=np.uint64)
    cov = nested.directions(live[L > lmin[0]])
    sets = {"one": cov[1:2], "identity": np.eye(nd), "two_ndim": np.vstack([np.eye(nd), cov]),
            "zero_row": np.vstack([cov[:2], np.zeros((1, nd)), np.eye(nd)[2:3]])}
    for name, D in sets.items():
        U, theta, Lg, status, nevals, moves = _against_reference(fit, U0, lmin, D, sid, 2 * nd, 400, seed=11)
        assert (status[:4] == -1).all(), name
        assert np.array_equal(U[:4], U0[:4], equal_nan=True) and not nevals[:4].any()
        assert ((U[4:] >= 0.0) & (U[4:] <= 1.0)).all(), name
        assert (status[12:] == 1).all() and (status[4:12] != 0).all(), name
    lib = fit._lib
    D = np.eye(nd)
    D[1, 2] = np.nan
    with pytest.raises(RuntimeError, match="D has a non-finite entry"):
        fit.slice_replace_batch(U0, lmin, D)
    with pytest.raises(ValueError):
        fit.slice_replace_batch(U0, lmin, np.eye(nd), stream_ids=np.arange(3))
    assert lib.mcalf_slice_replace_batch(fit._ctx, None, None, None, None, 0, C.addressof(_lib.mcalf_slice_opts(1, 1, 1, 0, 0)),
                                         None, None, None, None, None, None) == 0


# ---- the ndim-15 problem -----------------------------------------------------------------------------------------------------

def test_trajectories_two_lines_floated_resolution_and_continuum():
    kw, _ = _civ(npix=300, specres=(6.0, 9.0), contval=(0.9, 1.1))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.ndim == 15
        live = np.random.default_rng(2).random((128, 15))
        L = _logl(fit)(live)
        lmin = float(np.median(L))
        U0 = _starts(live, L, lmin, 33, np.random.default_rng(4))
        D = nested.directions(live[L > lmin])
        sid = np.arange(33, dtype=np.uint64) * np.uint64(2 ** 33 + 1)
        for nmoves, steps in ((1, 50), (30, 1500)):
            got = _against_reference(fit, U0, lmin, D, sid, nmoves, steps, seed=2 ** 63 + 9)
            assert (got[3] == 1).all()
        rc, dev = _device_call(fit, U0, lmin, D, sid, 30, 1500, seed=2 ** 63 + 9)
        assert rc == 0 and _same(dev, got)


# ---- invariance --------------------------------------------------------------------------------------------------------------

def test_results_do_not_depend_on_entry_batch_position_or_device_count(tiny):
    fit, live, L = tiny
    lmin = float(np.median(L))
    U0 = _starts(live, L, lmin, 65, np.random.default_rng(6))
    U0[7, 2] = 2.0                                                          # a bad start among them
    D = nested.directions(live[L > lmin])
    sid = np.arange(65, dtype=np.uint64) + np.uint64(100)
    ref = fit.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid)
    assert set(ref[3]) == {1, -1}
    assert ref[2].tobytes() == _logl(fit)(ref[0]).tobytes()
    assert _same(ref, fit.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid))      # two calls
    # the device entry (max_steps steps unconditionally), on the current stream and on a side stream, with and without theta
    side = torch.cuda.Stream()
    for stream, theta in ((None, True), (side, True), (side, False)):
        rc, dev = _device_call(fit, U0, lmin, D, sid, 8, 400, seed=4, stream=stream, theta=theta)
        assert rc == 0 and _same([a for k, a in enumerate(dev) if theta or k != 1], [a for k, a in enumerate(ref) if theta or k != 1])
    # a row alone, and the rows in another order
    for i in (0, 7, 64):
        one = fit.slice_replace_batch(U0[i:i + 1], lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid[i:i + 1])
        assert _same([a[i:i + 1] for a in ref], one), i
    perm = np.random.default_rng(0).permutation(65)
    assert _same([a[perm] for a in ref], fit.slice_replace_batch(U0[perm], lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid[perm]))
    # out of steps the same way
    short = fit.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=3, seed=4, stream_ids=sid)
    rc, dev = _device_call(fit, U0, lmin, D, sid, 8, 3, seed=4)
    assert rc == 0 and _same(dev, short) and (short[3] == 0).any()
    # another seed or another stream id is another trajectory
    assert not _same(ref[:1], fit.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=400, seed=5, stream_ids=sid)[:1])
    with mcalf_amd.als_fitter(None, device=[0, 0, 0], **tiny_problem(64)) as multi:
        assert _same(ref, multi.slice_replace_batch(U0, lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid))
        assert _same([a[:2] for a in ref], multi.slice_replace_batch(U0[:2], lmin, D, nmoves=8, max_steps=400, seed=4, stream_ids=sid[:2]))
        rc, _ = _device_call(multi, U0, lmin, D, sid, 8, 3)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in multi._lib.mcalf_last_error(multi._ctx)


# ---- uniformity ----------------------------------------------------------------------------------------------------------------

def test_unconstrained_chains_end_uniform_in_the_cube(tiny):
    """2048 chains from the centre, identity directions, 10 ndim moves, no constraint: the share of rows in which a coordinate
    never moved is 0.75^40 ~ 1e-5, and each coordinate's Kolmogorov-Smirnov distance from U(0, 1) must stay below
    2.8 / sqrt(2048) ~ 0.062, the critical value at about 1e-6."""
    fit, _, _ = tiny
    n, nd = 2048, fit.ndim
    U, theta, L, status, nevals, moves = fit.slice_replace_batch(np.full((n, nd), 0.5), -INF, np.eye(nd), nmoves=10 * nd, seed=7)
    assert (status == 1).all() and (moves == 10 * nd).all()
    grid = np.arange(1, n + 1) / n
    for k in range(nd):
        x = np.sort(U[:, k])
        ks = max((grid - x).max(), (x - (grid - 1.0 / n)).max())
        print(f"coordinate {k}: KS distance {ks:.4f} (bar {2.8 / np.sqrt(n):.4f})")
        assert ks < 2.8 / np.sqrt(n)


# ---- evidence end to end ---------------------------------------------------------------------------------------------------------

def _evidence_problem():
    kw = tiny_problem(64, seed=3)
    wl = kw["spectrum"][0]
    z0 = wl[32] / 1548.204 - 1.0
    flux = oracle_synth(kw, np.array([1.0, 13.3, z0 + 3e-5, 15.0])) + np.random.default_rng(11).normal(0.0, 0.05, 64)
    return dict(kw, spectrum=(wl, flux, np.full(64, 0.05)))


@pytest.fixture(scope="module")
def evidence():
    """(kwargs, ln Z by the midpoint rule with 96^3 nodes over the three continuous cube coordinates, the same with 64^3),
    evaluated with the C oracle once per module."""
    from oracle.c_oracle import COracle
    from mcalf_amd import workloads
    kw = _evidence_problem()
    orc = COracle(problem_from_kwargs(kw), threads=8)
    b = workloads.bounds_of(kw)
    lo, hi = b.min(axis=1), b.max(axis=1)

    def quad(m):
        u = (np.arange(m) + 0.5) / m
        g = np.stack(np.meshgrid(u, u, u, indexing="ij"), axis=-1).reshape(-1, 3)
        P = np.empty((g.shape[0], 4))
        P[:, 0] = 1.0
        P[:, 1:] = g * (hi[1:] - lo[1:]) + lo[1:]
        ll = orc.loglike_batch(P)
        return float(np.logaddexp.reduce(ll) - 3.0 * np.log(m))
    return kw, quad(96), quad(64)


def test_the_quadrature_has_converged(evidence):
    _, fine, coarse = evidence
    print(f"ln Z: 96^3 nodes {fine:.4f}, 64^3 nodes {coarse:.4f}")
    assert abs(fine - coarse) <= 0.05


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_nested_sampling_finds_the_evidence(evidence, seed, tmp_path):
    """|ln Z - quadrature| <= 4 sqrt(H / nlive), the margin being 4 standard errors of the nested-sampling estimator; no row
    may run out of its 200 steps."""
    kw, want, _ = evidence
    with mcalf_amd.als_fitter(None, **kw) as fit:
        res = fit.nested_sample(nlive=256, batch=64, nmoves=8, seed=seed, max_steps=200)
        err = np.sqrt(res.H / 256)
        print(f"seed {seed}: ln Z {res.logZ:.4f}, quadrature {want:.4f}: {abs(res.logZ - want) / err:.2f} standard errors of {err:.4f}; "
              f"H {res.H:.3f}, {res.rounds} rounds, {res.nevals} evaluations, {res.unfinished} unfinished")
        assert abs(res.logZ - want) <= 4.0 * err
        assert res.unfinished == 0
        assert abs(np.exp(res.logw).sum() - 1.0) <= 1e-12 and (np.diff(res.logL) >= 0.0).all()
        assert np.array_equal(res.theta, fit.scale_cube_batch(res.cube))
        ll, th = res.equal_weight_samples(np.random.default_rng(seed))
        path = str(tmp_path / "run_equal_weights.txt")
        write_equal_weights(path, ll, th)
        chain = np.loadtxt(path, ndmin=2)
        assert chain.shape == (ll.size, 2 + fit.ndim) and ll.size > 20
        assert np.isin(chain[:, 1], -2.0 * res.logL).all() and (chain[:, 0] == 1.0).all()
