"""GPU: the batched Levenberg-Marquardt fit (mcalf_maximize_batch[_device]) and the derivative kernels under it where a lane
of the row's wave owns MORE than one parameter: ndim 63 .. 130 on the problems of tests/many_components.py (one line, 20 .. 43
components 97 km/s apart, 513 .. 1068 pixels of 4 km/s), against tests/fit_reference.py, the float64 reference Jacobian, the
gradient reference and scipy.  At ndim 64 every lane owns one parameter, at 65 lane 0 alone owns two, at 129 three.  Helpers
and bars are those of tests/test_gpu_fit.py; every case is at most 16 rows, 1068 pixels and 15 outer iterations.

Every "late coordinate" case either sits beside a control row (or control coordinate) with the same defect at an index < 64,
or asserts that the index it is about is >= 64.

Bars.  One CG step and full CG: test_gpu_fit.py's.  Convergence: status 1 on every row, logL at least scipy's minus
ftol (1 + |logL|), the cube distance to scipy's optimum within 10 x the distance the numpy restatement itself has on the same
problem (tests/test_many_components_reference.py: `theta_bar`; 6.7e-7 .. 2.7e-5 measured there), as many outer iterations as
the restatement +- 1.  Gradient: 1e-7 S_k + 1e-9 (test_gpu_grad.py).  Fisher product: the bar of
test_gpu_model_deriv.py::test_fisher_matvec_with_bad_pixels.

Measured on an MI355X (every test prints its figures, pytest -s):
  one CG step      error at most 2.8e-14 against bars of 9.0e-10 .. 2.1e-9 (ndim 65 and 129, four rows each)
  full CG, 129     relative residual, device 1.0e-4 .. 3.9e-3, the restatement on the CPU 5.7e-4 .. 7.4e-3 (bars 5.7e-2 .. 7.4e-1)
  convergence      status 1 on every start, the restatement's iteration count (6 or 7) on every start; scipy's logL above the
                   device's by 1.8e-10 .. 3.6e-9 against bars of 1.3e-7 .. 2.7e-7; largest cube distance to scipy's optimum
                   1.49e-6 (ndim 63, bar 1.49e-5), 6.7e-7 (64, bar 6.7e-6), 1.36e-6 (65, bar 1.37e-5), 2.73e-5 (129, on R, bar
                   2.73e-4), 8.1e-7 (67 with a filler, bar 7.8e-6)
  zero gradient    status and iteration count of the restatement on every row, logL within 4.1e-9 of its (bars 6.6e-8 ..
                   2.0e-7), the free coordinates within 5.2e-13 cube units of its
  gradient         worst error / bar 2.4e-4 (ndim 65), 3.6e-4 (ndim 129, in a column >= 64)
  Fisher product   worst error / bar 6.5e-6 (ndim 65), 6.9e-6 (ndim 129)
With the fit's g_u.g_u and its NaN test cut to the first 64 coordinates (a library built that way, not committed), the
closed-form step at 129, the convergence at 129 and 67, the bad starts, three of the zero-gradient cases and both bit-invariance
cases fail."""
import numpy as np
import pytest
import torch

import fit_reference as fr
import grad_reference as gr
import many_components as mc
import mcalf_amd
import model_deriv_reference as mdr
from cases import problem_from_kwargs
from test_gpu_fit import FTOL, _box, _check_invariants, _clamped, _device_fit, _reference_system, _same
from test_gpu_model_deriv import FLOOR_REL
from test_many_components_reference import theta_bar

pytestmark = pytest.mark.gpu


def _coord(prob, comp, j):
    """Index of (N, z, b)[j] of component `comp`."""
    return prob.startind + 1 + 3 * comp + j


def _late(ndim):
    """The late indices a case is placed at: 64, and 128 where there is one."""
    return [64, 128] if ndim >= 129 else [64]


def _control(prob, k):
    """The coordinate of the same kind (N, z or b) as `k`, of component 3: an index < 64."""
    c = _coord(prob, 3, (k - prob.startind - 1) % 3)
    assert c < 64 <= k and prob.startind < k < prob.endind
    return c


# ---- one CG step in closed form; full CG -----------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [64, 65, 129])
def test_one_cg_step_in_closed_form(ndim):
    kw, truth = mc.many(ndim)
    prob = problem_from_kwargs(kw)
    P0 = mc.starts(kw, truth, 4, 11)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        lo, hi = _box(fit)
        L0 = fit.loglike_batch(P0)
        P, L, status, niter = fit.maximize_batch(P0, max_iter=1, cg_iters=1, lambda0=1.0, ftol=FTOL)
    s = hi - lo
    accepted = np.flatnonzero(L > L0)
    assert accepted.size >= 1 and np.all(niter == 1)
    for r in range(P0.shape[0]):
        if r not in accepted:
            assert P[r].tobytes() == P0[r].tobytes() and L[r] == L0[r]
            continue
        A, g, pin = _reference_system(prob, P0[r], lo, hi)
        x = (g @ g) / (g @ (A @ g + g)) * g
        inside = (P[r] > lo) & (P[r] < hi) & ~pin
        assert ndim == 64 or (inside[64:].any() and np.abs(x[64:]).max() > 0.0)      # the step has late coordinates to be wrong in
        got = (P[r] - P0[r]) / np.where(s > 0, s, 1.0)
        err = np.abs(got - x)[inside].max()
        print(f"ndim {ndim} row {r}: max|x| {np.abs(x).max():.3e}, error {err:.3e}, bar {1e-6 * np.abs(x).max():.3e}")
        assert err <= 1e-6 * np.abs(x).max()
        assert np.array_equal(P[r][pin], P0[r][pin])


def test_full_cg_solves_the_damped_system_at_ndim_129():
    kw, truth = mc.many(129)
    prob = problem_from_kwargs(kw)
    P0 = mc.starts(kw, truth, 4, 7)
    lam = 1e-2
    with mcalf_amd.als_fitter(None, **kw) as fit:
        lo, hi = _box(fit)
        L0 = fit.loglike_batch(P0)
        P, L, status, niter = fit.maximize_batch(P0, max_iter=1, cg_iters=None, lambda0=lam, ftol=FTOL)
    s = hi - lo
    accepted = np.flatnonzero(L > L0)
    assert accepted.size >= 1
    for r in accepted:
        A, g, pin = _reference_system(prob, P0[r], lo, hi)
        M = A + lam * np.eye(prob.ndim)
        x_cpu, _ = fr.cg(A, g, lam, prob.ndim)
        res_cpu = np.abs(M @ x_cpu - g).max() / np.abs(g).max()
        x = np.where(pin, 0.0, (P[r] - P0[r]) / np.where(s > 0, s, 1.0))
        assert np.all((P[r] > lo)[~pin] & (P[r] < hi)[~pin])              # no clamping: theta_1 - theta_0 is s x
        res = np.abs(M @ x - g).max() / np.abs(g).max()
        print(f"row {r}: CG relative residual, device {res:.3e}, fit_reference on the CPU {res_cpu:.3e}, bar {100 * res_cpu + 1e-6:.3e}")
        assert res <= 100 * res_cpu + 1e-6


# ---- convergence -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim,nfill", [(63, 0), (64, 0), (65, 0), (129, 0), (67, 1)])
def test_every_start_converges_to_scipys_optimum(ndim, nfill):
    kw, truth = mc.many(ndim, nfill)
    prob = problem_from_kwargs(kw)
    lo, hi = fr.box(prob)
    P0 = mc.starts(kw, truth, 4, 7)
    opt = dict(max_iter=15, cg_iters=mc.cg_iters(ndim), ftol=FTOL)
    ref = [fr.maximize_row(prob, p0, lo, hi, **opt) for p0 in P0]
    assert all(st == 1 for _, _, st, _ in ref)
    want = [fr.scipy_optimum(prob, p0, lo, hi) for p0 in P0]
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert np.array_equal(fit._lo, lo) and np.array_equal(fit._hi, hi)
        P, L, status, niter = fit.maximize_batch(P0, **opt)
        assert L.tobytes() == fit.loglike_batch(P).tobytes()
        if prob.startind >= 1:
            assert np.all(fit.loglike_grad_batch(P0)[1][:, 0] != 0.0)      # the resolution's column is live
    bar = theta_bar(ndim, nfill)
    for r, (ps, ls) in enumerate(want):
        dist = np.abs((P[r] - ps) / (hi - lo))
        print(f"ndim {ndim} nfill {nfill} start {r}: status {status[r]}, niter {niter[r]} (reference {ref[r][3]}), scipy - ours {ls - L[r]:.3e}, "
              f"bar {FTOL * (1 + abs(L[r])):.3e}, cube distance {dist.max():.3e} at {dist.argmax()}, bar {bar:.3e}")
    assert np.all(status == 1), status
    for r, (ps, ls) in enumerate(want):
        assert L[r] >= ls - FTOL * (1.0 + abs(L[r]))
        assert np.abs((P[r] - ps) / (hi - lo)).max() <= bar
        assert abs(int(niter[r]) - ref[r][3]) <= 1


# ---- decisive coordinates in the second and third turn ---------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [65, 129])
def test_bad_starts_clamping_and_inactive_slots_at_late_coordinates(ndim):
    """Rows 1 .. : a NaN at each late index and at its control index (status -1, returned as given, the neighbours' bits as
    without them); an entry beyond hi and one below lo at a late index and at the control (clamped); an active count that
    leaves the slots holding every late index inactive, their entries outside the box (kept bit for bit), and the same with
    the inactive slots starting below index 64."""
    kw, truth = mc.many(ndim)
    prob = problem_from_kwargs(kw)
    s0 = prob.startind
    late = _late(ndim)
    ctl = [_control(prob, k) for k in late]
    P0 = mc.starts(kw, truth, 16, 21)
    nan_rows = {1 + i: k for i, k in enumerate(late + ctl)}                # rows 1 .. 4 (ndim 129) or 1 .. 2
    for r, k in nan_rows.items():
        P0[r, k] = np.nan
    out_rows = {6 + i: k for i, k in enumerate(late + ctl)}                # rows 6 .. 9: beyond hi; 10 .. 13 hold them below lo
    for r, k in out_rows.items():
        P0[r, k] = 99.0
        P0[r + 4, k] = -99.0
    first_late = (64 - s0 - 1) // 3                                        # the component that holds index 64
    assert _coord(prob, first_late, 0) <= 64 <= _coord(prob, first_late, 2)
    P0[14, s0] = float(first_late)                                         # the slots from there on are inactive
    P0[14, _coord(prob, first_late, 0):prob.endind] = np.tile((15.5, 3.2, 77.0), prob.ncompmax - first_late)
    P0[15, s0] = 3.0                                                       # control: inactive from component 3 on
    P0[15, _coord(prob, 3, 0):prob.endind] = np.tile((15.5, 3.2, 77.0), prob.ncompmax - 3)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        lo, hi = _box(fit)
        out = fit.maximize_batch(P0, max_iter=6, ftol=FTOL)
        _check_invariants(fit, prob, P0, out)
        P, L, status, niter = out
        bad = sorted(nan_rows)
        good = [r for r in range(16) if r not in nan_rows]
        assert np.all(status[bad] == -1) and np.all(status[good] >= 0) and np.all(niter[good] >= 1)
        assert P[bad].tobytes() == P0[bad].tobytes()
        clean = P0.copy()
        clean[bad] = P0[0]
        other = fit.maximize_batch(clean, max_iter=6, ftol=FTOL)
        assert _same([a[good] for a in out], [a[good] for a in other])
        assert np.all(other[2][bad] == status[0]) and all(other[0][r].tobytes() == P[0].tobytes() for r in bad)
        # clamping, seen without an iteration on top: the clamped start itself
        P_, L_, s_, n_ = fit.maximize_batch(P0, max_iter=0)
        assert np.all(n_ == 0) and np.all(s_[bad] == -1) and np.all(s_[good] == 0)
        assert P_[good].tobytes() == _clamped(fit, prob, P0)[good].tobytes() and P_[bad].tobytes() == P0[bad].tobytes()
        assert L_[good].tobytes() == fit.loglike_batch(P_[good]).tobytes()
        for r, k in out_rows.items():
            assert P_[r, k] == hi[k] and P_[r + 4, k] == lo[k], (r, k)
            assert lo[k] <= P[r, k] <= hi[k] and lo[k] <= P[r + 4, k] <= hi[k]
        for r, c in ((14, first_late), (15, 3)):
            k0 = _coord(prob, c, 0)
            assert P[r, k0:prob.endind].tobytes() == P0[r, k0:prob.endind].tobytes() and P[r, s0] == P0[r, s0]
            assert np.all(P[r, k0:prob.endind:3] == 15.5)
            assert np.any(P[r, s0 + 1:k0] != P0[r, s0 + 1:k0])


@pytest.mark.parametrize("ndim", [65, 129])
def test_a_fixed_late_coordinate_keeps_its_bits(ndim):
    """lo == hi on every late index and on its control: bits kept on every row, the rest fits as usual."""
    kw, truth = mc.many(ndim)
    prob = problem_from_kwargs(kw)
    late = _late(ndim)
    fixed = late + [_control(prob, k) for k in late]
    P0 = mc.starts(kw, truth, 4, 22)
    P0[:, fixed] = truth[fixed]
    with mcalf_amd.als_fitter(None, **kw) as fit:
        fit._lo[fixed] = fit._hi[fixed] = truth[fixed]                    # before the box first goes to the device
        out = fit.maximize_batch(P0, max_iter=6, ftol=FTOL)
        _check_invariants(fit, prob, P0, out)
        P, L, status, niter = out
        assert P[:, fixed].tobytes() == P0[:, fixed].tobytes()
        free = np.setdiff1d(np.flatnonzero(fr.movable(prob, truth)), fixed)
        assert np.all(P[:, free] != P0[:, free]) and np.all(status >= 0) and np.all(niter >= 2)
        assert np.all(L > fit.loglike_batch(P0))


@pytest.mark.parametrize("ndim", [65, 129])
def test_a_bound_the_data_push_against_at_a_late_coordinate(ndim):
    """Data made with b = 10 under brange [18, 40] for the component whose b is a late coordinate (index 64 at ndim 65, 65 and
    128 at ndim 129) and for component 3 (the control): each ends with b exactly at lo.  (The numpy restatement does too,
    slowly: 13 .. 15 outer iterations, so the status is left open here.)"""
    prob0 = problem_from_kwargs(mc.many(ndim)[0])
    comps = sorted({(k - prob0.startind - 1) // 3 for k in _late(ndim)} | {3})
    kw, truth = mc.many(ndim, brange=(18.0, 40.0), b_truth={c: 10.0 for c in comps})
    prob = problem_from_kwargs(kw)
    kb = [_coord(prob, c, 2) for c in comps]
    assert kb[0] < 64 and all(k >= 64 for k in kb[1:]) and (ndim < 129 or 128 in kb) and (ndim != 65 or 64 in kb)
    P0 = mc.starts(kw, truth, 4, 23)
    P0[:, kb] = np.array([19.0, 22.0, 30.0, 18.0])[:, None]
    with mcalf_amd.als_fitter(None, **kw) as fit:
        out = fit.maximize_batch(P0, max_iter=15, ftol=FTOL)
        _check_invariants(fit, prob, P0, out)
        P, L, status, niter = out
    print(f"ndim {ndim}: status {status}, niter {niter}, b at {kb}: {P[:, kb].tolist()}")
    assert np.all(P[:, kb] == 18.0) and np.all(status >= 0)


# ---- the zero-gradient exit reads every turn -------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim,free_from,free_to", [(65, 64, 65), (129, 128, 129), (129, 64, 128), (65, 0, 64), (129, 0, 64)])
def test_the_zero_gradient_exit_reads_every_turn(ndim, free_from, free_to):
    """Every coordinate outside [free_from, free_to) is fixed with lo == hi at the start's value: g_u is non-zero only in the
    turn(s) that hold the free coordinates.  The row must not leave with status 2, must move every free coordinate, and
    must end as the numpy restatement does.  [0, 64) free is the complement: it fits as usual."""
    kw, truth = mc.many(ndim)
    prob = problem_from_kwargs(kw)
    lo, hi = fr.box(prob)
    P0 = mc.starts(kw, truth, 2, 24)
    keep = np.ones(ndim, dtype=bool)
    keep[free_from:free_to] = False
    P0[1, keep] = P0[0, keep]
    lo[keep] = hi[keep] = P0[0, keep]
    free = np.flatnonzero(~keep & fr.movable(prob, truth))
    assert free.size >= 1 and (free_from == 0 or free.min() >= 64)
    opt = dict(max_iter=12, cg_iters=mc.cg_iters(ndim), ftol=FTOL)
    ref = [fr.maximize_row(prob, p0, lo, hi, **opt) for p0 in P0]
    assert all(st == 1 for _, _, st, _ in ref)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        fit._lo[:], fit._hi[:] = lo, hi                                   # before the box first goes to the device
        L0 = fit.loglike_batch(P0)
        out = fit.maximize_batch(P0, **opt)
        _check_invariants(fit, prob, P0, out)
    P, L, status, niter = out
    for r in range(2):
        pr, lr, sr, nr_ = ref[r]
        dist = np.abs((P[r] - pr)[free] / (hi - lo)[free]).max()
        print(f"ndim {ndim}, free [{free_from}, {free_to}) row {r}: status {status[r]} (reference {sr}), niter {niter[r]} ({nr_}), "
              f"logL - reference's {L[r] - lr:.3e}, bar {FTOL * (1 + abs(lr)):.3e}, cube distance on the free coordinates {dist:.3e}")
        assert status[r] != 2 and status[r] == sr and abs(int(niter[r]) - nr_) <= 1 and niter[r] >= 1
        assert np.all(P[r, free] != P0[r, free]) and L[r] > L0[r]
        assert P[r, keep].tobytes() == P0[r, keep].tobytes()
        assert abs(L[r] - lr) <= FTOL * (1.0 + abs(lr))


# ---- bit invariance --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [65, 129])
def test_a_rows_bits_do_not_depend_on_batch_block_entry_or_device_count(ndim):
    kw, truth = mc.many(ndim)
    P0 = mc.starts(kw, truth, 16, 31)
    P0[7, ndim - 1] = np.nan                                              # the NaN row: decided by the last coordinate
    opt = dict(max_iter=4, ftol=FTOL)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        ref = fit.maximize_batch(P0, **opt)
        assert (ref[2] == -1).sum() == 1 and ref[2][7] == -1 and ref[3].max() >= 2
        assert _same(ref, fit.maximize_batch(P0, **opt))                            # two calls
        assert _same([a[3:11] for a in ref], fit.maximize_batch(P0[3:11], **opt))   # rows 3-10 alone
        for rpb in (1, 5, 0):
            assert _same(ref, fit.maximize_batch(P0, rows_per_block=rpb, **opt)), rpb
        side = torch.cuda.Stream()
        assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
        for stream, rpb in ((None, 0), (side, 5)):
            rc, dev = _device_fit(fit, P0, stream=stream, rows_per_block=rpb, **opt)
            assert rc == 0 and _same(ref, dev)
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as fit:
        assert _same(ref, fit.maximize_batch(P0, **opt))


# ---- underneath the fit ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("ndim", [65, 129])
def test_gradient_and_fisher_product_with_many_components(ndim):
    """Six rows near the truth, the last with an active count below ncompmax that leaves index 64 (and 128) inactive."""
    kw, truth = mc.many(ndim)
    prob = problem_from_kwargs(kw)
    P = mc.starts(kw, truth, 6, 41)
    P[5, prob.startind] = float((64 - prob.startind - 1) // 3) + 0.6
    W = mdr.kept_weights(prob)
    V = np.random.default_rng(42).uniform(-1.0, 1.0, P.shape) * mdr.tangent_scales(prob)
    V[:, prob.startind] = np.nan                                          # never read
    with mcalf_amd.als_fitter(None, **kw) as fit:
        ll, G = fit.loglike_grad_batch(P)
        assert ll.tobytes() == fit.loglike_batch(P).tobytes()
        FV = fit.fisher_matvec_batch(P, V)
        assert FV.tobytes() == fit.model_vjp_batch(P, W * fit.model_jvp_batch(P, V)).tobytes()
        assert fit.fisher_matvec_batch(P[3:4], V[3:4]).tobytes() == FV[3:4].tobytes()
    _, ref_G, S = gr.grad_batch(prob, P)
    ratio = np.abs(G - ref_G) / (1e-7 * S + 1e-9)
    at = np.unravel_index(np.argmax(ratio), ratio.shape)
    print(f"ndim {ndim}: gradient worst error / bar = {ratio.max():.3g} at row {at[0]}, column {at[1]}; "
          f"over the columns >= 64: {ratio[:, 64:].max():.3g}")
    assert np.isfinite(G).all() and ratio.max() <= 1.0
    assert np.all(G[:5, 64:] != 0.0) and np.all(G[5, 64:prob.endind] == 0.0) and np.all(G[:, prob.startind] == 0.0)
    worst = 0.0
    V0 = np.nan_to_num(V)
    for r in range(6):
        J = mdr.model_jacobian(prob, P[r])[1]
        dM, Si = mdr.jvp(J, V0[r])
        want, Sk = mdr.vjp(J, W * dM)
        bar = np.abs(J).T @ (W * (1e-7 * Si + FLOOR_REL * Si.max())) + 1e-7 * Sk + 1e-9
        worst = max(worst, float(np.max(np.abs(FV[r] - want) / bar)))
        assert FV[r, prob.startind] == 0.0
    print(f"ndim {ndim}: Fisher product worst error / bar = {worst:.3g}")
    assert worst <= 1.0 and np.all(FV[5, 64:prob.endind] == 0.0) and np.all(FV[:5, 64:] != 0.0)
