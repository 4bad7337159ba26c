"""GPU: the device Fisher product (mcalf_fisher_matvec_batch[_device]) and the batched Levenberg-Marquardt fit
(mcalf_maximize_batch[_device]) against the numpy restatement tests/fit_reference.py, the float64 reference Jacobian
(tests/model_deriv_reference.py) and scipy.optimize.least_squares.  Every case is at most 16 rows, 600 pixels and 30 outer
iterations.

Bars.  One CG step in closed form: 1e-6 max|x| (the products' own bars are 1e-7 relative and the two dot products are sums of
squares).  Full CG: the relative residual max|(A + lambda I)x - g| / max|g| with A from the reference Jacobian must be at
most 100 x the same figure of fit_reference.cg on the CPU, plus 1e-6; both figures are printed.  Convergence: status 1 on
every row, logL at least scipy's minus ftol (1 + |logL|), theta within fit_reference.THETA_BAR (cube units) of scipy's."""
import ctypes as C

import numpy as np
import pytest
import torch

import fit_reference as fr
import mcalf_amd
import model_deriv_reference as mdr
from cases import oracle_synth, problem_from_kwargs
from mcalf_amd import _lib, workloads
from test_grad_reference import bad_pixel_problem

pytestmark = pytest.mark.gpu

FTOL = 1e-10


def _civ(npix=300, specres=(8.0,), contval=(1.0,), ncomp=(1, 3), nfill=1, seed=0):
    """Two lines and a filler: data are the oracle's model of two components plus noise."""
    rng = np.random.default_rng(seed)
    wl = np.linspace(6185.0, 6215.0, npix + 2)[1:-1]
    kw = dict(fitrange=[[6185.0, 6215.0]], fitlines=["CIV 1548", "CIV 1550"], linepars=fr.CIV, ncomp=list(ncomp), nfill=nfill,
              specres=list(specres), contval=list(contval), Nrange=[12.5, 14.5], brange=[8.0, 40.0], zrange=[2.998, 3.004],
              spectrum=(wl, np.ones(npix), np.full(npix, 0.02)))
    prob = problem_from_kwargs(kw)
    truth = np.zeros(prob.ndim)
    if len(specres) > 1:
        truth[0] = 7.5
    if len(contval) > 1:
        truth[prob.startind - 1] = 1.0
    truth[prob.startind] = 2.0
    truth[prob.startind + 1:prob.startind + 7] = (13.5, 3.0003, 14.0, 13.2, 3.0016, 24.0)
    truth[prob.startind + 7:prob.endind] = np.tile((13.0, 3.001, 20.0), ncomp[1] - 2)
    if nfill:
        truth[prob.endind:] = np.tile((12.0, wl[npix // 3] / 250.0 - 1.0, 20.0), nfill)
    flux = oracle_synth(kw, truth) + rng.normal(0.0, 0.02, npix)
    return dict(kw, spectrum=(wl, flux, np.full(npix, 0.02))), truth


def _starts(kw, truth, n, seed, frac=0.03):
    """Rows at the truth plus `frac` of the box width, uniform; the ncomp slot as in the truth."""
    b = workloads.bounds_of(kw)
    lo, hi = b.min(axis=1), b.max(axis=1)
    P = truth + np.random.default_rng(seed).uniform(-1.0, 1.0, (n, truth.size)) * frac * (hi - lo)
    start = int(len(kw["specres"]) > 1) + int(len(kw["contval"]) > 1)
    P[:, start] = truth[start]
    return P


def _box(fit):
    return fit._lo.copy(), fit._hi.copy()


def _clamped(fit, prob, P0, jax=False):
    lo, hi = _box(fit)
    return np.array([np.where(fr.movable(prob, p, jax), fr.clamp(p, lo, hi), p) for p in P0])


def _device_fit(fit, P0, stream=None, **kw):
    """mcalf_maximize_batch_device on torch tensors: (P, logL, status, niter) as numpy arrays."""
    n = P0.shape[0]
    opts = _lib.mcalf_fit_opts(kw.get("max_iter", 50), kw.get("cg_iters", 0), kw.get("rows_per_block", 0), 0, kw.get("lambda0", 1e-3),
                               kw.get("ftol", FTOL))
    dP0 = torch.from_numpy(P0).cuda()
    dP = torch.full(P0.shape, -7.0, dtype=torch.float64, device="cuda")
    dL = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    dS = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    dN = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream() if stream is None else stream
    stream.wait_stream(torch.cuda.current_stream())
    rc = fit._lib.mcalf_maximize_batch_device(fit._ctx, dP0.data_ptr(), n, C.addressof(opts), dP.data_ptr(), dL.data_ptr(), dS.data_ptr(),
                                              dN.data_ptr(), C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    return rc, (dP.cpu().numpy(), dL.cpu().numpy(), dS.cpu().numpy(), dN.cpu().numpy())


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---- the Fisher entry ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["two_lines_filler", "bad_pixels"])
def test_fisher_entry_is_the_composed_route_bit_for_bit(which):
    if which == "bad_pixels":
        kw = bad_pixel_problem(specres=(6.0, 9.0), contval=(0.9, 1.1))
    else:
        kw, _ = _civ(npix=301, specres=(6.0, 9.0))
    prob = problem_from_kwargs(kw)
    W = mdr.kept_weights(prob)
    assert ((W == 0.0).sum() == 49) == (which == "bad_pixels")
    P = workloads.draw_P(kw, 8, np.random.default_rng(5))
    V = np.random.default_rng(6).uniform(-1.0, 1.0, P.shape) * mdr.tangent_scales(prob)
    V[:, prob.startind] = np.nan                                     # never read
    with mcalf_amd.als_fitter(None, **kw) as fit:
        want = fit.model_vjp_batch(P, W * fit.model_jvp_batch(P, V))
        got = fit.fisher_matvec_batch(P, V)
        assert got.tobytes() == want.tobytes()
        assert np.all(got[:, prob.startind] == 0.0) and np.isfinite(got).all()
        assert fit.fisher_matvec_batch(P[3:4], V[3:4]).tobytes() == want[3:4].tobytes()
        dP, dV = torch.from_numpy(P).cuda(), torch.from_numpy(V).cuda()
        side = torch.cuda.Stream()
        assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
        for _ in range(2):
            dFV = torch.full(P.shape, -7.0, dtype=torch.float64, device="cuda")
            side.wait_stream(torch.cuda.current_stream())
            assert fit._lib.mcalf_fisher_matvec_batch_device(fit._ctx, dP.data_ptr(), dV.data_ptr(), 8, dFV.data_ptr(),
                                                             C.c_void_p(side.cuda_stream)) == 0
            side.synchronize()
            assert dFV.cpu().numpy().tobytes() == want.tobytes()
        assert fit._lib.mcalf_fisher_matvec_batch(fit._ctx, None, None, 0, None) == 0
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as fit:
        assert fit.fisher_matvec_batch(P, V).tobytes() == want.tobytes()
        rc = fit._lib.mcalf_fisher_matvec_batch_device(fit._ctx, dP.data_ptr(), dV.data_ptr(), 8, dFV.data_ptr(), None)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in fit._lib.mcalf_last_error(fit._ctx)


# ---- one CG step in closed form; full CG -------------------------------------------------------------------------------------

def _many_components():
    """ndim 67: one line, ncomp [1, 22], 257 pixels -- a lane of the row's wave owns two parameters."""
    rng = np.random.default_rng(3)
    wl = np.linspace(6188.0, 6212.0, 257)
    kw = dict(fitrange=[[6187.9, 6212.1]], fitlines=["CIV 1548"], linepars=fr.CIV[:1], ncomp=[1, 22], nfill=0, specres=[8.0], contval=[1.0],
              Nrange=[12.5, 14.5], brange=[8.0, 40.0], zrange=[2.9975, 3.0115], spectrum=(wl, np.ones(257), np.full(257, 0.02)))
    truth = np.concatenate([[22.0], np.column_stack([rng.uniform(12.8, 13.4, 22), np.linspace(2.9985, 3.0105, 22), rng.uniform(12.0, 30.0, 22)]).ravel()])
    flux = oracle_synth(kw, truth) + rng.normal(0.0, 0.02, 257)
    return dict(kw, spectrum=(wl, flux, np.full(257, 0.02))), truth


def _reference_system(prob, th, lo, hi):
    """(A, g_u, pins) of the fit's linear system at `th`, from the float64 reference Jacobian."""
    _, G, F = fr.point(prob, th)
    s = hi - lo
    pin = fr.pins(prob, th, G, lo, hi)
    A = s[:, None] * F * s[None, :]
    A[pin, :] = 0.0
    A[:, pin] = 0.0
    return A, np.where(pin, 0.0, s * G), pin


@pytest.mark.parametrize("ndim", [10, 67])
def test_one_cg_step_in_closed_form(ndim):
    if ndim == 10:
        kw, P0 = fr.convergence_kwargs(), fr.convergence_starts()
    else:
        kw, truth = _many_components()
        P0 = _starts(kw, truth, 4, 11, frac=0.02)
    prob = problem_from_kwargs(kw)
    assert prob.ndim == ndim
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
        got = (P[r] - P0[r]) / np.where(s > 0, s, 1.0)
        err = np.abs(got - x)[inside].max()
        print(f"ndim {ndim} row {r}: max|x| {np.abs(x).max():.3e}, error {err:.3e}, bar {1e-6 * np.abs(x).max():.3e}")
        assert err <= 1e-6 * np.abs(x).max()
        assert np.array_equal(P[r][pin], P0[r][pin])


def test_full_cg_solves_the_damped_system():
    kw, P0 = fr.convergence_kwargs(), fr.convergence_starts()
    prob = problem_from_kwargs(kw)
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
        assert np.all((P[r] > lo)[~pin] & (P[r] < hi)[~pin])          # no clamping: theta_1 - theta_0 is s x
        res = np.abs(M @ x - g).max() / np.abs(g).max()
        print(f"row {r}: CG relative residual, device {res:.3e}, fit_reference on the CPU {res_cpu:.3e}, bar {100 * res_cpu + 1e-6:.3e}")
        assert res <= 100 * res_cpu + 1e-6


# ---- convergence ---------------------------------------------------------------------------------------------------------------

def test_every_start_converges_to_scipys_optimum():
    kw, P0 = fr.convergence_kwargs(), fr.convergence_starts()
    prob = problem_from_kwargs(kw)
    lo, hi = fr.box(prob)
    want = [fr.scipy_optimum(prob, p0, lo, hi) for p0 in P0]
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert np.array_equal(fit._lo, lo) and np.array_equal(fit._hi, hi)
        P, L, status, niter = fit.maximize_batch(P0, max_iter=30, ftol=FTOL)
        assert L.tobytes() == fit.loglike_batch(P).tobytes()
        p1, l1, s1, n1 = fit.maximize(P0[2], max_iter=30, ftol=FTOL)
        assert p1.tobytes() == P[2].tobytes() and l1 == L[2] and s1 == status[2] and n1 == niter[2]
    for r, (ps, ls) in enumerate(want):
        dist = np.abs((P[r] - ps) / (hi - lo)).max()
        print(f"start {r}: status {status[r]}, niter {niter[r]}, scipy - ours {ls - L[r]:.3e}, bar {FTOL * (1 + abs(L[r])):.3e}, "
              f"cube distance {dist:.3e}, bar {fr.THETA_BAR:.3e}")
    assert np.all(status == 1), status
    for r, (ps, ls) in enumerate(want):
        assert L[r] >= ls - FTOL * (1.0 + abs(L[r]))
        assert np.abs((P[r] - ps) / (hi - lo)).max() <= fr.THETA_BAR


def test_rejected_steps_follow_the_reference():
    """A far start at the default lambda0 = 1e-3: the barely damped steps overshoot and are rejected (the numpy restatement rejects
    9 of its 21 iterations) before the damping has grown enough.  Same end as the reference: status 1, logL within the stopping
    rule's bar ftol (1 + |logL|) (measured 1.6e-10 against 7.7e-8), theta within THETA_BAR (measured 5.6e-7), as many iterations."""
    kw = fr.convergence_kwargs()
    prob = problem_from_kwargs(kw)
    lo, hi = fr.box(prob)
    p0 = fr.TRUTH.copy()
    p0[1:] += np.tile([0.6, 4e-4, 12.0], 3) * np.array([1, -1, 1, -1, 1, -1, 1, 1, -1])
    trace = []
    p, logl, status, niter = fr.maximize_row(prob, p0, lo, hi, max_iter=30, lambda0=1e-3, ftol=FTOL, trace=trace)
    assert status == 1 and sum(not rec["accepted"] for rec in trace) >= 5
    with mcalf_amd.als_fitter(None, **kw) as fit:
        P, L, st, ni = fit.maximize_batch(p0[None, :], max_iter=30, lambda0=1e-3, ftol=FTOL)
    print(f"device: status {st[0]}, niter {ni[0]}, logL {L[0]!r}; reference: status {status}, niter {niter}, logL {logl!r}; "
          f"cube distance {np.abs((P[0] - p) / (hi - lo)).max():.3e}")
    assert st[0] == 1 and abs(int(ni[0]) - niter) <= 1
    assert abs(L[0] - logl) <= FTOL * (1.0 + abs(logl))
    assert np.abs((P[0] - p) / (hi - lo)).max() <= fr.THETA_BAR


# ---- invariants --------------------------------------------------------------------------------------------------------------

def _check_invariants(fit, prob, P0, out, jax=False):
    P, L, status, niter = out
    lo, hi = _box(fit)
    start = _clamped(fit, prob, P0, jax)
    Ls = fit.loglike_batch(start)
    for r in range(P0.shape[0]):
        mv = fr.movable(prob, P0[r], jax)
        assert P[r][~mv].tobytes() == P0[r][~mv].tobytes()           # the ncomp slot and the inactive slots: bit for bit
        if status[r] == -1:
            assert P[r].tobytes() == P0[r].tobytes() and niter[r] == 0
            continue
        assert L[r] >= Ls[r]
        assert np.all(P[r][mv] >= lo[mv]) and np.all(P[r][mv] <= hi[mv])
        fixed = mv & (hi == lo)
        assert P[r][fixed].tobytes() == start[r][fixed].tobytes()
    assert L.tobytes() == fit.loglike_batch(P).tobytes()


@pytest.mark.parametrize("specres,contval,jax", [((8.0,), (1.0,), False), ((6.0, 9.0), (1.0,), False), ((6.0, 9.0), (0.9, 1.1), False),
                                                   ((8.0,), (0.9, 1.1), True)])
def test_invariants_on_every_layout(specres, contval, jax):
    """startind 0, 1, 2 (a floated R on the numpy path among them) and a JAX-semantics context, with a filler, an active count
    below ncompmax, a fractional ncomp slot, inactive slots outside the box, starts outside the box and a NaN row."""
    kw, truth = _civ(specres=specres, contval=contval)
    prob = problem_from_kwargs(kw)
    s0 = prob.startind
    P0 = _starts(kw, truth, 8, 21)
    P0[1, s0] = 2.7                                                   # two active components
    P0[2, s0] = 1.0
    P0[:, s0 + 7:s0 + 10] = (15.5, 3.2, 77.0)                         # the inactive third slot, outside the box
    P0[3, s0 + 1] = 99.0                                              # outside the box: clamped to hi
    P0[4, s0 + 3] = -5.0
    P0[5, s0 + 2] = np.nan                                            # a bad start
    with mcalf_amd.als_fitter(None, conv_mode="jax" if jax else "numpy", **kw) as fit:
        out = fit.maximize_batch(P0, max_iter=12, ftol=FTOL)
        _check_invariants(fit, prob, P0, out, jax)
        P, L, status, niter = out
        assert status[5] == -1 and np.all(status[[0, 1, 2, 6, 7]] >= 0)
        # monotone: more iterations never lower logL, and a finished row is carried
        short = fit.maximize_batch(P0, max_iter=3, ftol=FTOL)
        ok = status != -1
        assert np.all(L[ok] >= short[1][ok])
        # the NaN row does not change its neighbours' bits
        clean = P0.copy()
        clean[5] = P0[6]
        other = fit.maximize_batch(clean, max_iter=12, ftol=FTOL)
        keep = [0, 1, 2, 3, 4, 6, 7]
        assert _same([a[keep] for a in out], [a[keep] for a in other])
        # max_iter = 0: the clamped start, its logL, status 0 (or -1), niter 0
        P_, L_, s_, n_ = fit.maximize_batch(P0, max_iter=0)
        start = _clamped(fit, prob, P0, jax)
        assert np.all(n_ == 0) and s_[5] == -1 and np.all(np.delete(s_, 5) == 0)
        assert np.delete(P_, 5, axis=0).tobytes() == np.delete(start, 5, axis=0).tobytes() and P_[5].tobytes() == P0[5].tobytes()
        assert np.delete(L_, 5).tobytes() == fit.loglike_batch(np.delete(start, 5, axis=0)).tobytes()


def test_a_fixed_coordinate_and_a_bound_the_data_push_against():
    """lo == hi on one z keeps its bits; data made with b = 10 under brange [18, 40] end with b exactly at lo."""
    rng = np.random.default_rng(4)
    wl = np.linspace(6188.0, 6200.0, 200)
    kw = dict(fitrange=[[6187.9, 6200.1]], fitlines=["CIV 1548"], linepars=fr.CIV[:1], ncomp=[1, 2], nfill=0, specres=[8.0], contval=[1.0],
              Nrange=[12.5, 14.5], brange=[18.0, 40.0], zrange=[2.998, 3.002], spectrum=(wl, np.ones(200), np.full(200, 0.02)))
    truth = np.array([2.0, 13.6, 2.9992, 10.0, 13.3, 3.0008, 25.0])
    flux = oracle_synth(dict(kw, brange=[5.0, 40.0]), truth) + rng.normal(0.0, 0.02, 200)
    kw = dict(kw, spectrum=(wl, flux, np.full(200, 0.02)))
    prob = problem_from_kwargs(kw)
    P0 = np.tile(truth, (4, 1))
    P0[:, 3] = (19.0, 22.0, 30.0, 18.0)
    P0[:, [1, 4]] += rng.uniform(-0.1, 0.1, (4, 2))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        fit._lo[5] = fit._hi[5] = 3.0008                              # before the box first goes to the device
        out = fit.maximize_batch(P0, max_iter=30, ftol=FTOL)
        _check_invariants(fit, prob, P0, out)
        P, L, status, niter = out
    print("status", status, "niter", niter, "b", P[:, 3])
    assert np.all(P[:, 3] == 18.0)
    assert P[:, 5].tobytes() == P0[:, 5].tobytes()
    assert np.all(status == 1)


# ---- bit invariance ------------------------------------------------------------------------------------------------------------

def test_a_rows_bits_do_not_depend_on_batch_block_entry_or_device_count():
    kw, truth = _civ(specres=(6.0, 9.0))
    P0 = _starts(kw, truth, 16, 31, frac=0.05)
    P0[7, 3] = np.nan
    opt = dict(max_iter=8, ftol=FTOL)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        ref = fit.maximize_batch(P0, **opt)
        assert (ref[2] == -1).sum() == 1 and ref[3].max() >= 2
        assert _same(ref, fit.maximize_batch(P0, **opt))                            # two calls
        assert _same([a[3:11] for a in ref], fit.maximize_batch(P0[3:11], **opt))   # rows 3-10 alone
        for rpb in (1, 5, 0):
            assert _same(ref, fit.maximize_batch(P0, rows_per_block=rpb, **opt)), rpb
        side = torch.cuda.Stream()
        for stream, rpb in ((None, 0), (side, 5), (side, 5)):
            rc, dev = _device_fit(fit, P0, stream=stream, rows_per_block=rpb, **opt)
            assert rc == 0 and _same(ref, dev)
        assert fit._lib.mcalf_maximize_batch(fit._ctx, None, 0, C.addressof(_lib.mcalf_fit_opts(1, 0, 0, 0, 1e-3, 0.0)), None, None, None, None) == 0
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as fit:
        assert _same(ref, fit.maximize_batch(P0, **opt))


# ---- refusals ------------------------------------------------------------------------------------------------------------------

def test_refusals():
    kw, truth = _civ()
    P0 = _starts(kw, truth, 4, 41)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        opts = _lib.mcalf_fit_opts(5, 0, 0, 0, 1e-3, FTOL)
        P, L = np.empty_like(P0), np.empty(4)
        st, ni = np.empty(4, dtype=np.int32), np.empty(4, dtype=np.int32)
        args = (P0.ctypes.data, 4, C.addressof(opts), P.ctypes.data, L.ctypes.data, st.ctypes.data, ni.ctypes.data)
        assert fit._lib.mcalf_maximize_batch(fit._ctx, *args) == _lib.MCALF_ERR_INVALID
        assert b"mcalf_set_prior has not been called" in fit._lib.mcalf_last_error(fit._ctx)
        fit._lo[2], fit._hi[2] = fit._hi[2], fit._lo[2]
        with pytest.raises(RuntimeError, match="lo > hi at parameter 2"):
            fit.maximize_batch(P0)
        fit._lo[2], fit._hi[2] = fit._hi[2], np.inf
        fit._prior_key = None
        with pytest.raises(RuntimeError, match="not finite"):
            fit.maximize_batch(P0)
        with pytest.raises(ValueError):
            fit.maximize_batch(P0[:, :-1])
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as fit:
        fit._ensure_prior()
        rc, _ = _device_fit(fit, P0, max_iter=2)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in fit._lib.mcalf_last_error(fit._ctx)
