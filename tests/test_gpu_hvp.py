"""GPU: the product of logL's exact Hessian with a vector -- mcalf_loglike_hvp_batch[_device] and the Python entries on it
(loglike_hvp_batch, lnlhood_hessp, lnlhood_hessian) -- against the float64 dense Hessian of tests/hess_reference.py
(Richardson-extrapolated central differences of the gradient reference; anchored, and its own error measured, on these very
problems by tests/test_hess_reference.py); rows and columns fixed by definition; symmetry on the device; the curvature term
vanishing where the residual does; bit equality across batch positions, entries, streams, device counts and passes.

The bar, per row:   |d HV_k| <= REL_BAR S_k + FLOOR_REL max_k S_k,   S_k = sum_j |v_j| sum_i W_i |J_ik| |J_ij|
(the Fisher product in absolute values, from tests/model_deriv_reference.py: a scale that cancellation between the Fisher and
the curvature term cannot shrink).
  REL_BAR   = 3.6e-6: ten times the reference's own worst error over these cases, 3.6e-7 S (tests/test_hess_reference.py:
              the R-R entry of a logN = 12 filler, where the curvature term is thirty times the Fisher scale), and not below
              the project's derivative bar of 1e-7.
  FLOOR_REL = DESIGN 3.7's rule: ten times the worst |d HV_k| / max S measured on an MI355X on the entries with
              S_k < 1e-6 max S (a tangent along one line's parameter, an entry of a line it barely overlaps: S_k is the
              product of two far wings while rounding scales with each line's own terms), never above 1e-9.
Every case prints its worst error / bar, its worst error in units of S_k on the entries above the small-S limit, and its
worst small-S error in units of max S (pytest -s), which is how the floor is measured again after a change of the kernels."""
import ctypes as C

import numpy as np
import pytest
import torch

import hess_reference as hr
import mcalf_amd
import model_deriv_reference as mdr
from mcalf_amd import _lib, workloads
from cases import problem_from_kwargs
from test_grad_reference import _kw, bad_pixel_problem
from test_hess_reference import CASES, REL_BAR, reference, tangent_rows
from test_model_deriv_reference import short_problem

pytestmark = pytest.mark.gpu

FLOOR_REL = 3.65e-13      # ten times 3.65e-14 (R_le_velstep_free; every other case at most 1.9e-14)


def _mode(jax):
    return "jax" if jax else "numpy"


def _bar(S):
    return REL_BAR * S + FLOOR_REL * S.max()


def _compare(HV, V, dense, which, what):
    """Worst error / bar of a batch of HVP rows against the dense reference of each row's theta; prints the measures the
    module docstring names.  Entries that are 0 by definition must be exactly 0."""
    worst, rel, small = 0.0, 0.0, 0.0
    for r, t in enumerate(which):
        H, _, A = dense[t]
        want, S = hr.hvp(H, A, V[r])
        assert np.isfinite(HV[r]).all(), (what, r)
        dead = np.all(A == 0.0, axis=0)
        assert np.all(HV[r][dead] == 0.0), (what, r)
        d = np.abs(HV[r] - want)
        worst = max(worst, float(np.max(d / _bar(S))))
        big = S >= hr.SMALL * S.max()
        rel = max(rel, float(np.max(d[big] / S[big])))
        lo = ~big & ~dead
        if lo.any():
            small = max(small, float(d[lo].max() / S.max()))
    print(f"HVP {what}: worst error / bar = {worst:.3g}, worst error = {rel:.3g} S, worst small-S error = {small:.3g} max S")
    return worst


def _fit(name, **more):
    kw, _, jax, _, _ = reference(name)
    return mcalf_amd.als_fitter(None, conv_mode=_mode(jax), **kw, **more)


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_reference(name):
    """Every problem of tests/test_hess_reference.py: CASES: per theta a random tangent and one tangent with a single
    non-zero entry per parameter class (for the wing-only damped line: along z alone and along b alone, the second-order
    cancellation case -- every Voigt evaluation from the asymptotic series)."""
    kw, prob, jax, thetas, dense = reference(name)
    P, V, which = tangent_rows(name)
    with _fit(name) as fit:
        if name == "wide_lsf":
            assert 2 * fit.info.n_cap + 64 > 4096
        HV = fit.loglike_hvp_batch(P, V)
        assert HV.shape == P.shape
        assert _compare(HV, V, dense, which, name) <= 1.0
        s = prob.startind
        assert np.all(HV[:, s] == 0.0)
        # the entries of V in columns that are 0 by definition are never read: any value there, the same bits
        W = V.copy()
        for r, t in enumerate(which):
            W[r, np.all(dense[t][2] == 0.0, axis=0)] = np.nan
        assert np.array_equal(fit.loglike_hvp_batch(P, W), HV)
        if name == "R_le_velstep_free":
            assert np.all(HV[:, 0] == 0.0) and np.isnan(W[:, 0]).all()
        if name.startswith("ncomp"):
            active = [int(min(max(np.floor(p[s]) if jax else np.trunc(p[s]), 0), 3)) for p in P]
            assert sorted(set(active)) == [0, 1, 2]
            for r, nc in enumerate(active):
                assert np.all(HV[r, s + 1 + 3 * nc: prob.endind] == 0.0) and np.isnan(W[r, s + 1 + 3 * nc: prob.endind]).all()
                assert np.all(HV[r, prob.endind:] != 0.0)                    # the filler is always active
        if name.startswith("bad_pixels"):
            assert (mdr.kept_weights(prob) == 0.0).sum() == 49


def test_veto_rows_and_rows_beyond_the_tap_cap_are_nan():
    kw, _, seed = workloads.config("A")
    P = workloads.draw_P(kw, 16, np.random.default_rng(21))
    V = np.random.default_rng(22).uniform(-1.0, 1.0, P.shape) * mdr.tangent_scales(problem_from_kwargs(kw))
    P[2] = [2.0, 14.5, 3.005, 40.0, 14.5, 3.006, 40.0]          # strong absorption where the data has none: vetoed
    with mcalf_amd.als_fitter(None, Asymmlike=True, gauss_cdf=[0, 0, 0], **kw) as fit:
        ll = fit.loglike_batch(P)
        keep = np.flatnonzero(np.isfinite(ll))
        assert ll[2] == -np.inf and keep.size >= 1
        HV = fit.loglike_hvp_batch(P, V)
        assert np.array_equal(np.isnan(HV).all(axis=1), ~np.isfinite(ll)) and np.array_equal(np.isnan(HV).any(axis=1), ~np.isfinite(ll))
        assert np.array_equal(HV[keep], fit.loglike_hvp_batch(P[keep], V[keep]))       # the neighbours: as on their own
    with mcalf_amd.als_fitter(None, **kw) as fit:                                      # and as without the veto
        assert np.array_equal(HV[keep], fit.loglike_hvp_batch(P[keep], V[keep]))
    kw = _kw(specres=(6.0, 9.0), contval=(0.9, 1.1))
    P = workloads.draw_P(kw, 6, np.random.default_rng(31))
    V = np.random.default_rng(32).uniform(-1.0, 1.0, P.shape) * mdr.tangent_scales(problem_from_kwargs(kw))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert np.ceil(3.0348 * (12.0 / 2.354820) / fit.velstep) > fit.info.n_cap
        own = fit.loglike_hvp_batch(P, V)
        assert np.isfinite(own).all()
        B = P.copy()
        B[1, 0] = 12.0                                                   # more taps than the context provisions
        B[4, 0] = 1e300
        HV = fit.loglike_hvp_batch(B, V)
        assert np.all(np.isnan(HV[[1, 4]]))
        assert np.array_equal(HV[[0, 2, 3, 5]], own[[0, 2, 3, 5]])


@pytest.mark.parametrize("jax", [False, True], ids=_mode)
def test_symmetry_on_the_device(jax):
    """<U, H V> against <H U, V> on 16 rows of the 600-pixel problem with 49 bad pixels, two independent tangent sets: within
    the two bars contracted with |U| and |V|."""
    kw = bad_pixel_problem(specres=(6.0, 9.0), contval=(0.9, 1.1))
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 16, np.random.default_rng(111))
    U, V = (np.random.default_rng(seed).uniform(-1.0, 1.0, P.shape) * mdr.tangent_scales(prob) for seed in (112, 113))
    with mcalf_amd.als_fitter(None, conv_mode=_mode(jax), **kw) as fit:
        HU, HV = fit.loglike_hvp_batch(P, U), fit.loglike_hvp_batch(P, V)
    assert np.isfinite(HU).all() and np.isfinite(HV).all()
    worst = 0.0
    for r, p in enumerate(P):
        A, _ = hr.fisher_abs(prob, p, jax)
        u, v = (np.where(np.all(A == 0.0, axis=0), 0.0, x[r]) for x in (U, V))
        bar = np.sum(np.abs(u) * _bar(A @ np.abs(v))) + np.sum(np.abs(v) * _bar(A @ np.abs(u)))
        worst = max(worst, abs(np.dot(u, HV[r]) - np.dot(HU[r], v)) / bar)
    print(f"HVP symmetry ({_mode(jax)}): worst |<U, H V> - <H U, V>| / bar = {worst:.3g}")
    assert worst <= 1.0


def test_dense_hessian_and_hessp():
    kw, prob, jax, thetas, dense = reference("civ_free_R_cont")
    H, _, A = dense[0]
    s = prob.startind
    with _fit("civ_free_R_cont") as fit:
        got = fit.lnlhood_hessian(thetas[0])
        v = np.random.default_rng(5).uniform(-1.0, 1.0, prob.ndim) * mdr.tangent_scales(prob)
        hp = fit.lnlhood_hessp(thetas[0], v)
        assert np.array_equal(hp, fit.loglike_hvp_batch(thetas[:1], v.reshape(1, -1))[0])
    assert got.shape == (prob.ndim, prob.ndim)
    dead = np.all(A == 0.0, axis=0)
    assert dead[s] and np.all(got[dead] == 0.0) and np.all(got[:, dead] == 0.0)
    worst = 0.0
    for j in np.flatnonzero(~dead):                                      # row j is H e_j
        worst = max(worst, float(np.max(np.abs(got[j] - H[:, j]) / _bar(A[:, j]))))
    asym = np.abs(got - got.T)
    print(f"lnlhood_hessian: worst error / bar = {worst:.3g}; worst asymmetry / bar = "
          f"{np.max(asym[A > 0] / (REL_BAR * A + FLOOR_REL * A.max(axis=0))[A > 0]):.3g}")
    assert worst <= 1.0
    want, S = hr.hvp(H, A, v)
    assert np.all(np.abs(hp - want) <= _bar(S))


@pytest.mark.parametrize("jax", [False, True], ids=_mode)
def test_curvature_term_vanishes_where_the_residual_does(jax):
    """The data are the noiseless model of `truth` on the context's own path; evaluated at `truth`, r = 0 on every pixel and
    H v = -J^T W J v: H v + fisher_matvec_batch(P, V) is 0 within the bar.  (A pass without the dq = -W dM terms would
    return 0 here instead of the Fisher product.)"""
    kw = _kw(specres=(6.0, 9.0), contval=(0.9, 1.1), ncomp=(2, 2))
    prob = problem_from_kwargs(kw)
    truth = workloads.draw_P(kw, 1, np.random.default_rng(7))[0]
    truth[prob.startind + 1: prob.startind + 7] = [13.6, 3.0031, 14.0, 13.9, 3.0049, 22.0]
    wl, _, err = kw["spectrum"]
    with mcalf_amd.als_fitter(None, conv_mode=_mode(jax), **kw) as fit:
        flux = fit.model_batch(truth.reshape(1, -1))[0]
    kw = dict(kw, spectrum=(wl, flux, err))
    P = np.tile(truth, (8, 1))
    V = np.random.default_rng(8).uniform(-1.0, 1.0, P.shape) * mdr.tangent_scales(prob)
    with mcalf_amd.als_fitter(None, conv_mode=_mode(jax), **kw) as fit:
        assert np.array_equal(fit.model_batch(truth.reshape(1, -1))[0], flux)
        HV, FV = fit.loglike_hvp_batch(P, V), fit.fisher_matvec_batch(P, V)
    A, _ = hr.fisher_abs(problem_from_kwargs(kw), truth, jax)
    worst = 0.0
    for r in range(8):
        S = A @ np.abs(np.where(np.all(A == 0.0, axis=0), 0.0, V[r]))
        worst = max(worst, float(np.max(np.abs(HV[r] + FV[r]) / _bar(S))))
        assert np.max(np.abs(FV[r])[S > 0] / S[S > 0]) > 1e-3                        # (the Fisher product itself is far above the bar)
    print(f"curvature term at r = 0 ({_mode(jax)}): worst |H v + F v| / bar = {worst:.3g}")
    assert worst <= 1.0


def _device_call(fit, dP, dV, n, dHV, stream):
    return fit._lib.mcalf_loglike_hvp_batch_device(fit._ctx, dP.data_ptr(), dV.data_ptr(), n, dHV.data_ptr(), C.c_void_p(stream))


def _bits(t):
    return t.view(torch.int64)


def test_bit_equality():
    """A row alone against the same row inside 300; the device entry on a non-default stream against the host entry, its
    operands left as they were; the gradient of the same context before and after (shared workspaces); two devices."""
    kw = _kw(specres=(6.0, 9.0), contval=(0.9, 1.1))
    prob = problem_from_kwargs(kw)
    n = 300
    P = workloads.draw_P(kw, n, np.random.default_rng(94))
    V = np.random.default_rng(95).uniform(-1.0, 1.0, P.shape) * mdr.tangent_scales(prob)
    V[:, prob.startind] = np.nan
    with mcalf_amd.als_fitter(None, **kw) as fit:
        ll0, G0 = fit.loglike_grad_batch(P)
        HV = fit.loglike_hvp_batch(P, V)
        assert np.isfinite(HV).all()
        ll1, G1 = fit.loglike_grad_batch(P)
        assert np.array_equal(G0, G1) and np.array_equal(ll0, ll1)
        assert np.array_equal(fit.loglike_hvp_batch(P, V), HV)
        for r in (0, 177, 299):
            assert np.array_equal(fit.loglike_hvp_batch(P[r:r + 1], V[r:r + 1])[0], HV[r])
        out = np.full(P.shape, -7.0)
        assert np.shares_memory(fit.loglike_hvp_batch(P, V, out=out), out) and np.array_equal(out, HV)
        with pytest.raises(ValueError):
            fit.loglike_hvp_batch(P[:4], V[:3])
        dP, dV = torch.from_numpy(P).cuda(), torch.from_numpy(V).cuda()
        kept = dP.clone(), dV.clone()
        dHV = torch.full(P.shape, -7.0, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        assert side.cuda_stream != torch.cuda.default_stream().cuda_stream
        for _ in range(2):                                               # (the second call allocates nothing)
            dHV.fill_(-7.0)
            side.wait_stream(torch.cuda.current_stream())
            assert _device_call(fit, dP, dV, n, dHV, side.cuda_stream) == 0
            side.synchronize()
            assert np.array_equal(dHV.cpu().numpy(), HV)
        assert torch.equal(_bits(dP), _bits(kept[0])) and torch.equal(_bits(dV), _bits(kept[1]))
        assert fit._lib.mcalf_loglike_hvp_batch_device(fit._ctx, None, None, 0, None, None) == 0
        assert fit._lib.mcalf_loglike_hvp_batch(fit._ctx, P.ctypes.data, None, 4, HV.ctypes.data) == _lib.MCALF_ERR_INVALID
        ll2, G2 = fit.loglike_grad_batch(P)
        assert np.array_equal(G0, G2) and np.array_equal(ll0, ll2)
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as fit:
        assert fit.info.ndevices == 2
        assert np.array_equal(fit.loglike_hvp_batch(P, V), HV)
        rc = _device_call(fit, dP, dV, 8, dHV, torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in fit._lib.mcalf_last_error(fit._ctx)


def test_two_passes():
    """70 000 rows of the 64-pixel, 49-tap problem: an HVP pass holds 3416 bytes of workspace per row there, so the byte
    budget would allow 117 000 rows and the 65 535-row cap of grid.y cuts the batch into passes of 65 535 and 4 465 rows.
    Every row has the bits it has in its half of the batch (one pass each), and 64 sampled rows -- both sides of the pass
    boundary among them -- match the reference."""
    kw = short_problem()
    prob = problem_from_kwargs(kw)
    n = 70000
    assert (384 << 20) // ((4 * 64 + 3 * 49 + 8 + 2 * 6 + prob.ndim) * 8) > 65535 and prob.wl.size == 64
    P = workloads.draw_P(kw, n, np.random.default_rng(70))
    V = np.random.default_rng(71).uniform(-1.0, 1.0, P.shape) * mdr.tangent_scales(prob)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.info.npix == 64 and fit.info.n_cap == 24
        HV = fit.loglike_hvp_batch(P, V)
        h = n // 2
        assert np.array_equal(fit.loglike_hvp_batch(P[:h], V[:h]), HV[:h]) and np.array_equal(fit.loglike_hvp_batch(P[h:], V[h:]), HV[h:])
    assert np.isfinite(HV).all()
    rows = np.unique(np.concatenate([[0, 65534, 65535, 65536, n - 1], np.random.default_rng(1).choice(n, 59, replace=False)]))
    dense = []
    for p in P[rows]:
        H, E = hr.hessian(prob, p)
        dense.append((H, E, hr.fisher_abs(prob, p)[0]))
    assert _compare(HV[rows], V[rows], dense, range(rows.size), "70000 rows, sampled") <= 1.0
