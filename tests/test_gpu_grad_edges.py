"""GPU: the analytic gradient (mcalf_loglike_grad_batch[_device]) where tests/test_gpu_grad.py does not take it: the seeded
random problems of tests/test_gpu_fuzz.py (single lines, triplets, a ~ 1e-11, logarithmic / jittered / masked grids,
several fit ranges, LSFs wider than the spectrum, bad pixels on every odd seed); a damped line seen only in its wing, where
the b column is the asymptotic series of e = H + u H_u + a H_a alone; spectra of one 256-pixel gradient tile +- 1 pixel,
two tiles, 64 and 8 pixels, and the smallest parameter layouts; a batch of more rows than one grid.y holds; the untested
arguments of the two entry points; resolutions outside the prior.

Bar against tests/grad_reference.py, as in tests/test_gpu_grad.py: |dG_k| <= 1e-7 S_k + 1e-9 per row and column; logL
bit-equal to loglike_batch.

Worst |dG| / bar measured on an MI355X (printed by the tests, `pytest -s`):
    random problems   0.023 (seed 10, numpy path); per seed 1.3e-5 .. 0.023, the JAX path within 2x of the numpy path
    wing only         1.2e-6 overall, set by the b column (S_b = 2.4 .. 8.1)
    tile shapes       at most 0.0020 (8 pixels); 255 / 256 / 257 / 512 / 513 / 64 pixels 6.8e-5 .. 6.7e-4
    smallest layouts  at most 0.0044 (no component and no filler, 600 pixels)
    70 000 rows       3.5e-4 on the 64 sampled rows
    R outside prior   2.2e-5"""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_reference as gr
import mcalf_amd
from mcalf_amd import _lib, workloads
from cases import ASYM_BRACKETS, bracket_counts, problem_from_kwargs, wing_only_problem, with_bad_pixels
from test_gpu_fuzz import random_problem
from test_gpu_grad import _assert_close, _civ

pytestmark = pytest.mark.gpu

GRAD_TILE = 256            # kGradBlock (grad_args.h)


def _worst(what, G, ref_G, S):
    fin = np.isfinite(ref_G).all(axis=1)
    r = np.abs(G[fin] - ref_G[fin]) / (1e-7 * S[fin] + 1e-9)
    print(f"{what}: worst |dG| / bar = {r.max() if r.size else 0.0:.3g}")
    _assert_close(G, ref_G, S, what)
    return r


def _check(kw, P, jax=False, what=""):
    prob = problem_from_kwargs(kw)
    with mcalf_amd.als_fitter(None, conv_mode="jax" if jax else "numpy", **kw) as fit:
        ll, G = fit.loglike_grad_batch(P)
        assert np.array_equal(ll, fit.loglike_batch(P)), what
    with np.errstate(divide="ignore", invalid="ignore"):
        _, ref_G, S = gr.grad_batch(prob, P, jax=jax)
    _worst(what, G, ref_G, S)
    return G, ref_G, S


@pytest.mark.parametrize("seed", range(14))
def test_gradient_of_random_problems(seed):
    """The problems and rows of test_random_problem_matches_oracle, both convolution modes, the same documented JAX
    refusals; on every odd seed 5 % of the pixels are bad (NaN flux, NaN error, zero error in turn)."""
    rng = np.random.default_rng(1000 + seed)
    kw = random_problem(rng)
    P = workloads.draw_P(kw, 5, rng)
    if seed & 1:
        npix = problem_from_kwargs(kw).wl.size
        idx = np.sort(np.random.default_rng(2000 + seed).choice(npix, size=max(1, npix // 20), replace=False))
        kw = with_bad_pixels(kw, idx, [("flux_nan", "err_nan", "err_zero")[k % 3] for k in range(idx.size)])
    for mode in ("numpy", "jax"):
        try:
            fit = mcalf_amd.als_fitter(None, conv_mode=mode, **kw)
        except RuntimeError as exc:
            # the refusals tests/test_gpu_fuzz.py documents (JAX semantics only); the reference raises there as well
            assert mode == "jax" and ("MCALF_ERR_RANGE" in str(exc) or "MCALF_ERR_INVALID" in str(exc))
            continue
        fit.close()
        G, ref_G, _ = _check(kw, P, jax=mode == "jax", what=f"seed {seed} {mode}")
        assert np.isfinite(ref_G).all() and np.isfinite(G).all()


def test_wing_only_damped_line():
    """tests/cases.py: wing_only_problem.  No pixel within |u| < 8.5 of the line, every truncation bracket of the
    asymptotic series populated (asserted from the reference's u), so an `e` series wrong in one bracket shows in the b
    column: its scale S_b holds no line core (2 .. 8 here, the 1e-9 floor of the bar is < 1 % of it)."""
    kw, P = wing_only_problem()
    prob = problem_from_kwargs(kw)
    total = np.zeros(len(ASYM_BRACKETS) - 1, dtype=int)
    for p in P:
        umin, counts = bracket_counts(prob, p)
        assert umin >= 8.5 and counts.sum() == prob.wl.size
        total += counts
    assert np.all(total >= 20), total
    G, ref_G, S = _check(kw, P, what="wing only")
    b = prob.startind + 3
    assert np.all(S[:, b] > 1.0)
    print("wing only, b column: worst |dG| / bar =", (np.abs(G[:, b] - ref_G[:, b]) / (1e-7 * S[:, b] + 1e-9)).max())
    # the same rows one at a time: each row alone stays inside one or two brackets per pixel range
    with mcalf_amd.als_fitter(None, **kw) as fit:
        for r, p in enumerate(P):
            assert np.array_equal(fit.lnlhood_grad(p)[1], G[r])


@pytest.mark.parametrize("npix", [GRAD_TILE - 1, GRAD_TILE, GRAD_TILE + 1, 2 * GRAD_TILE, 2 * GRAD_TILE + 1, 64, 8])
def test_tile_shapes(npix):
    """Spectra of one gradient tile (256 pixels) minus one, exactly one, one more, two, two and one more, 64 and 8 pixels;
    CIV doublet, free resolution and continuum, a 13-tap LSF at most (it wraps round the 8-pixel spectrum, as astropy's
    boundary='wrap' does).  JAX semantics too where the fixed grid fits the spectrum; where it does not, the documented
    refusal."""
    kw = _civ(npix=npix, specres=(6.0, 9.0), contval=(0.9, 1.1), velstep=2.0, seed=npix)
    P = workloads.draw_P(kw, 6, np.random.default_rng(npix))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        n = fit.info.n_cap
        assert fit.info.npix == npix and n == 6
    _check(kw, P, what=f"npix {npix}")
    if 2 * n + 1 <= npix:
        _check(kw, P, jax=True, what=f"npix {npix} jax")
    else:
        with pytest.raises(RuntimeError, match="MCALF_ERR_INVALID"):
            mcalf_amd.als_fitter(None, conv_mode="jax", **kw)


@pytest.mark.parametrize("ncomp,nfill", [((0, 0), 1), ((1, 1), 0), ((0, 0), 0)])
def test_smallest_parameter_layouts(ncomp, nfill):
    """One filler and no target component, one component and no filler, neither (the record list of a row is never
    empty: host_grad.cpp, grad_nslots)."""
    for npix in (GRAD_TILE + 1, 600):
        kw = _civ(npix=npix, specres=(6.0, 9.0), contval=(0.9, 1.1), ncomp=ncomp, nfill=nfill, velstep=2.0, seed=npix + nfill)
        P = workloads.draw_P(kw, 4, np.random.default_rng(3))
        G, _, _ = _check(kw, P, what=f"ncomp {ncomp} nfill {nfill} npix {npix}")
        assert G.shape[1] == 3 + 3 * ncomp[1] + 3 * nfill and np.all(G[:, 2] == 0.0)
        _check(kw, P, jax=True, what=f"ncomp {ncomp} nfill {nfill} npix {npix} jax")


def _short_problem():
    """64 pixels, one CIV component, a 49-tap LSF: ~2 KB of per-row workspace, so the byte bound of a pass alone
    (kGradChunkBytes = 384 MiB) would put ~200 000 rows into one launch."""
    kw = _civ(npix=64, ncomp=(1, 1), nfill=0, velstep=0.43, seed=64)
    assert int(np.ceil(3.0348 * (8.0 / 2.354820) / 0.43)) == 24
    return kw


def test_more_rows_than_one_grid_y():
    """70 000 rows of a 64-pixel problem in one call.  The pixel kernels carry the row on grid.y, which the device limits
    to 65 536 (hipDeviceAttributeMaxGridDimY on an MI355X), and the byte bound of a pass allows ~200 000 such rows:
    grad_chunk_rows() caps a pass at 65 535 rows, as the likelihood's wide path caps its own (host_wide.cpp).
    The call returns 0 (the wrapper raises otherwise), every row has the bits it has in a block of 4096, and 64 sampled
    rows -- both sides of the pass boundary among them -- match the reference."""
    kw = _short_problem()
    prob = problem_from_kwargs(kw)
    n = 70000
    P = workloads.draw_P(kw, n, np.random.default_rng(70))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.info.npix == 64 and fit.info.n_cap == 24
        ll, G = fit.loglike_grad_batch(P)
        assert np.array_equal(ll, fit.loglike_batch(P))
        for lo in range(0, n, 4096):
            l1, g1 = fit.loglike_grad_batch(P[lo:lo + 4096])
            assert np.array_equal(l1, ll[lo:lo + 4096]) and np.array_equal(g1, G[lo:lo + 4096]), lo
    assert np.isfinite(G).all()
    rows = np.unique(np.concatenate([[0, 65534, 65535, 65536, n - 1], np.random.default_rng(1).choice(n, 59, replace=False)]))
    _, ref_G, S = gr.grad_batch(prob, P[rows])
    _worst("70000 rows, sampled", G[rows], ref_G, S)


def test_entry_point_arguments():
    kw, _, seed = workloads.config("A")
    P = workloads.draw_P(kw, 300, np.random.default_rng(seed + 7))
    n, ndim = P.shape
    for device in (-1, [0, 0]):
        with mcalf_amd.als_fitter(None, device=device, **kw) as fit:
            ll, G = fit.loglike_grad_batch(P)
            # logL == NULL: G alone, the same bits
            G2 = np.full((n, ndim), -7.0)
            assert fit._lib.mcalf_loglike_grad_batch(fit._ctx, P.ctypes.data, n, None, G2.ctypes.data) == 0
            assert np.array_equal(G2, G)
            # batch == 0: nothing to do, whatever the pointers
            assert fit._lib.mcalf_loglike_grad_batch(fit._ctx, None, 0, None, None) == 0
            assert fit._lib.mcalf_loglike_grad_batch_device(fit._ctx, None, 0, None, None, None) == (
                0 if device == -1 else _lib.MCALF_ERR_INVALID)       # (a multi-device context refuses the entry as such)
            assert fit._lib.mcalf_loglike_grad_batch(fit._ctx, P.ctypes.data, -1, None, G2.ctypes.data) == _lib.MCALF_ERR_INVALID
            dP = torch.from_numpy(P).cuda()
            dL = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
            dG = torch.full((n, ndim), -7.0, dtype=torch.float64, device="cuda")
            if device == -1:
                # the device entry on torch's default stream and on a side stream: the same bits
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                assert fit._lib.mcalf_loglike_grad_batch_device(fit._ctx, dP.data_ptr(), n, dL.data_ptr(), dG.data_ptr(), st) == 0
                torch.cuda.synchronize()
                assert np.array_equal(dG.cpu().numpy(), G) and np.array_equal(dL.cpu().numpy(), ll)
                dL.fill_(-7.0)
                dG.fill_(-7.0)
                side = torch.cuda.Stream()
                side.wait_stream(torch.cuda.current_stream())
                with torch.cuda.stream(side):
                    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                    assert st.value != torch.cuda.default_stream().cuda_stream
                    assert fit._lib.mcalf_loglike_grad_batch_device(fit._ctx, dP.data_ptr(), n, dL.data_ptr(), dG.data_ptr(), st) == 0
                side.synchronize()
                assert np.array_equal(dG.cpu().numpy(), G) and np.array_equal(dL.cpu().numpy(), ll)
            else:
                # a multi-device context has no device-pointer entry: the error, and nothing written
                st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
                rc = fit._lib.mcalf_loglike_grad_batch_device(fit._ctx, dP.data_ptr(), n, dL.data_ptr(), dG.data_ptr(), st)
                assert rc == _lib.MCALF_ERR_INVALID
                assert b"not available on a multi-device context" in fit._lib.mcalf_last_error(fit._ctx)
                torch.cuda.synchronize()
                assert torch.all(dG == -7.0).item() and torch.all(dL == -7.0).item()


def test_resolution_outside_the_prior():
    """Free resolution in [6, 9] km/s.  R = 12 needs more taps than the context provisioned (ceil(3.0348 sigma) > n_cap):
    whatever loglike_batch gives for that row, loglike_grad_batch gives the same bits, and G is all NaN exactly where
    that logL is NaN or -inf.  R slightly above the prior with the provisioned tap count is an ordinary row.  R = NaN and
    R <= velstep rows (no convolution, hires_fitter.py:445) mixed with ordinary rows: the ordinary rows keep the bits
    they have in a batch of their own, the R column of the unconvolved rows is 0, and a NaN resolution gives the bits of
    any other unconvolved one."""
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1))
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 12, np.random.default_rng(31))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        n_cap, velstep = fit.info.n_cap, fit.velstep
        taps = lambda R: np.ceil(3.0348 * (R / 2.354820) / velstep)      # noqa: E731
        assert taps(12.0) > n_cap and taps(9.2) == n_cap and velstep > 1.0
        own_ll, own_G = fit.loglike_grad_batch(P)
        Q = P.copy()
        Q[1, 0] = 12.0
        Q[3, 0] = 9.2
        Q[5, 0] = np.nan
        Q[7, 0] = 0.5 * velstep
        Q[8] = Q[5]
        Q[8, 0] = 0.9 * velstep                                      # row 5 with a resolution that is a number
        Q[9, 0] = 1e300
        ll, G = fit.loglike_grad_batch(Q)
        assert np.array_equal(ll, fit.loglike_batch(Q), equal_nan=True)
        ordinary = [0, 2, 4, 6, 10, 11]
        assert np.array_equal(ll[ordinary], own_ll[ordinary]) and np.array_equal(G[ordinary], own_G[ordinary])
        assert np.array_equal(np.isnan(G).all(axis=1), ~(ll > -np.inf)) and np.array_equal(np.isnan(G).any(axis=1), ~(ll > -np.inf))
        assert not ll[1] > -np.inf and not ll[9] > -np.inf and np.isfinite(ll[[3, 5, 7, 8]]).all()
        assert np.all(G[[5, 7, 8], 0] == 0.0)
        assert ll[5] == ll[8] and np.array_equal(G[5], G[8])
    keep = [3, 7, 8]
    _, ref_G, S = gr.grad_batch(prob, Q[keep])
    _worst("R outside the prior", G[keep], ref_G, S)
