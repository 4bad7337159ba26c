"""GPU: the model Jacobian's products (mcalf_model_jvp_batch[_device], mcalf_model_vjp_batch[_device], fisher_matvec_batch,
model_jacobian) where tests/test_gpu_model_deriv.py does not take them: the seeded random problems of tests/test_gpu_fuzz.py
(single lines, triplets, a ~ 1e-11, logarithmic / jittered / masked grids, two fit ranges, LSFs that wrap round the spectrum
up to seven times, b down to 0.8 km/s, logN up to 20.5; bad pixels on every odd seed); spectra of one 256-pixel tile +- 1
pixel, two tiles, 64 and 8 pixels; the smallest parameter layouts; more rows than one grid.y holds; one context taken through
VJP, JVP and gradient in turn at growing and shrinking batch sizes; the operands of the device entries left as they were;
three shards of unequal size; the `out=` arguments; the Fisher product's symmetry and sign.

Reference: the float64 dense Jacobian of tests/model_deriv_reference.py, anchored on the oracle for these very problems by
tests/test_model_deriv_reference.py (`EDGE`).  Bars, per row, as in tests/test_gpu_model_deriv.py:
    JVP  |d dM_i| <= 1e-7 S_i + FLOOR_REL max_i S_i,   S_i = sum_k |v_k J_ik|
    VJP  |d G_k|  <= 1e-7 S_k + 1e-9,                  S_k = sum_i |q_i J_ik|
FLOOR_REL is that file's rule applied to this file's cases: ten times the worst |d dM_i| / max_i S_i measured on an MI355X
on the pixels with S_i < 1e-6 max_i S_i, never above 1e-9.  The worst here is 1.72e-15 (random problem 1; every
other case at most 1.2e-16, most of them 0: DESIGN 3.7 lists them), below the 1.33e-14 that set the existing floor, so
FLOOR_REL = 1.33e-13 holds for this file as well.

`model_jacobian` with neither a component nor a filler (F = 1 everywhere) has an R column that is 0 but for rounding: the
sum of the taps' R derivatives, which cancel.  A bar relative to that column would be a bar on the rounding itself, so the
column gets what float64 allows a sum of 2 n + 1 products: (2 n + 1) 2^-52 cont sum_k |dw_k/dR| for the device and as much
for the reference (`_tap_rounding`).  It is ~1e-16 against a continuum column of 1.

Worst error / bar measured on an MI355X (printed by the tests, `pytest -s`):
    random problems   JVP 0.011 (seed 1, both paths; per seed 3.0e-6 .. 0.011), VJP 0.0012 (seed 12, JAX path), Fisher
                      product 0.0074 (seed 9, numpy path); LSF wrapping seven times (seed 11): 1.9e-7 / 3.2e-4 / 0.0049
    tile shapes       JVP at most 2.8e-4 (513 pixels), VJP at most 1.5e-4 (8 pixels, 13 taps wrapped)
    smallest layouts  JVP at most 1.4e-4, VJP at most 3.4e-5 (one filler, 600 pixels); neither component nor filler:
                      JVP 9.2e-8, VJP 6.4e-7, model_jacobian 0.0045 (numpy) / 0.018 (JAX) with an R column of at most 6.6e-18
    70 000 rows       JVP 1.6e-4, VJP 5.3e-5 on the 64 sampled rows
    Fisher symmetry   |<U, F V> - <F U, V>| 7.3e-10 (numpy) / 1.2e-9 (JAX) of its bar; <V, F V> >= 4.7e3; each product
                      1.0e-4 of its own bar
The other tests compare bits."""
import functools

import numpy as np
import pytest
import torch

import grad_reference as gr
import mcalf_amd
import model_deriv_reference as mdr
from mcalf_amd import workloads
from cases import problem_from_kwargs, with_bad_pixels
from test_grad_reference import bad_pixel_problem
from test_gpu_fuzz import LINESETS
from test_gpu_model_deriv import _check, _civ, _device_call, _jacobians, _jvp_compare, _tangents, _vjp_compare
from test_model_deriv_reference import FUZZ_SEEDS, LAYOUTS, TILE_NPIX, fuzz_problem, layout_problem, short_problem, tile_problem

pytestmark = pytest.mark.gpu

FLOOR_REL = 1.33e-13


def _mode(jax):
    return "jax" if jax else "numpy"


def _full_taps(kw):
    """2 n + 1 of the widest LSF the prior allows (the numpy path's astropy count, hires_fitter.py:458)."""
    return 2 * int(np.ceil(3.0348 * (max(kw["specres"]) / 2.354820) / kw["velstep"])) + 1


@functools.lru_cache(maxsize=None)
def _fuzz_reach():
    """What the 14 random problems contain, from their kwargs alone."""
    kws = [fuzz_problem(seed)[0] for seed in FUZZ_SEEDS]
    return dict(triplet=sum(len(kw["linepars"]) == 3 for kw in kws),
                single=sum(len(kw["linepars"]) == 1 for kw in kws),
                weakgamma=sum(kw["linepars"] == LINESETS["weakgamma"] for kw in kws),
                two_ranges=sum(len(kw["fitrange"]) == 2 for kw in kws),
                lsf_wraps=sum(_full_taps(kw) > problem_from_kwargs(kw).wl.size for kw in kws),
                narrow_b=sum(kw["brange"][0] == 0.8 for kw in kws),
                damped_N=sum(kw["Nrange"][1] == 20.5 for kw in kws))


def _fisher_compare(FV, Js, V, W, what, startind):
    """Worst error / bar of Fisher products against J^T (W (J v)); the bar per column is the JVP's carried through J^T W
    plus the VJP's own for the cotangent W J v (test_fisher_matvec_with_bad_pixels).  Also returns the bars."""
    worst, bars = 0.0, []
    for r, J in enumerate(Js):
        dM, Si = mdr.jvp(J, np.where(np.isnan(V[r]), 0.0, V[r]))
        want, Sk = mdr.vjp(J, W * dM)
        bar = np.abs(J).T @ (W * (1e-7 * Si + FLOOR_REL * Si.max())) + 1e-7 * Sk + 1e-9
        worst = max(worst, float(np.max(np.abs(FV[r] - want) / bar)))
        assert FV[r, startind] == 0.0, (what, r)
        bars.append(bar)
    print(f"Fisher {what}: worst error / bar = {worst:.3g}")
    return worst, np.array(bars)


@pytest.mark.parametrize("jax", [False, True], ids=_mode)
@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_random_problems(seed, jax):
    """The problems and rows of test_random_problem_matches_oracle, the same documented JAX refusals; on every odd seed 5 %
    of the pixels are bad (NaN flux, NaN error, zero error in turn), which only the Fisher product's W sees."""
    reach = _fuzz_reach()
    assert all(count >= 1 for count in reach.values()), reach
    kw, P = fuzz_problem(seed)
    if seed & 1:
        npix = problem_from_kwargs(kw).wl.size
        idx = np.sort(np.random.default_rng(2000 + seed).choice(npix, size=max(1, npix // 20), replace=False))
        kw = with_bad_pixels(kw, idx, [("flux_nan", "err_nan", "err_zero")[k % 3] for k in range(idx.size)])
    prob = problem_from_kwargs(kw)
    try:
        fit = mcalf_amd.als_fitter(None, conv_mode=_mode(jax), **kw)
    except RuntimeError as exc:
        # the refusals tests/test_gpu_fuzz.py documents (JAX semantics only); the reference raises there as well
        assert jax and ("MCALF_ERR_RANGE" in str(exc) or "MCALF_ERR_INVALID" in str(exc))
        return
    V = _tangents(prob, P.shape[0], seed)
    Q = np.random.default_rng(3000 + seed).normal(0.0, 1.0, (P.shape[0], prob.wl.size))
    with fit:
        dM, G, FV = fit.model_jvp_batch(P, V), fit.model_vjp_batch(P, Q), fit.fisher_matvec_batch(P, V)
    assert dM.shape == Q.shape and G.shape == P.shape and FV.shape == P.shape
    assert np.isfinite(dM).all() and np.isfinite(G).all() and np.isfinite(FV).all()
    what = f"seed {seed} {_mode(jax)}"
    Js = _jacobians(prob, P, jax)
    wj, wv = _jvp_compare(dM, Js, V, what), _vjp_compare(G, Js, Q, what)
    W = mdr.kept_weights(prob)
    assert ((W == 0.0).sum() > 0) == bool(seed & 1)
    wf, _ = _fisher_compare(FV, Js, V, W, what, prob.startind)
    assert wj <= 1.0 and wv <= 1.0 and wf <= 1.0, (what, wj, wv, wf)
    assert np.all(G[:, prob.startind] == 0.0)


@pytest.mark.parametrize("npix", TILE_NPIX)
def test_tile_shapes(npix):
    """Spectra of one tile (256 pixels) minus one, exactly one, one more, two, two and one more, 64 and 8 pixels; CIV
    doublet, free resolution and continuum, 9 to 13 taps, which wrap round the 8-pixel spectrum on every row (all 8 pixels
    of every row are compared: the JVP has no reduction that could average a wrong one away).  JAX semantics too where
    the fixed grid fits the spectrum; where it does not, the documented refusal."""
    kw, P = tile_problem(npix)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        n = fit.info.n_cap
        assert fit.info.npix == npix and n == 6
    dM, _ = _check(kw, P, what=f"npix {npix}", seed=npix)
    assert dM.shape == (6, npix)
    if npix == 8:
        assert np.all(2 * np.ceil(3.0348 * (P[:, 0] / 2.354820) / 2.0) + 1 > npix)
    if 2 * n + 1 <= npix:
        _check(kw, P, jax=True, what=f"npix {npix} jax", seed=npix)
    else:
        with pytest.raises(RuntimeError, match="MCALF_ERR_INVALID"):
            mcalf_amd.als_fitter(None, conv_mode="jax", **kw)


def _tap_rounding(prob, p, jax):
    """What float64 allows the R column of a Jacobian whose taps' R derivatives cancel: a sum of 2 n + 1 products, each
    rounded to 2^-53 relative, on the device and in the reference."""
    R, cont, _ = mdr.row_parameters(prob, p, jax)
    _, dw = gr._taps(prob, R, jax)
    return 2 * dw.size * 2.0 ** -52 * abs(cont) * np.abs(dw).sum()


@pytest.mark.parametrize("ncomp,nfill", LAYOUTS)
def test_smallest_parameter_layouts(ncomp, nfill):
    """One filler and no target component, one component and no filler, neither (the record list of a row is never
    empty: host_grad.cpp, grad_nslots; jvp_forward then loops over nothing and F = 1).  With neither, the JVP is
    v_cont L(1) + v_R cont (dL/dR)(1) = v_cont, and `model_jacobian` is (0, 1, 0) on every pixel."""
    for npix in (257, 600):
        kw, P = layout_problem(ncomp, nfill, npix)
        prob = problem_from_kwargs(kw)
        assert prob.ndim == 3 + 3 * ncomp[1] + 3 * nfill
        for jax in (False, True):
            what = f"ncomp {ncomp} nfill {nfill} npix {npix} {_mode(jax)}"
            dM, G = _check(kw, P, jax=jax, what=what, seed=npix)
            if ncomp[1] or nfill:
                continue
            vc = _tangents(prob, P.shape[0], npix)[:, 1:2]
            assert np.all(np.abs(dM - vc) <= (1e-7 + FLOOR_REL) * np.abs(vc)), what
            with mcalf_amd.als_fitter(None, conv_mode=_mode(jax), **kw) as fit:
                J = fit.model_jacobian(P[0])
            _, want = mdr.model_jacobian(prob, P[0], jax=jax)
            assert J.shape == want.shape == (npix, 3)
            bar = 1e-7 * np.abs(want) + FLOOR_REL * np.abs(want).max(axis=0)
            bar[:, 0] += _tap_rounding(prob, P[0], jax)
            print(f"model_jacobian {what}: worst error / bar = {np.max(np.abs(J - want)[:, :2] / bar[:, :2]):.3g}, "
                  f"max |R column| = {np.abs(J[:, 0]).max():.3g}")
            assert np.all(np.abs(J - want) <= bar), what
            assert np.all(J[:, 2] == 0.0) and np.all(np.abs(J[:, 1] - 1.0) <= 1e-7)


def test_more_rows_than_one_grid_y():
    """70 000 rows of the 64-pixel, 49-tap problem in one JVP call and one VJP call: two passes, of 65 535 and 4 465 rows
    (grad_chunk_rows), whose offsets into V, dM, Q and G are the JVP's and the VJP's own (host_grad.cpp: bind).  Every row has the bits it
    has in a block of 4096, and 64 sampled rows -- both sides of the pass boundary among them -- match the reference."""
    kw = short_problem()
    prob = problem_from_kwargs(kw)
    n = 70000
    P = workloads.draw_P(kw, n, np.random.default_rng(70))
    V = _tangents(prob, n, 71)
    Q = np.random.default_rng(72).normal(0.0, 1.0, (n, prob.wl.size))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert fit.info.npix == 64 and fit.info.n_cap == 24
        dM, G = fit.model_jvp_batch(P, V), fit.model_vjp_batch(P, Q)
        for lo in range(0, n, 4096):
            hi = lo + 4096
            assert np.array_equal(fit.model_jvp_batch(P[lo:hi], V[lo:hi]), dM[lo:hi]), lo
            assert np.array_equal(fit.model_vjp_batch(P[lo:hi], Q[lo:hi]), G[lo:hi]), lo
    assert np.isfinite(dM).all() and np.isfinite(G).all()
    rows = np.unique(np.concatenate([[0, 65534, 65535, 65536, n - 1], np.random.default_rng(1).choice(n, 59, replace=False)]))
    Js = _jacobians(prob, P[rows], False)
    wj = _jvp_compare(dM[rows], Js, V[rows], "70000 rows, sampled")
    wv = _vjp_compare(G[rows], Js, Q[rows], "70000 rows, sampled")
    assert wj <= 1.0 and wv <= 1.0


def test_one_context_through_every_entry_in_turn():
    """VJP (64 rows), JVP (4096), gradient (512), VJP (4096), JVP (7), gradient (4096) on ONE context: the VJP comes first,
    so it runs before the q workspace exists (it reads the caller's cotangent and allocates none); the JVP then writes its
    T there and the gradient its q; the batch grows and shrinks.  Each result has the bits of the same call on a context
    of its own."""
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1))
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 4096, np.random.default_rng(91))
    V = _tangents(prob, 4096, 92)
    Q = np.random.default_rng(93).normal(0.0, 1.0, (4096, prob.wl.size))
    calls = [("vjp", slice(0, 64)), ("jvp", slice(0, 4096)), ("grad", slice(100, 612)), ("vjp", slice(0, 4096)),
             ("jvp", slice(4000, 4007)), ("grad", slice(0, 4096))]

    def run(fit, kind, s):
        if kind == "vjp":
            return (fit.model_vjp_batch(P[s], Q[s]),)
        if kind == "jvp":
            return (fit.model_jvp_batch(P[s], V[s]),)
        return fit.loglike_grad_batch(P[s])

    with mcalf_amd.als_fitter(None, **kw) as fit:
        shared = [run(fit, kind, s) for kind, s in calls]
    for (kind, s), got in zip(calls, shared):
        with mcalf_amd.als_fitter(None, **kw) as fresh:
            want = run(fresh, kind, s)
        assert kind == "grad" or np.isfinite(want[0]).all()
        for a, b in zip(got, want):
            assert np.array_equal(a, b, equal_nan=True), (kind, s)


def _bits(t):
    return t.view(torch.int64)


def test_device_entries_leave_their_operands_alone():
    """The VJP's pass reads the caller's cotangent through the q workspace pointer (a const_cast in host_grad.cpp: kProdVjp): after the
    device entries, on a side stream, dQ -- and dP, dV after the JVP -- hold the bits they held before."""
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1))
    prob = problem_from_kwargs(kw)
    n = 300
    P = workloads.draw_P(kw, n, np.random.default_rng(94))
    V = _tangents(prob, n, 95)
    Q = np.random.default_rng(96).normal(0.0, 1.0, (n, prob.wl.size))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        dM, G = fit.model_jvp_batch(P, V), fit.model_vjp_batch(P, Q)
        dP, dV, dQ = (torch.from_numpy(a).cuda() for a in (P, V, Q))
        kept = [t.clone() for t in (dP, dV, dQ)]
        ddM = torch.full(Q.shape, -7.0, dtype=torch.float64, device="cuda")
        dG = torch.full(P.shape, -7.0, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        assert _device_call(fit, "mcalf_model_vjp_batch_device", dP, dQ, n, dG, side.cuda_stream) == 0
        side.synchronize()
        assert torch.equal(_bits(dQ), _bits(kept[2])) and torch.equal(_bits(dP), _bits(kept[0]))
        assert _device_call(fit, "mcalf_model_jvp_batch_device", dP, dV, n, ddM, side.cuda_stream) == 0
        side.synchronize()
        assert torch.equal(_bits(dP), _bits(kept[0])) and torch.equal(_bits(dV), _bits(kept[1]))
        assert torch.equal(_bits(dQ), _bits(kept[2]))
        assert np.array_equal(ddM.cpu().numpy(), dM) and np.array_equal(dG.cpu().numpy(), G)
        # the host entries: the caller's arrays likewise
        P0, V0, Q0 = P.copy(), V.copy(), Q.copy()
        fit.model_vjp_batch(P, Q)
        fit.model_jvp_batch(P, V)
        assert np.array_equal(P, P0) and np.array_equal(V, V0, equal_nan=True) and np.array_equal(Q, Q0)


def test_uneven_shards():
    """1001 rows over three shards (334 + 334 + 333 or the like: not a multiple of 3): the bits of the single-device context."""
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1))
    prob = problem_from_kwargs(kw)
    n = 1001
    P = workloads.draw_P(kw, n, np.random.default_rng(97))
    V = _tangents(prob, n, 98)
    Q = np.random.default_rng(99).normal(0.0, 1.0, (n, prob.wl.size))
    with mcalf_amd.als_fitter(None, device=-1, **kw) as fit:
        dM, G = fit.model_jvp_batch(P, V), fit.model_vjp_batch(P, Q)
    assert np.isfinite(dM).all() and np.isfinite(G).all()
    with mcalf_amd.als_fitter(None, device=[0, 0, 0], **kw) as fit:
        assert fit.info.ndevices == 3
        assert np.array_equal(fit.model_jvp_batch(P, V), dM) and np.array_equal(fit.model_vjp_batch(P, Q), G)


def test_out_arguments():
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1))
    prob = problem_from_kwargs(kw)
    n, npix, ndim = 9, prob.wl.size, prob.ndim
    P = workloads.draw_P(kw, n, np.random.default_rng(101))
    V = _tangents(prob, n, 102)
    Q = np.random.default_rng(103).normal(0.0, 1.0, (n, npix))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        for call, X, width in ((fit.model_jvp_batch, V, npix), (fit.model_vjp_batch, Q, ndim)):
            want = call(P, X)
            out = np.full((n, width), -7.0)
            got = call(P, X, out=out)
            assert got.shape == (n, width) and np.shares_memory(got, out) and np.array_equal(out, want)
            with pytest.raises(ValueError):
                call(P, X, out=np.empty((n, width), dtype=np.float32))
            with pytest.raises(ValueError):
                call(P, X, out=np.empty((n - 1, width)))
            with pytest.raises(ValueError):
                call(P, X, out=np.empty((n, width + 1)))
            assert np.array_equal(call(P, X), want)                  # (a refused `out` leaves the context usable)


@pytest.mark.parametrize("jax", [False, True], ids=_mode)
def test_fisher_product_is_symmetric_and_positive(jax):
    """J^T W J on 16 rows of the 600-pixel problem with 49 bad pixels, two independent tangent sets U and V:
    |<U, F V> - <F U, V>| within the two propagated bars contracted with |U| and |V|, and <V, F V> >= -bar."""
    kw = bad_pixel_problem(specres=(6.0, 9.0), contval=(0.9, 1.1))
    prob = problem_from_kwargs(kw)
    W = mdr.kept_weights(prob)
    assert (W == 0.0).sum() == 49
    P = workloads.draw_P(kw, 16, np.random.default_rng(111))
    U, V = (np.nan_to_num(_tangents(prob, 16, seed)) for seed in (112, 113))
    with mcalf_amd.als_fitter(None, conv_mode=_mode(jax), **kw) as fit:
        FU, FV = fit.fisher_matvec_batch(P, U), fit.fisher_matvec_batch(P, V)
    Js = _jacobians(prob, P, jax)
    wu, bar_U = _fisher_compare(FU, Js, U, W, f"U {_mode(jax)}", prob.startind)
    wv, bar_V = _fisher_compare(FV, Js, V, W, f"V {_mode(jax)}", prob.startind)
    assert wu <= 1.0 and wv <= 1.0
    sym = np.abs(np.sum(U * FV, axis=1) - np.sum(FU * V, axis=1))
    bar = np.sum(np.abs(U) * bar_V, axis=1) + np.sum(np.abs(V) * bar_U, axis=1)
    quad = np.sum(V * FV, axis=1)
    print(f"Fisher symmetry ({_mode(jax)}): worst |<U, F V> - <F U, V>| / bar = {np.max(sym / bar):.3g}; "
          f"min <V, F V> = {quad.min():.3g}")
    assert np.all(sym <= bar)
    assert np.all(quad >= -np.sum(np.abs(V) * bar_V, axis=1))
