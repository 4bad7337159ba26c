"""GPU: spectra with bad data pixels -- NaN flux, NaN error, error 0 -- through every epilogue that restates the
reference's `np.nansum` (hires_fitter.py:292-294): the fused kernel's plain-logL loop and its general loop (chi2, the
asymmetric veto, the model output, the JAX boundary), the wide-LSF kernel, and the gradient's `q`.  Every other test of
the suite builds a finite spectrum (one NaN flux pixel in tests/test_gpu_parity.py apart).

The bad pixels sit where an epilogue could go wrong unseen (`bad_positions`): the first and the last pixel, both sides of
every tile seam of the fused kernel (`fit.info.tile`), of the gradient's 256-pixel tiles and of the wide kernel's
2048-pixel blocks, both sides of a boundary between 8-pixel thread groups, the last (partial) group of eight, a run longer
than a whole LSF window (2n + 1 pixels), and a random 7 %.  The oracle is `oracle.numpy_oracle` on the `Problem` built
from the same kwargs; the gradient's is tests/grad_reference.py (anchored on such a spectrum by central differences in
tests/test_grad_reference.py).  Bars, the suite's own: logL and chi2 |d| < 1e-7 + 2e-9 |want| (tests/test_gpu_fuzz.py),
the model 2e-10, G 1e-7 S_k + 1e-9 (tests/test_gpu_grad.py).

Worst error / bar measured on an MI355X (printed by every test, `pytest -s`):
    logL   A 3.7e-5   C 8.2e-5   C jax 8.2e-5   E 4.6e-6   wide (333 px) 2.5e-4   wide (4500 px) 1.6e-4
           (unit-cube rows: at most 4.0e-4, wide; under the veto: at most 2.5e-4, wide)
    chi2   A 3.6e-5   C 8.0e-5   E 4.6e-6   wide 3.5e-4   wide (4500 px) 6.0e-5
    G      A 1.9e-5   C 1.6e-4   C jax 1.6e-4   E 0.028   wide 0.20
    model  max |d| 3.2e-12 (C, targonly), bar 2e-10; bit-identical to the model of the finite spectrum everywhere"""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_reference as gr
import mcalf_amd
from mcalf_amd import _lib, workloads
from cases import BAD_KINDS, oracle_synth, problem_from_kwargs, with_bad_pixels
from oracle import numpy_oracle as o
from test_gpu_grad import _assert_close, _civ

pytestmark = pytest.mark.gpu

GRAD_TILE = 256            # kGradBlock (grad_args.h)
WIDE_BLOCK = 2048          # kWideBlockPix (kernel_args.h)


def bad_positions(info, rng, wide=False):
    """Sorted pixel indices of the cases the module docstring lists, for a context with `info` (mcalf_info_t)."""
    npix, tile, n = int(info.npix), int(info.tile), int(info.n_cap)
    idx = {0, npix - 1}
    for step in (tile, GRAD_TILE, WIDE_BLOCK):
        for s in range(step, npix, step):                       # both sides of every seam
            idx |= {s - 1, s}
    g = 8 * max(1, npix // 24)                                   # a boundary between two 8-pixel thread groups
    idx |= {g - 1, g}
    idx |= set(range(npix - (npix % 8 or 8), npix))             # the last group of eight (partial when npix % 8)
    # a whole LSF window and more; on a wide-LSF context the window is longer than the spectrum, so a third of it
    run = min(2 * n + 3, npix // 3)
    start = (npix // 2) | 1
    idx |= set(range(start, start + run))
    idx |= set(rng.choice(npix, size=int(0.07 * npix), replace=False).tolist())
    out = np.array(sorted(idx))
    assert out[0] == 0 and out[-1] == npix - 1 and (wide or run >= 2 * n + 1)
    return out


def mixed_kinds(idx, rng):
    return [BAD_KINDS[k] for k in rng.integers(0, len(BAD_KINDS), len(idx))]


def _info(kw, **extra):
    with mcalf_amd.als_fitter(None, **extra, **kw) as fit:
        info = fit.info
        return info, (int(info.npix), int(info.tile), int(info.ntiles), int(info.n_cap))


def _ratio(what, got, want):
    """The suite's logL bar; non-finite values must be the oracle's own."""
    fin = np.isfinite(want)
    assert np.array_equal(got[~fin], want[~fin], equal_nan=True), (what, got, want)
    r = np.abs(got[fin] - want[fin]) / (1e-7 + 2e-9 * np.abs(want[fin]))
    print(f"{what}: worst |d| / bar = {r.max() if r.size else 0.0:.3g}")
    assert np.all(r < 1.0), (what, got, want)


def _grad_ratio(what, G, ref_G, S):
    fin = np.isfinite(ref_G).all(axis=1)
    if fin.any():
        print(f"{what}: worst |dG| / bar = {(np.abs(G[fin] - ref_G[fin]) / (1e-7 * S[fin] + 1e-9)).max():.3g}")
    _assert_close(G, ref_G, S, what)


def _device_logl(fit, P):
    dP = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    out = torch.full((len(P),), float("nan"), dtype=torch.float64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    _lib.check(fit._lib.mcalf_loglike_batch_device(fit._ctx, dP.data_ptr(), len(P), out.data_ptr(), st), fit._ctx)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _wide(npix=333):
    if npix == 333:                                              # as test_grad_wide_lsf / test_gpu_wide_lsf.py build one
        return _civ(npix=333, specres=(6.0, 9.0), contval=(0.9, 1.1), nfill=2, velstep=0.0031, seed=333)
    return _civ(npix=npix, specres=(8.0, 8.5), velstep=0.0045, nfill=0, seed=npix)      # two fused tiles, three wide blocks


def _config(name):
    """(finite kwargs, rows, als_fitter extras, multi-tile?, wide?) of the settings the logL / chi2 / model cases run on."""
    if name in ("A", "C", "C_jax", "E"):
        kw, _, seed = workloads.config(name[0], oracle_synth)
        rng = np.random.default_rng(seed + 50)
        P = workloads.draw_P(kw, {"A": 8, "C": 8, "E": 4}[name[0]], rng, damped=2 if name == "E" else 0)
        return kw, P, (dict(conv_mode="jax") if name == "C_jax" else {}), name == "E", False
    kw = _wide(333 if name == "wide" else 4500)
    return kw, workloads.draw_P(kw, 4, np.random.default_rng(9)), {}, name == "wide4500", True


def _oracle_logl(prob, P, jax):
    with np.errstate(all="ignore"):
        return np.array([o.jax_loglike_f64(prob, p) for p in P]) if jax else o.loglike_batch(prob, P)


CONFIGS = ["A", "C", "C_jax", "E", "wide", "wide4500"]


@pytest.mark.parametrize("name", CONFIGS)
def test_bad_pixels_logl_chi2_model(name):
    """logL on the host entry, the device entry, the unit-cube entry and the scalar callable; chi2; the model both ways
    of `targonly`: a mix of NaN flux, NaN error and zero error at `bad_positions`, against the oracle."""
    kw, P, extra, multi, wide = _config(name)
    jax = bool(extra)
    rng = np.random.default_rng(77)
    info, (npix, tile, ntiles, n) = _info(kw, **extra)
    assert (ntiles > 1) == multi and ((2 * n + 64 > 4096) == wide)
    idx = bad_positions(info, rng, wide)
    bad = with_bad_pixels(kw, idx, mixed_kinds(idx, rng))
    nan_only = with_bad_pixels(kw, idx, [BAD_KINDS[k % 2] for k in range(idx.size)])   # (err = 0 makes chi2 infinite, as in the reference)
    prob = problem_from_kwargs(bad)
    assert prob.flux.size == npix and (~np.isfinite(prob.flux) | ~(np.abs(prob.err) > 0)).sum() == idx.size
    want = _oracle_logl(prob, P, jax)
    assert np.isfinite(want).all()
    with mcalf_amd.als_fitter(None, **extra, **kw) as fit:
        clean = fit.loglike_batch(P)
        clean_models = [fit.model_batch(P[:2], targonly=t) for t in ((False,) if jax else (False, True))]
    with mcalf_amd.als_fitter(None, **extra, **bad) as fit:
        got = fit.loglike_batch(P)
        _ratio(f"{name} logL", got, want)
        assert np.all(np.abs(got - clean) > 1.0)                                # (the dropped terms are not a rounding matter)
        assert np.array_equal(_device_logl(fit, P), got)
        assert np.array_equal(np.array([fit.lnlhood_worker(p) for p in P[:3]]), got[:3])
        cubes = rng.random((3, fit.ndim))
        theta, ll = fit.loglike_cube_batch(cubes)
        assert np.array_equal(ll, fit.loglike_batch(theta))
        _ratio(f"{name} cube logL", ll, _oracle_logl(prob, theta, jax))
        if not jax:                                                             # (the reference's JAX closure has no chi2 / targonly)
            with np.errstate(all="ignore"):
                want_chi2 = np.array([o.chi2(prob, p) for p in P])
            assert np.all(want_chi2 == np.inf)
            _ratio(f"{name} chi2 (err = 0 among the bad pixels)", fit.chi2_batch(P), want_chi2)
        for k, targ in enumerate((False,) if jax else (False, True)):
            m = fit.model_batch(P[:2], targonly=targ)
            assert np.array_equal(m, clean_models[k])                           # the model does not see the data
            ref = [o.jax_reconstruct_spec_f64(prob, p) if jax else o.reconstruct_spec(prob, p, targonly=targ) for p in P[:2]]
            d = max(np.abs(a - b).max() for a, b in zip(m, ref))
            print(f"{name} model targonly={targ}: max |d| = {d:.3g}")
            assert d < 2e-10
    if not jax:
        prob2 = problem_from_kwargs(nan_only)
        with mcalf_amd.als_fitter(None, **nan_only) as fit:
            chi2 = fit.chi2_batch(P)
            _ratio(f"{name} chi2", chi2, np.array([o.chi2(prob2, p) for p in P]))
            assert np.isfinite(chi2).all() and fit.chi2(P[0]) == chi2[0]
            _ratio(f"{name} logL (NaN flux / NaN error only)", fit.loglike_batch(P), _oracle_logl(prob2, P, False))


@pytest.mark.parametrize("name", ["A", "wide"])
def test_negative_error_is_squared_away(name):
    """The control: err < 0 drops nothing -- logL, chi2 and the model keep the bits of the finite spectrum -- and the
    oracle agrees."""
    kw, P, extra, _, wide = _config(name)
    rng = np.random.default_rng(78)
    info, _ = _info(kw)
    idx = bad_positions(info, rng, wide)
    neg = with_bad_pixels(kw, idx, "err_neg")
    with mcalf_amd.als_fitter(None, **kw) as fit:
        clean = fit.loglike_batch(P), fit.chi2_batch(P), fit.loglike_grad_batch(P)[1]
    with mcalf_amd.als_fitter(None, **neg) as fit:
        got = fit.loglike_batch(P), fit.chi2_batch(P), fit.loglike_grad_batch(P)[1]
    for a, b in zip(got, clean):
        assert np.array_equal(a, b)
    _ratio(f"{name} err < 0 logL", got[0], o.loglike_batch(problem_from_kwargs(neg), P))


@pytest.mark.parametrize("name", ["A", "E", "wide"])
def test_asymmetric_veto_with_bad_pixels(name):
    """hires_fitter.py:296-303 on spectra with bad pixels, thresholds pinned as tests/test_gpu_parity.py pins them: the
    -inf pattern is the oracle's.  err = 0 gives a residual of +inf (counted in both counters) where the flux is above the
    model and -inf (in neither) below; a NaN flux or error gives NaN (in neither).  On config A the bad pixels decide rows
    both ways: spectrum X zeroes the error of 45 pixels above a fair model (the row is vetoed only with them), spectrum Y
    blanks the pixels where an over-absorbed model lies below the data (the row is vetoed only without them)."""
    kw, P, _, _, wide = _config(name)
    rng = np.random.default_rng(79)
    info, (npix, tile, ntiles, n) = _info(kw)
    cdfs = ([5, 0, 0], [50, 30, 10], [3000, 3000, 3000])
    spectra = []
    if name == "A":
        P = workloads.draw_P(kw, 12, np.random.default_rng(21))
        P[0] = [2.0, 13.6, 2.999, 17.5, 13.8, 3.0, 20.0]            # a fair fit (tests/test_gpu_parity.py)
        P[1] = [2.0, 14.5, 3.005, 40.0, 14.5, 3.006, 40.0]          # strong absorption where the data has none
        prob0 = problem_from_kwargs(kw)
        d0 = prob0.flux - o.reconstruct_spec(prob0, P[0])
        above = np.flatnonzero(d0 > 0.01)
        below = np.flatnonzero(d0 < -0.01)
        x_idx = np.concatenate([above[np.linspace(0, above.size - 1, 45).astype(int)], below[::7], [0, npix - 1]])
        spectra.append(("X", with_bad_pixels(kw, np.unique(x_idx), "err_zero")))
        r1 = (prob0.flux - o.reconstruct_spec(prob0, P[1])) / prob0.err
        y_idx = np.flatnonzero(r1 > 3.5)
        spectra.append(("Y", with_bad_pixels(kw, y_idx, ["flux_nan", "err_nan"] * (y_idx.size // 2) + ["flux_nan"] * (y_idx.size % 2))))
    else:
        idx = bad_positions(info, rng, wide)
        kinds = ["err_zero" if k % 2 else m for k, m in enumerate(mixed_kinds(idx, rng))]
        spectra.append(("mixed", with_bad_pixels(kw, idx, kinds)))
    decided = set()
    for tag, bad in spectra:
        prob, prob0 = problem_from_kwargs(bad), problem_from_kwargs(kw)
        for cdf in cdfs:
            with np.errstate(all="ignore"):
                want = np.array([o.lnlhood_worker(prob, p, asymm_thresholds=(cdf[1], cdf[2])) for p in P])
                finite = np.array([o.lnlhood_worker(prob0, p, asymm_thresholds=(cdf[1], cdf[2])) for p in P])
            if np.any(np.isneginf(want) & ~np.isneginf(finite)):
                decided.add("vetoed by bad pixels")
            if np.any(~np.isneginf(want) & np.isneginf(finite)):
                decided.add("spared by bad pixels")
            with mcalf_amd.als_fitter(None, Asymmlike=True, gauss_cdf=cdf, **bad) as fit:
                got = fit.loglike_batch(P)
                assert np.array_equal(_device_logl(fit, P), got)
                assert fit.lnlhood_worker(P[0]) == got[0] and fit.lnlhood_worker(P[1]) == got[1]
                ll, G = fit.loglike_grad_batch(P)
            assert np.array_equal(np.isneginf(got), np.isneginf(want)), (name, tag, cdf, got, want)
            _ratio(f"{name} veto {tag} {cdf}", got, want)
            assert np.array_equal(ll, got) and np.array_equal(np.isnan(G).all(axis=1), np.isneginf(got))
    if name == "A":
        assert decided == {"vetoed by bad pixels", "spared by bad pixels"}, decided


@pytest.mark.parametrize("name,kind", [("A", "err_inf"), ("A", "flux_inf"), ("C_jax", "err_inf"), ("E", "flux_inf"),
                                       ("wide", "err_inf"), ("wide", "flux_inf")])
def test_infinite_error_or_flux_is_minus_inf(name, kind):
    """err = inf: the term is 0 - log(0) = +inf; flux = inf: (inf - m)^2 = +inf.  logL = -inf on every row, as in the
    oracle, and the gradient of such a row is all NaN."""
    kw, P, extra, multi, wide = _config(name)
    info, (npix, tile, ntiles, n) = _info(kw, **extra)
    seam = min(tile, npix - 1)                                   # (a single tile is the spectrum rounded up to eight pixels)
    for idx in ([npix - 1], [0, seam - 1, seam, npix // 2]):
        bad = with_bad_pixels(kw, idx, kind)
        # NaN pixels next to the infinite one do not hide it
        if len(idx) > 1:
            bad = with_bad_pixels(bad, [1, npix - 2], "flux_nan")
        want = _oracle_logl(problem_from_kwargs(bad), P[:2], bool(extra))
        assert np.all(np.isneginf(want))
        with mcalf_amd.als_fitter(None, **extra, **bad) as fit:
            got = fit.loglike_batch(P)
            ll, G = fit.loglike_grad_batch(P)
            assert np.all(np.isneginf(got)) and np.array_equal(ll, got) and np.isnan(G).all()
            assert np.array_equal(_device_logl(fit, P), got) and fit.lnlhood_worker(P[0]) == -np.inf


@pytest.mark.parametrize("name", ["A", "C_jax", "E", "wide"])
def test_the_three_kinds_of_bad_pixel_give_the_same_bits(name):
    """The same index set made bad by NaN flux, by NaN error and by zero error: the same terms are replaced by +0.0 in
    the same fixed order, so logL, chi2 apart (err = 0 leaves an infinite chi2 term, as in the reference), and G are
    bit-identical.  (No flux - model is exactly 0 here: the data carry noise.)"""
    kw, P, extra, _, wide = _config(name)
    rng = np.random.default_rng(80)
    info, _ = _info(kw, **extra)
    idx = bad_positions(info, rng, wide)
    out = []
    for kind in BAD_KINDS:
        with mcalf_amd.als_fitter(None, **extra, **with_bad_pixels(kw, idx, kind)) as fit:
            ll, G = fit.loglike_grad_batch(P)
            out.append((fit.loglike_batch(P), ll.copy(), G.copy()))
    assert np.isfinite(out[0][0]).all() and np.isfinite(out[0][2]).all()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)
    assert np.array_equal(out[0][0], out[0][1])


@pytest.mark.parametrize("name", ["A", "C", "C_jax", "E", "wide"])
def test_gradient_with_bad_pixels(name):
    """loglike_grad_batch on a spectrum with the mixed bad pixels of `bad_positions` against tests/grad_reference.py, on
    the numpy path, the JAX path and a wide-LSF context; its logL is loglike_batch's, bit for bit."""
    kw, P, extra, _, wide = _config(name)
    jax = bool(extra)
    rng = np.random.default_rng(81)
    info, _ = _info(kw, **extra)
    idx = bad_positions(info, rng, wide)
    bad = with_bad_pixels(kw, idx, mixed_kinds(idx, rng))
    prob = problem_from_kwargs(bad)
    with np.errstate(all="ignore"):
        want_ll, ref_G, S = gr.grad_batch(prob, P, jax=jax)
    assert np.isfinite(ref_G).all()
    with mcalf_amd.als_fitter(None, **extra, **bad) as fit:
        ll, G = fit.loglike_grad_batch(P)
        assert np.array_equal(ll, fit.loglike_batch(P))
        l1, g1 = fit.loglike_grad_batch(P[1:2])
        assert l1[0] == ll[1] and np.array_equal(g1[0], G[1])
    _ratio(f"{name} grad logL", ll, want_ll)
    _grad_ratio(f"{name} G", G, ref_G, S)
