"""CPU: the test-side reference of the model Jacobian (tests/model_deriv_reference.py), on the problems of
tests/test_grad_reference.py (`CASES`: both convolution paths, fixed and free resolution / continuum, R <= velstep, bad
pixels): its model against the oracle's, J v against central differences of the oracle's model, J^T (w (d - m)) against
the gradient reference, and the adjoint identity <q, J v> = <J^T q, v>.  The GPU products (tests/test_gpu_model_deriv.py)
are checked against this reference, so this is what anchors it.  Also: the new C entries refuse NULL arguments without
touching a device.

A second problem set (`EDGE`), the one tests/test_gpu_model_deriv_edges.py takes the kernels through, under the same four
bars and in both convolution modes: the 14 seeded random problems of tests/test_gpu_fuzz.py (single lines, triplets,
a ~ 1e-11, logarithmic / jittered / masked grids, two fit ranges, LSFs wider than the spectrum), spectra of one 256-pixel
tile +- 1 pixel, two tiles, 64 and 8 pixels, the three smallest parameter layouts, the wing-only damped line, two damped
rows of config E and the 64-pixel, 49-tap problem.  Where the JAX path's fixed tap grid is wider than the spectrum
(`JAX_REFUSED`) the oracle itself cannot form the model (its where() does not broadcast): exactly that is asserted, and
only that mode of that problem is left out.  Worst over the set: model against the oracle 8.9e-16, J v against central
differences 8.9e-7 max S (fuzz10, numpy path; every other one at most 1.4e-7), VJP against the gradient reference
1.7e-14 S, adjoint identity 7.3e-16 of sum |q dM|."""
import functools

import numpy as np
import pytest

import grad_reference as gr
import model_deriv_reference as mdr
from cases import oracle_synth, problem_from_kwargs, wing_only_problem
from mcalf_amd import _lib, workloads
from oracle import numpy_oracle as o
from test_gpu_fuzz import random_problem
from test_grad_reference import CASES, _away_from_tap_jumps, _kw, _rows

STEP = 1e-4


TILE_NPIX = (255, 256, 257, 512, 513, 64, 8)          # one gradient tile (kGradBlock = 256) -1, +0, +1; two; two + 1; 64; 8
LAYOUTS = (((0, 0), 1), ((1, 1), 0), ((0, 0), 0))     # one filler and no component, one component and no filler, neither
FUZZ_SEEDS = range(14)


def fuzz_problem(seed, nrows=5):
    """(kwargs, rows) of seed `seed` of tests/test_gpu_fuzz.py: test_random_problem_matches_oracle."""
    rng = np.random.default_rng(1000 + seed)
    kw = random_problem(rng)
    return kw, workloads.draw_P(kw, 5, rng)[:nrows]


def tile_problem(npix, nrows=6):
    """CIV doublet on `npix` pixels, free resolution and continuum, a 13-tap LSF at most (tests/test_gpu_grad_edges.py)."""
    kw = _kw(npix=npix, specres=(6.0, 9.0), contval=(0.9, 1.1), velstep=2.0, seed=npix)
    return kw, workloads.draw_P(kw, 6, np.random.default_rng(npix))[:nrows]


def layout_problem(ncomp, nfill, npix, nrows=4):
    kw = _kw(npix=npix, specres=(6.0, 9.0), contval=(0.9, 1.1), ncomp=ncomp, nfill=nfill, velstep=2.0, seed=npix + nfill)
    return kw, workloads.draw_P(kw, 4, np.random.default_rng(3))[:nrows]


def short_problem():
    """64 pixels, one CIV component and no filler, a 49-tap LSF: ~2 KB of per-row workspace."""
    kw = _kw(npix=64, ncomp=(1, 1), nfill=0, velstep=0.43, seed=64)
    assert int(np.ceil(3.0348 * (8.0 / 2.354820) / 0.43)) == 24
    return kw


def _config_E_damped():
    kw, _, seed = workloads.config("E", oracle_synth)
    return kw, workloads.draw_P(kw, 2, np.random.default_rng(seed), damped=2)


EDGE = {f"fuzz{seed}": (lambda seed=seed: fuzz_problem(seed, 2)) for seed in FUZZ_SEEDS}
EDGE.update({f"tile{npix}": (lambda npix=npix: tile_problem(npix, 2)) for npix in TILE_NPIX})
EDGE.update({f"layout{k}": (lambda l=l: layout_problem(l[0], l[1], 257, 2)) for k, l in enumerate(LAYOUTS)})
EDGE["wing_only"] = wing_only_problem
EDGE["config_E_damped"] = _config_E_damped
EDGE["short"] = lambda: (short_problem(), workloads.draw_P(short_problem(), 2, np.random.default_rng(70)))
# the JAX path's fixed tap grid is wider than the spectrum: the oracle's own where() cannot broadcast
JAX_REFUSED = {"fuzz10", "fuzz11", "tile8"}
EDGE_MODES = [(name, jax) for name in EDGE for jax in (False, True)]


def _problem(name, mode=None):
    """(problem, jax, rows) of a `CASES` entry (mode None) or of an `EDGE` entry in the given mode; None where the oracle
    refuses that mode."""
    if mode is not None:
        return _edge_problem(name, mode)
    kw, jax = CASES[name]
    prob = problem_from_kwargs(kw)
    # (the nudge keeps R +- 2e-6 max(1, R) inside one tap count; the central difference below moves R by STEP, so it is
    # asked for that step)
    P = _away_from_tap_jumps(prob, _rows(kw, 3, seed=len(name)), rel=STEP)
    return prob, jax, P


def _oracle_model(prob, p, jax):
    return o.jax_reconstruct_spec_f64(prob, p) if jax else o.reconstruct_spec(prob, p)


@functools.lru_cache(maxsize=None)
def _edge_problem(name, jax):
    """(problem, mode, rows) of one `EDGE` entry, or None where the oracle refuses the JAX path: a ValueError of numpy's
    broadcasting on exactly the `JAX_REFUSED` problems (anything else it raises is raised here).  Built once; the tests
    leave the rows as they are."""
    kw, P = EDGE[name]()
    prob = problem_from_kwargs(kw)
    if jax:
        try:
            _oracle_model(prob, P[0], True)
            refused = False
        except ValueError as exc:
            assert "operands could not be broadcast" in str(exc), exc
            refused = True
        assert refused == (name in JAX_REFUSED), (name, refused)
        assert refused == (2 * o.jax_half_size(prob) + 1 > prob.wl.size)
        if refused:
            return None
    return prob, jax, _away_from_tap_jumps(prob, P.copy(), rel=STEP)


# every problem of the four tests below: `CASES` under their own names (each names its mode), then `EDGE` in both modes
PROBLEMS = [(name, None) for name in sorted(CASES)] + EDGE_MODES
IDS = sorted(CASES) + [f"{name}-{'jax' if jax else 'numpy'}" for name, jax in EDGE_MODES]


@pytest.mark.parametrize("name,mode", PROBLEMS, ids=IDS)
def test_reference_model_is_the_oracles(name, mode):
    if (case := _problem(name, mode)) is None:
        return
    prob, jax, P = case
    for p in P:
        m, J = mdr.model_jacobian(prob, p, jax=jax)
        want = _oracle_model(prob, p, jax)
        assert np.all(np.abs(m - want) <= 1e-12), (name, np.abs(m - want).max())
        assert J.shape == (prob.wl.size, prob.ndim) and np.all(J[:, prob.startind] == 0.0)


@pytest.mark.parametrize("name,mode", PROBLEMS, ids=IDS)
def test_jvp_matches_central_differences_of_the_oracles_model(name, mode):
    """Step 1e-4 along a tangent scaled per column (1 for R and the continuum, 0.3 / 2e-5 / 3 for logN / z / b);
    max_i |J v - difference| <= 1e-5 max_i S_i.  Worst measured: 1.4e-7 (jax_bad_pixels) over `CASES`, 8.9e-7 (fuzz10) over `EDGE`."""
    if (case := _problem(name, mode)) is None:
        return
    prob, jax, P = case
    rng = np.random.default_rng(len(name) + 1)
    for p in P:
        v = rng.uniform(-1.0, 1.0, prob.ndim) * mdr.tangent_scales(prob)
        v[prob.startind] = 0.0                                       # (a step in ncomp is not a derivative)
        _, J = mdr.model_jacobian(prob, p, jax=jax)
        dM, S = mdr.jvp(J, v)
        cd = (_oracle_model(prob, p + STEP * v, jax) - _oracle_model(prob, p - STEP * v, jax)) / (2 * STEP)
        err = np.abs(dM - cd).max()
        print(f"{name}: max|J v - cd| / max S = {err / S.max():.2e}")
        assert err <= 1e-5 * S.max(), (name, err, S.max())


@pytest.mark.parametrize("name,mode", PROBLEMS, ids=IDS)
def test_vjp_of_the_weighted_residual_is_the_gradient_reference(name, mode):
    if (case := _problem(name, mode)) is None:
        return
    prob, jax, P = case
    for p in P:
        with np.errstate(divide="ignore", invalid="ignore"):
            _, want, S = gr.grad_row(prob, p, jax=jax)
            m, J = mdr.model_jacobian(prob, p, jax=jax)
            is2 = 1.0 / prob.err ** 2
            term = is2 * (prob.flux - m) ** 2 - np.log(is2)
            q = np.where(np.isnan(term), 0.0, is2 * (prob.flux - m))
        G, S2 = mdr.vjp(J, q)
        assert np.all(np.abs(G - want) <= 1e-12 * S), (name, np.abs(G - want) / np.maximum(S, 1e-300))
        assert np.allclose(S2, S, rtol=1e-9, atol=0.0)


@pytest.mark.parametrize("name,mode", PROBLEMS, ids=IDS)
def test_adjoint_identity(name, mode):
    if (case := _problem(name, mode)) is None:
        return
    prob, jax, P = case
    rng = np.random.default_rng(len(name) + 2)
    for p in P:
        _, J = mdr.model_jacobian(prob, p, jax=jax)
        v = rng.uniform(-1.0, 1.0, prob.ndim) * mdr.tangent_scales(prob)
        q = rng.normal(0.0, 1.0, prob.wl.size)
        dM, _ = mdr.jvp(J, v)
        G, _ = mdr.vjp(J, q)
        assert abs(np.dot(q, dM) - np.dot(G, v)) <= 1e-13 * np.sum(np.abs(q * dM))


def test_reference_zero_columns_and_weights():
    kw = _kw(ncomp=(0, 3), specres=(6.0, 9.0))
    prob = problem_from_kwargs(kw)
    p = _rows(kw, 1, seed=3)[0]
    for v, jax, active in ((1.7, False, 1), (1.7, True, 1), (-0.5, False, 0), (-0.5, True, 0)):
        p[prob.startind] = v
        _, J = mdr.model_jacobian(prob, p, jax=jax)
        assert np.all(J[:, prob.startind: prob.endind][:, 1 + 3 * active:] == 0.0) and np.all(J[:, prob.startind] == 0.0)
        assert np.all(np.abs(J[:, prob.endind:]).max(axis=0) > 0.0)          # the filler is always active
    prob = problem_from_kwargs(CASES["numpy_bad_pixels"][0])
    W = mdr.kept_weights(prob)
    assert (W == 0.0).sum() == 49 and np.all(np.isfinite(W))


def test_new_entries_refuse_null_arguments_without_a_gpu():
    lib = _lib.load()
    assert b"abi 9" in lib.mcalf_version()
    assert lib.mcalf_model_jvp_batch(None, None, None, 4, None) == -1
    assert lib.mcalf_model_vjp_batch(None, None, None, 4, None) == -1
    assert lib.mcalf_model_jvp_batch_device(None, None, None, 4, None, None) == -1
    assert lib.mcalf_model_vjp_batch_device(None, None, None, 4, None, None) == -1
    assert lib.mcalf_model_jvp_batch(None, None, None, -1, None) == -1
    assert b"NULL" in lib.mcalf_last_error(None)
