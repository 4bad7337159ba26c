"""CPU: the test-side reference of logL's Hessian (tests/hess_reference.py: Richardson-extrapolated central differences of the
gradient reference) on every problem tests/test_gpu_hvp.py takes the kernels through (`CASES`), and what anchors it:

  * its own error on H v in units of S_k = sum_j |v_j| sum_i W_i |J_ik| |J_ij| -- the larger of the Richardson estimate and
    half the asymmetry of the dense H, contracted with |v| -- for every tangent the GPU tests use.  Bar 1e-6: a case beyond
    it would need a better reference, not a wider GPU bar.  Worst measured: REFERENCE_ERROR below (3.6e-7, one filler and no
    component; every other case at most 4.6e-8);
  * H against -J^T W J + sum_i W_i r_i d2 m_i / dtheta2 with J from tests/model_deriv_reference.py and the curvature term
    from central differences of that Jacobian, same bar (worst measured 2.5e-8, config A);
  * rows and columns that are 0 by definition.

REL_BAR, the relative part of the GPU bar |d HV_k| <= REL_BAR S_k + floor, is ten times the worst reference error and not
below the project's derivative bar of 1e-7.

Also without a GPU: the two new C entries refuse NULL and negative arguments, and the version string still says abi 9."""
import functools

import numpy as np
import pytest

import hess_reference as hr
import model_deriv_reference as mdr
from cases import problem_from_kwargs, wing_only_problem
from mcalf_amd import _lib, workloads
from test_gpu_fuzz import LINESETS
from test_grad_reference import _kw, bad_pixel_problem
from test_model_deriv_reference import layout_problem, tile_problem

# Worst reference error over CASES and their tangents (test_reference_error prints each case's; pytest -s), and the bar it sets.
REFERENCE_ERROR = 3.6e-7      # filler_only: the R-R entry of a logN = 12 filler (curvature thirty times the Fisher scale)
REL_BAR = 3.6e-6

TILE_NPIX = (64, 255, 256, 257, 513)


def _draw(kw, n, seed):
    return workloads.draw_P(kw, n, np.random.default_rng(seed))


def _config_A():
    kw, _, seed = workloads.config("A")
    return kw, _draw(kw, 2, seed)


def _ncomp():
    kw = _kw(ncomp=(0, 3), specres=(6.0, 9.0))
    P = _draw(kw, 4, 11)
    P[:, 1] = [2.7, -0.5, 0.3, 1.2]
    return kw, P


def triplet_problem(npix=700, step=9.0, z0=1.2):
    """The MgII / MgI triplet of tests/test_gpu_fuzz.py (three lines per component) on a logarithmic grid that holds all
    three, two components and one filler, fixed resolution and a free continuum."""
    lines = LINESETS["triplet"]
    rng = np.random.default_rng(27)
    wl = 2824.0 * (1 + z0) * np.exp((np.arange(npix) - npix / 2) * step / 2.9979245e5)
    kw = dict(fitrange=[[wl[0] - 1e-3, wl[-1] + 1e-3]], fitlines=["L0", "L1", "L2"], linepars=lines, ncomp=[2, 2], nfill=1,
              specres=[20.0], contval=[0.9, 1.1], Nrange=[11.5, 13.5], brange=[6.0, 40.0],
              zrange=[z0 - 150 / 2.9979245e5 * (1 + z0), z0 + 150 / 2.9979245e5 * (1 + z0)], velstep=float(step),
              spectrum=(wl, 1 + rng.normal(0, 0.03, npix), rng.uniform(0.01, 0.05, npix)))
    return kw, _draw(kw, 2, 28)


def wrapping_problem():
    """249 taps over 151 pixels on the numpy path: the periodic convolution wraps round the spectrum."""
    kw = _kw(npix=151, ncomp=(1, 1), nfill=0, velstep=0.0834, seed=151)
    assert 2 * int(np.ceil(3.0348 * (8.0 / 2.354820) / 0.0834)) + 1 == 249
    return kw, _draw(kw, 2, 152)


def wide_problem():
    """A free resolution whose LSF has 2813 .. 4219 taps on 3000 pixels: wider than a 4096-pixel workgroup tile once its
    halo is counted (2 n_cap + 64 > 4096), so the context takes the likelihood's wide path."""
    kw = _kw(npix=3000, ncomp=(1, 1), nfill=0, specres=(6.0, 9.0), velstep=0.0055, seed=333)
    assert 2 * int(np.ceil(3.0348 * (9.0 / 2.354820) / 0.0055)) + 64 > 4096
    return kw, _draw(kw, 2, 334)


def _wing_only():
    kw, P = wing_only_problem()
    return kw, P


# name -> (builder of (kwargs, parameter vectors), JAX path?)
CASES = {
    "A_numpy": (_config_A, False),
    "A_jax": (_config_A, True),
    "civ_fixed": (lambda: (_kw(), _draw(_kw(), 2, 6)), False),
    "civ_free_R": (lambda: (_kw(specres=(6.0, 9.0)), _draw(_kw(specres=(6.0, 9.0)), 2, 6)), False),
    "civ_free_cont": (lambda: (_kw(contval=(0.9, 1.1)), _draw(_kw(contval=(0.9, 1.1)), 2, 6)), False),
    "civ_free_R_cont": (lambda: (_kw(specres=(6.0, 9.0), contval=(0.9, 1.1)), _draw(_kw(specres=(6.0, 9.0), contval=(0.9, 1.1)), 2, 6)), False),
    "R_le_velstep_fixed": (lambda: (_kw(velstep=10.0), _draw(_kw(velstep=10.0), 2, 5)), False),
    "R_le_velstep_free": (lambda: (_kw(specres=(6.0, 9.0), contval=(0.9, 1.1), velstep=10.0),
                                   _draw(_kw(specres=(6.0, 9.0), contval=(0.9, 1.1), velstep=10.0), 2, 5)), False),
    "ncomp_numpy": (_ncomp, False),
    "ncomp_jax": (_ncomp, True),
    "triplet": (triplet_problem, False),
    "filler_only": (lambda: layout_problem((0, 0), 1, 257, 2), False),
    "lsf_wraps": (wrapping_problem, False),
    "wide_lsf": (wide_problem, False),
    "bad_pixels_numpy": (lambda: (bad_pixel_problem(specres=(6.0, 9.0), contval=(0.9, 1.1)),
                                  _draw(bad_pixel_problem(specres=(6.0, 9.0), contval=(0.9, 1.1)), 2, 51)), False),
    "bad_pixels_jax": (lambda: (bad_pixel_problem(specres=(6.0, 9.0), contval=(0.9, 1.1)),
                                _draw(bad_pixel_problem(specres=(6.0, 9.0), contval=(0.9, 1.1)), 2, 51)), True),
    "wing_only": (_wing_only, False),
}
CASES.update({f"tile{npix}": ((lambda npix=npix: tile_problem(npix, 2)), False) for npix in TILE_NPIX})


@functools.lru_cache(maxsize=None)
def reference(name):
    """(kwargs, problem, jax, thetas, [(H, E, A)] per theta) of one case, built once; the tests leave it as it is."""
    build, jax = CASES[name]
    kw, thetas = build()
    prob = problem_from_kwargs(kw)
    dense = []
    for p in thetas:
        H, E = hr.hessian(prob, p, jax)
        A, _ = hr.fisher_abs(prob, p, jax)
        for a in (H, E, A):
            a.setflags(write=False)
        dense.append((H, E, A))
    thetas.setflags(write=False)
    return kw, prob, jax, thetas, dense


def tangent_rows(name):
    """(P, V, index of each row's theta) of a case: per theta one random tangent scaled per column, with NaN in the ncomp
    slot (never read), then -- for the first two thetas -- one tangent with a single non-zero entry per live parameter class."""
    _, prob, jax, thetas, _ = reference(name)
    rng = np.random.default_rng(len(name))
    P, V, which = [], [], []
    for t, p in enumerate(thetas):
        v = rng.uniform(-1.0, 1.0, prob.ndim) * mdr.tangent_scales(prob)
        v[prob.startind] = np.nan
        for u in [v] + (hr.class_tangents(prob, p, jax) if t < 2 else []):
            P.append(p)
            V.append(u)
            which.append(t)
    return np.array(P), np.array(V), which


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_error(name):
    _, prob, jax, thetas, dense = reference(name)
    P, V, which = tangent_rows(name)
    assert 4 <= len(P) <= 16
    worst = 0.0
    for v, t in zip(V, which):
        H, E, A = dense[t]
        worst = max(worst, hr.reference_error(H, E, A, v))
    print(f"{name}: reference error = {worst:.2e} S over {len(P)} tangents at {len(thetas)} thetas")
    assert worst <= 1e-6, (name, worst)
    assert worst <= REFERENCE_ERROR, (name, worst)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_is_gauss_newton_plus_curvature(name):
    _, prob, jax, thetas, dense = reference(name)
    P, V, which = tangent_rows(name)
    other = [hr.gauss_newton_plus_curvature(prob, p, jax) for p in thetas]
    worst = 0.0
    for v, t in zip(V, which):
        H, _, A = dense[t]
        want, S = hr.hvp(other[t], A, v)
        got, _ = hr.hvp(H, A, v)
        big = S >= hr.SMALL * S.max()
        worst = max(worst, float(np.max(np.abs(got - want)[big] / S[big])))
    print(f"{name}: |H v - (-J^T W J + curvature) v| = {worst:.2e} S")
    assert worst <= 1e-6, (name, worst)


def test_zero_rows_and_columns():
    for name, active in (("ncomp_numpy", (2, 0, 0, 1)), ("ncomp_jax", (2, 0, 0, 1))):
        _, prob, jax, thetas, dense = reference(name)
        s = prob.startind
        for p, (H, _, A), nc in zip(thetas, dense, active):
            dead = [s] + list(range(s + 1 + 3 * nc, prob.endind))
            assert np.all(H[dead] == 0.0) and np.all(H[:, dead] == 0.0) and np.all(A[dead] == 0.0)
            live = hr.live_columns(prob, p, jax)
            assert sorted(live + dead) == list(range(prob.ndim))
            assert np.all(np.diag(A)[live] > 0.0)
    _, prob, jax, thetas, dense = reference("R_le_velstep_free")
    for H, _, A in dense:
        assert np.all(H[0] == 0.0) and np.all(H[:, 0] == 0.0) and A[0, 0] == 0.0         # R does nothing: no convolution
    _, prob, _, _, _ = reference("bad_pixels_numpy")
    assert (mdr.kept_weights(prob) == 0.0).sum() == 49


def test_new_entries_refuse_null_arguments_without_a_gpu():
    lib = _lib.load()
    assert b"abi 9" in lib.mcalf_version()
    assert lib.mcalf_loglike_hvp_batch(None, None, None, 4, None) == -1
    assert b"NULL" in lib.mcalf_last_error(None)
    assert lib.mcalf_loglike_hvp_batch_device(None, None, None, 4, None, None) == -1
    assert b"NULL" in lib.mcalf_last_error(None)
    assert lib.mcalf_loglike_hvp_batch(None, None, None, -1, None) == -1
    assert lib.mcalf_loglike_hvp_batch_device(None, None, None, -1, None, None) == -1
    assert b"NULL" in lib.mcalf_last_error(None)
