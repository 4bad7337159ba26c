"""CPU: the test-side reference of the model Jacobian (tests/model_deriv_reference.py), on the problems of
tests/test_grad_reference.py (`CASES`: both convolution paths, fixed and free resolution / continuum, R <= velstep, bad
pixels): its model against the oracle's, J v against central differences of the oracle's model, J^T (w (d - m)) against
the gradient reference, and the adjoint identity <q, J v> = <J^T q, v>.  The GPU products (tests/test_gpu_model_deriv.py)
are checked against this reference, so this is what anchors it.  Also: the new C entries refuse NULL arguments without
touching a device."""
import numpy as np
import pytest

import grad_reference as gr
import model_deriv_reference as mdr
from cases import problem_from_kwargs
from mcalf_amd import _lib
from oracle import numpy_oracle as o
from test_grad_reference import CASES, _away_from_tap_jumps, _rows

STEP = 1e-4


def _problem(name):
    kw, jax = CASES[name]
    prob = problem_from_kwargs(kw)
    # (the nudge keeps R +- 2e-6 max(1, R) inside one tap count; the central difference below moves R by STEP, so it is
    # asked for that step)
    P = _away_from_tap_jumps(prob, _rows(kw, 3, seed=len(name)), rel=STEP)
    return prob, jax, P


def _oracle_model(prob, p, jax):
    return o.jax_reconstruct_spec_f64(prob, p) if jax else o.reconstruct_spec(prob, p)


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_model_is_the_oracles(name):
    prob, jax, P = _problem(name)
    for p in P:
        m, J = mdr.model_jacobian(prob, p, jax=jax)
        want = _oracle_model(prob, p, jax)
        assert np.all(np.abs(m - want) <= 1e-12), (name, np.abs(m - want).max())
        assert J.shape == (prob.wl.size, prob.ndim) and np.all(J[:, prob.startind] == 0.0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_jvp_matches_central_differences_of_the_oracles_model(name):
    """Step 1e-4 along a tangent scaled per column (1 for R and the continuum, 0.3 / 2e-5 / 3 for logN / z / b);
    max_i |J v - difference| <= 1e-5 max_i S_i.  Worst measured: 1.4e-7 (jax_bad_pixels)."""
    prob, jax, P = _problem(name)
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


@pytest.mark.parametrize("name", sorted(CASES))
def test_vjp_of_the_weighted_residual_is_the_gradient_reference(name):
    prob, jax, P = _problem(name)
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


@pytest.mark.parametrize("name", sorted(CASES))
def test_adjoint_identity(name):
    prob, jax, P = _problem(name)
    rng = np.random.default_rng(len(name) + 2)
    for p in P:
        _, J = mdr.model_jacobian(prob, p, jax=jax)
        v = rng.uniform(-1.0, 1.0, prob.ndim) * mdr.tangent_scales(prob)
        q = rng.normal(0.0, 1.0, prob.wl.size)
        dM, _ = mdr.jvp(J, v)
        G, _ = mdr.vjp(J, q)
        assert abs(np.dot(q, dM) - np.dot(G, v)) <= 1e-13 * np.sum(np.abs(q * dM))


def test_reference_zero_columns_and_weights():
    from test_grad_reference import _kw
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
