"""GPU: the model Jacobian's products with a vector -- mcalf_model_jvp_batch[_device], mcalf_model_vjp_batch[_device] and
the Python entries built on them (fisher_matvec_batch, model_jacobian) -- against the float64 dense Jacobian of
tests/model_deriv_reference.py (itself anchored on the oracle in tests/test_model_deriv_reference.py); the columns and
rows fixed by definition; the adjoint identity on the device; bit equality across batch positions, entries, device
counts, workspace passes and streams.

Bars, per row:
    JVP  |d dM_i| <= 1e-7 S_i + FLOOR_REL max_i S_i,   S_i = sum_k |v_k J_ik|
    VJP  |d G_k|  <= 1e-7 S_k + 1e-9,                  S_k = sum_i |q_i J_ik|     (the gradient's own bar)
The relative part is the gradient's.  The JVP's floor covers the pixels where the terms of ONE column cancel inside the
convolution (L(F dtau/dz) changes sign across a line, so |J_ik| can be far below the taps' sum of |F dtau|, which is what
rounding scales with).  It is ten times the worst |d dM_i| / max_i S_i measured on an MI355X on the pixels with
S_i < 1e-6 max_i S_i over every case of this file: 1.33e-14 (fractional ncomp, numpy path; every other case at most
7.3e-15: DESIGN 3.7 lists them), so FLOOR_REL = 1.33e-13, four orders below the cap of 1e-9.  With it the worst error / bar of a JVP
case is 0.10 (fractional ncomp), of a VJP case 0.012 (wide LSF).  Every case prints its worst error / bar and its worst
small-S error (pytest -s), which is how the floor is measured again after a change of the kernels."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import grad_reference as gr
import mcalf_amd
import model_deriv_reference as mdr
from mcalf_amd import _lib, workloads
from cases import oracle_synth, problem_from_kwargs, wing_only_problem
from test_grad_reference import bad_pixel_problem

pytestmark = pytest.mark.gpu

CIV = [(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8)]
FLOOR_REL = 1.33e-13


def _civ(npix=600, specres=(8.0,), contval=(1.0,), ncomp=(1, 3), nfill=1, velstep=None, seed=0):
    rng = np.random.default_rng(seed)
    wl = np.linspace(6180.0, 6220.0, npix + 2)[1:-1]
    kw = dict(fitrange=[[6180.0, 6220.0]], fitlines=["CIV 1548", "CIV 1550"], linepars=CIV, ncomp=list(ncomp), nfill=nfill,
              specres=list(specres), contval=list(contval), Nrange=[12.5, 14.5], brange=[8.0, 40.0], zrange=[2.995, 3.012],
              spectrum=(wl, 1 + rng.normal(0, 0.03, npix), rng.uniform(0.01, 0.05, npix)))
    if velstep is not None:
        kw["velstep"] = float(velstep)
    return kw


def _tangents(prob, n, seed):
    """Random tangents scaled per column; NaN in the ncomp slot, which the entries must never read."""
    V = np.random.default_rng(seed).uniform(-1.0, 1.0, (n, prob.ndim)) * mdr.tangent_scales(prob)
    V[:, prob.startind] = np.nan
    return V


def _jacobians(prob, P, jax):
    return [mdr.model_jacobian(prob, p, jax=jax)[1] for p in P]


def _jvp_compare(dM, Js, V, what):
    """Worst error / bar of a batch of JVP rows; prints it and the worst error on the small-S pixels (the floor's measure)."""
    worst, small = 0.0, 0.0
    for r, J in enumerate(Js):
        want, S = mdr.jvp(J, np.where(np.isnan(V[r]), 0.0, V[r]))
        d = np.abs(dM[r] - want)
        assert np.isfinite(dM[r]).all(), (what, r)
        if S.max() == 0.0:                             # J v is 0 by definition (nothing active, or F = 0 on every pixel): exactly 0
            assert np.all(dM[r] == 0.0), (what, r)     # (0 / 0 below would hide the row from np.max)
            continue
        worst = max(worst, float(np.max(d / (1e-7 * S + FLOOR_REL * S.max()))))
        lo = S < 1e-6 * S.max()
        if lo.any():
            small = max(small, float(d[lo].max() / S.max()))
    print(f"JVP {what}: worst error / bar = {worst:.3g}, worst small-S error = {small:.3g} max S")
    return worst


def _vjp_compare(G, Js, Q, what):
    worst = 0.0
    for r, J in enumerate(Js):
        want, S = mdr.vjp(J, Q[r])
        worst = max(worst, float(np.max(np.abs(G[r] - want) / (1e-7 * S + 1e-9))))
        assert np.all(G[r][np.all(J == 0.0, axis=0)] == 0.0), (what, r)        # columns that are 0 by definition: exactly 0
    print(f"VJP {what}: worst error / bar = {worst:.3g}")
    return worst


def _check(kw, P, jax=False, what="", seed=0):
    """JVP with random tangents and VJP with random cotangents of the rows P against the reference."""
    prob = problem_from_kwargs(kw)
    V = _tangents(prob, P.shape[0], seed)
    Q = np.random.default_rng(seed + 1).normal(0.0, 1.0, (P.shape[0], prob.wl.size))
    with mcalf_amd.als_fitter(None, conv_mode="jax" if jax else "numpy", **kw) as fit:
        dM = fit.model_jvp_batch(P, V)
        G = fit.model_vjp_batch(P, Q)
    assert dM.shape == (P.shape[0], prob.wl.size) and G.shape == P.shape
    Js = _jacobians(prob, P, jax)
    wj = _jvp_compare(dM, Js, V, what)
    wv = _vjp_compare(G, Js, Q, what)
    assert wj <= 1.0 and wv <= 1.0, (what, wj, wv)
    assert np.all(G[:, prob.startind] == 0.0)
    return dM, G


def test_config_A_fixture_problem():
    kw, _, seed = workloads.config("A")
    _check(kw, workloads.draw_P(kw, 8, np.random.default_rng(seed)), what="A")


def test_config_C_64_rows():
    kw, _, seed = workloads.config("C", oracle_synth)
    _check(kw, workloads.draw_P(kw, 64, np.random.default_rng(seed)), what="C")


def test_config_E_64_rows():
    kw, _, seed = workloads.config("E", oracle_synth)
    _check(kw, workloads.draw_P(kw, 64, np.random.default_rng(seed), damped=2), what="E")


def test_jax_path():
    kw, _, seed = workloads.config("C", oracle_synth)
    _check(kw, workloads.draw_P(kw, 32, np.random.default_rng(seed + 2)), jax=True, what="C jax")
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1))
    _check(kw, workloads.draw_P(kw, 8, np.random.default_rng(4)), jax=True, what="CIV free R, cont jax")


@pytest.mark.parametrize("specres,contval", [((8.0,), (1.0,)), ((6.0, 9.0), (1.0,)), ((8.0,), (0.9, 1.1)), ((6.0, 9.0), (0.9, 1.1))])
def test_free_and_fixed_resolution_and_continuum(specres, contval):
    kw = _civ(specres=specres, contval=contval)
    _check(kw, workloads.draw_P(kw, 8, np.random.default_rng(6)), what=f"CIV R {specres} cont {contval}")


def test_R_at_or_below_velstep():
    kw = _civ(specres=(8.0,), velstep=10.0)
    _check(kw, workloads.draw_P(kw, 6, np.random.default_rng(5)), what="R <= velstep")
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1), velstep=10.0)          # a free R that does nothing: its column is 0
    dM, G = _check(kw, workloads.draw_P(kw, 6, np.random.default_rng(5)), what="free R <= velstep")
    assert np.all(G[:, 0] == 0.0)


def test_wide_lsf():
    kw = _civ(npix=333, specres=(6.0, 9.0), contval=(0.9, 1.1), nfill=2, velstep=0.0031, seed=333)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert 2 * fit.info.n_cap + 64 > 4096
    _check(kw, workloads.draw_P(kw, 4, np.random.default_rng(9)), what="wide LSF")


def test_fractional_and_negative_ncomp():
    kw = _civ(ncomp=(0, 3), specres=(6.0, 9.0))
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 8, np.random.default_rng(11))
    s = prob.startind
    P[:, s] = [2.7, 1.2, -0.5, -1.5, 0.3, 3.0, 2.0, 0.999]
    for jax in (False, True):
        dM, G = _check(kw, P, jax=jax, what=f"ncomp jax={jax}")
        with mcalf_amd.als_fitter(None, conv_mode="jax" if jax else "numpy", **kw) as fit:
            V = _tangents(prob, 8, 0)
            for r, v in enumerate(P[:, s]):
                active = int(min(max(np.floor(v) if jax else np.trunc(v), 0), 3))
                assert np.all(G[r, s + 1 + 3 * active: s + 1 + 9] == 0.0)
                V[r, s + 1 + 3 * active: s + 1 + 9] = np.nan            # the tangent of an inactive component is never read
            assert np.array_equal(fit.model_jvp_batch(P, V), dM)


def test_wing_only_damped_line():
    kw, P = wing_only_problem()
    _check(kw, P, what="wing only")


def test_rows_beyond_the_tap_cap_are_nan_and_nonfinite_cotangents_propagate():
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1))
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 6, np.random.default_rng(31))
    V = _tangents(prob, 6, 2)
    Q = np.random.default_rng(3).normal(0.0, 1.0, (6, prob.wl.size))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        n_cap, velstep = fit.info.n_cap, fit.velstep
        assert np.ceil(3.0348 * (12.0 / 2.354820) / velstep) > n_cap
        own_dM, own_G = fit.model_jvp_batch(P, V), fit.model_vjp_batch(P, Q)
        B = P.copy()
        B[1, 0] = 12.0                                                   # more taps than the context provisions
        B[4, 0] = 1e300
        dM, G = fit.model_jvp_batch(B, V), fit.model_vjp_batch(B, Q)
        for bad in (1, 4):
            assert np.all(np.isnan(dM[bad])) and np.all(np.isnan(G[bad]))
        keep = [0, 2, 3, 5]
        assert np.array_equal(dM[keep], own_dM[keep]) and np.array_equal(G[keep], own_G[keep])
        assert np.isfinite(own_dM).all() and np.isfinite(own_G).all()
        Qn = Q.copy()
        Qn[0, 300] = np.nan                                              # Q is used as given
        Gn = fit.model_vjp_batch(P, Qn)
        assert np.all(np.isnan(Gn[0, :2])) and np.array_equal(Gn[1:], own_G[1:])


def test_vjp_of_the_weighted_residual_is_the_gradient():
    """Q = w (d - m) from model_batch, 0 on the pixels nansum drops: the VJP against loglike_grad_batch's G, within the
    gradient's own bar (S_k from the gradient reference), on 256 rows of config C."""
    kw, _, seed = workloads.config("C", oracle_synth)
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 256, np.random.default_rng(seed + 6))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        ll, G = fit.loglike_grad_batch(P)
        m = fit.model_batch(P)
        with np.errstate(divide="ignore", invalid="ignore"):
            is2 = 1.0 / prob.err ** 2
            term = is2 * (prob.flux - m) ** 2 - np.log(is2)
            Q = np.where(np.isnan(term), 0.0, is2 * (prob.flux - m))
        Gv = fit.model_vjp_batch(P, Q)
    assert np.isfinite(ll).all()
    _, _, S = gr.grad_batch(prob, P)
    ratio = np.abs(Gv - G) / (1e-7 * S + 1e-9)
    print(f"VJP of w (d - m) against the gradient: worst error / bar = {ratio.max():.3g}")
    assert np.all(ratio <= 1.0)


@pytest.mark.parametrize("jax", [False, True])
def test_adjoint_identity_on_the_device(jax):
    """<Q, jvp(P, V)> against <vjp(P, Q), V>: the two bars contracted with |Q| and |V|."""
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1), ncomp=(3, 3))
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 16, np.random.default_rng(41))
    V = np.nan_to_num(_tangents(prob, 16, 42))
    Q = np.random.default_rng(43).normal(0.0, 1.0, (16, prob.wl.size))
    with mcalf_amd.als_fitter(None, conv_mode="jax" if jax else "numpy", **kw) as fit:
        dM, G = fit.model_jvp_batch(P, V), fit.model_vjp_batch(P, Q)
    worst = 0.0
    for r, J in enumerate(_jacobians(prob, P, jax)):
        _, Si = mdr.jvp(J, V[r])
        _, Sk = mdr.vjp(J, Q[r])
        bar = np.sum(np.abs(Q[r]) * (1e-7 * Si + FLOOR_REL * Si.max())) + np.sum(np.abs(V[r]) * (1e-7 * Sk + 1e-9))
        worst = max(worst, abs(np.dot(Q[r], dM[r]) - np.dot(G[r], V[r])) / bar)
    print(f"adjoint identity (jax={jax}): worst |<Q, J v> - <J^T Q, v>| / bar = {worst:.3g}")
    assert worst <= 1.0


def test_fisher_matvec_with_bad_pixels():
    """J^T W J v from the reference's dense J on the 600-pixel problem with 49 bad pixels of the three kinds.  Bar, per
    column: the JVP's bar carried through J^T W, plus the VJP's own for the cotangent W J v."""
    for jax in (False, True):
        kw = bad_pixel_problem(specres=(6.0, 9.0), contval=(0.9, 1.1))
        prob = problem_from_kwargs(kw)
        W = mdr.kept_weights(prob)
        assert (W == 0.0).sum() == 49
        P = workloads.draw_P(kw, 8, np.random.default_rng(51))
        V = np.nan_to_num(_tangents(prob, 8, 52))
        with mcalf_amd.als_fitter(None, conv_mode="jax" if jax else "numpy", **kw) as fit:
            FV = fit.fisher_matvec_batch(P, V)
        worst = 0.0
        for r, J in enumerate(_jacobians(prob, P, jax)):
            dM, Si = mdr.jvp(J, V[r])
            want, Sk = mdr.vjp(J, W * dM)
            bar = np.abs(J).T @ (W * (1e-7 * Si + FLOOR_REL * Si.max())) + 1e-7 * Sk + 1e-9
            worst = max(worst, float(np.max(np.abs(FV[r] - want) / bar)))
            assert FV[r, prob.startind] == 0.0
        print(f"Fisher product (jax={jax}): worst error / bar = {worst:.3g}")
        assert worst <= 1.0


def test_model_jacobian():
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1), ncomp=(1, 3))
    prob = problem_from_kwargs(kw)
    p = workloads.draw_P(kw, 1, np.random.default_rng(61))[0]
    p[prob.startind] = 2.0
    with mcalf_amd.als_fitter(None, **kw) as fit:
        J = fit.model_jacobian(p)
    _, want = mdr.model_jacobian(prob, p)
    assert J.shape == want.shape == (prob.wl.size, prob.ndim)
    colmax = np.abs(want).max(axis=0)
    assert np.all(np.abs(J - want) <= 1e-7 * np.abs(want) + FLOOR_REL * colmax)
    assert np.all(J[:, colmax == 0.0] == 0.0) and (colmax == 0.0).sum() == 4       # ncomp and the third component


def _device_call(fit, name, dP, dX, n, dY, stream):
    return getattr(fit._lib, name)(fit._ctx, dP.data_ptr(), dX.data_ptr(), n, dY.data_ptr(), C.c_void_p(stream))


def test_bit_equality():
    kw, _, seed = workloads.config("C", oracle_synth)
    prob = problem_from_kwargs(kw)
    n = 4096
    P = workloads.draw_P(kw, n, np.random.default_rng(seed + 3))
    V = _tangents(prob, n, 71)
    Q = np.random.default_rng(72).normal(0.0, 1.0, (n, prob.wl.size))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        dM, G = fit.model_jvp_batch(P, V), fit.model_vjp_batch(P, Q)
        assert np.array_equal(fit.model_jvp_batch(P, V), dM) and np.array_equal(fit.model_vjp_batch(P, Q), G)
        for r in (0, 1777, 4095):                                      # a row alone
            assert np.array_equal(fit.model_jvp_batch(P[r:r + 1], V[r:r + 1])[0], dM[r])
            assert np.array_equal(fit.model_vjp_batch(P[r:r + 1], Q[r:r + 1])[0], G[r])
        # the device entries, on torch's current stream and on a side stream; the second call allocates nothing
        dP, dV, dQ = (torch.from_numpy(a).cuda() for a in (P, V, Q))
        ddM = torch.empty(Q.shape, dtype=torch.float64, device="cuda")
        dG = torch.empty(P.shape, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        for k in range(2):
            stream = side if k else torch.cuda.current_stream()
            ddM.fill_(-7.0)
            dG.fill_(-7.0)
            stream.wait_stream(torch.cuda.current_stream())
            assert _device_call(fit, "mcalf_model_jvp_batch_device", dP, dV, n, ddM, stream.cuda_stream) == 0
            assert _device_call(fit, "mcalf_model_vjp_batch_device", dP, dQ, n, dG, stream.cuda_stream) == 0
            stream.synchronize()
            if k:
                assert stream.cuda_stream != torch.cuda.default_stream().cuda_stream
            assert np.array_equal(ddM.cpu().numpy(), dM) and np.array_equal(dG.cpu().numpy(), G)
        assert fit._lib.mcalf_model_jvp_batch_device(fit._ctx, None, None, 0, None, None) == 0
        assert fit._lib.mcalf_model_vjp_batch(fit._ctx, None, None, 0, None) == 0
        assert fit._lib.mcalf_model_vjp_batch(fit._ctx, P.ctypes.data, None, 4, G.ctypes.data) == _lib.MCALF_ERR_INVALID
        with pytest.raises(ValueError):
            fit.model_jvp_batch(P[:4], V[:3])
        with pytest.raises(ValueError):
            fit.model_vjp_batch(P[:4], V[:4])
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as fit:
        assert np.array_equal(fit.model_jvp_batch(P[:1000], V[:1000]), dM[:1000])
        assert np.array_equal(fit.model_vjp_batch(P[:1000], Q[:1000]), G[:1000])
        rc = _device_call(fit, "mcalf_model_jvp_batch_device", dP, dV, 8, ddM, torch.cuda.current_stream().cuda_stream)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in fit._lib.mcalf_last_error(fit._ctx)


def test_workspace_passes():
    """2048 rows of config E need two passes over the per-row workspaces: the same bits as the two halves."""
    kw, _, seed = workloads.config("E", oracle_synth)
    prob = problem_from_kwargs(kw)
    n = 2048
    # the pass budget as the library's source states it; F and q / T alone (16 bytes per row and pixel) must exceed it,
    # or the call is one pass and this test compares nothing
    header = os.path.join(os.path.dirname(os.path.abspath(mcalf_amd.__file__)), "csrc", "grad_args.h")
    budget = int(re.search(r"kGradChunkBytes = size_t\((\d+)\) << 20", open(header).read()).group(1)) << 20
    assert budget // (16 * prob.wl.size) < n
    P = workloads.draw_P(kw, n, np.random.default_rng(seed + 4))
    V = _tangents(prob, n, 81)
    Q = np.random.default_rng(82).normal(0.0, 1.0, (n, prob.wl.size))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        dM, G = fit.model_jvp_batch(P, V), fit.model_vjp_batch(P, Q)
        h = n // 2
        assert np.array_equal(dM[:h], fit.model_jvp_batch(P[:h], V[:h])) and np.array_equal(dM[h:], fit.model_jvp_batch(P[h:], V[h:]))
        assert np.array_equal(G[:h], fit.model_vjp_batch(P[:h], Q[:h])) and np.array_equal(G[h:], fit.model_vjp_batch(P[h:], Q[h:]))
