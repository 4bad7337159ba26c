"""GPU: the analytic gradient of logL (mcalf_loglike_grad_batch[_device], mcalf_voigt_hjerting_grad) against the float64
reference of tests/grad_reference.py (itself checked against central differences in tests/test_grad_reference.py) and
against central differences of the oracle's logL; the columns and rows fixed by definition; bit equality across
calls, batch positions, entries, device counts and workspace passes; a scipy optimiser and the JAX closure's host half.

Bar against the reference, per row and column: |dG_k| <= 1e-7 S_k + 1e-9 with S_k = sum_i |q_i dm_i/dtheta_k|, the
size of the terms the column sums (so cancellation in G is not held against the kernels)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch
from scipy.special import wofz

import grad_reference as gr
import mcalf_amd
from mcalf_amd import _lib, workloads
from cases import oracle_synth, problem_from_kwargs
from oracle import numpy_oracle as o

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CIV = [(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8)]


def _assert_close(G, ref_G, S, what):
    fin = np.isfinite(ref_G).all(axis=1)
    assert np.array_equal(np.isnan(G).all(axis=1), ~fin), what
    d = np.abs(G[fin] - ref_G[fin])
    bar = 1e-7 * S[fin] + 1e-9
    worst = np.unravel_index(np.argmax(d / bar), d.shape)
    assert np.all(d <= bar), (what, worst, G[fin][worst], ref_G[fin][worst], S[fin][worst])


def _check(kw, P, jax=False, what=""):
    prob = problem_from_kwargs(kw)
    with mcalf_amd.als_fitter(None, conv_mode="jax" if jax else "numpy", **kw) as fit:
        ll, G = fit.loglike_grad_batch(P)
        ll_ref = fit.loglike_batch(P)
    want_ll, ref_G, S = gr.grad_batch(prob, P, jax=jax)
    assert np.array_equal(ll, ll_ref), what                          # logL is the likelihood's own
    _assert_close(G, ref_G, S, what)
    return G


def _civ(npix=600, specres=(8.0,), contval=(1.0,), ncomp=(1, 3), nfill=1, velstep=None, seed=0):
    rng = np.random.default_rng(seed)
    wl = np.linspace(6180.0, 6220.0, npix + 2)[1:-1]
    kw = dict(fitrange=[[6180.0, 6220.0]], fitlines=["CIV 1548", "CIV 1550"], linepars=CIV, ncomp=list(ncomp), nfill=nfill,
              specres=list(specres), contval=list(contval), Nrange=[12.5, 14.5], brange=[8.0, 40.0], zrange=[2.995, 3.012],
              spectrum=(wl, 1 + rng.normal(0, 0.03, npix), rng.uniform(0.01, 0.05, npix)))
    if velstep is not None:
        kw["velstep"] = float(velstep)
    return kw


def _g1():
    d = np.loadtxt(os.path.join(GOLD, "civ_mock_spec.txt"))
    return dict(fitrange=[[6180, 6220]], fitlines=["CIV 1548", "CIV 1550"], linepars=CIV, ncomp=[1, 1], specres=[8.0],
                Nrange=[12.0, 15.0], brange=[5.0, 40.0], zrange=[2.99, 3.01], spectrum=(d[:, 0], d[:, 1], d[:, 2]))


def test_voigt_hjerting_grad_against_scipy():
    x = np.concatenate([np.linspace(-30, 30, 1201), np.geomspace(30, 3000, 200), -np.geomspace(30, 3000, 200)])
    ys = np.concatenate([np.geomspace(1e-6, 0.1, 9), [0.005, 0.3, 1.0, 3.0]])      # y > 2^-8: the general range
    X, Y = (a.ravel() for a in np.meshgrid(x, ys))
    out = np.empty(3 * X.size)
    pd = C.POINTER(C.c_double)
    rc = _lib.load().mcalf_voigt_hjerting_grad(X.ctypes.data_as(pd), Y.ctypes.data_as(pd), X.size, out.ctypes.data_as(pd), -1)
    assert rc == 0
    H, Hx, Hy = out.reshape(-1, 3).T
    z = X + 1j * Y
    w = wofz(z)
    wp = -2 * z * w + 2j / np.sqrt(np.pi)
    # H: 1e-13 of |w| (scipy's wofz is ~2e-14); the partials: 1e-11 of |w'| plus the cancellation floor of the scipy-side
    # w' = -2 z w + 2i/sqrt(pi), 2 |z| |w| x 2e-14
    assert np.all(np.abs(H - w.real) <= 1e-13 * np.abs(w))
    floor = 4e-14 * np.abs(z) * np.abs(w)
    assert np.all(np.abs(Hx - wp.real) <= 1e-11 * np.abs(wp) + floor)
    assert np.all(np.abs(Hy + wp.imag) <= 1e-11 * np.abs(wp) + floor)


def test_voigt_hjerting_grad_against_mpmath(tmp_path_factory):
    """The entry on the points of tests/golden/voigt_grad_reference.npz, with the bars of tests/test_gpu_voigt_grad.py and no
    |z|-scaled floor; and bit for bit what the probe of voigt_grad.h returns, which ties that probe to the shipped object."""
    import voigt_grad_probe as vgp
    fx = vgp.Fixture()
    out = np.empty(3 * fx.n)
    pd = C.POINTER(C.c_double)
    rc = _lib.load().mcalf_voigt_hjerting_grad(fx.x.ctypes.data_as(pd), fx.y.ctypes.data_as(pd), fx.n, out.ctypes.data_as(pd), -1)
    assert rc == 0
    H, Hx, Hy = out.reshape(-1, 3).T
    dH, dHx, dHy = np.abs(H - fx.ref["wr"]), np.abs(Hx - fx.ref["dr"]), np.abs(Hy + fx.ref["di"])
    s = fx.series
    for name, err, q in (("H", dH, "wr"), ("H_x", dHx, "dr"), ("H_y", dHy, "di")):
        assert not vgp.worst(err, 1e-14 * np.abs(fx.ref[q]) + 1e-22, s, fx, "entry, series %s" % name).any(), name
    assert not vgp.worst(dH, 5e-15 * fx.cabs["wr"], fx.core, fx, "entry, core H").any()
    assert not vgp.worst(np.hypot(dHx, dHy), 2e-13 * fx.cabs["dr"], fx.core, fx, "entry, core (H_x, H_y)").any()
    dev = vgp.run_probe(vgp.load_probe(tmp_path_factory.mktemp("voigt_grad_probe")), fx.x, fx.y)
    assert np.array_equal(H, dev["wr"]) and np.array_equal(Hx, dev["dr"]) and np.array_equal(Hy, -dev["di"])


def test_grad_G1_and_config_A():
    kw = _g1()
    P = np.array([[1.0, 13.8, 3.0, 15.0], [1.0, 13.5, 3.0002, 22.0], [1.0, 14.2, 2.9995, 9.0]])
    _check(kw, P, what="G1")
    kwA, _, seed = workloads.config("A")
    _check(kwA, workloads.draw_P(kwA, 8, np.random.default_rng(seed)), what="A")


def test_grad_config_C_free_R_fillers():
    kw, _, seed = workloads.config("C", oracle_synth)
    _check(kw, workloads.draw_P(kw, 64, np.random.default_rng(seed)), what="C")


def test_grad_free_continuum():
    kwA, _, seed = workloads.config("A")
    kw = dict(kwA, contval=[0.9, 1.1])
    _check(kw, workloads.draw_P(kw, 8, np.random.default_rng(seed + 1)), what="A free cont")


def test_grad_config_E_damped():
    kw, _, seed = workloads.config("E", oracle_synth)
    _check(kw, workloads.draw_P(kw, 16, np.random.default_rng(seed), damped=2), what="E")


def test_grad_jax_path():
    kw, _, seed = workloads.config("C", oracle_synth)
    _check(kw, workloads.draw_P(kw, 32, np.random.default_rng(seed + 2)), jax=True, what="C jax")


def test_grad_R_at_or_below_velstep():
    kw = _civ(specres=(8.0,), velstep=10.0)
    G = _check(kw, workloads.draw_P(kw, 6, np.random.default_rng(5)), what="R <= velstep")
    assert np.isfinite(G).all()


def test_grad_wide_lsf():
    kw = _civ(npix=333, specres=(6.0, 9.0), contval=(0.9, 1.1), nfill=2, velstep=0.0031, seed=333)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        assert 2 * fit.info.n_cap + 64 > 4096
    _check(kw, workloads.draw_P(kw, 4, np.random.default_rng(9)), what="wide LSF")


def test_grad_fractional_and_negative_ncomp_and_fixed_columns():
    kw = _civ(ncomp=(0, 3), specres=(6.0, 9.0))
    P = workloads.draw_P(kw, 8, np.random.default_rng(11))
    s = 1
    P[:, s] = [2.7, 1.2, -0.5, -1.5, 0.3, 3.0, 2.0, 0.999]
    for jax in (False, True):
        G = _check(kw, P, jax=jax, what=f"ncomp jax={jax}")
        assert np.all(G[:, s] == 0.0)
        for r, v in enumerate(P[:, s]):
            active = int(min(max(np.floor(v) if jax else np.trunc(v), 0), 3))
            assert np.all(G[r, s + 1 + 3 * active: s + 1 + 9] == 0.0)


def test_grad_central_differences():
    kw = _civ(specres=(6.0, 9.0), contval=(0.9, 1.1), ncomp=(3, 3))
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 8, np.random.default_rng(13))
    for p in P:                                    # R away from the tap-count jumps
        while len({np.ceil(3.0348 * (r / 2.354820) / prob.velstep) for r in (p[0] - 1e-5, p[0] + 1e-5)}) > 1:
            p[0] += 1e-4
    with mcalf_amd.als_fitter(None, **kw) as fit:
        _, G = fit.loglike_grad_batch(P)
    _, _, S = gr.grad_batch(prob, P)
    cols = [k for k in range(prob.ndim) if k != prob.startind]
    for r, p in enumerate(P):
        cd = gr.central_differences(prob, p, cols)
        for k in cols:
            assert abs(G[r, k] - cd[k]) <= 1e-5 * S[r, k], (r, k, G[r, k], cd[k], S[r, k])


def test_grad_veto_rows_are_nan():
    kw, _, seed = workloads.config("A")
    P = workloads.draw_P(kw, 6, np.random.default_rng(21))
    P[0] = [2.0, 14.5, 3.005, 40.0, 14.5, 3.006, 40.0]          # strong absorption where the data has none: vetoed
    with mcalf_amd.als_fitter(None, Asymmlike=True, gauss_cdf=[0, 0, 0], **kw) as fit:
        ll, G = fit.loglike_grad_batch(P)
        assert np.array_equal(ll, fit.loglike_batch(P))
    assert ll[0] == -np.inf and np.all(np.isnan(G[0]))
    assert np.array_equal(np.isnan(G).all(axis=1), ~np.isfinite(ll))
    assert np.isfinite(G[np.isfinite(ll)]).all()


def test_grad_bit_equality():
    kw, _, seed = workloads.config("C", oracle_synth)
    P = workloads.draw_P(kw, 4096, np.random.default_rng(seed + 3))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        ll1, G1 = fit.loglike_grad_batch(P)
        ll2, G2 = fit.loglike_grad_batch(P)
        assert np.array_equal(G1, G2) and np.array_equal(ll1, ll2)
        for r in (0, 1777, 4095):
            l1, g1 = fit.loglike_grad_batch(P[r:r + 1])
            assert np.array_equal(g1[0], G1[r]) and l1[0] == ll1[r]
        # the device entry on the caller's stream
        dP = torch.from_numpy(P).cuda()
        dL = torch.empty(P.shape[0], dtype=torch.float64, device="cuda")
        dG = torch.empty(P.shape, dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream
        for _ in range(2):                         # (the second call allocates nothing)
            rc = fit._lib.mcalf_loglike_grad_batch_device(fit._ctx, dP.data_ptr(), P.shape[0], dL.data_ptr(), dG.data_ptr(),
                                                          C.c_void_p(stream))
            assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(dG.cpu().numpy(), G1) and np.array_equal(dL.cpu().numpy(), ll1)
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as fit:
        l3, G3 = fit.loglike_grad_batch(P[:1000])
    assert np.array_equal(G3, G1[:1000]) and np.array_equal(l3, ll1[:1000])


def test_grad_workspace_passes():
    kw, _, seed = workloads.config("E", oracle_synth)
    P = workloads.draw_P(kw, 2048, np.random.default_rng(seed + 4))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        _, G = fit.loglike_grad_batch(P)                              # more rows than one F / q pass holds
        _, Ga = fit.loglike_grad_batch(P[:1024])
        _, Gb = fit.loglike_grad_batch(P[1024:])
    assert np.array_equal(G, np.concatenate([Ga, Gb]))


def test_lnlhood_grad_with_lbfgsb():
    from scipy.optimize import minimize
    kw = _g1()
    truth = np.array([1.0, 13.8, 3.0, 15.0])
    with mcalf_amd.als_fitter(None, **kw) as fit:
        ll_truth = fit.lnlhood_worker(truth)
        x0 = truth + np.array([0.0, 0.3, 2e-4, 5.0])
        free = [1, 2, 3]

        def fun(x):
            p = truth.copy()
            p[free] = x
            ll, g = fit.lnlhood_grad(p)
            return -ll, -g[free]

        res = minimize(fun, x0[free], jac=True, method="L-BFGS-B",
                       bounds=[(12.0, 15.0), (2.999, 3.001), (5.0, 40.0)], options=dict(maxiter=500))
        assert -res.fun >= ll_truth - 1e-3, (res, ll_truth)


def test_jax_closure_host_grad():
    kw, _, seed = workloads.config("A")
    P = workloads.draw_P(kw, 16, np.random.default_rng(seed + 5)).astype(np.float32)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        f = fit.get_jax_likelihood(use_jax=False)
        ll, G = f.host_grad(P)
        want_ll, want_G = f.fitter.loglike_grad_batch(P.astype(np.float64))
        assert ll.dtype == np.float32 and G.dtype == np.float32 and G.shape == P.shape
        assert np.array_equal(ll, want_ll.astype(np.float32)) and np.array_equal(G, want_G.astype(np.float32))
        l1, g1 = f.host_grad(P[0])
        assert l1 == ll[0] and np.array_equal(g1, G[0])
