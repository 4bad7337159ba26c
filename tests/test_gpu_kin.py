"""GPU: batched optical-depth kinematics -- mcalf_kinematics_batch[_device] and the Python entries on it (mcalf_amd.kinematics:
kinematics_batch, dv90_batch, zabs_batch) -- against the numpy restatement of tests/kin_reference.py (itself anchored on closed forms by
tests/test_kin_host.py).  The bars (kin_reference.check_*), all against that restatement:

    I         |d| <= 1e-11 + 1e-9 |I|                        the equivalent widths' bar
    lam_mean  |d| <= 1e-11 + 2e-9 W,  W = wl[-1] - wl[0]     that bar carried through M1 / I
    lam_rms   |rms_got^2 - rms_ref^2| <= 1e-11 + 4e-9 W^2    as variances: the square root is not well conditioned near 0
    lam_q     |C_ref(lam_got) - q I_ref| <= 1e-11 + 1e-9 |I_ref| and e[0] <= lam_got <= e[npix], C_ref the piecewise-linear
              cumulative through (e[k+1], S_ref[k]): a bar on lambda itself would be ill-conditioned wherever the crossing pixel
              holds little of I

NaN and exact-0 cells must coincide.  Every comparison prints its worst error / bar (pytest -s).

Shapes: the pixel kernels' tile is 2048 pixels (four waves, 8 slabs of 64 consecutive pixels each), so 2 and 257 pixels are
partial first tiles, 2049 pixels put one pixel into a second tile and 4500 pixels are two full tiles and one of 404."""
import ctypes as C

import numpy as np
import pytest
import torch

import kin_reference as kr
import mcalf_amd
from cases import oracle_synth, problem_from_kwargs
from mcalf_amd import _lib, kinematics as kn, workloads

pytestmark = pytest.mark.gpu

CIV3 = [(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8), (1549.5, 0.05, 2.6e8)]      # (the third is made up: a line between the two)
Q3 = (0.05, 0.5, 0.95)


def _width(prob):
    return float(prob.wl[-1] - prob.wl[0])


def _compare(fit, prob, P, q, what, jax=False):
    kin = kn.kinematics_batch(fit, P, q=q)
    nq = len(q)
    assert kin.tau_int.shape == kin.lam_mean.shape == kin.lam_rms.shape == (len(P), prob.numlines)
    assert kin.lam_q.shape == (len(P), prob.numlines, nq)
    ref = kr.rows(prob, P, q, jax)
    kr.check_all(kin, ref, q, _width(prob), what)
    return kin, ref


def _edge_kw(npix, nlines, startind, ncompmax=3, nfill=1):
    wl = np.linspace(6180.0, 6220.0, npix + 2)[1:-1]
    rng = np.random.default_rng(npix)
    return dict(fitrange=[[6180.0, 6220.0]], fitlines=["CIV 1548", "CIV 1550", "made up"][:nlines], linepars=CIV3[:nlines],
                ncomp=[0, ncompmax], nfill=nfill, specres=[6.0, 9.0] if startind >= 1 else [8.0], contval=[0.9, 1.1] if startind == 2 else [1.0],
                Nrange=[12.5, 14.5], brange=[8.0, 40.0], zrange=[2.995, 3.012], velstep=float(np.median(np.diff(wl) / wl[1:]) * 2.9979245e5),
                spectrum=(wl, 1 + rng.normal(0, 0.03, npix), np.full(npix, 0.03)))


def _edge_rows(kw, s):
    """Count slots 0, 1, ncompmax, 2.7 and -1; NaN in the inactive slots; NaN in an active slot; the general Voigt path
    (an absurd column, b < 0: what tests/test_gpu_eqw.py sends there)."""
    P = workloads.draw_P(kw, 9, np.random.default_rng(3))
    P[:, s] = [0.0, 1.0, 3.0, 2.7, -1.0, 1.0, 2.0, 3.0, 3.0]
    P[5, s + 4:s + 10] = np.nan                                   # slots 1 and 2 of a row with one active component
    P[6, s + 2] = np.nan                                          # z of the first of two active components
    P[7, s + 1] = 30.0                                            # logN = 30: exp(-x^2) matters far beyond |x| = 8
    P[8, s + 3] = -12.0                                           # b < 0: a < 0, scipy's reflection -- K < 0 too, so this slot's tau is
    P[8, [s + 1, s + 4, s + 7]] = [12.5, 14.0, 14.0]              # NEGATIVE in the core; kept 30 times weaker than the other two, so I > 0
    return P


@pytest.mark.parametrize("npix,nlines,startind", [(2, 1, 0), (257, 2, 1), (2049, 3, 2), (4500, 2, 0)])
def test_edge_shapes(npix, nlines, startind):
    kw = _edge_kw(npix, nlines, startind)
    prob = problem_from_kwargs(kw)
    s = prob.startind
    assert s == startind and prob.wl.size == npix and prob.numlines == nlines
    P = _edge_rows(kw, s)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        kin, _ = _compare(fit, prob, P, Q3, f"edge {npix} px, {nlines} lines, startind {startind}")
        for r in (0, 4):                                                          # no active slot: I = 0 exactly, the rest NaN
            assert np.all(kin.tau_int[r] == 0.0) and np.isnan(kin.lam_mean[r]).all() and np.isnan(kin.lam_rms[r]).all() and np.isnan(kin.lam_q[r]).all()
        for r in (1, 2, 3, 5, 7):                                                 # NaN in inactive slots does not leak
            assert np.isfinite(kin.tau_int[r]).all() and np.isfinite(kin.lam_mean[r]).all() and np.isfinite(kin.lam_q[r]).all()
        assert np.all(kin.tau_int[[1, 2, 3, 5, 7]] > 0.0)
        assert all(np.isnan(a[6]).all() for a in kin)                             # NaN in an active slot: the whole row
        alone = kn.kinematics_batch(fit, np.delete(P, 6, axis=0), q=Q3)               # ... and only that row
        assert all(np.array_equal(a, np.delete(b, 6, axis=0), equal_nan=True) for a, b in zip(alone, kin))


def test_jax_context_floors_the_slot():
    kw = _edge_kw(257, 2, 1)
    prob = problem_from_kwargs(kw)
    s = prob.startind
    P = _edge_rows(kw, s)[:4]
    P[:, s] = [-0.5, 2.7, 1.0, 3.9]
    with mcalf_amd.als_fitter(None, conv_mode="jax", **kw) as fit:
        kin, ref = _compare(fit, prob, P, Q3, "JAX context", jax=True)
        assert np.all(kin.tau_int[0] == 0.0) and np.isnan(kin.lam_q[0]).all() and np.all(kin.tau_int[1:] > 0.0)


@pytest.fixture(scope="module")
def seam():
    """The 4500-pixel seam problem (two slots) and its context's results for: one component at lam0 with (N, b) = (13, 12) and
    (15.5, 6); two components of (13, 12) at lam0 -+ 3 Angstrom.  16 quantiles, 0 and 1 among them."""
    kw = kr.seam_kw(ncompmax=2)
    prob = problem_from_kwargs(kw)
    pad = [13.0, 3.0, 10.0]
    P = np.array([np.concatenate([kr.seam_row(kw, 13.0, 12.0), pad]), np.concatenate([kr.seam_row(kw, 15.5, 6.0), pad]),
                  kr.seam_row(kw, 13.0, 12.0, offsets=(-3.0, 3.0))])
    q = tuple(np.linspace(0.0, 1.0, 16)[[0, 15, 5]]) + (0.25, 0.5, 0.75) + tuple(np.linspace(0.0, 1.0, 16)[[1, 2, 3, 4, 6, 7, 8, 9, 10, 11]])
    assert len(q) == 16
    with mcalf_amd.als_fitter(None, **kw) as fit:
        kin, ref = _compare(fit, prob, P, q, "seam problem, 16 quantiles")
        dv90 = kn.dv90_batch(fit, P)
        zabs = kn.zabs_batch(fit, P)
    return kw, prob, P, q, kin, ref, dv90, zabs


def test_a_line_on_the_seam_of_two_tiles(seam):
    kw, prob, P, q, kin, ref, dv90, zabs = seam
    lam0 = kr.seam_lam0(kw)
    for r in (0, 1):
        print(f"seam row {r}: |lam_0.5 - lam0| = {abs(kin.lam_q[r, 0, 4] - lam0):.3g}, |lam_mean - lam0| = {abs(kin.lam_mean[r, 0] - lam0):.3g}")
        assert abs(kin.lam_q[r, 0, 4] - lam0) <= 1e-4                              # the crossing sits on the boundary of tiles 0 and 1
    # the Python helpers on the same rows
    assert np.all(dv90 > 0) and abs(dv90[0] / 12.0 - 2.32617) <= 2e-3             # (kinematics_batch's own q = 0.05, 0.5, 0.95)
    assert np.array_equal(zabs, kin.lam_mean[:, 0] / kr.CIV1548[0] - 1.0) and abs(zabs[0] - P[0, 2]) <= 1e-7


def test_two_components_and_a_gap(seam):
    """Two components of equal N and b 6 Angstrom apart: the median falls between them, on a pixel that holds less than 1e-4 of
    I (a core pixel holds 1e-2: a bar on lambda itself would be a hundred times looser there) -- the bar in C holds all the same
    (checked with all 16 quantiles in the fixture).  Not AT the midpoint: I scales with 1 + z, the redder component holds 1e-3
    more, and the median climbs 2.3 Doppler widths up its blue flank to collect the difference.  The quartiles sit on the centres."""
    kw, prob, P, q, kin, ref, _, _ = seam
    lam0 = kr.seam_lam0(kw)
    assert q[3:6] == (0.25, 0.5, 0.75)
    l25, l50, l75 = kin.lam_q[2, 0, 3:6]
    k = int(np.searchsorted(ref[2].e, l50)) - 1
    print(f"gap: lam_0.25 - (lam0 - 3) = {l25 - lam0 + 3:.3g}, lam_0.75 - (lam0 + 3) = {l75 - lam0 - 3:.3g}, lam_0.5 - lam0 = {l50 - lam0:.3g}, "
          f"t[k] / I at the median = {ref[2].t[0, k] / ref[2].I[0]:.3g}")
    assert abs(l25 - (lam0 - 3.0)) <= 0.05 and abs(l75 - (lam0 + 3.0)) <= 0.05
    assert ref[2].t[0, k] <= 1e-4 * ref[2].I[0] and lam0 - 3.0 < l50 < lam0 + 3.0


def test_q_handling(seam):
    kw, prob, P, q, kin, ref, _, _ = seam
    e = ref[0].e
    assert q[0] == 0.0 and q[1] == 1.0
    assert np.isfinite(kin.lam_q).all() and np.all(kin.lam_q[:, 0, 0] >= e[0]) and np.all(kin.lam_q[:, 0, 1] <= e[-1])
    assert np.all(kin.lam_q[:, 0, 0] < kin.lam_q[:, 0, 1])
    with mcalf_amd.als_fitter(None, **kw) as fit:
        # shared quantiles under another list: the same bits
        other = kn.kinematics_batch(fit, P, q=(0.5, 1.0, 0.25))
        assert np.array_equal(other.lam_q[:, :, 0], kin.lam_q[:, :, 4]) and np.array_equal(other.lam_q[:, :, 1], kin.lam_q[:, :, 1])
        assert np.array_equal(other.lam_q[:, :, 2], kin.lam_q[:, :, 3])
        assert all(np.array_equal(a, b) for a, b in zip(other[:3], kin[:3]))
        # nq = 0 with mom alone; lamq alone
        none = kn.kinematics_batch(fit, P, q=())
        assert none.lam_q.shape == (3, 1, 0) and all(np.array_equal(a, b) for a, b in zip(none[:3], kin[:3]))
        lamq = np.full((3, 1, 16), -7.0)
        only = kn.kinematics_batch(fit, P, q=q, out=(None, lamq))
        assert only.tau_int is None and only.lam_q is lamq and np.array_equal(lamq, kin.lam_q)
        mom = np.full((3, 1, 3), -7.0)
        both = kn.kinematics_batch(fit, P, q=(0.5,), out=(mom, np.empty((3, 1, 1))))
        assert np.array_equal(mom[:, :, 0], kin.tau_int) and np.array_equal(both.lam_rms, kin.lam_rms)
        with pytest.raises(ValueError):
            kn.kinematics_batch(fit, P, q=(0.5,), out=(np.zeros(3), None))
        with pytest.raises(RuntimeError):
            kn.kinematics_batch(fit, P, q=(0.5, 1.5))
        with pytest.raises(RuntimeError):
            kn.kinematics_batch(fit, P, q=np.linspace(0, 1, 17))


@pytest.fixture(scope="module")
def drawn_C():
    """256 draws of config C (4000 pixels, 11 slots x 2 lines, fillers) through the host entry, and their reference."""
    kw, _, seed = workloads.config("C", oracle_synth)
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 256, np.random.default_rng(seed))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        kin, ref = _compare(fit, prob, P, Q3, "config C, 256 rows")
    return kw, prob, P, kin


def test_config_C_draws(drawn_C):
    kw, prob, P, kin = drawn_C
    assert kin.tau_int.shape == (256, 2) and np.isfinite(kin.lam_q).all() and np.all(kin.tau_int > 0)
    assert np.all(np.diff(kin.lam_q, axis=2) > 0) and np.all(kin.lam_rms > 0)
    assert np.all(kin.lam_mean > prob.wl[0]) and np.all(kin.lam_mean < prob.wl[-1])


def test_config_E_shard_draws():
    kw, _, seed = workloads.config("E", oracle_synth)
    prob = problem_from_kwargs(kw)
    P = workloads.draw_P(kw, 64, np.random.default_rng(seed), damped=2)
    P[0, prob.startind + 1] = 20.5                                # one saturated damped component for certain
    assert np.all(P[:, prob.startind + 1::3].max(axis=1) >= 20.0) and prob.wl.size == 20000
    with mcalf_amd.als_fitter(None, **kw) as fit:
        kin, ref = _compare(fit, prob, P, Q3, "config E shard, 64 rows, damped")
        dv90 = kn.dv90_batch(fit, P)
    peak = max(float((r.t[0] / kr.dlambda(prob.wl)).max()) for r in ref)
    print(f"config E shard: largest tau of the reference {peak:.3g}")
    assert peak > 1e6 and np.isfinite(kin.tau_int).all() and np.isfinite(kin.lam_q).all()       # exp(-tau) is 0 there; tau is not
    assert dv90.shape == (64,) and np.all(dv90 > 0)
    assert np.array_equal(dv90, 2.9979245e5 * (kin.lam_q[:, 0, 2] - kin.lam_q[:, 0, 0]) / kin.lam_q[:, 0, 1])


def test_bits_do_not_depend_on_batch_position_or_outputs(drawn_C):
    kw, prob, P, kin = drawn_C
    with mcalf_amd.als_fitter(None, **kw) as fit:
        part = kn.kinematics_batch(fit, P[100:164], q=Q3)
        assert all(np.array_equal(a, b[100:164]) for a, b in zip(part, kin))
        none = kn.kinematics_batch(fit, P, q=())                                       # mom without lamq
        assert all(np.array_equal(a, b) for a, b in zip(none[:3], kin[:3]))
        other = kn.kinematics_batch(fit, P, q=(0.95, 0.3, 0.05, 0.5))                  # shared quantiles under another list
        assert np.array_equal(other.lam_q[:, :, [2, 3, 0]], kin.lam_q) and all(np.array_equal(a, b) for a, b in zip(other[:3], kin[:3]))


def test_the_device_entry_equals_the_host_entry(drawn_C):
    kw, prob, P, kin = drawn_C
    n, nl = len(P), prob.numlines
    mom = np.stack([kin.tau_int, kin.lam_mean, kin.lam_rms], axis=2)
    q = np.array(Q3)
    with mcalf_amd.als_fitter(None, **kw) as fit:
        dP = torch.from_numpy(P).cuda()
        kept = dP.clone()
        dM = torch.full((n, nl, 3), -7.0, dtype=torch.float64, device="cuda")
        dQ = torch.full((n, nl, 3), -7.0, dtype=torch.float64, device="cuda")
        side = torch.cuda.Stream()
        for _ in range(2):                                               # (the second call allocates nothing)
            dM.fill_(-7.0)
            dQ.fill_(-7.0)
            side.wait_stream(torch.cuda.current_stream())
            assert fit._lib.mcalf_kinematics_batch_device(fit._ctx, dP.data_ptr(), n, q.ctypes.data, 3, dM.data_ptr(), dQ.data_ptr(),
                                                          C.c_void_p(side.cuda_stream)) == 0
            side.synchronize()
            assert np.array_equal(dM.cpu().numpy(), mom) and np.array_equal(dQ.cpu().numpy(), kin.lam_q)
        assert torch.equal(dP.view(torch.int64), kept.view(torch.int64))
        assert fit._lib.mcalf_kinematics_batch_device(fit._ctx, None, 0, None, 0, dM.data_ptr(), None, None) == 0      # batch == 0: nothing to do
    with mcalf_amd.als_fitter(None, device=[0, 0], **kw) as fit:
        assert fit.info.ndevices == 2
        two = kn.kinematics_batch(fit, np.concatenate([P, P]), q=Q3)                  # (a device takes at least 256 rows: 256 each)
        assert fit.last_launch().devices_used == 2
        assert all(np.array_equal(a, np.concatenate([b, b])) for a, b in zip(two, kin))
        rc = fit._lib.mcalf_kinematics_batch_device(fit._ctx, dP.data_ptr(), 8, q.ctypes.data, 3, dM.data_ptr(), dQ.data_ptr(), None)
        assert rc == _lib.MCALF_ERR_INVALID and b"not available on a multi-device context" in fit._lib.mcalf_last_error(fit._ctx)


def test_a_batch_of_several_passes_equals_its_halves():
    """A pass holds at most 65535 rows (the row is the pixel kernels' grid.y): 70000 rows of a 2-pixel spectrum are two."""
    kw = _edge_kw(2, 2, 0, nfill=0)
    P = workloads.draw_P(kw, 70000, np.random.default_rng(12))
    with mcalf_amd.als_fitter(None, **kw) as fit:
        kin = kn.kinematics_batch(fit, P, q=Q3)
        h = [kn.kinematics_batch(fit, P[:35000], q=Q3), kn.kinematics_batch(fit, P[35000:], q=Q3)]
    assert all(np.array_equal(a, np.concatenate([x, y]), equal_nan=True) for a, x, y in zip(kin, h[0], h[1]))
    active = P[:, 0] >= 1.0
    assert np.isfinite(kin.lam_q[active]).all() and active[65535:].any() and np.all(kin.tau_int[~active] == 0.0)


def test_a_spectrum_of_one_pixel_is_refused():
    lib = _lib.load()
    wl, one, err = np.array([6200.0]), np.ones(1), np.full(1, 0.02)
    pd = C.POINTER(C.c_double)
    lines = (_lib.mcalf_line * 1)(_lib.mcalf_line(1548.204, 0.1899, 2.643e8))
    sp = _lib.mcalf_spec(npix=1, wl=wl.ctypes.data_as(pd), flux=one.ctypes.data_as(pd), err=err.ctypes.data_as(pd), velstep=1.0, nlines=1,
                         lines=lines, fill=_lib.mcalf_line(250.0, 0.1899, 2.643e8), ncompmax=2, nfill=0, freespecres=0, freecont=0,
                         specres_fixed=0.5, specres_max=0.5, contval_fixed=1.0, conv_mode=0, device=-1, asymmlike=0, asymm_n4=0.0, asymm_n5=0.0)
    ctx = C.c_void_p()
    _lib.check(lib.mcalf_create(C.byref(sp), C.byref(ctx)))
    try:
        P, M = np.array([[1.0, 13.0, 3.0, 10.0, 13.0, 3.0, 10.0]]), np.zeros(3)
        assert lib.mcalf_kinematics_batch(ctx, P.ctypes.data, 1, None, 0, M.ctypes.data, None) == _lib.MCALF_ERR_INVALID
        assert b"2 pixels" in lib.mcalf_last_error(ctx)
        assert lib.mcalf_kinematics_batch_device(ctx, P.ctypes.data, 1, None, 0, M.ctypes.data, None, None) == _lib.MCALF_ERR_INVALID
        assert b"2 pixels" in lib.mcalf_last_error(ctx)
    finally:
        lib.mcalf_destroy(ctx)
