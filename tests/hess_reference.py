"""Test-side reference for the Hessian-vector product of logL (mcalf_loglike_hvp_batch): float64, and no code shared with
the device's second-order arithmetic -- the dense H[ndim, ndim] = d2 logL / dtheta2 of ONE row from Richardson-extrapolated
central differences of the gradient reference (tests/grad_reference.py: grad_row), one column at a time:

    D(h)  = (G(theta + h e_k) - G(theta - h e_k)) / 2h                 on a ladder of steps, each half the one before
    R1(h) = (4 D(h/2) - D(h)) / 3,   R2 = (16 R1(h/2) - R1(h)) / 15,   R3 = (64 R2(h/2) - R2(h)) / 63
    H[k, :] = R3 of the best four consecutive steps, entry by entry (`_richardson`)

The steps are per column class, as grad_reference.central_differences takes them: h = REL max(1, |theta_k|) for R, the
continuum, logN and b, and REL_Z (1 + z) b / 30 km/s for a redshift (a line is b / c (1 + z) wide in z).  On the numpy path the LSF tap count
is held at the value it has at theta across the whole stencil (`held_tap_count`), which is what the library differentiates.
Rows and columns that are 0 by definition (the ncomp slot, inactive components, R where R <= velstep) are left exactly 0.

Any number of tangents at one theta then cost nothing more: H v = H @ v.  The scale the GPU tests measure errors against,
    S_k = sum_j |v_j| sum_i W_i |J_ik| |J_ij|        (the Fisher product in absolute values, tests/model_deriv_reference.py)
is one that cancellation between the Fisher and the curvature term cannot shrink."""
import contextlib

import numpy as np

import grad_reference as gr
import model_deriv_reference as mdr
from oracle import numpy_oracle as o

REL = 2e-3        # relative step of R, continuum, logN, b (the middle of the ladder below)
REL_Z = 2e-6      # of a redshift, times (1 + z) and b / 30 km/s (`column_step`)


def tap_half_width(prob, R):
    """The numpy path's astropy tap half-width at resolution R (hires_fitter.py:458)."""
    return int(np.ceil(3.0348 * (R / 2.354820) / prob.velstep))


LONG_TAPS = 500   # half-widths beyond this: the oracle's tap-by-tap Python loops are replaced by one circular FFT product


def _periodic(x, taps):
    """sum_k taps_k x[(i + k - n) mod npix] through the FFT: the taps folded onto the period, then one circular correlation."""
    n = (taps.size - 1) // 2
    folded = np.zeros(x.size)
    np.add.at(folded, (np.arange(taps.size) - n) % x.size, taps)
    return np.fft.irfft(np.fft.rfft(x) * np.conj(np.fft.rfft(folded)), x.size)


@contextlib.contextmanager
def held_tap_count(n):
    """Inside, the oracle's LSF has 2 n + 1 taps whatever the resolution (its Gaussian still follows R); restored on exit.
    n None leaves the oracle alone (the JAX path's grid is fixed already).  For an LSF of thousands of taps the oracle's
    periodic convolution and grad_reference._circular, each a Python loop over the taps, are stated as the circular
    correlation they are (the same taps on the same period, summed by an FFT), or a row would take minutes."""
    if n is None:
        yield
        return
    saved = o.lsf_kernel, o.convolve_model, gr._circular

    def fixed(fwhm, velstep):
        sigma = (fwhm / 2.354820) / velstep
        x = np.arange(-n, n + 1, dtype=float)
        return np.exp(-0.5 * x * x / (sigma * sigma)) / (np.sqrt(2 * np.pi) * sigma)

    def convolve(spec, fwhm, velstep):
        ker = fixed(fwhm, velstep)
        ker = ker / ker.sum()
        return _periodic(spec, ker) / ker.sum()

    o.lsf_kernel = fixed
    if n > LONG_TAPS:
        o.convolve_model = convolve
        gr._circular = _periodic
    try:
        yield
    finally:
        o.lsf_kernel, o.convolve_model, gr._circular = saved


def _held(prob, p, jax):
    R, _, _ = mdr.row_parameters(prob, p, jax)
    return None if (jax or not R > prob.velstep) else tap_half_width(prob, R)


def live_columns(prob, p, jax=False):
    """The columns of theta that logL depends on differentiably at p: not the ncomp slot, not the (N, z, b) of components at
    or beyond the active count, not R where R <= velstep on the numpy path."""
    R, _, nc = mdr.row_parameters(prob, p, jax)
    s = prob.startind
    cols = []
    if prob.freespecres and (jax or R > prob.velstep):
        cols.append(0)
    if prob.freecont:
        cols.append(1 if prob.freespecres else 0)
    cols += list(range(s + 1, s + 1 + 3 * nc)) + list(range(prob.endind, prob.ndim))
    return cols


def column_step(prob, p, k, rel=REL, rel_z=REL_Z):
    """The middle step of column k's ladder.  A redshift's is rel_z (1 + z) for a line of b = 30 km/s (1e-4 (1 + z) wide in
    z) and shrinks with b: a 2 km/s filler is fifteen times narrower, and the ladder's top step must stay inside the line."""
    is_z = k > prob.startind and (k - prob.startind - 1) % 3 == 1
    if is_z:
        return rel_z * (1.0 + abs(p[k])) * min(1.0, abs(p[k + 1]) / 30.0)
    return rel * max(1.0, abs(p[k]))


LADDER = (32.0, 16.0, 8.0, 4.0, 2.0, 1.0, 0.5, 0.25)      # multiples of the column's step at which D is evaluated


def _richardson(f, p, k, h):
    """(R3, error estimate) of the central differences of the vector function f along column k.  D is evaluated on the
    whole step ladder; every four consecutive steps give one three-level extrapolation R3 (error O(h^8)) with the estimate
    |R3 - R2(its three smaller steps)| + |R3 - R3(a neighbouring quadruple)|.  Large steps leave truncation error, small
    ones amplify the rounding of G and the 1e-13-relative seams of the gradient reference's Voigt function (scipy's wofz
    changes algorithm by region, the reference its formula at |z| = 8) by 1 / h; per entry, the quadruple with the smallest
    estimate is kept, with that estimate."""
    D = []
    for mult in LADDER:
        step = h * mult
        up, dn = p.copy(), p.copy()
        up[k] += step
        dn[k] -= step
        D.append((f(up) - f(dn)) / (2 * step))
    R1 = [(4 * D[i + 1] - D[i]) / 3 for i in range(len(D) - 1)]
    R2 = [(16 * R1[i + 1] - R1[i]) / 15 for i in range(len(R1) - 1)]
    R3 = np.array([(64 * R2[i + 1] - R2[i]) / 63 for i in range(len(R2) - 1)])
    own = np.array([np.abs(R3[i] - R2[i + 1]) for i in range(len(R3))])
    nb = np.abs(np.diff(R3, axis=0))
    est = own + np.minimum(np.vstack([nb, nb[-1:]]), np.vstack([nb[:1], nb]))
    best = np.argmin(est, axis=0)
    cols = np.arange(R3.shape[1])
    return R3[best, cols], est[best, cols]


def hessian(prob, p, jax=False, rel=REL, rel_z=REL_Z):
    """(H[ndim, ndim], E[ndim, ndim]) of one parameter vector: row k of H is d G / d theta_k, E its error estimate (the
    difference of the last two Richardson levels).  H is NOT symmetrised: its asymmetry is the second error measure."""
    p = np.asarray(p, dtype=float)
    H = np.zeros((prob.ndim, prob.ndim))
    E = np.zeros((prob.ndim, prob.ndim))
    cols = live_columns(prob, p, jax)

    def G(theta):
        with np.errstate(divide="ignore", invalid="ignore"):
            return gr.grad_row(prob, theta, jax=jax)[1]

    with held_tap_count(_held(prob, p, jax)):
        for k in cols:
            H[k], E[k] = _richardson(G, p, k, column_step(prob, p, k, rel, rel_z))
    dead = np.setdiff1d(np.arange(prob.ndim), cols)
    H[:, dead] = 0.0
    E[:, dead] = 0.0
    return H, E


def fisher_abs(prob, p, jax=False):
    """A[k, j] = sum_i W_i |J_ik| |J_ij| and the Jacobian it came from."""
    _, J = mdr.model_jacobian(prob, p, jax=jax)
    W = mdr.kept_weights(prob)
    return np.abs(J).T @ (W[:, None] * np.abs(J)), J


def hvp(H, A, v):
    """(H v, S) for one tangent; the entries of v in columns that are 0 by definition are ignored (NaN allowed there)."""
    v = np.where(np.all(A == 0.0, axis=0), 0.0, np.asarray(v, dtype=float))
    return H @ v, A @ np.abs(v)


SMALL = 1e-6      # entries with S_k below SMALL max_k S_k are judged by the floor, not by the relative bar


def reference_error(H, E, A, v):
    """The reference's own error on H v in units of S: with Err[k, j] the larger of the Richardson estimate and half the
    asymmetry, max over the entries k with S_k >= SMALL max S of (sum_j Err[k, j] |v_j|) / S_k.  (On the entries below
    that, S_k is the product of two lines' far wings and no relative statement can be made: the GPU tests' floor covers them.)"""
    v = np.where(np.all(A == 0.0, axis=0), 0.0, np.asarray(v, dtype=float))
    S = A @ np.abs(v)
    if S.max() == 0.0:
        return 0.0
    big = S >= SMALL * S.max()
    return float(np.max((np.maximum(E, 0.5 * np.abs(H - H.T)) @ np.abs(v))[big] / S[big]))


def class_tangents(prob, p, jax=False):
    """One tangent with a single non-zero entry per parameter class that is live at p: R, continuum, logN, z, b (of the
    first active component or filler), sized as model_deriv_reference.tangent_scales."""
    cols = live_columns(prob, p, jax)
    sc = mdr.tangent_scales(prob)
    first = [k for k in cols if k > prob.startind][:3]
    out = []
    for k in [c for c in cols if c < prob.startind] + first:
        v = np.zeros(prob.ndim)
        v[k] = sc[k]
        out.append(v)
    return out


def gauss_newton_plus_curvature(prob, p, jax=False, rel=REL, rel_z=REL_Z):
    """-J^T W J + sum_i W_i r_i d2 m_i / dtheta_k dtheta_j, the curvature term from Richardson central differences of the
    reference JACOBIAN (tests/model_deriv_reference.py) contracted with W r: a second route to H that never touches
    grad_row's adjoint formulation."""
    p = np.asarray(p, dtype=float)
    W = mdr.kept_weights(prob)
    cols = live_columns(prob, p, jax)
    with held_tap_count(_held(prob, p, jax)):
        m, J = mdr.model_jacobian(prob, p, jax=jax)
        q = W * np.where(W > 0.0, prob.flux - m, 0.0)

        def qJ(theta):
            return q @ mdr.model_jacobian(prob, theta, jax=jax)[1]

        C = np.zeros((prob.ndim, prob.ndim))
        for k in cols:
            C[k], _ = _richardson(qJ, p, k, column_step(prob, p, k, rel, rel_z))
    dead = np.setdiff1d(np.arange(prob.ndim), cols)
    C[:, dead] = 0.0
    return -(J.T @ (W[:, None] * J)) + C
