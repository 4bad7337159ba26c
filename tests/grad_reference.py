"""Test-side reference for the analytic gradient of logL (mcalf_loglike_grad_batch): float64 numpy / scipy, built on the
oracle's own `voigt_tau`, `convolve_model`, `lsf_kernel` and JAX-path functions.

With w = 1/err^2, F = exp(-sum tau), m = cont L(F) and q = w (d - m) (0 on the pixels nansum drops),
d logL / d theta = sum_i q_i dm_i/dtheta.  The reference forms dm/dtheta for every parameter explicitly (forward mode:
dm = -cont L(F dtau) for a line parameter, dm = cont (dL/dR)(F) for R, L(F) for the continuum), so it checks the
kernels' adjoint (L^T) formulation rather than restating it, and it yields the scale the GPU tests measure errors
against: S_k = sum_i |q_i dm_i/dtheta_k|.  Per (component, line), K = cne/dnu, H = Re w(u + i a), w' = -2 z w + 2i/sqrt(pi) (series for |z| >= 8):
    dtau/dN = ln10 tau,  dtau/dz = K Re w' (c/lambda)/dnu,  dtau/db = -(K/b)(H + u Re w' - a Im w').
On the numpy path the LSF tap count is held at its value for theta (G is the derivative within that piece);
dw_k/dsigma = w_k (k^2 - sum_j w_j j^2)/sigma^3 for the normalised taps."""
import numpy as np
from scipy.special import wofz

from oracle import numpy_oracle as o

LN10 = np.log(10.0)


def _asymptotic(z):
    """(w', (z w)') for |z| >= 8 from the Laplace series w = i/(sqrt(pi) z) sum_k (2k-1)!!/(2 z^2)^k differentiated term
    by term (24 terms, < 1e-18 dropped).  -2 z w + 2i/sqrt(pi) loses ~2|z|^2 times the relative error of w to
    cancellation there, and (z w)' = H + u H_u + a H_a cancels to O(1/|z|^2) of H (a damped line's Lorentzian wing does
    not depend on b)."""
    z = np.where(np.abs(z) < 8, 8.0, z)
    h = 1 / (2 * z * z)
    c = np.ones_like(z)
    t = np.zeros_like(z)
    e = np.zeros_like(z)
    for k in range(24):
        t = t - (2 * k + 1) * c
        e = e - 2 * k * c
        c = c * (2 * k + 1) * h
    return 1j / (np.sqrt(np.pi) * z * z) * t, 1j / (np.sqrt(np.pi) * z) * e


def _line_parts(prob, wl, logN, z, b, line):
    """tau and its (N, z, b) partials of one (component, line) on the grid `wl` [Angstrom]."""
    wrest, f, gam = line
    wave_cm, wrest_cm, b_cms = wl / 1e8, wrest / 1e8, b * 1e5
    tau = o.voigt_tau(wave_cm, logN, z, b_cms, wrest_cm, f, gam)
    dnu = b_cms / wrest_cm
    a = gam / (4 * np.pi * dnu)
    nu_obs = o.CCGS / wave_cm
    u = (nu_obs * (z + 1.0) - o.CCGS / wrest_cm) / dnu
    K = 0.014971475 * 10.0 ** logN * f / dnu
    z = u + 1j * a
    w = wofz(z)
    wp_far, e_far = _asymptotic(z)
    near = np.abs(z) < 8
    wp = np.where(near, -2 * z * w + 2j / np.sqrt(np.pi), wp_far)
    e = np.where(near, (1 - 2 * z * z) * w + 2j * z / np.sqrt(np.pi), e_far).real       # H + u H_u + a H_a = Re (z w)'
    return tau, LN10 * tau, K * wp.real * nu_obs / dnu, -(K / b) * e


def _taps(prob, R, jax):
    """Normalised taps w_k (k = -n..n) and dw_k/dR; n is the numpy path's astropy count or the JAX path's fixed grid."""
    sigma = (R / 2.354820) / prob.velstep
    if jax:
        n = o.jax_half_size(prob)
        k = np.arange(-n, n + 1, dtype=float)
        w = np.exp(-k ** 2 / (2 * sigma ** 2))
    else:
        w = o.lsf_kernel(R, prob.velstep)
        n = (w.size - 1) // 2
        k = np.arange(-n, n + 1, dtype=float)
    w = w / w.sum()
    dw = w * (k ** 2 - np.sum(w * k ** 2)) / sigma ** 3 / (2.354820 * prob.velstep)
    return w, dw


def _circular(x, taps):
    """sum_k taps_k x[(i + k - n) mod npix]: the periodic convolution with symmetric taps (astropy boundary='wrap')."""
    n = (taps.size - 1) // 2
    return sum(t * np.roll(x, -(k - n)) for k, t in enumerate(taps))


def grad_row(prob, p, jax=False, asymm_thresholds=None):
    """(logL, G[ndim], S[ndim]) of one parameter vector in float64; G is all NaN where logL is -inf or NaN."""
    p = np.asarray(p, dtype=float)
    ndim, s = prob.ndim, prob.startind
    G = np.zeros(ndim)
    S = np.zeros(ndim)
    if jax:
        logl = o.jax_loglike_f64(prob, p)
        R = p[0] if prob.freespecres else float(prob.specres[0])
        nc_raw = np.floor(p[s])
    else:
        logl = o.lnlhood_worker(prob, p, asymm_thresholds)
        R = p[0] if prob.freespecres else float(max(prob.specres))
        nc_raw = np.trunc(p[s])
    if not logl > -np.inf:
        return logl, np.full(ndim, np.nan), np.full(ndim, np.nan)
    cont = (p[1] if prob.freespecres else p[0]) if prob.freecont else float(prob.contval[0])
    nc = int(min(max(nc_raw, 0), prob.ncompmax))

    # every active (N, z, b) column: its tau partial (summed over the component's lines)
    tau = np.zeros_like(prob.wl)
    dtau = {}
    slots = [(1 + 3 * c + s, prob.lines) for c in range(nc)] + [(prob.endind + 3 * k, [prob.linefill]) for k in range(prob.nfill)]
    for col, lines in slots:
        logN, z, b = p[col:col + 3]
        acc = [np.zeros_like(prob.wl) for _ in range(3)]
        for line in lines:
            t, dN, dz, db = _line_parts(prob, prob.wl, logN, z, b, line)
            tau += t
            for j, d in enumerate((dN, dz, db)):
                acc[j] += d
        for j in range(3):
            dtau[col + j] = acc[j]
    F = np.exp(-tau)

    # the convolution L and dL/dR of the context's mode
    w, dw = _taps(prob, R, jax)
    if jax:
        h = (w.size - 1) // 2
        edge = np.zeros(F.size, dtype=bool)
        edge[:h] = edge[F.size - h:] = True

        def L(x):
            return np.where(edge, x, np.convolve(x, w, mode="same"))

        LRF = np.where(edge, 0.0, np.convolve(F, dw, mode="same"))
    elif R > prob.velstep:
        def L(x):
            return o.convolve_model(x, R, prob.velstep)

        LRF = _circular(F, dw)
    else:
        def L(x):
            return x

        LRF = np.zeros_like(F)

    LF = L(F)
    m = cont * LF
    ispec2 = 1.0 / prob.err ** 2
    with np.errstate(invalid="ignore"):
        term = ispec2 * (prob.flux - m) ** 2 - np.log(ispec2)
    q = np.where(np.isnan(term), 0.0, ispec2 * (prob.flux - m))

    dm = {}
    if prob.freespecres:
        dm[0] = cont * LRF
    if prob.freecont:
        dm[1 if prob.freespecres else 0] = LF
    for col, d in dtau.items():
        dm[col] = -cont * L(F * d)
    for col, d in dm.items():
        G[col] = np.sum(q * d)
        S[col] = np.sum(np.abs(q * d))
    return logl, G, S


def grad_batch(prob, P, jax=False, asymm_thresholds=None):
    rows = [grad_row(prob, p, jax, asymm_thresholds) for p in np.asarray(P, dtype=float)]
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows]))


def loglike(prob, p, jax=False, asymm_thresholds=None):
    return o.jax_loglike_f64(prob, p) if jax else o.lnlhood_worker(prob, p, asymm_thresholds)


def central_differences(prob, p, cols, jax=False, rel=1e-6, rel_z=1e-9):
    """d logL / d p[k] for k in `cols` by central differences of the oracle's logL: step rel * max(1, |p_k|), and
    rel_z * (1 + z) for a redshift (a line is ~1e-5 wide in z, so the usual step would straddle it)."""
    p = np.asarray(p, dtype=float)
    out = {}
    for k in cols:
        is_z = k > prob.startind and (k - prob.startind - 1) % 3 == 1
        h = rel_z * (1.0 + abs(p[k])) if is_z else rel * max(1.0, abs(p[k]))
        up, dn = p.copy(), p.copy()
        up[k] += h
        dn[k] -= h
        out[k] = (loglike(prob, up, jax) - loglike(prob, dn, jax)) / (2 * h)
    return out
