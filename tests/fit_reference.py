"""Test-side reference for the batched Levenberg-Marquardt fit (mcalf_maximize_batch): float64 numpy, ONE row at a time,
the algorithm of include/mcalf_hip.h restated with the oracle's `lnlhood_worker` for logL and the dense Jacobian of
tests/model_deriv_reference.py (`model_jacobian`) for the gradient G = J^T W (d - m) and the Fisher matrix J^T W J.  The
library never forms either matrix; the reference may, it is small.

Per row, in cube units s = hi - lo:
    start   the continuous, active entries clamped into the box; logL, G.  logL not finite, or a NaN among those entries
            (nansum then drops every pixel and logL is a finite 0): status -1, the row as given.
    pins    k is pinned if it may not move at all (the ncomp slot, an inactive (N, z, b), s_k == 0), if theta_k <= lo_k and
            G_k < 0, or if theta_k >= hi_k and G_k > 0.  g_u = s * G, pinned entries 0; all zero: status 2.
    step    (A + lambda I) x = g_u by `cg_iters` CG iterations from 0, A = s * (J^T W J) * s on the unpinned coordinates; the
            CG stops early when p.(A + lambda I)p <= 0 or r.r <= 1e-20 g_u.g_u.
    trial   T = clamp(theta + s * x); accepted iff logL(T) is finite and > logL(theta): lambda <- max(lambda / 10, 1e-15),
            status 1 if the gain <= ftol (1 + |logL(T)|); else lambda <- 10 lambda, status 3 beyond 1e12.

Measured on the CPU (tests/test_fit_reference.py: CIV doublet, 300 pixels, 3 components, six starts, ftol 1e-10) against
scipy.optimize.least_squares (trf, analytic Jacobian, tolerances 1e-15) from the same starts: the figures are in that
file's docstring: status 1 on every start after 6 outer iterations, no rejected step; logL below scipy's by 4.3e-11 ..
4.8e-10 against the stopping rule's own bar ftol (1 + |logL|) = 7.7e-8; the largest cube-unit distance to scipy's optimum
8.63e-7 (THETA_BAR below is 10 x that).  CG of the first outer iteration of start 0 at lambda 1e-2 (test_gpu_fit.py: full
CG): relative residual max|(A + lambda I)x - g| / max|g| as printed by that test."""
import numpy as np

import model_deriv_reference as mdr
from oracle import numpy_oracle as o

CG_TOL = 1e-20
LAMBDA_MIN, LAMBDA_MAX = 1e-15, 1e12
# 10 x the largest cube-unit distance between this reference's optimum and scipy's over the six starts of
# tests/test_fit_reference.py at ftol 1e-10 (measured there: see its docstring); the bar of the GPU convergence test.
THETA_BAR = 10 * 8.63e-7


def box(prob):
    return np.array([np.min(b) for b in prob.bounds], dtype=float), np.array([np.max(b) for b in prob.bounds], dtype=float)


def movable(prob, p, jax=False):
    """Coordinates the fit may change at all: not the ncomp slot, not the (N, z, b) of slots at or beyond the active count."""
    nc = mdr.row_parameters(prob, p, jax)[2]
    mv = np.ones(prob.ndim, dtype=bool)
    mv[prob.startind] = False
    mv[prob.startind + 1 + 3 * nc:prob.endind] = False
    return mv


def clamp(v, lo, hi):
    """min(max(v, lo), hi) that keeps a NaN."""
    return np.where(v < lo, lo, np.where(v > hi, hi, v))


def point(prob, p, jax=False):
    """(logL, G, J^T W J) at one parameter vector; G and the matrix are None where logL is not finite."""
    logl = o.jax_loglike_f64(prob, p) if jax else o.lnlhood_worker(prob, p)
    if not np.isfinite(logl):
        return logl, None, None
    m, J = mdr.model_jacobian(prob, p, jax)
    W = mdr.kept_weights(prob)
    q = np.where(W > 0, W * (prob.flux - m), 0.0)
    return logl, J.T @ q, J.T @ (W[:, None] * J)


def cg(A, g, lam, iters):
    """`iters` CG iterations on (A + lam I) x = g from x = 0 with the fit's two stopping rules; (x, iterations done)."""
    x = np.zeros_like(g)
    r = g.copy()
    p = g.copy()
    rr = gg = float(r @ r)
    for it in range(iters):
        Ap = A @ p + lam * p
        pAp = float(p @ Ap)
        if not pAp > 0:
            return x, it
        alpha = rr / pAp
        x = x + alpha * p
        r = r - alpha * Ap
        rrn = float(r @ r)
        if rrn <= CG_TOL * gg:
            return x, it + 1
        p = r + (rrn / rr) * p
        rr = rrn
    return x, iters


def pins(prob, th, G, lo, hi, jax=False):
    return ~movable(prob, th, jax) | ~(hi - lo > 0) | ((th <= lo) & (G < 0)) | ((th >= hi) & (G > 0))


def maximize_row(prob, p0, lo, hi, max_iter=50, cg_iters=None, lambda0=1e-3, ftol=1e-10, jax=False, trace=None):
    """(p, logL, status, niter) of one start.  `trace` (a list) receives one dict per outer iteration: the point before,
    the pins, x, the trial point, both logL, whether the step was accepted, lambda after."""
    p0 = np.asarray(p0, dtype=float)
    s = hi - lo
    cg_iters = prob.ndim if not cg_iters else cg_iters
    th = np.where(movable(prob, p0, jax), clamp(p0, lo, hi), p0)
    with np.errstate(all="ignore"):
        logl, G, F = point(prob, th, jax)
    if not np.isfinite(logl) or np.isnan(p0[movable(prob, p0, jax)]).any():
        return p0.copy(), logl, -1, 0
    lam, status, niter = lambda0, 0, 0
    for _ in range(max_iter):
        pin = pins(prob, th, G, lo, hi, jax)
        gu = np.where(pin, 0.0, s * G)
        if not gu @ gu > 0:
            status = 2
            break
        niter += 1
        A = s[:, None] * F * s[None, :]
        A[pin, :] = 0.0
        A[:, pin] = 0.0
        x, _ = cg(A, gu, lam, cg_iters)
        T = np.where(pin, th, clamp(th + s * x, lo, hi))
        lt, GT, FT = point(prob, T, jax)
        ok = bool(np.isfinite(lt) and lt > logl)
        rec = dict(theta=th.copy(), pin=pin.copy(), x=x.copy(), T=T.copy(), logL=logl, logL_T=lt, accepted=ok)
        if ok:
            gain = lt - logl
            th, logl, G, F = T, lt, GT, FT
            lam = max(lam / 10.0, LAMBDA_MIN)
            if gain <= ftol * (1.0 + abs(lt)):
                status = 1
        else:
            lam = 10.0 * lam
            if lam > LAMBDA_MAX:
                status = 3
        rec["lam"] = lam
        rec["after"] = th.copy()
        if trace is not None:
            trace.append(rec)
        if status:
            break
    return th, logl, status, niter


def maximize_batch(prob, P0, lo, hi, **kw):
    rows = [maximize_row(prob, p, lo, hi, **kw) for p in np.asarray(P0, dtype=float)]
    return (np.array([r[0] for r in rows]), np.array([r[1] for r in rows]), np.array([r[2] for r in rows], dtype=np.int32),
            np.array([r[3] for r in rows], dtype=np.int32))


# ---- the problem of the convergence tests (CPU: tests/test_fit_reference.py, GPU: tests/test_gpu_fit.py) -----------------

CIV = [(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8)]
TRUTH = np.array([3.0, 13.6, 3.0000, 15.0, 13.2, 3.0012, 25.0, 13.0, 3.0025, 20.0])


def convergence_kwargs():
    """als_fitter kwargs: 300 pixels of 6188-6212 A, CIV 1548 / 1550, ncomp [2, 3], R = 8 fixed, sigma 0.02; the data are the
    oracle's model of TRUTH plus default_rng(1) noise; box N [12.5, 14.5], z [2.998, 3.004], b [8, 40]."""
    wl = np.linspace(6188.0, 6212.0, 300)
    err = np.full(wl.size, 0.02)
    kw = dict(fitrange=[[6187.9, 6212.1]], fitlines=["CIV 1548", "CIV 1550"], linepars=CIV, ncomp=[2, 3], nfill=0, specres=[8.0],
              contval=[1.0], Nrange=[12.5, 14.5], brange=[8.0, 40.0], zrange=[2.998, 3.004], spectrum=(wl, np.ones(wl.size), err))
    import cases
    flux = cases.oracle_synth(kw, TRUTH) + np.random.default_rng(1).normal(0.0, 0.02, wl.size)
    return dict(kw, spectrum=(wl, flux, err))


def convergence_starts():
    """Six starts: TRUTH +- (0.2 dex, 1e-4, 4 km/s) uniform, default_rng(2)."""
    rng = np.random.default_rng(2)
    P = np.tile(TRUTH, (6, 1))
    P[:, 1:] += rng.uniform(-1.0, 1.0, (6, 9)) * np.tile([0.2, 1e-4, 4.0], 3)
    return P


def scipy_optimum(prob, p0, lo, hi):
    """scipy.optimize.least_squares (trf, analytic Jacobian, tolerances 1e-15) on sqrt(W) (d - m) over the movable coordinates
    of `p0`, inside the same box, x_scale = hi - lo: (p, logL)."""
    from scipy.optimize import least_squares
    p0 = np.asarray(p0, dtype=float)
    free = np.flatnonzero(movable(prob, p0) & (hi - lo > 0))
    sw = np.sqrt(mdr.kept_weights(prob))
    flux = np.where(sw > 0, prob.flux, 0.0)

    def full(x):
        p = p0.copy()
        p[free] = x
        return p

    def res(x):
        return sw * (flux - np.where(sw > 0, mdr.model_jacobian(prob, full(x))[0], 0.0))

    def jac(x):
        return -sw[:, None] * mdr.model_jacobian(prob, full(x))[1][:, free]

    sol = least_squares(res, np.clip(p0[free], lo[free], hi[free]), jac=jac, bounds=(lo[free], hi[free]), method="trf",
                        x_scale=(hi - lo)[free], ftol=1e-15, xtol=1e-15, gtol=1e-15, max_nfev=2000)
    p = full(sol.x)
    return p, o.lnlhood_worker(prob, p)
