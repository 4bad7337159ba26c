"""Test-side reference for the model Jacobian's products with a vector (mcalf_model_jvp_batch / mcalf_model_vjp_batch):
float64 numpy, the dense J[npix, ndim] = d m / d theta of ONE row, built from the gradient reference's own pieces
(tests/grad_reference.py: `_line_parts`, `_taps`, `_circular`) and the oracle's convolutions.

With F = exp(-sum tau) and m = cont L(F):
    J[:, R] = cont (dL/dR)(F),   J[:, cont] = L(F),   J[:, col] = -cont L(F dtau/dtheta_col)   for an active (N, z, b)
and 0 for the ncomp slot, the (N, z, b) of components at or beyond the row's active count, and R where R <= velstep.
L is the context's convolution (periodic with the astropy tap count held at the row's value on the numpy path, the
fixed grid with the edge reset on the JAX path).  The products and the scales the GPU tests measure errors against:
    jvp: J v,   S_i = sum_k |v_k J_ik|          vjp: J^T q,   S_k = sum_i |q_i J_ik|."""
import numpy as np

import grad_reference as gr
from oracle import numpy_oracle as o


def row_parameters(prob, p, jax=False):
    """(R, cont, active components) of a parameter vector, as grad_reference.grad_row decodes them."""
    s = prob.startind
    if jax:
        R = p[0] if prob.freespecres else float(prob.specres[0])
        nc_raw = np.floor(p[s])
    else:
        R = p[0] if prob.freespecres else float(max(prob.specres))
        nc_raw = np.trunc(p[s])
    cont = (p[1] if prob.freespecres else p[0]) if prob.freecont else float(prob.contval[0])
    return R, cont, int(min(max(nc_raw, 0), prob.ncompmax))


def model_jacobian(prob, p, jax=False):
    """(m[npix], J[npix, ndim]) of one parameter vector in float64."""
    p = np.asarray(p, dtype=float)
    s = prob.startind
    R, cont, nc = row_parameters(prob, p, jax)
    tau = np.zeros_like(prob.wl)
    dtau = {}
    slots = [(1 + 3 * c + s, prob.lines) for c in range(nc)] + [(prob.endind + 3 * k, [prob.linefill]) for k in range(prob.nfill)]
    for col, lines in slots:
        logN, z, b = p[col:col + 3]
        acc = [np.zeros_like(prob.wl) for _ in range(3)]
        for line in lines:
            parts = gr._line_parts(prob, prob.wl, logN, z, b, line)
            tau += parts[0]
            for j in range(3):
                acc[j] += parts[1 + j]
        for j in range(3):
            dtau[col + j] = acc[j]
    F = np.exp(-tau)

    w, dw = gr._taps(prob, R, jax)
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

        LRF = gr._circular(F, dw)
    else:
        def L(x):
            return x

        LRF = np.zeros_like(F)

    LF = L(F)
    J = np.zeros((F.size, prob.ndim))
    if prob.freespecres:
        J[:, 0] = cont * LRF
    if prob.freecont:
        J[:, 1 if prob.freespecres else 0] = LF
    for col, d in dtau.items():
        J[:, col] = -cont * L(F * d)
    return cont * LF, J


def jvp(J, v):
    """(J v, S[npix]) for one tangent."""
    terms = J * np.asarray(v, dtype=float)[None, :]
    return terms.sum(axis=1), np.abs(terms).sum(axis=1)


def vjp(J, q):
    """(J^T q, S[ndim]) for one cotangent."""
    terms = J * np.asarray(q, dtype=float)[:, None]
    return terms.sum(axis=0), np.abs(terms).sum(axis=0)


def kept_weights(prob):
    """W of the Fisher product: 1/err^2 on the pixels whose logL term np.nansum keeps, 0 elsewhere."""
    with np.errstate(divide="ignore", invalid="ignore"):
        w = 1.0 / prob.err ** 2
        term = w * prob.flux ** 2 - np.log(w)
    return np.where(np.isnan(term), 0.0, w)


def tangent_scales(prob):
    """Per-column sizes of a test tangent: 1 for R, the continuum (and the ignored ncomp slot), 0.3 / 2e-5 / 3 for
    logN / z / b -- a step that moves every kind of parameter by a comparable fraction of its range."""
    sc = np.ones(prob.ndim)
    for col in list(range(prob.startind + 1, prob.endind, 3)) + list(range(prob.endind, prob.ndim, 3)):
        sc[col:col + 3] = (0.3, 2e-5, 3.0)
    return sc
