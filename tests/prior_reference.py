"""Test-side reference for the Gaussian prior (mcalf_set_gauss_prior, mcalf_lnprior_batch): a float64 numpy restatement of the
fixed sequence of include/mcalf_hip.h -- one numpy ufunc call per operation (one correctly rounded IEEE operation, no FMA), the
64 lane partial sums, then the xor-butterfly 32 .. 1 -- and the three samplers' restatements (ns_reference, ens_reference,
pt_reference) run under it.  The constants c come from the library (mcalf_get_gauss_prior), not from np.log.

Nested sampling's step constrains logL + lnprior, so it is ns_reference.slice_replace over that sum.  The ensemble's and the
ladder's accept rules have to see py - px next to an untempered logL, so `ensemble` and `tempered` restate those two drivers
here around ens_reference.propose, pt_reference.propose and pt_reference.swap_round, which are used as they are."""
import numpy as np

import ens_reference as er
import ns_reference as nr
import pt_reference as pt

STRETCH, DE = er.STRETCH, er.DE
WAVE = 64


def lnprior(rows, lo, hi, mu, sigma, c, from_cube, int_slot=None):
    """lnprior [n] of `rows` [n, ndim] as the device computes it.  mu / sigma / c None: no Gaussian (0 / -inf by the box test).
    `int_slot`: the ncomp slot, which may carry no Gaussian (its truncation therefore never enters)."""
    rows = np.array(rows, dtype=float, ndmin=2)
    lo, hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
    n, ndim = rows.shape
    with np.errstate(invalid="ignore", over="ignore"):
        if from_cube:
            bad = ~((rows >= 0.0) & (rows <= 1.0))
            scaled = rows * (hi - lo)
            theta = scaled + lo
        else:
            bad = ~((rows >= lo) & (rows <= hi))
            theta = rows
        acc = np.zeros((n, WAVE))
        if mu is not None:
            mu, sigma, c = (np.asarray(v, dtype=float) for v in (mu, sigma, c))
            assert int_slot is None or sigma[int_slot] == 0.0
            for k in range(ndim):                                # a lane adds its terms in index order onto +0.0
                if sigma[k] > 0.0:
                    d = (theta[:, k] - mu[k]) / sigma[k]
                    dd = d * d
                    s = dd + c[k]
                    term = -0.5 * s
                    acc[:, k % WAVE] = acc[:, k % WAVE] + term
        lanes = np.arange(WAVE)
        m = WAVE // 2
        while m > 0:
            acc = acc + acc[:, lanes ^ m]
            m >>= 1
    return np.where(bad.any(axis=1), -np.inf, acc[:, 0])


def plain(theta, lo, hi, mu, sigma):
    """hires_fitter.py:218-234 as written: the formula the restatement reorders."""
    theta = np.array(theta, dtype=float, ndmin=2)
    out = np.full(theta.shape[0], -np.inf)
    for i, p in enumerate(theta):
        if all(a <= v <= b for v, a, b in zip(p, lo, hi)):
            out[i] = sum(-0.5 * (((p[k] - mu[k]) / sigma[k]) ** 2 + np.log(2.0 * np.pi * sigma[k] ** 2)) for k in range(p.size) if sigma[k] > 0.0)
    return out


def slice_replace(logL, lnp, U0, Lmin, D, sid, nmoves, max_steps, seed=0):
    """ns_reference.slice_replace under the prior: `lnp(U)` -> lnprior [n] of cube rows; the returned logL is the sum."""
    return nr.slice_replace(lambda U: np.asarray(logL(U), dtype=float) + np.asarray(lnp(U), dtype=float), U0, Lmin, D, sid, nmoves, max_steps, seed)


def ensemble(logL, lnp, U0, nsteps, thin=1, move=STRETCH, scale=None, seed=0, first_iter=0):
    """ens_reference.ensemble under the prior: (U, logL, status, naccept, CU, CL, PR), logL and CL the likelihood's, PR lnprior
    of the walkers.  The accept rule: q = (hastings + (ly - lx)) + (py - px) for the stretch move, (ly - lx) + (py - px) for DE."""
    U0 = np.array(U0, dtype=float, ndmin=2)
    n, ndim = U0.shape
    out = tempered(logL, lnp, U0[None], [1.0], nsteps, thin, 0, move, scale, seed, first_iter, 1)
    U, L, status, naccept, _, CU, CL, PR = out
    return U[0], L[0], status[0], naccept[0], CU[:, 0], CL[:, 0], PR[0]


def tempered(logL, lnp, U0, beta, nsteps, thin=1, swap_every=1, move=STRETCH, scale=None, seed=0, first_iter=0, chain_temps=1):
    """pt_reference.tempered under the prior: (U, logL, status, naccept, nswap, CU, CL, PR).  The temperature acts on logL alone:
    q = (hastings + beta (ly - lx)) + (py - px); a swap's rule is pt_reference's (the prior cancels) and exchanges PR with L."""
    U0 = np.array(U0, dtype=float)
    beta = np.array(beta, dtype=float).reshape(-1)
    T, n, ndim = U0.shape
    assert T == beta.size and n % 2 == 0 and n >= 4 and 0 <= chain_temps <= T
    m = n // 2
    scale = er.default_scale(move, ndim) if scale is None else float(scale)
    U = U0.copy()
    L = np.array(logL(U.reshape(T * n, ndim)), dtype=float).reshape(T, n)
    PR = np.array(lnp(U.reshape(T * n, ndim)), dtype=float).reshape(T, n)
    with np.errstate(invalid="ignore"):
        status = np.where(((U0 >= 0.0) & (U0 <= 1.0)).all(axis=2), 0, -1).astype(np.int32)
    naccept = np.zeros((T, n), dtype=np.int32)
    nswap = np.zeros((max(T - 1, 0), n), dtype=np.int32)
    nkeep = nsteps // thin
    CU, CL = np.empty((nkeep, chain_temps, n, ndim)), np.empty((nkeep, T, n))
    flat, flat_status = U.reshape(T * n, ndim), status.reshape(T * n)      # (views: row t n + w)
    for i in range(nsteps):
        g = first_iter + i
        for h in (0, 1):
            mov = np.arange(h * m, (h + 1) * m)
            Y, hastings, lnzeta, inside = (v.reshape((T, m) + v.shape[1:]) for v in pt.propose(flat, flat_status, T, h, 2 * g + h, move, scale, seed))
            LY = np.array(logL(Y.reshape(T * m, ndim)), dtype=float).reshape(T, m)
            PY = np.array(lnp(Y.reshape(T * m, ndim)), dtype=float).reshape(T, m)
            with np.errstate(invalid="ignore"):
                d = LY - L[:, mov]
                bd = beta[:, None] * d
                q = hastings + bd if move == STRETCH else bd
                dp = PY - PR[:, mov]
                q = q + dp
                acc = inside & (lnzeta < q)
            for t in range(T):
                U[t, mov[acc[t]]], L[t, mov[acc[t]]], PR[t, mov[acc[t]]] = Y[t, acc[t]], LY[t, acc[t]], PY[t, acc[t]]
                naccept[t, mov[acc[t]]] += 1
        if swap_every > 0 and (g + 1) % swap_every == 0:
            trace = []
            pt.swap_round(U, L, status, nswap, beta, (g + 1) // swap_every - 1, seed, trace)
            for t, j, _, accepted in trace:                      # the rows that changed places take their lnprior along
                k = np.flatnonzero(accepted)
                low = PR[t, k].copy()
                PR[t, k] = PR[t + 1, j[k]]
                PR[t + 1, j[k]] = low
        if (i + 1) % thin == 0:
            CU[(i + 1) // thin - 1], CL[(i + 1) // thin - 1] = U[:chain_temps], L
    return U, L, status, naccept, nswap, CU, CL, PR


def truncated_normal_cdf(x, mu, sigma, lo=0.0, hi=1.0):
    """Distribution function of N(mu, sigma^2) truncated to [lo, hi] at the points x, by math.erf."""
    import math
    phi = lambda v: 0.5 * (1.0 + math.erf((v - mu) / (sigma * math.sqrt(2.0))))
    a, b = phi(lo), phi(hi)
    return np.array([(phi(float(v)) - a) / (b - a) for v in np.asarray(x, dtype=float).reshape(-1)])


def ks_against(x, cdf):
    """Kolmogorov-Smirnov distance of the sample x [n] from the distribution function `cdf`."""
    x = np.sort(np.asarray(x, dtype=float))
    n = x.size
    F = cdf(x)
    grid = np.arange(1, n + 1) / n
    return float(max((grid - F).max(), (F - (grid - 1.0 / n)).max()))
