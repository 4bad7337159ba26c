"""Test-side reference for the tempered ensemble sampler (mcalf_tempered_batch): a float64 numpy restatement of the state
machine of include/mcalf_hip.h on top of ens_reference.py -- the within-temperature half-step with the tempered accept rule,
the swap rounds, the chain and the continuation -- with logL passed in as a callable.

As in ens_reference.py every operation of the accept rules is one numpy ufunc call (one correctly rounded IEEE operation, no
FMA), so a run computed here equals the device's bit for bit wherever `logL` returns the bits the device's decisions saw."""
import numpy as np

import ens_reference as er
from ns_reference import philox4x64

STRETCH, DE = er.STRETCH, er.DE
_U = np.uint64
_MASK = 0xFFFFFFFFFFFFFFFF


def _block(c0, c1, c2, seed):
    """The blocks [len(c2), 4] numpy's Philox(counter=[c0, c1, c2, 0], key=[seed, 2]) returns first: the function at counter
    (c0 + 1, c1, c2, 0)."""
    c2 = np.asarray(c2, dtype=np.uint64).reshape(-1)
    counter = np.zeros((c2.size, 4), dtype=np.uint64)
    counter[:, 0] = _U((int(c0) + 1) & _MASK)
    counter[:, 1] = _U(c1)
    counter[:, 2] = c2
    return philox4x64(counter, np.array([int(seed) & _MASK, 2], dtype=np.uint64))


def swap_pairs(r, T):
    """The lower temperatures t of the pairs (t, t + 1) of swap round `r`."""
    return list(range(int(r) % 2, T - 1, 2))


def swap_shift(r, t, n, seed):
    """The shift c of pair `t` in round `r`: position (t, w) meets position (t + 1, (w + c) mod n)."""
    return int(_block(r, 1, [t], seed)[0, 0] % _U(n))


def swap_partners(r, t, n, seed):
    w = np.arange(n, dtype=np.int64)
    return (w + swap_shift(r, t, n, seed)) % n


def swap_zeta(r, t, n, seed):
    """zeta [n] of the positions (t, w) in round `r`."""
    blk = _block(r, 0, t * n + np.arange(n), seed)
    return ((blk[:, 2] >> _U(11)) + _U(1)).astype(np.float64) * 2.0 ** -53


def swap_round(U, L, status, nswap, beta, r, seed, trace=None):
    """Swap round `r` on the state U [T, n, ndim], L [T, n] in place; nswap [T - 1, n] counts.  `trace` (a list) receives
    (t, partners [n], zeta [n], accepted [n]) of every pair.  (The words of all pairs are drawn in two calls: swap_shift and
    swap_zeta, pair by pair, give the same.)"""
    T, n = L.shape
    pairs = swap_pairs(r, T)
    if not pairs:
        return
    w = np.arange(n, dtype=np.int64)
    shifts = (_block(r, 1, pairs, seed)[:, 0] % _U(n)).astype(np.int64)
    rows = (np.array(pairs, dtype=np.int64)[:, None] * n + w).reshape(-1)
    zetas = (((_block(r, 0, rows, seed)[:, 2] >> _U(11)) + _U(1)).astype(np.float64) * 2.0 ** -53).reshape(len(pairs), n)
    lnzetas = er.ln(zetas)
    for p, t in enumerate(pairs):
        j = (w + shifts[p]) % n
        with np.errstate(invalid="ignore"):
            db = beta[t] - beta[t + 1]
            dl = L[t + 1][j] - L[t]
            q = db * dl
            acc = (status[t] == 0) & (status[t + 1][j] == 0) & (lnzetas[p] < q)
        k = np.flatnonzero(acc)
        x, lx = U[t, k].copy(), L[t, k].copy()
        U[t, k], L[t, k] = U[t + 1, j[k]], L[t + 1, j[k]]
        U[t + 1, j[k]], L[t + 1, j[k]] = x, lx
        nswap[t, k] += 1
        if trace is not None:
            trace.append((t, j, zetas[p], acc))


def tempered(logL, U0, beta, nsteps, thin=1, swap_every=1, move=STRETCH, scale=None, seed=0, first_iter=0, chain_temps=1, trace=None):
    """(U, logL, status, naccept, nswap, CU, CL) of mcalf_tempered_batch for the starts U0 [T, n, ndim]; `logL(U)` -> [rows]
    evaluates rows of the unit cube (the T n starts once, then the T m trial rows of every half-step, as the device does).
    `trace`: the swap rounds' (see swap_round), each preceded by ("round", r)."""
    U0 = np.array(U0, dtype=float)
    beta = np.array(beta, dtype=float).reshape(-1)
    T, n, ndim = U0.shape
    assert T == beta.size and n % 2 == 0 and n >= 4 and 0 <= chain_temps <= T
    m = n // 2
    scale = er.default_scale(move, ndim) if scale is None else float(scale)
    U = U0.copy()
    L = np.array(logL(U.reshape(T * n, ndim)), dtype=float).reshape(T, n)
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
            s = 2 * g + h
            mov = np.arange(h * m, (h + 1) * m)
            Y, hastings, lnzeta, inside = (v.reshape((T, m) + v.shape[1:]) for v in propose(flat, flat_status, T, h, s, move, scale, seed))
            LY = np.array(logL(Y.reshape(T * m, ndim)), dtype=float).reshape(T, m)
            with np.errstate(invalid="ignore"):
                d = LY - L[:, mov]
                bd = beta[:, None] * d
                q = hastings + bd if move == STRETCH else bd
                acc = inside & (lnzeta < q)
            for t in range(T):
                U[t, mov[acc[t]]], L[t, mov[acc[t]]] = Y[t, acc[t]], LY[t, acc[t]]
                naccept[t, mov[acc[t]]] += 1
        if swap_every > 0 and (g + 1) % swap_every == 0:
            r = (g + 1) // swap_every - 1
            if trace is not None:
                trace.append(("round", r))
            swap_round(U, L, status, nswap, beta, r, seed, trace)
        if (i + 1) % thin == 0:
            CU[(i + 1) // thin - 1], CL[(i + 1) // thin - 1] = U[:chain_temps], L
    return U, L, status, naccept, nswap, CU, CL


def propose(flat, flat_status, T, h, s, move, scale, seed):
    """ens_reference.propose for every temperature at once over the rows `flat` [T n, ndim]: (Y [T m, ndim], hastings,
    lnzeta, inside [T m]).  Moving row t n + h m + b draws the words of its row number and partners from the other half of
    its own temperature."""
    ndim = flat.shape[1]
    n = flat.shape[0] // T
    m = n // 2
    base = np.repeat(np.arange(T, dtype=np.int64) * n, m)
    mov = base + h * m + np.tile(np.arange(m, dtype=np.int64), T)
    other = base + (1 - h) * m
    blk = er.words(s, mov, seed)
    w0, w1, w2, w3 = (blk[:, i] for i in range(4))
    xi = (w1 >> _U(11)).astype(np.float64) * 2.0 ** -53
    zeta = ((w2 >> _U(11)) + _U(1)).astype(np.float64) * 2.0 ** -53
    x = flat[mov]
    with np.errstate(invalid="ignore", over="ignore"):
        if move == STRETCH:
            xj = flat[other + (w0 % _U(m)).astype(np.int64)]
            t1 = (scale - 1.0) * xi + 1.0
            z = (t1 * t1) / scale
            hastings = float(ndim - 1) * er.ln(z)
            Y = xj + z[:, None] * (x - xj)
        else:
            j1 = w0 % _U(m)
            j2 = (j1 + _U(1) + w3 % _U(m - 1)) % _U(m)
            gamma = scale * (1.0 + 1e-5 * (2.0 * xi - 1.0))
            hastings = np.zeros(T * m)
            Y = x + gamma[:, None] * (flat[other + j1.astype(np.int64)] - flat[other + j2.astype(np.int64)])
        inside = ((Y >= 0.0) & (Y <= 1.0)).all(axis=1) & (flat_status[mov] == 0)
    return np.where(inside[:, None], Y, x), hastings, er.ln(zeta), inside


def advance_with(logL, beta, move=STRETCH, scale=None, transform=None):
    """The `advance` callable of `tempering.tempered_sample` around `tempered`; theta = transform(U) (None: U itself)."""
    def advance(U0, nsteps, thin=1, swap_every=1, seed=0, first_iter=0, chain=True, chain_temps=1):
        U, L, status, naccept, nswap, CU, CL = tempered(logL, U0, beta, nsteps, thin, swap_every, move, scale, seed, first_iter, chain_temps)
        theta = U.copy() if transform is None else transform(U)
        return (U, theta, L, status, naccept, nswap) + ((CU, CL) if chain else (None, None))
    return advance
