"""Test-side reference for the ensemble sampler (mcalf_ensemble_batch): float64 numpy restatements of the fixed-sequence
logarithm, of both moves, of the decide rule, of the chain and of the continuation of include/mcalf_hip.h, with logL passed in
as a callable.  Philox4x64-10 is ns_reference's.

Only +, -, x, / and compare are used on the proposal, in `ln` and in the accept rule, each as one numpy ufunc call (one
correctly rounded IEEE operation, no FMA), so a run computed here equals the device's bit for bit wherever `logL` returns the
bits the device's decisions saw."""
import numpy as np

from ns_reference import philox4x64

STRETCH, DE = 0, 1
SQRT2 = float.fromhex("0x1.6a09e667f3bcdp+0")
LN2_HI, LN2_LO = float.fromhex("0x1.62e42feep-1"), float.fromhex("0x1.a39ef35793c76p-33")
LN_TERMS = 9
_U = np.uint64


def ln(x):
    """The library's logarithm of normal positive doubles (include/mcalf_hip.h), operation for operation."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    b = x.view(np.int64)
    e = ((b >> np.int64(52)) & np.int64(0x7FF)) - np.int64(1023)
    f = ((b & np.int64(0x000FFFFFFFFFFFFF)) | np.int64(0x3FF0000000000000)).view(np.float64)
    big = f > SQRT2
    f = np.where(big, f * 0.5, f)
    e = e + big
    r = (f - 1.0) / (f + 1.0)
    s = r * r
    p = np.full_like(s, 1.0 / (2 * LN_TERMS + 1))
    for i in range(LN_TERMS - 1, 0, -1):
        p = p * s + 1.0 / (2 * i + 1)
    t = r + r
    lnf = t + (t * s) * p
    ed = e.astype(np.float64)
    return ed * LN2_HI + (lnf + ed * LN2_LO)


def words(s, w, seed):
    """The block [len(w), 4] of global half-step `s` for the walkers `w`: what numpy's Philox(counter=[s, 0, w, 0],
    key=[seed, 1]) returns first, which is the Philox function at counter (s + 1, 0, w, 0) -- numpy's generator advances its
    counter before it draws."""
    w = np.asarray(w, dtype=np.uint64).reshape(-1)
    counter = np.zeros((w.size, 4), dtype=np.uint64)
    counter[:, 0] = _U((int(s) + 1) & 0xFFFFFFFFFFFFFFFF)
    counter[:, 2] = w
    return philox4x64(counter, np.array([int(seed) & 0xFFFFFFFFFFFFFFFF, 1], dtype=np.uint64))


def default_scale(move, ndim):
    return 2.0 if move == STRETCH else 2.38 / np.sqrt(2.0 * ndim)


def propose(U, h, s, move, scale, seed, status=None):
    """The proposals of half-step `h` (global number `s`) over the state `U` [n, ndim]: (Y [m, ndim], hastings [m],
    lnzeta [m], inside [m], partners [m, 1 or 2], raw [m, ndim]).  Walkers with status != 0 do not move (inside is False); a
    row of Y that is not inside holds the walker's own point, `raw` the proposal as computed."""
    n, ndim = U.shape
    m = n // 2
    mov = np.arange(h * m, (h + 1) * m)
    other = (1 - h) * m
    blk = words(s, mov, seed)
    w0, w1, w2, w3 = (blk[:, i] for i in range(4))
    xi = (w1 >> _U(11)).astype(np.float64) * 2.0 ** -53
    zeta = ((w2 >> _U(11)) + _U(1)).astype(np.float64) * 2.0 ** -53
    x = U[mov]
    with np.errstate(invalid="ignore", over="ignore"):
        if move == STRETCH:
            j = other + (w0 % _U(m)).astype(np.int64)
            t = (scale - 1.0) * xi + 1.0
            z = (t * t) / scale
            hastings = float(ndim - 1) * ln(z)
            xj = U[j]
            Y = xj + z[:, None] * (x - xj)
            partners = j[:, None]
        else:
            j1 = w0 % _U(m)
            j2 = (j1 + _U(1) + w3 % _U(m - 1)) % _U(m)
            j1, j2 = other + j1.astype(np.int64), other + j2.astype(np.int64)
            gamma = scale * (1.0 + 1e-5 * (2.0 * xi - 1.0))
            hastings = np.zeros(m)
            Y = x + gamma[:, None] * (U[j1] - U[j2])
            partners = np.stack([j1, j2], axis=1)
        inside = ((Y >= 0.0) & (Y <= 1.0)).all(axis=1)
    if status is not None:
        inside &= status[mov] == 0
    return np.where(inside[:, None], Y, x), hastings, ln(zeta), inside, partners, Y


def ensemble(logL, U0, nsteps, thin=1, move=STRETCH, scale=None, seed=0, first_iter=0, trace=None):
    """(U, logL, status, naccept, CU, CL) of mcalf_ensemble_batch; `logL(U)` -> [rows] evaluates rows of the unit cube (the n
    starts once, then the m trial rows of every half-step, as the device does).  `trace` (a list) receives (h, moving walkers,
    partners) of every half-step."""
    U0 = np.array(U0, dtype=float, ndmin=2)
    n, ndim = U0.shape
    assert n % 2 == 0 and n >= 4
    m = n // 2
    scale = default_scale(move, ndim) if scale is None else float(scale)
    U = U0.copy()
    L = np.array(logL(U), dtype=float).reshape(n)
    with np.errstate(invalid="ignore"):
        status = np.where(((U0 >= 0.0) & (U0 <= 1.0)).all(axis=1), 0, -1).astype(np.int32)
    naccept = np.zeros(n, dtype=np.int32)
    nkeep = nsteps // thin
    CU, CL = np.empty((nkeep, n, ndim)), np.empty((nkeep, n))
    for i in range(nsteps):
        for h in (0, 1):
            mov = np.arange(h * m, (h + 1) * m)
            Y, hastings, lnzeta, inside, partners, _ = propose(U, h, 2 * (first_iter + i) + h, move, scale, seed, status)
            if trace is not None:
                trace.append((h, mov, partners))
            LY = np.array(logL(Y), dtype=float).reshape(m)
            with np.errstate(invalid="ignore"):
                d = LY - L[mov]
                q = hastings + d if move == STRETCH else d
                acc = inside & (lnzeta < q)
            U[mov[acc]], L[mov[acc]] = Y[acc], LY[acc]
            naccept[mov[acc]] += 1
        if (i + 1) % thin == 0:
            CU[(i + 1) // thin - 1], CL[(i + 1) // thin - 1] = U, L
    return U, L, status, naccept, CU, CL


def advance_with(logL, move=STRETCH, scale=None, transform=None):
    """The `advance` callable of `ensemble.ensemble_sample` around `ensemble`; theta = transform(U) (None: U itself)."""
    def advance(U0, nsteps, thin=1, seed=0, first_iter=0, chain=True):
        U, L, status, naccept, CU, CL = ensemble(logL, U0, nsteps, thin, move, scale, seed, first_iter)
        theta = U.copy() if transform is None else transform(U)
        return (U, theta, L, status, naccept) + ((CU, CL) if chain else (None, None))
    return advance
