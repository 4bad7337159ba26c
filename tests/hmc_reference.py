"""Test-side reference for Hamiltonian Monte Carlo (mcalf_hmc_batch): a float64 numpy restatement of the fixed sequence of
include/mcalf_hip.h -- the decision words, the polar normals, the leapfrog steps with their one reflection, the dead
trajectories, the accept rule, the chain and the continuation -- with the gradient passed in as a callable
`grad(theta) -> (logL [n], G [n, ndim])`.  Philox4x64-10 is ns_reference's, `ln` is ens_reference's, the lane sums and the
butterfly are prior_reference's.

One numpy ufunc call per operation (one correctly rounded IEEE operation, no FMA; np.sqrt is correctly rounded), so a run
computed here equals the device's bit for bit wherever `grad` returns the bits the device's kernels saw."""
import numpy as np

import prior_reference as pr
from ens_reference import ln
from ns_reference import philox4x64

KEY = 4
DECISION = 1 << 63
ATTEMPTS = 16
WAVE = pr.WAVE
_U = np.uint64
_M64 = 0xFFFFFFFFFFFFFFFF


def _key(seed):
    return np.array([int(seed) & _M64, KEY], dtype=np.uint64)


def _x(word):
    return (word >> _U(11)).astype(np.float64) * 2.0 ** -53


def decision(g, wid, seed):
    """(xi, zeta) [n] of global iteration `g` for the walker ids `wid`: the block at counter (g + 1, 2^63, w, 0)."""
    wid = np.asarray(wid, dtype=np.uint64).reshape(-1)
    counter = np.zeros((wid.size, 4), dtype=np.uint64)
    counter[:, 0] = _U((int(g) + 1) & _M64)
    counter[:, 1] = _U(DECISION)
    counter[:, 2] = wid
    blk = philox4x64(counter, _key(seed))
    return _x(blk[:, 1]), ((blk[:, 2] >> _U(11)) + _U(1)).astype(np.float64) * 2.0 ** -53


def normals(g, wid, coords, seed, attempts=ATTEMPTS):
    """Standard normals [n, len(coords)] of global iteration `g` for the walker ids `wid` and the coordinates `coords`, by
    Marsaglia's polar method: the first candidate pair with 0 < q < 1 among the blocks of attempts 0 .. 15, else 0."""
    wid = np.asarray(wid, dtype=np.uint64).reshape(-1)
    coords = np.asarray(coords, dtype=np.uint64).reshape(-1)
    shape = (wid.size, coords.size)
    out, done = np.zeros(shape), np.zeros(shape, dtype=bool)
    counter = np.zeros(shape + (4,), dtype=np.uint64)
    counter[..., 0] = _U((int(g) + 1) & _M64)
    counter[..., 2] = wid[:, None]
    for att in range(attempts):
        counter[..., 1] = (_U(att) << _U(32)) | coords[None, :]
        blk = philox4x64(counter, _key(seed))
        for p in (0, 2):
            v1 = 2.0 * _x(blk[..., p]) - 1.0
            v2 = 2.0 * _x(blk[..., p + 1]) - 1.0
            q = v1 * v1 + v2 * v2
            ok = ~done & (q > 0.0) & (q < 1.0)
            qq = np.where(ok, q, 0.5)
            val = v1 * np.sqrt((-2.0 * ln(qq)) / qq)
            out = np.where(ok, val, out)
            done |= ok
        if done.all():
            break
    return out


def lane_sum(terms, cols):
    """The sum over the coordinates `cols` of terms [n, ndim] as the device takes it: lane k % 64 adds its coordinates in index
    order onto +0.0, then the xor-butterfly 32 .. 1 folds the 64 lanes."""
    acc = np.zeros((terms.shape[0], WAVE))
    for k in cols:
        acc[:, k % WAVE] = acc[:, k % WAVE] + terms[:, k]
    lanes = np.arange(WAVE)
    m = WAVE // 2
    while m > 0:
        acc = acc + acc[:, lanes ^ m]
        m >>= 1
    return acc[:, 0]


class Problem:
    """What the sequence needs to know of a context: the box, the ncomp slot and whether the cube transform truncates it, and
    the Gaussian prior (mu, sigma, c) or None.  `transform` (None: the restated cube transform) forms the theta rows of a
    launch; the GPU tests pass the library's own `scale_cube_batch`."""

    def __init__(self, lo, hi, slot, int_ncomp=True, gauss=None, transform=None):
        self.lo, self.hi = np.asarray(lo, dtype=float), np.asarray(hi, dtype=float)
        self.slot, self.int_ncomp, self.gauss, self.transform = slot, bool(int_ncomp), gauss, transform
        self.ndim = self.lo.size

    def frozen(self, scale):
        f = (self.hi == self.lo) | (np.asarray(scale, dtype=float) == 0.0)
        if self.slot is not None:
            f[self.slot] = True
        return f

    def theta(self, U):
        if self.transform is not None:
            return np.array(self.transform(U), dtype=float)
        scaled = U * (self.hi - self.lo)
        th = scaled + self.lo
        if self.int_ncomp and self.slot is not None:
            th[:, self.slot] = np.trunc(th[:, self.slot])
        return th

    def cube_grad(self, G, th):
        s = self.hi - self.lo
        g = s * G
        if self.gauss is not None:
            mu, sigma, _ = self.gauss
            for k in np.flatnonzero(np.asarray(sigma) > 0.0):
                d = (th[:, k] - mu[k]) / sigma[k]
                t = d / sigma[k]
                g[:, k] = g[:, k] - t * s[k]
        return g

    def lnprior(self, U):
        if self.gauss is None:
            return np.zeros(U.shape[0])
        mu, sigma, c = self.gauss
        return pr.lnprior(U, self.lo, self.hi, mu, sigma, c, True, self.slot)


def _finite_rows(L, g, free):
    return np.isfinite(L) & np.isfinite(g[:, free]).all(axis=1)


def leapfrog(prob, grad, x, gx, r, a, nleap, free, parked, trace=None, it=0):
    """`nleap` leapfrog steps from (x, r) with the cube gradient gx at x and the step lengths a [n, ndim], over the unfrozen
    columns `free`: (y, r, gy, LY, parked).  Rows that are `parked` on entry never move; a trajectory that dies is parked from
    that step on.  A parked row holds x in y (so every launch evaluates the walker's own point there); its r means nothing."""
    n, ndim = x.shape
    h = 0.5 * a
    y, gy, r = x.copy(), gx.copy(), r.copy()
    parked = parked.copy()
    LY = np.full(n, np.nan)
    for j in range(nleap):
        alive = ~parked
        kick = h * gy
        r[np.ix_(alive, free)] = (r + kick)[np.ix_(alive, free)]
        moved = y + a * r
        low, high = moved < 0.0, moved > 1.0
        refl = np.where(low, -moved, np.where(high, 2.0 - moved, moved))
        back = np.where(low | high, -r, r)
        if trace is not None:
            cnt = int((low | high)[np.ix_(alive, free)].sum())
            if cnt:
                trace.append(("reflect", it, j, cnt))
        y[np.ix_(alive, free)] = refl[np.ix_(alive, free)]
        r[np.ix_(alive, free)] = back[np.ix_(alive, free)]
        out = alive & ~((y[:, free] >= 0.0) & (y[:, free] <= 1.0)).all(axis=1)
        parked = parked | out
        y[parked] = x[parked]
        th = prob.theta(y)
        LY, GY = (np.array(v, dtype=float) for v in grad(th))
        LY, GY = LY.reshape(n), GY.reshape(n, ndim)
        gy = prob.cube_grad(GY, th)
        killed = ~parked & ~_finite_rows(LY, gy, free)
        if trace is not None and (out | killed).any():
            trace.append(("dead", it, j, np.flatnonzero(out | killed)))
        parked = parked | killed
        y[parked] = x[parked]
        alive = ~parked
        kick = h * gy
        r[np.ix_(alive, free)] = (r + kick)[np.ix_(alive, free)]
    return y, r, gy, LY, parked


def hmc(prob, grad, U0, nsteps, eps, nleap, scale=None, jitter=0.1, thin=1, seed=0, first_iter=0, wid=None, trace=None):
    """(U, logL, status, naccept, ndead, CU, CL) of mcalf_hmc_batch for the `Problem` prob.  `grad(theta)` evaluates the n theta
    rows of every launch, as the device does: the starts once, then the trajectories' rows of every leapfrog step (a dead
    trajectory's and a refused walker's row is the walker's own point).  `trace` (a list) receives ("reflect", iteration, step,
    count of reflected coordinates) and ("dead", iteration, step, walkers) events."""
    U0 = np.array(U0, dtype=float, ndmin=2)
    n, ndim = U0.shape
    scale = np.ones(ndim) if scale is None else np.asarray(scale, dtype=float).reshape(ndim)
    wid = np.arange(n, dtype=np.uint64) if wid is None else np.asarray(wid, dtype=np.uint64).reshape(n)
    frozen = prob.frozen(scale)
    free = np.flatnonzero(~frozen)
    eps, jitter = float(eps), float(jitter)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        U = U0.copy()
        th = prob.theta(U)
        L, G = (np.array(v, dtype=float) for v in grad(th))
        L, G = L.reshape(n), G.reshape(n, ndim)
        gx = prob.cube_grad(G, th)
        PR = prob.lnprior(U)
        inside = ((U0 >= 0.0) & (U0 <= 1.0)).all(axis=1)
        status = np.where(inside & _finite_rows(L, gx, free), 0, -1).astype(np.int32)
        naccept, ndead = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        nkeep = nsteps // thin
        CU, CL = np.empty((nkeep, n, ndim)), np.empty((nkeep, n))
        moves = status == 0
        for i in range(nsteps):
            g = first_iter + i
            xi, zeta = decision(g, wid, seed)
            e = eps * (1.0 + jitter * (2.0 * xi - 1.0))
            a = e[:, None] * scale[None, :]
            r = np.zeros((n, ndim))
            r[:, free] = normals(g, wid, free, seed)
            K0 = 0.5 * lane_sum(r * r, free)
            y, r, gy, LY, parked = leapfrog(prob, grad, U, gx, r, a, nleap, free, ~moves, trace, i)
            alive = ~parked
            K1 = 0.5 * lane_sum(np.where(alive[:, None], r * r, 0.0), free)
            PY = prob.lnprior(y) if prob.gauss is not None else np.zeros(n)
            q = ((LY + PY) - (L + PR)) + (K0 - K1)
            acc = alive & (ln(zeta) < q)
            U[acc], L[acc], gx[acc], PR[acc] = y[acc], LY[acc], gy[acc], PY[acc]
            naccept[acc] += 1
            ndead[moves & parked] += 1
            if (i + 1) % thin == 0:
                CU[(i + 1) // thin - 1], CL[(i + 1) // thin - 1] = U, L
    return U, L, status, naccept, ndead, CU, CL


def advance_with(prob, grad, nleap, jitter=0.1, transform=None):
    """The `advance` callable of `hmc.sample_with` around `hmc`; theta = transform(U) (None: prob.theta)."""
    def advance(U0, nsteps, eps, scale, thin=1, seed=0, first_iter=0, chain=True):
        U, L, status, naccept, ndead, CU, CL = hmc(prob, grad, U0, nsteps, eps, nleap, scale, jitter, thin, seed, first_iter)
        theta = prob.theta(U) if transform is None else transform(U)
        return (U, theta, L, status, naccept, ndead) + ((CU, CL) if chain else (None, None))
    return advance
