"""Test-side reference for the device-resident nested-sampling run (mcalf_nested_*): the numpy restatement of its rounds as
include/mcalf_hip.h states them -- stable rank, select, the Philox picks and stream ids, the replacement through
`ns_reference.slice_replace` with a logL callable, retire -- and of the evidence as nested.py computes it.  The direction rows of
a round come from a callable (default: `nested.directions`); the GPU tests pass the device's own D of each round instead, so that
every other step is compared exactly."""
import numpy as np

import ns_reference as nr
from mcalf_amd import nested

BUDGET, CONVERGED, PLATEAU, FULL = 0, 1, 2, 3


def key(L):
    return np.where(np.isnan(L), -np.inf, L)


def picks(seed, rnd, K, nstarts):
    """w0 mod nstarts of the blocks at counter (rnd + 1, 0, j, 0), key (seed, 3), j = 0 .. K - 1."""
    counter = np.zeros((K, 4), dtype=np.uint64)
    counter[:, 0] = np.uint64(rnd + 1)
    counter[:, 2] = np.arange(K, dtype=np.uint64)
    w0 = nr.philox4x64(counter, np.array([int(seed) & 0xFFFFFFFFFFFFFFFF, 3], dtype=np.uint64))[:, 0]
    return (w0 % np.uint64(nstarts)).astype(np.int64)


def select(L, K, seed, rnd):
    """(order, dying, lmin, r0, pick) of a round; pick is None on a plateau."""
    k = key(np.asarray(L, dtype=float))
    order = np.argsort(k, kind="stable")
    dying = order[:K]
    lmin = float(k[dying[-1]])
    r0 = int((k <= lmin).sum())
    nstarts = k.size - r0
    pick = order[r0 + picks(seed, rnd, K, nstarts)] if nstarts > 0 else None
    return order, dying, lmin, r0, pick


class Evidence:
    """nested.py's `die` and the tail of its `nested_sample`."""

    def __init__(self):
        self.logX, self.logZ, self.lw = 0.0, -np.inf, []

    def die(self, keys, n_first):
        n = n_first - np.arange(keys.size, dtype=float)
        lx = self.logX + np.concatenate([[0.0], np.cumsum(-1.0 / n)])
        lw = lx[:-1] + np.log(-np.expm1(-1.0 / n)) + keys
        self.logX = float(lx[-1])
        self.logZ = float(np.logaddexp(self.logZ, np.logaddexp.reduce(lw)))
        self.lw.append(lw)

    def converged(self, max_key, dlogz):
        with np.errstate(divide="ignore"):
            return self.logZ > -np.inf and max_key + self.logX < np.log(dlogz) + self.logZ

    def margin(self, max_key, dlogz):
        """How far the stop test is from flipping (inf while it cannot hold)."""
        with np.errstate(divide="ignore"):
            return abs(max_key + self.logX - np.log(dlogz) - self.logZ) if self.logZ > -np.inf and dlogz > 0 else np.inf


def finish(logL, nlive, K):
    """(logZ, H, logw) over the dead logL of a whole run (rounds of K, then the last nlive)."""
    logL = np.asarray(logL, dtype=float)
    ev = Evidence()
    rounds = (logL.size - nlive) // K
    for r in range(rounds):
        ev.die(key(logL[r * K:(r + 1) * K]), nlive)
    ev.die(key(logL[rounds * K:]), nlive)
    lw = np.concatenate(ev.lw)
    logZ = float(np.logaddexp.reduce(lw))
    logw = lw - logZ
    p = np.exp(logw)
    pos = p > 0.0
    return logZ, float(np.sum(p[pos] * (key(logL)[pos] - logZ))), logw


class Run:
    """The run, round by round.  `logl(U) -> [n]` evaluates cube rows (under a Gaussian prior: logL + lnprior); `init(U) -> [n]`
    (None: `logl`) gives the initial points' values.  `dirs(U_alive) -> D` makes a round's direction rows."""

    def __init__(self, logl, U0, K, nmoves, max_steps, seed=0, dlogz=1e-3, max_dead=None, dirs=nested.directions, init=None):
        self.logl, self.K, self.nmoves, self.max_steps, self.seed, self.dlogz, self.dirs = logl, int(K), int(nmoves), int(max_steps), seed, dlogz, dirs
        self.U = np.array(U0, dtype=float)
        self.nlive, self.ndim = self.U.shape
        self.L = np.array((init or logl)(self.U), dtype=float).reshape(self.nlive)
        self.max_dead = self.nlive + self.K * 10 ** 9 if max_dead is None else int(max_dead)
        self.nevals, self.unfinished, self.rounds, self.ndead = self.nlive, 0, 0, 0
        self.ev = Evidence()
        self.dead_u, self.dead_l = [], []
        self.last = None                                  # (dying, pick, D, lmin) of the last round
        self.margins = []

    def advance(self, max_rounds, D_of_round=None):
        """Rounds until a reason to stop, as mcalf_nested_advance tests them; returns the reason."""
        done = 0
        while True:
            mk = float(key(self.L).max())
            if self.ev.converged(mk, self.dlogz):
                return CONVERGED
            if self.ndead + self.K + self.nlive > self.max_dead:
                return FULL
            if done >= max_rounds:
                return BUDGET
            self.margins.append(self.ev.margin(mk, self.dlogz))
            order, dying, lmin, r0, pick = select(self.L, self.K, self.seed, self.rounds)
            if pick is None:
                self.last = (dying, None, None, lmin)
                return PLATEAU
            D = self.dirs(self.U[order[self.K:]]) if D_of_round is None else D_of_round(self.rounds)
            sid = np.arange(self.rounds * self.K, (self.rounds + 1) * self.K, dtype=np.uint64)
            Un, Ln, status, ne, _ = nr.slice_replace(self.logl, self.U[pick], np.full(self.K, lmin), D, sid, self.nmoves, self.max_steps, self.seed)
            assert (status >= 0).all() and (Ln > lmin).all()
            self.ev.die(key(self.L[dying]), self.nlive)
            self.dead_u.append(self.U[dying].copy()); self.dead_l.append(self.L[dying].copy())
            self.U[dying], self.L[dying] = Un, Ln
            self.unfinished += int((status == 0).sum())
            self.nevals += int(ne.sum())
            self.ndead += self.K
            self.rounds += 1
            self.last = (dying, pick, D, lmin)
            done += 1

    def finish(self):
        """(logZ, H, logw, cube, logL) with the remaining live points retired in key order."""
        order = np.argsort(key(self.L), kind="stable")
        cube = np.concatenate(self.dead_u + [self.U[order]])
        logL = np.concatenate(self.dead_l + [self.L[order]])
        return finish(logL, self.nlive, self.K) + (cube, logL)
