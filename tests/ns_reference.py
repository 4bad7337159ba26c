"""Test-side reference for nested sampling's replacement step (mcalf_slice_replace_batch): float64 numpy restatements of
Philox4x64-10 and of the lock-step state machine of include/mcalf_hip.h, with logL passed in as a callable.

Only +, -, x, /, min, max and compare are used on the proposal, each as one numpy ufunc call (one correctly rounded IEEE
operation, no FMA), so a trajectory computed here equals the device's bit for bit wherever `logL` returns the bits the device's
decisions saw."""
import numpy as np

M0, M1 = 0xD2E7470EE14C6C93, 0xCA5A826395121157
W0, W1 = 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhilo(a, b):
    """(high, low) 64-bit words of the 128-bit product of the constant `a` and the uint64 array `b`."""
    a_lo, a_hi = np.uint64(a & 0xFFFFFFFF), np.uint64(a >> 32)
    b_lo, b_hi = b & _M32, b >> _S32
    ll, lh, hl, hh = a_lo * b_lo, a_lo * b_hi, a_hi * b_lo, a_hi * b_hi
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32), (mid << _S32) | (ll & _M32)


def philox4x64(counter, key):
    """Philox4x64-10: `counter` [..., 4] and `key` [..., 2] (uint64, broadcast against each other) -> the block [..., 4]."""
    c = np.array(np.broadcast_arrays(*[np.asarray(counter, dtype=np.uint64)[..., i] for i in range(4)]), dtype=np.uint64)
    k = [np.asarray(key, dtype=np.uint64)[..., i].copy() for i in range(2)]
    c0, c1, c2, c3 = c[0], c[1], c[2], c[3]
    with np.errstate(over="ignore"):
        for _ in range(10):
            hi0, lo0 = _mulhilo(M0, c0)
            hi1, lo1 = _mulhilo(M1, c2)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k[0], lo1, hi0 ^ c3 ^ k[1], lo0
            k[0] = k[0] + np.uint64(W0)
            k[1] = k[1] + np.uint64(W1)
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1)


def words(it, sid, seed):
    """(w0, w1) of step `it` for the stream ids `sid` [n]: the block of counter (it, 0, sid, 0) and key (seed, 0)."""
    sid = np.asarray(sid, dtype=np.uint64).reshape(-1)
    counter = np.zeros((sid.size, 4), dtype=np.uint64)
    counter[:, 0] = np.uint64(it)
    counter[:, 2] = sid
    blk = philox4x64(counter, np.array([int(seed) & 0xFFFFFFFFFFFFFFFF, 0], dtype=np.uint64))
    return blk[:, 0], blk[:, 1]


def chord(x, d):
    """(tl, tr) of the line x + t d through the unit cube, rows of x and d [n, ndim]."""
    nz = d != 0.0
    safe = np.where(nz, d, 1.0)
    a, b = (0.0 - x) / safe, (1.0 - x) / safe
    tl = np.where(nz, np.minimum(a, b), -np.inf).max(axis=1)
    tr = np.where(nz, np.maximum(a, b), np.inf).min(axis=1)
    none = ~nz.any(axis=1)
    return np.where(none, 0.0, tl), np.where(none, 0.0, tr)


def slice_replace(logL, U0, Lmin, D, sid, nmoves, max_steps, seed=0):
    """(U, logL, status, nevals, moves) of mcalf_slice_replace_batch; `logL(U)` -> [n] evaluates rows of the unit cube (every
    row of the trial array at every step, finished rows included, as the device does)."""
    U0 = np.array(U0, dtype=float, ndmin=2)
    n, ndim = U0.shape
    D = np.array(D, dtype=float, ndmin=2)
    Lmin = np.broadcast_to(np.asarray(Lmin, dtype=float), (n,))
    sid = np.asarray(sid, dtype=np.uint64).reshape(n)
    U, Y = U0.copy(), U0.copy()
    L = np.array(logL(Y), dtype=float).reshape(n)
    with np.errstate(invalid="ignore"):
        good = ((U0 >= 0.0) & (U0 <= 1.0)).all(axis=1) & (L > Lmin)
    status = np.where(good, 1 if nmoves == 0 else 0, -1).astype(np.int32)
    nevals, moves = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    dirs = np.full(n, -1)
    tl, tr, t = np.zeros(n), np.zeros(n), np.zeros(n)
    LY = None

    def decide():
        live = status == 0
        with np.errstate(invalid="ignore"):
            acc = live & (LY > Lmin)
        U[acc], L[acc] = Y[acc], LY[acc]
        moves[acc] += 1
        dirs[acc] = -1
        status[acc & (moves == nmoves)] = 1
        rej = live & ~acc
        neg = t < 0.0
        tl[rej & neg] = t[rej & neg]
        tr[rej & ~neg] = t[rej & ~neg]

    for it in range(1, (max_steps if nmoves > 0 else 0) + 1):
        if LY is not None:
            decide()
        live = status == 0
        if not live.any():
            LY = None
            break
        w0, w1 = words(it, sid, seed)
        need = live & (dirs < 0)
        dirs[need] = (w0[need] % np.uint64(D.shape[0])).astype(np.int64)
        if need.any():
            tl[need], tr[need] = chord(U[need], D[dirs[need]])
        xi = (w1 >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        t[live] = (tl + (tr - tl) * xi)[live]
        with np.errstate(invalid="ignore"):
            y = U[live] + t[live, None] * D[dirs[live]]
            Y[live] = np.where(y < 0.0, 0.0, np.where(y > 1.0, 1.0, y))
        nevals[live] += 1
        LY = np.array(logL(Y), dtype=float).reshape(n)
    if LY is not None:
        decide()
    return U, L, status, nevals, moves


def replace_with(logL, max_steps=None, transform=None):
    """The `replace` callable of `nested.nested_sample` around `slice_replace`; theta = transform(U) (None: U itself)."""
    def replace(U0, Lmin, dirs, nmoves, seed, stream_ids):
        steps = 50 * nmoves if max_steps is None else max_steps
        U, L, status, nevals, moves = slice_replace(logL, U0, Lmin, dirs, stream_ids, nmoves, steps, seed)
        return U, (U.copy() if transform is None else transform(U)), L, status, nevals, moves
    return replace
