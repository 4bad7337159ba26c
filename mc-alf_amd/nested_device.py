"""Nested sampling with the run itself in the library: the live set and the dead points stay on the device from the first round
to the last (`mcalf_nested_open` / `_advance` / `_finish` / `_read`; include/mcalf_hip.h), and the host sees one small record per
round.  `nested.nested_sample` keeps the same books in numpy on the host around `slice_replace_batch`; the two draw their chain
starts from different generators, so their runs differ point by point and agree in distribution."""
from __future__ import annotations

import ctypes as C
import warnings

import numpy as np

from . import _lib
from .nested import NestedResult


def nested_sample_device(fit, nlive, batch=None, nmoves=None, max_steps=None, dlogz=1e-3, max_rounds=100000, seed=0, max_dead=None,
                         rounds_per_call=64):
    """Nested sampling of `fit`'s posterior (an `als_fitter`) until max(L_live) X < dlogz Z, a plateau of the live set or
    `max_rounds`; returns a `nested.NestedResult`, as `als_fitter.nested_sample` does, with the same defaults: `batch` None:
    nlive // 4 points replaced per round; `nmoves` None: 2 ndim slice moves per chain; `max_steps` None: 50 nmoves lock steps
    per round.  The initial points are `default_rng(seed).random((nlive, ndim))`.  `max_dead`: dead rows the device keeps, 8 (ndim + 1)
    bytes each, held by the fitter until it is closed (None: room for min(max_rounds, 64 nlive / batch) rounds -- ln X down to
    about -64, enough for an information H of some 50 nats at the default dlogz -- and never more than 1 GiB of live and dead rows).
    A run that fills it before it converges ends there with a RuntimeWarning and `stop_reason` 3: give a larger `max_dead`.
    `rounds_per_call`: rounds one library call runs before the host looks again (nothing of the result depends on it).  Under a Gaussian prior `logL` holds logL + lnprior and `lnprior` the prior's part."""
    nlive, ndim = int(nlive), fit.ndim
    K = max(1, nlive // 4) if batch is None else int(batch)
    if not 1 <= K < nlive:
        raise ValueError(f"batch must be in [1, nlive), got {K} with nlive {nlive}")
    nmoves = 2 * ndim if nmoves is None else int(nmoves)
    max_steps = 50 * nmoves if max_steps is None else int(max_steps)
    max_rounds, rounds_per_call = int(max_rounds), max(1, int(rounds_per_call))
    if max_dead is None:
        room = (1 << 30) // (8 * (ndim + 1)) - nlive
        max_dead = max(nlive + K, min(min(max_rounds, -(-64 * nlive // K)) * K + nlive, room))
    fit._ensure_prior()
    U0 = np.random.default_rng(seed).random((nlive, ndim))
    opts = _lib.mcalf_nested_opts(K, nmoves, max_steps, 0, int(seed) & 0xFFFFFFFFFFFFFFFF, float(dlogz), int(max_dead))
    lib, p = fit._lib, fit._ptr
    fit._call(lib.mcalf_nested_open, p(U0), nlive, C.addressof(opts))
    try:
        st = _lib.mcalf_nested_state_t()
        fit._call(lib.mcalf_nested_advance, 0, C.addressof(st))
        while st.reason == _lib.MCALF_NESTED_BUDGET and st.rounds < max_rounds:
            fit._call(lib.mcalf_nested_advance, min(rounds_per_call, max_rounds - st.rounds), C.addressof(st))
        if st.reason == _lib.MCALF_NESTED_FULL and st.rounds < max_rounds:
            warnings.warn(f"nested_sample_device: the {int(max_dead)} dead rows were full after {st.rounds} rounds, before the run converged "
                          f"(ln X {st.logX:.2f}); the evidence is that of the truncated run -- pass a larger max_dead", RuntimeWarning, stacklevel=2)
        logZ, err, H = C.c_double(), C.c_double(), C.c_double()
        fit._call(lib.mcalf_nested_finish, C.addressof(logZ), C.addressof(err), C.addressof(H))
        n = st.ndead + nlive
        cube, theta = np.empty((n, ndim)), np.empty((n, ndim))
        logL, logw = np.empty(n), np.empty(n)
        fit._call(lib.mcalf_nested_read, 0, n, p(cube), p(theta), p(logL), p(logw))
    finally:
        fit._call(lib.mcalf_nested_close)
    res = NestedResult(logZ=logZ.value, logZ_err=err.value, H=H.value, cube=cube, theta=theta, logL=logL, logw=logw, rounds=int(st.rounds),
                       nevals=int(st.nevals), unfinished=int(st.unfinished), nlive=nlive, stop_reason=int(st.reason))
    res.rows_launched = int(st.rows_launched)
    if fit._has_gauss():
        res.lnprior = fit.lnprior_batch(cube, cube=True)
    return res
