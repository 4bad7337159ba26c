"""Timing of a nested-sampling round with the run resident on the device (mcalf_nested_advance) against the host-driven round of
`als_fitter.nested_sample` (nested.py: argsort, covariance and Cholesky, start draw on the host, K starts and the direction matrix
to the device through `slice_replace_batch`, K rows back), in ns_timing.py's set-up: BASELINE configs C and B, nlive = 4 K with
K = 1024 and 4096, nmoves = 8, --burn untimed rounds that compress the live points, then --rounds timed rounds.
Both routes start from the same initial points and run in ONE process, a round of one after a round of the other, the order
alternating; the packing setting (--compact) is the same on both.  They draw their chain starts from different generators, so
their live sets differ point by point: the lock steps of every round are recorded next to its wall clock; "faster beyond the
spread" (the device route's slowest below the host route's fastest) is reported per round and per lock step separately.
The host route here (HostRoute) is a copy of the loop body of `nested.nested_sample`, timed in two parts; nothing ties the two
together, so an edit of nested.py's round has to be repeated here for the comparison to stay the parent's route.
Recorded per run: the median and min - max over the timed rounds of the wall clock per round and per lock step of both routes,
the host route's share outside `slice_replace_batch` (its book-keeping) and, from a second set of --rounds rounds with
mcalf_nested_set_timing on, the HIP-event time of every book-keeping kernel of the device route (rank, select, moments, Cholesky,
gather, retire) and of its replacement call.  One JSON line, also written to --out.
python tools/nsrun_timing.py [--configs C,B] [--chains 1024,4096] [--rounds 5] [--burn 20] [--nmoves 8] [--max-steps 400] [--compact] [--out profiles/nsrun_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcalf_amd  # noqa: E402
from mcalf_amd import _lib, nested, workloads  # noqa: E402

KERNELS = ("rank", "select", "moments", "cholesky", "gather", "replace", "retire")


def _synth(kw, p):
    """The config's truth spectrum from the device itself (the oracle is test infrastructure)."""
    with mcalf_amd.als_fitter(None, **kw) as fit:
        return fit.model_batch(p)[0]


class HostRoute:
    """The round of `nested.nested_sample`, its live set on the host."""

    def __init__(self, fit, U0, K, nmoves, max_steps, seed):
        self.fit, self.K, self.nmoves, self.max_steps, self.seed = fit, K, nmoves, max_steps, seed
        self.rng = np.random.default_rng(seed)
        self.U = U0.copy()
        self.L = fit.loglike_cube_batch(self.U, return_theta=False)
        self.next_id = 0

    def round(self):
        """(ms of the round, ms inside slice_replace_batch, lock steps)."""
        t0 = time.perf_counter()
        key = np.where(np.isnan(self.L), -np.inf, self.L)
        order = np.argsort(key, kind="stable")
        dying, alive = order[:self.K], order[self.K:]
        lmin = float(key[dying[-1]])
        starts = alive[key[alive] > lmin]
        D = nested.directions(self.U[alive])
        pick = starts[self.rng.integers(0, starts.size, self.K)]
        ids = np.arange(self.next_id, self.next_id + self.K, dtype=np.uint64)
        self.next_id += self.K
        U0 = np.ascontiguousarray(self.U[pick])
        t1 = time.perf_counter()
        Un, _, Ln, status, ne, _ = self.fit.slice_replace_batch(U0, np.full(self.K, lmin), D, nmoves=self.nmoves, max_steps=self.max_steps, seed=self.seed,
                                                                stream_ids=ids)
        t2 = time.perf_counter()
        assert (status >= 0).all() and (Ln > lmin).all()
        self.U[dying], self.L[dying] = Un, Ln
        t3 = time.perf_counter()
        return (t3 - t0) * 1e3, (t2 - t1) * 1e3, self.fit.slice_stats()["steps"]


class DeviceRoute:
    def __init__(self, fit, U0, K, nmoves, max_steps, seed, rounds_in_all):
        self.fit, self.lib = fit, fit._lib
        self.opts = _lib.mcalf_nested_opts(K, nmoves, max_steps, 0, seed, 0.0, U0.shape[0] + (rounds_in_all + 1) * K)
        self.st = _lib.mcalf_nested_state_t()
        fit._call(self.lib.mcalf_nested_open, U0.ctypes.data, U0.shape[0], C.addressof(self.opts))

    def round(self, n=1):
        """(ms of the call, lock steps of its last round)."""
        t0 = time.perf_counter()
        self.fit._call(self.lib.mcalf_nested_advance, n, C.addressof(self.st))
        ms = (time.perf_counter() - t0) * 1e3
        assert self.st.reason == _lib.MCALF_NESTED_BUDGET
        return ms, self.fit.slice_stats()["steps"]

    def kernel_ms(self):
        ms = np.zeros(len(KERNELS))
        self.fit._call(self.lib.mcalf_nested_last_times, ms.ctypes.data)
        return ms

    def close(self):
        self.fit._call(self.lib.mcalf_nested_close)


def _stat(v):
    v = np.asarray(v, dtype=float)
    return {"median": round(float(np.median(v)), 4), "min": round(float(v.min()), 4), "max": round(float(v.max()), 4)}


def _run(fit, K, rounds, burn, nmoves, max_steps, seed):
    U0 = np.random.default_rng(seed).random((4 * K, fit.ndim))
    host = HostRoute(fit, U0, K, nmoves, max_steps, seed)
    dev = DeviceRoute(fit, U0, K, nmoves, max_steps, seed, burn + 2 * rounds + 1)
    try:
        dev.round(burn)
        for _ in range(burn):
            host.round()
        rows = []
        for r in range(rounds + 1):                   # (round 0 warms both routes up)
            first_dev = r % 2 == 0
            d = dev.round() if first_dev else None
            h = host.round()
            d = d or dev.round()
            if r:
                rows.append({"device_ms": d[0], "device_steps": d[1], "host_ms": h[0], "host_replace_ms": h[1], "host_steps": h[2]})
        fit._call(fit._lib.mcalf_nested_set_timing, 1)
        kern = []
        for _ in range(rounds):
            dev.round()
            kern.append(dev.kernel_ms())
        fit._call(fit._lib.mcalf_nested_set_timing, 0)
    finally:
        dev.close()
    kern = np.array(kern)
    col = lambda k: [q[k] for q in rows]
    dms, hms = np.array(col("device_ms")), np.array(col("host_ms"))
    book = kern[:, [0, 1, 2, 3, 4, 6]].sum(axis=1)
    out = {"device_round_ms": _stat(dms), "host_round_ms": _stat(hms),
           "device_ms_per_step": _stat(dms / np.array(col("device_steps"))), "host_ms_per_step": _stat(hms / np.array(col("host_steps"))),
           "device_lock_steps": _stat(col("device_steps")), "host_lock_steps": _stat(col("host_steps")),
           "host_bookkeeping_ms": _stat(hms - np.array(col("host_replace_ms"))),
           "host_bookkeeping_share": _stat((hms - np.array(col("host_replace_ms"))) / hms),
           "device_kernel_ms": {name: _stat(kern[:, i]) for i, name in enumerate(KERNELS)},
           "device_bookkeeping_ms": _stat(book), "device_bookkeeping_share_of_kernel_time": _stat(book / kern.sum(axis=1)),
           "rank_share_of_kernel_time": _stat(kern[:, 0] / kern.sum(axis=1)), "rounds": rows}
    # faster only if the device route's slowest figure is below the host route's fastest: per round, and per lock step
    out["device_faster_per_round_beyond_the_spread"] = bool(out["device_round_ms"]["max"] < out["host_round_ms"]["min"])
    out["device_faster_per_lock_step_beyond_the_spread"] = bool(out["device_ms_per_step"]["max"] < out["host_ms_per_step"]["min"])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C,B")
    ap.add_argument("--chains", default="1024,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--burn", type=int, default=20)
    ap.add_argument("--nmoves", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=400)
    ap.add_argument("--compact", action="store_true", help="mcalf_set_slice_compact on, for both routes")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out = {"nmoves": args.nmoves, "max_steps": args.max_steps, "burn_rounds": args.burn, "timed_rounds": args.rounds, "compact": args.compact, "runs": []}
    for name in args.configs.split(","):
        kw, _, seed = workloads.config(name, _synth)
        with mcalf_amd.als_fitter(None, **kw) as fit:
            fit.set_slice_compact(args.compact)
            for K in (int(k) for k in args.chains.split(",")):
                res = _run(fit, K, args.rounds, args.burn, args.nmoves, args.max_steps, seed)
                out["runs"].append(dict({"config": name, "npix": int(fit.obj_wl.size), "ndim": int(fit.ndim), "chains": K, "nlive": 4 * K}, **res))
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
