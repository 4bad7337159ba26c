"""Timing of nested sampling's replacement step on BASELINE configs C (4000 pixels, ndim 47) and B (4000 pixels, ndim 25), with K = 1024 and K = 4096
chains.  nlive = 4 K uniform points of the cube; every round the K lowest die and K chains started from survivors replace them
under the K-th dead point's logL (directions: Cholesky factor of the survivors' covariance), as `nested.nested_sample` does.
The first --burn rounds (device route only, not timed) compress the live points, so that the timed rounds see a constraint that
rejects trials; round 0 warms both routes up.
Three routes through the same state machine, on the same inputs, alternating within one run (the order rotates every round):
  device  `slice_replace_batch` (host entry: H2D, the lock steps with the 4-byte count of live rows read after every step, D2H;
          wall clock) and mcalf_slice_replace_batch_device between HIP events on one stream (the steps the host entry ran);
  packed  the same host entry with `set_slice_compact(True)`: every step's logL launch runs over the rows that proposed a trial
          (sized by the count of the step before), not over all K (wall clock);
  numpy   what the library offered before: the numpy restatement of the state machine (tests/ns_reference.py) around
          `loglike_cube_batch`, one host round trip per step (wall clock).
Recorded per round: lock steps, ms per step and per round of each route, the rows each host-entry route handed to logL launches
and the trials (`slice_stats`), and the lock-step waste -- the share of evaluated rows that were already finished,
1 - sum(nevals) / (steps K).  Per run: the median over the timed rounds, and their minimum and maximum.  The routes must agree
bit for bit (exit status 1 otherwise).  One JSON line, also written to --out.
python tools/ns_timing.py [--configs C,B] [--chains 1024,4096] [--rounds 5] [--burn 20] [--nmoves 8] [--max-steps 400] [--gauss] [--out profiles/ns_timing.json]
--gauss: the same runs under a Gaussian prior on four coordinates (mcalf_set_gauss_prior); the numpy route is then
tests/prior_reference.py's."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mcalf_amd  # noqa: E402
import ns_reference as nr  # noqa: E402
from mcalf_amd import _lib, nested, workloads  # noqa: E402


def _synth(kw, p):
    """The config's truth spectrum from the device itself (the oracle is test infrastructure)."""
    with mcalf_amd.als_fitter(None, **kw) as fit:
        return fit.model_batch(p)[0]


def _device_entry_ms(fit, U0, lmin, D, sid, nmoves, steps, seed):
    n = U0.shape[0]
    opts = _lib.mcalf_slice_opts(nmoves, steps, D.shape[0], 0, seed)
    dU0, dD = torch.from_numpy(U0).cuda(), torch.from_numpy(np.ascontiguousarray(D)).cuda()
    dLmin = torch.full((n,), lmin, dtype=torch.float64, device="cuda")
    dsid = torch.from_numpy(sid.view(np.int64)).cuda()
    dU = torch.empty(U0.shape, dtype=torch.float64, device="cuda")
    dL = torch.empty(n, dtype=torch.float64, device="cuda")
    dS, dN, dM = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    stream = torch.cuda.current_stream()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    rc = fit._lib.mcalf_slice_replace_batch_device(fit._ctx, dU0.data_ptr(), dLmin.data_ptr(), dD.data_ptr(), dsid.data_ptr(), n,
                                                   C.addressof(opts), dU.data_ptr(), None, dL.data_ptr(), dS.data_ptr(), dN.data_ptr(),
                                                   dM.data_ptr(), C.c_void_p(stream.cuda_stream))
    b.record(stream)
    b.synchronize()
    assert rc == 0
    return a.elapsed_time(b), (dU.cpu().numpy(), dL.cpu().numpy(), dS.cpu().numpy(), dN.cpu().numpy(), dM.cpu().numpy())


def _set_gauss(fit):
    """--gauss: a Gaussian prior on the four coordinates behind the ncomp slot, centred on the middle of the box, a quarter of
    the box wide."""
    mu, sigma = np.zeros(fit.ndim), np.zeros(fit.ndim)
    k = slice(fit.startind + 1, fit.startind + 5)
    mu[k], sigma[k] = 0.5 * (fit._lo[k] + fit._hi[k]), 0.25 * (fit._hi[k] - fit._lo[k])
    fit.set_gauss_prior(mu, sigma)


def _run(fit, K, rounds, nmoves, max_steps, seed, burn, gauss=False):
    rng = np.random.default_rng(seed)
    nlive, logl = 4 * K, (lambda U: fit.loglike_cube_batch(U, return_theta=False))
    if gauss:                                         # (the constrained quantity: logL + lnprior, one rounded add)
        like = logl
        logl = lambda U: like(U) + fit.lnprior_batch(U, cube=True)
    U = rng.random((nlive, fit.ndim))
    L = logl(U)
    rows, next_id, same = [], 0, True
    for r in range(-burn, rounds + 1):                # (rounds < 0 compress the live points, device route only; round 0 warms both routes up)
        key = np.where(np.isnan(L), -np.inf, L)
        order = np.argsort(key, kind="stable")
        dying, alive = order[:K], order[K:]
        lmin = float(key[dying[-1]])
        ok = alive[key[alive] > lmin]
        D = nested.directions(U[alive])
        U0 = np.ascontiguousarray(U[ok[rng.integers(0, ok.size, K)]])
        sid = np.arange(next_id, next_id + K, dtype=np.uint64)
        next_id += K
        if r < 0:
            Un, _, Ln, _, _, _ = fit.slice_replace_batch(U0, lmin, D, nmoves=nmoves, max_steps=max_steps, seed=seed, stream_ids=sid)
            U[dying], L[dying] = Un, Ln
            continue
        t, stats = {}, {}
        routes = ("device", "packed", "numpy")
        for route in routes[r % 3:] + routes[:r % 3]:
            fit.set_slice_compact(route == "packed")
            t0 = time.perf_counter()
            if route == "device":
                got = fit.slice_replace_batch(U0, lmin, D, nmoves=nmoves, max_steps=max_steps, seed=seed, stream_ids=sid)
            elif route == "packed":
                packed = fit.slice_replace_batch(U0, lmin, D, nmoves=nmoves, max_steps=max_steps, seed=seed, stream_ids=sid)
            else:
                ref = nr.slice_replace(logl, U0, lmin, D, sid, nmoves, max_steps, seed)
            t[route] = (time.perf_counter() - t0) * 1e3
            stats[route] = fit.slice_stats()
        fit.set_slice_compact(False)
        Un, _, Ln, status, nevals, moves = got
        same &= all(a.tobytes() == b.tobytes() for a, b in zip(got, packed))
        same &= stats["device"]["compact"] == 0 and stats["packed"]["compact"] == 1
        same &= stats["device"]["trials"] == stats["packed"]["trials"] == int(nevals.sum())
        steps = int(nevals.max())
        t_dev, dev = _device_entry_ms(fit, U0, lmin, D, sid, nmoves, steps, seed)
        same &= all(a.tobytes() == b.tobytes() for a, b in zip((Ln, status, nevals, moves), ref[1:])) and np.array_equal(Un, ref[0])
        same &= all(a.tobytes() == b.tobytes() for a, b in zip((Un, Ln, status, nevals, moves), dev))
        U[dying], L[dying] = Un, Ln
        if r == 0:
            continue
        rows.append({"round": r, "lock_steps": steps, "evaluations_per_row_mean": round(float(nevals.mean()), 2),
                     "lock_step_waste": round(1.0 - float(nevals.sum()) / (steps * K), 4), "unfinished_rows": int((status == 0).sum()),
                     "host_entry_ms": round(t["device"], 2), "host_entry_ms_per_step": round(t["device"] / steps, 4),
                     "host_entry_rows_launched": stats["device"]["rows_launched"],
                     "packed_entry_ms": round(t["packed"], 2), "packed_entry_ms_per_step": round(t["packed"] / steps, 4),
                     "packed_entry_rows_launched": stats["packed"]["rows_launched"], "trials": stats["packed"]["trials"],
                     "host_over_packed_entry": round(t["device"] / t["packed"], 3),
                     "device_entry_ms": round(t_dev, 2), "device_entry_ms_per_step": round(t_dev / steps, 4),
                     "numpy_route_ms": round(t["numpy"], 2), "numpy_route_ms_per_step": round(t["numpy"] / steps, 4),
                     "numpy_over_host_entry": round(t["numpy"] / t["device"], 2)})
    keys = [k for k in rows[0] if k != "round"] if rows else []
    med = {k: round(float(np.median([q[k] for q in rows])), 4) for k in keys}
    spread = {k: [min(q[k] for q in rows), max(q[k] for q in rows)] for k in keys if k.endswith(("_ms", "_ms_per_step", "_rows_launched"))}
    return rows, med, spread, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C,B")
    ap.add_argument("--chains", default="1024,4096")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--burn", type=int, default=20)
    ap.add_argument("--nmoves", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=400)
    ap.add_argument("--gauss", action="store_true", help="a Gaussian prior on four coordinates (mcalf_set_gauss_prior)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out, same = {"gauss": args.gauss, "nmoves": args.nmoves, "max_steps": args.max_steps, "burn_rounds": args.burn, "runs": []}, True
    for name in args.configs.split(","):
        kw, _, seed = workloads.config(name, _synth)
        with mcalf_amd.als_fitter(None, **kw) as fit:
            if args.gauss:
                _set_gauss(fit)
            for K in (int(k) for k in args.chains.split(",")):
                rows, med, spread, ok = _run(fit, K, args.rounds, args.nmoves, args.max_steps, seed, args.burn, args.gauss)
                same &= ok
                out["runs"].append({"config": name, "npix": int(fit.obj_wl.size), "ndim": int(fit.ndim), "chains": K, "nlive": 4 * K,
                                    "routes_agree_bit_for_bit": ok, "median_over_rounds": med, "min_max_over_rounds": spread, "rounds": rows})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
