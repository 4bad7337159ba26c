"""Timing of the chain diagnostics at config C's shape (4096 walkers x ndim 47), three things in one process:

1. the device statistics pass: median ms of mcalf_chain_stats_device (HIP events on one stream) on a synthetic AR(1) chain on the
   device, T as large as `--chain-gib` (4) GiB allow, at L = T - 1 and at the converge run's L = ceil(c T / factor) + 1, and on the
   prefixes T = 100, 200, 400, ... a converge run checks;
2. the host route on the same data: D2H of the chain (wall clock) plus `ensemble._autocorr` of every (walker, coordinate) series,
   timed on the first `--host-walkers` (8) walkers and SCALED to all of them (the output says so: host_autocorr_scaled);
3. the converge run's overhead: `convergence.ensemble_sample_until` against `fit.ensemble_batch` of the same final length (wall
   clock, check_every 100, rtol 0 so that every check is made), and a check's cost as a fraction of the 100
   iterations between checks (mcalf_ensemble_batch_device of 100 iterations, HIP events).

One JSON line; `--out FILE` writes it to a file as well (profiles/conv_timing.json is such a record).  Nothing is asserted about the
times; the exit status is 1 only if two statistics calls on the same input differ in a bit.
python tools/conv_timing.py [--steps 5] [--warmup 1] [--chain-gib 4] [--host-walkers 8] [--run-steps 600] [--out FILE]"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcalf_amd  # noqa: E402
from mcalf_amd import _lib, convergence, ensemble, workloads  # noqa: E402

NWALKERS, C_SOKAL, FACTOR, CHECK_EVERY = 4096, 5.0, 50.0, 100


def _synth(kw, p):
    """The config's truth spectrum from the device itself (the oracle is test infrastructure)."""
    with mcalf_amd.als_fitter(None, **kw) as fit:
        return fit.model_batch(p)[0]


def _time_events(fn, steps, warmup):
    stream = torch.cuda.current_stream()
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ms = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        fn()
        b.record(stream)
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def _ar1_device(T, n, d, phi=0.9, seed=1):
    """An AR(1) chain [T, n, d] made on the device, mapped to 0.5 + 0.1 x."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    X = torch.empty((T, n, d), dtype=torch.float64, device="cuda")
    X[0] = torch.randn((n, d), dtype=torch.float64, device="cuda", generator=g)
    for t in range(1, T):
        X[t] = phi * X[t - 1] + math.sqrt(1.0 - phi * phi) * torch.randn((n, d), dtype=torch.float64, device="cuda", generator=g)
    return X.mul_(0.1).add_(0.5)


def _check_lag(T):
    return int(min(T - 1, math.ceil(C_SOKAL * T / FACTOR) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--chain-gib", type=float, default=4.0)
    ap.add_argument("--host-walkers", type=int, default=8)
    ap.add_argument("--run-steps", type=int, default=600)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    kw, _, seed = workloads.config("C", _synth)
    out = {"steps": args.steps, "warmup": args.warmup, "nwalkers": NWALKERS, "c": C_SOKAL, "factor": FACTOR, "check_every": CHECK_EVERY}
    with mcalf_amd.als_fitter(None, **kw) as fit:
        n, d = NWALKERS, fit.ndim
        T = int(args.chain_gib * 2 ** 30) // (n * d * 8)
        out.update(ndim=d, T=T, chain_bytes=T * n * d * 8)
        lib, ctx = fit._lib, fit._ctx
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        X = _ar1_device(T, n, d)
        dstats = torch.empty((d, 6), dtype=torch.float64, device="cuda")
        dinfo = torch.empty((d, 4), dtype=torch.int32, device="cuda")

        def stats(Tp, L):
            opts = _lib.mcalf_chain_opts(C_SOKAL, L)
            rc = lib.mcalf_chain_stats_device(ctx, X.data_ptr(), Tp, n, d, None, C.addressof(opts), dstats.data_ptr(), dinfo.data_ptr(), None, s)
            assert rc == 0, lib.mcalf_last_error(ctx)

        # 1. the device pass
        out["stats_full_lag_ms"] = round(_time_events(lambda: stats(T, T - 1), args.steps, args.warmup), 3)
        out["stats_check_lag"] = _check_lag(T)
        out["stats_check_lag_ms"] = round(_time_events(lambda: stats(T, _check_lag(T)), args.steps, args.warmup), 3)
        first = dstats.cpu().numpy().copy(), dinfo.cpu().numpy().copy()
        stats(T, _check_lag(T))
        torch.cuda.synchronize()
        same = first[0].tobytes() == dstats.cpu().numpy().tobytes() and first[1].tobytes() == dinfo.cpu().numpy().tobytes()
        out["tau_of_the_synthetic_chain"] = [round(float(first[0][:, 2].min()), 3), round(float(first[0][:, 2].max()), 3)]
        prefixes = [Tp for Tp in (100, 200, 400, 800, 1600) if Tp < T] + [T]
        check_ms = {Tp: _time_events(lambda: stats(Tp, _check_lag(Tp)), args.steps, args.warmup) for Tp in prefixes}
        out["check_ms_by_T"] = {str(Tp): round(ms, 3) for Tp, ms in check_ms.items()}

        # 2. the host route on the same data
        host = torch.empty(X.shape, dtype=torch.float64).pin_memory() if args.chain_gib <= 1.0 else torch.empty(X.shape, dtype=torch.float64)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host.copy_(X)
        torch.cuda.synchronize()
        out["host_d2h_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        Xh = host.numpy()
        nw = min(args.host_walkers, n)
        t0 = time.perf_counter()
        for w in range(nw):
            for k in range(d):
                ensemble._autocorr(Xh[:, w, k])
        sub = (time.perf_counter() - t0) * 1e3
        out.update(host_autocorr_walkers_timed=nw, host_autocorr_subset_ms=round(sub, 1), host_autocorr_scaled=True,
                   host_autocorr_all_walkers_ms=round(sub * n / nw, 1), host_route_ms=round(out["host_d2h_ms"] + sub * n / nw, 1))
        del host, Xh, X
        torch.cuda.empty_cache()

        # 3. the converge run against the plain run of the same length
        U0 = np.random.default_rng(seed).random((n, d))
        dU0 = torch.from_numpy(U0).cuda()
        dU, dT = (torch.empty((n, d), dtype=torch.float64, device="cuda") for _ in range(2))
        dL = torch.empty((n,), dtype=torch.float64, device="cuda")
        dS, dN = (torch.empty((n,), dtype=torch.int32, device="cuda") for _ in range(2))
        fit._ensure_prior()
        eopts = _lib.mcalf_ens_opts(CHECK_EVERY, 1, 0, 0, 2.0, seed, 0)

        def block():
            rc = lib.mcalf_ensemble_batch_device(ctx, dU0.data_ptr(), n, C.addressof(eopts), dU.data_ptr(), dT.data_ptr(), dL.data_ptr(),
                                                 dS.data_ptr(), dN.data_ptr(), None, None, s)
            assert rc == 0, lib.mcalf_last_error(ctx)

        block_ms = _time_events(block, args.steps, args.warmup)
        out["iterations_100_ms"] = round(block_ms, 3)
        out["check_over_100_iterations"] = {str(Tp): round(ms / block_ms, 4) for Tp, ms in check_ms.items()}
        steps = args.run_steps
        fit.ensemble_batch(U0, CHECK_EVERY, seed=seed)                                   # (warm-up: workspaces, the prior)
        t0 = time.perf_counter()
        plain = fit.ensemble_batch(U0, steps, seed=seed)
        t_plain = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        got = convergence._ensemble_converge(fit, U0, steps, check_every=CHECK_EVERY, factor=FACTOR, rtol=0.0, c=C_SOKAL, seed=seed)
        t_conv = (time.perf_counter() - t0) * 1e3
        same = same and got[5].tobytes() == plain[5].tobytes() and got[0].tobytes() == plain[0].tobytes()
        out.update(run_steps=steps, run_checks=int(got[9].shape[0]), run_plain_wall_ms=round(t_plain, 1), run_converge_wall_ms=round(t_conv, 1),
                   run_overhead_per_check_ms=round((t_conv - t_plain) / max(int(got[9].shape[0]), 1), 2))
    out["same_bits"] = bool(same)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
