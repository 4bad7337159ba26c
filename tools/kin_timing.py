"""Timing of the batched optical-depth kinematics: median ms of mcalf_kinematics_batch_device (HIP events on one stream; mom
and three quantiles) next to mcalf_eqw_batch_device with Wblend alone on the same rows in the same process -- that entry runs
the same Voigt pass ONCE, the kinematics run it twice (sums pass, scan pass), so a ratio near 2 is what the design predicts --
and of `kinematics_batch` (host entry: H2D, five kernels, D2H, synchronised; wall clock).  Config C's 4096 rows and a 2048-row
shard of config E by default.  One JSON line.  Nothing is asserted about the times; the exit status is 1 only if two calls on
the same input differ in a bit.
python tools/kin_timing.py [--configs C E] [--steps 20] [--warmup 3] [--batch N]"""
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
import mcalf_amd  # noqa: E402
from mcalf_amd import kinematics, workloads  # noqa: E402

BATCH = {"C": 4096, "E": 2048}
Q = np.array([0.05, 0.5, 0.95])


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


def _time_wall(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C", "E"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="rows per step (0: 4096 for C, 2048 for E, else the config's batch)")
    args = ap.parse_args()
    out = {"steps": args.steps, "warmup": args.warmup, "configs": {}}
    same = True
    for name in args.configs:
        kw, batch, seed = workloads.config(name, _synth)
        batch = args.batch or BATCH.get(name.upper(), batch)
        P = workloads.draw_P(kw, batch, np.random.default_rng(seed), damped=2 if name.upper() == "E" else 0)
        with mcalf_amd.als_fitter(None, **kw) as fit:
            nl = fit.numlines
            mom, lamq = np.empty((batch, nl, 3)), np.empty((batch, nl, Q.size))
            t_host = _time_wall(lambda: kinematics.kinematics_batch(fit, P, q=Q, out=(mom, lamq)), args.steps, args.warmup)
            again = kinematics.kinematics_batch(fit, P, q=Q)
            same = same and np.array_equal(again.lam_q, lamq, equal_nan=True) and np.array_equal(again.tau_int, mom[:, :, 0], equal_nan=True) \
                and np.array_equal(again.lam_mean, mom[:, :, 1], equal_nan=True) and np.array_equal(again.lam_rms, mom[:, :, 2], equal_nan=True)

            dP = torch.from_numpy(P).cuda()
            dM, dQ = torch.empty((batch, nl, 3), dtype=torch.float64, device="cuda"), torch.empty((batch, nl, Q.size), dtype=torch.float64, device="cuda")
            dB = torch.empty((batch, nl), dtype=torch.float64, device="cuda")
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            lib, ctx = fit._lib, fit._ctx

            def dev_kin():
                assert lib.mcalf_kinematics_batch_device(ctx, dP.data_ptr(), batch, Q.ctypes.data, Q.size, dM.data_ptr(), dQ.data_ptr(), s) == 0

            def dev_mom():
                assert lib.mcalf_kinematics_batch_device(ctx, dP.data_ptr(), batch, None, 0, dM.data_ptr(), None, s) == 0

            def dev_blend():
                assert lib.mcalf_eqw_batch_device(ctx, dP.data_ptr(), batch, 0, None, dB.data_ptr(), s) == 0

            d_kin = _time_events(dev_kin, args.steps, args.warmup)
            d_mom = _time_events(dev_mom, args.steps, args.warmup)
            d_blend = _time_events(dev_blend, args.steps, args.warmup)
            dev_kin()
            torch.cuda.synchronize()
            same = same and np.array_equal(dQ.cpu().numpy(), lamq, equal_nan=True) and np.array_equal(dM.cpu().numpy(), mom, equal_nan=True)
        out["configs"][name] = {"batch": batch, "npix": int(fit.obj.size), "ncompmax": int(fit.ncompmax), "nlines": nl, "nq": int(Q.size),
                                "kin_device_ms": round(d_kin, 4), "kin_device_mom_only_ms": round(d_mom, 4),
                                "eqw_blend_device_ms": round(d_blend, 4), "kin_over_eqw_blend": round(d_kin / d_blend, 3),
                                "kin_host_ms": round(t_host, 4), "kin_host_us_per_row": round(1e3 * t_host / batch, 4)}
    out["two_calls_same_bits"] = bool(same)
    print(json.dumps(out))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
