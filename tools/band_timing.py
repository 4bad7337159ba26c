"""Timing of the per-pixel posterior bands on BASELINE config C's problem: its 4096 rows and one longer chain.  Two routes to
(mean, var, quantiles 0.16 / 0.5 / 0.84, nvalid):
  band    `model_band_batch` (host entry: H2D, the model launch, the band kernels, D2H of 3 + K rows, synchronised; wall clock),
          and mcalf_model_band_batch_device between HIP events on one stream, split into SYNTHESIS -- mcalf_model_batch_device
          on the same rows between events -- and STATISTICS, the rest;
  host    what the library offered before: `model_batch` to the host (the whole [batch, npix] matrix over PCIe), then
          np.nanquantile / np.nanmean / np.nanvar on one core (wall clock, fewer repetitions: it takes seconds).
One JSON line, also written to --out when given.  Nothing is promised in advance: the figures are what they are.
python tools/band_timing.py [--batches 4096 16384] [--steps 10] [--warmup 2] [--host-steps 2] [--out profiles/band_timing.json]"""
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
from mcalf_amd import workloads  # noqa: E402

Q = (0.16, 0.5, 0.84)


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
    ap.add_argument("--batches", nargs="+", type=int, default=[4096, 16384], help="rows of the chain (config C's problem)")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-steps", type=int, default=2, help="repetitions of the host route")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    kw, _, seed = workloads.config("C", _synth)
    q = np.asarray(Q)
    out = {"config": "C", "q": list(Q), "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps, "chains": []}
    for batch in args.batches:
        P = workloads.draw_P(kw, batch, np.random.default_rng(seed))
        with mcalf_amd.als_fitter(None, **kw) as fit:
            npix = fit.obj_wl.size
            t_band = _time_wall(lambda: fit.model_band_batch(P, q=Q), args.steps, args.warmup)
            band = fit.model_band_batch(P, q=Q)

            t_copy = _time_wall(lambda: fit.model_batch(P), args.host_steps, 1)
            M = fit.model_batch(P)
            t_quant = _time_wall(lambda: np.nanquantile(M, q, axis=0), args.host_steps, 0)
            t_mom = _time_wall(lambda: (np.nanmean(M, axis=0), np.nanvar(M, axis=0)), args.host_steps, 0)
            want = np.nanquantile(M, q, axis=0)
            agree_q = float(np.max(np.abs(band.quantiles - want)))
            agree_m = float(np.max(np.abs(band.mean - np.nanmean(M, axis=0))))
            del M

            lib, ctx = fit._lib, fit._ctx
            dP = torch.from_numpy(P).cuda()
            f64 = dict(dtype=torch.float64, device="cuda")
            dM, dmean, dvar, dQ = torch.empty((batch, npix), **f64), torch.empty(npix, **f64), torch.empty(npix, **f64), torch.empty((len(Q), npix), **f64)
            dn = torch.empty(npix, dtype=torch.int64, device="cuda")
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)

            def dev_band():
                assert lib.mcalf_model_band_batch_device(ctx, dP.data_ptr(), batch, 0, q.ctypes.data, len(Q), dM.data_ptr(), dmean.data_ptr(),
                                                         dvar.data_ptr(), dQ.data_ptr(), dn.data_ptr(), s) == 0

            def dev_moments():
                assert lib.mcalf_model_band_batch_device(ctx, dP.data_ptr(), batch, 0, None, 0, dM.data_ptr(), dmean.data_ptr(),
                                                         dvar.data_ptr(), None, dn.data_ptr(), s) == 0

            def dev_model():
                assert lib.mcalf_model_batch_device(ctx, dP.data_ptr(), batch, 0, dM.data_ptr(), s) == 0

            # (alternating, so that a drift of the clock falls on all three alike)
            d_band, d_mom, d_model = [], [], []
            for _ in range(3):
                d_model.append(_time_events(dev_model, args.steps, args.warmup))
                d_band.append(_time_events(dev_band, args.steps, args.warmup))
                d_mom.append(_time_events(dev_moments, args.steps, args.warmup))
            d_band, d_mom, d_model = float(np.median(d_band)), float(np.median(d_mom)), float(np.median(d_model))
            assert np.array_equal(dQ.cpu().numpy(), band.quantiles)
        stats = d_band - d_model
        host = t_copy + t_quant + t_mom
        out["chains"].append({
            "batch": batch, "npix": int(npix), "matrix_MB": round(batch * npix * 8 / 1e6, 1),
            "band_host_entry_ms": round(t_band, 3), "band_device_ms": round(d_band, 4), "synthesis_device_ms": round(d_model, 4),
            "statistics_device_ms": round(stats, 4), "moments_only_statistics_device_ms": round(d_mom - d_model, 4),
            "selection_device_ms": round(d_band - d_mom, 4), "statistics_over_synthesis": round(stats / d_model, 2),
            "host_route_model_batch_ms": round(t_copy, 1), "host_route_nanquantile_ms": round(t_quant, 1),
            "host_route_nanmean_nanvar_ms": round(t_mom, 1), "host_route_ms": round(host, 1), "host_route_over_band_host_entry": round(host / t_band, 1),
            "max_abs_quantile_difference": float(f"{agree_q:.3g}"), "max_abs_mean_difference": float(f"{agree_m:.3g}")})
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
