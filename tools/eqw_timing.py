"""Timing of the batched equivalent widths: median ms of `eqw_batch` (host entry: H2D, three kernels, D2H, synchronised)
and of mcalf_eqw_batch_device (HIP events on one stream) next to `loglike_batch` / mcalf_loglike_batch_device on the same
rows -- config C's 4096 rows and a 2048-row shard of config E by default -- and the per-row time of the route the entry
replaces: `calc_w(p, k, reference_indexing=False)` looped over 64 rows and every line (one synchronous single-line
spectrum call and a numpy integration per row and line).  One JSON line.  The exit status is 1 when `eqw_batch` per row is
not faster than that loop per row on every config: a slower entry has no reason to exist.
python tools/eqw_timing.py [--configs C E] [--steps 20] [--warmup 3] [--batch N] [--loop-rows 64]"""
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

BATCH = {"C": 4096, "E": 2048}


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
    ap.add_argument("--loop-rows", type=int, default=64, help="rows of the looped calc_w route")
    args = ap.parse_args()
    out = {"steps": args.steps, "warmup": args.warmup, "configs": {}}
    ok = True
    for name in args.configs:
        kw, batch, seed = workloads.config(name, _synth)
        batch = args.batch or BATCH.get(name.upper(), batch)
        P = workloads.draw_P(kw, batch, np.random.default_rng(seed), damped=2 if name.upper() == "E" else 0)
        with mcalf_amd.als_fitter(None, **kw) as fit:
            nlines, ncm = fit.numlines, int(fit.ncompmax)
            wc, wb, ll = np.empty((batch, ncm, nlines)), np.empty((batch, nlines)), np.empty(batch)
            t_eqw = _time_wall(lambda: fit.eqw_batch(P, out=(wc, wb)), args.steps, args.warmup)
            t_comp = _time_wall(lambda: fit.eqw_batch(P, out=(wc, None), blend=False), args.steps, args.warmup)
            t_ll = _time_wall(lambda: fit.loglike_batch(P, out=ll), args.steps, args.warmup)
            nloop = min(args.loop_rows, batch)

            def loop():
                return [fit.calc_w(p, k, reference_indexing=False) for p in P[:nloop] for k in range(nlines)]

            t_loop = _time_wall(loop, max(1, args.steps // 4), 1)
            want = np.array(loop()).reshape(nloop, nlines)
            got = wc[:nloop].sum(axis=1)
            agree = float(np.max(np.abs(got - want) / (1e-11 + 1e-9 * np.abs(want))))

            dP = torch.from_numpy(P).cuda()
            dC, dB, dL = torch.from_numpy(wc).cuda(), torch.from_numpy(wb).cuda(), torch.from_numpy(ll).cuda()
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            lib, ctx = fit._lib, fit._ctx

            def dev_eqw():
                assert lib.mcalf_eqw_batch_device(ctx, dP.data_ptr(), batch, 0, dC.data_ptr(), dB.data_ptr(), s) == 0

            def dev_ll():
                assert lib.mcalf_loglike_batch_device(ctx, dP.data_ptr(), batch, dL.data_ptr(), s) == 0

            d_eqw = _time_events(dev_eqw, args.steps, args.warmup)
            d_ll = _time_events(dev_ll, args.steps, args.warmup)
        per_row, per_row_loop = t_eqw / batch, t_loop / nloop
        ok = ok and per_row < per_row_loop
        out["configs"][name] = {"batch": batch, "npix": int(fit.obj.size), "ncompmax": ncm, "nlines": nlines,
                                "eqw_ms": round(t_eqw, 4), "eqw_comp_only_ms": round(t_comp, 4), "loglike_ms": round(t_ll, 4),
                                "eqw_over_loglike": round(t_eqw / t_ll, 3), "eqw_device_ms": round(d_eqw, 4),
                                "loglike_device_ms": round(d_ll, 4), "eqw_us_per_row": round(1e3 * per_row, 4),
                                "looped_calc_w_rows": nloop, "looped_calc_w_us_per_row": round(1e3 * per_row_loop, 2),
                                "speedup_per_row": round(per_row_loop / per_row, 1), "agreement_error_over_bar": float(f"{agree:.3g}")}
    out["eqw_faster_than_looped_calc_w"] = ok
    print(json.dumps(out))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
