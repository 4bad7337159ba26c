"""Timing of the batched Levenberg-Marquardt fit on BASELINE config C's problem (4000 pixels, ndim 46): 4096 starts, prior-box
draws pulled halfway toward the truth row.  Two routes to a best-fit row:
  fit     `maximize_batch` (host entry: H2D, the fit with the live-row counter read after every outer iteration, D2H; wall
          clock) and mcalf_maximize_batch_device between HIP events on one stream (max_iter iterations unconditionally);
  scipy   what the library offered before: scipy.optimize.least_squares (trf, the same box, x_scale = hi - lo) driving
          `model_batch` / `model_jacobian` one row at a time, on 8 of the same rows (wall clock).
Recorded: outer iterations used, the status histogram, Fisher products issued, ms per row of each route.  The only bar: the fit's
host entry per row is faster than the looped route per row (exit status 1 otherwise).  One JSON line, also written to --out.
python tools/fit_timing.py [--batch 4096] [--max-iter 50] [--scipy-rows 8] [--out profiles/fit_timing.json]"""
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
from mcalf_amd import _lib, workloads  # noqa: E402


def _synth(kw, p):
    """The config's truth spectrum from the device itself (the oracle is test infrastructure)."""
    with mcalf_amd.als_fitter(None, **kw) as fit:
        return fit.model_batch(p)[0]


def _starts(kw, fit, batch, seed):
    """Prior-box draws pulled halfway toward the truth row: R 8, ten components of the mock generator's table, the eleventh slot
    inactive, the fillers negligible (N at its lower bound)."""
    lo, hi = fit._lo, fit._hi
    truth = 0.5 * (lo + hi)
    truth[0] = 8.0
    truth[fit.startind] = 10.0
    truth[fit.startind + 1:fit.startind + 31] = workloads.truth_vector(10)[1:]
    truth[fit.endind::3] = lo[fit.endind::3]
    P = 0.5 * (workloads.draw_P(kw, batch, np.random.default_rng(seed)) + truth)
    P[:, fit.startind] = 10.0
    return P


def _scipy_row(fit, p0, w):
    from scipy.optimize import least_squares
    lo, hi = fit._lo, fit._hi
    nc = int(p0[fit.startind])
    free = np.array([k for k in range(fit.ndim) if k != fit.startind and not (fit.startind + 1 + 3 * nc <= k < fit.endind)])
    sw = np.sqrt(w)
    flux = np.where(w > 0, fit.obj, 0.0)
    calls = [0, 0]

    def full(x):
        p = p0.copy()
        p[free] = x
        return p

    def res(x):
        calls[0] += 1
        return sw * (flux - np.where(w > 0, fit.model_batch(full(x))[0], 0.0))

    def jac(x):
        calls[1] += 1
        return -sw[:, None] * fit.model_jacobian(full(x))[:, free]

    sol = least_squares(res, np.clip(p0[free], lo[free], hi[free]), jac=jac, bounds=(lo[free], hi[free]), method="trf",
                        x_scale=(hi - lo)[free])
    return full(sol.x), calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--max-iter", type=int, default=50)
    ap.add_argument("--scipy-rows", type=int, default=8)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    kw, _, seed = workloads.config("C", _synth)
    batch = args.batch
    with mcalf_amd.als_fitter(None, **kw) as fit:
        P0 = _starts(kw, fit, batch, seed)
        cg = fit.ndim
        fit.maximize_batch(P0, max_iter=1)                            # grows every workspace
        t0 = time.perf_counter()
        P, L, status, niter = fit.maximize_batch(P0, max_iter=args.max_iter)
        t_host = (time.perf_counter() - t0) * 1e3
        L0 = fit.loglike_batch(P0)

        dP0 = torch.from_numpy(P0).cuda()
        dP = torch.empty(P0.shape, dtype=torch.float64, device="cuda")
        dL = torch.empty(batch, dtype=torch.float64, device="cuda")
        dS, dN = torch.empty(batch, dtype=torch.int32, device="cuda"), torch.empty(batch, dtype=torch.int32, device="cuda")
        used = int(niter.max())
        # the device entry runs its max_iter unconditionally: give it what the host entry ran (one more than the last step taken
        # when a row's zero projected gradient was found at the top of the next iteration) -- finished rows are carried
        dev_iters = min(args.max_iter, used + 1)
        opts = _lib.mcalf_fit_opts(dev_iters, 0, 0, 0, 1e-3, 1e-10)
        stream = torch.cuda.current_stream()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        rc = fit._lib.mcalf_maximize_batch_device(fit._ctx, dP0.data_ptr(), batch, C.addressof(opts), dP.data_ptr(), dL.data_ptr(),
                                                  dS.data_ptr(), dN.data_ptr(), C.c_void_p(stream.cuda_stream))
        b.record(stream)
        b.synchronize()
        assert rc == 0
        t_dev = a.elapsed_time(b)
        same = all(x.tobytes() == y.tobytes() for x, y in zip((dP.cpu().numpy(), dL.cpu().numpy(), dS.cpu().numpy(), dN.cpu().numpy()),
                                                              (P, L, status, niter)))

        with np.errstate(divide="ignore", invalid="ignore"):
            w = 1.0 / np.asarray(fit.obj_noise, dtype=float) ** 2
            w = np.where(np.isnan(w * np.asarray(fit.obj, dtype=float) ** 2 - np.log(w)), 0.0, w)
        rows = list(range(0, batch, max(1, batch // args.scipy_rows)))[:args.scipy_rows]
        t0 = time.perf_counter()
        sols = [_scipy_row(fit, P0[r], w) for r in rows]
        t_scipy = (time.perf_counter() - t0) * 1e3
        Ls = fit.loglike_batch(np.array([s[0] for s in sols]))

    hist = {str(int(k)): int(v) for k, v in zip(*np.unique(status, return_counts=True))}
    out = {"config": "C", "batch": batch, "npix": int(fit.obj_wl.size), "ndim": int(fit.ndim), "cg_iters": cg, "max_iter": args.max_iter,
           "lambda0": 1e-3, "ftol": 1e-10,
           "host_entry_ms": round(t_host, 1), "host_entry_ms_per_row": round(t_host / batch, 4),
           "device_entry_ms": round(t_dev, 1), "device_entry_outer_iterations": dev_iters, "device_entry_ms_per_row": round(t_dev / batch, 4),
           "device_entry_bits_equal_host_entry": same,
           "outer_iterations_max": used, "outer_iterations_median": float(np.median(niter)), "status_histogram": hist,
           "fisher_products_issued_host_entry_at_least": cg * used, "fisher_products_issued_device_entry": cg * dev_iters, "rows_per_product": batch,
           "median_logL_start": float(np.median(L0)), "median_logL_fit": float(np.median(L)),
           "scipy_rows": len(rows), "scipy_ms": round(t_scipy, 1), "scipy_ms_per_row": round(t_scipy / len(rows), 2),
           "scipy_model_calls_per_row": float(np.mean([s[1][0] for s in sols])), "scipy_jacobian_calls_per_row": float(np.mean([s[1][1] for s in sols])),
           "fit_minus_scipy_logL_on_those_rows": [float(f"{L[r] - l:.4g}") for r, l in zip(rows, Ls)],
           "scipy_over_fit_per_row": round((t_scipy / len(rows)) / (t_host / batch), 1)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return 0 if t_host / batch < t_scipy / len(rows) else 1


if __name__ == "__main__":
    sys.exit(main())
