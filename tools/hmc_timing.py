"""Timing and efficiency of Hamiltonian Monte Carlo (mcalf_hmc_batch) on BASELINE config C (4000 pixels, ndim 47) with 4096
walkers and trajectories of 8 leapfrog steps, against what it is built from and against the ensemble sampler's stretch move.
The walkers of both samplers start in the same ball of half-width --ball around the `maximize_batch` optimum next to the
config's truth.
  iteration  mcalf_hmc_batch_device between HIP events on one stream, --iters iterations per call under the step and the scales
             the driver's burn-in ended with, the run continued from call to call; ms per iteration, median of --reps calls
             after --warmup.  Against `nleap` bare mcalf_loglike_grad_batch_device launches over the same rows between HIP
             events: what an iteration's gradient work costs without the sampler's kernels (that entry is the parent commit's).
  efficiency `hmc.hmc_sample` (--hmc-burn iterations in --hmc-windows adapting windows, --hmc-steps kept) and `ensemble_sample` with the
             stretch move (--ens-burn, --ens-steps kept, every --ens-thin-th) from the same starts.  Per chain (every 16th walker
             of status 0) the integrated autocorrelation time with Sokal's window, the largest over the moving coordinates, in
             iterations; its median over the chains; effective samples per second of GPU time = walkers / (tau x seconds per
             iteration), the seconds from the event timing of that sampler's device entry.  A tau above a tenth of the kept
             length is a lower bound, and the figure says so.
No threshold is fixed for either figure.  One JSON line, also written to --out.
python tools/hmc_timing.py [--config C] [--walkers 4096] [--nleap 8] [--out profiles/hmc_timing.json]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mcalf_amd  # noqa: E402
from mcalf_amd import _lib, ensemble, hmc, workloads  # noqa: E402


def _synth(kw, p):
    """The config's truth spectrum from the device itself (the oracle is test infrastructure)."""
    with mcalf_amd.als_fitter(None, **kw) as fit:
        return fit.model_batch(p)[0]


def _start(fit):
    """The cube point of the `maximize_batch` optimum from the config's truth: ten components, the eleventh slot and the
    fillers mid-box with the fillers' columns at the low end, the resolution mid-box."""
    lo, hi = fit._lo, fit._hi
    p = 0.5 * (lo + hi)
    s = fit.startind
    truth = workloads.truth_vector(10)
    p[s:s + truth.size] = truth
    p[fit.endind::3] = lo[fit.endind::3] + 0.05 * (hi - lo)[fit.endind::3]
    P, _, status, _ = fit.maximize_batch(p.reshape(1, -1))
    best = P[0] if status[0] >= 0 else p
    u = np.clip((best - lo) / np.where(hi > lo, hi - lo, 1.0), 0.02, 0.98)
    u[s] = (10.5 - lo[s]) / (hi[s] - lo[s])
    return u


def _timed(fit, stream, call):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record(stream)
    rc = call()
    b.record(stream)
    b.synchronize()
    assert rc == 0, fit._lib.mcalf_last_error(fit._ctx)
    return a.elapsed_time(b)


def _iteration_times(fit, U, eps, scale, args):
    """(ms per HMC iteration, ms of nleap bare gradient launches, ms per stretch iteration), medians over --reps calls."""
    n, nd = U.shape
    f64 = dict(dtype=torch.float64, device="cuda")
    dU0, dU, dTh, dG = (torch.empty((n, nd), **f64) for _ in range(4))
    dL = torch.empty(n, **f64)
    dS, dN, dD = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
    stream = torch.cuda.current_stream()
    st = C.c_void_p(stream.cuda_stream)
    lib, ctx = fit._lib, fit._ctx
    scale = np.ascontiguousarray(scale, dtype=float)
    t_hmc, t_bare, t_ens = [], [], []
    cur, it = np.ascontiguousarray(U), 10 ** 6
    for k in range(args.warmup + args.reps):
        dU0.copy_(torch.from_numpy(cur))
        opts = _lib.mcalf_hmc_opts(args.iters, 1, args.nleap, 0, eps, 0.1, 0, it)
        ms = _timed(fit, stream, lambda: lib.mcalf_hmc_batch_device(ctx, dU0.data_ptr(), n, scale.ctypes.data, None, C.addressof(opts), dU.data_ptr(),
                                                                    dTh.data_ptr(), dL.data_ptr(), dS.data_ptr(), dN.data_ptr(), dD.data_ptr(), None, None, st))
        cur, it = dU.cpu().numpy(), it + args.iters

        def bare():
            for _ in range(args.nleap):
                rc = lib.mcalf_loglike_grad_batch_device(ctx, dTh.data_ptr(), n, dL.data_ptr(), dG.data_ptr(), st)
                if rc:
                    return rc
            return 0
        msb = _timed(fit, stream, bare)
        eo = _lib.mcalf_ens_opts(args.iters, 1, _lib.MCALF_ENS_STRETCH, 0, 2.0, 0, it)
        mse = _timed(fit, stream, lambda: lib.mcalf_ensemble_batch_device(ctx, dU0.data_ptr(), n, C.addressof(eo), dU.data_ptr(), None, dL.data_ptr(),
                                                                          dS.data_ptr(), dN.data_ptr(), None, None, st))
        if k >= args.warmup:
            t_hmc.append(ms / args.iters)
            t_bare.append(msb)
            t_ens.append(mse / args.iters)
    return float(np.median(t_hmc)), float(np.median(t_bare)), float(np.median(t_ens))


def _tau(res, moving, every=16):
    """Median over chains of the largest Sokal tau over the moving coordinates, in iterations; the chains taken."""
    ok = np.flatnonzero(res.status == 0)[::every]
    taus = [max(ensemble.sokal_tau(res.cube[:, w, k]) for k in moving) * res.thin for w in ok]
    return float(np.median(taus)), len(taus)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C")
    ap.add_argument("--walkers", type=int, default=4096)
    ap.add_argument("--nleap", type=int, default=8)
    ap.add_argument("--ball", type=float, default=0.005)
    ap.add_argument("--hmc-burn", type=int, default=200)
    ap.add_argument("--hmc-windows", type=int, default=10)
    ap.add_argument("--hmc-steps", type=int, default=150)
    ap.add_argument("--ens-burn", type=int, default=1000)
    ap.add_argument("--ens-steps", type=int, default=2000)
    ap.add_argument("--ens-thin", type=int, default=10)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    kw, _, seed = workloads.config(args.config, _synth)
    n = args.walkers
    with mcalf_amd.als_fitter(None, **kw) as fit:
        start = _start(fit)
        moving = [k for k in range(fit.ndim) if k != fit.startind and fit._hi[k] > fit._lo[k]]
        h = hmc.hmc_sample(fit, n, args.hmc_steps, burn=args.hmc_burn, start=start, ball=args.ball, seed=seed, eps=0.1, nleap=args.nleap, windows=args.hmc_windows)
        e = fit.ensemble_sample(n, args.ens_steps, burn=args.ens_burn, thin=args.ens_thin, start=start, ball=args.ball, seed=seed, move="stretch")
        ms_hmc, ms_bare, ms_ens = _iteration_times(fit, h.last, h.eps, h.scale, args)
        tau_h, chains_h = _tau(h, moving)
        tau_e, chains_e = _tau(e, moving)
        out = {"config": args.config, "npix": int(fit.obj_wl.size), "ndim": int(fit.ndim), "walkers": n, "nleap": args.nleap,
               "hmc_ms_per_iteration": round(ms_hmc, 3), "bare_gradient_launches_ms": round(ms_bare, 3),
               "iteration_over_bare": round(ms_hmc / ms_bare, 4), "stretch_ms_per_iteration": round(ms_ens, 3),
               "hmc": {"burn": args.hmc_burn, "windows": args.hmc_windows, "kept": args.hmc_steps, "eps": round(h.eps, 5), "window_accept": np.round(h.window_accept, 3).tolist(), "window_eps": np.round(h.window_eps, 4).tolist(),
                       "acceptance": round(float(h.accept_frac[h.status == 0].mean()), 3), "dead": int(h.ndead.sum()), "status0": int((h.status == 0).sum()),
                       "mean_logL_last": round(float(h.logL[-1][h.status == 0].mean()), 2),
                       "tau_iterations": round(tau_h, 2), "chains": chains_h, "tau_is_lower_bound": bool(tau_h > 0.1 * args.hmc_steps),
                       "ess_per_gpu_second": round(n / (tau_h * ms_hmc * 1e-3), 1)},
               "stretch": {"burn": args.ens_burn, "kept": args.ens_steps, "thin": args.ens_thin,
                           "acceptance": round(float(e.accept_frac[e.status == 0].mean()), 3), "mean_logL_last": round(float(e.logL[-1][e.status == 0].mean()), 2),
                           "tau_iterations": round(tau_e, 2), "chains": chains_e, "tau_is_lower_bound": bool(tau_e > 0.1 * args.ens_steps),
                           "ess_per_gpu_second": round(n / (tau_e * ms_ens * 1e-3), 1)}}
        out["hmc_over_stretch_ess_per_gpu_second"] = round(out["hmc"]["ess_per_gpu_second"] / out["stretch"]["ess_per_gpu_second"], 4)
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
