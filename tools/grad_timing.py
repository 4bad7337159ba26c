"""Device-entry timing of the analytic gradient, of the model Jacobian's products and of the Hessian-vector product: ms per
step of mcalf_loglike_grad_batch_device, mcalf_model_jvp_batch_device, mcalf_model_vjp_batch_device, the Fisher product (one
JVP, the weights, one VJP) and mcalf_loglike_hvp_batch_device (also over two gradient steps, what a finite difference of
the gradient costs) next to mcalf_loglike_batch_device on the same rows (configs C and E by default), HIP events on
one stream, warm-up, median over `--steps` steps; one JSON line.  python tools/grad_timing.py [--configs C E] [--steps 20] [--warmup 3] [--batch N]"""
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
from mcalf_amd import workloads  # noqa: E402


def _synth(kw, p):
    """The config's truth spectrum from the device itself (the oracle is test infrastructure)."""
    with mcalf_amd.als_fitter(None, **kw) as fit:
        return fit.model_batch(p)[0]


def _time(fn, steps, warmup):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["C", "E"])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=0, help="rows per step (0: the config's batch)")
    args = ap.parse_args()
    out = {"steps": args.steps, "warmup": args.warmup, "configs": {}}
    for name in args.configs:
        kw, batch, seed = workloads.config(name, _synth)
        batch = args.batch or batch
        P = workloads.draw_P(kw, batch, np.random.default_rng(seed), damped=2 if name.upper() == "E" else 0)
        with mcalf_amd.als_fitter(None, **kw) as fit:
            dP = torch.from_numpy(P).cuda()
            dL = torch.empty(batch, dtype=torch.float64, device="cuda")
            dG = torch.empty(P.shape, dtype=torch.float64, device="cuda")
            s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            lib, ctx = fit._lib, fit._ctx

            def logl():
                assert lib.mcalf_loglike_batch_device(ctx, dP.data_ptr(), batch, dL.data_ptr(), s) == 0

            def grad():
                assert lib.mcalf_loglike_grad_batch_device(ctx, dP.data_ptr(), batch, dL.data_ptr(), dG.data_ptr(), s) == 0

            # tangents and cotangents of order one per column / pixel; W = 1 / err^2 (the configs have no bad pixels)
            rng = np.random.default_rng(seed + 100)
            dV = torch.from_numpy(rng.uniform(-1.0, 1.0, P.shape)).cuda()
            dQ = torch.from_numpy(rng.normal(0.0, 1.0, (batch, fit.obj.size))).cuda()
            dM = torch.empty_like(dQ)
            dW = torch.from_numpy(1.0 / fit.obj_noise ** 2).cuda()

            def jvp():
                assert lib.mcalf_model_jvp_batch_device(ctx, dP.data_ptr(), dV.data_ptr(), batch, dM.data_ptr(), s) == 0

            def vjp():
                assert lib.mcalf_model_vjp_batch_device(ctx, dP.data_ptr(), dQ.data_ptr(), batch, dG.data_ptr(), s) == 0

            def fisher():
                jvp()
                dM.mul_(dW)
                assert lib.mcalf_model_vjp_batch_device(ctx, dP.data_ptr(), dM.data_ptr(), batch, dG.data_ptr(), s) == 0

            dHV = torch.empty_like(dG)

            def hvp():
                assert lib.mcalf_loglike_hvp_batch_device(ctx, dP.data_ptr(), dV.data_ptr(), batch, dHV.data_ptr(), s) == 0

            t_l = _time(logl, args.steps, args.warmup)
            t_g = _time(grad, args.steps, args.warmup)
            t_j = _time(jvp, args.steps, args.warmup)
            t_v = _time(vjp, args.steps, args.warmup)
            t_f = _time(fisher, args.steps, args.warmup)
            t_h = _time(hvp, args.steps, args.warmup)
        out["configs"][name] = {"batch": batch, "npix": int(fit.obj.size), "ndim": int(P.shape[1]), "logl_ms": round(t_l, 4),
                                "grad_ms": round(t_g, 4), "ratio": round(t_g / t_l, 3), "jvp_ms": round(t_j, 4),
                                "vjp_ms": round(t_v, 4), "fisher_ms": round(t_f, 4), "jvp_over_grad": round(t_j / t_g, 3),
                                "hvp_ms": round(t_h, 4), "hvp_over_two_grads": round(t_h / (2 * t_g), 3)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
