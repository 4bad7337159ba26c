"""Timing of the ensemble sampler's iteration on BASELINE configs C (4000 pixels, ndim 47) with 4096 walkers and B (4000 pixels,
ndim 25) with 1024.  The walkers start in a ball of half-width 0.05 around the best of as many uniform points of the cube and
make --burn iterations first (host entry, not timed), so that the timed iterations both accept and reject.
Per run and move, on the same walkers:
  device  mcalf_ensemble_batch_device between HIP events on one stream, --iters iterations per call (each two half-steps: propose
          kernel, cube logL launch over the m = n / 2 trial rows, decide kernel), the run continued from call to call; ms per
          iteration, median of --reps calls after --warmup;
  bare    two mcalf_loglike_cube_batch_device launches of m rows between HIP events: what an iteration's likelihood work costs
          without the sampler's kernels; median of --reps after --warmup;
  numpy   what the library offered before: the numpy restatement of the state machine (tests/ens_reference.py) around
          `loglike_cube_batch`, one host round trip per half-step (wall clock, --iters iterations, median of 3 calls).
The device route and the numpy route must agree bit for bit over the first call (exit status 1 otherwise).  No ratio is fixed
in advance.  One JSON line, also written to --out.
python tools/ens_timing.py [--runs C:4096,B:1024] [--iters 4] [--reps 20] [--warmup 3] [--burn 20] [--gauss] [--out profiles/ens_timing.json]
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
import ens_reference as er  # noqa: E402
import prior_reference as prr  # noqa: E402
from mcalf_amd import _lib, workloads  # noqa: E402

MOVES = {"stretch": er.STRETCH, "de": er.DE}


def _synth(kw, p):
    """The config's truth spectrum from the device itself (the oracle is test infrastructure)."""
    with mcalf_amd.als_fitter(None, **kw) as fit:
        return fit.model_batch(p)[0]


class _Device:
    """The device entry on torch tensors that stay allocated from call to call."""

    def __init__(self, fit, n):
        self.fit, self.n = fit, n
        f64 = dict(dtype=torch.float64, device="cuda")
        self.U0, self.U = torch.empty((n, fit.ndim), **f64), torch.empty((n, fit.ndim), **f64)
        self.L, self.LY = torch.empty(n, **f64), torch.empty(n, **f64)
        self.S, self.N = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
        self.stream = torch.cuda.current_stream()

    def _timed(self, call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        rc = call()
        b.record(self.stream)
        b.synchronize()
        assert rc == 0, self.fit._lib.mcalf_last_error(self.fit._ctx)
        return a.elapsed_time(b)

    def advance(self, U0, iters, move, seed, first_iter):
        """ms of one call of `iters` iterations from the host rows U0, and (U, logL, status, naccept)."""
        self.U0.copy_(torch.from_numpy(U0))
        opts = _lib.mcalf_ens_opts(iters, 1, MOVES[move], 0, er.default_scale(MOVES[move], self.fit.ndim), seed, first_iter)
        ms = self._timed(lambda: self.fit._lib.mcalf_ensemble_batch_device(
            self.fit._ctx, self.U0.data_ptr(), self.n, C.addressof(opts), self.U.data_ptr(), None, self.L.data_ptr(), self.S.data_ptr(),
            self.N.data_ptr(), None, None, C.c_void_p(self.stream.cuda_stream)))
        return ms, tuple(t.cpu().numpy() for t in (self.U, self.L, self.S, self.N))

    def bare(self):
        """ms of two cube logL launches of m rows over the current walkers' halves."""
        m, lib, ctx, st = self.n // 2, self.fit._lib, self.fit._ctx, C.c_void_p(self.stream.cuda_stream)

        def two():
            rc = lib.mcalf_loglike_cube_batch_device(ctx, self.U[:m].data_ptr(), m, None, self.LY[:m].data_ptr(), st)
            return rc or lib.mcalf_loglike_cube_batch_device(ctx, self.U[m:].data_ptr(), m, None, self.LY[m:].data_ptr(), st)
        return self._timed(two)


def _set_gauss(fit):
    """--gauss: a Gaussian prior on the four coordinates behind the ncomp slot, centred on the middle of the box, a quarter of
    the box wide."""
    mu, sigma = np.zeros(fit.ndim), np.zeros(fit.ndim)
    k = slice(fit.startind + 1, fit.startind + 5)
    mu[k], sigma[k] = 0.5 * (fit._lo[k] + fit._hi[k]), 0.25 * (fit._hi[k] - fit._lo[k])
    fit.set_gauss_prior(mu, sigma)


def _run(fit, n, move, seed, args):
    logl = lambda U: fit.loglike_cube_batch(U, return_theta=False)
    rng = np.random.default_rng(seed)
    draws = rng.random((n, fit.ndim))
    best = draws[np.nanargmax(logl(draws))]
    U = np.clip(best + 0.05 * (2.0 * rng.random((n, fit.ndim)) - 1.0), 0.0, 1.0)
    U = np.ascontiguousarray(fit.ensemble_batch(U, args.burn, move=move, seed=seed, chain=False)[0])
    dev = _Device(fit, n)
    it = args.burn
    # the first call: the device route and the numpy route on the same walkers
    _, got = dev.advance(U, args.iters, move, seed, it)
    t_np = []
    for _ in range(3):
        t0 = time.perf_counter()
        if args.gauss:
            ref = prr.ensemble(logl, lambda Y: fit.lnprior_batch(Y, cube=True), U, args.iters, args.iters, MOVES[move], None, seed, it)
        else:
            ref = er.ensemble(logl, U, args.iters, args.iters, MOVES[move], None, seed, it)
        t_np.append((time.perf_counter() - t0) * 1e3 / args.iters)
    same = np.array_equal(got[0], ref[0]) and got[1].tobytes() == ref[1].tobytes() and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    t_dev, t_bare, acc = [], [], []
    for k in range(args.warmup + args.reps):
        ms, got = dev.advance(U, args.iters, move, seed, it)
        U, it = np.ascontiguousarray(got[0]), it + args.iters
        bare = dev.bare()
        if k >= args.warmup:
            t_dev.append(ms / args.iters)
            t_bare.append(bare)
            acc.append(float(got[3].mean()) / args.iters)
    med = lambda v: round(float(np.median(v)), 4)
    return {"move": move, "walkers": n, "routes_agree_bit_for_bit": bool(same), "acceptance": round(float(np.mean(acc)), 3),
            "device_entry_ms_per_iteration": med(t_dev), "device_entry_min_max": [round(min(t_dev), 4), round(max(t_dev), 4)],
            "two_bare_launches_ms": med(t_bare), "two_bare_launches_min_max": [round(min(t_bare), 4), round(max(t_bare), 4)],
            "numpy_route_ms_per_iteration": med(t_np), "device_over_bare": round(float(np.median(t_dev) / np.median(t_bare)), 3),
            "numpy_over_device": round(float(np.median(t_np) / np.median(t_dev)), 2)}, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="C:4096,B:1024")
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burn", type=int, default=20)
    ap.add_argument("--gauss", action="store_true", help="a Gaussian prior on four coordinates (mcalf_set_gauss_prior)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out, same = {"gauss": args.gauss, "iterations_per_call": args.iters, "reps": args.reps, "warmup": args.warmup, "burn": args.burn, "runs": []}, True
    for run in args.runs.split(","):
        name, n = run.split(":")
        kw, _, seed = workloads.config(name, _synth)
        with mcalf_amd.als_fitter(None, **kw) as fit:
            if args.gauss:
                _set_gauss(fit)
            for move in MOVES:
                row, ok = _run(fit, int(n), move, seed, args)
                same &= ok
                out["runs"].append(dict({"config": name, "npix": int(fit.obj_wl.size), "ndim": int(fit.ndim)}, **row))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
