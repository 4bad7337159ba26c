"""Timing of the tempered ensemble sampler's iteration on BASELINE configs C (4000 pixels, ndim 47) with 8 temperatures of 512
walkers and B (4000 pixels, ndim 25) with 4 of 256, on the ladder `tempering.default_ladder(T, 1e-4)`.  The walkers of every
rung start in a ball of half-width 0.05 around the best of as many uniform points of the cube and make --burn iterations first
(host entry, not timed), so that the timed iterations both accept and reject.
Per run and move, on the same walkers, between HIP events on one stream, ms per iteration, median of --reps calls after --warmup:
  swaps     mcalf_tempered_batch_device with swap_every = 1, --iters iterations per call (each two half-steps -- propose kernel,
            cube logL launch over the T m trial rows, decide kernel -- and a swap kernel), the run continued from call to call;
  no_swaps  the same with swap_every = 0;
  bare      two mcalf_loglike_cube_batch_device launches of T m rows: what an iteration's likelihood work costs without the
            sampler's kernels;
  separate  T mcalf_ensemble_batch_device calls of n walkers, one per rung: the route without exchanges that the library
            offered before.
The first timed call of `swaps` must equal the numpy restatement (tests/pt_reference.py around `loglike_cube_batch`) bit for bit
(exit status 1 otherwise).  No ratio is fixed in advance.  One JSON line, also written to --out.
python tools/pt_timing.py [--runs C:8x512,B:4x256] [--moves stretch] [--iters 4] [--reps 20] [--warmup 3] [--burn 20] [--gauss] [--out profiles/pt_timing.json]
--gauss: the same runs under a Gaussian prior on four coordinates (mcalf_set_gauss_prior); the numpy route is then
tests/prior_reference.py's."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mcalf_amd  # noqa: E402
import ens_reference as er  # noqa: E402
import pt_reference as pr  # noqa: E402
import prior_reference as prr  # noqa: E402
from mcalf_amd import _lib, tempering, workloads  # noqa: E402

MOVES = {"stretch": er.STRETCH, "de": er.DE}


def _synth(kw, p):
    """The config's truth spectrum from the device itself (the oracle is test infrastructure)."""
    with mcalf_amd.als_fitter(None, **kw) as fit:
        return fit.model_batch(p)[0]


class _Device:
    """The device entries on torch tensors that stay allocated from call to call."""

    def __init__(self, fit, T, n, betas):
        self.fit, self.T, self.n, self.betas = fit, T, n, np.ascontiguousarray(betas, dtype=float)
        f64 = dict(dtype=torch.float64, device="cuda")
        self.U0, self.U = torch.empty((T, n, fit.ndim), **f64), torch.empty((T, n, fit.ndim), **f64)
        self.L, self.LY = torch.empty((T, n), **f64), torch.empty(T * n, **f64)
        self.S, self.N, self.W = (torch.empty((T, n), dtype=torch.int32, device="cuda") for _ in range(3))
        self.stream = torch.cuda.current_stream()

    def _timed(self, call):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(self.stream)
        rc = call()
        b.record(self.stream)
        b.synchronize()
        assert rc == 0, self.fit._lib.mcalf_last_error(self.fit._ctx)
        return a.elapsed_time(b)

    def _scale(self, move):
        return er.default_scale(MOVES[move], self.fit.ndim)

    def advance(self, U0, iters, move, seed, first_iter, swap_every):
        """ms of one tempered call of `iters` iterations from the host rows U0, and (U, logL, status, naccept, nswap)."""
        self.U0.copy_(torch.from_numpy(U0))
        opts = _lib.mcalf_pt_opts(iters, 1, MOVES[move], self.T, swap_every, 0, self._scale(move), seed, first_iter)
        ms = self._timed(lambda: self.fit._lib.mcalf_tempered_batch_device(
            self.fit._ctx, self.U0.data_ptr(), self.n, self.betas.ctypes.data, C.addressof(opts), self.U.data_ptr(), None, self.L.data_ptr(),
            self.S.data_ptr(), self.N.data_ptr(), self.W.data_ptr(), None, None, C.c_void_p(self.stream.cuda_stream)))
        return ms, tuple(t.cpu().numpy() for t in (self.U, self.L, self.S, self.N, self.W[:self.T - 1]))

    def separate(self, iters, move, seed, first_iter):
        """ms of T ensemble calls of n walkers, one per rung, from the rows advance() was last given."""
        opts = _lib.mcalf_ens_opts(iters, 1, MOVES[move], 0, self._scale(move), seed, first_iter)
        lib, ctx, st = self.fit._lib, self.fit._ctx, C.c_void_p(self.stream.cuda_stream)

        def calls():
            for t in range(self.T):
                rc = lib.mcalf_ensemble_batch_device(ctx, self.U0[t].data_ptr(), self.n, C.addressof(opts), self.U[t].data_ptr(), None, self.L[t].data_ptr(),
                                                     self.S[t].data_ptr(), self.N[t].data_ptr(), None, None, st)
                if rc:
                    return rc
            return 0
        return self._timed(calls)

    def bare(self):
        """ms of two cube logL launches of T m rows over the starts' rows."""
        rows, lib, ctx, st = self.T * self.n // 2, self.fit._lib, self.fit._ctx, C.c_void_p(self.stream.cuda_stream)
        flat = self.U0.view(self.T * self.n, self.fit.ndim)

        def two():
            rc = lib.mcalf_loglike_cube_batch_device(ctx, flat[:rows].data_ptr(), rows, None, self.LY[:rows].data_ptr(), st)
            return rc or lib.mcalf_loglike_cube_batch_device(ctx, flat[rows:].data_ptr(), rows, None, self.LY[rows:].data_ptr(), st)
        return self._timed(two)


def _set_gauss(fit):
    """--gauss: a Gaussian prior on the four coordinates behind the ncomp slot, centred on the middle of the box, a quarter of
    the box wide."""
    mu, sigma = np.zeros(fit.ndim), np.zeros(fit.ndim)
    k = slice(fit.startind + 1, fit.startind + 5)
    mu[k], sigma[k] = 0.5 * (fit._lo[k] + fit._hi[k]), 0.25 * (fit._hi[k] - fit._lo[k])
    fit.set_gauss_prior(mu, sigma)


def _run(fit, T, n, move, seed, args):
    logl = lambda U: fit.loglike_cube_batch(U, return_theta=False)
    betas = tempering.default_ladder(T, 1e-4)
    rng = np.random.default_rng(seed)
    draws = rng.random((T * n, fit.ndim))
    best = draws[np.nanargmax(logl(draws))]
    U = np.clip(best + 0.05 * (2.0 * rng.random((T, n, fit.ndim)) - 1.0), 0.0, 1.0)
    U = np.ascontiguousarray(fit.tempered_batch(U, betas, args.burn, move=move, seed=seed, chain=False)[0])
    dev = _Device(fit, T, n, betas)
    it = args.burn
    # the first call: the device route and the numpy route on the same walkers
    _, got = dev.advance(U, args.iters, move, seed, it, 1)
    if args.gauss:
        ref = prr.tempered(logl, lambda Y: fit.lnprior_batch(Y, cube=True), U, betas, args.iters, args.iters, 1, MOVES[move], None, seed, it, 0)
    else:
        ref = pr.tempered(logl, U, betas, args.iters, args.iters, 1, MOVES[move], None, seed, it, 0)
    same = np.array_equal(got[0], ref[0]) and got[1].tobytes() == ref[1].tobytes() and all(np.array_equal(got[k], ref[k]) for k in (2, 3, 4))
    t = {"swaps": [], "no_swaps": [], "bare": [], "separate": []}
    acc, swp = [], []
    for k in range(args.warmup + args.reps):
        no_swaps, _ = dev.advance(U, args.iters, move, seed, it, 0)
        separate = dev.separate(args.iters, move, seed, it)
        bare = dev.bare()
        swaps, got = dev.advance(U, args.iters, move, seed, it, 1)                 # (last: the run goes on from its walkers)
        U, it = np.ascontiguousarray(got[0]), it + args.iters
        if k >= args.warmup:
            for name, ms in (("swaps", swaps / args.iters), ("no_swaps", no_swaps / args.iters), ("bare", bare), ("separate", separate / args.iters)):
                t[name].append(ms)
            acc.append(got[3].mean(axis=1) / args.iters)
            swp.append(got[4].sum(axis=1) / np.maximum(tempering.swap_rounds(it - args.iters, args.iters, 1, T) * n, 1))
    med = lambda v: round(float(np.median(v)), 4)
    row = {"move": move, "temperatures": T, "walkers": n, "routes_agree_bit_for_bit": bool(same),
           "acceptance_per_rung": np.round(np.mean(acc, axis=0), 3).tolist(), "swap_fractions": np.round(np.mean(swp, axis=0), 3).tolist()}
    for name, label in (("swaps", "tempered_entry_ms_per_iteration"), ("no_swaps", "tempered_entry_without_swaps_ms_per_iteration"),
                        ("bare", "two_bare_launches_ms"), ("separate", "separate_ensemble_calls_ms_per_iteration")):
        row[label] = med(t[name])
        row[label.replace("_ms_per_iteration", "").replace("_ms", "") + "_min_max"] = [round(min(t[name]), 4), round(max(t[name]), 4)]
    row["tempered_over_bare"] = round(float(np.median(t["swaps"]) / np.median(t["bare"])), 3)
    row["separate_over_tempered"] = round(float(np.median(t["separate"]) / np.median(t["swaps"])), 2)
    return row, same


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", default="C:8x512,B:4x256")
    ap.add_argument("--moves", default="stretch")
    ap.add_argument("--iters", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--burn", type=int, default=20)
    ap.add_argument("--gauss", action="store_true", help="a Gaussian prior on four coordinates (mcalf_set_gauss_prior)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    out, same = {"gauss": args.gauss, "iterations_per_call": args.iters, "reps": args.reps, "warmup": args.warmup, "burn": args.burn, "runs": []}, True
    for run in args.runs.split(","):
        name, shape = run.split(":")
        T, n = (int(v) for v in shape.split("x"))
        kw, _, seed = workloads.config(name, _synth)
        with mcalf_amd.als_fitter(None, **kw) as fit:
            if args.gauss:
                _set_gauss(fit)
            for move in args.moves.split(","):
                row, ok = _run(fit, T, n, move, seed, args)
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
