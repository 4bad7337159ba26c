#!/usr/bin/env python3
"""A/B of two builds of the library: every plan of the likelihood's entries and every analysis entry once, each case in a FRESH
context, each build in a process of its own (MCALF_HIP_LIB); outputs compared bit for bit and the whole mcalf_last_launch record
field by field.

    python tools/ab_bits.py libA.so libB.so      # exit status 1 when anything differs
    python tools/ab_bits.py --child out.json     # the cases alone, with the library MCALF_HIP_LIB names (e.g. under a profiler)

Cases: the device entry (one block, three blocks), the zero-copy small call, the streaming launch, the row-block pipeline
(MCALF_STREAM=0), chi2, model and single-component output, the cube entry (small, streaming, staged), a wide-LSF context,
single-tile (C, B) and tiled (E) spectra; and, on a 300-pixel problem under both conv modes, with and without fillers, with
count slots from below 0 to above ncompmax: loglike_grad, model JVP / VJP, loglike_hvp, the Fisher product, eqw in both
indexings with and without Wblend, maximize."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(path):
    import ctypes as C
    import numpy as np
    import torch
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import mcalf_amd
    from mcalf_amd import _lib, workloads
    from cases import oracle_synth
    res = {}

    def bits(a):
        return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel().tolist()

    def record(fit):
        ll = fit.last_launch()
        return {f: int(getattr(ll, f)) for f, _ in ll._fields_}

    def case(name, kw, fn, env=None):
        """fn(fit) -> arrays, on a fresh context created under `env`."""
        for k, v in (env or {}).items():
            os.environ[k] = v
        try:
            with mcalf_amd.als_fitter(None, **kw) as fit:
                out = fn(fit)
                res[name] = {"out": [bits(a) for a in out], "last": record(fit)}
        finally:
            for k in env or {}:
                del os.environ[k]

    def device(P, chunks=0):
        def run(fit):
            n = P.shape[0]
            fit.set_chunks(chunks)
            dP = torch.from_numpy(P).cuda()
            out = torch.empty(n, dtype=torch.float64, device="cuda")
            st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
            _lib.check(fit._lib.mcalf_loglike_batch_device(fit._ctx, dP.data_ptr(), n, out.data_ptr(), st), fit._ctx)
            torch.cuda.synchronize()
            return [out.cpu().numpy()]
        return run

    def onecomp(fit):
        s = fit.startind
        z = 0.5 * float(fit._lo[s + 2] + fit._hi[s + 2])
        return [fit.reconstruct_onecomp(7.5, 0.95, 13.2 + 0.1 * k, z, 12.0 + k) for k in range(3)]

    for cfg, n in (("C", 4096), ("E", 1024), ("B", 1024)):
        kw, _, seed = workloads.config(cfg, oracle_synth)
        rng = np.random.default_rng(seed)
        P = workloads.draw_P(kw, n, rng, damped=2 if cfg == "E" else 0)
        cubes = rng.random((n, P.shape[1]))
        case(cfg + " dev", kw, device(P))
        case(cfg + " dev chunks 3", kw, device(P, 3))
        case(cfg + " small", kw, lambda fit: [fit.loglike_batch(P[:7])])              # the one-launch variant
        case(cfg + " host", kw, lambda fit: [fit.loglike_batch(P)])                   # streaming launch (zero-copy where it does not qualify)
        case(cfg + " chi2", kw, lambda fit: [fit.chi2_batch(P)])
        case(cfg + " model", kw, lambda fit: [fit.model_batch(P[:5]), fit.model_batch(P[:5], targonly=True)])
        case(cfg + " onecomp", kw, onecomp)
        case(cfg + " cube small", kw, lambda fit: list(fit.loglike_cube_batch(cubes[:700])))
        case(cfg + " cube", kw, lambda fit: list(fit.loglike_cube_batch(cubes)))
    for cfg, n in (("C", 2600), ("E", 1400), ("E", 13200)):                             # beyond 65536 parameters
        kw, _, seed = workloads.config(cfg, oracle_synth)
        rng = np.random.default_rng(seed + 1)
        P = workloads.draw_P(kw, n, rng, damped=2 if cfg == "E" else 0)
        cubes = rng.random((n, P.shape[1]))
        tag = "%s %d" % (cfg, n)
        case(tag + " host", kw, lambda fit: [fit.loglike_batch(P)])
        case(tag + " pipelined", kw, lambda fit: [fit.loglike_batch(P)], env={"MCALF_STREAM": "0"})
        case(tag + " cube", kw, lambda fit: list(fit.loglike_cube_batch(cubes)))            # E 13200: staged
        case(tag + " cube, no stream", kw, lambda fit: list(fit.loglike_cube_batch(cubes)), env={"MCALF_STREAM": "0"})
    # a wide-LSF context: the smallest geometry of tests/test_gpu_wide_lsf.py
    rng = np.random.default_rng(333)
    wl = np.linspace(6180.0, 6220.0, 335)[1:-1]
    kw = dict(fitrange=[[6180.0, 6220.0]], fitlines=["CIV 1548", "CIV 1550"], linepars=[(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8)],
              ncomp=[1, 3], nfill=2, specres=[6.0, 9.0], contval=[0.9, 1.1], Nrange=[12.0, 14.5], brange=[5.0, 40.0], zrange=[2.995, 3.012],
              spectrum=(wl, 1 + rng.normal(0, 0.03, 333), rng.uniform(0.01, 0.05, 333)), velstep=0.0031)
    P = workloads.draw_P(kw, 20, rng)
    cubes = rng.random((20, P.shape[1]))
    case("wide dev", kw, device(P))
    case("wide host", kw, lambda fit: [fit.loglike_batch(P), fit.chi2_batch(P)])
    case("wide model", kw, lambda fit: [fit.model_batch(P[:3])])
    case("wide onecomp", kw, lambda fit: [fit.reconstruct_onecomp(8.0, 0.95, 13.5, 3.0, 20.0)])
    case("wide cube", kw, lambda fit: list(fit.loglike_cube_batch(cubes)))
    # the analysis entries (gradient, Jacobian and Hessian products, Fisher product, equivalent widths, fit): both conv modes, with
    # and without fillers, rows whose count slot is 0, fractional, ncompmax and above it
    for mode in ("numpy", "jax"):
        for nfill in (0, 2):
            rng = np.random.default_rng(444 + nfill)
            wl = np.linspace(6185.0, 6215.0, 302)[1:-1]
            kw = dict(fitrange=[[6185.0, 6215.0]], fitlines=["CIV 1548", "CIV 1550"], linepars=[(1548.204, 0.1899, 2.643e8), (1550.781, 0.09475, 2.628e8)],
                      ncomp=[0, 3], nfill=nfill, specres=[6.0, 9.0], contval=[0.9, 1.1], Nrange=[12.5, 14.5], brange=[8.0, 40.0], zrange=[2.998, 3.004],
                      spectrum=(wl, 1 + rng.normal(0, 0.03, 300), np.full(300, 0.03)), conv_mode=mode)
            P = workloads.draw_P(kw, 12, rng)
            P[:, 2] = [0.0, 0.7, 1.0, 1.5, 2.0, 2.999, 3.0, 3.5, 4.2, 1e9, -0.5, -2.0]        # (startind 2: R and the continuum are free)
            V = rng.uniform(-1.0, 1.0, P.shape) * 1e-3
            Q = rng.normal(0.0, 1.0, (12, 300))
            tag = "%s nfill %d " % (mode, nfill)
            case(tag + "grad", kw, lambda fit: list(fit.loglike_grad_batch(P)))
            case(tag + "jvp", kw, lambda fit: [fit.model_jvp_batch(P, V)])
            case(tag + "vjp", kw, lambda fit: [fit.model_vjp_batch(P, Q)])
            case(tag + "hvp", kw, lambda fit: [fit.loglike_hvp_batch(P, V)])
            case(tag + "fisher", kw, lambda fit: [fit.fisher_matvec_batch(P, V)])
            for ref in (False, True):
                name = tag + ("eqw as written" if ref else "eqw layout")
                case(name, kw, lambda fit: list(fit.eqw_batch(P, reference_indexing=ref)))
                case(name + ", no blend", kw, lambda fit: [fit.eqw_batch(P, reference_indexing=ref, blend=False)[0]])
            case(tag + "maximize", kw, lambda fit: list(fit.maximize_batch(P, max_iter=4)))
    json.dump(res, open(path, "w"))


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
        sys.exit(0)
    outs = []
    for k, lib in enumerate(sys.argv[1:3]):
        path = "/tmp/ab_bits_%d.json" % k
        env = dict(os.environ, MCALF_HIP_LIB=os.path.abspath(lib))
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=env, check=True)
        outs.append(json.load(open(path)))
    bad = 0
    assert outs[0].keys() == outs[1].keys()
    for name in outs[0]:
        a, b = outs[0][name], outs[1][name]
        rows = sum(len(x) for x in a["out"])
        diff = sum(x != y for u, v in zip(a["out"], b["out"]) for x, y in zip(u, v)) + sum(len(u) != len(v) for u, v in zip(a["out"], b["out"]))
        fields = [f for f in a["last"] if a["last"][f] != b["last"][f]]
        bad += bool(diff) + bool(fields)
        print("%-24s %7d values %s; record %s; path %d blocks %d grid %d items %d" % (
            name, rows, "bit-equal" if not diff else "DIFFERENT in %d" % diff,
            "equal" if not fields else "DIFFERENT in %s (%s)" % (fields, [(a["last"][f], b["last"][f]) for f in fields]),
            a["last"]["path"], a["last"]["row_blocks"], a["last"]["grid"], a["last"]["items"]))
    for cfg in ("C", "E", "B"):
        print(cfg, "within build A: host == dev", outs[0][cfg + " host"]["out"] == outs[0][cfg + " dev"]["out"],
              "; build B:", outs[1][cfg + " host"]["out"] == outs[1][cfg + " dev"]["out"])
    print("RESULT:", "every output bit-equal, every record equal" if not bad else "%d cases differ" % bad)
    sys.exit(1 if bad else 0)
