"""Host-side mirror of `mcalf.routines.hires_fitter.als_fitter` for the likelihood hot path.

Same class name, constructor keywords, method names, argument order and return
conventions as the reference (hires_fitter.py:30-518) for everything the solver branches of
cli.py call on the likelihood path, so the solve step of an existing driver can switch
`from mcalf.routines import hires_fitter` to this module.  Every likelihood / model method is
a batch-of-one call into the HIP library (`libmcalf_hip.so`); `loglike_batch` /
`model_batch` are the vectorised entries.

NOT a complete replacement of the reference module (out of scope; the
list a maintainer needs is in INTEGRATION.md section 2): no solver dispatch, no plotting, no
chain readers -- the module-level `pc_analyzer` and `get_parnames` (hires_fitter.py:704-760),
which cli.py:345-348 calls after a PolyChord run, stay in `mcalf`.  The prior log-density is here: `lnprior`, the
`__call__` built on it and the `Gpriors` keyword (hires_fitter.py:218-234,509-518), evaluated on the device.  linetools is
replaced by an explicit `linepars=` argument plus a tiny built-in table (`LINE_TABLE`).

What needs no fitter lives in `config` and is imported back under its name here; the prior and sampler entries are the mixin of
`sampling`; the closure of `get_jax_likelihood` is built in `jax_bridge`.
"""
from __future__ import annotations

import collections
import ctypes as C
import gc

import numpy as np

from .. import _lib
from . import jax_bridge, sampling
from .config import (LINE_OVERRIDES, LINE_TABLE, _BOOL, _CONFIG_TABLE, _floats, _read_ascii_table,  # noqa: F401
                     apply_line_overrides, parse_gpriors, readconfig, sigma_clipped_median, write_equal_weights)

# what als_fitter.model_band_batch returns: per-pixel mean, variance, quantiles [len(q), npix] and the count of non-NaN rows
ModelBand = collections.namedtuple("ModelBand", "mean var quantiles nvalid")


class als_fitter(sampling.SamplingMixin):
    """Drop-in for `mcalf.routines.hires_fitter.als_fitter` (hires_fitter.py:30).

    Extra keywords (all optional): `spectrum=(wl, flux, err)` arrays instead of a file;
    `linepars=[(wrest, f, gamma), ...]` instead of a linetools lookup; `velstep=`;
    `conv_mode='numpy'|'jax'`; `device=` HIP ordinal, or a LIST of ordinals for one context that drives
    several GPUs of this process (`mcalf_create_multi`: the batched entries cut their rows into contiguous
    blocks, one per device, results bit-identical to one device; entries may repeat);
    `gauss_cdf=[n3, n4, n5]` to pin the asymmetric-veto thresholds the reference draws at random.
    """

    def __init__(self, specfile, fitrange, fitlines, ncomp, nfill=0, specres=[7.0], contval=[1.0],
                 Nrange=[11.5, 16], brange=[1, 30], zrange=None, Nrangefill=[11.5, 16], brangefill=[1, 30],
                 wrangefill=None, coldef=['Wave', 'Flux', 'Err'], Gpriors=None, Asymmlike=False, debug=False,
                 *, spectrum=None, linepars=None, velstep=None, conv_mode="numpy", device=-1, gauss_cdf=None,
                 database_linepars=False):
        # device-side state, set before anything can raise (close() reads it): context, ncomp flavour of the box sent, Gpriors sent, jax twin
        self._ctx, self._prior_key, self._gauss_sent, self._twin = None, None, False, None
        # public attributes under the names the reference's callers read (hires_fitter.py:46-60)
        self.specfile, self.fitrange, self.fitlines = specfile, fitrange, fitlines
        self.Gpriors, self.Asymmlike, self.debug = Gpriors, bool(Asymmlike), debug
        self.specres = list(np.atleast_1d(specres))
        self.contval = list(np.atleast_1d(contval))
        self.ncompmin, self.ncompmax = ncomp
        self.nfill = nfill
        if self.Asymmlike:
            print("Running asymmetric likelihood")
        self.freecont = len(self.contval) > 1          # hires_fitter.py:54-57
        self.freespecres = len(self.specres) > 1       # :59-62
        self.clight = 2.9979245e5                      # :65
        self.ccgs = 2.9979245e10                       # :66

        if spectrum is not None:
            obj_wl, obj, obj_noise = (np.asarray(a, dtype=float) for a in spectrum)
        else:
            obj_wl, obj, obj_noise = _read_ascii_table(specfile, coldef)
        okrange = np.zeros_like(obj_wl, dtype=bool)    # :75-78
        self.numfitranges = len(self.fitrange)
        for lo, hi in self.fitrange:
            okrange[(obj_wl > lo) & (obj_wl < hi)] = True
        self.obj = np.ascontiguousarray(obj[okrange])
        self.obj_noise = np.ascontiguousarray(obj_noise[okrange])
        self.obj_wl = np.ascontiguousarray(obj_wl[okrange])

        if velstep is None:                            # :84-87
            velsteps = (self.obj_wl[1:] - self.obj_wl[:-1]) / self.obj_wl[1:] * self.clight
            velstep = sigma_clipped_median(velsteps)
        self.velstep = float(velstep)

        self.numlines = len(fitlines)                  # :93-116
        if linepars is None:
            try:
                linepars = [LINE_TABLE[name] for name in fitlines]
            except KeyError as exc:
                raise KeyError(f"line {exc} is not in the built-in table; pass linepars=[(wrest,f,gamma),...]")
        if len(linepars) != self.numlines:
            raise ValueError(f"{self.numlines} fit lines but {len(linepars)} (wrest, f, gamma) triples")
        if database_linepars:                          # :100-110: the caller's triples are raw database values
            linepars = apply_line_overrides(fitlines, linepars)
        self.linepars = [dict(wrest=float(w), f=float(f), gamma=float(g)) for (w, f, g) in linepars]
        self.linefill = dict(self.linepars[0])         # :120-121
        self.linefill["wrest"] = 250.0

        # prior box, in the reference's order [R?][cont?][ncomp][N,z,b]*ncompmax [N,z,b]*nfill
        # (hires_fitter.py:124-200)
        self.cont_lims, self.res_lims = np.array(self.contval), np.array(self.specres)
        self.N_lims, self.b_lims = np.array(Nrange), np.array(brange)
        self.N_lims_fill, self.b_lims_fill = np.array(Nrangefill), np.array(brangefill)
        w0 = self.linepars[0]["wrest"]
        wf = self.linefill["wrest"]
        self.z_lims = [self._zbox(zrange, k, self.ncompmax, w0, as_wave=False,
                                  default=(self.fitrange[0][0] + 0.25, self.fitrange[0][1] - 0.25),
                                  what="Zrange") for k in range(self.ncompmax)]
        self.z_lims_fill = [self._zbox(wrangefill, k, self.nfill, wf, as_wave=True,
                                       default=(np.min(self.obj_wl) + 0.25, np.max(self.obj_wl) - 0.25),
                                       what="Wrangefill") for k in range(self.nfill)]
        self.startind = int(self.freecont) + int(self.freespecres)     # :169-174
        self.endind = self.startind + 3 * self.ncompmax + 1            # :176
        head = ([self.res_lims] if self.freespecres else []) + ([self.cont_lims] if self.freecont else [])
        comps = [lim for k in range(self.ncompmax) for lim in (self.N_lims, self.z_lims[k], self.b_lims)]
        fills = [lim for k in range(self.nfill) for lim in (self.N_lims_fill, self.z_lims_fill[k], self.b_lims_fill)]
        self.bounds = head + [ncomp] + comps + fills
        self.ndim = len(self.bounds)
        self._lo = np.array([np.min(b) for b in self.bounds], dtype=float)
        self._hi = np.array([np.max(b) for b in self.bounds], dtype=float)
        self._gauss = parse_gpriors(Gpriors, self.ndim)     # (mu, sigma) for the device, sent with the first _ensure_prior

        # Asymmetric-veto thresholds (hires_fitter.py:179-181): counts of a standard-normal draw
        # above 3, 4, 5 sigma.  The reference's draw is unseeded; pass gauss_cdf=[n3, n4, n5] to pin it.
        if gauss_cdf is None:
            gauss = np.random.normal(size=len(self.obj))
            gauss_cdf = [(gauss > 3).sum(), (gauss > 4).sum(), (gauss > 5).sum()]
        self.gauss_cdf = [int(v) for v in gauss_cdf]
        self.gracenum = 0.01 * len(self.obj)

        self.conv_mode = conv_mode
        self._open_context(device)

    @staticmethod
    def _zbox(spec, k, count, wrest, as_wave, default, what):
        """Redshift box of slot k.  `spec` None -> from the wavelength window `default`
        (hires_fitter.py:138-139,155-156); 2 numbers -> shared box; 2*count numbers -> per slot.
        `as_wave`: numbers are observed wavelengths (fillers, :158-162) rather than redshifts."""
        if spec is None:
            lo, hi, as_wave = default[0], default[1], True
        elif len(spec) == 2:
            lo, hi = spec[0], spec[1]
        elif (as_wave and len(spec) == 2 * count) or (not as_wave and len(spec) >= 2 * count):
            lo, hi = spec[2 * k], spec[2 * k + 1]
        else:
            raise ValueError(f"{what} keyword not understood.")
        if as_wave:
            lo, hi = lo / wrest - 1., hi / wrest - 1.
        return np.array((lo, hi))

    # ------------------------------------------------------------------ device context
    def _open_context(self, device):
        lib = _lib.load()
        sp = _lib.mcalf_spec()
        sp.npix = self.obj_wl.size
        self._keep = (np.ascontiguousarray(self.obj_wl), np.ascontiguousarray(self.obj),
                      np.ascontiguousarray(self.obj_noise))
        # (struct fields are typed pointers, which take no plain address: the one cast of the class)
        sp.wl, sp.flux, sp.err = (C.cast(a.__array_interface__["data"][0], C.POINTER(C.c_double)) for a in self._keep)
        sp.velstep = self.velstep
        sp.nlines = self.numlines
        lines = (_lib.mcalf_line * self.numlines)()
        for i, lp in enumerate(self.linepars):
            lines[i] = _lib.mcalf_line(lp["wrest"], lp["f"], lp["gamma"])
        sp.lines = lines
        sp.fill = _lib.mcalf_line(self.linefill["wrest"], self.linefill["f"], self.linefill["gamma"])
        sp.ncompmax, sp.nfill = int(self.ncompmax), int(self.nfill)
        sp.freespecres, sp.freecont = int(self.freespecres), int(self.freecont)
        jax = (self.conv_mode == "jax")
        # numpy path: float(max(specres)) (:415-417); JAX path: specres[0] (:572)
        sp.specres_fixed = float(self.specres[0]) if jax else float(max(self.specres))
        # LSF reach: numpy path max(specres); the JAX path sizes its fixed kernel grid from res_lims[1] when the
        # resolution is free (hires_fitter.py:549-550: the SECOND entry, not the maximum) and from max otherwise
        sp.specres_max = float(self.specres[1]) if (jax and self.freespecres) else float(max(self.specres))
        sp.contval_fixed = float(self.contval[0])
        sp.conv_mode = _lib.MCALF_CONV_SAME_EDGE_JAX if jax else _lib.MCALF_CONV_WRAP_NUMPY
        devices = None if np.ndim(device) == 0 else [int(d) for d in device]
        sp.device = int(device) if devices is None else devices[0]
        sp.asymmlike = int(bool(self.Asymmlike))
        sp.asymm_n4, sp.asymm_n5 = float(self.gauss_cdf[1]), float(self.gauss_cdf[2])
        ctx = C.c_void_p()
        if devices is None:
            _lib.check(lib.mcalf_create(C.byref(sp), C.byref(ctx)))
        else:
            _lib.check(lib.mcalf_create_multi(C.byref(sp), (C.c_int32 * len(devices))(*devices), len(devices), C.byref(ctx)))
        self._ctx, self._lib = ctx, lib
        info = _lib.mcalf_info_t()
        self._call(lib.mcalf_info, C.byref(info))
        assert info.ndim == self.ndim and info.startind == self.startind and info.endind == self.endind
        self.info = info
        # host-side call overhead matters for the one-theta-at-a-time solvers (a call is ~40 us on the GPU side):
        # one persistent parameter row / result slot with their addresses taken once, and a small cache of the
        # addresses of the caller's arrays (a sampler hands over the same buffers call after call)
        self._p1 = np.empty((1, self.ndim))
        self._o1 = np.empty(1)
        self._p1_ptr, self._o1_ptr = self._p1.ctypes.data, self._o1.ctypes.data

    def _ptr(self, arr):
        """Address of a C-contiguous array's data.  Only the context's OWN persistent one-theta buffers have their address
        cached (`ndarray.ctypes` costs a microsecond of a 15 us call): a caller's array may be reallocated in place
        (`ndarray.resize(refcheck=False)`) without changing its identity, so its address is read on every call."""
        if arr is self._p1:
            return self._p1_ptr
        if arr is self._o1:
            return self._o1_ptr
        return arr.__array_interface__["data"][0]

    def _optr(self, arr):
        """`_ptr` of an optional array: None stays None, the null pointer an entry takes for an output it is to leave out."""
        return None if arr is None else self._ptr(arr)

    def _call(self, fn, *args):
        """The one way into the library: `fn(ctx, *args)`, a nonzero return code raised with the context's message; arrays go in as
        `_ptr` / `_optr` addresses.  Only `loglike_batch` and `lnlhood_worker` spell it out in place (millions of 15 us calls)."""
        rc = fn(self._ctx, *args)
        if rc:
            _lib.check(rc, self._ctx)

    def _out(self, out, shape, name="out", what=None):
        """The array an entry writes a result of `shape` into: a new one, or the caller's `out` once it is seen to be float64,
        C-contiguous and of that size (returned as given, not reshaped), else ValueError `name` must be ... `what`."""
        if out is None:
            return np.empty(shape)
        if out.dtype != np.float64 or not out.flags.c_contiguous or out.size != int(np.prod(shape)):
            raise ValueError(f"{name} must be a C-contiguous float64 array {what or f'of shape {list(shape)}'}")
        return out

    def close(self):
        if self._twin is not None:
            self._twin.close()
            self._twin = None
        if self._ctx is not None:
            self._lib.mcalf_destroy(self._ctx)
            self._ctx = None

    def set_chunks(self, nchunks):
        """Row blocks a batch is issued in inside the library (0 = automatic, 1 = one launch per batch); results
        do not depend on it."""
        self._call(self._lib.mcalf_set_chunks, int(nchunks))

    def chunks_for(self, batch):
        return int(self._lib.mcalf_get_chunks(self._ctx, int(batch)))

    def set_resident(self, idle_us):
        """Resident one-theta evaluator (mcalf_set_resident): with `idle_us` > 0 the one-theta callables are answered by a
        workgroup that stays on the GPU between calls -- no kernel launch per call -- and leaves by itself after `idle_us`
        microseconds without one; 0 turns it off.  Same bits as the launched form."""
        self._call(self._lib.mcalf_set_resident, int(idle_us))

    def set_cu_mask(self, mask_words):
        """Restrict the context's own streams to the compute units of `mask_words` (uint32 words, bit i of word i // 32 =
        CU i; empty / None removes the mask) -- `mcalf_set_cu_mask`.  Results never depend on it; on anything but the
        eight XCDs of an unpartitioned MI355X large host batches take the row-block pipeline (`last_launch()`)."""
        words = np.ascontiguousarray([] if mask_words is None else mask_words, dtype=np.uint32)
        self._call(self._lib.mcalf_set_cu_mask, self._ptr(words) if words.size else None, int(words.size))

    def last_launch(self, sub=None):
        """What the last call of this context did (`mcalf_last_launch`): entry plan, row blocks, whether the fused
        kernel ran as the persistent grid, its grid and work-item count, the device entries it was cut over.
        `sub=k`: device entry k of a multi-device context (`mcalf_last_launch_sub`)."""
        info = _lib.mcalf_launch_info_t()
        if sub is None:
            self._call(self._lib.mcalf_last_launch, C.byref(info))
        else:
            self._call(self._lib.mcalf_last_launch_sub, int(sub), C.byref(info))
        return info

    def get_config(self):
        """The knobs the context runs under and the MCALF_* variables its environment had set (`mcalf_get_config`)."""
        buf = C.create_string_buffer(2048)
        self._call(self._lib.mcalf_get_config, buf, len(buf))
        return buf.value.decode()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, type, value, trace):
        self.close()
        gc.collect()

    # ------------------------------------------------------------------ prior transforms
    def _scale_cube_pc(self, cube):
        """Prior transform for PolyChord / dyPolyChord (hires_fitter.py:202-209): a new vector
        `cube * ptp(bounds) + min(bounds)` (separately rounded multiply and add, as numpy evaluates it),
        with the ncomp slot truncated like Python's int()."""
        theta = np.array(cube, dtype=float, copy=True)
        theta *= self._hi - self._lo
        theta += self._lo
        theta[self.startind] = int(theta[self.startind])
        return theta

    def _scale_cube_mn(self, cube, ndim, nparam):
        """Prior transform for MultiNest (hires_fitter.py:211-216): rescales the first `ndim` entries of
        `cube` -- possibly a C double pointer -- in place; the ncomp slot keeps its fraction."""
        for k in range(ndim):
            cube[k] = cube[k] * (self._hi[k] - self._lo[k]) + self._lo[k]
        return cube

    def scale_cube_batch(self, cubes, int_ncomp=True):
        """Vectorised prior transform on the device (rows of `cubes` in [0,1]^ndim)."""
        cubes = np.ascontiguousarray(cubes, dtype=float).reshape(-1, self.ndim)
        out = np.empty_like(cubes)
        self._call(self._lib.mcalf_scale_cube_batch, self._ptr(self._lo), self._ptr(self._hi), self._ptr(cubes), cubes.shape[0],
                   int(bool(int_ncomp)), self._ptr(out))
        return out

    def loglike_cube_batch(self, cubes, int_ncomp=True, return_theta=True):
        """Unit cube in -> (theta, logL) out: lnlhood_pc(_scale_cube_pc(cube)) for every row
        (hires_fitter.py:202-209, 250-262) in one device pass; the prior transform runs inside the
        per-sample set-up kernel.  `int_ncomp=False` gives the MultiNest flavour (:211-216)."""
        cubes = self._rows(cubes, self.ndim)
        self._ensure_prior(int_ncomp)
        logL = np.empty(cubes.shape[0])
        theta = np.empty_like(cubes) if return_theta else None
        self._call(self._lib.mcalf_loglike_cube_batch, self._ptr(cubes), cubes.shape[0], self._optr(theta), self._ptr(logL))
        return (theta, logL) if return_theta else logL

    # ------------------------------------------------------------------ batched entries
    def _rows(self, P, width):
        P = np.ascontiguousarray(P, dtype=float)
        if P.ndim == 1:
            P = P.reshape(1, -1)
        if P.shape[1] != width:
            raise ValueError(f"parameter rows must have {width} entries, got {P.shape[1]}")
        return P

    def loglike_batch(self, P, out=None):
        """logL[i] = lnlhood_worker(P[i]) for every row.  `out` (float64, C-contiguous, one entry per
        row) is filled in place when given; with `P` and `out` in page-locked host memory (e.g.
        `torch.empty(..., pin_memory=True).numpy()`) the two PCIe copies of the call are DMA transfers
        instead of staged ones."""
        P = self._rows(P, self.ndim)
        if out is None:
            out = np.empty(P.shape[0])
        elif out.dtype != np.float64 or not out.flags.c_contiguous or out.size != P.shape[0]:
            raise ValueError("out must be a C-contiguous float64 array with one entry per row")
        rc = self._lib.mcalf_loglike_batch(self._ctx, self._ptr(P), P.shape[0], self._ptr(out))
        if rc:
            _lib.check(rc, self._ctx)
        return out

    def loglike_grad_batch(self, P, out=None, grad_out=None):
        """(logL, G) for every row: logL[i] = lnlhood_worker(P[i]) as `loglike_batch` gives it, and
        G[i, k] = d logL[i] / d P[i, k], the analytic gradient under the context's `conv_mode` (HIP kernels).

        The ncomp column and the (N, z, b) of every component at or beyond the row's active count are exactly 0;
        rows whose logL is -inf (asymmetric veto) or NaN get an all-NaN row.  On the numpy path the LSF tap count
        ceil(3.0348 sigma) is held at its value for the row: G is the derivative within that piece, while logL
        itself jumps where the count changes; the R column is 0 when R <= velstep (no convolution).  `out` /
        `grad_out` (float64, C-contiguous, [batch] / [batch, ndim]) are filled in place when given."""
        P = self._rows(P, self.ndim)
        n = P.shape[0]
        out = self._out(out, (n,), what="with one entry per row")
        grad_out = self._out(grad_out, (n, self.ndim), "grad_out", "of shape [batch, ndim]")
        self._call(self._lib.mcalf_loglike_grad_batch, self._ptr(P), n, self._ptr(out), self._ptr(grad_out))
        return out, grad_out.reshape(n, self.ndim)

    def lnlhood_grad(self, p):
        """(logL, gradient) of one parameter vector: `lnlhood_worker(p)` and its analytic gradient
        (`loglike_grad_batch`).  Negated, it is what `scipy.optimize.minimize(..., jac=True)` takes."""
        self._check_scalar(p)
        ll, g = self.loglike_grad_batch(np.asarray(p, dtype=float).reshape(1, -1))
        return float(ll[0]), g[0]

    def _deriv_call(self, fn, P, X, xw, out, yw, what):
        P = self._rows(P, self.ndim)
        n = P.shape[0]
        X = np.ascontiguousarray(X, dtype=float)
        if X.ndim == 1:
            X = X.reshape(1, -1)
        if X.shape != (n, xw):
            raise ValueError(f"{what} must have shape [{n}, {xw}], got {list(X.shape)}")
        out = self._out(out, (n, yw), what=f"of shape [batch, {yw}]")
        self._call(fn, self._ptr(P), self._ptr(X), n, self._ptr(out))
        return out.reshape(n, yw)

    def model_jvp_batch(self, P, V, out=None):
        """dM[i, :] = J(P[i]) V[i, :], the directional derivative of the model `model_batch(P)[i]` along the parameter
        tangent V[i] ([batch, ndim] -> [batch, npix]; HIP kernels, the Jacobian J = d model / d theta is never formed).

        One tangent per row: k tangents at one theta are k rows that repeat it.  The ncomp entry of V and the (N, z, b)
        of components at or beyond the row's active count are ignored, as are the R / continuum entries the context
        fixes; on the numpy path the LSF tap count is held at its value for the row (as in `loglike_grad_batch`).  A
        row whose R needs more taps than the context provisions is all NaN.  `out` is filled in place when given."""
        return self._deriv_call(self._lib.mcalf_model_jvp_batch, P, V, self.ndim, out, self.obj_wl.size, "V")

    def model_vjp_batch(self, P, Q, out=None):
        """G[i, :] = J(P[i])^T Q[i, :]: the per-pixel cotangent Q[i] ([batch, npix]) pulled back to the parameters
        ([batch, ndim]) -- the gradient of any scalar of the model whose pixel derivative is Q.  `loglike_grad_batch` is
        the special case Q = (flux - model) / err^2 on the pixels nansum keeps.

        Q is used as given (non-finite entries propagate).  The ncomp column and the (N, z, b) of inactive components
        are exactly 0; a row whose R needs more taps than the context provisions is all NaN."""
        return self._deriv_call(self._lib.mcalf_model_vjp_batch, P, Q, self.obj_wl.size, out, self.ndim, "Q")

    def fisher_matvec_batch(self, P, V, out=None):
        """(J^T W J) V[i] per row, the Fisher matrix of the Gaussian likelihood at P[i] applied to V[i], matrix-free and on
        the device (`mcalf_fisher_matvec_batch`): one JVP pass, a per-pixel multiply by W and one VJP pass, without the
        [batch, npix] intermediate leaving the device -- bit for bit `model_vjp_batch(P, W * model_jvp_batch(P, V))`.
        W = 1 / err^2 on the pixels whose logL term np.nansum keeps (finite flux, finite non-zero error) and 0 elsewhere."""
        return self._deriv_call(self._lib.mcalf_fisher_matvec_batch, P, V, self.ndim, out, self.ndim, "V")

    def __call__(self, p):
        """hires_fitter.py:509-518: lnprior + lnlhood with the reference's two -inf short cuts (the reference names a method
        `lnlhood` that does not exist; this calls `lnlhood_worker`)."""
        lp = self.lnprior(p)
        if not np.isfinite(lp):
            return -np.inf
        lh = self.lnlhood_worker(p)
        if not np.isfinite(lh):
            return -np.inf
        return lh + lp

    def maximize_batch(self, P0, max_iter=50, cg_iters=None, lambda0=1e-3, ftol=1e-10, rows_per_block=0):
        """(P, logL, status, niter): every row of P0 polished to a maximum of logL inside the prior box by a batched
        Levenberg-Marquardt iteration on the device (`mcalf_maximize_batch`; HIP kernels, nothing dense is formed: the
        damped normal equations are solved by `cg_iters` conjugate-gradient iterations, one Fisher product each;
        None = ndim).

        The ncomp slot and the (N, z, b) of slots at or beyond a row's active count are returned bit for bit; the other
        entries of a start are clamped into the box first.  logL[i] is `loglike_batch(P)[i]` bit for bit and never
        below the clamped start's.  status: 1 converged (the last accepted gain is <= ftol (1 + |logL|)), 0 `max_iter`
        reached, 2 zero projected gradient, 3 damping beyond 1e12, -1 the start's logL is not finite (the row comes
        back as given).  niter: outer iterations the row took a step in.  `rows_per_block` bounds the rows fitted together
        (0: the library's rule); a row's result does not depend on it.  A Gaussian prior (`set_gauss_prior`) does not enter:
        the fit maximises logL alone."""
        P0 = self._rows(P0, self.ndim)
        n = P0.shape[0]
        self._ensure_prior()
        opts = _lib.mcalf_fit_opts(int(max_iter), 0 if cg_iters is None else int(cg_iters), int(rows_per_block), 0,
                                   float(lambda0), float(ftol))
        if cg_iters is not None and int(cg_iters) <= 0:
            raise ValueError("cg_iters must be positive (None: ndim)")
        P, logL = np.empty_like(P0), np.empty(n)
        status, niter = (np.empty(n, dtype=np.int32) for _ in range(2))
        self._call(self._lib.mcalf_maximize_batch, self._ptr(P0), n, C.addressof(opts), self._ptr(P), self._ptr(logL), self._ptr(status),
                   self._ptr(niter))
        return P, logL, status, niter

    def maximize(self, p0, **kw):
        """`maximize_batch` for one parameter vector: (p, logL, status, niter)."""
        self._check_scalar(p0)
        P, logL, status, niter = self.maximize_batch(np.asarray(p0, dtype=float).reshape(1, -1), **kw)
        return P[0], float(logL[0]), int(status[0]), int(niter[0])

    def loglike_hvp_batch(self, P, V, out=None):
        """HV[i, :] = H(P[i]) V[i, :] with H = d2 logL / dtheta2, the exact Hessian of `lnlhood_worker` under the context's
        `conv_mode` applied to one tangent per row ([batch, ndim] -> [batch, ndim]; HIP kernels, H is never formed).  It is
        the directional derivative of `loglike_grad_batch`'s gradient along V[i]: the Fisher term -J^T W J v of
        `fisher_matvec_batch` plus the curvature term sum_i W_i (d_i - m_i) (d2 m_i / dtheta2) v.

        The conventions are `loglike_grad_batch`'s: the ncomp entry, the (N, z, b) of components at or beyond the row's
        active count, the R / continuum entries the context fixes and R where R <= velstep (numpy path) are ignored in V
        and exactly 0 in HV; the tap count of the numpy path is held at its value for the row; rows whose logL is -inf or
        NaN, or whose R needs more taps than the context provisions, are all NaN.  `out` is filled in place when given."""
        return self._deriv_call(self._lib.mcalf_loglike_hvp_batch, P, V, self.ndim, out, self.ndim, "V")

    def lnlhood_hessp(self, p, v):
        """H(p) v for one parameter vector and one tangent (`loglike_hvp_batch`).  Negated, it is the `hessp` of
        `scipy.optimize.minimize(..., method="trust-ncg")` for the objective -lnlhood."""
        self._check_scalar(p)
        return self.loglike_hvp_batch(np.asarray(p, dtype=float).reshape(1, -1), np.asarray(v, dtype=float).reshape(1, -1))[0]

    def lnlhood_hessian(self, p):
        """The dense Hessian H[ndim, ndim] of logL at one parameter vector: one `loglike_hvp_batch` call of ndim rows that
        repeat `p`, with the identity's rows as tangents.  A convenience: it costs ndim passes over the spectrum; for
        products with a vector use `loglike_hvp_batch`, which never forms H.  Row k is H e_k; H is symmetric to rounding."""
        self._check_scalar(p)
        P = np.tile(np.asarray(p, dtype=float).reshape(1, -1), (self.ndim, 1))
        return self.loglike_hvp_batch(P, np.eye(self.ndim))

    def model_jacobian(self, p):
        """J[npix, ndim] = d model / d theta at one parameter vector: one `model_jvp_batch` call of ndim rows that
        repeat `p`, with the identity's rows as tangents.  It costs ndim Voigt passes over the spectrum; for products
        with a vector use `model_jvp_batch` / `model_vjp_batch`, which never form J."""
        self._check_scalar(p)
        P = np.tile(np.asarray(p, dtype=float).reshape(1, -1), (self.ndim, 1))
        return np.ascontiguousarray(self.model_jvp_batch(P, np.eye(self.ndim)).T)

    def chi2_batch(self, P):
        P = self._rows(P, self.ndim)
        out = np.empty(P.shape[0])
        self._call(self._lib.mcalf_chi2_batch, self._ptr(P), P.shape[0], self._ptr(out))
        return out

    def model_batch(self, P, targonly=False):
        """model[i, :] = reconstruct_spec(P[i], targonly)."""
        P = self._rows(P, self.ndim)
        out = np.empty((P.shape[0], self.obj_wl.size))
        self._call(self._lib.mcalf_model_batch, self._ptr(P), P.shape[0], int(bool(targonly)), self._ptr(out))
        return out

    def onecomp_batch(self, Q, fill=False, line=None):
        """Rows (R, cont, N, z, b) -> single-component spectra.  `fill`: the filler line;
        `line=k`: line k of the multiplet alone; default: every line of the component."""
        Q = self._rows(Q, 5)
        # The LDS halo of the context is provisioned from max(specres); the reference would simply build a longer
        # kernel (hires_fitter.py:458-459), so a wider request is an error here rather than a NaN spectrum.
        R = Q[:, 0]
        with np.errstate(invalid="ignore"):
            half = np.where(R > self.velstep, np.ceil(3.0348 * (R / 2.354820) / self.velstep), 0.0)
        if self.conv_mode != "jax" and np.any(half > self.info.n_cap):
            raise ValueError(f"specresolution {float(np.nanmax(R)):g} km/s needs an LSF kernel wider than the context was "
                             f"provisioned for (max(specres) = {max(self.specres):g} km/s); construct als_fitter with a "
                             "larger specres")
        out = np.empty((Q.shape[0], self.obj_wl.size))
        which = 1 if fill else (0 if line is None else 2 + int(line))
        self._call(self._lib.mcalf_onecomp_batch, self._ptr(Q), Q.shape[0], which, self._ptr(out))
        return out

    # ------------------------------------------------------------------ batched analysis pass
    def eqw_batch(self, P, reference_indexing=False, out=None, comp=True, blend=True):
        """Equivalent widths of every row on the device (HIP kernels; no spectrum is written to memory):
        `(Wcomp[batch, ncompmax, nlines], Wblend[batch, nlines])`, in Angstrom.

        `Wcomp[i, c, l]` is the rest-frame width of line `l` of the component in slot `c` alone -- the term `calc_w` sums
        (hires_fitter.py:488-489).  `Wblend[i, l]` is the observed-frame width of line `l` of all the row's slots TOGETHER,
        sum_pix (1 - exp(-sum_c tau_cl)) dlambda: where components overlap it is smaller than sum_c (1 + z_c) Wcomp[i, c, l].
        Nothing is convolved (the LSF does not change W) and the continuum does not enter.

        `reference_indexing=False`: slot `c` reads (N, z, b) at `startind + 1 + 3c` for `c` below the row's active count
        (clamped to [0, ncompmax] as the likelihood does); the other cells are exactly 0 and a NaN there does not leak.
        `reference_indexing=True`: all `ncompmax` slots, read from `startind + 3c` -- the reference as written (:481-482).
        `comp=False` / `blend=False` leave that output out (None is returned in its place); `out=(Wcomp, Wblend)` (float64,
        C-contiguous; an entry may be None) is filled in place.  A row's bits depend on nothing but the row."""
        P = self._rows(P, self.ndim)
        n = P.shape[0]
        shapes = ((n, int(self.ncompmax), self.numlines), (n, self.numlines))
        res = [self._out(None if out is None else out[k], shape, f"out[{k}]") if want else None
               for k, (want, shape) in enumerate(zip((comp, blend), shapes))]
        if res[0] is None and res[1] is None:
            raise ValueError("eqw_batch: at least one of comp / blend must be requested")
        self._call(self._lib.mcalf_eqw_batch, self._ptr(P), n, _lib.MCALF_EQW_AS_WRITTEN if reference_indexing else _lib.MCALF_EQW_LAYOUT,
                   self._optr(res[0]), self._optr(res[1]))
        return tuple(a if a is None or a.shape == shape else a.reshape(shape) for a, shape in zip(res, shapes))

    def calc_w_batch(self, P, lineid=0, reference_indexing=True):
        """`calc_w(P[i], lineid, reference_indexing)` for every row of a chain in one call: `eqw_batch`'s per-component
        widths of line `lineid` summed over the slots in slot order ([batch], Angstrom).  Rows whose continuum is zero or
        not finite are NaN, as the reference's `absorption / cont` (:488) makes them -- unless no slot is in use, where
        `calc_w` returns 0 before it divides."""
        P = self._rows(P, self.ndim)
        lineid = int(lineid)
        if not 0 <= lineid < self.numlines:
            raise ValueError(f"lineid must be in [0, {self.numlines}), got {lineid}")
        wcomp, _ = self.eqw_batch(P, reference_indexing=reference_indexing, blend=False)
        w = np.zeros(P.shape[0])
        for c in range(int(self.ncompmax)):
            w += wcomp[:, c, lineid]
        if reference_indexing:
            used = np.full(P.shape[0], int(self.ncompmax) > 0)
        else:
            with np.errstate(invalid="ignore"):
                used = (np.trunc(P[:, self.startind]) >= 1.0) & (int(self.ncompmax) > 0)
        if self.freecont:
            cont = P[:, 1 if self.freespecres else 0]
        else:
            cont = np.full(P.shape[0], _scalar(self.contval), dtype=float)
        w[used & ~(np.isfinite(cont) & (cont != 0))] = np.nan
        return w

    def model_band_batch(self, P, q=(0.16, 0.5, 0.84), targonly=False):
        """Where the chain `P` puts the model spectrum, per pixel, computed on the device (HIP kernels; no spectrum reaches
        the host): `ModelBand(mean[npix], var[npix], quantiles[len(q), npix], nvalid[npix])` over the rows of
        `model_batch(P, targonly)` that are not NaN at that pixel -- `np.nanmean`, `np.nanvar` (ddof 0, two passes) and
        `np.nanquantile(..., method="linear")`, the quantiles exact selections among the stored values.  `nvalid` (int64)
        counts those rows; a pixel without any is NaN in the other three.  `q=()` leaves the quantiles out (shape [0, npix]).
        The [batch, npix] matrix lives on the device for the length of the call only; beyond 4 GiB the call is refused (thin
        the chain).  The result does not depend on the device count of the context, and two calls give the same bits."""
        P = self._rows(P, self.ndim)
        qs = np.ascontiguousarray(np.atleast_1d(np.asarray(q, dtype=float)).reshape(-1))
        npix = self.obj_wl.size
        mean, var = np.empty(npix), np.empty(npix)
        quant = np.empty((qs.size, npix))
        nvalid = np.empty(npix, dtype=np.int64)
        self._call(self._lib.mcalf_model_band_batch, self._ptr(P), P.shape[0], int(bool(targonly)), self._ptr(qs) if qs.size else None, qs.size,
                   self._ptr(mean), self._ptr(var), self._ptr(quant) if qs.size else None, self._ptr(nvalid))
        return ModelBand(mean, var, quant, nvalid)

    def calc_N_batch(self, P):
        """`calc_N(P[i], reference_indexing=False)` for every row ([batch]; host numpy, no kernel): log10 of the summed
        columns of the slots with z < 10.  Rows that keep the same slots are summed together, each over exactly the entries
        `calc_N` sums and in its order, so the values agree bit for bit."""
        P = self._rows(P, self.ndim)
        allN = P[:, self.startind + 1::3]
        allz = P[:, self.startind + 2::3]
        k = min(allN.shape[1], allz.shape[1])
        allN, keep = allN[:, :k], allz[:, :k] < 10
        out = np.empty(P.shape[0])
        masks, which = np.unique(keep, axis=0, return_inverse=True)
        which = np.asarray(which).reshape(-1)
        with np.errstate(divide="ignore"):
            for m, mask in enumerate(masks):
                rows = np.flatnonzero(which == m)
                out[rows] = np.log10(np.sum(10 ** np.ascontiguousarray(allN[rows][:, mask]), axis=1))
        return out

    # ------------------------------------------------------------------ reference callables
    def _check_scalar(self, p):
        """The single-point callables of the reference raise where Python's `int()` does: a NaN or
        infinite ncomp slot (`int(p[startind])`, :428) is a ValueError / OverflowError, not a value.
        (The batched entries clamp the slot to [0, ncompmax] instead and never raise.)"""
        int(p[self.startind])

    def chi2(self, p):
        """hires_fitter.py:236-248 (returns `(+inf, [])` for an all-zero model, else a float)."""
        self._check_scalar(p)
        v = float(self.chi2_batch(p)[0])
        if v == np.inf:
            return +np.inf, []
        return v

    def lnlhood_pc(self, p):
        """hires_fitter.py:250-262 -> (logL, [])."""
        return self.lnlhood_worker(p), []

    def lnlhood_dy(self, p):
        """hires_fitter.py:264-272 -> float."""
        return self.lnlhood_worker(p)

    def lnlhood_mn(self, p, ndim, nparam):
        """hires_fitter.py:274-285: `p` may be a C double pointer, hence the copy."""
        parr = np.array([p[x] for x in range(self.ndim)])
        return self.lnlhood_worker(parr)

    def lnlhood_worker(self, p):
        """hires_fitter.py:287-328."""
        self._check_scalar(p)
        p = np.asarray(p, dtype=float)
        if p.shape != (self.ndim,):
            return float(self.loglike_batch(p)[0])          # (raises for a wrong length, as the batched entry does)
        self._p1[0, :] = p
        rc = self._lib.mcalf_loglike_batch(self._ctx, self._p1_ptr, 1, self._o1_ptr)
        if rc:
            _lib.check(rc, self._ctx)
        return float(self._o1[0])

    def reconstruct_spec(self, p, targonly=False):
        """hires_fitter.py:409-449."""
        self._check_scalar(p)
        return self.model_batch(p, targonly)[0]

    def reconstruct_onecomp(self, specresolution, continuum, N, z, b):
        """hires_fitter.py:379-392."""
        return self.onecomp_batch([specresolution, _scalar(continuum), N, z, b], fill=False)[0]

    def reconstruct_onecomp_fill(self, specresolution, continuum, N, z, b):
        """hires_fitter.py:394-406."""
        return self.onecomp_batch([specresolution, _scalar(continuum), N, z, b], fill=True)[0]

    def calc_w(self, p, lineid=0, reference_indexing=True):
        """Rest-frame equivalent width of line `lineid` (hires_fitter.py:467-491).

        `reference_indexing=True` (default) reproduces the reference AS WRITTEN: it loops over all `ncompmax`
        slots and slices `p[3*comp+startind : 3*comp+3+startind]` (:482), i.e. it starts at the ncomp slot
        instead of one past it, so the triples it integrates are (ncomp, N1, z1), (b1, N2, z2), ... read as
        (N, z, b).  `reference_indexing=False` follows the parameter layout of reconstruct_spec (:431) over the
        ACTIVE components -- what the routine evidently intends.  No solver calls either."""
        p = np.asarray(p, dtype=float)
        cont = (p[1] if self.freespecres else p[0]) if self.freecont else _scalar(self.contval)
        if reference_indexing:
            nc, first = int(self.ncompmax), self.startind
        else:
            nc, first = min(max(int(p[self.startind]), 0), self.ncompmax), self.startind + 1
        if nc == 0:
            return 0 if reference_indexing else 0.0
        comps = p[first: first + 3 * nc].reshape(nc, 3)                                    # read as (N, z, b)
        Q = np.column_stack([np.zeros(nc), np.full(nc, cont), comps])                      # R = 0: unconvolved (:483)
        absorption = self.onecomp_batch(Q, line=lineid)
        dlambda = np.diff(self.obj_wl)
        dlambda = np.insert(dlambda, 0, dlambda[0])
        w = np.sum((1 - (absorption / cont)) * dlambda, axis=1)                            # :488
        return float(np.sum(w / (1 + comps[:, 1])))                                        # :489

    def calc_N(self, p, reference_indexing=True):
        """Total column density log10(sum 10**N) of the slots with z < 10 (hires_fitter.py:493-505).

        `reference_indexing=True` (default) evaluates the reference's own expressions: `p[startind::3]` as N and
        `p[startind+1::3]` as z (:499-500) -- strides that start at the ncomp slot, so "N" is (ncomp, b1, b2, ...)
        and "z" is (N1, N2, ...); the two differ in length by one for every valid layout and numpy raises the same
        IndexError the reference raises.  `reference_indexing=False` strides from the first N slot, as the layout
        (:431) implies; the z cut then drops the fillers, which sit at z ~ 24."""
        p = np.asarray(p, dtype=float)
        if reference_indexing:
            allN = p[self.startind::3]
            allz = p[self.startind + 1::3]
            okN = (allz < 10)
            try:
                allN = 10 ** allN[okN]
            except IndexError as exc:
                raise IndexError(f"{exc} -- calc_N(reference_indexing=True) evaluates the reference's expressions as "
                                 "written (hires_fitter.py:499-503), which fail like this for every valid parameter "
                                 "vector; pass reference_indexing=False for the total column density") from exc
            return np.log10(np.sum(allN))
        allN = p[self.startind + 1::3]
        allz = p[self.startind + 2::3]
        n = min(allN.size, allz.size)
        allN, allz = allN[:n], allz[:n]
        return np.log10(np.sum(10 ** allN[allz < 10]))

    @classmethod
    def from_config(cls, run_params, **extra):
        """Construct from the dict `readconfig` returns, exactly as cli.py:73-76 does."""
        return cls(run_params['specfile'], run_params['wavefit'], run_params['linelist'], run_params['ncomp'],
                   nfill=run_params['nfill'], specres=run_params['specres'], contval=run_params['contval'],
                   Nrange=run_params['Nrange'], brange=run_params['brange'], zrange=run_params['zrange'],
                   Nrangefill=run_params['Nrangefill'], brangefill=run_params['brangefill'],
                   wrangefill=run_params['wrangefill'], coldef=run_params['coldef'],
                   Asymmlike=run_params['asymmlike'], **extra)

    def get_jax_likelihood(self, use_jax=None):
        """Counterpart of the closure hires_fitter.py:521-695 returns (`log_likelihood` of cli.py:237,256):
        `log_likelihood(p) -> float32 scalar` with the JAX path's semantics -- theta in float32, floor() on the
        ncomp slot (:616), one exp of the summed optical depth (:663), LSF kernel on the fixed grid of the
        largest resolution (:549-560), zero-padded 'same' convolution that is always applied (:674), first / last
        half_size pixels reset to the unconvolved model (:677-681) -- evaluated by the HIP kernel
        (`conv_mode='jax'` context) in float64 and rounded to float32 on return.  float32 arithmetic itself is
        not reproduced: the reference's own float32 path loses 0.6 in logL to cancellation.

        The closure is batch-capable: `p` of shape [..., ndim] gives float32 [...].  With JAX installed (and
        `use_jax` not False) it is wrapped in `jax.pure_callback`, so it can be traced, jitted and vmapped by
        jaxns exactly like the reference's closure; without JAX it is the plain host function.  `use_jax=True`
        raises ImportError when JAX is absent, as the reference does (:523-524).

        Under JAX the closure is a `jax.custom_vjp`: its backward pass is a `pure_callback` into the twin's analytic
        gradient (`loglike_grad_batch`, float32 in and out), so `jax.grad` works on it as on the reference's plain-JAX
        closure.  The host half of that pass is `.host_grad(p) -> (logL, G)` (float32, G of shape p.shape), on both
        the JAX-wrapped and the plain closure."""
        twin = self if self.conv_mode == "jax" else self._jax_twin()
        return jax_bridge.jax_likelihood(twin, self.ndim, use_jax)

    def _jax_twin(self):
        """A second context over the same arrays with the JAX path's boundary semantics (kept for the
        lifetime of this object)."""
        if self._twin is None:
            self._twin = als_fitter(
                None, self.fitrange, self.fitlines, [self.ncompmin, self.ncompmax], nfill=self.nfill,
                specres=self.specres, contval=self.contval, Nrange=list(self.N_lims), brange=list(self.b_lims),
                zrange=[z for lim in self.z_lims for z in lim], Nrangefill=list(self.N_lims_fill),
                brangefill=list(self.b_lims_fill),
                wrangefill=[(1 + z) * self.linefill["wrest"] for lim in self.z_lims_fill for z in lim] or None,
                Asymmlike=False, spectrum=(self.obj_wl, self.obj, self.obj_noise),
                linepars=[(lp["wrest"], lp["f"], lp["gamma"]) for lp in self.linepars], velstep=self.velstep,
                conv_mode="jax", device=self.info.device, gauss_cdf=self.gauss_cdf)
        return self._twin


def _scalar(v):
    return float(np.asarray(v, dtype=float).reshape(-1)[0])
