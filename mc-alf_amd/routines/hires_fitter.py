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
which cli.py:345-348 calls after a PolyChord run, stay in `mcalf` -- and no prior log-density (`lnprior` and the `__call__`
built on it, hires_fitter.py:218-234,509-518, which no solver branch calls).  linetools is
replaced by an explicit `linepars=` argument plus a tiny built-in table (`LINE_TABLE`).
"""
from __future__ import annotations

import collections
import ctypes as C
import gc
from typing import Optional, Sequence

import numpy as np

from .. import _lib

# what als_fitter.model_band_batch returns: per-pixel mean, variance, quantiles [len(q), npix] and the count of non-NaN rows
ModelBand = collections.namedtuple("ModelBand", "mean var quantiles nvalid")

# (wrest [A], f, gamma [1/s]).  CIV: pinned by the reference's own test spectra
# (SURVEY.md section 4).  HI 1215: Morton (2003), NOT pinned (linetools absent).
LINE_TABLE = {
    "CIV 1548": (1548.204, 0.1899, 2.643e8),
    "CIV 1550": (1550.781, 0.09475, 2.628e8),
    "HI 1215": (1215.67, 0.4164, 6.265e8),
}

# The atomic constants the reference itself holds: after the database look-up it REPLACES f and gamma of three CrII
# lines (hires_fitter.py:100-110, "from atomic database in RCooke ALIS code"); wrest stays the database's.
LINE_OVERRIDES = {
    "CrII 2066": dict(f=0.0512, gamma=4.17e8),
    "CrII 2062": dict(f=0.0759, gamma=4.06e8),
    "CrII 2056": dict(f=0.103, gamma=4.07e8),
}


def apply_line_overrides(fitlines, linepars):
    """`linepars` = [(wrest, f, gamma), ...] as a database returned them for `fitlines`, with the reference's in-file
    overrides applied by line name (hires_fitter.py:100-110).  `wrest` must still come from the caller: the linetools
    'ISM' list the reference reads it from is not available here."""
    out = []
    for name, (w, f, g) in zip(fitlines, linepars):
        o = LINE_OVERRIDES.get(name)
        out.append((float(w), float(o["f"]), float(o["gamma"])) if o else (float(w), float(f), float(g)))
    return out


def sigma_clipped_median(x, sigma=3.0, maxiters=5):
    """Median after iterative sigma clipping about the median (the `med` that
    `astropy.stats.sigma_clipped_stats` returns with its defaults; hires_fitter.py:85).
    Pinned only for grids where nothing is clipped (both reference fixtures)."""
    x = np.asarray(x, dtype=float)
    x = x[np.isfinite(x)]
    for _ in range(maxiters):
        med, std = np.median(x), np.std(x)
        keep = np.abs(x - med) <= sigma * std
        if keep.all():
            break
        x = x[keep]
    return float(np.median(x))


def _read_ascii_table(path, coldef):
    """Minimal stand-in for `astropy.io.ascii.read` (hires_fitter.py:69-72) on plain-text tables: whitespace-,
    comma- or tab-separated columns whose names are either a `# Wave Flux Err` comment line (np.savetxt header,
    as in the reference's testdata) or a bare first line (what `ascii.write` / a CSV export produce); without any
    header the columns are taken in `coldef` order."""
    names, skip, delim = None, 0, None

    def split(text):
        return [t.strip() for t in text.split(",")] if "," in text else text.split()

    with open(path) as fh:
        for line in fh:
            s = line.strip()
            if not s:
                skip += 1
                continue
            if s.startswith("#"):
                names = split(s.lstrip("#").strip())
                skip += 1
                continue
            if "," in s:
                delim = ","
            try:
                [float(t) for t in split(s)]
            except ValueError:
                names = split(s)
                skip += 1
            break
    data = np.loadtxt(path, comments="#", skiprows=skip, ndmin=2, delimiter=delim)
    if names is None or len(names) != data.shape[1]:
        names = list(coldef)
    idx = [names.index(c) for c in coldef]
    return data[:, idx[0]], data[:, idx[1]], data[:, idx[2]]


def parse_gpriors(Gpriors, ndim):
    """(mu, sigma) [ndim] of the reference's `Gpriors` keyword (hires_fitter.py:34, :225-230): a flat sequence of 2 ndim entries
    `[val_0, sig_0, val_1, sig_1, ...]`, each a number or the string 'none'; a pair with either entry 'none' carries no Gaussian
    (sigma 0, mu 0).  None -> None."""
    if Gpriors is None:
        return None
    g = list(Gpriors)
    if len(g) != 2 * ndim:
        raise ValueError(f"Gpriors must have 2 * ndim = {2 * ndim} entries [val_0, sig_0, val_1, sig_1, ...], got {len(g)}")
    mu, sigma = np.zeros(ndim), np.zeros(ndim)
    for k in range(ndim):
        val, sig = g[2 * k], g[2 * k + 1]
        if (isinstance(val, str) and val == 'none') or (isinstance(sig, str) and sig == 'none'):
            continue
        mu[k], sigma[k] = float(val), float(sig)
        if not sigma[k] > 0.0:
            raise ValueError(f"Gpriors: the width of parameter {k} must be > 0 (or 'none'), got {sig!r}")
    return mu, sigma


class als_fitter:
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
        self._ctx = None
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
        pd = C.POINTER(C.c_double)
        sp.wl, sp.flux, sp.err = (a.ctypes.data_as(pd) for a in self._keep)
        sp.velstep = self.velstep
        sp.nlines = self.numlines
        lines = (_lib.mcalf_line * self.numlines)()
        for i, lp in enumerate(self.linepars):
            lines[i] = _lib.mcalf_line(lp["wrest"], lp["f"], lp["gamma"])
        sp.lines = lines
        sp.fill = _lib.mcalf_line(self.linefill["wrest"], self.linefill["f"], self.linefill["gamma"])
        sp.ncompmax = int(self.ncompmax)
        sp.nfill = int(self.nfill)
        sp.freespecres = int(self.freespecres)
        sp.freecont = int(self.freecont)
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
        sp.asymm_n4 = float(self.gauss_cdf[1])
        sp.asymm_n5 = float(self.gauss_cdf[2])
        ctx = C.c_void_p()
        if devices is None:
            _lib.check(lib.mcalf_create(C.byref(sp), C.byref(ctx)))
        else:
            _lib.check(lib.mcalf_create_multi(C.byref(sp), (C.c_int32 * len(devices))(*devices), len(devices), C.byref(ctx)))
        self._ctx = ctx
        self._lib = lib
        info = _lib.mcalf_info_t()
        _lib.check(lib.mcalf_info(ctx, C.byref(info)), ctx)
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

    def close(self):
        twin = getattr(self, "_twin", None)
        if twin is not None:
            twin.close()
            self._twin = None
        if self._ctx is not None:
            self._lib.mcalf_destroy(self._ctx)
            self._ctx = None

    def set_chunks(self, nchunks):
        """Row blocks a batch is issued in inside the library (0 = automatic, 1 = one launch per batch); results
        do not depend on it."""
        _lib.check(self._lib.mcalf_set_chunks(self._ctx, int(nchunks)), self._ctx)

    def chunks_for(self, batch):
        return int(self._lib.mcalf_get_chunks(self._ctx, int(batch)))

    def set_resident(self, idle_us):
        """Resident one-theta evaluator (mcalf_set_resident): with `idle_us` > 0 the one-theta callables are answered by a
        workgroup that stays on the GPU between calls -- no kernel launch per call -- and leaves by itself after `idle_us`
        microseconds without one; 0 turns it off.  Same bits as the launched form."""
        _lib.check(self._lib.mcalf_set_resident(self._ctx, int(idle_us)), self._ctx)

    def set_cu_mask(self, mask_words):
        """Restrict the context's own streams to the compute units of `mask_words` (uint32 words, bit i of word i // 32 =
        CU i; empty / None removes the mask) -- `mcalf_set_cu_mask`.  Results never depend on it; on anything but the
        eight XCDs of an unpartitioned MI355X large host batches take the row-block pipeline (`last_launch()`)."""
        words = np.ascontiguousarray([] if mask_words is None else mask_words, dtype=np.uint32)
        ptr = words.ctypes.data_as(C.POINTER(C.c_uint32)) if words.size else None
        _lib.check(self._lib.mcalf_set_cu_mask(self._ctx, ptr, int(words.size)), self._ctx)

    def last_launch(self, sub=None):
        """What the last call of this context did (`mcalf_last_launch`): entry plan, row blocks, whether the fused
        kernel ran as the persistent grid, its grid and work-item count, the device entries it was cut over.
        `sub=k`: device entry k of a multi-device context (`mcalf_last_launch_sub`)."""
        info = _lib.mcalf_launch_info_t()
        if sub is None:
            _lib.check(self._lib.mcalf_last_launch(self._ctx, C.byref(info)), self._ctx)
        else:
            _lib.check(self._lib.mcalf_last_launch_sub(self._ctx, int(sub), C.byref(info)), self._ctx)
        return info

    def get_config(self):
        """The knobs the context runs under and the MCALF_* variables its environment had set (`mcalf_get_config`)."""
        buf = C.create_string_buffer(2048)
        _lib.check(self._lib.mcalf_get_config(self._ctx, buf, len(buf)), self._ctx)
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
        pd = C.POINTER(C.c_double)
        _lib.check(self._lib.mcalf_scale_cube_batch(
            self._ctx, self._lo.ctypes.data_as(pd), self._hi.ctypes.data_as(pd), cubes.ctypes.data_as(pd),
            cubes.shape[0], int(bool(int_ncomp)), out.ctypes.data_as(pd)), self._ctx)
        return out

    def loglike_cube_batch(self, cubes, int_ncomp=True, return_theta=True):
        """Unit cube in -> (theta, logL) out: lnlhood_pc(_scale_cube_pc(cube)) for every row
        (hires_fitter.py:202-209, 250-262) in one device pass; the prior transform runs inside the
        per-sample set-up kernel.  `int_ncomp=False` gives the MultiNest flavour (:211-216)."""
        cubes = self._rows(cubes, self.ndim)
        pd = C.POINTER(C.c_double)
        self._ensure_prior(int_ncomp)
        logL = np.empty(cubes.shape[0])
        theta = np.empty_like(cubes) if return_theta else None
        _lib.check(self._lib.mcalf_loglike_cube_batch(
            self._ctx, cubes.ctypes.data_as(pd), cubes.shape[0],
            theta.ctypes.data_as(pd) if return_theta else None, logL.ctypes.data_as(pd)), self._ctx)
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
        if out is None:
            out = np.empty(n)
        elif out.dtype != np.float64 or not out.flags.c_contiguous or out.size != n:
            raise ValueError("out must be a C-contiguous float64 array with one entry per row")
        if grad_out is None:
            grad_out = np.empty((n, self.ndim))
        elif grad_out.dtype != np.float64 or not grad_out.flags.c_contiguous or grad_out.size != n * self.ndim:
            raise ValueError("grad_out must be a C-contiguous float64 array of shape [batch, ndim]")
        rc = self._lib.mcalf_loglike_grad_batch(self._ctx, self._ptr(P), n, self._ptr(out), self._ptr(grad_out))
        if rc:
            _lib.check(rc, self._ctx)
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
        if out is None:
            out = np.empty((n, yw))
        elif out.dtype != np.float64 or not out.flags.c_contiguous or out.size != n * yw:
            raise ValueError(f"out must be a C-contiguous float64 array of shape [batch, {yw}]")
        rc = fn(self._ctx, self._ptr(P), self._ptr(X), n, self._ptr(out))
        if rc:
            _lib.check(rc, self._ctx)
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

    def _ensure_prior(self, int_ncomp=None):
        """The prior box on the device (`mcalf_set_prior`), sent once per ncomp flavour.  `int_ncomp=None`: any flavour
        that is already there will do (the box is the same), the PolyChord one if none is."""
        have = getattr(self, "_prior_key", None)
        key = (True if have is None else have) if int_ncomp is None else bool(int_ncomp)
        if have != key:
            pd = C.POINTER(C.c_double)
            _lib.check(self._lib.mcalf_set_prior(self._ctx, self._lo.ctypes.data_as(pd),
                                                 self._hi.ctypes.data_as(pd), int(key)), self._ctx)
            self._prior_key = key
        if self._gauss is not None and not getattr(self, "_gauss_sent", False):
            mu, sigma = self._gauss
            _lib.check(self._lib.mcalf_set_gauss_prior(self._ctx, self._ptr(mu), self._ptr(sigma)), self._ctx)
            self._gauss_sent = True

    def set_gauss_prior(self, mu, sigma):
        """Gaussian prior factors on top of the box (`mcalf_set_gauss_prior`): parameter k carries
        exp(-0.5 ((theta_k - mu[k]) / sigma[k])^2) / sqrt(2 pi sigma[k]^2) where sigma[k] > 0 and none where sigma[k] == 0, not
        renormalised for the truncation by the box (hires_fitter.py:230).  `lnprior_batch`, `slice_replace_batch` /
        `nested_sample`, `ensemble_batch` / `ensemble_sample` and `tempered_batch` / `tempered_sample` honour it;
        `maximize_batch` does not.  The ncomp slot cannot carry one."""
        mu = np.ascontiguousarray(mu, dtype=float).reshape(-1)
        sigma = np.ascontiguousarray(sigma, dtype=float).reshape(-1)
        if mu.size != self.ndim or sigma.size != self.ndim:
            raise ValueError(f"mu and sigma must have ndim = {self.ndim} entries, got {mu.size} and {sigma.size}")
        self._gauss = None                                   # (what the constructor parsed is superseded)
        self._ensure_prior()
        _lib.check(self._lib.mcalf_set_gauss_prior(self._ctx, self._ptr(mu), self._ptr(sigma)), self._ctx)

    def clear_gauss_prior(self):
        """Back to the flat box: every entry runs the code path, and returns the bits, of a fitter that never had a Gaussian."""
        self._gauss = None
        self._ensure_prior()
        _lib.check(self._lib.mcalf_set_gauss_prior(self._ctx, None, None), self._ctx)

    @property
    def gauss_prior(self):
        """(mu, sigma, c) [ndim] as the library holds them (`mcalf_get_gauss_prior`), c[k] = ln(2 pi sigma[k]^2) as the kernels
        add it; None when no Gaussian is set."""
        self._ensure_prior()
        mu, sigma, c = (np.empty(self.ndim) for _ in range(3))
        n = C.c_int32(0)
        _lib.check(self._lib.mcalf_get_gauss_prior(self._ctx, self._ptr(mu), self._ptr(sigma), self._ptr(c), C.byref(n)), self._ctx)
        return (mu, sigma, c) if n.value > 0 else None

    def lnprior_batch(self, rows, cube=False):
        """lnprior[i] of every row on the device (`mcalf_lnprior_batch`; a HIP kernel): -inf for a row with a NaN or an entry
        outside the box, else the sum of the Gaussian factors' logarithms (hires_fitter.py:218-234), an exact 0 without any.
        `cube=True`: the rows are unit-cube rows, mapped through the box as `loglike_cube_batch` maps them."""
        rows = self._rows(rows, self.ndim)
        self._ensure_prior()
        out = np.empty(rows.shape[0])
        _lib.check(self._lib.mcalf_lnprior_batch(self._ctx, self._ptr(rows), rows.shape[0], int(bool(cube)), self._ptr(out)), self._ctx)
        return out

    def lnprior(self, p):
        """hires_fitter.py:218-234."""
        return float(self.lnprior_batch(np.asarray(p, dtype=float))[0])

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

    def _cube_posterior(self, U):
        """(theta, logL + lnprior) of unit-cube rows: the callable the host drivers start from."""
        theta, logL = self.loglike_cube_batch(U)
        return (theta, logL + self.lnprior_batch(U, cube=True)) if self._has_gauss() else (theta, logL)

    def _cube_with_prior(self, U):
        """(theta, logL, lnprior) of unit-cube rows, lnprior by one pass over the rows already transformed."""
        theta, logL = self.loglike_cube_batch(U)
        return theta, logL, self.lnprior_batch(theta)

    def _has_gauss(self):
        self._ensure_prior()
        n = C.c_int32(0)
        _lib.check(self._lib.mcalf_get_gauss_prior(self._ctx, None, None, None, C.byref(n)), self._ctx)
        return n.value > 0

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
        P = np.empty_like(P0)
        logL = np.empty(n)
        status = np.empty(n, dtype=np.int32)
        niter = np.empty(n, dtype=np.int32)
        _lib.check(self._lib.mcalf_maximize_batch(self._ctx, self._ptr(P0), n, C.addressof(opts), self._ptr(P), self._ptr(logL),
                                                  status.ctypes.data, niter.ctypes.data), self._ctx)
        return P, logL, status, niter

    def maximize(self, p0, **kw):
        """`maximize_batch` for one parameter vector: (p, logL, status, niter)."""
        self._check_scalar(p0)
        P, logL, status, niter = self.maximize_batch(np.asarray(p0, dtype=float).reshape(1, -1), **kw)
        return P[0], float(logL[0]), int(status[0]), int(niter[0])

    def slice_replace_batch(self, U0, Lmin, dirs, nmoves=None, max_steps=None, seed=0, stream_ids=None):
        """(U, theta, logL, status, nevals, moves): nested sampling's replacement step on the device
        (`mcalf_slice_replace_batch`; HIP kernels).  Every row of U0 (unit cube, [batch, ndim]) is a chain that makes
        `nmoves` (None: 2 ndim) slice-sampling moves along rows of `dirs` ([ndirs, ndim], shared by all rows) under the
        hard constraint logL > Lmin[row] (`Lmin`: a scalar or one value per row), in lock step for at most `max_steps`
        (None: 50 nmoves) steps of one trial per row.

        theta holds the transformed rows of U and logL[i] is `loglike_cube_batch(U)[i]` bit for bit.  status: 1 the row
        made its moves, 0 `max_steps` reached (the row holds its last accepted point, which satisfies the constraint),
        -1 the start lies outside the cube, has a NaN or does not satisfy the constraint (the row comes back as given).
        nevals: trials the row evaluated; moves: accepted ones.  The random words of a row are Philox4x64-10 of (step,
        stream_ids[row], seed) -- `stream_ids` (None: arange) must be distinct -- so a row's result does not depend on its
        batch or its position.

        Under a Gaussian prior (`Gpriors`, `set_gauss_prior`) the constrained quantity is logL + lnprior, evaluated inside the
        step's own kernels: `Lmin` bounds that sum and logL[i] is `loglike_cube_batch(U)[i] + lnprior_batch(U, cube=True)[i]`
        bit for bit."""
        U0 = self._rows(U0, self.ndim)
        n = U0.shape[0]
        dirs = self._rows(dirs, self.ndim)
        Lmin = np.ascontiguousarray(np.broadcast_to(np.asarray(Lmin, dtype=float), (n,)))
        sid = np.arange(n, dtype=np.uint64) if stream_ids is None else np.ascontiguousarray(stream_ids, dtype=np.uint64).reshape(-1)
        if sid.size != n:
            raise ValueError(f"stream_ids must have one entry per row ({n}), got {sid.size}")
        nmoves = 2 * self.ndim if nmoves is None else int(nmoves)
        max_steps = 50 * nmoves if max_steps is None else int(max_steps)
        self._ensure_prior()
        opts = _lib.mcalf_slice_opts(nmoves, max_steps, dirs.shape[0], 0, int(seed) & 0xFFFFFFFFFFFFFFFF)
        U, theta = np.empty_like(U0), np.empty_like(U0)
        logL = np.empty(n)
        status, nevals, moves = (np.empty(n, dtype=np.int32) for _ in range(3))
        _lib.check(self._lib.mcalf_slice_replace_batch(self._ctx, self._ptr(U0), self._ptr(Lmin), self._ptr(dirs), sid.ctypes.data, n,
                                                       C.addressof(opts), self._ptr(U), self._ptr(theta), self._ptr(logL),
                                                       status.ctypes.data, nevals.ctypes.data, moves.ctypes.data), self._ctx)
        return U, theta, logL, status, nevals, moves

    def set_slice_compact(self, on):
        """Packing of the live rows in `slice_replace_batch` (`mcalf_set_slice_compact`; off by default, MCALF_NS_COMPACT gives
        the initial value).  On: every lock step launches the likelihood over the rows that proposed a trial only, instead of
        over all rows of the call.  Results never depend on it, bit for bit; `slice_stats()` shows what it saves."""
        _lib.check(self._lib.mcalf_set_slice_compact(self._ctx, int(bool(on))), self._ctx)

    def slice_stats(self):
        """What the last `slice_replace_batch` call launched (`mcalf_slice_last_stats`), as a dict: `batch` its rows,
        `rows_launched` the rows handed to likelihood launches (the start launch included), `trials` the trials its rows
        proposed (the sum of nevals), `steps` the lock steps issued, `compact` whether the call packed its trial rows.
        All 0 before the first call."""
        st = _lib.mcalf_slice_stats_t()
        _lib.check(self._lib.mcalf_slice_last_stats(self._ctx, C.byref(st)), self._ctx)
        return {name: int(getattr(st, name)) for name, _ in st._fields_}

    def nested_sample(self, nlive, batch=None, nmoves=None, dlogz=1e-3, max_rounds=100000, seed=0, max_steps=None):
        """Nested sampling of this problem's posterior with the device's own two entries: `loglike_cube_batch` for the
        initial live points and `slice_replace_batch` for every replacement round (`nested.nested_sample` keeps the books).
        Returns a `nested.NestedResult`: logZ, logZ_err, H, the dead points with their log weights, and
        `equal_weight_samples(rng)`, whose output goes into `write_equal_weights`.  Its `rows_launched` counts the rows
        handed to likelihood launches: nlive for the initial points and `slice_stats()["rows_launched"]` of every round
        (`set_slice_compact(True)` lowers it; nothing else of the result depends on that setting).  Under a Gaussian prior
        (`Gpriors`, `set_gauss_prior`) both entries work on logL + lnprior: nested sampling of L g under the box measure, so
        `logL` holds that sum, `lnprior` the prior's part, and logZ is ln of the integral of L g over the cube."""
        from .. import nested
        launched = [int(nlive)]

        def replace(U0, Lmin, dirs, nmoves, seed, stream_ids):
            out = self.slice_replace_batch(U0, Lmin, dirs, nmoves=nmoves, max_steps=max_steps, seed=seed, stream_ids=stream_ids)
            launched[0] += self.slice_stats()["rows_launched"]
            return out

        gauss = self._has_gauss()
        res = nested.nested_sample(self._cube_posterior if gauss else (lambda U: self.loglike_cube_batch(U)), replace, self.ndim, nlive, batch=batch,
                                   nmoves=nmoves, dlogz=dlogz, max_rounds=max_rounds, seed=seed)
        res.rows_launched = launched[0]
        if gauss:
            res.lnprior = self.lnprior_batch(res.cube, cube=True)
        return res

    def ensemble_batch(self, U0, nsteps, thin=1, move="stretch", scale=None, seed=0, first_iter=0, chain=True):
        """(U, theta, logL, status, naccept, chainU, chainL): `nsteps` iterations of an affine-invariant ensemble sampler on
        the device (`mcalf_ensemble_batch`; HIP kernels).  The rows of U0 (unit cube, [nwalkers, ndim]; nwalkers even, >= 4)
        are the walkers; the halves [0, n / 2) and [n / 2, n) move in turn, each with partners from the other.  `move`:
        "stretch" (Goodman & Weare; `scale` = a > 1, None: 2.0) or "de" (differential evolution; `scale` = g > 0, None:
        2.38 / sqrt(2 ndim)).  The target is `loglike_cube_batch`'s logL with a flat prior over the cube; the integer `ncomp`
        slot is sampled with it, since the cube transform truncates it.

        theta holds the transformed rows of U and logL[i] is `loglike_cube_batch(U)[i]` bit for bit.  status: 0, or -1 for a
        walker whose start lies outside the cube or has a NaN (it never moves and comes back as given).  naccept: accepted
        proposals per walker.  chainU [nsteps // thin, nwalkers, ndim] and chainL [nsteps // thin, nwalkers] hold the state
        after every thin-th iteration, kept on the device until the call ends (`chain=False`: None, None).  The random words
        are Philox4x64-10 of (half-step, walker, seed): calling again with the returned U and `first_iter` advanced by
        `nsteps` is, bit for bit, the longer call.

        Under a Gaussian prior (`Gpriors`, `set_gauss_prior`) the target is logL + lnprior: the accept rule gains
        lnprior(trial) - lnprior(walker), evaluated inside the step's own kernels, while logL and chainL stay the likelihood's
        (`lnprior_batch(U, cube=True)` gives the prior's part)."""
        U0 = self._rows(U0, self.ndim)
        n = U0.shape[0]
        moves = {"stretch": _lib.MCALF_ENS_STRETCH, "de": _lib.MCALF_ENS_DE}
        if move not in moves:
            raise ValueError(f"move must be 'stretch' or 'de', got {move!r}")
        if scale is None:
            scale = 2.0 if move == "stretch" else 2.38 / np.sqrt(2.0 * self.ndim)
        nsteps, thin = int(nsteps), int(thin)
        self._ensure_prior()
        opts = _lib.mcalf_ens_opts(nsteps, thin, moves[move], 0, float(scale), int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_iter) & 0xFFFFFFFFFFFFFFFF)
        U, theta = np.empty_like(U0), np.empty_like(U0)
        logL = np.empty(n)
        status, naccept = (np.empty(n, dtype=np.int32) for _ in range(2))
        nkeep = nsteps // thin if chain and nsteps >= 0 and thin >= 1 else 0
        CU, CL = (np.empty((nkeep, n, self.ndim)), np.empty((nkeep, n))) if chain else (None, None)
        _lib.check(self._lib.mcalf_ensemble_batch(self._ctx, self._ptr(U0), n, C.addressof(opts), self._ptr(U), self._ptr(theta), self._ptr(logL),
                                                  status.ctypes.data, naccept.ctypes.data, self._ptr(CU) if chain else None,
                                                  self._ptr(CL) if chain else None), self._ctx)
        return U, theta, logL, status, naccept, CU, CL

    def ensemble_sample(self, nwalkers, nsteps, burn=0, thin=1, start=None, ball=None, seed=0, move="stretch", scale=None):
        """Ensemble MCMC of this problem's posterior with the device's own two entries: `ensemble_batch` for the burn-in and
        for the kept run (two calls, whatever their length) and `loglike_cube_batch` for the transformed rows of the kept
        chain (`ensemble.ensemble_sample` keeps the books).  The walkers start uniformly in the cube, or in a ball of
        half-width `ball` around the cube point `start` (e.g. a `maximize_batch` optimum mapped into the cube).  Returns an
        `ensemble.EnsembleResult`: the chain in cube and theta coordinates, logL, the acceptance fractions,
        `autocorr_time()`, and `flat()`, whose output goes into `write_equal_weights`, `model_band_batch` and `eqw_batch`."""
        from .. import ensemble

        def advance(U0, nsteps, thin=1, seed=0, first_iter=0, chain=True):
            return self.ensemble_batch(U0, nsteps, thin=thin, move=move, scale=scale, seed=seed, first_iter=first_iter, chain=chain)

        return ensemble.ensemble_sample(self._cube_with_prior if self._has_gauss() else (lambda U: self.loglike_cube_batch(U)), advance, self.ndim, nwalkers, nsteps, burn=burn, thin=thin,
                                        start=start, ball=ball, seed=seed)

    def tempered_batch(self, U0, betas, nsteps, thin=1, swap_every=1, move="stretch", scale=None, seed=0, first_iter=0, chain=True, chain_temps=1):
        """(U, theta, logL, status, naccept, nswap, chainU, chainL): `nsteps` iterations of the ensemble sampler of
        `ensemble_batch` at T = len(betas) temperatures at once, with swaps between neighbouring temperatures
        (`mcalf_tempered_batch`; HIP kernels).  U0 [T, nwalkers, ndim] holds the starts of every rung (unit cube; nwalkers even,
        >= 4); rung t samples logL^betas[t] (betas finite, >= 0, strictly decreasing; 1 <= T <= 64).  A half-step moves one half
        of every rung, T x nwalkers / 2 trial rows through one likelihood launch; after every global iteration g with
        (g + 1) % swap_every == 0 (0: never) every other pair of neighbouring rungs, alternating from round to round, exchanges
        walkers along a random shift, a swap costing no likelihood evaluation.

        U, theta [T, nwalkers, ndim], logL, status, naccept [T, nwalkers]: as `ensemble_batch`'s, per position; logL is always
        the untempered `loglike_cube_batch` value.  nswap [T - 1, nwalkers]: accepted swaps of position (t, w) with rung t + 1.
        chainL [nsteps // thin, T, nwalkers] keeps logL of every rung (the evidence needs them), chainU
        [nsteps // thin, chain_temps, nwalkers, ndim] the rows of the first `chain_temps` rungs (`chain=False`: None, None).
        The random words are Philox4x64-10 of (half-step or swap round, position, seed): calling again with the returned U and
        `first_iter` advanced by `nsteps` is, bit for bit, the longer call, and one rung at beta = 1 is `ensemble_batch`.

        Under a Gaussian prior (`Gpriors`, `set_gauss_prior`) rung t samples logL^betas[t] times the prior's Gaussian factors:
        the temperature acts on logL alone, the swap rule is unchanged (the prior cancels between rungs), and the rung at
        beta = 0 samples the Gaussian factors over the cube; logL and chainL stay the likelihood's."""
        U0 = np.ascontiguousarray(U0, dtype=float)
        betas = np.ascontiguousarray(betas, dtype=float).reshape(-1)
        T = betas.size
        if U0.ndim != 3 or U0.shape[0] != T or U0.shape[2] != self.ndim:
            raise ValueError(f"U0 must be [len(betas) = {T}, nwalkers, ndim = {self.ndim}], got {U0.shape}")
        n = U0.shape[1]
        moves = {"stretch": _lib.MCALF_ENS_STRETCH, "de": _lib.MCALF_ENS_DE}
        if move not in moves:
            raise ValueError(f"move must be 'stretch' or 'de', got {move!r}")
        if scale is None:
            scale = 2.0 if move == "stretch" else 2.38 / np.sqrt(2.0 * self.ndim)
        nsteps, thin, chain_temps = int(nsteps), int(thin), int(chain_temps)
        self._ensure_prior()
        opts = _lib.mcalf_pt_opts(nsteps, thin, moves[move], T, int(swap_every), chain_temps, float(scale), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                  int(first_iter) & 0xFFFFFFFFFFFFFFFF)
        U, theta = np.empty_like(U0), np.empty_like(U0)
        logL = np.empty((T, n))
        status, naccept = (np.empty((T, n), dtype=np.int32) for _ in range(2))
        nswap = np.zeros((max(T - 1, 0), n), dtype=np.int32)
        nkeep = nsteps // thin if chain and nsteps >= 0 and thin >= 1 else 0
        CU, CL = (np.empty((nkeep, min(max(chain_temps, 0), T), n, self.ndim)), np.empty((nkeep, T, n))) if chain else (None, None)
        _lib.check(self._lib.mcalf_tempered_batch(self._ctx, self._ptr(U0), n, self._ptr(betas), C.addressof(opts), self._ptr(U), self._ptr(theta),
                                                  self._ptr(logL), status.ctypes.data, naccept.ctypes.data, nswap.ctypes.data,
                                                  self._ptr(CU) if chain else None, self._ptr(CL) if chain else None), self._ctx)
        return U, theta, logL, status, naccept, nswap, CU, CL

    def tempered_sample(self, nwalkers, nsteps, ntemps=8, betas=None, burn=0, thin=1, swap_every=1, start=None, ball=None, seed=0, move="stretch",
                        scale=None):
        """Parallel tempering of this problem's posterior with the device's own two entries: `tempered_batch` for the burn-in
        and for the kept run (two calls, whatever their length) and `loglike_cube_batch` for the transformed rows of the cold
        rung (`tempering.tempered_sample` keeps the books).  `betas` (None: `tempering.default_ladder(ntemps, 1e-4)`, which
        ends at the prior) is the ladder; every rung holds `nwalkers` walkers, started uniformly in the cube or in a ball of
        half-width `ball` around the cube point `start`.  Returns a `tempering.TemperedResult`: logL of every rung, the
        acceptance and swap fractions per rung, `cold()` -- the beta[0] rung as an `ensemble.EnsembleResult` -- and the
        evidence by `logZ_stepping_stone()` and `logZ_ti()`.  Under a Gaussian prior the result carries `ln_prior_mass`, the
        ladder's Z at beta = 0, which both evidence routes add: they then report ln of the integral of L g over the cube, as
        `nested_sample` does."""
        from .. import tempering
        betas = tempering.default_ladder(ntemps, 1e-4) if betas is None else betas

        def advance(U0, nsteps, thin=1, swap_every=1, seed=0, first_iter=0, chain=True, chain_temps=1):
            return self.tempered_batch(U0, betas, nsteps, thin=thin, swap_every=swap_every, move=move, scale=scale, seed=seed, first_iter=first_iter,
                                       chain=chain, chain_temps=chain_temps)

        gauss = self._has_gauss()
        res = tempering.tempered_sample(self._cube_with_prior if gauss else (lambda U: self.loglike_cube_batch(U)), advance, self.ndim, nwalkers, nsteps, betas,
                                        burn=burn, thin=thin, swap_every=swap_every, start=start, ball=ball, seed=seed)
        if gauss:
            mu, sigma, _ = self.gauss_prior
            res.ln_prior_mass = tempering.ln_prior_mass(self._lo, self._hi, mu, sigma)
        return res

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
        pd = C.POINTER(C.c_double)
        _lib.check(self._lib.mcalf_chi2_batch(self._ctx, P.ctypes.data_as(pd), P.shape[0],
                                              out.ctypes.data_as(pd)), self._ctx)
        return out

    def model_batch(self, P, targonly=False):
        """model[i, :] = reconstruct_spec(P[i], targonly)."""
        P = self._rows(P, self.ndim)
        out = np.empty((P.shape[0], self.obj_wl.size))
        pd = C.POINTER(C.c_double)
        _lib.check(self._lib.mcalf_model_batch(self._ctx, P.ctypes.data_as(pd), P.shape[0], int(bool(targonly)),
                                               out.ctypes.data_as(pd)), self._ctx)
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
        pd = C.POINTER(C.c_double)
        _lib.check(self._lib.mcalf_onecomp_batch(self._ctx, Q.ctypes.data_as(pd), Q.shape[0], which,
                                                 out.ctypes.data_as(pd)), self._ctx)
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
        res = []
        for k, (want, shape) in enumerate(zip((comp, blend), shapes)):
            arr = None if out is None else out[k]
            if not want:
                arr = None
            elif arr is None:
                arr = np.empty(shape)
            elif arr.dtype != np.float64 or not arr.flags.c_contiguous or arr.size != int(np.prod(shape)):
                raise ValueError(f"out[{k}] must be a C-contiguous float64 array of shape {list(shape)}")
            res.append(arr)
        if res[0] is None and res[1] is None:
            raise ValueError("eqw_batch: at least one of comp / blend must be requested")
        rc = self._lib.mcalf_eqw_batch(self._ctx, self._ptr(P), n, _lib.MCALF_EQW_AS_WRITTEN if reference_indexing else _lib.MCALF_EQW_LAYOUT,
                                       None if res[0] is None else self._ptr(res[0]), None if res[1] is None else self._ptr(res[1]))
        if rc:
            _lib.check(rc, self._ctx)
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
        rc = self._lib.mcalf_model_band_batch(self._ctx, self._ptr(P), P.shape[0], int(bool(targonly)),
                                              self._ptr(qs) if qs.size else None, qs.size, self._ptr(mean), self._ptr(var),
                                              self._ptr(quant) if qs.size else None, self._ptr(nvalid))
        if rc:
            _lib.check(rc, self._ctx)
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
        ndim = self.ndim

        def host_loglike(p):
            p32 = np.asarray(p, dtype=np.float32)                        # jaxns hands float32 live points (:529-536)
            if p32.shape[-1:] != (ndim,):
                raise ValueError(f"parameter vectors must have {ndim} entries")
            rows = np.ascontiguousarray(p32.reshape(-1, ndim), dtype=np.float64)
            ll = twin.loglike_batch(rows).astype(np.float32)
            return ll.reshape(p32.shape[:-1]) if p32.ndim > 1 else ll.reshape(())[()]

        def host_grad(p):
            p32 = np.asarray(p, dtype=np.float32)
            if p32.shape[-1:] != (ndim,):
                raise ValueError(f"parameter vectors must have {ndim} entries")
            rows = np.ascontiguousarray(p32.reshape(-1, ndim), dtype=np.float64)
            ll, g = twin.loglike_grad_batch(rows)
            ll = ll.astype(np.float32)
            return (ll.reshape(p32.shape[:-1]) if p32.ndim > 1 else ll.reshape(())[()]), g.astype(np.float32).reshape(p32.shape)

        try:
            if use_jax is False:
                raise ImportError
            import jax
            import jax.numpy as jnp
        except ImportError:
            if use_jax:
                raise ImportError("JAX is not available.")
            host_loglike.fitter = twin
            host_loglike.host_grad = host_grad
            return host_loglike

        def value(p):                                                    # pragma: no cover - needs JAX
            shape = jax.ShapeDtypeStruct(p.shape[:-1], jnp.float32)
            return jax.pure_callback(lambda q: np.asarray(host_loglike(q), dtype=np.float32).reshape(q.shape[:-1]),
                                     shape, p, vmap_method="expand_dims")

        @jax.custom_vjp
        def log_likelihood(p):                                           # pragma: no cover - needs JAX
            return value(jnp.asarray(p, dtype=jnp.float32))

        def fwd(p):                                                      # pragma: no cover - needs JAX
            p = jnp.asarray(p)
            return value(p.astype(jnp.float32)), p

        def bwd(p, ct):                                                  # pragma: no cover - needs JAX
            # the callback is float32 in and out; the cotangent goes back in the primal's dtype (float64 under x64)
            p32 = p.astype(jnp.float32)
            g = jax.pure_callback(lambda q: np.asarray(host_grad(q)[1], dtype=np.float32).reshape(q.shape),
                                  jax.ShapeDtypeStruct(p32.shape, jnp.float32), p32, vmap_method="expand_dims")
            return ((jnp.asarray(ct, dtype=jnp.float32)[..., None] * g).astype(p.dtype),)

        log_likelihood.defvjp(fwd, bwd)
        log_likelihood.fitter = twin
        log_likelihood.host = host_loglike
        log_likelihood.host_grad = host_grad
        return log_likelihood

    def _jax_twin(self):
        """A second context over the same arrays with the JAX path's boundary semantics (kept for the
        lifetime of this object)."""
        if getattr(self, "_twin", None) is None:
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


# ---------------------------------------------------------------------------------------------
# Module-level helpers of the reference module (usable without an als_fitter instance)
# ---------------------------------------------------------------------------------------------

def write_equal_weights(path, logl, samples):
    """Chain file in the layout the CLI writes (cli.py:314-325):
    columns [weight = 1, -2 logL, parameters...]."""
    logl = np.asarray(logl, dtype=float).reshape(-1)
    samples = np.asarray(samples, dtype=float).reshape(logl.size, -1)
    np.savetxt(path, np.column_stack([np.ones_like(logl), -2.0 * logl, samples]))


_BOOL = {'True': True, 'False': False}


def _floats(txt):
    return np.array(txt.split(','), dtype=float)


# (section, option, key, default, converter); converter=None keeps the string
_CONFIG_TABLE = [
    ('input', 'coldef', 'coldef', ['Wave', 'Flux', 'Err'], lambda t: [x.strip() for x in t.split(',')]),
    ('input', 'specres', 'specres', np.array([7.0]), _floats),
    ('input', 'asymmlike', 'asymmlike', False, lambda t: _BOOL[t]),
    ('input', 'solver', 'solver', 'polychord', None),
    ('components', 'ncomp', 'ncomp', np.array((1, 1), dtype=int), lambda t: np.array(t.split(','), dtype=int)),
    ('components', 'nfill', 'nfill', 0, int),
    ('components', 'contval', 'contval', np.array([1]), _floats),
    ('components', 'Nrange', 'Nrange', np.array((11.5, 16)), _floats),
    ('components', 'brange', 'brange', np.array((1, 30)), _floats),
    ('components', 'zrange', 'zrange', None, _floats),
    ('components', 'Nrangefill', 'Nrangefill', np.array((11.5, 16)), _floats),
    ('components', 'brangefill', 'brangefill', np.array((1, 30)), _floats),
    ('components', 'wrangefill', 'wrangefill', None, _floats),
    ('plots', 'nmaxcols', 'nmaxcols', 5, lambda t: int(t[0])),        # first character only (:886)
    ('plots', 'yrange', 'yrange', np.array((-0.1, 1.2)), _floats),
    ('run', 'dofit', 'dofit', True, lambda t: _BOOL[t]),
    ('run', 'doplot', 'doplot', True, lambda t: _BOOL[t]),
    ('run', 'showprogress', 'showprogress', False, lambda t: _BOOL[t]),
    ('run', 'device', 'device', 'cpu', None),
]


def readconfig(configfile=None, logger=None):
    """INI file -> run-parameter dict with the keys, defaults and quirks of hires_fitter.py:762-969
    (mandatory input.specfile / wavefit / linelist; literal 'True'/'False' booleans; chaindir and
    plotdir prefixed by outdir; solver sections copied verbatim)."""
    try:
        import configparser
    except ImportError:  # pragma: no cover
        import ConfigParser as configparser
    cfg = configparser.ConfigParser()
    cfg.read(configfile)
    for opt in ('specfile', 'wavefit', 'linelist'):
        if not cfg.has_option('input', opt):
            raise configparser.NoOptionError('input', opt)
    edges = cfg.get('input', 'wavefit').split(',')
    if len(edges) % 2 == 1:
        raise ValueError("Number of wavefit values must be even")
    wavefit = [(float(edges[2 * i]), float(edges[2 * i + 1])) for i in range(len(edges) // 2)]

    def opt(section, name, default, conv=None):
        if not cfg.has_option(section, name):
            return default
        txt = cfg.get(section, name)
        return txt if conv is None else conv(txt)

    datadir = opt('pathing', 'datadir', './')
    outdir = opt('pathing', 'outdir', './')
    run = {'specfile': datadir + cfg.get('input', 'specfile'),
           'wavefit': wavefit,
           'linelist': [x.strip() for x in cfg.get('input', 'linelist').split(',')],
           'chaindir': outdir + opt('pathing', 'chaindir', 'fits/'),
           'plotdir': outdir + opt('pathing', 'plotdir', 'plots/'),
           'chainfmt': opt('pathing', 'chainfmt', 'pc_fits_{}_{1}')}
    for section, name, key, default, conv in _CONFIG_TABLE:
        run[key] = opt(section, name, default, conv)
    for section in ('mn_settings', 'pc_settings', 'jaxns_settings'):
        if cfg.has_section(section):
            run[section] = {o: _BOOL.get(cfg.get(section, o), cfg.get(section, o)) for o in cfg.options(section)}
    return run
