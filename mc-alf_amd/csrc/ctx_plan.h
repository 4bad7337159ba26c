// What mcalf_create decides from the spec alone, before it touches a device: the checks of the spec, the launch geometry
// (CtxShape) and the host tables it uploads (CtxTables).  Header only, plain C++17 and no HIP include, so that
// tests/stubs/ctx_plan_check.cpp plans on the CPU exactly what host_abi.cpp: create_impl uploads, and
// tests/stubs/segment_search_check.cpp lays its grids out with fill_nu.  The float expressions, and their order, are the
// reference's numpy expressions: nu, ispec2 and lgis feed the kernels, and the GPU parity tests compare bits.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/mcalf_hip.h"
#include "kernel_args.h"

namespace mcalf {

// Every scalar of a context that follows from the spec (and MCALF_LINES_PER_SYNC); mcalf_ctx inherits them.
struct CtxShape {
    // problem
    long npix = 0;
    int nlines = 0, ncompmax = 0, nfill = 0, freespecres = 0, freecont = 0, conv_mode = 0;
    int ndim = 0, startind = 0, endind = 0;
    double specres_fixed = 0, specres_max = 0, contval_fixed = 1, velstep = 0;
    int asymm = 0;
    double veto4 = 0, veto5 = 0;
    // geometry
    int n_cap = 0, tile = 0, ntiles = 0, ncl_cap = 0, jax_half = 0, selfhalo = 0, lps = 4;
    size_t lds_bytes = 0, lds_bytes_inline = 0;    // (the one-launch variant of small calls folds 4 lines per barrier)
    // LSF wider than a workgroup tile (host_wide.cpp): n_cap is 0 for such a context (the tile carries no halo); wide_n_cap is
    // the half-width provisioned from specres_max.
    int wide = 0, wide_n_cap = 0;
    // from the tables: the widest interpolable segment, and for single-tile contexts the real segments and whether the set-up
    // may search their ends (kernel_args.h)
    double dnu_seg = 0;
    int seg_nreal = 0, seg_search = 0;
};

// The host arrays mcalf_create uploads.
struct CtxTables {
    std::vector<double> nu;                    // kExtMax entries for a self-halo context (virtual pixels past the spectrum), else npix
    std::vector<double> ispec2, lgis;          // [npix] 1/err^2 and its log
    std::vector<LineDev> lines;                // [nlines + 1]: the lines, then the filler
    std::vector<unsigned long long> segok;     // [ntiles] bit m: segment m of the tile may be interpolated
};

inline int plan_fail(std::string* msg, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
inline int plan_fail(std::string* msg, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    *msg = buf;
    return code;
}

// The FWHM the halo is provisioned for: specres_max, or the fixed resolution where that is the larger one.
inline double provisioned_specres(const mcalf_spec& sp) {
    double rmax = sp.specres_max;
    if (!sp.freespecres && !(rmax >= sp.specres_fixed)) rmax = sp.specres_fixed;
    return rmax;
}

// The refusals that need no device and no arithmetic.
inline int check_spec(const mcalf_spec* sp, std::string* msg) {
    if (!sp) return plan_fail(msg, MCALF_ERR_INVALID, "spec is NULL");
    if (sp->npix <= 0 || !sp->wl || !sp->flux || !sp->err)
        return plan_fail(msg, MCALF_ERR_INVALID, "npix must be > 0 and wl/flux/err non-NULL");
    if (sp->npix > (1 << 30)) return plan_fail(msg, MCALF_ERR_RANGE, "npix too large");
    if (sp->nlines <= 0 || !sp->lines) return plan_fail(msg, MCALF_ERR_INVALID, "need at least one line");
    if (sp->ncompmax < 0 || sp->nfill < 0) return plan_fail(msg, MCALF_ERR_INVALID, "negative component counts");
    if (!(sp->velstep > 0.0)) return plan_fail(msg, MCALF_ERR_INVALID, "velstep must be > 0");
    if (sp->conv_mode != MCALF_CONV_WRAP_NUMPY && sp->conv_mode != MCALF_CONV_SAME_EDGE_JAX)
        return plan_fail(msg, MCALF_ERR_INVALID, "unknown conv_mode %d", sp->conv_mode);
    const double rmax = provisioned_specres(*sp);
    if (!(rmax > 0.0) || !std::isfinite(rmax))
        return plan_fail(msg, MCALF_ERR_INVALID, "specres_max must be finite and > 0");
    return MCALF_OK;
}

// ---- the geometry ---------------------------------------------------------------------------------------------------------
// The LDS of a workgroup is laid out by ItemLds (kernel_args.h), the kernel's own carve-up: the folded tables of two barriers'
// lines, the records, the taps, the reduction slots, the interpolation weights, then the tile region.
// Pixels (tile and halo) a workgroup can hold: the tile region has ONE size (tile_doubles), so it is all of kExtMax when the
// fixed part and the region fit the budget, and nothing otherwise.
inline size_t tile_extent(int lps, int ncl_cap, int n_cap) {
    return ItemLds(lps, ncl_cap, n_cap).bytes(kExtMax) > kLdsBudget ? 0 : (size_t)kExtMax;
}
// Lines per barrier: 5 when that saves a barrier at the context's largest line count and the extra folded tables cost no
// tile pixels (LDS), else 4.
inline int auto_lines_per_sync(int ncl_cap, int n_cap) {
    return ((ncl_cap + 4) / 5 < (ncl_cap + 3) / 4 && tile_extent(5, ncl_cap, n_cap) == tile_extent(4, ncl_cap, n_cap)) ? 5 : 4;
}
// MCALF_LINES_PER_SYNC over it: 4 always, 5 under the same fit test.
inline int pick_lines_per_sync(int ncl_cap, int n_cap, int forced) {
    if (forced == 4 || (forced == 5 && tile_extent(5, ncl_cap, n_cap) == tile_extent(4, ncl_cap, n_cap))) return forced;
    return auto_lines_per_sync(ncl_cap, n_cap);
}
inline bool lsf_fits_tile(int lps, int ncl_cap, int n_cap) { return tile_extent(lps, ncl_cap, n_cap) >= 2 * (size_t)n_cap + 64; }

// The LSF half-width provisioned from specres_max (hires_fitter.py:458, and :557-559 for the fixed JAX grid, a float32 ceil).
inline int lsf_reach(int conv_mode, double rmax, double velstep) {
    const double sigma_max = (rmax / kFwhmToSigma) / velstep;
    if (conv_mode == MCALF_CONV_SAME_EDGE_JAX) return (int)std::ceil((float)(kKernelReach * sigma_max));
    return (rmax > velstep) ? (int)std::ceil(kKernelReach * sigma_max) : 0;
}

// Tiles are multiples of 8 pixels (the epilogue works in aligned groups of 8), balanced over the spectrum.
inline void plan_tiling(long npix, size_t ext, int n_cap, int* tile_out, int* ntiles_out) {
    const long tmax = ((long)ext - 2 * n_cap) & ~7L;
    long tile = std::min(tmax, (npix + 7) & ~7L);
    long ntiles = (npix + tile - 1) / tile;
    tile = (((npix + ntiles - 1) / ntiles) + 7) & ~7L;
    ntiles = (npix + tile - 1) / tile;
    *tile_out = (int)tile;
    *ntiles_out = (int)ntiles;
}

// The problem and geometry fields of `s` (everything but dnu_seg / seg_nreal / seg_search, which plan_tables adds) from a
// spec that passed check_spec.  lines_per_sync: MCALF_LINES_PER_SYNC (-1: not set).
inline int plan_shape(const mcalf_spec& sp, int lines_per_sync, CtxShape* out, std::string* msg) {
    CtxShape& s = *out;
    s = CtxShape();
    const double rmax = provisioned_specres(sp);
    s.npix = sp.npix;
    s.nlines = sp.nlines;
    s.ncompmax = sp.ncompmax;
    s.nfill = sp.nfill;
    s.freespecres = sp.freespecres ? 1 : 0;
    s.freecont = sp.freecont ? 1 : 0;
    s.conv_mode = sp.conv_mode;
    s.specres_fixed = sp.specres_fixed;
    s.specres_max = rmax;
    s.contval_fixed = sp.contval_fixed;
    s.velstep = sp.velstep;
    s.asymm = sp.asymmlike ? 1 : 0;                                  // hires_fitter.py:296-303
    s.veto4 = sp.asymm_n4 + 0.01 * (double)sp.npix;                  // gauss_cdf[1] + gracenum (:181,302)
    s.veto5 = sp.asymm_n5 + 0.01 * (double)sp.npix;                  // gauss_cdf[2] + gracenum (:300)
    s.startind = s.freecont + s.freespecres;                         // hires_fitter.py:169-174
    s.endind = s.startind + 3 * s.ncompmax + 1;                      // :176
    s.ndim = s.endind + 3 * s.nfill;                                 // :184-200

    s.n_cap = lsf_reach(s.conv_mode, rmax, sp.velstep);
    if (s.conv_mode == MCALF_CONV_SAME_EDGE_JAX) {
        s.jax_half = s.n_cap;
        if (2L * s.jax_half + 1 > s.npix)
            return plan_fail(msg, MCALF_ERR_INVALID,
                             "JAX-path LSF kernel (%d taps) is longer than the spectrum (%ld px): the reference's "
                             "jnp.convolve(..., 'same') / jnp.where (hires_fitter.py:674-681) cannot broadcast either",
                             2 * s.jax_half + 1, s.npix);
    }
    s.ncl_cap = std::max(1, s.ncompmax * s.nlines + s.nfill);
    s.lps = pick_lines_per_sync(s.ncl_cap, s.n_cap, lines_per_sync);
    if (!lsf_fits_tile(s.lps, s.ncl_cap, s.n_cap)) {
        // The LSF does not fit a workgroup tile with its halo: the fused kernel then runs without convolution (a tile
        // without halo) and the wide kernels convolve behind it (launch_wide) -- the reference simply builds a longer
        // kernel (hires_fitter.py:458-464; JAX semantics: its fixed grid, :549-560, whatever its length).
        if (2.0 * (double)s.n_cap + 1.0 > 6.0e7)
            return plan_fail(msg, MCALF_ERR_RANGE,
                             "LSF half-width %d px (specres_max %.3g km/s at %.3g km/s/px) with %d component-lines does not "
                             "fit a %d-pixel workgroup tile / the %zu-byte LDS budget", s.n_cap, rmax, sp.velstep,
                             s.ncl_cap, kExtMax, kLdsBudget);
        s.wide = 1;
        s.wide_n_cap = s.n_cap;
        s.n_cap = 0;
        s.lps = auto_lines_per_sync(s.ncl_cap, s.n_cap);
    }
    if (!lsf_fits_tile(s.lps, s.ncl_cap, s.n_cap))
        return plan_fail(msg, MCALF_ERR_RANGE, "%d component-lines do not fit the %zu-byte LDS budget", s.ncl_cap, kLdsBudget);
    plan_tiling(s.npix, tile_extent(s.lps, s.ncl_cap, s.n_cap), s.n_cap, &s.tile, &s.ntiles);
    s.lds_bytes = ItemLds(s.lps, s.ncl_cap, s.n_cap).bytes(s.tile + 2 * s.n_cap);
    s.lds_bytes_inline = ItemLds(4, s.ncl_cap, s.n_cap).bytes(s.tile + 2 * s.n_cap);
    s.selfhalo = (s.ntiles == 1 && s.n_cap < s.npix) ? 1 : 0;
    return MCALF_OK;
}

// ---- the tables -----------------------------------------------------------------------------------------------------------
// Is the wavelength grid recognisably linear (1) or logarithmic (2) over its last 64 pixels?  0: neither, or too short.
inline int grid_kind(const double* wl, long n) {
    if (n < 66) return 0;
    const double d = wl[n - 1] - wl[n - 2], r = wl[n - 1] / wl[n - 2];
    bool lin = true, lg = true;
    for (long i = n - 64; i < n - 1; ++i) {
        if (!(std::fabs((wl[i + 1] - wl[i]) - d) <= 1e-9 * std::fabs(d))) lin = false;
        if (!(std::fabs(wl[i + 1] / wl[i] - r) <= 1e-9 * std::fabs(r - 1.0))) lg = false;
    }
    return lin ? 1 : (lg ? 2 : 0);
}

// nu[0, nu_len) of a spectrum of n pixels: the pixel frequencies at z = 0, and past them (self-halo contexts index nu by
// thread, 0 .. kExtMax-1) VIRTUAL pixels.  Up to the next multiple of 64 they continue the wavelength grid when it is
// recognisably linear or logarithmic (so that the last, partial segment can be interpolated like the others; the virtual
// pixels' own results are never stored), else they repeat the last value; beyond that nothing is ever stored: nu = 0 puts
// these lanes at u = -nu0/dnu, thousands of Doppler widths away from every line, so their segments go the cheap node-only way.
inline void fill_nu(const double* wl, long n, long nu_len, double* nu) {
    for (long i = 0; i < n; ++i) {
        const double wave_cm = wl[i] / 1e8;                // hires_fitter.py:376
        nu[i] = kCcgs / wave_cm;                           // :362 at zp1 = 1
    }
    if (nu_len <= n) return;
    const long upto = std::min<long>(nu_len, (n + 63) & ~63L);
    const int kind = grid_kind(wl, n);
    // the common step from the pixels 64 apart (averages the grid's own rounding noise)
    const double step = kind == 1 ? (wl[n - 1] - wl[n - 65]) / 64.0
                      : kind == 2 ? std::exp(std::log(wl[n - 1] / wl[n - 65]) / 64.0) : 0.0;
    for (long i = n; i < nu_len; ++i) {
        if (kind != 0 && i < upto) {
            const double m = (double)(i - (n - 1));
            const double w = kind == 1 ? wl[n - 1] + m * step : wl[n - 1] * std::pow(step, m);
            nu[i] = kCcgs / (w / 1e8);
        } else {
            nu[i] = (i >= upto) ? 0.0 : nu[i - 1];
        }
    }
}

// Far-wing interpolation set-up: which 64-pixel segments of each tile may be interpolated in pixel-index space.  A segment
// qualifies when it lies inside the tile's extent without crossing the periodic seam and nu(pixel) itself is reproduced by
// the 8-node interpolant to 1e-15 (true for linear / logarithmic wavelength grids, false across masked gaps).  Returns the
// largest |nu(last) - nu(first)| of a qualifying real segment.
inline double segment_masks(const CtxShape& s, const std::vector<double>& nu, std::vector<unsigned long long>* segok) {
    const long nu_len = (long)nu.size();
    segok->assign(s.ntiles, 0ULL);
    double dnu_seg = 0.0;
    for (int t = 0; t < s.ntiles; ++t) {
        const long t0 = (long)t * s.tile;
        const long tlen = std::min<long>(s.tile, s.npix - t0);
        const long ext0 = s.selfhalo ? 0 : t0 - s.n_cap, extCount = tlen + 2L * s.n_cap;
        for (int m = 0; m < 64; ++m) {
            const long i0 = 64L * m;
            const long e0 = ext0 + i0;
            if (s.selfhalo) {
                if (e0 + 63 >= nu_len) continue;
                if (e0 >= ((s.npix + 63) & ~63L)) {            // wholly virtual (nu = 0): nothing to get wrong
                    (*segok)[t] |= 1ULL << m;
                    continue;
                }
                // otherwise: real pixels, the last segment completed by the virtual continuation of the grid
            } else {
                if (i0 + 64 > extCount) continue;
                if (e0 < 0 || e0 + 63 >= s.npix) continue;
            }
            bool ok = true;
            const double dir = nu[e0 + 63] - nu[e0];
            for (int i = 0; i < 64 && ok; ++i) {
                double v = 0.0;
                for (int k = 0; k < VT_INODES; ++k) v += VT_INTERP_W_HOST[i * VT_INODES + k] * nu[e0 + VT_INTERP_NODES[k]];
                const double x = nu[e0 + i];
                if (!std::isfinite(x) || !(std::fabs(v - x) <= 1e-15 * std::fabs(x))) ok = false;
                if (i > 0 && !((nu[e0 + i] - nu[e0 + i - 1]) * dir > 0.0)) ok = false;   // strictly monotonic
            }
            if (!ok) continue;
            (*segok)[t] |= 1ULL << m;
            dnu_seg = std::max(dnu_seg, std::fabs(dir));
        }
    }
    return dnu_seg;
}

// The tables of a planned shape (float64 host arithmetic identical to the reference's numpy expressions), and the three
// fields of the shape that follow from them.
inline void plan_tables(const mcalf_spec& sp, CtxShape* shape, CtxTables* t) {
    CtxShape& s = *shape;
    t->nu.assign(s.selfhalo ? (size_t)kExtMax : (size_t)s.npix, 0.0);
    fill_nu(sp.wl, s.npix, (long)t->nu.size(), t->nu.data());
    t->ispec2.resize(s.npix);
    t->lgis.resize(s.npix);
    for (long i = 0; i < s.npix; ++i) {
        t->ispec2[i] = 1.0 / (sp.err[i] * sp.err[i]);      // hires_fitter.py:292
        t->lgis[i] = std::log(t->ispec2[i]);               // :294
    }
    t->lines.resize(s.nlines + 1);
    for (int l = 0; l <= s.nlines; ++l) {
        const mcalf_line& src = (l < s.nlines) ? sp.lines[l] : sp.fill;
        t->lines[l].wrest_cm = src.wrest_A / 1e8;          // :376
        t->lines[l].f = src.f;
        t->lines[l].gamma4pi = src.gamma / (4.0 * M_PI);   // :361
        t->lines[l].nujk = kCcgs / t->lines[l].wrest_cm;   // :359
    }
    s.dnu_seg = segment_masks(s, t->nu, &t->segok);
    // The set-up finds a record's segment-mask word by boundary search where the ends of the tile's real segments form a
    // monotone sequence (established here, once; a wavelength array out of order keeps the walk over all 64 segments).
    s.seg_search = (s.selfhalo && seg_ends_searchable(t->nu.data(), s.npix, &s.seg_nreal)) ? 1 : 0;
}

}  // namespace mcalf
