"""What the reference module offers that needs no fitter, and so no device: the built-in line tables, the plain-text
spectrum reader, the `Gpriors` parser, the chain writer and the INI reader (`readconfig`).  `hires_fitter` imports every
name back, so each stays reachable as `hires_fitter.NAME`, where the reference keeps it."""
from __future__ import annotations

import configparser

import numpy as np

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
