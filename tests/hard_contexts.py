"""The contexts on which `launch()` leaves the plain route -- several tiles, a wide LSF, JAX convolution semantics, bad pixels,
the asymmetric veto, row blocks, the persistent grid -- each as the kwargs of `als_fitter`, at the smallest shape that still
takes its path.  Shared by tests/test_sampler_contexts_host.py (the numpy oracle alone checks that every input does what the GPU
tests rely on) and tests/test_gpu_sampler_contexts.py (the samplers and the fitter on each of them).  A plain module like
tests/cases.py: nothing here touches a device."""
import numpy as np

from cases import BAD_KINDS, problem_from_kwargs, tiny_problem, with_bad_pixels
from oracle import numpy_oracle as o
from test_gpu_fit import _civ
from test_gpu_wide_lsf import _problem

NAMES = ("two_tile", "wide", "wide_two_tile", "jax", "bad_pixels", "veto", "chunked", "persistent")

TILE = 4096                         # pixels of a workgroup tile, halo included: an LSF of 2 n_cap + 64 > TILE is `wide`
BAD_AT = (0, 150, 299)              # the first, an interior and the last fitted pixel of the 300-pixel problem
VETO_CDF = [50, 10, 5]              # more than 10 pixels above 4 sigma or 5 above 5 sigma (plus 1 % of the pixels): logL = -inf
CHUNKS = 3                          # `fit.set_chunks` of the `chunked` context

# the start ball of every GPU test: half-width BALL round the best of NDRAW uniform draws of default_rng(DRAW_SEED) ...
NDRAW, DRAW_SEED, BALL, BALL_SEED = 128, 2, 0.05, 4
# ... but on `veto`, whose ball is placed across the veto's edge (tests/test_sampler_contexts_host.py: by the numpy oracle
# between 10 % and 90 % of its draws are vetoed)
VETO_CENTRE = np.array([0.5, 0.3, 0.5, 0.5])
VETO_HALF = 0.2


def _two_lines():
    """The 300-pixel problem of the sampler tests: CIV 1548 / 1550, three components, a filler, free resolution and continuum."""
    return _civ(npix=300, specres=(6.0, 9.0), contval=(0.9, 1.1))[0]


def two_tile():
    return _civ(npix=4500, specres=(6.0, 9.0), contval=(0.9, 1.1))[0]


def wide():
    return _problem(333, 0.0031, (6.0, 9.0), (0.9, 1.1), nfill=2)


def wide_two_tile():
    return _problem(4500, 0.0045, (8.0, 8.5))


def jax():
    return dict(_two_lines(), conv_mode="jax")


def bad_pixels():
    return with_bad_pixels(_two_lines(), BAD_AT, BAD_KINDS)


def bad_pixels_clean():
    """`bad_pixels` before its pixels were made bad."""
    return _two_lines()


def veto():
    return dict(tiny_problem(64), Asymmlike=True, gauss_cdf=list(VETO_CDF))


def chunked():
    """To be followed by `fit.set_chunks(CHUNKS)`."""
    return tiny_problem(64)


def persistent():
    """The persistent grid is a matter of the launch's size: `persistent_walkers`."""
    return tiny_problem(64)


def kwargs(name):
    return globals()[name]()


def persistent_walkers(compute_units):
    """Walkers whose half-ensemble has 4 x 2 x (compute units) items on this one-tile context: the smallest launch that takes
    the persistent grid (host_launch.cpp: launch_range)."""
    return 2 * 4 * 2 * int(compute_units)


def n_cap(kw):
    """The LSF half-width the context provisions (the formula tests/test_gpu_wide_lsf.py asserts of `fit.info.n_cap`)."""
    return int(np.ceil(3.0348 * (max(kw["specres"]) / 2.354820) / kw["velstep"]))


def is_wide(kw):
    return kw.get("velstep") is not None and kw.get("conv_mode", "numpy") == "numpy" and 2 * n_cap(kw) + 64 > TILE


def draws(ndim):
    return np.random.default_rng(DRAW_SEED).random((NDRAW, ndim))


def ball(centre, half, n, seed=BALL_SEED):
    """`n` rows of the ball, as tests/test_gpu_ens.py draws them."""
    centre = np.asarray(centre, dtype=float)
    return np.clip(centre + half * (2.0 * np.random.default_rng(seed).random((n, centre.size)) - 1.0), 0.0, 1.0)


def veto_ball(n, seed=BALL_SEED):
    return ball(VETO_CENTRE, VETO_HALF, n, seed)


def wide_rows_per_pass(npix, n_cap_, batch):
    """Live points per pass of a wide-LSF launch (host_wide.cpp): each scratch buffer stays below 512 MiB."""
    per_row = 8 * max(int(npix), 2 * int(n_cap_) + 1)
    return int(min(batch, 65535, max(1, (512 << 20) // per_row)))


def fit_case(name):
    """(centre, free, max_iter) of the Levenberg-Marquardt comparison on `two_tile`, `wide`, `jax` or `bad_pixels`: the starts
    are `test_gpu_fit._starts` round the parameter row `centre`, the box is narrowed to that row in every coordinate but `free`
    and the ncomp slot, and both sides make at most `max_iter` outer iterations.

    The bars of that comparison (tests/test_gpu_fit.py: the stopping rule's own ftol (1 + |logL|) and fit_reference.THETA_BAR)
    hold between two runs that end at one well-defined optimum, or that have made one well-conditioned step; they say nothing
    about two paths through a flat valley.  With everything free these problems are flat: the filler at logN 12 is invisible,
    the resolution is bimodal, the third component is blended (the restatement alone, from these starts, rejects half of its
    steps and needs 50 to 100 iterations, with the resolution ending at either bound).  So the two-line problems float what
    their data determine -- the continuum and the (N, z, b) of the two components the data were made with -- and the
    restatement converges from every start in 5 or 6 accepted steps (status 1).  On `wide` the LSF spans 3742 of 333 pixels
    and wraps round the spectrum 22 times, so a model is flat whatever its lines are and the data determine the continuum
    alone: logL is exactly quadratic in it, one damped step lands on the optimum, and every later decision compares two
    values that are equal to rounding.  There the comparison is that one step (max_iter 1: accepted, with a gain 1e5 to 1e8
    times the stopping rule's bar)."""
    kw = kwargs(name)
    prob = problem_from_kwargs(kw)
    s = prob.startind
    if name == "wide":
        lo = np.array([np.min(b) for b in prob.bounds], dtype=float)
        hi = np.array([np.max(b) for b in prob.bounds], dtype=float)
        centre = 0.5 * (lo + hi)
        centre[s] = float(prob.ncompmax)
        centre[s + 1:prob.endind:3] = lo[s + 1]            # every column density at its lower bound
        centre[prob.endind::3] = lo[prob.endind]           # (the two fillers' too)
        return centre, [s - 1], 1
    npix = {"two_tile": 4500, "jax": 300, "bad_pixels": 300}[name]
    centre = _civ(npix=npix, specres=(6.0, 9.0), contval=(0.9, 1.1))[1]
    return centre, [s - 1] + list(range(s + 1, s + 7)), 30


def oracle_theta(kw, U):
    """The cube rows U as parameter rows (hires_fitter.py:202-209)."""
    prob = problem_from_kwargs(kw)
    return np.array([o.scale_cube_pc(prob, u) for u in np.atleast_2d(U)])


def oracle_loglike(kw, P):
    """logL of the parameter rows P by the numpy oracle, under the context's own semantics: the float64 restatement of the
    JAX path for `conv_mode="jax"`, the veto with the context's thresholds for `Asymmlike`, `loglike_batch` otherwise."""
    prob = problem_from_kwargs(kw)
    P = np.atleast_2d(np.asarray(P, dtype=float))
    with np.errstate(all="ignore"):
        if kw.get("conv_mode") == "jax":
            return np.array([o.jax_loglike_f64(prob, p) for p in P])
        if kw.get("Asymmlike"):
            return np.array([o.lnlhood_worker(prob, p, asymm_thresholds=tuple(kw["gauss_cdf"][1:])) for p in P])
        return o.loglike_batch(prob, P)


def oracle_cube_loglike(kw, U):
    return oracle_loglike(kw, oracle_theta(kw, U))
