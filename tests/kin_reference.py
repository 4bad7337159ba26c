"""The yardstick of mcalf_kinematics_batch: the optical-depth kinematics of ONE parameter vector restated in numpy from nothing
but the oracle's `voigt_tau` and `decode` (oracle/numpy_oracle.py), operation for operation as include/mcalf_hip.h states them:

    tau[k]   = sum_{c < nc} tau_cl(wl[k])          slots in slot order, one accumulator from 0.0
    t[k]     = tau[k] dlam[k]                      dlam = insert(diff(wl), 0, diff(wl)[0])
    S        = cumsum(t) (sequential),  I = S[-1]
    lam_mean = piv + M1 / I,   piv = wl[npix // 2],  M1 = cumsum(t (wl - piv))[-1]
    lam_rms  = sqrt(cumsum(t (wl - lam_mean)^2)[-1] / I)
    e        = cell edges [npix + 1]
    lam_q    = e[k+1] - (e[k+1] - e[k]) frac,  k the first pixel with !(S[k] < q I) (none: npix - 1), frac = (S[k] - q I) / t[k]
               clamped to [0, 1], 0 where t[k] > 0 does not hold

I not finite or 0: the other three are NaN.  Every operation is one ufunc; the sums are np.cumsum, which adds in order.  The
comparison helpers below carry the bars of tests/test_gpu_kin.py."""
import math

import numpy as np

from oracle import numpy_oracle as o

TOL_ABS, TOL_REL = 1e-11, 1e-9            # the equivalent widths' bar (tests/eqw_reference.py)
CIV1548 = (1548.204, 0.1899, 2.643e8)


def seam_kw(ncompmax=1):
    """The seam problem of the CPU and GPU tests: 4500 pixels, CIV 1548 alone, components placed relative to `seam_lam0`, which
    lies midway between pixels 2047 and 2048 -- the boundary of the pixel kernels' tiles 0 and 1."""
    wl = np.linspace(6180.0, 6220.0, 4502)[1:-1]
    return dict(fitrange=[[6180.0, 6220.0]], fitlines=["CIV 1548"], linepars=[CIV1548], ncomp=[0, ncompmax], specres=[8.0],
                Nrange=[12.0, 16.0], brange=[1.0, 40.0], zrange=[2.99, 3.03], velstep=float(np.median(np.diff(wl) / wl[1:]) * o.CLIGHT_KMS),
                spectrum=(wl, np.ones_like(wl), np.full_like(wl, 0.02)))


def seam_lam0(kw):
    wl = kw["spectrum"][0]
    return 0.5 * (wl[2047] + wl[2048])


def seam_row(kw, N, b, offsets=(0.0,)):
    """One row of the seam problem: a component of (N, b) at seam_lam0 + offset for every offset (Angstrom)."""
    p = [float(len(offsets))]
    for d in offsets:
        p += [N, (seam_lam0(kw) + d) / CIV1548[0] - 1.0, b]
    return np.array(p)


def active_count(prob, p, jax=False):
    slot = float(p[prob.startind])
    if not math.isfinite(slot):
        return 0
    nc = math.floor(slot) if jax else o.decode(prob, p)[2]
    return min(max(int(nc), 0), prob.ncompmax)


def dlambda(wl):
    dl = np.diff(wl)
    return np.insert(dl, 0, dl[0])


def edges(wl):
    dl = dlambda(wl)
    e = np.empty(wl.size + 1)
    e[0] = wl[0] - dl[0] / 2
    e[1:-1] = (wl[:-1] + wl[1:]) / 2
    e[-1] = wl[-1] + dl[-1] / 2
    return e


def terms(prob, p, jax=False):
    """t[nlines, npix] of one row."""
    p = np.asarray(p, dtype=float)
    nc, first = active_count(prob, p, jax), prob.startind + 1
    tau = np.zeros((prob.numlines, prob.wl.size))
    with np.errstate(all="ignore"):
        for c in range(nc):
            N, z, b = p[first + 3 * c: first + 3 * c + 3]
            for l, (wrest, f, gam) in enumerate(prob.lines):
                tau[l] = tau[l] + o.voigt_tau(prob.wl / 1e8, N, z, b * 1e5, wrest / 1e8, f, gam)
        return tau * dlambda(prob.wl)


def quantile(wl_edges, S, t, I, q):
    """lam_q of one line from its cumulative S, its terms t and its total I."""
    target = q * I
    ge = ~(S < target)
    k = int(np.argmax(ge)) if ge.any() else S.size - 1
    frac = 0.0
    if t[k] > 0:
        frac = min(max((S[k] - target) / t[k], 0.0), 1.0)
    return wl_edges[k + 1] - (wl_edges[k + 1] - wl_edges[k]) * frac


class Row:
    """Everything of one row: I, lam_mean, lam_rms [nlines], lam_q [nlines, nq], and the cumulatives S [nlines, npix]."""

    def __init__(self, prob, p, q=(), jax=False):
        wl = prob.wl
        q = np.atleast_1d(np.asarray(q, dtype=float))
        self.e = edges(wl)
        t = terms(prob, p, jax)
        nl = prob.numlines
        self.t, self.S = t, np.cumsum(t, axis=1)
        self.I = self.S[:, -1].copy()
        self.lam_mean, self.lam_rms, self.lam_q = np.full(nl, np.nan), np.full(nl, np.nan), np.full((nl, q.size), np.nan)
        piv = wl[wl.size // 2]
        with np.errstate(all="ignore"):
            for l in range(nl):
                I = self.I[l]
                if not np.isfinite(I) or I == 0:
                    continue
                self.lam_mean[l] = piv + np.cumsum(t[l] * (wl - piv))[-1] / I
                d = wl - self.lam_mean[l]
                self.lam_rms[l] = np.sqrt(np.cumsum(t[l] * d * d)[-1] / I)
                for j, qq in enumerate(q):
                    self.lam_q[l, j] = quantile(self.e, self.S[l], t[l], I, qq)

    def C(self, l, lam):
        """The piecewise-linear cumulative of line l through (e[k+1], S[k]) with C(e[0]) = 0, at wavelength lam."""
        return float(np.interp(lam, self.e, np.concatenate([[0.0], self.S[l]])))


def rows(prob, P, q=(), jax=False):
    return [Row(prob, p, q, jax) for p in np.atleast_2d(P)]


# ---- the bars of the GPU tests: each returns the worst error / bar and raises AssertionError where a cell misses ----------
def _same_nan_and_zero(got, want, what):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN cells differ"
    assert np.array_equal(got == 0.0, want == 0.0), f"{what}: exact-0 cells differ"
    return got, want, np.isfinite(want)


def check_I(got, ref_rows):
    want = np.array([r.I for r in ref_rows])
    got, want, fin = _same_nan_and_zero(got, want, "I")
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), "I: infinite cells differ"
    ratio = np.abs(got[fin] - want[fin]) / (TOL_ABS + TOL_REL * np.abs(want[fin]))
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"I: worst error / bar {worst:.3g}"
    return worst


def check_mean(got, ref_rows, W):
    want = np.array([r.lam_mean for r in ref_rows])
    got, want, fin = _same_nan_and_zero(got, want, "lam_mean")
    ratio = np.abs(got[fin] - want[fin]) / (TOL_ABS + 2 * TOL_REL * W)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"lam_mean: worst error / bar {worst:.3g}"
    return worst


def check_rms(got, ref_rows, W):
    """Compared as variances: the square root is not well conditioned near 0."""
    want = np.array([r.lam_rms for r in ref_rows])
    got, want, fin = _same_nan_and_zero(got, want, "lam_rms")
    ratio = np.abs(got[fin] ** 2 - want[fin] ** 2) / (TOL_ABS + 4 * TOL_REL * W * W)
    worst = float(ratio.max()) if ratio.size else 0.0
    assert worst <= 1.0, f"lam_rms: worst error / bar (variances) {worst:.3g}"
    return worst


def check_quantiles(got, ref_rows, q):
    """|C_ref(lam_got) - q I_ref| within the bar of I, and lam_got inside [e[0], e[npix]]; NaN cells coincide with the
    reference's (its lam_q is NaN exactly where I is 0 or not finite)."""
    got = np.asarray(got, dtype=float)
    q = np.atleast_1d(np.asarray(q, dtype=float))
    want = np.array([r.lam_q for r in ref_rows]).reshape(got.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "lam_q: NaN cells differ"
    worst = 0.0
    for i, r in enumerate(ref_rows):
        for l in range(got.shape[1]):
            for j in range(q.size):
                lam = got[i, l, j]
                if np.isnan(lam):
                    continue
                assert r.e[0] <= lam <= r.e[-1], f"lam_q[{i}, {l}, {j}] = {lam} outside [{r.e[0]}, {r.e[-1]}]"
                worst = max(worst, abs(r.C(l, lam) - q[j] * r.I[l]) / (TOL_ABS + TOL_REL * abs(r.I[l])))
    assert worst <= 1.0, f"lam_q: worst error / bar (in C) {worst:.3g}"
    return worst


def check_all(kin, ref_rows, q, W, what=""):
    """The four bars on a Kinematics result; prints and returns the worst ratios (I, mean, rms, quantiles)."""
    w = (check_I(kin.tau_int, ref_rows), check_mean(kin.lam_mean, ref_rows, W), check_rms(kin.lam_rms, ref_rows, W),
         check_quantiles(kin.lam_q, ref_rows, q) if len(np.atleast_1d(q)) else 0.0)
    print(f"kinematics {what}: worst error / bar: I {w[0]:.3g}, lam_mean {w[1]:.3g}, lam_rms {w[2]:.3g}, lam_q {w[3]:.3g}")
    return w
