"""The chain diagnostics of include/mcalf_hip.h (mcalf_chain_stats, mcalf_ensemble_converge) restated in numpy: direct sums, not
an FFT, accumulated in np.longdouble, so that the restatement's own rounding is negligible next to a float64 kernel's.  The
definitions are the header's; the order of a sum does not matter at this precision."""
import math

import numpy as np

LD = np.longdouble


def sokal_window(rho, c):
    """(tau, M, reached, margin) of the ACF rho [L + 1]: tau(m) = 2 sum_{t <= m} rho(t) - 1, M the smallest m with m >= c tau(m)
    (else M = L, reached False); margin = min over m <= M of |m - c tau(m)|, how far the rule's comparisons stand off."""
    rho = np.asarray(rho, dtype=LD)
    tau = 2.0 * np.cumsum(rho) - 1.0
    m = np.arange(rho.size)
    with np.errstate(invalid="ignore"):
        ok = m >= c * tau
    reached = bool(ok.any())
    M = int(np.argmax(ok)) if reached else rho.size - 1
    with np.errstate(invalid="ignore"):
        margin = float(np.min(np.abs(m[:M + 1] - c * tau[:M + 1])))
    return float(tau[M]), M, reached, margin


def acov(xc, L, c=None, chunk=32):
    """c(tau) = sum_{t <= T - 1 - tau} xc[t] xc[t + tau] along axis 0 for tau = 0 .. L (the biased sum).  With `c`, xc [T, n] of one
    coordinate: the lags are made `chunk` at a time and the rest is left NaN once the walker-averaged ACF so far has reached
    its window -- the rule reads nothing behind M."""
    T = xc.shape[0]
    out = np.full((L + 1,) + xc.shape[1:], np.nan, dtype=LD)
    for tau in range(L + 1):
        out[tau] = (xc[:T - tau] * xc[tau:]).sum(axis=0)
        if c is not None and (tau + 1) % chunk == 0:
            live = out[0] != 0
            with np.errstate(invalid="ignore", divide="ignore"):
                rho = (out[:tau + 1, live] / out[0, live]).sum(axis=1) / LD(max(int(live.sum()), 1))
            if sokal_window(rho, c)[2]:
                break
    return out


def chain_stats(X, status=None, c=5.0, max_lag=None, full_acf=True):
    """A dict of the outputs of mcalf_chain_stats for the chain X [T, n, d]: mean var tau tau_mean rhat ess (float64 [d]),
    M M_mean nused flags (int [d]), acf [d, L + 1], and the window margins margin, margin_mean [d].  full_acf=False leaves the
    ACF behind a window that was reached NaN (a replay of many checks of a long chain wants tau alone)."""
    X = np.asarray(X, dtype=float)
    T, n, d = X.shape
    L = T - 1 if not max_lag else int(max_lag)
    used = np.ones(n, dtype=bool) if status is None else np.asarray(status) == 0
    x = X[:, used, :].astype(LD)
    nok = int(used.sum())
    out = {k: np.full(d, np.nan) for k in ("mean", "var", "tau", "tau_mean", "rhat", "ess", "margin", "margin_mean")}
    out.update({k: np.zeros(d, dtype=np.int64) for k in ("M", "M_mean", "nused", "flags")})
    out["acf"] = np.full((d, L + 1), np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        # constancy is decided exactly, as the header has it: a series with x_t == x_0 for every t has its means = x_0, not a
        # rounded sum's; a coordinate in which every used walker is constant at ONE value v has mean = v
        konst = (x == x[0]).all(axis=0)                                       # [nok, d]
        frozen = konst.all(axis=0) & (x[0] == x[0, :1]).all(axis=0) if nok else np.zeros(d, dtype=bool)
        mean = x.sum(axis=(0, 1)) / (LD(T) * nok)
        if nok:
            mean = np.where(frozen, x[0, 0], mean)
        var = ((x - mean) ** 2).sum(axis=(0, 1)) / (LD(T) * nok - 1) if nok else np.full(d, np.nan)
        h = T // 2
        halves = np.concatenate([x[:h], x[T - h:]], axis=1)                   # [h, 2 nok, d]
        m = np.where(np.concatenate([konst, konst], axis=0), halves[0], halves.mean(axis=0))
        s2 = ((halves - m) ** 2).sum(axis=0) / LD(h - 1)
        W = s2.mean(axis=0)
        mbar = np.where(frozen, x[0, 0], m.mean(axis=0)) if nok else m.mean(axis=0)
        B = h * ((m - mbar) ** 2).sum(axis=0) / LD(2 * nok - 1)
        rhat = np.sqrt((LD(h - 1) / h * W + B / h) / W)
        rhat = np.where(W == 0, np.nan, rhat)
        xc = x - np.where(konst, x[0], x.mean(axis=0))
        series = x.sum(axis=1) / LD(nok)                                      # [T, d]
        sc = series - np.where((series == series[0]).all(axis=0), series[0], series.mean(axis=0))
        if full_acf:
            cw, cm = acov(xc, L), acov(sc, L)                                 # [L + 1, nok, d], [L + 1, d]
        else:
            cw = np.stack([acov(xc[:, :, k], L, c) for k in range(d)], axis=2)
            cm = np.stack([acov(sc[:, k:k + 1], L, c)[:, 0] for k in range(d)], axis=1)
    out["mean"], out["var"], out["rhat"] = mean.astype(float), np.asarray(var).astype(float), rhat.astype(float)
    for k in range(d):
        live = cw[0, :, k] != 0                                               # (a NaN is not 0: it stays in)
        nused = int(live.sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            rho = (cw[:, live, k] / cw[0, live, k]).sum(axis=1) / LD(nused)
            rho_m = cm[:, k] / cm[0, k] if cm[0, k] != 0 else np.full(L + 1, np.nan, dtype=LD)
        tau, M, reached, margin = sokal_window(rho, c)
        tau_m, M_m, reached_m, margin_m = sokal_window(rho_m, c)
        out["acf"][k] = rho.astype(float)
        out["tau"][k], out["M"][k], out["margin"][k] = tau, M, margin
        out["tau_mean"][k], out["M_mean"][k], out["margin_mean"][k] = tau_m, M_m, margin_m
        out["nused"][k] = nused
        out["flags"][k] = int(reached) | (int(reached_m) << 1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["ess"][k] = float(LD(nok) * T / LD(tau))
    return out


def check_lag(T, c, factor):
    """The lag of a convergence check over T kept steps: min(T - 1, ceil(c T / factor) + 1)."""
    return int(min(T - 1, math.ceil(c * T / factor) + 1))


def check_verdict(T, tau, tau_prev, reached, nused, factor, rtol):
    """(ok, margin): whether a check with T kept steps converges -- every live coordinate (nused > 0) has its window reached,
    T >= factor tau and |tau - tau_prev| <= rtol tau (tau_prev None: the first check, never) -- and the smallest relative
    distance of those comparisons from their thresholds over the live coordinates (inf where none was made)."""
    ok, margin = tau_prev is not None, np.inf
    for k in range(len(tau)):
        if nused[k] <= 0:
            continue
        if not reached[k] or not np.isfinite(tau[k]):
            ok = False
            continue
        margin = min(margin, abs(T - factor * tau[k]) / (factor * tau[k]))
        good = T >= factor * tau[k]
        if tau_prev is not None:
            margin = min(margin, abs(abs(tau[k] - tau_prev[k]) - rtol * tau[k]) / max(rtol * tau[k], 1e-300))
            good = good and abs(tau[k] - tau_prev[k]) <= rtol * tau[k]
        ok = ok and good
    return ok, margin


def converge_rule(Ts, tau_hist, reached, nused, factor, rtol):
    """The index of the first check that stops the run (None: none does) and the smallest margin of the checks up to it; check j
    (from 0) has Ts[j] kept steps, tau_hist[j], reached[j], nused[j] [d]."""
    margin = np.inf
    for j in range(len(Ts)):
        ok, mg = check_verdict(Ts[j], tau_hist[j], tau_hist[j - 1] if j else None, reached[j], nused[j], factor, rtol)
        margin = min(margin, mg)
        if ok:
            return j, margin
    return None, margin


def ar1(T, n, d, phi, seed=1):
    """AR(1) chains x_t = phi x_{t-1} + sqrt(1 - phi^2) eps, stationary from t = 0, mapped to 0.5 + 0.1 x: [T, n, d]."""
    rng = np.random.default_rng(seed)
    eps = rng.standard_normal((T, n, d))
    x = np.empty((T, n, d))
    x[0] = eps[0]
    for t in range(1, T):
        x[t] = phi * x[t - 1] + math.sqrt(1.0 - phi * phi) * eps[t]
    return 0.5 + 0.1 * x
