// The evidence arithmetic of a nested-sampling run: what nested.py's `die` and the tail of its `nested_sample` compute, restated
// for the library's own run (host_nsrun.cpp).  Pure C++ with no HIP, so that the CPU tests drive it from a stand-alone program
// (tests/stubs/ns_evidence_check.cpp).
//
// A block of `count` points, sorted by key, dies at live counts n_first, n_first - 1, ...: point i at n_i = n_first - i has
//   ln w_i = ln X_i + ln(-expm1(-1 / n_i)) + key_i,   ln X_i = ln X + (c_0 + ... + c_{i-1}),  c_i = -1 / n_i  (a running sum),
// ln X drops to ln X + (c_0 + ... + c_{count-1}) and the running ln Z takes logaddexp of the block's weights folded from the
// left.  key = logL with NaN as -inf: such a point carries no weight.  A run is `rounds` blocks of K points at n_first = nlive
// and a last block of the nlive remaining points at nlive ... 1; its ln Z is ONE left fold over all weights (the running value
// only steers the stop), H = sum of p_i (key_i - ln Z) over the p_i = exp(ln w_i - ln Z) > 0.
// Not part of the kernel-source hash (mc-alf_amd/build.py).
#pragma once
#include <cmath>
#include <cstdint>
#include <limits>

namespace mcalf {

inline double ns_key(double logl) { return logl != logl ? -std::numeric_limits<double>::infinity() : logl; }

// numpy's logaddexp: equal arguments (both -inf included) give x + ln 2.
inline double ns_logaddexp(double x, double y) {
    if (x == y) return x + 0.693147180559945309417232121458176568;
    const double d = x - y;
    if (d > 0.0) return x + std::log1p(std::exp(-d));
    if (d <= 0.0) return y + std::log1p(std::exp(d));
    return x + y;                                               // (a NaN among them)
}

struct NsEvidence {
    double logX = 0.0;
    double logZ = -std::numeric_limits<double>::infinity();     // the running value

    // `count` points with logL `logl`, in death order, dying from live count n_first down; lw (NULL: not wanted) takes their
    // unnormalised log weights.
    void die(const double* logl, int64_t count, int64_t n_first, double* lw) {
        double csum = 0.0, block = 0.0;
        for (int64_t i = 0; i < count; ++i) {
            const double n = (double)(n_first - i);
            const double w = (logX + csum) + std::log(-std::expm1(-1.0 / n)) + ns_key(logl[i]);
            csum = i == 0 ? -1.0 / n : csum + -1.0 / n;
            block = i == 0 ? w : ns_logaddexp(block, w);
            if (lw) lw[i] = w;
        }
        if (count > 0) {
            logX = logX + csum;
            logZ = ns_logaddexp(logZ, block);
        }
    }

    // The stop test before a round: the largest live key times the remaining volume against dlogz of the evidence so far.
    bool converged(double max_key, double dlogz) const {
        return logZ > -std::numeric_limits<double>::infinity() && max_key + logX < std::log(dlogz) + logZ;
    }
};

// The whole run over its `ndead` dead logL (rounds of K, then the last nlive; ndead = rounds K + nlive): the normalised log
// weights into logw [ndead], ln Z and H.
inline void ns_finish(const double* logl, int64_t ndead, int64_t nlive, int64_t K, double* logw, double* logZ, double* H) {
    NsEvidence ev;
    const int64_t rounds = (ndead - nlive) / K;
    for (int64_t r = 0; r < rounds; ++r) ev.die(logl + r * K, K, nlive, logw + r * K);
    ev.die(logl + rounds * K, nlive, nlive, logw + rounds * K);
    double z = ndead > 0 ? logw[0] : -std::numeric_limits<double>::infinity();
    for (int64_t i = 1; i < ndead; ++i) z = ns_logaddexp(z, logw[i]);
    double h = 0.0;
    for (int64_t i = 0; i < ndead; ++i) {
        logw[i] = logw[i] - z;
        const double p = std::exp(logw[i]);
        if (p > 0.0) h += p * (ns_key(logl[i]) - z);
    }
    *logZ = z;
    *H = h;
}

}  // namespace mcalf
