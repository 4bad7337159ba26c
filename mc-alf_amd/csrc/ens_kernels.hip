// Device side of the ensemble sampler (mcalf_ensemble_batch) and of its tempered form (mcalf_tempered_batch), for gfx950:
// T temperatures of n walkers in the unit cube, each cut into the halves [0, m) and [m, n), moved by the affine-invariant
// stretch move or by the differential-evolution move with partners from the half of the same temperature that stands still,
// and exchanged between neighbouring temperatures in swap rounds.  mcalf_ensemble_batch is T = 1 with beta = 1, where beta d
// is d bit for bit.  The likelihood is the cube logL launch's (kernels.hip, issued by host_ens.cpp between the propose and the
// decide kernel of a half-step); what lives here is the proposal, the accept rule, the swap and the chain.
//
//   ONE wave64 per walker, lane k owns coordinates k, k + 64, ... (any ndim).  The inside-the-cube test folds every turn of the
//   lane's loop and is made wave-uniform by a ballot.  The scalars of a walker (its random words, z or gamma, ln z, ln zeta)
//   are computed by every lane alike.
// The random words of moving walker w of temperature t in global half-step s are the block numpy's
// Philox(counter=[s, 0, t n + w, 0], key=[seed, 1]) returns first: that generator advances its counter before it draws, so the
// block is Philox4x64-10 at (s + 1, 0, t n + w, 0) -- as the slice step's word block of step 1 is the first one of
// Philox(counter=[0, 0, sid, 0]).  A swap round r draws under key [seed, 2]: the shift of pair t at counter [r, 1, t, 0], zeta
// of position (t, w) at [r, 0, t n + w, 0].  The words depend on nothing else, so a walker's results depend on the starts and
// the options alone.
// Every product, quotient, sum and difference of the proposal, of ens_ln and of the accept rules is a separately rounded IEEE
// operation: contraction to FMA is switched off for this whole file (as in ns_kernels.hip), so that numpy restates a run exactly
// (tests/ens_reference.py, tests/pt_reference.py).  No atomics: a swap round's exchanges are disjoint pairs of rows.
// Under a Gaussian prior (mcalf_set_gauss_prior; a.prior.mu != NULL) L, CL and the temperature stay the likelihood's; PR [T n]
// holds lnprior of the walkers (row_lnprior of prior_device.h: the start kernel fills it, the propose kernel hands an inside
// trial's value over through aux[2], a swap exchanges it with L), and the accept rule is q + (py - px).  Without one no kernel
// reads or writes PR or aux[2].
#include <hip/hip_runtime.h>

#include "ens_args.h"

#pragma clang fp contract(off)

#include "ens_ln.h"
#include "prior_device.h"
#include "wave_row.h"

using namespace mcalf;

__global__ __launch_bounds__(kEnsWave) void mcalf_ens_start_kernel(const EnsArgs a) {
    const int w = blockIdx.x, lane = threadIdx.x;              // (a row of the T n)
    const size_t o = (size_t)w * a.ndim;
    int bad = 0;
    for (int k = lane; k < a.ndim; k += kEnsWave) {
        const double v = a.U0[o + k];
        a.U[o + k] = v;
        bad |= outside_unit(v);
    }
    const bool outside = __any(bad);
    const double pr = a.prior.mu ? row_lnprior(a.prior, a.U0 + o, 1) : 0.0;
    if (lane != 0) return;
    if (a.prior.mu) a.PR[w] = pr;
    a.status[w] = outside ? kEnsBadStart : kEnsOk;
    a.naccept[w] = 0;
    if (w < (a.ntemps - 1) * a.n) a.nswap[w] = 0;
}

__global__ __launch_bounds__(kEnsWave) void mcalf_ens_propose_kernel(const EnsArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int t = b / a.m, base = t * a.n;                     // the temperature; its first row
    const int w = base + a.half * a.m + (b - t * a.m), other = base + (1 - a.half) * a.m;
    const double* x = a.U + (size_t)w * a.ndim;
    double* y = a.Y + (size_t)b * a.ndim;
    const bool moves = __builtin_amdgcn_readfirstlane(a.status[w]) == kEnsOk;
    uint64_t wd[4];
    philox4x64_10(a.step + 1, (uint64_t)w, a.seed, kEnsKey1, wd);      // (numpy's generator draws at counter + 1)
    const uint64_t m = (uint64_t)a.m;
    const double xi = (double)(wd[1] >> 11) * 0x1.0p-53;
    const double zeta = (double)((wd[2] >> 11) + 1) * 0x1.0p-53;
    double hastings = 0.0;
    int out = 0;
    if (!moves) {
        out = 1;
    } else if (a.move == kEnsStretch) {
        const double* xj = a.U + (size_t)(other + (int)(wd[0] % m)) * a.ndim;
        const double t1 = (a.scale - 1.0) * xi + 1.0;
        const double z = (t1 * t1) / a.scale;
        hastings = (double)(a.ndim - 1) * ens_ln(z);
        for (int k = lane; k < a.ndim; k += kEnsWave) {
            const double pj = xj[k];
            const double v = pj + z * (x[k] - pj);
            y[k] = v;
            out |= outside_unit(v);
        }
    } else {
        const uint64_t j1 = wd[0] % m, j2 = (j1 + 1 + wd[3] % (m - 1)) % m;
        const double* x1 = a.U + (size_t)(other + (int)j1) * a.ndim;
        const double* x2 = a.U + (size_t)(other + (int)j2) * a.ndim;
        const double gamma = a.scale * (1.0 + 1e-5 * (2.0 * xi - 1.0));
        for (int k = lane; k < a.ndim; k += kEnsWave) {
            const double v = x[k] + gamma * (x1[k] - x2[k]);
            y[k] = v;
            out |= outside_unit(v);
        }
    }
    const bool outside = __any(out);
    if (outside)                                               // the trial row is the walker's own point, as a finished slice row's
        for (int k = lane; k < a.ndim; k += kEnsWave) y[k] = x[k];
    // lnprior of an inside trial, while the wave has y: every lane reads back the entries it wrote itself
    const double py = a.prior.mu && !outside ? row_lnprior(a.prior, y, 1) : 0.0;
    if (lane != 0) return;
    if (a.prior.mu && !outside) a.aux[2 * (size_t)a.ntemps * a.m + b] = py;
    a.aux[b] = hastings;
    a.aux[(size_t)a.ntemps * a.m + b] = ens_ln(zeta);
    a.inside[b] = outside ? 0 : 1;
}

__global__ __launch_bounds__(kEnsWave) void mcalf_ens_decide_kernel(const EnsArgs a) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const int t = b / a.m, base = t * a.n, bl = b - t * a.m;
    const int w = base + a.half * a.m + bl;
    double* x = a.U + (size_t)w * a.ndim;
    if (__builtin_amdgcn_readfirstlane(a.inside[b])) {
        const double* y = a.Y + (size_t)b * a.ndim;
        const double ly = a.LY[b], lx = a.L[w];
        const double d = a.beta[t] * (ly - lx);                // (beta 0 and a trial of -inf: NaN, rejected)
        double q = a.move == kEnsStretch ? a.aux[b] + d : d;
        double py = 0.0;
        if (a.prior.mu) {                                      // the prior's ratio, untempered: (aux + beta d) + (py - px)
            py = a.aux[2 * (size_t)a.ntemps * a.m + b];
            q = q + (py - a.PR[w]);
        }
        if (a.aux[(size_t)a.ntemps * a.m + b] < q) {           // (any NaN: false)
            for (int k = lane; k < a.ndim; k += kEnsWave) x[k] = y[k];
            if (lane == 0) {
                a.L[w] = ly;
                if (a.prior.mu) a.PR[w] = py;
                a.naccept[w] += 1;
            }
        }
    }
    if (!a.keep) return;
    // The state after the iteration (half 1 has just decided): walker bl stood still in this half-step, and what this wave wrote
    // of walker m + bl above is read back by the lane that wrote it.
    for (int r = 0; r < 2; ++r) {
        const int v = base + r * a.m + bl;
        if (a.CU && t < a.chain_temps) {
            const double* src = a.U + (size_t)v * a.ndim;
            double* dst = a.CU + (size_t)v * a.ndim;
            for (int k = lane; k < a.ndim; k += kEnsWave) dst[k] = src[k];
        }
        if (a.CL && lane == 0) a.CL[v] = a.L[v];
    }
}

// One exchange of swap round a.round: block p n + w is position (t, w), t = pair0 + 2 p, against position (t + 1, j).  The map
// w -> j is a shift, so no row is in two exchanges and no two waves touch the same row.
__global__ __launch_bounds__(kEnsWave) void mcalf_ens_swap_kernel(const EnsArgs a) {
    const int blk = blockIdx.x, lane = threadIdx.x;
    const int p = blk / a.n, w = blk - p * a.n, t = a.pair0 + 2 * p;
    const uint64_t n = (uint64_t)a.n;
    uint64_t wd[4];
    philox4x64_10(a.round + 1, 1, (uint64_t)t, a.seed, kEnsKey2, wd);
    const int j = (int)(((uint64_t)w + wd[0] % n) % n);
    const size_t lo = (size_t)t * a.n + w, hi = (size_t)(t + 1) * a.n + j;
    philox4x64_10(a.round + 1, 0, (uint64_t)lo, a.seed, kEnsKey2, wd);
    const double zeta = (double)((wd[2] >> 11) + 1) * 0x1.0p-53;
    const bool both = a.status[lo] == kEnsOk && a.status[hi] == kEnsOk;
    const double ll = a.L[lo], lh = a.L[hi];
    const double q = (a.beta[t] - a.beta[t + 1]) * (lh - ll);
    if (!__builtin_amdgcn_readfirstlane(both && ens_ln(zeta) < q ? 1 : 0)) return;      // (any NaN: false)
    double* x = a.U + lo * a.ndim;
    double* y = a.U + hi * a.ndim;
    for (int k = lane; k < a.ndim; k += kEnsWave) {
        const double v = x[k];
        x[k] = y[k];
        y[k] = v;
    }
    if (lane != 0) return;
    a.L[lo] = lh;
    a.L[hi] = ll;
    if (a.prior.mu) {                                          // (the prior cancels in the rule above; the rows take theirs along)
        const double pl = a.PR[lo];
        a.PR[lo] = a.PR[hi];
        a.PR[hi] = pl;
    }
    a.nswap[lo] += 1;
}

namespace mcalf {
const void* ens_kernel_ptr(EnsKernel k) {
    static const void* const table[] = {(const void*)&mcalf_ens_start_kernel, (const void*)&mcalf_ens_propose_kernel,
                                        (const void*)&mcalf_ens_decide_kernel, (const void*)&mcalf_ens_swap_kernel};   // in the order of enum EnsKernel
    static_assert(sizeof(table) / sizeof(table[0]) == kEnsKernelCount, "one entry per EnsKernel");
    return table[k];
}
}  // namespace mcalf

// The chain-diagnostics kernels (mcalf_chain_stats, mcalf_ensemble_converge): one device translation unit with the sampler whose
// chain they read.  (Not a stand-alone header: it must come last, under this file's `fp contract(off)`.)
#include "chain_kernels.h"
