// Device side of Hamiltonian Monte Carlo (mcalf_hmc_batch), for gfx950: n independent walkers in the unit cube, each making
// trajectories of nleap leapfrog steps with a diagonal mass, reflected at the cube's walls.  The likelihood and its gradient are
// the gradient launch's (grad_kernels.hip, issued by host_hmc.cpp between two kernels of a trajectory); what lives here is the
// momentum draw, the integrator, the accept rule, the book-keeping of dead trajectories and the chain.
//
//   ONE wave64 per walker, lane k owns coordinates k, k + 64, ... (any ndim); no LDS.  Whether a trajectory dies folds every
//   turn of the lane's loop and is made wave-uniform by a ballot.  The scalars of a walker (its decision words, the step size,
//   ln zeta) are computed by every lane alike; the momentum of coordinate k is drawn by the lane that owns it.
// The words of walker id w in global iteration g are Philox4x64-10 blocks under key (seed, 4): the decision block at counter
// (g + 1, 2^63, w, 0), the momentum blocks of coordinate k at (g + 1, (attempt << 32) | k, w, 0).  They depend on nothing else, so
// a walker's results depend on its start, its id and the options alone.
// Every product, quotient, sum, difference and square root of the sequence (include/mcalf_hip.h) is a separately rounded IEEE
// operation: contraction to FMA is switched off for this whole file (as in ens_kernels.hip), so that numpy restates a run exactly
// (tests/hmc_reference.py).  No atomics: a wave touches its own walker's rows alone.
// A frozen coordinate (the ncomp slot, hi == lo, scale == 0) has momentum 0 and is never kicked, drifted or tested: y_k = x_k.
// A trajectory that has died, and a walker of status -1, keep the walker's own point and its theta in their Y and TH rows: the
// launches that follow evaluate it and nothing reads what they leave.
#include <hip/hip_runtime.h>

#include "hmc_args.h"

#pragma clang fp contract(off)

#include "ens_ln.h"
#include "prior_device.h"
#include "wave_row.h"

using namespace mcalf;

namespace {

// Neither a NaN nor an infinity: the exponent field is not all ones.
__device__ __forceinline__ bool finite(double v) { return (__double_as_longlong(v) & 0x7ff0000000000000LL) != 0x7ff0000000000000LL; }

__device__ __forceinline__ bool frozen(const HmcArgs& a, int k) {
    return k == a.slot || a.prior.hi[k] == a.prior.lo[k] || a.scale[k] == 0.0;
}

// theta_k of the cube value v: the two operations of the cube transform, and its truncation of the ncomp slot.
__device__ __forceinline__ double to_theta(const HmcArgs& a, int k, double v) {
    const double lo = a.prior.lo[k];
    const double scaled = v * (a.prior.hi[k] - lo);
    const double th = scaled + lo;
    return a.prior_int && k == a.slot ? trunc(th) : th;
}

// g_k, the derivative of the target along cube coordinate k, from the launch's G_k at theta_k.
__device__ __forceinline__ double cube_grad(const HmcArgs& a, int k, double G, double th) {
    const double s = a.prior.hi[k] - a.prior.lo[k];
    double g = s * G;
    if (a.prior.mu) {
        const double sg = a.prior.sigma[k];
        if (sg > 0.0) {
            const double d = (th - a.prior.mu[k]) / sg;
            const double t = d / sg;
            const double ts = t * s;
            g = g - ts;
        }
    }
    return g;
}

// 1 if what the launch left for row w kills the trajectory: logL not finite, or an unfrozen g_k not finite.  Wave-uniform.
__device__ __forceinline__ bool launch_kills(const HmcArgs& a, int w, int lane) {
    const size_t o = (size_t)w * a.ndim;
    int bad = finite(a.LY[w]) ? 0 : 1;
    for (int k = lane; k < a.ndim; k += kHmcWave)
        if (!frozen(a, k)) bad |= finite(cube_grad(a, k, a.GY[o + k], a.TH[o + k])) ? 0 : 1;
    return __any(bad);
}

// The walker's own point into its trajectory rows, and the flag that says so.
__device__ __forceinline__ void park(const HmcArgs& a, int w, int lane) {
    const size_t o = (size_t)w * a.ndim;
    for (int k = lane; k < a.ndim; k += kHmcWave) {
        const double v = a.U[o + k];
        a.Y[o + k] = v;
        a.TH[o + k] = to_theta(a, k, v);
    }
    if (lane == 0) a.dead[w] = 1;
}

// The step size of walker id `id` in this iteration, and zeta of its accept rule.
__device__ __forceinline__ double step_size(const HmcArgs& a, uint64_t id, double* zeta) {
    uint64_t wd[4];
    philox4x64_10(a.iter + 1, kHmcDecision, id, a.seed, kHmcKey, wd);
    const double xi = (double)(wd[1] >> 11) * 0x1.0p-53;
    *zeta = (double)((wd[2] >> 11) + 1) * 0x1.0p-53;
    const double two_xi = 2.0 * xi;
    const double c = two_xi - 1.0;
    const double jc = a.jitter * c;
    const double f = 1.0 + jc;
    return a.eps * f;
}

// A standard normal for coordinate k by Marsaglia's polar method: the first of up to 32 candidate pairs inside the unit disc.
__device__ __forceinline__ double polar_normal(const HmcArgs& a, uint64_t id, int k) {
    for (int att = 0; att < kHmcAttempts; ++att) {
        uint64_t wd[4];
        philox4x64_10(a.iter + 1, ((uint64_t)att << 32) | (uint64_t)k, id, a.seed, kHmcKey, wd);
        for (int p = 0; p < 4; p += 2) {
            const double x1 = (double)(wd[p] >> 11) * 0x1.0p-53, x2 = (double)(wd[p + 1] >> 11) * 0x1.0p-53;
            const double t1 = 2.0 * x1, t2 = 2.0 * x2;
            const double v1 = t1 - 1.0, v2 = t2 - 1.0;
            const double q1 = v1 * v1, q2 = v2 * v2;
            const double q = q1 + q2;
            if (q > 0.0 && q < 1.0) {
                const double num = -2.0 * ens_ln(q);
                const double ratio = num / q;
                return v1 * __dsqrt_rn(ratio);
            }
        }
    }
    return 0.0;
}

// The drift of coordinate k and its one reflection: y and r are updated, 1 comes back if y is still outside (or a NaN).
__device__ __forceinline__ int drift(double ak, double& y, double& r) {
    const double step = ak * r;
    y = y + step;
    if (y < 0.0) { y = -y; r = -r; }
    else if (y > 1.0) { y = 2.0 - y; r = -r; }
    return outside_unit(y);
}

}  // namespace

// Behind the gradient launch over theta(U0), which left logL in L and the gradient rows in GY (TH holds theta(U0)).
__global__ __launch_bounds__(kHmcWave) void mcalf_hmc_start_kernel(const HmcArgs a) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)w * a.ndim;
    int bad = finite(a.L[w]) ? 0 : 1;
    for (int k = lane; k < a.ndim; k += kHmcWave) {
        const double v = a.U0[o + k];
        a.U[o + k] = v;
        bad |= outside_unit(v);
        const double g = cube_grad(a, k, a.GY[o + k], a.TH[o + k]);
        a.G[o + k] = g;
        if (!frozen(a, k)) bad |= finite(g) ? 0 : 1;
    }
    const bool refused = __any(bad);
    const double pr = a.prior.mu ? row_lnprior(a.prior, a.U0 + o, 1) : 0.0;
    if (lane != 0) return;
    a.aux[a.n + w] = pr;
    a.status[w] = refused ? kHmcBadStart : kHmcOk;
    a.naccept[w] = 0;
    a.ndead[w] = 0;
}

// The start of a trajectory: the momenta, K0, the first half kick and the first drift.
__global__ __launch_bounds__(kHmcWave) void mcalf_hmc_draw_kernel(const HmcArgs a) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)w * a.ndim;
    if (__builtin_amdgcn_readfirstlane(a.status[w]) != kHmcOk) { park(a, w, lane); return; }
    const uint64_t id = a.wid ? a.wid[w] : (uint64_t)w;
    double zeta;
    const double eps = step_size(a, id, &zeta);
    double acc = 0.0;
    int out = 0;
    for (int k = lane; k < a.ndim; k += kHmcWave) {
        double y = a.U[o + k], r = 0.0;
        if (!frozen(a, k)) {
            r = polar_normal(a, id, k);
            const double rr = r * r;
            acc = acc + rr;
            const double ak = eps * a.scale[k];
            const double hk = 0.5 * ak;
            const double kick = hk * a.G[o + k];
            r = r + kick;
            out |= drift(ak, y, r);
        }
        a.R[o + k] = r;
        a.Y[o + k] = y;
        a.TH[o + k] = to_theta(a, k, y);
    }
    const double k0 = 0.5 * uniform(wave_sum(acc));
    if (__any(out)) { park(a, w, lane); }                      // (every lane reads back the entries it wrote itself)
    else if (lane == 0) a.dead[w] = 0;
    if (lane == 0) a.aux[w] = k0;
}

// Between two leapfrog steps: the half kick that ends the step whose launch has just finished, the half kick that begins the
// next one -- two additions, not one -- and its drift.
__global__ __launch_bounds__(kHmcWave) void mcalf_hmc_step_kernel(const HmcArgs a) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)w * a.ndim;
    if (__builtin_amdgcn_readfirstlane(a.dead[w])) return;     // (its rows hold the walker's own point already)
    if (launch_kills(a, w, lane)) { park(a, w, lane); return; }
    const uint64_t id = a.wid ? a.wid[w] : (uint64_t)w;
    double zeta;
    const double eps = step_size(a, id, &zeta);
    int out = 0;
    for (int k = lane; k < a.ndim; k += kHmcWave) {
        if (frozen(a, k)) continue;
        const double gy = cube_grad(a, k, a.GY[o + k], a.TH[o + k]);
        double y = a.Y[o + k], r = a.R[o + k];
        const double ak = eps * a.scale[k];
        const double hk = 0.5 * ak;
        const double kick = hk * gy;
        r = r + kick;
        r = r + kick;
        out |= drift(ak, y, r);
        a.R[o + k] = r;
        a.Y[o + k] = y;
        a.TH[o + k] = to_theta(a, k, y);
    }
    if (__any(out)) park(a, w, lane);
}

// Behind a trajectory's last launch: the last half kick, K1 and the accept rule; then the chain slot.
__global__ __launch_bounds__(kHmcWave) void mcalf_hmc_decide_kernel(const HmcArgs a) {
    const int w = blockIdx.x, lane = threadIdx.x;
    const size_t o = (size_t)w * a.ndim;
    const bool moves = __builtin_amdgcn_readfirstlane(a.status[w]) == kHmcOk;
    bool dead = moves && __builtin_amdgcn_readfirstlane(a.dead[w]);
    if (moves && !dead) dead = launch_kills(a, w, lane);
    if (moves && !dead) {
        const uint64_t id = a.wid ? a.wid[w] : (uint64_t)w;
        double zeta;
        const double eps = step_size(a, id, &zeta);
        double acc = 0.0;
        for (int k = lane; k < a.ndim; k += kHmcWave) {
            if (frozen(a, k)) continue;
            const double gy = cube_grad(a, k, a.GY[o + k], a.TH[o + k]);
            const double ak = eps * a.scale[k];
            const double hk = 0.5 * ak;
            const double kick = hk * gy;
            const double r = a.R[o + k] + kick;
            const double rr = r * r;
            acc = acc + rr;
        }
        const double k1 = 0.5 * uniform(wave_sum(acc));
        const double py = a.prior.mu ? row_lnprior(a.prior, a.Y + o, 1) : 0.0;
        const double ly = a.LY[w];
        const double ty = ly + py;
        const double tx = a.L[w] + a.aux[a.n + w];
        const double dt = ty - tx;
        const double dk = a.aux[w] - k1;
        const double q = dt + dk;
        if (ens_ln(zeta) < q) {                                // (any NaN: false)
            for (int k = lane; k < a.ndim; k += kHmcWave) {
                a.U[o + k] = a.Y[o + k];
                a.G[o + k] = cube_grad(a, k, a.GY[o + k], a.TH[o + k]);
            }
            if (lane == 0) {
                a.L[w] = ly;
                a.aux[a.n + w] = py;
                a.naccept[w] += 1;
            }
        }
    }
    if (dead && lane == 0) a.ndead[w] += 1;
    // The state after the iteration: what this wave wrote of its walker above is read back by the lane that wrote it.
    if (a.CU)
        for (int k = lane; k < a.ndim; k += kHmcWave) a.CU[o + k] = a.U[o + k];
    if (a.CL && lane == 0) a.CL[w] = a.L[w];
}

__global__ __launch_bounds__(kHmcPut) void mcalf_hmc_put_kernel(const HmcPutArgs p) {
    const int i = threadIdx.x;
    if (i < p.count) p.dst[i] = p.v[i];
}

namespace mcalf {
const void* hmc_kernel_ptr(HmcKernel k) {
    static const void* const table[] = {(const void*)&mcalf_hmc_start_kernel, (const void*)&mcalf_hmc_draw_kernel, (const void*)&mcalf_hmc_step_kernel,
                                        (const void*)&mcalf_hmc_decide_kernel, (const void*)&mcalf_hmc_put_kernel};   // in the order of enum HmcKernel
    static_assert(sizeof(table) / sizeof(table[0]) == kHmcKernelCount, "one entry per HmcKernel");
    return table[k];
}
}  // namespace mcalf
