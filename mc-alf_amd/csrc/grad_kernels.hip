// The derivative kernels for gfx950, float64: the analytic gradient of logL (mcalf_loglike_grad_batch), the model Jacobian's
// products with a vector (mcalf_model_jvp_batch / _vjp_batch) and the product of logL's exact Hessian with a vector
// (mcalf_loglike_hvp_batch).  host_grad.cpp holds the kernel sequence of each product.
//
// With w = 1/err^2, m = cont L(F), F = exp(-sum tau) and q_i = w_i (d_i - m_i) (0 on the pixels nansum drops):
//     dlogL/dtheta = sum_i q_i dm_i/dtheta
//     cont : sum_i q_i L(F)_i                 R : sum_i q_i cont (dL/dR)(F)_i      (dw_k/dsigma = w_k (k^2 - sum_j w_j j^2) / sigma^3)
//     N, z, b of a component : sum_i g_i dtau_i/dtheta,   g = -F cont L^T q
// L is the context's convolution: the periodic one with the astropy tap count on the numpy path (none when R <= velstep),
// the fixed grid with the edge reset on the JAX path; L^T is its transpose.  Per (component, line), K = cne/dnu:
//     dtau/dN = ln10 tau,   dtau/dz = K H_u (c/lambda)/dnu,   dtau/db = -(K/b)(H + u H_u + a H_a)
// J v (JVP), J = dm/dtheta: dtau = sum_c (ln10 tau_c v_N + K H_u (nu/dnu) v_z - (K/b) e v_b), T = -F dtau,
//     dM = cont L(T) + v_cont L(F) + v_R cont (dL/dR)(F).
// J^T q (VJP): the gradient with the caller's cotangent in place of w (d - m) (the q pointer IS the caller's array) and no
//     logL, so no veto rule: only rows whose tap count exceeds the cap are NaN.
// H v (HVP): see the comment above the hvp kernels.
//
// What every kernel shares, each written once:
//   lsf_forward<kWhat>   one walk over a pixel's taps: L F, (dL/dR) F, (d2L/dR2) F, L T, (dL/dR) T as the template asks;
//                        the JAX edge reset, the periodic wrap with the division by bot, the pass-through of a row without taps
//   lsf_transposed<kTan> the same for L^T q, (dL/dR)^T q, L^T dq
//   comp_of, line_sums, zero_inactive   a row's active targets, then its fillers: (slot0, nl, col); the first-order sums of one
//   reduce_cont_R        the continuum / R / ncomp cells of a tile's partials
//   tap_m2, tap_centre   sum_k w_k (k - n)^2 and c_k = (k - n)^2 - that
// Every sum keeps ONE order (no atomics), so a row's bits do not depend on its batch, its pass or its device: each
// accumulator of a walk is its own sequential sum over k, acc += taps[k] * f, divided by bot after the loop; block_sum /
// block_sum3 are a fixed LDS tree; finalize sums the tiles in order.  The convolutions read the workspace in HBM, so any LSF
// width the likelihood accepts works.
#include <hip/hip_runtime.h>

#include "grad_args.h"
#include "voigt_grad.h"

using namespace mcalf;

namespace {

constexpr double kLn10 = 2.302585092994045684;

struct RowInfo { double R, cont; int n, nc; bool bad; double bot; };

__device__ __forceinline__ RowInfo row_info(const GradArgs& a, int r) {
    const double* w = a.rows + (size_t)r * kGradRow;
    RowInfo o;
    o.R = w[0]; o.cont = w[1]; o.n = (int)w[2]; o.nc = (int)w[3]; o.bad = w[4] != 0.0; o.bot = w[5];
    return o;
}

// Sum of v over the workgroup (kGradBlock threads), the same tree every time; every thread gets the result.
__device__ __forceinline__ double block_sum(double v, double* lds) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = kGradBlock / 2; s > 0; s >>= 1) {
        if (t < s) lds[t] += lds[t + s];
        __syncthreads();
    }
    return lds[0];
}

// Three sums at once (lds: 3 * kGradBlock doubles); the result is valid in thread 0.
__device__ __forceinline__ void block_sum3(double& x, double& y, double& z, double* lds) {
    const int t = threadIdx.x;
    __syncthreads();
    lds[t] = x; lds[kGradBlock + t] = y; lds[2 * kGradBlock + t] = z;
    __syncthreads();
#pragma unroll
    for (int s = kGradBlock / 2; s > 0; s >>= 1) {
        if (t < s) {
            lds[t] += lds[t + s];
            lds[kGradBlock + t] += lds[kGradBlock + t + s];
            lds[2 * kGradBlock + t] += lds[2 * kGradBlock + t + s];
        }
        __syncthreads();
    }
    x = lds[0]; y = lds[kGradBlock]; z = lds[2 * kGradBlock];
}

// ---- the LSF walks ----

// The sums a forward walk carries besides L F; the others stay 0 and cost nothing (kWhat is a template argument).
enum : unsigned { kLsfR = 1, kLsfRR = 2, kLsfT = 4, kLsfRT = 8 };          // (dL/dR) F, (d2L/dR2) F, L T, (dL/dR) T
struct Lsf { double cF, rF, rrF, cT, rT; };

// The context's convolution at pixel i of row r, applied to F (a.F) and, with kLsfT, to T (a.q).
template <unsigned kWhat>
__device__ __forceinline__ Lsf lsf_forward(const GradArgs& a, const RowInfo& ri, int r, int i) {
    const double* F = a.F + (size_t)r * a.npix;
    const double* T = a.q + (size_t)r * a.npix;
    const double* taps = a.taps + (size_t)r * a.tapcap;
    const double* dtaps = a.dtaps + (size_t)r * a.tapcap;
    const double* ddtaps = (kWhat & kLsfRR) ? a.ddtaps + (size_t)r * a.tapcap : nullptr;   // (no such workspace outside the HVP)
    Lsf s = {0.0, 0.0, 0.0, 0.0, 0.0};
    auto tap = [&](int k, int j) {                                             // tap k reads pixel j
        const double f = F[j];
        s.cF += taps[k] * f;
        if (kWhat & kLsfR) s.rF += dtaps[k] * f;
        if (kWhat & kLsfRR) s.rrF += ddtaps[k] * f;
        if (kWhat & kLsfT) {
            const double tt = T[j];
            s.cT += taps[k] * tt;
            if (kWhat & kLsfRT) s.rT += dtaps[k] * tt;
        }
    };
    const int h = ri.n;
    if (a.lay.jax ? (i < h || i >= a.npix - h) : h == 0) {                         // :677-681 edge reset; R <= velstep: no convolution (:445)
        s.cF = F[i];
        if (kWhat & kLsfT) s.cT = T[i];
    } else if (a.lay.jax) {
        for (int k = 0; k <= 2 * h; ++k) tap(k, i + k - h);
    } else {
        int j = (int)(((long)i - h) % a.npix);
        if (j < 0) j += a.npix;
        for (int k = 0; k <= 2 * h; ++k) {                                     // periodic boundary (:463-464)
            tap(k, j);
            if (++j == a.npix) j = 0;
        }
        s.cF = s.cF / ri.bot; s.rF = s.rF / ri.bot; s.rrF = s.rrF / ri.bot; s.cT = s.cT / ri.bot; s.rT = s.rT / ri.bot;
    }
    return s;
}

// The transpose at pixel i: L^T q and, with kTan, (dL/dR)^T q and L^T dq.
struct LsfT { double lq, rq, ldq; };

template <bool kTan>
__device__ __forceinline__ LsfT lsf_transposed(const GradArgs& a, const RowInfo& ri, int r, int i, const double* q, const double* dq) {
    const double* taps = a.taps + (size_t)r * a.tapcap;
    const double* dtaps = a.dtaps + (size_t)r * a.tapcap;
    LsfT s = {0.0, 0.0, 0.0};
    auto tap = [&](int k, int o) {                                             // output o read pixel i through tap k
        const double qo = q[o];
        s.lq += taps[k] * qo;
        if (kTan) {
            s.rq += dtaps[k] * qo;
            s.ldq += taps[k] * dq[o];
        }
    };
    const int h = ri.n;
    if (a.lay.jax ? (i < h || i >= a.npix - h) : h == 0) {                         // an edge pixel is its own output; no taps
        s.lq = q[i];
        if (kTan) s.ldq = dq[i];
    }
    if (a.lay.jax) {
        // interior outputs o = i - k + h with tap k read pixel i
        const int klo = max(0, i + 2 * h - a.npix + 1), khi = min(2 * h, i);
        for (int k = klo; k <= khi; ++k) tap(k, i - k + h);
    } else if (h > 0) {
        int j = (int)(((long)i + h) % a.npix);
        for (int k = 0; k <= 2 * h; ++k) {
            tap(k, j);
            if (--j < 0) j = a.npix - 1;
        }
        s.lq = s.lq / ri.bot; s.rq = s.rq / ri.bot; s.ldq = s.ldq / ri.bot;
    }
    return s;
}

// ---- the walk over a row's components ----

__device__ __forceinline__ const double* rec_of(const GradArgs& a, int r, int slot) {
    return a.recs + ((size_t)r * a.nslots + slot) * kGradRec;
}

// Component c of a row's ri.nc + a.lay.nfill: the active targets, then the fillers.  Its records are slots [slot0, slot0 + nl) of
// the record list (the ncompmax * nlines target slots, then the nfill filler slots); its (N, z, b) are columns [col, col + 3).
struct Comp { int slot0, nl, col; };

__device__ __forceinline__ Comp comp_of(const GradArgs& a, const RowInfo& ri, int c) {
    const bool fill = c >= ri.nc;
    Comp o;
    o.slot0 = fill ? a.lay.ncompmax * a.lay.nlines + (c - ri.nc) : c * a.lay.nlines;
    o.nl = fill ? 1 : a.lay.nlines;
    o.col = fill ? filler_col(a.lay, c - ri.nc) : target_col(a.lay, c);
    return o;
}

// First order, summed over a component's lines at one pixel: tau, dtau/dz, dtau/db (dtau/dN = ln10 tau).
struct LineSums { double sN, sz, sb; };

__device__ __forceinline__ LineSums line_sums(const GradArgs& a, int r, const Comp& k, double nu) {
    LineSums s = {0.0, 0.0, 0.0};
    for (int l = 0; l < k.nl; ++l) {
        const double* rec = rec_of(a, r, k.slot0 + l);
        const double u = nu * rec[0] - rec[1], y = rec[2], K = rec[3];
        double wr, wi, dr, di, e;
        faddeeva_dw(u, y, wr, wi, dr, di, e);
        s.sN += K * wr;                                     // tau
        s.sz += K * dr * (nu * rec[4]);                     // K H_u du/dz
        s.sb -= K * rec[5] * e;                             // (K/b)(H + u H_u + a H_a)
    }
    return s;
}

// Inactive components: exactly 0 (one thread of the tile).
__device__ __forceinline__ void zero_inactive(const GradArgs& a, const RowInfo& ri, double* out) {
    for (int c = ri.nc; c < a.lay.ncompmax; ++c) {
        const int col = target_col(a.lay, c);
        out[col] = out[col + 1] = out[col + 2] = 0.0;
    }
}

__device__ __forceinline__ double* part_of(const GradArgs& a, int r) {
    return a.part + ((size_t)r * a.ntiles + blockIdx.x) * a.lay.ndim;
}

// A tile's continuum and R partials summed over its pixels, and the ncomp cell.  has_R false: the R cell is exactly 0.
__device__ __forceinline__ void reduce_cont_R(const GradArgs& a, int r, double pc, double pR, bool has_R, double* lds) {
    pc = block_sum(pc, lds);
    pR = block_sum(pR, lds);
    if (threadIdx.x == 0) {
        double* out = part_of(a, r);
        if (a.lay.freespecres) out[0] = has_R ? pR : 0.0;
        if (a.lay.freecont) out[cont_col(a.lay)] = pc;
        out[a.lay.startind] = 0.0;                                                 // the ncomp slot
    }
}

// ---- tap moments ----

__device__ __forceinline__ bool no_taps(const GradArgs& a, int n) { return !a.lay.jax && n == 0; }

// sum_k w_k (k - n)^2 over the 2n + 1 taps (each thread reads the taps it wrote itself); every thread gets it.
__device__ __forceinline__ double tap_m2(const double* taps, int n, double* lds) {
    double m2 = 0.0;
    for (int k = threadIdx.x; k <= 2 * n; k += kGradBlock) {
        const double dk = (double)(k - n);
        m2 += taps[k] * dk * dk;
    }
    return block_sum(m2, lds);
}

__device__ __forceinline__ double tap_centre(int k, int n, double m2) {
    const double dk = (double)(k - n);
    return dk * dk - m2;
}

}  // namespace

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_setup_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    const int r = blockIdx.x;
    const int t = threadIdx.x;
    const double* p = a.P + (size_t)r * a.lay.ndim;
    const double R = row_resolution(a.lay, p), cont = row_continuum(a.lay, p);
    const int nc = active_components(a.lay, p[a.lay.startind]);

    const int ntarget = a.lay.ncompmax * a.lay.nlines;
    for (int slot = t; slot < a.nslots; slot += kGradBlock) {
        int q;
        const LineDev* ln;
        if (slot < ntarget) {
            const int c = slot / a.lay.nlines;
            q = target_col(a.lay, c);
            ln = a.lines + (slot - c * a.lay.nlines);
        } else {
            q = filler_col(a.lay, slot - ntarget);
            ln = a.lines + a.lay.nlines;
        }
        const double logN = p[q], z = p[q + 1], b = p[q + 2];
        const LineScale s = line_scale(z, b, *ln, pow(10.0, logN));
        double* rec = a.recs + ((size_t)r * a.nslots + slot) * kGradRec;
        rec[0] = s.A;                                                              // u = nu A - B
        rec[1] = s.B;
        rec[2] = s.a;
        rec[3] = s.K;
        rec[4] = s.rdnu;
        rec[5] = 1.0 / b;
    }

    // taps: the numpy path's astropy count (none when R <= velstep), the JAX path's fixed grid
    const double sigma = (R / kFwhmToSigma) / a.velstep;
    const LsfWidth lw = lsf_half_width(R, a.velstep, a.lay.jax, a.jax_half, a.n_cap);
    const int n = lw.n;
    const bool bad = lw.bad;
    double* taps = a.taps + (size_t)r * a.tapcap;
    double* dtaps = a.dtaps + (size_t)r * a.tapcap;
    const double inv2s2 = 0.5 / (sigma * sigma);
    double s = 0.0;
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double dk = (double)(k - n);
        s += exp(-(dk * dk) * inv2s2);
    }
    const double wsum = block_sum(s, lds);
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double dk = (double)(k - n);
        taps[k] = no_taps(a, n) ? 1.0 : exp(-(dk * dk) * inv2s2) / wsum;
    }
    const double m2 = tap_m2(taps, n, lds);
    double bs = 0.0;
    const double dsig = 1.0 / (kFwhmToSigma * a.velstep * sigma * sigma * sigma);     // dsigma/dR / sigma^3
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double w = taps[k];
        dtaps[k] = no_taps(a, n) ? 0.0 : w * tap_centre(k, n, m2) * dsig;
        bs += w;
    }
    const double bot = block_sum(bs, lds);                                         // astropy divides by the tap sum (1 to rounding)
    if (t == 0) {
        double* w = a.rows + (size_t)r * kGradRow;
        w[0] = R; w[1] = cont; w[2] = (double)n; w[3] = (double)nc; w[4] = bad ? 1.0 : 0.0; w[5] = a.lay.jax ? 1.0 : bot;
        w[6] = w[7] = 0.0;
    }
}

// tau is ONE accumulator over every slot in the walk's order; jvp_forward sums per component first.  The two associations
// differ in their bits, so neither kernel takes the other's form.
__global__ __launch_bounds__(kGradBlock) void mcalf_grad_forward_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    const double nu = a.nu[i];
    double tau = 0.0;
    for (int c = 0; c < ri.nc + a.lay.nfill; ++c) {
        const Comp k = comp_of(a, ri, c);
        for (int l = 0; l < k.nl; ++l) {
            const double* rec = rec_of(a, r, k.slot0 + l);
            double wr, wi, dr, di, e;
            faddeeva_dw(nu * rec[0] - rec[1], rec[2], wr, wi, dr, di, e);
            tau += rec[3] * wr;
        }
    }
    a.F[(size_t)r * a.npix + i] = exp(-tau);
}

// kCot: q is the caller's cotangent (a.q points at it) instead of w (d - m).
template <bool kCot>
__device__ __forceinline__ void model_tile(const GradArgs& a, double* lds) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    const RowInfo ri = row_info(a, r);
    double pc = 0.0, pR = 0.0;
    if (i < a.npix) {
        const Lsf s = lsf_forward<kLsfR>(a, ri, r, i);
        double qv;
        if (kCot) {
            qv = a.q[(size_t)r * a.npix + i];
        } else {
            const double is2 = a.ispec2[i];
            const double res = a.obj[i] - ri.cont * s.cF;
            const double term = is2 * res * res - a.lgis[i];
            qv = isnan(term) ? 0.0 : is2 * res;                                    // the pixels nansum keeps (:294)
            a.q[(size_t)r * a.npix + i] = qv;
        }
        pc = qv * s.cF;
        pR = qv * ri.cont * s.rF;
    }
    reduce_cont_R(a, r, pc, pR, true, lds);
}

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_model_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    model_tile<false>(a, lds);
}

__global__ __launch_bounds__(kGradBlock) void mcalf_vjp_model_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    model_tile<true>(a, lds);
}

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_adjoint_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    const LsfT s = lsf_transposed<false>(a, ri, r, i, a.q + (size_t)r * a.npix, nullptr);
    double* F = a.F + (size_t)r * a.npix;
    F[i] = -F[i] * ri.cont * s.lq;
}

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_deriv_kernel(const GradArgs a) {
    __shared__ double lds[3 * kGradBlock];
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    const RowInfo ri = row_info(a, r);
    const bool valid = i < a.npix;
    const double g = valid ? a.F[(size_t)r * a.npix + i] : 0.0;
    const double nu = valid ? a.nu[i] : a.nu[0];
    double* out = part_of(a, r);
    for (int c = 0; c < ri.nc + a.lay.nfill; ++c) {
        const Comp k = comp_of(a, ri, c);
        LineSums s = line_sums(a, r, k, nu);
        s.sN *= g * kLn10; s.sz *= g; s.sb *= g;
        block_sum3(s.sN, s.sz, s.sb, lds);
        if (threadIdx.x == 0) { out[k.col] = s.sN; out[k.col + 1] = s.sz; out[k.col + 2] = s.sb; }
    }
    if (threadIdx.x == 0) zero_inactive(a, ri, out);
}

// kVeto: rows whose logL is -inf (veto) or NaN get NaN too (the VJP has no logL).
template <bool kVeto>
__device__ __forceinline__ void finalize_cell(const GradArgs& a) {
    const long e = (long)blockIdx.x * kGradBlock + threadIdx.x;
    if (e >= (long)a.nrows * a.lay.ndim) return;
    const int r = (int)(e / a.lay.ndim), k = (int)(e - (long)r * a.lay.ndim);
    const double lg = kVeto ? a.logL[r] : 0.0;
    double s;
    if (a.rows[(size_t)r * kGradRow + 4] != 0.0 || !(lg > -INFINITY)) {
        s = NAN;                                                                    // too many taps, veto (-inf) or NaN row
    } else {
        s = 0.0;
        const double* p = a.part + (size_t)r * a.ntiles * a.lay.ndim + k;
        for (int t = 0; t < a.ntiles; ++t) s += p[(size_t)t * a.lay.ndim];
    }
    a.G[(size_t)r * a.lay.ndim + k] = s;
}

__global__ __launch_bounds__(kGradBlock) void mcalf_grad_finalize_kernel(const GradArgs a) { finalize_cell<true>(a); }

__global__ __launch_bounds__(kGradBlock) void mcalf_vjp_finalize_kernel(const GradArgs a) { finalize_cell<false>(a); }

// JVP, the one Voigt pass: per pixel tau and its directional derivative along the row's tangent, the deriv kernel's line sums
// contracted with v instead of reduced over pixels.  Records and tangent entries are row-uniform (scalar loads); the ncomp
// slot of v and the (N, z, b) of inactive components are never read.
__global__ __launch_bounds__(kGradBlock) void mcalf_jvp_forward_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    const double* v = a.V + (size_t)r * a.lay.ndim;
    const double nu = a.nu[i];
    double tau = 0.0, dtau = 0.0;
    for (int c = 0; c < ri.nc + a.lay.nfill; ++c) {
        const Comp k = comp_of(a, ri, c);
        const LineSums s = line_sums(a, r, k, nu);
        tau += s.sN;
        dtau += kLn10 * s.sN * v[k.col] + s.sz * v[k.col + 1] + s.sb * v[k.col + 2];
    }
    const double F = exp(-tau);
    a.F[(size_t)r * a.npix + i] = F;
    a.q[(size_t)r * a.npix + i] = -F * dtau;
}

// JVP, the convolutions: dM = cont L(T) + v_cont L(F) + v_R cont (dL/dR)(F).
__global__ __launch_bounds__(kGradBlock) void mcalf_jvp_model_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    double* out = a.dM + (size_t)r * a.npix;
    if (ri.bad) {                                                                  // more taps than the context provisions
        out[i] = NAN;
        return;
    }
    const double* v = a.V + (size_t)r * a.lay.ndim;
    const double vR = a.lay.freespecres ? v[0] : 0.0;
    const double vc = a.lay.freecont ? v[cont_col(a.lay)] : 0.0;
    const Lsf s = lsf_forward<kLsfR | kLsfT>(a, ri, r, i);
    out[i] = ri.cont * s.cT + vc * s.cF + vR * ri.cont * s.rF;
}

// ---- The Hessian-vector product of logL (mcalf_loglike_hvp_batch): forward mode over the gradient's reverse pass. ----
// With d(.) the directional derivative along the row's tangent v, T = dF (jvp_forward) and dM = d m (jvp_model's sum):
//     q = W (d - m),  dq = -W dM                                          (W = 1/err^2 on the pixels nansum keeps, else 0)
//     (H v)_cont = sum_i [dq L(F) + q (L(T) + v_R (dL/dR) F)]
//     (H v)_R    = sum_i [dq cont (dL/dR) F + q v_cont (dL/dR) F + q cont ((dL/dR) T + v_R (d2L/dR2) F)]
//     g = -F cont L^T q,   dg = -T cont L^T q - F v_cont L^T q - F cont v_R (dL/dR)^T q - F cont L^T dq
//     (H v)_k    = sum_i [dg_i dtau_i/dtheta_k + g_i sum_k' d2tau_i/dtheta_k dtheta_k' v_k']      k, k' the (N, z, b) of ONE component
// Per (component, line), s = nu/dnu (du/dz), z = u + i a ~ 1/b:
//     d2tau/dN dtheta = ln10 dtau/dtheta,   d2tau/dz2 = K s^2 Re w'',   d2tau/dz db = -(K s/b) Re (z w)'',   d2tau/db2 = (K/b^2) Re (z^2 w)''
// The entries of v that are 0 columns of the gradient are never read; R's is not read either when the row has no taps (R <= velstep).

namespace {

struct RowTangent { double vR, vc; };

__device__ __forceinline__ RowTangent row_tangent(const GradArgs& a, int r, const RowInfo& ri) {
    const double* v = a.V + (size_t)r * a.lay.ndim;
    RowTangent o;
    o.vR = (a.lay.freespecres && (a.lay.jax || ri.n > 0)) ? v[0] : 0.0;
    o.vc = a.lay.freecont ? v[cont_col(a.lay)] : 0.0;
    return o;
}

}  // namespace

// d2 w_k / dR2 of the normalised taps: with c_k = k^2 - sum_j w_j j^2 and var = sum_j w_j c_j^2,
//     d2 w_k / dsigma2 = w_k ((c_k^2 - var) / sigma^6 - 3 c_k / sigma^4),   dsigma/dR constant.
__global__ __launch_bounds__(kGradBlock) void mcalf_hvp_taps_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    const int r = blockIdx.x;
    const int t = threadIdx.x;
    const RowInfo ri = row_info(a, r);
    const int n = ri.n;
    const double* taps = a.taps + (size_t)r * a.tapcap;
    double* ddtaps = a.ddtaps + (size_t)r * a.tapcap;
    const double sigma = (ri.R / kFwhmToSigma) / a.velstep;
    const double m2 = tap_m2(taps, n, lds);
    double var = 0.0;
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double c = tap_centre(k, n, m2);
        var += taps[k] * c * c;
    }
    var = block_sum(var, lds);
    const double s2 = sigma * sigma, is4 = 1.0 / (s2 * s2), is6 = is4 / s2;
    const double dsdR = 1.0 / (kFwhmToSigma * a.velstep);
    for (int k = t; k <= 2 * n; k += kGradBlock) {
        const double c = tap_centre(k, n, m2);
        ddtaps[k] = no_taps(a, n) ? 0.0 : taps[k] * ((c * c - var) * is6 - 3.0 * c * is4) * (dsdR * dsdR);
    }
}

// q, dq and the continuum / R partials of H v from one forward walk with all five sums.
__global__ __launch_bounds__(kGradBlock) void mcalf_hvp_model_kernel(const GradArgs a) {
    __shared__ double lds[kGradBlock];
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    const RowInfo ri = row_info(a, r);
    const RowTangent rt = row_tangent(a, r, ri);
    double pc = 0.0, pR = 0.0;
    if (i < a.npix) {
        const Lsf s = lsf_forward<kLsfR | kLsfRR | kLsfT | kLsfRT>(a, ri, r, i);
        const double is2 = a.ispec2[i];
        const double res = a.obj[i] - ri.cont * s.cF;
        const double term = is2 * res * res - a.lgis[i];
        const bool drop = isnan(term);                                             // the pixels nansum drops: W = 0
        const double dM = ri.cont * s.cT + rt.vc * s.cF + rt.vR * ri.cont * s.rF;
        const double qv = drop ? 0.0 : is2 * res;
        const double dqv = drop ? 0.0 : -is2 * dM;
        a.hq[(size_t)r * a.npix + i] = qv;
        a.hdq[(size_t)r * a.npix + i] = dqv;
        pc = dqv * s.cF + qv * (s.cT + rt.vR * s.rF);
        pR = (dqv * ri.cont + qv * rt.vc) * s.rF + qv * ri.cont * (s.rT + rt.vR * s.rrF);
    }
    reduce_cont_R(a, r, pc, pR, a.lay.jax || ri.n > 0, lds);
}

// g and dg in place of F and T from one transposed walk with all three sums.
__global__ __launch_bounds__(kGradBlock) void mcalf_hvp_adjoint_kernel(const GradArgs a) {
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    if (i >= a.npix) return;
    const RowInfo ri = row_info(a, r);
    const RowTangent rt = row_tangent(a, r, ri);
    const LsfT s = lsf_transposed<true>(a, ri, r, i, a.hq + (size_t)r * a.npix, a.hdq + (size_t)r * a.npix);
    double* F = a.F + (size_t)r * a.npix;
    double* T = a.q + (size_t)r * a.npix;
    const double f = F[i], tt = T[i];
    F[i] = -f * ri.cont * s.lq;
    T[i] = -(tt * ri.cont + f * rt.vc) * s.lq - f * ri.cont * (rt.vR * s.rq + s.ldq);
}

// The second-order Voigt pass: per active component the three sums of dg dtau/dtheta_k + g (d2tau/dtheta_k dtheta_k') v_k'.
__global__ __launch_bounds__(kGradBlock) void mcalf_hvp_deriv_kernel(const GradArgs a) {
    __shared__ double lds[3 * kGradBlock];
    const int r = blockIdx.y;
    const int i = blockIdx.x * kGradBlock + threadIdx.x;
    const RowInfo ri = row_info(a, r);
    const bool valid = i < a.npix;
    const double g = valid ? a.F[(size_t)r * a.npix + i] : 0.0;
    const double dg = valid ? a.q[(size_t)r * a.npix + i] : 0.0;
    const double nu = valid ? a.nu[i] : a.nu[0];
    const double* v = a.V + (size_t)r * a.lay.ndim;
    double* out = part_of(a, r);
    for (int c = 0; c < ri.nc + a.lay.nfill; ++c) {
        const Comp k = comp_of(a, ri, c);
        double tN = 0.0, tz = 0.0, tb = 0.0, tzz = 0.0, tzb = 0.0, tbb = 0.0;
        for (int l = 0; l < k.nl; ++l) {
            const double* rec = rec_of(a, r, k.slot0 + l);
            const double u = nu * rec[0] - rec[1], y = rec[2], K = rec[3], s = nu * rec[4], ib = rec[5];
            double wr, dr, e, d2, e2, e3;
            faddeeva_d2w(u, y, wr, dr, e, d2, e2, e3);
            tN += K * wr;                                   // tau
            tz += K * dr * s;                               // K H_u du/dz
            tb -= K * ib * e;                               // -(K/b) Re (z w)'
            tzz += K * s * s * d2;
            tzb -= K * s * ib * e2;
            tbb += K * ib * ib * e3;
        }
        const double vN = kLn10 * v[k.col], vz = v[k.col + 1], vb = v[k.col + 2];
        double sN = kLn10 * (dg * tN + g * (tN * vN + tz * vz + tb * vb));
        double sz = dg * tz + g * (tz * vN + tzz * vz + tzb * vb);
        double sb = dg * tb + g * (tb * vN + tzb * vz + tbb * vb);
        block_sum3(sN, sz, sb, lds);
        if (threadIdx.x == 0) { out[k.col] = sN; out[k.col + 1] = sz; out[k.col + 2] = sb; }
    }
    if (threadIdx.x == 0) zero_inactive(a, ri, out);
}

__global__ void mcalf_grad_hjert_kernel(const double* x, const double* y, long n, double* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double wr, wi, dr, di, e;
    faddeeva_dw(x[i], y[i], wr, wi, dr, di, e);
    out[3 * i] = wr;
    out[3 * i + 1] = dr;          // dH/dx = Re w'
    out[3 * i + 2] = -di;         // dH/dy = Re(i w') = -Im w'
}

namespace mcalf {
const void* grad_kernel_ptr(GradKernel k) {
    static const void* const table[] = {                                           // in the order of enum GradKernel
        (const void*)&mcalf_grad_setup_kernel,    (const void*)&mcalf_hvp_taps_kernel,
        (const void*)&mcalf_grad_forward_kernel,  (const void*)&mcalf_grad_model_kernel,   (const void*)&mcalf_vjp_model_kernel,
        (const void*)&mcalf_grad_adjoint_kernel,  (const void*)&mcalf_grad_deriv_kernel,   (const void*)&mcalf_jvp_forward_kernel,
        (const void*)&mcalf_jvp_model_kernel,     (const void*)&mcalf_hvp_model_kernel,    (const void*)&mcalf_hvp_adjoint_kernel,
        (const void*)&mcalf_hvp_deriv_kernel,     (const void*)&mcalf_grad_finalize_kernel, (const void*)&mcalf_vjp_finalize_kernel,
        (const void*)&mcalf_grad_hjert_kernel};
    static_assert(sizeof(table) / sizeof(table[0]) == kGradKernelCount, "one entry per GradKernel");
    return table[k];
}
}  // namespace mcalf
