// Device side of a device-resident nested-sampling run (mcalf_nested_*), for gfx950: the book-keeping of one round around the
// replacement step of ns_kernels.hip.  The live set UL / LL and the dead rows UD / LD stay in HBM for the whole run; a round is
//   rank     key(L) = L with NaN as -inf; rank[i] = #{ j : key_j < key_i, or key_j == key_i and j < i }, compared as doubles
//            (-0.0 == 0.0; ties keep index order: numpy's stable argsort), counted over LDS-staged tiles of kNsrBlock keys, 32 rows a
//            workgroup;
//            order[rank[i]] = i.  Integers only.
//   select   dying = order[0, K), lmin = key[order[K - 1]], r0 = rows with key <= lmin (a binary search of the sorted order),
//            nstarts = nlive - r0, pick_j = order[r0 + w0 mod nstarts] with w0 of the Philox block at counter (round + 1, 0, j, 0),
//            key (seed, 3); the dead keys, lmin and the largest key go into the round record.
//   moments  mean and covariance (divisor n - 1) of the cube rows of the n = nlive - K survivors order[K, nlive), two passes.  The
//            survivors are cut into kNsrChunks contiguous chunks of R = ceil(n / kNsrChunks) rows, chunk c = [c R, min((c + 1) R, n));
//            a chunk's sum runs over its rows in that order from 0.0, the chunk sums are added in the order c = 0, 1, ... from 0.0
//            (an empty chunk adds 0.0).  mean_k = sum / n; the covariance's entry (a, b), a >= b, is the sum of
//            (x_a - mean_a)(x_b - mean_b), a rounded difference each, a rounded product, a rounded add, divided by n - 1.
//   Cholesky ONE workgroup: the packed lower triangle in LDS (in HBM above kNsrCholLds bytes), jitter 1e-9 max(mean of the
//            variances, 1e-300) on the diagonal, left-looking column by column: s_i = a_ij - sum_{k < j} l_ik l_jk in the order
//            k = 0, 1, ..., l_jj = sqrt(s_j), l_ij = s_i / l_jj.  D = the factor's transpose as rows.  A non-finite entry of the
//            covariance or a pivot that is not positive: D = diag(std), 1 where the variance is not finite and positive.
//   gather   U0_j = UL[pick_j], Lmin_j = lmin (+inf in a plateau round: every start is then refused and nothing moves),
//            sid_j = round K + j.
//   retire   the replacements with status < 0 or not (L > lmin) are counted; at zero the dying rows go to the dead slots
//            ndead + j in death order and the replacements into the live rows they leave.
// No floating-point atomics anywhere: a round's bits depend on the live set, the round number and the options alone.
// Contraction to FMA is switched off for the whole file, as in ns_kernels.hip: every product and sum is rounded separately.
#include <hip/hip_runtime.h>

#include "ns_round_args.h"

#pragma clang fp contract(off)

#include "wave_row.h"

using namespace mcalf;

namespace {

__device__ __forceinline__ double nsr_key(double l) { return l != l ? -__builtin_inf() : l; }
__device__ __forceinline__ double rec_double(const NsrArgs& a, int word) { return __longlong_as_double((long long)a.rec[(size_t)a.K + word]); }
__device__ __forceinline__ long long rec_int(const NsrArgs& a, int word) { return (long long)a.rec[(size_t)a.K + word]; }
__device__ __forceinline__ void rec_put(const NsrArgs& a, int word, double v) { a.rec[(size_t)a.K + word] = (uint64_t)__double_as_longlong(v); }
__device__ __forceinline__ void rec_put(const NsrArgs& a, int word, long long v) { a.rec[(size_t)a.K + word] = (uint64_t)v; }

// Row a of the packed lower triangle that holds entry p: a (a + 1) / 2 <= p < (a + 1) (a + 2) / 2.
__device__ __forceinline__ int tri_row(int p) {
    int a = (int)((__builtin_sqrt(8.0 * (double)p + 1.0) - 1.0) * 0.5);
    while ((a + 1) * (a + 2) / 2 <= p) ++a;
    while (a * (a + 1) / 2 > p) --a;
    return a;
}

// The survivors chunk c sums: [lo, hi) of the n.
__device__ __forceinline__ void chunk_bounds(int n, int c, int* lo, int* hi) {
    const int R = (n + kNsrChunks - 1) / kNsrChunks;
    const long long l = (long long)c * R, h = l + R;
    *lo = (int)(l < n ? l : n);
    *hi = (int)(h < n ? h : n);
}

}  // namespace

// The initial points after their replacement call (Lmin = -inf, nmoves = 0): a row it refused (status < 0) whose logL is above
// -inf lies outside the cube or holds a NaN -- outside the prior's support -- and takes logL = -inf, so that it dies first and
// carries no weight; a NaN or -inf logL stays as it is.
__global__ __launch_bounds__(kNsrBlock) void mcalf_nsr_init_kernel(const NsrArgs a) {
    const int i = blockIdx.x * kNsrBlock + threadIdx.x;
    if (i < a.nlive && a.status[i] < 0 && a.LL[i] > -__builtin_inf()) a.LL[i] = -__builtin_inf();
}

// A workgroup ranks kNsrRankRows rows; its kNsrBlock threads are kNsrRankRows rows x kNsrRankSlices slices of every staged tile of
// kNsrBlock keys: thread (row r, slice q) counts among the keys q W .. q W + W - 1 of each tile, W = kNsrBlock / kNsrRankSlices,
// and the slices' counts (integers) are added through LDS.
__global__ __launch_bounds__(kNsrBlock) void mcalf_nsr_rank_kernel(const NsrArgs a) {
    constexpr int kWidth = kNsrBlock / kNsrRankSlices;
    static_assert(kNsrRankRows * kNsrRankSlices == kNsrBlock, "one thread per (row, slice)");
    __shared__ double keys[kNsrBlock];
    __shared__ int part[kNsrRankSlices][kNsrRankRows];
    const int tid = threadIdx.x, r = tid % kNsrRankRows, q = tid / kNsrRankRows, i = blockIdx.x * kNsrRankRows + r;
    const double ki = i < a.nlive ? nsr_key(a.LL[i]) : 0.0;
    int count = 0;
    for (int t0 = 0; t0 < a.nlive; t0 += kNsrBlock) {
        const int j = t0 + tid;
        keys[tid] = j < a.nlive ? nsr_key(a.LL[j]) : __builtin_inf();     // (past the end: j > i and never below a key)
        __syncthreads();
#pragma unroll 8
        for (int e = q * kWidth; e < (q + 1) * kWidth; ++e) {
            const double kj = keys[e];
            count += (kj < ki || (kj == ki && t0 + e < i)) ? 1 : 0;
        }
        __syncthreads();
    }
    part[q][r] = count;
    __syncthreads();
    if (q != 0 || i >= a.nlive) return;
    int rank = 0;
#pragma unroll
    for (int s = 0; s < kNsrRankSlices; ++s) rank += part[s][r];
    a.rank[i] = rank;
    a.order[rank] = i;
}

__global__ __launch_bounds__(kNsrBlock) void mcalf_nsr_select_kernel(const NsrArgs a) {
    __shared__ int s_r0;
    const int tid = threadIdx.x;
    if (tid == 0) {
        const double lmin = nsr_key(a.LL[a.order[a.K - 1]]);
        int lo = a.K, hi = a.nlive;                             // the first position whose key is above lmin (nlive: none)
        while (lo < hi) {
            const int mid = lo + (hi - lo) / 2;
            if (nsr_key(a.LL[a.order[mid]]) > lmin) hi = mid;
            else lo = mid + 1;
        }
        s_r0 = lo;
        rec_put(a, kRecLmin, lmin);
        rec_put(a, kRecMaxKey, nsr_key(a.LL[a.order[a.nlive - 1]]));
        rec_put(a, kRecR0, (long long)lo);
        rec_put(a, kRecNstarts, (long long)(a.nlive - lo));
    }
    __syncthreads();
    const int r0 = s_r0, nstarts = a.nlive - r0;
    for (int j = tid; j < a.K; j += kNsrBlock) {
        const int d = a.order[j];
        a.dying[j] = d;
        a.rec[j] = (uint64_t)__double_as_longlong(nsr_key(a.LL[d]));
        uint64_t w[4];
        philox4x64_10(a.round + 1, (uint64_t)j, a.seed, 3, w);
        a.pick[j] = nstarts > 0 ? a.order[r0 + (int)(w[0] % (uint64_t)nstarts)] : d;
    }
}

__global__ __launch_bounds__(kNsrWave) void mcalf_nsr_mean_kernel(const NsrArgs a) {
    constexpr int kOwn = kNsrCovMaxDim / kNsrWave;              // coordinates a lane owns at most
    const int c = blockIdx.x, lane = threadIdx.x;
    int lo, hi;
    chunk_bounds(a.nlive - a.K, c, &lo, &hi);
    double acc[kOwn];
#pragma unroll
    for (int q = 0; q < kOwn; ++q) acc[q] = 0.0;
    for (int s = lo; s < hi; ++s) {
        const double* x = a.UL + (size_t)__builtin_amdgcn_readfirstlane(a.order[a.K + s]) * a.ndim;
#pragma unroll
        for (int q = 0; q < kOwn; ++q) {
            const int k = lane + q * kNsrWave;
            if (k < a.ndim) acc[q] = acc[q] + x[k];
        }
    }
#pragma unroll
    for (int q = 0; q < kOwn; ++q) {
        const int k = lane + q * kNsrWave;
        if (k < a.ndim) a.meanpart[(size_t)c * a.ndim + k] = acc[q];
    }
}

__global__ __launch_bounds__(kNsrBlock) void mcalf_nsr_cov_kernel(const NsrArgs a) {
    __shared__ double mean[kNsrCovMaxDim];
    __shared__ double xc[kNsrCovTile][kNsrCovMaxDim];
    const int c = blockIdx.x, tid = threadIdx.x, n = a.nlive - a.K, ndim = a.ndim, npairs = ndim * (ndim + 1) / 2;
    for (int k = tid; k < ndim; k += kNsrBlock) {
        double s = 0.0;
        for (int q = 0; q < kNsrChunks; ++q) s = s + a.meanpart[(size_t)q * ndim + k];
        mean[k] = s / (double)n;
    }
    double* part = a.covpart + (size_t)c * npairs;
    for (int p = tid; p < npairs; p += kNsrBlock) part[p] = 0.0;
    int lo, hi;
    chunk_bounds(n, c, &lo, &hi);
    __syncthreads();
    for (int s0 = lo; s0 < hi; s0 += kNsrCovTile) {
        const int m = hi - s0 < kNsrCovTile ? hi - s0 : kNsrCovTile;
        for (int e = tid; e < m * ndim; e += kNsrBlock) {
            const int r = e / ndim, k = e - r * ndim;
            xc[r][k] = a.UL[(size_t)a.order[a.K + s0 + r] * ndim + k] - mean[k];
        }
        __syncthreads();
        for (int p = tid; p < npairs; p += kNsrBlock) {        // (a thread's own entries of its workgroup's own partial)
            const int i = tri_row(p), j = p - i * (i + 1) / 2;
            double acc = part[p];
            for (int r = 0; r < m; ++r) acc = acc + xc[r][i] * xc[r][j];
            part[p] = acc;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kNsrBlock) void mcalf_nsr_chol_kernel(const NsrArgs a) {
    extern __shared__ double lds_tri[];
    __shared__ int s_bad;
    __shared__ double s_jitter;
    const int tid = threadIdx.x, n = a.nlive - a.K, ndim = a.ndim, npairs = ndim * (ndim + 1) / 2;
    double* A = a.chol_in_lds ? lds_tri : a.tri;                // the packed lower triangle: entry (i, j), j <= i, at i (i + 1) / 2 + j
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int bad = 0;
    for (int p = tid; p < npairs; p += kNsrBlock) {
        double s = 0.0;
        for (int q = 0; q < kNsrChunks; ++q) s = s + a.covpart[(size_t)q * npairs + p];
        const double v = n > 1 ? s / (double)(n - 1) : 0.0;    // (one survivor: a zero covariance)
        A[p] = v;
        bad |= (v - v == 0.0) ? 0 : 1;                          // (NaN or infinite)
        const int i = tri_row(p);
        if (p == i * (i + 1) / 2 + i) a.var[i] = v;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int k = 0; k < ndim; ++k) s = s + a.var[k];
        const double mv = s / (double)ndim;
        s_jitter = 1e-9 * (mv > 1e-300 ? mv : 1e-300);
    }
    __syncthreads();
    bool failed = s_bad != 0;
    if (!failed) {
        for (int k = tid; k < ndim; k += kNsrBlock) A[k * (k + 1) / 2 + k] = A[k * (k + 1) / 2 + k] + s_jitter;
        __syncthreads();
        for (int j = 0; j < ndim; ++j) {
            const double* lj = A + j * (j + 1) / 2;
            for (int i = j + tid; i < ndim; i += kNsrBlock) {
                double* li = A + i * (i + 1) / 2;
                double s = li[j];
                for (int k = 0; k < j; ++k) s = s - li[k] * lj[k];
                if (i != j) li[j] = s;                          // (row j's own entries are read by the others until the barrier)
                else if (s > 0.0) s_jitter = s;                 // the pivot, handed over through LDS
                else s_bad = 1;
            }
            __syncthreads();
            if (s_bad) { failed = true; break; }
            const double d = __builtin_sqrt(s_jitter);
            for (int i = j + tid; i < ndim; i += kNsrBlock) {
                double* li = A + i * (i + 1) / 2;
                li[j] = i == j ? d : li[j] / d;
            }
            __syncthreads();
        }
    }
    for (int e = tid; e < ndim * ndim; e += kNsrBlock) {
        const int r = e / ndim, c = e - r * ndim;
        double v;
        if (failed) {
            const double var = a.var[r];
            const double sd = (var - var == 0.0 && var > 0.0) ? __builtin_sqrt(var) : 0.0;
            v = c == r ? (sd > 0.0 ? sd : 1.0) : 0.0;
        } else {
            v = c >= r ? A[c * (c + 1) / 2 + r] : 0.0;          // D = (factor)^T: row r of D is column r of the factor
        }
        a.D[e] = v;
    }
}

__global__ __launch_bounds__(kNsrWave) void mcalf_nsr_gather_kernel(const NsrArgs a) {
    const int j = blockIdx.x, lane = threadIdx.x;
    const int p = __builtin_amdgcn_readfirstlane(a.pick[j]);
    const double* x = a.UL + (size_t)p * a.ndim;
    double* u = a.U0 + (size_t)j * a.ndim;
    for (int k = lane; k < a.ndim; k += kNsrWave) u[k] = x[k];
    if (lane != 0) return;
    a.Lmin[j] = rec_int(a, kRecNstarts) > 0 ? rec_double(a, kRecLmin) : __builtin_inf();
    a.sid[j] = a.round * (uint64_t)a.K + (uint64_t)j;
}

__global__ __launch_bounds__(kNsrBlock) void mcalf_nsr_retire_kernel(const NsrArgs a) {
    __shared__ int s_bad[kNsrBlock], s_first[kNsrBlock], s_zero[kNsrBlock];
    __shared__ long long s_ne[kNsrBlock];
    __shared__ double s_max[kNsrBlock];
    const int tid = threadIdx.x;
    const bool plateau = rec_int(a, kRecNstarts) == 0;
    const double lmin = rec_double(a, kRecLmin);
    int bad = 0, first = a.K, zero = 0;
    long long ne = 0;
    double mx = -__builtin_inf();
    for (int j = tid; j < a.K; j += kNsrBlock) {                // (every workgroup counts all K rows: integers, the same everywhere)
        const int st = a.status[j];
        const double l = a.Ln[j];
        if (st < 0 || !(l > lmin)) {
            bad += 1;
            first = j < first ? j : first;
        }
        zero += st == 0 ? 1 : 0;
        ne += a.nevals[j];
        const double k = nsr_key(l);
        mx = k > mx ? k : mx;
    }
    s_bad[tid] = bad; s_first[tid] = first; s_zero[tid] = zero; s_ne[tid] = ne; s_max[tid] = mx;
    __syncthreads();
    for (int h = kNsrBlock / 2; h > 0; h >>= 1) {
        if (tid < h) {
            s_bad[tid] += s_bad[tid + h];
            s_first[tid] = s_first[tid + h] < s_first[tid] ? s_first[tid + h] : s_first[tid];
            s_zero[tid] += s_zero[tid + h];
            s_ne[tid] += s_ne[tid + h];
            s_max[tid] = s_max[tid + h] > s_max[tid] ? s_max[tid + h] : s_max[tid];
        }
        __syncthreads();
    }
    const int nbad = plateau ? 0 : s_bad[0];
    if (blockIdx.x == 0 && tid == 0) {
        rec_put(a, kRecBad, (long long)nbad);
        rec_put(a, kRecFirstBad, (long long)(nbad ? s_first[0] : -1));
        rec_put(a, kRecNevals, s_ne[0]);
        rec_put(a, kRecUnfinished, (long long)s_zero[0]);
        const double before = rec_double(a, kRecMaxKey);        // (select left the largest key of the round's live set)
        if (!plateau && nbad == 0) rec_put(a, kRecMaxKey, s_max[0] > before ? s_max[0] : before);
    }
    if (plateau || nbad != 0) return;                           // the live and the dead set stay as they were
    const int lane = tid & (kNsrWave - 1), wave = tid / kNsrWave, waves = kNsrBlock / kNsrWave;
    for (int j = blockIdx.x * waves + wave; j < a.K; j += gridDim.x * waves) {
        const int d = __builtin_amdgcn_readfirstlane(a.dying[j]);
        double* live = a.UL + (size_t)d * a.ndim;
        double* dead = a.UD + ((size_t)a.ndead + j) * a.ndim;
        const double* repl = a.Un + (size_t)j * a.ndim;
        for (int k = lane; k < a.ndim; k += kNsrWave) {
            dead[k] = live[k];
            live[k] = repl[k];
        }
        if (lane == 0) {
            a.LD[(size_t)a.ndead + j] = a.LL[d];
            a.LL[d] = a.Ln[j];
        }
    }
}

__global__ __launch_bounds__(kNsrWave) void mcalf_nsr_final_kernel(const NsrArgs a) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const int src = __builtin_amdgcn_readfirstlane(a.order[r]);
    const double* live = a.UL + (size_t)src * a.ndim;
    double* dead = a.UD + ((size_t)a.ndead + r) * a.ndim;
    for (int k = lane; k < a.ndim; k += kNsrWave) dead[k] = live[k];
    if (lane == 0) a.LD[(size_t)a.ndead + r] = a.LL[src];
}

namespace mcalf {
const void* nsr_kernel_ptr(NsrKernel k) {
    static const void* const table[] = {(const void*)&mcalf_nsr_init_kernel, (const void*)&mcalf_nsr_rank_kernel, (const void*)&mcalf_nsr_select_kernel,
                                        (const void*)&mcalf_nsr_mean_kernel, (const void*)&mcalf_nsr_cov_kernel,
                                        (const void*)&mcalf_nsr_chol_kernel, (const void*)&mcalf_nsr_gather_kernel,
                                        (const void*)&mcalf_nsr_retire_kernel, (const void*)&mcalf_nsr_final_kernel};   // in the order of enum NsrKernel
    static_assert(sizeof(table) / sizeof(table[0]) == kNsrKernelCount, "one entry per NsrKernel");
    return table[k];
}
}  // namespace mcalf
