// libmcalf_hip.so -- MI355X (gfx950) implementation of the MC-ALF likelihood hot path.
//
// Per call, on the caller's stream:
//   mcalf_sample_kernel  one wave per live point s: decode p_s (optionally from a unit-cube row), the
//                        (component,line) records, the LSF taps                hires_fitter.py:412-431,357-364,454-459
//   mcalf_fused_kernel   one workgroup per (live point s, pixel tile T):
//     1. tau(pixel) = sum_cl K_cl H(u_cl(pixel), a_cl): per line a node pass (far wings at 8 nodes per 64-pixel
//        segment, interpolated once per sample) and per-pixel evaluation of the rest; flux = exp(-tau) into an
//        LDS tile with +-n halo                                               hires_fitter.py:365,377,430-442
//     2. sliding-window Gaussian LSF from LDS (periodic / zero-pad)           hires_fitter.py:452-464 / :667-681
//     3. x continuum, Gaussian log-likelihood terms, nansum, wave + LDS reduce   hires_fitter.py:292-294
//   mcalf_finalize_kernel  only when a spectrum needs several tiles: adds the per-tile partials in fixed order
//                        (no float atomics anywhere, so a sharded batch equals the unsharded one bit for bit).
//
// This file is the DEVICE side, ONE translation unit: the __global__ kernels and, at its end, the table of kernel entry
// points the host files launch through (kernel_args.h declares it together with the argument block).  What the kernels
// are made of comes from a header per stage:
//   wave_util.h        the XCD a wave runs on, tile positions, DPP sums, wave-uniform values, accumulators tied to a register
//   sample_setup.h     the set-up of a live point by one wave (records, segment-mask words, taps, header); the hand-out order
//   stream_handover.h  the streaming launch: waits and stamps, its set-up phase, its way out
//   line_eval.h        eval_line, eval_general_lines
//   fused_item.h       the work item: its LDS (ItemLds of kernel_args.h) and geometry, request_item, one function per
//                      phase -- ticket take / resolve / publish, fold_group, component_loop, flux_to_tile,
//                      convolve_tile, likelihood_terms, reduce_and_store -- and fused_items, the loop that calls them
//   wide_lsf.h         the taps and convolution kernels behind the fused one when the LSF is wider than a tile
// The C ABI (include/mcalf_hip.h) lives in
// host_abi.cpp (contexts, launches, the entries), host_stream.cpp (the streaming launch of the host-pointer entries),
// broker.cpp (resident evaluator, likelihood broker) and comm.cpp (RCCL gather).
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_args.h"
#include "voigt_device.h"
#include "wave_util.h"
#include "sample_setup.h"
#include "stream_handover.h"
#include "line_eval.h"
#include "fused_item.h"
#include "wide_lsf.h"

namespace mcalf {

template <bool kZeroPad>
__global__ __launch_bounds__(kSetupBlockMax) void mcalf_sample_kernel(const KArgs a, long batch) {
    // one WAVE per live point, blockDim.x / 64 live points per workgroup (the waves never synchronise); with an
    // ordered hand-out workgroup 0 builds the order and the live points start at workgroup 1
    int blk = blockIdx.x;
    if (a.order) {
        if (blk == 0) { build_order<kZeroPad>(a, batch); return; }
        --blk;
    }
    const long s = (long)blk * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (s >= batch) return;
    const int lane = threadIdx.x & 63;
    if (s == 0 && lane == 0) *a.queue = 0u;          // item queue of the fused kernel that follows on the stream
    __shared__ double sEnds[kSetupBlockMax / 64][kSegEnds];
    double* ends = sEnds[threadIdx.x >> 6];
    if (a.selfhalo) fill_segment_ends(a, lane, ends);
    setup_sample<kZeroPad>(a, s, lane, a.recs + (size_t)s * a.ncl_cap * kRecStride,
                           a.taps + (a.taps_shared ? 0 : (size_t)s * (2 * a.n_cap + 8)), !a.taps_shared || s == 0, a.hdr + s, true,
                           a.selfhalo != 0, ends);
}

template <bool kZeroPad, bool kSelfHalo, int kLinesPerSync, bool kInline, bool kStream>
__global__ __launch_bounds__(kBlock, kMinWaves) void mcalf_fused_kernel(const KArgs a) {
    static_assert(!(kInline && kStream), "the one-launch variant of small calls has no queue to stream through");
    extern __shared__ __align__(16) double smem[];
    if constexpr (kStream) {
        stream_setup_phase<kZeroPad, kSelfHalo>(a, threadIdx.x, xcd_id(), reinterpret_cast<int*>(smem));

        // (the item loop's arguments start their lives here: fresh_kargs)
        const KArgs fresh = fresh_kargs();
        fused_items<kZeroPad, kSelfHalo, kLinesPerSync, kInline, kStream>(fresh, smem);
    } else {
        fused_items<kZeroPad, kSelfHalo, kLinesPerSync, kInline, kStream>(a, smem);
    }
}

// RESIDENT one-theta evaluator (opt-in: mcalf_set_resident).  The solvers call the likelihood one theta at a time
// (lnlhood_pc / _dy / _mn, hires_fitter.py:250-285), and of such a call's 18 us only 11 are the kernel: the rest is the
// launch -- and launches of different processes serialise at 8.5 us each.  So ONE workgroup stays on the chip between calls
// and takes its requests from a page-locked mailbox: the host writes the row and bumps `req`; thread 0 polls `req` (a PCIe
// read per look), the workgroup copies the row into LDS with system-scope loads (nothing of a request is ever read
// through a cache), runs the one-launch variant's item on it -- same code, same bits -- and the result goes out as a
// system-scope store, followed by `ack`.  The kernel LEAVES after `idle_ticks` without a request (or when told to):
// state = leaving, one more look at `req` (a request that slipped in is served, state = running again), state = gone.
// The host treats "gone" as "launch another one"; a request posted behind the last look is therefore never lost, and no
// wave can stay behind: every wait is bounded by the idle limit.
// (mailbox and shared words: ResidentBox / ResidentShared in kernel_args.h)
template <bool kZeroPad, bool kSelfHalo>
__global__ __launch_bounds__(kBlock, 2) void mcalf_resident_kernel(const KArgs a, ResidentBox* boxes, ResidentShared* shared,
                                                                           long long idle_ticks, int row_offset_doubles) {
    extern __shared__ __align__(16) double smem[];
    double* sRow = smem + row_offset_doubles;            // behind everything the item uses
    unsigned* sCtl = reinterpret_cast<unsigned*>(sRow + kResRowMax);
    const int tid = threadIdx.x;
    ResidentBox* box = boxes + blockIdx.x;
    const unsigned long long t_launch = __builtin_amdgcn_s_memrealtime();
    // the number of the last request this mailbox has had answered: what comes next is new
    unsigned seen = __hip_atomic_load(&box->ack, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    while (true) {
        if (tid == 0) {
            unsigned r;
            while (true) {
                // (`req` and `quit` share eight bytes: ONE PCIe read per look)
                const unsigned long long both = __hip_atomic_load(reinterpret_cast<unsigned long long*>(&box->req), __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_SYSTEM);
                r = (unsigned)both;
                if (r != seen) break;
                bool leave = (unsigned)(both >> 32) != 0u || __hip_atomic_load(&shared->leave, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
                if (!leave && blockIdx.x == 0) {         // workgroup 0 keeps the launch's clock
                    const unsigned long long last = __hip_atomic_load(&shared->last, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    const unsigned long long since = last > t_launch ? last : t_launch;
                    if ((long long)(__builtin_amdgcn_s_memrealtime() - since) > idle_ticks) leave = true;
                }
                if (leave) {
                    __hip_atomic_store(&shared->leave, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&box->state, kResLeaving, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    stream_stores_done();                // (a read does not pass the posted write: the host has "leaving" before this look)
                    r = __hip_atomic_load(&box->req, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    if (r != seen) { __hip_atomic_store(&box->state, kResRunning, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); break; }
                    __hip_atomic_store(&box->state, kResGone, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                    break;
                }
                __builtin_amdgcn_s_sleep(2);
            }
            sCtl[0] = r;
        }
        __syncthreads();
        const unsigned r = sCtl[0];
        __syncthreads();
        if (r == seen) return;                           // (workgroup-uniform) gone
        // the row, past every cache
        if (tid < kResRowMax) {
            const unsigned long long bits = __hip_atomic_load(reinterpret_cast<unsigned long long*>(box->row) + tid, __ATOMIC_RELAXED,
                                                               __HIP_MEMORY_SCOPE_SYSTEM);
            sRow[tid] = __builtin_bit_cast(double, bits);
        }
        __syncthreads();
        KArgs b = fresh_kargs();                         // (for every request: see there)
        // (the item of workgroup k is "live point k": its row is the one in LDS, its result slot the mailbox's)
        const int rowlen = b.ndim;
        b.P = sRow - (size_t)blockIdx.x * rowlen;
        b.out = &box->result - blockIdx.x;
        fused_items<kZeroPad, kSelfHalo, 4, true, false>(b, smem);
        if (tid == 0) {                                  // (thread 0 stored the result itself)
            stream_stores_done();
            __hip_atomic_store(&box->ack, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            __hip_atomic_fetch_max(&shared->last, __builtin_amdgcn_s_memrealtime(), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        seen = r;
        __syncthreads();
    }
}

// done_word != nullptr (the streaming launch of a TILED spectrum): `out` is page-locked host memory the host reads as soon as
// *done_word == gen -- results go out as system-scope stores, and the last workgroup to finish (fin_count, re-armed by
// it) writes the word behind them, as stream_exit() does for single-tile spectra.
__global__ void mcalf_finalize_kernel(const double* partial, double* out, long batch, int ntiles, int mode,
                                      int asymm, double veto4, double veto5, unsigned int* fin_count, unsigned int* done_word,
                                      unsigned int gen) {
    const long s = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s < batch) {
        double sum = 0.0, cnt = 0.0, c4 = 0.0, c5 = 0.0;
        for (int t = 0; t < ntiles; ++t) {
            const double* pr = partial + (s * ntiles + t) * 4;
            sum += pr[0]; cnt += pr[1]; c4 += pr[2]; c5 += pr[3];
        }
        const double val = finalize_value(mode, sum, cnt, asymm != 0, c4, c5, veto4, veto5);
        if (done_word) __hip_atomic_store(out + s, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        else out[s] = val;
    }
    if (done_word) {                                         // (grid-uniform)
        stream_stores_done();
        __syncthreads();
        if (threadIdx.x == 0 && atomicAdd(fin_count, 1u) == gridDim.x - 1) {
            __hip_atomic_store(fin_count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            stream_stores_done();
            __hip_atomic_store(done_word, gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

__global__ void mcalf_hjert_kernel(const double* x, const double* y, long n, double* out, const double* tabs,
                                   int node_form) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = hjert_folded(x[i], y[i], tabs, node_form != 0);
}

__global__ void mcalf_scale_cube_kernel(const double* lo, const double* hi, const double* cube, long total,
                                        int ndim, int slot, int int_ncomp, double* theta) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int d = (int)(i % ndim);
    // separately rounded multiply and add (no FMA contraction), as numpy evaluates
    // cube*ptp + min (hires_fitter.py:206 / :214)
    double v;
    {
#pragma clang fp contract(off)
        const double scaled = cube[i] * (hi[d] - lo[d]);
        v = scaled + lo[d];
    }
    if (int_ncomp && d == slot) v = trunc(v);        // :207-208
    theta[i] = v;
}

// Single-component rows (R, cont, N, z, b) with the continuum set to 1: what the fused kernel of a wide-LSF context gets
// (it must deliver the UNCONVOLVED, continuum-free spectrum; mode OneComp reads the continuum from the row itself).
__global__ void mcalf_wide_rows_kernel(const double* rows, double* out, long batch) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= batch * 5) return;
    out[i] = (i % 5 == 1) ? 1.0 : rows[i];
}

// One bit per XCD that runs a workgroup of the launch (the host launches a few workgroups per CU on the context's
// stream: mcalf_create, mcalf_set_cu_mask): the XCDs a streaming launch on that stream can count on.
__global__ void mcalf_xcd_probe_kernel(unsigned int* mask) {
    if (threadIdx.x == 0) atomicOr(mask, 1u << xcd_raw());
}

// ---- kernel entry points for the host files (kernel_args.h) -------------------------------------------------------------
#define MCALF_K(J, S, L, I, T) reinterpret_cast<const void*>(&mcalf_fused_kernel<J, S, L, I, T>)
static const void* const kFusedKernels[] = {
    // [group: batch 4 / batch 5 / one-launch / streaming 4 / streaming 5 lines per barrier][jax][selfhalo]
    MCALF_K(false, false, 4, false, false), MCALF_K(false, true, 4, false, false), MCALF_K(true, false, 4, false, false), MCALF_K(true, true, 4, false, false),
    MCALF_K(false, false, 5, false, false), MCALF_K(false, true, 5, false, false), MCALF_K(true, false, 5, false, false), MCALF_K(true, true, 5, false, false),
    MCALF_K(false, false, 4, true, false),  MCALF_K(false, true, 4, true, false),  MCALF_K(true, false, 4, true, false),  MCALF_K(true, true, 4, true, false),
    MCALF_K(false, false, 4, false, true),  MCALF_K(false, true, 4, false, true),  MCALF_K(true, false, 4, false, true),  MCALF_K(true, true, 4, false, true),
    MCALF_K(false, false, 5, false, true),  MCALF_K(false, true, 5, false, true),  MCALF_K(true, false, 5, false, true),  MCALF_K(true, true, 5, false, true),
};
#undef MCALF_K
const void* fused_kernel_ptr(bool jax, bool selfhalo, int lps, bool inl, bool stream) {
    const int group = stream ? (lps == 5 ? 4 : 3) : inl ? 2 : (lps == 5 ? 1 : 0);
    return kFusedKernels[4 * group + (jax ? 2 : 0) + (selfhalo ? 1 : 0)];
}
int fused_kernel_count() { return (int)(sizeof(kFusedKernels) / sizeof(kFusedKernels[0])); }
const void* fused_kernel_at(int i) { return kFusedKernels[i]; }
const void* resident_kernel_ptr(bool jax, bool selfhalo) {
    if (jax) return selfhalo ? reinterpret_cast<const void*>(&mcalf_resident_kernel<true, true>)
                             : reinterpret_cast<const void*>(&mcalf_resident_kernel<true, false>);
    return selfhalo ? reinterpret_cast<const void*>(&mcalf_resident_kernel<false, true>)
                    : reinterpret_cast<const void*>(&mcalf_resident_kernel<false, false>);
}
const void* sample_kernel_ptr(bool jax) {
    return jax ? reinterpret_cast<const void*>(&mcalf_sample_kernel<true>) : reinterpret_cast<const void*>(&mcalf_sample_kernel<false>);
}
const void* finalize_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_finalize_kernel); }
const void* hjert_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_hjert_kernel); }
const void* scale_cube_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_scale_cube_kernel); }
const void* xcd_probe_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_xcd_probe_kernel); }
const void* wide_taps_kernel_ptr(bool jax) {
    return jax ? reinterpret_cast<const void*>(&mcalf_wide_taps_kernel<true>) : reinterpret_cast<const void*>(&mcalf_wide_taps_kernel<false>);
}
const void* wide_conv_kernel_ptr(bool jax) {
    return jax ? reinterpret_cast<const void*>(&mcalf_wide_conv_kernel<true>) : reinterpret_cast<const void*>(&mcalf_wide_conv_kernel<false>);
}
const void* wide_rows_kernel_ptr() { return reinterpret_cast<const void*>(&mcalf_wide_rows_kernel); }

}  // namespace mcalf
