// Fused likelihood kernel (kernels.hip), the streaming single launch: how waves of ONE launch hand live points to each other
// (waits, stamps), the set-up phase of a workgroup and its way out of the kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_args.h"
#include "sample_setup.h"

namespace mcalf {

// ---- streaming single launch: hand-over between waves, waits ---------------------------------------------------------
// Waves of ONE launch hand data to each other here (records / taps / header of a live point, its stamp, the HBM copy of
// its parameter row), and the host hands rows to the launch while it runs.  The eight XCDs of an MI355X each have their
// own L2, which is not coherent with the others' for ordinary device memory: across XCDs a hand-over needs an agent-scope
// release (write back the producer's L2) and acquire (invalidate the consumer's) -- measured here at 4x the launch's
// duration when done per row and per item.  So nothing is handed over ACROSS XCDs: the live points are dealt out to the
// XCDs in blocks of eight rows (block k -> XCD k % 8), every XCD sets up ITS rows with its own workgroups and consumes
// them with its own workgroups through its own queue (xcd_id(): the hardware's XCC_ID, not an assumption about the
// dispatch order).  Producer and consumer of a row share one L2, which IS coherent: plain stores, a wait for their
// acknowledgement (s_waitcnt vmcnt(0): they are in the L2), then the stamp; the consumer sees the stamp and reads the row
// with plain loads.  Rows own their 128-byte lines, so a consumer's L1 never holds a line of a row it has not been handed.
// Stamps and queue counters are device-scope atomics, which meet in memory.  The host's rows and words are page-locked
// coherent memory, read past every cache; RESULTS go to page-locked memory as system-scope stores (write-through), because
// the host reads them as soon as the completion word says so, ahead of the end-of-kernel write-back -- plain stores were
// measured to linger in one XCD's L2 past that word (rows of one XCD missing from the first call's results).
__device__ __forceinline__ void stream_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void stream_compiler_barrier() { asm volatile("" ::: "memory"); }

// Every wait is bounded (a.spin_ticks of the 100 MHz s_memrealtime clock): a wave that runs out of patience raises
// status[0], after which nobody waits any more -- the rows still missing are published as unusable (`bad`: logL = -inf)
// and the grid drains; the host sees status[0] and fails the call.  No wave can stay behind in the kernel.
__device__ __forceinline__ bool stream_gave_up(const KArgs& a) {
    return __hip_atomic_load(a.status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0u;
}

// Wait until the host has staged row r (a.arrived counts the rows staged so far).  false: gave up.
__device__ __forceinline__ bool stream_wait_arrived(const KArgs& a, unsigned r, unsigned& seen) {
    if (seen > r) return true;
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while (true) {
        seen = __hip_atomic_load(a.arrived, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        stream_compiler_barrier();                       // (the row's loads are issued behind this one's return)
        if (seen > r) return true;
        if ((long long)(__builtin_amdgcn_s_memrealtime() - t0) > a.spin_ticks || stream_gave_up(a)) {
            __hip_atomic_store(a.status, kStreamHostLate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            return false;
        }
        __builtin_amdgcn_s_sleep(32);                    // (~1 us: a poll is a PCIe read)
    }
}

// Wait until live point s is set up (every lane of the workgroup calls this with the same s).  Its records, taps
// and header were written by a wave of this XCD, into the L2 both share, before its stamp.
__device__ __forceinline__ void stream_wait_ready(const KArgs& a, int s, unsigned early) {
    if (early != a.gen) {
        const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
        while (__hip_atomic_load(a.ready + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != a.gen) {
            if ((long long)(__builtin_amdgcn_s_memrealtime() - t0) > a.spin_ticks) {   // (never seen: the producers' own waits are bounded)
                __hip_atomic_store(a.status, kStreamStampLate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                break;
            }
            __builtin_amdgcn_s_sleep(4);
        }
    }
    stream_compiler_barrier();
}

// Streaming single launch, set-up phase of a workgroup on XCD x (one WAVE per live point, as in mcalf_sample_kernel; same
// setup_sample(), same bits).  A workgroup claims local blocks (eight consecutive rows each) of ITS XCD with one atomic --
// one of the first `eager_rows` blocks, which any workgroup of the XCD may take; then, a dedicated workgroup only (the
// first `stream_wgs` to start on the XCD), `rest_chunk` / 8 of the remaining ones, in ticket order, until none is left.
// Thread 0 alone asks the host's row count (every wave polling a word of host memory saturated the PCIe read queue the
// rows themselves come through).  Rows that live in host memory are first copied to HBM by the whole workgroup --
// coalesced, all loads of the claim in flight at once, ONE PCIe round trip instead of setup_sample's two or three
// dependent ones -- and set up from the copy.  Claims are dynamic on purpose: a row is owned by a workgroup that is
// running, never by one that waits for a slot.
template <bool kZeroPad, bool kSelfHalo>
__device__ __forceinline__ void stream_setup_phase(const KArgs& a, int tid, int x, int* sClaim) {
    const int lane = tid & 63, wave = tid >> 6;
    // (the wave's table of segment ends, once for all its rows: behind the claim words, in LDS the item loop lays out afresh)
    double* ends = reinterpret_cast<double*>(sClaim) + 16 + wave * kSegEnds;
    if (kSelfHalo) fill_segment_ends(a, lane, ends);
    constexpr int nx = kXcds;
    const int nloc = stream_rows_of(a.nrows, x, nx), nblk = (nloc + 7) >> 3;      // this XCD's live points / local blocks
    const int eager = min(a.eager_rows, nblk);
    KArgs as = a;
    if (a.Pdev) as.P = a.Pdev;                           // the rows are set up from their copy in HBM
    unsigned seen = a.arrived ? 0u : (unsigned)a.nrows;  // (thread 0's view of the host's row count)
    if (tid == 0) sClaim[3] = (int)atomicAdd(&a.sctl->arrive[x], 1u);
    __syncthreads();
    const bool dedicated = sClaim[3] < a.stream_wgs;
    bool rest = false;
    // A dedicated workgroup shares its CU with a workgroup that is in the component loop at raised priority; the
    // set-up is a chain of latencies with few instructions: it goes first, and the queue stays ahead of the consumers.
    __builtin_amdgcn_s_setprio(3);
    while (true) {
        if (tid == 0) {
            const int want = rest ? max(a.rest_chunk >> 3, 1) : 1, lim = rest ? nblk : eager;
            const int c = rest ? eager + (int)atomicAdd(&a.sctl->sq_rest[x], (unsigned)want) : (int)atomicAdd(&a.sctl->sq_eager[x], 1u);
            const int cnt = c < lim ? min(want, lim - c) : 0;
            int ok = 1;
            if (cnt != 0 && a.arrived) {                 // (rows arrive in order: the claim's last row is the one to wait for)
                const int last = min(stream_row(x, 8 * (c + cnt) - 1, nx), a.nrows - 1);
                ok = stream_wait_arrived(a, (unsigned)last, seen) ? 1 : 0;
            }
            sClaim[0] = c; sClaim[1] = cnt; sClaim[2] = ok;
        }
        __syncthreads();
        const int c = sClaim[0], cnt = sClaim[1];
        const bool ok = sClaim[2] != 0;
        __syncthreads();                                 // (the slots are rewritten by the next claim)
        if (cnt == 0) {
            if (!rest && dedicated) { rest = true; continue; }
            break;
        }
        if (a.Pdev && ok) {                              // host -> HBM, block after block (a block's rows are contiguous)
            const int perBlock = 8 * a.ndim, n = cnt * perBlock;
            for (int i0 = tid; i0 < n; i0 += 4 * kBlock) {
                double v[4];
                size_t at[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int i = i0 + k * kBlock, blk = i / perBlock;
                    at[k] = (size_t)stream_row(x, 8 * (c + blk), nx) * a.ndim + (size_t)(i - blk * perBlock);
                    v[k] = (i < n && at[k] < (size_t)a.nrows * a.ndim) ? a.P[at[k]] : 0.0;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (i0 + k * kBlock < n && at[k] < (size_t)a.nrows * a.ndim) a.Pdev[at[k]] = v[k];
            }
            stream_stores_done();
            __syncthreads();
        }
        // the wave's rows of the claim (one per block), one after the other; ONE wait for the L2's acknowledgements, then
        // their stamps (a wait per row put the stores' round trip on the path of every row)
        for (int k = 0; k < cnt; ++k) {
            const int r = stream_row(x, 8 * (c + k) + wave, nx);
            if (r >= a.nrows) continue;
            SampleHdr* hdrp = reinterpret_cast<SampleHdr*>(reinterpret_cast<double*>(a.hdr) + (size_t)r * a.hdr_stride);
            if (ok) {
                setup_sample<kZeroPad>(as, (long)r, lane, a.recs + (size_t)r * a.rec_stride, a.taps + (size_t)r * a.tap_stride, true, hdrp, true,
                                       kSelfHalo, ends);
            } else if (lane == 0) {                      // gave up on the host: a row nobody will mistake for a result
                SampleHdr h;
                h.cont = 0.0; h.bot = 1.0; h.ncl = 0; h.n = 0; h.bad = 1; h.ngeneral = 0;
                *hdrp = h;
            }
        }
        stream_stores_done();                            // the rows' records / taps / headers are in the L2 before their stamps
        if (lane < cnt) {
            const int r = stream_row(x, 8 * (c + lane) + wave, nx);
            if (r < a.nrows) __hip_atomic_store(a.ready + r, a.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();
}

// A workgroup of the streaming launch leaves the kernel: the last one out re-arms the queues for the next launch and
// tells the host (status[1] = gen; every result of every workgroup has been acknowledged by the memory system by
// then, and results and word travel to the host as posted writes in that order -- the host polls this word instead of
// waiting for the stream's signal).  Thread 0 wrote the workgroup's results itself.
__device__ __forceinline__ void stream_exit(const KArgs& a, int tid) {
    if (tid != 0) return;
    stream_stores_done();
    if (atomicAdd(&a.sctl->exited, 1u) == gridDim.x - 1) {
        // status[2] / [3]: the fewest / most workgroups an XCD received.  An XCD's rows are set up and evaluated by ITS
        // workgroups only: with status[2] == 0 one of them got none (a partition mode or CU mask the context's probe did
        // not reflect) and its result slots are untouched -- the host then does not take the launch for an answer
        // (run_host_stream fails over to the row-block pipeline).
        unsigned lo = ~0u, hi = 0u;
        for (int k = 0; k < kXcds; ++k) {
            const unsigned n = __hip_atomic_load(&a.sctl->arrive[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            lo = min(lo, n); hi = max(hi, n);
        }
        __hip_atomic_store(a.status + 2, lo, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(a.status + 3, hi, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        for (int k = 0; k < kXcds; ++k) {
            __hip_atomic_store(&a.sctl->arrive[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.sctl->sq_eager[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.sctl->sq_rest[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(&a.sctl->queue[k], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __hip_atomic_store(&a.sctl->exited, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        stream_stores_done();
        __hip_atomic_store(a.status + 1, a.gen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace mcalf
