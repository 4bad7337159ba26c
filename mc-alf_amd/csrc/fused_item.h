// Fused likelihood kernel (kernels.hip), the work item: its LDS and geometry, what a workgroup loads for it, the phases an
// item goes through -- each a function of its own, in the order they run -- and fused_items(), the loop over the items of a
// launch that calls them.  Everything here is inlined into ONE kernel per instantiation: the empty-asm launderings, the
// scheduling barriers and the remarks on what spilled stand next to the statements they protect.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

#include "kernel_args.h"
#include "voigt_device.h"
#include "wave_util.h"
#include "sample_setup.h"
#include "stream_handover.h"
#include "line_eval.h"

namespace mcalf {

// What an instantiation's flags (kSelfHalo: a.selfhalo chooses it on the host; kInline; kStream) decide for its phases.
template <bool kSelfHalo, bool kInline, bool kStream>
struct ItemFlags {
    // the records carry segment-mask words (setup_sample(..., segMasks)) and the nodes sit on adjacent segments: eval_line<true>
    static constexpr bool kPreMask = kSelfHalo && !kInline;
    // batch launches read the LSF taps as scalar operands, straight from the set-up kernel's rows.  (The one-launch variant
    // has no row in memory -- wave 0 writes the taps into sW; a streaming launch reads rows that workgroups of the SAME
    // launch have just written, which the scalar data cache does not see: both read the taps from sW.)
    static constexpr bool kTapsScalar = !kInline && !kStream;
    // ticket -> work item: with an ordered hand-out, ticket t is tile (t % ntiles) of live point order[t / ntiles]
    static constexpr bool kOrdered = kSelfHalo && !kInline && !kStream;   // (the host passes a.order only to these instantiations)
    // The next ticket is published to the workgroup behind the component loop -- where the queue's answer (and the
    // order look-up) has long arrived -- rather than before the item's first barrier.  (A streaming launch's queue
    // is shared by all XCDs: published at once, its atomic's round trip to memory sat on every item's path, +7 %.)
    static constexpr bool kDeferTicket = kOrdered || kStream;
};

// ---- the LDS of a workgroup --------------------------------------------------------------------------------------------
// The regions of ItemLds (kernel_args.h: the one layout, which the host sizes the launch from) as pointers.
struct ItemSmem {
    double* sTab;    // 2 x kLinesPerSync folded tables
    double* sRec;    // ncl_cap * 8
    double* sW;      // taps, zero-padded to a multiple of 8
    double* sRed;    // kRedDoubles: 3 * kWaves partials + the next item index
    double* sWt;     // [8][64] interpolation weights, node-major
    double* sF;      // tile_doubles(tile + 2 n_cap)
    // The universal table T lives in the LDS region that later holds the flux tile (T is dead once
    // the component loop ends).  Each thread folds ONE coefficient slot per line.
    double* sT;
    int* sNext;      // [0] the next ticket, [1] the work item it stands for, [2] (streaming launch) a look at its row's stamp
};
template <int kLinesPerSync>
__device__ __forceinline__ ItemSmem carve_item_lds(const KArgs& a, double* smem) {
    const ItemLds at(kLinesPerSync, a.ncl_cap, a.n_cap);
    static_assert(kLinesPerSync * kTabPad >= kBlock, "the node sums fit the idle half of the folded tables");
    ItemSmem m;
    m.sTab = smem + at.tab;
    m.sRec = smem + at.rec;
    m.sW = smem + at.taps;
    m.sRed = smem + at.red;
    m.sWt = smem + at.wt;
    m.sF = smem + at.tile;
    m.sT = m.sF;
    m.sNext = reinterpret_cast<int*>(m.sRed + 3 * kWaves);
    return m;
}

// ---- item geometry -----------------------------------------------------------------------------------------------------
// Work item w = (live point s, pixel tile tileIdx), for request_item and the item loop alike.
// The tile always carries the full provisioned halo n_cap (so that its 64-pixel segments are the
// same for every sample); a sample with a shorter kernel simply starts `shift` entries in.
//
// Self-halo mode (a spectrum that fits ONE tile, the usual case): the periodic halo of the convolution
// consists of copies of the tile's own pixels, so only the npix real pixels are evaluated -- thread index =
// pixel index, every 64-pixel segment starts at a multiple of 64 and none crosses the seam -- and each
// flux value is stored at its body position and, near the ends, at its halo position too.  (With the halo
// evaluated as part of the tile, the segments that contain the seam cannot be interpolated; the three
// waves that own them then hold every barrier of the component loop back.)
struct ItemGeom {
    int s, tileIdx;     // live point, tile
    int t0, tlen;       // first pixel of the tile, its pixels
    int ext0, extCount; // first pixel of the tile with its provisioned halo (may be negative), its pixels
};
template <bool selfHalo>
__device__ __forceinline__ ItemGeom item_geom(const KArgs& a, int w) {
    ItemGeom g;
    g.s = selfHalo ? w : w / a.ntiles;           // (self-halo: a spectrum of ONE tile -- no division)
    g.tileIdx = selfHalo ? 0 : w - g.s * a.ntiles;
    g.t0 = g.tileIdx * a.tile;
    g.tlen = min(a.tile, a.npix - g.t0);
    g.ext0 = selfHalo ? 0 : g.t0 - a.n_cap;
    g.extCount = g.tlen + 2 * a.n_cap;
    return g;
}
constexpr int kTRegs = (VT_NY * VT_NTOT + kBlock - 1) / kBlock;   // a thread's slices of the universal table T
constexpr int kRecRegs = 2;                                        // ... and of the records: covers ncl_cap <= 128 without a second trip
__device__ __forceinline__ int rec_total(const KArgs& a) { return a.ncl_cap * kRecStride; }   // doubles of a live point's records,
__device__ __forceinline__ int tap_total(const KArgs& a) { return 2 * a.n_cap + 8; }          // ... and of its tap row

// ---- the next item's loads ---------------------------------------------------------------------------------------------
// Everything the next work item needs from global memory, requested while the current item is still in its
// convolution / likelihood phase (the loads then have the whole reduction to land in).
struct ItemLoads {
    double treg[kTRegs];                                    // this thread's slice of the universal table T
    double rreg[kRecRegs];                                  // its slice of the sample's records
    double tapreg;                                          // its LSF tap (batch instantiations: unused, the taps are scalar operands)
    double nu[kPpt];                                        // pixel frequencies of the tile
    double nuNode;                                          // this lane's interpolation node
    unsigned long long tileMask;                            // interpolable segments of the tile
    SampleHdr hd;
};

// The eight node offsets of a segment, a byte each (byte k = VT_INTERP_NODES[k]): a lane forms the offset of its node by
// a shift and a mask.  Indexed by the lane, the table is a global load, and the node's own load waits for its answer.
constexpr unsigned long long interp_node_word() {
    unsigned long long v = 0;
    for (int k = 0; k < VT_INODES; ++k) v |= (unsigned long long)VT_INTERP_NODES[k] << (8 * k);
    return v;
}
constexpr unsigned long long kNodeWord = interp_node_word();
static_assert(VT_INODES == 8 && kNodeWord == 0x3F3C3327180C0300ULL, "node offsets 0, 3, 12, 24, 39, 51, 60, 63: one byte each");
__device__ __forceinline__ int interp_node(int k) { return (int)((kNodeWord >> (8 * (k & 7))) & 0xFFu); }

// Eight LSF taps, read through the constant address space with a wave-uniform address: one scalar load of sixteen dwords.
typedef double TapGroupV __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(4))) const TapGroupV __attribute__((aligned(8))) TapGroup;

// Issue every global load of work item w: no load's address depends on another load's answer, and nothing here reads
// a loaded value, so no wait sits between the first load and the last -- they are drained in one place, at the top of the
// item that uses them (the header's counts, wave-uniform, stay in vector registers until then: see fused_items).  The
// record and tap copies run to their provisioned sizes, which do not depend on the header: slots beyond the sample's own
// counts hold stale values that are never read.
// kCoh: the streaming launch -- header, records and taps of a live point were written by a wave of the SAME launch on the
// same XCD, into rows of their own 128-byte lines (a.hdr_stride / rec_stride / tap_stride); see stream_setup_phase.
template <bool kZeroPad, bool selfHalo, bool kInline, bool kCoh = false>
__device__ __forceinline__ void request_item(const KArgs& a, int w, int tid, ItemLoads& L) {
    // The thread index is laundered through an empty asm so that the (item-invariant) load addresses are formed
    // here, from one register, instead of being hoisted out of the item loop and kept alive -- ~30 registers --
    // through the component loop, which sits at the kernel's 128-register limit.
    asm volatile("" : "+v"(tid));
    const int recTotal = rec_total(a), tapTotal = tap_total(a);
    const ItemGeom g = item_geom<selfHalo>(a, w);
    const int s = g.s;
    // (no test around the load: a slice past the table's end re-reads its last entry and is never stored)
#pragma unroll
    for (int i = 0; i < kTRegs; ++i) L.treg[i] = a.tabs[min(tid + i * kBlock, VT_NY * VT_NTOT - 1)];
    if (!kInline) {                                      // (one-launch variant: the workgroup sets the live point up itself)
        // (plain, cached loads in both cases.  Streaming launch: the row was set up by a wave of THIS XCD -- its L2 holds
        // what was written -- and owns its 128-byte lines, so this CU's L1 has not seen them before)
        const double* gr = a.recs + (size_t)s * (kCoh ? a.rec_stride : recTotal);
        const double* gt = a.taps + (kCoh ? (size_t)s * a.tap_stride : (a.taps_shared ? 0 : (size_t)s * tapTotal));
        L.hd = kCoh ? *reinterpret_cast<const SampleHdr*>(reinterpret_cast<const double*>(a.hdr) + (size_t)s * a.hdr_stride) : a.hdr[s];
#pragma unroll
        for (int i = 0; i < kRecRegs; ++i) L.rreg[i] = gr[min(tid + i * kBlock, recTotal - 1)];   // (as the T slices: no test)
        if (kCoh) L.tapreg = gt[min(tid, tapTotal - 1)];    // (batch launches read the tap row with scalar loads: convolve_tile)
    }
    const int ext0 = g.ext0;
    // (the pixel count passes through an empty asm: the reciprocal the wrap's `%` needs is then formed here, per
    // item, instead of being hoisted out of the item loop and held -- spilled, in the multi-tile instantiations --
    // through the component loop)
    int npixW = a.npix;
    asm volatile("" : "+s"(npixW));
#pragma unroll
    for (int j = 0; j < kPpt; ++j) {
        int e = ext0 + tid + j * kBlock;
        if (!selfHalo && (e < 0 || e >= a.npix)) {          // (self-halo: nu is padded to the thread count)
            if (kZeroPad) e = 0;                             // jnp.convolve 'same' zero padding (:674)
            else { e %= npixW; if (e < 0) e += npixW; }      // astropy boundary='wrap'
        }
        L.nu[j] = a.nu[e];
    }
    L.nuNode = 0.0;
    L.tileMask = 0;
    if (kFarInterp && selfHalo && !kInline) {
        // segment masks from the set-up (eval_line<true>): the wave holds the nodes of the ADJACENT segments 8 wv .. 8 wv + 7,
        // and which of them are interpolated comes with each line
        const int wv = tid >> 6, ln = tid & 63;
        L.nuNode = a.nu[kBlock * wv + 64 * (ln >> 3) + interp_node(ln)];
    } else if (kFarInterp) {
        const int wv = tid >> 6, ln = tid & 63;
        int e = ext0 + 64 * wv + kBlock * (ln >> 3) + interp_node(ln);
        if (!selfHalo && (e < 0 || e >= a.npix)) { e %= npixW; if (e < 0) e += npixW; }   // such segments are never interpolated
        L.nuNode = a.nu[e];
        L.tileMask = a.segok[g.tileIdx];                                       // bit m = segment m = wave + 8 j
    }
}

// The arguments of the kernel, read afresh from the kernel-argument segment (through a pointer the compiler cannot see
// through): their live ranges then start at the call.  The streaming launch calls it between its set-up phase and its item
// loop -- with one set of values alive across both phases the set-up's scalar-register pressure spilled the loop's
// arguments for their whole life (183 scalar spills, ~500 more v_readlane reloads on every item's path) -- and the resident
// kernel for every request (kept alive across the waiting loop they cost the item 150 scalar spills).
// (a typed copy out of the constant address space: pointers loaded from there are known to be global, so the loop
// keeps its global_load / global_atomic instructions -- copied word by word they became generic pointers, and a
// FLAT load also counts as an LDS operation: every LDS wait of the loop then waited for HBM)
__device__ __forceinline__ KArgs fresh_kargs() {
    typedef __attribute__((address_space(4))) const KArgs ArgSeg;
    ArgSeg* kp = (ArgSeg*)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(kp));
    return *(const KArgs*)kp;                            // (an aggregate copy: the compiler splits it into scalar loads of typed fields)
}

// ---- ticket hand-over: take, resolve, publish --------------------------------------------------------------------------
// The queue a workgroup takes its tickets from.  Streaming launch: this workgroup's XCD, whose queue hands out LOCAL
// tickets over the XCD's own live points.
struct ItemQueue {
    unsigned int* queue;
    int xcd, nItems;
    // tickets the grid's workgroups start with (the queue continues behind them); the workgroups of a streaming launch
    // -- whose set-up phase is over: see the kernel -- all start from their XCD's queue
    int firstTickets;
};
template <bool kStream>
__device__ __forceinline__ ItemQueue item_queue(const KArgs& a) {
    ItemQueue q;
    q.xcd = kStream ? xcd_id() : 0;
    q.nItems = kStream ? stream_rows_of(a.nrows, q.xcd, kXcds) * a.ntiles : a.nitems;
    q.queue = kStream ? &a.sctl->queue[q.xcd] : a.queue;
    q.firstTickets = kStream ? 0 : (int)gridDim.x;
    return q;
}
// ticket -> work item.  Streaming launch: local ticket t of the XCD = tile (t % ntiles) of its local live point t / ntiles
template <bool kOrdered, bool kStream>
__device__ __forceinline__ int item_of(const KArgs& a, const ItemQueue& q, int t) {
    if (kStream) { const int j = t / a.ntiles; return stream_row(q.xcd, j, kXcds) * a.ntiles + (t - j * a.ntiles); }
    return (kOrdered && a.order) ? a.order[t] : t;
}

// The first item of a workgroup; false (streaming launch, workgroup-uniform): nothing left for a late-comer.
template <bool kOrdered, bool kStream>
__device__ __forceinline__ bool first_item(const KArgs& a, const ItemQueue& q, const ItemSmem& lds, int tid0, int& w) {
    if (kStream) {
        if (tid0 == 0) lds.sNext[0] = (int)atomicAdd(q.queue, 1u);
        __syncthreads();
        const int t = lds.sNext[0];
        __syncthreads();
        if (t >= q.nItems) return false;
        w = item_of<kOrdered, kStream>(a, q, t);
        stream_wait_ready(a, w / a.ntiles, 0u);
    } else {
        w = item_of<kOrdered, kStream>(a, q, (int)blockIdx.x);   // grid <= nItems
    }
    return true;
}

// What thread 0 holds of the next ticket between take_ticket and publish_ticket (ONE value at a time through the loop).
struct HeldTicket {
    int wHeld = 0;
    unsigned stHeld = 0u, tRaw = 0u;
};

// Ticket of the item after this one: the first comes from the grid, the rest from the queue.  With an
// ordered hand-out (single-tile instantiations) the ticket still has to be looked up in a.order -- a second
// memory round trip that depends on the first.  Only the atomic is issued here: wave 0 reaches the item's first
// barrier without waiting for its answer.  The look-up follows behind the component loop (resolve_ticket): the
// ticket goes to sNext there -- nobody has read sNext since the barrier behind the previous item's publish, and
// nobody will before this item's -- and the item it stands for is published behind the node interpolation and
// the exponentials, which cover its way from memory; thread 0 holds ONE value at a time through the loop.
// The tiled batch instantiations publish the ticket at once.
template <bool kDeferTicket>
__device__ __forceinline__ void take_ticket(const KArgs& a, const ItemQueue& q, const ItemSmem& lds, int tid, HeldTicket& held,
                                            double (&nu)[kPpt], double& nuNode) {
    if (kDeferTicket) {
        // The frequencies are waited for HERE, with everything else request_item loaded: answers come back in the
        // order of issue and are counted that way, so a wait for a frequency behind the atomic -- in the first line
        // of the component loop -- would be a wait for the atomic's answer too.
        asm volatile("" : "+v"(nuNode));
#pragma unroll
        for (int j = 0; j < kPpt; ++j) asm volatile("" : "+v"(nu[j]));
    }
    if (tid == 0) {
        if (kDeferTicket) {
            // (the queue is addressed through an offset of 0 that the compiler takes for a per-lane value.  For an
            // atomic on a wave-uniform address it counts the active lanes, lets one lane add the count and hands
            // every lane its share behind a wait for the answer, right here -- for the one lane that takes a ticket)
            int qoff = 0;
            asm volatile("" : "+v"(qoff));
            if (a.persist) held.tRaw = atomicAdd(q.queue + qoff, 1u);
        } else {
            const int tHeld = a.persist ? q.firstTickets + (int)atomicAdd(q.queue, 1u) : q.nItems;
            lds.sNext[0] = tHeld; lds.sNext[1] = tHeld;
        }
    }
}
template <bool kOrdered, bool kStream>
__device__ __forceinline__ void resolve_ticket(const KArgs& a, const ItemQueue& q, const ItemSmem& lds, int tid, HeldTicket& held) {
    // (the first use of the atomic's answer stays here -- in EVERY wave: the wait for it then stands ahead of the
    // branch, where it costs the other waves nothing; inside, they would meet it where the register is next
    // written, behind the look-up's load, which the in-order counter would make wave 0 wait for as well)
    asm volatile("" : "+v"(held.tRaw));
    if (tid == 0) {
        const int tHeld = a.persist ? q.firstTickets + (int)held.tRaw : q.nItems;
        lds.sNext[0] = tHeld;
        held.wHeld = (tHeld < q.nItems) ? item_of<kOrdered, kStream>(a, q, tHeld) : 0;
        // (streaming launch: thread 0 also takes a first look at the next row's stamp -- the answer lands while
        // the rest of the component loop runs and travels to the workgroup with the ticket)
        if (kStream && tHeld < q.nItems)
            held.stHeld = __hip_atomic_load(a.ready + held.wHeld / a.ntiles, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}
template <bool kStream>
__device__ __forceinline__ void publish_ticket(const ItemSmem& lds, int tid, const HeldTicket& held) {
    if (tid == 0) { lds.sNext[1] = held.wHeld; if (kStream) lds.sNext[2] = (int)held.stHeld; }   // (sNext[0]: resolve_ticket)
}
// Behind the barrier that follows the publish: the next ticket, and the work item it stands for.
__device__ __forceinline__ void read_ticket(const ItemSmem& lds, int& tNext, int& wNext) {
    tNext = __builtin_amdgcn_readfirstlane(lds.sNext[0]);
    wNext = __builtin_amdgcn_readfirstlane(lds.sNext[1]);
}

// ---- 1. stage the item: ItemLoads into LDS, header into scalars ------------------------------------------------------
// The per-sample set-up comes from mcalf_sample_kernel (or the streaming set-up phase): header, records, taps.  The copy of
// the loads into LDS is written out in fused_items (see there); these are the pieces around it.
// The thread's pixel frequencies, and its optical depths at their start.
template <bool kZeroPad, bool selfHalo>
__device__ __forceinline__ void start_pixels(const KArgs& a, const ItemGeom& g, int tid, const ItemLoads& L, double (&nu)[kPpt],
                                             double (&tau)[kPpt]) {
#pragma unroll
    for (int j = 0; j < kPpt; ++j) {
        const int idx = tid + j * kBlock;
        const int e = g.ext0 + idx;
        const bool zero = kZeroPad && !selfHalo && (e < 0 || e >= a.npix);
        nu[j] = L.nu[j];
        tau[j] = (zero && idx < g.extCount) ? INFINITY : 0.0;  // exp(-inf) = 0
    }
}
// far-wing interpolation state: the wave's interpolable segments (bit 8 j: segment wave + 8 j)
template <bool kPreMask>
__device__ __forceinline__ unsigned long long wave_segments(int tid, unsigned long long tileMask) {
    unsigned long long segOk = 0;
    if (kFarInterp && !kPreMask) {                    // (kPreMask: the mask words have it folded in)
        const int wv = tid >> 6;
#pragma unroll
        for (int j = 0; j < kPpt; ++j) segOk |= ((tileMask >> (wv + 8 * j)) & 1ULL) << (8 * j);
        segOk = uniform64(segOk);
    }
    return segOk;
}
__device__ __forceinline__ SampleHdr* inline_header_slot(const ItemSmem& lds) {
    static_assert(sizeof(SampleHdr) <= kWaves * sizeof(double), "header fits the scratch slot");
    return reinterpret_cast<SampleHdr*>(lds.sRed + 2 * kWaves);   // (one-launch variant; the slot is scratch until the reduction)
}
// The header as the item uses it, behind the item's first barrier.
struct ItemHdr {
    double cont, bot;
    int ncl, n, ngeneral;
    bool bad;
};
template <bool kInline, bool kStream>
__device__ __forceinline__ ItemHdr item_header(const KArgs& a, const ItemSmem& lds, SampleHdr hd) {
    if (kInline) hd = *inline_header_slot(lds);
    ItemHdr h;
    // (streaming instantiations: continuum and tap sum are the same in every lane -- say so, and they ride through the
    // component loop in scalar registers; as vector values the tiled instantiation spilled them to scratch.  The batch
    // instantiations are left as they were: their register allocation is what was measured.)
    h.cont = kStream ? __builtin_bit_cast(double, uniform64(__builtin_bit_cast(unsigned long long, hd.cont))) : hd.cont;
    h.bot = kStream ? __builtin_bit_cast(double, uniform64(__builtin_bit_cast(unsigned long long, hd.bot))) : hd.bot;
    // (streaming launch: a wait that ran out may leave a header nobody wrote -- keep its counts inside the buffers)
    h.ncl = kStream ? min(max(hd.ncl, 0), a.ncl_cap) : hd.ncl;
    h.n = kStream ? min(max(hd.n, 0), a.n_cap) : hd.n;
    h.ngeneral = hd.ngeneral;
    h.bad = hd.bad != 0;
    return h;
}

// ---- 2. tau for this thread's pixels: fold a group of lines, the component loop -------------------------------------
// Fold the group of kLinesPerSync lines that starts at record cl0 into `tabs`: a thread folds ONE coefficient slot of each.
template <int kLinesPerSync>
__device__ __forceinline__ void fold_group(const ItemSmem& lds, double* tabs, int tid, int cl0, int ncl_run) {
    const bool hasCoef = tid < VT_NTOT;
    const int coefPos = tid + (tid >= VT_Z0_OFF ? 1 : 0) + (tid >= VT_ZF_OFF ? 1 : 0);
    const bool coreCoef = tid < VT_NCORE;
    if (hasCoef) {
        double Tn[VT_NY];
#pragma unroll
        for (int nn = 0; nn < VT_NY; ++nn) Tn[nn] = lds.sT[nn * VT_NTOT + tid];
        // No test per line: past the last record the last one is folded again into a slot nobody reads.
        // The group's Horner chains are written step by step ACROSS the lines, so that they issue
        // interleaved (the fold sits on every wave's path to the barrier; chain after chain it is bound by
        // the latency of 6 dependent FMAs per line).
        double fy[kLinesPerSync], fs[kLinesPerSync], fc[kLinesPerSync];
#pragma unroll
        for (int l = 0; l < kLinesPerSync; ++l) {
            const double* rec = lds.sRec + min(cl0 + l, ncl_run - 1) * kRecStride;
            fy[l] = rec[3];
            fs[l] = coreCoef ? rec[4] : rec[5];
            fc[l] = Tn[VT_NY - 1];
        }
#pragma unroll
        for (int nn = VT_NY - 2; nn >= 0; --nn) {
#pragma unroll
            for (int l = 0; l < kLinesPerSync; ++l) fc[l] = fma(fc[l], fy[l], Tn[nn]);
            __builtin_amdgcn_sched_barrier(0);
        }
#pragma unroll
        for (int l = 0; l < kLinesPerSync; ++l) tabs[l * kTabPad + coefPos] = fc[l] * fs[l];   // = fold_coef()
    } else if (tid >= kBlock - 64 && tid < kBlock - 64 + 3) {
        // the last wave folds nothing: three of its lanes copy each line's [uthr, A, B] behind its coefficients
        // (kPreMask: slot 7 of the record holds the line's segment-mask word instead -- copied as the 8 bytes it is)
        const int which = tid - (kBlock - 64);                                 // 0: uthr / mask word, 1: A, 2: B
        const int src = (which == 0) ? 7 : which - 1;
#pragma unroll
        for (int l = 0; l < kLinesPerSync; ++l)
            tabs[l * kTabPad + kLineLds + which] = lds.sRec[min(cl0 + l, ncl_run - 1) * kRecStride + src];
    }
}

// The component loop: every (component, line) of the sample added to the thread's optical depths, then the lines of the
// general path.  Returns the half of the double-buffered tables that the last group of lines did NOT use.
template <int kLinesPerSync, bool kPreMask>
__device__ __forceinline__ int component_loop(const ItemSmem& lds, int tid, const ItemHdr& h, const double (&nu)[kPpt], double (&tau)[kPpt],
                                              double nuNode, double& farNode, unsigned long long segOk, int wvU) {
    int buf = 0;
    const int ncl_run = h.ncl;
    // kLinesPerSync lines are folded per workgroup barrier (their tables are double-buffered), which
    // halves the barriers and averages the per-wave core/wing imbalance over more work.
    for (int cl0 = 0; cl0 < ncl_run; cl0 += kLinesPerSync) {
        // Wave priority falls as the workgroup progresses, so of the two workgroups sharing a CU the one
        // that is behind gets the issue slots (measured -3.5 % at config B).
        if (4 * cl0 < ncl_run) __builtin_amdgcn_s_setprio(3);
        else if (4 * cl0 < 2 * ncl_run) __builtin_amdgcn_s_setprio(2);
        else if (4 * cl0 < 3 * ncl_run) __builtin_amdgcn_s_setprio(1);
        else __builtin_amdgcn_s_setprio(0);
        double* tabs = lds.sTab + buf * (kLinesPerSync * kTabPad);
        fold_group<kLinesPerSync>(lds, tabs, tid, cl0, ncl_run);
        __syncthreads();
        buf ^= 1;
        // one copy of the (large) per-line body: keeps the loop inside the instruction cache
        const int lmax = __builtin_amdgcn_readfirstlane(min(kLinesPerSync, ncl_run - cl0));   // (kept scalar)
#pragma unroll 1
        for (int l = 0; l < lmax; ++l) eval_line<kPreMask>(tabs + l * kTabPad, nu, tau, nuNode, farNode, segOk, wvU);
    }
    if (h.ngeneral > 0 && ncl_run > 0) eval_general_lines(lds.sRec, h.ncl, nu, tau);
    __builtin_amdgcn_s_setprio(0);
    return buf;
}

// ---- flux to tile: node interpolation, exp_neg, body and halo stores -------------------------------------------------
// Interpolate the far-wing node sums to the pixels (tau[j] += sum_k W[lane][k] F[segment j][node k]),
// then flux = exp(-tau) into the LDS tile.  The node sums travel through the (now dead) folded-table
// region, one 64-entry row per wave; the tile holds only the sample's own halo n (<= n_cap).
// kPreMask: the sums of pixel wave w's slot j (segment w + 8 j) are held by NODE wave j, lanes 8 w .. 8 w + 7, so
// they cross waves.  They are stored AHEAD of the barrier, into the half of the double-buffered tables that the
// last group of lines did not use (`buf` by now): nobody has read it since the barrier of that group, which
// every wave passed after its last read of it.
template <bool kZeroPad, bool selfHalo, int kLinesPerSync, bool kPreMask>
__device__ __forceinline__ void flux_to_tile(const KArgs& a, const ItemSmem& lds, const ItemGeom& g, int tid, int n, int buf,
                                             const double (&tau)[kPpt], double farNode) {
    const int shift = a.n_cap - n;
    double wrow[VT_INODES];
    double* sFar = kPreMask ? lds.sTab + buf * (kLinesPerSync * kTabPad) + 8 * (tid >> 6) : lds.sTab + (tid >> 6) * 64;
    constexpr int kFarSlot = kPreMask ? 64 : 8;        // doubles between the node sums of a wave's consecutive pixel slots
    if (kFarInterp) {
        if (kPreMask) lds.sTab[buf * (kLinesPerSync * kTabPad) + tid] = farNode;
        __syncthreads();                               // every wave is done reading the folded tables
        if (!kPreMask) sFar[tid & 63] = farNode;
#pragma unroll
        for (int k = 0; k < VT_INODES; ++k) wrow[k] = lds.sWt[k * 64 + (tid & 63)];
    }
    const int extTight = g.tlen + 2 * n;
    // Tile positions of this thread's pixels: a step of kBlock pixels (a multiple of 8) moves an element by
    // kBlock / 8 slots inside its plane, so ONE position per destination (body, low halo copy, high halo copy)
    // serves all eight pixels as base + 64 j.
    const int posBody = tile_pos(selfHalo ? tid + n : tid - shift);
    const int posLow = tile_pos(tid + n + a.npix), posHigh = tile_pos(tid + n - a.npix);   // (self-halo copies)
    static_assert(kBlock % 8 == 0, "tile_pos(i + kBlock) == tile_pos(i) + kBlock / 8");
    // Two pixels per round: their interpolation sums and exponentials are independent chains the scheduler
    // interleaves (one pixel at a time the phase is bound by the latency of a single ~35-instruction chain).
    // The fences keep it at two: without them the compiler issues the node sums of all eight segments at
    // once and spills them.
    static_assert(kPpt % 2 == 0, "pixels are processed in pairs");
#pragma unroll
    for (int j0 = 0; j0 < kPpt; j0 += 2) {
        double fl[2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = j0 + jj;
            double tj = tau[j];
            if (kFarInterp) {
                double add = 0.0;
#pragma unroll
                for (int k = 0; k < VT_INODES; ++k) add = fma(wrow[k], sFar[kFarSlot * j + k], add);
                tj += add;
            }
            fl[jj] = exp_neg(tj);                      // :377 (product of exp == exp of sum)
        }
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int j = j0 + jj;
            if (selfHalo) {
                const int p = tid + j * kBlock;        // pixel index; tile layout [n halo | npix body | n halo]
                if (p < a.npix) {
                    lds.sF[posBody + (kBlock / 8) * j] = fl[jj];
                    // periodic copies (astropy boundary='wrap'); the JAX path pads with zeros instead (:674).
                    // Only the first / last pixel groups can hold halo pixels: a scalar test skips the rest.
                    if (j * kBlock < n && p < n) lds.sF[posLow + (kBlock / 8) * j] = kZeroPad ? 0.0 : fl[jj];
                    if ((j + 1) * kBlock > a.npix - n && p >= a.npix - n) lds.sF[posHigh + (kBlock / 8) * j] = kZeroPad ? 0.0 : fl[jj];
                }
            } else {
                const int pos = tid + j * kBlock - shift;
                if (pos >= 0 && pos < extTight) lds.sF[posBody + (kBlock / 8) * j] = fl[jj];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        asm volatile("" ::: "memory");
    }
    if (tid < kTileSlack) {
        double zero = 0.0;
        asm volatile("" : "+v"(zero));                 // formed here: hoisted out of the item loop it was spilled
        lds.sF[tile_pos(extTight + tid)] = zero;
    }
}

// ---- 3. the LSF convolution ------------------------------------------------------------------------------------------
// One group of taps of the register sliding window, the ONE body of every variant: `weight(r)` is tap r of the group;
// a whole group has eight, the remainder `rem` < 8 (wave-uniform).  Per tap one new flux value is read from LDS for
// eight FMAs.
template <bool kWhole, class Weight>
__device__ __forceinline__ void tap_group(const double*& fp, double (&win)[8], double (&top)[8], int rem, Weight weight) {
    ++fp;
#pragma unroll
    for (int r = 0; r < (kWhole ? 8 : 7); ++r) {
        if (!kWhole && r >= rem) break;
        const double wgt = weight(r);
#pragma unroll
        for (int m = 0; m < 8; ++m) top[m] = fma(win[(m + r) & 7], wgt, top[m]);
        win[r] = fp[r * kPlaneStride];                 // element base + q0 + r + 8
    }
}
// Register sliding window: this thread owns outputs base..base+7 (top[]); per tap one new flux value
// and one (broadcast) weight are read for eight FMAs.  s: the live point (its tap row), n: its half-width.
template <bool kTapsScalar>
__device__ __forceinline__ void convolve_tile(const KArgs& a, const ItemSmem& lds, int tid, int s, int n, double (&top)[8]) {
    double win[8];
    const double* fp = lds.sF + tid;                   // element 8 tid + 8 c + r  ->  fp[r * kPlaneStride + c]
    const int ntaps = 2 * n + 1;
    const int rem = ntaps & 7;                         // the last 1..7 taps (2n+1 is odd): no zero-weight padding taps
    if constexpr (kTapsScalar) {
        // The weights are the same in every lane and every wave, and the set-up kernel has left the live point's
        // row in memory: a group of eight comes as ONE scalar load (sixteen dwords) and every FMA takes its weight
        // as the scalar operand.  Two register sets take turns, each group issuing the load of the one behind it,
        // so no weight is ever moved; the row holds 2 n_cap + 8 doubles and 2 n + 1 is odd, so the group behind a
        // whole one -- at least the remainder's -- always lies inside the row.
        const int su = __builtin_amdgcn_readfirstlane(s);
        const TapGroup* gw = (const TapGroup*)(a.taps + (a.taps_shared ? (size_t)0 : (size_t)su * tap_total(a)));
        TapGroupV wA = gw[0], wB;
#pragma unroll
        for (int m = 0; m < 8; ++m) { win[m] = fp[m * kPlaneStride]; top[m] = 0.0; }
        auto whole = [&](const TapGroupV& wg) {
            tap_group<true>(fp, win, top, 8, [&](int r) { return wg[r]; });
            // (a group's reads stay its own: issued among the FMAs of the group before, or merged with the next
            // group's into two-address reads, they held a second window of sixteen registers, which the kernel
            // does not have -- one to five spills.  Inside the group the scheduler is free: it sends the reads out
            // four at a time, into the registers of the values they replace)
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("" ::: "memory");
        };
        int groups = ntaps >> 3;                       // whole groups of eight taps
        // (the first group's weights are waited for HERE, with the window: left to the loop, the wait stands at the loop's
        // top, behind the load of the next group, and is taken on every trip -- scalar loads are counted out of order)
        asm volatile("" : : "s"(wA[0]));
        // (ONE exit, at the loop's top, and one copy of the remainder behind it: with a second exit between the halves,
        // with the odd group peeled off ahead of the loop or behind it, or with a remainder per register set, the
        // window and the sums were copied where the paths meet, or spilled: up to 77 registers to scratch)
        bool inB = false;                              // the remainder's weights: which set holds them
        for (; groups > 0; groups -= 2) {
            wB = *++gw;
            __builtin_amdgcn_sched_barrier(0);         // (the load goes out at the group's top, ahead of its reads)
            whole(wA);
            if (groups > 1) {
                wA = *++gw;
                __builtin_amdgcn_sched_barrier(0);
                whole(wB);
            } else {
                inB = true;
            }
        }
        const TapGroupV& wl = inB ? wB : wA;
        tap_group<false>(fp, win, top, rem, [&](int r) { return wl[r]; });
    } else {
#pragma unroll
        for (int m = 0; m < 8; ++m) { win[m] = fp[m * kPlaneStride]; top[m] = 0.0; }
        const double* wp = lds.sW;                     // the weights: broadcast reads from LDS
        for (int q0 = 0; q0 + 8 <= ntaps; q0 += 8) {   // whole groups of eight taps
            tap_group<true>(fp, win, top, 8, [&](int r) { return wp[r]; });
            wp += 8;
        }
        tap_group<false>(fp, win, top, rem, [&](int r) { return wp[r]; });
    }
}

// ---- 4. continuum and likelihood terms -------------------------------------------------------------------------------
// The data of a thread's 8 pixels, requested ahead of the convolution and consumed after it (the
// device arrays carry 8 doubles of padding, so the 64-byte reads never need a bounds test).  The loads
// are unconditional on purpose -- model-only calls simply ignore them: defined under `if (reduces)`
// the 24 values become phi(undef, load) ranges that the register allocator of the persistent loop
// spills one load at a time.
// (three arrays of the caller's, not one struct of arrays: with the struct the single-tile numpy batch instantiations
// came out one vector register short of what they were measured with)
__device__ __forceinline__ void load_pixel_data(const KArgs& a, size_t o0, double (&ob)[8], double (&is2)[8], double (&lg)[8]) {
#pragma unroll
    for (int m = 0; m < 8; ++m) { ob[m] = a.obj[o0 + m]; is2[m] = a.ispec2[o0 + m]; lg[m] = a.lgis[o0 + m]; }
}
// The sums a thread contributes to its item's result.
struct ItemSums {
    double acc, nnz, c4, c5;
};
// Model = convolution / tap sum x continuum for the thread's outputs base .. base + 7: its likelihood terms are returned, the
// model itself goes to a.model.
template <bool kZeroPad>
__device__ __forceinline__ ItemSums likelihood_terms(const KArgs& a, const ItemSmem& lds, const ItemGeom& g, const ItemHdr& h, int base,
                                                 bool reduces, const double (&top)[8], const double (&ob)[8], const double (&is2)[8], const double (&lg)[8]) {
    double acc = 0.0, nnz = 0.0, c4 = 0.0, c5 = 0.0;
    const int s = g.s, t0 = g.t0, tlen = g.tlen, n = h.n;
    const double cont = h.cont;
    const bool bad = h.bad;
    const size_t o0 = (size_t)(t0 + base);
    const double ibot = 1.0 / h.bot;
    // The plain log-likelihood (no model output, no asymmetric veto, numpy boundary) gets its own loop: in
    // the general one below every pixel drags the mode / veto / output tests along as selects and reloads
    // of spilled scalars (~30 vector instructions per pixel against ~12 here).  Same arithmetic, same order.
    const bool plainLogL = !kZeroPad && a.mode == kModeLogL && !a.asymm && a.model == nullptr;
    if (plainLogL) {
        if (!bad) {                                      // (bad: every term is NaN and is dropped)
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                double mval = top[m] * ibot;
                mval *= cont;                                                          // :447
                const double d = ob[m] - mval;
                double term = is2[m] * (d * d);
                term = (term - lg[m]) + a.log2pi;                                   // :294
                acc += (base + m < tlen && !isnan(term)) ? term : 0.0;             // np.nansum
            }
        }
    } else if (!kZeroPad && a.mode != kModeLogL && a.mode != kModeChi2 && a.model != nullptr) {
        // Model output alone (reconstruct_spec / reconstruct_onecomp for a batch, numpy boundary): eight
        // consecutive pixels per thread, 64 contiguous bytes, nothing else -- same arithmetic as above.
        double* mrow = a.model + (size_t)s * a.npix + t0 + base;
#pragma unroll
        for (int m = 0; m < 8; ++m) {
            double mval = top[m] * ibot;
            mval *= cont;                                                              // :447
            if (bad) mval = NAN;
            if (base + m < tlen) mrow[m] = mval;
        }
    } else
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        const int i = base + m;
        const bool live = i < tlen;
        const int pix = t0 + i;
        double mval = kZeroPad ? top[m] : top[m] * ibot;
        if (kZeroPad && (pix < n || pix >= a.npix - n)) mval = lds.sF[tile_pos(min(i, tlen - 1) + n)];   // :677-681 edge reset
        mval *= cont;                                                                  // :447 / :683
        if (bad) mval = NAN;
        if (a.model && live) a.model[(size_t)s * a.npix + pix] = mval;
        if (reduces) {
            const double d = ob[m] - mval;
            double term = is2[m] * (d * d);
            if (a.mode == kModeLogL) term = (term - lg[m]) + a.log2pi;              // :294
            if (live && !isnan(term)) acc += term;                                     // np.nansum
            if (a.mode == kModeChi2 && live && mval != 0.0) nnz += 1.0;      // only chi2 asks whether the model is all zero (:241)
            if (a.asymm) {                                                             // :298-302 (rare: loaded here)
                const double resid = d / a.err[o0 + m];
                if (live && resid > 4.0) c4 += 1.0;
                if (live && resid > 5.0) c5 += 1.0;
            }
        }
    }
    return ItemSums{acc, nnz, c4, c5};
}

// ---- 5. reduction and result store -----------------------------------------------------------------------------------
// The workgroup's sums in fixed order (deterministic), and the item's result -- or, for a tiled spectrum, its partial --
// written by thread 0.  Ends the item: behind its barrier every wave is past its reads of the flux tile and the taps.
template <bool kInline, bool kStream>
__device__ __forceinline__ void reduce_and_store(const KArgs& a, const ItemSmem& lds, const ItemGeom& g, int tid, bool reduces, bool bad,
                                                 ItemSums sum) {
    if (reduces) {
        sum.acc = wave_sum_to_last(sum.acc);
        if (a.mode == kModeChi2) sum.nnz = wave_sum_to_last(sum.nnz);
        const int wave = tid >> 6;
        if ((tid & 63) == 63) { lds.sRed[wave] = sum.acc; lds.sRed[kWaves + wave] = sum.nnz; }
    }
    double t4 = 0.0, t5 = 0.0;
    if (reduces && a.asymm) {                        // rare path: two more workgroup sums
        __syncthreads();
        t4 = block_sum(sum.c4, lds.sRed + 2 * kWaves, tid);
        t5 = block_sum(sum.c5, lds.sRed + 2 * kWaves, tid);
    }
    __syncthreads();                                 // every wave is past its reads of the flux tile and the taps
    if (reduces && tid == 0) {
        double ssum = 0.0, scnt = 0.0;
#pragma unroll
        for (int wv = 0; wv < kWaves; ++wv) { ssum += lds.sRed[wv]; scnt += lds.sRed[kWaves + wv]; }
        // LSF wider than the provisioned halo: the model was not computed (the reference would build a longer
        // kernel); the row must not look like a valid likelihood -> logL = -inf, chi2 = +inf
        if (bad) { ssum = INFINITY; scnt = 1.0; }
        if (a.ntiles == 1) {
            const double val = finalize_value(a.mode, ssum, scnt, a.asymm != 0, t4, t5, a.veto4, a.veto5);
            // (streaming launch: the result goes to page-locked host memory and the host reads it as soon as the
            // launch's completion word says so, ahead of the end-of-kernel cache write-back: a system-scope store,
            // written through -- plain stores were seen to linger in one XCD's L2 past the completion word)
            // (one-launch variant: its results go to page-locked memory too, and the host -- or, for the resident
            // kernel, the next request -- reads them while the kernel is still there)
            if (kStream || kInline) __hip_atomic_store(a.out + g.s, val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            else a.out[g.s] = val;
        } else {
            double* pr = a.partial + ((size_t)g.s * a.ntiles + g.tileIdx) * 4;
            pr[0] = ssum; pr[1] = scnt; pr[2] = t4; pr[3] = t5;
        }
    }
}

// ---- the item loop -----------------------------------------------------------------------------------------------------
// PERSISTENT kernel: the grid is the number of workgroup slots of the chip (2 per CU), and every workgroup walks
// over work items w = (live point, pixel tile): its first item is blockIdx.x, the following ones come from an
// atomic queue (a.queue, reset by the set-up kernel of the same launch), so that fast and slow samples balance
// out.  Per item nothing is re-launched: the next item's records / taps / table slices / frequencies are
// requested before the likelihood terms of the current one and written to LDS behind the barrier that ends it.
// Every wave leaves the item loop at the same item count (the queue value is broadcast through LDS), so no wave
// is ever left behind a barrier.
// kInline (small calls -- the one-theta-at-a-time solvers): there is no set-up kernel; wave 0 of the workgroup runs
// setup_sample() for its live point straight into LDS (one launch instead of two on a latency-bound path; every tile of
// a tiled spectrum repeats the set-up, which costs nothing when the chip is empty).
// kStream (the host-pointer entries' large batches): ONE launch for the whole call, no set-up kernel, no copy command.
// The grid sets the live points up itself (stream_setup_phase) while the parameter rows are still arriving in the
// page-locked block the kernel reads them from, and an item goes to the component loop once its row's stamp is there.
template <bool kZeroPad, bool kSelfHalo, int kLinesPerSync, bool kInline, bool kStream>
__device__ __forceinline__ void fused_items(const KArgs& a, double* smem) {
    typedef ItemFlags<kSelfHalo, kInline, kStream> F;
    const ItemSmem lds = carve_item_lds<kLinesPerSync>(a, smem);
    const int tid0 = threadIdx.x;
    if (kFarInterp) lds.sWt[(tid0 & 7) * 64 + (tid0 >> 3)] = a.wtab[tid0];      // kBlock == 64 * VT_INODES
    const ItemQueue q = item_queue<kStream>(a);
    int w;
    if (!first_item<F::kOrdered, kStream>(a, q, lds, tid0, w)) {
        stream_exit(a, tid0);
        return;
    }
    ItemLoads L;
    request_item<kZeroPad, kSelfHalo, kInline, kStream>(a, w, tid0, L);

    while (true) {
        // Per item the thread index passes through an empty asm: everything derived from it (LDS offsets, tile
        // positions, global addresses -- dozens of registers) is then formed where it is used instead of being
        // hoisted out of the item loop and kept alive through the component loop, which sits at the kernel's
        // 128-register limit.
        int tid = tid0;
        asm volatile("" : "+v"(tid));
        const ItemGeom g = item_geom<kSelfHalo>(a, w);

        // ---- 1. stage the item; take the next ticket ---------------------------------------------------------------
        double nu[kPpt], tau[kPpt];
        start_pixels<kZeroPad, kSelfHalo>(a, g, tid, L, nu, tau);
        double nuNode = L.nuNode;                          // this lane's node pixel
        double farNode = 0.0;
        const unsigned long long segOk = wave_segments<F::kPreMask>(tid, L.tileMask);
        const int wvU = F::kPreMask ? __builtin_amdgcn_readfirstlane(tid >> 6) : 0;   // the wave's index, as a scalar
        SampleHdr hd;
        // ItemLoads into LDS, the header's counts into scalars.  (This phase stays inline: as a function of its own, the
        // compiler merged the record stores' blocks and put a wait for ALL of the item's loads ahead of them -- the tiled
        // batch instantiation was 0.3 % slower at config E, more than the run-to-run spread.)
        const int recTotal = rec_total(a), tapTotal = tap_total(a);
        if (kInline) {
            if (tid < 64) setup_sample<kZeroPad>(a, g.s, tid, lds.sRec, lds.sW, true, inline_header_slot(lds), g.tileIdx == 0, false);
        } else {
            hd = L.hd;
            // The header's counts are the same in every lane, and the compiler knows it: left alone it reads them back into
            // scalar registers right behind the load -- every wave then waits in request_item for a full memory round
            // trip, with the record, tap and frequency loads not yet issued.  Through an empty asm they stay vector
            // values up to here, the top of the item that uses them, where the loads are drained anyway.
            asm volatile("" : "+v"(hd.ncl), "+v"(hd.n), "+v"(hd.bad), "+v"(hd.ngeneral));
            hd.ncl = __builtin_amdgcn_readfirstlane(hd.ncl);
            hd.n = __builtin_amdgcn_readfirstlane(hd.n);
            hd.bad = __builtin_amdgcn_readfirstlane(hd.bad);
            hd.ngeneral = __builtin_amdgcn_readfirstlane(hd.ngeneral);
#pragma unroll
            for (int i = 0; i < kRecRegs; ++i)
                if (tid + i * kBlock < recTotal) lds.sRec[tid + i * kBlock] = L.rreg[i];
            if (recTotal > kRecRegs * kBlock) {
                const double* gr = a.recs + (size_t)g.s * (kStream ? a.rec_stride : recTotal);
                for (int i = tid + kRecRegs * kBlock; i < recTotal; i += kBlock) lds.sRec[i] = gr[i];
            }
            if (kStream && tid < tapTotal) lds.sW[tid] = L.tapreg;
            if (kStream && tapTotal > kBlock) {
                const double* gt = a.taps + (size_t)g.s * a.tap_stride;
                for (int i = tid + kBlock; i < tapTotal; i += kBlock) lds.sW[i] = gt[i];
            }
        }
#pragma unroll
        for (int i = 0; i < kTRegs; ++i) {
            const int idx = tid + i * kBlock;
            if (idx < VT_NY * VT_NTOT) lds.sT[idx] = L.treg[i];
        }
        HeldTicket held;
        take_ticket<F::kDeferTicket>(a, q, lds, tid, held, nu, nuNode);
        __syncthreads();                                   // publishes sRec, sW, sT, sNext (and the header of the one-launch variant)
        const ItemHdr h = item_header<kInline, kStream>(a, lds, hd);
        int tNext = 0, wNext = 0;
        if (!F::kDeferTicket) read_ticket(lds, tNext, wNext);

        // ---- 2. tau for this thread's pixels; resolve the ticket ----------------------------------------------------
        const int buf = component_loop<kLinesPerSync, F::kPreMask>(lds, tid, h, nu, tau, nuNode, farNode, segOk, wvU);
        // (behind the loop, not inside it: a loop that loads from memory and reads a register loaded ahead of it gets a
        // full drain in front of its first iteration -- wave 0 would wait for the atomic right behind the first barrier)
        if (F::kDeferTicket) resolve_ticket<F::kOrdered, kStream>(a, q, lds, tid, held);
        flux_to_tile<kZeroPad, kSelfHalo, kLinesPerSync, F::kPreMask>(a, lds, g, tid, h.n, buf, tau, farNode);
        if (F::kDeferTicket) publish_ticket<kStream>(lds, tid, held);
        __syncthreads();                                   // publishes the flux tile (and the deferred ticket)
        if (F::kDeferTicket) read_ticket(lds, tNext, wNext);
        // Streaming launch: thread 0's look at the next row's stamp (taken while the component loop ran; the set-up runs
        // far ahead of the queue, so it normally says "set up" and nobody has to ask memory again)
        unsigned stampNext = 0u;
        if (kStream) stampNext = (unsigned)__builtin_amdgcn_readfirstlane(lds.sNext[2]);

        // ---- 3+4. convolution, continuum, likelihood terms ----------------------------------------------------------
        ItemSums sum = {0.0, 0.0, 0.0, 0.0};
        const int base = 8 * tid;                          // this thread owns outputs base .. base + 7
        const bool reduces = (a.mode == kModeLogL || a.mode == kModeChi2);
        if (base < g.tlen) {
            double ob[8], is2[8], lg[8];
            load_pixel_data(a, (size_t)(g.t0 + base), ob, is2, lg);
            double top[8];
            convolve_tile<F::kTapsScalar>(a, lds, tid, g.s, h.n, top);
            sum = likelihood_terms<kZeroPad>(a, lds, g, h, base, reduces, top, ob, is2, lg);
        }

        // ---- request the next item ----------------------------------------------------------------------------------
        const bool more = tNext < q.nItems;
        // The next item's global loads go out here (the pixel data of this item are consumed, so the registers
        // are free): they land while the reduction and the barrier that ends the item run.
        __builtin_amdgcn_sched_barrier(0);
        // (unconditional -- the last item of a workgroup re-requests a valid item it never uses -- so that the
        // loads REDEFINE every register of L: behind a condition the old values would have to stay alive through
        // the whole item for the merge)
        if (kStream && more) stream_wait_ready(a, wNext / a.ntiles, stampNext);
        if (!kInline) request_item<kZeroPad, kSelfHalo, kInline, kStream>(a, more ? wNext : w, tid, L);   // (one-launch variant: one item per workgroup)
        __builtin_amdgcn_sched_barrier(0);

        // ---- 5. reduction and result store --------------------------------------------------------------------------
        reduce_and_store<kInline, kStream>(a, lds, g, tid, reduces, h.bad, sum);
        if (kInline || !more) break;                     // wave-uniform: every wave of the workgroup leaves here
        w = wNext;
    }
    if (kStream) stream_exit(a, tid0);
}

}  // namespace mcalf
