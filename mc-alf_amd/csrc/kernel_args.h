// What the device code (kernels.hip) and the host side of libmcalf_hip.so (host_abi.cpp, host_stream.cpp, broker.cpp,
// comm.cpp) share: the launch geometry, the kernel-argument block, the words a streaming or resident launch exchanges
// with the host, and the table of kernel entry points the host launches through hipLaunchKernel.  Plain C++ -- the
// host files are compiled without the HIP language mode.  Part of the kernel-source hash (mc-alf_amd/build.py): a
// change of a layout here changes what the device code does.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "voigt_tables.h"

namespace mcalf {

constexpr int kBlock = 512;
constexpr int kPpt = 8;                 // pixels per thread: (tile + halo) <= kBlock * kPpt
constexpr int kExtMax = kBlock * kPpt;  // 4096 pixels = 32 KiB of LDS
constexpr int kWaves = kBlock / 64;
constexpr int kRecStride = 8;           // doubles per (component,line) record in LDS
constexpr int kTabPad = VT_NTOT + 7;    // folded table in LDS: zone0 / zoneF shifted to stay 16-B aligned, then uthr, A, B
constexpr int kZ0Lds = VT_Z0_OFF + 1;
constexpr int kZFLds = VT_ZF_OFF + 2;
constexpr int kLineLds = kZFLds + VT_FDEG + 1;   // [uthr, A, B] of the line, right behind its zone-F coefficients: the
                                                 // node pass reads all ten doubles off ONE base address (5 x ds_read_b128).
                                                 // Single-tile contexts behind a set-up: [W, A, B], W the line's 64-bit
                                                 // segment-mask word (bit 8 i + v: segment 8 v + i is interpolated), which
                                                 // the set-up leaves in slot 7 of the record in place of uthr
static_assert(kLineLds + 3 <= kTabPad && (kLineLds % 2) == 1, "line constants pair up with the last zone-F coefficient");
// Lines folded per workgroup barrier of the component loop: 4 or 5, chosen per context (whichever needs fewer
// barriers for the context's largest line count; measured on MI355X: config C, 20-24 lines, -0.8 % with 5;
// config E, 16 lines, +1.3 % with 5).  The fused kernel is instantiated for both (fused_kernel_ptr).
static_assert(kBlock == 64 * VT_INODES, "one interpolation weight per thread");
static_assert(kPpt == 8, "the skip tests of eval_line treat the eight segments of a wave as two halves");
static_assert(VT_NTOT <= kBlock - 64 && (kZ0Lds % 2) == 0 && (kZFLds % 2) == 0 && (kTabPad % 2) == 0, "LDS table layout");
constexpr int kRedDoubles = 3 * kWaves + 2;   // per-wave partials (sum, count, scratch) + the next work-item index
constexpr int kTileSlack = 16;           // zero-filled entries past the halo (sliding-window over-read)
constexpr size_t kLdsBudget = 78 * 1024;   // two workgroups per CU (160 KiB); needs the MaxDynamicSharedMemorySize attribute
constexpr bool kFarInterp = true;          // far wings at 8 nodes per 64-pixel segment (tools/interp_check.py builds the other variant)
constexpr double kInterpC = 1.0e-3;        // interpolation error <= kInterpC (du/u0)^8 (measured 4.4e-4, tools/ + DESIGN.md)
constexpr double kInterpTol = 1.0e-15;     // allowed optical-depth error per (line, pixel) from the interpolation
constexpr double kCcgs = 2.9979245e10;  // hires_fitter.py:66
constexpr double kFwhmToSigma = 2.354820;   // hires_fitter.py:454
constexpr double kKernelReach = 3.0348;     // hires_fitter.py:458
constexpr double kTauConst = 0.014971475;   // hires_fitter.py:364

enum Mode : int { kModeLogL = 0, kModeModel = 1, kModeChi2 = 2, kModeOneComp = 3 };

struct LineDev {
    double wrest_cm;  // wrest/1e8                 hires_fitter.py:376
    double f;
    double gamma4pi;  // gamma / (4 pi)            hires_fitter.py:361 (a = gamma4pi / dnu)
    double nujk;      // ccgs / wrest_cm           hires_fitter.py:359
};

// Per-sample set-up, one wave per live point: decode, (component,line) records, LSF taps.  Runs once per
// sample ahead of the fused kernel (whose workgroups -- several per sample when the spectrum is tiled --
// then start with plain coalesced loads instead of a chain of dependent loads and libm calls).
struct SampleHdr {
    double cont;     // continuum
    double bot;      // tap sum astropy's loop divides by (1 on the JAX path)
    int ncl;         // records in use
    int n;           // LSF half-width of this sample
    int bad;         // LSF wider than the provisioned halo
    int ngeneral;    // records that need the general Voigt path
};

struct KArgs {
    const double* nu;       // [npix] ccgs / (wl/1e8): pixel frequency at z = 0
    const double* obj;      // [npix]
    const double* ispec2;   // [npix] 1/err^2
    const double* lgis;     // [npix] log(ispec2)
    const double* err;      // [npix] obj_noise (asymmetric veto only)
    const double* P;        // [batch][ndim]  (mode OneComp: [batch][5])
    double* partial;        // [batch][ntiles][4]  (sum, nonzero-count, #resid>4, #resid>5)
    double* out;            // logL / chi2 [batch]   (written directly when ntiles == 1)
    double* model;          // [batch][npix] or nullptr
    const LineDev* lines;   // [nlines] then the filler line at [nlines]
    const double* tabs;     // T[VT_NY][VT_NTOT]
    double* recs;           // [batch][ncl_cap][8] records written by the sample kernel
    double* taps;           // [batch][2 n_cap + 8] normalised LSF taps, zero padded
    SampleHdr* hdr;         // [batch]
    const double* wtab;     // [64][8] Lagrange weights of the far-wing interpolation
    const unsigned long long* segok;   // [ntiles] bit m: 64-pixel segment m of the tile may be interpolated
    int npix, ndim, ntiles, tile, n_cap, ncl_cap;
    int nlines, ncompmax, nfill, startind, endind, freespecres, freecont;
    int targonly, mode, jax_half, onecomp_fill, asymm;
    int taps_shared;        // 1: fixed resolution -> every live point has the same LSF taps, stored once (row 0)
    int selfhalo;           // 1: single-tile spectrum whose halo entries are copies of the tile's own pixels (see fused kernel)
    double specres_fixed, contval_fixed, velstep, log2pi;
    double dnu_seg;         // largest |nu(first) - nu(last)| over the 64-pixel segments
    double veto4, veto5;    // asymmetric veto: allowed counts of resid > 4 / > 5 (threshold + grace)
    // unit-cube input (mcalf_loglike_cube_batch*): P holds cube rows and the prior transform of
    // hires_fitter.py:202-216 is applied while decoding; nullptr = P holds theta
    const double* prior_lo;
    const double* prior_hi;
    double* theta_out;      // [batch][ndim] transformed parameters, or nullptr
    int prior_int;          // 1: int() on the ncomp slot (_scale_cube_pc), 0: leave (_scale_cube_mn)
    // persistent fused kernel: work items (live point x tile) of this launch and its item queue
    int nitems, persist;
    // Segment-mask words of single-tile contexts (the end of this file), wave-uniform: > 0 = the tile's real segments
    // (ceil(npix / 64), the virtually continued last one included), whose end frequencies mcalf_create found monotone -- the
    // set-up finds a record's word by boundary search; 0 = the walk over all 64 segments.  (In the padding in front of
    // `queue`: the layout, and with it the fused kernels' machine code, is the one without it.)
    int seg_search;
    unsigned int* queue;    // reset to 0 by the set-up kernel of the same launch
    // Hand-out order of the persistent kernel (single-tile spectra): ticket t of the queue is live point
    // order[t] -- the live points sorted by their component count, longest first (written by one extra workgroup
    // of the set-up kernel); nullptr = ticket order.  Scheduling only: a live point's arithmetic does not depend on who evaluates it when.
    int* order;
    // Streaming single launch (mcalf_fused_kernel<..., kStream = true>, the host-pointer entries): there is no set-up
    // kernel and no copy command.  The grid sets the live points up itself -- the first `stream_wgs` workgroups keep
    // doing so, row after row as the rows arrive, until none is left, and only then join the others at the item queue
    // -- and a work item is handed to the component loop once its row's stamp says it is set up.
    struct StreamCtl* sctl; // per-XCD item queues and row queues, exit count (self-resetting: the last workgroup out zeroes them)
    unsigned int* ready;    // [batch] ready[s] == gen: live point s is set up (records, taps, header in HBM)
    const unsigned int* arrived;   // rows of P the host has staged so far (page-locked, device-mapped word); nullptr: all
    unsigned int* status;   // page-locked, device-mapped: [0] != 0: a wait ran out (the call fails over), [1] = gen when the grid
                            // has drained, [2] / [3] = fewest / most workgroups an XCD received
    unsigned int gen;       // stamp of this call
    int nrows;              // live points of this launch
    int stream_wgs;         // workgroups PER XCD (the first ones to start there) dedicated to the set-up until the XCD's rows are done
    int eager_rows;         // local BLOCKS (of 8 rows) per XCD that whichever workgroup of the XCD gets there first sets up (the
                            // rows the XCD's first items need; all of them when P is resident in HBM)
    long long spin_ticks;   // longest wait, in ticks of s_memrealtime (100 MHz)
    double* Pdev;           // [batch][ndim] in HBM: where the workgroups copy rows that live in host memory; nullptr: P is in HBM
    int rest_chunk;         // rows a dedicated workgroup claims at a time (a multiple of 8: whole blocks)
    int rec_stride, tap_stride, hdr_stride;   // doubles between the records / taps / headers of consecutive live points in the
                            // streaming workspaces: multiples of a 128-byte line, so that no two live points share one
};

// XCDs of an MI355X in SPX mode.  The streaming launch keeps every hand-over inside one of them: block k of eight rows
// belongs to XCD k % 8, and only workgroups that run there set it up and evaluate it.  On any other device shape -- a DPX /
// QPX / CPX partition, a CU-masked stream -- some of the eight would receive no workgroup, so the host takes the launch
// only where the context's probe kernel saw workgroups on exactly these eight (host_stream.cpp) and otherwise runs the
// row-block pipeline; after every launch it also checks that each XCD did receive workgroups (status[2]).
constexpr int kXcds = 8;
struct StreamCtl {                      // per XCD x: its own queues over ITS live points (blocks of 8 rows, block k -> XCD k % 8)
    unsigned int arrive[kXcds];         // workgroups of the launch that started on XCD x (the first few are its set-up workgroups)
    unsigned int sq_eager[kXcds];       // local blocks claimed of [0, eager_blocks): any workgroup of the XCD
    unsigned int sq_rest[kXcds];        // local blocks claimed of the rest: the XCD's dedicated workgroups
    unsigned int queue[kXcds];          // local tickets handed out by the XCD's item queue
    unsigned int exited;                // workgroups that have left the kernel
    unsigned int fin_exited;            // workgroups of the finalize kernel behind it (tiled spectra) that have finished
};
// status[0] of a streaming launch (0 = nobody gave up)
constexpr unsigned kStreamHostLate = 1u;     // a wait for the host's row count ran out
constexpr unsigned kStreamStampLate = 2u;    // a wait for a row's stamp ran out

// Live points of XCD x of n when the rows are dealt out in blocks of eight (block k -> XCD k % n), and the row
// behind the XCD's local index j.  (constexpr: host and device; tests/test_host_logic.py checks the partition through
// mcalf_stream_partition.)
constexpr int stream_rows_of(int nrows, int x, int n) {
    const int nblocks = (nrows + 7) >> 3;
    if (nblocks <= x) return 0;
    const int nbx = (nblocks - x + n - 1) / n;
    return 8 * nbx - ((nblocks - 1) % n == x ? 8 * nblocks - nrows : 0);
}
constexpr int stream_row(int x, int j, int n) { return 8 * n * (j >> 3) + 8 * x + (j & 7); }

// LDS flux tile, "mod-8 planar": element i lives in plane (i & 7) at index (i >> 3).  The convolution
// thread that owns outputs 8g..8g+7 then reads every plane at consecutive indices with compile-time
// offsets (no address arithmetic, lanes hit consecutive slots); the plane stride 516 == 4 (mod 32)
// also keeps the lane-contiguous flux stores conflict free.
constexpr int kPlaneStride = (kExtMax + kTileSlack) / 8 + 2;      // 516
static_assert(kPlaneStride % 32 == 4, "plane stride must be 4 mod 32");
constexpr int tile_doubles(int) {
    return 8 * kPlaneStride > VT_NY * VT_NTOT ? 8 * kPlaneStride : VT_NY * VT_NTOT;   // the region doubles as the T table
}

// The dynamic LDS of a workgroup of the fused kernel, as offsets in doubles from its start: the ONE definition that the
// kernel carves its shared memory with (fused_item.h) and that the host sizes the launch, the lines per barrier and the
// resident kernel's row offset from (ctx_plan.h).  lps: lines folded per barrier.
struct ItemLds {
    long tab;        // 2 x lps folded tables (kTabPad each), double-buffered
    long rec;        // ncl_cap records of kRecStride
    long taps;       // 2 n_cap + 8: the LSF taps, zero-padded to a multiple of 8
    long red;        // kRedDoubles: 3 * kWaves partials + the next item index
    long wt;         // [VT_INODES][64] interpolation weights, node-major
    long tile;       // the flux tile (tile_doubles), which holds the universal table T until the component loop ends
    constexpr ItemLds(int lps, int ncl_cap, int n_cap)
        : tab(0), rec(tab + 2 * (long)lps * kTabPad), taps(rec + (long)ncl_cap * kRecStride), red(taps + 2 * (long)n_cap + 8),
          wt(red + kRedDoubles), tile(wt + 64 * VT_INODES) {}
    constexpr size_t doubles(int ext) const { return (size_t)tile + (size_t)tile_doubles(ext); }   // with a tile region of `ext` pixels
    constexpr size_t bytes(int ext) const { return doubles(ext) * sizeof(double); }
};

constexpr int kSetupBlockMax = 512;
constexpr int kMinWaves = 4;            // waves per SIMD the fused kernel is compiled for (2 workgroups of 8 waves per CU)

// What a result slot of a page-locked block holds until its kernel has written it: a quiet NaN with a payload no
// arithmetic produces (the kernels' NaNs are the canonical one or carry an operand's payload).
constexpr uint64_t kResultPending = 0x7FF8C0DEC0DE0001ull;

// RESIDENT one-theta evaluator (mcalf_resident_kernel): the mailbox it serves and the words the workgroups of one
// resident launch share.
constexpr unsigned kResRunning = 1u, kResLeaving = 2u, kResGone = 3u;
constexpr int kResRowMax = 64;
struct alignas(64) ResidentBox {
    unsigned int req;            // host: number of the request whose row is in `row` (written last, release)
    unsigned int quit;           // host: non-zero = leave at the next look
    unsigned int ack;            // device: number of the last request answered
    unsigned int state;          // device: kResRunning / kResLeaving / kResGone
    double result;               // device; the host fills it with kResultPending before it posts a request
    double pad[5];
    double row[kResRowMax];      // host: the parameter row
};
// Words the workgroups of ONE resident launch share (device memory, zeroed by the host before the launch): the time of
// the launch's last answered request, and the word that tells everybody to leave.  A launch may hold one workgroup (a
// context's own evaluator) or one per mailbox (the broker: workgroup k serves mailbox k); its workgroups leave TOGETHER --
// when workgroup 0 finds that none of them has answered anything for `idle_ticks`, or when a mailbox says `quit` -- so
// that one launch on one stream is all there ever is (hardware queues are few: a launch per mailbox, each on its own
// stream, had the resident kernels of one queue wait for each other's idle limits).
struct ResidentShared {
    unsigned long long last;     // s_memrealtime of the last answer of any workgroup of the launch
    unsigned int leave;          // non-zero: everybody leaves (after a last look at their mailboxes)
    unsigned int pad;
};

// ---- kernel entry points (defined at the end of kernels.hip; the host launches them with hipLaunchKernel) -------------
#define MCALF_INTERNAL __attribute__((visibility("hidden")))      // not part of what the library exports
// The instantiations of the fused kernel: (JAX semantics, self-halo tile, lines per barrier) for batches, the one-launch
// variant (set-up inside the kernel, always 4 lines per barrier) for small calls, the streaming launch of the
// host-pointer entries.
MCALF_INTERNAL const void* fused_kernel_ptr(bool jax, bool selfhalo, int lps, bool inl = false, bool stream = false);
MCALF_INTERNAL int fused_kernel_count();                       // every instantiation, for hipFuncSetAttribute
MCALF_INTERNAL const void* fused_kernel_at(int i);
MCALF_INTERNAL const void* resident_kernel_ptr(bool jax, bool selfhalo);
MCALF_INTERNAL const void* sample_kernel_ptr(bool jax);        // (const KArgs a, long batch)
MCALF_INTERNAL const void* finalize_kernel_ptr();              // (const double* partial, double* out, long batch, int ntiles, int mode, int asymm, double veto4, double veto5, unsigned* fin_count, unsigned* done_word, unsigned gen)
MCALF_INTERNAL const void* hjert_kernel_ptr();                 // (const double* x, const double* y, long n, double* out, const double* tabs, int node_form)
MCALF_INTERNAL const void* scale_cube_kernel_ptr();            // (const double* lo, const double* hi, const double* cube, long total, int ndim, int slot, int int_ncomp, double* theta)
MCALF_INTERNAL const void* xcd_probe_kernel_ptr();             // (unsigned int* mask): ORs 1 << XCC_ID of every workgroup into *mask
// LSF wider than a workgroup tile (kernels.hip, "wide" kernels): taps per live point, convolution + terms from HBM
constexpr int kWideBlockThreads = 256;
constexpr int kWideBlockPix = 8 * kWideBlockThreads;       // output pixels per workgroup of the wide convolution (eight per thread)
constexpr int kWideTapChunk = 512;                         // taps staged in LDS per pass
MCALF_INTERNAL const void* wide_taps_kernel_ptr(bool jax);             // (const KArgs a, double* taps, long tap_stride, SampleHdr* hdr), grid = rows
MCALF_INTERNAL const void* wide_conv_kernel_ptr(bool jax);             // (const KArgs a, const double* flux, const double* taps, long tap_stride, const SampleHdr* hdr, int nblocks), grid = (ceil(npix / kWideBlockPix), rows)
MCALF_INTERNAL const void* wide_rows_kernel_ptr();             // (const double* rows, double* out, long batch): (R, cont, N, z, b) rows with cont := 1

// ---- segment-mask words of single-tile contexts -----------------------------------------------------------------------
// Which of a tile's 64 segments (64 pixels each) a line's far wing is interpolated on.  Plain C++ that compiles for the host
// and for the device from ONE source: the set-up (kernels.hip, setup_sample) forms the words with it, mcalf_create checks
// the search's precondition with it, and tests/stubs/segment_search_check.cpp compares search and walk word for word on
// the CPU.
//
// A segment is interpolated for a line (A, B, uthr) when both of its end pixels have u >= uthr, or both u <= -uthr, with
// u = fma(nu, A, -B) -- the fused kernel's own expression and its own four comparisons (eval_line) -- and the context allows
// it (segok).  The WALK evaluates that at all 128 ends.  The SEARCH uses that fl(nu A - B) is monotone in nu for fixed A and
// B, whatever the sign of A (rounding is monotone): along a monotone sequence of end frequencies each of the predicates
// u >= uthr and u <= -uthr holds on a prefix or on a suffix, so two evaluations at the outer ends and a bisection between
// them find where its run begins or ends -- the same fma and comparisons at actual end frequencies, only fewer of them:
// 2 + 2 (floor(log2(2 nreal - 1)) + 1) <= 16 instead of 128.  u is NaN at one end exactly when it is at all of them (NaN in A or
// B, or inf - inf: none depends on nu as long as every nu is finite and positive), and then no predicate holds anywhere.
#if defined(__HIPCC__) || defined(__CUDACC__)
#define MCALF_HD __host__ __device__ __forceinline__
#else
#define MCALF_HD inline
#endif

constexpr int kSegs = 64;               // segments of a tile
constexpr int kSegEnds = 2 * kSegs;     // end table: entry 2 m = first pixel frequency of segment m, 2 m + 1 = its last

// Index into nu[] of entry k of the end table.
MCALF_HD int seg_end_pixel(int k) { return 64 * (k >> 1) + 63 * (k & 1); }

MCALF_HD double seg_u(double nu, double A, double B) { return std::fma(nu, A, -B); }
MCALF_HD bool seg_above(double u, double uthr) { return u >= uthr; }
MCALF_HD bool seg_below(double u, double uthr) { return u <= -uthr; }

// Bit m = segment m  ->  bit 8 i + v = segment 8 v + i (the layout of the records' words: byte i belongs to the wave that
// evaluates the pixels of segments i, i + 8, ..): the transpose of the 8 x 8 bit matrix.
MCALF_HD uint64_t seg_transpose(uint64_t x) {
    uint64_t t;
    t = (x ^ (x >> 7)) & 0x00AA00AA00AA00AAull;  x ^= t ^ (t << 7);
    t = (x ^ (x >> 14)) & 0x0000CCCC0000CCCCull; x ^= t ^ (t << 14);
    t = (x ^ (x >> 28)) & 0x00000000F0F0F0F0ull; x ^= t ^ (t << 28);
    return x;
}

// The walk: every segment, both ends.  `ends` has kSegEnds entries, `ok` bit m = segment m may be interpolated.
MCALF_HD uint64_t seg_word_walk(double A, double B, double uthr, const double* ends, uint64_t ok) {
    uint64_t w = 0;
    for (int m = 0; m < kSegs; ++m) {
        const double u0 = seg_u(ends[2 * m], A, B), u1 = seg_u(ends[2 * m + 1], A, B);
        const bool in = (seg_above(u0, uthr) && seg_above(u1, uthr)) || (seg_below(u0, uthr) && seg_below(u1, uthr));
        if (in && ((ok >> m) & 1ull)) w |= 1ull << (8 * (m & 7) + (m >> 3));      // (placed by the layout's definition, not by seg_transpose)
    }
    return w;
}

// The search.  Precondition (seg_ends_searchable): ends[0 .. 2 nreal) finite, positive and monotone, the segments from
// nreal on wholly virtual (nu = 0 at both ends: ONE classification, evaluated with the same fma at nu = 0).
MCALF_HD uint64_t seg_word_search(double A, double B, double uthr, const double* ends, int nreal, uint64_t ok) {
    const int last = 2 * nreal - 1;
    const double uF = seg_u(ends[0], A, B), uV = seg_u(0.0, A, B);
    const bool aF = seg_above(uF, uthr), bF = seg_below(uF, uthr);
    // aPos / bPos: the last end at which the predicate still has the value it has at end 0 (`last`: it never changes), by
    // steps of falling powers of two from the largest one <= last (the same for every record of the context); a step past
    // the last end looks at the last end.  Both predicates in one loop, so that their two loads are in flight together.
    int aPos = 0, bPos = 0;
    for (int step = 1 << (31 - __builtin_clz((unsigned)last)); step > 0; step >>= 1) {
        const int ai = aPos + step < last ? aPos + step : last, bi = bPos + step < last ? bPos + step : last;
        if (seg_above(seg_u(ends[ai], A, B), uthr) == aF) aPos = ai;
        if (seg_below(seg_u(ends[bi], A, B), uthr) == bF) bPos = bi;
    }
    // A predicate true at end 0 holds at the ends [0, pos + 1): on the segments [0, (pos + 1) / 2) with both ends.  One false
    // at end 0 holds at the ends [pos + 1, 2 nreal): on the real segments from (pos + 2) / 2 on.  n <= 64: shifted in two halves.
    const int aN = (aPos + (aF ? 1 : 2)) >> 1, bN = (bPos + (bF ? 1 : 2)) >> 1;
    const uint64_t aFrom = (~0ull << (aN >> 1)) << (aN - (aN >> 1)), bFrom = (~0ull << (bN >> 1)) << (bN - (bN >> 1));   // bits n ..
    const uint64_t real = ~((~0ull << (nreal >> 1)) << (nreal - (nreal >> 1)));
    uint64_t w = ((aF ? ~aFrom : aFrom) | (bF ? ~bFrom : bFrom)) & real;
    if (seg_above(uV, uthr) || seg_below(uV, uthr)) w |= ~real;
    return seg_transpose(w & ok);
}

// Host, once per context: may the records of a spectrum with this pixel-frequency table (4096 entries, nu[i] of the
// real and the virtually continued pixels, 0 beyond) take the search?  The ends of the nreal = ceil(npix / 64) real
// segments must be finite, positive and monotone -- equal neighbours allowed, either direction -- and every later end 0.
inline bool seg_ends_searchable(const double* nu, long npix, int* nreal_out) {
    const int nreal = (int)((npix + 63) / 64);
    if (nreal_out) *nreal_out = nreal;
    if (npix < 1 || nreal > kSegs) return false;
    bool up = true, down = true;
    for (int k = 0; k < 2 * nreal; ++k) {
        const double v = nu[seg_end_pixel(k)];
        if (!std::isfinite(v) || !(v > 0.0)) return false;
        if (k > 0) {
            const double p = nu[seg_end_pixel(k - 1)];
            if (v < p) up = false;
            if (v > p) down = false;
        }
    }
    for (int k = 2 * nreal; k < kSegEnds; ++k)
        if (nu[seg_end_pixel(k)] != 0.0) return false;
    return up || down;
}

}  // namespace mcalf
