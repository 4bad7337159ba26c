// Host side of libmcalf_hip.so, shared by every one of its host translation units:
// the context behind the opaque mcalf_ctx of include/mcalf_hip.h and the internal functions one file offers the others.
// Plain C++ against the HIP runtime API; kernels are launched through the entry-point table of kernel_args.h.  What a context
// decides from its spec alone -- the checks, the launch geometry, the host tables -- is ctx_plan.h (no HIP there: the CPU tests
// plan with it); mcalf_ctx inherits the planned scalars (CtxShape) and adds what belongs to a device.
#pragma once
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>   // types only: the library is resolved at run time (mcalf_comm_*), never linked

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#pragma GCC visibility push(default)     // the C ABI is what the library exports; everything else stays inside it
#include "../../include/mcalf_hip.h"
#pragma GCC visibility pop
#include "kernel_args.h"
#include "ctx_plan.h"
#include "grad_args.h"
#include "ns_evidence.h"
#include "prior_args.h"
#include "theta_row.h"

#define MCALF_STR_(x) #x
#define MCALF_STR(x) MCALF_STR_(x)

namespace mcalf {
constexpr int kMaxChunks = 8;
constexpr size_t kSmallDoubles = 65536;     // up to 512 KB of parameters (and as many results) go the zero-copy way
constexpr int64_t kStreamTiledMaxItems = 65536;   // tiled spectra stream up to this many work items (host_stream.cpp: run_host_stream)
}  // namespace mcalf
using namespace mcalf;

// A persistent helper thread of a context (the other devices of a multi-device context: host_multi.cpp; the staging copy
// of a large pageable batch: host_pipeline.cpp).  One job at a time: post(), then wait().  The thread looks for the next job
// for a short while after one -- a sampler calls back to back -- and then sleeps on a condition variable.
typedef int (*WorkFn)(void* who, int64_t lo, int64_t hi, void* arg);
struct HostWorker {
    std::thread th;
    std::mutex m;
    std::condition_variable cv;
    std::atomic<unsigned> posted{0}, done{0};
    bool quit = false;
    int device = -1;                        // hipSetDevice once, when the thread starts (-1: the thread makes no HIP call)
    void* who = nullptr;
    WorkFn fn = nullptr;
    void* arg = nullptr;
    int64_t lo = 0, hi = 0;
    int rc = 0;

    void start() { th = std::thread([this] { loop(); }); }
    void loop() {
        if (device >= 0) (void)hipSetDevice(device);
        unsigned seen = 0;
        for (;;) {
            bool got = false;
            for (int i = 0; i < 40000 && !got; ++i) {          // 40000 pause instructions (~1 ms) of looking before the thread gives the core up
                got = posted.load(std::memory_order_acquire) != seen;
                if (!got) __builtin_ia32_pause();
            }
            if (!got) {
                std::unique_lock<std::mutex> lk(m);
                cv.wait(lk, [&] { return quit || posted.load(std::memory_order_acquire) != seen; });
                if (posted.load(std::memory_order_acquire) == seen) return;      // quit
            }
            rc = fn(who, lo, hi, arg);
            ++seen;
            done.store(seen, std::memory_order_release);
        }
    }
    void post(WorkFn f, void* a, int64_t l, int64_t h) {
        std::lock_guard<std::mutex> lk(m);                    // (the thread tests its predicate under this lock: no lost wake-up)
        fn = f; arg = a; lo = l; hi = h;
        posted.fetch_add(1, std::memory_order_release);
        cv.notify_one();
    }
    int wait() {
        const unsigned want = posted.load(std::memory_order_relaxed);
        for (unsigned long spins = 0; done.load(std::memory_order_acquire) != want; ++spins) {
            if ((spins & 0xFFFul) == 0xFFFul) std::this_thread::yield();
            else __builtin_ia32_pause();
        }
        return rc;
    }
    void stop() {
        { std::lock_guard<std::mutex> lk(m); quit = true; cv.notify_one(); }
        if (th.joinable()) th.join();
    }
};

// Every tunable the ENVIRONMENT of the loading process may set, read ONCE per context at the top of mcalf_create
// (host_config.cpp: the only place the library looks at its environment).  -1 / empty = the variable is not set (or not valid): the
// context then keeps its built-in value.  mcalf_get_config prints the EFFECTIVE values the context runs under, and which
// of them the environment supplied, so a measured number can name its knobs.
struct EnvKnobs {
    int lines_per_sync = -1;                // MCALF_LINES_PER_SYNC   4 / 5
    int persist = -1;                       // MCALF_PERSIST          0 / 1
    int order = -1;                         // MCALF_ORDER            0 / 1
    int inline_max = -1;                    // MCALF_INLINE_MAX       work items
    int resident_us = -1;                   // MCALF_RESIDENT_US      0 .. 1000000
    int setup_block = -1;                   // MCALF_SETUP_BLOCK      64 .. 512, a multiple of 64
    int host_plan[kMaxChunks] = {};         // MCALF_HOST_PLAN        "1,3,4": relative sizes of the pipelined entry's row blocks
    int host_plan_n = 0;
    int host_first_kb = -1;                 // MCALF_HOST_FIRST_KB    bytes (KiB) of the pipelined entry's first row block
    int host_trace = -1;                    // MCALF_HOST_TRACE       0 / 1: host-side time per phase of the pipelined entry
    int stage_threads = -1;                 // MCALF_STAGE_THREADS    helper threads of the staging copy (0: the calling thread alone)
    int stream = -1;                        // MCALF_STREAM           0 / 1 / 2
    int stream_wgs = -1;                    // MCALF_STREAM_WGS
    int stream_min = -1;                    // MCALF_STREAM_MIN       1 .. 64 work items per workgroup slot
    int stream_poll = -1;                   // MCALF_STREAM_POLL      0 / 1
    int stream_eager = -1;                  // MCALF_STREAM_EAGER
    int stream_chunk = -1;                  // MCALF_STREAM_CHUNK     8 .. 512, a multiple of 8
    int stream_device = -1;                 // MCALF_STREAM_DEVICE    0 / 1 / 2
    int stream_trace = -1;                  // MCALF_STREAM_TRACE     0 / 1
    double stream_timeout_s = -1.0;         // MCALF_STREAM_TIMEOUT   seconds, (0, 60]
    int chunks = -1;                        // MCALF_CHUNKS           0 .. 8
    int ns_compact = -1;                    // MCALF_NS_COMPACT       0 / 1
    std::string rccl_lib;                   // MCALF_RCCL_LIB         (read when the first mcalf_comm_* call loads RCCL)
#ifdef MCALF_TESTING
    int test_fail_preflight = -1;           // MCALF_TEST_FAIL_PREFLIGHT
    long test_xcd_mask = -1;                // MCALF_TEST_XCD_MASK
    int test_starve = -1;                   // MCALF_TEST_STARVE
#endif
};
EnvKnobs read_environment();                // host_config.cpp

// Diagnostics (MCALF_HOST_TRACE / MCALF_STREAM_TRACE): accumulators of ONE context (a context is not re-entrant, so they need no
// lock; the entries of a multi-device context each keep and print their own), printed when the context is destroyed.
struct HostTrace { double stage_us = 0, stage_bytes = 0, helper_bytes = 0, helper_wait_us = 0, enqueue_us = 0, wait_us = 0, out_us = 0, first_enqueued_us = 0;
                   double call_copy_us = 0, call_order_us = 0, call_launch_us = 0, call_copy_max = 0; long calls = 0, blocks = 0;
                   double small_prep_us = 0, small_launch_us = 0, small_copy_us = 0, small_poll_us = 0, small_out_us = 0; long small_calls = 0; };
struct BlockTimeline { int n = 0; long rows[kMaxChunks]; float h2d0[kMaxChunks], h2d1[kMaxChunks], done[kMaxChunks]; double host_enq[kMaxChunks], call_h2d[kMaxChunks], call_order[kMaxChunks], call_launch[kMaxChunks]; int pinned = 0; double sync_us = 0; };
struct StreamTrace { double t[6] = {}; long n = 0; };

// A buffer the context owns: device memory (hipFree) or a page-locked host block (kPinned: hipHostFree), with its capacity in
// elements.  It reads as the plain pointer wherever one is wanted and is released when the context is deleted -- in
// mcalf_destroy that is after the resident kernel has been told to leave (hipFree waits for the device).
template <typename T, bool kPinned = false>
struct DevBuf {
    T* p = nullptr; size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)(kPinned ? hipHostFree((void*)p) : hipFree((void*)p)); }
    operator T*() const { return p; }
    T* operator->() const { return p; }
};
template <typename T> using PinBuf = DevBuf<T, true>;

// A device-resident nested-sampling run (host_nsrun.cpp: mcalf_nested_*).  The buffers are grown by mcalf_nested_open and stay
// with the context when a run is closed, as every workspace does: a second run of the same or a smaller size allocates nothing.
struct NsRun {
    enum Phase { kClosed, kOpen, kFinished };
    Phase phase = kClosed;
    mcalf_nested_opts opts = {};
    int64_t nlive = 0, ndead = 0, rounds = 0, nevals = 0, unfinished = 0, rows_launched = 0;
    double max_key = 0.0;                   // the largest live key, from the last round's record
    int32_t reason = 0;                     // why the last mcalf_nested_advance returned
    bool have_last = false;                 // a round has selected: mcalf_nested_last_round has something to report
    bool timing = false, timed = false;     // mcalf_nested_set_timing; the last round was timed
    NsEvidence ev;                          // ln X and the running ln Z
    double logZ = 0.0, H = 0.0;             // mcalf_nested_finish's
    std::vector<double> logw, host_l;       // the normalised log weights and the dead logL they were made from
    std::vector<double> keys;               // the dead keys of a round's record, as doubles
    DevBuf<double> UL, LL, UD, LD, meanpart, covpart, tri, var, D, U0, Lmin, Un, Ln, theta;
    DevBuf<int32_t> rank, order, dying, pick, status, nevals_row, moves;
    DevBuf<uint64_t> sid, rec;
    PinBuf<uint64_t> h_rec;
    hipEvent_t ev_t[8] = {};                // around the book-keeping kernels of a timed round
    float last_ms[7] = {};                  // rank, select, moments, Cholesky, gather, replace, retire
    // Device bytes the run's buffers hold (mcalf_nested_footprint).
    size_t device_bytes() const {
        size_t d = 0, i = 0;
        for (const DevBuf<double>* b : {&UL, &LL, &UD, &LD, &meanpart, &covpart, &tri, &var, &D, &U0, &Lmin, &Un, &Ln, &theta}) d += b->cap;
        for (const DevBuf<int32_t>* b : {&rank, &order, &dying, &pick, &status, &nevals_row, &moves}) i += b->cap;
        return d * sizeof(double) + i * sizeof(int32_t) + (sid.cap + rec.cap) * sizeof(uint64_t);
    }
    ~NsRun() { for (hipEvent_t e : ev_t) if (e) (void)hipEventDestroy(e); }
};

struct mcalf_ctx : CtxShape {               // (the problem and geometry fields: ctx_plan.h)
    HostTrace htrace;
    BlockTimeline btrace;
    StreamTrace strace;
    EnvKnobs env;                           // what the environment said when the context was created
    int device = 0;
    std::string arch;
    std::string err;
    int inline_max_items = 0;                      // launches of at most this many work items take the one-launch variant
    // device buffers
    DevBuf<double> d_nu, d_obj, d_ispec2, d_lgis, d_err, d_tabs, d_wtab;
    DevBuf<LineDev> d_lines;
    DevBuf<unsigned long long> d_segok;
    // workspaces (grown on demand)
    DevBuf<double> d_P, d_out, d_partial, d_model, d_bounds, d_prior, d_recs, d_taps;
    DevBuf<SampleHdr> d_hdr;
    hipStream_t stream = nullptr;
    // optional per-launch timing of the fused kernel (mcalf_profile_begin / _end)
    std::vector<hipEvent_t> ev;
    size_t ev_used = 0;
    bool profiling = false;
    // Small host-pointer calls (the one-theta-at-a-time solvers): parameters and results travel through a
    // page-locked, device-mapped staging block that the kernels read / write directly -- no copy commands.
    // Resident one-theta evaluator (mcalf_set_resident; off by default): its mailbox, its own stream, what the host
    // believes about the kernel, the next request number
    PinBuf<ResidentBox> h_box;          // page-locked, coherent, device-mapped
    ResidentBox* d_box = nullptr;       // the same memory as the device sees it
    DevBuf<ResidentShared> d_res_shared;      // device words of the evaluator's launch (idle clock, leave flag)
    hipStream_t res_stream = nullptr;
    int resident_us = 0;                // idle limit in microseconds; 0 = no resident kernel
    bool res_alive = false;
    unsigned res_seq = 0;
    long res_launches = 0, res_calls = 0;
    std::vector<double> h_prior;        // the prior box as mcalf_set_prior took it: lo[ndim], hi[ndim] (host copy)
    PinBuf<double> h_small;             // host address
    double* d_small = nullptr;          // the same memory as the device sees it
    // prior box of mcalf_set_prior (device copy in d_prior: lo[ndim] then hi[ndim])
    bool prior_set = false;
    int prior_int = 0;
    // Gaussian factors of mcalf_set_gauss_prior (host_prior.cpp), next to the box: mu[ndim], sigma[ndim], c[ndim] on the device and
    // on the host, and the number of coordinates that carry one (0: none is set; a multi-device parent holds the count alone)
    DevBuf<double> d_gauss;
    std::vector<double> h_gauss;
    int ngauss = 0;
    // Chunked issue: a batch is cut into row blocks that go to the caller's stream and to context-owned
    // auxiliary streams (fork / join through events), so that the set-up kernel and the first workgroups of
    // block k+1 run in the tail of block k.  chunks_req: 0 = automatic, n = exactly n blocks (1 = off).
    int chunks_req = 0;
    int host_plan[kMaxChunks] = {};            // MCALF_HOST_PLAN: relative sizes of the row blocks of the pipelined
    int host_plan_n = 0;                       // host-pointer entry (0 = the built-in plan: first block by BYTES, then doubling)
    int host_first_kb = 128;                   // MCALF_HOST_FIRST_KB: parameter bytes (KiB) of the pipelined entry's first row block
    int host_trace = 0;                        // MCALF_HOST_TRACE=1 (diagnostic): host-side time per phase of the pipelined entry
    int stage_threads = 0;                     // MCALF_STAGE_THREADS: helper threads of the pageable -> page-locked staging copy
    std::vector<std::unique_ptr<HostWorker>> stagers;   // (started by the first call that uses them)
    int num_cu = 256;
    int persist = 1;                    // fused kernel as a persistent grid (MCALF_PERSIST=0: one workgroup per item)
    int setup_block = 512;              // threads per workgroup of the set-up kernel (MCALF_SETUP_BLOCK: 64 .. 512)
    DevBuf<unsigned int> d_queue;       // [kMaxChunks] work-item queues of the persistent kernel
    DevBuf<int> d_order;                // [batch] hand-out order of the persistent kernel (per row block)
    int ordered = 1;                    // MCALF_ORDER=0: hand the live points out in row order
    hipStream_t aux[kMaxChunks - 1] = {};
    hipEvent_t ev_fork = nullptr, ev_join[kMaxChunks - 1] = {};
    hipEvent_t ev_h2d[kMaxChunks] = {};     // row-block pipeline: block k's rows are in HBM (recorded on the copy stream, aux[1])
    // multi-GPU: the communicator of mcalf_comm_init (one process per GPU, RCCL over xGMI)
    ncclComm_t comm = nullptr;
    int comm_ranks = 0, comm_rank = -1;
    hipStream_t comm_stream = nullptr;      // the exchange runs here, behind an event of the launch stream
    hipEvent_t ev_kernels = nullptr;        // launch stream -> comm stream: this step's logL block is complete
    hipEvent_t ev_comm[2] = {};             // comm stream -> launch stream: exchange of call k (slot k & 1) has landed
    bool ev_comm_used[2] = {};
    unsigned comm_calls = 0;
    int comm_overlap = 0;                   // 0: every gather call ends with the launch stream waiting for its exchange
    bool comm_dead = false;                 // aborted after a failure inside an exchange
#ifdef MCALF_TESTING
    bool fail_preflight = false;            // MCALF_TEST_FAIL_PREFLIGHT=1 (test builds only): an injected workspace-growth failure
#endif
    // page-locked staging of the host-pointer entries: parameter rows in, scalars out
    PinBuf<double> h_stage;
    // Streaming single launch of the host-pointer entries (run_host_stream): queues / stamps in HBM, the words the host
    // and the kernel exchange in a page-locked, device-mapped block (h_ctl: [0] status, [1] generation of the last
    // launch that has drained, [16] rows staged so far -- a cache line of its own)
    // (ONE allocation, carved up by hand: records, taps, parameter rows, headers, stamps of `sws_rows` live points, then the
    // queues; its capacity counts live points, not elements)
    DevBuf<void> d_sws;
    size_t sws_rows = 0;
    double *s_recs = nullptr, *s_taps = nullptr, *s_P = nullptr;
    size_t s_rec_stride = 0, s_tap_stride = 0, s_hdr_stride = 0;
    SampleHdr* s_hdr = nullptr;
    StreamCtl* d_sctl = nullptr;
    unsigned int* d_ready = nullptr;
    PinBuf<volatile unsigned int> h_ctl;
    unsigned int* d_ctl = nullptr;          // the same words as the device sees them
    unsigned int stream_gen = 0;            // stamp of the last streaming launch; never restarts (a regrown workspace is zero-filled, and
                                            // a restarted count could meet the completion word of an earlier launch: h_ctl[1])
    // Which XCDs the context's stream reaches: bit i = the probe kernel saw a workgroup with hardware XCC_ID i
    // (stream_probe_xcds: mcalf_create, mcalf_set_cu_mask).  The streaming launch is built for exactly 0xFF.
    unsigned int xcd_mask = 0;
    std::vector<uint32_t> cu_mask;          // mcalf_set_cu_mask: the CU mask of the context's own streams (empty: none)
    int stream_on = 1;                      // MCALF_STREAM: 0 = the row-block pipeline of round 2 instead; 1 = automatic (spectra that fit
                                            // one tile always, tiled ones up to kStreamTiledMaxItems work items: measured, config E's
                                            // 16384 x 5 items run 0.5 % faster through the pipeline, 8192 x 5 items 3 % slower); 2 = always
    int stream_min = 4;                     // MCALF_STREAM_MIN: work items per workgroup slot from which a host-pointer batch streams
    int stream_wgs = 16;                    // MCALF_STREAM_WGS: workgroups dedicated to the set-up while rows are outstanding
    int stream_eager = 0;                   // MCALF_STREAM_EAGER: blocks of 8 rows per XCD any workgroup may set up (0: what the first items need)
    int stream_chunk = 32;                  // MCALF_STREAM_CHUNK: rows such a workgroup claims (and copies to HBM) at a time
    int stream_trace = 0;                   // MCALF_STREAM_TRACE=1 (diagnostic): host-side time per phase of the streaming entry
    int stream_device = 0;                  // MCALF_STREAM_DEVICE=1 (diagnostic): the *_device scalar entries take the streaming launch too
    int stream_poll = 1;                    // MCALF_STREAM_POLL=0: wait for the stream's signal instead of polling h_ctl[1]
    double stream_timeout_s = 0.5;          // MCALF_STREAM_TIMEOUT: longest wait of a wave inside the kernel
    // LSF wider than a workgroup tile (numpy boundary): the fused kernel runs WITHOUT convolution and continuum into
    // d_wide, two more kernels do taps, periodic convolution, continuum and terms from HBM (host_wide.cpp: launch_wide).
    // Whether a context is one, and the half-width it provisions, are CtxShape's wide and wide_n_cap.
    DevBuf<double> d_wide, d_wtaps, d_wpartial, d_wrows;
    DevBuf<SampleHdr> d_whdr;
    mcalf_launch_info_t last = {};      // what the last call did (mcalf_last_launch)
    // The staging arena of the host-pointer analysis entries (host_staged.cpp: run_staged): the device side of a call's arrays,
    // carved per call in column order.  Nothing in it is alive between calls.
    DevBuf<char> stage_dev;
    // The derivative entries' device buffers (host_grad.cpp), all grown on demand: the per-row workspaces of one pass -- the
    // seven every product shares, then the HVP's three -- and logL of a batch.
    enum { kGbRows, kGbRecs, kGbTaps, kGbDtaps, kGbF, kGbQ, kGbPart, kGbShared, kGbDdtaps = kGbShared, kGbHq, kGbHdq, kGbHvp,
           kGbLogL = kGbHvp, kGbCount };
    DevBuf<double> gb[kGbCount];
    // The equivalent-width entries (host_eqw.cpp): the wavelength steps [npix] (hires_fitter.py:485-486; none for a one-pixel
    // spectrum) and the two per-row workspaces of one pass, grown on demand.
    DevBuf<double> d_dlam;
    enum { kEbRecs, kEbPart, kEbCount };
    DevBuf<double> eb[kEbCount];
    // The optical-depth kinematics entries (host_kin.cpp): the wavelengths [npix] and the cell edges [npix + 1] (none for a
    // one-pixel spectrum) and the four per-row workspaces of one pass, grown on demand.
    DevBuf<double> d_wl, d_edge;
    enum { kKbRecs, kKbPart, kKbHead, kKbCand, kKbCount };
    DevBuf<double> kb[kKbCount];
    // The posterior-band entries (host_band.cpp), grown on demand: the per-block partials and counts, the per-pixel mean / count
    // a call keeps for itself when the caller wants neither, and the selected order statistics.  The [batch][npix] model matrix
    // is NOT among them: the host entry releases it before it returns, the device entry is handed the caller's.
    enum { kBbPart, kBbMean, kBbCount, kBbSel, kBbBufs };
    DevBuf<double> bb[kBbBufs];
    // The Fisher product and the fit (host_fit.cpp), grown on demand.  d_fitw: W [npix] of the Fisher product, built by its first
    // call (released with the context, after the resident evaluator has left).  kFbDM: the [rows][npix] workspace of one row block
    // of a Fisher product; the per-row vectors [rows][ndim] and scalars [rows] of one row block of a fit.  fit_int: the CG-frozen
    // flag [rows] and the pins [rows][ndim]; d_fit_live: the counter of live rows the host entry reads after every outer iteration.
    DevBuf<double> d_fitw;
    enum { kFbDM, kFbT, kFbG, kFbGT, kFbGu, kFbX, kFbR, kFbPv, kFbV, kFbFV, kFbScal, kFbCount };
    DevBuf<double> fb[kFbCount];
    DevBuf<int32_t> fit_int;
    DevBuf<unsigned int> d_fit_live;
    // The nested-sampling replacement primitive (host_ns.cpp), grown on demand.  The trial rows [batch][ndim] the logL launch
    // evaluates, their logL [batch], the brackets [3][batch] and the direction index [batch] of one call.  d_ns_live: the counter
    // of rows that proposed a trial, which the host entry reads after every step through the page-locked word h_ns_live.
    // ns_pack: the step stamps [batch] and, for a call that packs its trial rows (ns_compact, mcalf_set_slice_compact), their
    // slots and the packed row list [batch] each; kNbYc: the packed trial rows; ev_ns: recorded behind the copy of the count, so
    // that the host waits for the count and not for the step's logL launch.
    // ns_stats: what the last slice call launched (mcalf_slice_last_stats; a multi-device parent holds the sum over its entries).
    enum { kNbY, kNbLY, kNbBrk, kNbYc, kNbCount };
    DevBuf<double> nb[kNbCount];
    DevBuf<int32_t> ns_dir, ns_pack;
    DevBuf<unsigned int> d_ns_live;
    PinBuf<unsigned int> h_ns_live;
    hipEvent_t ev_ns = nullptr;
    int ns_compact = 0;                     // MCALF_NS_COMPACT / mcalf_set_slice_compact
    mcalf_slice_stats_t ns_stats = {};
    NsRun nsrun;                            // the device-resident run of mcalf_nested_* (a multi-device parent: its first entry's)
    // The ensemble sampler (host_ens.cpp), grown on demand.  The trial rows [T m][ndim] of the moving halves of its T temperatures
    // (mcalf_ensemble_batch: one), their logL [T m], the Hastings term and ln zeta [2][T m] and the inside flags [T m] of one half-step.  The chain is NOT among them: the host entry
    // releases it before it returns, the device entry is handed the caller's.
    enum { kEnY, kEnLY, kEnAux, kEnCount };
    DevBuf<double> enb[kEnCount];
    DevBuf<int32_t> ens_inside;
    DevBuf<double> ens_pr;                  // lnprior of the walkers [T n], grown by a call under a Gaussian prior only
    // Hamiltonian Monte Carlo (host_hmc.cpp), grown on demand.  The walkers' cube gradient, the momenta, the trajectories'
    // positions, their theta rows and the gradient rows the launch leaves [n][ndim] each; its logL [n]; K0 and lnprior [2][n];
    // the call's scale [ndim]; the dead flags [n] and the walker ids [n].  The chain is NOT among them, as the ensemble's.
    enum { kHmG, kHmR, kHmY, kHmTheta, kHmGY, kHmLY, kHmAux, kHmScale, kHmCount };
    DevBuf<double> hmb[kHmCount];
    DevBuf<int32_t> hmc_dead;
    DevBuf<uint64_t> hmc_wid;
    // The chain diagnostics (host_chain.h), grown on demand.  chain_ws: the per-walker sums, the ensemble-mean series, the walker
    // blocks' partial ACFs and the ACF of one statistics pass, carved per call.  The run to convergence: the walkers a block
    // starts from [n][ndim] and the block's own accept counts [n].
    DevBuf<double> chain_ws, chain_u;
    DevBuf<int32_t> chain_acc;
    // Single-process multi-device context (mcalf_create_multi, host_multi.cpp): the parent holds one complete context per
    // device entry and a worker thread for each but the first; it owns no device memory itself (its problem / geometry
    // fields, its CtxShape, are a copy of sub-context 0's, for mcalf_info).
    std::vector<mcalf_ctx*> subs;
    struct MultiPool* pool = nullptr;
    int multi_last_active = 0;              // sub-contexts the last call was cut over
};
inline bool is_multi(const mcalf_ctx* ctx) { return !ctx->subs.empty(); }
constexpr int kCtlWords = 64, kCtlArrived = 16, kCtlFinalized = 4;   // ([4]: stamp of the last streaming launch whose FINALIZE kernel has finished)

// ---- host_abi.cpp ---------------------------------------------------------------------------------------------------
int set_err(mcalf_ctx* ctx, int code, const char* fmt, ...) __attribute__((format(printf, 3, 4)));
void set_last_error(const std::string& msg);          // the thread's message (mcalf_last_error(NULL))

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e_ = (expr);                                                                 \
        if (e_ != hipSuccess)                                                                   \
            return set_err(ctx, MCALF_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));  \
    } while (0)

template <typename T> inline int grow(mcalf_ctx* ctx, DevBuf<T>& buf, size_t need_elems) {
    if (need_elems <= buf.cap) return MCALF_OK;
    if (buf.p) HIP_TRY(ctx, hipFree(buf.p));
    buf.p = nullptr; buf.cap = 0;
    HIP_TRY(ctx, hipMalloc((void**)&buf.p, need_elems * sizeof(T)));
    buf.cap = need_elems;
    return MCALF_OK;
}

// The same for a page-locked host block.
template <typename T> inline int grow(mcalf_ctx* ctx, PinBuf<T>& buf, size_t need_elems) {
    if (need_elems <= buf.cap) return MCALF_OK;
    if (buf.p) HIP_TRY(ctx, hipHostFree((void*)buf.p));
    buf.p = nullptr; buf.cap = 0;
    HIP_TRY(ctx, hipHostMalloc((void**)&buf.p, need_elems * sizeof(T), hipHostMallocDefault));
    buf.cap = need_elems;
    return MCALF_OK;
}

// The launch of a kernel that takes ONE argument block by value.  `expr` is what a failure names, as HIP_TRY would have named
// the call; LAUNCH_BLOCK writes it from the call's own expressions.
template <typename T>
inline int launch_block(mcalf_ctx* ctx, const void* kernel, const T& args, dim3 grid, dim3 block, hipStream_t stream, const char* expr) {
    void* argv[] = {(void*)&args};
    const hipError_t e = hipLaunchKernel(kernel, grid, block, argv, 0, stream);
    return e == hipSuccess ? MCALF_OK : set_err(ctx, MCALF_ERR_HIP, "%s failed: %s", expr, hipGetErrorString(e));
}
#define LAUNCH_BLOCK(ctx, kernel, a, grid, block, stream) \
    launch_block(ctx, kernel, a, grid, block, stream, "hipLaunchKernel(" #kernel ", " #grid ", " #block ", args, 0, " #stream ")")

inline double now_us() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3;
}

inline bool mode_reduces(int mode) { return mode == kModeLogL || mode == kModeChi2; }   // one scalar per live point (else pixel rows)

// One batch for the kernels: the mode, the rows as the DEVICE addresses them, where the results go, the stream.  from_cube: dP
// holds unit-cube rows, mapped through the prior box while decoding; d_theta (optional) receives the transformed rows.
struct LaunchReq {
    int mode; const double* dP; int64_t batch; hipStream_t stream;
    int targonly = 0, onecomp_fill = 0;
    double *d_out = nullptr, *d_model = nullptr, *d_theta = nullptr;
    bool from_cube = false;
    LaunchReq(int mode_, const double* dP_, int64_t batch_, hipStream_t stream_) : mode(mode_), dP(dP_), batch(batch_), stream(stream_) {}
    bool reduces() const { return mode_reduces(mode); }
    int rowlen(const mcalf_ctx* ctx) const { return mode == kModeOneComp ? 5 : ctx->ndim; }
};
// One call of a host-pointer entry: the caller's rows and arrays.  theta_out (from_cube only, optional): the transformed rows.
struct HostReq {
    int mode; const double* P; int64_t batch; int rowlen;
    int targonly = 0, fill = 0;
    double *out_scalar = nullptr, *out_model = nullptr;
    bool from_cube = false; double* theta_out = nullptr;
    bool reduces() const { return mode_reduces(mode); }
    // the same request on device rows (the outputs are the plan's to set)
    LaunchReq on_device(const double* dP, hipStream_t stream) const {
        LaunchReq q(mode, dP, batch, stream);
        q.targonly = targonly; q.onecomp_fill = fill; q.from_cube = from_cube;
        return q;
    }
};

// The launch record of a call (mcalf_last_launch): every entry starts it from zero, so that no field of an earlier call
// survives; the plan that ends up evaluating a host-pointer call names itself with set_path.
inline void set_path(mcalf_ctx* ctx, int path, bool pinned_in, bool pinned_out) {
    ctx->last.path = path; ctx->last.pinned_in = pinned_in ? 1 : 0; ctx->last.pinned_out = pinned_out ? 1 : 0;
}
inline void begin_call(mcalf_ctx* ctx, int path, bool pinned_in, bool pinned_out) { ctx->last = mcalf_launch_info_t(); set_path(ctx, path, pinned_in, pinned_out); }

int ensure_small(mcalf_ctx* ctx);                      // the page-locked block of small calls
int pick_device(mcalf_ctx* ctx, int requested, int* out_dev, std::string* arch);   // a usable gfx950 device (-1: the current one)
bool is_pinned_host(const void* p);
// A stream of the context: created with the context's CU mask when it has one (mcalf_set_cu_mask).
int create_stream(mcalf_ctx* ctx, hipStream_t* out, int priority = 0);

void apply_environment(mcalf_ctx* ctx);                // host_config.cpp: the environment's snapshot over the built-in values
// Entries that make no sense on a multi-device parent (device pointers belong to ONE device; a communicator, a resident
// kernel, a profile to one context) refuse it.
#define MCALF_SINGLE_ONLY(ctx, what)                                                                              \
    do {                                                                                                          \
        if ((ctx) && is_multi(ctx))                                                                               \
            return set_err(ctx, MCALF_ERR_INVALID, "%s: not available on a multi-device context (mcalf_create_multi); " \
                           "use a single-device context per GPU", what);                                          \
    } while (0)

// ---- host_launch.cpp: the batch kernels ---------------------------------------------------------------------------------
// The kernel arguments of rows [row0, row0 + nrows) of a batch (everything but the launch geometry).
// wide_stage (contexts whose LSF is wider than a tile, launch_wide): which of the launch's kernels the block is for
enum { kWideNone = 0, kWideFused = 1, kWideKernels = 2 };
KArgs make_kargs(const mcalf_ctx* ctx, const LaunchReq& q, int64_t row0, int64_t nrows, int chunk, int wide_stage = kWideNone);
int launch(mcalf_ctx* ctx, const LaunchReq& q);        // enqueue one batch on q.stream (asynchronous)
// Rows [row0, row0 + nrows) of the batch on `stream` (a row block has a stream of its own): set-up, fused kernel, finalize when tiled.
int launch_range(mcalf_ctx* ctx, const LaunchReq& q, int64_t row0, int64_t nrows, int chunk, hipStream_t stream, bool timed_ok,
                 int wide_stage = kWideNone);
// What the cube samplers (host_ns.cpp, host_ens.cpp) put around their own kernels: logL of the `n` unit-cube rows at Y into LY,
// exactly what mcalf_loglike_cube_batch_device(Y) writes; the transformed rows of U, as that launch forms them.
int cube_logl(mcalf_ctx* ctx, const double* Y, const double* LY, int64_t n, hipStream_t stream);
int cube_to_theta(mcalf_ctx* ctx, const double* U, double* theta, int64_t n, hipStream_t stream);
int launch_preflight(mcalf_ctx* ctx, int mode, int64_t batch);   // what can fail WITHOUT anything having been enqueued
int launch_finalize(mcalf_ctx* ctx, const KArgs& a, int64_t nrows, int mode, hipStream_t stream, int nparts = 0, bool signal = false);
int grow_sample_ws(mcalf_ctx* ctx, int64_t batch);     // the per-live-point workspaces of the set-up kernel
int pick_chunks(const mcalf_ctx* ctx, int64_t batch);
constexpr int kCopyStream = 1;          // aux[1]: the copy stream of the row-block pipeline; aux[0]: its second compute stream
int ensure_aux(mcalf_ctx* ctx, int naux, bool pipeline = false);
// The event pair around a fused launch while a profile is being taken (mcalf_profile_begin) and has room for it.
int profile_start(mcalf_ctx* ctx, hipStream_t stream, bool* timed);
int profile_stop(mcalf_ctx* ctx, hipStream_t stream, bool timed);

// ---- host_wide.cpp: an LSF wider than a workgroup tile ------------------------------------------------------------------
int64_t wide_rows_per_pass(const mcalf_ctx* ctx, int64_t batch);
int grow_wide_ws(mcalf_ctx* ctx, int64_t rows, bool partials, bool onecomp_rows);   // the scratch of one pass of `rows` live points
int launch_wide(mcalf_ctx* ctx, const LaunchReq& q);

// ---- host_pipeline.cpp: the row-block pipeline of a large host-pointer batch ----------------------------------------------
int ensure_stage(mcalf_ctx* ctx, size_t need);         // the page-locked staging block (h_stage) of at least `need` doubles
int run_host_pipelined(mcalf_ctx* ctx, const HostReq& h);
void host_trace_report(mcalf_ctx* ctx);                // MCALF_HOST_TRACE, the zero-copy call's and the pipeline's phases

// ---- host_multi.cpp: one process driving several devices ---------------------------------------------------------------
void multi_release(mcalf_ctx* ctx);                    // stops the workers, destroys the sub-contexts
// Rows [lo, hi) of `batch` that sub-context k of n evaluates (contiguous blocks; the arithmetic of mc-alf_amd/dist.py).
inline void multi_bounds(int64_t batch, int n, int k, int64_t* lo, int64_t* hi) {     // (shard_bounds of dist.py: sizes differ by at most one)
    const int64_t base = batch / n, extra = batch % n;
    *lo = (int64_t)k * base + std::min<int64_t>(k, extra);
    *hi = *lo + base + (k < extra ? 1 : 0);
}
int multi_active(const mcalf_ctx* ctx, int64_t batch);  // sub-contexts a batch of this size is cut over (>= 1)
// fn(sub, k, lo, hi) on every active sub-context concurrently (sub 0 on the calling thread); first error wins.
int multi_run(mcalf_ctx* ctx, int64_t batch, WorkFn fn, void* arg);      // (fn's `who` is the sub-context)

// ---- host_staged.cpp: the staged call of the host-pointer analysis entries ----------------------------------------------
// One array of a call.  `count`: elements per row for an array that is cut with the rows (`rows`), else elements in all.
// `own`: the body supplies the device side itself (a workspace, an allocation of the call) by setting its dev[] slot; the
// arena reserves nothing for it.  An array that is not `present` (an optional output the caller left NULL) has dev[] NULL.
struct StageCol { void* host; size_t elem, count; bool rows, out, present, own; };
inline StageCol stage_in(const void* host, size_t elem, size_t count, bool rows = true) {
    return {const_cast<void*>(host), elem, count, rows, false, host != nullptr, false};
}
inline StageCol stage_out(void* host, size_t elem, size_t count, bool rows = true, bool own = false) {
    return {host, elem, count, rows, true, host != nullptr, own};
}
constexpr int kStageMaxCols = 12;
enum StageShard { kStageCutRows, kStageFirstDevice };    // a multi-device context: the rows over its devices / all on its first
// The entry's device driver over `rows` rows of (sub-)context `ctx` on `stream`; dev[i] is the device side of column i.
typedef int (*StageBody)(mcalf_ctx* ctx, void** dev, int64_t rows, hipStream_t stream, void* arg);
struct StagePlan {
    StageCol cols[kStageMaxCols]; int ncols;
    int64_t batch; StageShard shard;
    int pin_in, pin_out;          // the columns whose page-lockedness the launch record reports (-1: none, reported as 0)
    StageBody body; void* arg;
};
// shard, hipSetDevice, begin_call(MCALF_PATH_HOST_STAGED), the arena, the inputs to the device in column order, the body, the
// outputs back in column order, hipStreamSynchronize -- all on the context's stream.
int run_staged(mcalf_ctx* ctx, const StagePlan& plan);

// ---- host_stream.cpp: ONE streaming launch for a large host-pointer batch ----------------------------------------------
int stream_probe_xcds(mcalf_ctx* ctx);                 // which XCDs the context's stream reaches (ctx->xcd_mask)
int stream_prepare(mcalf_ctx* ctx, int mode, int64_t batch);
int ensure_ctl(mcalf_ctx* ctx);                        // the page-locked words a launch and the host exchange (h_ctl / d_ctl)
int stream_launch(mcalf_ctx* ctx, const LaunchReq& q, int wgs, int64_t eager_rows, bool staged, bool host_rows);
bool stream_qualifies(const mcalf_ctx* ctx, int64_t batch);
void host_scale_cube(const mcalf_ctx* ctx, const double* cube, int64_t batch, double* theta);
int run_host_stream(mcalf_ctx* ctx, const HostReq& h, bool* taken);
void stream_trace_report(mcalf_ctx* ctx);

// ---- broker.cpp: resident one-theta evaluator ---------------------------------------------------------------------------
void resident_stop(mcalf_ctx* ctx);
bool resident_serves(const mcalf_ctx* ctx, int mode, int64_t batch, int rowlen, bool from_cube);
int resident_call(mcalf_ctx* ctx, const double* row, int rowlen, double* out);

// ---- host_grad.cpp: the derivative products, for host_fit.cpp -----------------------------------------------------------
// The device rows of one call: parameters [batch, ndim], the second input (V or Q; none for the gradient), the primary
// output (G, dM or HV) and logL [batch] (NULL: the context's own buffer).
struct Call { const double *P, *X; double *Y, *L; };
struct Product {
    const char* device_entry;     // the name its device-pointer entry reports
    int nws;                      // its per-row workspaces are ctx->gb[0, nws); they also cut its passes
    bool own_q;                   // false: `q` is the caller's array, no q workspace is grown (the passes are cut all the same)
    bool logl, l_out;             // logL of the batch first (the veto rule); logL is an output of the entry too
    bool has_x, x_pix, y_pix;     // a second input; X / Y rows are npix wide (else ndim)
    GradKernel seq[8];            // the kernels of a pass in order, kGradKernelCount after the last
    void (*bind)(GradArgs& a, const Call& c, size_t cell0, size_t pix0, int64_t row0);   // the row pointers of the pass at row0 (P is the driver's)
};
extern const Product kProdGrad, kProdJvp, kProdVjp, kProdHvp;
int run_product(mcalf_ctx* ctx, const Product& p, Call c, int64_t batch, hipStream_t stream);   // product `p` over device rows, on `stream`
// What host_hmc.cpp puts between its own kernels, next to cube_logl / cube_to_theta: logL into L and the gradient rows into G
// for the `n` device theta rows at P, exactly what mcalf_loglike_grad_batch_device(P) issues and writes.
int theta_logl_grad(mcalf_ctx* ctx, const double* P, double* L, double* G, int64_t n, hipStream_t stream);

// ---- host_ns.cpp: the replacement step, for host_nsrun.cpp ---------------------------------------------------------------
// The device rows of one call of the replacement primitive.
struct NsRows {
    const double *U0, *Lmin, *D; const uint64_t* sid;
    double *U, *theta, *logL; int32_t *status, *nevals, *moves;
};
// The call over `batch` device rows on `stream`; poll: the host reads the count of live rows after every step and stops at 0.
int run_ns(mcalf_ctx* ctx, const NsRows& r, int64_t batch, const mcalf_slice_opts& o, hipStream_t stream, bool poll);

// ---- host_prior.cpp: the Gaussian prior -----------------------------------------------------------------------------------
// The prior block of a (single-device) context whose box is set, for a kernel's arguments; mu is NULL when no Gaussian is set.
inline PriorDev prior_dev(const mcalf_ctx* ctx) {
    const double* g = ctx->ngauss > 0 ? ctx->d_gauss.p : nullptr;
    const size_t n = (size_t)ctx->ndim;
    return {ctx->d_prior, ctx->d_prior + n, g, g ? g + n : nullptr, g ? g + 2 * n : nullptr, ctx->ndim};
}

// How the context's parameter rows are read, for a kernel's arguments (theta_row.h).
inline RowLayout row_layout(const mcalf_ctx* ctx) {
    return {ctx->ndim, ctx->nlines, ctx->ncompmax, ctx->nfill, ctx->startind, ctx->endind, ctx->freespecres, ctx->freecont,
            ctx->conv_mode == MCALF_CONV_SAME_EDGE_JAX ? 1 : 0, ctx->specres_fixed, ctx->contval_fixed};
}

// ---- host_eqw.cpp: the equivalent-width entries -------------------------------------------------------------------------
int eqw_prepare(mcalf_ctx* ctx, const double* wl);     // mcalf_create: dlam on the device

// ---- host_kin.cpp: the optical-depth kinematics entries -----------------------------------------------------------------
int kin_prepare(mcalf_ctx* ctx, const double* wl);     // mcalf_create: wl and the cell edges on the device

// ---- comm.cpp -----------------------------------------------------------------------------------------------------------
void comm_release(mcalf_ctx* ctx);
