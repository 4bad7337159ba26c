// libmcalf_hip.so, host side: the row-block pipeline of a large host-pointer batch (run_host_pipelined) -- its plan, its
// staging copy and helper threads, its tracing -- and the page-locked staging block it shares with the streaming launch.
#include <new>

#include "host_ctx.h"

// MCALF_HOST_TRACE=1 (diagnostic; accumulators in the context: host_ctx.h): where a call of the row-block pipeline spends its host
// time, printed when the context is destroyed (mean microseconds per call): staging copies by the calling thread (and the rate they
// ran at), copies its helpers took over, enqueueing split by API call, the wait for the streams, the copy of the results.
// MCALF_HOST_TRACE=2: additionally the GPU-side timeline of the LAST pipelined call -- per row block the times (us after the call
// began) at which its H2D copy started and ended and its kernels ended on the device, and when the host enqueued it.
namespace {
// The staging copy of one call, shared between the calling thread (blocks from the front, in the order the GPU wants
// them) and the helper threads (blocks from the back): whoever claims a block copies it; `copied` says it is there.
struct StageJob {
    const double* src; double* dst; int rowlen; int nchunks;
    const int64_t* bounds;
    std::atomic<int> claim[kMaxChunks];
    std::atomic<int> copied[kMaxChunks];
    std::atomic<long long> helper_bytes{0};
};
int stage_from_back(void*, int64_t, int64_t, void* arg) {
    StageJob* j = static_cast<StageJob*>(arg);
    for (int c = j->nchunks - 1; c >= 1; --c) {            // (block 0 is the calling thread's: nothing may delay it)
        int free_ = 0;
        if (!j->claim[c].compare_exchange_strong(free_, 2)) { if (free_ == 1) break; else continue; }   // met the calling thread: done
        const size_t off = (size_t)j->bounds[c] * j->rowlen, cnt = (size_t)(j->bounds[c + 1] - j->bounds[c]) * j->rowlen;
        std::memcpy(j->dst + off, j->src + off, cnt * sizeof(double));
        j->helper_bytes.fetch_add((long long)(cnt * sizeof(double)), std::memory_order_relaxed);
        j->copied[c].store(1, std::memory_order_release);
    }
    return 0;
}
}  // namespace

void host_trace_report(mcalf_ctx* ctx) {
    if (ctx->host_trace && ctx->htrace.small_calls > 0) {
        const HostTrace& t = ctx->htrace;
        const double n = (double)t.small_calls;
        std::fprintf(stderr, "mcalf host trace (zero-copy small calls, %ld calls; us per call): copy into the page-locked block %.2f, launch calls %.2f, "
                     "theta rows on the host %.2f, wait for the results %.2f, results out %.2f\n", t.small_calls,
                     t.small_prep_us / n, t.small_launch_us / n, t.small_copy_us / n, t.small_poll_us / n, t.small_out_us / n);
        if (ctx->htrace.calls == 0) ctx->htrace = HostTrace();
    }
    if (!ctx->host_trace || ctx->htrace.calls == 0) return;
    const HostTrace& t = ctx->htrace;
    const double n = (double)t.calls;
    std::fprintf(stderr, "mcalf host trace (row-block pipeline, %ld calls, %.1f blocks per call; us per call): staging copy by the caller %.1f "
                 "(%.2f GB/s), by helpers %.0f KB (waited %.1f), first block enqueued at %.1f, enqueue %.1f (of it: hipMemcpyAsync calls %.1f [longest single "
                 "call %.1f], event record + wait %.1f, launches %.1f), wait for the streams %.1f, "
                 "results out %.1f\n", t.calls, (double)t.blocks / n, t.stage_us / n, t.stage_us > 0 ? t.stage_bytes / t.stage_us * 1e-3 : 0.0,
                 t.helper_bytes / n / 1024.0, t.helper_wait_us / n, t.first_enqueued_us / n, t.enqueue_us / n, t.call_copy_us / n, t.call_copy_max,
                 t.call_order_us / n, t.call_launch_us / n, t.wait_us / n, t.out_us / n);
    ctx->htrace = HostTrace();
    const BlockTimeline& b = ctx->btrace;
    for (int c = 0; c < b.n; ++c)
        std::fprintf(stderr, "mcalf host trace, last call (%s rows), block %d: %ld rows, enqueued by the host at %.1f us (calls: copy %.1f, ordering %.1f, launches %.1f); "
                     "on the device: H2D %.1f .. %.1f, kernels done %.1f\n", b.pinned ? "page-locked" : "pageable", c, b.rows[c], b.host_enq[c], b.call_h2d[c], b.call_order[c],
                     b.call_launch[c], b.h2d0[c] * 1e3, b.h2d1[c] * 1e3, b.done[c] * 1e3);
    if (b.n) std::fprintf(stderr, "mcalf host trace, last call: the stream waits returned %.1f us after the call began\n", b.sync_us);
    ctx->btrace = BlockTimeline();
}

// The row blocks of a pipelined host-pointer call.  The FIRST block is sized by BYTES (ctx->host_first_kb KiB of
// parameter rows: the GPU starts after ~10 us of staging whatever the batch is -- as 1/8 of the batch, config E's first
// block was 0.8 MB of host memcpy before the first kernel), each following block twice the one before, the last takes
// the rest (large launches run the persistent grid and leave fewer tails).  An explicit request (mcalf_set_chunks) gives
// equal blocks, MCALF_HOST_PLAN relative sizes.
static int plan_row_blocks(const mcalf_ctx* ctx, int64_t batch, int rowlen, bool pin_in, int64_t* bounds) {
    int weights[kMaxChunks];
    int nchunks = 0;
    if (ctx->chunks_req > 0 || ctx->host_plan_n > 0) {
        if (ctx->chunks_req > 0) for (nchunks = 0; nchunks < ctx->chunks_req && nchunks < kMaxChunks; ++nchunks) weights[nchunks] = 1;
        else for (nchunks = 0; nchunks < ctx->host_plan_n; ++nchunks) weights[nchunks] = ctx->host_plan[nchunks];
        if ((int64_t)nchunks > batch) nchunks = (int)batch;
        int total = 0, run = 0;
        for (int c = 0; c < nchunks; ++c) total += weights[c];
        bounds[0] = 0;
        for (int c = 0; c < nchunks; ++c) { run += weights[c]; bounds[c + 1] = batch * run / total; }
        return nchunks;
    }
    // page-locked rows need no staging copy: the first block only has to cover the latency of its own H2D command
    int64_t first = std::max<int64_t>(64, (int64_t)ctx->host_first_kb * 1024 / ((int64_t)rowlen * (int64_t)sizeof(double)));
    if (pin_in) first *= 2;
    bounds[0] = 0;
    int64_t size = first, at = 0;
    while (nchunks < kMaxChunks - 1 && at + size + size / 2 < batch) {      // (no sliver at the end: the last block takes the rest)
        at += size;
        bounds[++nchunks] = at;
        size *= 2;
    }
    bounds[++nchunks] = batch;
    return nchunks;
}

int ensure_stage(mcalf_ctx* ctx, size_t need) {
    if (need <= ctx->h_stage.cap) return MCALF_OK;
    if (ctx->h_stage) HIP_TRY(ctx, hipHostFree(ctx->h_stage));
    ctx->h_stage.p = nullptr; ctx->h_stage.cap = 0;
    // coherent: the streaming kernel reads rows of this block while the host is still writing later ones
    HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_stage.p, need * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
    ctx->h_stage.cap = need;
    return MCALF_OK;
}

// Large scalar-output batches through host pointers: the rows are cut into blocks; the H2D copies of ALL blocks go to a
// copy stream of their own, one behind the other as the host stages them, and block k's kernels (set-up + fused, on two
// alternating streams) wait for the event behind its copy -- so block k+1's rows are in HBM long before block k's kernels
// end, and its set-up runs in their tail.  (Round 5 queued every block's copy on the block's own stream: the copy of
// block k+2 then waited for the kernels of block k, and the GPU idled for the copy + set-up at every second block
// boundary -- measured with MCALF_HOST_TRACE=2, profiles/r06_pipeline_timeline.txt.)  Pageable caller memory
// is staged through a page-locked block of the context (the host copies block k+1 in while the GPU works on
// block k; with MCALF_STAGE_THREADS helper threads copy the batch's last blocks meanwhile); page-locked caller memory
// is used by the copy engines directly.
int run_host_pipelined(mcalf_ctx* ctx, const HostReq& h) {
    const double* P = h.P; double* out_scalar = h.out_scalar;
    const int64_t batch = h.batch; const int rowlen = h.rowlen;
    int rc;
    const bool trace = ctx->host_trace != 0;
    const double t_begin = trace ? now_us() : 0.0;
    const bool pin_in = is_pinned_host(P), pin_out = is_pinned_host(out_scalar);
    int64_t bounds[kMaxChunks + 1];
    int nchunks = plan_row_blocks(ctx, batch, rowlen, pin_in, bounds);
    if (ctx->profiling) { nchunks = 1; bounds[1] = batch; }
    if ((rc = ensure_aux(ctx, 2, true))) return rc;
    for (hipEvent_t& e : ctx->ev_h2d)
        if (!e) HIP_TRY(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    if (h.reduces() && ctx->ntiles > 1 && (rc = grow(ctx, ctx->d_partial, (size_t)batch * ctx->ntiles * 4))) return rc;
    if ((rc = grow_sample_ws(ctx, batch))) return rc;
    if ((rc = ensure_stage(ctx, (pin_in ? 0 : (size_t)batch * rowlen) + (pin_out ? 0 : (size_t)batch)))) return rc;
    double* stage_in = pin_in ? nullptr : ctx->h_stage;
    hipStream_t copy_stream = ctx->aux[kCopyStream];
    double* stage_out = pin_out ? out_scalar : ctx->h_stage + (pin_in ? 0 : (size_t)batch * rowlen);
    // Results: the kernels write logL straight into the page-locked block (its device address), 8 bytes per live
    // point over PCIe, which saves the D2H copy command of every block -- the last one is on the critical path.
    double* d_stage_out = nullptr;
    if (hipHostGetDevicePointer((void**)&d_stage_out, stage_out, 0) != hipSuccess) {
        (void)hipGetLastError();
        d_stage_out = nullptr;                            // (caller's page-locked memory that is not device-mapped)
    }
    set_path(ctx, MCALF_PATH_HOST_PIPELINED, pin_in, pin_out); ctx->last.row_blocks = nchunks;
    LaunchReq q = h.on_device(ctx->d_P, ctx->stream);         // (every row block on a stream of its own: below)
    q.d_out = d_stage_out ? d_stage_out : ctx->d_out.p;
    hipStream_t streams[2] = {ctx->stream, ctx->aux[0]};
    // Helpers of the staging copy (pageable rows, at least 1 MB of them): they take blocks from the back while this
    // thread stages and enqueues from the front.
    StageJob job;
    int helpers = 0;
    if (!pin_in && ctx->stage_threads > 0 && nchunks > 2 && (size_t)batch * rowlen * sizeof(double) >= ((size_t)1 << 20)) {
        job.src = P; job.dst = stage_in; job.rowlen = rowlen; job.nchunks = nchunks; job.bounds = bounds;
        for (int c = 0; c < kMaxChunks; ++c) { job.claim[c].store(0, std::memory_order_relaxed); job.copied[c].store(0, std::memory_order_relaxed); }
        while ((int)ctx->stagers.size() < ctx->stage_threads) {
            std::unique_ptr<HostWorker> w(new (std::nothrow) HostWorker());
            if (!w) break;
            w->start();
            ctx->stagers.push_back(std::move(w));
        }
        helpers = (int)ctx->stagers.size();
        for (int h = 0; h < helpers; ++h) ctx->stagers[h]->post(stage_from_back, &job, 0, 0);
    }
    // A failure in block k leaves blocks < k in flight on both streams, reading the staging block / the caller's
    // page-locked rows and writing the caller's results: never return under them (the next call may free the
    // staging block, the caller its arrays).  Every error below therefore BREAKS out of the loop and is reported behind
    // the waits for the helpers and the three streams.
    hipError_t he = hipSuccess;
    const char* what = "";
    rc = MCALF_OK;
    double t_stage = 0, t_enq = 0, t_hwait = 0, t_first = 0, stage_bytes = 0;
    const bool timeline = ctx->host_trace >= 2;
    hipEvent_t tev[3 * kMaxChunks + 1] = {};
    if (timeline) {
        for (hipEvent_t& e : tev) (void)hipEventCreate(&e);
        (void)hipEventRecord(tev[3 * kMaxChunks], ctx->stream);
        ctx->btrace = BlockTimeline();
        ctx->btrace.pinned = pin_in ? 1 : 0;
    }
    for (int c = 0; c < nchunks && rc == MCALF_OK && he == hipSuccess; ++c) {
        const int64_t r0 = bounds[c], n = bounds[c + 1] - r0;
        if (n == 0) continue;
        hipStream_t st = streams[c & 1];
        const double* src = P + (size_t)r0 * rowlen;
        const double t0 = trace ? now_us() : 0.0;
        if (!pin_in) {
            int free_ = 0;
            if (helpers == 0 || job.claim[c].compare_exchange_strong(free_, 1)) {
                std::memcpy(stage_in + (size_t)r0 * rowlen, src, (size_t)n * rowlen * sizeof(double));
                stage_bytes += (double)n * rowlen * sizeof(double);
                if (trace) t_stage += now_us() - t0;
            } else {                                      // a helper has it (or has had it): wait for its last byte
                while (job.copied[c].load(std::memory_order_acquire) == 0) __builtin_ia32_pause();
                if (trace) t_hwait += now_us() - t0;
            }
            src = stage_in + (size_t)r0 * rowlen;
        }
        const double t1 = trace ? now_us() : 0.0;
        if (timeline) (void)hipEventRecord(tev[3 * c], copy_stream);
        const double tc0 = trace ? now_us() : 0.0;
        he = hipMemcpyAsync(ctx->d_P + (size_t)r0 * rowlen, src, (size_t)n * rowlen * sizeof(double), hipMemcpyHostToDevice, copy_stream);
        if (he != hipSuccess) { what = "H2D copy of a row block"; break; }
        const double tc1 = trace ? now_us() : 0.0;
        if (timeline) (void)hipEventRecord(tev[3 * c + 1], copy_stream);
        he = hipEventRecord(ctx->ev_h2d[c], copy_stream);
        if (he == hipSuccess) he = hipStreamWaitEvent(st, ctx->ev_h2d[c], 0);
        if (he != hipSuccess) { what = "ordering a row block's kernels behind its H2D copy"; break; }
        const double tc2 = trace ? now_us() : 0.0;
        rc = launch_range(ctx, q, r0, n, c, st, nchunks == 1);
        if (rc != MCALF_OK) break;
        if (!d_stage_out) {
            he = hipMemcpyAsync(stage_out + r0, ctx->d_out + r0, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st);
            if (he != hipSuccess) { what = "D2H copy of a result block"; break; }
        }
        if (trace) {
            const double tc3 = now_us();
            ctx->htrace.call_copy_us += tc1 - tc0; ctx->htrace.call_order_us += tc2 - tc1; ctx->htrace.call_launch_us += tc3 - tc2;
            ctx->htrace.call_copy_max = std::max(ctx->htrace.call_copy_max, tc1 - tc0);
            if (timeline) { ctx->btrace.call_h2d[c] = tc1 - tc0; ctx->btrace.call_order[c] = tc2 - tc1; ctx->btrace.call_launch[c] = tc3 - tc2; }
        }
        if (timeline) { (void)hipEventRecord(tev[3 * c + 2], st); ctx->btrace.rows[c] = (long)n; ctx->btrace.host_enq[c] = now_us() - t_begin; ctx->btrace.n = c + 1; }
        if (trace) { const double t2 = now_us(); t_enq += t2 - t1; if (c == 0) t_first = t2 - t_begin; }
    }
    for (int h = 0; h < helpers; ++h) (void)ctx->stagers[h]->wait();      // (the job lives on this frame)
    const double t_w0 = trace ? now_us() : 0.0;
    const hipError_t s0 = hipStreamSynchronize(ctx->stream);
    hipError_t s1 = (nchunks > 1) ? hipStreamSynchronize(ctx->aux[0]) : hipSuccess;
    { const hipError_t s2 = hipStreamSynchronize(copy_stream); if (s1 == hipSuccess) s1 = s2; }    // (a copy no kernel waited for, after a failure)
    const double t_w1 = trace ? now_us() : 0.0;
    if (timeline) {                                       // (read and released whatever the call's outcome)
        ctx->btrace.sync_us = t_w1 - t_begin;
        for (int c = 0; c < ctx->btrace.n; ++c) {
            (void)hipEventElapsedTime(&ctx->btrace.h2d0[c], tev[3 * kMaxChunks], tev[3 * c]);
            (void)hipEventElapsedTime(&ctx->btrace.h2d1[c], tev[3 * kMaxChunks], tev[3 * c + 1]);
            (void)hipEventElapsedTime(&ctx->btrace.done[c], tev[3 * kMaxChunks], tev[3 * c + 2]);
        }
        for (hipEvent_t e : tev) if (e) (void)hipEventDestroy(e);
        (void)hipGetLastError();
    }
    if (rc != MCALF_OK) return rc;                                   // (message set by launch_range)
    if (he != hipSuccess) return set_err(ctx, MCALF_ERR_HIP, "%s failed: %s", what, hipGetErrorString(he));
    if (s0 != hipSuccess || s1 != hipSuccess)
        return set_err(ctx, MCALF_ERR_HIP, "stream synchronisation failed: %s", hipGetErrorString(s0 != hipSuccess ? s0 : s1));
    if (!pin_out) std::memcpy(out_scalar, stage_out, (size_t)batch * sizeof(double));
    if (trace) {
        HostTrace& t = ctx->htrace;
        t.calls++; t.blocks += nchunks; t.stage_us += t_stage; t.stage_bytes += stage_bytes; t.helper_wait_us += t_hwait;
        t.helper_bytes += helpers ? (double)job.helper_bytes.load() : 0.0; t.enqueue_us += t_enq; t.first_enqueued_us += t_first;
        t.wait_us += t_w1 - t_w0; t.out_us += now_us() - t_w1;
    }
    return MCALF_OK;
}
