// libmcalf_hip.so, host side: the launch of the batch kernels -- kernel arguments, workspaces, the set-up / fused / finalize
// sequence of a row block, row blocks over the context's auxiliary streams.  (A wide-LSF context's launch is host_wide.cpp.)
#include <cmath>

#include "host_ctx.h"

int grow_sample_ws(mcalf_ctx* ctx, int64_t batch) {
    int rc;
    if ((rc = grow(ctx, ctx->d_recs, (size_t)batch * ctx->ncl_cap * kRecStride))) return rc;
    if ((rc = grow(ctx, ctx->d_taps, (size_t)batch * (2 * (size_t)ctx->n_cap + 8)))) return rc;
    if ((rc = grow(ctx, ctx->d_hdr, (size_t)batch))) return rc;
    if ((rc = grow(ctx, ctx->d_order, (size_t)batch))) return rc;
    return MCALF_OK;
}

// The kernel arguments of rows [row0, row0 + nrows) of a batch (everything but the launch geometry).
// `chunk` selects the row of the shared tap table this block writes and reads (fixed-resolution contexts).
KArgs make_kargs(const mcalf_ctx* ctx, const LaunchReq& q, int64_t row0, int64_t nrows, int chunk, int wide_stage) {
    const int mode = q.mode, rowlen = q.rowlen(ctx);
    const size_t tapTotal = 2 * (size_t)ctx->n_cap + 8;
    KArgs a = {};
    a.taps_shared = (!ctx->freespecres && mode != kModeOneComp) ? 1 : 0;
    a.recs = ctx->d_recs + (size_t)row0 * ctx->ncl_cap * kRecStride;
    a.taps = ctx->d_taps + (a.taps_shared ? (size_t)chunk : (size_t)row0) * tapTotal;
    a.hdr = ctx->d_hdr + row0;
    a.nu = ctx->d_nu; a.obj = ctx->d_obj; a.ispec2 = ctx->d_ispec2; a.lgis = ctx->d_lgis; a.err = ctx->d_err;
    a.asymm = (mode == kModeLogL) ? ctx->asymm : 0; a.veto4 = ctx->veto4; a.veto5 = ctx->veto5;
    a.P = q.dP + (size_t)row0 * rowlen;
    a.partial = ctx->d_partial ? ctx->d_partial + (size_t)row0 * ctx->ntiles * 4 : nullptr;
    a.out = q.d_out ? q.d_out + row0 : nullptr;
    a.model = q.d_model ? q.d_model + (size_t)row0 * ctx->npix : nullptr;
    a.lines = ctx->d_lines; a.tabs = ctx->d_tabs; a.wtab = ctx->d_wtab; a.segok = ctx->d_segok; a.dnu_seg = ctx->dnu_seg;
    a.npix = (int)ctx->npix; a.ndim = ctx->ndim; a.ntiles = ctx->ntiles; a.tile = ctx->tile;
    a.n_cap = ctx->n_cap; a.ncl_cap = ctx->ncl_cap;
    a.nlines = ctx->nlines; a.ncompmax = ctx->ncompmax; a.nfill = ctx->nfill;
    a.startind = ctx->startind; a.endind = ctx->endind;
    a.freespecres = ctx->freespecres; a.freecont = ctx->freecont;
    a.targonly = q.targonly; a.mode = mode; a.jax_half = ctx->jax_half; a.onecomp_fill = q.onecomp_fill;
    a.selfhalo = ctx->selfhalo; a.seg_search = ctx->seg_search ? ctx->seg_nreal : 0;
    a.specres_fixed = ctx->specres_fixed; a.contval_fixed = ctx->contval_fixed; a.velstep = ctx->velstep;
    a.log2pi = std::log(2.0 * M_PI);
    a.prior_lo = q.from_cube ? ctx->d_prior : nullptr;
    a.prior_hi = q.from_cube ? ctx->d_prior + ctx->ndim : nullptr;
    a.theta_out = (q.from_cube && q.d_theta) ? q.d_theta + (size_t)row0 * ctx->ndim : nullptr;
    a.prior_int = ctx->prior_int;
    a.nitems = (int)(nrows * ctx->ntiles);
    a.nrows = (int)nrows;
    a.queue = ctx->d_queue + chunk;
    if (wide_stage == kWideFused) {
        // the convolution-free fused launch of a wide-LSF context: no resolution exceeds this step (hires_fitter.py:445), the
        // continuum is 1 -- the wide kernels apply both afterwards (the layout fields startind / endind stay the context's)
        // (JAX semantics convolve unconditionally on their fixed grid: a grid of half-width 0 -- the single tap 1 -- is the
        // identity, and its edge reset covers no pixel; velstep stays, sigma must remain finite there)
        a.freecont = 0; a.contval_fixed = 1.0;
        if (ctx->conv_mode == MCALF_CONV_SAME_EDGE_JAX) a.jax_half = 0; else a.velstep = 1e300;
    } else if (wide_stage == kWideKernels) {
        a.n_cap = ctx->wide_n_cap;                        // (arguments of the wide kernels)
    }
    return a;
}

// The finalize kernel of a tiled spectrum behind the fused kernel of `a` (adds the per-tile partials in fixed order).
int launch_finalize(mcalf_ctx* ctx, const KArgs& a, int64_t nrows, int mode, hipStream_t stream, int nparts, bool signal) {
    const int fb = 256;
    const double* partial = a.partial;
    double* out = a.out;
    long n = (long)nrows;
    int ntiles = nparts > 0 ? nparts : ctx->ntiles, m = mode, asymm = a.asymm;   // (partials per live point)
    double v4 = a.veto4, v5 = a.veto5;
    // signal: the streaming launch of a tiled spectrum -- the kernel tells the host (h_ctl[kCtlFinalized] = the launch's stamp)
    unsigned int* fin_count = signal ? &ctx->d_sctl->fin_exited : nullptr;
    unsigned int* done_word = signal ? ctx->d_ctl + kCtlFinalized : nullptr;
    unsigned int gen = ctx->stream_gen;
    void* fargs[] = {(void*)&partial, (void*)&out, (void*)&n, (void*)&ntiles, (void*)&m, (void*)&asymm, (void*)&v4, (void*)&v5,
                     (void*)&fin_count, (void*)&done_word, (void*)&gen};
    HIP_TRY(ctx, hipLaunchKernel(finalize_kernel_ptr(), dim3((unsigned)((nrows + fb - 1) / fb)), dim3(fb), fargs, 0, stream));
    return MCALF_OK;
}

int profile_start(mcalf_ctx* ctx, hipStream_t stream, bool* timed) {
    if ((*timed = ctx->profiling && ctx->ev_used + 2 <= ctx->ev.size())) HIP_TRY(ctx, hipEventRecord(ctx->ev[ctx->ev_used], stream));
    return MCALF_OK;
}
int profile_stop(mcalf_ctx* ctx, hipStream_t stream, bool timed) {
    if (timed) HIP_TRY(ctx, hipEventRecord(ctx->ev[ctx->ev_used + 1], stream));
    if (timed) ctx->ev_used += 2;
    return MCALF_OK;
}

// Enqueue rows [row0, row0 + nrows) of a batch on `stream`: set-up kernel, fused kernel, finalize when tiled.
int launch_range(mcalf_ctx* ctx, const LaunchReq& q, int64_t row0, int64_t nrows, int chunk, hipStream_t stream, bool timed_ok, int wide_stage) {
    const int mode = q.mode;
    int rc;
    KArgs a = make_kargs(ctx, q, row0, nrows, chunk, wide_stage);
    // Persistent grid = the workgroup slots of the chip (2 per CU: LDS and the 4 waves per SIMD the kernel's
    // registers allow); correctness does not depend on how many of them are resident at once.  Used once every
    // slot sees at least four items: measured on MI355X, 8 items per slot (config C) -3.5 % and 160 per slot
    // (config E) -12 % in kernel time, but 2 per slot (config B) +2 % -- there the queue and the prefetch cost
    // more than the two workgroup launches they replace, so small launches keep one workgroup per item.
    const int64_t slots = 2LL * ctx->num_cu;
    a.persist = (ctx->persist && a.nitems >= 4 * slots) ? 1 : 0;
    // Ordered hand-out while a slot sees at most 16 items: measured on MI355X, config C's spectrum, -2.2 % kernel time
    // at 8 items per slot (4096 live points) and nothing at 64 (32768), where the ordering workgroup -- its keys no
    // longer fit its registers -- would lengthen the set-up kernel by 47 us instead.
    a.order = (a.persist && ctx->ordered && ctx->selfhalo && mode != kModeOneComp && a.nitems <= 16 * slots)
                  ? ctx->d_order + row0 : nullptr;
    const dim3 grid((unsigned)(a.persist ? slots : a.nitems)), block(kBlock);
    ctx->last.persistent = a.persist; ctx->last.grid = (int32_t)grid.x; ctx->last.items = a.nitems;
    ctx->last.lines_per_sync = ctx->lps; ctx->last.selfhalo = ctx->selfhalo; ctx->last.ordered = a.order ? 1 : 0;
    // Small launches (the one-theta-at-a-time solvers, a handful of live points): ONE kernel, every workgroup sets
    // its live point up itself (mcalf_fused_kernel<..., kInline = true>) -- the set-up kernel and the dependent-launch
    // gap behind it are a fifth of such a call's latency.  Same set-up code, same bits.
    const bool inl = !a.persist && a.nitems <= ctx->inline_max_items;
    ctx->last.inline_setup = inl ? 1 : 0;
    if (!inl) {
        const int per_wg = ctx->setup_block / 64;             // live points per set-up workgroup (one wave each)
        const dim3 sgrid((unsigned)((nrows + per_wg - 1) / per_wg) + (a.order ? 1u : 0u)), sblock((unsigned)ctx->setup_block);
        long nrows_arg = (long)nrows;
        void* sargs[] = {(void*)&a, (void*)&nrows_arg};
        HIP_TRY(ctx, hipLaunchKernel(sample_kernel_ptr(ctx->conv_mode == MCALF_CONV_SAME_EDGE_JAX), sgrid, sblock, sargs, 0, stream));
    }
    bool timed = false;
    if (timed_ok && (rc = profile_start(ctx, stream, &timed))) return rc;
    {
        void* kargs[] = {(void*)&a};
        HIP_TRY(ctx, hipLaunchKernel(fused_kernel_ptr(ctx->conv_mode == MCALF_CONV_SAME_EDGE_JAX, ctx->selfhalo != 0, ctx->lps, inl),
                                     grid, block, kargs, inl ? ctx->lds_bytes_inline : ctx->lds_bytes, stream));
    }
    HIP_TRY(ctx, hipGetLastError());
    if ((rc = profile_stop(ctx, stream, timed))) return rc;
    if (q.reduces() && ctx->ntiles > 1) return launch_finalize(ctx, a, nrows, mode, stream);
    return MCALF_OK;
}

// Row blocks a *_device batch is issued in.  Automatic = ONE: measured on MI355X (config C, 4096 live points), every
// extra block costs ~20 us of cross-stream event traffic and buys nothing, because the persistent fused kernel
// leaves no launch tail for the next block to fill (0.267 / 0.287 / 0.309 / 0.327 ms per batch with 1 / 2 / 3 / 4
// blocks).  The knob stays for callers that want to interleave their own work, and for the host-pointer entry,
// where blocks overlap the PCIe copies with the kernels (run_host_pipelined).
int pick_chunks(const mcalf_ctx* ctx, int64_t batch) {
    int n = ctx->chunks_req > 0 ? ctx->chunks_req : 1;
    if (n > kMaxChunks) n = kMaxChunks;
    if ((int64_t)n > batch) n = (int)batch;
    return n < 1 ? 1 : n;
}

int ensure_aux(mcalf_ctx* ctx, int naux, bool pipeline) {
    if (!ctx->ev_fork) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    for (int i = 0; i < naux; ++i) {
        if (!ctx->aux[i]) {
            const int rc = create_stream(ctx, &ctx->aux[i], !pipeline ? 0 : (i == kCopyStream ? +1 : -1));
            if (rc) return rc;
        }
        if (!ctx->ev_join[i]) HIP_TRY(ctx, hipEventCreateWithFlags(&ctx->ev_join[i], hipEventDisableTiming));
    }
    return MCALF_OK;
}

static int64_t chunk_begin(int64_t batch, int nchunks, int c) { return batch * c / nchunks; }

// Everything of a launch that can fail WITHOUT anything having been enqueued: the range check and the growth of
// the per-sample workspaces (hipMalloc).  The collective entry runs it before it enqueues anything, so that a rank
// that fails here can still take its part in the exchange (mcalf_loglike_gatherv_device).
int launch_preflight(mcalf_ctx* ctx, int mode, int64_t batch) {
    if (batch == 0) return MCALF_OK;
    if (batch < 0 || batch * (int64_t)ctx->ntiles > 0x7fff0000LL)
        return set_err(ctx, MCALF_ERR_RANGE, "batch %lld too large", (long long)batch);
    int rc;
#ifdef MCALF_TESTING
    if (ctx->fail_preflight) return set_err(ctx, MCALF_ERR_NOMEM, "workspace growth failed (injected by MCALF_TEST_FAIL_PREFLIGHT)");
#endif
    if (mode_reduces(mode) && ctx->ntiles > 1 && (rc = grow(ctx, ctx->d_partial, (size_t)batch * ctx->ntiles * 4)))
        return rc;
    return grow_sample_ws(ctx, batch);
}

// Enqueue one batch on q.stream (asynchronous).  With several row blocks, blocks 1.. go to the context's
// auxiliary streams between a fork event recorded on the stream and join events it waits for, so the call
// keeps plain stream semantics for the caller (and can be captured into a hipGraph).
int launch(mcalf_ctx* ctx, const LaunchReq& q) {
    const int64_t batch = q.batch; const hipStream_t stream = q.stream;
    if (batch == 0) return MCALF_OK;
    int rc;
    if (ctx->wide) return launch_wide(ctx, q);
    // MCALF_STREAM_DEVICE=1 (diagnostic): device-pointer batches through the streaming single launch as well -- every
    // row is there from the start, so the whole grid sets up eight live points per workgroup and goes on to the items
    if (ctx->stream_device && q.reduces() && !q.from_cube && !q.d_model && ctx->chunks_req <= 1 &&
        stream_qualifies(ctx, batch) && ctx->xcd_mask == (1u << kXcds) - 1u) {
        if ((rc = stream_prepare(ctx, q.mode, batch))) return rc;
        ctx->last.row_blocks = 1;
        if (ctx->stream_device == 2) {                     // ... with the host entries' split: a few rows eagerly, the rest by dedicated workgroups
            const int grid = 2 * ctx->num_cu, wgs = std::min((ctx->stream_wgs + kXcds - 1) / kXcds * kXcds, grid / 2 / kXcds * kXcds);
            const int64_t first_rows = ((grid - wgs) / kXcds + ctx->ntiles - 1) / ctx->ntiles;
            return stream_launch(ctx, q, wgs, (first_rows + 7) / 8, false, false);
        }
        return stream_launch(ctx, q, 0, batch, false, false);
    }
    if ((rc = launch_preflight(ctx, q.mode, batch))) return rc;
    const int nchunks = ctx->profiling ? 1 : pick_chunks(ctx, batch);
    ctx->last.row_blocks = nchunks;
    if (nchunks == 1) return launch_range(ctx, q, 0, batch, 0, stream, true);
    if ((rc = ensure_aux(ctx, nchunks - 1))) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev_fork, stream));
    for (int c = 0; c < nchunks; ++c) {
        const int64_t r0 = chunk_begin(batch, nchunks, c), r1 = chunk_begin(batch, nchunks, c + 1);
        hipStream_t st = (c == 0) ? stream : ctx->aux[c - 1];
        if (c > 0) HIP_TRY(ctx, hipStreamWaitEvent(st, ctx->ev_fork, 0));
        if ((rc = launch_range(ctx, q, r0, r1 - r0, c, st, false))) return rc;
        if (c > 0) HIP_TRY(ctx, hipEventRecord(ctx->ev_join[c - 1], st));
    }
    for (int c = 1; c < nchunks; ++c) HIP_TRY(ctx, hipStreamWaitEvent(stream, ctx->ev_join[c - 1], 0));
    return MCALF_OK;
}

// logL of the `n` unit-cube rows at Y into LY, exactly what mcalf_loglike_cube_batch_device(Y) writes.
int cube_logl(mcalf_ctx* ctx, const double* Y, const double* LY, int64_t n, hipStream_t stream) {
    LaunchReq q(kModeLogL, Y, n, stream);
    q.d_out = const_cast<double*>(LY); q.from_cube = true;
    return launch(ctx, q);
}

// The transformed rows of the `n` unit-cube rows at U, as the cube launch forms them.
int cube_to_theta(mcalf_ctx* ctx, const double* U, double* theta, int64_t n, hipStream_t stream) {
    const double *lo = ctx->d_prior, *hi = ctx->d_prior + ctx->ndim, *cube = U;
    long total = (long)((size_t)n * (size_t)ctx->ndim);
    int nd = ctx->ndim, slot = ctx->startind, as_int = ctx->prior_int;
    void* kargs[] = {(void*)&lo, (void*)&hi, (void*)&cube, (void*)&total, (void*)&nd, (void*)&slot, (void*)&as_int, (void*)&theta};
    HIP_TRY(ctx, hipLaunchKernel(scale_cube_kernel_ptr(), dim3((unsigned)((total + 255) / 256)), dim3(256), kargs, 0, stream));
    return MCALF_OK;
}
