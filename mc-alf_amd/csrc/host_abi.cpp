// libmcalf_hip.so, host side: contexts and the C ABI of include/mcalf_hip.h -- creation and teardown, the device-pointer
// and host-pointer entries and the plan of a host-pointer call, prior transform, diagnostics.  (The launch of the batch
// kernels is host_launch.cpp, a wide-LSF context's host_wide.cpp, the row-block pipeline host_pipeline.cpp, the streaming
// launch host_stream.cpp, the resident evaluator and the likelihood broker broker.cpp, the RCCL gather comm.cpp; the
// kernels are kernels.hip.)  There is no CPU fallback: every entry point fails with MCALF_ERR_NODEVICE when no gfx950
// device is present.
#include <cmath>
#include <new>

#include "host_ctx.h"

static thread_local std::string g_last_error;
void set_last_error(const std::string& msg) { g_last_error = msg; }

int set_err(mcalf_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    if (ctx) ctx->err = buf;
    return code;
}

int pick_device(mcalf_ctx* ctx, int requested, int* out_dev, std::string* arch) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return set_err(ctx, MCALF_ERR_NODEVICE, "no HIP device available (%s); libmcalf_hip has no CPU fallback",
                       e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    int dev = requested;
    if (dev < 0) {
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
    }
    if (dev >= count) return set_err(ctx, MCALF_ERR_INVALID, "device %d out of range (count %d)", dev, count);
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return set_err(ctx, MCALF_ERR_NODEVICE, "device %d is %s; this library is built for gfx950 only", dev,
                       prop.gcnArchName);
    *out_dev = dev;
    if (arch) *arch = prop.gcnArchName;
    return MCALF_OK;
}

static int upload_tables(mcalf_ctx* ctx, double** d_tabs) {
    HIP_TRY(ctx, hipMalloc((void**)d_tabs, sizeof(VT_T_HOST)));
    HIP_TRY(ctx, hipMemcpy(*d_tabs, VT_T_HOST, sizeof(VT_T_HOST), hipMemcpyHostToDevice));
    return MCALF_OK;
}

#ifndef MCALF_SRC_HASH
#define MCALF_SRC_HASH "unstamped"      // mc-alf_amd/build.py passes the sha256 of the kernel sources
#endif
extern "C" const char* mcalf_version(void) { return "mcalf_hip 0.4 (gfx950, abi " MCALF_STR(MCALF_ABI_VERSION) ") src " MCALF_SRC_HASH; }

extern "C" const char* mcalf_last_error(const mcalf_ctx* ctx) {
    return ctx ? ctx->err.c_str() : g_last_error.c_str();
}

// Everything that is not a plain free, in order; the context's buffers (DevBuf) go with `delete ctx`, which is after the
// resident kernel has been told to leave.
extern "C" void mcalf_destroy(mcalf_ctx* ctx) {
    if (!ctx) return;
    if (is_multi(ctx) || ctx->pool) {                     // a multi-device parent owns its sub-contexts and workers, nothing else
        multi_release(ctx);
        delete ctx;
        return;
    }
    stream_trace_report(ctx);
    host_trace_report(ctx);
    for (auto& w : ctx->stagers) w->stop();
    ctx->stagers.clear();
    (void)hipSetDevice(ctx->device);
    comm_release(ctx);
    resident_stop(ctx);
    if (ctx->res_stream) (void)hipStreamDestroy(ctx->res_stream);
    for (hipEvent_t e : ctx->ev) (void)hipEventDestroy(e);
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_ns) (void)hipEventDestroy(ctx->ev_ns);
    for (hipEvent_t e : ctx->ev_h2d)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_join)
        if (e) (void)hipEventDestroy(e);
    for (hipStream_t st : ctx->aux)
        if (st) (void)hipStreamDestroy(st);
    if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
    if (ctx->ev_kernels) (void)hipEventDestroy(ctx->ev_kernels);
    for (hipEvent_t e : ctx->ev_comm)
        if (e) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

static int create_impl(const mcalf_spec* sp, mcalf_ctx* ctx) {
    // check, pick the device, plan (ctx_plan.h: everything the spec decides), upload
    std::string why;
    int rc = check_spec(sp, &why);
    if (rc) return set_err(ctx, rc, "%s", why.c_str());
    if ((rc = pick_device(ctx, sp->device, &ctx->device, &ctx->arch))) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    CtxShape& shape = *ctx;
    CtxTables tab;
    if ((rc = plan_shape(*sp, ctx->env.lines_per_sync, &shape, &why))) return set_err(ctx, rc, "%s", why.c_str());
    plan_tables(*sp, &shape, &tab);

    const size_t nb = (size_t)ctx->npix * sizeof(double);
    const size_t nbp = nb + 8 * sizeof(double);          // the epilogue reads 8 pixels per thread without a bounds test
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_nu.p, tab.nu.size() * sizeof(double)));
    for (DevBuf<double>* b : {&ctx->d_obj, &ctx->d_ispec2, &ctx->d_lgis, &ctx->d_err}) {
        HIP_TRY(ctx, hipMalloc((void**)&b->p, nbp));
        HIP_TRY(ctx, hipMemset(b->p, 0, nbp));
    }
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_lines.p, tab.lines.size() * sizeof(LineDev)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_nu, tab.nu.data(), tab.nu.size() * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_obj, sp->flux, nb, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_ispec2, tab.ispec2.data(), nb, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_lgis, tab.lgis.data(), nb, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_err, sp->err, nb, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_lines, tab.lines.data(), tab.lines.size() * sizeof(LineDev), hipMemcpyHostToDevice));
    if ((rc = upload_tables(ctx, &ctx->d_tabs.p))) return rc;
    if ((rc = eqw_prepare(ctx, sp->wl))) return rc;
    if ((rc = kin_prepare(ctx, sp->wl))) return rc;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_segok.p, tab.segok.size() * sizeof(unsigned long long)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_segok, tab.segok.data(), tab.segok.size() * sizeof(unsigned long long), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_wtab.p, sizeof(VT_INTERP_W_HOST)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_wtab, VT_INTERP_W_HOST, sizeof(VT_INTERP_W_HOST), hipMemcpyHostToDevice));
    // more than 64 KiB of dynamic LDS needs the attribute (2 workgroups x 78 KiB fit the 160 KiB of a CU)
    for (int k = 0; k < fused_kernel_count(); ++k)
        HIP_TRY(ctx, hipFuncSetAttribute(fused_kernel_at(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsBudget));
    if ((rc = create_stream(ctx, &ctx->stream))) return rc;
    hipDeviceProp_t prop;
    HIP_TRY(ctx, hipGetDeviceProperties(&prop, ctx->device));
    ctx->num_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if ((rc = stream_probe_xcds(ctx))) return rc;         // (the streaming launch is for one device shape only)
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_queue.p, kMaxChunks * sizeof(unsigned int)));
    HIP_TRY(ctx, hipMemset(ctx->d_queue, 0, kMaxChunks * sizeof(unsigned int)));
    // (the environment's snapshot was applied at the top of mcalf_create; what depends on the device is finished here)
    ctx->inline_max_items = ctx->env.inline_max >= 0 ? ctx->env.inline_max : 2 * ctx->num_cu;   // launches that fit the chip in one round of workgroups
    if (ctx->env.stream_wgs >= 0) ctx->stream_wgs = std::min(ctx->env.stream_wgs, ctx->num_cu);
    return MCALF_OK;
}

extern "C" int mcalf_create(const mcalf_spec* spec, mcalf_ctx** out) {
    if (!out) return set_err(nullptr, MCALF_ERR_INVALID, "out is NULL");
    *out = nullptr;
    mcalf_ctx* ctx = new (std::nothrow) mcalf_ctx();
    if (!ctx) return set_err(nullptr, MCALF_ERR_NOMEM, "out of host memory");
    ctx->env = read_environment();                        // ONE snapshot per context; nothing else reads the environment
    apply_environment(ctx);
    int rc = create_impl(spec, ctx);
    if (rc != MCALF_OK) {
        g_last_error = ctx->err;
        mcalf_destroy(ctx);
        return rc;
    }
    *out = ctx;
    return MCALF_OK;
}

extern "C" int mcalf_info(const mcalf_ctx* ctx, mcalf_info_t* info) {
    if (!ctx || !info) return set_err(nullptr, MCALF_ERR_INVALID, "NULL argument");
    memset(info, 0, sizeof *info);
    info->abi_version = MCALF_ABI_VERSION;
    info->ndim = ctx->ndim;
    info->startind = ctx->startind;
    info->endind = ctx->endind;
    info->n_cap = ctx->wide ? ctx->wide_n_cap : ctx->n_cap;      // (what specres_max provisions, wherever the convolution runs)
    info->tile = ctx->tile;
    info->ntiles = ctx->ntiles;
    info->device = ctx->device;
    info->npix = ctx->npix;
    snprintf(info->arch, sizeof info->arch, "%s", ctx->arch.c_str());
    info->ndevices = is_multi(ctx) ? (int32_t)ctx->subs.size() : 1;
    for (int k = 0; k < info->ndevices && k < 16; ++k) info->devices[k] = is_multi(ctx) ? ctx->subs[k]->device : ctx->device;
    return MCALF_OK;
}

extern "C" int mcalf_last_launch(const mcalf_ctx* ctx, mcalf_launch_info_t* info) {
    if (!ctx || !info) return set_err(nullptr, MCALF_ERR_INVALID, "NULL argument");
    if (is_multi(ctx)) {                                  // sub-context 0's launch, and how many devices the call was cut over
        const int rc = mcalf_last_launch(ctx->subs[0], info);
        info->devices_used = ctx->multi_last_active;
        return rc;
    }
    *info = ctx->last;
    info->xcd_mask = (int32_t)ctx->xcd_mask;
    info->devices_used = 1;
    return MCALF_OK;
}

// A stream of the context: non-blocking, or -- with a CU mask (mcalf_set_cu_mask) -- restricted to the mask's CUs.
// priority: +1 the copy stream, -1 the second compute stream of the row-block pipeline, 0 everything else.  A process has
// few hardware queues (GPU_MAX_HW_QUEUES, 4 by default) and HIP deals its streams to them per PRIORITY level: in a process
// with many streams (an application with several contexts; bench.py's legs next to its main context) two of the pipeline's
// three streams can land on ONE queue -- its row blocks then run strictly one after the other (measured with
// MCALF_HOST_TRACE=2: config E's host step 2.90 -> 2.99 ms), or its copies wait behind kernels again.  Streams of different
// priority levels take their queues from different pools, so the three never share.
int create_stream(mcalf_ctx* ctx, hipStream_t* out, int priority) {
    if (!ctx->cu_mask.empty()) {
        HIP_TRY(ctx, hipExtStreamCreateWithCUMask(out, (uint32_t)ctx->cu_mask.size(), ctx->cu_mask.data()));
        return MCALF_OK;
    }
    int least = 0, greatest = 0;
    if (priority != 0 && hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest) {
        HIP_TRY(ctx, hipStreamCreateWithPriority(out, hipStreamNonBlocking, priority > 0 ? greatest : least));
        return MCALF_OK;
    }
    (void)hipGetLastError();
    HIP_TRY(ctx, hipStreamCreateWithFlags(out, hipStreamNonBlocking));
    return MCALF_OK;
}

// A setting of a multi-device parent goes to its first n sub-contexts; the first failure is reported with the sub-context's message.
template <typename F>
static int forward_to_subs(mcalf_ctx* ctx, int n, F call) {
    for (int k = 0; k < n; ++k) {
        const int rc = call(ctx->subs[k]);
        if (rc) return set_err(ctx, rc, "%s", ctx->subs[k]->err.c_str());
    }
    return MCALF_OK;
}

extern "C" int mcalf_set_cu_mask(mcalf_ctx* ctx, const uint32_t* mask, int32_t nwords) {
    if (!ctx) return set_err(nullptr, MCALF_ERR_INVALID, "ctx is NULL");
    if (nwords < 0 || nwords > 64 || (nwords > 0 && !mask)) return set_err(ctx, MCALF_ERR_INVALID, "CU mask: 0 .. 64 words");
    bool any = nwords == 0;
    for (int32_t i = 0; i < nwords; ++i) any = any || mask[i] != 0u;
    if (!any) return set_err(ctx, MCALF_ERR_INVALID, "CU mask selects no compute unit");
    if (is_multi(ctx)) return forward_to_subs(ctx, (int)ctx->subs.size(), [&](mcalf_ctx* sub) { return mcalf_set_cu_mask(sub, mask, nwords); });
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // EVERY stream the context owns is replaced: the launch stream and its auxiliaries, the resident evaluator's (its
    // kernel is told to leave first: the next one-theta call starts another one on the new stream) and the exchange
    // stream of the library's gather (pending exchanges are waited for; it is re-created by the next gather).
    resident_stop(ctx);
    if (ctx->res_stream) { HIP_TRY(ctx, hipStreamSynchronize(ctx->res_stream)); HIP_TRY(ctx, hipStreamDestroy(ctx->res_stream)); ctx->res_stream = nullptr; }
    if (ctx->comm_stream) { HIP_TRY(ctx, hipStreamSynchronize(ctx->comm_stream)); HIP_TRY(ctx, hipStreamDestroy(ctx->comm_stream)); ctx->comm_stream = nullptr; }
    // the context's own streams are idle between its (synchronous) host-pointer calls; wait anyway, then replace them
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    for (hipStream_t& st : ctx->aux)
        if (st) { HIP_TRY(ctx, hipStreamSynchronize(st)); HIP_TRY(ctx, hipStreamDestroy(st)); st = nullptr; }
    HIP_TRY(ctx, hipStreamDestroy(ctx->stream));
    ctx->stream = nullptr;
    ctx->cu_mask.assign(mask, mask + nwords);
    int rc = create_stream(ctx, &ctx->stream);
    if (rc != MCALF_OK) {                                 // (a mask the runtime refuses: back to an unrestricted stream)
        ctx->cu_mask.clear();
        const std::string why = ctx->err;
        if (create_stream(ctx, &ctx->stream) != MCALF_OK) return rc;
        (void)stream_probe_xcds(ctx);
        return set_err(ctx, rc, "%s (the context keeps an unrestricted stream)", why.c_str());
    }
    return stream_probe_xcds(ctx);
}

extern "C" int mcalf_reserve(mcalf_ctx* ctx, int64_t batch) {
    if (!ctx || batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "bad arguments");
    if (is_multi(ctx)) {                                  // every device's largest shard of such a batch
        const int n = multi_active(ctx, batch);
        return forward_to_subs(ctx, n, [&](mcalf_ctx* sub) { return mcalf_reserve(sub, (batch + n - 1) / n); });
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = grow(ctx, ctx->d_P, (size_t)batch * std::max(ctx->ndim, 5)))) return rc;
    if ((rc = grow(ctx, ctx->d_out, (size_t)batch))) return rc;
    if ((rc = grow(ctx, ctx->d_partial, (size_t)batch * ctx->ntiles * 4))) return rc;
    if ((rc = grow_sample_ws(ctx, batch))) return rc;
    if (ctx->wide && batch > 0) {                         // the scratch of a wide-LSF launch (one pass of launch_wide)
        const int64_t rows = wide_rows_per_pass(ctx, batch);
        if (rows < 1) return set_err(ctx, MCALF_ERR_RANGE, "wide LSF: one live point exceeds the scratch of a pass");
        if ((rc = grow_wide_ws(ctx, rows, true, true))) return rc;
    }
    return MCALF_OK;
}

extern "C" int32_t mcalf_get_chunks(const mcalf_ctx* ctx, int64_t batch) {
    if (ctx && is_multi(ctx)) return mcalf_get_chunks(ctx->subs[0], batch);
    return (ctx && batch > 0) ? pick_chunks(ctx, batch) : 0;
}

extern "C" int mcalf_set_chunks(mcalf_ctx* ctx, int32_t nchunks) {
    if (!ctx || nchunks < 0 || nchunks > kMaxChunks)
        return set_err(ctx, MCALF_ERR_INVALID, "nchunks must be 0 (automatic) .. %d", kMaxChunks);
    ctx->chunks_req = nchunks;
    for (mcalf_ctx* sub : ctx->subs) sub->chunks_req = nchunks;
    return MCALF_OK;
}

extern "C" int mcalf_profile_begin(mcalf_ctx* ctx, int32_t max_launches) {
    if (!ctx || max_launches <= 0) return set_err(ctx, MCALF_ERR_INVALID, "bad arguments");
    MCALF_SINGLE_ONLY(ctx, "mcalf_profile_begin");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    while (ctx->ev.size() < 2 * (size_t)max_launches) {
        hipEvent_t e;
        HIP_TRY(ctx, hipEventCreate(&e));
        ctx->ev.push_back(e);
    }
    ctx->ev_used = 0;
    ctx->profiling = true;
    return MCALF_OK;
}

extern "C" int mcalf_profile_end(mcalf_ctx* ctx, double* mean_ms, int32_t* launches) {
    if (!ctx || !mean_ms) return set_err(ctx, MCALF_ERR_INVALID, "bad arguments");
    MCALF_SINGLE_ONLY(ctx, "mcalf_profile_end");
    ctx->profiling = false;
    double sum = 0.0;
    const size_t n = ctx->ev_used / 2;
    for (size_t i = 0; i < n; ++i) {
        HIP_TRY(ctx, hipEventSynchronize(ctx->ev[2 * i + 1]));
        float ms = 0.f;
        HIP_TRY(ctx, hipEventElapsedTime(&ms, ctx->ev[2 * i], ctx->ev[2 * i + 1]));
        sum += ms;
    }
    *mean_ms = n ? sum / (double)n : 0.0;
    if (launches) *launches = (int32_t)n;
    ctx->ev_used = 0;
    return MCALF_OK;
}

extern "C" int mcalf_loglike_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, double* dlogL,
                                          void* stream) {
    if (!ctx || (batch > 0 && (!dP || !dlogL))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    MCALF_SINGLE_ONLY(ctx, "mcalf_loglike_batch_device");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    LaunchReq q(kModeLogL, dP, batch, (hipStream_t)stream); q.d_out = dlogL;
    return launch(ctx, q);
}

extern "C" int mcalf_model_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, int32_t targonly,
                                        double* dflux, void* stream) {
    if (!ctx || (batch > 0 && (!dP || !dflux))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    MCALF_SINGLE_ONLY(ctx, "mcalf_model_batch_device");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    LaunchReq q(kModeModel, dP, batch, (hipStream_t)stream);
    q.targonly = targonly ? 1 : 0; q.d_model = dflux;
    return launch(ctx, q);
}

// True when `p` is page-locked host memory the copy engines can read / write directly.
bool is_pinned_host(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();                          // ordinary pageable memory: not an error for us
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// The page-locked, device-mapped block small calls go through: parameters in its first half, results in its second.
int ensure_small(mcalf_ctx* ctx) {
    if (!ctx->h_small) {
        // (coherent: the host fills the result slots before a launch and reads them while it runs)
        HIP_TRY(ctx, hipHostMalloc((void**)&ctx->h_small.p, 2 * kSmallDoubles * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent));
        HIP_TRY(ctx, hipHostGetDevicePointer((void**)&ctx->d_small, ctx->h_small, 0));
    }
    return MCALF_OK;
}

// Small scalar-output calls (up to kSmallDoubles parameters: single-theta calls, config B's batch), zero-copy: a
// single-theta call is dominated by the latency of its two copy commands.  from_cube / theta_out: as in run_host_stream.
static int run_host_small(mcalf_ctx* ctx, const HostReq& h) {
    const double* P = h.P; const int64_t batch = h.batch;
    int rc;
    if (resident_serves(ctx, h.mode, batch, h.rowlen, h.from_cube)) return resident_call(ctx, P, h.rowlen, h.out_scalar);
    if ((rc = ensure_small(ctx))) return rc;
    const bool trace = ctx->host_trace != 0;
    const double ts0 = trace ? now_us() : 0.0;
    // (Copy first, launch afterwards.  Round 6 tried the other order for calls of >= 32 KB -- the set-up kernel's workgroups
    // waiting for the host's row count, so that the launch latency would run under the copy: the copy of config B's 200 KB
    // takes 1.5 us, the waits' PCIe looks cost 8 us; docs/optimisation_log.md 8f.)
    std::memcpy(ctx->h_small, P, (size_t)batch * h.rowlen * sizeof(double));
    set_path(ctx, MCALF_PATH_HOST_ZEROCOPY, false, false); ctx->last.stream_fallback = 0;   // (of a streaming attempt that did not take the call)
    // Completion is read off the results: their slots are filled with a NaN no kernel produces, and the call is over
    // when none is left -- a stream wait costs an interrupt and a thread wake-up on top of the kernel, a fifth of a
    // one-theta call.  (The stream is asked now and then, so that a failed launch cannot keep the call here.)
    uint64_t* res = reinterpret_cast<uint64_t*>(ctx->h_small + kSmallDoubles);
    const bool poll = ctx->stream_poll != 0;
    if (poll)
        for (int64_t i = 0; i < batch; ++i) __atomic_store_n(res + i, kResultPending, __ATOMIC_RELEASE);
    const double ts1 = trace ? now_us() : 0.0;
    LaunchReq q = h.on_device(ctx->d_small, ctx->stream);
    q.d_out = ctx->d_small + kSmallDoubles;
    if ((rc = launch(ctx, q))) return rc;
    const double ts2 = trace ? now_us() : 0.0;
    if (h.theta_out) host_scale_cube(ctx, P, batch, h.theta_out);       // (under the launch)
    const double ts3 = trace ? now_us() : 0.0;
    bool done = false;
    if (poll) {
        int64_t left = batch;                            // results [left, batch) have been seen
        for (unsigned long spins = 1;; ++spins) {
            while (left > 0 && __atomic_load_n(res + left - 1, __ATOMIC_ACQUIRE) != kResultPending) --left;
            if (left == 0) { done = true; break; }
            if ((spins & 0x3FFFul) == 0 && hipStreamQuery(ctx->stream) != hipErrorNotReady) break;
            __builtin_ia32_pause();
        }
    }
    if (!done) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->last.stream_polled = done ? 1 : 0;
    const double ts4 = trace ? now_us() : 0.0;
    std::memcpy(h.out_scalar, ctx->h_small + kSmallDoubles, (size_t)batch * sizeof(double));
    if (trace) {
        HostTrace& t = ctx->htrace;
        t.small_calls++; t.small_prep_us += ts1 - ts0; t.small_launch_us += ts2 - ts1; t.small_copy_us += ts3 - ts2;
        t.small_poll_us += ts4 - ts3; t.small_out_us += now_us() - ts4;
    }
    return MCALF_OK;
}

// Host-pointer entries: the ONE place that chooses the plan of a call -- zero-copy, streaming, pipelined or staged.
static int run_host(mcalf_ctx* ctx, const HostReq& h);
static int host_shard(void* sub, int64_t lo, int64_t hi, void* arg) {      // rows [lo, hi) of a multi-device call, on sub-context `sub`
    HostReq h = *static_cast<const HostReq*>(arg);
    h.P += (size_t)lo * h.rowlen;
    h.batch = hi - lo;
    if (h.out_scalar) h.out_scalar += lo;
    if (h.out_model) h.out_model += (size_t)lo * static_cast<mcalf_ctx*>(sub)->npix;
    if (h.theta_out) h.theta_out += (size_t)lo * h.rowlen;
    return run_host(static_cast<mcalf_ctx*>(sub), h);
}
static int run_host(mcalf_ctx* ctx, const HostReq& h) {
    const int64_t batch = h.batch;
    if (!ctx) return set_err(nullptr, MCALF_ERR_INVALID, "ctx is NULL");
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "negative batch");
    if (batch == 0) return MCALF_OK;
    if (!h.P || (!h.out_scalar && !h.out_model)) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    if (is_multi(ctx)) return multi_run(ctx, batch, host_shard, const_cast<HostReq*>(&h));   // contiguous row blocks, one per device, straight into the caller's arrays
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_HOST_STAGED, false, false);    // (the plan that takes the call names itself: set_path)
    const size_t total = (size_t)batch * h.rowlen;
    const bool scalar = h.out_scalar && !h.out_model;
    int rc; bool taken = false;
    if (scalar && total <= kSmallDoubles && (size_t)batch <= kSmallDoubles) {
        // (a batch that is small in bytes but reaches the streaming launch's item count -- MCALF_STREAM_MIN items per
        // workgroup slot -- streams: one launch that sets its live points up itself, instead of set-up + fused kernel)
        if (h.reduces() && stream_qualifies(ctx, batch) && ((rc = run_host_stream(ctx, h, &taken)) != MCALF_OK || taken)) return rc;
        return run_host_small(ctx, h);
    }
    // (grown before the streaming attempt, as the theta entries always did: every plan below finds its buffers)
    if ((rc = grow(ctx, ctx->d_P, total))) return rc;
    if (h.out_scalar && (rc = grow(ctx, ctx->d_out, (size_t)batch))) return rc;
    if (h.out_model && (rc = grow(ctx, ctx->d_model, (size_t)batch * ctx->npix))) return rc;
    // a large scalar call: ONE streaming launch where it qualifies (never a wide-LSF context: stream_qualifies), else the
    // row-block pipeline; tiled or wide cube calls and model output: staged copies
    if (scalar && h.reduces() && ((rc = run_host_stream(ctx, h, &taken)) != MCALF_OK || taken)) return rc;
    if (scalar && !ctx->wide && !h.from_cube) return run_host_pipelined(ctx, h);
    set_path(ctx, MCALF_PATH_HOST_STAGED, false, false);
    // (the transformed rows of a cube call come back from the device, through d_model)
    if (h.theta_out && (rc = grow(ctx, ctx->d_model, total))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_P, h.P, total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    LaunchReq q = h.on_device(ctx->d_P, ctx->stream);
    q.d_out = h.out_scalar ? ctx->d_out.p : nullptr;
    q.d_model = h.out_model ? ctx->d_model.p : nullptr;
    q.d_theta = h.theta_out ? ctx->d_model.p : nullptr;
    if ((rc = launch(ctx, q))) return rc;
    if (h.out_scalar) HIP_TRY(ctx, hipMemcpyAsync(h.out_scalar, ctx->d_out, (size_t)batch * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (h.out_model) HIP_TRY(ctx, hipMemcpyAsync(h.out_model, ctx->d_model, (size_t)batch * ctx->npix * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (h.theta_out) HIP_TRY(ctx, hipMemcpyAsync(h.theta_out, ctx->d_model, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MCALF_OK;
}

extern "C" int mcalf_loglike_batch(mcalf_ctx* ctx, const double* P, int64_t batch, double* logL) {
    return run_host(ctx, HostReq{kModeLogL, P, batch, ctx ? ctx->ndim : 0, 0, 0, logL});
}

extern "C" int mcalf_chi2_batch(mcalf_ctx* ctx, const double* P, int64_t batch, double* chi2) {
    return run_host(ctx, HostReq{kModeChi2, P, batch, ctx ? ctx->ndim : 0, 0, 0, chi2});
}

extern "C" int mcalf_model_batch(mcalf_ctx* ctx, const double* P, int64_t batch, int32_t targonly, double* flux) {
    return run_host(ctx, HostReq{kModeModel, P, batch, ctx ? ctx->ndim : 0, targonly ? 1 : 0, 0, nullptr, flux});
}

extern "C" int mcalf_onecomp_batch(mcalf_ctx* ctx, const double* Q, int64_t batch, int32_t which, double* flux) {
    if (ctx && (which < 0 || which >= 2 + ctx->nlines))
        return set_err(ctx, MCALF_ERR_INVALID, "onecomp: `which` must be 0 (all lines), 1 (filler) or 2+k with k < %d",
                       ctx->nlines);
    return run_host(ctx, HostReq{kModeOneComp, Q, batch, 5, 0, which, nullptr, flux});
}

extern "C" int mcalf_set_prior(mcalf_ctx* ctx, const double* lo, const double* hi, int32_t int_ncomp) {
    if (!ctx) return set_err(nullptr, MCALF_ERR_INVALID, "ctx is NULL");
    if (!lo || !hi) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    if (is_multi(ctx)) {
        const int rc = forward_to_subs(ctx, (int)ctx->subs.size(), [&](mcalf_ctx* sub) { return mcalf_set_prior(sub, lo, hi, int_ncomp); });
        if (rc == MCALF_OK) ctx->prior_set = true;
        return rc;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_prior) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_prior.p, 2 * (size_t)ctx->ndim * sizeof(double)));
    // synchronous copies: the caller's arrays are borrowed for this call only, and a later *_device call may
    // run on any stream
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(ctx->d_prior, lo, ctx->ndim * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->d_prior + ctx->ndim, hi, ctx->ndim * sizeof(double), hipMemcpyHostToDevice));
    ctx->h_prior.assign(lo, lo + ctx->ndim);
    ctx->h_prior.insert(ctx->h_prior.end(), hi, hi + ctx->ndim);
    ctx->prior_set = true;
    ctx->prior_int = int_ncomp ? 1 : 0;
    return MCALF_OK;
}

extern "C" int mcalf_loglike_cube_batch_device(mcalf_ctx* ctx, const double* dcube, int64_t batch, double* dtheta,
                                               double* dlogL, void* stream) {
    if (!ctx || (batch > 0 && (!dcube || !dlogL))) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    MCALF_SINGLE_ONLY(ctx, "mcalf_loglike_cube_batch_device");
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "mcalf_set_prior has not been called");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    LaunchReq q(kModeLogL, dcube, batch, (hipStream_t)stream);
    q.d_out = dlogL; q.from_cube = true; q.d_theta = dtheta;
    return launch(ctx, q);
}

extern "C" int mcalf_loglike_cube_batch(mcalf_ctx* ctx, const double* cube, int64_t batch, double* theta,
                                        double* logL) {
    if (!ctx) return set_err(nullptr, MCALF_ERR_INVALID, "ctx is NULL");
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "negative batch");
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "mcalf_set_prior has not been called");
    if (batch == 0) return MCALF_OK;
    if (!cube || !logL) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    // the plans of mcalf_loglike_batch, with the prior transform applied while the rows are decoded; the transformed rows are
    // formed on the host under the launch (zero-copy, streaming) or come back from the device (staged)
    return run_host(ctx, HostReq{kModeLogL, cube, batch, ctx->ndim, 0, 0, logL, nullptr, true, theta});
}

extern "C" int mcalf_scale_cube_batch(mcalf_ctx* ctx, const double* lo, const double* hi, const double* cube,
                                      int64_t batch, int32_t int_ncomp, double* theta) {
    if (!ctx) return set_err(nullptr, MCALF_ERR_INVALID, "ctx is NULL");
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "negative batch");
    if (batch == 0) return MCALF_OK;
    if (!lo || !hi || !cube || !theta) return set_err(ctx, MCALF_ERR_INVALID, "NULL argument");
    if (is_multi(ctx)) return mcalf_scale_cube_batch(ctx->subs[0], lo, hi, cube, batch, int_ncomp, theta);   // (a few bytes per row: one device)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t total = (size_t)batch * ctx->ndim;
    int rc;
    if ((rc = grow(ctx, ctx->d_P, total))) return rc;
    if ((rc = grow(ctx, ctx->d_model, total))) return rc;
    if (!ctx->d_bounds) HIP_TRY(ctx, hipMalloc((void**)&ctx->d_bounds.p, 2 * (size_t)ctx->ndim * sizeof(double)));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bounds, lo, ctx->ndim * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_bounds + ctx->ndim, hi, ctx->ndim * sizeof(double), hipMemcpyHostToDevice,
                                ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_P, cube, total * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    {
        const double *lo_d = ctx->d_bounds, *hi_d = ctx->d_bounds + ctx->ndim, *cube_d = ctx->d_P;
        long n = (long)total;
        int nd = ctx->ndim, slot = ctx->startind, as_int = int_ncomp;
        double* theta_d = ctx->d_model;
        void* kargs[] = {(void*)&lo_d, (void*)&hi_d, (void*)&cube_d, (void*)&n, (void*)&nd, (void*)&slot, (void*)&as_int, (void*)&theta_d};
        HIP_TRY(ctx, hipLaunchKernel(scale_cube_kernel_ptr(), dim3((unsigned)((total + 255) / 256)), dim3(256), kargs, 0, ctx->stream));
    }
    HIP_TRY(ctx, hipMemcpyAsync(theta, ctx->d_model, total * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MCALF_OK;
}

static int hjerting_impl(const double* x, const double* y, int64_t n, double* out, int32_t device, int node_form) {
    if (n < 0 || (n > 0 && (!x || !y || !out))) return set_err(nullptr, MCALF_ERR_INVALID, "bad arguments");
    if (n == 0) return MCALF_OK;
    int dev = 0;
    int rc = pick_device(nullptr, device, &dev, nullptr);
    if (rc) return rc;
    HIP_TRY(nullptr, hipSetDevice(dev));
    double *dx = nullptr, *dy = nullptr, *dout = nullptr, *dtabs = nullptr;
    const size_t nb = (size_t)n * sizeof(double);
    hipError_t em = hipMalloc((void**)&dx, nb);
    if (em == hipSuccess) em = hipMalloc((void**)&dy, nb);
    if (em == hipSuccess) em = hipMalloc((void**)&dout, nb);
    if (em != hipSuccess) rc = set_err(nullptr, MCALF_ERR_HIP, "hjerting: hipMalloc failed: %s", hipGetErrorString(em));
    else rc = upload_tables(nullptr, &dtabs);
    if (rc == MCALF_OK) {
        hipError_t e = hipMemcpy(dx, x, nb, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dy, y, nb, hipMemcpyHostToDevice);
        if (e == hipSuccess) {
            long cnt = (long)n;
            void* kargs[] = {(void*)&dx, (void*)&dy, (void*)&cnt, (void*)&dout, (void*)&dtabs, (void*)&node_form};
            e = hipLaunchKernel(hjert_kernel_ptr(), dim3((unsigned)((n + 255) / 256)), dim3(256), kargs, 0, nullptr);
        }
        if (e == hipSuccess) e = hipMemcpy(out, dout, nb, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = set_err(nullptr, MCALF_ERR_HIP, "hjerting: %s", hipGetErrorString(e));
    }
    for (double* b : {dx, dy, dout, dtabs})
        if (b) (void)hipFree(b);
    return rc;
}

extern "C" int mcalf_voigt_hjerting(const double* x, const double* y, int64_t n, double* out, int32_t device) {
    return hjerting_impl(x, y, n, out, device, 0);
}

extern "C" int mcalf_voigt_hjerting_nodes(const double* x, const double* y, int64_t n, double* out, int32_t device) {
    return hjerting_impl(x, y, n, out, device, 1);
}
