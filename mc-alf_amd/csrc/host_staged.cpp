// libmcalf_hip.so, host side: the staged call every host-pointer analysis entry makes (gradient, JVP, VJP, HVP, Fisher product,
// fit, equivalent widths, posterior bands, slice step, ensemble sampler).  An entry describes its arrays as columns and hands
// over its device driver; run_staged does the rest: the multi-device split, the arena, the copies in and out, the wait.
// (The likelihood's own host-pointer entries -- zero-copy, pipelined, streaming: host_abi.cpp's HostReq plans -- are not these.)
#include "host_ctx.h"

namespace {

constexpr size_t kStageAlign = 256;       // every column starts on this boundary of the arena

size_t col_bytes(const StageCol& c, int64_t batch) { return c.elem * c.count * (c.rows ? (size_t)batch : 1); }

// Rows [lo, hi) of the plan on one device of a multi-device context: the columns cut with the rows start at row lo.
int staged_shard(void* sub, int64_t lo, int64_t hi, void* arg) {
    StagePlan part = *static_cast<const StagePlan*>(arg);
    for (int i = 0; i < part.ncols; ++i) {
        StageCol& c = part.cols[i];
        if (c.rows && c.present) c.host = static_cast<char*>(c.host) + (size_t)lo * c.count * c.elem;
    }
    part.batch = hi - lo;
    return run_staged(static_cast<mcalf_ctx*>(sub), part);
}

}  // namespace

int run_staged(mcalf_ctx* ctx, const StagePlan& plan) {
    if (is_multi(ctx)) {
        if (plan.shard == kStageCutRows)                  // contiguous row blocks, one per device, straight into the caller's arrays
            return multi_run(ctx, plan.batch, staged_shard, const_cast<StagePlan*>(&plan));
        mcalf_ctx* sub = ctx->subs[0];                    // the rows have to meet on one device: bit for bit a single-device call
        ctx->multi_last_active = 1;
        const int rc = run_staged(sub, plan);
        return rc ? set_err(ctx, rc, "device entry 0 (HIP device %d): %s", sub->device, sub->err.c_str()) : MCALF_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const auto pinned = [&](int col) { return col >= 0 && is_pinned_host(plan.cols[col].host); };
    begin_call(ctx, MCALF_PATH_HOST_STAGED, pinned(plan.pin_in), pinned(plan.pin_out));   // H2D, launch, D2H on the context's stream
    size_t off[kStageMaxCols], total = 0;
    for (int i = 0; i < plan.ncols; ++i) {
        const StageCol& c = plan.cols[i];
        off[i] = total;
        if (c.present && !c.own) total += (col_bytes(c, plan.batch) + kStageAlign - 1) / kStageAlign * kStageAlign;
    }
    int rc;
    if ((rc = grow(ctx, ctx->stage_dev, total))) return rc;
    void* dev[kStageMaxCols];
    for (int i = 0; i < plan.ncols; ++i) dev[i] = plan.cols[i].present && !plan.cols[i].own ? ctx->stage_dev.p + off[i] : nullptr;
    const hipStream_t st = ctx->stream;
    for (int i = 0; i < plan.ncols; ++i) {
        const StageCol& c = plan.cols[i];
        if (c.present && !c.out) HIP_TRY(ctx, hipMemcpyAsync(dev[i], c.host, col_bytes(c, plan.batch), hipMemcpyHostToDevice, st));
    }
    if ((rc = plan.body(ctx, dev, plan.batch, st, plan.arg))) return rc;
    for (int i = 0; i < plan.ncols; ++i) {
        const StageCol& c = plan.cols[i];
        if (c.present && c.out) HIP_TRY(ctx, hipMemcpyAsync(c.host, dev[i], col_bytes(c, plan.batch), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return MCALF_OK;
}
