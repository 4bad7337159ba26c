// Host side of the Gaussian prior: mcalf_set_gauss_prior / mcalf_get_gauss_prior (the factors next to the box of mcalf_set_prior,
// on every sub-context of a multi-device context) and mcalf_lnprior_batch[_device] over the prior kernel (prior_kernels.hip).  The
// samplers' drivers (host_ns.cpp, host_ens.cpp) hand the same block (prior_dev of host_ctx.h) to their own kernels.
#include "host_ctx.h"

namespace {

// What a failed launch of the prior kernel is reported as.
constexpr char kPriorLaunch[] = "hipLaunchKernel(prior_kernel_ptr(), dim3(rows), dim3(kPriorWave), args, 0, stream)";

// Everything that is wrong with a call before any device work; `name` is the entry that reports it.
int lnprior_check(mcalf_ctx* ctx, const char* name, const double* rows, int64_t batch, int32_t from_cube, const double* out) {
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: batch must be >= 0, got %lld", name, (long long)batch);
    if (batch > 0 && !rows) return set_err(ctx, MCALF_ERR_INVALID, "%s: rows is NULL", name);
    if (batch > 0 && !out) return set_err(ctx, MCALF_ERR_INVALID, "%s: lnprior is NULL", name);
    if (from_cube != 0 && from_cube != 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: from_cube must be 0 or 1, got %d", name, from_cube);
    if (batch > 0x7fff0000LL) return set_err(ctx, MCALF_ERR_RANGE, "%s: batch %lld too large", name, (long long)batch);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "%s: mcalf_set_prior has not been called (the box is part of the prior)", name);
    return MCALF_OK;
}

int run_lnprior(mcalf_ctx* ctx, const double* drows, int64_t batch, int from_cube, double* dout, hipStream_t stream) {
    if (batch <= 0) return MCALF_OK;
    const PriorArgs a = {prior_dev(ctx), drows, dout, from_cube};
    return launch_block(ctx, prior_kernel_ptr(), a, dim3((unsigned)batch), dim3(kPriorWave), stream, kPriorLaunch);
}

int lnprior_body(mcalf_ctx* ctx, void** dev, int64_t rows, hipStream_t stream, void* arg) {
    return run_lnprior(ctx, (const double*)dev[0], rows, *static_cast<const int*>(arg), (double*)dev[1], stream);
}

}  // namespace

extern "C" int mcalf_set_gauss_prior(mcalf_ctx* ctx, const double* mu, const double* sigma) {
    if (!ctx) return set_err(nullptr, MCALF_ERR_INVALID, "mcalf_set_gauss_prior: ctx is NULL");
    if ((mu == nullptr) != (sigma == nullptr))
        return set_err(ctx, MCALF_ERR_INVALID, "mcalf_set_gauss_prior: %s is NULL (both NULL clears the prior)", mu ? "sigma" : "mu");
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "mcalf_set_gauss_prior: mcalf_set_prior has not been called (the Gaussian factors go with its box)");
    const int ndim = ctx->ndim;
    if (mu) {
        char msg[256];
        if (gauss_prior_check(mu, sigma, ndim, ctx->startind, msg, sizeof msg)) return set_err(ctx, MCALF_ERR_INVALID, "mcalf_set_gauss_prior: %s", msg);
    }
    if (is_multi(ctx)) {
        for (mcalf_ctx* sub : ctx->subs) {
            const int rc = mcalf_set_gauss_prior(sub, mu, sigma);
            if (rc) return set_err(ctx, rc, "%s", sub->err.c_str());
        }
        ctx->ngauss = ctx->subs[0]->ngauss;
        return MCALF_OK;
    }
    if (!mu) {                                             // cleared: the kernels see no Gaussian (the arrays stay allocated)
        ctx->ngauss = 0;
        ctx->h_gauss.clear();
        return MCALF_OK;
    }
    std::vector<double> h(3 * (size_t)ndim);
    std::copy(mu, mu + ndim, h.begin());
    std::copy(sigma, sigma + ndim, h.begin() + ndim);
    const int ngauss = gauss_prior_constants(sigma, ndim, h.data() + 2 * (size_t)ndim);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = grow(ctx, ctx->d_gauss, h.size()))) return rc;
    // synchronous copy, as mcalf_set_prior's: a later *_device call may run on any stream
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipMemcpy(ctx->d_gauss, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    ctx->h_gauss.swap(h);
    ctx->ngauss = ngauss;                                  // (every sigma 0: no Gaussian, as if cleared)
    return MCALF_OK;
}

extern "C" int mcalf_get_gauss_prior(const mcalf_ctx* ctx, double* mu, double* sigma, double* c, int32_t* ngauss) {
    if (!ctx) return set_err(nullptr, MCALF_ERR_INVALID, "mcalf_get_gauss_prior: ctx is NULL");
    if (!ngauss) return set_err(nullptr, MCALF_ERR_INVALID, "mcalf_get_gauss_prior: ngauss is NULL");
    const mcalf_ctx* src = is_multi(ctx) ? ctx->subs[0] : ctx;
    const size_t n = (size_t)src->ndim;
    const bool set = src->ngauss > 0;
    *ngauss = set ? src->ngauss : 0;
    double* const outs[3] = {mu, sigma, c};
    for (int j = 0; j < 3; ++j)
        if (outs[j])
            for (size_t k = 0; k < n; ++k) outs[j][k] = set ? src->h_gauss[j * n + k] : 0.0;
    return MCALF_OK;
}

extern "C" int mcalf_lnprior_batch(mcalf_ctx* ctx, const double* rows, int64_t batch, int32_t from_cube, double* lnprior) {
    const int rc = lnprior_check(ctx, "mcalf_lnprior_batch", rows, batch, from_cube, lnprior);
    if (rc) return rc;
    if (batch == 0) return MCALF_OK;
    int cube = from_cube;
    const StagePlan plan = {{stage_in(rows, sizeof(double), (size_t)ctx->ndim), stage_out(lnprior, sizeof(double), 1)},
                            2, batch, kStageCutRows, 0, 1, lnprior_body, &cube};
    return run_staged(ctx, plan);
}

extern "C" int mcalf_lnprior_batch_device(mcalf_ctx* ctx, const double* drows, int64_t batch, int32_t from_cube, double* dlnprior, void* stream) {
    const int rc = lnprior_check(ctx, "mcalf_lnprior_batch_device", drows, batch, from_cube, dlnprior);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_lnprior_batch_device");
    if (batch == 0) return MCALF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_lnprior(ctx, drows, batch, from_cube, dlnprior, (hipStream_t)stream);
}
