// Host side of the ensemble-sampler kernels (ens_kernels.hip): mcalf_ensemble_batch, mcalf_tempered_batch and their _device
// forms -- T temperatures of n walkers in the unit cube moved by the stretch or the DE move, half against half, and exchanged
// between neighbouring temperatures in swap rounds.  mcalf_ensemble_batch is the same driver with ONE temperature at beta = 1
// and no swap round.  A driver over the cube logL launch (host_launch.cpp: launch() with from_cube) -- no Voigt code of its own.
// A half-step is the propose kernel, one logL launch over the T m trial rows (the set-up kernel and the fused kernel, as
// mcalf_loglike_cube_batch_device issues them) and the decide kernel, which also fills the chain slot of an iteration that is
// kept and has no swap; after a swap kernel the slot is filled by device-to-device copies (its kept part is contiguous).
// Nothing is read back during a call: the loop is issued in one go.
#include <cmath>

#include "ens_args.h"
#include "host_ctx.h"

static_assert(sizeof(mcalf_ens_opts) == 40, "mcalf_ens_opts is 40 bytes");
static_assert(sizeof(mcalf_pt_opts) == 48, "mcalf_pt_opts is 48 bytes");
static_assert((int)MCALF_ENS_STRETCH == (int)kEnsStretch && (int)MCALF_ENS_DE == (int)kEnsDE, "the kernels' move numbers are the header's");
static_assert((int)MCALF_PT_MAX_TEMPS == (int)kEnsMaxTemps, "the argument block holds the header's largest ladder");

namespace {

constexpr int64_t kEnsMaxChainBytes = 4LL << 30;      // largest chain (CU and CL together) a call may keep on the device

// The arrays of a call; every row array holds the T temperatures one after the other.
struct EnsRows {
    const double* U0;
    double *U, *theta, *logL; int32_t *status, *naccept, *nswap;
    double *CU, *CL;
};

// Bytes one chain slot takes on the device: the arrays the caller wants (CU of the first chain_temps temperatures, CL of all).
int64_t slot_bytes(const mcalf_ctx* ctx, const EnsRows& r, int64_t n, const mcalf_pt_opts& o) {
    return n * ((r.CU ? (int64_t)ctx->ndim * o.chain_temps : 0) + (r.CL ? o.ntemps : 0)) * (int64_t)sizeof(double);
}

// Everything that is wrong with a call before any device work; `name` is the entry that reports it.  `o`: the options in
// their tempered form (with_ladder false: mcalf_ensemble_batch's, one temperature, whose ladder is the entry's own).
int ens_check(mcalf_ctx* ctx, const char* name, const EnsRows& r, int64_t n, const mcalf_pt_opts* o, const double* beta, bool with_ladder) {
    if (!o) return set_err(ctx, MCALF_ERR_INVALID, "%s: opts is NULL", name);
    if (o->ntemps < 1 || o->ntemps > kEnsMaxTemps)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: ntemps must be in [1, %d], got %d", name, kEnsMaxTemps, o->ntemps);
    if (n < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be >= 0, got %lld", name, (long long)n);
    if (n % 2 != 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be even (two halves move in turn), got %lld", name, (long long)n);
    if (n > 0 && n < 4) return set_err(ctx, MCALF_ERR_INVALID, "%s: nwalkers must be >= 4 (the DE move takes two partners from a half), got %lld", name, (long long)n);
    if (n > 0 && !r.U0) return set_err(ctx, MCALF_ERR_INVALID, "%s: U0 is NULL", name);
    if (n > 0 && !r.U) return set_err(ctx, MCALF_ERR_INVALID, "%s: U is NULL", name);
    if (n > 0 && !r.logL) return set_err(ctx, MCALF_ERR_INVALID, "%s: logL is NULL", name);
    if (n > 0 && !r.status) return set_err(ctx, MCALF_ERR_INVALID, "%s: status is NULL", name);
    if (n > 0 && !r.naccept) return set_err(ctx, MCALF_ERR_INVALID, "%s: naccept is NULL", name);
    if (n > 0 && o->ntemps > 1 && !r.nswap) return set_err(ctx, MCALF_ERR_INVALID, "%s: nswap is NULL", name);
    if (with_ladder) {
        if (!beta) return set_err(ctx, MCALF_ERR_INVALID, "%s: beta is NULL", name);
        for (int t = 0; t < o->ntemps; ++t) {
            if (!std::isfinite(beta[t])) return set_err(ctx, MCALF_ERR_INVALID, "%s: beta[%d] must be finite, got %g", name, t, beta[t]);
            if (beta[t] < 0.0) return set_err(ctx, MCALF_ERR_INVALID, "%s: beta[%d] must be >= 0, got %g", name, t, beta[t]);
            if (t > 0 && !(beta[t] < beta[t - 1]))
                return set_err(ctx, MCALF_ERR_INVALID, "%s: beta must be strictly decreasing, got beta[%d] = %g after %g", name, t, beta[t], beta[t - 1]);
        }
        if (o->swap_every < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: swap_every must be >= 0 (0: never), got %d", name, o->swap_every);
        if (o->chain_temps < 0 || o->chain_temps > o->ntemps)
            return set_err(ctx, MCALF_ERR_INVALID, "%s: chain_temps must be in [0, ntemps = %d], got %d", name, o->ntemps, o->chain_temps);
    }
    if (o->nsteps < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: nsteps must be >= 0, got %d", name, o->nsteps);
    if (o->thin < 1) return set_err(ctx, MCALF_ERR_INVALID, "%s: thin must be >= 1, got %d", name, o->thin);
    if (o->move != MCALF_ENS_STRETCH && o->move != MCALF_ENS_DE)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: move must be MCALF_ENS_STRETCH (0) or MCALF_ENS_DE (1), got %d", name, o->move);
    if (!std::isfinite(o->scale)) return set_err(ctx, MCALF_ERR_INVALID, "%s: scale must be finite, got %g", name, o->scale);
    if (o->move == MCALF_ENS_STRETCH && !(o->scale > 1.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: scale must be > 1 for the stretch move, got %g", name, o->scale);
    if (o->move == MCALF_ENS_DE && !(o->scale > 0.0)) return set_err(ctx, MCALF_ERR_INVALID, "%s: scale must be > 0 for the DE move, got %g", name, o->scale);
    if (n > 0x7fff0000LL / o->ntemps) {                    // (before the context: the rows of a call are its arguments' alone)
        if (with_ladder) return set_err(ctx, MCALF_ERR_RANGE, "%s: ntemps x nwalkers = %d x %lld rows too large", name, o->ntemps, (long long)n);
        return set_err(ctx, MCALF_ERR_RANGE, "%s: nwalkers %lld too large", name, (long long)n);
    }
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (!ctx->prior_set) return set_err(ctx, MCALF_ERR_INVALID, "%s: mcalf_set_prior has not been called (the walkers move in its unit cube)", name);
    const int64_t per = slot_bytes(ctx, r, n, *o), nkeep = o->nsteps / o->thin;
    if (per > 0 && nkeep > kEnsMaxChainBytes / per)
        return set_err(ctx, MCALF_ERR_RANGE, "%s: a chain of nkeep %lld slots of %lld walkers x %d coordinates exceeds the %lld bytes one call may keep "
                       "on the device; the largest nkeep for this ensemble is %lld (raise thin)", name, (long long)nkeep, (long long)(n * o->ntemps), ctx->ndim,
                       (long long)kEnsMaxChainBytes, (long long)(kEnsMaxChainBytes / per));
    return MCALF_OK;
}

// mcalf_ensemble_batch's options as a ladder of one temperature that never swaps.
mcalf_pt_opts one_temperature(const mcalf_ens_opts& o) { return {o.nsteps, o.thin, o.move, 1, 0, 1, o.scale, o.seed, o.first_iter}; }
constexpr double kBetaOne[1] = {1.0};

// What a failed launch of a kernel of ens_kernels.hip is reported as.
constexpr char kEnsLaunch[] = "hipLaunchKernel(ens_kernel_ptr(k), dim3(grid), dim3(kEnsWave), args, 0, stream)";

// The call over T x `n` device rows on `stream`: issued in one go, nothing is read back.
int run_ens(mcalf_ctx* ctx, const EnsRows& r, int64_t n, const mcalf_pt_opts& o, const double* beta, hipStream_t stream) {
    if (n <= 0) return MCALF_OK;
    const size_t T = (size_t)o.ntemps, nb = (size_t)n, m = nb / 2, ndim = (size_t)ctx->ndim, rows = T * nb, moving = T * m;
    int rc;
    if ((rc = grow(ctx, ctx->enb[mcalf_ctx::kEnY], moving * ndim)) || (rc = grow(ctx, ctx->enb[mcalf_ctx::kEnLY], moving)) ||
        (rc = grow(ctx, ctx->enb[mcalf_ctx::kEnAux], moving * kEnsAux)) || (rc = grow(ctx, ctx->ens_inside, moving)) ||
        (ctx->ngauss > 0 && (rc = grow(ctx, ctx->ens_pr, rows))))
        return rc;
    EnsArgs a = {};
    a.U0 = r.U0; a.U = r.U; a.L = r.logL; a.status = r.status; a.naccept = r.naccept; a.nswap = r.nswap;
    a.Y = ctx->enb[mcalf_ctx::kEnY]; a.LY = ctx->enb[mcalf_ctx::kEnLY]; a.aux = ctx->enb[mcalf_ctx::kEnAux]; a.inside = ctx->ens_inside;
    a.seed = o.seed; a.scale = o.scale; a.n = (int)n; a.m = (int)m; a.ndim = ctx->ndim; a.move = o.move;
    a.ntemps = o.ntemps; a.chain_temps = o.chain_temps;
    for (size_t t = 0; t < T; ++t) a.beta[t] = beta[t];
    a.prior = prior_dev(ctx);
    a.PR = a.prior.mu ? ctx->ens_pr.p : nullptr;
    const dim3 all((unsigned)rows), half((unsigned)moving), wave(kEnsWave);
    if ((rc = launch_block(ctx, ens_kernel_ptr(kEnsStart), a, all, wave, stream, kEnsLaunch)) || (rc = cube_logl(ctx, a.U, a.L, (int64_t)rows, stream))) return rc;
    double* const chainU = o.chain_temps > 0 ? r.CU : nullptr;
    const size_t slotU = (size_t)o.chain_temps * nb * ndim;
    for (int i = 0; i < o.nsteps; ++i) {
        const bool keep = (i + 1) % o.thin == 0 && (chainU || r.CL);
        const size_t slot = keep ? (size_t)((i + 1) / o.thin - 1) : 0;
        // the swap round this iteration ends with, if any: keyed to the global iteration, so that a continuation is the longer call
        const uint64_t g1 = o.first_iter + (uint64_t)i + 1;
        const bool round = o.swap_every > 0 && g1 % (uint64_t)o.swap_every == 0;
        a.round = round ? g1 / (uint64_t)o.swap_every - 1 : 0;
        a.pair0 = (int)(a.round & 1);
        const unsigned npairs = round ? (unsigned)((o.ntemps - a.pair0) / 2) : 0;      // t = pair0, pair0 + 2, ... with t + 1 < T
        double* const slotCU = keep && chainU ? chainU + slot * slotU : nullptr;
        double* const slotCL = keep && r.CL ? r.CL + slot * rows : nullptr;
        for (int h = 0; h < 2; ++h) {
            a.half = h; a.step = 2 * (o.first_iter + (uint64_t)i) + (uint64_t)h;
            a.keep = keep && h == 1 && npairs == 0 ? 1 : 0;   // (with a swap to come the slot is filled behind it)
            a.CU = a.keep ? slotCU : nullptr;
            a.CL = a.keep ? slotCL : nullptr;
            if ((rc = launch_block(ctx, ens_kernel_ptr(kEnsPropose), a, half, wave, stream, kEnsLaunch)) || (rc = cube_logl(ctx, a.Y, a.LY, (int64_t)moving, stream)) ||
                (rc = launch_block(ctx, ens_kernel_ptr(kEnsDecide), a, half, wave, stream, kEnsLaunch)))
                return rc;
        }
        if (npairs == 0) continue;
        if ((rc = launch_block(ctx, ens_kernel_ptr(kEnsSwap), a, dim3(npairs * (unsigned)n), wave, stream, kEnsLaunch))) return rc;
        if (slotCU) HIP_TRY(ctx, hipMemcpyAsync(slotCU, r.U, slotU * sizeof(double), hipMemcpyDeviceToDevice, stream));
        if (slotCL) HIP_TRY(ctx, hipMemcpyAsync(slotCL, r.logL, rows * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    if (r.theta) return cube_to_theta(ctx, r.U, r.theta, (int64_t)rows, stream);      // the transformed rows of the walkers
    return MCALF_OK;
}

// The host entry's call: the options, the chain arrays the caller wants, and the chain itself (the CU slots, then the CL slots),
// which lives as long as the call.
struct EnsCall { const char* name; const mcalf_pt_opts* o; const double* beta; int64_t n; size_t nCU, nCL; DevBuf<double> chain; };
enum EnsCol { kColU0, kColU, kColTheta, kColL, kColStatus, kColNaccept, kColNswap, kColCU, kColCL, kEnsCols };

// The host entry's device driver (host_staged.cpp: run_staged) over the T n rows; columns in the order of EnsCol, the chain's
// two its own.
int ens_body(mcalf_ctx* ctx, void** dev, int64_t, hipStream_t stream, void* arg) {
    EnsCall* c = static_cast<EnsCall*>(arg);
    if (c->nCU + c->nCL > 0 && hipMalloc((void**)&c->chain.p, (c->nCU + c->nCL) * sizeof(double)) != hipSuccess) {
        (void)hipGetLastError();
        c->chain.p = nullptr;
        return set_err(ctx, MCALF_ERR_NOMEM, "%s: no device memory for the chain of %zu slots (%.1f MB); raise thin", c->name,
                       (size_t)(c->o->nsteps / c->o->thin), (double)(c->nCU + c->nCL) * 8e-6);
    }
    dev[kColCU] = c->nCU ? c->chain.p : nullptr;
    dev[kColCL] = c->nCL ? c->chain.p + c->nCU : nullptr;
    const EnsRows d = {(const double*)dev[kColU0], (double*)dev[kColU], (double*)dev[kColTheta], (double*)dev[kColL], (int32_t*)dev[kColStatus],
                       (int32_t*)dev[kColNaccept], (int32_t*)dev[kColNswap], (double*)dev[kColCU], (double*)dev[kColCL]};
    const int rc = run_ens(ctx, d, c->n, *c->o, c->beta, stream);
    if (rc) (void)hipStreamSynchronize(stream);           // (the chain is freed behind the stream)
    return rc;
}

// The walkers have to meet on one device: a multi-device context's first.
int ens_host(mcalf_ctx* ctx, const char* name, const EnsRows& r, int64_t n, const mcalf_pt_opts& o, const double* beta) {
    const size_t d = sizeof(double), i = sizeof(int32_t), ndim = (size_t)ctx->ndim, nkeep = (size_t)(o.nsteps / o.thin);
    const size_t T = (size_t)o.ntemps;
    EnsCall call = {name, &o, beta, n, r.CU ? nkeep * (size_t)o.chain_temps * (size_t)n * ndim : 0, r.CL ? nkeep * T * (size_t)n : 0, {}};   // (the chain is released when the call returns)
    StagePlan plan = {{stage_in(r.U0, d, ndim), stage_out(r.U, d, ndim), stage_out(r.theta, d, ndim), stage_out(r.logL, d, 1), stage_out(r.status, i, 1),
                       stage_out(r.naccept, i, 1), stage_out(r.nswap, i, (T - 1) * (size_t)n, false),
                       stage_out(r.CU, d, call.nCU, false, true), stage_out(r.CL, d, call.nCL, false, true)},
                      kEnsCols, (int64_t)T * n, kStageFirstDevice, kColU0, kColU, ens_body, &call};
    plan.cols[kColNswap].present = r.nswap && T > 1;      // (one temperature has no neighbour)
    plan.cols[kColCU].present = call.nCU > 0;             // (a call that keeps no slot has no chain)
    plan.cols[kColCL].present = call.nCL > 0;
    return run_staged(ctx, plan);
}

int ens_device(mcalf_ctx* ctx, const EnsRows& r, int64_t n, const mcalf_pt_opts& o, const double* beta, hipStream_t stream) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_ens(ctx, r, n, o, beta, stream);
}

}  // namespace

extern "C" int mcalf_ensemble_batch(mcalf_ctx* ctx, const double* U0, int64_t nwalkers, const mcalf_ens_opts* opts, double* U, double* theta,
                                    double* logL, int32_t* status, int32_t* naccept, double* CU, double* CL) {
    const EnsRows r = {U0, U, theta, logL, status, naccept, nullptr, CU, CL};
    const mcalf_pt_opts o = opts ? one_temperature(*opts) : mcalf_pt_opts();
    const int rc = ens_check(ctx, "mcalf_ensemble_batch", r, nwalkers, opts ? &o : nullptr, kBetaOne, false);
    if (rc) return rc;
    if (nwalkers == 0) return MCALF_OK;
    return ens_host(ctx, "mcalf_ensemble_batch", r, nwalkers, o, kBetaOne);
}

extern "C" int mcalf_ensemble_batch_device(mcalf_ctx* ctx, const double* dU0, int64_t nwalkers, const mcalf_ens_opts* opts, double* dU,
                                           double* dtheta, double* dlogL, int32_t* dstatus, int32_t* dnaccept, double* dCU, double* dCL,
                                           void* stream) {
    const EnsRows r = {dU0, dU, dtheta, dlogL, dstatus, dnaccept, nullptr, dCU, dCL};
    const mcalf_pt_opts o = opts ? one_temperature(*opts) : mcalf_pt_opts();
    const int rc = ens_check(ctx, "mcalf_ensemble_batch_device", r, nwalkers, opts ? &o : nullptr, kBetaOne, false);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_ensemble_batch_device");
    if (nwalkers == 0) return MCALF_OK;
    return ens_device(ctx, r, nwalkers, o, kBetaOne, (hipStream_t)stream);
}

extern "C" int mcalf_tempered_batch(mcalf_ctx* ctx, const double* U0, int64_t nwalkers, const double* beta, const mcalf_pt_opts* opts, double* U,
                                    double* theta, double* logL, int32_t* status, int32_t* naccept, int32_t* nswap, double* CU, double* CL) {
    const EnsRows r = {U0, U, theta, logL, status, naccept, nswap, CU, CL};
    const int rc = ens_check(ctx, "mcalf_tempered_batch", r, nwalkers, opts, beta, true);
    if (rc) return rc;
    if (nwalkers == 0) return MCALF_OK;
    return ens_host(ctx, "mcalf_tempered_batch", r, nwalkers, *opts, beta);
}

extern "C" int mcalf_tempered_batch_device(mcalf_ctx* ctx, const double* dU0, int64_t nwalkers, const double* beta, const mcalf_pt_opts* opts,
                                           double* dU, double* dtheta, double* dlogL, int32_t* dstatus, int32_t* dnaccept, int32_t* dnswap,
                                           double* dCU, double* dCL, void* stream) {
    const EnsRows r = {dU0, dU, dtheta, dlogL, dstatus, dnaccept, dnswap, dCU, dCL};
    const int rc = ens_check(ctx, "mcalf_tempered_batch_device", r, nwalkers, opts, beta, true);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_tempered_batch_device");
    if (nwalkers == 0) return MCALF_OK;
    return ens_device(ctx, r, nwalkers, *opts, beta, (hipStream_t)stream);
}

// The chain diagnostics and the run to convergence, which drives run_ens above in blocks: one translation unit with the sampler.
// (Not a stand-alone header: it defines C entries and must come last, behind run_ens and ens_check.)
#include "host_chain.h"
