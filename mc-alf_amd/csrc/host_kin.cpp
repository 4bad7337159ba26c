// Host side of the optical-depth kinematics kernels (kin_kernels.hip): mcalf_kinematics_batch and
// mcalf_kinematics_batch_device.  One driver (run_kin) issues the equivalent widths' set-up kernel (the records are the same)
// and the four kinematics kernels pass by pass over row blocks, under host_eqw.cpp's rule: the per-row workspaces of a pass
// within kGradChunkBytes, at most 65535 rows (the row is grid.y of the pixel kernels).  The wavelengths and the npix + 1 cell
// edges are device arrays of the context, computed once in mcalf_create.
#include <cmath>

#include "host_ctx.h"
#include "kin_args.h"

namespace {

int kin_ntiles(const mcalf_ctx* ctx) { return (int)((ctx->npix + kKinTile - 1) / kKinTile); }
int64_t kin_nrec(const mcalf_ctx* ctx) { return (int64_t)ctx->ncompmax * ctx->nlines; }
// doubles per row of the four per-row workspaces; the candidates' for `nq` quantiles
int64_t recs_row(const mcalf_ctx* ctx) { return std::max<int64_t>(1, kin_nrec(ctx)) * kEqwRec; }
int64_t part_row(const mcalf_ctx* ctx) { return (int64_t)ctx->nlines * 2 * kin_ntiles(ctx) * kKinSlabs; }
int64_t head_row(const mcalf_ctx* ctx) { return (int64_t)ctx->nlines * kKinHead; }
int64_t cand_row(const mcalf_ctx* ctx, int nq) { return (int64_t)ctx->nlines * kin_ntiles(ctx) * kKinWaves * std::max(1, nq) * kKinCand; }

// Rows per pass, for every nq alike (the candidates counted at kKinMaxQ): a row's pass does not depend on the quantiles asked for.
constexpr int64_t kKinMaxRows = 65535;
int64_t kin_chunk_rows(const mcalf_ctx* ctx) {
    const int64_t per_row = (recs_row(ctx) + part_row(ctx) + head_row(ctx) + cand_row(ctx, kKinMaxQ)) * (int64_t)sizeof(double);
    return std::min<int64_t>(kKinMaxRows, std::max<int64_t>(1, (int64_t)kGradChunkBytes / per_row));
}

int grow_buf(mcalf_ctx* ctx, int b, size_t elems) { return grow(ctx, ctx->kb[b], elems); }

// Everything that is wrong with a call before any device work, and before a row of P is read; `name` is the entry that reports it.
int kin_check(mcalf_ctx* ctx, const char* name, const double* P, int64_t batch, const double* q, int32_t nq, const double* mom, const double* lamq) {
    if (batch < 0) return set_err(ctx, MCALF_ERR_INVALID, "%s: batch must be >= 0, got %lld", name, (long long)batch);
    if (batch > 0 && !P) return set_err(ctx, MCALF_ERR_INVALID, "%s: P is NULL", name);
    if (nq < 0 || nq > kKinMaxQ) return set_err(ctx, MCALF_ERR_INVALID, "%s: nq must be in [0, %d], got %d", name, kKinMaxQ, nq);
    if (!mom && !lamq) return set_err(ctx, MCALF_ERR_INVALID, "%s: mom and lamq are both NULL", name);
    if (nq > 0 && !q) return set_err(ctx, MCALF_ERR_INVALID, "%s: q is NULL with nq = %d", name, nq);
    if (nq > 0 && !lamq) return set_err(ctx, MCALF_ERR_INVALID, "%s: lamq is NULL with nq = %d", name, nq);
    if (nq == 0 && lamq) return set_err(ctx, MCALF_ERR_INVALID, "%s: lamq is given with nq = 0", name);
    for (int j = 0; j < nq; ++j)
        if (!std::isfinite(q[j]) || q[j] < 0.0 || q[j] > 1.0)
            return set_err(ctx, MCALF_ERR_INVALID, "%s: q[%d] = %g is not a fraction in [0, 1]", name, j, q[j]);
    if (!ctx) return set_err(ctx, MCALF_ERR_INVALID, "%s: ctx is NULL", name);
    if (ctx->npix < 2)
        return set_err(ctx, MCALF_ERR_INVALID, "%s: npix = %ld, the kinematics need a spectrum of at least 2 pixels "
                       "(dlam[0] = wl[1] - wl[0])", name, ctx->npix);
    return MCALF_OK;
}

// The batch on `stream`, device pointers: the workspaces of one pass (grown once: a later call of as many rows and quantiles or
// fewer allocates nothing), then the five kernels pass by pass; every kernel takes its argument block by value.
int run_kin(mcalf_ctx* ctx, const double* dP, int64_t batch, const double* q, int32_t nq, double* dmom, double* dlamq, hipStream_t stream) {
    if (batch <= 0) return MCALF_OK;
    const int64_t chunk = kin_chunk_rows(ctx);
    const size_t rows = (size_t)std::min(batch, chunk);
    int rc;
    if ((rc = grow_buf(ctx, mcalf_ctx::kKbRecs, rows * (size_t)recs_row(ctx))) || (rc = grow_buf(ctx, mcalf_ctx::kKbPart, rows * (size_t)part_row(ctx))) ||
        (rc = grow_buf(ctx, mcalf_ctx::kKbHead, rows * (size_t)head_row(ctx))) || (rc = grow_buf(ctx, mcalf_ctx::kKbCand, rows * (size_t)cand_row(ctx, nq))))
        return rc;
    EqwArgs s = {};                                       // the set-up kernel's view: layout indexing, the records alone
    s.lines = ctx->d_lines; s.recs = ctx->kb[mcalf_ctx::kKbRecs]; s.indexing = kEqwIndexLayout; s.lay = row_layout(ctx);
    s.npix = (int)ctx->npix;
    KinArgs a = {};
    a.nu = ctx->d_nu; a.dlam = ctx->d_dlam; a.wl = ctx->d_wl; a.edge = ctx->d_edge; a.tabs = ctx->d_tabs;
    a.recs = ctx->kb[mcalf_ctx::kKbRecs]; a.part = ctx->kb[mcalf_ctx::kKbPart]; a.head = ctx->kb[mcalf_ctx::kKbHead]; a.cand = ctx->kb[mcalf_ctx::kKbCand];
    a.npix = (int)ctx->npix; a.ntiles = kin_ntiles(ctx); a.nq = nq; a.lay = s.lay;
    for (int j = 0; j < nq; ++j) a.q[j] = q[j];
    for (int64_t row0 = 0; row0 < batch; row0 += chunk) {
        s.P = dP + (size_t)row0 * ctx->ndim;
        a.mom = dmom ? dmom + (size_t)row0 * ctx->nlines * 3 : nullptr;
        a.lamq = dlamq ? dlamq + (size_t)row0 * ctx->nlines * nq : nullptr;
        s.nrows = a.nrows = (int)std::min(chunk, batch - row0);
        const dim3 pixel_grid((unsigned)a.ntiles, (unsigned)a.nrows), cell_grid((unsigned)(((size_t)a.nrows * ctx->nlines + 63) / 64));
        if ((rc = LAUNCH_BLOCK(ctx, eqw_kernel_ptr(kEqwSetup), s, dim3((unsigned)a.nrows), dim3(64), stream)) ||
            (rc = LAUNCH_BLOCK(ctx, kin_kernel_ptr(kKinSums), a, pixel_grid, dim3(kKinBlock), stream)) ||
            (rc = LAUNCH_BLOCK(ctx, kin_kernel_ptr(kKinOffsets), a, cell_grid, dim3(64), stream)) ||
            (rc = LAUNCH_BLOCK(ctx, kin_kernel_ptr(kKinScan), a, pixel_grid, dim3(kKinBlock), stream)) ||
            (rc = LAUNCH_BLOCK(ctx, kin_kernel_ptr(kKinFinalize), a, cell_grid, dim3(64), stream)))
            return rc;
    }
    return MCALF_OK;
}

// The host entry's call: what its device driver needs beyond the columns P, mom, lamq.
struct KinCall { const double* q; int32_t nq; };

int host_body(mcalf_ctx* ctx, void** dev, int64_t rows, hipStream_t stream, void* arg) {
    const KinCall* c = static_cast<const KinCall*>(arg);
    return run_kin(ctx, (const double*)dev[0], rows, c->q, c->nq, (double*)dev[1], (double*)dev[2], stream);
}

int run_host(mcalf_ctx* ctx, const double* P, int64_t batch, const double* q, int32_t nq, double* mom, double* lamq) {
    KinCall call = {q, nq};
    const size_t d = sizeof(double), nl = (size_t)ctx->nlines;
    StagePlan plan = {{stage_in(P, d, (size_t)ctx->ndim), stage_out(mom, d, nl * 3), stage_out(lamq, d, nl * (size_t)nq)},
                      3, batch, kStageCutRows, 0, mom ? 1 : 2, host_body, &call};
    return run_staged(ctx, plan);
}

}  // namespace

// wl and the cell edges on the device: e[0] = wl[0] - dlam[0] / 2, e[k] = (wl[k-1] + wl[k]) / 2, e[npix] = wl[npix-1] +
// dlam[npix-1] / 2, with eqw_prepare's dlam.  A one-pixel spectrum has none (the entries refuse it).
int kin_prepare(mcalf_ctx* ctx, const double* wl) {
    if (ctx->npix < 2) return MCALF_OK;
    const size_t n = (size_t)ctx->npix;
    std::vector<double> edge(n + 1);
    edge[0] = wl[0] - (wl[1] - wl[0]) / 2;
    for (size_t k = 1; k < n; ++k) edge[k] = (wl[k - 1] + wl[k]) / 2;
    edge[n] = wl[n - 1] + (wl[n - 1] - wl[n - 2]) / 2;
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_wl.p, n * sizeof(double)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_wl, wl, n * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMalloc((void**)&ctx->d_edge.p, (n + 1) * sizeof(double)));
    HIP_TRY(ctx, hipMemcpy(ctx->d_edge, edge.data(), (n + 1) * sizeof(double), hipMemcpyHostToDevice));
    return MCALF_OK;
}

extern "C" int mcalf_kinematics_batch(mcalf_ctx* ctx, const double* P, int64_t batch, const double* q, int32_t nq, double* mom, double* lamq) {
    const int rc = kin_check(ctx, "mcalf_kinematics_batch", P, batch, q, nq, mom, lamq);
    if (rc || batch == 0) return rc;
    return run_host(ctx, P, batch, q, nq, mom, lamq);
}

extern "C" int mcalf_kinematics_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, const double* q, int32_t nq, double* dmom,
                                             double* dlamq, void* stream) {
    const int rc = kin_check(ctx, "mcalf_kinematics_batch_device", dP, batch, q, nq, dmom, dlamq);
    if (rc) return rc;
    MCALF_SINGLE_ONLY(ctx, "mcalf_kinematics_batch_device");
    if (batch == 0) return MCALF_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    begin_call(ctx, MCALF_PATH_DEVICE, false, false);
    return run_kin(ctx, dP, batch, q, nq, dmom, dlamq, (hipStream_t)stream);
}
