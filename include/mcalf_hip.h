/* mcalf_hip.h -- C ABI of libmcalf_hip.so: the MI355X (gfx950) implementation of the
 * MC-ALF likelihood hot path (Voigt synthesis -> exp(-tau) -> Gaussian-LSF convolution
 * -> Gaussian log-likelihood) for a batch of live points.
 *
 * Every entry point is `extern "C"`, takes plain pointers and sizes, never throws, and
 * returns 0 (MCALF_OK) or a negative MCALF_ERR_* code; the message is available from
 * mcalf_last_error().  Per-sample numerical failures are VALUES in the output
 * (nan / -inf), not errors -- as in the reference, where invalid models surface through
 * np.nansum (hires_fitter.py:294).
 *
 * Reference interfaces replaced (paths relative to /root/reference/mcalf/routines/):
 *   mcalf_create           <- als_fitter.__init__ data/layout state   hires_fitter.py:32-200
 *   mcalf_loglike_batch    <- als_fitter.lnlhood_worker (per row)     hires_fitter.py:287-328
 *                             (and the closure of get_jax_likelihood  hires_fitter.py:685-693
 *                              when conv_mode = MCALF_CONV_SAME_EDGE_JAX)
 *   mcalf_model_batch      <- als_fitter.reconstruct_spec(p,targonly) hires_fitter.py:409-449
 *   mcalf_onecomp_batch    <- reconstruct_onecomp / _onecomp_fill     hires_fitter.py:379-406
 *   mcalf_chi2_batch       <- als_fitter.chi2                         hires_fitter.py:236-248
 *   mcalf_scale_cube_batch <- _scale_cube_pc / _scale_cube_mn         hires_fitter.py:202-216
 *   mcalf_loglike_cube_batch <- lnlhood_pc(_scale_cube_pc(cube))      hires_fitter.py:202-209,250-262
 *   mcalf_loglike_grad_batch <- jax.grad of the get_jax_likelihood closure  hires_fitter.py:521-695
 *                             (no counterpart on the numpy path: finite differences of lnlhood_worker)
 *   mcalf_loglike_hvp_batch  <- jax.jvp(jax.grad(...)) / jax.hessian of the same closure   hires_fitter.py:521-695
 *   mcalf_eqw_batch        <- als_fitter.calc_w                       hires_fitter.py:467-491
 *                             (every row of a chain at once, per component and per line, and the blended profile's width)
 *   mcalf_voigt_hjerting[_nodes] <- scipy.special.wofz(u + i a).real  hires_fitter.py:365
 *                             / voigt_jax.hjert                       voigt_jax.py:121-127
 *   mcalf_set_cu_mask, mcalf_stream_partition
 *                          <- the solver hands over host arrays and trusts the float it gets back
 *                             (hires_fitter.py:250-262,287-294): the host-pointer entries must be right on ANY
 *                             gfx950 device shape (partition modes, CU masks), not only the one they are fastest on
 *   mcalf_set_resident     <- the solvers' one-theta calling pattern  hires_fitter.py:250-285
 *                             (lnlhood_pc / _dy / _mn, one call per proposed point)
 *   mcalf_broker_serve[_resident], mcalf_mailbox_call
 *                          <- one solver rank per core, each calling  ../cli.py:37-41,110
 *                             the likelihood serially (PolyChord's MPI workers)
 *   mcalf_comm_* / mcalf_loglike_gather[v]_device
 *                          <- data parallelism over live points       ../cli.py:110,274-280
 *   mcalf_create_multi, mcalf_last_launch_sub
 *                          <- ONE process holds the whole batch       ../cli.py:274-280 (jaxns vmaps the likelihood over
 *                             the live points inside one Python process): one context that drives several devices
 *   mcalf_get_config       <- (none: the reference has no tunables on this path; the library says which of its own
 *                             the loading process's environment has set)
 *
 * Ownership: the context owns all device memory it allocates.  Host pointers passed to
 * any call are borrowed for the duration of that call only.  `*_device` entries take
 * DEVICE pointers valid on the context's GPU and enqueue on the given hipStream_t
 * (passed as void*; NULL = the legacy default stream) without synchronising.
 *
 * Threading: a context is not re-entrant (one in-flight call per context, and every
 * asynchronous call of a context on the same stream); distinct contexts are independent.
 * A resolution beyond the provisioned specres_max makes a row's model NaN, its logL -inf and
 * its chi2 +inf (the reference would allocate a longer kernel).  The provisioned LSF itself may be of
 * ANY width, under both boundary modes: one whose halo does not fit a 4096-pixel workgroup tile is
 * convolved by a second pair of kernels behind the fused one (same entries, same conventions;
 * hires_fitter.py:458-464 / the fixed grid of :549-560).  Only a MCALF_CONV_SAME_EDGE_JAX grid longer than
 * the spectrum is refused (MCALF_ERR_INVALID): the reference's jnp.convolve / jnp.where cannot broadcast
 * it either.
 */
#ifndef MCALF_HIP_H
#define MCALF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCALF_ABI_VERSION 9   /* 2: mcalf_last_launch, gatherv / overlap / join, version string carries the source hash
                                 3: MCALF_PATH_HOST_STREAM, mcalf_launch_info_t grows by stream_setup_wgs / stream_polled
                                 4: mcalf_broker_serve
                                 5: mcalf_set_resident, mcalf_broker_serve_resident
                                 6: mcalf_set_cu_mask, mcalf_stream_partition, mcalf_launch_info_t grows by xcd_mask / stream_wgs_min /
                                    stream_wgs_max / stream_fallback (the streaming launch is taken only on the device shape it
                                    was built for, and checked after every launch)
                                 7: mcalf_create_multi, mcalf_last_launch_sub, mcalf_get_config; mcalf_info_t grows by ndevices /
                                    devices[16], mcalf_launch_info_t by devices_used
                                 8: mcalf_loglike_grad_batch[_device], mcalf_voigt_hjerting_grad (the analytic gradient of logL)
                                 9: mcalf_model_jvp_batch[_device], mcalf_model_vjp_batch[_device] (the model Jacobian's products
                                    with a vector)
                                    (added within 9, nothing else changed: mcalf_loglike_hvp_batch[_device], the product of
                                    logL's exact Hessian with a vector;
                                    mcalf_eqw_batch[_device], batched equivalent widths;
                                    mcalf_model_band_batch[_device], per-pixel mean, variance and quantiles of the model
                                    over the rows of a chain;
                                    mcalf_fisher_matvec_batch[_device], the Fisher product J^T W J v on the device, and
                                    mcalf_maximize_batch[_device], batched Levenberg-Marquardt maximisation of logL;
                                    mcalf_slice_replace_batch[_device], nested sampling's replacement step: batched slice
                                    moves in the unit cube under a likelihood constraint;
                                    mcalf_set_slice_compact, mcalf_slice_last_stats: the host entry of the replacement step
                                    packs the rows that proposed a trial, and what a slice call launched;
                                    mcalf_ensemble_batch[_device], the ensemble MCMC sampler: stretch and DE moves of a walker
                                    set in the unit cube, the chain kept on the device;
                                    mcalf_tempered_batch[_device], parallel tempering of that sampler: a ladder of temperatures
                                    moved in the same launches, swaps between neighbours;
                                    mcalf_nested_open / _advance / _finish / _read / _last_round / _close / _footprint /
                                    _set_timing / _last_times, a nested-sampling run whose live and dead points stay on the device;
                                    mcalf_hmc_batch[_device], Hamiltonian Monte Carlo of independent walkers in the unit cube,
                                    driven by the analytic gradient;
                                    mcalf_chain_stats[_device], chain diagnostics on the device: autocorrelation time, split
                                    R-hat and effective sample size, and mcalf_ensemble_converge[_device], the ensemble sampler
                                    run until they say it has converged) */

enum {
    MCALF_OK = 0,
    MCALF_ERR_INVALID = -1,   /* bad argument / inconsistent spec          */
    MCALF_ERR_HIP = -2,       /* a HIP runtime call failed                 */
    MCALF_ERR_NODEVICE = -3,  /* no usable gfx950 device                   */
    MCALF_ERR_RANGE = -4,     /* problem exceeds a build-time capacity     */
    MCALF_ERR_NOMEM = -5,
    MCALF_ERR_COMM = -6       /* RCCL missing or a collective call failed  */
};

enum {
    MCALF_CONV_WRAP_NUMPY = 0,    /* numpy path: periodic boundary, per-sample kernel length,
                                     convolution skipped when R <= velstep (hires_fitter.py:445-464) */
    MCALF_CONV_SAME_EDGE_JAX = 1  /* JAX path: fixed kernel grid from max specres, zero padding,
                                     edges reset to the unconvolved model, always convolved,
                                     floor() on the ncomp slot (hires_fitter.py:549-560,616,667-681) */
};

typedef struct mcalf_ctx mcalf_ctx;

/* One transition: rest wavelength [Angstrom], oscillator strength, damping gamma [1/s]. */
typedef struct {
    double wrest_A;
    double f;
    double gamma;
} mcalf_line;

/* Problem definition: what als_fitter.__init__ leaves in `self` for the likelihood to read. */
typedef struct {
    int64_t npix;            /* number of selected pixels                                    */
    const double* wl;        /* [npix] obj_wl, Angstrom            (host, copied)            */
    const double* flux;      /* [npix] obj                         (host, copied)            */
    const double* err;       /* [npix] obj_noise                   (host, copied)            */
    double velstep;          /* km/s per pixel (hires_fitter.py:84-87)                       */
    int32_t nlines;          /* numlines                                                     */
    const mcalf_line* lines; /* [nlines] linepars                  (host, copied)            */
    mcalf_line fill;         /* linefill (hires_fitter.py:120-121)                           */
    int32_t ncompmax;        /* upper bound of the ncomp slot                                */
    int32_t nfill;           /* number of filler components                                  */
    int32_t freespecres;     /* 1: p[0] is the LSF FWHM                                      */
    int32_t freecont;        /* 1: continuum is a free parameter                             */
    double specres_fixed;    /* FWHM km/s used when !freespecres: max(specres) for the numpy
                                path, specres[0] for the JAX path                            */
    double specres_max;      /* largest FWHM any sample may carry (sizes the LDS halo and the
                                fixed JAX kernel grid)                                       */
    double contval_fixed;    /* continuum when !freecont                                     */
    int32_t conv_mode;       /* MCALF_CONV_*                                                 */
    int32_t device;          /* HIP device ordinal, or -1 for the current device             */
    int32_t asymmlike;       /* 1: asymmetric veto of hires_fitter.py:296-303 in loglike      */
    double asymm_n4;         /* gauss_cdf[1]: allowed count of (obj-model)/err > 4 before the
                                0.01*npix grace (the reference draws it from an unseeded
                                np.random.normal, :179-181, so it is an input here)          */
    double asymm_n5;         /* gauss_cdf[2]: same for > 5                                    */
} mcalf_spec;

typedef struct {
    int32_t abi_version;
    int32_t ndim;       /* [freespecres] + [freecont] + 1 + 3*ncompmax + 3*nfill             */
    int32_t startind;   /* index of the ncomp slot      (hires_fitter.py:169-174)            */
    int32_t endind;     /* first filler parameter       (hires_fitter.py:176)                */
    int32_t n_cap;      /* LSF half-width (pixels) provisioned from specres_max              */
    int32_t tile;       /* pixels per workgroup tile                                         */
    int32_t ntiles;     /* tiles per sample                                                  */
    int32_t device;     /* HIP device ordinal in use                                         */
    int64_t npix;
    char arch[32];      /* gcnArchName of the device                                         */
    int32_t ndevices;   /* device entries of the context: 1, or what mcalf_create_multi took */
    int32_t devices[16];/* their HIP ordinals (entries may repeat)                           */
} mcalf_info_t;

/* Create / destroy.  mcalf_create never returns a half-built context: on failure *out is
 * NULL and mcalf_last_error(NULL) holds the message. */
int mcalf_create(const mcalf_spec* spec, mcalf_ctx** out);
/* ONE context over several devices of this process (spec->device is ignored; `devices` lists 1 .. 16 HIP ordinals, an
 * ordinal may repeat -- two entries on one GPU are two independent sub-contexts).  The reference's large batches arise
 * inside one process (jaxns vmaps the likelihood over the live points, cli.py:274-280): the host-pointer entries of such
 * a context -- mcalf_loglike_batch, _chi2_batch, _model_batch, _onecomp_batch, _loglike_cube_batch -- cut the rows into
 * contiguous blocks whose sizes differ by at most one (entry k of the n entries in use; an entry gets at least 256
 * rows, so small calls and the one-theta callables run on entry 0 alone), issue every device's call concurrently -- the
 * calling thread drives entry 0, a helper thread of the context each of the others -- and every device writes its block of
 * results straight into the caller's array: no collective, no device-to-device traffic.  A live point's arithmetic does
 * not depend on the shard: the results equal the single-device ones bit for bit.  mcalf_set_prior / _set_chunks /
 * _set_cu_mask / _reserve apply to every entry, mcalf_set_resident to entry 0; the *_device entries, the profile brackets,
 * the broker and the mcalf_comm_* family need a single-device context (MCALF_ERR_INVALID). */
int mcalf_create_multi(const mcalf_spec* spec, const int32_t* devices, int32_t ndevices, mcalf_ctx** out);
/* How a multi-device context of `nentries` device entries cuts a batch: *entries_used = the entries that take part (every one
 * of them gets at least 256 rows), [*lo, *hi) = the rows of entry k (empty for an entry that sits the call out).  Pure host
 * arithmetic, no device needed -- the functions mcalf_create_multi's contexts use; block sizes differ by at most one, the
 * first batch % entries_used entries take the longer ones (mc-alf_amd/dist.py::shard_bounds, the split of the one-process-
 * per-GPU form). */
int mcalf_shard_bounds(int64_t batch, int32_t nentries, int32_t k, int32_t* entries_used, int64_t* lo, int64_t* hi);
void mcalf_destroy(mcalf_ctx* ctx);
int mcalf_info(const mcalf_ctx* ctx, mcalf_info_t* info);
const char* mcalf_last_error(const mcalf_ctx* ctx);
/* "mcalf_hip <version> (gfx950, abi <n>) src <hash>": <hash> = first 16 hex digits of the sha256 over the kernel
 * sources the library was built from ("unstamped" for a build that did not go through mc-alf_amd/build.py). */
const char* mcalf_version(void);
/* The configuration the context runs under, as text ("name=value ..." followed by "[env: ...]", the MCALF_* variables that
 * were set and valid when the context was created -- the library reads its environment exactly once per context, in
 * mcalf_create): written into buf (n bytes, always terminated; ~600 bytes suffice). */
int mcalf_get_config(const mcalf_ctx* ctx, char* buf, int64_t n);

/* Pre-size the context's device workspaces for batches up to `batch` rows so that later
 * calls (including *_device calls captured into a hipGraph) allocate nothing. */
int mcalf_reserve(mcalf_ctx* ctx, int64_t batch);

/* logL[i] = lnlhood_worker(P[i, :]) for i < batch.   P row-major [batch][ndim], host. */
int mcalf_loglike_batch(mcalf_ctx* ctx, const double* P, int64_t batch, double* logL);
/* flux[i, :] = reconstruct_spec(P[i, :], targonly).  flux row-major [batch][npix], host. */
int mcalf_model_batch(mcalf_ctx* ctx, const double* P, int64_t batch, int32_t targonly, double* flux);
/* chi2[i] = nansum(ispec2 (obj - model)^2); +inf when the model is identically zero. */
int mcalf_chi2_batch(mcalf_ctx* ctx, const double* P, int64_t batch, double* chi2);
/* Single-component spectra: rows of Q are (R, cont, N, z, b).  which = 0: every line of the
 * component (reconstruct_onecomp); 1: the filler line (reconstruct_onecomp_fill); 2 + k: line k
 * alone (the per-line model calc_w integrates, hires_fitter.py:483). */
int mcalf_onecomp_batch(mcalf_ctx* ctx, const double* Q, int64_t batch, int32_t which, double* flux);

/* Resident one-theta evaluator (off by default).  The solvers call the likelihood one theta at a time (lnlhood_pc / _dy /
 * _mn: hires_fitter.py:250-285); of such a call about a third is the kernel LAUNCH, and launches of different processes
 * serialise.  With idle_us > 0, mcalf_loglike_batch calls of ONE row on a spectrum that fits one pixel tile are answered by
 * one workgroup that STAYS on the chip between calls and takes its requests from a page-locked mailbox -- same arithmetic,
 * same bits, no launch.  The kernel leaves by itself after idle_us microseconds without a request (the next call starts
 * another one), so a device-wide synchronisation never waits longer than that; idle_us = 0 tells it to leave now and turns
 * the mode off.  Other entries of the context are not affected (the evaluator has its own stream and its own memory).
 * The environment variable MCALF_RESIDENT_US gives the initial value. */
int mcalf_set_resident(mcalf_ctx* ctx, int32_t idle_us);

/* Likelihood broker, serving side: MANY one-theta-at-a-time solver ranks (PolyChord runs one MPI rank per core, each calling
 * lnlhood_pc(theta) serially: cli.py:37-41, 110; hires_fitter.py:250-262) served by ONE thread of ONE process that owns the
 * device contexts.  The request block lives wherever the caller puts it (mc-alf_amd/broker.py: POSIX shared memory); rank s
 * writes its row theta[s * theta_stride ..], then bumps req[s * counter_stride]; the server evaluates every open request of
 * the moment as one small batch on a context that is free, writes logl[s * logl_stride] and then sets ack[..] to the
 * request number.  With several contexts, requests that arrive while a launch is in flight leave at once on the next free
 * context.  Returns when *stop becomes non-zero (after answering what is in flight) or after max_seconds (0: never). */
typedef struct {
    int32_t slots;              /* request slots, one per solver rank */
    int32_t ndim;               /* doubles per parameter row (the contexts' ndim) */
    volatile uint64_t* req;     /* [slots * counter_stride] */
    volatile uint64_t* ack;     /* [slots * counter_stride] */
    int64_t counter_stride;     /* in 64-bit words (8: one cache line per slot) */
    const double* theta;        /* [slots * theta_stride] */
    int64_t theta_stride;       /* in doubles, >= ndim */
    double* logl;               /* [slots * logl_stride] */
    int64_t logl_stride;        /* in doubles */
    volatile uint64_t* stop;
    uint64_t* stats;            /* optional [2]: launches and thetas served so far (incremented) */
    double idle_sleep_after_s;  /* spin this long without a request before yielding the core between polls */
} mcalf_broker_t;
int mcalf_broker_serve(mcalf_ctx* const* ctxs, int32_t nctx, const mcalf_broker_t* b, double max_seconds);

/* The broker with RESIDENT evaluators: every solver rank gets a workgroup that stays on the chip and takes the rank's requests
 * straight from its mailbox in the shared block -- no server thread and no launch on a call's path.  `boxes` points to `slots`
 * mailboxes of MCALF_MAILBOX_BYTES each (64-byte aligned, zero-filled by whoever creates the block), laid out as
 *   uint32 req, quit, ack, state;  double result;  double reserved[5];  double row[64]
 * Rank s: result <- the bit pattern MCALF_RESULT_PENDING, row <- theta, then req <- req + 1 (in that order; a release store);
 * spin until result differs from the pattern.  This call page-locks the block (hipHostRegister) and keeps ONE launch of
 * `slots` workgroups alive while requests come (workgroup k polls mailbox k; they leave TOGETHER after idle_us without a
 * request on any mailbox, and the next request starts the launch again -- one launch on one stream, because hardware queues
 * are few); it returns when *stop becomes non-zero (every workgroup has left by then) or after max_seconds (0: never).  Serves spectra of one pixel tile with at
 * most 64 parameters (MCALF_ERR_RANGE otherwise: use mcalf_broker_serve).
 * Co-residency: a mailbox is served only while its workgroup is on the chip, and all `slots` workgroups of the launch are
 * expected to be there at once -- one per compute unit, so `slots` may not exceed the device's CU count (MCALF_ERR_INVALID;
 * 256 on an unpartitioned MI355X).  While another kernel occupies compute units (a batch call of this process, another
 * process), workgroups that find no CU leave their mailboxes unpolled until one frees up: such a call waits, it is not lost. */
#define MCALF_MAILBOX_BYTES 576
#define MCALF_RESULT_PENDING 0x7FF8C0DEC0DE0001ull
int mcalf_broker_serve_resident(mcalf_ctx* ctx, void* boxes, int32_t slots, volatile uint64_t* stop, int32_t idle_us,
                                uint64_t* stats, double max_seconds);

/* A rank's side of the mailbox protocol, for solvers written in C / C++ / Fortran (header-only; the Python ranks do the same in
 * mc-alf_amd/broker.py): logL of theta[0 .. ndim) through the mailbox at `box`.  Spins until the rank's workgroup has answered
 * (the result slot no longer holds the pending pattern, or -- should the answer itself be that pattern -- `ack` equals the
 * request number); returns the canonical NaN when *stop (may be NULL) becomes non-zero first, or when max_spins (0: no limit)
 * looks have passed without an answer: a server that has died raises no stop flag, so a caller that cannot watch the server
 * process should pass a limit (a look is ~10 ns; 3e9 is about half a minute). */
#if defined(__GNUC__) || defined(__clang__)
static inline double mcalf_mailbox_call_bounded(void* box, const double* theta, int32_t ndim, const volatile uint64_t* stop,
                                                uint64_t max_spins) {
    volatile uint32_t* words = (volatile uint32_t*)box;            /* req, quit, ack, state */
    volatile uint64_t* result = (volatile uint64_t*)((char*)box + 16);
    double* row = (double*)((char*)box + 64);
    union { uint64_t u; double d; } v;
    int32_t i;
    uint64_t spins = 0;
    const uint32_t seq = words[0] + 1u;
    *result = MCALF_RESULT_PENDING;
    for (i = 0; i < ndim; ++i) row[i] = theta[i];
    __atomic_store_n(&words[0], seq, __ATOMIC_RELEASE);            /* the request number, last */
    while ((v.u = __atomic_load_n(result, __ATOMIC_ACQUIRE)) == MCALF_RESULT_PENDING) {
        if (__atomic_load_n(&words[2], __ATOMIC_ACQUIRE) == seq) { v.u = __atomic_load_n(result, __ATOMIC_ACQUIRE); break; }
        ++spins;
        if ((stop && (spins & 0xFFFFu) == 0 && *stop) || (max_spins && spins >= max_spins)) { v.u = 0x7FF8000000000000ull; break; }
    }
    return v.d;
}
static inline double mcalf_mailbox_call(void* box, const double* theta, int32_t ndim, const volatile uint64_t* stop) {
    return mcalf_mailbox_call_bounded(box, theta, ndim, stop, 0);
}
#endif

/* Row blocks a batch is issued in (0 = automatic [default], n <= 8 = exactly n).  Automatic means ONE block
 * for the *_device entries (the persistent fused kernel leaves no launch tail worth filling; measured) and, for
 * the host-pointer entries with large batches, ONE streaming launch (MCALF_PATH_HOST_STREAM: spectra that fit one pixel
 * tile, and tiled ones up to 65536 work items -- live points x tiles; MCALF_STREAM=2 streams larger tiled batches too; an
 * explicit block count, MCALF_STREAM=0, a larger tiled batch or a launch below the persistent-grid threshold selects the
 * row-block pipeline instead: a first block of
 * 128 KiB of parameter rows (MCALF_HOST_FIRST_KB; twice that for page-locked input), every following block twice the one
 * before, the last one taking the rest, so that the GPU starts after ~10 us of staging and block k+1's staging copy,
 * H2D copy and per-sample set-up run under block k's kernel).  With more than one block in a *_device call the
 * blocks after the first run on context-owned streams between a fork event recorded on the caller's stream and
 * join events that stream waits for: the call keeps plain stream semantics (and can be captured into a
 * hipGraph).  Results do not depend on the setting (every live point is evaluated independently).  The
 * environment variable MCALF_CHUNKS gives the initial value. */
int mcalf_set_chunks(mcalf_ctx* ctx, int32_t nchunks);
/* Row blocks a *_device call of `batch` rows is issued in under the current setting. */
int32_t mcalf_get_chunks(const mcalf_ctx* ctx, int64_t batch);

/* Same, device pointers + stream, asynchronous.
 * Stream rule: all asynchronous calls of ONE context must be issued on ONE stream (the context's per-sample
 * workspaces are shared by its launches and ordered only by that stream); call mcalf_reserve(batch) first when
 * the call is to be captured into a hipGraph or must not allocate (a *_device call otherwise grows the
 * workspaces on first use, which synchronises the device). */
int mcalf_loglike_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, double* dlogL, void* stream);
int mcalf_model_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, int32_t targonly,
                             double* dflux, void* stream);

/* The analytic gradient of logL: logL[i] as mcalf_loglike_batch gives it and G[i, k] = d logL[i] / d P[i, k]
 * (batch x ndim, row-major) under the context's conv_mode.  Columns that are 0 by definition: the ncomp slot and
 * the (N, z, b) of every component at or beyond the row's active count.  Rows whose logL is -inf (asymmetric veto)
 * or NaN get an all-NaN row of G.  On the numpy path the LSF tap count is held at its value for the row: G is the
 * derivative within that piece (logL itself jumps where the count changes); the R column is 0 when R <= velstep.
 * Host pointers, synchronous; `logL` may be NULL.  A multi-device context cuts the batch into contiguous row
 * blocks, one per device, written straight into the caller's arrays.  A row's result does not depend on its
 * batch, its position or the device count (every reduction runs in a fixed order). */
int mcalf_loglike_grad_batch(mcalf_ctx* ctx, const double* P, int64_t batch, double* logL, double* G);
/* Same, device pointers, on the caller's stream (single-device contexts).  After one call of the same or a larger
 * batch it allocates and synchronises nothing. */
int mcalf_loglike_grad_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, double* dlogL, double* dG,
                                    void* stream);

/* The model Jacobian's products with a vector, matrix-free.  J(P[i]) [k, c] = d m_k / d P[i, c] (npix x ndim) is the
 * Jacobian of the full model m = mcalf_model_batch(targonly = 0) of row i under the context's conv_mode; it is never
 * formed.  P, V, G are batch x ndim, Q and dM batch x npix, all row-major.
 *   JVP:  dM[i, :] = J(P[i]) V[i, :]     the directional derivative of the model along a parameter tangent
 *   VJP:  G[i, :]  = J(P[i])^T Q[i, :]   the caller's per-pixel cotangent pulled back to the parameters
 * (the gradient of logL is the VJP of Q = (d - m) / err^2 on the pixels nansum keeps; a Fisher product J^T W J v is one
 * JVP and one VJP).  ONE tangent or cotangent per row: the batch axis is the vector axis, so k vectors at one theta are
 * k rows that repeat it.  Columns that are 0 by definition, as in the gradient: the ncomp slot and the (N, z, b) of every
 * component at or beyond the row's active count -- those entries of V are ignored and those of G are exactly 0, as are
 * the R / continuum entries when the context fixes them.  Q is used as given (non-finite entries propagate).  On the
 * numpy path the LSF tap count is held at its value for the row; a row whose tap count exceeds what the context
 * provisions (R beyond specres_max) gets an all-NaN row.  Host pointers, synchronous; a multi-device context cuts the
 * batch into contiguous row blocks, one per device, written straight into the caller's arrays.  A row's result does not
 * depend on its batch, its position or the device count (every reduction runs in a fixed order). */
int mcalf_model_jvp_batch(mcalf_ctx* ctx, const double* P, const double* V, int64_t batch, double* dM);
int mcalf_model_vjp_batch(mcalf_ctx* ctx, const double* P, const double* Q, int64_t batch, double* G);
/* Same, device pointers, on the caller's stream (single-device contexts).  After one call of the same or a larger
 * batch they allocate and synchronise nothing. */
int mcalf_model_jvp_batch_device(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* ddM, void* stream);
int mcalf_model_vjp_batch_device(mcalf_ctx* ctx, const double* dP, const double* dQ, int64_t batch, double* dG, void* stream);

/* The product of logL's exact Hessian with a vector: HV[i, :] = (d2 logL[i] / dtheta2)(P[i]) V[i, :] under the context's
 * conv_mode, P, V, HV all batch x ndim, row-major.  With r = d - m, W = 1/err^2 on the pixels nansum keeps (0 elsewhere) and
 * J the model Jacobian,  H v = -J^T W (J v) + sum_i W_i r_i (d2 m_i / dtheta2) v : the Gauss-Newton (Fisher) term AND the
 * curvature term, the directional derivative along v of the whole gradient mcalf_loglike_grad_batch computes.  Neither H
 * nor J is formed.  The conventions are that entry's:
 *   - ONE tangent per row: the batch axis is the vector axis, so k vectors at one theta are k rows that repeat it (the dense
 *     Hessian is ndim rows with the identity's rows as tangents);
 *   - the ncomp slot and the (N, z, b) of every component at or beyond the row's active count: those entries of V are
 *     ignored (never read) and those of HV are exactly 0; likewise R / the continuum when the context fixes them, and R when
 *     R <= velstep on the numpy path (no convolution);
 *   - on the numpy path the LSF tap count is held at its value for the row;
 *   - rows whose logL is -inf (asymmetric veto) or NaN, or whose tap count exceeds what the context provisions (R beyond
 *     specres_max), get an all-NaN row; logL for that rule comes from the likelihood's own launch;
 *   - a row's result does not depend on its batch, its position, the pass it falls in or the device count (no atomics,
 *     every reduction in a fixed order).
 * Host pointers, synchronous; a multi-device context cuts the batch into contiguous row blocks exactly as the gradient does. */
int mcalf_loglike_hvp_batch(mcalf_ctx* ctx, const double* P, const double* V, int64_t batch, double* HV);
/* Same, device pointers, on the caller's stream (single-device contexts); dP and dV are only read.  After one call of the
 * same or a larger batch it allocates and synchronises nothing. */
int mcalf_loglike_hvp_batch_device(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* dHV, void* stream);

/* Equivalent widths of every row, on the device, without a spectrum reaching memory (the analysis pass over a chain:
 * als_fitter.calc_w, hires_fitter.py:467-491).  P is batch x ndim.  With dlam[0] = wl[1] - wl[0], dlam[i] = wl[i] - wl[i-1]
 * (:485-486) and tau_cl the optical depth of line l of the component in slot c alone (voigt_tau, :331-367):
 *   Wcomp[i, c, l] = ( sum_pix (1 - exp(-tau_cl(pix))) dlam[pix] ) / (1 + z_c)      batch x ncompmax x nlines, rest frame, Angstrom
 *   Wblend[i, l]   =   sum_pix (1 - exp(-sum_c tau_cl(pix))) dlam[pix]              batch x nlines, observed frame, Angstrom
 * the second summed over the same slots: the width of the absorption system in line l, which overlapping components make
 * smaller than sum_c (1 + z_c) Wcomp.  Either output may be NULL, not both.  Nothing is convolved (the periodic, normalised
 * LSF does not change W) and the continuum does not enter (the reference's (cont v) / cont; the NaN it gives for a zero or
 * non-finite continuum is the caller's to reproduce).  Fillers take no part.  The Voigt function is the likelihood's.
 *   MCALF_EQW_LAYOUT      slot c reads (N, z, b) at startind + 1 + 3c for c below the row's active count -- int() of the
 *                         ncomp slot on the numpy path, floor on the JAX path, clamped to [0, ncompmax], as the likelihood
 *                         decodes it; the cells of the other slots are exactly 0 and their parameters are never read.
 *   MCALF_EQW_AS_WRITTEN  all ncompmax slots, slot c reading (N, z, b) at startind + 3c: the reference as written (:481-482),
 *                         its triples shifted by one against the layout.
 * The conventions are the derivative entries': per-row numerical failures are values (a NaN in one row touches only that
 * row); no atomics, every reduction in one fixed order, so a row's bits do not depend on its batch, its position, the pass it
 * falls in, the outputs requested or the device count; a multi-device context cuts the rows as mcalf_loglike_grad_batch
 * does.  MCALF_ERR_INVALID before any device work for: a NULL context, batch < 0, a NULL P with batch > 0, both outputs
 * NULL, an indexing outside {0, 1}, a spectrum of fewer than 2 pixels (dlambda[0] needs two).  batch == 0 does nothing. */
enum { MCALF_EQW_LAYOUT = 0, MCALF_EQW_AS_WRITTEN = 1 };
int mcalf_eqw_batch(mcalf_ctx* ctx, const double* P, int64_t batch, int32_t indexing, double* Wcomp, double* Wblend);
/* Same, device pointers, on the caller's stream (single-device contexts).  After one call of the same or a larger batch it
 * allocates and synchronises nothing. */
int mcalf_eqw_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, int32_t indexing, double* dWcomp, double* dWblend,
                           void* stream);

/* Optical-depth kinematics of every row and target line, on the device (the analysis pass over a chain): WHERE in wavelength
 * the model's absorption sits -- the integral of tau, its centroid, its width, and the wavelengths below which given fractions
 * of it lie (q = 0.05 and 0.95 bound the Delta v90 interval of Prochaska & Wolfe 1997).  Taken on the model's tau, not on a
 * flux, so a saturated core does not spoil them.  P is batch x ndim.  For row i and line l, with nc the row's active count as
 * MCALF_EQW_LAYOUT reads it, slot c < nc reading (N, z, b) at startind + 1 + 3c, and dlam as mcalf_eqw_batch has it:
 *   tau[k]   = sum_{c < nc} tau_cl(wl[k])       the slots in slot order into one accumulator that starts at 0.0; tau_cl is
 *                                               mcalf_eqw_batch's (the folded tables, K hjert_general, nothing for |1 + z| > 1e100)
 *   t[k]     = tau[k] dlam[k]
 *   S[k]     = sum_{j <= k} t[j],   I = S[npix - 1]                  integral of tau dlambda, Angstrom, observed frame
 *   piv      = wl[npix / 2],   M1 = sum t[k] (wl[k] - piv),   lam_mean = piv + M1 / I
 *   V        = ( sum t[k] (wl[k] - lam_mean)^2 ) / I,   lam_rms = sqrt(V)       centred on the finished mean, a second pass
 *   e[0]     = wl[0] - dlam[0] / 2,  e[k] = (wl[k-1] + wl[k]) / 2,  e[npix] = wl[npix-1] + dlam[npix-1] / 2        cell edges
 *   lam_q    : target = q I; k the first pixel for which S[k] < target is false (none: npix - 1); frac = (S[k] - target) / t[k]
 *              clamped to [0, 1], 0 where t[k] > 0 does not hold; lam_q = e[k+1] - (e[k+1] - e[k]) frac -- continuous across
 *              pixels, unbiased on a uniform grid
 *   mom[i, l, :]  = I, lam_mean, lam_rms        batch x nlines x 3
 *   lamq[i, l, j] = lam_q[j]                    batch x nlines x nq
 * I not finite or 0: lam_mean, lam_rms and every lam_q are NaN, I stays as computed; nc = 0 gives I = 0 exactly.  A NaN in an
 * active slot makes that row's outputs NaN and touches no other row; the parameters of the other slots are never read.  Nothing
 * is convolved, the continuum does not enter, fillers take no part.  A spectrum of several fit ranges has ONE wide dlam at each
 * gap, as als_fitter.calc_w has: the pixel after a gap weighs its tau with the gap's width.
 * Either output may be NULL, not both; lamq == NULL exactly when nq == 0; nq <= 16; every q[j] finite and in [0, 1].  No
 * floating-point atomics, every sum in ONE order (inside a wave of 64 consecutive pixels a fixed scan, the waves in pixel
 * order), I is the last value of the device's own S: a row's bits do not depend on its batch, its position, the pass it
 * falls in, nq, the values of q, the outputs requested or the device count.  Row passes hold at most 65535 rows and 384 MiB of
 * per-row workspace.  MCALF_ERR_INVALID before any device work for: a NULL context, batch < 0, a NULL P with batch > 0, nq
 * outside [0, 16], nq > 0 with a NULL q or lamq, lamq with nq == 0, a q[j] not finite or outside [0, 1], mom and lamq both
 * NULL, a spectrum of fewer than 2 pixels.  batch == 0 does nothing.  Host pointers, synchronous; a multi-device context cuts
 * the rows as mcalf_eqw_batch does. */
int mcalf_kinematics_batch(mcalf_ctx* ctx, const double* P, int64_t batch, const double* q, int32_t nq, double* mom, double* lamq);
/* Same, device pointers, on the caller's stream (single-device contexts).  q is a HOST array, read during the call (its values
 * travel in the kernels' argument block).  After one call of the same or a larger batch and nq it allocates and synchronises
 * nothing. */
int mcalf_kinematics_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, const double* q, int32_t nq, double* dmom,
                                  double* dlamq, void* stream);

/* Per-pixel posterior bands of the model over the rows of a chain, on the device, without a spectrum reaching the host (the
 * reference's plot pass overplots 100 sampled spectra instead, mcalf/cli.py:398-418).  With M[i, :] = mcalf_model_batch(P[i],
 * targonly) under the context's conv_mode -- the same kernels, the same bits, wide LSFs and tiled spectra included -- and,
 * for pixel k, the rows whose M[i, k] is not NaN (np.nanmean / np.nanvar / np.nanquantile):
 *   nvalid[k]   [npix]      how many such rows there are
 *   mean[k]     [npix]      their arithmetic mean
 *   var[k]      [npix]      their population variance (ddof 0), in TWO passes: the mean first, then the centred squares (a
 *                           continuum pixel is 1 with a spread of 1e-10: E[x^2] - mean^2 would be rounding noise there)
 *   Q[j, k]     [nq][npix]  the q[j]-quantile under numpy's default "linear" rule: h = (nvalid - 1) q[j], lo = x_(floor h),
 *                           hi = x_(min(floor h + 1, nvalid - 1)), Q = lo + (hi - lo) (h - floor h), x_(r) the r-th smallest
 *                           valid value -- an EXACT selection among the stored values (radix select), no histogram estimate
 * A pixel with nvalid == 0 has NaN in mean, var and Q.  Any of mean, var, Q, nvalid may be NULL, not all; Q == NULL exactly
 * when nq == 0; nq <= 16; every q[j] finite and in [0, 1].  The conventions are the derivative entries': a row's numerical
 * failure is a value (an all-NaN row simply does not count); no floating-point atomics, every floating-point sum in ONE order
 * that depends on neither the batch, the grid nor the outputs requested (rows in blocks of 256, a block's rows in row order
 * per 64, the blocks in block order; the radix histograms are integer counters); two calls on the same input give the same bits.
 * Memory: the statistic needs every row resident.  The host entry allocates the batch x npix matrix on the device and
 * RELEASES it before it returns; the context keeps per-pixel buffers and batch / 256 rows of partial sums only.
 * batch * npix * 8 bytes above 4 GiB is MCALF_ERR_RANGE (the message names the largest batch for this spectrum: thin the
 * chain), before any device work and before a row of P is read.  MCALF_ERR_INVALID, likewise before any device work, for: a
 * NULL context, batch < 0, a NULL P with batch > 0, all outputs NULL, nq outside [0, 16], nq > 0 with a NULL q or Q (or Q
 * with nq == 0), a q[j] not finite or outside [0, 1], targonly outside {0, 1}.  batch == 0 fills the requested outputs
 * with NaN and nvalid with 0.  Host pointers, synchronous.  A multi-device context runs the whole call on its first device
 * entry -- all rows have to meet on one device -- so the result is bit for bit a single-device context's. */
int mcalf_model_band_batch(mcalf_ctx* ctx, const double* P, int64_t batch, int32_t targonly, const double* q, int32_t nq,
                           double* mean, double* var, double* Q, int64_t* nvalid);
/* Same, device pointers, on the caller's stream (single-device contexts).  q is a HOST array, read during the call (its
 * values travel in the kernels' argument block: nothing of the caller's is read after the call returns).  dM is the caller's
 * [batch][npix] workspace (NULL with batch > 0: MCALF_ERR_INVALID); ON RETURN dM HOLDS THE MODEL ROWS, exactly what
 * mcalf_model_batch_device(dP, batch, targonly) writes.  After one call of the same or a larger batch and nq it allocates
 * and synchronises nothing. */
int mcalf_model_band_batch_device(mcalf_ctx* ctx, const double* dP, int64_t batch, int32_t targonly, const double* q, int32_t nq,
                                  double* dM, double* dmean, double* dvar, double* dQ, int64_t* dnvalid, void* stream);

/* The Fisher product of the Gaussian likelihood, matrix-free and on the device: FV[i, :] = J(P[i])^T W J(P[i]) V[i, :], P, V
 * and FV batch x ndim, row-major.  J is the model Jacobian of mcalf_model_jvp_batch; W = 1 / err^2 on the pixels whose logL term
 * nansum keeps (finite flux, finite non-zero error) and 0 elsewhere -- a device array of the context, built by the first call.
 * One call is one JVP pass, one per-pixel multiply dM <- W (.) dM and one VJP pass with dM as the cotangent, row block by row
 * block inside a context-owned [rows][npix] workspace (rows * npix * 8 bytes within 384 MiB, at most 65535 rows): the
 * [batch][npix] intermediate never leaves the device.  The result is bit for bit mcalf_model_vjp_batch(P, W * mcalf_model_jvp_batch(P, V)),
 * and the conventions are those entries': ignored entries of V and exact-0 columns of FV (the ncomp slot, inactive (N, z, b), R /
 * continuum the context fixes), an all-NaN row when R needs more taps than the context provisions, every reduction in a fixed
 * order, a multi-device context cutting the rows as the gradient does.  MCALF_ERR_INVALID before any device work for a NULL
 * context, batch < 0 or a NULL array with batch > 0; batch == 0 does nothing. */
int mcalf_fisher_matvec_batch(mcalf_ctx* ctx, const double* P, const double* V, int64_t batch, double* FV);
/* Same, device pointers, on the caller's stream (single-device contexts).  After one call of the same or a larger batch it
 * allocates and synchronises nothing. */
int mcalf_fisher_matvec_batch_device(mcalf_ctx* ctx, const double* dP, const double* dV, int64_t batch, double* dFV, void* stream);

/* Batched Levenberg-Marquardt maximisation of logL: every row of P0 (batch x ndim) is polished independently to a maximum of
 * logL -- exactly mcalf_loglike_batch's value -- over its continuous, active parameters inside the box of mcalf_set_prior
 * (MCALF_ERR_INVALID if none is set, if a bound is not finite or if lo > hi).  Never changed: the ncomp slot (its bits are
 * kept, a fractional 2.7 included) and the (N, z, b) of slots at or beyond the row's active count; R and the continuum move only
 * where the context floats them.  The fit works in cube coordinates, s = hi - lo, u = (theta - lo) / s; s == 0 fixes a coordinate.
 * Per row:
 *   start   the continuous, active entries of P0 are clamped into the box; logL and its gradient G there.  A start whose logL
 *           is not finite (asymmetric veto, R beyond the tap cap) or that has a NaN among those entries (nansum drops every
 *           pixel of such a row: its logL is a finite 0) has status -1 and its row is returned as given.
 *   pins    coordinate k does not move in this iteration if theta_k <= lo_k and G_k < 0, if theta_k >= hi_k and G_k > 0, or if
 *           s_k == 0.  g_u = s (.) G with the pinned entries 0; all zero: status 2.
 *   step    (A + lambda I) x = g_u by conjugate gradients from x = 0, A = s (.) J^T W J (.) s on the unpinned coordinates,
 *           cg_iters iterations, one Fisher product (above) each; a row's CG stops early when p.(A + lambda I)p <= 0 or
 *           r.r <= 1e-20 g_u.g_u.  Nothing dense is formed.
 *   trial   T = clamp(theta + s (.) x, lo, hi); accepted iff logL(T) is finite and > logL(theta): theta <- T, lambda <-
 *           max(lambda / 10, 1e-15), and status 1 if the gain is <= ftol (1 + |logL(T)|).  Rejected: lambda <- 10 lambda, status
 *           3 once lambda exceeds 1e12; theta stays.
 * status 0: max_iter outer iterations were run.  niter counts the outer iterations a row took a step in.  logL never decreases,
 * and on return logL[i] is the likelihood of P[i] bit for bit (for a status -1 row: of its clamped start).  Rows run in lock
 * step and finished rows are carried unchanged; every sum has one order (a wave per row, one fixed butterfly), so a row's bits
 * depend on its own start and the options alone -- not on its batch, its position, the row block or the device count.
 * A fit costs about (cg_iters + 1) Voigt passes per outer iteration and row. */
typedef struct {
    int32_t max_iter;        /* outer iterations, >= 0 (0: the clamped start, its logL, status 0 or -1, niter 0) */
    int32_t cg_iters;        /* CG iterations per outer iteration; 0 = ndim */
    int32_t rows_per_block;  /* 0 = rows * npix * 8 bytes within 384 MiB, at most 65535; else rows fitted together (bounds the workspace) */
    int32_t reserved;
    double lambda0;          /* initial damping, cube units, > 0 */
    double ftol;             /* >= 0 */
} mcalf_fit_opts;
/* Host pointers, synchronous: P (batch x ndim), logL, status, niter (batch each) are outputs; P0 and P must not overlap.  After
 * every outer iteration the call reads the count of live rows (4 bytes) and stops at 0.  A multi-device context cuts the rows
 * as the gradient does.  All argument checks (NULL arrays, batch < 0, negative counts, lambda0 not finite or <= 0, ftol not
 * finite or < 0, the prior box) come before any device work and name the argument.  batch == 0 does nothing. */
int mcalf_maximize_batch(mcalf_ctx* ctx, const double* P0, int64_t batch, const mcalf_fit_opts* opts, double* P, double* logL,
                         int32_t* status, int32_t* niter);
/* Same, device pointers (opts is a host struct, read during the call), on the caller's stream (single-device contexts).  It
 * runs max_iter iterations unconditionally and never synchronises; the bits are the host entry's.  After one call of the same
 * or a larger batch and block size it allocates nothing. */
int mcalf_maximize_batch_device(mcalf_ctx* ctx, const double* dP0, int64_t batch, const mcalf_fit_opts* opts, double* dP, double* dlogL,
                                int32_t* dstatus, int32_t* dniter, void* stream);

/* Nested sampling's replacement step: every row of U0 (batch x ndim, a point of the unit cube of mcalf_set_prior's box --
 * MCALF_ERR_INVALID if none is set) is a chain that makes nmoves slice-sampling moves under the hard constraint
 * logL > Lmin[row], logL being exactly mcalf_loglike_cube_batch's value.  D (ndirs x ndim, row-major) holds the direction
 * rows, shared by all rows of the call; sid[row] is the row's random stream (the caller makes them distinct).  Rows run in
 * lock step, one trial per row and step:
 *   start    logL(U0) by one cube launch.  A row whose start has an entry outside [0, 1] or a NaN, or for which
 *            logL(U0) > Lmin is false (a NaN logL makes it false; Lmin = -inf passes every finite logL and +inf), has status -1
 *            and is returned as given, with logL = logL(U0).
 *   step it = 1 .. max_steps, for a row with x its point, (w0, w1, w2, w3) = Philox4x64-10 of counter (it, 0, sid, 0) and key
 *   (seed, 0) (multipliers 0xD2E7470EE14C6C93, 0xCA5A826395121157, Weyl constants 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B --
 *   numpy's Philox(counter=[0, 0, sid, 0], key=[seed, 0]) returns exactly these blocks; w2 and w3 are reserved):
 *     decide   (from the second step on) the trial y of the step before is accepted iff logL(y) > Lmin: x <- y, logL <- logL(y),
 *              moves + 1, and the row needs a new direction; at moves == nmoves the row is finished, status 1.  Rejected:
 *              tl <- t if t < 0, else tr <- t.
 *     propose  a row that needs a direction takes d = D[w0 mod ndirs] and the chord of its line through the cube:
 *              tl = max_k min(a_k, b_k), tr = min_k max(a_k, b_k) over the k with d_k != 0, a_k = (0 - x_k) / d_k,
 *              b_k = (1 - x_k) / d_k; tl = tr = 0 if d is all zero.  Then xi = (w1 >> 11) 2^-53, t = tl + (tr - tl) xi and
 *              y_k = x_k + t d_k clamped into [0, 1] (y < 0 ? 0 : (y > 1 ? 1 : y)); nevals + 1.
 *   Every product, quotient, sum and difference above is ONE correctly rounded IEEE operation (nothing is contracted to an
 *   FMA), so a trajectory can be restated exactly on the host.  The point sits at t = 0, inside every bracket: a move always ends.
 * status 0: max_steps steps were run; the row holds its last accepted point, which satisfies the constraint.  A finished row is
 * carried unchanged (its trial row is its own point, its nevals stops).  On return logL[i] is mcalf_loglike_cube_batch(U)[i] bit
 * for bit, theta (optional, NULL: not wanted) holds the transformed rows of U as that entry forms them, nevals the trials the row
 * evaluated (its start not counted) and moves the accepted ones.  A row's results depend on its own (U0 row, Lmin, sid), on D and
 * on the options alone -- not on its batch, its position or the device count.  A step is one step kernel and one cube logL launch
 * (set-up kernel + fused kernel) over all rows, finished ones included (mcalf_set_slice_compact, below: over the rows that proposed
 * a trial). */
typedef struct {
    int32_t nmoves;          /* accepted moves per row, >= 0 (0: the checked start, status 1 or -1) */
    int32_t max_steps;       /* lock steps, >= 0 */
    int32_t ndirs;           /* rows of D, >= 1 */
    int32_t reserved;
    uint64_t seed;           /* the Philox key */
} mcalf_slice_opts;
/* Host pointers, synchronous: U, theta (batch x ndim), logL, status, nevals, moves (batch each) are outputs; U0 and U must not
 * overlap.  After every step the call reads the count of rows that proposed a trial (4 bytes) and stops at 0.  A multi-device
 * context cuts the rows into contiguous blocks as the fit does.  All argument checks (opts or an array NULL, batch < 0, nmoves < 0,
 * max_steps < 0, ndirs < 1, no prior set, a non-finite entry of D) come before any device work and name the argument.
 * batch == 0 does nothing. */
int mcalf_slice_replace_batch(mcalf_ctx* ctx, const double* U0, const double* Lmin, const double* D, const uint64_t* sid, int64_t batch,
                              const mcalf_slice_opts* opts, double* U, double* theta, double* logL, int32_t* status, int32_t* nevals,
                              int32_t* moves);
/* Same, device pointers (opts is a host struct, read during the call; the entries of dD are not checked), on the caller's stream
 * (single-device contexts).  It runs max_steps steps unconditionally and never synchronises; the bits are the host entry's.
 * After one call of the same or a larger batch it allocates nothing. */
int mcalf_slice_replace_batch_device(mcalf_ctx* ctx, const double* dU0, const double* dLmin, const double* dD, const uint64_t* dsid,
                                     int64_t batch, const mcalf_slice_opts* opts, double* dU, double* dtheta, double* dlogL,
                                     int32_t* dstatus, int32_t* dnevals, int32_t* dmoves, void* stream);

/* Packing the live rows.  0 (default): every lock step of mcalf_slice_replace_batch evaluates all rows.  1: the host entry packs
 * the rows that proposed a trial -- a pack kernel lists them in ascending row order, a gather kernel copies their trial rows
 * together -- and launches the cube logL over those only.  The launch of step `it` is sized by the count of step it - 1, which
 * the host has read by then and which bounds the count of step it (rows only ever finish); the surplus slots evaluate the trial
 * row of row 0 and are never read.  So the host waits for the 4-byte count of a step, not for the step's logL launch, and a call
 * launches at most 2 batch + sum(nevals) rows instead of batch (1 + steps).  Results never depend on the setting, bit for bit:
 * logL does not depend on a row's position or batch, and the random words are keyed by (step, stream id, seed).  Applies to every
 * entry of a multi-device context.  The environment variable MCALF_NS_COMPACT (0 / 1) gives a context's initial value;
 * mcalf_get_config prints "ns_compact=%d".  The *_device entry ignores it: it never synchronises, so it cannot size a launch by a
 * device-side count.  ctx NULL or on outside {0, 1}: MCALF_ERR_INVALID. */
int mcalf_set_slice_compact(mcalf_ctx* ctx, int32_t on);

/* What the last mcalf_slice_replace_batch[_device] call of this context launched.  A multi-device context reports the sum over
 * the entries the call was cut over for batch, rows_launched and trials, and the largest steps among them.  The device entry
 * reports rows_launched = (max_steps + 1) batch (batch when nmoves == 0), trials = -1, steps = max_steps (0 when nmoves == 0) and
 * compact = 0.  Before any slice call, and after one of batch 0, everything is 0.  ctx or out NULL: MCALF_ERR_INVALID. */
typedef struct {
    int64_t batch;          /* rows of the last slice call of this context */
    int64_t rows_launched;  /* rows handed to cube logL launches by that call, the start launch included */
    int64_t trials;         /* trials its rows proposed (= sum of nevals); -1 for the device entry (unknown to the host) */
    int32_t steps;          /* lock steps whose logL launch was issued */
    int32_t compact;        /* 1: the call packed its trial rows */
} mcalf_slice_stats_t;      /* 32 bytes */
int mcalf_slice_last_stats(const mcalf_ctx* ctx, mcalf_slice_stats_t* out);

/* The ensemble sampler: n = nwalkers walkers in the unit cube of mcalf_set_prior's box (MCALF_ERR_INVALID if none is set), cut
 * into the halves [0, m) and [m, n), m = n / 2 (n even, >= 4).  logL is exactly mcalf_loglike_cube_batch's value.  One iteration
 * is two half-steps h = 0, 1; in half-step h the walkers of half h move, with partners from the other half as it stands then.
 *   start    logL(U0) by one cube launch over all n rows.  A walker whose start has an entry outside [0, 1] or a NaN has
 *            status -1 and never moves: its row is returned as given (others may still draw it as a partner; such proposals are
 *            decided by the rules below).  Every other walker has status 0.
 *   words    for moving walker w (its index among the n) and global half-step s = 2 (first_iter + i) + h, i the iteration within
 *            the call: (w0, w1, w2, w3) = the block numpy's Philox(counter=[s, 0, w, 0], key=[seed, 1]) returns first, with the
 *            constants of the slice step above.  That generator advances its counter before it draws (the slice step's block of
 *            step 1 is the first of counter 0 in the same way), so it is the Philox4x64-10 function at counter (s + 1, 0, w, 0).
 *            xi = (w1 >> 11) 2^-53;  zeta = ((w2 >> 11) + 1) 2^-53, in (0, 1].
 *   stretch  (MCALF_ENS_STRETCH, scale = a > 1)  j = the other half's first index + w0 mod m;  t = (a - 1) xi + 1,  z = t t / a;
 *            y_k = x_j,k + z (x_k - x_j,k);  q = (ndim - 1) ln z + (logL(y) - logL(x)).
 *   DE       (MCALF_ENS_DE, scale = g > 0)  j1 = w0 mod m, j2 = (j1 + 1 + w3 mod (m - 1)) mod m, both in the other half;
 *            gamma = g (1 + 1e-5 (2 xi - 1));  y_k = x_k + gamma (x_j1,k - x_j2,k);  q = logL(y) - logL(x)  (a symmetric move).
 *   decide   y is inside iff every 0 <= y_k <= 1 (a NaN fails).  A walker whose y is not inside puts its own point in its trial
 *            row and is rejected whatever the launch returns.  Otherwise it is accepted iff ln zeta < q (any NaN: false):
 *            x <- y, logL <- logL(y), naccept + 1.
 *   ln       for normal positive x = f 2^e, f in [1, 2) from the bits:  if f > 0x1.6a09e667f3bcdp+0: f <- 0.5 f, e <- e + 1;
 *            r = (f - 1) / (f + 1);  s = r r;  p = 1/19, then p <- p s + 1 / (2 i + 1) for i = 8 .. 1;  t = r + r;
 *            lnf = t + (t s) p;  ln x = e 0x1.62e42feep-1 + (lnf + e 0x1.a39ef35793c76p-33).  Within 1e-13 of the true
 *            logarithm, relatively (measured: DESIGN 3.13); zeta >= 2^-53 and z in [1 / a, a] are normal.
 *   chain    after every iteration i with (i + 1) mod thin == 0 the device copies the state into slot (i + 1) / thin - 1 of
 *            CU [nkeep][n][ndim] and CL [nkeep][n], nkeep = nsteps / thin: a run of any length reaches the host once.
 * Every product, quotient, sum and difference above is ONE correctly rounded IEEE operation (nothing is contracted to an FMA)
 * and there are no floating-point atomics, so a run can be restated exactly on the host; a walker's results depend on (U0, opts)
 * alone.  Taking the last U as U0 with first_iter advanced by nsteps is, bit for bit, the longer call.  A half-step is a propose
 * kernel over the m moving walkers, one cube logL launch over their m trial rows and a decide kernel (which also fills the
 * chain slot).  theta (optional) holds the transformed rows of U as the cube launch forms them. */
enum { MCALF_ENS_STRETCH = 0, MCALF_ENS_DE = 1 };
typedef struct {
    int32_t nsteps;          /* iterations, >= 0 (0: the checked start and its logL) */
    int32_t thin;            /* every thin-th iteration goes into the chain, >= 1 */
    int32_t move;            /* MCALF_ENS_STRETCH or MCALF_ENS_DE */
    int32_t reserved;
    double scale;            /* a > 1 of the stretch move, g > 0 of the DE move; finite */
    uint64_t seed;           /* the Philox key word 0 */
    uint64_t first_iter;     /* the iteration number of the call's first iteration (continuation) */
} mcalf_ens_opts;            /* 40 bytes */
/* Host pointers, synchronous: U, theta (n x ndim; theta NULL: not wanted), logL, status, naccept (n each) and the chain CU, CL
 * (each NULL: not wanted) are outputs; U0 and U must not overlap.  A multi-device context runs the whole call on its first device
 * entry (the walkers have to meet on one device): bit for bit a single-device context's result.  All argument checks (ctx, opts
 * or a required array NULL; nwalkers negative, odd, or below 4 when non-zero; nsteps < 0; thin < 1; move outside {0, 1}; scale not
 * finite, <= 1 for the stretch move, <= 0 for the DE move; no prior set) come before any device work and name the argument.
 * A chain above 4 GiB on the device is MCALF_ERR_RANGE (the message names the largest nkeep).  nwalkers == 0 does nothing. */
int mcalf_ensemble_batch(mcalf_ctx* ctx, const double* U0, int64_t nwalkers, const mcalf_ens_opts* opts, double* U, double* theta,
                         double* logL, int32_t* status, int32_t* naccept, double* CU, double* CL);
/* Same, device pointers (opts is a host struct, read during the call), on the caller's stream (single-device contexts).  It never
 * synchronises; the bits are the host entry's.  After one call of the same or a larger size it allocates nothing. */
int mcalf_ensemble_batch_device(mcalf_ctx* ctx, const double* dU0, int64_t nwalkers, const mcalf_ens_opts* opts, double* dU,
                                double* dtheta, double* dlogL, int32_t* dstatus, int32_t* dnaccept, double* dCU, double* dCL,
                                void* stream);

/* Parallel tempering of the ensemble sampler: T = ntemps temperatures (1 <= T <= MCALF_PT_MAX_TEMPS) of n = nwalkers walkers
 * each, temperature t sampling logL^beta[t].  `beta` is a HOST array of T doubles in both entries, read during the call as opts
 * is: every beta finite and >= 0, strictly decreasing in t (beta[0] = 1 is the posterior, beta[T - 1] = 0 the prior).  The state
 * is U [T][n][ndim] and logL [T][n]; row t n + w of every array is walker w of temperature t, and the logL stored is always the
 * UNTEMPERED value of mcalf_loglike_cube_batch.  Every temperature is cut into the halves [0, m) and [m, n), m = n / 2.
 *   start    logL(U0) by one cube launch over all T n rows.  A position (t, w) whose start has an entry outside [0, 1] or a NaN
 *            has status -1: it never moves and never swaps (others may draw it as a partner, of a move or of a swap).
 *   half-step  the ensemble sampler's, for every temperature at once: the partners of walker (t, w) come from the other half
 *            of temperature t; its words are the block numpy's Philox(counter=[s, 0, t n + w, 0], key=[seed, 1]) returns first,
 *            s = 2 (first_iter + i) + h (at T = 1 the ensemble sampler's words); xi, zeta and the proposals of both moves are
 *            as above.  y not inside: rejected, as above.  Otherwise d = logL(y) - logL(x);  q = hastings + beta[t] d with
 *            hastings = (ndim - 1) ln z for the stretch move, and q = beta[t] d for the DE move;  accepted iff ln zeta < q
 *            (any NaN: false -- a trial of -inf is rejected at every beta, beta = 0 included, where 0 (-inf) is NaN).
 *            beta[t] d is one rounded product; at beta = 1 it is d.  One propose kernel over T m blocks, one cube logL launch
 *            over the T m trial rows, one decide kernel.
 *   swaps    g = first_iter + i is the global iteration.  After the second half-step of every iteration with
 *            (g + 1) mod swap_every == 0 (swap_every 0: never) and before the chain slot is filled, swap round
 *            r = (g + 1) / swap_every - 1 is made: the pairs of temperatures (t, t + 1) for every t = r mod 2, r mod 2 + 2, ...
 *            with t + 1 < T (disjoint).  Pair t has the shift c = w0 mod n, w0 from the block numpy's
 *            Philox(counter=[r, 1, t, 0], key=[seed, 2]) returns first (the function at counter (r + 1, 1, t, 0)); position
 *            (t, w) meets position (t + 1, j), j = (w + c) mod n -- a bijection, so every row is in at most one exchange of the
 *            round.  zeta = ((w2 >> 11) + 1) 2^-53 from the block of Philox(counter=[r, 0, t n + w, 0], key=[seed, 2]);
 *            q = (beta[t] - beta[t + 1]) (logL[t + 1][j] - logL[t][w])  (a difference, a difference, a product);
 *            the two are exchanged iff both positions have status 0 and ln zeta < q (any NaN: false): the two U rows in all
 *            ndim coordinates and the two logL values change places, nswap[t][w] + 1.  status, naccept and nswap belong to
 *            positions, not to states.  nswap [T - 1][n] counts the accepted swaps of position (t, w) with temperature t + 1
 *            (T = 1: not touched, may be NULL).
 *   chain    after every iteration i (call-local) with (i + 1) mod thin == 0 the state after that iteration's swaps goes into
 *            slot (i + 1) / thin - 1 of CL [nkeep][T][n] (all temperatures: the evidence needs them) and of
 *            CU [nkeep][chain_temps][n][ndim] (the first chain_temps temperatures, 0 <= chain_temps <= T).
 * The arithmetic rules, ln and the 4 GiB cap on the chain are the ensemble sampler's.  A position's results depend on (U0, beta,
 * opts) alone; taking the last U as U0 with first_iter advanced by nsteps is, bit for bit, the longer call (the swap rounds are
 * keyed to g).  With ntemps = 1 and beta = {1} the results are mcalf_ensemble_batch's bit for bit. */
enum { MCALF_PT_MAX_TEMPS = 64 };
typedef struct {
    int32_t nsteps;          /* iterations, >= 0 (0: the checked start and its logL) */
    int32_t thin;            /* every thin-th iteration goes into the chain, >= 1 */
    int32_t move;            /* MCALF_ENS_STRETCH or MCALF_ENS_DE */
    int32_t ntemps;          /* T, 1 .. MCALF_PT_MAX_TEMPS */
    int32_t swap_every;      /* a swap round after every swap_every-th global iteration, >= 0 (0: never) */
    int32_t chain_temps;     /* temperatures whose rows CU keeps, 0 .. T */
    double scale;            /* a > 1 of the stretch move, g > 0 of the DE move; finite */
    uint64_t seed;           /* the Philox key word 0 */
    uint64_t first_iter;     /* the global iteration number of the call's first iteration (continuation) */
} mcalf_pt_opts;             /* 48 bytes */
/* Host pointers, synchronous: U, theta (T n x ndim; theta NULL: not wanted), logL, status, naccept (T n each), nswap
 * ((T - 1) n) and the chain CU, CL (each NULL: not wanted) are outputs; U0 and U must not overlap.  A multi-device context runs
 * the whole call on its first device entry: bit for bit a single-device context's result.  All argument checks come before any
 * device work and name the argument: mcalf_ensemble_batch's, and beta NULL; ntemps outside [1, 64]; a beta that is not finite, is
 * negative or is not below its predecessor; swap_every < 0; chain_temps outside [0, T]; nswap NULL with T > 1; ntemps x nwalkers
 * above 0x7fff0000 rows (MCALF_ERR_RANGE).  nwalkers == 0 does nothing. */
int mcalf_tempered_batch(mcalf_ctx* ctx, const double* U0, int64_t nwalkers, const double* beta, const mcalf_pt_opts* opts, double* U,
                         double* theta, double* logL, int32_t* status, int32_t* naccept, int32_t* nswap, double* CU, double* CL);
/* Same, device pointers (beta and opts are host arrays, read during the call: beta travels in the kernels' argument block), on
 * the caller's stream (single-device contexts).  It never synchronises; the bits are the host entry's.  After one call of the
 * same or a larger size it allocates nothing. */
int mcalf_tempered_batch_device(mcalf_ctx* ctx, const double* dU0, int64_t nwalkers, const double* beta, const mcalf_pt_opts* opts,
                                double* dU, double* dtheta, double* dlogL, int32_t* dstatus, int32_t* dnaccept, int32_t* dnswap,
                                double* dCU, double* dCL, void* stream);

/* Hamiltonian Monte Carlo: n = nwalkers INDEPENDENT walkers in the unit cube of mcalf_set_prior's box (MCALF_ERR_INVALID if none
 * is set), each making nsteps iterations of one trajectory of nleap leapfrog steps, in lock step, with a diagonal mass.  The
 * target is the other samplers': logL, plus lnprior under mcalf_set_gauss_prior; logL is exactly mcalf_loglike_cube_batch's value
 * and its gradient is mcalf_loglike_grad_batch_device's row.  `scale` [ndim] and `wid` [n] are HOST arrays in both entries, read
 * during the call as opts is: scale[k] >= 0 is the length of coordinate k in cube units (its inverse square is the mass),
 * wid[w] the id that keys walker w's random words (NULL: 0 .. n - 1; the ids must be distinct, as the slice step's sid).
 *   frozen   coordinate k is frozen if it is the ncomp slot (startind of mcalf_info, whatever the int_ncomp flavour), if
 *            hi_k == lo_k or if scale[k] == 0.  Its momentum is exactly 0, it never moves and does not enter the kinetic
 *            energy.  So a walker keeps its component count -- different walkers may hold different counts -- and moves that
 *            change the count belong to the ensemble and the nested samplers.
 *   gradient with s_k = hi_k - lo_k and theta = u s + lo (the two operations of the cube transform; the ncomp slot truncated as
 *            there), G the gradient launch's row at theta:  g_k = s_k G_k;  under a Gaussian prior, for every k with
 *            sigma_k > 0:  d = (theta_k - mu_k) / sigma_k;  t = d / sigma_k;  g_k <- g_k - t s_k  (a product, then a
 *            difference).  pr = lnprior of the row as mcalf_lnprior_batch gives it, or an exact 0 without a Gaussian.
 *   start    one gradient launch over all n rows of theta(U0).  A walker whose start has an entry outside [0, 1] or a NaN,
 *            whose logL is not finite or whose g has a non-finite unfrozen entry has status -1: it never moves and comes back
 *            as given.  Every other walker has status 0.
 *   words    g = first_iter + i is the global iteration, w the walker's id, the key (seed, 4); a block is the Philox4x64-10
 *            function with the constants of the slice step above.  The decision block is the one at counter (g + 1, 2^63, w, 0):
 *            xi = (w1 >> 11) 2^-53;  zeta = ((w2 >> 11) + 1) 2^-53.  The momentum of unfrozen coordinate k is a standard normal
 *            by Marsaglia's polar method from the blocks at (g + 1, (a << 32) | k, w, 0), attempts a = 0, 1, ..., 15: with
 *            x(word) = (word >> 11) 2^-53 the candidate pairs of a block are (v1, v2) = (2 x(w0) - 1, 2 x(w1) - 1), then
 *            (2 x(w2) - 1, 2 x(w3) - 1);  q = v1 v1 + v2 v2;  the first candidate with 0 < q < 1 gives
 *            r_k = v1 sqrt((-2 ln q) / q), ln the ensemble sampler's above.  If all 32 candidates fail (probability 4e-22)
 *            r_k = 0.
 *   trajectory  eps' = eps (1 + jitter (2 xi - 1));  a_k = eps' scale[k];  h_k = 0.5 a_k;  K0 = 0.5 sum r_k r_k;  y = x,
 *            gy = g(x).  Each of the nleap steps:  r_k <- r_k + h_k gy_k;  y_k <- y_k + a_k r_k;  ONE reflection -- if
 *            y_k < 0: y_k <- -y_k, r_k <- -r_k; else if y_k > 1: y_k <- 2 - y_k, r_k <- -r_k;  the gradient launch at
 *            theta(y);  r_k <- r_k + h_k gy_k with the new gy.  (Two neighbouring half kicks are two additions.)
 *   dead     a trajectory is dead from the step where a reflected y_k is still outside [0, 1] or is a NaN, where the launch's
 *            logL is not finite, or where an unfrozen gy_k is not finite.  A dead trajectory puts the walker's own x into its
 *            row for every later launch, is rejected, and adds one to ndead[w].
 *   decide   K1 = 0.5 sum r_k r_k;  q = ((L(y) + pr(y)) - (L(x) + pr(x))) + (K0 - K1).  Accepted iff the trajectory is not
 *            dead and ln zeta < q (any NaN: false):  x <- y, logL <- L(y), g <- gy, naccept + 1.  g is kept across iterations:
 *            an iteration costs exactly nleap gradient launches.
 *   chain    the ensemble sampler's: after every iteration i with (i + 1) mod thin == 0 the state goes into slot
 *            (i + 1) / thin - 1 of CU [nkeep][n][ndim] and CL [nkeep][n], nkeep = nsteps / thin.
 * Every product, quotient, sum, difference and square root above is ONE correctly rounded IEEE operation (nothing is contracted
 * to an FMA) and there are no floating-point atomics.  A sum over coordinates is taken as the prior's: a lane adds its
 * coordinates k, k + 64, ... in index order onto +0.0, then the xor-butterfly 32 .. 1 folds the 64 lanes.  So a run is restated
 * exactly on the host, given the device's own gradient.  A walker's results depend on its start row, its id, opts and scale
 * alone -- not on the batch, its position in it or the stream -- and taking the last U as U0 with first_iter advanced by nsteps
 * is, bit for bit, the longer call.  A leapfrog step is one kernel of the sampler's and one gradient launch over the n rows;
 * nothing is read back during a call.  theta (optional) holds the transformed rows of U as the cube launch forms them. */
typedef struct {
    int32_t nsteps;          /* iterations, >= 0 (0: the checked start, its logL and status) */
    int32_t thin;            /* every thin-th iteration goes into the chain, >= 1 */
    int32_t nleap;           /* leapfrog steps of a trajectory, >= 1 */
    int32_t reserved;
    double eps;              /* the step size, finite and > 0 */
    double jitter;           /* its relative jitter per walker and iteration, in [0, 1) */
    uint64_t seed;           /* the Philox key word 0 */
    uint64_t first_iter;     /* the iteration number of the call's first iteration (continuation) */
} mcalf_hmc_opts;            /* 48 bytes */
/* Host pointers, synchronous: U, theta (n x ndim; theta NULL: not wanted), logL, status, naccept, ndead (n each) and the chain CU,
 * CL (each NULL: not wanted) are outputs; U0 and U must not overlap.  A multi-device context runs the whole call on its first
 * device entry, bit for bit a single-device context's result: cutting independent walkers over devices needs a strided copy of
 * the chain and is left out -- a caller can split the walkers over contexts by wid and gets the same bits.  All argument checks
 * (ctx, opts or a required array NULL; nwalkers < 0; nsteps < 0; thin < 1; nleap < 1; eps not finite or <= 0; jitter outside
 * [0, 1); a scale entry negative or not finite; no prior set) come before any device work and name the argument.  A chain above
 * 4 GiB on the device is MCALF_ERR_RANGE (the ensemble sampler's message).  nwalkers == 0 does nothing. */
int mcalf_hmc_batch(mcalf_ctx* ctx, const double* U0, int64_t nwalkers, const double* scale, const uint64_t* wid, const mcalf_hmc_opts* opts,
                    double* U, double* theta, double* logL, int32_t* status, int32_t* naccept, int32_t* ndead, double* CU, double* CL);
/* Same, device pointers (scale, wid and opts stay host arrays: they travel in kernel argument blocks), on the caller's stream
 * (single-device contexts).  It never synchronises; the bits are the host entry's.  After one call of the same or a larger size
 * it allocates nothing. */
int mcalf_hmc_batch_device(mcalf_ctx* ctx, const double* dU0, int64_t nwalkers, const double* scale, const uint64_t* wid,
                           const mcalf_hmc_opts* opts, double* dU, double* dtheta, double* dlogL, int32_t* dstatus, int32_t* dnaccept,
                           int32_t* dndead, double* dCU, double* dCL, void* stream);

/* Chain diagnostics: per coordinate k of a chain X [T][n][d] (T = nkeep kept steps, n = nwalkers, d = ndim, the chain's OWN width:
 * any d >= 1, not tied to the context's -- a chain of theta rows or of derived quantities is as good as one of cube rows; row
 * (t, w, .) is d contiguous doubles, as CU of the samplers) the pooled mean and variance, the walker-averaged integrated
 * autocorrelation time with Sokal's window, the same of the ensemble-mean series, split R-hat and the effective sample size.
 * A walker w with status[w] != 0 is left out of everything (status NULL: all are used); nok is the number of walkers used.
 * With x_t = X[t][w][k], sums over t taken t ascending from +0.0:
 *   per walker  S_w = sum_t x_t;  delta_w = (sum_t (x_t - x_0)) / T;  h = T / 2 (integer);  m_w1 = (sum_{t < h} x_t) / h,  m_w2 = (sum_{t >= T - h} x_t) / h
 *            (for odd T the middle state is in neither half).  A series with x_t == x_0 for every t is CONSTANT: its m_w1 and
 *            m_w2 are x_0 by definition, not the rounded sums' (T copies of 0.3 do not add up to 0.3 T), and its centred values
 *            are 0, so that its c_w(0) below is 0 exactly.  The centred value of any other series is
 *            xc_t = (x_t - x_0) - delta_w, both differences rounded: x_t - x_0 is exact for values within a factor of two of
 *            each other, so a walker that has hardly moved keeps its digits (x_t - S_w / T would lose those of x_0 / |xc_t|).
 *            Then, in a second pass,
 *            c_w(0) = sum_t xc_t^2 by one fma per step;  q_w = sum_t (x_t - mean)^2;
 *            s2_w1 = (sum_{t < h} (x_t - m_w1)^2) / (h - 1),  s2_w2 likewise over the last h states.
 *   walker sums  a sum over walkers is taken in ONE fixed order: lane l of 64 adds the used walkers l, l + 64, ... in that order
 *            from +0.0, then the xor-butterfly 32 .. 1 folds the 64 lanes, as the prior's sums are folded.
 *   mean, var  mean = (sum_w S_w) / (T nok);  var = (sum_w q_w) / (T nok - 1): pooled over the T nok values, two-pass, ddof 1
 *            (NaN when nok = 0).  Where every used walker is constant at ONE value v (a frozen coordinate) mean and mbar below are
 *            v: var is 0 and W is 0, exactly.
 *   rhat     split R-hat over the 2 nok half chains:  mbar = (sum_w (m_w1 + m_w2)) / (2 nok);  W = (sum_w (s2_w1 + s2_w2)) / (2 nok);
 *            B = h (sum_w ((m_w1 - mbar)^2 + (m_w2 - mbar)^2)) / (2 nok - 1);  rhat = sqrt(((h - 1) / h W + B / h) / W), NaN where W == 0.
 *   ACF      L = max_lag, or T - 1 when max_lag == 0.  c_w(tau) = sum_{t = 0}^{T - 1 - tau} xc_t xc_{t + tau} for
 *            tau = 0 .. L, t ascending, one fma per step (the biased sum the zero-padded FFT route gives; at tau = 0 it is
 *            c_w(0) above bit for bit).  rho_w(tau) = c_w(tau) / c_w(0).  A walker with c_w(0) == 0 is constant in this
 *            coordinate (it is stuck, or the coordinate is frozen) and is left out; nused is the number that remain.  The used
 *            walkers are cut into blocks of 64 consecutive walker indices; a block adds its rho_w(tau) w ascending from +0.0,
 *            the blocks are added in block order from +0.0, and rho(tau) = that sum / nused.  rho(0) = 1.
 *   tau, M   tau(m) = 2 (sum_{t <= m} rho(t)) - 1, the sum running from +0.0;  M = the smallest m in [0, L] with m >= c tau(m),
 *            tau = tau(M), flag bit 0 set ("window reached").  If there is none: M = L, tau = tau(L), bit 0 clear.  nused == 0
 *            makes rho, and so tau, NaN.  tau is in kept steps.
 *   tau_mean, M_mean, flag bit 1   the same rule, the same sums, on the ONE series m_t = (sum_w x_t,w) / nok (w ascending over the
 *            used walkers) as a chain of one walker, constancy decided in the same way: NaN when that series has no variance.
 *   ess      nok T / tau.
 * A NaN anywhere in coordinate k of a used walker makes every floating-point output of coordinate k NaN (its M and M_mean are L,
 * its flags clear; c_w(0) = NaN is not 0, so the walker counts in nused) and touches no other coordinate.
 * stats [d][6] = mean, var, tau, tau_mean, rhat, ess;  info [d][4] = M, M_mean, nused, flags;  acf [d][L + 1] = rho (NULL: not
 * wanted).  There are no floating-point atomics and every sum has one order: the bits of every output depend on (X, status,
 * opts) alone, not on the device's CU count, the stream or the entry.  The walker blocks' partial sums live in a workspace of
 * the context of ceil(n / 64) d (L + 1) doubles; above 1 GiB the call is refused with MCALF_ERR_RANGE and the message names the
 * largest max_lag that fits. */
typedef struct {
    double c;                /* Sokal's window constant, finite and > 0 */
    int64_t max_lag;         /* 0: L = nkeep - 1; else L = max_lag in [1, nkeep - 1] */
} mcalf_chain_opts;          /* 16 bytes */
/* Host pointers, synchronous.  A multi-device context runs the call on its first device entry.  All argument checks (X, opts,
 * stats or info NULL; nkeep < 4 -- split R-hat needs halves of at least 2; nwalkers < 1; ndim < 1; c not finite or <= 0; max_lag
 * outside {0} and [1, nkeep - 1]; sizes that overflow) come before any device work and name the argument, ctx NULL last. */
int mcalf_chain_stats(mcalf_ctx* ctx, const double* X, int64_t nkeep, int64_t nwalkers, int32_t ndim, const int32_t* status,
                      const mcalf_chain_opts* opts, double* stats, int32_t* info, double* acf);
/* Same, device pointers (opts is a host struct), on the caller's stream (single-device contexts).  It never synchronises; the
 * bits are the host entry's.  After one call of the same or a larger size it allocates nothing. */
int mcalf_chain_stats_device(mcalf_ctx* ctx, const double* dX, int64_t nkeep, int64_t nwalkers, int32_t ndim, const int32_t* dstatus,
                             const mcalf_chain_opts* opts, double* dstats, int32_t* dinfo, double* dacf, void* stream);

/* The ensemble sampler run until its chain has converged, or for opts->nsteps iterations at the most.  U0, opts and the outputs
 * U .. CL are mcalf_ensemble_batch's, CU and CL sized for nkeep = nsteps / thin slots; CU is required here (the statistics are
 * its), nwalkers >= 4.  The run is a sequence of ensemble calls ("blocks") of check_every thin iterations each (a shorter last
 * one if nsteps is not a multiple; the nsteps mod thin iterations behind the last kept step are not made), each continuing the one before through first_iter and writing the next slots of the ONE
 * device chain.  A block starts as every ensemble call does -- the start kernel and one likelihood launch over all nwalkers rows
 * -- and the walkers it starts from are a device copy of the last block's: one likelihood evaluation per walker and block on top
 * of the plain run's 2 x check_every x thin half-launches.  After each block, with T kept steps so far and T >= 4, a CHECK takes the statistics above of the chain prefix
 * CU [0, T) with c = conv->c, status = the walkers' and L = min(T - 1, ceil(c T / factor) + 1) -- no converged verdict can need
 * a longer lag: M ~ c tau <= c T / factor.  A coordinate is live when its nused > 0 (frozen coordinates are skipped).  The run
 * stops at the first check j >= 2 (counted from 1) at which every live coordinate has its window reached (flag bit 0),
 * T >= factor tau and |tau - tau of check j - 1| <= rtol tau; a NaN tau on a live coordinate never converges.
 *   nkept      T at the stop, or nsteps / thin if the run never stopped; converged 0 or 1; nchecks the checks made
 *   tau_hist   [nchecks][ndim] the tau of every check (kept steps); capacity ceil((nsteps / thin) / check_every) rows
 *   stats, info  [ndim][6], [ndim][4]: those of the last check (zero if there was none)
 * Because a continued ensemble call is the longer call bit for bit and blocks end on kept steps, U, theta, logL, status, naccept
 * and the first nkept slots of CU and CL are, bit for bit, those of mcalf_ensemble_batch with nsteps = nkept thin (naccept is the
 * sum of the blocks'); slots past nkept are not written.  Argument checks: conv, nkept, converged, nchecks, tau_hist, stats, info
 * or CU NULL; check_every < 1; factor, rtol or c not finite, factor or c <= 0, rtol < 0; then mcalf_ensemble_batch's, the 4 GiB
 * limit on the chain included; all before any device work, ctx NULL among the last. */
typedef struct {
    int32_t check_every;     /* kept steps between checks, >= 1 */
    int32_t reserved;
    double factor;           /* the run is long enough at T >= factor tau; finite and > 0 */
    double rtol;             /* tau has settled at |tau - tau_previous| <= rtol tau; finite and >= 0 */
    double c;                /* Sokal's window constant, finite and > 0 */
} mcalf_converge_opts;       /* 32 bytes */
/* Host pointers, synchronous.  A multi-device context runs the whole call on its first device entry. */
int mcalf_ensemble_converge(mcalf_ctx* ctx, const double* U0, int64_t nwalkers, const mcalf_ens_opts* opts, const mcalf_converge_opts* conv,
                            double* U, double* theta, double* logL, int32_t* status, int32_t* naccept, double* CU, double* CL,
                            int64_t* nkept, int32_t* converged, int32_t* nchecks, double* tau_hist, double* stats, int32_t* info);
/* Same with dU0, dU .. dCL, dstats and dinfo device pointers, on the caller's stream (single-device contexts); nkept, converged,
 * nchecks and tau_hist stay HOST outputs.  After every check it copies the ndim values of tau and the flags to the host and
 * waits for the stream: it is the one entry of the sampler family that synchronises.  The bits are the host entry's. */
int mcalf_ensemble_converge_device(mcalf_ctx* ctx, const double* dU0, int64_t nwalkers, const mcalf_ens_opts* opts,
                                   const mcalf_converge_opts* conv, double* dU, double* dtheta, double* dlogL, int32_t* dstatus,
                                   int32_t* dnaccept, double* dCU, double* dCL, int64_t* nkept, int32_t* converged, int32_t* nchecks,
                                   double* tau_hist, double* dstats, int32_t* dinfo, void* stream);

/* A device-resident nested-sampling run: the live set UL [nlive][ndim] / LL [nlive] and the dead rows UD [max_dead][ndim] /
 * LD [max_dead] stay on the device from mcalf_nested_open to mcalf_nested_close; a round transfers no rows, only one record of
 * K + 8 words.  key(L) = L with NaN as -inf.  With K = batch, round r (r = 0, 1, ... over the whole run) is
 *   rank     rank[i] = #{ j : key_j < key_i, or key_j == key_i and j < i }, compared as doubles (-0.0 == 0.0; ties keep index
 *            order: numpy's stable argsort); order[rank[i]] = i.
 *   select   dying = order[0, K) in that order; lmin = key[order[K - 1]]; r0 = rows with key <= lmin; nstarts = nlive - r0.
 *            nstarts == 0 is a plateau: the run stops before anything dies.  Chain j starts from
 *            pick_j = order[r0 + w0 mod nstarts], w0 the first word of the Philox4x64-10 block at counter (r + 1, 0, j, 0) and
 *            key (seed, 3) -- numpy's Philox(counter=[r, 0, j, 0], key=[seed, 3]) returns it first.  (Key word 1: 0 the slice
 *            step, 1 the ensemble moves, 2 the tempering swaps, 3 these picks.)  Its stream id is r K + j.
 *   moments  mean and covariance (divisor n - 1) of the cube rows of the n = nlive - K survivors order[K, nlive), those equal to
 *            lmin included, in two passes.  The survivors are cut into 128 contiguous chunks of ceil(n / 128) rows; a chunk's sum
 *            runs over its rows in order, the chunk sums are added in chunk order.  One survivor: a zero covariance.
 *   Cholesky of the covariance with 1e-9 max(mean of the variances, 1e-300) added to the diagonal; D = (factor)^T, ndim direction
 *            rows [ndim][ndim], upper triangular.  A non-finite entry of the covariance or a pivot that is not positive:
 *            D = diag(std), 1 where the variance is not finite and positive.
 *   replace  mcalf_slice_replace_batch's step (above) over the K device rows U0_j = UL[pick_j], Lmin_j = lmin, sid_j, with
 *            ndirs = ndim, as the host entry runs it: it reads the 4-byte count after every step, and honours
 *            mcalf_set_slice_compact and a Gaussian prior (the constrained quantity and every L here are then logL + lnprior).
 *   retire   replacements with status < 0 or not (L > lmin) are counted.  At zero the dying rows (U, L) go to the dead slots
 *            ndead + 0 .. K - 1 in death order and the replacements into the live rows they leave.  Otherwise the call ends with
 *            MCALF_ERR_INVALID naming the first such row, the live and the dead set as they were before the round.
 * Integer results only in rank and select, no floating-point atomics anywhere: a round's bits depend on the live set, r and the
 * options alone -- not on how the rounds are cut into calls, on the packing or on the device count.  The evidence is nested.py's:
 * point j of a round dies at live count nlive - j, ln X dropping by 1 / (nlive - j), ln w = ln X + ln(-expm1(-1 / n)) + key; after
 * the last round the remaining live points die in key order at counts nlive .. 1; ln Z is one left fold of logaddexp over all
 * weights, H = sum p (key - ln Z), logZ_err = sqrt(max(H, 0) / nlive).  nlive <= 262144 (the rank is counted: nlive^2 comparisons
 * a round) and ndim <= 256, MCALF_ERR_RANGE otherwise.  A multi-device context runs the whole run on its first device entry: bit
 * for bit a single-device context's.  A context holds one run at a time. */
typedef struct {
    int32_t batch;           /* K: rows replaced per round, 1 <= K < nlive */
    int32_t nmoves;          /* slice moves per replacement chain, >= 0 */
    int32_t max_steps;       /* lock steps of a round's replacement call, >= 0 */
    int32_t reserved;
    uint64_t seed;           /* the Philox key word 0 of the picks and of the slice step */
    double dlogz;            /* the stop test's tolerance, >= 0 (0: never stops) */
    int64_t max_dead;        /* dead rows the device keeps, >= nlive + K (rounds K + nlive are needed for a run of `rounds`) */
} mcalf_nested_opts;         /* 40 bytes */
enum { MCALF_NESTED_BUDGET = 0, MCALF_NESTED_CONVERGED = 1, MCALF_NESTED_PLATEAU = 2, MCALF_NESTED_FULL = 3 };
typedef struct {
    int64_t nlive, ndead;    /* live rows; dead rows so far */
    int64_t rounds;          /* rounds completed over the whole run */
    int64_t nevals;          /* likelihood evaluations: the initial points and every trial of every chain */
    int64_t unfinished;      /* replacements that came back with status 0 (kept: they satisfy their constraint) */
    int64_t rows_launched;   /* rows handed to likelihood launches, the initial nlive included */
    double logX, logZ;       /* ln X and the running ln Z (it steers the stop; mcalf_nested_finish makes the final one) */
    double max_key;          /* the largest live key */
    int32_t reason;          /* why the last mcalf_nested_advance returned: MCALF_NESTED_* */
    int32_t reserved;
} mcalf_nested_state_t;      /* 80 bytes */
/* Opens a run from the host rows U0 [nlive][ndim] of the unit cube: allocates the state (buffers a context already holds from an
 * earlier run of the same or a larger size are reused: nothing is allocated then) and evaluates the initial points by one
 * replacement call with Lmin = -inf and nmoves = 0 -- logL (+ lnprior under a Gaussian prior).  A row that call refuses (a NaN or
 * an entry outside the cube: no prior mass) takes logL = -inf unless its logL is NaN; with the rows of NaN or -inf logL it sorts
 * first and carries no weight.  Refused before any device work, naming the
 * argument (MCALF_ERR_INVALID): ctx, U0 or opts NULL; no prior set; batch outside [1, nlive); nmoves < 0; max_steps < 0; dlogz
 * negative or NaN; max_dead < nlive + batch; a run already open.  MCALF_ERR_RANGE: nlive above 262144 or ndim above 256 (the
 * message names the cap); a state above 4 GiB (the message names the largest max_dead). */
int mcalf_nested_open(mcalf_ctx* ctx, const double* U0, int64_t nlive, const mcalf_nested_opts* opts);
/* Runs rounds until the stop test max key + ln X < ln dlogz + ln Z holds before a round (reason 1), a round finds a plateau
 * (2), the dead rows cannot take another round plus the final nlive (3: ndead + K + nlive > max_dead), or max_rounds rounds of
 * this call have run (0) -- tested in that order.  out (NULL: not wanted) takes the state.  Calls continue each other: a round's
 * bits do not depend on how the rounds were cut into calls.  MCALF_ERR_INVALID: ctx NULL, max_rounds < 0, no open run, a
 * finished run, a replacement outside its constraint. */
int mcalf_nested_advance(mcalf_ctx* ctx, int32_t max_rounds, mcalf_nested_state_t* out);
/* Retires the remaining live points in key order (ndead grows by nlive), reads the dead logL once (one device-to-host copy of
 * LD) and computes ln Z, sqrt(max(H, 0) / nlive) and H (each pointer NULL: not wanted); the normalised log weights are kept for
 * mcalf_nested_read.  Afterwards the run only reads and closes.  MCALF_ERR_INVALID: ctx NULL, no open run, a finished run. */
int mcalf_nested_finish(mcalf_ctx* ctx, double* logZ, double* logZ_err, double* H);
/* Dead rows [first, first + count) in death order into the host arrays cube, theta [count][ndim], logL, logw [count]; any of
 * them NULL: not wanted.  theta is made on the fly by mcalf_scale_cube_batch's kernel (never stored).  MCALF_ERR_INVALID: ctx
 * NULL, no run, a range outside [0, ndead], logw before mcalf_nested_finish. */
int mcalf_nested_read(mcalf_ctx* ctx, int64_t first, int64_t count, double* cube, double* theta, double* logL, double* logw);
/* What the last round selected (a plateau round included), for tests and diagnostics: dying, pick [K], D [ndim][ndim], lmin
 * [1]; any NULL: not wanted.  MCALF_ERR_INVALID: ctx NULL, no run, no round yet. */
int mcalf_nested_last_round(mcalf_ctx* ctx, int32_t* dying, int32_t* pick, double* D, double* lmin);
/* Ends the run (finished or not); its device buffers stay with the context for the next run and are released by mcalf_destroy.
 * Without a run it does nothing.  ctx NULL: MCALF_ERR_INVALID. */
int mcalf_nested_close(mcalf_ctx* ctx);
/* Device bytes the context holds for its runs (the live and dead rows of the largest run so far and the rounds' workspaces;
 * 0 before the first mcalf_nested_open).  The dead rows dominate: max_dead (ndim + 1) 8 bytes.  It grows only when a run needs a
 * larger buffer than any before it: a value that does not change over a run says that the run allocated nothing.  ctx or
 * device_bytes NULL: MCALF_ERR_INVALID. */
int mcalf_nested_footprint(const mcalf_ctx* ctx, int64_t* device_bytes);
/* Per-kernel times of a round, for tools: with on = 1 every following round records HIP events around its book-keeping kernels
 * (0, the default: none; mcalf_nested_close turns it off again, so it is set on an open run).  mcalf_nested_last_times: milliseconds of the last round's rank, select, moments (both passes),
 * Cholesky, gather, replacement call and retire into ms [7].  MCALF_ERR_INVALID: ctx or ms NULL, on outside {0, 1}, no run, the
 * last round was not timed. */
int mcalf_nested_set_timing(mcalf_ctx* ctx, int32_t on);
int mcalf_nested_last_times(mcalf_ctx* ctx, double* ms);

/* What the LAST call of this context actually did (tests and benchmarks assert on the path taken instead of
 * inferring it from batch sizes).  `path`: which entry plan ran; the remaining fields describe the last fused-kernel
 * launch of that call. */
enum {
    MCALF_PATH_NONE = 0,          /* no call yet                                                              */
    MCALF_PATH_DEVICE = 1,        /* a *_device entry (caller's device pointers and stream)                   */
    MCALF_PATH_HOST_ZEROCOPY = 2, /* host pointers, small call: theta / logL through the page-locked mapped block */
    MCALF_PATH_HOST_PIPELINED = 3,/* host pointers, large scalar-output call: row blocks over two streams     */
    MCALF_PATH_HOST_STAGED = 4,   /* host pointers, model output: H2D, launch, D2H on the context's stream    */
    MCALF_PATH_HOST_STREAM = 5    /* host pointers, large scalar-output call: ONE streaming launch, no copy commands --
                                     the grid reads the parameter rows from page-locked memory while the host is still
                                     staging them, sets the live points up itself and writes logL into page-locked memory */
};
typedef struct {
    int32_t path;           /* MCALF_PATH_*                                                                   */
    int32_t row_blocks;     /* row blocks the call was issued in                                              */
    int32_t persistent;     /* 1: the last fused launch ran the persistent grid with the work-item queue      */
    int32_t grid;           /* workgroups of the last fused launch                                            */
    int64_t items;          /* work items (live points x tiles) of the last fused launch                      */
    int32_t lines_per_sync; /* lines folded per workgroup barrier (4 or 5)                                    */
    int32_t selfhalo;       /* 1: single-tile spectrum, halo entries are copies of the tile's own pixels      */
    int32_t pinned_in;      /* host-pointer entries: the parameter rows were page-locked caller memory        */
    int32_t pinned_out;     /* host-pointer entries: the result array was page-locked caller memory           */
    int32_t inline_setup;   /* 1: small launch -- ONE kernel, the per-sample set-up ran inside the fused kernel;
                               3: no launch at all -- the context's resident evaluator answered (mcalf_set_resident) */
    int32_t ordered;        /* 1: the persistent grid handed the live points out sorted by component count      */
    int32_t stream_setup_wgs; /* MCALF_PATH_HOST_STREAM: workgroups of the grid dedicated to the set-up while rows were outstanding */
    int32_t stream_polled;  /* MCALF_PATH_HOST_STREAM: 1 = completion seen through the kernel's page-locked word, 0 = stream signal;
                               MCALF_PATH_HOST_ZEROCOPY: 1 = completion read off the results in page-locked memory */
    int32_t xcd_mask;       /* bit i: the context's probe kernel saw workgroups of its stream on XCD i (hardware XCC_ID).  The
                               streaming launch deals rows to XCDs 0 .. 7 and is taken only when this is exactly 0xFF */
    int32_t stream_wgs_min; /* MCALF_PATH_HOST_STREAM (and a launch discarded as STARVED): the fewest / most workgroups of the */
    int32_t stream_wgs_max; /* launch an XCD received, counted by the kernel -- every XCD's rows are evaluated by ITS workgroups only */
    int32_t stream_fallback;/* host-pointer entries, what kept the call from being ONE streaming launch although its size asked
                               for one: 0 nothing (or not applicable), MCALF_STREAM_FALLBACK_* otherwise -- the row-block
                               pipeline (MCALF_PATH_HOST_PIPELINED) evaluated the call instead, same bits */
    int32_t devices_used;   /* device entries the call was cut over (1 for a single-device context)                   */
} mcalf_launch_info_t;
enum {
    MCALF_STREAM_FALLBACK_SHAPE = 1,     /* the stream does not reach exactly the eight XCDs of an unpartitioned MI355X
                                            (DPX / QPX / CPX partition, CU mask): decided before anything was launched */
    MCALF_STREAM_FALLBACK_TIMEOUT = 2,   /* a wait inside the launch ran out (host thread stalled > MCALF_STREAM_TIMEOUT) */
    MCALF_STREAM_FALLBACK_STARVED = 3    /* the launch drained, but an XCD that was dealt rows had received no workgroup:
                                            its rows were never evaluated, the launch's results were discarded */
};
int mcalf_last_launch(const mcalf_ctx* ctx, mcalf_launch_info_t* info);
/* The same for device entry k of a multi-device context (mcalf_last_launch itself reports entry 0 and devices_used). */
int mcalf_last_launch_sub(const mcalf_ctx* ctx, int32_t k, mcalf_launch_info_t* info);

/* Restrict EVERY stream the context owns -- the launch stream of the host-pointer entries and its auxiliaries, the resident
 * evaluator's stream (its kernel is stopped first; the next one-theta call starts another), the exchange stream of the
 * library's gather (pending exchanges are waited for) -- (*_device entries run on the CALLER's stream) to the
 * compute units of `mask` -- bit i % 32 of word i / 32 = CU i in the runtime's numbering (hipExtStreamCreateWithCUMask; on a
 * multi-XCD device consecutive bits go round the XCDs: bit i = CU i / 8 of XCD i % 8) -- as an embedding application does to
 * share one GPU between ranks.  nwords = 0 removes the mask.  The context waits for its streams, re-creates them and probes
 * again which XCDs they reach: on anything but all eight XCDs of an unpartitioned MI355X large host-pointer batches take the
 * row-block pipeline instead of the streaming launch (mcalf_launch_info_t.xcd_mask / .stream_fallback say so).  Measured on
 * ROCm 7.2 / MI355X (tools/explore/cu_mask_probe.py): an XCD whose share of the mask is EMPTY runs unrestricted, so a mask
 * slows a stream down but cannot take an XCD away from it -- what does is a partition mode (DPX / QPX / CPX).  A masked
 * stream is a BLOCKING stream in HIP's sense (hipExtStreamCreateWithCUMask has no non-blocking form): it synchronises with
 * work on the legacy default stream, which an unmasked context's streams do not.  Results never depend on the mask. */
int mcalf_set_cu_mask(mcalf_ctx* ctx, const uint32_t* mask, int32_t nwords);

/* How a streaming launch deals the rows of a batch to `nxcd` XCDs (blocks of eight rows, block k -> XCD k % nxcd): for
 * every row r < nrows, owner[r] = its XCD and local[r] = its index in that XCD's queue.  Pure host arithmetic (no
 * device needed) -- the same constexpr functions the kernels use; tests check that it is a bijection for every count. */
int mcalf_stream_partition(int32_t nrows, int32_t nxcd, int32_t* owner, int32_t* local);

/* Measurement aid: between _begin and _end every fused-kernel launch of this context is bracketed by
 * HIP events on the stream it is launched on (at most max_launches of them); _end waits for them and
 * returns the mean duration in milliseconds of mcalf_fused_kernel alone (the small per-sample set-up
 * kernel that precedes it is outside the bracket). */
int mcalf_profile_begin(mcalf_ctx* ctx, int32_t max_launches);
int mcalf_profile_end(mcalf_ctx* ctx, double* mean_ms, int32_t* launches);

/* Prior transform: theta = cube * ptp(bounds) + min(bounds) per dimension; when
 * int_ncomp != 0 the ncomp slot is truncated like Python int() (_scale_cube_pc), otherwise
 * left as is (_scale_cube_mn).  lo/hi are [ndim] host arrays; cube/theta [batch][ndim] host. */
int mcalf_scale_cube_batch(mcalf_ctx* ctx, const double* lo, const double* hi, const double* cube,
                           int64_t batch, int32_t int_ncomp, double* theta);

/* Unit cube in -> logL out: the composition lnlhood_pc(_scale_cube_pc(cube))
 * (hires_fitter.py:202-209 + :250-262) without materialising theta on the host.  mcalf_set_prior stores
 * the box (lo/hi [ndim], host, copied) and whether the ncomp slot is truncated (_scale_cube_pc) or not
 * (_scale_cube_mn); the prior transform is then applied inside the per-sample set-up kernel with numpy's
 * rounding (separate multiply and add), so logL is bit-identical to mcalf_loglike_batch on the rows
 * mcalf_scale_cube_batch returns.  theta / dtheta may be NULL; otherwise they receive the transformed
 * rows [batch][ndim] (what the sampler stores as the live point). */
int mcalf_set_prior(mcalf_ctx* ctx, const double* lo, const double* hi, int32_t int_ncomp);
int mcalf_loglike_cube_batch(mcalf_ctx* ctx, const double* cube, int64_t batch, double* theta, double* logL);
int mcalf_loglike_cube_batch_device(mcalf_ctx* ctx, const double* dcube, int64_t batch, double* dtheta,
                                    double* dlogL, void* stream);

/* Gaussian priors (the reference's Gpriors keyword: lnprior, hires_fitter.py:218-234, and __call__, :509-518); added within
 * ABI 9.  The prior of a context is its box times one Gaussian factor per parameter that carries one, NOT renormalised for the
 * truncation by the box (the reference's convention, :230).  For a row theta, the box lo / hi and mu[k], sigma[k]:
 *   lnprior(theta) = -inf                                                       if any theta_k is NaN or outside [lo_k, hi_k]
 *                  = sum over k with sigma[k] > 0 of  -0.5 (((theta_k - mu[k]) / sigma[k])^2 + c_k),  c_k = ln(2 pi sigma[k]^2)
 *                    otherwise; with no Gaussian coordinate the sum is an exact 0.
 * The arithmetic is a fixed sequence of separately rounded IEEE operations (no FMA), so that numpy restates it bit for bit
 * (tests/prior_reference.py):
 *   c_k     computed ONCE by std::log on the host when the prior is set, and stored: mcalf_get_gauss_prior returns the bits
 *   theta_k the row's entry; for a unit-cube row u:  p = u_k (hi_k - lo_k);  theta_k = p + lo_k   (the arithmetic of
 *           mcalf_scale_cube_batch, so theta has the bits mcalf_loglike_cube_batch returns; the ncomp slot never carries a
 *           Gaussian, so its truncation does not enter).  A cube entry outside [0, 1] or NaN: -inf
 *   term    d = (theta_k - mu_k) / sigma_k;  dd = d d;  s = dd + c_k;  term = -0.5 s
 *   row     ONE wave64 owns a row, lane l owns coordinates l, l + 64, ...: it adds its terms in index order onto +0.0
 *           (coordinates with sigma[k] == 0 are skipped, not added as zeros); the 64 lane sums are folded by the xor-butterfly
 *           v <- v + v[lane ^ m], m = 32, 16, ..., 1.
 *
 * mcalf_set_gauss_prior: mu, sigma [ndim] host arrays (copied); needs mcalf_set_prior first.  sigma[k] == 0: no Gaussian on k.
 * Refused with MCALF_ERR_INVALID, naming the argument and the index, before any device work: sigma[k] negative, NaN or
 * infinite; a non-finite mu[k] where sigma[k] > 0; sigma[k] > 0 on the ncomp slot (the box truncates that slot to an integer: a
 * density on it has no defined mass).  NULL, NULL clears the prior.  A later mcalf_set_prior with another box keeps the
 * Gaussian.  On a multi-device context every device entry receives it.
 * mcalf_get_gauss_prior: what the kernels use -- mu, sigma, c [ndim] (each may be NULL; zeros when none is set) and the number
 * of Gaussian coordinates (0 when none is set).
 * mcalf_lnprior_batch: rows [batch][ndim] -> lnprior [batch]; from_cube 1: unit-cube rows, 0: parameter rows.  With no Gaussian
 * set: 0 / -inf by the box test alone.  A multi-device context cuts the rows over its devices.  batch == 0 does nothing.
 * mcalf_lnprior_batch_device: the same over device pointers on `stream`; never synchronises, never allocates; refuses a
 * multi-device context.
 *
 * What honours it.  mcalf_slice_replace_batch[_device]: the constrained quantity is logL + lnprior (one rounded add), for the
 * start's test against Lmin, for every trial, and in the returned logL, which is then
 * mcalf_loglike_cube_batch(U) + mcalf_lnprior_batch(U, from_cube = 1) bit for bit -- nested sampling of L g under the box
 * measure.  mcalf_ensemble_batch / mcalf_tempered_batch[_device]: logL, CL and the temperature stay the likelihood's; the accept
 * rule of a half-step is  q = (h + beta (ly - lx)) + (py - px)  for the stretch move (h its Hastings term) and
 * q = beta (ly - lx) + (py - px)  for the DE move, py / px lnprior of the trial and of the walker; a proposal outside the cube
 * never has its prior read; a swap's rule is unchanged (the prior cancels between rungs), and the rung at beta = 0 samples the
 * Gaussian factors over the cube.  With no Gaussian set all of them run the code path, and return the bits, they did before.
 * mcalf_maximize_batch does NOT: it maximises logL alone (a MAP fit needs a diagonal term in its CG operator). */
int mcalf_set_gauss_prior(mcalf_ctx* ctx, const double* mu, const double* sigma);
int mcalf_get_gauss_prior(const mcalf_ctx* ctx, double* mu, double* sigma, double* c, int32_t* ngauss);
int mcalf_lnprior_batch(mcalf_ctx* ctx, const double* rows, int64_t batch, int32_t from_cube, double* lnprior);
int mcalf_lnprior_batch_device(mcalf_ctx* ctx, const double* drows, int64_t batch, int32_t from_cube, double* dlnprior,
                               void* stream);

/* Multi-GPU inside the library (the reference's only parallelism is data parallelism over live
 * points: PolyChord's MPI workers cli.py:110, jaxns' vmap cli.py:275-280).  One process per GPU, each with its own
 * context; the context owns an RCCL communicator (xGMI on one node).  Rank 0 obtains a 128-byte id with
 * mcalf_comm_unique_id and hands it to the other ranks by any means (MPI, torch.distributed, a file); every rank
 * then calls mcalf_comm_init (collective).
 *
 * mcalf_loglike_gatherv_device evaluates the rank's own contiguous block of live points on `stream` and enqueues ONE
 * grouped send / receive exchange (what ncclGather is) that lands every rank's logL block in dlogL_all on `root`:
 * block r at offset counts[0] + ... + counts[r-1].  `counts` is a HOST array [nranks] that every rank passes
 * identically (ragged shards allowed, zeros allowed; counts[rank] must equal batch_local); NULL means every rank
 * evaluates batch_local rows (mcalf_loglike_gather_device is that form).  dlogL_all may be NULL on the other ranks.
 * By default the exchange is enqueued on `stream` itself, right behind the kernels (plain stream semantics: what
 * follows on `stream` sees the gathered vector; nothing crosses streams).  With mcalf_comm_set_overlap(ctx, 1) and more
 * than one rank it runs on a context-owned stream behind an event of `stream`, so that the root's NEXT kernels do not
 * queue behind receives that wait for its peers: the exchange of call k overlaps the kernels of call k+1, the caller
 * alternates between TWO (dlogL_local, dlogL_all) buffer pairs -- the library orders call k+2 behind exchange k -- and
 * calls mcalf_comm_join(ctx, stream) before it consumes a result.
 * Nothing synchronises the host.  Because a live point's arithmetic does not depend on the shard, the gathered
 * vector equals the single-GPU result bit for bit.
 *
 * Errors never leave a peer waiting:
 *   - MCALF_ERR_INVALID from the argument checks: nothing was enqueued on this rank (a programming error that every
 *     rank of a correct SPMD caller makes alike).
 *   - a LOCAL failure (workspace growth, kernel launch): the rank still takes its part in the exchange with a block
 *     of NaNs, then returns its error code; the peers complete, the root sees NaN rows for that rank, and the
 *     communicator stays usable.
 *   - a failure inside the exchange itself (RCCL / event calls): the communicator is aborted (ncclCommAbort),
 *     MCALF_ERR_COMM is returned and every later gather is refused until mcalf_comm_destroy + mcalf_comm_init.
 * RCCL is loaded at run time by the first of these calls (MCALF_ERR_COMM if it is absent; MCALF_RCCL_LIB names an
 * explicit library); single-GPU use never touches it. */
#define MCALF_COMM_ID_BYTES 128
int mcalf_comm_unique_id(void* id128);
int mcalf_comm_init(mcalf_ctx* ctx, const void* id128, int32_t nranks, int32_t rank);
int mcalf_comm_info(const mcalf_ctx* ctx, int32_t* nranks, int32_t* rank);
int mcalf_comm_destroy(mcalf_ctx* ctx);
int mcalf_comm_set_overlap(mcalf_ctx* ctx, int32_t on);
int mcalf_comm_join(mcalf_ctx* ctx, void* stream);
int mcalf_loglike_gather_device(mcalf_ctx* ctx, const double* dP, int64_t batch_local, double* dlogL_local,
                                double* dlogL_all, int32_t root, void* stream);
int mcalf_loglike_gatherv_device(mcalf_ctx* ctx, const double* dP, int64_t batch_local, double* dlogL_local,
                                 double* dlogL_all, const int64_t* counts, int32_t root, void* stream);

/* Diagnostic: out[i] = H(x[i], y[i]) = Re w(x + i y) evaluated by the device Voigt function
 * (host pointers).  device = -1 for the current device. */
int mcalf_voigt_hjerting(const double* x, const double* y, int64_t n, double* out, int32_t device);
/* Same with the arithmetic an interpolation NODE gets: between x_c (6.2 for K = 1) and 8 the zone-1 wing
 * polynomial with exp(-x^2) dropped, instead of the core table a directly evaluated pixel uses there. */
int mcalf_voigt_hjerting_nodes(const double* x, const double* y, int64_t n, double* out, int32_t device);
/* The gradient path's Voigt function and its partials: out[3i], out[3i+1], out[3i+2] = H, dH/dx, dH/dy at
 * (x[i], y[i]), y >= 0 (host pointers; device = -1 for the current device). */
int mcalf_voigt_hjerting_grad(const double* x, const double* y, int64_t n, double* out, int32_t device);

#ifdef __cplusplus
}
#endif
#endif /* MCALF_HIP_H */
