/*
 * blr_mi355x.h -- C ABI of the MI355X (gfx950) implementation of the posterior / logpdf / marginals /
 * rand hot path of BayesianLinearRegressors.jl.
 *
 * The reference has no FFI boundary: its "operator API" is Julia dispatch on
 * FiniteGP{<:BayesianLinearRegressor} (reference src/bayesian_linear_regression.jl:33-69).  The entry
 * points below are what a `ccall` from those methods binds; each one cites the reference lines it
 * replaces.  INTEGRATION.md shows the Julia side.
 *
 * Conventions
 *   - everything is column-major (Julia native); sizes/strides are int64_t (Julia Int), in ELEMENTS;
 *   - `_f64` / `_f32` suffix = element type of X, y, s, mw, Lw and of the array outputs;
 *     the log marginal likelihood is ALWAYS double (reference :84 promotes through log(2pi)::Float64);
 *   - the caller owns every buffer; no pointer is retained after a call returns;
 *   - calls are synchronous w.r.t. the handle's stream unless the handle was put in async mode
 *     (blr_set_async): then DEVICE-memspace calls only enqueue and the caller synchronises;
 *   - no C++ exception crosses this boundary.
 *
 * Return codes (LAPACK `info` semantics)
 *      0  success
 *     >0  (single-problem calls) Cholesky broke at leading minor k: the matrix is not positive
 *         definite -> the Julia shim throws PosDefException(k), as `cholesky` at reference :78/:86 would
 *     <0  argument -k is invalid (shape/stride/enum/NULL) -> DimensionMismatch / ErrorException
 *         (the reference's own checks are :74 and :26-31)
 *  <= -1000  HIP runtime failure: -(1000 + hipError_t); text via blr_last_error()
 *   Batched calls fill info[B] per regressor (0 / k>0) and return 0 when the launch itself succeeded:
 *   one non-SPD regressor does not poison the batch.
 */
#ifndef BLR_MI355X_H
#define BLR_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BLR_ABI_VERSION 1

/* layout of X -- mirrors x_as_colvecs, reference :20-31 (index/shape work, bit-exact) */
#define BLR_LAYOUT_COLVECS 0 /* X is D x N column-major: element (d,n) at X[d + n*ldx], ldx >= D   (:22) */
#define BLR_LAYOUT_ROWVECS 1 /* X is N x D column-major: element (d,n) at X[n + d*ldx], ldx >= N   (:24) */

/* observation-noise covariance Sigma_y (FiniteGP field, reference :79) */
#define BLR_NOISE_ISOTROPIC 0 /* s points to ONE variance  (AbstractGPs f(x, sigma^2))  */
#define BLR_NOISE_DIAGONAL 1  /* s[N] variances            (Diagonal(v))                */
#define BLR_NOISE_DENSE 2     /* N x N symmetric matrix (upper triangle read, as LAPACK 'U'), column-major: only the
                                 *_dense_noise entry points and blr_mean_and_cov_* take it (moderate N, <= 16384) */

/* prior precision Lambda_w (struct field, reference :11-14; _cholesky at :78) */
#define BLR_PRIOR_DENSE 0        /* Lw: D x D symmetric, UPPER triangle read (as LAPACK potrf 'U'), ldl >= D */
#define BLR_PRIOR_UPPER_FACTOR 1 /* Lw: upper factor U with Lambda_w = U'U (PDMat / previous T, :93); strictly-lower part ignored */
#define BLR_PRIOR_DIAGONAL 2     /* Lw: d[D], Lambda_w = Diagonal(d); ldl ignored */

/* where the pointers of a call live */
#define BLR_MEM_HOST 0   /* host pointers: the library stages through its own device workspace */
#define BLR_MEM_DEVICE 1 /* device pointers (hipMalloc / torch / CUDA.jl-style allocator)       */

typedef struct blr_handle blr_handle;

/* ---- lifetime ------------------------------------------------------------------------------- */
int blr_abi_version(void);
int blr_device_count(void);                       /* number of visible HIP devices (0 if none)          */
int blr_create(int device, blr_handle** out);     /* one handle per Julia task / thread                  */
int blr_destroy(blr_handle* h);
const char* blr_last_error(blr_handle* h);        /* valid until the next call on h; never NULL         */
/* A handle's work is ordered by ONE stream at a time: switching streams drains the old one first.  Not supported: capturing a
 * handle's launches into a HIP graph and replaying them, and calls on one handle from two streams / threads at once (the large-D
 * factorisation keeps arrival counters and tagged exchange words per handle) -- use one handle per stream.  The stream being
 * left must still be alive when blr_set_stream / blr_reset_stream is called (it is drained); if it has been destroyed already the
 * whole device is drained instead and the switch still happens. */
int blr_set_stream(blr_handle* h, void* hip_stream); /* run on the caller's hipStream_t; NULL = the HIP null stream */
int blr_reset_stream(blr_handle* h);              /* back to the handle's own (non-blocking) stream      */
int blr_set_async(blr_handle* h, int async);      /* 1: DEVICE-memspace calls return after enqueue       */
int blr_synchronize(blr_handle* h);
/* Run-time switches of the handle (A/B measurements and tests; the defaults are the measured best).  `key` is one of NO_LDSDMA,
 * NO_WAVE_KERNEL, NO_GRAM_RING, NO_DIAG_SPLIT, NO_XCD_SWIZZLE, NO_MFMA_PROJECT, NO_I8_GRAM, NO_I8_DIAG, NO_I8_FACTOR, NO_I8_ROWVECS, NO_I8_DENSE, NO_I8_FALLBACK, NO_BF16X3, NO_PLANES, NO_FP16_PLANES, PLANES8, NO_SPEC_ROWMAX, NO_MULTI_PLANES, NO_MARG_GEMM, NO_GRAD_GEMM, NO_DOWNDATE_LDS, PLAN_DEBUG (flags: any non-empty value = on),
 * WAVE_SPLIT = 1|2|4, CHAIN_BATCH = 1..128, CHAIN_WS_MB, I8_PROBE_MIN = 256..2^20, I8_GROUPS = 6|7, RAGGED_ITEM = 1..2^30 (tests: observations per work item of blr_marginals_ragged_* / blr_loo_ragged_*, rounded up to 64), MAX_CHUNK = 1..65535 (tests: at most that many regressors per chunk / slice of every batched entry point, so that small batches cross the seams over-bound batches cross), SWEEP = always|never|auto, GRAM_SPLITS = "o,d[,nlong]" (README.md);
 * a "BLR_MI355X_" prefix is accepted.  value NULL or "" restores the built-in default.  The environment variables
 * BLR_MI355X_<KEY> are read ONCE, by blr_create -- no entry point reads the environment.  -> 0, or -2 / -3 (unknown key /
 * malformed value). */
int blr_set_option(blr_handle* h, const char* key, const char* value);
/* Which kernel family the most recent blr_posterior_* / blr_logpdf_* dispatch of this handle launched -- what a profile of the call
 * shows: "fused_i8_kernel", "fused_small_kernel<double, 8, 4>", "fused_wave_kernel<double, 4, 1>", "gram_tile_kernel<float>" (the
 * large-D pipeline), ...; "none" before the first call.  The pointer stays valid until the next call on the handle.  (bench.py labels
 * its roofline with it instead of re-deriving the dispatcher's decision.)  The int8 route decides on the device what it keeps: when
 * it handed more than half of the call's regressors back to the fp64 kernel (heavy-tailed inputs: the probe slice sends the rest of
 * the batch there) the answer is "fused_small_kernel<double, 8, 4> (int8 route handed back K of B)" -- after an int8-route call this
 * function therefore drains the handle's stream. */
const char* blr_last_route(blr_handle* h);
/* Counters of the handle since blr_create / blr_reset_stats.  key: "i8_regressors" = regressors sent down the int8-sliced Gram route
 * (blr_posterior_batched_f64 above); "i8_handed_back" = those of them that route could not finish (rows outgrowing their scale
 * beyond what it corrects in place, non-finite inputs) and the fp64 kernel redid inside the same call -- each of these cost two
 * passes over its data (reading it synchronises the handle's stream); "planes_redone" = fp32 updates at D > 128 (ColVecs) whose
 * SAMPLED row scales did not hold -- the operand planes of the Gram product are scaled per row by a power of two taken from the first 32
 * columns of every column chunk (doubled: an entry up to 16 x the sample's largest still fits); an entry beyond that sends the call
 * through the exact row maxima and the planes pass a second time (one more read of X; option NO_SPEC_ROWMAX = 1 always takes the exact
 * maxima: one more read of X on every call); "loo_degenerate" = observations blr_loo_batched_* gave NaN because their 1 - h_n was
 * <= 0 or not finite (reading it synchronises the handle's stream); "kfold_degenerate" = folds blr_kfold_batched_* or
 * blr_kfold_multi_batched_* (once per fold, whatever S is) gave NaN because the Cholesky of their I - H~ met a pivot <= 0 or not finite, and folds blr_kfold_large_batched_* gave NaN because that of their
 * A - G_f did (reading it synchronises the handle's stream); "last_chunks" = chunks / slices of regressors the handle's most
 * recent call launched (NOT cumulative: every entry point starts it at 1; a batch beyond grid.y = 65535, a workspace or image bound, or
 * option MAX_CHUNK, goes in several; blr_update_factor_ragged_* / blr_downdate_factor_ragged_* count the launches of their
 * regressors with observations, 0 when there is none); "ragged_sweep", "ragged_refit", "ragged_idle" = regressors on each route of
 * the handle's most recent blr_update_factor_ragged_* / blr_downdate_factor_ragged_* call (NOT cumulative; host-side integers);
 * "workspace_bytes" = device scratch the handle holds now.
 * The variance route of the handle's most recent blr_marginals_batched_* call (NOT cumulative; host-side integers): "marg_block_rt"
 * = 32 or 16, the tile height of marg_blocksub_kernel (block forward substitution on LDS-resident tiles of inputs: D > 128, 16 | D,
 * aligned ColVecs, factor or dense prior, D <= 1152 in fp32 / 512 in fp64), or 0 when the call ran anywhere else (diagonal prior,
 * D <= 128, the tall-matrix sweep, mean only); "marg_block_walk" = tiles the busiest workgroup of that kernel walked (the largest
 * ceil(tiles / grid.x) over the call's launches; 0 with "marg_block_rt" = 0); "marg_block_renumbered" = 1 if any of those launches
 * renumbered its workgroups so that an XCD gets whole regressors (more than one regressor and a grid that is a multiple of 8).
 * The kernels of the handle's most recent blr_sample_weights_* / blr_apply_weights_* / blr_rand_* / blr_rand_batched_* call (NOT
 * cumulative; a host-side bitmask, cleared at the entry of these four and set where the launch is picked): "draw_route" = weights
 * 1 diag_sample_kernel | 2 sample_weights_mfma_kernel (+ 4 when its 16-byte loader of the factor applies: D = 128, ld a multiple
 * of the vector width, 16-byte aligned pointer) | 8 the D > 128 wave solves | 16 / 32 rand_batched_solve_kernel with one / four
 * draws per wave, or-ed with the projection 64 fused into the solve | 128 the scalar tiles | 256 the matrix-core tiles | none of the
 * three: no projection ran (tests assert it, so that a case meant for one kernel cannot pass on another).
 * -> 0, -2 unknown key, -3 NULL value. */
int blr_get_stat(blr_handle* h, const char* key, int64_t* value);
int blr_reset_stats(blr_handle* h);
/* The handle's device scratch (factorisation workspaces of D > 128 calls -- up to 8 GiB for a large batched call, see CHAIN_WS_MB --
 * the feature matrix of blr_posterior_rff_*, the int8 / marginal side buffers, the statistics buffer of blr_logpdf_grid_*, the offsets / order of blr_posterior_ragged_*, column 0's evidences and -- T_post = NULL -- the factors of blr_posterior_multi_batched_*) only ever GROWS between calls; this drains the
 * stream and frees all of it.  The next call allocates what it needs again. */
int blr_release_workspace(blr_handle* h);

/* ---- device memory helpers (so a host language needs no HIP binding of its own) -------------- */
int blr_device_alloc(blr_handle* h, size_t bytes, void** dptr);
int blr_device_free(blr_handle* h, void* dptr);
int blr_memcpy_h2d(blr_handle* h, void* dst_device, const void* src_host, size_t bytes);
int blr_memcpy_d2h(blr_handle* h, void* dst_host, const void* src_device, size_t bytes);

/* ---- timing helpers: HIP events on the handle's stream (bench.py roofline leg) ---------------- */
int blr_timer_start(blr_handle* h);
int blr_timer_stop(blr_handle* h, float* elapsed_ms); /* records, synchronises, returns the interval */

/* ---- fused inference: replaces __compute_inference_quantities + logpdf + posterior ------------
 * reference src/bayesian_linear_regression.jl:72-89 (shared quantities), :55-58 (logpdf),
 * :60-69 (posterior), :92-93 (__build_Lambda).  One pass produces everything both need:
 *   A = Lw + X S X'   T = chol(A).U   mw' = mw + A^-1 X S (y - X'mw)
 *   logpdf = -1/2 [N log 2pi + logdet Sy + d'Sd + logdet A - logdet Lw - |T^-T b|^2]
 * Outputs (each may be NULL to skip it):
 *   mw_post[D]; T_post D x D upper factor (strictly-lower part written as zero), ldt >= D;
 *   Lw_post D x D full symmetric A, ldlp >= D; logpdf (double).
 * In-place form: with prior_kind = BLR_PRIOR_UPPER_FACTOR, mw_post == mw and T_post == Lw are allowed (every read of the
 * prior state completes before the first write; blr_update_factor_* relies on it).  mw_post and T_post of a regressor whose
 * info != 0 are left untouched at every D (Lw_post may already hold A): a resident state survives a bad batch.
 * Batched form: regressor i reads X + i*strideX, y + i*stridey, s + i*strides, mw + i*stridemw,
 * Lw + i*strideLw and writes the outputs at their strides; a stride of 0 shares an input.
 * Numerics: results are bit-reproducible from call to call (fixed accumulation order, no floating-point atomics).  fp64
 * accuracy against the reference's op sequence in LAPACK: evidence 1e-10 relative, mw', T, Lw' 1e-9 (tests/test_gpu_parity.py).
 * One shape takes a different route to the same numbers: D = 128 in fp64 -- aligned ColVecs or RowVecs (16-byte aligned rows), isotropic or
 * diagonal noise, any prior kind, 512 <= N <= 16384 (+ a last partial block of up to 31 columns, added in fp64) -- forms X X' on the int8
 * matrix cores from an exact 48-bit splitting of the inputs against per-row power-of-two scales (csrc/blr_fused_i8.hpp); everything after
 * the Gram matrix is fp64 as elsewhere.  Its error model, stated BEFORE the tests that hold it to it (tests/test_gpu_parity.py test_i8_*,
 * test_c2_shape_fp64):
 *   - entries of Lw' within 1e-13 of sqrt(Lw'_ii Lw'_jj) (measured: 3e-14) instead of a few ulp of themselves -- an entry that nearly
 *     cancels is off by that much of its row's and column's scale, not of itself;
 *   - the evidence within the 1e-10 above; where delta'Sigma^-1 delta and |T^-T b|^2 cancel (data explained by the weights) the error is
 *     1e-14 of delta'Sigma^-1 delta: |d logpdf| <= 1e-11 |logpdf| + 1e-14 delta'Sigma^-1 delta is what the tests assert;
 *   - inputs whose low mantissa bits are zero (float32 values, integers, powers of two) are covered: the digits are BALANCED (bytes of
 *     the integer + 0x8080808080, minus 128), so a zero low digit is 0 and its truncated products vanish; what is truncated is zero-mean
 *     unless the low digits of a row are a constant non-zero pattern (every entry = integer + 1/3): 1e-13 there (tools/i8_digits_emul.py);
 *   - six digit groups under isotropic noise, seven under diagonal noise (the rows' bounds are then bounds of x times the LARGEST
 *     1 / sqrt(s_n), loose by the spread of the variances).  Option I8_GROUPS = 7 keeps the seventh group under isotropic noise too:
 *     entries within 1e-14 (measured) instead of 3e-14 of their scale at 0.8 x the rate; I8_GROUPS = 6 drops it under diagonal noise
 *     where the variances are of one magnitude: 3e-14 x (largest / typical 1 / sqrt(s_n))^2, 1.2 x the rate;
 *   - an entry that outgrows its row's scale (taken from the first 96 columns, 2 - 4 x their largest entry) is corrected in fp64 inside the
 *     kernel; a regressor with more than one such 32-column block in 16 (heavy-tailed features), Inf / NaN, or a prior mean that explains
 *     the data to three digits is REDONE on the fp64 matrix pipe inside the same call -- it then costs two passes; blr_get_stat(h,
 *     "i8_handed_back", ..) counts them, and a batch of more than 4096 regressors (option I8_PROBE_MIN) whose first 256 were handed back by more than a quarter
 *     sends the rest to the fp64 kernel directly.
 * blr_set_option(h, "NO_I8_GRAM", "1") keeps every regressor on the fp64 matrix pipe.
 * fp32, D > 128, aligned ColVecs: the Gram matrix is formed on the bf16 matrix cores from an EXACT three-way split of every fp32 operand
 * (x = h + m + l, each rounded to nearest), keeping the six products hh, hm, mh, mm, hl, lh under fp32 accumulation: the dropped ones are
 * 2^-24 of |a||b| each and zero-mean, the result is as accurate as an fp32 fma chain (tools/bf3_unit.hip; tests hold A to 4 x the error
 * of fp32 LAPACK on the same inputs, test_c3_full_size / test_c5_full_size).  blr_set_option(h, "NO_BF16X3", "1") uses the fp32 matrix
 * instruction instead.
 */
int blr_posterior_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,
                              const double* X, int64_t ldx, int64_t strideX,
                              const double* y, int64_t stridey,
                              int noise_kind, const double* s, int64_t strides,
                              int prior_kind, const double* mw, int64_t stridemw,
                              const double* Lw, int64_t ldl, int64_t strideLw,
                              double* mw_post, int64_t stride_mwpost,
                              double* T_post, int64_t ldt, int64_t strideT,
                              double* Lw_post, int64_t ldlp, int64_t strideLp,
                              double* logpdf, int32_t* info);
int blr_posterior_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,
                              const float* X, int64_t ldx, int64_t strideX,
                              const float* y, int64_t stridey,
                              int noise_kind, const float* s, int64_t strides,
                              int prior_kind, const float* mw, int64_t stridemw,
                              const float* Lw, int64_t ldl, int64_t strideLw,
                              float* mw_post, int64_t stride_mwpost,
                              float* T_post, int64_t ldt, int64_t strideT,
                              float* Lw_post, int64_t ldlp, int64_t strideLp,
                              double* logpdf, int32_t* info);

/* ---- regressors with UNEQUAL observation counts in one call -----------------------------------------------------
 * Replaces: reference src/bayesian_linear_regression.jl:55-58 (logpdf), :60-69 (posterior) and :72-89 (shared quantities) under a
 * map over fxs of different lengths -- which blr_posterior_batched_* (one N for the batch) serves only by a loop of calls or by
 * padding every regressor to the longest one.
 * The observations of all regressors are packed side by side: regressor b owns observations [offsets[b], offsets[b+1]), N_b =
 * offsets[b+1] - offsets[b].  ColVecs: X is D x offsets[B] column-major, ldx >= D, regressor b starts at X + offsets[b]*ldx.
 * RowVecs: X is offsets[B] x D column-major, ldx >= offsets[B], regressor b starts at X + offsets[b], its element (d,n) at
 * + n + d*ldx.  y + offsets[b].  Diagonal noise: s + offsets[b] (strides ignored); isotropic noise: s + b*strides (0: one variance
 * for all regressors); dense noise is an argument error.  The prior, the prior mean, the outputs (each may be NULL), info[B], the
 * in-place form under BLR_PRIOR_UPPER_FACTOR and the return codes are those of blr_posterior_batched_*: every regressor has its own
 * status, mw_post and T_post of a regressor with info != 0 are left untouched and its logpdf is NaN, the call returns 0 when the
 * launch succeeded; output strides that overlap for B > 1 are argument errors.
 * offsets is shape metadata like N: ALWAYS a host array of B + 1 entries, in both memspaces; offsets[0] >= 0, non-decreasing (N_b = 0
 * is allowed: the posterior is the prior, the evidence 0), every N_b <= 2^30 (the bound on N of blr_posterior_batched_*); a
 * violation is argument error -6.  The argument checks come before the handle's.  B = 0 is a no-op.
 * D <= 128 (csrc/blr_ragged.hpp): ONE launch of one workgroup per regressor running the phases of the fused kernel --
 * streaming Gram on the fp64 / fp32 matrix cores, blocked Cholesky, back substitution -- on the regressor's slice.  The host orders
 * the regressors by descending N_b (ties by index), workgroup i takes the i-th longest: with the hardware's in-order dispatch that is
 * longest-first list scheduling.  offsets and that order (12 bytes per regressor) are uploaded to the handle's workspace
 * (blr_release_workspace frees it).  This route always uses these phases: the int8-sliced Gram and the one-wave kernel stay with the
 * equal-count entry point.  The LDS-DMA loader needs ColVecs with 16-byte aligned X and ldx (no condition on offsets); other ColVecs
 * data and RowVecs take the generic loaders.
 * Numerics: the outputs of regressor b are bit for bit those of blr_posterior_batched_* with B = 1 on its slice on a handle with
 * NO_I8_GRAM = 1 and NO_WAVE_KERNEL = 1 (the same code on the same data); bit-reproducible from call to call, independent of B, of
 * the other regressors' data and of any permutation of the batch.
 * Async handle, device memspace: the call only enqueues the kernel, but the upload of offsets / order drains the handle's stream
 * first (it may block the host); the library is finished with the caller's offsets array when the call returns.
 * D > 128: correct, not fast -- one regressor after the other through the pipeline of blr_posterior_batched_* with B = 1; the call
 * synchronises whatever the handle's async flag says.
 * _f32: X, y, s, mw, Lw, mw_post, T_post, Lw_post are float; logpdf stays double. */
int blr_posterior_ragged_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                             const int64_t* offsets, /* HOST array of B + 1 entries in both memspaces */
                             const double* X, int64_t ldx, const double* y,
                             int noise_kind, const double* s, int64_t strides,
                             int prior_kind, const double* mw, int64_t stridemw,
                             const double* Lw, int64_t ldl, int64_t strideLw,
                             double* mw_post, int64_t stride_mwpost,
                             double* T_post, int64_t ldt, int64_t strideT,
                             double* Lw_post, int64_t ldlp, int64_t strideLp,
                             double* logpdf, int32_t* info);
int blr_posterior_ragged_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                             const int64_t* offsets, /* HOST array of B + 1 entries in both memspaces */
                             const float* X, int64_t ldx, const float* y,
                             int noise_kind, const float* s, int64_t strides,
                             int prior_kind, const float* mw, int64_t stridemw,
                             const float* Lw, int64_t ldl, int64_t strideLw,
                             float* mw_post, int64_t stride_mwpost,
                             float* T_post, int64_t ldt, int64_t strideT,
                             float* Lw_post, int64_t ldlp, int64_t strideLp,
                             double* logpdf, int32_t* info);

/* ---- marginals of regressors with UNEQUAL observation counts in one call ------------------------------------------------------
 * Replaces: reference src/bayesian_linear_regression.jl:33 (mean), :40-43 (var) and :47 (mean_and_var) under a map over fxs of
 * different lengths -- which blr_marginals_batched_* (one N for the batch) serves only by a loop of calls or by padding every
 * regressor to the longest one.
 * Packing: exactly blr_posterior_ragged_*'s.  offsets is ALWAYS a host array of B + 1 entries, in both memspaces; offsets[0] >= 0,
 * non-decreasing, every N_b = offsets[b+1] - offsets[b] <= 2^30; a violation is argument error -6.  ColVecs: regressor b's inputs
 * start at X + offsets[b]*ldx (ldx >= D); RowVecs: at X + offsets[b] (ldx >= offsets[B]).  Diagonal noise: s + offsets[b];
 * isotropic noise: s + b*strides; dense noise is an argument error.  mw + b*stridemw, Lw + b*strideLw; all three prior kinds, with
 * the meaning blr_marginals_batched_* gives them.
 * Outputs: element n of regressor b is written at mean[offsets[b] + n] / var[offsets[b] + n] -- packed as the inputs are; there are
 * no output strides, so nothing can overlap.  Either may be NULL; with var == NULL neither s nor Lw is read (both may be NULL).
 * info[B]: the status of a dense prior's factorisation (> 0: not positive definite; the outputs of that regressor are left
 * untouched), 0 otherwise.  The call returns 0 when the launches succeeded.  N_b = 0 writes nothing for that regressor; B = 0 is a
 * no-op.  The argument checks come before the handle's: a NULL handle with valid arguments returns -1.
 * D <= 128 (csrc/blr_marg_ragged.hpp, csrc/blr_ragged_items.hpp): the host cuts every regressor into work items of at
 * most W observations (W a multiple of 64, about one round of resident workgroups over the call; handle option RAGGED_ITEM forces it
 * for tests) and launches one workgroup per item -- a regressor far longer than the others is spread over the chip instead of
 * ending the call alone.  D = 128 with a factor or dense prior, ColVecs with 16-byte aligned X and ldx or RowVecs: the
 * triangular inverse image once per regressor, then the product stream of blr_marginals_batched_* over the item's tiles (a mean-only
 * call of such a shape runs the same kernel without image and product: the route never depends on the outputs requested).  Any other
 * D <= 128 shape: the triangular sweep over LDS-resident tiles of 64 inputs.  offsets and the item table (8 + 12 bytes per
 * regressor and item) are uploaded to the handle's workspace (counted by blr_get_stat "workspace_bytes", freed by
 * blr_release_workspace).
 * Bit promises (to this entry point itself): results are bit-reproducible from call to call; the bits of regressor b are those of
 * this entry point with B = 1 on its slice -- independent of B, of the other regressors' data and counts, of any permutation of the
 * batch, of the chunking (option MAX_CHUNK) and of how a regressor is cut into work items; the bits of one output do not depend on
 * which other outputs are requested; host and device memspace give the same bits; no float atomics.  NOT promised: bit-equality with
 * blr_marginals_batched_* (it routes by N and runs its products in another order).
 * Async handle, device memspace: the call only enqueues kernels, but the upload of offsets and the item table drains the handle's
 * stream first (it may block the host); the library is finished with the caller's offsets array when the call returns.
 * D > 128: correct, not fast -- one regressor after the other through blr_marginals_batched_* with B = 1; the call synchronises
 * whatever the handle's async flag says.
 * _f32: X, s, mw, Lw, mean, var are float. */
int blr_marginals_ragged_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                             const int64_t* offsets, /* HOST array of B + 1 entries in both memspaces */
                             const double* X, int64_t ldx,
                             int noise_kind, const double* s, int64_t strides,
                             int prior_kind, const double* mw, int64_t stridemw,
                             const double* Lw, int64_t ldl, int64_t strideLw,
                             double* mean, double* var, int32_t* info);
int blr_marginals_ragged_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                             const int64_t* offsets, /* HOST array of B + 1 entries in both memspaces */
                             const float* X, int64_t ldx,
                             int noise_kind, const float* s, int64_t strides,
                             int prior_kind, const float* mw, int64_t stridemw,
                             const float* Lw, int64_t ldl, int64_t strideLw,
                             float* mean, float* var, int32_t* info);

/* ---- exact LEAVE-ONE-OUT predictives of regressors with UNEQUAL observation counts in one call ----------------------------------
 * Replaces: reference src/bayesian_linear_regression.jl:55-58 (logpdf) applied to each held-out point given the rest, under a map
 * over fxs of different lengths -- blr_loo_batched_* once per regressor, or with every regressor padded to the longest one.
 * Packing: blr_posterior_ragged_*'s, as for blr_marginals_ragged_* above (offsets: host array, B + 1 entries, violation -6); y and a
 * diagonal s are read at + offsets[b], isotropic s at b*strides; dense noise is an argument error.
 * State (mw + b*stridemw, T + b*strideT) as blr_posterior_ragged_* writes it: T upper, only its upper triangle is read; NOT modified.
 * The formulas, the NaN rule and the "loo_degenerate" statistic are those of blr_loo_batched_*.
 * Outputs: loo_mean, loo_var, loo_logpdf are packed -- element n of regressor b at index offsets[b] + n, no strides; loo_total[B]
 * and info[B] are per regressor.  Any of the four may be NULL; with loo_total requested and loo_logpdf NULL the log densities go
 * through handle workspace.  info rule and order unchanged: T has a non-positive diagonal entry j -> j, else the first non-positive
 * s_i -> i, for diagonal noise counted WITHIN the regressor's slice; the outputs (loo_total included) of a regressor with info != 0
 * are left untouched; the call still returns 0.  N_b = 0 writes nothing per observation, loo_total[b] = 0 and info[b] is the state's
 * status.  B = 0 is a no-op.  The argument checks come before the handle's: a NULL handle with valid arguments returns -1.
 * Kernels, work items, workspace, the async rule and the D > 128 route (blr_loo_batched_* with B = 1 per regressor; synchronises):
 * as blr_marginals_ragged_*; the tile loads also fetch y_n and the double-precision epilogue runs at the store.
 * Bit promises (to this entry point itself): bit-reproducible from call to call; the bits of regressor b are those of this entry
 * point with B = 1 on its slice -- independent of B, of the other regressors' data and counts, of any permutation of the batch, of
 * the chunking and of how a regressor is cut into work items; loo_total[b] is a fixed-order sum that depends on N_b only; the bits
 * of one output do not depend on which other outputs are requested; host and device memspace give the same bits; no float
 * atomics.  NOT promised: bit-equality with blr_loo_batched_*.
 * _f32: X, y, s, mw, T, loo_mean, loo_var are float; loo_logpdf and loo_total stay double. */
int blr_loo_ragged_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                       const int64_t* offsets, /* HOST array of B + 1 entries in both memspaces */
                       const double* X, int64_t ldx, const double* y,
                       int noise_kind, const double* s, int64_t strides,
                       const double* mw, int64_t stridemw, const double* T, int64_t ldt, int64_t strideT,
                       double* loo_mean, double* loo_var, double* loo_logpdf, double* loo_total, int32_t* info);
int blr_loo_ragged_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                       const int64_t* offsets, /* HOST array of B + 1 entries in both memspaces */
                       const float* X, int64_t ldx, const float* y,
                       int noise_kind, const float* s, int64_t strides,
                       const float* mw, int64_t stridemw, const float* T, int64_t ldt, int64_t strideT,
                       float* loo_mean, float* loo_var, double* loo_logpdf, double* loo_total, int32_t* info);

/* ---- exact LEAVE-FOLD-OUT (K-fold) predictives of regressors with UNEQUAL observation counts in one call -------------------------
 * Replaces: reference src/bayesian_linear_regression.jl:55-58 (logpdf) applied to each held-out FOLD given the rest, under a map
 * over fxs of different lengths -- blr_kfold_batched_* once per regressor (padding to the longest regressor is no alternative here:
 * it changes the folds).
 * Packing: blr_posterior_ragged_*'s, as for blr_loo_ragged_* above (offsets: host array, B + 1 entries, violation -6); y and a
 * diagonal s are read at + offsets[b], isotropic s at b*strides; dense noise is an argument error.
 * State (mw + b*stridemw, T + b*strideT) as blr_posterior_ragged_* writes it: T upper, only its upper triangle is read; NOT modified.
 * Folds: regressor b has the folds [f F, min((f + 1) F, N_b)) of ITS OWN slice, nfolds_b = ceil(N_b / F); F > N_b gives one fold.
 * 1 <= F <= 64.  The formulas, the NaN rule and the "kfold_degenerate" statistic are those of blr_kfold_batched_*.
 * Outputs: kf_mean and kf_var are packed by observations -- element n of regressor b at index offsets[b] + n; kf_logpdf is packed by
 * FOLDS -- fold f of regressor b at index fold_offsets[b] + f, fold_offsets[0] = 0, fold_offsets[b + 1] = fold_offsets[b] +
 * nfolds_b (blr_kfold_ragged_fold_offsets below computes the table; kf_logpdf holds fold_offsets[B] doubles); kf_total[B] and
 * info[B] are per regressor.  Any of the four may be NULL; with kf_total requested and kf_logpdf NULL the log densities go through
 * handle workspace.  info rule and order as blr_kfold_batched_*: T has a non-positive diagonal entry j -> j, else the first
 * non-positive s_i -> i, for diagonal noise counted WITHIN the regressor's slice; the outputs (kf_total included) of a regressor
 * with info != 0 are left untouched; the call still returns 0.  N_b = 0 writes nothing per observation or fold, kf_total[b] = 0
 * and info[b] is the state's status.  B = 0 is a no-op that touches nothing.
 * Argument errors (negative position; checked before the handle, so a NULL handle with valid arguments returns -1): memspace -2;
 * layout -3; B outside 0..2^30 -4; D outside 1..8192 -5; offsets NULL, offsets[0] < 0, decreasing, a count above 2^30 -- or, at
 * D > 128, above 16384 -- -6; F outside 1..64 -7; X NULL with observations -8; ldx < D (ColVecs) or < max(offsets[B], 1) (RowVecs)
 * -9; y NULL with observations -10; noise_kind dense -11; s NULL with observations -12; strides < 0 -13; mw NULL -14; stridemw < 0
 * -15; T NULL -16; ldt < D -17; strideT < 0 -18; info NULL -23.
 * D <= 128 (csrc/blr_kfold_ragged.hpp, csrc/blr_kfold_ragged_plan.hpp), per chunk of regressors (at most 65535, 256
 * MiB of images, 256 MiB of rows of Z but never fewer than one regressor, option MAX_CHUNK; blr_get_stat "last_chunks"): the status
 * and the triangular inverse image once per regressor; one workgroup per work item of blr_loo_ragged_*'s table (option RAGGED_ITEM)
 * whitens the item's observations, z_n = T^-T x_n and x_n'mw, into handle workspace, packed as the observations are, reading X once;
 * then a flat grid of one workgroup per pack of floor(64 / F) consecutive folds of ONE regressor runs blr_kfold_batched_*'s fold
 * body; then the totals.  The flat grid holds fewer than 2^24 packs: only ONE regressor of more than 2^24 floor(64 / F) F
 * observations (above 5.5e8, F >= 33) exceeds that, and the call then fails with the launch's HIP runtime error (<= -1000), as
 * blr_kfold_batched_* does at such an N.  offsets, the pack and fold tables and the items (24 bytes per regressor, 12 per item) are uploaded to the
 * handle's workspace (counted by blr_get_stat "workspace_bytes", freed by blr_release_workspace).
 * Bit promises (D <= 128): EVERY output of regressor b -- kf_mean, kf_var, its folds of kf_logpdf and kf_total[b] -- is bit for bit
 * what blr_kfold_batched_* with B = 1 writes on that slice with the same F.  Hence the bits are independent of B, of the other
 * regressors' data and counts, of any permutation of the batch, of the chunking (option MAX_CHUNK), of how a regressor is cut into
 * work items (option RAGGED_ITEM) and of which outputs are requested; host and device memspace give the same bits; results are
 * bit-reproducible from call to call; no float atomics.
 * Async handle, device memspace: the call only enqueues kernels, but the upload of the tables drains the handle's stream first (it
 * may block the host); the library is finished with the caller's offsets array when the call returns.
 * D > 128: correct, not fast -- one regressor after the other through blr_kfold_batched_* with B = 1; the call synchronises
 * whatever the handle's async flag says.
 * _f32: X, y, s, mw, T, kf_mean, kf_var are float; kf_logpdf and kf_total stay double. */
int blr_kfold_ragged_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                         const int64_t* offsets, /* HOST array of B + 1 entries in both memspaces */
                         int64_t F, const double* X, int64_t ldx, const double* y,
                         int noise_kind, const double* s, int64_t strides,
                         const double* mw, int64_t stridemw, const double* T, int64_t ldt, int64_t strideT,
                         double* kf_mean, double* kf_var, double* kf_logpdf, double* kf_total, int32_t* info);
int blr_kfold_ragged_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                         const int64_t* offsets, /* HOST array of B + 1 entries in both memspaces */
                         int64_t F, const float* X, int64_t ldx, const float* y,
                         int noise_kind, const float* s, int64_t strides,
                         const float* mw, int64_t stridemw, const float* T, int64_t ldt, int64_t strideT,
                         float* kf_mean, float* kf_var, double* kf_logpdf, double* kf_total, int32_t* info);
/* fold_offsets[B + 1] of blr_kfold_ragged_*: host arithmetic only -- no handle, no device.  What callers size kf_logpdf with
 * (fold_offsets[B] doubles).  Argument errors at the positions of blr_kfold_ragged_*: B -4, offsets -6, F -7; fold_offsets NULL
 * -21 (the output it sizes).  B = 0 writes fold_offsets[0] = 0. */
int blr_kfold_ragged_fold_offsets(int64_t B, const int64_t* offsets, int64_t F, int64_t* fold_offsets /* HOST, B + 1 entries */);

/* ---- exact LEAVE-FOLD-OUT (K-fold) predictives for LARGE folds of regressors with UNEQUAL observation counts in one call ---------
 * Replaces: reference src/bayesian_linear_regression.jl:55-58 (logpdf) applied to each held-out FOLD given the rest, under a map
 * over fxs of different lengths with K folds EACH -- blr_kfold_large_batched_* once per regressor: K folds on unequal counts mean a
 * fold size per regressor, F_b = ceil(N_b / K), usually far above the 64 of blr_kfold_ragged_* (padding changes the folds).
 * Packing, state, noise: exactly those of blr_kfold_ragged_* above (offsets: host array, B + 1 entries; y and a diagonal s are read
 * at + offsets[b], isotropic s at b*strides; dense noise is an argument error; T upper, only its triangle is read; NOT modified).
 * Folds: regressor b has the folds [f F_b, min((f + 1) F_b, N_b)) of ITS OWN slice with F_b = fold_sizes[b] >= 1 (host array, B
 * entries); F_b > N_b gives one fold; nfolds_b = ceil(N_b / F_b) <= 1024.  blr_kfold_large_ragged_fold_sizes below computes
 * F_b = max(1, ceil(N_b / K)).
 * Outputs: kf_mean and kf_var are packed by observations -- element n of regressor b at index offsets[b] + n; kf_logpdf is packed by
 * FOLDS -- fold f of regressor b at index fold_offsets[b] + f (blr_kfold_large_ragged_fold_offsets below computes the table;
 * kf_logpdf holds fold_offsets[B] doubles); kf_total[B] and info[B] are per regressor.  Any of the first four may be NULL; with
 * kf_total requested and kf_logpdf NULL the log densities go through handle workspace.
 * The formulas and the precision, the NaN rule, the "kfold_degenerate" statistic, the info rule and its order and "the outputs of a
 * regressor with info != 0 are left untouched" are those of blr_kfold_large_batched_* (its block below); for diagonal noise the index
 * i of a non-positive s_i is counted WITHIN the regressor's slice, as in blr_kfold_ragged_*.
 * N_b = 0 writes nothing per observation or fold, kf_total[b] = 0 and info[b] is the state's status.  B = 0 is a no-op that touches
 * nothing.  1 <= D <= 128, as blr_kfold_large_batched_*.
 * Argument errors (negative position; checked before the handle, so a NULL handle with valid arguments returns -1): memspace -2;
 * layout -3; B outside 0..2^30 -4; D outside 1..128 -5; offsets NULL, offsets[0] < 0, decreasing, a count above 2^30 -6; fold_sizes
 * NULL with B > 0, an entry < 1, or ceil(N_b / F_b) > 1024 -7; X NULL with observations -8; ldx < D (ColVecs) or
 * < max(offsets[B], 1) (RowVecs) -9; y NULL with observations -10; noise_kind dense -11; s NULL with observations -12; strides < 0
 * -13; mw NULL -14; stridemw < 0 -15; T NULL -16; ldt < D -17; strideT < 0 -18; info NULL -23.
 * Route (csrc/blr_kfold_large_ragged.hpp, csrc/blr_kfold_large_ragged_plan.hpp): the launch list of
 * blr_kfold_large_batched_* per chunk of regressors with flat grids driven by host-planned tables -- one workgroup per (regressor,
 * fold, column block) for the statistics, per fold for the factors, per (regressor, fold, tile group) for the predictions; the
 * kernels run the bodies the equal-count kernels run.  Chunks: consecutive regressors whose statistics, factors and images stay
 * within 256 MiB each, at most 65535, never fewer than one, option MAX_CHUNK; blr_get_stat "last_chunks".  X is read twice.
 * offsets, the fold table, the records (40 bytes per regressor) and the items (16 bytes each) are uploaded to the handle's workspace
 * (counted by blr_get_stat "workspace_bytes", freed by blr_release_workspace).
 * Bit promises: EVERY output of regressor b -- kf_mean, kf_var, its folds of kf_logpdf and kf_total[b] -- is bit for bit what
 * blr_kfold_large_batched_* with B = 1, N = N_b, F = F_b writes on that slice.  Hence the bits are independent of B, of the other
 * regressors' data, counts and fold sizes, of any permutation of the batch, of the chunking (option MAX_CHUNK) and of which outputs
 * are requested; host and device memspace give the same bits; results are bit-reproducible from call to call; no float atomics.
 * Async handle, device memspace: the call only enqueues kernels, but the upload of the tables drains the handle's stream first (it
 * may block the host); the library is finished with the caller's offsets and fold_sizes arrays when the call returns.
 * _f32: X, y, s, mw, T, kf_mean, kf_var are float; kf_logpdf and kf_total stay double. */
int blr_kfold_large_ragged_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                               const int64_t* offsets,    /* HOST array of B + 1 entries in both memspaces */
                               const int64_t* fold_sizes, /* HOST array of B entries in both memspaces */
                               const double* X, int64_t ldx, const double* y,
                               int noise_kind, const double* s, int64_t strides,
                               const double* mw, int64_t stridemw, const double* T, int64_t ldt, int64_t strideT,
                               double* kf_mean, double* kf_var, double* kf_logpdf, double* kf_total, int32_t* info);
int blr_kfold_large_ragged_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                               const int64_t* offsets,    /* HOST array of B + 1 entries in both memspaces */
                               const int64_t* fold_sizes, /* HOST array of B entries in both memspaces */
                               const float* X, int64_t ldx, const float* y,
                               int noise_kind, const float* s, int64_t strides,
                               const float* mw, int64_t stridemw, const float* T, int64_t ldt, int64_t strideT,
                               float* kf_mean, float* kf_var, double* kf_logpdf, double* kf_total, int32_t* info);
/* The two tables of blr_kfold_large_ragged_*: host arithmetic only -- no handle, no device.
 * fold_sizes[b] = max(1, ceil(N_b / K)): K folds per regressor (N_b < K: folds of one; N_b = 0: 1, no fold).  Argument errors: B -4
 * and offsets -6 as in blr_kfold_large_ragged_*; K outside 1..1024 -3 (its own position); fold_sizes NULL with B > 0 -7.
 * fold_offsets[0] = 0, fold_offsets[b + 1] = fold_offsets[b] + nfolds_b: what callers size kf_logpdf with.  Argument errors at the
 * positions of blr_kfold_large_ragged_*: B -4, offsets -6, fold_sizes -7; fold_offsets NULL -21 (the output it sizes). */
int blr_kfold_large_ragged_fold_sizes(int64_t B, const int64_t* offsets, int64_t K, int64_t* fold_sizes /* HOST out, B entries */);
int blr_kfold_large_ragged_fold_offsets(int64_t B, const int64_t* offsets, const int64_t* fold_sizes,
                                        int64_t* fold_offsets /* HOST out, B + 1 entries */);

/* ---- S target columns per regressor in one call: the batched multi-output posterior ---------------------------------
 * Replaces: reference src/bayesian_linear_regression.jl:55-58 (logpdf), :60-69 (posterior) and :72-89 (shared quantities) under a
 * map over fxs with MATRIX targets -- which blr_posterior_batched_* serves only by S calls with the y pointer stepped by one
 * column (X read S times, the Gram matrix formed and factorised S times) and blr_logpdf_multi_* only for one data set, without the
 * factor.
 * Regressor b reads X + b*strideX, Y + b*strideY (N x S column-major, ldY >= N), s + b*strides, mw + b*stridemw, Lw + b*strideLw; a
 * stride of 0 shares an input (strideX = 0 and strideY = 0 included).  Column s of regressor b gets exactly what
 * blr_posterior_batched_* gives for (X_b, Y_b[:, s], s_b, mw_b, Lw_b): its mean at mw_post + b*stride_mwpost + s*ldmp (D x S per
 * regressor, ldmp >= D), its evidence at logpdf[b*stride_lp + s] (double).  T_post (the upper factor) and Lw_post do not depend on
 * the column: ONE of each per regressor, written as blr_posterior_batched_* writes them.  info[B]: one status per regressor for the
 * shared factorisation, with that entry point's LAPACK codes; when info[b] != 0 every mean and the factor of that regressor are left
 * untouched and all S of its evidences are NaN.  The call returns 0 when the launches succeeded.  Any output may be NULL.
 * Isotropic or diagonal noise (dense noise: argument error), all three prior kinds, both layouts of X, both memspaces.  Aliasing an
 * output with an input is not supported: mw_post == mw or T_post == Lw is an argument error (the columns after the first still need
 * the prior mean).  Output strides that overlap for B > 1 are argument errors: stride_mwpost < ldmp*S, stride_lp < S, and the
 * T_post / Lw_post rules of blr_posterior_batched_*.  The argument checks come before the handle's.  B = 0 or S = 0 is a no-op;
 * N = 0 is allowed (every column's mean is the prior mean, its evidence 0).  Limits: 1 <= D <= 8192, S <= 2^20, N <= 2^30.
 * D <= 128 (csrc/blr_multi.hpp).  Step 1: column 0 of every regressor goes through the dispatch of
 * blr_posterior_batched_*, unchanged -- int8-sliced, one-wave or fused kernel, whatever the shape gets there (blr_last_route names
 * it); the factor goes to T_post, or to handle workspace when T_post is NULL (B D^2 elements, counted by "workspace_bytes", freed
 * by blr_release_workspace).  Step 2: ONE launch of multi_cols_kernel over regressors x column passes (63 further columns per pass)
 * streams X once per pass: residuals of all its columns, b_s = X S^-1 (y_s - X'mw) on the fp64 / fp32 matrix cores, q_s in double;
 * then the two triangular solves against the finished factor held as a packed triangle in LDS, and
 *   logpdf_s = logpdf_0 + (q_0 - |u_0|^2) / 2 - (q_s - |u_s|^2) / 2      (u_s = T^-T b_s; the log-determinants are column 0's).
 * The launch count does not depend on B.  An async handle in device memspace only enqueues; column 0's status is read on the device.
 * D > 128: correct, not fast -- one regressor after the other, column 0 through the pipeline of blr_posterior_batched_*, the further
 * columns through that of blr_logpdf_multi_*; the call synchronises whatever the handle's async flag says.
 * Numerics: bit-reproducible from call to call; the bits of a regressor do not depend on B or on its position; for s >= 1 they do
 * not depend on S, on the column's position or on the other columns' data.  Column 0, T_post, Lw_post and info are bit for bit what
 * blr_posterior_batched_* writes on the same handle for (X, Y[:, 0]): with S = 1 the call IS that entry point.  Columns s >= 1 hold
 * the accuracy stated there for the route column 0 took (the factor is the same; their own products are fp64 / fp32 as the element
 * type says, never int8).
 * _f32: X, Y, s, mw, Lw, mw_post, T_post, Lw_post are float; logpdf stays double. */
int blr_posterior_multi_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S,
                                    const double* X, int64_t ldx, int64_t strideX,
                                    const double* Y, int64_t ldY, int64_t strideY,
                                    int noise_kind, const double* s, int64_t strides,
                                    int prior_kind, const double* mw, int64_t stridemw,
                                    const double* Lw, int64_t ldl, int64_t strideLw,
                                    double* mw_post, int64_t ldmp, int64_t stride_mwpost,
                                    double* T_post, int64_t ldt, int64_t strideT,
                                    double* Lw_post, int64_t ldlp, int64_t strideLp,
                                    double* logpdf, int64_t stride_lp, int32_t* info);
int blr_posterior_multi_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S,
                                    const float* X, int64_t ldx, int64_t strideX,
                                    const float* Y, int64_t ldY, int64_t strideY,
                                    int noise_kind, const float* s, int64_t strides,
                                    int prior_kind, const float* mw, int64_t stridemw,
                                    const float* Lw, int64_t ldl, int64_t strideLw,
                                    float* mw_post, int64_t ldmp, int64_t stride_mwpost,
                                    float* T_post, int64_t ldt, int64_t strideT,
                                    float* Lw_post, int64_t ldlp, int64_t strideLp,
                                    double* logpdf, int64_t stride_lp, int32_t* info);

/* single regressor, host pointers; returns info (see "Return codes") */
int blr_posterior_f64(blr_handle* h, int layout, int64_t D, int64_t N, const double* X, int64_t ldx,
                      const double* y, int noise_kind, const double* s,
                      int prior_kind, const double* mw, const double* Lw, int64_t ldl,
                      double* mw_post, double* T_post, int64_t ldt, double* Lw_post, int64_t ldlp,
                      double* logpdf);
int blr_posterior_f32(blr_handle* h, int layout, int64_t D, int64_t N, const float* X, int64_t ldx,
                      const float* y, int noise_kind, const float* s,
                      int prior_kind, const float* mw, const float* Lw, int64_t ldl,
                      float* mw_post, float* T_post, int64_t ldt, float* Lw_post, int64_t ldlp,
                      double* logpdf);

/* ---- marginal stream: replaces mean (:33), var (:40-43), mean_and_var (:47) --------------------
 *   mean_n = x_n' mw          var_n = |Uw^-T x_n|^2 + Sy_nn
 * mean or var may be NULL (mean-only = evaluating a function sample, sampling_functions.jl:17-19).
 */
int blr_marginals_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,
                              const double* X, int64_t ldx, int64_t strideX,
                              int noise_kind, const double* s, int64_t strides,
                              int prior_kind, const double* mw, int64_t stridemw,
                              const double* Lw, int64_t ldl, int64_t strideLw,
                              double* mean, int64_t stridemean, double* var, int64_t stridevar,
                              int32_t* info);
int blr_marginals_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,
                              const float* X, int64_t ldx, int64_t strideX,
                              int noise_kind, const float* s, int64_t strides,
                              int prior_kind, const float* mw, int64_t stridemw,
                              const float* Lw, int64_t ldl, int64_t strideLw,
                              float* mean, int64_t stridemean, float* var, int64_t stridevar,
                              int32_t* info);

/* ---- S mean columns and one variance per input: marginals of the batched multi-output posterior -------------------
 * Replaces: reference src/bayesian_linear_regression.jl:33 (mean), :40-43 (var) and :47 (mean_and_var) under a map over fxs whose
 * regressors come from matrix targets -- the S column posteriors blr_posterior_multi_batched_* returns per regressor share one
 * factor, which blr_marginals_batched_* serves only by S calls (X read S times, the triangular work redone unless var is NULL on
 * S - 1 of them) and blr_apply_weights_* only for one regressor, without the variance.
 * Regressor b reads X + b*strideX, s + b*strides, M + b*strideM (D x S column-major, ldm >= D: exactly the mw_post block of
 * blr_posterior_multi_batched_*, ldmp / stride_mwpost) and Lw + b*strideLw; a stride of 0 shares an input (strideX = 0 -- one
 * candidate set -- and strideM = 0 included).
 *   mean[b*stridemean + n + c*ldmean] = x_n' M_b[:, c]           (N x S column-major per regressor, ldmean >= N; :33 per column)
 *   var[b*stridevar + n]              = |U_b^-T x_n|^2 + Sy_nn    (:40-43; one per input and regressor: it does not depend on the column)
 * mean or var may be NULL; with var == NULL, s and Lw may be NULL.  S = 0 computes var only (M and mean are ignored).  No-ops
 * returning 0: B = 0, N = 0, S = 0 with var == NULL.  Isotropic or diagonal noise (dense noise: argument error), all three prior
 * kinds (a dense prior is factorised once per regressor, a diagonal one needs no factor), both layouts of X with any ldx, both
 * memspaces.  info[B]: 0, or the LAPACK code of a dense prior that is not positive definite -- the outputs of that regressor are
 * then left untouched and the call still returns 0.  Argument errors are the negative position of the offending argument and are
 * checked before the handle (a NULL handle with valid arguments returns -1); output strides that overlap for B > 1 are argument
 * errors: stridemean < ldmean*S, stridevar < N.  Limits: 1 <= D <= 8192, N <= 2^30, 0 <= S <= 2^20.
 * D <= 128 (csrc/blr_marg_multi.hpp): the triangular inverse of every factor once per regressor (the image kernel of
 * blr_marginals_batched_*), then ONE launch of marginals_cols_kernel per chunk of regressors (at most 65535, images within 256 MiB)
 * over (column passes x groups of 64-input tiles, regressors); the launch count does not depend on S, and on B only through the
 * chunks.  A pass takes 16 columns of M, held in registers as matrix-core operands; the tile of inputs sits in LDS as rows; X is
 * streamed once per pass and var is produced by pass 0 only.  An async handle in device memspace only enqueues.
 * D > 128: correct, not fast -- var through the route of blr_marginals_batched_* with mean = NULL for the batch, the means one
 * regressor after the other through the product of blr_apply_weights_*; the call synchronises whatever the handle's async flag says.
 * Numerics: mean and var hold the bounds of blr_marginals_batched_* against the fp64 reference (rtol = atol = 1e-10 in fp64, 2e-4 in
 * fp32 on well-conditioned priors); the mean is a matrix-core product here, so no bit-equality with that entry point is promised.
 * Promised: results are bit-reproducible from call to call; the bits of regressor b do not depend on B or on its position in the
 * batch; the bits of column c do not depend on S, on c's position (pass included) or on the other columns' data; the bits of var do
 * not depend on S or on whether mean is requested; host and device memspace give the same bits.
 * _f32: X, s, M, Lw, mean, var are float. */
int blr_marginals_multi_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S,
                                    const double* X, int64_t ldx, int64_t strideX,
                                    int noise_kind, const double* s, int64_t strides,
                                    int prior_kind, const double* M, int64_t ldm, int64_t strideM,
                                    const double* Lw, int64_t ldl, int64_t strideLw,
                                    double* mean, int64_t ldmean, int64_t stridemean,
                                    double* var, int64_t stridevar,
                                    int32_t* info);
int blr_marginals_multi_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S,
                                    const float* X, int64_t ldx, int64_t strideX,
                                    int noise_kind, const float* s, int64_t strides,
                                    int prior_kind, const float* M, int64_t ldm, int64_t strideM,
                                    const float* Lw, int64_t ldl, int64_t strideLw,
                                    float* mean, int64_t ldmean, int64_t stridemean,
                                    float* var, int64_t stridevar,
                                    int32_t* info);

/* ---- joint predictive covariance of a batch of regressors: mean and the full N x N covariance per regressor ------------------------
 * Replaces: reference src/bayesian_linear_regression.jl:33 (mean), :35-38 (cov) and :45 (mean_and_cov) under a map over fxs -- until
 * now a loop of blr_mean_and_cov_* calls: one regressor per call, a drain of the stream per call, D and N padded to 128 on the
 * large-D tall-matrix route, temporaries allocated and freed per call.
 * Regressor b reads X + b*strideX, s + b*strides, mw + b*stridemw and Lw + b*strideLw; a stride of 0 shares an input (strideX = 0 --
 * one candidate set for all regressors -- and strideLw = 0 included).
 *   mean[b*stridemean + n] = x_n' mw_b                                                        (:33)
 *   C + b*strideC          = X_b' Lw_b^-1 X_b + Sigma_y, the FULL symmetric N x N matrix, column-major, ldc >= N   (:35-38, :45)
 * mean may be NULL (mw may then be NULL); C may be NULL -- a mean-only call: s and Lw are then not read and every status is 0.
 * Noise: ISOTROPIC (s is one variance), DIAGONAL (s[N]) or DENSE (N x N, lds >= N, upper triangle read, as blr_mean_and_cov_*
 * takes it; lds is ignored for the other kinds).  All three prior kinds, both layouts of X with any ldx, both memspaces.
 * info[B]: 0, or k > 0 for a dense Lw_b that is not positive definite at leading minor k, or k > 0 for the first non-positive
 * diagonal entry k of an upper factor or a diagonal prior (the rule of blr_rand_batched_*); the outputs of that regressor are then
 * left untouched and the call still returns 0.  Argument errors are the negative position of the offending argument and are
 * checked before the handle (a NULL handle with valid arguments returns -1); outputs that overlap for B > 1 are argument errors:
 * stridemean < N, strideC < ldc*N.  No-ops returning 0: B = 0, N = 0, mean and C both NULL.  Limits: 1 <= D <= 8192, N <= 16384
 * (the bound of blr_mean_and_cov_*).
 * D <= 128 (csrc/blr_cov_batched.hpp): once per call a dense prior's factor per regressor and every status; then per
 * chunk of regressors the triangular inverse of every factor (the image kernel of blr_marginals_batched_*), ONE launch of
 * cov_whiten_kernel (groups of 64-input tiles, regressors: X is read once, z_n = U^-T x_n is formed once per input and kept as a row
 * of 16 ceil(D/16) elements in the handle's workspace, the mean comes from the same tile) and ONE launch of cov_tiles_kernel (tile
 * pairs i <= j, regressors: the 64 x 64 block Z_i Z_j' on the matrix cores, k = d ascending, + Sigma_y, stored as block (i, j) and as
 * its transpose).  The launch count depends on B only through the chunks.  A chunk holds at most 65535 regressors (grid.y), at most
 * 256 MiB of images (factor priors) and at most 256 MiB of Z rows, but never fewer than one regressor (16 MiB of Z at D = 128,
 * N = 16384 in fp64); handle option MAX_CHUNK caps it further and blr_get_stat "last_chunks" reports the count.  The workspace is the
 * handle's: counted by "workspace_bytes", freed by blr_release_workspace.  An async handle in device memspace only enqueues.
 * D > 128: correct, not fast -- one regressor after the other through the launches of blr_mean_and_cov_* into a staging matrix that
 * is copied to C only when the regressor's status is 0; the call synchronises per regressor whatever the handle's async flag says.
 * Numerics: against the fp64 reference on well-conditioned priors rtol 1e-9 / atol 1e-10 in fp64, rtol = atol = 2e-4 in fp32.
 * Promised: results are bit-reproducible from call to call; the bits of regressor b do not depend on B, on its position in the
 * batch, on the chunking or on the other regressors' data; host and device memspace give the same bits; C is exactly symmetric
 * (C[m, n] and C[n, m] carry the same bits: both are stored from one accumulator); the bits of C do not depend on whether mean is
 * requested.  No float atomics, every sum in a fixed order.  NOT promised: bit-equality with blr_mean_and_cov_* or with var of
 * blr_marginals_batched_* (the products run in a different order).
 * _f32: X, s, mw, Lw, mean, C are float. */
int blr_mean_and_cov_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,
                                 const double* X, int64_t ldx, int64_t strideX,
                                 int noise_kind, const double* s, int64_t lds, int64_t strides,
                                 int prior_kind, const double* mw, int64_t stridemw,
                                 const double* Lw, int64_t ldl, int64_t strideLw,
                                 double* mean, int64_t stridemean,
                                 double* C, int64_t ldc, int64_t strideC,
                                 int32_t* info);
int blr_mean_and_cov_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,
                                 const float* X, int64_t ldx, int64_t strideX,
                                 int noise_kind, const float* s, int64_t lds, int64_t strides,
                                 int prior_kind, const float* mw, int64_t stridemw,
                                 const float* Lw, int64_t ldl, int64_t strideLw,
                                 float* mean, int64_t stridemean,
                                 float* C, int64_t ldc, int64_t strideC,
                                 int32_t* info);

/* ---- draws: replaces rand (:49-53) and the weight draws of sampling_functions.jl:29,35,44 ------
 * The host keeps drawing the normals so its RNG stream is the reference's:
 *   Z1 = randn(rng, D, S) FIRST, then Z2 = randn(rng, N, S).
 *   W = mw .+ Uw \ Z1 ;  Y = X'W .+ sqrt.(s) .* Z2          (Y is N x S, ldy >= N)
 */
int blr_rand_f64(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S,
                 const double* X, int64_t ldx, int noise_kind, const double* s,
                 int prior_kind, const double* mw, const double* Lw, int64_t ldl,
                 const double* Z1, int64_t ldz1, const double* Z2, int64_t ldz2,
                 double* Y, int64_t ldy);
int blr_rand_f32(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S,
                 const float* X, int64_t ldx, int noise_kind, const float* s,
                 int prior_kind, const float* mw, const float* Lw, int64_t ldl,
                 const float* Z1, int64_t ldz1, const float* Z2, int64_t ldz2,
                 float* Y, int64_t ldy);
/*   Y = X'W for S GIVEN weight vectors W (D x S, ldw >= D): evaluation of S function samples at the inputs,
 *   replaces (s::BLRFunctionSample)(X) = ϕ(X)'s.w  (src/sampling_functions.jl:16-18) for a batch of samples; also the two
 *   large products of the reverse-mode rule of rand (README.md:56-60: W̄ = X Ȳ and X̄ = W Ȳ', both "apply" calls on
 *   re-interpreted layouts -- julia/BLRMI355X.jl rand_pullback).  Y is N x S, ldy >= N. */
int blr_apply_weights_f64(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S,
                          const double* X, int64_t ldx, const double* W, int64_t ldw, double* Y, int64_t ldy);
int blr_apply_weights_f32(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S,
                          const float* X, int64_t ldx, const float* W, int64_t ldw, float* Y, int64_t ldy);
/*   W = mw .+ Uw \ Z   (D x S) */
int blr_sample_weights_f64(blr_handle* h, int memspace, int64_t D, int64_t S,
                           int prior_kind, const double* mw, const double* Lw, int64_t ldl,
                           const double* Z, int64_t ldz, double* W, int64_t ldw);
int blr_sample_weights_f32(blr_handle* h, int memspace, int64_t D, int64_t S,
                           int prior_kind, const float* mw, const float* Lw, int64_t ldl,
                           const float* Z, int64_t ldz, float* W, int64_t ldw);

/* ---- draws from B regressors in one call: rand (:49-53) and the weight draws of sampling_functions.jl:27-49 under a map ----
 * For each regressor b (inputs at ptr + b*stride; a stride of 0 shares an input, e.g. one candidate set X or one prior):
 *   W_b = mw_b + U_b \ Z1_b         (D x S; U_b the upper factor of Lw_b, of whichever prior kind)
 *   Y_b = X_b' W_b + sqrt.(s_b) .* Z2_b   (N x S; the host's normals, as blr_rand_*)
 *   Z2 == NULL: noise-free function values Y_b = X_b' W_b (Thompson sampling, BLRFunctionSample evaluation at
 *     sampling_functions.jl:16-18); noise_kind and s are then ignored.
 *   W == NULL: the weights are not returned.  Y == NULL: weights only.  N == 0 is allowed (X may then be NULL).  S == 0: no-op.
 *   Output strides of B > 1 must not overlap: strideW >= ldw*S, strideY >= ldy*S (else the negative argument index).
 *   info[B]: 0, or k > 0 -- a dense Lw_b not positive definite at leading minor k, or the first non-positive diagonal entry k
 *   of an upper factor / Diagonal prior.  A failed regressor's outputs are left untouched and the call still returns 0.
 *   s is not checked (as blr_rand_*).  Both memspaces; DEVICE memspace in async mode only enqueues.
 * The bits of W_b and Y_b do not depend on B, on b's position or on the other regressors' data, and repeat from call to call.
 * D <= 128: [one batched Cholesky of a dense prior] + one launch of the weight solve, with the projection fused into it when
 *   N*S <= 512, else one more launch; the launch count does not depend on B.
 * D > 128 (up to 8192): one regressor after the other on the blr_sample_weights_* / blr_rand_* kernels -- correct, not fast,
 *   and it synchronises (the status of every regressor is needed on the host before the loop).
 */
int blr_rand_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S,
                         const double* X, int64_t ldx, int64_t strideX,
                         int noise_kind, const double* s, int64_t strides,
                         int prior_kind, const double* mw, int64_t stridemw,
                         const double* Lw, int64_t ldl, int64_t strideLw,
                         const double* Z1, int64_t ldz1, int64_t strideZ1,
                         const double* Z2, int64_t ldz2, int64_t strideZ2,
                         double* W, int64_t ldw, int64_t strideW,
                         double* Y, int64_t ldy, int64_t strideY,
                         int32_t* info);
int blr_rand_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S,
                         const float* X, int64_t ldx, int64_t strideX,
                         int noise_kind, const float* s, int64_t strides,
                         int prior_kind, const float* mw, int64_t stridemw,
                         const float* Lw, int64_t ldl, int64_t strideLw,
                         const float* Z1, int64_t ldz1, int64_t strideZ1,
                         const float* Z2, int64_t ldz2, int64_t strideZ2,
                         float* W, int64_t ldw, int64_t strideW,
                         float* Y, int64_t ldy, int64_t strideY,
                         int32_t* info);

/* ---- draws from a batched multi-output state: S column posteriors per regressor share one factor, R draws per column ---------------
 * Replaces: reference src/bayesian_linear_regression.jl:49-53 (rand) and src/sampling_functions.jl:16-49 (weight draws, function
 * samples) under a map over fxs whose regressors come from matrix targets -- until now S calls of blr_rand_batched_* with mw stepped
 * by a column: every call reads every factor again per (regressor, block of draws), reads X again and pays its own launches.
 * Regressor b reads X + b*strideX, s + b*strides, M + b*strideM (D x S column-major, ldm >= D: exactly the mw_post block of
 * blr_posterior_multi_batched_* and the M of the other multi entry points), Lw + b*strideLw, Z1 + b*strideZ1 (D x S*R, ldz1 >= D) and
 * Z2 + b*strideZ2 (N x S*R, ldz2 >= N); a stride of 0 shares an input (strideX = 0, strideLw = 0 and strideM = 0 included).  Its S
 * column posteriors are N(M_b[:, c], (U_b'U_b)^-1), U_b the upper factor of Lw_b under whichever prior kind.  R draws per column;
 * draw j = c*R + r (0 <= c < S, 0 <= r < R: the R draws of a column are contiguous):
 *   W[b*strideW + j*ldw + :] = M_b[:, c] + U_b \ Z1_b[:, j]                  (D x S*R, ldw >= D; :51)
 *   Y[b*strideY + j*ldy + :] = X_b' W_b[:, j] + sqrt.(s_b) .* Z2_b[:, j]     (N x S*R, ldy >= N; :52-53)
 * The host draws the normals, so its RNG stream stays the reference's (per column Z1_c FIRST, then Z2_c).
 *   Z2 == NULL: noise-free function values Y = X'W (sampling_functions.jl:16-18); noise_kind and s are then ignored.
 *   W == NULL: the weights are not returned.  Y == NULL: weights only (X may be NULL).  N == 0 is allowed.
 * No-ops returning 0: B = 0, S = 0, R = 0, W and Y both NULL.  Isotropic or diagonal noise (dense noise: argument error), all three
 * prior kinds, both layouts of X with any ldx, both memspaces.  s is not checked (as blr_rand_batched_*).
 * info[B]: 0, or k > 0 for a dense Lw_b that is not positive definite at leading minor k, or k > 0 for the first non-positive
 * diagonal entry k of an upper factor or a diagonal prior (the rule of blr_rand_batched_*); W and Y of that regressor are then left
 * untouched and the call still returns 0.  Argument errors are the negative position of the offending argument and are checked
 * before the handle (a NULL handle with valid arguments returns -1); ldm < D is -17; outputs that overlap for B > 1 are argument
 * errors: strideW < ldw*S*R (-30), strideY < ldy*S*R (-33).  Limits: 1 <= D <= 8192, N <= 2^30, S*R <= 2^20.
 * D <= 128 (csrc/blr_rand_multi.hpp): [one batched Cholesky of a dense prior], then per chunk of regressors ONE launch
 * of rand_cols_solve_kernel (passes of 16 draw columns x regressors: the status, the factor once into LDS as a packed triangle, the
 * back substitution of four columns per wave, + M[:, j / R]; W goes to the caller and, when Y is wanted, as matrix-core operand images
 * of 16 ceil(D/16) x 16 elements per pass into the handle's workspace) and, when Y is wanted, ONE launch of rand_cols_project_kernel
 * (groups of 64-input tiles x regressors, the regressor fastest when X is shared: a workgroup keeps its tile of X in LDS and loops
 * over the passes, so X is read once whatever S*R is; + sqrt(s_n) Z2[n, j] at the store).  The launch count does not depend on S or
 * R, and on B only through the chunks.  A chunk holds at most 65535 regressors (grid.y) and at most 256 MiB of operand images, but
 * never fewer than one regressor (1 GiB of images at D = 128, S*R = 2^20 in fp64); handle option MAX_CHUNK caps it further and
 * blr_get_stat "last_chunks" reports the count.  The workspace is the handle's: counted by "workspace_bytes", freed by
 * blr_release_workspace.  An async handle in device memspace only enqueues.
 * D > 128: correct, not fast -- column by column through the route of blr_rand_batched_* (mw = M + c*ldm; Z1, Z2, W, Y stepped by R
 * columns); the call synchronises whatever the handle's async flag says.
 * Numerics: against the fp64 reference on well-conditioned priors rtol 1e-10 / atol 1e-11 in fp64, 2e-4 max(1, max|ref|) in fp32.
 * Promised: results repeat bit for bit from call to call; the bits of regressor b do not depend on B, on b's position, on the
 * chunking or on the other regressors' data; the bits of draw (c, r) depend only on that regressor's X, s and factor and on M[:, c],
 * Z1[:, j], Z2[:, j] -- not on S, on R, on j's position (pass and slot included) or on the other columns and draws; host and device
 * memspace give the same bits; the bits of Y do not depend on whether W is requested.  No float atomics, every sum in a fixed order.
 * NOT promised: bit-equality with blr_rand_batched_* (the solve multiplies by reciprocal pivots and the projection runs on the
 * matrix cores).
 * _f32: X, s, M, Lw, Z1, Z2, W, Y are float. */
int blr_rand_multi_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, int64_t R,
                               const double* X, int64_t ldx, int64_t strideX,
                               int noise_kind, const double* s, int64_t strides,
                               int prior_kind, const double* M, int64_t ldm, int64_t strideM,
                               const double* Lw, int64_t ldl, int64_t strideLw,
                               const double* Z1, int64_t ldz1, int64_t strideZ1,
                               const double* Z2, int64_t ldz2, int64_t strideZ2,
                               double* W, int64_t ldw, int64_t strideW,
                               double* Y, int64_t ldy, int64_t strideY,
                               int32_t* info);
int blr_rand_multi_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, int64_t R,
                               const float* X, int64_t ldx, int64_t strideX,
                               int noise_kind, const float* s, int64_t strides,
                               int prior_kind, const float* M, int64_t ldm, int64_t strideM,
                               const float* Lw, int64_t ldl, int64_t strideLw,
                               const float* Z1, int64_t ldz1, int64_t strideZ1,
                               const float* Z2, int64_t ldz2, int64_t strideZ2,
                               float* W, int64_t ldw, int64_t strideW,
                               float* Y, int64_t ldy, int64_t strideY,
                               int32_t* info);

/* ---- random-Fourier basis (BASELINE config 5): phi(x) = scale * cos(Omega' x + phase) ---------------------
 * The reference's BasisFunctionRegressor takes any callable phi (src/basis_function_regression.jl:7-9,41) and ships
 * none; this is the feature map of config 5, applied on the device so Phi never crosses PCIe.
 *   Xin: Din x N column-major (ColVecs of the raw inputs), Omega: Din x D column-major, phase[D];
 *   Phi : D x N column-major (ldphi >= D).
 * blr_posterior_rff_* = features + fused inference in one call (Phi lives in the handle's workspace):
 * the remaining arguments are those of blr_posterior_batched_* with B = 1.  fp32 at D > 128 with Din <= 832 evaluates
 * the basis inside the Gram's operand pass (Phi never exists; blr_last_route ends in " (basis in planes pass)"); a wider
 * input (a conservative cap: that pass then stays within 64 KiB of LDS), fp64 and D <= 128 materialise Phi first.
 */
int blr_rff_features_f64(blr_handle* h, int memspace, int64_t Din, int64_t D, int64_t N,
                         const double* Xin, int64_t ldxin, const double* Omega, int64_t ldo, const double* phase,
                         double scale, double* Phi, int64_t ldphi);
int blr_rff_features_f32(blr_handle* h, int memspace, int64_t Din, int64_t D, int64_t N,
                         const float* Xin, int64_t ldxin, const float* Omega, int64_t ldo, const float* phase,
                         float scale, float* Phi, int64_t ldphi);
int blr_posterior_rff_f64(blr_handle* h, int memspace, int64_t Din, int64_t D, int64_t N,
                          const double* Xin, int64_t ldxin, const double* Omega, int64_t ldo, const double* phase,
                          double scale, const double* y, int noise_kind, const double* s,
                          int prior_kind, const double* mw, const double* Lw, int64_t ldl,
                          double* mw_post, double* T_post, int64_t ldt, double* Lw_post, int64_t ldlp,
                          double* logpdf, int32_t* info);
int blr_posterior_rff_f32(blr_handle* h, int memspace, int64_t Din, int64_t D, int64_t N,
                          const float* Xin, int64_t ldxin, const float* Omega, int64_t ldo, const float* phase,
                          float scale, const float* y, int noise_kind, const float* s,
                          int prior_kind, const float* mw, const float* Lw, int64_t ldl,
                          float* mw_post, float* T_post, int64_t ldt, float* Lw_post, int64_t ldlp,
                          double* logpdf, int32_t* info);

/* ---- gradient of the log marginal likelihood -------------------------------
 * The reverse-mode rule of logpdf(fx, y) (reference src/bayesian_linear_regression.jl:55-58): what Zygote derives from
 * the reference's Julia code (README.md:56-71, examples/nn-blr.jl:35-37) and a ccall-backed logpdf has to supply
 * itself (a ChainRules rrule in the shim).  One call = fused posterior + two MFMA sweeps per tile of inputs.
 *   logpdf[B]            the value itself
 *   dX                   dL/dX, SAME layout as X (lddx, stridedX)
 *   dy[N], ds[N]         dL/dy_n; dL/ds_n per observation (isotropic noise: the scalar gradient is their sum)
 *   dmw[D]               dL/dmw
 *   mw_post[D], Ainv     posterior mean and A^-1 = (Lw + X S X')^-1 (D x D, ldai): the caller forms
 *                        dL/dLw = -(m m' + Ainv - Lw^-1)/2 with m = mw_post - mw (D x D host work)
 * Any output except logpdf/info may be NULL.  Arguments up to strideLw are those of blr_posterior_batched_*, except that N >= 1
 * (N = 0 is an argument error).  A regressor with info[b] != 0 (as blr_posterior_batched_* reports it) gets logpdf[b] = NaN and
 * dmw = 0; its dX, dy, ds, mw_post and Ainv are left untouched -- on either device route; the call still returns 0.
 * mw_post must NOT alias mw here (the in-place form blr_posterior_batched_* allows): dmw is refined from mw_post - mw after the
 * posterior has been written (one step in double, dmw = P + Lw A^-1 (X S r - P) with P = Lw (mw_post - mw)). */
int blr_logpdf_grad_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,
                                const double* X, int64_t ldx, int64_t strideX, const double* y, int64_t stridey,
                                int noise_kind, const double* s, int64_t strides, int prior_kind, const double* mw,
                                int64_t stridemw, const double* Lw, int64_t ldl, int64_t strideLw, double* logpdf,
                                double* dX, int64_t lddx, int64_t stridedX, double* dy, int64_t stridedy, double* ds,
                                int64_t strideds, double* dmw, int64_t stridedmw, double* mw_post,
                                int64_t stride_mwpost, double* Ainv, int64_t ldai, int64_t strideAi, int32_t* info);
int blr_logpdf_grad_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N,
                                const float* X, int64_t ldx, int64_t strideX, const float* y, int64_t stridey,
                                int noise_kind, const float* s, int64_t strides, int prior_kind, const float* mw,
                                int64_t stridemw, const float* Lw, int64_t ldl, int64_t strideLw, double* logpdf,
                                float* dX, int64_t lddx, int64_t stridedX, float* dy, int64_t stridedy, float* ds,
                                int64_t strideds, float* dmw, int64_t stridedmw, float* mw_post,
                                int64_t stride_mwpost, float* Ainv, int64_t ldai, int64_t strideAi, int32_t* info);

/* ---- shared-X multi-output evidence -------------------------------------------
 * logpdf(fx, Y::AbstractMatrix) of the AbstractGPs secondary API (exercised through TestUtils at reference
 * test/bayesian_linear_regression.jl:7-9): the S columns of Y (N x S, ldY) share X, so the Gram matrix and its
 * Cholesky factor are formed ONCE; per column only X S (y_s - X'mw) (one D x N x S GEMM) and two triangular
 * solves remain.  logpdf[S]; mw_post (D x S, ldmp) optionally receives the posterior mean of every column
 * (NULL: skipped); info: one status for the shared factorisation (LAPACK semantics). */
int blr_logpdf_multi_f64(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const double* X,
                         int64_t ldx, const double* Y, int64_t ldY, int noise_kind, const double* s, int prior_kind,
                         const double* mw, const double* Lw, int64_t ldl, double* logpdf, double* mw_post, int64_t ldmp,
                         int32_t* info);
int blr_logpdf_multi_f32(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const float* X,
                         int64_t ldx, const float* Y, int64_t ldY, int noise_kind, const float* s, int prior_kind,
                         const float* mw, const float* Lw, int64_t ldl, double* logpdf, float* mw_post, int64_t ldmp,
                         int32_t* info);

/* ---- N-sharded single regressor ("one-exchange N-sharding") -------------------------
 * A regressor too large for one GPU's share of time (config 3) splits its N observations over ranks.  Everything the
 * update needs from the data is additive over column blocks:
 *   blr_gram_stats_*            per rank, on its columns: stats = (DP + 128) x DP column-major (lds >= DP + 128,
 *                               DP = 128 ceil(D/128)): lower triangle of X S X' in rows [0, DP), row DP = (X S (y - X'mw))';
 *                               scal[2] = { (y - X'mw)' S (y - X'mw), logdet Sigma_y } of the block.
 *   (host)                      ONE sum over ranks of `stats` and `scal` (RCCL all-reduce through torch.distributed /
 *                               MPI.jl) -- the only exchange.
 *   blr_posterior_from_stats_*  on every rank (redundant D x D work): adds the prior precision (dense or diagonal),
 *                               factorises, solves; outputs as blr_posterior_*.  `stats` is overwritten.
 * Device pointers only.  Works for any D (the large-D pipeline); N_total = observations over all ranks. */
int blr_gram_stats_f64(blr_handle* h, int layout, int64_t D, int64_t N, const double* X, int64_t ldx, const double* y,
                       int noise_kind, const double* s, const double* mw, double* stats, int64_t lds, double* scal);
int blr_gram_stats_f32(blr_handle* h, int layout, int64_t D, int64_t N, const float* X, int64_t ldx, const float* y,
                       int noise_kind, const float* s, const float* mw, float* stats, int64_t lds, double* scal);
int blr_posterior_from_stats_f64(blr_handle* h, int64_t D, int64_t N_total, double* stats, int64_t lds, const double* scal,
                                 int prior_kind, const double* mw, const double* Lw, int64_t ldl, double* mw_post,
                                 double* T_post, int64_t ldt, double* Lw_post, int64_t ldlp, double* logpdf, int32_t* info);
int blr_posterior_from_stats_f32(blr_handle* h, int64_t D, int64_t N_total, float* stats, int64_t lds, const double* scal,
                                 int prior_kind, const float* mw, const float* Lw, int64_t ldl, float* mw_post,
                                 float* T_post, int64_t ldt, float* Lw_post, int64_t ldlp, double* logpdf, int32_t* info);

/* ---- dense noise covariance and full predictive covariance -------------------------
 * reference src/bayesian_linear_regression.jl:79-82 (the general _cholesky(Sigma_y) branch of the shared quantities -- what
 * the reference's own toy problems use, test/test_utils.jl:7-8), :35-38 / :45 (cov, mean_and_cov), :52 (rand).
 * A dense Sigma_y (N x N, ldsy >= N, upper triangle read) is whitened away on the device: blocked Cholesky L L' = Sigma_y with
 * X and y carried through the panel solves (X L^-T, L^-1 y), then the ordinary update with unit noise; logpdf gets
 * -logdet(Sigma_y)/2.  N <= 16384.  Outputs as blr_posterior_*; info > 0: Sigma_y, Lw or Lw + X Sy^-1 X' not positive definite.
 *   blr_mean_and_cov_*   mean[N] (may be NULL) and C = X' Lw^-1 X + Sigma_y as the FULL symmetric N x N matrix (ldc >= N);
 *                        noise_kind ISOTROPIC / DIAGONAL / DENSE (s = the scalar, the N variances, or the N x N matrix with lds)
 *   blr_rand_dense_noise_*   Y = X'(mw + Uw \ Z1) + Us' Z2 with Us = chol(Sigma_y).U; RETURNS info (0, or k > 0) */
int blr_posterior_dense_noise_f64(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, const double* X, int64_t ldx,
                                  const double* y, const double* Sy, int64_t ldsy, int prior_kind, const double* mw,
                                  const double* Lw, int64_t ldl, double* mw_post, double* T_post, int64_t ldt, double* Lw_post,
                                  int64_t ldlp, double* logpdf, int32_t* info);
int blr_posterior_dense_noise_f32(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, const float* X, int64_t ldx,
                                  const float* y, const float* Sy, int64_t ldsy, int prior_kind, const float* mw,
                                  const float* Lw, int64_t ldl, float* mw_post, float* T_post, int64_t ldt, float* Lw_post,
                                  int64_t ldlp, double* logpdf, int32_t* info);
int blr_mean_and_cov_f64(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, const double* X, int64_t ldx,
                         int noise_kind, const double* s, int64_t lds, int prior_kind, const double* mw, const double* Lw,
                         int64_t ldl, double* mean, double* C, int64_t ldc, int32_t* info);
int blr_mean_and_cov_f32(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, const float* X, int64_t ldx,
                         int noise_kind, const float* s, int64_t lds, int prior_kind, const float* mw, const float* Lw,
                         int64_t ldl, float* mean, float* C, int64_t ldc, int32_t* info);
int blr_rand_dense_noise_f64(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const double* X,
                             int64_t ldx, const double* Sy, int64_t ldsy, int prior_kind, const double* mw, const double* Lw,
                             int64_t ldl, const double* Z1, int64_t ldz1, const double* Z2, int64_t ldz2, double* Y, int64_t ldy);
int blr_rand_dense_noise_f32(blr_handle* h, int memspace, int layout, int64_t D, int64_t N, int64_t S, const float* X,
                             int64_t ldx, const float* Sy, int64_t ldsy, int prior_kind, const float* mw, const float* Lw,
                             int64_t ldl, const float* Z1, int64_t ldz1, const float* Z2, int64_t ldz2, float* Y, int64_t ldy);

/* ---- rank-k update of a RESIDENT posterior state ----------------------------------------------
 * Replaces: reference test/bayesian_linear_regression.jl:49-70 ("repeated conditioning", posterior(f'1(X2, S2), y2)) and
 * src/bayesian_linear_regression.jl:93 (the posterior carries mw', Lw' forward; every further call re-derives :72-89 from
 * Lw' at O(D^3)).
 * State, updated IN PLACE: mw[B][D] and the upper factor T[B] (D x D, ldt, T'T = precision; the strictly-lower part is not
 * read and may be overwritten with zeros) -- exactly the (mw_post, T_post) pair blr_posterior_batched_* writes.
 * k new observations per regressor: X (D x k ColVecs / k x D RowVecs), y[k], isotropic or diagonal noise s.
 * logpdf[B] (may be NULL) = log p(y_k | state before the call), the evidence increment: summing it over successive calls
 * gives the evidence of all the data (chain rule).  info[B]: 0, or LAPACK-style i > 0 on BOTH routes, checked in the
 * reference's order (:78 prior, :79 noise, :86 posterior): T has a non-positive diagonal entry i (the state is not a Cholesky
 * factor), else s_i is not positive, else the leading minor of order i of the updated precision is not positive definite.
 * Routes (measured; BLR_MI355X_SWEEP=always|never at blr_create, or blr_set_option(h, "SWEEP", ...), overrides, "always" meaning D <= 128 and k <= 16):
 *   k <= 1, D <= 128 (and D > 64 or B < 256): one sweep of D Givens rotations over the factor held in LDS -- O(D^2),
 *     orthogonal transformations only; the state is untouched when info != 0;
 *   otherwise: the same state re-factored in place by blr_posterior_batched_* with the old factor entering as D
 *     pseudo-observations (cost independent of k; that entry point supports mw_post == mw and T_post == Lw for
 *     BLR_PRIOR_UPPER_FACTOR: every read of the old state completes before the first write).  The state is untouched
 *     when info != 0, at every D. */
int blr_update_factor_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, const double* X,
                          int64_t ldx, int64_t strideX, const double* y, int64_t stridey, int noise_kind, const double* s,
                          int64_t strides, double* mw, int64_t stridemw, double* T, int64_t ldt, int64_t strideT,
                          double* logpdf, int32_t* info);
int blr_update_factor_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, const float* X,
                          int64_t ldx, int64_t strideX, const float* y, int64_t stridey, int noise_kind, const float* s,
                          int64_t strides, float* mw, int64_t stridemw, float* T, int64_t ldt, int64_t strideT,
                          double* logpdf, int32_t* info);

/* ---- rank-k DOWNDATE of a resident posterior state: forget observations --------------------------------------------
 * Undoes: reference test/bayesian_linear_regression.jl:49-70 ("repeated conditioning"): the inverse of blr_update_factor_*.
 * Reports: src/bayesian_linear_regression.jl:55-58 (logpdf), for the REMOVED data given the data that remains.
 * Arguments exactly as blr_update_factor_* (memspace, layout, B, D, k, X / ldx / strideX, y / stridey, noise_kind / s /
 * strides, mw / stridemw, T / ldt / strideT, logpdf, info; a stride of 0 shares an input).  If the state (mw, T) is the
 * posterior given a data set that contains the k observations (X, y, s), it becomes, IN PLACE, the posterior without them:
 * T''T' = T'T - X S^-1 X' (T' upper with a positive diagonal) and T''T' mw' = T'T mw - X S^-1 y.
 * logpdf[B] (may be NULL) = log p(y_k | state after the call), in double: at k = 1 the exact leave-one-out predictive density;
 * update(X, y) followed by downdate(X, y) reports the same number twice, up to rounding.
 * info[B], checked in this order: T has a non-positive diagonal entry j (the update's code, and it wins), else s_i is not
 * positive -> i, else removing an observation leaves a precision that is not positive definite -> j, the leading minor of
 * that precision which fails, at the first observation (in order) whose removal fails.  On any info != 0 the state is
 * bit-for-bit untouched and logpdf is NaN.
 * Limits: 1 <= D <= 8192, any k >= 0 (k = 0 is a no-op), isotropic or diagonal noise (dense noise: argument error), host or
 * device memspace; an async handle returns after enqueue, as for the update.  Results are bit-reproducible and do not depend
 * on B or on a regressor's position in the batch.
 * Kernels (csrc/blr_downdate.hpp): per observation a forward solve, then D rotations applied column by column
 * (LINPACK dchdd), O(k D^2).  D <= 128: one workgroup per regressor with [T | u] in LDS; larger D: a row-major workspace copy
 * of the state in global memory, the rotations spread over several workgroups per regressor.  Option NO_DOWNDATE_LDS
 * (blr_set_option / BLR_MI355X_NO_DOWNDATE_LDS) forces the global-memory kernel at D <= 128. */
int blr_downdate_factor_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, const double* X,
                            int64_t ldx, int64_t strideX, const double* y, int64_t stridey, int noise_kind, const double* s,
                            int64_t strides, double* mw, int64_t stridemw, double* T, int64_t ldt, int64_t strideT,
                            double* logpdf, int32_t* info);
int blr_downdate_factor_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, const float* X,
                            int64_t ldx, int64_t strideX, const float* y, int64_t stridey, int noise_kind, const float* s,
                            int64_t strides, float* mw, int64_t stridemw, float* T, int64_t ldt, int64_t strideT,
                            double* logpdf, int32_t* info);

/* ---- update / DOWNDATE of resident states that received UNEQUAL numbers of observations, in one call ---------------------
 * Replaces: reference test/bayesian_linear_regression.jl:49-70 ("repeated conditioning", posterior(f'b(X_b, S_b), y_b)) under a map
 * over posteriors that each received a different number of observations -- most of them none: the step of an online or bandit
 * loop after a round of draws.  Without it the caller groups the regressors by count, gathers each group's states, calls
 * blr_update_factor_* / blr_downdate_factor_* once per distinct k and scatters the results back, or loops over B = 1 calls.
 * Packing of X, y and diagonal s: exactly blr_posterior_ragged_*'s.  offsets: HOST array of B + 1 non-decreasing entries in both
 * memspaces; regressor b owns observations [offsets[b], offsets[b+1]), k_b = their number (0 allowed; at most 2^30).  Isotropic
 * noise is read at s + b * strides; dense noise is an argument error.  State, updated IN PLACE: mw[B][D] at stridemw and the upper
 * factors T[B] (D x D, ldt) at strideT, with the stride rules of blr_update_factor_*; the strictly-lower part of T is never
 * read (the re-factorisation route overwrites it with zeros, as blr_update_factor_* does; the other routes leave it alone).
 * Per regressor the call means the equal-count entry point with B = 1, k = k_b on the regressor's slice:
 *   update:    logpdf[b] = log p(y_b | state before the call);   downdate: logpdf[b] = log p(y_b | state after the call);
 *   info[b]: the equal-count codes in the same order (factor, noise, posterior), observation indices counted inside the regressor's
 *   own slice (1-based).  info[b] != 0: the state of b is bit-for-bit untouched and logpdf[b] is NaN; the other regressors are not
 *   affected and the call returns 0.
 *   k_b = 0: the state keeps its bits and is not inspected, logpdf[b] = 0, info[b] = 0 (blr_update_multi_factor_*'s k = 0).
 * Every info[b] and every requested logpdf[b] (logpdf may be NULL) is written, idle regressors included, in both memspaces.
 * Returns 0 or -(position of the bad argument); the argument checks come before the handle's (a NULL handle with valid arguments:
 * -1), B = 0 is a no-op.  offsets is copied to the device with the plan's lists: the stream is drained once per call, and the
 * caller's offsets array is free when the call returns, on an async handle too.
 * Routes (csrc/blr_revise_ragged_plan.hpp).  The route of a regressor follows from (D, k_b, options) alone, never from
 * B or from the other regressors.  One workgroup per regressor with observations, longest first; idle regressors cost none.
 *   update, D <= 128:   k_b = 1: the Givens sweep of blr_update_factor_* (update_ragged_sweep_kernel); k_b >= 2: the state
 *     re-factored in place by blr_posterior_ragged_*'s kernel.  SWEEP=always: k_b <= 16 sweeps; SWEEP=never: every one re-factors.
 *   downdate, D <= 128: blr_downdate_factor_*'s LDS body for every k_b (downdate_ragged_kernel).
 *   D > 128, or a downdate under NO_DOWNDATE_LDS: correct, not fast -- the regressors with observations go one after the other
 *     through the equal-count entry point with B = 1; the call synchronises.
 *   Option MAX_CHUNK caps the regressors per launch; blr_get_stat "last_chunks" counts the launches of regressors with observations
 *   (0 when there is none), "ragged_sweep" / "ragged_refit" / "ragged_idle" the regressors on each route of the most recent call
 *   (a downdate counts its regressors under "ragged_sweep").
 * Bit promises.  Sweep route and downdate: regressor b has bit for bit what blr_update_factor_* (on a SWEEP=always handle) /
 * blr_downdate_factor_* with B = 1, k = k_b writes on its slice.  Re-factorisation route: the bits of blr_posterior_ragged_* with
 * BLR_PRIOR_UPPER_FACTOR in place (mw_post = mw, T_post = Lw = T) on that slice.  Either way independent of B, of a permutation of
 * the batch, of the other regressors' data and counts and of MAX_CHUNK; host and device memspace give the same bits; reproducible
 * from call to call; no float atomics.
 * Limits: 1 <= D <= 8192, isotropic or diagonal noise, single-output states. */
int blr_update_factor_ragged_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                                 const int64_t* offsets, /* HOST, B + 1 entries, both memspaces */
                                 const double* X, int64_t ldx, const double* y,
                                 int noise_kind, const double* s, int64_t strides,
                                 double* mw, int64_t stridemw, double* T, int64_t ldt, int64_t strideT,
                                 double* logpdf, int32_t* info);
int blr_update_factor_ragged_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                                 const int64_t* offsets, /* HOST, B + 1 entries, both memspaces */
                                 const float* X, int64_t ldx, const float* y,
                                 int noise_kind, const float* s, int64_t strides,
                                 float* mw, int64_t stridemw, float* T, int64_t ldt, int64_t strideT,
                                 double* logpdf, int32_t* info);
int blr_downdate_factor_ragged_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                                   const int64_t* offsets, /* HOST, B + 1 entries, both memspaces */
                                   const double* X, int64_t ldx, const double* y,
                                   int noise_kind, const double* s, int64_t strides,
                                   double* mw, int64_t stridemw, double* T, int64_t ldt, int64_t strideT,
                                   double* logpdf, int32_t* info);
int blr_downdate_factor_ragged_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D,
                                   const int64_t* offsets, /* HOST, B + 1 entries, both memspaces */
                                   const float* X, int64_t ldx, const float* y,
                                   int noise_kind, const float* s, int64_t strides,
                                   float* mw, int64_t stridemw, float* T, int64_t ldt, int64_t strideT,
                                   double* logpdf, int32_t* info);

/* ---- rank-k update / DOWNDATE of a resident MULTI-OUTPUT state: one factor, S mean columns ------------------------------
 * blr_update_multi_factor_* replaces: reference test/bayesian_linear_regression.jl:49-70 ("repeated conditioning") and
 * src/bayesian_linear_regression.jl:93 under MATRIX targets -- S calls of blr_update_factor_* on S private copies of the factor, or a
 * refit with blr_posterior_multi_batched_*.  blr_downdate_multi_factor_* is its inverse and reports :55-58 (logpdf) for the REMOVED
 * data given the data that remains, per column -- S calls of blr_downdate_factor_*.
 * State, updated IN PLACE: M (D x S column-major per regressor, ldm >= D, strideM) -- exactly the mw_post block of
 * blr_posterior_multi_batched_* and the M of blr_marginals_multi_batched_* -- and the ONE upper factor T[B] (D x D, ldt, T'T =
 * precision; only the upper triangle is read or written, as for blr_update_factor_*).
 * k observations per regressor: X (D x k ColVecs / k x D RowVecs, ldx), Y (k x S column-major, ldY >= k), isotropic or diagonal
 * noise s.  A stride of 0 shares an input (strideX, strideY, strides).
 * With W = X S^-1/2 the new precision T''T' = T'T +- W W' does not involve Y.  Column 0 and the factor are the single-column entry
 * point's; every further column c costs, with E_c = S^-1/2 (Y_c - X'm_c) against its mean before the call (upper sign: update),
 *   u_c = T'^-T (W E_c)    m_c' = m_c +- T'^-1 u_c    logpdf_c = -1/2 [k log 2pi + sum log s_i +- 2 sum_j log(T'_jj / T_jj) + |E_c|^2 -+ |u_c|^2].
 * logpdf[b * stride_lp + c] (double; may be NULL): update: log p(Y_c | state before the call); downdate: log p(Y_c | state after the
 * call) -- the contract of blr_update_factor_* / blr_downdate_factor_* per column.
 * info[B]: one status per regressor, the codes of the single-column entry point of the same direction, in its order.  When
 * info[b] != 0 all S means and the factor of regressor b are bit-for-bit untouched and its S evidences are NaN; the call returns 0.
 * S = 1 promise: column 0, T and info are bit for bit what blr_update_factor_* / blr_downdate_factor_* write on the same handle for
 * (X, Y[:, 0]), whatever S is (handle options SWEEP and NO_DOWNDATE_LDS included); with S = 1 the call IS that entry point.
 * Bit promises: the bits of a regressor do not depend on B or on its position in the batch; for c >= 1 the bits of a column do not
 * depend on S, on the column's position (pass included) or on the other columns' data; host and device memspace give the same bits;
 * repeated calls on restored state give the same bits.
 * Argument errors (negative position; checked before the handle, so a NULL handle with valid arguments returns -1): memspace,
 * layout, B, D, k, S out of range, dense noise (14), ldY < k (12), ldm < D (18), and for B > 1 strideM < ldm * S (19),
 * stride_lp < S (24) and the T rules of blr_update_factor_* (21, 22).  B = 0, S = 0 or k = 0 is a no-op returning 0; with k = 0 and
 * a non-NULL logpdf every evidence is 0 (info 0) and the state keeps its bits.
 * Limits: 1 <= D <= 8192, 0 <= S <= 2^20, 0 <= k <= 2^30, host or device memspace; an async handle in device memspace only
 * enqueues at D <= 128.
 * Kernels (csrc/blr_state_cols.hpp).  D <= 128: three launches (fp32: four) whatever B and S are -- the old diagonal
 * of T into the handle's workspace (state_diag_kernel; the log-determinant term; fp32 also the whole old factor, state_save_kernel,
 * B D^2 elements of workspace), the single-column call, then state_cols_kernel over (regressors, passes of 16 columns) with the
 * finished factor in LDS.  fp32: a column's mean is m_c +- T'^-1 u_c or the solution of A'm_c' = A m_c +- X S^-1 y_c (right-hand
 * side in double from the old factor), whichever solved vector is smaller: the error of the fp32 factor then enters times
 * min(|m_c' - m_c|, |m_c'|).  D > 128 is correct, not fast: column 0 through the large-D
 * update / downdate route (which may synchronise), the other columns one workgroup per (column, regressor) with T' read from global
 * memory. */
int blr_update_multi_factor_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, int64_t S,
                                const double* X, int64_t ldx, int64_t strideX, const double* Y, int64_t ldY, int64_t strideY,
                                int noise_kind, const double* s, int64_t strides, double* M, int64_t ldm, int64_t strideM,
                                double* T, int64_t ldt, int64_t strideT, double* logpdf, int64_t stride_lp, int32_t* info);
int blr_update_multi_factor_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, int64_t S,
                                const float* X, int64_t ldx, int64_t strideX, const float* Y, int64_t ldY, int64_t strideY,
                                int noise_kind, const float* s, int64_t strides, float* M, int64_t ldm, int64_t strideM,
                                float* T, int64_t ldt, int64_t strideT, double* logpdf, int64_t stride_lp, int32_t* info);
int blr_downdate_multi_factor_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, int64_t S,
                                  const double* X, int64_t ldx, int64_t strideX, const double* Y, int64_t ldY, int64_t strideY,
                                  int noise_kind, const double* s, int64_t strides, double* M, int64_t ldm, int64_t strideM,
                                  double* T, int64_t ldt, int64_t strideT, double* logpdf, int64_t stride_lp, int32_t* info);
int blr_downdate_multi_factor_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t k, int64_t S,
                                  const float* X, int64_t ldx, int64_t strideX, const float* Y, int64_t ldY, int64_t strideY,
                                  int noise_kind, const float* s, int64_t strides, float* M, int64_t ldm, int64_t strideM,
                                  float* T, int64_t ldt, int64_t strideT, double* logpdf, int64_t stride_lp, int32_t* info);

/* ---- exact LEAVE-ONE-OUT predictives of the observations a posterior state contains -----------------------------------
 * Replaces: a loop of blr_downdate_factor_* at k = 1 (then blr_update_factor_* to put the observation back) per observation,
 * and reference src/bayesian_linear_regression.jl:55-58 (logpdf) applied to each held-out point given the rest.
 * State (mw, T) as blr_posterior_batched_* writes it (mw_post, T_post) or a resident state holds it: T upper, only its upper
 * triangle is read; NOT modified.  It must be conditioned on a data set that contains the N observations (X, y, s); the
 * outputs are then, for every n, the predictive of y_n given everything else the state holds.  With A = T'T, mw' = mw:
 *   sigma2_n = x_n'A^-1 x_n,  m_n = x_n'mw',  r_n = y_n - m_n,  1 - h_n = (s_n - sigma2_n) / s_n
 *   loo_var_n = s_n / (1 - h_n)  (noise included, as var(fx) includes Sigma_y),  loo_mean_n = y_n - r_n / (1 - h_n)
 *   loo_logpdf_n = -1/2 [log 2 pi + log s_n - log(1 - h_n) + r_n^2 / (s_n (1 - h_n))]   (double, whatever the element type)
 *   loo_total[b] = sum_n loo_logpdf_n in a fixed order (the LOO-CV score).
 * Any of loo_mean, loo_var, loo_logpdf, loo_total may be NULL.  sigma2_n and m_n are computed in the element type, the rest in
 * double.  Results are bit-reproducible, independent of B and of a regressor's position in the batch; no float atomics.
 * NaN rule: an observation whose 1 - h_n is <= 0 in floating point or not finite (the state does not contain it, or h_n is
 * within rounding of 1) gets NaN in its three outputs (so loo_total is NaN) and is counted by blr_get_stat "loo_degenerate".
 * info[B], checked in the update's and downdate's order: T has a non-positive diagonal entry j -> j, else s_i is not
 * positive -> i; the outputs of such a regressor are left untouched.  The call returns 0 (negative on argument errors, which
 * are checked before the handle).
 * Limits: 1 <= D <= 8192, N >= 0 (N = 0: loo_total = 0), isotropic or diagonal noise (dense noise is an argument error: its
 * "one observation" is a block), ColVecs or RowVecs, host or device memspace; an async handle only enqueues (device memspace).
 * Kernels (csrc/blr_loo.hpp): one marginal pass.  D = 128, aligned ColVecs or RowVecs, N >= 64: the triangular
 * inverse image and the product stream of blr_marginals_batched_* with the epilogue at the store; any other shape: the
 * marginal routes with zero noise into handle workspace (chunks of regressors), then an epilogue kernel.
 * _f32: X, y, s, mw, T, loo_mean, loo_var are float; loo_logpdf and loo_total stay double. */
int blr_loo_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const double* X,
                        int64_t ldx, int64_t strideX, const double* y, int64_t stridey, int noise_kind, const double* s,
                        int64_t strides, const double* mw, int64_t stridemw, const double* T, int64_t ldt, int64_t strideT,
                        double* loo_mean, int64_t stride_lm, double* loo_var, int64_t stride_lv, double* loo_logpdf,
                        int64_t stride_ll, double* loo_total, int32_t* info);
int blr_loo_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const float* X,
                        int64_t ldx, int64_t strideX, const float* y, int64_t stridey, int noise_kind, const float* s,
                        int64_t strides, const float* mw, int64_t stridemw, const float* T, int64_t ldt, int64_t strideT,
                        float* loo_mean, int64_t stride_lm, float* loo_var, int64_t stride_lv, double* loo_logpdf,
                        int64_t stride_ll, double* loo_total, int32_t* info);

/* ---- exact LEAVE-ONE-OUT predictives of a MULTI-OUTPUT state: S target columns, one leverage per input ----------------------
 * Replaces: reference src/bayesian_linear_regression.jl:55-58 (logpdf) per held-out point and COLUMN given the rest -- the repeated
 * conditioning of test/bayesian_linear_regression.jl:49-70 once per observation and column, i.e. a loop of
 * blr_downdate_multi_factor_* / blr_update_multi_factor_* at k = 1, or S calls of blr_loo_batched_* (which read X S times and redo
 * |T^-T x_n|^2 S times).
 * State (M, T) as blr_posterior_multi_batched_* writes it (mw_post block D x S, ldm >= D; T_post) or blr_update_multi_factor_* keeps
 * it: T upper, only the upper triangle read; NOT modified.  It must be conditioned on a data set that contains the N observations
 * (X, Y (N x S column-major per regressor, ldY >= N), s).  With A = T'T:
 *   sigma2_n = |T^-T x_n|^2,  1 - h_n = (s_n - sigma2_n) / s_n,  loo_var[n] = s_n / (1 - h_n)   once per input (noise included)
 *   m_nc = x_n'M[:, c],  r_nc = Y[n, c] - m_nc,  loo_mean[n, c] = Y[n, c] - r_nc / (1 - h_n)
 *   loo_logpdf[n, c] = -1/2 [log 2 pi + log s_n - log(1 - h_n) + r_nc^2 / (s_n (1 - h_n))]     (double in both element types)
 *   loo_total[b * stride_lt + c] = sum_n loo_logpdf[n, c] in a fixed order (the LOO-CV score of column c; double).
 * sigma2_n and m_nc are computed in the element type, the rest in double.  A stride of 0 shares an input: strideX = 0, strideY = 0,
 * strideM = 0, strides = 0 and strideT = 0 included.
 * Outputs: loo_mean (N x S, ld_lm >= N), loo_var (N: ONE per input), loo_logpdf (N x S, ld_ll >= N), loo_total (S per regressor).
 * Any of them may be NULL; with loo_total requested and loo_logpdf NULL the log densities go through handle workspace.
 * info[B], as blr_loo_batched_* and in its order: T has a non-positive diagonal entry j -> j, else s_i is not positive -> i; every
 * output of such a regressor is left untouched; the call returns 0.
 * NaN rule: an input whose 1 - h_n is <= 0 in floating point or not finite gets NaN in loo_var, in all S of its means and log
 * densities, and so in every one of the S totals; it is counted ONCE (not S times) by blr_get_stat "loo_degenerate".
 * Argument errors (negative position; checked before the handle, so a NULL handle with valid arguments returns -1): memspace (2),
 * layout (3), B (4), D (5), N (6), S (7) out of range, ldx too small (9), ldY < N (12), dense noise (14), ldm < D (18), ldt < D (21),
 * ld_lm < N (24), ld_ll < N (29), a negative input stride, a NULL X / Y / s (N > 0) / M / T / info, and for B > 1 overlapping
 * outputs: stride_lm < ld_lm * S (25), stride_lv < N (27), stride_ll < ld_ll * S (30), stride_lt < S (32).  B = 0 or S = 0 is a
 * no-op returning 0.  N = 0: every requested total is 0 and info is 0 (for a state that passes the check).
 * Limits: 1 <= D <= 8192, 0 <= N <= 2^30, 0 <= S <= 2^20, ColVecs or RowVecs with any ldx, isotropic or diagonal noise, host or
 * device memspace; an async handle in device memspace only enqueues at D <= 128.
 * Bit promises: results are bit-reproducible from call to call; the bits of a regressor do not depend on B or on its position in
 * the batch; the bits of column c do not depend on S, on c's position (pass included) or on the other columns of Y and M; the bits
 * of loo_var do not depend on S or on which other outputs are requested; host and device memspace give the same bits.  No
 * bit-equality with blr_loo_batched_* is promised: the products run in a different order.
 * Kernels (csrc/blr_loo_multi.hpp).  D <= 128: per chunk of regressors (<= 65535, images within 256 MiB) the status
 * (loo_check_kernel), the triangular inverse as an MFMA image (marg_image_kernel), loo_cols_kernel over (tile groups, regressors)
 * -- a workgroup keeps its 64-input tile, forms the leverage once and loops over the passes of 16 columns, so X is read once
 * whatever S is -- and the totals (loo_cols_total_kernel); the launch count does not depend on S.  D > 128 is correct, not fast:
 * the large-D variance route of blr_marginals_batched_* with zero noise and the means as X'M into handle workspace (chunks of
 * regressors), then an epilogue kernel; this route may synchronise.
 * _f32: X, Y, s, M, T, loo_mean and loo_var are float; loo_logpdf and loo_total stay double. */
int blr_loo_multi_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S,
                              const double* X, int64_t ldx, int64_t strideX, const double* Y, int64_t ldY, int64_t strideY,
                              int noise_kind, const double* s, int64_t strides, const double* M, int64_t ldm, int64_t strideM,
                              const double* T, int64_t ldt, int64_t strideT, double* loo_mean, int64_t ld_lm, int64_t stride_lm,
                              double* loo_var, int64_t stride_lv, double* loo_logpdf, int64_t ld_ll, int64_t stride_ll,
                              double* loo_total, int64_t stride_lt, int32_t* info);
int blr_loo_multi_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S,
                              const float* X, int64_t ldx, int64_t strideX, const float* Y, int64_t ldY, int64_t strideY,
                              int noise_kind, const float* s, int64_t strides, const float* M, int64_t ldm, int64_t strideM,
                              const float* T, int64_t ldt, int64_t strideT, float* loo_mean, int64_t ld_lm, int64_t stride_lm,
                              float* loo_var, int64_t stride_lv, double* loo_logpdf, int64_t ld_ll, int64_t stride_ll,
                              double* loo_total, int64_t stride_lt, int32_t* info);

/* ---- exact LEAVE-FOLD-OUT (K-fold) predictives of the observations a posterior state contains ------------------------------
 * Replaces: a loop of blr_downdate_factor_* (forget the fold) / blr_mean_and_cov_* or blr_marginals_batched_* (predict it) /
 * blr_update_factor_* (put it back) per fold and regressor, or K refits through blr_posterior_batched_*; reference
 * src/bayesian_linear_regression.jl:55-58 (logpdf) of each held-out fold given the rest.
 * State (mw, T) as for blr_loo_batched_*: T upper, only its upper triangle is read; NOT modified.  It must be conditioned on a
 * data set that contains the N observations (X, y, s).  Folds are contiguous blocks of F observations: fold f is
 * [f F, min((f + 1) F, N)) with n_f members, nfolds = ceil(N / F).  With A = T'T, z_n = T^-T x_n, q_n = 1 / sqrt(s_n),
 * r_n = y_n - x_n'mw and Z_f the fold's rows z_n':
 *   G~ = I - diag(q) Z_f Z_f' diag(q) = L L'     (n_f x n_f; positive definite iff the state really contains the fold)
 *   u = L^-1 (q .* r),   g = L^-T u
 *   kf_mean_n = y_n - sqrt(s_n) g_n                     (predictive mean of y_n given all the other FOLDS)
 *   kf_var_n  = s_n [G~^-1]_nn = s_n |L^-1 e_n|^2       (noise included, as var(fx) includes Sigma_y)
 *   kf_logpdf[f] = -1/2 [n_f log 2 pi + sum log s_n - 2 sum log L_ii + |u|^2]   (the JOINT density of the fold; double)
 *   kf_total[b] = sum_f kf_logpdf[f] in a fixed order (the K-fold CV score; double).
 * At F = 1 these are the numbers of blr_loo_batched_*.  Z Z' and x_n'mw are computed in the element type on the matrix cores; from G~
 * onwards everything is double in both element types.
 * Outputs: kf_mean and kf_var [N] per regressor in the element type, kf_logpdf [nfolds] per regressor, kf_total [B].  Any of them may
 * be NULL; with kf_total requested and kf_logpdf NULL the log densities go through handle workspace.  A stride of 0 shares an input
 * (strideX, stridey, strides, stridemw and strideT included).
 * Sizes: 1 <= F <= 64, and F > N is allowed: one fold, the predictive under the state minus ALL of the data.  1 <= D <= 8192;
 * 0 <= N <= 2^30 at D <= 128 and N <= 16384 at D > 128 (that route goes through an N x N covariance).  Isotropic or diagonal noise;
 * dense noise is an argument error (it couples the folds).  ColVecs or RowVecs with any ldx, host or device memspace.  At D <= 128 the
 * rows z_n of a chunk of regressors live in handle workspace: 16 ceil(D / 16) elements per observation.
 * No-ops: B = 0 returns 0 and touches nothing; N = 0 gives kf_total = 0 and info = 0 (for a state that passes the check).
 * Argument errors (negative position; checked before the handle, so a NULL handle with valid arguments returns -1): memspace (2),
 * layout (3), B (4), D (5), N (6; N > 16384 at D > 128 included), F (7) out of range, ldx too small (9), dense noise (13), ldt < D (19),
 * a negative input stride (10, 12, 15, 17, 20), a NULL X / y / s (N > 0; 8, 11, 14) / mw (16) / T (18) / info (28), and for B > 1
 * overlapping outputs: stride_km < N (22), stride_kv < N (24), stride_kl < nfolds (26).
 * info[B], as blr_loo_batched_* and in its order: T has a non-positive diagonal entry j -> j, else s_i is not positive -> i; every
 * output of such a regressor is left untouched; the call returns 0.
 * NaN rule: a fold whose Cholesky of G~ meets a pivot <= 0 or not finite (the state does not contain the fold, or a leverage is
 * within rounding of 1) gets NaN in kf_mean and kf_var of all its members and in its kf_logpdf, and so in kf_total; it is counted
 * once by blr_get_stat "kfold_degenerate".  Every other fold of the regressor is unaffected, bit for bit.
 * Bit promises: results are bit-reproducible from call to call; the bits of a regressor do not depend on B, on its position in the
 * batch, on the chunking or on the other regressors; the bits of fold f depend only on that regressor's T and mw and on the fold's
 * own X, y and s -- not on N, on the other folds or on where the fold lands inside a workgroup; the bits of one output do not
 * depend on which others are requested; host and device memspace give the same bits.  No float atomics.  NOT promised:
 * bit-equality with blr_loo_batched_* at F = 1 (the products run in a different order).
 * Kernels (csrc/blr_kfold.hpp).  D <= 128, four launches per chunk of regressors (chunks by the rules of
 * blr_mean_and_cov_batched_*: grid.y <= 65535, 256 MiB of images, 256 MiB of rows z_n, never fewer than one regressor; option
 * MAX_CHUNK and blr_get_stat "last_chunks" are honoured): the status (loo_check_kernel), the triangular inverse as an MFMA image
 * (marg_image_kernel), cov_whiten_kernel for the rows z_n and x_n'mw (X is read once), and kfold_kernel over (fold packs,
 * regressors) -- a workgroup takes floor(64 / F) consecutive folds, forms their 64 x 64 product on the matrix cores, and runs the
 * Cholesky, L^-1 and the epilogue in double in LDS, every fold bounded to its own rows and columns -- then the totals
 * (loo_total_kernel).  An async handle in device memspace only enqueues.  D > 128 is correct, not fast: one regressor after the
 * other through the launches of blr_mean_and_cov_* into a staging covariance whose diagonal blocks the fold kernel reads
 * (G~_ij = 2 delta_ij - C_ij q_i q_j); this route SYNCHRONISES, async handle or not.
 * _f32: X, y, s, mw, T, kf_mean, kf_var are float; kf_logpdf and kf_total stay double. */
int blr_kfold_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t F, const double* X,
                          int64_t ldx, int64_t strideX, const double* y, int64_t stridey, int noise_kind, const double* s,
                          int64_t strides, const double* mw, int64_t stridemw, const double* T, int64_t ldt, int64_t strideT,
                          double* kf_mean, int64_t stride_km, double* kf_var, int64_t stride_kv, double* kf_logpdf,
                          int64_t stride_kl, double* kf_total, int32_t* info);
int blr_kfold_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t F, const float* X,
                          int64_t ldx, int64_t strideX, const float* y, int64_t stridey, int noise_kind, const float* s,
                          int64_t strides, const float* mw, int64_t stridemw, const float* T, int64_t ldt, int64_t strideT,
                          float* kf_mean, int64_t stride_km, float* kf_var, int64_t stride_kv, double* kf_logpdf,
                          int64_t stride_kl, double* kf_total, int32_t* info);

/* ---- exact LEAVE-FOLD-OUT (K-fold) predictives for LARGE folds: the fold is removed in weight space -------------------------
 * Replaces: a loop of blr_downdate_factor_* (forget the fold) / blr_marginals_batched_* (predict it) / blr_update_factor_* (put it
 * back) per fold and regressor, or K refits through blr_posterior_batched_* on the other folds' data; reference
 * src/bayesian_linear_regression.jl:55-58 (logpdf) of each held-out fold given the rest.  blr_kfold_batched_* computes the same
 * quantities in observation space and stops at folds of 64; the K-fold cross-validation people run has K = 5 or 10, folds of N / K.
 * Arguments, outputs, shapes and strides are those of blr_kfold_batched_*, in the same order: the state (mw, T), T upper, only its
 * upper triangle is read, NOT modified, conditioned on a data set that contains the N observations (X, y, s); fold f is
 * [f F, min((f + 1) F, N)) with n_f members, nfolds = ceil(N / F).  With A = T'T and r0_n = y_n - x_n'mw:
 *   G_f = X_f S_f^-1 X_f'    d_f = X_f S_f^-1 r0    q_f = r0' S_f^-1 r0    l_f = sum log s_n      (one pass over the fold's rows)
 *   A_f = A - G_f = U_f'U_f                       (positive definite iff the state really contains the fold)
 *   u_f = U_f^-T d_f,   mw_f = mw - U_f^-1 u_f
 *   kf_mean_n = x_n'mw_f                               (predictive mean of y_n given all the other FOLDS)
 *   kf_var_n  = s_n + |U_f^-T x_n|^2                   (noise included, as var(fx) includes Sigma_y)
 *   kf_logpdf[f] = -1/2 [n_f log 2 pi + l_f + logdet A - logdet A_f + q_f + |u_f|^2]   (the JOINT density of the fold; double)
 *   kf_total[b] = sum_f kf_logpdf[f] in a fixed order (the K-fold CV score; double).
 * Precision: A_f, its factor, mw_f, kf_mean and kf_var are in the element type; A = T'T, G_f and d_f are accumulated in double
 * from the element-type inputs in both element types and the difference A - G_f is rounded to the element type once; q_f, l_f, the
 * two logdet, |u_f|^2, kf_logpdf and kf_total are double in both element types.  Cancellation: A - G_f subtracts what the fold contributed from
 * everything the state knows.  A fold that carries nearly all of the state's information leaves a small difference of large numbers
 * and loses that many digits (a fold with 19/20 of the information: a factor of about 20 in every output); float32 shows it first.
 * Outputs: kf_mean and kf_var [N] per regressor in the element type, kf_logpdf [nfolds] per regressor, kf_total [B].  Any of them may
 * be NULL; with kf_total requested and kf_logpdf NULL the log densities go through handle workspace.  A stride of 0 shares an input
 * (strideX, stridey, strides, stridemw and strideT included).
 * Sizes: 1 <= D <= 128.  F >= 1 with ceil(N / F) <= 1024: this route is for few, large folds, many small ones belong to
 * blr_kfold_batched_*.  F > N is allowed: one fold, the predictive under the state minus ALL of the data.  0 <= N <= 2^30.  Isotropic
 * or diagonal noise; dense noise is an argument error (it couples the folds).  ColVecs or RowVecs with any ldx, host or device
 * memspace.
 * No-ops: B = 0 returns 0 and touches nothing; N = 0 gives kf_total = 0 and info = 0 (for a state that passes the check).
 * Argument errors (negative position, those of blr_kfold_batched_*; checked before the handle, so a NULL handle with valid arguments
 * returns -1): memspace (2), layout (3), B (4), D (5; D > 128 included), N (6) out of range, F < 1 or ceil(N / F) > 1024 (7), ldx too
 * small (9), dense noise (13), ldt < D (19), a negative input stride (10, 12, 15, 17, 20), a NULL X / y / s (N > 0; 8, 11, 14) / mw
 * (16) / T (18) / info (28), and for B > 1 overlapping outputs: stride_km < N (22), stride_kv < N (24), stride_kl < nfolds (26).
 * info[B], as blr_loo_batched_* and in its order: T has a non-positive diagonal entry j -> j, else s_i is not positive -> i; every
 * output of such a regressor is left untouched; the call returns 0.
 * NaN rule: a fold whose factorisation of A_f meets a pivot <= 0 or not finite (the state does not contain the fold, or the fold
 * carries all of the state's information to within rounding) gets NaN in kf_mean and kf_var of all its members and in its
 * kf_logpdf, and so in kf_total; it is counted once by blr_get_stat "kfold_degenerate".  Every other fold of the regressor keeps
 * its bits.
 * Bit promises: results are bit-reproducible from call to call; the bits of a regressor do not depend on B, on its position in the
 * batch, on the chunking or on the other regressors; the bits of fold f depend only on that regressor's T and mw and on the fold's
 * own X, y, s and row count -- not on N or on the other folds; the bits of one output do not depend on which others are
 * requested; host and device memspace give the same bits.  No float atomics.  NOT promised: bit-equality with blr_kfold_batched_*
 * (the two work in different spaces; they agree to rounding at F <= 64).
 * Kernels (csrc/blr_kfold_large.hpp), a fixed number of launches per chunk of regressors whatever B and the fold
 * count are: the status (loo_check_kernel); A = T'T in the packed layout and logdet A (kfl_state_kernel); the statistics of every
 * (regressor, fold, column block), centred at the state's mean: in fp64 by the streaming Gram phase of the posterior kernel without
 * a prior (kfl_stats_kernel), in fp32 by kfl_stats32_kernel, which widens the float rows and accumulates in double on the fp64
 * matrix instruction (the column blocks of a fold follow from n_f alone; kfl_reduce_kernel adds them in a fixed order when a fold
 * has more than one); one workgroup per (regressor, fold) factors A - G_f in LDS, solves for mw_f and writes kf_logpdf[f]
 * (kfl_factor_kernel); for kf_mean / kf_var the triangular inverses of the U_f as MFMA images (marg_image_kernel) and
 * kfl_predict_kernel over (64-input tiles of a fold, fold, regressor), rows bounded to the fold; the totals (loo_total_kernel).  X is
 * read twice per call whatever the fold count is.  Workspace per (regressor, fold): the statistics, D^2 elements of U_f, D of mw_f
 * and one image; the regressors go in chunks that keep each of these buffers within 256 MiB and grid.y <= 65535, never fewer than
 * one regressor (option MAX_CHUNK and blr_get_stat "last_chunks" are honoured).  An async handle in device memspace only enqueues.
 * _f32: X, y, s, mw, T, kf_mean, kf_var are float; kf_logpdf and kf_total stay double. */
int blr_kfold_large_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t F, const double* X,
                                int64_t ldx, int64_t strideX, const double* y, int64_t stridey, int noise_kind, const double* s,
                                int64_t strides, const double* mw, int64_t stridemw, const double* T, int64_t ldt, int64_t strideT,
                                double* kf_mean, int64_t stride_km, double* kf_var, int64_t stride_kv, double* kf_logpdf,
                                int64_t stride_kl, double* kf_total, int32_t* info);
int blr_kfold_large_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t F, const float* X,
                                int64_t ldx, int64_t strideX, const float* y, int64_t stridey, int noise_kind, const float* s,
                                int64_t strides, const float* mw, int64_t stridemw, const float* T, int64_t ldt, int64_t strideT,
                                float* kf_mean, int64_t stride_km, float* kf_var, int64_t stride_kv, double* kf_logpdf,
                                int64_t stride_kl, double* kf_total, int32_t* info);

/* ---- exact LEAVE-FOLD-OUT (K-fold) predictives of a MULTI-OUTPUT state: S target columns, one factor per fold ---------------------
 * Replaces: S calls of blr_kfold_batched_* on the columns (M[:, c], Y[:, c]), which read X S times, form z_n = T^-T x_n S times and
 * factor every fold's 64 x 64 hat block S times; reference src/bayesian_linear_regression.jl:55-58 (logpdf) of each held-out fold
 * and COLUMN given the rest.
 * State (M, T) as for blr_loo_multi_batched_*: M the D x S block of means (ldm >= D), T upper, only its upper triangle is read; NOT
 * modified.  It must be conditioned on a data set that contains the N observations (X, Y (N x S column-major per regressor,
 * ldY >= N), s).  Folds as for blr_kfold_batched_*: fold f is [f F, min((f + 1) F, N)) with n_f members, nfolds = ceil(N / F).
 * With z_n = T^-T x_n, q_n = 1 / sqrt(s_n) and Z_f the fold's rows z_n':
 *   G~ = I - diag(q) Z_f Z_f' diag(q) = L L'           once per fold (positive definite iff the state really contains the fold)
 *   kf_var[n] = s_n |L^-1 e_n|^2                       ONE per input: it does not depend on the column (noise included)
 *   r_nc = Y[n, c] - x_n'M[:, c],   u_c = L^-1 (q .* r_c),   g_c = L^-T u_c
 *   kf_mean[n, c] = Y[n, c] - sqrt(s_n) g_nc
 *   kf_logpdf[f, c] = -1/2 [n_f log 2 pi + sum log s_n - 2 sum log L_ii + |u_c|^2]   (the JOINT density of the fold; double)
 *   kf_total[b * stride_kt + c] = sum_f kf_logpdf[f, c] in a fixed order (the K-fold CV score of column c; double).
 * At S = 1 these are the numbers of blr_kfold_batched_*, at F = 1 those of blr_loo_multi_batched_*.  Z Z' and x_n'M[:, c] are
 * computed in the element type on the matrix cores (the means from X and M, not from z_n'(T M)); from G~ onwards everything is
 * double in both element types.
 * Outputs: kf_mean (N x S, ld_km >= N) and kf_var (N) in the element type, kf_logpdf (nfolds x S column-major per regressor,
 * ld_kl >= nfolds, double), kf_total (S per regressor, stride_kt between regressors, double).  Any of them may be NULL; with
 * kf_total requested and kf_logpdf NULL the log densities go through handle workspace.  A stride of 0 shares an input (strideX,
 * strideY, strides, strideM and strideT included).
 * Sizes: 1 <= F <= 64, and F > N is allowed: one fold.  1 <= D <= 128: there is no slow route, D > 128 is an argument error (5).
 * 0 <= S <= 2^20, 0 <= N <= 2^30, and the means workspace of one regressor must be addressable: S * 64 ceil(N / 64) <= 2^28
 * elements, else an argument error at S's position (7).  Isotropic or diagonal noise; dense noise is an argument error (it couples
 * the folds).  ColVecs or RowVecs with any ldx, host or device memspace.
 * No-ops: B = 0 or S = 0 returns 0 and touches nothing; N = 0 gives every requested total = 0 and info = 0 (for a state that
 * passes the check).
 * Argument errors (negative position; checked before the handle, so a NULL handle with valid arguments returns -1): memspace (2),
 * layout (3), B (4), D (5), N (6), S (7), F (8) out of range, ldx too small (10), ldY < N (13), dense noise (15), ldm < D (19),
 * ldt < D (22), ld_km < N (25), ld_kl < nfolds (30), a negative input stride (11, 14, 17, 20, 23), a NULL X / Y / s (N > 0; 9, 12,
 * 16) / M (18) / T (21) / info (34), and for B > 1 overlapping outputs: stride_km < ld_km * S (26), stride_kv < N (28),
 * stride_kl < ld_kl * S (31), stride_kt < S (33).
 * info[B], as blr_loo_batched_* and in its order: T has a non-positive diagonal entry j -> j, else s_i is not positive -> i; every
 * output of such a regressor is left untouched; the call returns 0.
 * NaN rule: a fold whose Cholesky of G~ meets a pivot <= 0 or not finite gets NaN in kf_var of its members, in all S of their
 * means and in its S log densities, and so in all S totals; it is counted ONCE (not S times) by blr_get_stat "kfold_degenerate".
 * Every other fold of the regressor keeps its bits.  A NaN in one column of Y stays in that column.
 * Bit promises: results are bit-reproducible from call to call; the bits of a regressor do not depend on B, on its position in the
 * batch, on the chunking or on the memspace; the bits of fold f depend only on that regressor's T and M and on the fold's own rows;
 * the bits of column c do not depend on S, on c's position (pass and wave included) or on the other columns of Y and M; the bits
 * of kf_var do not depend on S or on which outputs are requested.  No float atomics.  NOT promised: bit-equality with
 * blr_kfold_batched_* or blr_loo_multi_batched_*.
 * Kernels (csrc/blr_kfold_multi.hpp), a launch list per chunk of regressors that does not depend on S or on the fold
 * count (chunks: grid.y <= 65535, 256 MiB each of images, of rows z_n and of means, never fewer than one regressor; option
 * MAX_CHUNK and blr_get_stat "last_chunks" are honoured): the status (loo_check_kernel), the triangular inverse as an MFMA image
 * (marg_image_kernel), kfold_whiten_cols_kernel -- X is read once: the rows z_n and, in passes of 16 columns of M, the S means
 * into handle workspace --, kfold_cols_kernel over (fold packs, regressors) -- the product, the Cholesky and L^-1 of
 * blr_kfold_batched_*'s kernel once per pack, then an epilogue over the S columns, four at a time, with L^-1 read-only in LDS --
 * and the totals (loo_cols_total_kernel).  An async handle in device memspace only enqueues.
 * _f32: X, Y, s, M, T, kf_mean and kf_var are float; kf_logpdf and kf_total stay double. */
int blr_kfold_multi_batched_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, int64_t F,
                                const double* X, int64_t ldx, int64_t strideX, const double* Y, int64_t ldY, int64_t strideY,
                                int noise_kind, const double* s, int64_t strides, const double* M, int64_t ldm, int64_t strideM,
                                const double* T, int64_t ldt, int64_t strideT, double* kf_mean, int64_t ld_km, int64_t stride_km,
                                double* kf_var, int64_t stride_kv, double* kf_logpdf, int64_t ld_kl, int64_t stride_kl,
                                double* kf_total, int64_t stride_kt, int32_t* info);
int blr_kfold_multi_batched_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, int64_t S, int64_t F,
                                const float* X, int64_t ldx, int64_t strideX, const float* Y, int64_t ldY, int64_t strideY,
                                int noise_kind, const float* s, int64_t strides, const float* M, int64_t ldm, int64_t strideM,
                                const float* T, int64_t ldt, int64_t strideT, float* kf_mean, int64_t ld_km, int64_t stride_km,
                                float* kf_var, int64_t stride_kv, double* kf_logpdf, int64_t ld_kl, int64_t stride_kl,
                                double* kf_total, int64_t stride_kt, int32_t* info);

/* ---- evidence of one data set under a GRID of (prior scale, noise scale) settings, from one pass over the data ------------
 * Replaces: blr_posterior_batched_* called with strideX = 0, stridey = 0 and one scaled (s, Lw) pair per setting, which re-forms
 * the D x D Gram matrix per setting; reference src/bayesian_linear_regression.jl:55-58 (logpdf) on
 * BayesianLinearRegressor(mw, alpha L0)(x, tau S0) -- type-II maximum likelihood over (alpha, tau), Bishop 3.5.
 * Base prior precision L0 = Lw (DENSE: upper triangle read; DIAGONAL), base noise S0 = s (isotropic or diagonal); setting g of
 * regressor b is Lw = alpha[b][g] L0, Sy = tau[b][g] S0 (stride_alpha / stride_tau = 0: one grid shared by all regressors; alpha or
 * tau NULL: all ones).  With
 *   G0 = X S0^-1 X'    b0 = X S0^-1 (y - X'mw)    q0 = (y - X'mw)' S0^-1 (y - X'mw)    l0 = logdet S0
 *   A = alpha L0 + G0 / tau      T = chol(A).U      u = T^-T b0 / tau      mw' = mw + T^-1 u
 *   logpdf[b][g] = -1/2 [N log 2 pi + N log tau + l0 + q0 / tau + logdet A - D log alpha - logdet L0 - |u|^2]
 * which is what blr_posterior_batched_* returns for that (s, Lw) pair.  best[b] (may be NULL) = the smallest g among the settings
 * with the largest finite evidence, -1 when no setting succeeded.  mw_best, T_best (each may be NULL): (mw_post, T_post) exactly as
 * blr_posterior_batched_* writes them (T upper, strictly-lower part zero) for the setting best[b]; left untouched when best[b] = -1.
 * info[b][g], LAPACK style, in the reference's order (:78 prior, :79 noise, :86 posterior): alpha_g not positive or not finite -> 1
 * (leading minor 1 of the prior), a base prior that is not positive definite -> its failing leading minor for all G settings of
 * that regressor, tau_g not positive or not finite -> 1 (observation 1), a base noise entry s_i not positive -> i for all G
 * settings, else the failing leading minor of A; logpdf of a failed setting is NaN.  The call returns 0 (negative argument
 * indices on argument errors, which are checked before the handle; output strides that overlap for B > 1 are argument errors).
 * Limits: 1 <= D <= 8192, N >= 0, 0 <= G <= 2^20 (G = 0 or B = 0: no-op), B max(G, 8) < 2^24 (argument error 21 beyond), stride_lp >= G, stride_info >= G;
 * isotropic or diagonal base noise (dense: argument error), DENSE or DIAGONAL base prior (BLR_PRIOR_UPPER_FACTOR is an argument
 * error: pass a carried-forward factor as U'U); ColVecs or RowVecs, any ldx; host or device memspace; an async handle only enqueues
 * (device memspace, D <= 128).  Bit-reproducible; the bits of regressor b do not depend on B or on its position, those of setting
 * g not on G or on its position (no float atomics, fixed summation orders).
 * Kernels (csrc/blr_grid.hpp).  D <= 128: X is read ONCE per regressor by the streaming Gram phase of the fused
 * kernel (fp64 / fp32 matrix cores; never the int8-sliced Gram) into a statistics buffer of the handle -- N is cut into column
 * blocks of about 1024 (at most 8, a function of N alone) that are added in a fixed order; then one workgroup per (regressor,
 * setting) builds A in LDS, factors it and writes the evidence; one argmax launch; one more launch over the B winners for mw_best /
 * T_best.  The launches do not depend on B or G.  The statistics buffer takes ceil(D/16)*16 * (ceil(D/16)*16 + 3) / 2 elements per
 * column block and regressor (blr_release_workspace frees it).
 * D > 128: correct, not fast -- every setting's scaled operands go through the pipeline of blr_posterior_batched_* (the Gram matrix
 * is formed again per setting), the winners once more; the call synchronises whatever the handle's async flag says.
 * _f32: X, y, s, mw, Lw, alpha, tau, mw_best, T_best are float; logpdf stays double. */
int blr_logpdf_grid_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const double* X, int64_t ldx,
                        int64_t strideX, const double* y, int64_t stridey, int noise_kind, const double* s, int64_t strides,
                        int prior_kind, const double* mw, int64_t stridemw, const double* Lw, int64_t ldl, int64_t strideLw,
                        int64_t G, const double* alpha, int64_t stride_alpha, const double* tau, int64_t stride_tau,
                        double* logpdf, int64_t stride_lp, int64_t* best, double* mw_best, int64_t stride_mwbest,
                        double* T_best, int64_t ldt, int64_t strideT, int32_t* info, int64_t stride_info);
int blr_logpdf_grid_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, int64_t N, const float* X, int64_t ldx,
                        int64_t strideX, const float* y, int64_t stridey, int noise_kind, const float* s, int64_t strides,
                        int prior_kind, const float* mw, int64_t stridemw, const float* Lw, int64_t ldl, int64_t strideLw,
                        int64_t G, const float* alpha, int64_t stride_alpha, const float* tau, int64_t stride_tau,
                        double* logpdf, int64_t stride_lp, int64_t* best, float* mw_best, int64_t stride_mwbest,
                        float* T_best, int64_t ldt, int64_t strideT, int32_t* info, int64_t stride_info);

/* ---- the evidence grid for regressors with UNEQUAL observation counts ----------------------------------------------------
 * Replaces: a loop of B calls of blr_logpdf_grid_* with B = 1 (six launches and a staging round trip each), or G calls of
 * blr_posterior_ragged_* on scaled operands (the D x D Gram matrices formed G times); reference
 * src/bayesian_linear_regression.jl:55-58 (logpdf) on BayesianLinearRegressor(mw, alpha L0)(x, tau S0), per setting, under a map
 * over fxs of different lengths.
 * Packing exactly as in blr_posterior_ragged_*: `offsets` is a HOST array of B + 1 entries in both memspaces (non-decreasing,
 * offsets[0] >= 0, every count <= 2^30; a violation is argument error -6); regressor b owns N_b = offsets[b+1] - offsets[b]
 * observations.  ColVecs slices start at X + offsets[b]*ldx, RowVecs slices at X + offsets[b] with ldx >= offsets[B]; y at
 * y + offsets[b]; diagonal base noise at s + offsets[b], isotropic base noise at s + b*strides (strides = 0: one shared variance);
 * dense noise is an argument error.  N_b = 0 is allowed: the statistics are zero and the evidence is what blr_logpdf_grid_*
 * returns at N = 0.
 * The prior (DENSE or DIAGONAL; BLR_PRIOR_UPPER_FACTOR is an argument error: pass a carried-forward factor as U'U), the settings
 * (alpha, tau and their strides; NULL: all ones), logpdf[b][g], info[b][g] with its rules and their order, best[b] and the refit
 * outputs mw_best / T_best mean what they mean for blr_logpdf_grid_* and are checked in its order; under diagonal noise a base
 * noise entry s_i <= 0 reports i, 1-based within the regressor's OWN slice.  The argument checks come before the handle's; B = 0 or
 * G = 0 is a no-op.  Limits: B G < 2^24 and sum_b S_b < 2^24 (S_b: the column blocks of regressor b, at most 8), argument error on
 * G (-19) beyond either, checked before anything runs.
 * Bit promise: every output of regressor b -- logpdf[b][.], info[b][.], best[b], mw_best and T_best of b -- has the bits of
 * blr_logpdf_grid_* with B = 1 on its slice under the same handle options.  The bits are therefore independent of B, of the other
 * regressors, of any permutation of the batch, and of G and a setting's position; host and device memspace give the same bits; no
 * float atomics are used.
 * Kernels (csrc/blr_grid_ragged.hpp).  D <= 128: the launches of blr_logpdf_grid_*, with the statistics pass over a
 * flat list of (regressor, column block) items -- the blocks blr_logpdf_grid_* cuts at N = N_b -- sorted longest block first: one
 * regressor of 2^20 observations among short ones streams on eight workgroups at once.  The statistics buffer takes sum_b S_b blocks
 * (counted by workspace_bytes, freed by blr_release_workspace); there is no chunk loop (last_chunks = 1); blr_last_route names the
 * statistics kernel.  The host tables travel in one upload, which drains the stream.
 * D > 128: correct, not fast -- blr_logpdf_grid_* with B = 1 on each slice, one after the other; the call synchronises.
 * _f32: X, y, s, mw, Lw, alpha, tau, mw_best, T_best are float; logpdf stays double. */
int blr_logpdf_grid_ragged_f64(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets,
                               const double* X, int64_t ldx, const double* y, int noise_kind, const double* s, int64_t strides,
                               int prior_kind, const double* mw, int64_t stridemw, const double* Lw, int64_t ldl,
                               int64_t strideLw, int64_t G, const double* alpha, int64_t stride_alpha, const double* tau,
                               int64_t stride_tau, double* logpdf, int64_t stride_lp, int64_t* best, double* mw_best,
                               int64_t stride_mwbest, double* T_best, int64_t ldt, int64_t strideT, int32_t* info,
                               int64_t stride_info);
int blr_logpdf_grid_ragged_f32(blr_handle* h, int memspace, int layout, int64_t B, int64_t D, const int64_t* offsets,
                               const float* X, int64_t ldx, const float* y, int noise_kind, const float* s, int64_t strides,
                               int prior_kind, const float* mw, int64_t stridemw, const float* Lw, int64_t ldl,
                               int64_t strideLw, int64_t G, const float* alpha, int64_t stride_alpha, const float* tau,
                               int64_t stride_tau, double* logpdf, int64_t stride_lp, int64_t* best, float* mw_best,
                               int64_t stride_mwbest, float* T_best, int64_t ldt, int64_t strideT, int32_t* info,
                               int64_t stride_info);

/* ---- sharded log-evidence: fixed-order sum of logpdf[B] on the device ----------
 * Deterministic (no float atomics): the same bits for the same B regardless of launch geometry.
 * The cross-rank step is one RCCL all-gather of these per-rank partials done by the host framework
 * (torch.distributed / MPI.jl); the data path has no other collective. */
int blr_logpdf_sum(blr_handle* h, int memspace, int64_t B, const double* logpdf, double* total);

/* ---- the exchange itself, RCCL called directly (SURVEY.md 8b contract, 8e) ---------------------------------------
 * For hosts without a collective library of their own (a Julia session per GPU): one process per GPU, one handle per
 * process.  Rank 0 obtains 128 opaque bytes with blr_comm_unique_id and ships them to the other ranks by any means (a file,
 * Distributed.jl, MPI, a socket); every rank then calls blr_comm_init(h, nranks, rank, id) -- collective, like
 * ncclCommInitRank.  librccl is loaded on first use (no link-time dependency; a single-GPU host never needs it).
 *   blr_logpdf_allgather_sum   every rank passes its `count` per-regressor log evidences (device); logpdf_all (device,
 *                              nranks * count doubles, rank order == regressor order) receives the all-gather and *total
 *                              (device) the fixed-order sum of it -- the same bits on every rank, and for every rank count
 *                              that gathers the SAME vector (a batch divisible by the rank count; uneven blocks are
 *                              zero-padded to equal counts by the caller, which moves elements between the lanes of the
 *                              sum: the totals then agree to rounding only).
 *                              Without a communicator (nranks = 1) it degenerates to copy + blr_logpdf_sum.
 *   blr_allreduce_sum          in-place sum over ranks of a device buffer (the `stats` / `scal` exchange of the N-sharded
 *                              single regressor below: is_f64 = 0 for float, 1 for double)
 * Errors: -(2000 + ncclResult_t); -2001 when librccl cannot be loaded; text via blr_last_error. */
#define BLR_UNIQUE_ID_BYTES 128
int blr_comm_unique_id(void* id128);
int blr_comm_init(blr_handle* h, int nranks, int rank, const void* id128);
int blr_comm_destroy(blr_handle* h);
int blr_comm_size(blr_handle* h);
int blr_comm_rank(blr_handle* h);
int blr_logpdf_allgather_sum(blr_handle* h, int64_t count, const double* logpdf_local, double* logpdf_all, double* total);
int blr_allreduce_sum(blr_handle* h, int is_f64, void* buf, int64_t count);
/* The N-sharded single regressor in ONE call per rank: blr_gram_stats_* on this rank's N_local columns, the
 * in-place all-reduce of `stats` (lds * DP elements, DP = 128 ceil(D/128)) and `scal` over the handle's communicator, then
 * blr_posterior_from_stats_* -- every rank ends with the same posterior and evidence of all N_total observations.  `stats`
 * ((DP + 128) x DP, lds >= DP + 128) and `scal` (2 doubles) are caller-provided device scratch; all pointers device.
 * Without a communicator it is the single-GPU update through the statistics path.
 * Reproducibility: every rank gets the SAME bits, but -- unlike blr_logpdf_allgather_sum (all-gather + one fixed-order sum) --
 * the statistics go through ncclAllReduce, a floating-point sum whose order depends on the rank count and the ring: results
 * for different numbers of ranks agree to rounding, not bit for bit. */
int blr_posterior_nsharded_f64(blr_handle* h, int layout, int64_t D, int64_t N_local, int64_t N_total, const double* X,
                               int64_t ldx, const double* y, int noise_kind, const double* s, int prior_kind,
                               const double* mw, const double* Lw, int64_t ldl, double* stats, int64_t lds, double* scal,
                               double* mw_post, double* T_post, int64_t ldt, double* Lw_post, int64_t ldlp, double* logpdf,
                               int32_t* info);
int blr_posterior_nsharded_f32(blr_handle* h, int layout, int64_t D, int64_t N_local, int64_t N_total, const float* X,
                               int64_t ldx, const float* y, int noise_kind, const float* s, int prior_kind, const float* mw,
                               const float* Lw, int64_t ldl, float* stats, int64_t lds, double* scal, float* mw_post,
                               float* T_post, int64_t ldt, float* Lw_post, int64_t ldlp, double* logpdf, int32_t* info);

#ifdef __cplusplus
}
#endif
#endif /* BLR_MI355X_H */
