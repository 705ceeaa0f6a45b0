/*
 * jstsp.h — C ABI of libjstsp_mi355x.so: the MI355X (gfx950) implementation of the
 * sparse channel-estimation solver path of vlaxose/jstsp19.
 *
 * This is the drop-in boundary.  Each entry point replaces one MATLAB
 * function of the reference (cited per function as path:line under /root/reference) and
 * is what a MEX gateway (mex/), a ctypes binding (jstsp19_amd/_lib.py) or any other FFI
 * binds.  Plain pointers and sizes only.
 *
 * Conventions (all entry points)
 *  - Arrays are COLUMN-MAJOR (MATLAB order, basic_system_functions/vec.m:1-2), complex
 *    values INTERLEAVED {re, im} (jstsp_c32 == float[2]).
 *  - `batch` independent problems are stacked along a trailing (slowest) dimension.
 *    batch == 1 with 2-D inputs is exactly the un-batched MATLAB call.
 *  - `memspace` says where EVERY array argument of that call lives:
 *      JSTSP_HOST   — host memory; the library copies in/out (PCIe included in the call);
 *      JSTSP_DEVICE — memory of the context's GPU (hipMalloc / a torch CUDA tensor); nothing is
 *                     copied and the work is stream-ordered on the context's stream: outputs are
 *                     valid for later work on that stream.  Most calls return without waiting for
 *                     the GPU.  EXCEPTIONS (the host needs a value the device computed):
 *                     jstsp_proposed_algorithm_* waits for its stream up to three times - twice at
 *                     setup (the flag of the block-Toeplitz probe of B, see jstsp_last_dictionary_block)
 *                     and once at the end (the per-trial overflow flags, see jstsp_last_fused_fallbacks;
 *                     jstsp_proposed_algorithm_begin_c32 / _end split the call there: _begin returns while the GPU works);
 *                     eigen-decompositions above order 128 (csrc/eig_large.hip) wait once per sweep.
 *    Per-problem scalar arrays (tau_Y, tau_S, rho ...) are always HOST doubles.
 *  - Return value: 0 = ok; < 0 = bad argument (JSTSP_E_*); > 0 = hipError_t of a failed
 *    HIP call.  jstsp_last_error() gives a thread-local message.  No exception crosses
 *    the boundary.  The library never keeps a caller pointer after the call returns
 *    (JSTSP_HOST) / after the stream work completes (JSTSP_DEVICE).
 *  - A context owns one HIP stream and a grow-only device workspace; it is not
 *    thread-safe — use one context per thread / per parfor worker process.
 */
#ifndef JSTSP_H
#define JSTSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct jstsp_ctx jstsp_ctx;
typedef struct { float re, im; } jstsp_c32;
typedef struct { double re, im; } jstsp_c64;   /* MATLAB's own element type (interleaved complex double) */

enum { JSTSP_HOST = 0, JSTSP_DEVICE = 1 };

enum {
    JSTSP_OK = 0,
    JSTSP_E_NULL = -1,      /* required pointer is NULL                      */
    JSTSP_E_SHAPE = -2,     /* non-positive / inconsistent dimensions        */
    JSTSP_E_UNSUPPORTED = -3, /* shape outside what the kernels implement    */
    JSTSP_E_ARG = -4,       /* bad enum / flag value                         */
    JSTSP_E_NOMEM = -5,     /* workspace allocation failed                   */
    JSTSP_E_ILLCOND = -6    /* a factor Gram is too ill-conditioned for the fp32 Gram-inverse path (JSTSP_HOST calls;
                               JSTSP_DEVICE calls are asynchronous: query jstsp_last_conditioning) */
};

/* type argument of proposed_algorithm: 'approximate' vs anything else ('std')
 * (basic_system_functions/proposed_algorithm.m:23-30,45-54). */
enum { JSTSP_TYPE_APPROXIMATE = 0, JSTSP_TYPE_STD = 1 };

/* ---- context ---------------------------------------------------------------------- */
int  jstsp_create(int device_id, jstsp_ctx **out);
int  jstsp_destroy(jstsp_ctx *ctx);
/* Run on an externally owned hipStream_t (e.g. torch's current stream).  NULL is taken literally: HIP's
 * default (null) stream.  JSTSP_DEVICE calls are ordered on this stream, so it must be the stream on
 * which the caller produces the inputs and consumes the outputs. */
int  jstsp_set_stream(jstsp_ctx *ctx, void *hip_stream);
/* Back to a private non-blocking stream owned by the context (the state after jstsp_create). */
int  jstsp_use_own_stream(jstsp_ctx *ctx);
int  jstsp_synchronize(jstsp_ctx *ctx);
const char *jstsp_last_error(void);
const char *jstsp_version(void);
/* Device bytes currently held by the context's workspace. */
size_t jstsp_workspace_bytes(const jstsp_ctx *ctx);

/* ---- Environment ----------------------------------------------------------------------
 * The shipped library reads the 15 variables below and no others.  All are diagnostic, resource or A/B switches whose every
 * setting stays inside the accuracy statement ("Accuracy" below); each is parsed ONCE at the entry of each API call (none is
 * latched for the process, except JSTSP_HOST_THREADS which is read when a host dictionary is staged), so a setting may differ from
 * call to call and is constant within one.  Unset = the default, which is the path every reported number and every parity
 * statement refers to.  Every one is toggled by a test of tests/ that asserts the contract (tests/test_capi_symbols.py checks
 * this list against the sources and against the tests).
 *   JSTSP_H2=0            strict complex-fp32 MFMA (v_mfma_f32_32x32x2_f32) for every contraction; default 1: contractions of
 *                         at least 2^22 complex MACs per problem run as split-f16 MFMA with fp32 accumulation (fp32-equivalent,
 *                         see "Accuracy" below); 2: split-f16 whatever the size
 *   JSTSP_FUSED=0|2       proposed_algorithm: 0 three kernels per iteration instead of the one-pass kernel (csrc/fused.hip); 2 the
 *                         one-pass kernel, but between two passes Res = A^H Tc - R v and P1 = G_A Res as two launches (default 1:
 *                         one launch that keeps the tile of Res on chip, csrc/gradstep.hip; same bits - the A/B and test handle),
 *                         the recomputation of R v inline as three launches (default: early on a side stream, first factor in one
 *                         launch) and a memset of the pass's operand maxima (default: zeroed by the step kernel)
 *   JSTSP_FUSED_PARTS=n   column ranges per problem in that pass (default: 4, 2 or 1 by divisibility of M / 32)
 *   JSTSP_FUSED_KBACK=b   headroom bits of the operand scale the pass predicts (default 4; a negative value is the test hook
 *                         that forces the per-trial re-solve, jstsp_last_fused_fallbacks)
 *   JSTSP_TOEPLITZ=0|1    0: the dictionary is not probed for block-Toeplitz structure; 1: probed, compact image with the
 *                         general pass kernel only; default 2: block height 64 also takes the window kernel
 *   JSTSP_OVERLAP=0|1     side streams between the kernels of an iteration (default: on with the one-pass kernel; same bits)
 *   JSTSP_HOST_PIPELINE=0 a JSTSP_HOST proposed_algorithm call of 128 or more problems as ONE staged solve (default: its two halves on
 *                         two internal contexts, the upload of the second overlapping the solve of the first; same bits)
 *   JSTSP_HOST_COMPACT=0  a JSTSP_HOST dictionary is uploaded whole (default 1: per-trial dictionaries of 64 MiB or more are tested
 *                         for the block-Toeplitz structure on the host while they are staged and uploaded as first block +
 *                         leading columns - bit-identical results; 2: at any size)
 *   JSTSP_HOST_THREADS=n  host threads of that test (default: half the hardware threads within the cgroup quota, at most 16)
 *   JSTSP_MC_EIG_STOP=x   mc_svt / mc_admm, matrices of order 65..128: the eigen-decomposition of iteration i starts from the basis of
 *                         iteration i - 1 and runs no further Jacobi sweep once the Gram in that basis has relative off-diagonals
 *                         below x (default 1e-4: an inexact inner solve, error against the float64 oracle unchanged at 5e-5 /
 *                         9e-5 after 20 iterations, mc_svt 1.7 times faster; 0: every call converged)
 *   JSTSP_LANCZOS=0       Householder + Sturm instead of Lanczos for the spectral norms of convergence_error
 *   JSTSP_LANCZOS_WARM=0  every lambda_max of an ADMM loop by the cold n-step Lanczos run (no warm start from the previous
 *                         iteration's Ritz vector)
 *   JSTSP_LANCZOS_VERIFY=n  a warm-started lambda_max is checked against the cold run every n-th call (default 32;
 *                         0 never, 1 always - then every returned value is the cold one; jstsp_last_lanczos_mismatches)
 *   JSTSP_EIG128=0        general Jacobi kernel (basis in HBM) for Gram orders 65..128
 *   JSTSP_BJ_MASK=0       block Jacobi (orders above 128) without streams restricted to a subset of the compute units
 * (JSTSP_DEVICE=<id> is read by the MEX gateway, not by the library.)
 * jstsp_build_trials_from_channel_c32 adds no variable: the form of the channel and its normalisation are arguments. */

/* ---- kernel-level entry points (the north-star correlation / synthesis) ------------ */

/* Accuracy of the two products below (and of the same contractions inside the solvers).  Results are fp32.  Large
 * contractions (m*n*k >= 2^22) run on the f16 matrix pipe with every fp32 operand split x = h + l into two halves of a
 * power-of-two scaled value (22-23 significant bits) and fp32 accumulation: the error of a product is bounded like an fp32
 * GEMM's, |err| <= c k 2^-24 max_k|a_ik| max_k|b_kj|, i.e. fp32 relative accuracy with respect to the LARGEST terms of each
 * sum.  These two entry points scale the rows / columns along the indices that are not contracted (rows of K and of B in
 * correlate; rows of A*S and columns of B in synthesize) by exact powers of two to a common magnitude first, so a row that
 * is 1e-8 of the rest of its problem still comes out with fp32 relative accuracy (tests/test_gpu_hgemm.py).  Along the
 * contracted index the bound above holds: an addend far below the largest addends of its sum contributes with fewer
 * digits, as it does to an fp32 sum.  Inside the solvers the scales are per problem (the ADMM state has no such
 * dynamic range).
 *
 * Accuracy of the SOLVERS against a float64 evaluation of the same algorithm on the same inputs (oracle/cpu_port.cpp) - what was
 * measured, not a guarantee for inputs unlike these.  proposed_algorithm / proposed_algorithm_angles at N = 64, M = 4096, Gr = 64,
 * G2 = 512, Imax = 100 on Monte-Carlo trials of the reference's system model, 10 SNR points from -15 to 12 dB:
 *   NMSE (plot_errorVSsnr.m:138-141), the contract:  |dNMSE| <= 1e-6 per trial.  Two fixtures of 2560 proposed_algorithm trials
 *     each (tests/test_gpu_parity_tail.py; profiles/r05_parity_heldout_and_setA.json): the one the library's defaults were
 *     chosen on - max 7.3e-7, 99th percentile 4.5e-7, rms 1.4e-7 - and a HELD-OUT one (another generator seed, never used to
 *     choose anything): max 8.3e-7 (three-output call) / 9.1e-7 (two-output call), rms 1.4e-7; proposed_algorithm_angles (1280
 *     held-out trials) max 5.2e-7.  The mean over the realisations of a sweep point - what the reference's drivers report (:170) -
 *     is within 3e-8.  (The defaults of round 4 reached 8.7e-7 on their own tuning set and 1.08e-6 / 1.15e-6 on the held-out one:
 *     one trial of 2560 outside the contract.)
 *   configs[4]'s full frame (N = 64, M = 65 536, Gr = 64, G2 = 4096, one pilot set, Imax = 100; tests/test_gpu_config5_imax100.py,
 *     8 float64 trials of bench.py's configs4 inputs): |dNMSE| max 2.7e-7 (2.0e-7 at the bench's batch 32, 2.7e-7 with JSTSP_H2=0),
 *     S 1.7e-6 of max|S|, convergence_error 2.2e-5 (profiles/r07_measured_tolerances.json).
 *   S, Y:  max|dS| <= 1e-5 max|S| is what the tests assert (round 6: tests/conftest.py TOL_S, 5x the measured errors - <= 2.0e-6
 *     at every shape of the suite, the full-size sets included; profiles/r06_measured_tolerances.json).
 *   convergence_error:  5e-4 relative per entry is what the tests assert (TOL_CE; the first entry of column 3 is Inf, as :51
 *     makes it); measured <= 1.0e-4.  Columns 1:2 are ratios of spectral norms: lambda_max of Grams formed - from 1024 columns on - on
 *     the high f16 plane of X, V1, V2 (11-bit operands: 2^-12 / sqrt(columns) relative on lambda_max, nothing feeds back into the iterates) by a warm-started
 *     Lanczos run (see jstsp_last_lanczos_mismatches): each within 2e-5 of the eigenvalue of that Gram.
 * Only the NMSE carries the 1e-6 statement.  The error of S grows like the square root of the iteration count (the iterate has
 * directions the gradient step does not damp), so Imax well above 100 will exceed these figures proportionally.
 * What it took: the Grams A'*A and B*B' in float64 (with plain fp32-accuracy Grams - rounds 1-3 - the same
 * measurement gives max 1.95e-6), and, round 5, every coefficient of the iteration map (rho, 1/rho, 1/(1+rho), 1-rho, 1-1/rho,
 * 1/(Omega+2rho)) held as two floats derived in float64 from the caller's rho: rounding each to fp32 on its own breaks the
 * relations between them at the 3e-8 level, a constant perturbation that the dual variables integrate. */

/* out = A' * K * B'   (Gr x G2)   — `K2'*k` of proposed_algorithm.m:47 in structured form,
 * `A'*r` of OMP.m:17 when the dictionary is kron(B.', A).
 * K: N x M x batch.  A: N x Gr, B: G2 x M; strideA/strideB = elements between consecutive
 * problems' A / B (0 = one dictionary shared by the whole batch). */
int jstsp_correlate_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                        const jstsp_c32 *K, const jstsp_c32 *A, long long strideA,
                        const jstsp_c32 *B, long long strideB,
                        jstsp_c32 *out, int memspace);

/* out = A * S * B   (N x M)   — `K2*s` / `A*S*B` of proposed_algorithm.m:38,58. */
int jstsp_synthesize_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                         const jstsp_c32 *S, const jstsp_c32 *A, long long strideA,
                         const jstsp_c32 *B, long long strideB,
                         jstsp_c32 *out, int memspace);

/* Res = A' * Tc - RV  and  P1 = GA * Res   (Gr x G2): the 64-term products of the gradient step - the second factor of
 * `K2'*k - R*v` and the first factor of `R*res`, proposed_algorithm.m:47-48 - in one launch on the f16 matrix pipe (the solver
 * itself forms them as fp32-MFMA products; N = Gr = 64, G2 a multiple of 64; else JSTSP_E_UNSUPPORTED).  These sums live in the space of
 * the iterate v, where the iteration forgets nothing, so they are formed to fp32-OUTPUT accuracy: operands split three ways
 * into f16 (33 bits: the fp32 values exactly), exact f16 x f16 products, float64 final sums.
 * Tc: N x G2 x batch; A: N x Gr; GA: Gr x Gr Hermitian (strides 0 = shared); RV: Gr x G2 x batch or NULL. */
int jstsp_gradient_head_c32(jstsp_ctx *ctx, int N, int Gr, int G2, int batch, const jstsp_c32 *Tc,
                            const jstsp_c32 *A, long long strideA, const jstsp_c32 *GA, long long strideG,
                            const jstsp_c32 *RV, jstsp_c32 *Res_out, jstsp_c32 *P1_out, int memspace);

/* ---- solvers ------------------------------------------------------------------------ */

/* [S, Y, convergence_error] = proposed_algorithm(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type)
 *   basic_system_functions/proposed_algorithm.m:1-73
 * [S, Y, convergence_error] = proposed_algorithm_angles(subY, Omega, indx_S, A, B, Imax, ...)
 *   basic_system_functions/proposed_algorithm_angles.m:1-85   (when indx_S != NULL)
 *
 * subY  : N x M x batch complex.       Omega : N x M x batch float (0/1 sampling mask).
 * A     : N x Gr (strideA as above).   B     : G2 x M (strideB as above).
 * tau_Y, tau_S, rho : host double[batch].
 * indx_S: NULL, or Gr*G2 x batch int32, 1-BASED column-major linear indices into S in
 *         descending-magnitude order (plot_errorVSsnr.m:143); same memspace as the arrays.
 * S_out : Gr x G2 x batch.   Y_out : N x M x batch (may be NULL).
 * ce_out: NULL (spectral norms are then not computed), or Imax x 3 x batch DOUBLE,
 *         column-major (ce[i + Imax*c + 3*Imax*t]); same memspace as the arrays. */
int jstsp_proposed_algorithm_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                                 const jstsp_c32 *subY, const float *Omega,
                                 const jstsp_c32 *A, long long strideA,
                                 const jstsp_c32 *B, long long strideB,
                                 int Imax, const double *tau_Y, const double *tau_S,
                                 const double *rho, int type, const int32_t *indx_S,
                                 jstsp_c32 *S_out, jstsp_c32 *Y_out, double *ce_out,
                                 int memspace);

/* The same solve in two phases, for arrays in DEVICE memory: _begin enqueues the whole solve and the copies into S_out / Y_out /
 * ce_out on the context's stream and returns WITHOUT waiting for it (its only waits are the two reads of the block-Toeplitz
 * probe at setup, i.e. for work enqueued BEFORE the solve); _end waits for the solve's completion event, looks at the per-trial
 * overflow flags (copied to pinned host memory by _begin) and, in the pathological case that any is set, enqueues the second
 * solve of those trials (see jstsp_last_fused_fallbacks).  Between the two calls the host is free - e.g. to prepare the next
 * batch - and the context may be used for other work; outputs are final in stream order after _end.
 * Contract: every array argument stays allocated, and the inputs unmodified, until _end has returned; tau_Y / tau_S / rho are
 * copied by _begin.  Exactly one _end per _begin (it frees *pending); fallbacks may be NULL. */
typedef struct jstsp_pending jstsp_pending;
int jstsp_proposed_algorithm_begin_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                                       const jstsp_c32 *subY, const float *Omega,
                                       const jstsp_c32 *A, long long strideA,
                                       const jstsp_c32 *B, long long strideB,
                                       int Imax, const double *tau_Y, const double *tau_S,
                                       const double *rho, int type, const int32_t *indx_S,
                                       jstsp_c32 *S_out, jstsp_c32 *Y_out, double *ce_out,
                                       jstsp_pending **pending);
int jstsp_proposed_algorithm_end(jstsp_ctx *ctx, jstsp_pending *pending, int *fallbacks);

/* Trials of the last jstsp_proposed_algorithm_c32/_c64 call on this context that were solved a second time.  The default
 * iteration for N = 64 (one pass over the dictionary per iteration, csrc/fused.hip) forms `k` (proposed_algorithm.m:43) and
 * consumes it in the same kernel, so the f16 scale of its split is PREDICTED from the previous iteration's max|k| with
 * 2^6 of headroom.  A trial whose k grows faster than that raises a per-trial flag; at the end of the solve the library
 * reads the flags (ONE stream synchronisation per call, also for JSTSP_DEVICE) and solves exactly those trials again with
 * the three-kernel iteration, whose scales are exact maxima, writing over their S / Y / convergence_error.  No status code
 * is involved: the call returns the same results as the three-kernel iteration for them.  *count is 0 for every input
 * that is a measurement of the reference's system model. */
int jstsp_last_fused_fallbacks(jstsp_ctx *ctx, int *count);

/* Spectral norms inside the ADMM loops (convergence_error of proposed_algorithm.m:67,69, sparse_admm.m:32, mc_admm.m:28):
 * lambda_max of each Gram is computed by a Lanczos run that starts from the Ritz vector of the SAME matrix one iteration
 * earlier and stops when the residual of the Ritz pair is below 1e-5 lambda (a cold n-step run otherwise, and always at the
 * first iteration).  Every JSTSP_LANCZOS_VERIFY-th call (default 32) the cold run is done as well, for all matrices of the
 * call, and its value returned; *count = how many of those checks differed from the warm-started value by more than 2e-5
 * relative in ALL solves on this context since the previous call of this function (the counter is cumulative and cleared by the
 * read: a re-solve of overflowed trials, the chunks of a sweep and both halves of a pipelined JSTSP_HOST call are covered;
 * 0 on every input measured so far; one stream synchronisation). */
int jstsp_last_lanczos_mismatches(jstsp_ctx *ctx, int *count);

/* lambda_max of a sequence of batches of Hermitian matrices (n <= 128): G is [steps][batch][n*n] column-major, lam is
 * [steps][batch] floats.  Matrix t of step s is warm-started from matrix t of step s - 1, exactly as the ADMM loops drive the
 * kernel for convergence_error (proposed_algorithm.m:67,69; sparse_admm.m:32; mc_admm.m:28) - the entry exists so that the
 * tracking can be checked on spectra the solvers do not produce (flat, clustered, crossing eigenvalues).  Accuracy of each
 * value: 2e-5 relative (residual of the Ritz pair below 1e-5 lambda; typically 1e-6), a cold run's 1.5e-6 at step 0. */
int jstsp_lambda_max_sequence_c32(jstsp_ctx *ctx, int n, int batch, int steps, const jstsp_c32 *G, float *lam, int memspace);

/* Structure the last jstsp_proposed_algorithm_c32/_c64 call on this context found in its dictionary B (G2 x M).  The
 * dictionaries of the reference's drivers stack L delayed copies of one pilot frame under the transmit steering vectors
 * (errorVSsnr.m:36-47), which makes them block-Toeplitz: B(ld*Gt + g, m) == B(g, m - ld) for m >= ld, G2 = L*Gt.  The
 * library PROBES that (exact comparison of every entry, once per call) and, where it holds, streams only the first block
 * in each iteration and forms G_B = B B^H from its first block row (1 / L of the product; that also for shapes the one-pass
 * iteration does not take).  *gt = the block height used, 0 = none found (any B is accepted; an unstructured one just costs
 * the full read).  JSTSP_TOEPLITZ=0 in the environment skips the probe.
 * What the structure changes in the results: with JSTSP_TOEPLITZ=1 (compact image, same kernel, same products) NOTHING -
 * bit-identical to the unstructured path.  With the default (2), block height 64 takes the window kernel, which applies the
 * leading columns of each delayed block as separate fp32 terms: fp32-EQUIVALENT to the unstructured path (same accuracy
 * against float64, S within 2e-5 relative of it), not bit-identical.  The probe covers ALL dictionaries of a call and the
 * kernel is chosen per call: one unstructured B among per-trial dictionaries moves every trial of that call to the general
 * kernel, so a trial's result BITS (not its accuracy) can depend on its batch mates.  Results of one call with given inputs
 * are bit-reproducible from run to run. */
int jstsp_last_dictionary_block(jstsp_ctx *ctx, int *gt);

/* S_ls = pinv(A)*Y*pinv(B)   — the LS baseline of the drivers (plot_errorVSsnr.m:83).
 * Factors that fit the in-LDS float64 pinv kernel (see jstsp_pinv_c32; every shape the reference's drivers use)
 * get MATLAB's SVD-based pinv, any rank, any aspect ratio.  Larger factors take the fp32 Gram-inverse route
 * G_A^-1 A^H Y B^H G_B^-1, which needs full rank (N >= Gr, M >= G2, else JSTSP_E_UNSUPPORTED) and loses
 * cond(G) * 6e-8 of relative accuracy.  A JSTSP_HOST call returns JSTSP_E_ILLCOND instead of a truncated or unconverged
 * inverse: when lambda_min/lambda_max < 1e-6, when the eigen route (order <= 128) met an eigenvalue at or below
 * n*eps32*lambda_max (order 128: 1.5e-5), or when Newton-Schulz (order > 128) left a residual ||I - G X||_F / sqrt(n)
 * above 64 times its rounding floor eps32 * lambda_max/lambda_min (JSTSP_DEVICE: jstsp_last_conditioning).
 * Y: N x M x batch; S_out: Gr x G2 x batch. */
int jstsp_ls_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c32 *Y,
                 const jstsp_c32 *A, long long strideA, const jstsp_c32 *B, long long strideB,
                 jstsp_c32 *S_out, int memspace);

/* P = pinv(A)   — MATLAB's pinv as the drivers call it (plot_errorVSsnr.m:83): SVD-based (one-sided Jacobi in
 * float64 on the device), singular values <= max(size(A))*eps(norm(A)) dropped.  A: rows x cols x batch,
 * P: cols x rows x batch.  The matrix must fit the in-LDS kernel: (max*min + min^2) * 16 B <= 156 KiB
 * (e.g. 64 x 64, 140 x 16, 512 x 16), else JSTSP_E_UNSUPPORTED. */
int jstsp_pinv_c32(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c32 *A, jstsp_c32 *P, int memspace);

/* Conditioning of the last call on this context that (pseudo-)inverted a dictionary factor (jstsp_ls_c32,
 * jstsp_pinv_c32, proposed_algorithm 'std'): *rcond_min = the smallest sigma_min/sigma_max of a factor (for the fp32
 * Gram-inverse path of factors too large for the pinv kernel: sqrt(lambda_min/lambda_max) of the Gram, and the
 * relative accuracy of that path is about 6e-8 / rcond^2; 0 when the eigen route dropped a component or a Newton-Schulz
 * residual exceeded its rounding floor; for Newton-Schulz, lambda_min/lambda_max is 1 / (lambda_max(G) lambda_max(G^-1))
 * from the large-order eigen solver, which makes such a call wait for the stream); *ns_residual_max = the largest
 * ||I - G X||_F / sqrt(n) left by the Newton-Schulz inverse of Grams of order > 128 (0 if none ran), reported only.
 * The call's digits are there exactly when rcond_min^2 >= 1e-6: the rule by which a JSTSP_HOST call returns
 * JSTSP_E_ILLCOND.  Measured (tests/test_gpu_std_parity.py): relative error <= 13 * 6e-8 * cond through the pinv
 * kernel and <= 8.2 * 6e-8 * cond^2 through a Gram inverse; on the Gram routes rcond_min is as accurate as the inverse
 * (within 0.1 % of numpy's sigma_min/sigma_max for geometric spectra up to cond 700, 8 % at cond 800 with two
 * clusters).  Synchronises the context's stream.  Either pointer may be NULL. */
int jstsp_last_conditioning(jstsp_ctx *ctx, double *rcond_min, double *ns_residual_max);

/* X = svt(Y, tau)   benchmark_algorithms/svt.m:1-15.   Y, X: Mr x Mt x batch; tau host double[batch]. */
int jstsp_svt_c32(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c32 *Y,
                  const double *tau, jstsp_c32 *X, int memspace);

/* [x_hat, indexSet, v, targetMatrix] = OMP(A, v, m, snr)   benchmark_algorithms/OMP.m:1-32
 * Dense dictionary A: measures x size_d (strideA 0 = shared); v: measures x batch.
 * x_hat: size_d x batch; index_out: m x batch int32 (1-based); target_out: measures x m x batch
 * (may be NULL).  `snr` is unused by the reference and has no parameter here.
 * Selection (OMP.m:17, [~, idx] = max(abs(A'*r))), the same for jstsp_omp_kron_c32: |c|^2 is compared in float64 formed
 * from the fp32 correlation (no overflow or underflow for any finite fp32 input); every atom within 1e-5 of the largest
 * |c| (at most 8 of them) is rescored in float64 by one routine shared by every path, and the largest score wins, the
 * first index among equal ones (MATLAB max; NaN never wins).  So the index set does not depend on the batch size, on
 * whether the dictionary is shared, or on the correlation kernel (gemv, fp32 MFMA, split-f16) wherever the float64
 * margin of every selection is above the orthogonalisation round-off, about 1e-6 relative: exact and near ties of the
 * first iteration, a residual that is exactly 0 (index 1 is then re-selected), v = 0, and inputs scaled by any power of
 * two that keeps them finite are decided as the float64 reference decides them.  A later-iteration near-tie below that
 * round-off can still go either way: the Gram-Schmidt variants (CGS2 for up to 64 problems, MGS above, the Cholesky
 * update of the coefficient-domain Kronecker path) differ in the last bits of the residual. */
int jstsp_omp_c32(jstsp_ctx *ctx, int measures, int size_d, int batch,
                  const jstsp_c32 *A, long long strideA, const jstsp_c32 *v, int m,
                  jstsp_c32 *x_hat, int32_t *index_out, jstsp_c32 *target_out, int memspace);

/* OMP on the Kronecker dictionary Phi = kron(Bf.', Af) given by its factors (never formed):
 * Af: N x Gr, Bf: G2 x M, y: N*M x batch, atoms indexed g + Gr*h (1-based in index_out).
 * In the coefficient domain (Cholesky of the factor Grams) while the factor fits 150 KiB of LDS (m <= 96), with
 * measurement-space Gram-Schmidt above; the selection contract is jstsp_omp_c32's. */
int jstsp_omp_kron_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                       const jstsp_c32 *Af, long long strideA, const jstsp_c32 *Bf,
                       long long strideB, const jstsp_c32 *y, int m,
                       jstsp_c32 *x_hat, int32_t *index_out, int memspace);

/* CoSaMP — the seventh estimator of the timing figure:  s_cosamp = CoSaMP(Phi, y, numOfnz)   plot_time_comparisions.m:96
 * The 3-argument function the driver calls is not vendored, so this is the published algorithm (Needell & Tropp, "CoSaMP:
 * Iterative signal recovery from incomplete and inaccurate samples", Algorithm 1); MATLAB parity is unpinned.
 * One problem: dictionary Phi (measures x size_d), data u, sparsity K, iters >= 1, tol >= 0.
 *     a = 0;  kept = {};  v = u
 *     for it = 1 .. iters
 *         c     = Phi' * v
 *         Omega = the min(2K, size_d) indices of largest |c|^2        (equal values: the smaller index first)
 *         T     = sort(Omega U kept)                                  (|T| <= 3K)
 *         b     = argmin_b || Phi(:,T) b - u ||_2
 *         kept  = the K positions of T with largest |b|^2             (equal values: the smaller index first)
 *         a     = 0;  a(kept) = b(kept)                               (pruned, not re-solved)
 *         v     = u - Phi a
 *         if ||v||_2 <= tol * ||u||_2: stop this problem              (tol = 0: never)
 * `kept` is the index set that was kept, whether or not a kept coefficient is exactly zero.  u = 0 returns a = 0 after zero
 * iterations (resid_out 0, support_out all 0).  JSTSP_E_ARG unless 1 <= K, 2K <= size_d and 3K <= measures (the least
 * squares is then never under-determined), iters >= 1 and tol >= 0.
 * Arithmetic: the whole iteration - c, the least squares, |.|^2, the norms and every selection, prune and stop decision -
 * is float64 on the device for BOTH element types (products of two fp32 values are exact in float64, so a _c32 call is a
 * float64 evaluation on exactly its inputs; the _c64 entries do not narrow).  x_hat is rounded once to fp32 for _c32.
 * Form (csrc/cosamp.hip): coefficient domain.  c0 = Phi' u and G = Phi' Phi are formed once; c = c0 - G a; b solves the
 * gathered normal equations G(T,T) b = c0(T) by Cholesky with one step of refinement; ||v||^2 = ||u||^2 - 2 Re(a' c0) + a' G a
 * (so a relative residual below about 1e-7 is reported as rounding leaves it, possibly 0).  The dense entry forms G
 * (size_d <= 4096); the Kronecker entry never does: an entry of G is one entry of Af' Af times one of conj(Bf Bf').
 * JSTSP_E_UNSUPPORTED: K > 256, size_d > 65536, a dense size_d > 4096, a float64 workspace above 24 GiB.
 * Rank: when a Cholesky pivot of G(T,T) is at or below 1e-12 times its largest diagonal entry (Phi(:,T) numerically rank
 * deficient, for instance a repeated column: both copies tie and enter T together), that problem stops, keeps the iterate
 * it had before this iteration and reports status 1; the other problems are unaffected and the call returns JSTSP_OK.
 * A, u as in jstsp_omp_c32.  x_hat: size_d x batch.  support_out: K x batch int32, 1-based, ascending.  iters_out: int32
 * per problem, iterations completed.  resid_out: double per problem, ||v|| / ||u|| at return.  status_out: int32 per
 * problem, 0 or 1.  The last four may each be NULL.  One launch per step for the whole batch; no flag is read back per
 * iteration; a repeated call is bit-identical and a problem's result does not depend on the batch around it. */
int jstsp_cosamp_c32(jstsp_ctx *ctx, int measures, int size_d, int batch,
                     const jstsp_c32 *A, long long strideA, const jstsp_c32 *u, int K, int iters, double tol,
                     jstsp_c32 *x_hat, int32_t *support_out, int32_t *iters_out, double *resid_out,
                     int32_t *status_out, int memspace);
/* CoSaMP on Phi = kron(Bf.', Af) given by its factors, conventions of jstsp_omp_kron_c32 (atoms indexed g + Gr*h).  The
 * driver's dictionary is of this kind: Phi = kron((B*B').', A), y = vec(Y*B')  (plot_time_comparisions.m:74-75). */
int jstsp_cosamp_kron_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                          const jstsp_c32 *Af, long long strideA, const jstsp_c32 *Bf, long long strideB,
                          const jstsp_c32 *y, int K, int iters, double tol,
                          jstsp_c32 *x_hat, int32_t *support_out, int32_t *iters_out, double *resid_out,
                          int32_t *status_out, int memspace);

/* Joint (MMV) OMP — the drivers' "OMP with MMV" baseline and the second stage of their TSSR recipe
 *   spx.pursuit.joint.OrthogonalMatchingPursuit(A, K).solve(Y)  ->  .Z      plot_errorVSsnr.m:116-117, :158-162
 * sparse-plex is not vendored and not version-pinned (README.md:9): this is the published simultaneous OMP
 * (one support for all columns; atom = argmax_g ||A(:,g)' * R||_p, p = pnorm in {2, 1}; least squares on the support),
 * stopping after K atoms, when all min(N, Gr) independent atoms are in, or when ||R||_F <= 1e-6 ||Y||_F.
 * A: N x Gr (strideA 0 = shared); Y: N x S x batch; Z_out: Gr x S x batch; index_out: NULL or K x batch int32
 * (1-based atoms in selection order, 0 beyond the count); count_out: NULL or batch int32 (atoms selected).
 * Contract (tests/test_gpu_mmv_omp_paths.py, against the float64 oracle on the same complex64 values):
 *   Stop rules, tested in this order per atom: (1) min(K, N, Gr) atoms are in; (2) the chosen atom a is dependent on the
 *   support: ||a - Q Q' a||^2 <= 1e-10 ||a||^2 after two Gram-Schmidt passes (float64 sums), or a = 0 - it is NOT added, the
 *   count stays; (3) after an atom is added, ||R||_F^2 <= 1e-12 ||Y||_F^2 (float64 sums) - the atom counts.  Y = 0 returns
 *   support [1], count 1, Z = 0.  A residual within rounding of rule (3) (a noiseless Y = A Z0: fp32 leaves 1e-7..1e-8 ||Y||)
 *   may take the device one atom further than float64; the first atoms and Z agree.
 *   Ties: the lowest index wins.  Every atom's score is the same arithmetic in the same order, so equal columns and columns
 *   differing by a factor -1 or +-1i score bit-equal and tie exactly.  A selection whose float64 relative gap to the runner-up
 *   is >= 1e-3 is the float64 selection; Z is then within 1e-4 of the float64 Z relative to max|Z| when
 *   cond(A(:,support)) <= 100 (measured: profiles/mmv_measured_tolerances.json, mmv_paths.*.Z).
 *   Scale: each problem is solved on Y * 2^-e with e the exponent of its largest finite component, and Z is scaled back.
 *   Both scalings are exact unless a value underflows (a component of Y more than 2^125 times smaller than the largest, or
 *   an entry of Z below the normal fp32 range): supports and counts do not depend on the scale of Y over the whole fp32
 *   range, and Z of Y * 2^k is Z of Y times 2^k bit for bit (tested: Y * 2^+-70, 2^+-100, asserted on the bits); atoms
 *   with norms within 2^+-40 of 1 are supported (tested: A * 2^+-40, same support, Z within 1e-6 of the rescaled Z),
 *   beyond that the fp32 row scores ||A(:,g)' R||^2 may overflow or vanish.  A NaN or Inf in a problem's Y (tested: NaN,
 *   +Inf, -Inf) ends that problem with a count in [0, K] and status 0; other problems of the batch are not affected.  A repeated call is bit-identical and a problem's
 *   result does not depend on the batch around it or on the memspace. */
int jstsp_mmv_omp_c32(jstsp_ctx *ctx, int N, int Gr, int S, int batch, const jstsp_c32 *A, long long strideA,
                      const jstsp_c32 *Y, int K, int pnorm, jstsp_c32 *Z_out, int32_t *index_out,
                      int32_t *count_out, int memspace);

/* [S, convergence_error] = sparse_admm(Htrue, OH, Dr, Dt, Imax)   benchmark_algorithms/sparse_admm.m:1-36
 * Htrue, OH: Mr x Mt x batch; Dr: Mr x Gr, Dt: Mt x Gt (shared by the batch; Gr*Gt == Mr*Mt
 * as the reference requires, :16).  S_out: Mr x Mt x batch; ce_out: NULL or Imax x batch double. */
int jstsp_sparse_admm_c32(jstsp_ctx *ctx, int Mr, int Mt, int Gr, int Gt, int batch,
                          const jstsp_c32 *Htrue, const jstsp_c32 *OH,
                          const jstsp_c32 *Dr, const jstsp_c32 *Dt, int Imax,
                          jstsp_c32 *S_out, double *ce_out, int memspace);

/* X = mc_svt(OH, Omega, Imax, tau, rho)   benchmark_algorithms/mc_svt.m:1-12 */
int jstsp_mc_svt_c32(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c32 *OH,
                     const float *Omega, int Imax, const double *tau, const double *rho,
                     jstsp_c32 *X_out, int memspace);

/* [X, convergence_error] = mc_admm(Htrue, OH, Omega, Imax, tau, rho)   benchmark_algorithms/mc_admm.m:1-34 */
int jstsp_mc_admm_c32(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c32 *Htrue,
                      const jstsp_c32 *OH, const float *Omega, int Imax, const double *tau,
                      const double *rho, jstsp_c32 *X_out, double *ce_out, int memspace);

/* x = vamp(y, A, sigma, L)   benchmark_algorithms/vamp.m:1-55 (VampGlmEst.m:347-511 with the
 * Bernoulli-Gaussian denoiser SparseScaEstim/CAwgnEstimIn and the CAwgnEstimOut likelihood).
 * Dense dictionary A: M x N with min(M, N) <= 2048 (strideA 0 = shared); y: M x batch; x_out: N x batch.  Above order 128 the
 * eigen-decomposition of A*A' (or A'*A) is the library's block Jacobi (csrc/eig_large.hip): the drivers' own call
 * vamp(y, kron((B*B').', A), 1, numOfnz) with its 512 x 512 dictionary (plot_errorVSsnr.m:79-80,100) goes through unchanged.
 * M <= N runs VampGlmEst.m:402-406 with U, d from A*A'; M > N runs :407-411 with V, d from the eigen-decomposition of
 * A'*A - vamp.m passes opt.U and opt.d but no opt.V, so VampGlmEst.m:196-218 recomputes both in that case.
 * sigma = noise variance passed to the likelihood (every driver passes 1), L = expected number of
 * non-zeros, nit = iterations (the reference always runs 100: its stopping rule is commented out). */
int jstsp_vamp_c32(jstsp_ctx *ctx, int M, int N, int batch, const jstsp_c32 *y, const jstsp_c32 *A,
                   long long strideA, double sigma, double L, int nit, jstsp_c32 *x_out, int memspace);

/* The same for the dictionary the drivers actually pass (plot_errorVSsnr.m:79-80,100):
 *   Phi = kron(Gb.', Af),  y = vec(Y),  Af: Na x Gr (min(Na, Gr) <= 2048; Na > Gr is the M > N branch),  Gb: G2 x G2 Hermitian (G2 <= 8192; above 128
 *   its eigen-decomposition is the library's block Jacobi (csrc/eig_large.hip) - as is every Gram eigenproblem above order 128:
 *   svt / mc_svt / mc_admm / proposed_algorithm with min(rows, cols) in 129..2048, sparse_admm with max(Mr, Mt) in 129..2048).
 * Phi is never formed.  Y: Na x G2 x batch; X_out: Gr x G2 x batch (x = vec(X)). */
int jstsp_vamp_kron_c32(jstsp_ctx *ctx, int Na, int Gr, int G2, int batch, const jstsp_c32 *Y,
                        const jstsp_c32 *Af, long long strideA, const jstsp_c32 *Gb, long long strideG,
                        double sigma, double L, int nit, jstsp_c32 *X_out, int memspace);

/* The two scalar estimators VAMP is built from, stand-alone (they run inside every VAMP iteration as
 * device functions of csrc/vamp_kernels.h - these entries call exactly those functions on arrays, so that they can be tested and used
 * by themselves).  float64 in and out, n real coordinates (the reference real-stacks the complex system, vamp.m:3-4).
 *   jstsp_sparse_sca_estim_f64:  [xhat, xvar] = SparseScaEstim(CAwgnEstimIn(0, var0), p1).estim(rhat, rvar)
 *     MPbased_solvers/main/SparseScaEstim.m:76-166 around main/CAwgnEstimIn.m:94-102,181-184: the Bernoulli-Gaussian posterior mean and
 *     variance with the COMPLEX log-likelihood branch of :100-103 (what vamp.m's r1init = eps*1i selects on real-stacked data), the
 *     activity exponent clipped at +-500 (:108-109), rvar floored at eps (:96).  rvar: one value for all coordinates.
 *   jstsp_cawgn_estim_out_f64:  [zhat, zvar] = CAwgnEstimOut(y, wvar).estim(phat, pvar), scale = 1
 *     MPbased_solvers/main/CAwgnEstimOut.m:97-108: gain = pvar / (pvar + wvar), zhat = gain (y - phat) + phat, zvar = wvar gain
 *     (zvar is one value, returned through *zvar on the host). */
int jstsp_sparse_sca_estim_f64(jstsp_ctx *ctx, long long n, const double *rhat, double rvar, double var0, double p1, double *xhat,
                               double *xvar, int memspace);
int jstsp_cawgn_estim_out_f64(jstsp_ctx *ctx, long long n, const double *y, const double *phat, double pvar, double wvar, double *zhat,
                              double *zvar, int memspace);

/* nmse[t] = min(1, norm(S - Zbar)^2 / norm(Zbar)^2) with spectral norms
 *   plot_errorVSsnr.m:138-141.   S, Zbar: R x C x batch, min(R, C) <= 2048; nmse: batch doubles (same memspace).
 * Conventions (those of the host formula, of MATLAB and of jstsp_nmse_spectral_f64): S == Zbar gives exactly 0; Zbar == 0 gives NaN
 * for S == 0 (0/0) and 1 for any other S (x/0 = Inf, capped); a trial with a NaN or Inf entry in S or in Zbar gives NaN and leaves
 * the other trials of the batch alone.
 * Input scale: D = S - Zbar and Zbar are each brought to a largest |re|, |im| in [1, 2) by an exact power of two per trial before
 * the Gram is formed and the scale is undone in double, so the result does not depend on the unit of the operands: any finite
 * complex64 operands whose difference S - Zbar is finite (the NMSE is the same at 2^-40 and 2^+40 times the operands).
 * min(R, C) > 128: lambda_max is the Rayleigh quotient, in double, of the leading column of the block Jacobi's basis. */
int jstsp_nmse_spectral_c32(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c32 *S,
                            const jstsp_c32 *Zbar, double *nmse, int memspace);

/* rate[t] = log2(real(det(eye(R) + 1/R * Zbar*Zbar' / (noise_var + norm(Zbar - S)^2/norm(Zbar)^2))))
 *   plot_rateVSframelength.m:81,113,130,135 (spectral norms, NMSE not capped).  S, Zbar: R x C x batch, min(R, C) <= 128
 * (the eigenvalues are those of the Gram of the smaller side; R itself may be larger); rate: batch doubles (same memspace).
 * Conventions: S == Zbar scores with an NMSE of exactly 0; Zbar == 0 gives NaN for S == 0 (0/0) and 0 for any other S (no signal:
 * log2 det(I)); a trial with a NaN or Inf entry in S or in Zbar gives NaN and leaves the other trials alone.
 * Input scale: as jstsp_nmse_spectral_c32 - the eigenvalues are taken of the scaled Zbar (Rayleigh quotients of the Jacobi basis, in
 * double; a negative one is rounding noise: summed while |lambda c| < 2^-10, clamped to 0 beyond) and brought back in double. */
int jstsp_rate_c32(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c32 *S, const jstsp_c32 *Zbar,
                   double noise_var, double *rate, int memspace);

/* ---- device-side construction of the solver inputs (the caller side of the path) ------------
 * plot_errorVSsnr.m:57-136 for trials [trial0, trial0 + batch) of sweep point `sweep_idx`:
 * channel (wideband_mmwave_channel.m:1-39), 4-QAM Toeplitz pilots (qam4mod.m:7-8, plot_errorVSsnr.m:63-67),
 * noise (:60), random spatial sampling (proposed_hbf.m:1-44), A and B (:132-136), tau_Y / tau_Z / rho
 * (:127-130, rho from the 6th largest eigenvalue as eigs() returns it) and indx_S (:143).
 * Random numbers: Philox4x32-10 keyed by (seed, sweep_idx, global trial index) - independent of
 * batch and of the sharding over GPUs. */
typedef struct jstsp_model {
    int Nt, Nr, L;          /* antennas, delay taps                                  plot_errorVSsnr.m:8-12 */
    int T_prop;             /* training length of the proposed scheme (T*Nt)         :23                     */
    int Mr, Mr_e;           /* RF chains sampled per slot / extended                 :15-16                  */
    int Gr, Gt;             /* dictionary sizes                                      :13-14                  */
    int clusters, rays;     /* total_num_of_clusters, total_num_of_rays              :18-19 (ignored for a supplied channel) */
    int T_hbf;              /* training length of the conventional HBF baseline (0 = not wanted) :22         */
    int shared_pilots;      /* 0: new pilots every trial (plot_errorVSsnr.m:63-67); 1: one pilot set per sweep point */
    double noise_var;       /* 10^(-snr_db/10)                                       :49                     */
    /* what the sibling drivers change in the construction (all-zero = plot_errorVSsnr.m):                   */
    int beamformer;         /* JSTSP_BF_ZC: createBeamformer(Nr,'ZC') :124; JSTSP_BF_DFT: 'fft' (plot_errorVSframelength.m:123,
                               plot_errorVSnt.m:123, plot_rateVSframelength.m:116) and 'ps' (plot_errorVSadmmiters.m:47,
                               plot_errorVSzy.m:53) - createBeamformer.m:5 and :12-13 are the same unitary DFT matrix */
    int rho_rule;           /* JSTSP_RHO_MIN6: min(eigs(Y'*Y)) :129-130; JSTSP_RHO_MAX: max(eigs(Y'*Y))
                               (plot_errorVSdelays.m:128, plot_errorVSnrf.m:128, plot_errorVSnt.m:129, plot_errorVSpaths.m:128) */
    double rho_scale;       /* factor on rho (0 = 1; plot_errorVSzy.m:65 halves it; plot_errorVSsnr_approx.m:51-53's
                               rho = sqrt(lambda_6 (tau_X + tau_S)/2) with tau_S = tau_X/2 is sqrt(0.75) x the :129-130 rule) */
    int pilots;             /* JSTSP_PILOTS_QAM4: 4-QAM symbols (qam4mod.m:7-8, plot_errorVSsnr.m:63-67);
                               JSTSP_PILOTS_GAUSS: s = 1/sqrt(2)*(randn + 1j*randn), the training of
                               wideband_hybBF_comm_system_training.m:19-22 (the builder of plot_errorVSsnr_approx.m:46: with
                               beamformer = JSTSP_BF_DFT (:10), Mr = round(subSamplingRatio*Nr) (:5), Mr_e = Nr, T_prop = T
                               and rho_scale = sqrt(0.75) this call IS that function + the driver's lines :50-58) */
} jstsp_model;
/* createBeamformer.m kinds.  JSTSP_BF_QUANTIZED ('quantized', N_q = 6, :25-31) and JSTSP_BF_QUANTIZED4 ('quantized_4',
 * N_q = 4, :18-24) are for jstsp_beamformer_* and jstsp_ase_trials_c32; jstsp_build_trials_c32 accepts only ZC and DFT. */
enum { JSTSP_BF_ZC = 0, JSTSP_BF_DFT = 1, JSTSP_BF_QUANTIZED = 2, JSTSP_BF_QUANTIZED4 = 3 };
enum { JSTSP_RHO_MIN6 = 0, JSTSP_RHO_MAX = 1 };
enum { JSTSP_PILOTS_QAM4 = 0, JSTSP_PILOTS_GAUSS = 1 };

/* Output arrays of jstsp_build_trials_c32 (NULL = not wanted); column-major per trial, trial index last.
 * With N = Mr_e, M = T_prop, G2 = L*Gt, Np = clusters*rays: */
typedef struct jstsp_trials {
    jstsp_c32 *subY;        /* N x M x batch                                                                  */
    float *Omega;           /* N x M x batch                                                                  */
    jstsp_c32 *A;           /* N x Gr        (trial-independent: beamformer x DFT dictionary)                 */
    jstsp_c32 *B;           /* G2 x M x batch                                                                 */
    jstsp_c32 *Zbar;        /* Gr x G2 x batch   the true angle-delay channel [Z_1 ... Z_L]                   */
    jstsp_c32 *H;           /* Nr x (Nt*L) x batch   [H_1 ... H_L]                                            */
    int32_t *indx_S;        /* (Gr*G2) x batch, 1-based: stable descending order of |vec(Zbar)|               */
    double *tau_Y, *tau_Z, *rho;   /* batch each, HOST memory in either memspace                              */
    jstsp_c32 *Y_hbf;       /* Nr x T_hbf x batch    hbf.m:24                                                 */
    jstsp_c32 *A_hbf;       /* Nr x Gr               plot_errorVSsnr.m:74                                     */
    jstsp_c32 *B_hbf;       /* G2 x T_hbf x batch    :75-78 (requires B)                                      */
    /* the raw draws, for checking the construction against a CPU restatement */
    jstsp_c32 *gains;       /* (L*Np) x batch, index l*Np + p                                                 */
    float *u_r, *u_t;       /* Np x batch     uniform draws of tap 1's angle samplers                         */
    jstsp_c32 *noise;       /* Nr x T_prop x batch   randn + 1j*randn, unscaled                               */
    uint8_t *qam_idx;       /* batch x Nt x T_prop (row-major), values 0..3 in the alphabet order of qam4mod.m:7 */
    jstsp_c32 *pilot_sym;   /* batch x Nt x T_prop (row-major): the pilot symbols s (JSTSP_PILOTS_GAUSS: the draws
                               randn + 1j*randn BEFORE the 1/sqrt(2) of ...training.m:20; QAM4: the alphabet values) */
} jstsp_trials;

int jstsp_build_trials_c32(jstsp_ctx *ctx, const jstsp_model *model, uint64_t seed, int sweep_idx,
                           long long trial0, int batch, const jstsp_trials *out, int memspace);

/* The same construction from a channel the caller supplies - NYUSIM or ray-tracing output, a measured channel - instead of the
 * drawn one: the first lines of plot_errorVSsnr_nyuwireless.m (:60-69), which loads Hf{l}, one matrix per delay tap, and cuts and
 * scales it.  Everything downstream of H is the code of jstsp_build_trials_c32 (csrc/inputgen.hip: one body, two entry points).
 *  - Hsrc: column-major taps as MATLAB stores H(:,:,l): tap l starts at Hsrc + l*ld_rows*ld_cols, its entry (r, s) is at
 *    r + ld_rows*s; ld_rows >= Nr, ld_cols >= Nt, the leading Nr x Nt block is used (Hfl(1:Nr, 1:Nt), :63-64).  strideH = 0: one
 *    channel for every trial (what the driver does); otherwise trial t of the call reads Hsrc + t*strideH, strideH >=
 *    L*ld_rows*ld_cols.  Same memspace as the outputs.
 *  - normalize, per tap, with s = norm(H_l), the largest singular value: JSTSP_CHAN_ASIS H_l as given (the stored bits are the
 *    input bits); JSTSP_CHAN_REFERENCE H_l / s^2 - lines :65-66 AS WRITTEN, rho = 1/norm(H(:,:,l))^2; H(:,:,l) = rho*H(:,:,l), which
 *    leaves a tap of spectral norm 1/s, not 1: the quirk is kept; JSTSP_CHAN_UNIT H_l / s.  Each entry is scaled in float64 and
 *    rounded once to fp32.
 *  - sigma_max: L x batch doubles (L when strideH = 0), HOST memory in either memspace like tau_Y; receives s in every mode;
 *    NULL = not wanted.  s is sqrt(lambda_max) of the float64 Hermitian Gram on the smaller side (order min(Nr, Nt) <= 64, in
 *    LDS, the Jacobi of the float64 solvers), of the tap scaled exactly by a power of two so that taps of size 2^+-40 lose
 *    nothing; a value does not depend on the batch it is computed in.
 *  - model: clusters and rays are ignored (may be 0); every other field means what it means above.
 *  - out: gains, u_r and u_t must be NULL (JSTSP_E_ARG: nothing was drawn); H returns the cut and scaled channel in the builder's
 *    layout.  Noise, pilot symbols and Omega come from the same Philox streams: for equal model, seed, sweep and trial both entry
 *    points return the same noise, qam_idx, pilot_sym and Omega bits.
 *  - JSTSP_E_SHAPE: ld_rows < Nr, ld_cols < Nt, a non-zero stride that is too short; JSTSP_E_ARG: bad normalize; JSTSP_E_NULL:
 *    Hsrc NULL; JSTSP_E_ILLCOND: a NaN or Inf in a used block, or s == 0 under _REFERENCE / _UNIT - the message names the tap and
 *    the trial, and no output has been written (entries outside the used block are never read); JSTSP_E_UNSUPPORTED:
 *    min(Nr, Nt) > 64 when s is needed (JSTSP_CHAN_ASIS without sigma_max has no such limit).
 *  - The call waits for its stream once before it builds (s and the flag word come to the host in one copy), in either memspace.
 *  Asserted (tests/test_gpu_measured_channel.py): the drawn path's H passed back JSTSP_CHAN_ASIS returns every array of the drawn
 *  call on the bits; against the float64 oracle on the cut and scaled channel the tolerances of jstsp_build_trials_c32; sigma_max
 *  within 1e-12 relative of numpy's norm(H_l, 2). */
enum { JSTSP_CHAN_ASIS = 0, JSTSP_CHAN_REFERENCE = 1, JSTSP_CHAN_UNIT = 2 };
int jstsp_build_trials_from_channel_c32(jstsp_ctx *ctx, const jstsp_model *model, uint64_t seed, int sweep_idx,
                                        long long trial0, int batch,
                                        const jstsp_c32 *Hsrc, int ld_rows, int ld_cols, long long strideH, int normalize,
                                        const jstsp_trials *out, double *sigma_max, int memspace);

/* The same construction for frame `frame` of a time-varying channel: trial t is a SEQUENCE of channels and `frame` the position in
 * it - what a warm start of the ADMM (jstsp_proposed_resume_f64 / _c32) is measured on.  The geometry of a sequence is fixed and
 * its path gains follow a first-order autoregression; one body with the two builders above (csrc/inputgen.hip).
 *  - Geometry: u_r, u_t (wideband_mmwave_channel.m:20-24) are those of jstsp_build_trials_c32 for the same (seed, sweep_idx, trial),
 *    on the bits, at every frame.
 *  - Gains: let w_k[i] be the gain draw of jstsp_build_trials_c32 (wideband_mmwave_channel.m:19, 1/sqrt(2) (randn + 1j*randn), fp32) at Philox
 *    element i + (k << 32) of the trial's gain stream, so that w_0 is that call's `gains`.  Then
 *        g_f = corr^f w_0 + sqrt(1 - corr^2) * sum_{k=1..f} corr^(f-k) w_k,
 *    the recursion g_f = corr g_{f-1} + sqrt(1 - corr^2) w_f in closed form: every frame has the statistics of a drawn channel
 *    (:19), and E[g_f conj(g_{f-k})] = corr^k.  Each component is accumulated in float64 in ascending k, one fma per term on the
 *    widened fp32 draws with the coefficient pow(corr, f-k) (times sqrt(1 - corr^2) for k >= 1) in float64, and rounded once to
 *    fp32.  A term whose coefficient is exactly zero is skipped: frame 0 returns the bits of w_0 for any corr, corr = 1 returns
 *    w_0 at every frame, corr = 0 returns w_f.  A frame is a function of (seed, sweep_idx, trial, frame, corr) alone: of no earlier
 *    call, of no batch and of no sharding.  COST: O(frame) Philox calls per gain, L*Np*batch gains per call.
 *  - Channel: wideband_mmwave_channel.m:24-38 on (g_f, u_r, u_t), the kernel of jstsp_build_trials_c32 unchanged.
 *  - Noise (plot_errorVSsnr.m:60), pilot symbols (:63-67) and Omega (proposed_hbf.m:36-40) of frame f are those of
 *    jstsp_build_trials_c32 with the 64-bit sweep word sweep_idx + ((uint64_t)frame << 32) in the Philox key; with shared_pilots
 *    the shared key is formed from the same word.  Frame 0 therefore IS jstsp_build_trials_c32: every array, on the bits.
 *  - Everything after H (R, subY, Zbar, A, B, tau_Y / tau_Z / rho, indx_S, the *_hbf outputs) is the code of jstsp_build_trials_c32.
 *  - out: gains returns g_f; u_r, u_t, noise, qam_idx, pilot_sym and H as in jstsp_build_trials_c32.
 *  - JSTSP_E_ARG: corr outside [0, 1] or NaN, frame < 0 or frame > 65535; every other code as jstsp_build_trials_c32.  Nothing is
 *    written before the arguments are accepted.
 *  Asserted (tests/test_gpu_tracking.py): frame 0 equals the drawn call on the bits for corr in {0, 0.5, 1}; corr = 1 keeps gains,
 *  H, Zbar and indx_S of frame 0 while noise, pilots, Omega and subY change; g_f within 2^-23 max|g| of the float64 recursion run
 *  on the innovations the corr = 0 calls return; the oracle's tolerances of jstsp_build_trials_c32 downstream of (g_f, u_r, u_t);
 *  a trial's arrays do not depend on the batch it is built in nor on the memspace; |g_f|^2 and the lag correlations corr^k within
 *  5 sigma over 4096 sequences. */
int jstsp_build_trials_tracked_c32(jstsp_ctx *ctx, const jstsp_model *model, uint64_t seed, int sweep_idx,
                                   long long trial0, int batch, int frame, double corr,
                                   const jstsp_trials *out, int memspace);

/* jstsp_build_trials_tracked_c32 with one addition: the angle of every path performs a random walk from frame to frame, so the
 * support of Zbar moves across the dictionary grid - the case a warm start's inherited v, S does not fit.  A fourth channel source
 * of the one body (csrc/inputgen.hip); jstsp_model and jstsp_trials are unchanged.
 *  - Model: let phi_0[p] = beta*(e0 - cosh(u[p])) be the angle the drawn call forms from u_r or u_t (wideband_mmwave_channel.m:56-62).
 *    Then phi_f[p] = phi_0[p] + drift * sum_{k=1..f} z_k[p]: drift is the standard deviation of one frame's increment, in radians;
 *    the walk is independent per path and per array end (receive, transmit).  No mean reversion.
 *  - Draws: z_k[p] is the first component of the Box-Muller pair on the Philox word at element p + (k << 32) of the trial's u_r
 *    (receive) or u_t (transmit) stream - the second counter word is unused by these streams (Np < 2^32); element p at k = 0 stays
 *    the uniform draw u.  The device of the gains above.
 *  - Arithmetic: one thread per (path, end) sums the widened fp32 normals in float64 in ascending k and multiplies ONCE by drift
 *    (the offsets are exactly linear in drift); the channel kernel adds the offset once to phi_0 in float64 and forms the steering
 *    phase sincos(-pi*sin(-phi_f)*n) in float64 as before.  A frame is a function of (seed, sweep_idx, trial, frame, corr, drift)
 *    alone: of no earlier call, of no batch and of no sharding.  COST: O(frame) Philox calls per angle, 2*Np*batch angles per call,
 *    on top of the gains' O(frame).
 *  - Channel: wideband_mmwave_channel.m:24-38 on (g_f, phi_f).  The drawn, tracked, capacity and spectrum paths launch the
 *    kernel without the offsets and generate what they generated before.
 *  - out: u_r, u_t are the drawn call's bits at every frame; gains is g_f of the tracked entry; everything after H is the shared
 *    body, so indx_S is the frame's own true order.  dphi_r, dphi_t: Np x batch doubles each, in the memspace of the other arrays,
 *    receive phi_f - phi_0; NULL = not wanted.
 *  - Identities: drift == 0 at any frame returns every array of jstsp_build_trials_tracked_c32 on the bits; frame 0 at any drift
 *    returns jstsp_build_trials_c32 on the bits; dphi_* compare equal to zero in both cases.
 *  - JSTSP_E_ARG: drift < 0, NaN or Inf; corr and frame as jstsp_build_trials_tracked_c32 (the messages keep the prefix
 *    build_trials_tracked).  Nothing is written before the arguments are accepted.
 *  Asserted (tests/test_gpu_drift.py): the two identities on all 16 arrays; dphi(drift = s) == s * dphi(drift = 1) exactly, at
 *  frame 65535 too; keyed by (seed, sweep, sequence, end), not by batch or memspace; H within 2e-6 of the float64 channel on
 *  (gains, phi_0 + dphi) and the oracle's tolerances downstream; increments of mean 0, variance 1 and no correlation between
 *  frames, ends, paths and sequences within 5 sigma over 4096 sequences; the refusals. */
int jstsp_build_trials_tracked_drift_c32(jstsp_ctx *ctx, const jstsp_model *model, uint64_t seed, int sweep_idx,
                                         long long trial0, int batch, int frame, double corr, double drift,
                                         const jstsp_trials *out, double *dphi_r, double *dphi_t, int memspace);

/* [~, indx] = sort(abs(vec(S)), 'descend') per trial (plot_errorVSsnr.m:143), for an S that is not the true channel's - the
 * previous frame's estimate of a tracker - without leaving the device (csrc/support.hip).  S: Gr x G2 x batch, column-major;
 * indx_S: (Gr*G2) x batch, 1-based, the layout every indx_S argument of the solvers takes.  The _f64 form reads interleaved
 * (re, im) doubles, the memory of a jstsp_c64 array.
 *  - Key: |z|^2 = x*x + y*y, in fp32 (_c32) or float64 (_f64).  Equal keys come in ascending index: the exact zeros of a
 *    soft-thresholded S follow the non-zeros in index order.  A NaN key sorts before everything, +Inf next, as MATLAB's
 *    descending sort does; NaNs tie with each other whatever their payload.
 *  - _c32 forms its key with the device function of the trial builder (csrc/support_key.h) and sorts the same 64-bit words
 *    (key above index) by the same segmented radix sort: support_order(Zbar) of a built trial is its indx_S on the bits.
 *  - _f64: the keys alone are sorted; an entry's class is the first position of its key in its trial's sorted keys; the words
 *    (class above index) are sorted.  No step relies on a stable sort.  One route per precision; an order is a function of its own
 *    trial alone: of no batch and no memspace.  COST: one (_c32) or two (_f64) radix sorts of Gr*G2*batch 64-bit words.
 *  - Workspace from the context's arena: 16 (_c32) or 24 (_f64) bytes per entry plus the sort's own, per chunk of at most
 *    2^31 - 1 entries.  Both memspaces.
 *  - JSTSP_E_SHAPE: a non-positive dimension or Gr*G2 >= 2^31; JSTSP_E_NULL: a NULL array.  Nothing is written then.
 *  Asserted (tests/test_gpu_support_order.py): equal to the builder's indx_S on Zbar; exact against a stable host argsort of the
 *  negated key on engineered ties, an all-zero trial, a NaN and an Inf, a 64 x 512 continuous trial and a solver's own sparse S, in
 *  both precisions; independent of batch and memspace; proposed_algorithm_angles_f64 on it returns the bits of the builder's. */
int jstsp_support_order_c32(jstsp_ctx *ctx, int Gr, int G2, int batch, const jstsp_c32 *S, int32_t *indx_S, int memspace);
int jstsp_support_order_f64(jstsp_ctx *ctx, int Gr, int G2, int batch, const double *S, int32_t *indx_S, int memspace);

/* The order of a support widened over neighbouring angle cells (csrc/support.hip): a support prior that can follow a peak which
 * moves a cell per frame.  S: Gr x (Gt*L) x batch as jstsp_support_order_* takes it, column c = l*Gt + g transmit cell g of delay
 * tap l; indx_S: (Gr*Gt*L) x batch, 1-based column-major linear indices.  In the key space of csrc/support_key.h (key =
 * ~bits(|z|^2), NaN -> 0, a smaller key is a larger magnitude):
 *    own(r, l, g) = key(S(r, l*Gt + g))
 *    nbr(r, l, g) = min over |dr| <= wr, |dg| <= wt of own((r + dr) mod Gr, l, (g + dg) mod Gt)
 *  - Both angle grids are DFT grids (wideband_mmwave_channel.m:9-10), so the window is circular in r and in g; it never crosses
 *    a delay block: g wraps inside its own l.
 *  - primary = 0 ("neighbourhood"): ascending (nbr, own, index) - a strong entry, directly followed by its window in order of the
 *    window entries' own magnitude.  primary = 1 ("ties"): ascending (own, nbr, index) - the plain order, equal own keys (the exact
 *    zeros of a masked, thresholded S) ordered by their strongest neighbour instead of by index.
 *  - wr = wt = 0: nbr == own, and either primary is jstsp_support_order_* on the bits (and takes its route).  A NaN propagates to
 *    its window (key 0), as it would in MATLAB's max.
 *  - Route: one kernel reads S once and writes own and nbr - per (trial, delay block, tile) the keys in LDS (64 x 64 at most),
 *    the minimum along the rows, then along the columns; a block of at most 64 x 64 wraps by its LDS index, a larger one is
 *    tiled with a halo read through the ring.  Then the _f64 route of jstsp_support_order_* with one more field: the own keys
 *    sorted alone, class = lower bound in that list (nbr values are own keys), the words (class_a << 2w | class_b << w | index)
 *    sorted over 3w bits.  An order is a function of its own trial alone: of no batch, no chunk and no memspace.  COST: two radix
 *    sorts of Gr*Gt*L*batch 64-bit words in either precision; workspace 32 bytes per entry plus the sort's own.  Both memspaces.
 *  - Refused, indx_S untouched: JSTSP_E_SHAPE - Gr, Gt, L or batch not positive, or Gr*Gt*L > 2^21 (3w <= 63 bits);
 *    JSTSP_E_ARG - a negative radius; JSTSP_E_ARG - 2*wr+1 > Gr or 2*wt+1 > Gt (the window would meet itself round the ring);
 *    JSTSP_E_ARG - primary not 0 or 1; JSTSP_E_NULL - a NULL array.
 *  Asserted (tests/test_gpu_support_order_wide.py), exact against the numpy reference of tests/wide_ref.py in both precisions and
 *  both primaries: engineered 6 x 4 x 3 trials (corner spikes, overlapping windows, ties, zeros, a NaN and an Inf) at five radii,
 *  5 x 7 at the largest legal window, a 64 x 512 trial, a tiled 64 x 512 x 1 and a 150 x 70 x 1 block at a radius above one
 *  launch's halo; radius 0 equal to jstsp_support_order_*; no batch or memspace dependence; the solver round trip; the refusals. */
int jstsp_support_order_wide_c32(jstsp_ctx *ctx, int Gr, int Gt, int L, int batch, const jstsp_c32 *S,
                                 int wr, int wt, int primary, int32_t *indx_S, int memspace);
int jstsp_support_order_wide_f64(jstsp_ctx *ctx, int Gr, int Gt, int L, int batch, const double *S,
                                 int wr, int wt, int primary, int32_t *indx_S, int memspace);

/* The head of an order without the sort (csrc/support_top.hip, the kernel in csrc/support_top.h): indx_top(:, t), count x batch,
 * 1-based, is the first `count` entries of jstsp_support_order_f64 of trial t, bit for bit.  V: Gr x G2 x batch interleaved
 * (re, im) doubles, the memory of a jstsp_c64 array.
 *  - Key and order: support_key(double2) of csrc/support_key.h, ascending key, equal keys in ascending index; a NaN first, then
 *    +Inf - the order of jstsp_support_order_f64.
 *  - 1 <= count <= min(Gr*G2, JSTSP_SUPPORT_TOP_MAX); JSTSP_E_ARG otherwise.  The other refusals are those of
 *    jstsp_support_order_f64 (JSTSP_E_SHAPE, JSTSP_E_NULL, a bad memspace).  Nothing is written on a refusal.
 *  - Route: one workgroup of 1024 threads per trial, one launch for the batch.  A radix select on the 64-bit key (eight
 *    histogram passes, top byte first) gives the count-th key thr; the entries with key < thr are compacted into LDS; those with
 *    key == thr are admitted in ascending index by an ordered ballot count until count is reached and written straight to
 *    their places, so a tie class of any size - the exact zeros of a thresholded S - costs no LDS; the strict part is sorted in
 *    LDS by (key, index) with a bitonic network.  Static LDS 48 KiB (4096 keys and indices) plus a histogram; no dynamic LDS.
 *  - Every count is an integer sum in a fixed order: a trial's list depends on no batch and no memspace.
 *  - No workspace on the device path; a JSTSP_HOST call stages V and the list in the context's arena, per chunk of at most
 *    2^31 - 1 entries.  COST: ten reads of the trial, which stays in L2; no vendor sort.
 *  - The same kernel has a second writer, rank[e] for every entry of the trial (position in the list, or 0x7fffffff): what
 *    jstsp_proposed_refresh_f64 runs inside its loop.
 *  Asserted (tests/test_gpu_support_top.py), exact against jstsp_support_order_f64(V)(1:count, :) and a stable host argsort:
 *  engineered 6 x 4 x 3 trials with duplicate magnitudes across the threshold, a NaN and an +Inf; g = 1, 255, 257; count = 1 and
 *  count = g; 64 x 128 with 6000 exact zeros at count 4096 (a tie class larger than the LDS list); 64 x 512 at counts 4096 and
 *  510; values scaled by 2^+-500; an all-zero trial; no batch or memspace dependence; the refusals. */
#define JSTSP_SUPPORT_TOP_MAX 4096
int jstsp_support_top_f64(jstsp_ctx *ctx, int Gr, int G2, int batch, const double *V, int count, int32_t *indx_top, int memspace);
/* The same for an fp32 S (Gr x G2 x batch jstsp_c32): the first `count` entries of jstsp_support_order_c32 of each trial, bit for
 * bit.  One template body with the float64 kernel; the key is the 32-bit support_key(float2) of csrc/support_key.h - the trial
 * builder's indx_S and jstsp_support_order_c32's - so the radix select takes four passes, and the static LDS is 32 KiB (4096 keys
 * and 4096 indices of 4 bytes) plus the histogram.  count, the refusals and their messages, the staging of a JSTSP_HOST call and
 * the second writer (rank) are those of jstsp_support_top_f64; jstsp_proposed_refresh_c32 runs the kernel inside its loop.
 *  Asserted (tests/test_gpu_support_top32.py), exact against jstsp_support_order_c32(S)(1:count, :) and a stable host argsort of
 *  the fp32 key: g = 12, 1000, 1025, 8192, 32768 at count 1, 40, g (g <= 4096) and 4096; duplicate magnitudes across the
 *  threshold, a zero tie class larger than count, NaN entries, a strict part of 4095 entries; no batch or memspace dependence;
 *  the refusals. */
int jstsp_support_top_c32(jstsp_ctx *ctx, int Gr, int G2, int batch, const jstsp_c32 *S, int count, int32_t *indx_top, int memspace);

/* ---- achievable spectral efficiency of the combiners (plot_capacity.m, plot_ee.m; csrc/capacity.hip) ----------------------
 * createBeamformer(N, kind) (createBeamformer.m:5-32) for kind = JSTSP_BF_ZC ('ZC'), JSTSP_BF_DFT ('fft' = 'ps'),
 * JSTSP_BF_QUANTIZED ('quantized') and JSTSP_BF_QUANTIZED4 ('quantized_4'): W (N x N, column-major, same memspace).  The
 * phase of every entry is reduced in integers before sincospi; the quantized kinds keep the reference's construction, each of
 * the 2^Nq phase indices repeated ceil(N/2^Nq) times in a row (at N = 64 'quantized' is the unitary DFT; at N = 128 its
 * columns come in identical pairs; at N = 32 it is not orthogonal).  Asserted (tests/test_gpu_capacity.py), N in
 * {1, 7, 32, 64, 100, 128, 256}: |W - W_64| sqrt(N) < 1e-6 for the _c32 form (measured 1.9e-7) and < 4e-14 N for the _c64
 * form (measured 8.3e-15 N: the float64 transcription's own error on its unreduced phases); both memspaces give the same bits. */
int jstsp_beamformer_c32(jstsp_ctx *ctx, int N, int kind, jstsp_c32 *W, int memspace);
int jstsp_beamformer_c64(jstsp_ctx *ctx, int N, int kind, jstsp_c64 *W, int memspace);

/* ase[t] = real(log2(det(eye(Mr) + scale * W_c' * (Y_t Y_t') * W_c)))   plot_capacity.m:47,52,57,64, plot_ee.m:48-65
 * with W_c = W(:, cols(:, t)) (cols: Mr x batch, 1-based, same memspace) or W(:, 1:Mr) when cols is NULL (hbf.m:23).
 * Y: Nr x T x batch; W: Nr x Ncols, shared by the batch; ase: batch doubles (same memspace).  The scale of the drivers is
 * 1/(square_noise_variance * Nt).  P = W_c' Y is accumulated in fp64 from the operands, the Gram is taken on the smaller side
 * (n = min(Mr, T), Sylvester) and factorised by an fp64 Cholesky; n > 64 returns JSTSP_E_UNSUPPORTED.  A column index outside
 * 1..Ncols gives NaN for its own trial (nothing is read through it); non-finite input gives NaN.  The _c64 form reads double
 * operands and computes the same way.  Asserted (tests/test_gpu_capacity.py): relative error against float64 on the same operand
 * values <= 1e-13 (_c32) / 1e-14 (_c64) (measured 2.3e-15 / 2.3e-16) for Mr < T, Mr > T, Mr = 1, Mr = Ncols, T = 1, n = 64 and
 * duplicated columns, in both memspaces; Y = 0 gives 0 exactly; cols = NULL gives the bits of cols = 1..Mr; prefixes of one
 * codebook give a non-decreasing ASE; an Inf or NaN in Y gives NaN for its own trial only (both forms). */
int jstsp_ase_c32(jstsp_ctx *ctx, int Nr, int T, int Ncols, int Mr, int batch, const jstsp_c32 *Y, const jstsp_c32 *W,
                  const int32_t *cols, double scale, double *ase, int memspace);
int jstsp_ase_c64(jstsp_ctx *ctx, int Nr, int T, int Ncols, int Mr, int batch, const jstsp_c64 *Y, const jstsp_c64 *W,
                  const int32_t *cols, double scale, double *ase, int memspace);

/* One combiner design of jstsp_ase_trials_c32: the codebook createBeamformer(Nr, kind) and
 *   pool = 0: its first n_cols columns (hbf.m:23; plot_capacity.m:45-57: DBF = ('ZC', Nr), HBF-PS = ('quantized', Mr),
 *             HBF-ZC = ('ZC', Mr));
 *   pool > 0: n_cols columns drawn per trial from the first pool, ind = randperm(pool), ind(1:n_cols) (plot_capacity.m:61-64:
 *             proposed = ('quantized', Mr, Mr_e)). */
typedef struct { int kind; int n_cols; int pool; } jstsp_ase_design;

/* plot_capacity.m:35-64 / plot_ee.m:36-65 for trials [trial0, trial0 + batch) of sweep point sweep_idx: the ASE of every design
 * on one realisation.  The channel H and the pilot symbols of trial t are exactly those jstsp_build_trials_c32 returns for
 * trial t of the same (model, seed, sweep_idx) (same Philox streams); Y = [H_1 .. H_L] Psi is noise-free (the drivers call
 * hbf / proposed_hbf with N = zeros) and T = model->T_prop; scale = 1/(noise_var * Nt).  Fields read: Nt, Nr, L, T_prop,
 * clusters, rays, shared_pilots, noise_var, pilots.  The codebook columns are generated from their phase indices on the device
 * (never read from memory).  The column subsets of the pool > 0 designs: the n_cols smallest of pool Philox keys (stream 7,
 * element (design index << 32) + i).  ase: n_designs x batch (ase[d + n_designs*t]); cols (optional, NULL = not wanted): per trial
 * the 1-based subsets of the pool > 0 designs one after the other, in design order (sum of their n_cols) x batch.  Both in
 * memspace.  1 <= n_designs <= 8; min(n_cols, T_prop) <= 64.  No _c64 form: no complex array crosses this boundary.
 * Asserted: relative error <= 2e-12 per trial (measured 3.7e-13) against float64 ASE of jstsp_build_trials_c32's H and pilot
 * symbols with the returned columns (three panel shapes, four Mr values, all four designs); a trial's values and columns do
 * not depend on the batch it is computed in, nor on the memspace; the pilot options (shared_pilots, JSTSP_PILOTS_GAUSS) follow
 * jstsp_build_trials_c32; the subsets are uniform (per-index frequency n_cols/pool within 5 sigma); panel-1
 * means at 2000 trials lie within 4 standard errors of a numpy run of the reference's own samplers. */
int jstsp_ase_trials_c32(jstsp_ctx *ctx, const jstsp_model *model, const jstsp_ase_design *designs, int n_designs,
                         uint64_t seed, int sweep_idx, long long trial0, int batch, double *ase, int32_t *cols,
                         int memspace);

/* ---- singular values, and the spectrum sweep of plot_rankR.m (csrc/svdvals.hip) ---------------------------------------------
 * sv(:, t) = svd(Y_t): the min(rows, cols) singular values of each matrix, descending, as doubles in the memspace of Y
 * (sv[k + min(rows, cols)*t]).  Y: rows x cols x batch, column-major.  Computed by a one-sided (Hestenes) Jacobi iteration in
 * float64 on the columns of Y itself (of Y^H when rows < cols), one workgroup per matrix with the matrix in LDS - NOT through
 * a Gram matrix, which squares the condition number and returns a zero singular value near sqrt(eps) sigma_1: the values that
 * decide a numerical rank are accurate to eps sigma_1 here.  No singular vectors (jstsp_svd_f64 returns them).  The operand is scaled by a power of two
 * first, so any finite input is safe; the sweeps stop when one rotates nothing (|c_p^H c_q| <= sqrt(m) eps |c_p| |c_q| for
 * every pair; columns that have fallen to eps |Y|_F / sqrt(n) are zero singular values and are left alone) or after 30.  Shapes: min(rows, cols) <= 64 and rows * cols <= 8192 (128 KiB of complex double), else
 * JSTSP_E_UNSUPPORTED - there is no fall-back.  An Inf or NaN entry gives NaN for all values of its own matrix only.  The _c64
 * form reads double operands and computes the same way.  Asserted (tests/test_gpu_singular_values.py) against
 * numpy.linalg.svd in float64 on the same operand values: max_k |sv_k - ref_k| / ref_1 <= 9e-14 for 32x50, 64x50, 128x50,
 * 50x128, 64x64, 128x64, 1x7, 7x1, 5x5, rank 6, sigma graded over 12 decades, repeated sigma (measured 1.8e-14); the zero
 * matrix gives exact zeros; both memspaces give the same bits; sv(Y) = sv(Y^H) = sv(Y Q) for a permutation Q within that bound;
 * sv_1^2 agrees with jstsp_lambda_max_sequence_c32 on Y Y^H within that entry's 2e-5. */
int jstsp_singular_values_c32(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c32 *Y, double *sv, int memspace);
int jstsp_singular_values_c64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *Y, double *sv, int memspace);

/* plot_rankR.m:24-50 for trials [trial0, trial0 + batch) of sweep point sweep_idx: the first n_keep <= min(Nr, T_prop) singular
 * values of the noise-free Y = [H_1 .. H_L] Psi (Nr x T_prop; proposed_hbf.m:15-20 with N = zeros), sv[k + n_keep*t] in
 * memspace.  The channel H and the pilot symbols of trial t are exactly those jstsp_build_trials_c32 returns for trial t of
 * the same (model, seed, sweep_idx) (same Philox streams and kernels, csrc/inputgen.h); Y is formed in fp64 in LDS from those
 * fp32 operands; no noise and no Omega is drawn.  Fields read: Nt, Nr, L, T_prop, clusters, rays, shared_pilots, pilots.
 * Shapes as jstsp_singular_values_c32 on Nr x T_prop.  No _c64 form: no complex array crosses this boundary.
 * Asserted: max_k |sv_k - ref_k| / ref_1 <= 5e-14 (measured 9.7e-15) against the float64 SVD of Y rebuilt from
 * jstsp_build_trials_c32's H and pilot symbols, for the six panels of the figure at L = 1, 4, 8; a trial's values do not depend
 * on the batch it is computed in, nor on the memspace; the pilot options follow jstsp_build_trials_c32; over 256 trials per
 * point sv_{r+1} / sv_1, r = min(Np, L Nt, Nr, T), stays within 10 x the largest value of the float64 reference (H is fp32, so
 * the tail is of order 6e-8 sqrt(Nr Nt L), not zero). */
int jstsp_rank_trials_c32(jstsp_ctx *ctx, const jstsp_model *model, uint64_t seed, int sweep_idx, long long trial0, int batch,
                          int n_keep, double *sv, int memspace);

/* ---- singular values at every driver size, and the spectrum sweep on any channel (csrc/svdvals.hip) -------
 * jstsp_spectrum_c32 / _c64: sv[k + n_keep*t], k < n_keep <= min(rows, cols): the leading singular values of Y_t, descending,
 * as doubles in the memspace of Y; every other convention as jstsp_singular_values_*.  With m = max(rows, cols) and
 * n = min(rows, cols), three routes, none through a Gram matrix:
 *   - a shape jstsp_singular_values_* accepts: that kernel, and its bits;
 *   - n <= 64, m <= 65536: a float64 tall-skinny QR in front of the same Jacobi.  After a pass that finds the largest component, one workgroup
 *     per matrix walks the oriented operand once in chunks of 128 (n <= 48) or 64 rows and reduces each stack [R; chunk] to a new n x n
 *     triangle by Householder reflections in LDS; sv(R) = sv(Y), and R goes to the Jacobi kernel's own code.  The operand is
 *     scaled by a power of two on load (largest component into [1/2, 1)) and the values scaled back: both exact;
 *   - 64 < n <= 512, m <= 8192: the one-sided Jacobi of jstsp_pinv_f64 on the operand in global memory, without the inverse.
 *     Like that entry it waits for the context's stream once per sweep, and takes batch <= 65535.
 * JSTSP_E_UNSUPPORTED: n > 512, m > 65536, n > 64 with m > 8192, or a workspace (the staged copy of a JSTSP_HOST operand, the
 * float64 arrays of the third route) above 24 GiB - the message names the largest batch that fits.  A non-finite entry gives NaN
 * for its own matrix only; the zero matrix gives exact zeros; a repeated call returns the same bits (no atomics, every sum in a
 * fixed order); a matrix's values depend neither on the batch around it nor on the memspace; sv(Y 2^k) = sv(Y) 2^k on the bits.
 * Asserted (tests/test_gpu_spectrum.py) against numpy.linalg.svd in float64 on the same operand values, max_k |sv_k - ref_k| / ref_1:
 * <= 1.1e-13 on the QR route (measured 2.2e-14) and <= 3.6e-13 on the third (measured 7.2e-14), under the 1e-10 fixed beforehand
 * that no Gram route can meet, on random operands, rank 6, sigma graded over 12 decades and repeated sigma
 * (profiles/spectrum_measured_tolerances.json).  Unpivoted QR promises this ABSOLUTE bound only: a value far below sigma_1 is not relatively accurate. */
int jstsp_spectrum_c32(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c32 *Y, int n_keep, double *sv, int memspace);
int jstsp_spectrum_c64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *Y, int n_keep, double *sv, int memspace);

/* jstsp_rank_trials_c32 at any of those shapes of Nr x T_prop, on the drawn channel or on a supplied one.
 *   Hsrc == NULL: the drawn channel; on a shape jstsp_rank_trials_c32 accepts, that entry's bits (ld_rows, ld_cols, strideH,
 *   normalize and sigma_max are ignored).
 *   Hsrc != NULL: trial t's channel is cut from Hsrc and scaled; ld_rows, ld_cols, strideH, normalize and sigma_max mean what they
 *   mean in jstsp_build_trials_from_channel_c32 (one implementation, csrc/inputgen.h), error codes included: JSTSP_E_ILLCOND for a
 *   NaN or Inf in a used block, and then nothing is written.  clusters and rays are ignored.  The pilots come from the same Philox
 *   streams, so Y is the noise-free receive signal of the trial that entry builds for the same arguments.
 * On the QR route each entry of Y is formed once, in fp64 from the fp32 operands, as its chunk is loaded; on the third route Y is
 * written to the workspace first.  The call waits for its stream once when a channel is supplied.  Asserted: <= 5.5e-14 (measured
 * 1.1e-14) against the float64 SVD of Y rebuilt from the builder's H and pilot symbols at 64 x 160, 32 x 300 and 128 x 100, drawn
 * and supplied channels; a trial's values depend neither on the batch nor on the memspace; sigma_max has the builder's bits. */
int jstsp_spectrum_trials_c32(jstsp_ctx *ctx, const jstsp_model *model, uint64_t seed, int sweep_idx, long long trial0, int batch,
                              const jstsp_c32 *Hsrc, int ld_rows, int ld_cols, long long strideH, int normalize,
                              int n_keep, double *sv, double *sigma_max, int memspace);

/* ---- scoring a float64 estimate on the device (csrc/svdvals.hip) ------------------------------------------
 * jstsp_nmse_spectral_f64: nmse[t] = min(1, e_t), e_t = (sigma_1(S_t - Zbar_t) / sigma_1(Zbar_t))^2 (plot_errorVSsnr.m:138-141; the
 * quotient first, then the square).  jstsp_rate_f64: rate[t] = sum_k log2(1 + sigma_k(Zbar_t)^2 / (R (noise_var + e_t))) over all
 * min(R, C) values of Zbar_t, = log2 det(I + Zbar Zbar^H / (R (noise_var + e))) of plot_rateVSframelength.m:81, with e NOT capped
 * and R the row count of Zbar in either orientation.  S, Zbar: R x C x batch complex doubles, column-major; the result is
 * double[batch] in the memspace of the operands.  Unlike jstsp_nmse_spectral_c64 / jstsp_rate_c64, which narrow to the fp32
 * Gram/Lanczos kernels, nothing is narrowed and no Gram matrix is formed: the singular values come from the three routes of
 * jstsp_spectrum_c64, at its shapes (else JSTSP_E_UNSUPPORTED, and batch <= 65535 on the third route).  D = S - Zbar is formed in
 * float64 from the operands - as it is loaded on the first two routes, where the power-of-two scale is found from |D|'s own
 * largest component and D never reaches memory; into the workspace on the third - so an error 1e-9 of Zbar keeps its digits.
 *  - errors: JSTSP_E_NULL (ctx, S, Zbar, result), JSTSP_E_SHAPE (a non-positive size), JSTSP_E_ARG (bad memspace; noise_var < 0 or
 *    NaN); a workspace above 24 GiB is JSTSP_E_UNSUPPORTED and the message names the largest batch that fits.
 *  - a non-finite entry in S_t or Zbar_t gives NaN for trial t only; S == Zbar gives exactly 0.0 (and the rate of noise_var alone);
 *    S = 3 Zbar gives e = 4 exactly (NMSE 1.0); Zbar == 0 gives what the quotient gives: NaN for S == 0 (0/0), else e = Inf, NMSE 1.
 *  - no atomics, every sum in a fixed order: a trial's value depends neither on the batch around it, nor on the memspace, nor on a
 *    repeated call; the NMSE of (2^k S, 2^k Zbar) has the bits of that of (S, Zbar).
 * Asserted (tests/test_gpu_score64.py) against numpy.linalg.norm(., 2) and det in float64 on the same operand values, per trial
 * |x - ref| / |ref|: NMSE <= 3.0e-14 / 7.8e-14 / 7.5e-14 on the three routes (measured 5.9e-15 / 1.5e-14 / 1.5e-14), rate <= 5.3e-14 /
 * 9.3e-14 / 9.9e-14 (measured 1.0e-14 / 1.9e-14 / 2.0e-14; profiles/score64_measured_tolerances.json), all under the 1e-10 fixed
 * beforehand, including S = Zbar (1 + 1e-9 eps), where the NMSE is 2e-18 and jstsp_nmse_spectral_c64 returns 1e-16 .. 4e-16. */
int jstsp_nmse_spectral_f64(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c64 *S, const jstsp_c64 *Zbar,
                            double *nmse, int memspace);
int jstsp_rate_f64(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c64 *S, const jstsp_c64 *Zbar,
                   double noise_var, double *rate, int memspace);

/* ---- the reference's own element type at the boundary ------------------------------------------
 * Same functions, same argument meaning, arrays as MATLAB holds them: interleaved complex DOUBLE, and the 0/1 masks as
 * double (proposed_hbf.m:36-41 builds Omega with zeros()).  Inputs are narrowed and outputs widened on the device;
 * the arithmetic in between is the _c32 path's (results agree with the float64 reference to
 * fp32 accuracy, not beyond).  tau / rho / ce / index arrays are as in the _c32 form.  A JSTSP_HOST 'std' call
 * reports JSTSP_E_ILLCOND like its _c32 form. */
int jstsp_correlate_c64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                        const jstsp_c64 *K, const jstsp_c64 *A, long long strideA,
                        const jstsp_c64 *B, long long strideB, jstsp_c64 *out, int memspace);
int jstsp_synthesize_c64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                         const jstsp_c64 *S, const jstsp_c64 *A, long long strideA,
                         const jstsp_c64 *B, long long strideB, jstsp_c64 *out, int memspace);
/* proposed_algorithm.m:1 / proposed_algorithm_angles.m:1 */
int jstsp_proposed_algorithm_c64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                                 const jstsp_c64 *subY, const double *Omega,
                                 const jstsp_c64 *A, long long strideA,
                                 const jstsp_c64 *B, long long strideB,
                                 int Imax, const double *tau_Y, const double *tau_S,
                                 const double *rho, int type, const int32_t *indx_S,
                                 jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out, int memspace);
/* svt.m:1 */
int jstsp_svt_c64(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c64 *Y,
                  const double *tau, jstsp_c64 *X, int memspace);
/* OMP.m:1 */
int jstsp_omp_c64(jstsp_ctx *ctx, int measures, int size_d, int batch,
                  const jstsp_c64 *A, long long strideA, const jstsp_c64 *v, int m,
                  jstsp_c64 *x_hat, int32_t *index_out, jstsp_c64 *target_out, int memspace);
/* sparse_admm.m:1 */
int jstsp_sparse_admm_c64(jstsp_ctx *ctx, int Mr, int Mt, int Gr, int Gt, int batch,
                          const jstsp_c64 *Htrue, const jstsp_c64 *OH,
                          const jstsp_c64 *Dr, const jstsp_c64 *Dt, int Imax,
                          jstsp_c64 *S_out, double *ce_out, int memspace);
/* mc_svt.m:1, mc_admm.m:1 */
int jstsp_mc_svt_c64(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c64 *OH,
                     const double *Omega, int Imax, const double *tau, const double *rho,
                     jstsp_c64 *X_out, int memspace);
int jstsp_mc_admm_c64(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c64 *Htrue,
                      const jstsp_c64 *OH, const double *Omega, int Imax, const double *tau,
                      const double *rho, jstsp_c64 *X_out, double *ce_out, int memspace);
/* vamp.m:1.  Round 6: the two _c64 VAMP entries (this one and jstsp_vamp_kron_c64 below) COMPUTE in float64 on the device
 * (csrc/vamp64.hip: float64 storage, products, Jacobi eigen-decompositions of the factor Grams), unlike every other _c64 entry,
 * which narrows to the fp32 path.  Reason: at the reference's only operating point (nit = 100, sigma = 1, no stopping rule:
 * vamp.m:9,38,45, VampGlmEst.m:505-511) the iteration amplifies rounding differences ~1e9-fold, so that two float64 restatements
 * of the recurrences separate as well.  What tests/test_gpu_vamp64.py asserts against oracle/vamp.py: x within
 * 1e-9 at nit = 12; at nit = 50 and 100 inside the spread of the two float64 restatements (median and maximum over the trials of a
 * point); at nit = 100 the mean NMSE of a point within 0.01 (statistical parity, not per trial).  The _c32 entries keep the
 * fp32-storage path (per-iteration parity for ~12 iterations, statistical parity at 100).  Unlike the other
 * JSTSP_DEVICE calls these two synchronise the context's stream (the convergence test of the float64 Jacobi reads its
 * off-diagonal norm on the host once per sweep). */
int jstsp_vamp_c64(jstsp_ctx *ctx, int M, int N, int batch, const jstsp_c64 *y, const jstsp_c64 *A,
                   long long strideA, double sigma, double L, int nit, jstsp_c64 *x_out, int memspace);

/* plot_errorVSsnr.m:83 (pinv(A)*Y*pinv(B)), pinv, the joint OMP of :116-117, the drivers' vamp call :79-80,100, the NMSE
 * of :138-141 and the rate of plot_rateVSframelength.m:81 - arguments as in their _c32 forms */
int jstsp_ls_c64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *Y,
                 const jstsp_c64 *A, long long strideA, const jstsp_c64 *B, long long strideB,
                 jstsp_c64 *S_out, int memspace);
int jstsp_pinv_c64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A, jstsp_c64 *P, int memspace);
int jstsp_mmv_omp_c64(jstsp_ctx *ctx, int N, int Gr, int S, int batch, const jstsp_c64 *A, long long strideA,
                      const jstsp_c64 *Y, int K, int pnorm, jstsp_c64 *Z_out, int32_t *index_out,
                      int32_t *count_out, int memspace);
int jstsp_vamp_kron_c64(jstsp_ctx *ctx, int Na, int Gr, int G2, int batch, const jstsp_c64 *Y,
                        const jstsp_c64 *Af, long long strideA, const jstsp_c64 *Gb, long long strideG,
                        double sigma, double L, int nit, jstsp_c64 *X_out, int memspace);
int jstsp_nmse_spectral_c64(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c64 *S,
                            const jstsp_c64 *Zbar, double *nmse, int memspace);
/* CoSaMP (plot_time_comparisions.m:96) on doubles: like the two VAMP entries these do not narrow (see jstsp_cosamp_c32) */
int jstsp_cosamp_c64(jstsp_ctx *ctx, int measures, int size_d, int batch,
                     const jstsp_c64 *A, long long strideA, const jstsp_c64 *u, int K, int iters, double tol,
                     jstsp_c64 *x_hat, int32_t *support_out, int32_t *iters_out, double *resid_out,
                     int32_t *status_out, int memspace);
int jstsp_cosamp_kron_c64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                          const jstsp_c64 *Af, long long strideA, const jstsp_c64 *Bf, long long strideB,
                          const jstsp_c64 *y, int K, int iters, double tol,
                          jstsp_c64 *x_hat, int32_t *support_out, int32_t *iters_out, double *resid_out,
                          int32_t *status_out, int memspace);
int jstsp_rate_c64(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c64 *S, const jstsp_c64 *Zbar,
                   double noise_var, double *rate, int memspace);

/* ---- proposed_algorithm in float64 -----------------------------------------------------------------
 * proposed_algorithm.m:1-73 / proposed_algorithm_angles.m:1-85 ('approximate') evaluated in FLOAT64 on the device
 * (csrc/proposed64.hip, csrc/zgemm64.hip): storage, products, reductions, eigen-decompositions, thresholds and every scalar
 * (1/rho, rho/(rho+1), 1/(Omega+2 rho), tau/rho, alpha) are doubles; nothing is narrowed anywhere - unlike
 * jstsp_proposed_algorithm_c64, which takes the same arrays and narrows them to the fp32 solver.  This is the library's reference
 * path: what MATLAB would have returned to more than six digits, and the float64 side of a parity fixture at device speed
 * (tools/float64_reference.py).  Arguments, layouts, NULL-able outputs (Y_out, ce_out, indx_S), both memspaces and the error
 * conventions are those of jstsp_proposed_algorithm_c64 / jstsp_svt_c64 / jstsp_correlate_c64 / jstsp_synthesize_c64.
 *  - products: a batched complex float64 GEMM on v_mfma_f64_16x16x4_f64, four real accumulations per complex product (no
 *    3-multiplication form), split along k in a fixed order for the small Grams; no atomics - a repeated call returns the same
 *    bits and a trial's result does not depend on the batch around it.
 *  - svt: Y = U diag(max(0, 1 - tau/sigma)) U^H Z through the Hermitian eigen-decomposition of the Gram on the smaller side,
 *    n = min(N, M), sigma = sqrt(lambda).  Guard (that of the float64 host port the committed fixtures were solved with): a
 *    non-positive eigenvalue is a singular value at rounding level and is dropped; the output is all zeros exactly when NO
 *    eigenvalue is positive (the zero argument of iteration 1, svt.m:8-12).
 *  - n <= 64: two-sided cyclic Jacobi in LDS, convergence decided on the device (a sweep that rotates nothing, at most 30): no
 *    device-to-host read inside the iteration loop.  64 < n <= 512: the global-memory Jacobi of csrc/vamp64.hip, which reads one
 *    norm per sweep on the host - such a call synchronises the context's stream in every iteration.  That Jacobi sweeps ALL
 *    matrices of the call while any of them is above its stop criterion: for 64 < n a trial of jstsp_svt_f64 /
 *    jstsp_proposed_algorithm_f64 may get sweeps it would not get alone, so its last bits can depend on the batch around it
 *    (within the bounds asserted below; for n <= 64 they do not).  jstsp_mc_svt_f64 / jstsp_mc_admm_f64 ask the same Jacobi to
 *    leave a converged matrix alone and are batch-independent at every order.  n > 512: JSTSP_E_UNSUPPORTED.  Every call synchronises the stream once at entry (the per-trial scalars are staged from the caller's
 *    host arrays) and a JSTSP_HOST call at exit.
 *  - convergence_error(i, 1:2) from lambda_max of the n x n Grams of V1, V2, X (the same Jacobi); skipped when ce_out is NULL.
 *  - type: JSTSP_TYPE_APPROXIMATE only; JSTSP_TYPE_STD returns JSTSP_E_UNSUPPORTED (use jstsp_proposed_algorithm_c64).
 *    Alg. 1 ('std') in float64 is an entry of its own, jstsp_proposed_std_f64 below, which takes the least-squares factors.
 *  - workspace: about 72 MiB per trial at BASELINE configs[1] with per-trial B; above 24 GiB the call returns
 *    JSTSP_E_UNSUPPORTED with the largest batch that fits in the message (the Python wrappers chunk the batch).
 * Asserted (tests/test_gpu_f64_gemm.py, test_gpu_f64_proposed.py, test_gpu_f64_fullsize.py): the two kernel-level entries
 * entrywise within 8 (k1 + k2 + 8) 2^-53 (|A| |S| |B|) of numpy complex128; S and Y within 1e-10 of max|ref|, convergence_error
 * within 1e-8, NMSE within 1e-11 of oracle/solvers.py and the committed goldens; |dNMSE| <= 1e-9 per trial against the float64
 * host port at BASELINE configs[1] (measured values: DESIGN.md section 6). */
int jstsp_correlate_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                        const jstsp_c64 *K, const jstsp_c64 *A, long long strideA,
                        const jstsp_c64 *B, long long strideB, jstsp_c64 *out, int memspace);      /* A' K B' */
int jstsp_synthesize_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                         const jstsp_c64 *S, const jstsp_c64 *A, long long strideA,
                         const jstsp_c64 *B, long long strideB, jstsp_c64 *out, int memspace);     /* A S B */
int jstsp_proposed_algorithm_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                                 const jstsp_c64 *subY, const double *Omega,
                                 const jstsp_c64 *A, long long strideA,
                                 const jstsp_c64 *B, long long strideB,
                                 int Imax, const double *tau_Y, const double *tau_S,
                                 const double *rho, int type, const int32_t *indx_S,
                                 jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out, int memspace);
int jstsp_svt_f64(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c64 *Y,
                  const double *tau, jstsp_c64 *X, int memspace);

/* ---- pinv and the least-squares estimate in float64 ------------------------------------------------
 * MATLAB's SVD-based pinv (pinv.m) and S_ls = pinv(A)*Y*pinv(B) (plot_errorVSsnr.m:83) computed and returned in FLOAT64
 * (csrc/pinv64.hip), for factors of any driver size - unlike jstsp_pinv_c64 / jstsp_ls_c64, which store complex fp32 and
 * leave a factor that does not fit one workgroup's LDS to the fp32 Gram inverse (JSTSP_E_ILLCOND on the drivers' B_hbf).
 *  - route: one-sided (Hestenes) Jacobi on the columns of W = A (rows >= cols) or A^H in global memory, the rotations
 *    accumulated in V:  W V = U Sigma,  pinv(W) = V Sigma^-2 (W V)^H, assembled by the f64-MFMA GEMM.  No Gram matrix is formed:
 *    the error grows like cond * 2^-53, not like its square.
 *  - drop rule (pinv.m's default tolerance): sigma_k is kept iff sigma_k > max(rows, cols) * eps(sigma_max),
 *    eps(x) = 2^(floor(log2 x) - 52).
 *  - P: cols x rows x batch, column-major complex double.  rcond_out: NULL or double[batch], the smallest KEPT sigma over
 *    sigma_max (0 for the zero matrix); rank_out: NULL or int32[batch], the number of kept singular values.  Both live in
 *    the call's memspace, like A and P.  jstsp_ls_f64: arguments as jstsp_ls_c64 (a stride is 0 - the factor is shared and
 *    inverted ONCE for the call - or the size of one factor); rcond_out: NULL or double[2] in the call's memspace, the
 *    smallest rcond over the A factors and over the B factors of the call.
 *  - limits: min(rows, cols) <= 512 and max(rows, cols) <= 8192 per matrix / factor, batch <= 65535; otherwise, or when the
 *    float64 workspace would exceed 24 GiB, JSTSP_E_UNSUPPORTED (the message names the largest batch that fits).
 *  - an ill-conditioned or rank-deficient matrix is NOT an error: both entries return JSTSP_OK and the caller reads
 *    rcond_out / rank_out (there is no JSTSP_E_ILLCOND on this path, and jstsp_last_conditioning is not touched).  A NaN or
 *    Inf in a matrix gives NaN for that matrix's P, rcond NaN and rank 0, and leaves its batch mates alone.
 *  - every sum is formed in a fixed order and there are no atomics: a repeated call returns the same bits, and a matrix's
 *    result does not depend on the batch around it.
 *  - both memspaces.  Like jstsp_vamp_c64 these calls synchronise the context's stream, also with JSTSP_DEVICE: whether a
 *    matrix of the call is still rotating is read on the host once per sweep.
 * Asserted (tests/test_gpu_pinv64.py): ||P - P_exact||_2 / ||P_exact||_2 <= 8 max(d_numpy, cond 2^-53) for cond up to 1e10
 * on shapes from 7 x 13 to 512 x 4096, full rank and rank-deficient (measured values: DESIGN.md section 9d). */
int jstsp_pinv_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A,
                   jstsp_c64 *P, double *rcond_out, int32_t *rank_out, int memspace);
int jstsp_ls_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *Y,
                 const jstsp_c64 *A, long long strideA, const jstsp_c64 *B, long long strideB,
                 jstsp_c64 *S_out, double *rcond_out, int memspace);

/* ---- [U,S,V] = svd(A,'econ') and the best rank-R approximation in float64 (csrc/svd64.hip) -----------------
 * jstsp_svd_f64: the leading n_keep <= n = min(rows, cols) singular triplets of each matrix of A (rows x cols x batch,
 * column-major), A_t = U diag(sv) V^H when n_keep = n (plot_rankR.m:49, vamp.m:32).  One-sided (Hestenes) Jacobi in float64 on the
 * columns of A itself (of A^H when rows < cols) with the rotations accumulated - no Gram matrix.
 *  - outputs, all in the call's memspace and column-major: U rows x n_keep x batch, sv n_keep x batch descending (sv[k + n_keep*t]),
 *    V cols x n_keep x batch - V, not V^H, as MATLAB returns it.  U, V, rank_out (int32[batch]) and conv_out (int32[batch]) may
 *    each be NULL = not wanted; sv may not.  Equal singular values keep column order.
 *  - rank_out[t]: the number of singular values the drop rule of jstsp_pinv_f64 keeps, sigma_k > max(rows, cols) * eps(sigma_max)
 *    (one implementation).  The short-side factor - V when rows >= cols, else U - is the accumulated rotations and always a
 *    full set of orthonormal columns.  The long-side factor is column / norm and has ZERO columns for k >= rank: one-sided Jacobi
 *    leaves those columns at rounding level and does not orthogonalise them, so there is nothing to normalise.  sv still carries
 *    the computed values for those k.
 *  - conv_out[t]: 1 when a sweep rotated nothing, 0 when the sweep cap (30 on the first route, 40 on the second) ended the iteration
 *    - the value-only entries above stop silently at the cap; a caller who uses vectors needs to know.
 *  - two routes, chosen by the shape alone.  n <= 64 and (m + n) n complex doubles (m = max(rows, cols)) plus scratch within
 *    160 KiB of LDS - 64 x 64, 32 x 140, 128 x 50: one workgroup per matrix, ONE launch, no host read; the kernel of
 *    jstsp_singular_values_* with V carried under each column and the factors written in its epilogue; sv has that entry's bits on
 *    the shapes it takes.  Everything else up to 512 x 8192: the global-memory Jacobi of jstsp_pinv_f64, unchanged, and a kernel
 *    that sorts and writes the factors; like that entry it waits for the context's stream once per sweep (also with JSTSP_DEVICE) and
 *    takes batch <= 65535; sv has the bits of jstsp_spectrum_c64 for n > 64.
 *  - conventions of jstsp_spectrum_c64 and jstsp_pinv_f64: the operand is scaled by a power of two on load and the values scaled
 *    back, both exact, so svd(A 2^k) returns U, V on the bits and sv 2^k on the bits; a NaN or Inf entry gives NaN in U, sv, V,
 *    rank 0 and conv 0 for its own matrix only; the zero matrix gives sv = 0, rank 0, a zero long-side factor and the identity's
 *    leading columns in the short-side factor; no atomics, every sum in a fixed order: a repeated call returns the same bits, and
 *    a matrix's result depends neither on the batch around it nor on the memspace.
 *  - errors: JSTSP_E_SHAPE for a non-positive size; JSTSP_E_ARG for n_keep outside 1..n; JSTSP_E_NULL when A or sv is NULL;
 *    JSTSP_E_UNSUPPORTED for n > 512, max(rows, cols) > 8192, batch > 65535 on the second route, or a workspace above 24 GiB (the
 *    message names the largest batch that fits).
 *  - not done here: a long side above 8192 (jstsp_svd_tall_f64 below takes n <= 64 up to 65536 by a QR route that keeps its
 *    reflectors; U Sigma = A V would lose the orthogonality of the columns of small sigma); a _c32 form (the Python wrapper widens its input); jstsp_pinv_f64 and jstsp_svt_f64 keep their
 *    own kernels and bits; no environment switch selects a route.
 * jstsp_lowrank_f64: X_t = sum_{k < min(R, rank_t)} sigma_k u_k v_k^H, rows x cols x batch, the best rank-R approximation in the
 * spectral and Frobenius norms, formed as (U_R Sigma_R) V_R^H on the f64 matrix pipe from the factors of the same decomposition.
 * 1 <= R <= n (JSTSP_E_ARG otherwise).  tail_out: NULL or double[batch], sigma_{R+1} (0 when R >= n) = ||A - X||_2 (Eckart-Young).
 * Limits, non-finite handling (X and tail NaN for that matrix only) and batch independence as above.
 * Asserted (tests/test_gpu_svd64.py) with s1 = sigma_1 of numpy.linalg.svd, on 64x64, 32x140, 140x32, 128x50, 7x13, 13x7, 33x3, 5x5,
 * 1x7, 7x1 (first route) and 96x300, 200x97, 66x520, 520x66, 40x600 (second), random, rank 6, sigma graded over 12 decades and
 * repeated sigma: max_k |sv_k - ref_k| / s1 <= 9e-14 (first route) / 3.6e-13 (second); ||A - U diag(sv) V^H||_2 / s1,
 * max |Q^H Q - I| over the kept columns of the long-side factor and over all columns of the short-side factor each within 4 x the
 * worst value of a numpy restatement of the algorithm over the same problem set (tests/svd64_problems.py,
 * tests/test_svd64_problems.py; measured values: DESIGN.md section 9k, profiles/svd64_measured_tolerances.json); rank_out equal
 * to the drop rule on numpy's values; conv_out 1 throughout; the rank-6 projector within Wedin's bound; the low-rank residual
 * against tail_out and numpy; V diag(1/sv) U^H against jstsp_pinv_f64; isolation, memspace, repeat and power-of-two invariance on
 * the bits. */
int jstsp_svd_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A, int n_keep,
                  jstsp_c64 *U, double *sv, jstsp_c64 *V, int32_t *rank_out, int32_t *conv_out, int memspace);
int jstsp_lowrank_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A, int R,
                      jstsp_c64 *X, double *tail_out, int memspace);

/* ---- the same for a long side up to 65536: the QR route with the reflectors kept (csrc/svd64.hip) ---------------
 * jstsp_svd_tall_f64 / jstsp_lowrank_tall_f64: arguments, layouts, NULL-able outputs, both memspaces, the error codes and every
 * convention of jstsp_svd_f64 / jstsp_lowrank_f64 (V, not V^H; sv descending, equal values keep column order; the zero matrix; NaN
 * for the matrix with a non-finite entry only; no atomics, fixed summation order, a result independent of the batch and of the
 * memspace; svd(A 2^k) = U, V on the bits and sv 2^k on the bits), for n = min(rows, cols) <= 64 and m = max(rows, cols) <= 65536 in
 * either orientation (A^H is reduced when rows < cols and the factors swap on the way out).  JSTSP_E_UNSUPPORTED for anything
 * else, for a workspace above 24 GiB (the message names the largest batch that fits) and, jstsp_lowrank_tall_f64 only, for
 * batch > 65535.
 *  - ALWAYS the QR route, whatever the shape - small shapes are legal: (1) forward, one workgroup per matrix: the chunked Householder
 *    reduction [R; chunk] -> R of jstsp_spectrum_* (same chunk rule - 128 rows for n <= 48, else 64 -, same power-of-two prescale on
 *    load, the same code) with the reflectors kept: the tails stay where the operand's rows were, in a workspace of the operand's
 *    size, beside the head and the factor 1 / (|x| (|x| + |alpha|)) of every (chunk, column); then, in the same launch, the in-LDS
 *    Jacobi of jstsp_svd_f64's first route on the n x n triangle, R = U_R diag(sv) V^H.  (2) backward, one workgroup per matrix:
 *    the reflectors applied to [U_R(:, :n_keep); 0], last chunk first, one wave per output column; the rows below the top block
 *    are the long-side factor.  (3) what the back-application leaves in the top block E - zero in exact arithmetic, of size
 *    eps sigma_1 / sigma_k in column k in floating point - is exactly what the rows below lack, L^H L = I - E^H E; the long-side
 *    factor is multiplied by I + E^H E / 2, which makes it orthonormal to rounding level also for sigma_k < 1e-8 sigma_1.
 *    The correction couples the kept columns: the long-side columns of a call with a smaller n_keep agree with the leading ones of
 *    n_keep = n to rounding level, not on the bits (sv, the short-side factor, rank_out and conv_out do, on the bits).
 *    The short-side factor is V of the Jacobi, unchanged; sv its values scaled back.  Three launches (one when the long-side
 *    factor is not asked for), nothing read on the host: a JSTSP_DEVICE call does not wait for the stream.
 *  - rank_out and the zero columns of the long-side factor follow the drop rule with the long side of A:
 *    sigma_k > max(rows, cols) * eps(sigma_max).
 *  - sv has the bits of jstsp_spectrum_c64 wherever that entry reduces the same way (rows * cols > 8192): the same reduction and
 *    the same rotations.
 *  - workspace per matrix beside operand and outputs: 16 m n + 24 n ceil(m / chunk) + 16 (n n_keep + n_keep^2) bytes.
 * Asserted (tests/test_gpu_svd64_tall.py) against numpy.linalg.svd on 5x3, 3x5, 1x7, 7x1, 128x48, 130x48, 129x49, 64x64, 200x64,
 * 64x200, 8193x2, 2x8193, 9000x33 (random, rank 6, sigma graded over 12 decades, repeated sigma) and one 64x65536 matrix:
 * max_k |sv_k - ref_k| / s1 <= 1.1e-13; sv within 2.2e-13 s1 of jstsp_spectrum_c64; ||A - U diag(sv) V^H||_2 / s1 and
 * max |Q^H Q - I| of both factors each within 4 x the worst value of the numpy restatement of the route
 * (tests/svd64_tall_problems.py, tests/golden/svd64_tall_restatement_worst.json; measured values: DESIGN.md section 9k,
 * profiles/svd64_tall_measured_tolerances.json); rank_out equal to the drop rule on numpy's values; conv_out 1; the low-rank
 * residual against tail_out and numpy; U diag(sv) V^H against jstsp_svd_f64's; isolation, memspace, repeat and power-of-two
 * invariance on the bits. */
int jstsp_svd_tall_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A, int n_keep,
                       jstsp_c64 *U, double *sv, jstsp_c64 *V, int32_t *rank_out, int32_t *conv_out, int memspace);
int jstsp_lowrank_tall_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A, int R,
                           jstsp_c64 *X, double *tail_out, int memspace);

/* ---- proposed_algorithm 'std' (Alg. 1) in float64 -----------------------------------------------------
 * The 'std' branch of proposed_algorithm.m / proposed_algorithm_angles.m (:29, :53; angles :29, :64) evaluated in FLOAT64 on the
 * device (csrc/proposed64.hip): the iteration of jstsp_proposed_algorithm_f64 - same kernels, same svt guard, same doubles
 * everywhere - with the gradient step on V replaced by the least-squares solve v = U\(L\k), which for K2 = kron(B.', A) of full
 * column rank is V = pinv(A) K pinv(B): two f64-MFMA products per iteration.  G_A, G_B, the carried V, Res and RRes are not
 * allocated; convergence_error(:, 3) stays 0 (proposed_algorithm.m:6).  Arguments, layouts, NULL-able outputs (Y_out, ce_out,
 * indx_S) and both memspaces as jstsp_proposed_algorithm_f64, plus:
 *  - PA, PB: NULL, or pinv(A) (Gr x N) and pinv(B) (M x G2), column-major, in the call's memspace, shared exactly as A / B are
 *    (strideA == 0: one PA; otherwise one per trial, Gr N elements apart; likewise PB).  A NULL factor is computed by the
 *    call with the routine of jstsp_pinv_f64 (a shared factor is inverted once); a given one is used as it is, so a caller
 *    that solves several times on the same dictionaries (plot_errorVSsnr_approx.m: Imax 10 / 30 / 50) inverts them once.
 *    Passing the output of jstsp_pinv_f64 returns the bits of the NULL call.
 *  - rcond_out: NULL or double[2] in the call's memspace, as jstsp_ls_f64: the smallest rcond over the A factors and over the
 *    B factors the call computed; NaN for a side whose factor was given.
 *  - rank rule: N >= Gr and M >= G2, else JSTSP_E_UNSUPPORTED (the rule of jstsp_proposed_algorithm_c32 'std').  A computed
 *    factor of which jstsp_pinv_f64's drop rule keeps fewer singular values than it has columns (A) / rows (B), or that holds
 *    a NaN or Inf, returns JSTSP_E_ILLCOND before the first iteration; the message names the factor and the trial.
 *  - limits: min(N, M) <= 512, fewer than 2^31 entries per trial, batch <= 65535, and for a factor the call inverts those of
 *    jstsp_pinv_f64 (min(rows, cols) <= 512, max(rows, cols) <= 8192); otherwise, or above 24 GiB of workspace,
 *    JSTSP_E_UNSUPPORTED (the message names the largest batch that fits).
 *  - no atomics in any sum: a repeated call returns the same bits; for min(N, M) <= 64 a trial's bits do not depend on the
 *    batch around it (above, the note on the global Jacobi of jstsp_proposed_algorithm_f64 applies).  A call that computes a
 *    factor synchronises the context's stream (jstsp_pinv_f64).
 * Asserted (tests/test_gpu_std64.py): S and Y within 1e-10 of max|ref|, convergence_error within 1e-8 of oracle/solvers.py
 * proposed_algorithm(..., 'std') (measured values: DESIGN.md section 9h). */
int jstsp_proposed_std_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                           const jstsp_c64 *subY, const double *Omega,
                           const jstsp_c64 *A, long long strideA,
                           const jstsp_c64 *B, long long strideB,
                           const jstsp_c64 *PA, const jstsp_c64 *PB,
                           int Imax, const double *tau_Y, const double *tau_S, const double *rho,
                           const int32_t *indx_S,
                           jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out, double *rcond_out, int memspace);

/* ---- resuming and warm-starting the float64 ADMM (csrc/proposed64.hip) -------------------------------
 * The state of the iteration (proposed_algorithm.m:8-12, :27) as an argument: a solve can be split into legs, continued by a
 * caller who watches convergence_error, or started from the iterate of another problem (the previous frame of a slowly varying
 * channel).
 *  - layout: one trial's state is one contiguous block of jstsp_c64, column-major, [X | V1 | V2 | C] (N M each) then [v | S]
 *    (Gr G2 each); jstsp_admm_state_elems(N, M, Gr, G2) = 4 N M + 2 Gr G2 is its length and the stride between trials (0 for a
 *    shape that is not positive).  S is stored, not recomputed from v: in _angles the mask depends on the iteration index.
 *    The state lives in the call's memspace.
 *  - jstsp_proposed_resume_f64 / jstsp_proposed_std_resume_f64 take the arguments of jstsp_proposed_algorithm_f64 /
 *    jstsp_proposed_std_f64 and, in front of memspace, it0, state_in, state_out.  The call runs iterations it0 + 1 ... it0 + Imax
 *    of the reference loop from state_in and, when state_out is not NULL, writes the state after the last of them.
 *    state_in == NULL: from zero, and it0 must be 0 (JSTSP_E_ARG otherwise) - the bits of the sibling.  it0 < 0, or it0 + Imax
 *    beyond int: JSTSP_E_ARG.  Limits and error codes are otherwise those of the sibling.
 *  - ce_out: Imax x 3 x batch, the rows of the iterations THIS call ran.  Row 1, column 3 is |dv|^2 / |v_prev|^2 with the loaded
 *    v: finite when v != 0, Inf or NaN exactly as proposed_algorithm.m:51 makes it otherwise.  'std' keeps the column 0.
 *  - _angles: the mask of iteration it of the call has min(10 + 5 (it0 + it), Gr G2) entries (angles :36).
 *  - Xs = A S B is recomputed from the loaded S by the product the iteration uses.  'std' does not carry v (:53 recomputes it):
 *    the v of state_in is ignored there, the v of state_out is that of the last iteration.
 *  - state_out == state_in is allowed: the state is read whole before anything is written.  state_in is not modified otherwise.
 *  - a non-finite value in one trial's state stays in that trial.
 *  - The float64 solver carries nothing else between iterations: legs (a, b) return S, Y and the convergence_error rows of one
 *    call with Imax = a + b, bit for bit, for min(N, M) <= 64; above, the note on the global Jacobi of
 *    jstsp_proposed_algorithm_f64 applies to a leg as it does to a call (the same batch gives the same bits).
 *  - A JSTSP_HOST call stages the state with the other arrays: one staged solve.
 *  - jstsp_proposed_resume_c32: the same for the fp32 solver, jstsp_proposed_algorithm_c32's arguments plus it0, state_in, state_out
 *    (jstsp_c32, the same layout and stride).  What differs from the float64 entries:
 *      . the fp32 loop never stores C (after every iteration C == -V2): state_out holds C = -V2, and a state_in with C != -V2 - any
 *        state that is not an iterate of its own problem - is honoured in the first iteration through D = C + V2 (csrc/resume.hip).
 *      . not carried: the warm-started Jacobi basis of the svt and the Lanczos Ritz vectors (both start cold, as in a call from
 *        zero), the phase of the R v refresh (R v is recomputed from the loaded v in the call's first iteration), and the operand
 *        maxima (taken from the loaded data).  A split fp32 solve is therefore fp32-equivalent to the uninterrupted one, NOT
 *        bit-identical; state_in == NULL, it0 == 0 runs jstsp_proposed_algorithm_c32's code on one stream-ordered solve.
 *      . a trial whose k scale overflows in the fused pass is solved again from its state_in at it0 (jstsp_last_fused_fallbacks).
 *      . a JSTSP_HOST call is ONE staged solve: the two-halves host pipeline of jstsp_proposed_algorithm_c32 is not used.
 *    jstsp_proposed_resume_c64 is that entry at the reference's element type: every array, the state included, is narrowed to the
 *    fp32 solver and widened back as jstsp_proposed_algorithm_c64 does (the MEX command 'proposed_algorithm_resume' binds it).
 *    There is no _begin / _end pair for a resumed call.
 * Asserted (tests/test_gpu_resume64.py): splits of Imax = 6 against the siblings in bits, with and without indx_S; from an
 * arbitrary state S and Y within 1e-10 of max|ref| and convergence_error within 1e-8 of tests/resume_ref.py. */
size_t jstsp_admm_state_elems(int N, int M, int Gr, int G2);
int jstsp_proposed_resume_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                              const jstsp_c32 *subY, const float *Omega,
                              const jstsp_c32 *A, long long strideA,
                              const jstsp_c32 *B, long long strideB,
                              int Imax, const double *tau_Y, const double *tau_S,
                              const double *rho, int type, const int32_t *indx_S,
                              jstsp_c32 *S_out, jstsp_c32 *Y_out, double *ce_out,
                              int it0, const jstsp_c32 *state_in, jstsp_c32 *state_out, int memspace);
int jstsp_proposed_resume_c64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                              const jstsp_c64 *subY, const double *Omega,
                              const jstsp_c64 *A, long long strideA,
                              const jstsp_c64 *B, long long strideB,
                              int Imax, const double *tau_Y, const double *tau_S,
                              const double *rho, int type, const int32_t *indx_S,
                              jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out,
                              int it0, const jstsp_c64 *state_in, jstsp_c64 *state_out, int memspace);
int jstsp_proposed_resume_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                              const jstsp_c64 *subY, const double *Omega,
                              const jstsp_c64 *A, long long strideA,
                              const jstsp_c64 *B, long long strideB,
                              int Imax, const double *tau_Y, const double *tau_S,
                              const double *rho, int type, const int32_t *indx_S,
                              jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out,
                              int it0, const jstsp_c64 *state_in, jstsp_c64 *state_out, int memspace);
int jstsp_proposed_std_resume_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                                  const jstsp_c64 *subY, const double *Omega,
                                  const jstsp_c64 *A, long long strideA,
                                  const jstsp_c64 *B, long long strideB,
                                  const jstsp_c64 *PA, const jstsp_c64 *PB,
                                  int Imax, const double *tau_Y, const double *tau_S, const double *rho,
                                  const int32_t *indx_S,
                                  jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out, double *rcond_out,
                                  int it0, const jstsp_c64 *state_in, jstsp_c64 *state_out, int memspace);

/* ---- the float64 ADMM with its support refreshed from its own iterate (csrc/proposed64.hip) ------------
 * Alg. 2 ('approximate') only: the body of jstsp_proposed_resume_f64 with a support policy.  A "Proposed - PAI" whose indx_S is
 * the top of the solver's own v, taken inside the loop by the selection kernel of jstsp_support_top_f64: nothing comes back to the
 * host and no vendor sort runs.  With g = Gr*G2, R = min(g, JSTSP_SUPPORT_TOP_MAX), i = it0 + it the global 1-based iteration
 * and cnt(i) = min(10 + 5 i, g) (angles :36):
 *  - refresh iterations: i > refresh_start and (i - refresh_start - 1) % refresh_period == 0 for refresh_period >= 1; only
 *    i == refresh_start + 1 for refresh_period == 0.  A function of the global index, never of call boundaries.
 *  - at a refresh iteration the gradient step runs without a mask (v and convergence_error(:, 3) do not depend on the mask), the
 *    top R of the new v become the rank, and S = soft(v) .* [rank < cnt(i)] is rewritten from the stored v by the expression of
 *    the step: the bits a masked step would have written.
 *  - at every other iteration the step runs under the rank in force - that of the last refresh; before the first refresh of the
 *    call that of indx_S, or none when indx_S is NULL.  indx_S: n_indx entries per trial, 1-based, stride n_indx; entries outside
 *    1..g are ignored, entries that are not listed are never admitted.
 *  - LIMIT: a refreshed order lists R entries and entries outside it are never admitted: for g > 4096 the mask stops growing at
 *    4096 entries, from iteration 818 on (the reference runs 100).
 *  - indx_out (R x batch, 1-based; NULL: not wanted): the list of the call's last refresh, written if and only if the call ran a
 *    refresh - a function of it0, Imax, refresh_start and refresh_period.  A later leg passes it as indx_S with n_indx = R, the
 *    same start and period and its own it0: legs return the bits of the uninterrupted call (for min(N, M) <= 64; above, the note
 *    on the global Jacobi of jstsp_proposed_algorithm_f64 applies).
 *  - JSTSP_E_ARG: refresh_start < 0, refresh_period < 0, n_indx outside 1..g with indx_S, n_indx != 0 without it; it0 and the
 *    states as jstsp_proposed_resume_f64.  Limits, the workspace and its 24 GiB refusal are the family's; the rank array exists
 *    in every call.  The other entries keep their bits: the policy is off for them.
 * Asserted (tests/test_gpu_refresh64.py): with refresh_start >= it0 + Imax the bits of jstsp_proposed_resume_f64; for four
 * policies S, Y, convergence_error, the state and the order equal to the chain of one-iteration calls of the existing entries
 * with jstsp_support_order_f64 between them, bit for bit; legs that pass the order on; S and Y within 1e-10 of max|ref| and
 * convergence_error within 1e-8 of tests/refresh_ref.py; the refusals. */
int jstsp_proposed_refresh_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                               const jstsp_c64 *subY, const double *Omega,
                               const jstsp_c64 *A, long long strideA,
                               const jstsp_c64 *B, long long strideB,
                               int Imax, const double *tau_Y, const double *tau_S, const double *rho,
                               const int32_t *indx_S, int n_indx, int refresh_start, int refresh_period,
                               jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out,
                               int it0, const jstsp_c64 *state_in, jstsp_c64 *state_out,
                               int32_t *indx_out, int memspace);

/* ---- the float64 ADMM that stops each trial when its iterate has settled (csrc/proposed64.hip) ----------
 * Alg. 2 ('approximate') only: the body, the limits and the arguments of jstsp_proposed_refresh_f64 (refresh_period < 0: no
 * support policy, the body of jstsp_proposed_resume_f64; indx_S then has n_indx entries per trial, 0 meaning Gr*G2), with a
 * stopping rule on convergence_error(i, 3) = ||v_i - v_{i-1}||^2 / ||v_{i-1}||^2 (proposed_algorithm.m:51), the column the
 * gradient step already sums per trial in one workgroup.
 *  - THE RULE: trial t runs the global iterations it0 + 1, ...; it stops after the first iteration i with i - it0 >= min_iters and
 *    ce(i, 3) <= tol[t], failing that after it0 + Imax.  Memoryless - a function of i, it0 and the iterate - so a trial that came
 *    back unstopped is resumed by a later call and legs compose.  tol: batch doubles on the host, as tau_Y; a tol[t] that is zero,
 *    negative or NaN never stops its trial, nor does the Inf of iteration 1 from a zero state, nor a NaN.  min_iters >= 1.
 *  - iters_out[t] (required, int32): the iterations this call ran for trial t, 1 .. Imax.  ce3_out[t] (optional): ce(., 3) of its
 *    last iteration; the rule stopped the trial exactly when iters_out[t] >= min_iters && ce3_out[t] <= tol[t].
 *  - S_out, Y_out, state_out, indx_out hold what the loop held after the trial's LAST iteration; the rows of ce_out after it are
 *    NaN.  indx_out (R x batch) is written when the call can run a refresh within Imax; the row of a trial that stopped before
 *    its first refresh is all zeros (no 1-based list holds a zero): the order in force for it is still the caller's indx_S.
 *  - THE CONTRACT, for min(N, M) <= 64: for every trial S, Y, the state, the order and the rows of ce are the bits
 *    jstsp_proposed_refresh_f64 (without a policy jstsp_proposed_resume_f64) returns for that trial ALONE with Imax =
 *    iters_out[t] - whatever the batch around it, whatever `check`, in both memspaces.  Above order 64 the global Jacobi sweeps a
 *    call's matrices together (the note of jstsp_proposed_algorithm_f64): iters_out and the values to rounding, not the bits.
 *  - Mechanism: a stopped trial costs nothing further.  A test kernel sets a flag per slot after every iteration, a capture
 *    kernel writes what has JUST stopped to the trial's own place in the outputs (a trial is captured at the iteration where it
 *    stops, so `check` never changes a result), and every `check` >= 1 iterations an ordered count over the flags gives the
 *    survivors' new slots: the host reads one int (one stream synchronisation per `check` iterations), a gather kernel moves every
 *    per-trial array of the survivors to the front of a shadow set - never in place, never writing a caller's array - once at
 *    least a sixteenth of the slots have stopped (moving the survivors costs about a sixth of an iteration), and every later
 *    launch is sized to the count; the call returns when it is zero.  With no positive tol nothing is read back, no shadow
 *    set exists, and the call is the sibling on the bits with iters_out = Imax.
 *  - Workspace: the sibling's plus the shadow set (one more copy of X, V1, V2, C, A S B, v, S, subY, Omega, the rank, per-trial
 *    dictionaries and their Grams; two of the inputs in a JSTSP_DEVICE call), measured with the rest; the 24 GiB refusal applies.
 *  - JSTSP_E_NULL: tol or iters_out NULL; JSTSP_E_ARG: min_iters < 1, check < 1; everything the siblings refuse.
 * Asserted (tests/test_gpu_until64.py): iters against tests/until_ref.py, whose decisions all keep a margin of 1e-3 from their
 * threshold (tests/test_until_ref.py); per trial the bits of the sibling run alone over iters[t] iterations, for check 1, 3, 64,
 * both memspaces, B shared and per trial, indx_S and two policies; a batch of duplicates; warm starts, min_iters and legs; tol = 0;
 * a NaN trial; a batch that leaves the loop early; the refusals. */
int jstsp_proposed_until_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                             const jstsp_c64 *subY, const double *Omega,
                             const jstsp_c64 *A, long long strideA,
                             const jstsp_c64 *B, long long strideB,
                             int Imax, const double *tau_Y, const double *tau_S, const double *rho,
                             const int32_t *indx_S, int n_indx, int refresh_start, int refresh_period,
                             const double *tol, int min_iters, int check,
                             jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out,
                             int it0, const jstsp_c64 *state_in, jstsp_c64 *state_out, int32_t *indx_out,
                             int32_t *iters_out, double *ce3_out, int memspace);

/* ---- a float64 least-squares re-fit of an estimate on its support (csrc/refit64.hip) -------------------
 * A stage AFTER a solve, not a solver: the ADMM takes one steepest-descent step per iteration (proposed_algorithm.m:47-51), so its
 * S is not the least-squares fit on its own strong entries.  A few conjugate-gradient steps on the normal equations of
 * min ||Omega .* (A S B) - subY||_F, restricted to K entries of S, finish that.  Layouts, strides (0 = shared), memspaces and the
 * 24 GiB workspace refusal are those of jstsp_proposed_resume_f64; there is no eigen-decomposition, so min(N, M) is not limited.
 * Per trial, with g = Gr*G2:
 *  - support T: with indx_S (1-based, n_indx entries per trial, stride n_indx; K <= n_indx <= g) its first K entries, entries
 *    outside 1..g ignored; with indx_S == NULL (n_indx == 0) the first K entries of jstsp_support_order_f64(S_in), taken by the
 *    selection kernel of jstsp_support_top_f64 (ascending key, equal keys in ascending index; K <= JSTSP_SUPPORT_TOP_MAX).
 *    K == g: no mask, with or without indx_S.  m is the indicator of T.
 *  - G(x) = m .* (A^H ((Omega .* Omega) .* (A x B)) B^H) + lam x;  b = m .* (A^H (Omega .* subY) B^H).
 *  - x = m .* S_in; r = b - G(x); p = r; gamma_0 = gamma = <r, r>; for k = 1 .. iters: q = G(p); delta = Re<p, q>;
 *    alpha = gamma / delta; x += alpha p; r -= alpha q; gamma' = <r, r>; p = r + (gamma' / gamma) p; gamma = gamma'.
 *  - a trial FREEZES at the first k at whose start gamma == 0 or (tol > 0 and) gamma <= tol^2 gamma_0, or whose delta is not
 *    positive and finite (a NaN trial; lam = 0 and a direction in the null space).  Its x stays as it is.  The flag and the scalars
 *    live on the device: nothing is read back inside the loop, with or without tol.
 *  - S_out = x (S_out may be S_in).  iters_out (int32 per trial, NULL: not wanted): the steps taken, 0 .. iters.  resid_out
 *    ((iters + 1) x batch doubles, NULL: not wanted): gamma_0 .. gamma_iters, NaN after the trial's last step.
 *  - K and iters are regularisers (K = g with many steps fits the noise): both are the caller's, neither has a default here.
 *  - every sum runs in a fixed order inside one workgroup per trial and the products are those of jstsp_correlate_f64 /
 *    jstsp_synthesize_f64: a repeated call returns the same bits, and a trial's bits depend neither on its batch mates, nor on a
 *    shared or per-trial dictionary, nor on the memspace.  A NaN stays in its own trial.
 *  - Refused, outputs untouched: JSTSP_E_ARG - K < 1, K > g, K > JSTSP_SUPPORT_TOP_MAX without indx_S (unless K == g), n_indx
 *    outside K..g with indx_S or non-zero without it, iters < 1, lam or tol negative or NaN, a bad memspace; JSTSP_E_NULL - ctx,
 *    subY, Omega, A, B, S_in or S_out NULL; JSTSP_E_SHAPE - a non-positive size, a non-zero stride shorter than its factor;
 *    JSTSP_E_UNSUPPORTED - 2^31 or more entries in one trial's array, batch > 65535, a workspace above 24 GiB.
 * Asserted (tests/test_gpu_refit64.py) on the problems of tests/resume_problems.py, K in {4, 40, g}, iters in {1, 6}, lam in
 * {0, 0.1}, and one 64 x 256, 64 x 128 trial at K = 4096: S_out within 1e-10 of max|ref| and resid within 1e-8 of
 * tests/refit_ref.py (at K = 4 only, entries below 1e-10 gamma_0 against that floor), iters_out equal; the same bits from a repeated call, a
 * trial alone, the other memspace and indx_S = jstsp_support_order_f64(S_in); the objective does not increase; the zero problem,
 * a NaN trial, tol, every refusal. */
int jstsp_refit_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                    const jstsp_c64 *subY, const double *Omega,
                    const jstsp_c64 *A, long long strideA,
                    const jstsp_c64 *B, long long strideB,
                    const jstsp_c64 *S_in, const int32_t *indx_S, int n_indx, int K,
                    int iters, double lam, double tol,
                    jstsp_c64 *S_out, double *resid_out, int32_t *iters_out, int memspace);

/* ---- the fp32 ADMM with its support refreshed from its own iterate (csrc/proposed.hip) ------------------
 * jstsp_proposed_resume_c32 with the support policy of jstsp_proposed_refresh_f64 above: the same schedule on the global
 * iteration index, the same R = min(Gr*G2, JSTSP_SUPPORT_TOP_MAX) and its LIMIT, the same indx_S (n_indx entries per trial, stride
 * n_indx), the same indx_out (R x batch, written if and only if the call runs a refresh).  What is the fp32 solver's own:
 *  - type: JSTSP_TYPE_APPROXIMATE only; JSTSP_TYPE_STD is refused with JSTSP_E_UNSUPPORTED.
 *  - a refresh iteration, all on the context's main stream in front of the A S product: the gradient step without a mask, the
 *    selection kernel of jstsp_support_top_c32 on the new v (rank for every entry; the list when indx_out is wanted), and
 *    S = soft(v) .* [rank < cnt(i)] rewritten from the stored v by the step's own expression - the bits a masked step would have
 *    written.  v, Y and convergence_error of that iteration do not depend on the mask.  Beside a resident eigen-decomposition (the
 *    fused pass with convergence_error, Gr*G2 >= 8192) the selection runs as a 512-thread workgroup, as the step does; the lists
 *    do not depend on the workgroup's size.
 *  - the key is the fp32 |v|^2 of jstsp_support_order_c32: indx_out == jstsp_support_top_c32(v, R) of the state's v on the bits.
 *  - one staged solve in either memspace, state_out may be state_in, and a trial flagged by the fused pass is solved again from
 *    its state_in at it0 under the same policy, as in jstsp_proposed_resume_c32; the indx_out of such a trial comes from the
 *    re-solve.  As for every split fp32 solve, legs are fp32-equivalent to the uninterrupted call, not bit-identical.
 *  - JSTSP_E_ARG: refresh_start < 0, refresh_period < 0, n_indx outside 1..Gr*G2 with indx_S, n_indx != 0 without it, it0 < 0 or
 *    it0 != 0 without state_in.  Every message starts with "proposed_algorithm refresh: "; nothing is written on a refusal.
 *  - without a refresh in the call the launches, allocations apart from the rank array, and bits are those of
 *    jstsp_proposed_resume_c32.  No other entry passes a policy: their launches and bits are unchanged.
 * jstsp_proposed_refresh_c64 is the entry at the reference's element type, narrowed and widened as jstsp_proposed_resume_c64.
 * Asserted (tests/test_gpu_refresh32.py): on the window kernel, the general fused pass, JSTSP_FUSED=0 and an unfused shape - no
 * refresh: the bits of the resumed entries; one refresh at the call's last iteration: v and Y of the plain call, indx_out ==
 * jstsp_support_top_c32(v, R), S the plain S on the head and zero elsewhere, bit for bit; legs against the whole call and
 * tests/refresh_ref.py within the fp32 solver's tolerances; the re-solve; NaN isolation; memspaces; the refusals; the _c64 form. */
int jstsp_proposed_refresh_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                               const jstsp_c32 *subY, const float *Omega,
                               const jstsp_c32 *A, long long strideA,
                               const jstsp_c32 *B, long long strideB,
                               int Imax, const double *tau_Y, const double *tau_S, const double *rho, int type,
                               const int32_t *indx_S, int n_indx, int refresh_start, int refresh_period,
                               jstsp_c32 *S_out, jstsp_c32 *Y_out, double *ce_out,
                               int it0, const jstsp_c32 *state_in, jstsp_c32 *state_out,
                               int32_t *indx_out, int memspace);
int jstsp_proposed_refresh_c64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                               const jstsp_c64 *subY, const double *Omega,
                               const jstsp_c64 *A, long long strideA,
                               const jstsp_c64 *B, long long strideB,
                               int Imax, const double *tau_Y, const double *tau_S, const double *rho, int type,
                               const int32_t *indx_S, int n_indx, int refresh_start, int refresh_period,
                               jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out,
                               int it0, const jstsp_c64 *state_in, jstsp_c64 *state_out,
                               int32_t *indx_out, int memspace);

/* ---- the fp32 ADMM that stops each trial when its iterate has settled (csrc/proposed.hip, csrc/until.hip) ----
 * jstsp_proposed_refresh_c32 (refresh_period < 0: no support policy, the body of jstsp_proposed_resume_c32; indx_S then has n_indx
 * entries per trial, 0 meaning Gr*G2) with the stopping rule of jstsp_proposed_until_f64 above, word for word: THE RULE, tol
 * (batch doubles on the host; zero, negative or NaN never stops), min_iters, iters_out (required), ce3_out (optional) and what
 * S_out, Y_out, state_out, indx_out and the rows of ce_out hold are described there.  What is the fp32 solver's own:
 *  - type: JSTSP_TYPE_APPROXIMATE only; JSTSP_TYPE_STD is refused with JSTSP_E_UNSUPPORTED.
 *  - ce(i, 3) is the double the gradient step's kernel writes per trial in one workgroup, in a fixed order; nothing new is summed.
 *  - NO COMPACTION: a stopped trial runs on in its batch until every trial has stopped, and nothing it writes later is returned.
 *    So neither `check` nor the other trials' tol can change a trial's result - to the bit - and what the rule saves is the
 *    iterations after max(iters_out); the gap between mean and max is what a compaction would still buy.
 *  - Mechanism, all on the context's main stream: after the gradient step (and a refresh's rewrite of S) one thread per trial
 *    tests row i of ce(:, 3); the trials it has just stopped - all that still run, in the call's last iteration - are captured in
 *    two halves, S, v, the order, Y, X, V1 in front of the synthesis (the pass at the end of the iteration overwrites X and V1
 *    with those of i + 1) and V2, C behind it, into the caller's arrays (JSTSP_DEVICE) or their staging.  Under a live rule Y is
 *    stored by every iteration instead of the last one only.  Every `check` >= 1 iterations one kernel counts the running trials,
 *    the host reads that int with one synchronisation and leaves the loop at zero, after the main stream has waited for both side
 *    streams; then the rows of ce_out after iters_out[t] are set to NaN.  The default of the Python wrapper is check = 1,
 *    the fastest of 1, 2, 4, 8, 16 at BASELINE configs[1] (DESIGN.md section 9u has the measurement).
 *  - a trial flagged by the fused pass AT THE ITERATION WHERE IT STOPPED is solved again from its state_in under the same rule
 *    (a flag it raises later, running on, concerns iterations that are not returned).
 *  - with no positive tol nothing is read back, Y is stored as in the sibling, and the call is the sibling on the bits with
 *    iters_out = Imax.  No other entry passes a rule: their launches and bits are unchanged.
 *  - against the sibling run for one trial alone with Imax = iters_out[t]: fp32-equivalent (within the fp32 solver's tolerances),
 *    the order equal.  Measured per branch: the bits are equal on the three-kernel iteration and on a shape
 *    without a pass, not behind a fused pass, where the sibling's last iteration ends in the unfused synthesis and the stopped
 *    trial's in a pass.
 *  - JSTSP_E_NULL: tol or iters_out NULL; JSTSP_E_ARG: min_iters < 1, check < 1; everything the siblings refuse.
 * jstsp_proposed_until_c64 is the entry at the reference's element type, narrowed and widened as jstsp_proposed_refresh_c64.
 * Asserted (tests/test_gpu_until32.py): iters against tests/until_ref.py on the window kernel, the general pass, JSTSP_FUSED=0 and
 * an unfused shape, whose decisions keep a margin of 5e-2 (tests/test_until32_ref.py); values within the fp32 solver's tolerances
 * of the reference and of the sibling; check 1, 3, 64, other trials' tol and duplicates on the bytes; tol <= 0 or NaN: the
 * sibling's bytes; the early exit and the call after it; the re-solve; min_iters, warm starts, legs, a NaN trial; the refusals. */
int jstsp_proposed_until_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                             const jstsp_c32 *subY, const float *Omega,
                             const jstsp_c32 *A, long long strideA,
                             const jstsp_c32 *B, long long strideB,
                             int Imax, const double *tau_Y, const double *tau_S, const double *rho, int type,
                             const int32_t *indx_S, int n_indx, int refresh_start, int refresh_period,
                             const double *tol, int min_iters, int check,
                             jstsp_c32 *S_out, jstsp_c32 *Y_out, double *ce_out,
                             int it0, const jstsp_c32 *state_in, jstsp_c32 *state_out, int32_t *indx_out,
                             int32_t *iters_out, double *ce3_out, int memspace);
int jstsp_proposed_until_c64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                             const jstsp_c64 *subY, const double *Omega,
                             const jstsp_c64 *A, long long strideA,
                             const jstsp_c64 *B, long long strideB,
                             int Imax, const double *tau_Y, const double *tau_S, const double *rho, int type,
                             const int32_t *indx_S, int n_indx, int refresh_start, int refresh_period,
                             const double *tol, int min_iters, int check,
                             jstsp_c64 *S_out, jstsp_c64 *Y_out, double *ce_out,
                             int it0, const jstsp_c64 *state_in, jstsp_c64 *state_out, int32_t *indx_out,
                             int32_t *iters_out, double *ce3_out, int memspace);

/* ---- joint OMP and matrix completion in float64 -----------------------------------------------------
 * The "OMP with MMV" column (plot_errorVSsnr.m:116-117) and the TSSR / "SVT-based" recipe (:151-162) evaluated in FLOAT64 on the
 * device - unlike jstsp_mmv_omp_c64 / jstsp_mc_svt_c64 / jstsp_mc_admm_c64, which narrow the same arrays to the fp32 kernels.
 * jstsp_mmv_omp_f64 (csrc/mmv_omp64.hip): the algorithm, shapes, strideA, NULL-able index_out / count_out, both memspaces and the
 * Gr <= 4096 limit of jstsp_mmv_omp_c32; every stored value and every sum is a double (residual, basis, triangular factor,
 * coefficients, row scores, dot products, back-substitution, Z).  Contract (tests/test_gpu_mmv_omp64.py, against
 * oracle/solvers.py mmv_omp on the same values):
 *   Stop rules, in this order per atom, with the constants of the fp32 entry: (1) min(K, N, Gr) atoms are in; (2) the chosen atom
 *   is dependent on the support, ||a - Q Q' a||^2 <= 1e-10 ||a||^2 after two Gram-Schmidt passes, or a = 0 - not added;
 *   (3) ||R||_F^2 <= 1e-12 ||Y||_F^2 after an atom is added - it counts.  Y = 0 returns support [1], count 1, Z = 0.
 *   Selections: a selection whose float64 relative gap to the runner-up is >= 1e-9, or exactly 0, is the oracle's; Z is then within
 *   1e-12 of the oracle's relative to max|Z| when cond(A(:,support)) <= 100.
 *   Ties: the lowest index wins.  A correlation is carried in four real fma chains joined at the end and |c|^2 is a sum of two
 *   rounded squares, so columns equal to column j, to -column j or to +-1i column j score bit-equal.
 *   Scale: each problem is solved on Y * 2^-e, e the exponent of its largest finite component (frexp / ldexp, exact unless a
 *   component more than 2^1021 times smaller underflows), ||Y||_F^2 is summed on the scaled values: supports and counts do not
 *   depend on the scale of Y, and Z of Y * 2^k is Z of Y times 2^k bit for bit (tested: k = +-100, +-400).
 *   A NaN or Inf in a problem's Y ends that problem with a count in [0, K] and status 0; its batch mates are not affected.
 *   No atomics, every sum in a fixed order: a repeated call returns the same bits, and a problem's result does not depend on the
 *   batch around it or on the memspace.
 * jstsp_mc_svt_f64 / jstsp_mc_admm_f64 (csrc/mc64.hip): mc_svt.m:1-12 and mc_admm.m:1-34 with the dense solve written as
 * b ./ (Omega + rho).  Arguments as the _c64 entries, Omega a double array; tau, rho: host double[batch]; ce_out: NULL (Htrue may
 * then be NULL too) or Imax x batch double, sigma_max(X - Htrue)^2 / sigma_max(Htrue)^2, not capped.  The svt is the one of
 * jstsp_svt_f64 (csrc/svt64.h), with its guard - non-positive eigenvalues dropped, all zeros exactly when none is positive - and
 * its limits: min(Mr, Mt) <= 512, batch <= 65535, a workspace above 24 GiB is JSTSP_E_UNSUPPORTED.  The eigen-decomposition runs
 * to convergence in every iteration (no warm start, no early stop, no environment switch).  Imax = 0 returns zeros.  Both calls
 * synchronise the context's stream at entry (the scalars are staged) and at exit, in both memspaces; for 64 < min(Mr, Mt) also
 * once per Jacobi sweep.  Deterministic, and a trial's bits do not depend on the batch around it, also for 64 < min(Mr, Mt): the
 * global-memory Jacobi is told to leave a matrix alone from the sweep on at whose start it meets the stop criterion itself
 * (jstsp_svt_f64 and jstsp_proposed_algorithm_f64 keep the behaviour they had: see their block above).
 * Asserted (tests/test_gpu_mc64.py, test_gpu_tssr64.py): X within 1e-10 of max|X_ref| and convergence_error within 1e-8 of
 * oracle/solvers.py mc_svt / mc_admm; the TSSR chain within 1e-10 (Y_svt) and 1e-9 (S_tssr, S_svt) of oracle/solvers.py tssr
 * (measured on MI355X: Z 3.7e-15, mc_svt X 1.1e-14, mc_admm X 1.6e-13 and ce 7.2e-13, the TSSR chain 1.2e-14; DESIGN.md section 9e,
 * profiles/tssr64_measured_tolerances.json). */
int jstsp_mmv_omp_f64(jstsp_ctx *ctx, int N, int Gr, int S, int batch, const jstsp_c64 *A, long long strideA,
                      const jstsp_c64 *Y, int K, int pnorm, jstsp_c64 *Z_out, int32_t *index_out,
                      int32_t *count_out, int memspace);
int jstsp_mc_svt_f64(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c64 *OH, const double *Omega,
                     int Imax, const double *tau, const double *rho, jstsp_c64 *X_out, int memspace);
int jstsp_mc_admm_f64(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c64 *Htrue, const jstsp_c64 *OH,
                      const double *Omega, int Imax, const double *tau, const double *rho,
                      jstsp_c64 *X_out, double *ce_out, int memspace);

/* ---- OMP (dense and Kronecker) and sparse_admm in float64 -------------------------------------------
 * OMP.m:1-32 and sparse_admm.m:1-36 evaluated in FLOAT64 on the device - unlike jstsp_omp_c64 / jstsp_sparse_admm_c64, which narrow
 * the same arrays to the fp32 kernels.  Arguments, layouts, NULL-able outputs (target_out; ce_out, with which Htrue may be NULL), both
 * memspaces and the error codes are those of jstsp_omp_c64 / jstsp_omp_kron_c32 / jstsp_sparse_admm_c64; every stored value and every
 * sum is a double.  No atomics and every sum in a fixed order: a repeated call returns the same bits, and a problem's result does not
 * depend on its batch mates, on whether a dictionary is shared (stride 0) or on the memspace.  The device reference for the fp32
 * selection contract of jstsp_omp_c32, and the float64 OMP column of tools/run_time_comparison.py --omp-f64.
 * jstsp_omp_f64 / jstsp_omp_kron_f64 (csrc/omp64.hip): exactly m iterations, chosen atoms are not excluded, x = pinv(targetMatrix) v.
 *   Measurement space: an orthonormal basis of the distinct selected atoms (two passes of classical Gram-Schmidt per atom), the
 *   triangular factor, one back-substitution at the end; launches per iteration for the whole batch, nothing read back on the host.
 *   Correlation: dense - one wave per atom, four real fma chains joined at the end; Kronecker - Af^H R Bf^H by two f64-MFMA products
 *   (what jstsp_correlate_f64 computes), Phi is never formed.
 *   Selection: the score is |c|^2 as a sum of two rounded squares; the first index among equal scores, a NaN never wins.  Columns
 *   equal to column j, to -column j or to +-1i column j score bit-equal (dense), and so do the atoms built on equal or negated rows
 *   of Bf (Kronecker).  A selection whose float64 relative gap to the runner-up is >= 1e-9, or exactly 0, is the one of
 *   oracle/solvers.py omp_literal on the same values; x_hat is then within 1e-12 of it relative to max|x_hat|.
 *   Re-selection: an index already in the index set leaves span and residual unchanged; its coefficient is split equally over its
 *   copies and x_hat keeps the last one (OMP.m:29-32), as jstsp_omp_c32 does.  A new index whose atom lies in the span of the chosen
 *   ones (||a - Q Q' a||^2 <= 1e-20 ||a||^2, or a = 0) adds nothing and keeps the coefficient 0.  v = 0 gives all ones, x_hat = 0.
 *   target_out: the selected columns, bit-equal to A's.
 *   Scale: each problem is solved on v * 2^-e, e the exponent of the largest finite component of v (frexp / ldexp), and x_hat is
 *   scaled back by 2^e: index sets do not depend on the scale of v, and x_hat of v * 2^k is x_hat * 2^k bit for bit (tested: k =
 *   +-70, +-100, +-400).  A NaN or Inf in a problem's v ends that problem with status 0 and arbitrary indices in [1, size_d]; its
 *   batch mates are not affected.
 *   Limits (JSTSP_E_UNSUPPORTED): m <= 1024; measures (N M) <= 65536; size_d (Gr G2) <= 1048576; batch <= 65535; a float64
 *   workspace (about 16 measures m bytes per problem) above 24 GiB - the message names the largest batch that fits.  As in the fp32
 *   entries m is not limited by measures or size_d.  JSTSP_DEVICE calls are asynchronous on the context's stream.
 * jstsp_sparse_admm_f64 (csrc/sparse_admm64.hip): the structured form of jstsp_sparse_admm_c32 - factor Grams by the f64-MFMA GEMM,
 *   their eigen-decompositions once per call by the float64 Jacobi (in LDS up to order 64, in global memory above), A'OH once, per
 *   iteration one element-wise kernel (V = R + Z/rho, soft threshold, RHS), four products around the divide by lr lt^T - rho, and
 *   Z += rho (R - S).  rho = 0.01 and tau_s = 1e-4 in double.  ce_out: Imax x batch, sigma_max(Dr S Dt^H - Htrue)^2 /
 *   sigma_max(Htrue)^2, not capped.  Gr == Mr and Gt == Mt (JSTSP_E_SHAPE otherwise); max(Mr, Mt) <= 512 and batch <= 65535, else
 *   JSTSP_E_UNSUPPORTED; Imax = 0 returns zeros.  A denominator lr lt - rho that is exactly 0 gives what IEEE gives (the reference's
 *   singular B \), not an error.  A non-finite eigenvalue of a factor Gram - a NaN or Inf in Dr / Dt - returns JSTSP_E_ILLCOND before
 *   the first iteration.  The call synchronises the context's stream (the eigenvalues are checked on the host; with ce_out and
 *   64 < min(Mr, Mt) also once per Jacobi sweep), in both memspaces.
 * Asserted (tests/test_gpu_omp64.py, test_gpu_sparse_admm64.py): every index set equal to the oracle's on the engineered rows of
 * tests/omp_problems.py and tests/omp64_problems.py, x_hat within 1e-12 of max|x_ref|; S within 1e-10 of max|S_ref| and
 * convergence_error within 1e-8 of oracle/solvers.py sparse_admm (measured values: DESIGN.md section 9f,
 * profiles/omp64_measured_tolerances.json). */
int jstsp_omp_f64(jstsp_ctx *ctx, int measures, int size_d, int batch,
                  const jstsp_c64 *A, long long strideA, const jstsp_c64 *v, int m,
                  jstsp_c64 *x_hat, int32_t *index_out, jstsp_c64 *target_out, int memspace);
int jstsp_omp_kron_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch,
                       const jstsp_c64 *Af, long long strideA, const jstsp_c64 *Bf, long long strideB,
                       const jstsp_c64 *y, int m, jstsp_c64 *x_hat, int32_t *index_out, int memspace);
int jstsp_sparse_admm_f64(jstsp_ctx *ctx, int Mr, int Mt, int Gr, int Gt, int batch,
                          const jstsp_c64 *Htrue, const jstsp_c64 *OH, const jstsp_c64 *Dr,
                          const jstsp_c64 *Dt, int Imax, jstsp_c64 *S_out, double *ce_out, int memspace);

/* Per-kernel timing of the last proposed_algorithm call made with profiling enabled:
 * jstsp_set_profiling(ctx, 1) brackets every launch of the dominant kernel with HIP
 * events on the context's stream; jstsp_get_profile() returns launches and total ms. */
int jstsp_set_profiling(jstsp_ctx *ctx, int enable);
int jstsp_get_profile(jstsp_ctx *ctx, const char *kernel, int *launches, double *total_ms);

#ifdef __cplusplus
}
#endif
#endif /* JSTSP_H */
