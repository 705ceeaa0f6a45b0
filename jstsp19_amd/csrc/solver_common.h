// Host-side helpers shared by the solver drivers: GEMM call shorthands, batched SVT,
// spectral norms, host<->device staging.
#pragma once
#include "common.h"
#include <climits>
#include <vector>

namespace jstsp {

// Column-major matrix view of a batched operand: element (r, c) of problem t at
// p[t*st + r + ld*c]; st == 0 => one matrix shared by the whole batch.
struct Mat {
    const float2 *p; long long st; int ld;
};

// C = alpha * op(A) * op(B) + beta * D, all column-major; opX in {'N','C'} ('C' = conj. transpose)
int gemm(jstsp_ctx *ctx, char opA, char opB, int m, int n, int k, int batch, Mat A, Mat B, float2 *C,
         long long sCt, int ldc, float alpha = 1.f, const float2 *D = nullptr, long long sDt = 0,
         int ldd = 0, float beta = 0.f, int tag = GEMM_MISC, int splitk = 1, long long sCsplit = 0);

// Gram of a dictionary factor with float64 products and sums (gram64.hip): side 'L' G = X^H X (cols x cols), 'R' G = X X^H
// (rows x rows); X rows x cols column-major (ld = rows), sXt = 0: shared; G order n, ld = n, exactly Hermitian; Glo (optional,
// same layout): the part of the float64 sum that the fp32 G does not hold
int gram_f64(jstsp_ctx *ctx, char side, const float2 *X, long long sXt, int rows, int cols, int count, float2 *G, long long sGt,
             float2 *Glo = nullptr);

// The 64-term products of the gradient step on the f16 matrix pipe (hsmall.hip), N = Gr = 64:
//   Tc = sum of `parts` partial sums (P[t sPt + p sPp + n + 64 g]) [+ leading-column terms of a block-Toeplitz dictionary: Kf, Bdl],
//   Res = A^H Tc - RV (RV may be NULL), P1 = G_A Res, pmax[t] = max|P1| (atomicMax; may be NULL); Tc stored if non-NULL
bool grad_head_shape_ok(int N, int Gr, int G2);
int launch_grad_head(jstsp_ctx *ctx, int G2, int batch, const float2 *P, long long sPt, long long sPp, int parts, const float2 *Kf,
                     const float2 *Bdl, long long sBdl, const float2 *A, long long sA, const float2 *GA, long long sGA,
                     const float2 *RV, float2 *Tc, float2 *Res, float2 *P1, uint32_t *pmax);

// Descriptor only (the caller may attach a fused epilogue before launch_cgemm).
GemmDesc make_gemm(char opA, char opB, int m, int n, int k, int batch, Mat A, Mat B, float2 *C, long long sCt,
                   int ldc, float alpha = 1.f, const float2 *D = nullptr, long long sDt = 0, int ldd = 0,
                   float beta = 0.f, int splitk = 1, long long sCsplit = 0);

// Workspace of the Gram-form SVT / spectral norm of rows x cols matrices.
struct GramWS {
    int rows = 0, cols = 0, n = 0, nsplit = 1, batch = 0;
    bool left = true;          // true: G = Z Z^H (rows <= cols); false: G = Z^H Z
    float2 *Gpart = nullptr;   // batch * nsplit * n*n
    float2 *Q = nullptr;       // batch * n*n
    float2 *Vg = nullptr;      // eigenvectors in HBM when they do not fit in LDS
    float2 *Uwarm = nullptr;   // eigenvector basis of the previous call (warm start): NE x NE padded for n <= 64, n x n above
    float2 *Twarm = nullptr;   // n > 64: temporary of the warm-start transform G <- Uw^H (G Uw)
    mutable int warm = 0;      // 1 once Uwarm holds a basis
    // Orders 65..128, warm-started sequences only: no (further) Jacobi sweep is run once the Gram in the previous basis has all
    // relative off-diagonals |g_pq| / sqrt(g_pp g_qq) below this level (0: the end-of-sweep rule alone, which confirms convergence
    // with a sweep that starts below 1e-4).  An inexact inner solve for the fixed-point loops that can take it (mc_svt, mc_admm).
    float eig_stop = 0.f;
    mutable LanczosWarm lz;    // norm workspaces (need_q == false, n <= 128): warm-start record of the Lanczos lambda_max kernel
    static size_t bytes(int rows, int cols, int batch, bool need_q, int force_nsplit = 0);
    int alloc(Arena &a, int rows, int cols, int batch, bool need_q, int force_nsplit = 0);
};

// G partials of Z (split-K over the long dimension).
int gram_partials(jstsp_ctx *ctx, const GramWS &w, const float2 *Z, long long sZt);
// Y = svt(Z, tau_t): tau from prm[t].tauY_rho, or tau[t] when tau != nullptr.  Y may alias nothing.
// `sequence` = true: successive calls see slowly varying inputs (an ADMM loop), so the
// eigenvector basis of the previous call warm-starts the Jacobi sweeps.
int svt_batched(jstsp_ctx *ctx, const GramWS &w, const float2 *Z, const TrialParams *prm,
                const float *tau, float2 *Y, bool sequence = false);
// The two halves of svt_batched: Gram + eigen-decomposition -> projector Q; then Y = Z - Q Z.
// amax != nullptr (per-problem bound on max(|re|,|im|) of Z): Gram on the split-f16 path when rows <= 64
int svt_prepare(jstsp_ctx *ctx, const GramWS &w, const float2 *Z, const TrialParams *prm, const float *tau,
                bool sequence, const uint32_t *amax = nullptr, const float2 *Z2 = nullptr,
                bool gram_done = false);   // gram_done: the partials of G are already in the workspace
                // Z2 (split-f16 Gram path only): the svt argument is Z - prm[t].irho * Z2, never stored
int svt_apply(jstsp_ctx *ctx, const GramWS &w, const float2 *Z, float2 *Y);

// resume.hip: the state block of a resumed proposed_algorithm call to and from the solver's arrays, and K -= D of its first iteration
int launch_resume_unpack(jstsp_ctx *ctx, long long nm, long long g, int batch, const float2 *state, float2 *X, float2 *V1, float2 *V2, float2 *Cb,
                         float2 *V, float2 *S, const float2 *subY, float2 *subY1, const TrialParams *prm, bool explicit_c);
int launch_resume_fix_k(jstsp_ctx *ctx, long long n, float2 *K, const float2 *D);
int launch_resume_pack(jstsp_ctx *ctx, long long nm, long long g, int batch, const float2 *X, const float2 *V1, const float2 *V2, const float2 *Cb,
                       const float2 *V, const float2 *S, float2 *state);

// until.hip: the stopping rule of jstsp_proposed_until_c32 (proposed.hip says where each runs).  flag[t]: 0 running, 1 stopped by
// this iteration (the captures' cue), 2 stopped earlier.
struct UntilWS {
    int32_t *flag = nullptr, *iters = nullptr, *left = nullptr;     // per trial, per trial, the one int the host reads
    double *ce3 = nullptr, *tol = nullptr;
    uint32_t *ovf = nullptr;                        // the pass's overflow flag of a trial as it stood when the trial stopped
    float2 *S = nullptr, *Y = nullptr;              // where a stopped trial's S and Y go: the caller's arrays, or their staging
    int32_t *top = nullptr;                         // ... and its order; the state goes to ProposedWS::sout
    int32_t *top_loop = nullptr;                    // the list the loop's refreshes write (a stopped trial runs on and rewrites its row)
};
int launch_until_init(jstsp_ctx *ctx, int batch, const UntilWS &u);
// after iteration k (1-based) of the call, row `it` of ce (batch x 3 x Imax): stops the running trials the rule says, all when `last`
int launch_until_test(jstsp_ctx *ctx, int batch, int k, int min_iters, bool last, const double *ce, int Imax, int it, const uint32_t *ovf_now,
                      const UntilWS &u);
// the trials with flag 1: S, Y, [X | V1 | . | . | v | S] of the state, the order (zeros when no refresh has run: have_top false)
int launch_until_capture_head(jstsp_ctx *ctx, long long nm, long long g, int R, int batch, const float2 *X, const float2 *V1, const float2 *Y,
                              const float2 *V, const float2 *S, bool have_top, const UntilWS &u, float2 *state);
// ... and behind the synthesis [. | . | V2 | C | . | .] of the state; Cb as launch_resume_pack's
int launch_until_capture_tail(jstsp_ctx *ctx, long long nm, long long g, int batch, const float2 *V2, const float2 *Cb, const UntilWS &u, float2 *state);
int launch_until_count(jstsp_ctx *ctx, int batch, const UntilWS &u);        // *left = trials still running
int launch_until_mask_ce(jstsp_ctx *ctx, int batch, int Imax, const UntilWS &u, double *ce);   // rows after iters[t]: NaN

// Gram partials of problems [t0, t0 + count) only (same workspace layout as gram_partials).
int gram_partials_range(jstsp_ctx *ctx, const GramWS &w, const float2 *Z, long long sZt, int t0, int count,
                        const uint32_t *amax = nullptr, const float2 *Z2 = nullptr,
                        const TrialParams *zprm = nullptr, bool norm_only = false);
// lam[t] = lambda_max of the Gram partials already in the workspace, all w.batch problems
// The warm-start record of a norm workspace: all vectors invalid, the context's mismatch counter zeroed (on ctx->stream;
// once per solve, before the first lambda_max of its loop).  `call` of the record is set by the loop's owner.
int lanczos_warm_reset(jstsp_ctx *ctx, const GramWS &w);
int lmax_from_partials(jstsp_ctx *ctx, const GramWS &w, float *lam, bool lanczos = false);
int lmax_from_partials_range(jstsp_ctx *ctx, const GramWS &w, int first, int count, float *lam, bool lanczos);   // matrices [first, first + count)
// Make sure the context's side streams / events exist.
int ensure_side_streams(jstsp_ctx *ctx);
int ensure_bj_resources(jstsp_ctx *ctx);    // ctx->bj_stream / bj_ev (common.h)
bool ensure_cu_streams(jstsp_ctx *ctx);     // false: no masked streams on this runtime (callers use the side streams)
// Temporarily route the launch helpers (which use ctx->stream) to another stream.
struct StreamScope {
    jstsp_ctx *c; hipStream_t saved;
    StreamScope(jstsp_ctx *ctx, hipStream_t s) : c(ctx), saved(ctx->stream) { c->stream = s; }
    ~StreamScope() { c->stream = saved; }
};
// lam[t] = sigma_max(Z_t)^2   (lanczos: the per-iteration convergence-error curves; Householder + Sturm otherwise)
int sigma_max_sq(jstsp_ctx *ctx, const GramWS &w, const float2 *Z, float *lam, bool lanczos = false);

// Ginv[t] = G[t]^-1 for `count` Hermitian PD n x n matrices (hinv.hip).  Its temporaries are taken first (take) and used
// afterwards (the call with a HinvWS); the call without one takes them from ctx->arena itself.  A caller may rewind the arena to
// where it stood before take() once the inverse has been enqueued.
struct HinvWS {
    float2 *T1 = nullptr, *T2 = nullptr, *Vg = nullptr;
    float *lam = nullptr;
    void take(Arena &a, int n, int count);
};
size_t hinv_bytes(int n, int count);        // what take() takes
int hermitian_inverse(jstsp_ctx *ctx, int n, int count, const float2 *G, float2 *Ginv, const HinvWS &w);
int hermitian_inverse(jstsp_ctx *ctx, int n, int count, const float2 *G, float2 *Ginv);

// pinv of small matrices in float64 (pinv.hip): P[t] (cols x rows) = pinv(A[t]) (rows x cols) when the matrix fits in LDS
bool pinv_fits(int rows, int cols);
int launch_pinv(jstsp_ctx *ctx, int rows, int cols, int count, const float2 *A, long long sAt, int lda, float2 *P,
                long long sPt, int ldp, float *rcond_out = nullptr);
// The context's conditioning record (common.h: jstsp_ctx::diag): allocate on first use / reset at the start of a call.
int ensure_diag(jstsp_ctx *ctx);
int diag_reset(jstsp_ctx *ctx);
// After the stream has been synchronised: JSTSP_E_ILLCOND when a Gram inverse of the call lost all its fp32 digits.
int diag_check_host(jstsp_ctx *ctx, const char *what);

// A proposed_algorithm solve whose device work has been enqueued but whose results are still in the context's workspace
// (proposed.hip): the halves of a pipelined JSTSP_HOST call.  Valid until the next solve on that context.
struct PendingSolve {
    bool want_ce = false;               // convergence_error was asked for and has rows (Imax > 0)
    const float2 *dS = nullptr, *dY = nullptr;
    const double *dce = nullptr;
    const uint32_t *ovf = nullptr;      // the per-trial overflow flags (NULL: the solve did not use the fused pass)
};
// Everything a proposed_algorithm solve is given (the arguments of jstsp_proposed_resume_c32, include/jstsp.h; Cx / Re: complex / real
// element).  Per-trial arrays are contiguous, trial index slowest: a sub-batch is this record with its pointers moved, by sub() only.
template <class Cx, class Re> struct AdmmProblemOf {
    int N = 0, M = 0, Gr = 0, G2 = 0, batch = 0;
    const Cx *subY = nullptr; const Re *Omega = nullptr; const Cx *A = nullptr, *B = nullptr;
    const double *tau_Y = nullptr, *tau_S = nullptr, *rho = nullptr;
    long long strideA = 0, strideB = 0;          // elements between the dictionaries of two trials, 0 = one for the batch
    int Imax = 0, type = 0;
    const int32_t *indx_S = nullptr;
    Cx *S_out = nullptr, *Y_out = nullptr; double *ce_out = nullptr;
    int it0 = 0; const Cx *state_in = nullptr; Cx *state_out = nullptr;
    int memspace = JSTSP_HOST;
    // The support policy of jstsp_proposed_refresh_c32 (include/jstsp.h; every other entry passes none): indx_S lists n_indx entries
    // per trial, the global 1-based iteration i refreshes the rank from the solver's own v when refresh_at(i), and the list of the
    // call's last refresh goes to indx_out (R() entries per trial; NULL: not wanted).
    bool policy = false;
    int n_indx = 0, start = 0, period = 0;
    int32_t *indx_out = nullptr;
    // The stopping rule of jstsp_proposed_until_c32 (include/jstsp.h; every other entry passes none: iters_out == NULL): trial t stops
    // after the first iteration k of the call with k >= min_iters and ce(k, 3) <= tol[t] (host doubles, as tau_Y); every `check`
    // iterations the host reads how many trials still run.  live(): some tol is positive, so a trial can stop before Imax.
    bool rule = false;                           // the entry takes a rule: tol and iters_out are then required (check_rule_arrays)
    const double *tol = nullptr;
    int min_iters = 0, check = 0;
    int32_t *iters_out = nullptr; double *ce3_out = nullptr;
    void set_policy(int n, int start_, int period_, int32_t *order_out) { policy = true; n_indx = n; start = start_; period = period_; indx_out = order_out; }
    void set_rule(const double *tol_, int min_iters_, int check_, int32_t *iters, double *ce3)
    {
        rule = true; tol = tol_; min_iters = min_iters_; check = check_; iters_out = iters; ce3_out = ce3;
    }
    bool until() const { return iters_out != nullptr; }
    bool live() const
    {
        for (int t = 0; until() && tol && t < batch; ++t)
            if (tol[t] > 0.0) return true;
        return false;
    }
    size_t nm() const { return (size_t)N * M; }
    size_t g() const { return (size_t)Gr * G2; }
    size_t state_elems() const { return 4 * nm() + 2 * g(); }
    size_t listed() const { return n_indx ? (size_t)n_indx : g(); }                  // entries per trial of indx_S (0: every entry)
    size_t R() const { return std::min<size_t>(g(), JSTSP_SUPPORT_TOP_MAX); }       // entries of a refreshed order
    bool refresh_at(long long i) const { return policy && i > start && (period ? (i - start - 1) % period == 0 : i == (long long)start + 1); }
    bool runs_refresh() const          // a function of it0, Imax, start and period alone
    {
        for (int it = 0; it < Imax; ++it)
            if (refresh_at((long long)it0 + it + 1)) return true;
        return false;
    }
    // Trials t0 .. t0 + cnt - 1.  A NULL pointer stays NULL, a zero stride stays the shared dictionary.  No product wraps: the
    // entries have checked every factor (positive shape, 0 <= t0 < batch, strides 0 or at least one dictionary), and each
    // offset lies inside an array of `batch` such slices that the caller holds in memory.
    AdmmProblemOf sub(int t0, int cnt) const
    {
        auto at = [t0](auto *p, size_t per) { return p ? p + (size_t)t0 * per : nullptr; };
        AdmmProblemOf s = *this;
        s.batch = cnt;
        s.subY = at(subY, nm()); s.Omega = at(Omega, nm()); s.A = at(A, (size_t)strideA); s.B = at(B, (size_t)strideB);
        s.tau_Y = at(tau_Y, 1); s.tau_S = at(tau_S, 1); s.rho = at(rho, 1); s.indx_S = at(indx_S, listed());
        s.indx_out = at(indx_out, R());
        s.tol = at(tol, 1); s.iters_out = at(iters_out, 1); s.ce3_out = at(ce3_out, 1);
        s.S_out = at(S_out, g()); s.Y_out = at(Y_out, nm()); s.ce_out = at(ce_out, (size_t)3 * Imax);
        s.state_in = at(state_in, state_elems()); s.state_out = at(state_out, state_elems());
        return s;
    }
};
using AdmmProblem = AdmmProblemOf<jstsp_c32, float>;          // what the solver takes
using AdmmProblem64 = AdmmProblemOf<jstsp_c64, double>;       // the same arrays as the _c64 entries receive them (c64.hip)

// The argument checks that the entries of the family share - fp32, _c64 and float64 (proposed.hip, c64.hip, proposed64.hip) - each
// worded once; nmf names the entry in the message.  An entry applies them in its own order between its own checks, so which
// refusal wins for a given bad call is the entry's business.
// ... the resumed pair: iterations it0 + 1 .. it0 + Imax, from state_in (NULL: from zero, and then it0 is 0)
template <class Cx, class Re> int check_resumed(const char *nmf, const AdmmProblemOf<Cx, Re> &p)
{
    JSTSP_REQUIRE(p.it0 >= 0 && p.it0 <= INT_MAX - p.Imax, JSTSP_E_ARG, "%s: it0 = %d with Imax = %d: need 0 <= it0 and it0 + Imax within int", nmf,
                  p.it0, p.Imax);
    JSTSP_REQUIRE(p.state_in || p.it0 == 0, JSTSP_E_ARG, "%s: it0 = %d without state_in: a call from zero starts at iteration 1 (it0 = 0)", nmf, p.it0);
    return 0;
}
// ... the support policy: its schedule, and its list (jstsp_proposed_until_c32 words the schedule's refusal itself: schedule = false)
template <class Cx, class Re> int check_policy(const char *nmf, const AdmmProblemOf<Cx, Re> &p, bool schedule = true)
{
    JSTSP_REQUIRE(!schedule || (p.start >= 0 && p.period >= 0), JSTSP_E_ARG, "%s: refresh_start = %d, refresh_period = %d: neither may be negative", nmf,
                  p.start, p.period);
    JSTSP_REQUIRE(p.indx_S ? p.n_indx >= 1 && p.n_indx <= (long long)p.g() : p.n_indx == 0, JSTSP_E_ARG,
                  "%s: n_indx = %d: need 1 <= n_indx <= Gr * G2 = %lld with indx_S, and 0 without", nmf, p.n_indx, (long long)p.g());
    return 0;
}
// ... the stopping rule: its arrays, its counts, and the list of a call without a policy (fmt takes nmf, n_indx and Gr * G2: the _c64
// entry, which judges the list before it narrows it, has words of its own)
template <class Cx, class Re> int check_rule_arrays(const char *nmf, const AdmmProblemOf<Cx, Re> &p)
{
    JSTSP_REQUIRE(p.tol && p.iters_out, JSTSP_E_NULL, "%s: tol and iters_out are required", nmf);
    return 0;
}
template <class Cx, class Re> int check_rule_counts(const char *nmf, const AdmmProblemOf<Cx, Re> &p)
{
    JSTSP_REQUIRE(p.min_iters >= 1 && p.check >= 1, JSTSP_E_ARG, "%s: min_iters = %d, check = %d: both must be at least 1", nmf, p.min_iters, p.check);
    return 0;
}
template <class Cx, class Re>
int check_rule_list(const char *nmf, const AdmmProblemOf<Cx, Re> &p,
                    const char *fmt = "%s: n_indx = %d: need 0 (all) or 1 <= n_indx <= Gr * G2 = %lld with indx_S, and 0 without")
{
    JSTSP_REQUIRE(p.n_indx >= 0 && (p.indx_S || p.n_indx == 0) && p.n_indx <= (long long)p.g(), JSTSP_E_ARG, fmt, nmf, p.n_indx, (long long)p.g());
    return 0;
}

// jstsp_proposed_resume_c32, _refresh_c32 (the record has a policy) and _until_c32 (it has a rule) behind their C prototypes
// (proposed.hip): that entry's checks in its order, then one staged solve with its recovery.  c64.hip calls it with the narrowed record.
int proposed_resumed_entry(jstsp_ctx *ctx, AdmmProblem &p);

// Runs of consecutive trials in an ascending list of flagged ones: fn(first trial, count) for each, until one fails.
template <class F> int for_each_run(const std::vector<int> &ovf, F &&fn)
{
    for (size_t i = 0, j; i < ovf.size(); i = j) {
        j = i + 1;
        while (j < ovf.size() && ovf[j] == ovf[j - 1] + 1) ++j;
        JSTSP_TRY(fn(ovf[i], (int)(j - i)));
    }
    return 0;
}
// The indices of the set words of a host copy of the per-trial overflow flags, appended to *out.
inline void flagged_trials(const uint32_t *flags, size_t n, std::vector<int> *out)
{
    for (size_t t = 0; t < n; ++t)
        if (flags[t]) out->push_back((int)t);
}
// The same from the device array (NULL: the solve did not use the fused pass): one copy, ONE synchronisation of ctx->stream.
int read_flagged_trials(jstsp_ctx *ctx, const uint32_t *dev_flags, int batch, std::vector<int> *out);

// The frame of a JSTSP_HOST call that runs as two halves on two contexts of the device (proposed.hip, c64.hip): trials
// t0[k] .. t0[k] + cnt[k] - 1 on cx[k]; close() leaves the call's fallbacks and dictionary block in the caller's context.
struct HostPipeline {
    jstsp_ctx *cx[2] = {nullptr, nullptr};
    int t0[2] = {0, 0}, cnt[2] = {0, 0}, fallbacks = 0;
    int open(jstsp_ctx *ctx, int batch)
    {
        if (!ctx->helper) JSTSP_TRY(jstsp_create(ctx->device, &ctx->helper));
        cx[0] = ctx; cx[1] = ctx->helper;
        t0[1] = cnt[0] = ((batch / 2 + 7) / 8) * 8; cnt[1] = batch - cnt[0];
        return 0;
    }
    // (a failure inside the pipeline - typically JSTSP_E_NOMEM for the helper's workspace - must not return while the other
    //  half still reads the caller's host arrays or writes its outputs: both streams are drained first)
    int drained(int rc) const
    {
        if (rc) for (int k = 0; k < 2; ++k) { DeviceScope ds(cx[k]->device); (void)hipStreamSynchronize(cx[k]->stream); }
        return rc;
    }
    void close() const
    {
        cx[0]->fused_fallbacks = fallbacks;
        cx[0]->last_dict_block = (cx[0]->last_dict_block == cx[1]->last_dict_block) ? cx[0]->last_dict_block : 0;
    }
};
#define JSTSP_TRY_PIPE(pipe, expr) do { int rc_ = (pipe).drained(expr); if (rc_ != 0) return rc_; } while (0)

// For a caller that stages its own inputs (c64.hip), every array of the record in device memory.  enqueue: the whole solve without
// its final copies and flag read (the record's outputs are not written); resolve: a run of flagged trials again, unfused.
int proposed_enqueue_device(jstsp_ctx *ctx, const AdmmProblem &p, bool want_ce, PendingSolve *out);
int proposed_resolve_device(jstsp_ctx *ctx, const AdmmProblem &run);

// Host -> device scalar block.
int upload(jstsp_ctx *ctx, void *dst, const void *src, size_t bytes);

// Staging of an array argument according to memspace: returns a device pointer (the caller's
// pointer for JSTSP_DEVICE, an arena copy for JSTSP_HOST).
template <class T> int stage_in(jstsp_ctx *ctx, const T *src, size_t n, int memspace, const T **out)
{
    if (memspace == JSTSP_DEVICE) { *out = src; return 0; }
    T *d = ctx->arena.get<T>(n);
    JSTSP_REQUIRE(d, JSTSP_E_NOMEM, "workspace exhausted while staging an input");
    JSTSP_HIP(hipMemcpyAsync(d, src, n * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    *out = d;
    return 0;
}
template <class T> int stage_out(jstsp_ctx *ctx, T *dst, const T *dev, size_t n, int memspace)
{
    if (!dst) return 0;
    JSTSP_HIP(hipMemcpyAsync(dst, dev, n * sizeof(T),
                             memspace == JSTSP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost,
                             ctx->stream));
    return 0;
}
inline size_t rnd256(size_t b) { return (b + 255) & ~size_t(255); }
inline const float2 *as_f2(const jstsp_c32 *p) { return reinterpret_cast<const float2 *>(p); }
inline float2 *as_f2(jstsp_c32 *p) { return reinterpret_cast<float2 *>(p); }

// Opens the workspace of a call on the context's arena: layout(Arena &) takes every array of the call, staged inputs (Arena::in)
// included, and nothing else - no HIP call, no launch.  It runs on a measuring arena, the arena is grown to the measured peak,
// and the same function then hands out the arrays and uploads the inputs of a host call.  There is no second statement of the
// size; two passes that disagree are an internal error, found here by one comparison instead of a check per array.
template <class Layout> int arena_open(jstsp_ctx *ctx, const char *nm, Layout &&layout)
{
    Arena m = Arena::measuring();
    layout(m);
    Arena &a = ctx->arena;
    JSTSP_TRY(a.reserve(m.peak));
    a.reset();
    a.st = ctx->stream;
    layout(a);
    JSTSP_REQUIRE(!a.overrun && a.off == m.off && a.peak == m.peak, JSTSP_E_NOMEM,
                  "%s: internal error: the workspace was measured as %zu bytes (ending at %zu) and laid out as %zu (ending at %zu)%s", nm,
                  m.peak, m.off, a.peak, a.off, a.overrun ? ", past its end" : "");
    if (a.err != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);    // (the uploads before it may still read the caller's arrays)
        set_error("%s: staging an input on the device failed: %s", nm, hipGetErrorString(a.err));
        return (int)a.err;
    }
    return 0;
}

// Host-side staging of a block-Toeplitz dictionary (hostpack.hip): T = float2 or double2 (narrowed while copying).
// *gt_out = the block height when the compact route was taken (Bdev then receives the expanded array on ctx->stream), 0 otherwise
// (nothing uploaded).  Cdev: device room for the compact form, host_toeplitz_compact_elems() float2.
template <class T>
int host_toeplitz_stage(jstsp_ctx *ctx, const T *Bh, int G2, int M, int nB, float2 *Bdev, float2 *Cdev, size_t cdev_elems, int *gt_out);
size_t host_toeplitz_compact_elems(int G2, int M, int nB);

// ---- one pass over the dictionary per iteration (fused.hip) ---------------------------------
struct FusedWS {
    uint4 *Bf = nullptr; long long sBf = 0;       // tile images of B, uint4 per problem
    uint4 *ASp = nullptr; long long sAS = 0;      // B-operand fragments of (A S)^T, re-packed every iteration
    float2 *Ppart = nullptr;                      // [batch][parts][N x G2] partial sums of K B^H
    uint32_t *ovf = nullptr;                      // [batch]: raised for a trial when a k entry left the f16 range of its scale
    uint4 *Wqp = nullptr;                         // B-operand fragments of (I - Q)^T, 2048 uint4 per problem
    int parts = 0;
    // block-Toeplitz dictionary (fused.hip, "compact image"): B(ld Gt + g, m) == B(g, m - ld) bit for bit for m >= ld.
    // Then only block 0 (+ the ld leading columns of block ld) is stored, and the pass's refill reads it at shifted columns.
    uint4 *Ec = nullptr; long long sEc = 0;       // compact image, uint4 per problem; Bf stays NULL then
    int gt = 0, ecols = 0, ehalo = 0;             // block height (0: unstructured), chunks per image row, halo chunks before column 0
    // v2 (block height 64, fused_pass64_kernel): the LDS tile is the 39-column window of block 0 itself; the leading columns
    // m < ld of block ld (outside the Toeplitz part) are applied as fp32 corrections around the pass
    int v2 = 0;
    const float2 *Bsrc = nullptr; long long sBsrc = 0;    // the caller's dictionary
    float2 *Bdl = nullptr; long long sBdl = 0;            // its leading columns, row-major: [nB][G2][8]
    float2 *XsD = nullptr, *Kf = nullptr;                 // [batch][4][64 x 8]: (A S) Delta of this iteration in four partial sums; [batch][64 x 8]: k(:, 0..6) of the pass
};
struct FusedDesc {
    const uint4 *Bf; long long sBf;               // 0: one dictionary for the batch
    const uint32_t *bmax; int sbmax;
    const uint4 *ASp; long long sAS;
    const uint32_t *wmax;                         // [batch] max|A S|
    const uint32_t *kmax_prev;                    // [batch] max|k| of the previous iteration
    float2 *X, *V1, *V2;                          // N x M state, updated in place
    const float2 *subY, *Y; const float *invD;
    long long snm;
    const TrialParams *prm;
    float2 *Ppart;
    uint32_t *kmax_out, *xmax, *v1max, *zmax, *v2max, *ovf;
    int M, G2, batch, parts;
    // Y formed in the pass (instead of read from Y): fragments of I - Q, the svt argument Z of the next iteration and its
    // maximum, where to put the Z after that; Yout != NULL: also store Y (the last pass: Y is an output of the solver)
    const uint4 *Wqp; const float2 *Zin; const uint32_t *zmax_in; float2 *Zout, *Yout;
    int kback;                                    // headroom of the predicted k scale in bits (KBACK; JSTSP_FUSED_KBACK: tests)
    const uint4 *Ec; long long sEc; int gsh, ecols, ehalo;   // compact image of a block-Toeplitz dictionary (gsh = log2 Gt; 0: none)
    int v2; const float2 *XsD; float2 *Kf;                   // fused_pass64_kernel (see FusedWS)
    int inv_is_omega;                             // invD points at the caller's Omega (16-byte aligned): 1 / (Omega + 2 rho) is formed in the
                                                  // pass as two floats (common.h: admm_invd) instead of read as one rounded float
};
bool fused_shape_ok(int N, int M, int G2, int parts);
size_t fused_bytes(int M, int G2, int nB, int batch, int parts);
int fused_probe_toeplitz(jstsp_ctx *ctx, Arena &ar, const float2 *B, long long sBt, int G2, int M, int nB, int *gt);   // syncs
// G_B = B B^H (G2 x G2, column-major) of a block-Toeplitz dictionary from its first block row G0 = B(0:gt, :) B^H (gt x G2)
int toeplitz_gram_assemble(jstsp_ctx *ctx, const float2 *B, long long sBt, int G2, int M, int gt, int nB, const float2 *G0,
                           const float2 *G0lo, float2 *G, float2 *Glo);     // G0lo, Glo optional: low-order parts (float64 = hi + lo)
int fused_alloc(Arena &ar, FusedWS &f, int M, int G2, int nB, int batch, int parts, int gt, int v2);
int fused_pack_b(jstsp_ctx *ctx, FusedWS &f, const float2 *B, long long sBt, int G2, int M, int nB, const uint32_t *bmax);
int fused_pack_as(jstsp_ctx *ctx, const FusedWS &f, const float2 *W, long long sWt, int G2, int M, int batch, const uint32_t *wmax);
int launch_fused_pass(jstsp_ctx *ctx, const FusedDesc &d);
int fused_reduce(jstsp_ctx *ctx, const FusedWS &f, int G2, int M, int batch, float2 *Tc);
int fused_pack_wq(jstsp_ctx *ctx, const FusedWS &f, const float2 *Q, int batch);      // from the raw Q of svt_prepare

// ---- fused launches of the gradient step between two passes (gradstep.hip; JSTSP_FUSED=2 runs the separate launches) -----------------------------
bool grad_fused_shape(int N, int Gr, int G2);
// Res = A^H Tc - R v and P1 = G_A Res (+ max|P1| into pmax[t]) in one launch: the bits of the two cgemm launches it replaces
int launch_grad_res_p1(jstsp_ctx *ctx, const float2 *A, long long sAt, const float2 *Tc, const float2 *RV, float2 *Res,
                       const float2 *GA, long long sGAt, float2 *P1, uint32_t *pmax, int G2, int batch);
// first factor of the recomputation of R v, P1 = G_A,hi V + (G_A,lo V), in one launch: the bits of the two cgemm launches it
// replaces (P1 = G_A,lo V; P1 = G_A,hi V + P1); no maximum is formed
int launch_grad_refresh_p1(jstsp_ctx *ctx, const float2 *V, const float2 *GA, const float2 *GAlo, long long sGAt, float2 *P1, int G2,
                           int batch);

}  // namespace jstsp
