// Singular values in float64 by one-sided (Hestenes) Jacobi, and the spectrum sweep of plot_rankR.m:
//
//   plot_rankR.m:49 ([U,S,V] = svd(Y); only diag(S) is used) -> svdvals_kernel: the singular values of given matrices
//   plot_rankR.m:24-50                                        -> rank_sweep_kernel: the channel and pilots of
//                                                                jstsp_build_trials_c32's trial t, the noise-free
//                                                                Y = sum_l H_l Psi_bar_l (proposed_hbf.m:15-20), its values
//
// Why not a Gram: the other spectral kernels of the library (eig*.hip, vamp64.hip) decompose Y Y^H, whose condition number is
// the square of Y's, so a zero singular value comes back near sqrt(eps) sigma_1 even in float64 - and the figure is about
// exactly that tail.  Here the rotations act on the columns of Y itself: one workgroup holds the matrix in LDS as complex
// double, oriented to n = min(rows, cols) columns of length m = max(rows, cols) (Y^H when rows < cols), and runs cyclic sweeps
// over the column pairs.  For a pair (p, q): a = |c_p|^2, b = |c_q|^2, g = c_p^H c_q; if |g| > tol sqrt(a b) the plane rotation
//   c_p <- c c_p - s w* c_q,  c_q <- s c_p + c w* c_q,   w = g / |g|,  t = sign(z) / (|z| + sqrt(1 + z^2)),  z = (b - a) / (2 |g|)
// makes the two columns orthogonal.  The n/2 disjoint pairs of a round-robin round run in parallel, one wave per pair with
// the three inner products by wave reductions; a column is a run of consecutive 16-byte elements, so the 64 lanes of a wave
// read whole 256-byte bank rows without conflicts.  The loop ends when a full sweep rotates nothing, or after SV_SWEEPS
// sweeps.  The singular values are the final column norms, sorted; no singular vector is formed (svd64.hip keeps them: the same sweep loop, jacobi64.h).  The operand is scaled by a
// power of two to max |entry| in [1/2, 1) first (exact), so no squared norm overflows or underflows; a non-finite entry
// gives NaN for that matrix.  Columns that have shrunk to eps |Y|_F / sqrt(n) are not rotated any further (jacobi_sweeps).
//
// Beyond the LDS limit (jstsp_spectrum_c32 / _c64 / jstsp_spectrum_trials_c32) - still no Gram:
//   n <= 64, m <= 65536: tsqr_values_kernel.  One workgroup per matrix walks the oriented operand once (after the scale pre-pass), in chunks of 128 (n <= 48)
//     or 64 rows, and reduces each stack [R; chunk] to a new n x n triangle R by Householder reflections in LDS (a reflector of
//     column j touches row j of R and the chunk only, so R stays triangular); Householder, not Gram-Schmidt, because the operands
//     of interest have rank 4..24 of 32..64 and a column in the span of the earlier ones must not be normalised.  The chunks are
//     walked in order, so the result does not depend on the batch; the next chunk is fetched into registers while the current one
//     is reduced.  R then goes to singular_values_block above, unchanged: sv(R) = sv(Y).  A pre-pass finds the largest component
//     and the loader multiplies by the power of two that brings it into [1/2, 1) (the trial loader: by a power of two from the
//     bound 2 L Nt max|H| max|pilot|, its entries being sums), undone at the end; both exact.
//   64 < n <= 512, m <= 8192: the global-memory one-sided Jacobi of pinv64.hip without the inverse (pinv64_values), which
//     synchronises the stream once per sweep.
#include "inputgen.h"
#include "jacobi64.h"
#include "pinv64.h"
#include "tsqr64.h"

using namespace jstsp;

namespace {

constexpr int SV_ELEMS = 8192;      // rows * cols: 128 KiB of complex double in LDS

// After A (m x n, oriented) has been written: scale, sweep, sort.  LDS behind A: n doubles (norms), SV_RED doubles.
__device__ void singular_values_block(double2 *A, int m, int n, int n_keep, double *out)
{
    double *nrm = reinterpret_cast<double *>(A + (size_t)m * n), *red = nrm + n;
    double unscale, fro2;
    if (prescale(A, m, 0, n, red, &unscale, &fro2)) {
        for (int i = threadIdx.x; i < n_keep; i += blockDim.x) out[i] = __builtin_nan("");
        return;
    }
    jacobi_sweeps(A, m, 0, n, fro2);
    sorted_norms(A, m, 0, n, nrm, unscale, n_keep, out);
}

inline size_t sv_lds_bytes(int m, int n) { return (size_t)m * n * sizeof(double2) + (size_t)(n + SV_RED) * sizeof(double); }
inline bool sv_fits(int rows, int cols) { return std::min(rows, cols) <= SV_NMAX && (long long)rows * cols <= SV_ELEMS; }

template <class T> __global__ __launch_bounds__(64 * SV_WAVES) void svdvals_kernel(int rows, int cols, const T *Y, double *sv)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x;
    const bool tall = rows >= cols;
    const int m = tall ? rows : cols, n = tall ? cols : rows;
    const T *Yt = Y + (size_t)rows * cols * t;
    for (int e = threadIdx.x; e < rows * cols; e += blockDim.x) {
        const double2 v = ld2(Yt[e]);
        if (tall) lds[e] = v;
        else lds[e / rows + m * (e % rows)] = make_double2(v.x, -v.y);            // Y^H
    }
    singular_values_block(lds, m, n, n, sv + (size_t)n * t);
}

// One workgroup per trial: Y = [H_1 .. H_L] Psi (proposed_hbf.m:15-20 with N = 0), Nr x Tp, in LDS, then its singular values.
__global__ __launch_bounds__(64 * SV_WAVES) void rank_sweep_kernel(Model mdl, const float2 *Hmat, const float2 *psym, float pscale,
                                                                   int n_keep, double *sv)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x;
    const bool tall = mdl.Nr >= mdl.Tp;
    const int m = tall ? mdl.Nr : mdl.Tp, n = tall ? mdl.Tp : mdl.Nr;
    const float2 *H = Hmat + (size_t)t * mdl.Nr * mdl.NtL;
    const float2 *sym = psym + (size_t)t * mdl.Nt * mdl.Tp;
    for (int e = threadIdx.x; e < mdl.Nr * mdl.Tp; e += blockDim.x) {
        const int r = e % mdl.Nr, j = e / mdl.Nr;
        const double2 v = received_entry(mdl, H, sym, pscale, r, j);
        if (tall) lds[e] = v;
        else lds[j + m * r] = make_double2(v.x, -v.y);
    }
    singular_values_block(lds, m, n, n_keep, sv + (size_t)n_keep * t);
}


// ---- beyond the LDS limit, n <= 64: tall-skinny QR in front of the Jacobi -------------------------------------------------------
// (the chunk rule, the matrix loader and the reduction tq_reduce: tsqr64.h, shared with svd64.hip)

// a loader like MatrixLoader: the noise-free receive signal of a trial, entry by entry (received_entry, inputgen.h): each entry is formed once
struct TrialLoader {
    Model mdl;
    const float2 *H, *sym;
    float pscale;
    int rows, cols;
    __device__ void bind(int t) { H += (size_t)t * mdl.Nr * mdl.NtL; sym += (size_t)t * mdl.Nt * mdl.Tp; }
    __device__ bool scan(double *red, int *ex) const
    {
        double hmax = 0.0, smax = 0.0;
        int bad = 0;
        for (int e = threadIdx.x; e < mdl.Nr * mdl.NtL; e += blockDim.x) {
            const float2 v = H[e];
            bad |= !isfinite(v.x) || !isfinite(v.y);
            hmax = fmax(hmax, (double)fmaxf(fabsf(v.x), fabsf(v.y)));
        }
        for (int e = threadIdx.x; e < mdl.Nt * mdl.Tp; e += blockDim.x) {
            const float2 v = sym[e];
            bad |= !isfinite(v.x) || !isfinite(v.y);
            smax = fmax(smax, (double)fmaxf(fabsf(v.x * pscale), fabsf(v.y * pscale)));
        }
        if (block_max_or_bad(hmax, bad, red)) return true;
        __syncthreads();                                           // every wave has read the maxima of H
        if (block_max_or_bad(smax, 0, red)) return true;
        const double bound = 2.0 * (double)mdl.NtL * hmax * smax;  // |re|, |im| of an entry: a sum of 2 L Nt products
        int e2 = 0;
        if (bound > 0.0) frexp(bound, &e2);
        *ex = e2;
        return false;
    }
    __device__ __forceinline__ double2 at(int r, int c, double sc) const
    {
        const double2 v = received_entry(mdl, H, sym, pscale, r, c);
        return make_double2(v.x * sc, v.y * sc);
    }
};

template <class L> __global__ __launch_bounds__(TQ_THREADS) void tsqr_values_kernel(L ld, int n_keep, double *sv)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x, tid = threadIdx.x;
    ld.bind(t);
    const bool tall = ld.rows >= ld.cols;
    const int m = tall ? ld.rows : ld.cols, n = tall ? ld.cols : ld.rows, C = tq_chunk(n);
    double2 *R = lds, *Ck = lds + (size_t)n * n;
    double *scr = reinterpret_cast<double *>(Ck);
    double *out = sv + (size_t)n_keep * t;
    int ex = 0;
    if (ld.scan(scr, &ex)) {
        for (int i = tid; i < n_keep; i += TQ_THREADS) out[i] = __builtin_nan("");
        return;
    }
    const double sc = ldexp(1.0, -ex);
    for (int e = tid; e < n * n; e += TQ_THREADS) R[e] = make_double2(0.0, 0.0);
    // chunk entry e of rows [i0, i0 + cc): consecutive threads on consecutive addresses of the operand - down a column of a tall
    // one, along the contiguous rows x cc block of a wide one (whose adjoint is what is reduced)
    double2 pre[TQ_PRE];
    auto fetch = [&](int i0) {
        const int cc = min(C, m - i0);
#pragma unroll
        for (int q = 0; q < TQ_PRE; ++q) {
            const int e = tid + q * TQ_THREADS;
            if (e < cc * n) {
                if (tall) pre[q] = ld.at(i0 + e % cc, e / cc, sc);
                else {
                    const double2 v = ld.at(e % n, i0 + e / n, sc);
                    pre[q] = make_double2(v.x, -v.y);
                }
            }
        }
    };
    fetch(0);
    for (int i0 = 0; i0 < m; i0 += C) {
        const int cc = min(C, m - i0);
        __syncthreads();                                           // the chunk before this one is reduced (first: the scan's scratch is read)
#pragma unroll
        for (int q = 0; q < TQ_PRE; ++q) {
            const int e = tid + q * TQ_THREADS;
            if (e < cc * n) Ck[tall ? e % cc + C * (e / cc) : e / n + C * (e % n)] = pre[q];
        }
        __syncthreads();
        if (i0 + C < m) fetch(i0 + C);
        tq_reduce(R, Ck, n, C, cc);
    }
    // nrm and red of singular_values_block lie behind R, in the chunk's place; the values go through LDS to be scaled back
    double *vals = scr + n + SV_RED;
    singular_values_block(R, n, n, n_keep, vals);
    __syncthreads();
    const double back = ldexp(1.0, ex);
    for (int i = tid; i < n_keep; i += TQ_THREADS) out[i] = vals[i] * back;
}

template <class L> int tsqr_launch(hipStream_t st, const L &ld, int n, int batch, int n_keep, double *sv)
{
    const size_t sh = tq_lds_bytes(n) < 1024 ? 1024 : tq_lds_bytes(n);
    JSTSP_HIP(hipFuncSetAttribute((const void *)tsqr_values_kernel<L>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    tsqr_values_kernel<L><<<batch, TQ_THREADS, sh, st>>>(ld, n_keep, sv);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

// ---- 64 < n <= 512: the operand as complex double for pinv64_values ---------------------------------------------------------------
__global__ __launch_bounds__(256) void widen_kernel(long long cnt, const float2 *src, double2 *dst)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < cnt; e += (long long)gridDim.x * 256) dst[e] = ld2(src[e]);
}

__global__ __launch_bounds__(256) void received_kernel(Model mdl, const float2 *Hmat, const float2 *psym, float pscale, double2 *Y)
{
    const int t = blockIdx.y;
    const float2 *H = Hmat + (size_t)t * mdl.Nr * mdl.NtL, *sym = psym + (size_t)t * mdl.Nt * mdl.Tp;
    const long long cnt = (long long)mdl.Nr * mdl.Tp;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < cnt; e += (long long)gridDim.x * 256)
        Y[(size_t)t * cnt + e] = received_entry(mdl, H, sym, pscale, (int)(e % mdl.Nr), (int)(e / mdl.Nr));
}

// sv[k + n_keep t] = full[k + n t], k < n_keep
__global__ __launch_bounds__(256) void leading_kernel(int n, int n_keep, long long cnt, const double *full, double *sv)
{
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e < cnt) sv[e] = full[e % n_keep + (long long)n * (e / n_keep)];
}

inline bool spectrum_shape_ok(int rows, int cols) { return sv_fits(rows, cols) || tq_fits(rows, cols) || pinv64_shape_ok(rows, cols); }
#define SPECTRUM_LIMITS "min(rows, cols) <= 512, max(rows, cols) <= 65536, and max(rows, cols) <= 8192 when min(rows, cols) > 64"

template <class T>
int singular_values_impl(jstsp_ctx *ctx, int rows, int cols, int batch, const T *Y, double *sv, int memspace, const char *what)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "%s: NULL context", what);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "%s: bad memspace", what);
    JSTSP_REQUIRE(Y && sv, JSTSP_E_NULL, "%s: NULL argument", what);
    JSTSP_REQUIRE(rows > 0 && cols > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", what);
    JSTSP_REQUIRE(sv_fits(rows, cols), JSTSP_E_UNSUPPORTED, "%s: need min(rows, cols) <= %d and rows * cols <= %d", what, SV_NMAX,
                  SV_ELEMS);
    JSTSP_ENTER(ctx);
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    const size_t nY = (size_t)rows * cols * batch, nS = (size_t)n * batch;
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(ctx->arena.reserve(rnd256(nY * sizeof(T)) + rnd256(nS * 8) + 4096));
        ctx->arena.reset();
    }
    const T *y;
    JSTSP_TRY(stage_in(ctx, Y, nY, memspace, &y));
    double *o = memspace == JSTSP_DEVICE ? sv : ctx->arena.get<double>(nS);
    JSTSP_REQUIRE(o, JSTSP_E_NOMEM, "%s: workspace exhausted", what);
    const size_t sh = sv_lds_bytes(m, n);
    JSTSP_HIP(hipFuncSetAttribute((const void *)svdvals_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    svdvals_kernel<T><<<batch, sv_threads(n), sh, ctx->stream>>>(rows, cols, y, o);
    JSTSP_HIP(hipGetLastError());
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(stage_out(ctx, sv, o, nS, memspace));
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}


template <class T>
int spectrum_impl(jstsp_ctx *ctx, int rows, int cols, int batch, const T *Y, int n_keep, double *sv, int memspace, const char *what)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "%s: NULL context", what);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "%s: bad memspace", what);
    JSTSP_REQUIRE(Y && sv, JSTSP_E_NULL, "%s: NULL argument", what);
    JSTSP_REQUIRE(rows > 0 && cols > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", what);
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    JSTSP_REQUIRE(n_keep >= 1 && n_keep <= n, JSTSP_E_SHAPE, "%s: need 1 <= n_keep <= min(rows, cols)", what);
    JSTSP_REQUIRE(spectrum_shape_ok(rows, cols), JSTSP_E_UNSUPPORTED, "%s: %d x %d: need " SPECTRUM_LIMITS, what, rows, cols);
    const bool host = memspace == JSTSP_HOST;
    const size_t nY = (size_t)rows * cols * batch, nS = (size_t)n_keep * batch;
    if (sv_fits(rows, cols)) {                                     // the LDS kernel and its bits
        if (n_keep == n) return singular_values_impl(ctx, rows, cols, batch, Y, sv, memspace, what);
        JSTSP_ENTER(ctx);
        hipStream_t st = ctx->stream;
        const T *y;
        double *full, *o;
        Slab s(st);
        JSTSP_TRY(ws64_open(s, what, batch, [&](Slab &w, int b) {
            y = w.in(Y, (size_t)rows * cols * b, host);
            full = w.get<double>((size_t)n * b);
            o = w.out(sv, (size_t)n_keep * b, host);
        }));
        const size_t sh = sv_lds_bytes(m, n);
        JSTSP_HIP(hipFuncSetAttribute((const void *)svdvals_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        svdvals_kernel<T><<<batch, sv_threads(n), sh, st>>>(rows, cols, y, full);
        leading_kernel<<<(unsigned)((nS + 255) / 256), 256, 0, st>>>(n, n_keep, (long long)nS, full, o);
        JSTSP_HIP(hipGetLastError());
        if (host) {
            JSTSP_TRY(s.copy_back(sv, o, nS));
            JSTSP_HIP(hipStreamSynchronize(st));
        }
        return 0;
    }
    JSTSP_ENTER(ctx);
    hipStream_t st = ctx->stream;
    Slab s(st);
    if (tq_fits(rows, cols)) {
        const T *y;
        double *o;
        JSTSP_TRY(ws64_open(s, what, batch, [&](Slab &w, int b) {
            y = w.in(Y, (size_t)rows * cols * b, host);
            o = w.out(sv, (size_t)n_keep * b, host);
        }));
        JSTSP_TRY(tsqr_launch(st, MatrixLoader<T>{y, rows, cols}, n, batch, n_keep, o));
        if (host) {
            JSTSP_TRY(s.copy_back(sv, o, nS));
            JSTSP_HIP(hipStreamSynchronize(st));
        }
        return 0;
    }
    JSTSP_REQUIRE(batch <= 65535, JSTSP_E_UNSUPPORTED, "%s: %d x %d, batch %d: orders above 64 need batch <= 65535", what, rows, cols, batch);
    constexpr bool narrow = sizeof(T) == sizeof(float2);
    const T *y;
    double2 *y64 = nullptr;
    double *o;
    Pinv64Arrays pv{};
    JSTSP_TRY(ws64_open(s, what, batch, [&](Slab &w, int b) {
        y = w.in(Y, (size_t)rows * cols * b, host);
        if (narrow) y64 = w.get<double2>((size_t)rows * cols * b);
        o = w.out(sv, (size_t)n_keep * b, host);
        pv.W = w.get<double2>((size_t)m * n * b); pv.V = w.get<double2>((size_t)n * n * b);
        pv.meta = w.get<PvMeta>(b);
        pv.any = w.get<int>(1);
    }));
    const double2 *a;
    if constexpr (narrow) {
        widen_kernel<<<grid_for((long long)nY), 256, 0, st>>>((long long)nY, y, y64);
        JSTSP_HIP(hipGetLastError());
        a = y64;
    } else {
        a = y;
    }
    JSTSP_TRY(pinv64_values(st, pv, rows, cols, batch, a, (long long)rows * cols, n_keep, o));
    if (host) {
        JSTSP_TRY(s.copy_back(sv, o, nS));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

// ---- scoring a float64 estimate: spectral NMSE and rate (jstsp_nmse_spectral_f64 / jstsp_rate_f64) --------
// sigma_1(S - Zbar) and the values of Zbar on the three routes above, then one thread per trial.  D = S - Zbar is formed in
// float64 from the operands: as it is loaded on the LDS and QR routes (never stored, and the power-of-two scale is found from
// |D|'s own largest component - D may be 1e-9 of Zbar), into the workspace on the third.

// One workgroup per (trial, operand): operand 0 is D, operand 1 is Zbar; LDS and threads as svdvals_kernel.
__global__ __launch_bounds__(64 * SV_WAVES) void score_values_kernel(int rows, int cols, const double2 *S, const double2 *Z, int z_keep,
                                                                     double *svD, double *svZ)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x;
    const bool diff = blockIdx.y == 0, tall = rows >= cols;
    const int m = tall ? rows : cols, n = tall ? cols : rows;
    const double2 *St = S + (size_t)rows * cols * t, *Zt = Z + (size_t)rows * cols * t;
    for (int e = threadIdx.x; e < rows * cols; e += blockDim.x) {
        double2 v = Zt[e];
        if (diff) {
            const double2 s = St[e];
            v = make_double2(s.x - v.x, s.y - v.y);
        }
        if (tall) lds[e] = v;
        else lds[e / rows + m * (e % rows)] = make_double2(v.x, -v.y);
    }
    if (diff) singular_values_block(lds, m, n, 1, svD + t);
    else singular_values_block(lds, m, n, z_keep, svZ + (size_t)z_keep * t);
}

__global__ __launch_bounds__(256) void subtract_kernel(long long cnt, const double2 *S, const double2 *Z, double2 *D)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < cnt; e += (long long)gridDim.x * 256)
        D[e] = make_double2(S[e].x - Z[e].x, S[e].y - Z[e].y);
}

// One thread per trial.  e = (sigma_1(D) / sigma_1(Zbar))^2, the quotient first (plot_errorVSsnr.m:138-141).  NMSE: min(1, e),
// NaN stays NaN.  Rate (plot_rateVSframelength.m:81): log2 det(I + Zbar Zbar^H / (R (noise_var + e))) as the sum over the z_keep = n
// values of Zbar, k ascending, with e not capped.
__global__ __launch_bounds__(256) void score_finish_kernel(int batch, int z_keep, int rate, double R, double noise_var, const double *svD,
                                                           const double *svZ, double *out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= batch) return;
    const double *z = svZ + (size_t)z_keep * t;
    const double q = svD[t] / z[0], e = q * q;
    if (!rate) {
        out[t] = e > 1.0 ? 1.0 : e;
        return;
    }
    const double den = R * (noise_var + e);
    double acc = 0.0;
    for (int k = 0; k < z_keep; ++k) acc += log2(1.0 + z[k] * z[k] / den);
    out[t] = acc;
}

int score_impl(jstsp_ctx *ctx, int rows, int cols, int batch, const double2 *S, const double2 *Z, bool rate, double noise_var, double *res,
               int memspace, const char *what)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "%s: NULL context", what);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "%s: bad memspace", what);
    JSTSP_REQUIRE(S && Z && res, JSTSP_E_NULL, "%s: NULL argument", what);
    JSTSP_REQUIRE(rows > 0 && cols > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", what);
    JSTSP_REQUIRE(!rate || noise_var >= 0.0, JSTSP_E_ARG, "%s: noise_var must be >= 0", what);     // (a NaN fails the comparison)
    JSTSP_REQUIRE(spectrum_shape_ok(rows, cols), JSTSP_E_UNSUPPORTED, "%s: %d x %d: need " SPECTRUM_LIMITS, what, rows, cols);
    const int m = std::max(rows, cols), n = std::min(rows, cols), z_keep = rate ? n : 1;
    const bool host = memspace == JSTSP_HOST, lds = sv_fits(rows, cols), qr = !lds && tq_fits(rows, cols);
    JSTSP_REQUIRE(lds || qr || batch <= 65535, JSTSP_E_UNSUPPORTED, "%s: %d x %d, batch %d: orders above 64 need batch <= 65535", what, rows,
                  cols, batch);
    JSTSP_ENTER(ctx);
    hipStream_t st = ctx->stream;
    const size_t nY = (size_t)rows * cols;
    const double2 *s, *z;
    double2 *D = nullptr;
    double *svD, *svZ, *o;
    Pinv64Arrays pv{};
    Slab w(st);
    JSTSP_TRY(ws64_open(w, what, batch, [&](Slab &a, int b) {
        s = a.in(S, nY * b, host);
        z = a.in(Z, nY * b, host);
        svD = a.get<double>((size_t)b);
        svZ = a.get<double>((size_t)z_keep * b);
        o = a.out(res, (size_t)b, host);
        if (!lds && !qr) {
            D = a.get<double2>(nY * b);
            pv.W = a.get<double2>((size_t)m * n * b); pv.V = a.get<double2>((size_t)n * n * b);
            pv.meta = a.get<PvMeta>(b);
            pv.any = a.get<int>(1);
        }
    }));
    if (lds) {
        const size_t sh = sv_lds_bytes(m, n);
        JSTSP_HIP(hipFuncSetAttribute((const void *)score_values_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        score_values_kernel<<<dim3(batch, 2), sv_threads(n), sh, st>>>(rows, cols, s, z, z_keep, svD, svZ);
        JSTSP_HIP(hipGetLastError());
    } else if (qr) {                                               // tsqr_values_kernel twice: the spectrum entries keep their kernel
        JSTSP_TRY(tsqr_launch(st, DiffLoader<double2>{s, z, rows, cols}, n, batch, 1, svD));
        JSTSP_TRY(tsqr_launch(st, MatrixLoader<double2>{z, rows, cols}, n, batch, z_keep, svZ));
    } else {
        const long long cnt = (long long)nY * batch;
        subtract_kernel<<<grid_for(cnt), 256, 0, st>>>(cnt, s, z, D);
        JSTSP_HIP(hipGetLastError());
        JSTSP_TRY(pinv64_values(st, pv, rows, cols, batch, D, (long long)nY, 1, svD));
        JSTSP_TRY(pinv64_values(st, pv, rows, cols, batch, z, (long long)nY, z_keep, svZ));
    }
    score_finish_kernel<<<(batch + 255) / 256, 256, 0, st>>>(batch, z_keep, rate ? 1 : 0, (double)rows, noise_var, svD, svZ, o);
    JSTSP_HIP(hipGetLastError());
    if (host) {
        JSTSP_TRY(w.copy_back(res, o, (size_t)batch));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

}  // namespace

extern "C" {

int jstsp_nmse_spectral_f64(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c64 *S, const jstsp_c64 *Zbar, double *nmse, int memspace)
{
    return score_impl(ctx, R, C, batch, reinterpret_cast<const double2 *>(S), reinterpret_cast<const double2 *>(Zbar), false, 0.0, nmse,
                      memspace, "nmse_spectral_f64");
}

int jstsp_rate_f64(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c64 *S, const jstsp_c64 *Zbar, double noise_var, double *rate,
                   int memspace)
{
    return score_impl(ctx, R, C, batch, reinterpret_cast<const double2 *>(S), reinterpret_cast<const double2 *>(Zbar), true, noise_var, rate,
                      memspace, "rate_f64");
}

int jstsp_singular_values_c32(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c32 *Y, double *sv, int memspace)
{
    return singular_values_impl(ctx, rows, cols, batch, reinterpret_cast<const float2 *>(Y), sv, memspace, "singular_values_c32");
}

int jstsp_singular_values_c64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *Y, double *sv, int memspace)
{
    return singular_values_impl(ctx, rows, cols, batch, reinterpret_cast<const double2 *>(Y), sv, memspace, "singular_values_c64");
}

int jstsp_rank_trials_c32(jstsp_ctx *ctx, const jstsp_model *mp, uint64_t seed, int sweep_idx, long long trial0, int batch,
                          int n_keep, double *sv, int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "rank_trials: NULL context");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "rank_trials: bad memspace");
    JSTSP_REQUIRE(mp && sv, JSTSP_E_NULL, "rank_trials: NULL argument");
    JSTSP_ENTER(ctx);
    Model m{};
    m.Nt = mp->Nt; m.Nr = mp->Nr; m.L = mp->L; m.Tp = mp->T_prop; m.clusters = mp->clusters; m.rays = mp->rays;
    JSTSP_REQUIRE(m.Nt > 0 && m.Nr > 0 && m.L > 0 && m.Tp > 0 && m.clusters > 0 && m.rays > 0 && batch > 0 && trial0 >= 0 &&
                      sweep_idx >= 0,
                  JSTSP_E_SHAPE, "rank_trials: bad model dimensions");
    JSTSP_REQUIRE(m.L <= m.Tp, JSTSP_E_SHAPE, "rank_trials: L > T_prop");
    JSTSP_REQUIRE(mp->pilots == JSTSP_PILOTS_QAM4 || mp->pilots == JSTSP_PILOTS_GAUSS, JSTSP_E_ARG, "rank_trials: bad pilots kind");
    const int rows = m.Nr, cols = m.Tp, n = std::min(rows, cols), mm = std::max(rows, cols);
    JSTSP_REQUIRE(n_keep >= 1 && n_keep <= n, JSTSP_E_SHAPE, "rank_trials: need 1 <= n_keep <= min(Nr, T_prop)");
    m.Np = m.clusters * m.rays; m.NtL = m.Nt * m.L;
    JSTSP_REQUIRE(sv_fits(rows, cols) && channel_lds_bytes(m) <= 150 * 1024, JSTSP_E_UNSUPPORTED,
                  "rank_trials: need min(Nr, T_prop) <= %d and Nr * T_prop <= %d", SV_NMAX, SV_ELEMS);
    const size_t nS = (size_t)n_keep * batch;
    JSTSP_TRY(ctx->arena.reserve(operands_bytes(m, (size_t)batch) + rnd256(nS * 8) + 4096));
    ctx->arena.reset();
    Operands op;
    JSTSP_TRY(draw_operands(ctx, m, mp, seed, (uint64_t)sweep_idx, trial0, batch, &op));
    double *o = memspace == JSTSP_DEVICE ? sv : ctx->arena.get<double>(nS);
    JSTSP_REQUIRE(o, JSTSP_E_NOMEM, "rank_trials: workspace exhausted");
    const size_t sh = sv_lds_bytes(mm, n);
    JSTSP_HIP(hipFuncSetAttribute((const void *)rank_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    rank_sweep_kernel<<<batch, sv_threads(n), sh, ctx->stream>>>(m, op.Hmat, op.psym, op.pscale, n_keep, o);
    JSTSP_HIP(hipGetLastError());
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(stage_out(ctx, sv, o, nS, memspace));
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

int jstsp_spectrum_c32(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c32 *Y, int n_keep, double *sv, int memspace)
{
    return spectrum_impl(ctx, rows, cols, batch, reinterpret_cast<const float2 *>(Y), n_keep, sv, memspace, "spectrum_c32");
}

int jstsp_spectrum_c64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *Y, int n_keep, double *sv, int memspace)
{
    return spectrum_impl(ctx, rows, cols, batch, reinterpret_cast<const double2 *>(Y), n_keep, sv, memspace, "spectrum_c64");
}

int jstsp_spectrum_trials_c32(jstsp_ctx *ctx, const jstsp_model *mp, uint64_t seed, int sweep_idx, long long trial0, int batch,
                              const jstsp_c32 *Hsrc, int ld_rows, int ld_cols, long long strideH, int normalize, int n_keep, double *sv,
                              double *sigma_max, int memspace)
{
    const char *what = "spectrum_trials";
    if (!Hsrc && ctx && mp && sv && (memspace == JSTSP_HOST || memspace == JSTSP_DEVICE) && mp->T_prop > 0 && mp->Nr > 0 &&
        sv_fits(mp->Nr, mp->T_prop))
        return jstsp_rank_trials_c32(ctx, mp, seed, sweep_idx, trial0, batch, n_keep, sv, memspace);   // the LDS kernel and its bits
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "%s: NULL context", what);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "%s: bad memspace", what);
    JSTSP_REQUIRE(mp && sv, JSTSP_E_NULL, "%s: NULL argument", what);
    JSTSP_ENTER(ctx);
    const bool given = Hsrc != nullptr;
    Model m{};
    m.Nt = mp->Nt; m.Nr = mp->Nr; m.L = mp->L; m.Tp = mp->T_prop; m.clusters = mp->clusters; m.rays = mp->rays;
    if (given) m.clusters = m.rays = 1;             // (ignored: nothing is drawn for the channel)
    JSTSP_REQUIRE(m.Nt > 0 && m.Nr > 0 && m.L > 0 && m.Tp > 0 && m.clusters > 0 && m.rays > 0 && batch > 0 && trial0 >= 0 &&
                      sweep_idx >= 0,
                  JSTSP_E_SHAPE, "%s: bad model dimensions", what);
    JSTSP_REQUIRE(m.L <= m.Tp, JSTSP_E_SHAPE, "%s: L > T_prop", what);
    JSTSP_REQUIRE(mp->pilots == JSTSP_PILOTS_QAM4 || mp->pilots == JSTSP_PILOTS_GAUSS, JSTSP_E_ARG, "%s: bad pilots kind", what);
    const int rows = m.Nr, cols = m.Tp, n = std::min(rows, cols), mm = std::max(rows, cols);
    JSTSP_REQUIRE(n_keep >= 1 && n_keep <= n, JSTSP_E_SHAPE, "%s: need 1 <= n_keep <= min(Nr, T_prop)", what);
    m.Np = m.clusters * m.rays; m.NtL = m.Nt * m.L;
    JSTSP_REQUIRE(spectrum_shape_ok(rows, cols), JSTSP_E_UNSUPPORTED, "%s: Nr x T_prop = %d x %d: need " SPECTRUM_LIMITS, what, rows, cols);
    JSTSP_REQUIRE(given || channel_lds_bytes(m) <= 150 * 1024, JSTSP_E_UNSUPPORTED, "%s: steering tables exceed the LDS", what);
    const bool lds = sv_fits(rows, cols), qr = !lds && tq_fits(rows, cols);
    JSTSP_REQUIRE(lds || qr || batch <= 65535, JSTSP_E_UNSUPPORTED, "%s: orders above 64 need batch <= 65535", what);
    const bool host = memspace == JSTSP_HOST;
    const size_t b = (size_t)batch, nS = (size_t)n_keep * b, nQ = (size_t)m.Nt * m.Tp, nR = (size_t)rows * cols;
    // ---- workspace: the float64 family's limit, with the largest batch that fits -------------------------------------------------
    auto bytes = [&](size_t bb) {
        size_t need = operands_bytes(m, bb) + rnd256((size_t)n_keep * bb * 8) + 4096;
        if (!lds && !qr) need += rnd256(bb * nR * 16) + rnd256(bb * mm * n * 16) + rnd256(bb * n * n * 16) + rnd256(bb * sizeof(PvMeta)) + 256;
        return need;
    };
    if (bytes(b) > WS64_LIMIT) {
        int fit = batch;
        while (fit > 1 && bytes((size_t)fit) > WS64_LIMIT) fit = fit > 64 ? fit - fit / 16 : fit - 1;
        set_error("%s: the workspace would be %.1f GiB (limit 24); the largest batch that fits is about %d", what,
                  (double)bytes(b) / (double)((size_t)1 << 30), fit);
        return JSTSP_E_UNSUPPORTED;
    }
    // ---- channel and pilots ------------------------------------------------------------------------------------------------------
    hipStream_t st = ctx->stream;
    Operands op;
    if (given) {
        const GivenChannel g{reinterpret_cast<const float2 *>(Hsrc), ld_rows, ld_cols, strideH, normalize, sigma_max};
        float2 *Hmat = nullptr;
        JSTSP_TRY(given_channel_hmat(ctx, m.Nr, m.Nt, m.L, trial0, batch, g, memspace, bytes(b), nullptr, &Hmat));
        float2 *psym = ctx->arena.get<float2>(b * nQ);
        uint8_t *qam = ctx->arena.get<uint8_t>(b * nQ);
        JSTSP_REQUIRE(psym && qam, JSTSP_E_NOMEM, "%s: workspace exhausted", what);
        const int gauss = mp->pilots == JSTSP_PILOTS_GAUSS;
        draw_noise_qam_kernel<<<dim3(grid_for((long long)nQ, 1024), batch), 256, 0, st>>>(m, seed, (uint64_t)sweep_idx, trial0, nullptr, qam,
                                                                                          mp->shared_pilots, gauss, psym);
        JSTSP_HIP(hipGetLastError());
        op = Operands{Hmat, psym, gauss ? 0.70710678f : 1.f};
    } else {
        JSTSP_TRY(ctx->arena.reserve(bytes(b)));
        ctx->arena.reset();
        JSTSP_TRY(draw_operands(ctx, m, mp, seed, (uint64_t)sweep_idx, trial0, batch, &op));
    }
    double *o = host ? ctx->arena.get<double>(nS) : sv;
    JSTSP_REQUIRE(o, JSTSP_E_NOMEM, "%s: workspace exhausted", what);
    if (lds) {
        const size_t sh = sv_lds_bytes(mm, n);
        JSTSP_HIP(hipFuncSetAttribute((const void *)rank_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        rank_sweep_kernel<<<batch, sv_threads(n), sh, st>>>(m, op.Hmat, op.psym, op.pscale, n_keep, o);
        JSTSP_HIP(hipGetLastError());
    } else if (qr) {
        JSTSP_TRY(tsqr_launch(st, TrialLoader{m, op.Hmat, op.psym, op.pscale, rows, cols}, n, batch, n_keep, o));
    } else {
        Pinv64Arrays pv{};
        double2 *Y = ctx->arena.get<double2>(b * nR);
        pv.W = ctx->arena.get<double2>(b * mm * n); pv.V = ctx->arena.get<double2>(b * n * n);
        pv.meta = ctx->arena.get<PvMeta>(b);
        pv.any = ctx->arena.get<int>(1);
        JSTSP_REQUIRE(Y && pv.W && pv.V && pv.meta && pv.any, JSTSP_E_NOMEM, "%s: workspace exhausted", what);
        received_kernel<<<dim3(grid_for((long long)nR, 64), batch), 256, 0, st>>>(m, op.Hmat, op.psym, op.pscale, Y);
        JSTSP_HIP(hipGetLastError());
        JSTSP_TRY(pinv64_values(st, pv, rows, cols, batch, Y, (long long)nR, n_keep, o));
    }
    if (host) {
        JSTSP_TRY(stage_out(ctx, sv, o, nS, memspace));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

}  // extern "C"
