// jstsp_svd_f64 / jstsp_lowrank_f64 - [U,S,V] = svd(A,'econ') (plot_rankR.m:49, vamp.m:32) and the best rank-R approximation, in
// float64, batched: the one-sided (Hestenes) Jacobi of svdvals.hip and pinv64.hip with the singular vectors kept.
//
// With W = A (rows >= cols) or A^H, m x n, m >= n, the rotations make the columns of W V orthogonal: W V = Q Sigma.  The
// short-side factor is V, the accumulated rotations (a full set of orthonormal columns whatever the rank); the long-side factor
// is Q = column / norm.  A column of W V whose norm the drop rule of jstsp_pinv_f64 drops (pinv64_drop_tol, pinv64.h) is
// rounding residue that the iteration never orthogonalised: the long-side factor has a ZERO column there.  For rows >= cols
// U = Q and V = V; for rows < cols the operand was A^H = V_A Sigma U_A^H, so the two swap roles on the way out.
//
// Two routes, chosen by the shape alone:
//   LDS: n <= 64 and (m + n) n complex doubles plus scratch within 159 of the 160 KiB (64 x 64, 32 x 140, 128 x 50 ...): svd64_lds_kernel,
//     one workgroup per matrix, one launch, no host read.  Column j of the operand and column j of V are ONE run of m + n
//     consecutive 16-byte elements in LDS: jacobi_sweeps (jacobi64.h) forms the inner products over the first m and rotates all
//     m + n, so the 64 lanes of a pair's wave still read whole 256-byte bank rows.  The epilogue - norms, places, drop rule,
//     factors - runs in the same kernel.  The prescale, the sweeps and the norms are the code of svdvals_kernel with the same
//     workgroup size: sv has the bits of jstsp_singular_values_c64 wherever that entry takes the shape.
//   global: everything else up to 512 x 8192: p64_decompose of pinv64.hip unchanged, then p64_vectors_kernel (pinv64_svd).  Waits
//     for the stream once per sweep; sv has the bits of jstsp_spectrum_c64's third route.
// jstsp_lowrank_f64 multiplies (U_R Sigma_R) V_R^H of the same decomposition on the f64 matrix pipe (zgemm64).
//
// jstsp_svd_tall_f64 / jstsp_lowrank_tall_f64 - the same results for n <= 64 and a long side up to 65536, always by the QR route
// ("QR route"): the chunked Householder reduction of svdvals.hip (tq_reduce, tsqr64.h) with the reflectors
// kept, the same in-LDS Jacobi with vectors on the n x n triangle R = U_R Sigma V^H, and the reflectors applied back to
// [U_R; 0], last chunk first.  See the section further down.
#include "jacobi64.h"
#include "pinv64.h"
#include "tsqr64.h"

using namespace jstsp;

namespace {

constexpr size_t SVD_LDS_LIMIT = 159 * 1024;        // of the CU's 160 KiB: 1 KiB stays free for what the compiler allocates statically (256 bytes today)

// operand and V, the norms, the reduction scratch, the places
inline size_t svd_lds_bytes(int m, int n) { return (size_t)(m + n) * n * sizeof(double2) + (size_t)(n + SV_RED) * sizeof(double) + (size_t)n * sizeof(int); }
inline bool svd_lds_fits(int m, int n) { return n <= SV_NMAX && svd_lds_bytes(m, n) <= SVD_LDS_LIMIT; }

__global__ __launch_bounds__(64 * SV_WAVES) void svd64_lds_kernel(int rows, int cols, const double2 *A, int n_keep, double2 *U, double *sv,
                                                                   double2 *V, int32_t *rank, int32_t *conv)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    const bool tall = rows >= cols;
    const int m = tall ? rows : cols, n = tall ? cols : rows, ld = m + n;
    double *nrm = reinterpret_cast<double *>(lds + (size_t)ld * n), *red = nrm + n;
    int *place = reinterpret_cast<int *>(red + SV_RED);
    const double2 *At = A + (size_t)rows * cols * t;
    double *out = sv + (size_t)n_keep * t;
    double2 *Lt = tall ? U : V, *St = tall ? V : U;               // long side: m x n_keep; short side: n x n_keep
    if (Lt) Lt += (size_t)t * m * n_keep;
    if (St) St += (size_t)t * n * n_keep;
    for (int e = tid; e < rows * cols; e += nt) {
        const double2 v = At[e];
        if (tall) lds[e % m + ld * (e / m)] = v;
        else lds[e / rows + ld * (e % rows)] = make_double2(v.x, -v.y);           // A^H
    }
    for (int e = tid; e < n * n; e += nt) lds[m + e % n + ld * (e / n)] = make_double2(e % n == e / n ? 1.0 : 0.0, 0.0);
    double unscale, fro2;
    if (prescale(lds, m, n, n, red, &unscale, &fro2)) {
        const double q = __builtin_nan("");
        for (int k = tid; k < n_keep; k += nt) out[k] = q;
        if (Lt) for (int e = tid; e < m * n_keep; e += nt) Lt[e] = make_double2(q, q);
        if (St) for (int e = tid; e < n * n_keep; e += nt) St[e] = make_double2(q, q);
        if (tid == 0) {
            if (rank) rank[t] = 0;
            if (conv) conv[t] = 0;
        }
        return;
    }
    const bool done = jacobi_sweeps(lds, m, n, n, fro2);
    column_norms(lds, m, n, n, nrm);
    for (int i = tid; i < n; i += nt) {
        const int pl = norm_place(nrm, n, i);
        place[i] = pl;
        if (pl < n_keep) out[pl] = nrm[i] * unscale;
    }
    if (tid == 0) {
        double smax = 0.0;
        for (int k = 0; k < n; ++k) smax = fmax(smax, nrm[k]);
        const double tol = pinv64_drop_tol(m, smax);
        int kept = 0;
        for (int k = 0; k < n; ++k) kept += nrm[k] > tol;
        red[0] = tol;
        if (rank) rank[t] = kept;
        if (conv) conv[t] = done ? 1 : 0;
    }
    __syncthreads();
    const double tol = red[0];
    if (Lt)
        for (int e = tid; e < m * n; e += nt) {
            const int j = e / m, i = e % m, pl = place[j];
            if (pl >= n_keep) continue;
            const double s = nrm[j];
            const double2 x = lds[i + ld * j];
            Lt[i + (size_t)m * pl] = s > tol ? make_double2(x.x / s, x.y / s) : make_double2(0.0, 0.0);
        }
    if (St)
        for (int e = tid; e < n * n; e += nt) {
            const int j = e / n, i = e % n, pl = place[j];
            if (pl < n_keep) St[i + (size_t)n * pl] = lds[m + i + ld * j];
        }
}

// US(:, k, t) = U(:, k, t) sv(k, t), k < R, in place; U: rows x nk per matrix, sv: nk per matrix
__global__ __launch_bounds__(256) void svd64_scale_kernel(int rows, int nk, int R, double2 *U, const double *sv)
{
    const int t = blockIdx.y;
    double2 *Ut = U + (size_t)t * rows * nk;
    const double *s = sv + (size_t)t * nk;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < rows * R; e += gridDim.x * 256) {
        const double f = s[e / rows];
        Ut[e] = make_double2(Ut[e].x * f, Ut[e].y * f);
    }
}

// tail[t] = sigma_{R+1} of matrix t, 0 when there is none
__global__ __launch_bounds__(256) void svd64_tail_kernel(int batch, int nk, int R, const double *sv, double *tail)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < batch) tail[t] = nk > R ? sv[R + (size_t)nk * t] : 0.0;
}

// the workspace of the global route (w.Vs and w.ws stay unused)
void svd_layout(Slab &w, Pinv64Arrays &pv, int m, int n, int b)
{
    pv.W = w.get<double2>((size_t)m * n * b); pv.V = w.get<double2>((size_t)n * n * b);
    pv.meta = w.get<PvMeta>(b);
    pv.any = w.get<int>(1);
}

// every array on the device; U, V, rank, conv: nullptr = not wanted
int svd_run(hipStream_t st, const Pinv64Arrays &pv, int rows, int cols, int batch, const double2 *A, int n_keep, double2 *U, double *sv, double2 *V,
            int32_t *rank, int32_t *conv)
{
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    if (!svd_lds_fits(m, n)) return pinv64_svd(st, pv, rows, cols, batch, A, (long long)rows * cols, n_keep, U, sv, V, rank, conv);
    const size_t sh = svd_lds_bytes(m, n);
    JSTSP_HIP(hipFuncSetAttribute((const void *)svd64_lds_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    svd64_lds_kernel<<<batch, sv_threads(n), sh, st>>>(rows, cols, A, n_keep, U, sv, V, rank, conv);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

// what every entry of this file asks of its arguments before it looks at the shape limits of its route
int svd_check_args(jstsp_ctx *ctx, const char *nm, int rows, int cols, int batch, const void *A, const void *out, int keep,
                   const char *keep_name, int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_REQUIRE(rows > 0 && cols > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", nm);
    JSTSP_REQUIRE(A && out, JSTSP_E_NULL, "%s: NULL argument", nm);
    const int n = std::min(rows, cols);
    JSTSP_REQUIRE(keep >= 1 && keep <= n, JSTSP_E_ARG, "%s: need 1 <= %s <= min(rows, cols) = %d, got %d", nm, keep_name, n, keep);
    return 0;
}

int svd_check(jstsp_ctx *ctx, const char *nm, int rows, int cols, int batch, const void *A, const void *out, int keep, const char *keep_name,
              int memspace)
{
    JSTSP_TRY(svd_check_args(ctx, nm, rows, cols, batch, A, out, keep, keep_name, memspace));
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    JSTSP_REQUIRE(pinv64_shape_ok(rows, cols), JSTSP_E_UNSUPPORTED, "%s: %d x %d: need min(rows, cols) <= %d and max(rows, cols) <= %d", nm, rows,
                  cols, PV_MAX_ORDER, PV_MAX_LONG);
    JSTSP_REQUIRE(svd_lds_fits(m, n) || batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: %d x %d, batch %d: shapes beyond one workgroup's LDS need batch <= 65535", nm, rows, cols, batch);
    return 0;
}

// ---- the QR route: vectors for n <= 64 and a long side up to 65536 ------------------------------------------------------------------
// With W = A (rows >= cols) or A^H, m x n, scaled by a power of two: [0; W] = Q [R; 0], Q the product of the reflectors of
// tq_reduce, one per (chunk, column).  R = U_R Sigma V^H by the Jacobi with vectors, so W = (Q [U_R; 0])(rows n ..) Sigma V^H:
//   forward  (svd64_tall_forward_kernel, one workgroup per matrix): the reduction of tsqr_values_kernel, chunk after chunk; after
//     tq_reduce the chunk buffer holds the reflector tails y_j, which go to Y in the operand's place, and tq_reduce<true> leaves
//     u_1 and 1 / (|x| (|x| + |alpha|)) of every reflector in refl.  Then, in the same launch, the Jacobi on R with V under it
//     (the layout of svd64_lds_kernel), the values, the drop rule with the long side m of the OPERAND, the short-side factor,
//     and T = U_R(:, :n_keep) with the dropped columns zero.
//   backward (svd64_tall_backward_kernel, one workgroup per matrix): the chunks from last to first; per chunk W = 0 (cc x n_keep)
//     and for j = n - 1 .. 0, every column q:  d = conj(u_1) T(j, q) + y_j^H W(:, q),  f = d / (|x| (|x| + |alpha|)),
//     T(j, q) -= u_1 f,  W(:, q) -= y_j f.  W is then the finished block of rows of the long-side factor.  One wave per output
//     column (four at a time): column q of T lives in the registers of its wave (lane j holds T(j, q)), W in two complex doubles
//     per lane and column, so LDS holds the tails of one chunk only; no wave waits for another within a chunk.
//   correction (svd64_tall_correct_kernel): in exact arithmetic the top block T ends as zero.  In floating point it ends as
//     E = (rounding of the reduction) V / sigma_k, of size eps sigma_1 / sigma_k in column k, and the rows below it lack exactly
//     that: L^H L = I - E^H E.  For sigma_k / sigma_1 < 1e-8 that is above rounding level (8e-10 on values graded over 12
//     decades).  The backward kernel therefore leaves G = E^H E / 2 (n_keep x n_keep), and L <- L (I + G) restores
//     L^H L = I to O(|G|^2), 64 rows per workgroup.  A zero column of T gives a zero row and column of G: it stays zero.
// The three launches read nothing on the host; no atomics, every sum in a fixed order.
constexpr int TB_Q = 4;         // output columns a wave carries through a chunk at a time
constexpr int TB_G = 2;         // such groups per wave: 8 waves x 2 x 4 = 64 columns
constexpr int TC_ROWS = 64;     // rows of the long-side factor per workgroup of the correction
static_assert(TB_Q * TB_G * (TQ_THREADS / 64) >= TQ_NMAX, "every output column needs a wave");
static_assert(TQ_PRE * TQ_THREADS >= 128 * 48 && TQ_PRE * TQ_THREADS >= 64 * 64, "a chunk has to fit the prefetch registers");
static_assert(3 * TQ_NMAX <= TQ_THREADS, "one thread per reflector scalar");

struct TallArrays {
    double2 *Y;         // m x n per matrix: the reflector tails, rows i0 .. i0 + cc of column j at i0 + m j
    double *refl;       // 3 n per (matrix, chunk): u_1.re, u_1.im, 1 / (|x| (|x| + |alpha|)) (0: no reflector) of column j at 3 j
    double2 *T;         // n x n_keep per matrix: the leading left vectors of R, dropped columns zero
    double2 *G;         // n_keep x n_keep per matrix: half the Gram matrix of what the back-application left in T
    int *bad;           // per matrix: a non-finite entry
};

__host__ __device__ inline int tall_chunks(int m, int n) { return (m + tq_chunk(n) - 1) / tq_chunk(n); }

void tall_layout(Slab &w, TallArrays &ta, int m, int n, int nk, int b)
{
    ta.Y = w.get<double2>((size_t)m * n * b);
    ta.refl = w.get<double>((size_t)3 * n * tall_chunks(m, n) * b);
    ta.T = w.get<double2>((size_t)n * nk * b); ta.G = w.get<double2>((size_t)nk * nk * b);
    ta.bad = w.get<int>(b);
}

// R and the chunk (the Jacobi's operand and V afterwards: 2 n n <= n n + C n), the norms, the reduction scratch, the places
inline size_t tall_fwd_lds(int n) { return std::max<size_t>(1024, tq_lds_bytes(n) + (size_t)(n + SV_RED) * sizeof(double) + (size_t)n * sizeof(int)); }
inline size_t tall_bwd_lds(int n) { return (size_t)tq_chunk(n) * n * sizeof(double2) + (size_t)3 * n * sizeof(double); }
inline size_t tall_cor_lds(int nk) { return ((size_t)nk * nk + (size_t)TC_ROWS * nk) * sizeof(double2); }

// S: the short-side factor, n x n_keep per matrix, or nullptr
__global__ __launch_bounds__(TQ_THREADS) void svd64_tall_forward_kernel(int rows, int cols, const double2 *A, int n_keep, TallArrays ws, double *sv,
                                                                         double2 *S, int32_t *rank, int32_t *conv)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x, tid = threadIdx.x;
    MatrixLoader<double2> ld{A, rows, cols};
    ld.bind(t);
    const bool tall = rows >= cols;
    const int m = tall ? rows : cols, n = tall ? cols : rows, C = tq_chunk(n), ld2n = 2 * n;
    double2 *R = lds, *Ck = lds + (size_t)n * n;
    double *scr = reinterpret_cast<double *>(Ck);
    double *nrm = reinterpret_cast<double *>(Ck + (size_t)C * n), *red = nrm + n;
    int *place = reinterpret_cast<int *>(red + SV_RED);
    double2 *Yt = ws.Y + (size_t)t * m * n, *Tt = ws.T + (size_t)t * n * n_keep;
    double *rf = ws.refl + (size_t)t * 3 * n * tall_chunks(m, n), *out = sv + (size_t)n_keep * t;
    if (S) S += (size_t)t * n * n_keep;
    int ex = 0;
    bool bad = ld.scan(scr, &ex);
    double unscale = 1.0, fro2 = 0.0;
    if (!bad) {
        const double sc = ldexp(1.0, -ex);
        for (int e = tid; e < n * n; e += TQ_THREADS) R[e] = make_double2(0.0, 0.0);
        double2 pre[TQ_PRE];                                       // (the fetch order of tsqr_values_kernel)
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
            __syncthreads();                                       // the tails of the chunk before this one are stored
#pragma unroll
            for (int q = 0; q < TQ_PRE; ++q) {
                const int e = tid + q * TQ_THREADS;
                if (e < cc * n) Ck[tall ? e % cc + C * (e / cc) : e / n + C * (e % n)] = pre[q];
            }
            __syncthreads();
            if (i0 + C < m) fetch(i0 + C);
            tq_reduce<true>(R, Ck, n, C, cc, rf + (size_t)3 * n * (i0 / C));
            // every column was last written before a barrier of tq_reduce
            for (int e = tid; e < cc * n; e += TQ_THREADS) Yt[i0 + e % cc + (size_t)m * (e / cc)] = Ck[e % cc + C * (e / cc)];
        }
        // R (ld n) -> column j of R followed by column j of V = I (ld 2 n), through registers: the two layouts overlap
        __syncthreads();
        double2 tmp[(TQ_NMAX * TQ_NMAX + TQ_THREADS - 1) / TQ_THREADS];
#pragma unroll
        for (int q = 0; q < (TQ_NMAX * TQ_NMAX + TQ_THREADS - 1) / TQ_THREADS; ++q) {
            const int e = tid + q * TQ_THREADS;
            tmp[q] = e < n * n ? R[e] : make_double2(0.0, 0.0);
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < (TQ_NMAX * TQ_NMAX + TQ_THREADS - 1) / TQ_THREADS; ++q) {
            const int e = tid + q * TQ_THREADS;
            if (e < n * n) {
                lds[e % n + ld2n * (e / n)] = tmp[q];
                lds[n + e % n + ld2n * (e / n)] = make_double2(e % n == e / n ? 1.0 : 0.0, 0.0);
            }
        }
        bad = prescale(lds, n, n, n, red, &unscale, &fro2);
    }
    if (bad) {
        const double q = __builtin_nan("");
        for (int k = tid; k < n_keep; k += TQ_THREADS) out[k] = q;
        if (S) for (int e = tid; e < n * n_keep; e += TQ_THREADS) S[e] = make_double2(q, q);
        if (tid == 0) {
            ws.bad[t] = 1;                                         // the long-side factor: svd64_tall_backward_kernel
            if (rank) rank[t] = 0;
            if (conv) conv[t] = 0;
        }
        return;
    }
    const bool done = jacobi_sweeps(lds, n, n, n, fro2);
    column_norms(lds, n, n, n, nrm);
    const double back = ldexp(1.0, ex);
    for (int i = tid; i < n; i += TQ_THREADS) {
        const int pl = norm_place(nrm, n, i);
        place[i] = pl;
        if (pl < n_keep) out[pl] = nrm[i] * unscale * back;        // (both powers of two)
    }
    if (tid == 0) {
        double smax = 0.0;
        for (int k = 0; k < n; ++k) smax = fmax(smax, nrm[k]);
        const double tol = pinv64_drop_tol(m, smax);               // the long side of the operand, not of R
        int kept = 0;
        for (int k = 0; k < n; ++k) kept += nrm[k] > tol;
        red[0] = tol;
        ws.bad[t] = 0;
        if (rank) rank[t] = kept;
        if (conv) conv[t] = done ? 1 : 0;
    }
    __syncthreads();
    const double tol = red[0];
    for (int e = tid; e < n * n; e += TQ_THREADS) {
        const int j = e / n, i = e % n, pl = place[j];
        if (pl >= n_keep) continue;
        const double s = nrm[j];
        const double2 x = lds[i + ld2n * j];
        Tt[i + n * pl] = s > tol ? make_double2(x.x / s, x.y / s) : make_double2(0.0, 0.0);
        if (S) S[i + n * pl] = lds[n + i + ld2n * j];
    }
}

// L: the long-side factor, m x n_keep per matrix
__global__ __launch_bounds__(TQ_THREADS) void svd64_tall_backward_kernel(int m, int n, int n_keep, TallArrays ws, double2 *L)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int C = tq_chunk(n), nch = tall_chunks(m, n);
    double2 *Ck = lds;
    double *rfl = reinterpret_cast<double *>(lds + (size_t)C * n);
    const double2 *Yt = ws.Y + (size_t)t * m * n, *Tt = ws.T + (size_t)t * n * n_keep;
    const double *rf = ws.refl + (size_t)t * 3 * n * nch;
    double2 *Lt = L + (size_t)t * m * n_keep, *Gt = ws.G + (size_t)t * n_keep * n_keep;
    if (ws.bad[t]) {
        const double q = __builtin_nan("");
        for (size_t e = tid; e < (size_t)m * n_keep; e += TQ_THREADS) Lt[e] = make_double2(q, q);
        return;
    }
    // group g of wave w: the columns TB_Q (w + 8 g) .. + TB_Q; lane j holds T(j, q)
    double2 Tq[TB_G][TB_Q];
#pragma unroll
    for (int g = 0; g < TB_G; ++g)
#pragma unroll
        for (int qq = 0; qq < TB_Q; ++qq) {
            const int q = TB_Q * (w + (TQ_THREADS / 64) * g) + qq;
            Tq[g][qq] = q < n_keep && lane < n ? Tt[lane + n * q] : make_double2(0.0, 0.0);
        }
    double2 pre[TQ_PRE];
    double prf = 0.0;
    auto fetch = [&](int c) {
        const int i0 = c * C, cc = min(C, m - i0);
#pragma unroll
        for (int q = 0; q < TQ_PRE; ++q) {
            const int e = tid + q * TQ_THREADS;
            pre[q] = e < cc * n ? Yt[i0 + e % cc + (size_t)m * (e / cc)] : make_double2(0.0, 0.0);
        }
        if (tid < 3 * n) prf = rf[(size_t)3 * n * c + tid];
    };
    fetch(nch - 1);
    for (int c = nch - 1; c >= 0; --c) {
        const int i0 = c * C, cc = min(C, m - i0);
        __syncthreads();                                           // the chunk after this one is applied
#pragma unroll
        for (int q = 0; q < TQ_PRE; ++q) {
            const int e = tid + q * TQ_THREADS;
            if (e < cc * n) Ck[e % cc + C * (e / cc)] = pre[q];
        }
        if (tid < 3 * n) rfl[tid] = prf;
        __syncthreads();
        if (c > 0) fetch(c - 1);
        const bool r0 = lane < cc, r1 = lane + 64 < cc;
#pragma unroll
        for (int g = 0; g < TB_G; ++g) {
            const int q0 = TB_Q * (w + (TQ_THREADS / 64) * g);
            if (q0 >= n_keep) continue;
            double2 W0[TB_Q], W1[TB_Q];                            // rows lane and lane + 64 of the chunk
#pragma unroll
            for (int qq = 0; qq < TB_Q; ++qq) W0[qq] = W1[qq] = make_double2(0.0, 0.0);
            for (int j = n - 1; j >= 0; --j) {
                const double inv = rfl[3 * j + 2];
                if (inv == 0.0) continue;                          // no reflector (the same in every lane)
                const double u0x = rfl[3 * j], u0y = rfl[3 * j + 1];
                const double2 y0 = r0 ? Ck[lane + C * j] : make_double2(0.0, 0.0), y1 = r1 ? Ck[lane + 64 + C * j] : make_double2(0.0, 0.0);
                double dr[TB_Q], di[TB_Q];
#pragma unroll
                for (int qq = 0; qq < TB_Q; ++qq) {
                    dr[qq] = y0.x * W0[qq].x + y0.y * W0[qq].y;    // conj(y) W
                    di[qq] = y0.x * W0[qq].y - y0.y * W0[qq].x;
                    dr[qq] += y1.x * W1[qq].x + y1.y * W1[qq].y;
                    di[qq] += y1.x * W1[qq].y - y1.y * W1[qq].x;
                }
#pragma unroll
                for (int qq = 0; qq < TB_Q; ++qq) {
                    dr[qq] = wave_sum(dr[qq]);
                    di[qq] = wave_sum(di[qq]);
                }
#pragma unroll
                for (int qq = 0; qq < TB_Q; ++qq) {
                    const double tx = __shfl(Tq[g][qq].x, j), ty = __shfl(Tq[g][qq].y, j);
                    const double er = dr[qq] + (u0x * tx + u0y * ty), ei = di[qq] + (u0x * ty - u0y * tx);      // + conj(u_1) T(j, q)
                    const double fr = er * inv, fi = ei * inv;
                    if (lane == j) Tq[g][qq] = make_double2(tx - (u0x * fr - u0y * fi), ty - (u0x * fi + u0y * fr));
                    W0[qq] = make_double2(W0[qq].x - (y0.x * fr - y0.y * fi), W0[qq].y - (y0.x * fi + y0.y * fr));
                    W1[qq] = make_double2(W1[qq].x - (y1.x * fr - y1.y * fi), W1[qq].y - (y1.x * fi + y1.y * fr));
                }
            }
#pragma unroll
            for (int qq = 0; qq < TB_Q; ++qq) {
                if (q0 + qq >= n_keep) continue;
                if (r0) Lt[i0 + lane + (size_t)m * (q0 + qq)] = W0[qq];
                if (r1) Lt[i0 + lane + 64 + (size_t)m * (q0 + qq)] = W1[qq];
            }
        }
    }
    // what is left in T (zero in exact arithmetic): G = T^H T / 2 for svd64_tall_correct_kernel
    __syncthreads();
#pragma unroll
    for (int g = 0; g < TB_G; ++g)
#pragma unroll
        for (int qq = 0; qq < TB_Q; ++qq) {
            const int q = TB_Q * (w + (TQ_THREADS / 64) * g) + qq;
            if (q < n_keep && lane < n) Ck[lane + n * q] = Tq[g][qq];
        }
    __syncthreads();
    for (int e = tid; e < n_keep * n_keep; e += TQ_THREADS) {
        const double2 *a = Ck + n * (e % n_keep), *b = Ck + n * (e / n_keep);
        double gr = 0.0, gi = 0.0;
        for (int j = 0; j < n; ++j) {
            gr += a[j].x * b[j].x + a[j].y * b[j].y;               // conj(a) b
            gi += a[j].x * b[j].y - a[j].y * b[j].x;
        }
        Gt[e] = make_double2(0.5 * gr, 0.5 * gi);
    }
}

// L(i0 .. i0 + TC_ROWS, :) <- L(i0 .., :) (I + G), in place: a workgroup holds its rows and G in LDS
__global__ __launch_bounds__(256) void svd64_tall_correct_kernel(int m, int n_keep, int nblk, TallArrays ws, double2 *L)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x / nblk, i0 = (blockIdx.x % nblk) * TC_ROWS, tid = threadIdx.x, rows = min(TC_ROWS, m - i0);
    if (ws.bad[t]) return;                                         // (NaN already)
    double2 *Gh = lds, *tile = lds + (size_t)n_keep * n_keep;
    const double2 *Gt = ws.G + (size_t)t * n_keep * n_keep;
    double2 *Lt = L + (size_t)t * m * n_keep;
    for (int e = tid; e < n_keep * n_keep; e += 256) Gh[e] = Gt[e];
    for (int e = tid; e < TC_ROWS * n_keep; e += 256) {
        const int i = e % TC_ROWS, q = e / TC_ROWS;
        tile[e] = i < rows ? Lt[i0 + i + (size_t)m * q] : make_double2(0.0, 0.0);
    }
    __syncthreads();
    for (int e = tid; e < TC_ROWS * n_keep; e += 256) {
        const int i = e % TC_ROWS, q = e / TC_ROWS;
        if (i >= rows) continue;
        double2 acc = tile[e];
        for (int k = 0; k < n_keep; ++k) {
            const double2 a = tile[i + TC_ROWS * k], g = Gh[k + n_keep * q];
            acc.x += a.x * g.x - a.y * g.y;
            acc.y += a.x * g.y + a.y * g.x;
        }
        Lt[i0 + i + (size_t)m * q] = acc;
    }
}

// every array on the device; U, V, rank, conv: nullptr = not wanted
int tall_run(hipStream_t st, const TallArrays &ta, int rows, int cols, int batch, const double2 *A, int n_keep, double2 *U, double *sv, double2 *V,
             int32_t *rank, int32_t *conv)
{
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    double2 *L = rows >= cols ? U : V, *S = rows >= cols ? V : U;
    JSTSP_HIP(hipFuncSetAttribute((const void *)svd64_tall_forward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tall_fwd_lds(n)));
    svd64_tall_forward_kernel<<<batch, TQ_THREADS, tall_fwd_lds(n), st>>>(rows, cols, A, n_keep, ta, sv, S, rank, conv);
    JSTSP_HIP(hipGetLastError());
    if (!L) return 0;
    JSTSP_HIP(hipFuncSetAttribute((const void *)svd64_tall_backward_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tall_bwd_lds(n)));
    svd64_tall_backward_kernel<<<batch, TQ_THREADS, tall_bwd_lds(n), st>>>(m, n, n_keep, ta, L);
    JSTSP_HIP(hipGetLastError());
    const int nblk = (m + TC_ROWS - 1) / TC_ROWS;       // (nblk * batch < 2^31 wherever Y, 16 m n batch bytes, is within the 24 GiB)
    JSTSP_HIP(hipFuncSetAttribute((const void *)svd64_tall_correct_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)tall_cor_lds(n_keep)));
    svd64_tall_correct_kernel<<<(unsigned)((long long)nblk * batch), 256, tall_cor_lds(n_keep), st>>>(m, n_keep, nblk, ta, L);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

int tall_check(jstsp_ctx *ctx, const char *nm, int rows, int cols, int batch, const void *A, const void *out, int keep, const char *keep_name,
               int memspace)
{
    JSTSP_TRY(svd_check_args(ctx, nm, rows, cols, batch, A, out, keep, keep_name, memspace));
    JSTSP_REQUIRE(tq_fits(rows, cols), JSTSP_E_UNSUPPORTED, "%s: %d x %d: need min(rows, cols) <= %d and max(rows, cols) <= %d", nm, rows, cols,
                  TQ_NMAX, TQ_MMAX);
    return 0;
}
}  // namespace

extern "C" {

int jstsp_svd_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A_, int n_keep, jstsp_c64 *U_, double *sv_, jstsp_c64 *V_,
                  int32_t *rank_out, int32_t *conv_out, int memspace)
{
    const char *nm = "svd (float64)";
    JSTSP_TRY(svd_check(ctx, nm, rows, cols, batch, A_, sv_, n_keep, "n_keep", memspace));
    JSTSP_ENTER(ctx);
    const bool host = memspace == JSTSP_HOST;
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    const bool lds = svd_lds_fits(m, n);
    hipStream_t st = ctx->stream;
    const double2 *A;
    double2 *U = nullptr, *V = nullptr;
    double *sv;
    int32_t *rk = nullptr, *cv = nullptr;
    Pinv64Arrays pv{};
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nm, batch, [&](Slab &w, int b) {
        A = w.in(reinterpret_cast<const double2 *>(A_), (size_t)rows * cols * b, host);
        if (U_) U = w.out(reinterpret_cast<double2 *>(U_), (size_t)rows * n_keep * b, host);
        sv = w.out(sv_, (size_t)n_keep * b, host);
        if (V_) V = w.out(reinterpret_cast<double2 *>(V_), (size_t)cols * n_keep * b, host);
        if (rank_out) rk = w.out(rank_out, b, host);
        if (conv_out) cv = w.out(conv_out, b, host);
        if (!lds) svd_layout(w, pv, m, n, b);
    }));
    JSTSP_TRY(svd_run(st, pv, rows, cols, batch, A, n_keep, U, sv, V, rk, cv));
    if (host) {
        if (U_) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(U_), U, (size_t)rows * n_keep * batch));
        JSTSP_TRY(s.copy_back(sv_, sv, (size_t)n_keep * batch));
        if (V_) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(V_), V, (size_t)cols * n_keep * batch));
        if (rank_out) JSTSP_TRY(s.copy_back(rank_out, rk, batch));
        if (conv_out) JSTSP_TRY(s.copy_back(conv_out, cv, batch));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

int jstsp_lowrank_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A_, int R, jstsp_c64 *X_, double *tail_out, int memspace)
{
    const char *nm = "lowrank (float64)";
    JSTSP_TRY(svd_check(ctx, nm, rows, cols, batch, A_, X_, R, "R", memspace));
    JSTSP_ENTER(ctx);
    const bool host = memspace == JSTSP_HOST;
    const int m = std::max(rows, cols), n = std::min(rows, cols), nk = std::min(R + 1, n);      // sigma_{R+1} is the tail
    const bool lds = svd_lds_fits(m, n);
    hipStream_t st = ctx->stream;
    const double2 *A;
    double2 *U, *V, *X, *gws;
    double *sv, *tail = nullptr;
    Pinv64Arrays pv{};
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nm, batch, [&](Slab &w, int b) {
        A = w.in(reinterpret_cast<const double2 *>(A_), (size_t)rows * cols * b, host);
        X = w.out(reinterpret_cast<double2 *>(X_), (size_t)rows * cols * b, host);
        if (tail_out) tail = w.out(tail_out, b, host);
        U = w.get<double2>((size_t)rows * nk * b); V = w.get<double2>((size_t)cols * nk * b);
        sv = w.get<double>((size_t)nk * b);
        gws = w.get<double2>(std::max<size_t>(1, zgemm64_ws_elems(rows, cols, R, b)));
        if (!lds) svd_layout(w, pv, m, n, b);
    }));
    JSTSP_TRY(svd_run(st, pv, rows, cols, batch, A, nk, U, sv, V, nullptr, nullptr));
    svd64_scale_kernel<<<dim3((unsigned)std::min<size_t>(((size_t)rows * R + 255) / 256, 1024), batch), 256, 0, st>>>(rows, nk, R, U, sv);
    JSTSP_HIP(hipGetLastError());
    // X = (U_R Sigma_R) V_R^H; a column the drop rule dropped is zero in the long-side factor, so the sum ends at min(R, rank)
    JSTSP_TRY(zgemm64(st, 'N', 'C', rows, cols, R, batch, Mat64{U, (long long)rows * nk, rows}, Mat64{V, (long long)cols * nk, cols}, X,
                      (long long)rows * cols, rows, gws));
    if (tail_out) {
        svd64_tail_kernel<<<(batch + 255) / 256, 256, 0, st>>>(batch, nk, R, sv, tail);
        JSTSP_HIP(hipGetLastError());
    }
    if (host) {
        JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(X_), X, (size_t)rows * cols * batch));
        if (tail_out) JSTSP_TRY(s.copy_back(tail_out, tail, batch));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

int jstsp_svd_tall_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A_, int n_keep, jstsp_c64 *U_, double *sv_, jstsp_c64 *V_,
                       int32_t *rank_out, int32_t *conv_out, int memspace)
{
    const char *nm = "svd_tall (float64)";
    JSTSP_TRY(tall_check(ctx, nm, rows, cols, batch, A_, sv_, n_keep, "n_keep", memspace));
    JSTSP_ENTER(ctx);
    const bool host = memspace == JSTSP_HOST;
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    hipStream_t st = ctx->stream;
    const double2 *A;
    double2 *U = nullptr, *V = nullptr;
    double *sv;
    int32_t *rk = nullptr, *cv = nullptr;
    TallArrays ta{};
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nm, batch, [&](Slab &w, int b) {
        A = w.in(reinterpret_cast<const double2 *>(A_), (size_t)rows * cols * b, host);
        if (U_) U = w.out(reinterpret_cast<double2 *>(U_), (size_t)rows * n_keep * b, host);
        sv = w.out(sv_, (size_t)n_keep * b, host);
        if (V_) V = w.out(reinterpret_cast<double2 *>(V_), (size_t)cols * n_keep * b, host);
        if (rank_out) rk = w.out(rank_out, b, host);
        if (conv_out) cv = w.out(conv_out, b, host);
        tall_layout(w, ta, m, n, n_keep, b);
    }));
    JSTSP_TRY(tall_run(st, ta, rows, cols, batch, A, n_keep, U, sv, V, rk, cv));
    if (host) {
        if (U_) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(U_), U, (size_t)rows * n_keep * batch));
        JSTSP_TRY(s.copy_back(sv_, sv, (size_t)n_keep * batch));
        if (V_) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(V_), V, (size_t)cols * n_keep * batch));
        if (rank_out) JSTSP_TRY(s.copy_back(rank_out, rk, batch));
        if (conv_out) JSTSP_TRY(s.copy_back(conv_out, cv, batch));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

int jstsp_lowrank_tall_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A_, int R, jstsp_c64 *X_, double *tail_out, int memspace)
{
    const char *nm = "lowrank_tall (float64)";
    JSTSP_TRY(tall_check(ctx, nm, rows, cols, batch, A_, X_, R, "R", memspace));
    JSTSP_REQUIRE(batch <= 65535, JSTSP_E_UNSUPPORTED, "%s: batch %d: the product needs batch <= 65535", nm, batch);
    JSTSP_ENTER(ctx);
    const bool host = memspace == JSTSP_HOST;
    const int m = std::max(rows, cols), n = std::min(rows, cols), nk = std::min(R + 1, n);      // sigma_{R+1} is the tail
    hipStream_t st = ctx->stream;
    const double2 *A;
    double2 *U, *V, *X, *gws;
    double *sv, *tail = nullptr;
    TallArrays ta{};
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nm, batch, [&](Slab &w, int b) {
        A = w.in(reinterpret_cast<const double2 *>(A_), (size_t)rows * cols * b, host);
        X = w.out(reinterpret_cast<double2 *>(X_), (size_t)rows * cols * b, host);
        if (tail_out) tail = w.out(tail_out, b, host);
        U = w.get<double2>((size_t)rows * nk * b); V = w.get<double2>((size_t)cols * nk * b);
        sv = w.get<double>((size_t)nk * b);
        gws = w.get<double2>(std::max<size_t>(1, zgemm64_ws_elems(rows, cols, R, b)));      // (R <= 64: the product is not cut along k)
        tall_layout(w, ta, m, n, nk, b);
    }));
    JSTSP_TRY(tall_run(st, ta, rows, cols, batch, A, nk, U, sv, V, nullptr, nullptr));
    svd64_scale_kernel<<<dim3((unsigned)std::min<size_t>(((size_t)rows * R + 255) / 256, 1024), batch), 256, 0, st>>>(rows, nk, R, U, sv);
    JSTSP_HIP(hipGetLastError());
    JSTSP_TRY(zgemm64(st, 'N', 'C', rows, cols, R, batch, Mat64{U, (long long)rows * nk, rows}, Mat64{V, (long long)cols * nk, cols}, X,
                      (long long)rows * cols, rows, gws));
    if (tail_out) {
        svd64_tail_kernel<<<(batch + 255) / 256, 256, 0, st>>>(batch, nk, R, sv, tail);
        JSTSP_HIP(hipGetLastError());
    }
    if (host) {
        JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(X_), X, (size_t)rows * cols * batch));
        if (tail_out) JSTSP_TRY(s.copy_back(tail_out, tail, batch));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

}  // extern "C"
