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
#include "jacobi64.h"
#include "pinv64.h"

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

int svd_check(jstsp_ctx *ctx, const char *nm, int rows, int cols, int batch, const void *A, const void *out, int keep, const char *keep_name,
              int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_REQUIRE(rows > 0 && cols > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", nm);
    JSTSP_REQUIRE(A && out, JSTSP_E_NULL, "%s: NULL argument", nm);
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    JSTSP_REQUIRE(keep >= 1 && keep <= n, JSTSP_E_ARG, "%s: need 1 <= %s <= min(rows, cols) = %d, got %d", nm, keep_name, n, keep);
    JSTSP_REQUIRE(pinv64_shape_ok(rows, cols), JSTSP_E_UNSUPPORTED, "%s: %d x %d: need min(rows, cols) <= %d and max(rows, cols) <= %d", nm, rows,
                  cols, PV_MAX_ORDER, PV_MAX_LONG);
    JSTSP_REQUIRE(svd_lds_fits(m, n) || batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: %d x %d, batch %d: shapes beyond one workgroup's LDS need batch <= 65535", nm, rows, cols, batch);
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

}  // extern "C"
