// jstsp_refit_f64 - a float64 least-squares re-fit of an estimate on its support (include/jstsp.h): a stage
// AFTER the ADMM of proposed64.hip, which returns an S that is not the least-squares fit on its own strong entries (one steepest-
// descent step per iteration, proposed_algorithm.m:47-51).  Per trial, with g = Gr G2, T the support (the first K entries of
// indx_S, or of jstsp_support_order_f64(S_in) by the selection kernel of support_top.h) and m its indicator:
//   G(x) = m .* (A^H ((Omega .* Omega) .* (A x B)) B^H) + lam x        the normal operator of min ||Omega .* (A x B) - subY||_F on T
//   b    = m .* (A^H (Omega .* subY) B^H)
//   x = m .* S_in;  r = b - G(x);  p = r;  gamma = <r, r>;  for k = 1 .. iters:
//       q = G(p);  delta = Re<p, q>;  alpha = gamma / delta;  x += alpha p;  r -= alpha q;  gamma' = <r, r>;
//       p = r + (gamma' / gamma) p;  gamma = gamma'
// conjugate gradients from the given estimate.  A trial FREEZES at the first k at whose start gamma == 0 or gamma <= tol^2 gamma_0
// (tol > 0), or whose delta is not positive and finite: its x stays, its steps stay k - 1.  The flag, gamma, gamma_0 and the step
// count live on the device and nothing is read back inside the loop.
// Launches: the two products of b and the four of G(x) once, four products per step (zgemm64.hip, f64 MFMA), an element-wise kernel
// between the two halves of an operator, and ONE workgroup per trial for the step - shaped like step_v64_kernel of proposed64.hip:
// delta, then x and r with gamma', then p, the mask applied on every write, every sum in a fixed order (no atomics in a sum).  The
// arrays stay dense Gr x G2 with exact zeros off T.  A trial's bits depend on its own data alone: not on the batch, not on a
// shared or per-trial dictionary (the splits of zgemm64 are a function of the shape), not on the memspace.
#include "support_top.h"
#include "ws64.h"
#include "zgemm64.h"

#include <algorithm>
#include <climits>
#include <cmath>

namespace jstsp {
namespace {

inline dim3 rf_grid(long long per, int batch) { return dim3((unsigned)std::max<long long>(1, std::min<long long>((per + 255) / 256, 2048)), batch); }

// rank[e] = position of entry e (0-based) among the first cnt entries of indx_S (1-based linear indices, n per trial); an index
// outside 1 .. g is ignored
__global__ __launch_bounds__(256) void refit_rank_init_kernel(long long n, int32_t *rank)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) rank[e] = ST_UNLISTED;
}
__global__ __launch_bounds__(256) void refit_rank_kernel(int g, int n, int cnt, const int32_t *indx, int32_t *rank)
{
    const long long o = (long long)blockIdx.y * g, oi = (long long)blockIdx.y * n;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < cnt; p += (long long)gridDim.x * 256) {
        const int32_t e = indx[oi + p] - 1;
        if (e >= 0 && e < g) atomicMin(&rank[o + e], (int32_t)p);           // (an integer minimum: the order of arrival does not show)
    }
}

// x = m .* S_in (x may be S_in)
__global__ __launch_bounds__(256) void refit_mask_kernel(long long g, int K, const int32_t *rank, const double2 *S, double2 *x)
{
    const long long o = (long long)blockIdx.y * g;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < g; e += (long long)gridDim.x * 256) {
        const bool in = !rank || rank[o + e] < K;
        x[o + e] = in ? S[o + e] : make_double2(0.0, 0.0);
    }
}

// between the two halves of an operator: X = (Omega .* Omega) .* X (sq), or X = Omega .* Y (the right-hand side)
__global__ __launch_bounds__(256) void refit_weight_kernel(long long n, int sq, const double *Omega, const double2 *Y, double2 *X)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const double o = Omega[e], w = sq ? o * o : o;
        const double2 y = Y[e];
        X[e] = make_double2(w * y.x, w * y.y);
    }
}

// the per-trial scalars of the recurrence
struct Refit64 {
    double *gam, *gam0;         // gamma of the next step, gamma_0
    int32_t *frozen, *steps;
    double *resid;              // (iters + 1) per trial, or NULL
};

// r = m .* bb - (m .* q + lam x);  p = r;  gamma_0 = <r, r>;  the row of resid: gamma_0, then NaN.  bb arrives in r, q = the
// unmasked products of x.  One workgroup per trial.
__global__ __launch_bounds__(256) void refit_init_kernel(int g, int K, int iters, double lam, const int32_t *rank, const double2 *x, const double2 *q,
                                                         double2 *r, double2 *p, Refit64 sc)
{
    __shared__ double sh[4];
    const int t = blockIdx.x;
    const long long o = (long long)t * g;
    double gm = 0.0;
    for (long long e = threadIdx.x; e < g; e += 256) {
        double2 v = make_double2(0.0, 0.0);
        if (!rank || rank[o + e] < K) {
            const double2 b = r[o + e], w = q[o + e], xe = x[o + e];
            v = make_double2(b.x - (w.x + lam * xe.x), b.y - (w.y + lam * xe.y));
        }
        r[o + e] = v; p[o + e] = v;
        gm += v.x * v.x + v.y * v.y;
    }
    gm = block_sum64(gm, sh);
    if (sc.resid)
        for (long long k = threadIdx.x; k <= iters; k += 256) sc.resid[(long long)t * (iters + 1) + k] = k ? __builtin_nan("") : gm;
    if (threadIdx.x == 0) { sc.gam[t] = gm; sc.gam0[t] = gm; sc.frozen[t] = 0; sc.steps[t] = 0; }
}

// step k of the recurrence on q = the unmasked products of p.  One workgroup per trial; every sum in a fixed order.
__global__ __launch_bounds__(256) void refit_step_kernel(int g, int K, int iters, int k, double lam, double tol, const int32_t *rank, const double2 *q,
                                                         double2 *x, double2 *r, double2 *p, Refit64 sc)
{
    __shared__ double sh[4];
    const int t = blockIdx.x;
    if (sc.frozen[t]) return;
    const long long o = (long long)t * g;
    const double gm = sc.gam[t], g0 = sc.gam0[t];
    if (gm == 0.0 || (tol > 0.0 && gm <= tol * tol * g0)) {         // (false for a NaN on the left)
        if (threadIdx.x == 0) sc.frozen[t] = 1;
        return;
    }
    double dl = 0.0;
    for (long long e = threadIdx.x; e < g; e += 256) {
        if (rank && !(rank[o + e] < K)) continue;
        const double2 pe = p[o + e], w = q[o + e];
        dl += pe.x * (w.x + lam * pe.x) + pe.y * (w.y + lam * pe.y);
    }
    dl = block_sum64(dl, sh);
    if (!(dl > 0.0 && dl <= DBL_MAX)) {                             // not positive and finite: a NaN trial, a vanished direction
        if (threadIdx.x == 0) sc.frozen[t] = 1;
        return;
    }
    const double alpha = gm / dl;
    double gn = 0.0;
    for (long long e = threadIdx.x; e < g; e += 256) {
        if (rank && !(rank[o + e] < K)) continue;                   // (x, r and p hold exact zeros there)
        const double2 pe = p[o + e], w = q[o + e];
        double2 xe = x[o + e], re = r[o + e];
        xe.x += alpha * pe.x; xe.y += alpha * pe.y;
        re.x -= alpha * (w.x + lam * pe.x); re.y -= alpha * (w.y + lam * pe.y);
        x[o + e] = xe; r[o + e] = re;
        gn += re.x * re.x + re.y * re.y;
    }
    gn = block_sum64(gn, sh);
    const double beta = gn / gm;
    for (long long e = threadIdx.x; e < g; e += 256) {                    // (every thread reads the r it wrote itself)
        if (rank && !(rank[o + e] < K)) continue;
        const double2 re = r[o + e], pe = p[o + e];
        p[o + e] = make_double2(re.x + beta * pe.x, re.y + beta * pe.y);
    }
    if (threadIdx.x == 0) {
        sc.gam[t] = gn; sc.steps[t] = k;
        if (sc.resid) sc.resid[(long long)t * (iters + 1) + k] = gn;
    }
}

}  // namespace
}  // namespace jstsp

using namespace jstsp;

extern "C" int jstsp_refit_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *subY_, const double *Omega_,
                               const jstsp_c64 *A_, long long strideA, const jstsp_c64 *B_, long long strideB, const jstsp_c64 *S_in_,
                               const int32_t *indx_S_, int n_indx, int K, int iters, double lam, double tol, jstsp_c64 *S_out_, double *resid_out,
                               int32_t *iters_out, int memspace)
{
    const char *nmf = "refit (float64)";
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", nmf);
    JSTSP_REQUIRE((strideA == 0 || strideA >= (long long)N * Gr) && (strideB == 0 || strideB >= (long long)G2 * M), JSTSP_E_SHAPE,
                  "%s: a factor stride is 0 (shared) or at least the size of one factor", nmf);
    JSTSP_REQUIRE(subY_ && Omega_ && A_ && B_ && S_in_ && S_out_, JSTSP_E_NULL, "%s: NULL argument", nmf);
    JSTSP_REQUIRE((long long)Gr * G2 < (1ll << 31) && (long long)N * M < (1ll << 31) && (long long)Gr * M < (1ll << 31) &&
                      (long long)N * G2 < (1ll << 31) && batch <= 65535,
                  JSTSP_E_UNSUPPORTED, "%s: more than 2^31 entries per trial or more than 65535 trials", nmf);
    const long long gl = (long long)Gr * G2;
    JSTSP_REQUIRE(K >= 1 && K <= gl, JSTSP_E_ARG, "%s: K = %d: need 1 <= K <= Gr * G2 = %lld", nmf, K, gl);
    JSTSP_REQUIRE(indx_S_ || K == gl || K <= JSTSP_SUPPORT_TOP_MAX, JSTSP_E_ARG,
                  "%s: K = %d without indx_S: the selection kernel lists at most %d entries (K = Gr * G2 = %lld needs no list)", nmf, K,
                  JSTSP_SUPPORT_TOP_MAX, gl);
    JSTSP_REQUIRE(indx_S_ ? n_indx >= K && n_indx <= gl : n_indx == 0, JSTSP_E_ARG,
                  "%s: n_indx = %d: need K = %d <= n_indx <= Gr * G2 = %lld with indx_S, and 0 without", nmf, n_indx, K, gl);
    JSTSP_REQUIRE(iters >= 1 && iters < INT_MAX, JSTSP_E_ARG, "%s: iters = %d: need at least 1", nmf, iters);
    JSTSP_REQUIRE(lam >= 0.0 && tol >= 0.0, JSTSP_E_ARG, "%s: lam = %g, tol = %g: neither may be negative or NaN", nmf, lam, tol);
    static_assert(ST_MAX == JSTSP_SUPPORT_TOP_MAX, "the kernel's LDS list is the header's limit");

    const bool host = memspace == JSTSP_HOST, masked = K < gl;
    const size_t nm1 = (size_t)N * M, g1 = (size_t)gl;
    hipStream_t st = ctx->stream;
    const double2 *subY, *A, *B, *Sin;
    const double *Omega;
    const int32_t *indx = nullptr;
    double2 *x, *r, *p, *q, *Xs, *T, *W, *gws;
    int32_t *rank = nullptr;
    Refit64 sc;
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nmf, batch, [&](Slab &w, int b) {
        const size_t enm = nm1 * b, eg = g1 * b;
        subY = w.in(reinterpret_cast<const double2 *>(subY_), enm, host);
        Omega = w.in(Omega_, enm, host);
        A = w.in(reinterpret_cast<const double2 *>(A_), dict_elems(strideA, (size_t)N * Gr, b), host);
        B = w.in(reinterpret_cast<const double2 *>(B_), dict_elems(strideB, (size_t)G2 * M, b), host);
        Sin = w.in(reinterpret_cast<const double2 *>(S_in_), eg, host);
        if (indx_S_ && masked) indx = w.in(indx_S_, (size_t)n_indx * b, host);
        x = w.out(reinterpret_cast<double2 *>(S_out_), eg, host);
        sc.resid = resid_out ? w.out(resid_out, (size_t)(iters + 1) * b, host) : nullptr;
        sc.steps = iters_out ? w.out(iters_out, b, host) : w.get<int32_t>(b);
        for (double2 **a : {&r, &p, &q}) *a = w.get<double2>(eg);
        Xs = w.get<double2>(enm); T = w.get<double2>((size_t)Gr * M * b); W = w.get<double2>((size_t)N * G2 * b);
        if (masked) rank = w.get<int32_t>(eg);
        sc.gam = w.get<double>(b); sc.gam0 = w.get<double>(b); sc.frozen = w.get<int32_t>(b);
        size_t e = 1;
        const int shp[4][3] = {{N, G2, Gr}, {N, M, G2}, {Gr, M, N}, {Gr, G2, M}};
        for (const auto &z : shp) e = std::max(e, zgemm64_ws_elems(z[0], z[1], z[2], b));
        gws = w.get<double2>(e);
    }));

    const int g = (int)gl;
    const long long sNM = (long long)nm1, sG = gl, sT = (long long)Gr * M, sW = (long long)N * G2;
    const Mat64 Am{A, strideA, N}, Bm{B, strideB, G2};
    const dim3 gg = rf_grid(gl, batch);
    const unsigned gnm = (unsigned)std::min<size_t>((nm1 * batch + 255) / 256, 4096);
    // the support, and x = m .* S_in
    if (masked && indx) {
        hipLaunchKernelGGL(refit_rank_init_kernel, dim3((unsigned)std::min<size_t>((g1 * batch + 255) / 256, 4096)), dim3(256), 0, st,
                           (long long)(g1 * batch), rank);
        hipLaunchKernelGGL(refit_rank_kernel, rf_grid(K, batch), dim3(256), 0, st, g, n_indx, K, indx, rank);
    } else if (masked) {
        hipLaunchKernelGGL(support_top_kernel<double2>, dim3(batch), dim3(ST_THREADS), 0, st, g, K, Sin, (int32_t *)nullptr, rank);
    }
    hipLaunchKernelGGL(refit_mask_kernel, gg, dim3(256), 0, st, gl, K, rank, Sin, x);
    JSTSP_HIP(hipGetLastError());
    // dst = A^H (w .* src) B^H, the second half of an operator (src N x M; w = Omega or Omega .* Omega)
    auto back = [&](int sq, const double2 *src, double2 *dst) -> int {
        hipLaunchKernelGGL(refit_weight_kernel, dim3(gnm), dim3(256), 0, st, (long long)(nm1 * batch), sq, Omega, src, Xs);
        JSTSP_TRY(zgemm64(st, 'C', 'N', Gr, M, N, batch, Am, Mat64{Xs, sNM, N}, T, sT, Gr, gws));                     // A^H ...
        JSTSP_TRY(zgemm64(st, 'N', 'C', Gr, G2, M, batch, Mat64{T, sT, Gr}, Bm, dst, sG, Gr, gws));                   // ... B^H
        return 0;
    };
    // q = A^H ((Omega .* Omega) .* (A v B)) B^H
    auto normal = [&](const double2 *v) -> int {
        JSTSP_TRY(zgemm64(st, 'N', 'N', N, G2, Gr, batch, Am, Mat64{v, sG, Gr}, W, sW, N, gws));                      // A v
        JSTSP_TRY(zgemm64(st, 'N', 'N', N, M, G2, batch, Mat64{W, sW, N}, Bm, Xs, sNM, N, gws));                      // ... B
        return back(1, Xs, q);
    };
    JSTSP_TRY(back(0, subY, r));
    JSTSP_TRY(normal(x));
    hipLaunchKernelGGL(refit_init_kernel, dim3(batch), dim3(256), 0, st, g, K, iters, lam, rank, x, q, r, p, sc);
    for (int k = 1; k <= iters; ++k) {
        JSTSP_TRY(normal(p));
        hipLaunchKernelGGL(refit_step_kernel, dim3(batch), dim3(256), 0, st, g, K, iters, k, lam, tol, rank, q, x, r, p, sc);
    }
    JSTSP_HIP(hipGetLastError());
    if (host) {
        JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(S_out_), x, g1 * batch));
        if (resid_out) JSTSP_TRY(s.copy_back(resid_out, sc.resid, (size_t)(iters + 1) * batch));
        if (iters_out) JSTSP_TRY(s.copy_back(iters_out, sc.steps, (size_t)batch));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}
