// Batched inverse of Hermitian positive-definite Gram matrices — the least-squares branch of
// proposed_algorithm ('std', proposed_algorithm.m:29,53): v = U\(L\k) with [L,U] = lu(K2) is the
// least-squares solution K2^+ k; with K2 = kron(B.', A) of full column rank
//     K2^+ k = vec( (A^H A)^-1 A^H K B^H (B B^H)^-1 ),
// so the LU of the (N*M) x (Gr*G2) Kronecker matrix becomes two small Hermitian inverses.
//   n <= 128 : eigen-decomposition (Jacobi, eig.hip)  G^-1 = U diag(1/lambda) U^H; a Gram with an eigenvalue at or
//              below n*eps*lambda_max is singular at fp32 resolution: its components are dropped (pinv semantics) and
//              its ratio goes to the record as 0, so that the call is refused instead of returning a truncated inverse
//   n  > 128 : Newton-Schulz  X <- X (2I - G X),  X0 = I / ||G||_1, all on the MFMA GEMM, NS_STEPS steps, then
//              ||I - G X||_F / sqrt(n) and lambda_min/lambda_max = 1 / (lambda_max(G) lambda_max(X)) are measured
// This is the route for factors too large for the float64 pinv kernel (pinv.hip), which every shape of the
// reference's own drivers takes instead.  Accuracy here is cond(G) * eps_fp32: lambda_min/lambda_max and the
// Newton-Schulz residual go to the context's conditioning record (jstsp_last_conditioning), and JSTSP_HOST calls
// fail with JSTSP_E_ILLCOND instead of returning digits that are not there.
#include "solver_common.h"
#include <algorithm>

namespace jstsp {

// T = U * diag(1/lam)   (column scaling).  Eigenvalues of the fp32 Gram at or below n*eps*lam_max (and non-positive
// ones) are noise: their components are dropped, as pinv drops singular values below its tolerance.  The ratio
// lam_min/lam_max of each matrix is folded into the context's conditioning record - as 0 when a component was dropped:
// the inverse is then truncated, and the record must make the call fail (diag_check_host), not report a ratio above
// the refusal threshold (1e-6 < n*eps for n >= 9).
__global__ __launch_bounds__(256) void scale_cols_inv_kernel(int n, const float2 *U, const float *lam, float2 *T,
                                                             uint32_t *rcond_min_bits)
{
    const int t = blockIdx.y;
    const long long base = (long long)t * n * n;
    const float *l = lam + (long long)t * n;
    float lmax = 0.f, lmin = 3.4e38f;
    for (int i = 0; i < n; ++i) { lmax = fmaxf(lmax, l[i]); lmin = fminf(lmin, l[i]); }
    const float cut = (float)n * 1.1920929e-7f * lmax;
    if (blockIdx.x == 0 && threadIdx.x == 0 && rcond_min_bits)
        atomicMin(rcond_min_bits, __float_as_uint(lmax > 0.f && lmin > cut ? lmin / lmax : 0.f));
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n * n; e += gridDim.x * 256) {
        const float lv = l[e / n];
        const float s = lv > cut ? 1.f / lv : 0.f;
        const float2 u = U[base + e];
        T[base + e] = make_float2(u.x * s, u.y * s);
    }
}

// After Newton-Schulz, one workgroup per matrix (P = G X; lg, lx: lambda_max of G and of X, exact eigenvalue solves):
//   q   = 1 / (lambda_max(G) lambda_max(X))  = lambda_min/lambda_max of G once X = G^-1.  A direction that has not
//         converged cannot raise q above the refusal threshold: X grows along it by 2 per step, to 2^NS_STEPS / ||G||_1;
//   res = ||I - P||_F / sqrt(n), the rms of the eigenvalues of I - G X (a max-entry residual sees an unconverged
//         direction v only as |e| |v_i| |v_j|).  Converged, it is the rounding floor of the inverse, about
//         eps32 * lambda_max/lambda_min; more than NS_RES_FLOOR times that is not rounding, and q is recorded as 0.
// The batch's largest res and smallest q go to the conditioning record (float bits; NaN -> res +inf, q 0).
constexpr double NS_RES_FLOOR = 64.0 * 5.9604645e-8;
__global__ __launch_bounds__(256) void ns_check_kernel(int n, const float2 *P, const float *lg, const float *lx,
                                                       uint32_t *res_max_bits, uint32_t *ratio_min_bits)
{
    __shared__ double sh[4];
    const long long base = (long long)blockIdx.x * n * n;
    double se = 0.0;
    for (int e = threadIdx.x; e < n * n; e += 256) {
        const float2 p = P[base + e];
        const double d = ((e % n == e / n) ? 1.0 : 0.0) - (double)p.x;
        se += d * d + (double)p.y * p.y;
    }
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = se;
    __syncthreads();
    if (threadIdx.x == 0) {
        se = sh[0] + sh[1] + sh[2] + sh[3];
        const double res = sqrt(se / n);
        atomicMax(res_max_bits, res == res ? __float_as_uint((float)res) : 0x7f800000u);
        double q = 1.0 / ((double)lg[blockIdx.x] * (double)lx[blockIdx.x]);
        if (!(q == q && q > 0.0) || !(res * q <= NS_RES_FLOOR)) q = 0.0;
        atomicMin(ratio_min_bits, __float_as_uint((float)fmin(q, 1.0)));
    }
}

// X0 = I / ||G||_1   (one workgroup per matrix)
__global__ __launch_bounds__(256) void ns_init_kernel(int n, const float2 *G, float2 *X)
{
    __shared__ float sh[4];
    const int t = blockIdx.x;
    const float2 *g = G + (long long)t * n * n;
    float best = 0.f;
    for (int j = threadIdx.x; j < n; j += 256) {
        float s = 0.f;
        for (int i = 0; i < n; ++i) { const float2 v = g[i + (long long)n * j]; s += sqrtf(v.x * v.x + v.y * v.y); }
        best = fmaxf(best, s);
    }
    for (int o = 32; o > 0; o >>= 1) best = fmaxf(best, __shfl_xor(best, o));
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = best;
    __syncthreads();
    const float nrm = fmaxf(fmaxf(sh[0], sh[1]), fmaxf(sh[2], sh[3]));
    float2 *x = X + (long long)t * n * n;
    for (int e = threadIdx.x; e < n * n; e += 256) x[e] = make_float2((e % n == e / n) ? 1.f / nrm : 0.f, 0.f);
}

// P <- 2I - P
__global__ __launch_bounds__(256) void two_i_minus_kernel(int n, float2 *P)
{
    const int t = blockIdx.y;
    const long long base = (long long)t * n * n;
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n * n; e += gridDim.x * 256) {
        float2 p = P[base + e];
        p.x = ((e % n == e / n) ? 2.f : 0.f) - p.x;
        p.y = -p.y;
        P[base + e] = p;
    }
}

void HinvWS::take(Arena &a, int n, int count)
{
    const size_t nn = (size_t)n * n;
    T1 = a.get<float2>(count * nn);
    T2 = a.get<float2>(count * nn);
    lam = a.get<float>((size_t)count * n);
    const int ne = (n + 1) & ~1;
    Vg = (n <= 128 && eig_needs_global_v(n)) ? a.get<float2>((size_t)count * ne * ne) : nullptr;
}

size_t hinv_bytes(int n, int count)
{
    Arena m = Arena::measuring();
    HinvWS w;
    w.take(m, n, count);
    return m.peak;
}

int hermitian_inverse(jstsp_ctx *ctx, int n, int count, const float2 *G, float2 *Ginv)
{
    HinvWS w;
    w.take(ctx->arena, n, count);
    JSTSP_REQUIRE(!ctx->arena.overrun, JSTSP_E_NOMEM, "hermitian_inverse: workspace exhausted");
    return hermitian_inverse(ctx, n, count, G, Ginv, w);
}

// Ginv[t] = G[t]^-1 for `count` Hermitian positive-definite n x n matrices.
int hermitian_inverse(jstsp_ctx *ctx, int n, int count, const float2 *G, float2 *Ginv, const HinvWS &w)
{
    const size_t nn = (size_t)n * n;
    JSTSP_TRY(ensure_diag(ctx));
    float2 *T1 = w.T1, *T2 = w.T2, *Vg = w.Vg;
    float *lam = w.lam;
    const long long s = (long long)nn;
    const dim3 grid((unsigned)std::min<size_t>((nn + 255) / 256, 64), (unsigned)count);
    if (n <= 128) {
        JSTSP_TRY(launch_eig(ctx, EIG_VECS, n, count, G, s, 1, 0, nullptr, nullptr, T1, lam, Vg));   // T1 = U
        hipLaunchKernelGGL(scale_cols_inv_kernel, grid, dim3(256), 0, ctx->stream, n, T1, lam, T2, ctx->diag + 2);   // T2 = U / lam
        JSTSP_HIP(hipGetLastError());
        return gemm(ctx, 'N', 'C', n, n, n, count, Mat{T2, s, n}, Mat{T1, s, n}, Ginv, s, n);           // (U/lam) U^H
    }
    // Newton-Schulz: X_{k+1} = X_k (2I - G X_k); I - G X_k = (I - G X_0)^(2^k), the slowest direction starts at
    // 1 - lambda_min / ||G||_1 with ||G||_1 <= sqrt(n) lambda_max.  It reaches fp32 resolution (e^-16) once
    // 2^k lambda_min / ||G||_1 >= 16: NS_STEPS = 32 covers every Gram above the refusal threshold
    // (lambda_min/lambda_max >= 1e-6) up to order 7e4.  24 steps cover it only up to lambda_max/lambda_min ~ 1e6 / sqrt(n)
    // when ||G||_1 ~ sqrt(n) lambda_max (eigenvectors spread over all coordinates): cond(factor) ~ 250 at order 256.  Steps
    // beyond convergence leave X at G^-1 (the iteration is self-correcting to first order).
    constexpr int NS_STEPS = 32;
    hipLaunchKernelGGL(ns_init_kernel, dim3(count), dim3(256), 0, ctx->stream, n, G, Ginv);
    float2 *X = Ginv, *Xn = T2;
    for (int it = 0; it < NS_STEPS; ++it) {
        JSTSP_TRY(gemm(ctx, 'N', 'N', n, n, n, count, Mat{G, s, n}, Mat{X, s, n}, T1, s, n));           // T1 = G X
        hipLaunchKernelGGL(two_i_minus_kernel, grid, dim3(256), 0, ctx->stream, n, T1);                 // T1 = 2I - G X
        JSTSP_TRY(gemm(ctx, 'N', 'N', n, n, n, count, Mat{X, s, n}, Mat{T1, s, n}, Xn, s, n));          // Xn = X T1
        std::swap(X, Xn);
    }
    // what the fixed number of steps left (||I - G X||_F / sqrt(n)) and lambda_min/lambda_max, into the conditioning record:
    // lambda_max of G and of X = G^-1 from the large-order eigen solver (eig_large.hip: it waits for the stream once per sweep)
    JSTSP_TRY(gemm(ctx, 'N', 'N', n, n, n, count, Mat{G, s, n}, Mat{X, s, n}, T1, s, n));
    float *lg = lam, *lx = lam + count;                       // (lam holds count * n >= 2 * count floats)
    JSTSP_TRY(launch_lmax(ctx, n, count, G, s, 1, 0, lg));
    JSTSP_TRY(launch_lmax(ctx, n, count, X, s, 1, 0, lx));
    hipLaunchKernelGGL(ns_check_kernel, dim3(count), dim3(256), 0, ctx->stream, n, T1, lg, lx, ctx->diag + 1, ctx->diag + 2);
    JSTSP_HIP(hipGetLastError());
    if (X != Ginv) JSTSP_HIP(hipMemcpyAsync(Ginv, X, count * nn * sizeof(float2), hipMemcpyDeviceToDevice, ctx->stream));
    return 0;
}

}  // namespace jstsp
