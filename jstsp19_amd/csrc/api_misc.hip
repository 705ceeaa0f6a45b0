// Kernel-level entry points (correlate / synthesize), svt, the matrix-completion baselines
// mc_svt / mc_admm and the spectral-norm NMSE of the drivers.
#include "solver_common.h"
#include <algorithm>

namespace jstsp {

__global__ __launch_bounds__(256) void diff_kernel(long long n, const float2 *a, const float2 *b, float2 *o)
{
    const long long stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        o[i] = make_float2(a[i].x - b[i].x, a[i].y - b[i].y);
}

// nmse = min(1, num/den)   (plot_errorVSsnr.m:138-141; NaN stays NaN: `NaN > 1` is false)
__global__ void ratio_cap_kernel(int batch, const float *num, const float *den, double *out, int cap,
                                 long long ostride, long long ooff)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < batch) {
        double e = (double)num[t] / (double)den[t];
        if (cap && e > 1.0) e = 1.0;
        out[(long long)t * ostride + ooff] = e;
    }
}

// ---- the two scoring entries (jstsp_nmse_spectral_c32 / jstsp_rate_c32) work on operands scaled per trial by an exact power of two.
// lmax_kernel squares Gram entries (a fourth power of the input) and guards with absolute constants (1e-30f, +-1e30f): at an input
// scale of 2^-40 its reflector norm underflows, at 2^+40 its squared off-diagonal overflows, and over an all-zero matrix it returns
// its floor instead of 0.  D = S - Zbar and Zbar are therefore brought to a largest |re|, |im| in [1, 2) before the Gram (every fp32
// operation on them is then the same operation on other exponents: results at ordinary magnitudes keep their digits), the scale is
// undone in double on the two lambda_max, an all-zero operand scores exactly 0, and a trial with a non-finite entry scores NaN
// without its values ever reaching the eigen-solvers (fminf / fmaxf drop a NaN: the Sturm count then returns a finite number).
// sigma_max_sq itself is untouched: the ADMM loops that call it once per iteration do not pay for this.

// mx[2 t], mx[2 t + 1] = largest |re|, |im| over D[t] = S[t] - Zbar[t] and over Zbar[t], as the bits of a non-negative float: NaN
// orders above Inf and Inf above every finite value, so a non-finite entry wins the maximum (mx zeroed beforehand)
__global__ __launch_bounds__(256) void score_absmax_kernel(long long n, int batch, const float2 *S, const float2 *Zb, uint32_t *mx)
{
    const long long stride = (long long)gridDim.x * 256;
    for (int t = blockIdx.y; t < batch; t += gridDim.y) {
        const long long base = (long long)t * n;
        uint32_t md = 0u, mz = 0u;
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            const float2 s = S[base + i], z = Zb[base + i];
            md = max(md, max(__float_as_uint(s.x - z.x) & 0x7fffffffu, __float_as_uint(s.y - z.y) & 0x7fffffffu));
            mz = max(mz, max(__float_as_uint(z.x) & 0x7fffffffu, __float_as_uint(z.y) & 0x7fffffffu));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            md = max(md, (uint32_t)__shfl_xor((int)md, o));
            mz = max(mz, (uint32_t)__shfl_xor((int)mz, o));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicMax(&mx[2 * t], md);
            atomicMax(&mx[2 * t + 1], mz);
        }
    }
}

__device__ __forceinline__ bool score_bad(uint32_t m) { return m >= 0x7f800000u; }
__device__ __forceinline__ int score_exp(uint32_t m) { return (m > 0u && !score_bad(m)) ? ilogbf(__uint_as_float(m)) : 0; }

// D[t] = (S[t] - Zbar[t]) 2^-ed, Zs[t] = Zbar[t] 2^-ez with the exponents of mx; zeros for a trial with a non-finite entry
__global__ __launch_bounds__(256) void score_scale_kernel(long long n, int batch, const float2 *S, const float2 *Zb, const uint32_t *mx,
                                                          float2 *D, float2 *Zs)
{
    const long long stride = (long long)gridDim.x * 256;
    for (int t = blockIdx.y; t < batch; t += gridDim.y) {
        const long long base = (long long)t * n;
        const uint32_t md = mx[2 * t], mz = mx[2 * t + 1];
        const bool bad = score_bad(md) || score_bad(mz);
        const int ed = -score_exp(md), ez = -score_exp(mz);
        for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
            const float2 s = S[base + i], z = Zb[base + i];
            D[base + i] = bad ? make_float2(0.f, 0.f) : make_float2(ldexpf(s.x - z.x, ed), ldexpf(s.y - z.y, ed));
            Zs[base + i] = bad ? make_float2(0.f, 0.f) : make_float2(ldexpf(z.x, ez), ldexpf(z.y, ez));
        }
    }
}

// e = norm(S - Zbar)^2 / norm(Zbar)^2 from the lambda_max of the scaled operands: NaN for a non-finite entry, an all-zero operand
// counts as exactly 0 (0/0 = NaN and x/0 = Inf, as the host formula and MATLAB give them)
__device__ __forceinline__ double score_e(int t, const float *num, const float *den, const uint32_t *mx)
{
    const uint32_t md = mx[2 * t], mz = mx[2 * t + 1];
    if (score_bad(md) || score_bad(mz)) return (double)NAN;
    const double nu = md ? ldexp((double)num[t], 2 * score_exp(md)) : 0.0;
    const double de = mz ? ldexp((double)den[t], 2 * score_exp(mz)) : 0.0;
    return nu / de;
}

// out[t] = Re(u^H G u) / (u^H u) in double for the column u of the basis U[t] whose eigenvalue lam[t][:] is the largest; G = the sum
// of the Gram partials.  The quotient is exact to the SQUARE of the basis' error, so the last rotations of the block Jacobi - whose
// number depends on the other matrices of the batch - do not reach its float bits, where the fp32 quotients of eig_large.hip (an
// fp32 product G U) moved by an ulp between a trial scored alone and in a batch.  n <= 2048; one workgroup per trial.
__global__ __launch_bounds__(256) void score_top_rayleigh_kernel(int n, const float2 *Gpart, long long sGt, int nsplit, long long sGs,
                                                                 const float2 *U, const float *lam, float *out)
{
    const int t = blockIdx.x, tid = threadIdx.x;
    __shared__ double ur[2048], ui[2048], red[8];
    __shared__ int top;
    if (tid == 0) {
        int c = 0;
        for (int i = 1; i < n; ++i) if (lam[(size_t)t * n + i] > lam[(size_t)t * n + c]) c = i;
        top = c;
    }
    __syncthreads();
    const float2 *u = U + ((size_t)t * n + top) * n;
    for (int i = tid; i < n; i += 256) { ur[i] = u[i].x; ui[i] = u[i].y; }
    __syncthreads();
    double num = 0.0, den = 0.0;
    const float2 *G = Gpart + (long long)t * sGt;
    for (long long e = tid; e < (long long)n * n; e += 256) {
        const int i = (int)(e % n), j = (int)(e / n);
        double gx = 0.0, gy = 0.0;
        for (int s = 0; s < nsplit; ++s) {
            const float2 g = G[(long long)s * sGs + e];
            gx += g.x; gy += g.y;
        }
        num += ur[i] * (gx * ur[j] - gy * ui[j]) + ui[i] * (gx * ui[j] + gy * ur[j]);      // Re(conj(u_i) g_ij u_j)
    }
    for (int i = tid; i < n; i += 256) den += ur[i] * ur[i] + ui[i] * ui[i];
    for (int o = 32; o > 0; o >>= 1) { num += __shfl_xor(num, o); den += __shfl_xor(den, o); }
    if ((tid & 63) == 0) { red[tid >> 6] = num; red[4 + (tid >> 6)] = den; }
    __syncthreads();
    if (tid == 0) out[t] = (float)(((red[0] + red[1]) + (red[2] + red[3])) / ((red[4] + red[5]) + (red[6] + red[7])));
}

// nmse = min(1, e)   (plot_errorVSsnr.m:138-141; NaN stays NaN: `NaN > 1` is false)
__global__ void score_nmse_kernel(int batch, const float *num, const float *den, const uint32_t *mx, double *out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < batch) {
        double e = score_e(t, num, den, mx);
        if (e > 1.0) e = 1.0;
        out[t] = e;
    }
}

// mc_svt.m:9   Y = Y + rho (OH - Omega .* X)
__global__ __launch_bounds__(256) void mc_svt_update_kernel(long long nm, float2 *Y, const float2 *OH,
                                                            const float *Omega, const float2 *X,
                                                            const TrialParams *prm)
{
    const int t = blockIdx.y;
    const TrialParams p = prm[t];               // (rho as two floats: common.h)
    const long long base = (long long)t * nm, stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nm; i += stride) {
        const float om = Omega[base + i];
        const float2 x = X[base + i], oh = OH[base + i];
        float2 y = Y[base + i];
        const float dx = oh.x - om * x.x, dy = oh.y - om * x.y;
        y.x = fmaf(p.rho, dx, y.x) + p.rho_lo * dx;
        y.y = fmaf(p.rho, dy, y.y) + p.rho_lo * dy;
        Y[base + i] = y;
    }
}

// mc_admm.m:24-26   Y = (OH + Z + rho X) ./ (Omega + rho);  Z = Z + rho (X - Y);  Zn = Y - Z/rho (next svt arg)
__global__ __launch_bounds__(256) void mc_admm_update_kernel(long long nm, float2 *Y, float2 *Z,
                                                             const float2 *OH, const float *invD,
                                                             const float2 *X, const TrialParams *prm,
                                                             float2 *Zn)
{
    const int t = blockIdx.y;
    const TrialParams p = prm[t];               // (rho, 1/rho as two floats each: common.h)
    const long long base = (long long)t * nm, stride = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nm; i += stride) {
        const float id = invD[base + i];
        const float2 x = X[base + i], oh = OH[base + i];
        float2 z = Z[base + i];
        const float2 y = make_float2(((oh.x + z.x) + mul2(p.rho, p.rho_lo, x.x)) * id, ((oh.y + z.y) + mul2(p.rho, p.rho_lo, x.y)) * id);
        z.x = admm_v1(p, z.x, x.x, y.x);        // Z + rho (X - Y)
        z.y = admm_v1(p, z.y, x.y, y.y);
        Y[base + i] = y;
        Z[base + i] = z;
        Zn[base + i] = make_float2(admm_z(p, y.x, z.x), admm_z(p, y.y, z.y));
    }
}

// lam[t][c] = Re(u_c^H G u_c) / (u_c^H u_c) in double: G the sum of the Gram partials, u_c column c of the basis jacobi_kernel
// returned.  The diagonal that kernel ends with has been through sweeps x (n - 1) fp32 rotations, each of which leaves eps |largest
// entry| in the diagonal entries it touches - of the order of a near-zero eigenvalue itself; a Rayleigh quotient is exact to the
// SQUARE of the basis' error (1e-12 lambda_max).  n <= 128; grid (n, batch).
__global__ __launch_bounds__(256) void rate_rayleigh_kernel(int n, const float2 *Gpart, long long sGt, int nsplit, long long sGs,
                                                            const float2 *U, double *lam)
{
    const int c = blockIdx.x, t = blockIdx.y, tid = threadIdx.x;
    __shared__ double ur[128], ui[128], red[8];
    const float2 *u = U + ((size_t)t * n + c) * n;
    for (int i = tid; i < n; i += 256) { ur[i] = u[i].x; ui[i] = u[i].y; }
    __syncthreads();
    double num = 0.0, den = 0.0;
    const float2 *G = Gpart + (long long)t * sGt;
    for (int e = tid; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        double gx = 0.0, gy = 0.0;
        for (int s = 0; s < nsplit; ++s) {
            const float2 g = G[(long long)s * sGs + e];
            gx += g.x; gy += g.y;
        }
        num += ur[i] * (gx * ur[j] - gy * ui[j]) + ui[i] * (gx * ui[j] + gy * ur[j]);      // Re(conj(u_i) g_ij u_j)
    }
    for (int i = tid; i < n; i += 256) den += ur[i] * ur[i] + ui[i] * ui[i];
    for (int o = 32; o > 0; o >>= 1) { num += __shfl_xor(num, o); den += __shfl_xor(den, o); }
    if ((tid & 63) == 0) { red[tid >> 6] = num; red[4 + (tid >> 6)] = den; }
    __syncthreads();
    if (tid == 0) lam[(size_t)t * n + c] = ((red[0] + red[1]) + (red[2] + red[3])) / ((red[4] + red[5]) + (red[6] + red[7]));
}

// rate[t] = sum_i log2(1 + lam_i / (R (noise_var + e)))   (plot_rateVSframelength.m:81: log2 det(I + Zbar Zbar'/(R (..))));
// lam: the eigenvalues of the Gram of the scaled Zbar (score_scale_kernel, rate_rayleigh_kernel), brought back in double
__global__ __launch_bounds__(256) void rate_kernel(int batch, int n, int R, const double *lam, const float *num,
                                                   const float *den, const uint32_t *mx, double noise_var, double *rate)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= batch) return;
    const double e = score_e(t, num, den, mx);
    const double c = 1.0 / ((double)R * (noise_var + e));
    const int ez2 = 2 * score_exp(mx[2 * t + 1]);
    double acc = 0.0;
    // A negative eigenvalue of a Gram is rounding noise, and the noise of the near-zero eigenvalues has either sign with a sum the
    // trace pins down: while |lam c| is small the negative terms are kept, so that they cancel the positive noise to first order
    // (clamping them all to 0 left a bias: 2.6e-5 of the rate at 128 x 600 with a rank-4 Zbar); larger negative terms are clamped.
    for (int i = 0; i < n; ++i) {
        const double x = ldexp(lam[(long long)t * n + i], ez2) * c;
        acc += log2(1.0 + ((x < 0.0 && !(x > -0x1p-10)) ? 0.0 : x));
    }
    rate[t] = acc;
}

// ---- equilibration of the public correlate / synthesize on the split-f16 path -----------------------------------
// The split x = h + l of hgemm.hip is exact to 2^-23 of the per-PROBLEM maximum.  A row of K (or of B) far below that
// maximum would keep fewer digits than an fp32 product gives it, although the output row it produces depends on nothing
// else.  Rows / columns along the indices that are NOT contracted are therefore scaled by exact powers of two to a
// common magnitude before the split and scaled back afterwards: every output row and column then carries fp32 relative
// accuracy with respect to its own operands.  (Along the contracted index the accuracy is that of the sum's largest terms,
// as in any fp32 product whose addends differ in magnitude.)

// e[t][i] = exponent of max(|re|, |im|) over row i (axis 0) or column i (axis 1) of the rows x cols matrix X[t]; 0 for a zero line
__global__ __launch_bounds__(256) void axis_exp_kernel(int rows, int cols, const float2 *X, long long sXt, int axis, int32_t *e)
{
    const int t = blockIdx.y, tid = threadIdx.x;
    const float2 *x = X + (long long)t * sXt;
    __shared__ float red[256];
    if (axis == 0) {
        const int r = blockIdx.x * 64 + (tid & 63), ph = tid >> 6;
        float m = 0.f;
        if (r < rows)
            for (int c = ph; c < cols; c += 4) {
                const float2 v = x[r + (long long)rows * c];
                m = fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y)));
            }
        red[tid] = m;
        __syncthreads();
        if (ph == 0 && r < rows) {
            m = fmaxf(fmaxf(red[tid], red[tid + 64]), fmaxf(red[tid + 128], red[tid + 192]));
            e[(long long)t * rows + r] = (m > 0.f && m < INFINITY) ? ilogbf(m) : 0;
        }
    } else {
        const int c = blockIdx.x * 4 + (tid >> 6), l = tid & 63;
        float m = 0.f;
        if (c < cols)
            for (int r = l; r < rows; r += 64) {
                const float2 v = x[r + (long long)rows * c];
                m = fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y)));
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if (l == 0 && c < cols) e[(long long)t * cols + c] = (m > 0.f && m < INFINITY) ? ilogbf(m) : 0;
    }
}

// out[t][i, j] = in[t][i, j] * 2^(sign * (er[t][i] + ec[t][j]))   (er / ec may be NULL; strides 0 = shared by the batch)
__global__ __launch_bounds__(256) void scale2_kernel(int rows, int cols, const float2 *in, long long sIn, float2 *out, long long sOut,
                                                     const int32_t *er, long long ser, const int32_t *ec, long long sec, int sign)
{
    const int t = blockIdx.y;
    const long long n = (long long)rows * cols, stride = (long long)gridDim.x * 256;
    const float2 *x = in + (long long)t * sIn;
    float2 *o = out + (long long)t * sOut;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const int r = (int)(i % rows), c = (int)(i / rows);
        const int ex = sign * ((er ? er[(long long)t * ser + r] : 0) + (ec ? ec[(long long)t * sec + c] : 0));
        const float2 v = x[i];
        o[i] = make_float2(ldexpf(v.x, ex), ldexpf(v.y, ex));
    }
}

static int axis_exp(jstsp_ctx *ctx, int rows, int cols, const float2 *X, long long sXt, int count, int axis, int32_t *e)
{
    const dim3 g(axis == 0 ? (rows + 63) / 64 : (cols + 3) / 4, count);
    hipLaunchKernelGGL(axis_exp_kernel, g, dim3(256), 0, ctx->stream, rows, cols, X, sXt, axis, e);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

static dim3 grid2(long long n, int batch);
static int scale2(jstsp_ctx *ctx, int rows, int cols, int count, const float2 *in, long long sIn, float2 *out, long long sOut,
                  const int32_t *er, long long ser, const int32_t *ec, long long sec, int sign)
{
    hipLaunchKernelGGL(scale2_kernel, grid2((long long)rows * cols, count), dim3(256), 0, ctx->stream, rows, cols, in, sIn, out,
                       sOut, er, ser, ec, sec, sign);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

static dim3 grid2(long long n, int batch)
{
    long long blocks = std::max<long long>(1, std::min<long long>((n + 255) / 256, (4096 + batch - 1) / batch));
    return dim3((unsigned)blocks, (unsigned)batch);
}

// D = S - Zbar and a copy of Zbar, each trial scaled by its own power of two (mx: 2 * batch words, see score_absmax_kernel)
static int score_operands(jstsp_ctx *ctx, long long n, int batch, const float2 *S, const float2 *Zb, uint32_t *mx, float2 *D, float2 *Zs)
{
    dim3 g = grid2(n, batch);
    g.y = (unsigned)std::min(batch, 65535);
    JSTSP_HIP(hipMemsetAsync(mx, 0, (size_t)2 * batch * sizeof(uint32_t), ctx->stream));
    hipLaunchKernelGGL(score_absmax_kernel, g, dim3(256), 0, ctx->stream, n, batch, S, Zb, mx);
    hipLaunchKernelGGL(score_scale_kernel, g, dim3(256), 0, ctx->stream, n, batch, S, Zb, mx, D, Zs);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

// sigma_max^2 for the scoring entries.  Orders above 128 take the block Jacobi WITH its basis (EIG_VECS) and the Rayleigh quotient of
// the leading column against the original Gram (score_top_rayleigh_kernel), where the EIG_LMAX mode of sigma_max_sq returns the diagonal of a matrix that went
// through (blocks - 1) x sweeps two-sided fp32 updates - 3e-6 relative per lambda_max, up to 1.05e-5 on an NMSE near 1 (129 x 140,
// 300 trials), against the 2e-6 the project asserts there.  U: batch * n * n, lam: batch * n (n = w.n > 128 only).
static int score_sigma_max_sq(jstsp_ctx *ctx, const GramWS &w, const float2 *Z, float2 *U, float *lam, float *out)
{
    if (w.n <= 128) return sigma_max_sq(ctx, w, Z, out);
    const long long sG = (long long)w.n * w.n;
    JSTSP_TRY(gram_partials(ctx, w, Z, (long long)w.rows * w.cols));
    JSTSP_TRY(launch_eig(ctx, EIG_VECS, w.n, w.batch, w.Gpart, sG * w.nsplit, w.nsplit, sG, nullptr, nullptr, U, lam, nullptr));
    hipLaunchKernelGGL(score_top_rayleigh_kernel, dim3(w.batch), dim3(256), 0, ctx->stream, w.n, w.Gpart, sG * w.nsplit, w.nsplit, sG, U, lam, out);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

static int check_common(jstsp_ctx *ctx, int memspace, const char *what = nullptr)
{
    const char *pre = what ? what : "", *sep = what ? ": " : "";
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "%s%sctx is NULL", pre, sep);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "%s%sbad memspace %d", pre, sep, memspace);
    return 0;
}

static int upload_tau_rho(jstsp_ctx *ctx, int batch, const double *tau, const double *rho, TrialParams *prm)
{
    std::vector<TrialParams> hp(batch);
    for (int t = 0; t < batch; ++t) {
        hp[t] = make_trial_params(rho ? rho[t] : 1.0, tau[t], 0.0);
    }
    return upload(ctx, prm, hp.data(), batch * sizeof(TrialParams));
}

}  // namespace jstsp

using namespace jstsp;

// mc_svt / mc_admm are fixed-point loops whose svt argument moves little from one iteration to the next: the eigen-decomposition of
// iteration i starts from the basis of iteration i - 1 and (orders 65..128, GramWS::eig_stop) runs no further sweep once the Gram
// in that basis has relative off-diagonals below this level - an inexact inner solve.  Measured at configs[2] (128 x 128, 20
// iterations, 16 trials against the float64 oracle): max error of X 5.18e-5 / 9.15e-5 (mc_svt / mc_admm) with the level at 0,
// 5.15e-5 / 9.16e-5 at 1e-4 (the default), 5.13e-5 / 9.18e-5 at 1e-3, 5.5e-5 / 5.5e-4 at 1e-2; mc_svt x 20 at 1024 trials
// 0.112 / 0.066 / 0.051 / 0.050 s.  JSTSP_MC_EIG_STOP overrides (0: every call converged to the end-of-sweep rule).
static float mc_eig_stop()
{
    const char *e = getenv("JSTSP_MC_EIG_STOP");
    return e ? (float)atof(e) : 1e-4f;
}

// One packed b operand for the batch and a shape hgemm_pair_kernel takes: the a operand (rows x Kd per problem, column-major, leading
// dimension `rows`) in fragment order as well - the two-trials-per-workgroup kernel reads packed operands only (hgemm.hip)
// Its shape and array (none when its k padding differs from the b pack's), then the packing into it.
static void pair_apack_take(Arena &a, HPack &ap, int Kd, int batch, const HPack &bp)
{
    ap.KS = 4 * ((Kd + 63) / 64); ap.JT = 2; ap.count = batch;
    ap.st = (long long)ap.JT * ap.KS * 256;
    ap.data = ap.KS == bp.KS ? a.get<uint4>((size_t)batch * ap.st) : nullptr;
}
static int pair_apack(jstsp_ctx *ctx, const HPack &ap, const float2 *Aop, long long sAt, int rows, int Kd, const uint32_t *amax, HGemmDesc &hd)
{
    if (!ap.data) return 0;
    JSTSP_TRY(hgemm_repack(ctx, ap, Aop, sAt, rows, 1, 0, Kd, rows, amax));
    hd.Ap = ap.data; hd.sApt = ap.st; hd.aKS = ap.KS;
    return 0;
}

extern "C" {

int jstsp_correlate_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c32 *K_,
                        const jstsp_c32 *A_, long long strideA, const jstsp_c32 *B_, long long strideB,
                        jstsp_c32 *out, int memspace)
{
    JSTSP_TRY(check_common(ctx, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(K_ && A_ && B_ && out, JSTSP_E_NULL, "correlate: NULL array argument");
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0, JSTSP_E_SHAPE, "correlate: bad shape");
    const size_t nm = (size_t)N * M, g = (size_t)Gr * G2, ng = (size_t)N * G2;
    const bool h2 = use_hgemm(N, G2, M);
    const int nB = strideB ? batch : 1;
    const bool pair = h2 && !strideB && hgemm_pair_shape(N, G2, batch);
    const float2 *K, *A, *B;
    float2 *Tc, *O, *Ks = nullptr, *Bs = nullptr;
    int32_t *eK = nullptr, *eB = nullptr;
    uint32_t *amax = nullptr;
    HPack pk, ap;
    JSTSP_TRY(arena_open(ctx, "correlate", [&](Arena &a) {
        K = a.in(as_f2(K_), batch * nm, memspace);
        A = a.in(as_f2(A_), dict_elems(strideA, (size_t)N * Gr, batch), memspace);
        B = a.in(as_f2(B_), dict_elems(strideB, (size_t)G2 * M, batch), memspace);
        Tc = a.get<float2>(batch * ng);
        O = a.get<float2>(batch * g);
        if (!h2) return;
        eK = a.get<int32_t>((size_t)batch * N); eB = a.get<int32_t>((size_t)nB * G2);
        Ks = a.get<float2>(batch * nm); Bs = a.get<float2>((size_t)nB * G2 * M);
        hgemm_pack_take(pk, a, M, G2, nB);
        amax = a.get<uint32_t>(batch);
        if (pair) pair_apack_take(a, ap, M, batch, pk);
    }));
    // A^H (K B^H): the cheaper association (N*M*G2 + Gr*N*G2 MACs)
    if (h2) {
        // rows of K (index n) and rows of B (index g) are not contracted: equilibrate them (see axis_exp_kernel)
        const long long sBs = strideB ? (long long)G2 * M : 0;
        JSTSP_TRY(axis_exp(ctx, N, M, K, (long long)nm, batch, 0, eK));
        JSTSP_TRY(scale2(ctx, N, M, batch, K, (long long)nm, Ks, (long long)nm, eK, N, nullptr, 0, -1));
        JSTSP_TRY(axis_exp(ctx, G2, M, B, strideB, nB, 0, eB));
        JSTSP_TRY(scale2(ctx, G2, M, nB, B, strideB, Bs, sBs, eB, G2, nullptr, 0, -1));
        // b(k = m, j = g) = conj(B[g + G2 m]) packed once; a = K
        JSTSP_TRY(hgemm_pack_fill(ctx, pk, Bs, sBs, G2, 1, 1, M, G2, (long long)G2 * M));
        JSTSP_TRY(hgemm_absmax(ctx, Ks, (long long)nm, (long long)nm, batch, amax));
        HGemmDesc hd{Ks, (long long)nm, N, amax, pk.data, strideB ? pk.st : 0, pk.bmax, strideB ? 1 : 0, pk.KS, pk.JT,
                     Tc, (long long)ng, N, N, G2, M, batch, EPI_NONE, nullptr, nullptr, nullptr};
        if (pair) JSTSP_TRY(pair_apack(ctx, ap, Ks, (long long)nm, N, M, amax, hd));
        JSTSP_TRY(launch_hgemm(ctx, hd, "correlate"));
        JSTSP_TRY(scale2(ctx, N, G2, batch, Tc, (long long)ng, Tc, (long long)ng, eK, N, eB, strideB ? G2 : 0, +1));
    } else
    JSTSP_TRY(gemm(ctx, 'N', 'C', N, G2, M, batch, Mat{K, (long long)nm, N}, Mat{B, strideB, G2}, Tc,
                   (long long)ng, N, 1.f, nullptr, 0, 0, 0.f, GEMM_CORRELATE));
    JSTSP_TRY(gemm(ctx, 'C', 'N', Gr, G2, N, batch, Mat{A, strideA, N}, Mat{Tc, (long long)ng, N}, O,
                   (long long)g, Gr));
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out), O, batch * g, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int jstsp_synthesize_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c32 *S_,
                         const jstsp_c32 *A_, long long strideA, const jstsp_c32 *B_, long long strideB,
                         jstsp_c32 *out, int memspace)
{
    JSTSP_TRY(check_common(ctx, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(S_ && A_ && B_ && out, JSTSP_E_NULL, "synthesize: NULL array argument");
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0, JSTSP_E_SHAPE, "synthesize: bad shape");
    const size_t nm = (size_t)N * M, g = (size_t)Gr * G2, ng = (size_t)N * G2;
    const bool h2 = use_hgemm(N, M, G2);
    const int nB = strideB ? batch : 1;
    const bool pair = h2 && !strideB && hgemm_pair_shape(N, M, batch);
    const float2 *S, *A, *B;
    float2 *W, *O, *Bs = nullptr;
    int32_t *eW = nullptr, *eB = nullptr;
    uint32_t *amax = nullptr;
    HPack pk, ap;
    JSTSP_TRY(arena_open(ctx, "synthesize", [&](Arena &a) {
        S = a.in(as_f2(S_), batch * g, memspace);
        A = a.in(as_f2(A_), dict_elems(strideA, (size_t)N * Gr, batch), memspace);
        B = a.in(as_f2(B_), dict_elems(strideB, (size_t)G2 * M, batch), memspace);
        W = a.get<float2>(batch * ng);
        O = a.get<float2>(batch * nm);
        if (!h2) return;
        eW = a.get<int32_t>((size_t)batch * N); eB = a.get<int32_t>((size_t)nB * M);
        Bs = a.get<float2>((size_t)nB * G2 * M);
        hgemm_pack_take(pk, a, G2, M, nB);
        amax = a.get<uint32_t>(batch);
        if (pair) pair_apack_take(a, ap, G2, batch, pk);
    }));
    JSTSP_TRY(gemm(ctx, 'N', 'N', N, G2, Gr, batch, Mat{A, strideA, N}, Mat{S, (long long)g, Gr}, W,
                   (long long)ng, N));
    if (h2) {
        // rows of A S (index n) and columns of B (index m) are not contracted: equilibrate them (see axis_exp_kernel)
        const long long sBs = strideB ? (long long)G2 * M : 0;
        JSTSP_TRY(axis_exp(ctx, N, G2, W, (long long)ng, batch, 0, eW));
        JSTSP_TRY(scale2(ctx, N, G2, batch, W, (long long)ng, W, (long long)ng, eW, N, nullptr, 0, -1));
        JSTSP_TRY(axis_exp(ctx, G2, M, B, strideB, nB, 1, eB));
        JSTSP_TRY(scale2(ctx, G2, M, nB, B, strideB, Bs, sBs, nullptr, 0, eB, M, -1));
        // b(k = g, j = m) = B[g + G2 m] packed once; a = A S
        JSTSP_TRY(hgemm_pack_fill(ctx, pk, Bs, sBs, 1, G2, 0, G2, M, (long long)G2 * M));
        JSTSP_TRY(hgemm_absmax(ctx, W, (long long)ng, (long long)ng, batch, amax));
        HGemmDesc hd{W, (long long)ng, N, amax, pk.data, strideB ? pk.st : 0, pk.bmax, strideB ? 1 : 0, pk.KS, pk.JT,
                     O, (long long)nm, N, N, M, G2, batch, EPI_NONE, nullptr, nullptr, nullptr};
        if (pair) JSTSP_TRY(pair_apack(ctx, ap, W, (long long)ng, N, G2, amax, hd));
        JSTSP_TRY(launch_hgemm(ctx, hd, "synthesize"));
        JSTSP_TRY(scale2(ctx, N, M, batch, O, (long long)nm, O, (long long)nm, eW, N, eB, strideB ? M : 0, +1));
    } else
    JSTSP_TRY(gemm(ctx, 'N', 'N', N, M, G2, batch, Mat{W, (long long)ng, N}, Mat{B, strideB, G2}, O,
                   (long long)nm, N, 1.f, nullptr, 0, 0, 0.f, GEMM_SYNTH));
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(out), O, batch * nm, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int jstsp_ls_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c32 *Y_, const jstsp_c32 *A_,
                 long long strideA, const jstsp_c32 *B_, long long strideB, jstsp_c32 *S_out, int memspace)
{
    // S_ls = pinv(A)*Y*pinv(B) (plot_errorVSsnr.m:83).  Per factor:
    //   fits the in-LDS float64 kernel (pinv.hip; every shape of the reference's drivers): SVD-based pinv as MATLAB's;
    //   larger: pinv(A) = (A^H A)^-1 A^H (N >= Gr), pinv(B) = B^H (B B^H)^-1 (M >= G2) through the fp32 Gram inverse
    //           (hinv.hip), conditioning recorded / checked.
    JSTSP_TRY(check_common(ctx, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(Y_ && A_ && B_ && S_out, JSTSP_E_NULL, "ls: NULL array argument");
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0, JSTSP_E_SHAPE, "ls: bad shape");
    const bool pA = pinv_fits(N, Gr), pB = pinv_fits(G2, M);
    JSTSP_REQUIRE((pA || N >= Gr) && (pB || M >= G2), JSTSP_E_UNSUPPORTED,
                  "ls: a factor too large for the float64 pinv kernel must have full rank (A: N >= Gr, B: M >= G2)");
    const size_t nm = (size_t)N * M, g = (size_t)Gr * G2, ng = (size_t)N * G2;
    const int nA = strideA ? batch : 1, nB = strideB ? batch : 1;
    const float2 *Y, *A, *B;
    float2 *Tc, *Tc2, *R1, *S, *PB = nullptr, *GB = nullptr, *GBi = nullptr, *PA = nullptr, *GA = nullptr, *GAi = nullptr;
    HinvWS hB, hA;
    JSTSP_TRY(arena_open(ctx, "ls", [&](Arena &a) {
        Y = a.in(as_f2(Y_), batch * nm, memspace);
        A = a.in(as_f2(A_), dict_elems(strideA, (size_t)N * Gr, batch), memspace);
        B = a.in(as_f2(B_), dict_elems(strideB, (size_t)G2 * M, batch), memspace);
        Tc = a.get<float2>(batch * ng); Tc2 = a.get<float2>(batch * ng); R1 = a.get<float2>(batch * g);
        S = a.get<float2>(batch * g);
        // (the temporaries of an inverse are given back once it is enqueued: what follows lies over them, later in the stream)
        if (pB) PB = a.get<float2>((size_t)nB * M * G2);
        else {
            GB = a.get<float2>((size_t)nB * G2 * G2); GBi = a.get<float2>((size_t)nB * G2 * G2);
            const size_t mark = a.off;
            hB.take(a, G2, nB);
            a.off = mark;
        }
        if (pA) PA = a.get<float2>((size_t)nA * Gr * N);
        else {
            GA = a.get<float2>((size_t)nA * Gr * Gr); GAi = a.get<float2>((size_t)nA * Gr * Gr);
            const size_t mark = a.off;
            hA.take(a, Gr, nA);
            a.off = mark;
        }
    }));
    JSTSP_TRY(diag_reset(ctx));
    const Mat Am{A, strideA, N}, Bm{B, strideB, G2};
    const long long sg = (long long)g, sng = (long long)ng;
    // ---- B side: Tc = Y pinv(B)   (N x G2)
    if (pB) {
        JSTSP_TRY(launch_pinv(ctx, G2, M, nB, B, strideB, G2, PB, (long long)M * G2, M));
        JSTSP_TRY(gemm(ctx, 'N', 'N', N, G2, M, batch, Mat{Y, (long long)nm, N}, Mat{PB, strideB ? (long long)M * G2 : 0, M},
                       Tc, sng, N, 1.f, nullptr, 0, 0, 0.f, GEMM_CORRELATE));
    } else {
        JSTSP_TRY(gemm(ctx, 'N', 'C', G2, G2, M, nB, Bm, Bm, GB, (long long)G2 * G2, G2));
        JSTSP_TRY(hermitian_inverse(ctx, G2, nB, GB, GBi, hB));
        JSTSP_TRY(gemm(ctx, 'N', 'C', N, G2, M, batch, Mat{Y, (long long)nm, N}, Bm, Tc2, sng, N, 1.f, nullptr, 0, 0, 0.f,
                       GEMM_CORRELATE));
        JSTSP_TRY(gemm(ctx, 'N', 'N', N, G2, G2, batch, Mat{Tc2, sng, N}, Mat{GBi, strideB ? (long long)G2 * G2 : 0, G2},
                       Tc, sng, N));
    }
    // ---- A side: S = pinv(A) Tc   (Gr x G2)
    if (pA) {
        JSTSP_TRY(launch_pinv(ctx, N, Gr, nA, A, strideA, N, PA, (long long)Gr * N, Gr));
        JSTSP_TRY(gemm(ctx, 'N', 'N', Gr, G2, N, batch, Mat{PA, strideA ? (long long)Gr * N : 0, Gr}, Mat{Tc, sng, N}, S, sg,
                       Gr));
    } else {
        JSTSP_TRY(gemm(ctx, 'C', 'N', Gr, Gr, N, nA, Am, Am, GA, (long long)Gr * Gr, Gr));
        JSTSP_TRY(hermitian_inverse(ctx, Gr, nA, GA, GAi, hA));
        JSTSP_TRY(gemm(ctx, 'C', 'N', Gr, G2, N, batch, Am, Mat{Tc, sng, N}, R1, sg, Gr));
        JSTSP_TRY(gemm(ctx, 'N', 'N', Gr, G2, Gr, batch, Mat{GAi, strideA ? (long long)Gr * Gr : 0, Gr}, Mat{R1, sg, Gr}, S,
                       sg, Gr));
    }
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(S_out), S, batch * g, memspace));
    if (memspace == JSTSP_HOST) {
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
        JSTSP_TRY(diag_check_host(ctx, "ls"));
    }
    return 0;
}

int jstsp_pinv_c32(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c32 *A_, jstsp_c32 *P_, int memspace)
{
    JSTSP_TRY(check_common(ctx, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(A_ && P_, JSTSP_E_NULL, "pinv: NULL array argument");
    JSTSP_REQUIRE(rows > 0 && cols > 0 && batch > 0, JSTSP_E_SHAPE, "pinv: bad shape");
    JSTSP_REQUIRE(pinv_fits(rows, cols), JSTSP_E_UNSUPPORTED,
                  "pinv: %d x %d does not fit the in-LDS float64 kernel ((max*min + min^2) * 16 B <= 156 KiB)", rows, cols);
    const size_t n = (size_t)rows * cols;
    const float2 *A;
    float2 *P;
    JSTSP_TRY(arena_open(ctx, "pinv", [&](Arena &a) {
        A = a.in(as_f2(A_), batch * n, memspace);
        P = memspace == JSTSP_DEVICE ? as_f2(P_) : a.get<float2>(batch * n);
    }));
    JSTSP_TRY(diag_reset(ctx));
    JSTSP_TRY(launch_pinv(ctx, rows, cols, batch, A, (long long)n, rows, P, (long long)n, cols));
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(P_), P, batch * n, memspace));
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

int jstsp_svt_c32(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c32 *Y_, const double *tau,
                  jstsp_c32 *X_, int memspace)
{
    JSTSP_TRY(check_common(ctx, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(Y_ && tau && X_, JSTSP_E_NULL, "svt: NULL argument");
    JSTSP_REQUIRE(Mr > 0 && Mt > 0 && batch > 0, JSTSP_E_SHAPE, "svt: bad shape");
    JSTSP_REQUIRE(std::min(Mr, Mt) <= 2048, JSTSP_E_UNSUPPORTED, "svt: min(Mr, Mt) = %d > 2048",
                  std::min(Mr, Mt));
    const size_t nm = (size_t)Mr * Mt;
    const float2 *Y;
    TrialParams *prm;
    float2 *X;
    GramWS w;
    JSTSP_TRY(arena_open(ctx, "svt", [&](Arena &a) {
        Y = a.in(as_f2(Y_), batch * nm, memspace);
        prm = a.get<TrialParams>(batch);
        X = a.get<float2>(batch * nm);
        (void)w.alloc(a, Mr, Mt, batch, true);
    }));
    JSTSP_TRY(upload_tau_rho(ctx, batch, tau, nullptr, prm));
    JSTSP_TRY(svt_batched(ctx, w, Y, prm, nullptr, X));
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(X_), X, batch * nm, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int jstsp_nmse_spectral_c32(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c32 *S_,
                            const jstsp_c32 *Zbar_, double *nmse, int memspace)
{
    JSTSP_TRY(check_common(ctx, memspace, "nmse"));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(S_ && Zbar_ && nmse, JSTSP_E_NULL, "nmse: NULL argument");
    JSTSP_REQUIRE(R > 0 && C > 0 && batch > 0, JSTSP_E_SHAPE, "nmse: bad shape");
    JSTSP_REQUIRE(std::min(R, C) <= 2048, JSTSP_E_UNSUPPORTED, "nmse: min(R, C) = %d > 2048", std::min(R, C));
    const size_t n = (size_t)R * C;
    const int ng = std::min(R, C);
    const bool big = ng > 128;                  // (block Jacobi with its basis: score_sigma_max_sq)
    const float2 *S, *Zb;
    float2 *D, *Zs, *U;
    uint32_t *mx;
    float *num, *den, *lam;
    double *o;
    GramWS w;
    JSTSP_TRY(arena_open(ctx, "nmse", [&](Arena &a) {
        S = a.in(as_f2(S_), batch * n, memspace);
        Zb = a.in(as_f2(Zbar_), batch * n, memspace);
        D = a.get<float2>(batch * n); Zs = a.get<float2>(batch * n);
        mx = a.get<uint32_t>((size_t)2 * batch);
        num = a.get<float>(batch); den = a.get<float>(batch);
        o = a.get<double>(batch);
        U = big ? a.get<float2>((size_t)batch * ng * ng) : nullptr;
        lam = big ? a.get<float>((size_t)batch * ng) : nullptr;
        (void)w.alloc(a, R, C, batch, false);
    }));
    JSTSP_TRY(score_operands(ctx, (long long)n, batch, S, Zb, mx, D, Zs));
    JSTSP_TRY(score_sigma_max_sq(ctx, w, D, U, lam, num));
    JSTSP_TRY(score_sigma_max_sq(ctx, w, Zs, U, lam, den));
    hipLaunchKernelGGL(score_nmse_kernel, dim3((batch + 255) / 256), dim3(256), 0, ctx->stream, batch, num, den, mx, o);
    JSTSP_HIP(hipGetLastError());
    JSTSP_TRY(stage_out(ctx, nmse, o, (size_t)batch, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int jstsp_lambda_max_sequence_c32(jstsp_ctx *ctx, int n, int batch, int steps, const jstsp_c32 *G_, float *lam, int memspace)
{
    // lambda_max of a SEQUENCE of batches of Hermitian matrices, matrix t of step s warm-started from matrix t of step s - 1:
    // the kernel behind convergence_error(:,1:2) (proposed_algorithm.m:67,69) as the ADMM loops drive it, on the caller's matrices
    JSTSP_TRY(check_common(ctx, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(G_ && lam, JSTSP_E_NULL, "lambda_max_sequence: NULL argument");
    JSTSP_REQUIRE(n > 0 && n <= 128 && batch > 0 && steps > 0, JSTSP_E_SHAPE, "lambda_max_sequence: 1 <= n <= 128, batch, steps > 0");
    const size_t nn = (size_t)n * n, tot = (size_t)steps * batch;
    const float2 *G;
    float *o;
    GramWS w;                                   // (only the warm-start record and the shape are used)
    w.n = n; w.batch = batch; w.nsplit = 1;
    w.lz.ne = lanczos_ne(n);
    JSTSP_TRY(arena_open(ctx, "lambda_max_sequence", [&](Arena &a) {
        G = a.in(as_f2(G_), tot * nn, memspace);
        w.lz.x = a.get<float2>((size_t)batch * w.lz.ne);
        w.lz.state = a.get<int>((size_t)batch);
        o = a.get<float>(tot);
    }));
    JSTSP_TRY(lanczos_warm_reset(ctx, w));
    for (int s = 0; s < steps; ++s) {
        w.lz.call = s;
        JSTSP_TRY(launch_lmax(ctx, n, batch, G + (size_t)s * batch * nn, (long long)nn, 1, 0, o + (size_t)s * batch, true,
                              w.lz.mismatch ? &w.lz : nullptr, 0));
    }
    JSTSP_TRY(stage_out(ctx, lam, o, tot, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int jstsp_rate_c32(jstsp_ctx *ctx, int R, int C, int batch, const jstsp_c32 *S_, const jstsp_c32 *Zbar_,
                   double noise_var, double *rate, int memspace)
{
    // log2(real(det(eye(Nr) + 1/Nr*Zbar*Zbar'*1/(noise_var + norm(Zbar-S)^2/norm(Zbar)^2))))  (plot_rateVSframelength.m:81)
    // = sum_i log2(1 + lambda_i(Zbar Zbar') / (Nr (noise_var + e))): the eigenvalues of the Gram of the smaller side
    // (det(I + c Z Z') = det(I + c Z' Z)); the NMSE e is NOT capped in that script.
    JSTSP_TRY(check_common(ctx, memspace, "rate"));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(S_ && Zbar_ && rate, JSTSP_E_NULL, "rate: NULL argument");
    JSTSP_REQUIRE(R > 0 && C > 0 && batch > 0, JSTSP_E_SHAPE, "rate: bad shape");
    JSTSP_REQUIRE(std::min(R, C) <= 128, JSTSP_E_UNSUPPORTED, "rate: min(R, C) = %d > 128", std::min(R, C));
    const size_t n = (size_t)R * C;
    const int ng = std::min(R, C), ne = (ng + 1) & ~1;
    const float2 *S, *Zb;
    float2 *D, *Zs, *U, *Vg;
    uint32_t *mx;
    float *num, *den, *lam;
    double *o, *lamd;
    GramWS w;
    JSTSP_TRY(arena_open(ctx, "rate", [&](Arena &a) {
        S = a.in(as_f2(S_), batch * n, memspace);
        Zb = a.in(as_f2(Zbar_), batch * n, memspace);
        D = a.get<float2>(batch * n); Zs = a.get<float2>(batch * n);
        mx = a.get<uint32_t>((size_t)2 * batch);
        num = a.get<float>(batch); den = a.get<float>(batch);
        o = a.get<double>(batch);
        U = a.get<float2>((size_t)batch * ng * ng);
        lam = a.get<float>((size_t)batch * ng);
        lamd = a.get<double>((size_t)batch * ng);
        Vg = eig_needs_global_v(ng) ? a.get<float2>((size_t)batch * ne * ne) : nullptr;
        (void)w.alloc(a, R, C, batch, false);
    }));
    JSTSP_TRY(score_operands(ctx, (long long)n, batch, S, Zb, mx, D, Zs));
    JSTSP_TRY(sigma_max_sq(ctx, w, D, num));
    JSTSP_TRY(sigma_max_sq(ctx, w, Zs, den));                     // leaves the Gram partials of the scaled Zbar in the workspace
    const long long sG = (long long)w.n * w.n;
    JSTSP_TRY(launch_eig(ctx, EIG_VECS, w.n, batch, w.Gpart, sG * w.nsplit, w.nsplit, sG, nullptr, nullptr, U, lam, Vg));
    hipLaunchKernelGGL(rate_rayleigh_kernel, dim3(w.n, batch), dim3(256), 0, ctx->stream, w.n, w.Gpart, sG * w.nsplit, w.nsplit, sG, U, lamd);
    hipLaunchKernelGGL(rate_kernel, dim3((batch + 255) / 256), dim3(256), 0, ctx->stream, batch, w.n, R, lamd, num, den,
                       mx, noise_var, o);
    JSTSP_HIP(hipGetLastError());
    JSTSP_TRY(stage_out(ctx, rate, o, (size_t)batch, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int jstsp_mc_svt_c32(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c32 *OH_, const float *Omega_,
                     int Imax, const double *tau, const double *rho, jstsp_c32 *X_out, int memspace)
{
    JSTSP_TRY(check_common(ctx, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(OH_ && Omega_ && tau && rho && X_out, JSTSP_E_NULL, "mc_svt: NULL argument");
    JSTSP_REQUIRE(Mr > 0 && Mt > 0 && batch > 0 && Imax >= 0, JSTSP_E_SHAPE, "mc_svt: bad shape");
    JSTSP_REQUIRE(std::min(Mr, Mt) <= 2048, JSTSP_E_UNSUPPORTED, "mc_svt: min(Mr, Mt) = %d > 2048",
                  std::min(Mr, Mt));
    const size_t nm = (size_t)Mr * Mt;
    const float2 *OH;
    const float *Omega;
    TrialParams *prm;
    float2 *Y, *X;
    GramWS w;
    JSTSP_TRY(arena_open(ctx, "mc_svt", [&](Arena &a) {
        OH = a.in(as_f2(OH_), batch * nm, memspace);
        Omega = a.in(Omega_, batch * nm, memspace);
        prm = a.get<TrialParams>(batch);
        Y = a.get<float2>(batch * nm); X = a.get<float2>(batch * nm);
        (void)w.alloc(a, Mr, Mt, batch, true);
    }));
    w.eig_stop = mc_eig_stop();
    JSTSP_TRY(upload_tau_rho(ctx, batch, tau, rho, prm));
    JSTSP_HIP(hipMemsetAsync(Y, 0, batch * nm * sizeof(float2), ctx->stream));     // mc_svt.m:5
    JSTSP_HIP(hipMemsetAsync(X, 0, batch * nm * sizeof(float2), ctx->stream));
    for (int it = 0; it < Imax; ++it) {                                              // :7
        JSTSP_TRY(svt_batched(ctx, w, Y, prm, nullptr, X, true));                    // :8
        hipLaunchKernelGGL(mc_svt_update_kernel, grid2((long long)nm, batch), dim3(256), 0, ctx->stream,
                           (long long)nm, Y, OH, Omega, X, prm);                     // :9
    }
    JSTSP_HIP(hipGetLastError());
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(X_out), X, batch * nm, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}

int jstsp_mc_admm_c32(jstsp_ctx *ctx, int Mr, int Mt, int batch, const jstsp_c32 *Htrue_,
                      const jstsp_c32 *OH_, const float *Omega_, int Imax, const double *tau,
                      const double *rho, jstsp_c32 *X_out, double *ce_out, int memspace)
{
    JSTSP_TRY(check_common(ctx, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(OH_ && Omega_ && tau && rho && X_out, JSTSP_E_NULL, "mc_admm: NULL argument");
    JSTSP_REQUIRE(!ce_out || Htrue_, JSTSP_E_NULL, "mc_admm: convergence_error needs Htrue");
    JSTSP_REQUIRE(Mr > 0 && Mt > 0 && batch > 0 && Imax >= 0, JSTSP_E_SHAPE, "mc_admm: bad shape");
    JSTSP_REQUIRE(std::min(Mr, Mt) <= 2048, JSTSP_E_UNSUPPORTED, "mc_admm: min(Mr, Mt) = %d > 2048",
                  std::min(Mr, Mt));
    const size_t nm = (size_t)Mr * Mt;
    const bool want_ce = ce_out != nullptr;
    const float2 *OH, *Htrue = nullptr;
    const float *Omega;
    TrialParams *prm;
    float2 *X, *Y, *Z, *Zn, *D;
    float *invD, *num, *den;
    double *ce;
    GramWS w, wn;
    JSTSP_TRY(arena_open(ctx, "mc_admm", [&](Arena &a) {
        OH = a.in(as_f2(OH_), batch * nm, memspace);
        Omega = a.in(Omega_, batch * nm, memspace);
        if (want_ce) Htrue = a.in(as_f2(Htrue_), batch * nm, memspace);
        prm = a.get<TrialParams>(batch);
        X = a.get<float2>(batch * nm); Y = a.get<float2>(batch * nm); Z = a.get<float2>(batch * nm);
        Zn = a.get<float2>(batch * nm); D = a.get<float2>(batch * nm);
        invD = a.get<float>(batch * nm);
        num = a.get<float>(batch); den = a.get<float>(batch);
        ce = a.get<double>((size_t)batch * std::max(Imax, 1));
        (void)w.alloc(a, Mr, Mt, batch, true);
        if (want_ce) (void)wn.alloc(a, Mr, Mt, batch, false);
    }));
    w.eig_stop = mc_eig_stop();
    JSTSP_TRY(upload_tau_rho(ctx, batch, tau, rho, prm));
    hipStream_t st = ctx->stream;
    JSTSP_HIP(hipMemsetAsync(X, 0, batch * nm * sizeof(float2), st));                // mc_admm.m:6-8
    JSTSP_HIP(hipMemsetAsync(Y, 0, batch * nm * sizeof(float2), st));
    JSTSP_HIP(hipMemsetAsync(Z, 0, batch * nm * sizeof(float2), st));
    JSTSP_HIP(hipMemsetAsync(Zn, 0, batch * nm * sizeof(float2), st));
    JSTSP_TRY(launch_inv_d(ctx, (long long)nm, batch, Omega, 1.f, prm, invD));        // :11-17  A = diag(Omega) + rho I
    if (want_ce) JSTSP_TRY(sigma_max_sq(ctx, wn, Htrue, den));
    if (want_ce) JSTSP_TRY(lanczos_warm_reset(ctx, wn));       // the error curve's lambda_max, warm-started from iteration to iteration
    const long long tot = (long long)batch * nm;
    for (int it = 0; it < Imax; ++it) {                                               // :20
        JSTSP_TRY(svt_batched(ctx, w, Zn, prm, nullptr, X, true));                    // :22  X = svt(Y - Z/rho, tau/rho)
        hipLaunchKernelGGL(mc_admm_update_kernel, grid2((long long)nm, batch), dim3(256), 0, st, (long long)nm,
                           Y, Z, OH, invD, X, prm, Zn);                               // :24-26
        if (want_ce) {                                                                // :28
            hipLaunchKernelGGL(diff_kernel, dim3((unsigned)std::min<long long>((tot + 255) / 256, 4096)),
                               dim3(256), 0, st, tot, X, Htrue, D);
            JSTSP_TRY(sigma_max_sq(ctx, wn, D, num, true));
            hipLaunchKernelGGL(ratio_cap_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, batch, num, den,
                               ce, 0, (long long)Imax, (long long)it);
        }
    }
    JSTSP_HIP(hipGetLastError());
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(X_out), X, batch * nm, memspace));
    if (want_ce && Imax > 0) JSTSP_TRY(stage_out(ctx, ce_out, ce, (size_t)batch * Imax, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"

// Res = A' * Tc - RV,  P1 = GA * Res   (Gr x G2 per problem; N = Gr = 64, G2 a multiple of 64): the gradient step's 64-term
// products `K2'*k - R*v` (second factor) and the first factor of `R*res` (proposed_algorithm.m:47-48) in one launch
// (csrc/hsmall.hip: three-way split-f16 operands, float64 final sums).  Tc: N x G2 x batch; A: N x Gr (strideA 0 = shared); GA: Gr x Gr
// Hermitian (strideG 0 = shared); RV: Gr x G2 x batch or NULL.
extern "C" int jstsp_gradient_head_c32(jstsp_ctx *ctx, int N, int Gr, int G2, int batch, const jstsp_c32 *Tc_, const jstsp_c32 *A_,
                                       long long strideA, const jstsp_c32 *GA_, long long strideG, const jstsp_c32 *RV_,
                                       jstsp_c32 *Res_out, jstsp_c32 *P1_out, int memspace)
{
    JSTSP_TRY(check_common(ctx, memspace));
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(Tc_ && A_ && GA_ && Res_out && P1_out, JSTSP_E_NULL, "gradient_head: NULL array argument");
    JSTSP_REQUIRE(batch > 0 && grad_head_shape_ok(N, Gr, G2), JSTSP_E_UNSUPPORTED,
                  "gradient_head: N = %d, Gr = %d, G2 = %d (needs N = Gr = 64, G2 a multiple of 64)", N, Gr, G2);
    const size_t ng = (size_t)N * G2, g = (size_t)Gr * G2;
    const float2 *Tc, *A, *GA, *RV = nullptr;
    float2 *Res, *P1;
    JSTSP_TRY(arena_open(ctx, "gradient_head", [&](Arena &a) {
        Tc = a.in(as_f2(Tc_), batch * ng, memspace);
        A = a.in(as_f2(A_), dict_elems(strideA, (size_t)N * Gr, batch), memspace);
        GA = a.in(as_f2(GA_), dict_elems(strideG, (size_t)Gr * Gr, batch), memspace);
        if (RV_) RV = a.in(as_f2(RV_), batch * g, memspace);
        Res = a.get<float2>(batch * g); P1 = a.get<float2>(batch * g);
    }));
    JSTSP_TRY(launch_grad_head(ctx, G2, batch, Tc, (long long)ng, 0, 1, nullptr, nullptr, 0, A, strideA, GA, strideG, RV, nullptr, Res, P1, nullptr));
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(Res_out), Res, batch * g, memspace));
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(P1_out), P1, batch * g, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
