// The stopping rule of jstsp_proposed_until_c32 (proposed.hip): small streaming kernels beside the fp32 ADMM
// loop, none of which touches an array the loop reads.  A trial stops after the first iteration k of the call with k >= min_iters
// and convergence_error(k, 3) <= tol[t] - the double step_v_kernel (admm.hip) has just written for it - and is CAPTURED at that
// iteration: its S, Y, packed state (resume.hip's layout) and order go to its place in the outputs, in two halves, because the
// fp32 loop holds X, V1 of an iteration only in front of the synthesis and V2 only behind it.  The trial itself runs on in the
// batch (no compaction); nothing it writes later is returned.
#include "solver_common.h"

namespace jstsp {
namespace {

__global__ __launch_bounds__(256) void until_init_kernel(int batch, int32_t *flag, int32_t *iters, double *ce3, uint32_t *ovf)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= batch) return;
    flag[t] = 0; iters[t] = 0; ce3[t] = 0.0; ovf[t] = 0u;
}

// One thread per trial.  `c <= tl` is false for a NaN on either side and for the Inf of iteration 1 from a zero state; tl > 0.
__global__ __launch_bounds__(256) void until_test_kernel(int batch, int k, int min_iters, int last, const double *ce, int Imax, int it,
                                                         const double *tol, const uint32_t *ovf_now, int32_t *flag, int32_t *iters,
                                                         double *ce3, uint32_t *ovf)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= batch) return;
    const int32_t f = flag[t];
    if (f == 1) flag[t] = 2;
    if (f != 0) return;
    const double c = ce[(long long)t * 3 * Imax + 2 * (long long)Imax + it], tl = tol[t];
    if (!(last || (k >= min_iters && tl > 0.0 && c <= tl))) return;
    flag[t] = 1; iters[t] = k; ce3[t] = c;
    ovf[t] = ovf_now ? ovf_now[t] : 0u;
}

__global__ __launch_bounds__(256) void until_capture_head_kernel(long long nm, long long g, int R, const int32_t *flag, const float2 *X,
                                                                 const float2 *V1, const float2 *Y, const float2 *V, const float2 *S,
                                                                 const int32_t *top, float2 *S_out, float2 *Y_out, float2 *state,
                                                                 int32_t *top_out)
{
    const long long t = blockIdx.y;
    if (flag[t] != 1) return;
    const long long e0 = (long long)blockIdx.x * 256 + threadIdx.x, step = (long long)gridDim.x * 256;
    float2 *s = state ? state + t * (4 * nm + 2 * g) : nullptr;
    for (long long e = e0; e < g; e += step) {
        const float2 sv = S[t * g + e];
        S_out[t * g + e] = sv;
        if (s) { s[4 * nm + e] = V[t * g + e]; s[4 * nm + g + e] = sv; }
    }
    if (Y_out)
        for (long long e = e0; e < nm; e += step) Y_out[t * nm + e] = Y[t * nm + e];
    if (s)
        for (long long e = e0; e < nm; e += step) { s[e] = X[t * nm + e]; s[nm + e] = V1[t * nm + e]; }
    if (top_out)
        for (long long e = e0; e < R; e += step) top_out[t * R + e] = top ? top[t * R + e] : 0;
}

__global__ __launch_bounds__(256) void until_capture_tail_kernel(long long nm, long long g, const int32_t *flag, const float2 *V2, const float2 *Cb,
                                                                 float2 *state)
{
    const long long t = blockIdx.y;
    if (flag[t] != 1) return;
    float2 *s = state + t * (4 * nm + 2 * g);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nm; e += (long long)gridDim.x * 256) {
        const float2 v2 = V2[t * nm + e];
        s[2 * nm + e] = v2;
        s[3 * nm + e] = Cb ? Cb[t * nm + e] : make_float2(-v2.x, -v2.y);
    }
}

__global__ __launch_bounds__(256) void until_count_kernel(int batch, const int32_t *flag, int32_t *left)
{
    int n = 0;
    for (int c = 0; c < batch; c += 256) n += __syncthreads_count(c + (int)threadIdx.x < batch && flag[c + threadIdx.x] == 0);
    if (threadIdx.x == 0) *left = n;
}

__global__ __launch_bounds__(256) void until_mask_ce_kernel(int Imax, const int32_t *iters, double *ce)
{
    const int t = blockIdx.y, k = iters[t];
    for (int e = blockIdx.x * 256 + threadIdx.x; e < 3 * Imax; e += gridDim.x * 256)
        if (e % Imax >= k) ce[(long long)t * 3 * Imax + e] = __builtin_nan("");
}

// (few workgroups per trial: in most iterations every one of them only reads its flag)
inline dim3 cgrid(long long per, int batch) { return dim3((unsigned)std::max<long long>(1, std::min<long long>((per + 255) / 256, 64)), batch); }

}  // namespace

int launch_until_init(jstsp_ctx *ctx, int batch, const UntilWS &u)
{
    hipLaunchKernelGGL(until_init_kernel, dim3((batch + 255) / 256), dim3(256), 0, ctx->stream, batch, u.flag, u.iters, u.ce3, u.ovf);
    JSTSP_HIP(hipGetLastError());
    return 0;
}
int launch_until_test(jstsp_ctx *ctx, int batch, int k, int min_iters, bool last, const double *ce, int Imax, int it, const uint32_t *ovf_now,
                      const UntilWS &u)
{
    hipLaunchKernelGGL(until_test_kernel, dim3((batch + 255) / 256), dim3(256), 0, ctx->stream, batch, k, min_iters, last ? 1 : 0, ce, Imax, it, u.tol,
                       ovf_now, u.flag, u.iters, u.ce3, u.ovf);
    JSTSP_HIP(hipGetLastError());
    return 0;
}
int launch_until_capture_head(jstsp_ctx *ctx, long long nm, long long g, int R, int batch, const float2 *X, const float2 *V1, const float2 *Y,
                              const float2 *V, const float2 *S, bool have_top, const UntilWS &u, float2 *state)
{
    hipLaunchKernelGGL(until_capture_head_kernel, cgrid(std::max(nm, g), batch), dim3(256), 0, ctx->stream, nm, g, R, u.flag, X, V1, Y, V, S,
                       have_top ? u.top_loop : (const int32_t *)nullptr, u.S, u.Y, state, u.top);
    JSTSP_HIP(hipGetLastError());
    return 0;
}
int launch_until_capture_tail(jstsp_ctx *ctx, long long nm, long long g, int batch, const float2 *V2, const float2 *Cb, const UntilWS &u, float2 *state)
{
    hipLaunchKernelGGL(until_capture_tail_kernel, cgrid(nm, batch), dim3(256), 0, ctx->stream, nm, g, u.flag, V2, Cb, state);
    JSTSP_HIP(hipGetLastError());
    return 0;
}
int launch_until_count(jstsp_ctx *ctx, int batch, const UntilWS &u)
{
    hipLaunchKernelGGL(until_count_kernel, dim3(1), dim3(256), 0, ctx->stream, batch, u.flag, u.left);
    JSTSP_HIP(hipGetLastError());
    return 0;
}
int launch_until_mask_ce(jstsp_ctx *ctx, int batch, int Imax, const UntilWS &u, double *ce)
{
    hipLaunchKernelGGL(until_mask_ce_kernel, dim3((unsigned)std::max(1, std::min((3 * Imax + 255) / 256, 64)), batch), dim3(256), 0, ctx->stream, Imax,
                       u.iters, ce);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

}  // namespace jstsp
