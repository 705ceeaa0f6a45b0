// The state of a resumed fp32 proposed_algorithm call (jstsp_proposed_resume_c32, proposed.hip): streaming kernels that move one
// trial's block [X | V1 | V2 | C] (N M each) [v | S] (Gr G2 each) (include/jstsp.h: jstsp_admm_state_elems) to and from the
// solver's per-array batches, and the two corrections that let the loop's first iteration start from a state with C != -V2.
//
// The loop never stores C (common.h: after every iteration C == -V2).  C enters an iteration only through V2 + rho C (:38) and
// V2/rho + C (:43); :61-65 use V2 alone.  With D = C + V2 of the loaded state
//   b = [b with C = -V2] + rho D        -> the first X update reads subY + rho D in place of subY
//   k = [k with C = -V2] - D            -> K -= D after that update (the caller then takes max|K| again)
// and after the first iteration D = 0.  A state that is an iterate has D = 0 and both corrections are exact no-ops.
#include "solver_common.h"

namespace jstsp {
namespace {

inline dim3 rgrid(long long per, int batch) { return dim3((unsigned)std::max<long long>(1, std::min<long long>((per + 255) / 256, 1024)), batch); }

// explicit_c: Cb = C (the element-wise path keeps C); otherwise Cb = D and subY1 = subY + rho D (two-float rho, as the loop's own)
__global__ __launch_bounds__(256) void resume_unpack_kernel(long long nm, long long g, const float2 *state, float2 *X, float2 *V1, float2 *V2,
                                                            float2 *Cb, float2 *V, float2 *S, const float2 *subY, float2 *subY1,
                                                            const TrialParams *prm, int explicit_c)
{
    const long long t = blockIdx.y;
    const float2 *s = state + t * (4 * nm + 2 * g);
    const TrialParams p = prm[t];
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nm; e += (long long)gridDim.x * 256) {
        const float2 x = s[e], v1 = s[nm + e], v2 = s[2 * nm + e], c = s[3 * nm + e];
        const long long o = t * nm + e;
        X[o] = x; V1[o] = v1; V2[o] = v2;
        if (explicit_c) Cb[o] = c;
        else {
            const float2 d = make_float2(c.x + v2.x, c.y + v2.y), sy = subY[o];
            Cb[o] = d;
            subY1[o] = make_float2(sy.x + mul2(p.rho, p.rho_lo, d.x), sy.y + mul2(p.rho, p.rho_lo, d.y));
        }
    }
    s += 4 * nm;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < g; e += (long long)gridDim.x * 256) {
        V[t * g + e] = s[e]; S[t * g + e] = s[g + e];
    }
}

__global__ __launch_bounds__(256) void resume_fix_k_kernel(long long n, float2 *K, const float2 *D)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const float2 k = K[e], d = D[e];
        K[e] = make_float2(k.x - d.x, k.y - d.y);
    }
}

// Cb != NULL: C as the element-wise path computed it; NULL: C = -V2 (what the loop's updates make it)
__global__ __launch_bounds__(256) void resume_pack_kernel(long long nm, long long g, const float2 *X, const float2 *V1, const float2 *V2,
                                                          const float2 *Cb, const float2 *V, const float2 *S, float2 *state)
{
    const long long t = blockIdx.y;
    float2 *s = state + t * (4 * nm + 2 * g);
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nm; e += (long long)gridDim.x * 256) {
        const long long o = t * nm + e;
        const float2 v2 = V2[o];
        s[e] = X[o]; s[nm + e] = V1[o]; s[2 * nm + e] = v2;
        s[3 * nm + e] = Cb ? Cb[o] : make_float2(-v2.x, -v2.y);
    }
    s += 4 * nm;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < g; e += (long long)gridDim.x * 256) {
        s[e] = V[t * g + e]; s[g + e] = S[t * g + e];
    }
}

}  // namespace

int launch_resume_unpack(jstsp_ctx *ctx, long long nm, long long g, int batch, const float2 *state, float2 *X, float2 *V1, float2 *V2, float2 *Cb,
                         float2 *V, float2 *S, const float2 *subY, float2 *subY1, const TrialParams *prm, bool explicit_c)
{
    hipLaunchKernelGGL(resume_unpack_kernel, rgrid(nm, batch), dim3(256), 0, ctx->stream, nm, g, state, X, V1, V2, Cb, V, S, subY, subY1, prm,
                       explicit_c ? 1 : 0);
    JSTSP_HIP(hipGetLastError());
    return 0;
}
int launch_resume_fix_k(jstsp_ctx *ctx, long long n, float2 *K, const float2 *D)
{
    hipLaunchKernelGGL(resume_fix_k_kernel, dim3((unsigned)std::max<long long>(1, std::min<long long>((n + 255) / 256, 4096))), dim3(256), 0, ctx->stream, n, K, D);
    JSTSP_HIP(hipGetLastError());
    return 0;
}
int launch_resume_pack(jstsp_ctx *ctx, long long nm, long long g, int batch, const float2 *X, const float2 *V1, const float2 *V2, const float2 *Cb,
                       const float2 *V, const float2 *S, float2 *state)
{
    hipLaunchKernelGGL(resume_pack_kernel, rgrid(nm, batch), dim3(256), 0, ctx->stream, nm, g, X, V1, V2, Cb, V, S, state);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

}  // namespace jstsp
