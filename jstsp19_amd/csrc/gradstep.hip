// Fused launches of the gradient step between two passes of proposed_algorithm (proposed_algorithm.m:47-48), taken only in the
// window behind a fused pass (proposed.hip: svt_split) at N = Gr = 64.  They remove launches and HBM round trips of the chain
//   partial sums -> Tc -> Res = A^H Tc - R v -> P1 = G_A Res -> RRes = P1 G_B -> step
// and change no rounding: every sum is formed by the same instructions on the same operands in the same order as in the
// launches they replace (JSTSP_FUSED=2 runs those; tests/test_gpu_gradstep.py compares the bits).
//
// grad_res_p1_kernel: Res = A^H Tc - R v and P1 = G_A Res (+ max|P1|) per (trial, 64 columns of G2) in ONE workgroup.  With
// N = Gr = 64 the 64 x 64 tile of Res that a workgroup of cgemm_kernel<64, ...> produces is the WHOLE k range of the second
// product for those columns: the tile goes to HBM once (the step needs it) and stays in LDS as the b panel of G_A Res, whose a
// operand (G_A, 32 KiB, shared by all tiles of a trial) is read from L2 straight into MFMA fragments.  Both products are the
// v_mfma_f32_32x32x2_f32 chains of cgemm_kernel<64, TAG, false, false, EPI_NONE>: k = 0..63 in pairs, per pair
// re += b_re a_re, im += b_re a_im, re += (-b_im) a_im, im += b_im a_re, MFMA A-op = b, B-op = a, accumulators from zero.
// Footprint: 33 280 bytes of LDS (that of cgemm_kernel<64>: four workgroups per CU alone, one beside two Gram workgroups),
// 256 threads; registers: DESIGN.md section 5.
#include "solver_common.h"

namespace jstsp {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int GK = 16;          // k rows of a staged panel
constexpr int GLD = 65;         // LDS row pitch of a 64-wide panel (transposing stores without bank conflicts)

__global__ __launch_bounds__(256) void grad_res_p1_kernel(const float2 *A, long long sAt, const float2 *Tc, const float2 *RV,
                                                          float2 *Res, const float2 *GA, long long sGAt, float2 *P1,
                                                          uint32_t *pmax, int G2, int batch)
{
    __shared__ float2 smem[4 * GK * GLD];       // product 1: [2][GK][GLD] a panels | [2][GK][GLD] b panels; product 2: Res tile [64][GLD]
    // same workgroup -> (trial, tile) map as cgemm: the tiles of a trial share A, G_A on one XCD's L2
    const int tiles = G2 / 64;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int t = (slot / tiles) * 8 + xcd;
    if (t >= batch) return;
    const int n0 = (slot % tiles) * 64;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave & 1, wj = wave >> 1, l31 = lane & 31, lhi = lane >> 5;
    const float2 *Ap = A + (long long)t * sAt;                                  // A[k + 64 i]: a(i, k) = conj(A[k, i])
    const long long cbase = (long long)t * 64 * G2 + 64ll * n0;                 // column n0 of this trial's 64 x G2 arrays
    const float2 *Tp = Tc + cbase;                                              // b(k, j) = Tc[k + 64 j]
    float2 *sA = smem, *sB = smem + 2 * GK * GLD;

    // panel element e = tid + 256 p: row/column e / 16, k = e % 16 (both sources are contiguous along k)
    const int pk = tid & 15, pr = tid >> 4;
    float2 ra[4], rb[4];
    auto gload = [&](int k0) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            ra[p] = Ap[k0 + pk + 64 * (pr + 16 * p)];
            rb[p] = Tp[k0 + pk + 64 * (pr + 16 * p)];
        }
    };
    auto sstore = [&](int buf) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            sA[buf * GK * GLD + pk * GLD + pr + 16 * p] = make_float2(ra[p].x, -ra[p].y);
            sB[buf * GK * GLD + pk * GLD + pr + 16 * p] = rb[p];
        }
    };

    f32x16 are, aim;
#pragma unroll
    for (int r = 0; r < 16; ++r) { are[r] = 0.f; aim[r] = 0.f; }

    // ---- product 1: A^H Tc, k = 0..63 in four double-buffered panels ---------------------------------------------------
    gload(0);
    sstore(0);
    __syncthreads();
    for (int kt = 0; kt < 64 / GK; ++kt) {
        const int buf = kt & 1;
        const bool refresh = kt + 1 < 64 / GK;
        if (refresh) gload((kt + 1) * GK);
        const float2 *a = sA + buf * GK * GLD + wi * 32 + l31;
        const float2 *bb = sB + buf * GK * GLD + wj * 32 + l31;
        float2 av = a[lhi * GLD], bv = bb[lhi * GLD];
#pragma unroll
        for (int kp = 0; kp < GK / 2; ++kp) {
            float2 an = av, bn = bv;
            if (kp + 1 < GK / 2) {
                const int kr = 2 * (kp + 1) + lhi;
                an = a[kr * GLD];
                bn = bb[kr * GLD];
            }
            are = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, av.x, are, 0, 0, 0);
            aim = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, av.y, aim, 0, 0, 0);
            are = __builtin_amdgcn_mfma_f32_32x32x2f32(-bv.y, av.y, are, 0, 0, 0);
            aim = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.y, av.x, aim, 0, 0, 0);
            av = an; bv = bn;
        }
        if (refresh) sstore(buf ^ 1);
        __syncthreads();
    }

    // ---- Res = A^H Tc - R v: to HBM, and into LDS as the b panel of the second product (row k = gi) ----------------------
    const int gi = wi * 32 + l31;
    // (the first G_A fragments are requested before the tile is exchanged: a(i, k) = G_A[i + 64 k], lane: k = 2 kp + lhi)
    const float2 *Gp = GA + (long long)t * sGAt + gi + 64 * lhi;
    float2 ga[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) ga[q] = Gp[128 * q];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int j = wj * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        const long long ix = cbase + gi + 64ll * j;
        const float2 dv = RV[ix];
        const float2 o = make_float2(are[r] - dv.x, aim[r] - dv.y);
        Res[ix] = o;
        smem[gi * GLD + j] = o;
        are[r] = 0.f; aim[r] = 0.f;
    }
    __syncthreads();

    // ---- product 2: P1 = G_A Res, k = 0..63 ------------------------------------------------------------------------------
    const float2 *rs = smem + wj * 32 + l31;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float2 gn[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) gn[q] = (c < 3) ? Gp[128 * (8 * (c + 1) + q)] : ga[q];
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int kp = 8 * c + q;
            const float2 av = ga[q], bv = rs[(2 * kp + lhi) * GLD];
            are = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, av.x, are, 0, 0, 0);
            aim = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, av.y, aim, 0, 0, 0);
            are = __builtin_amdgcn_mfma_f32_32x32x2f32(-bv.y, av.y, are, 0, 0, 0);
            aim = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.y, av.x, aim, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) ga[q] = gn[q];
    }
    float tmax = 0.f;           // max(|re|, |im|) of P1: the scale of the split-f16 G_B apply
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int j = wj * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        P1[cbase + gi + 64ll * j] = make_float2(are[r], aim[r]);
        tmax = fmaxf(tmax, fmaxf(fabsf(are[r]), fabsf(aim[r])));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tmax = fmaxf(tmax, __shfl_xor(tmax, o));
    if (lane == 0) atomicMax(&pmax[t], __float_as_uint(tmax));
}

// grad_refresh_p1_kernel: the first factor of the recomputation of R v, P1 = G_A,hi V + (G_A,lo V), per (trial, 64 columns of G2)
// in ONE workgroup instead of two launches of cgemm_kernel<64, ...> (P1 = G_A,lo V, then P1 = G_A,hi V + 1 * P1) between which
// P1 made an HBM round trip and V was read twice.  The 64 x 64 tile of V is the whole k range of both products: it is staged in
// LDS once, as the Res tile above is; the G_A fragments come from L2.  The two chains run one after the other from zero
// accumulators, each k = 0..63 in pairs in the order of the cgemm loop; the lo product, already an fp32 accumulator, is the beta
// term of the hi one: the cgemm epilogue forms 1 * acc + 1 * P1, which is the one rounding of acc + lo.  max|P1| is not formed
// (the fp64-master second factor of the recomputation takes no scale).  Footprint of grad_res_p1_kernel.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void grad_refresh_p1_kernel(const float2 *V, const float2 *GA, const float2 *GAlo, long long sGAt,
                                                              float2 *P1, int G2, int batch)
{
    __shared__ float2 smem[64 * GLD];           // V tile: b(k, j) at [k][j]
    const int tiles = G2 / 64;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int t = (slot / tiles) * 8 + xcd;
    if (t >= batch) return;
    const int n0 = (slot % tiles) * 64;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave & 1, wj = wave >> 1, l31 = lane & 31, lhi = lane >> 5;
    const long long cbase = (long long)t * 64 * G2 + 64ll * n0;                 // column n0 of this trial's 64 x G2 arrays
    const int gi = wi * 32 + l31;
    // a(i, k) = G[i + 64 k], lane: k = 2 kp + lhi; the first fragments of the lo factor are requested before the tile is staged
    const float2 *Gl = GAlo + (long long)t * sGAt + gi + 64 * lhi, *Gh = GA + (long long)t * sGAt + gi + 64 * lhi;
    float2 ga[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) ga[q] = Gl[128 * q];
    {
        // the tile is contiguous: element e = tid + 256 p is b(k = e % 64, j = e / 64)
        const float2 *Vp = V + cbase;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            float2 rv[8];
#pragma unroll
            for (int p = 0; p < 8; ++p) rv[p] = Vp[tid + 256 * (8 * h + p)];
#pragma unroll
            for (int p = 0; p < 8; ++p) smem[(tid & 63) * GLD + (tid >> 6) + 4 * (8 * h + p)] = rv[p];
        }
    }
    __syncthreads();

    const float2 *rs = smem + wj * 32 + l31 + lhi * GLD;
    f32x16 are, aim, lre, lim;
#pragma unroll
    for (int r = 0; r < 16; ++r) { are[r] = 0.f; aim[r] = 0.f; lre[r] = 0.f; lim[r] = 0.f; }
    // eight chunks of eight k pairs: 0..3 G_A,lo V, 4..7 G_A,hi V; the fragments of the next chunk are requested before the
    // MFMAs of this one (the last chunk requests its own again: no branch in the loop)
#pragma unroll 1
    for (int c = 0; c < 8; ++c) {
        const int cn = min(c + 1, 7);
        const float2 *Gn = ((cn < 4) ? Gl : Gh) + 1024 * (cn & 3);
        float2 gn[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) gn[q] = Gn[128 * q];
        if (c == 4) {                           // the lo product is complete: the hi chain starts from zero
            lre = are; lim = aim;
#pragma unroll
            for (int r = 0; r < 16; ++r) { are[r] = 0.f; aim[r] = 0.f; }
        }
        const float2 *rc = rs + 16 * GLD * (c & 3);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float2 av = ga[q], bv = rc[2 * q * GLD];
            are = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, av.x, are, 0, 0, 0);
            aim = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, av.y, aim, 0, 0, 0);
            are = __builtin_amdgcn_mfma_f32_32x32x2f32(-bv.y, av.y, are, 0, 0, 0);
            aim = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.y, av.x, aim, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) ga[q] = gn[q];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int j = wj * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        P1[cbase + gi + 64ll * j] = make_float2(are[r] + lre[r], aim[r] + lim[r]);
    }
}

}  // namespace

bool grad_fused_shape(int N, int Gr, int G2) { return N == 64 && Gr == 64 && G2 >= 64 && G2 % 64 == 0; }

int launch_grad_res_p1(jstsp_ctx *ctx, const float2 *A, long long sAt, const float2 *Tc, const float2 *RV, float2 *Res,
                       const float2 *GA, long long sGAt, float2 *P1, uint32_t *pmax, int G2, int batch)
{
    JSTSP_REQUIRE(G2 >= 64 && G2 % 64 == 0 && batch > 0 && pmax, JSTSP_E_ARG, "gradient step: fused Res / P1 launch at G2 = %d", G2);
    const long long grid = (long long)((batch + 7) / 8) * 8 * (G2 / 64);
    JSTSP_REQUIRE(grid < (1ll << 31), JSTSP_E_UNSUPPORTED, "gradient step: grid too large");
    hipLaunchKernelGGL(grad_res_p1_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, A, sAt, Tc, RV, Res, GA, sGAt, P1,
                       pmax, G2, batch);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

int launch_grad_refresh_p1(jstsp_ctx *ctx, const float2 *V, const float2 *GA, const float2 *GAlo, long long sGAt, float2 *P1, int G2,
                           int batch)
{
    JSTSP_REQUIRE(G2 >= 64 && G2 % 64 == 0 && batch > 0 && GA && GAlo, JSTSP_E_ARG, "gradient step: fused first factor of R v at G2 = %d", G2);
    const long long grid = (long long)((batch + 7) / 8) * 8 * (G2 / 64);
    JSTSP_REQUIRE(grid < (1ll << 31), JSTSP_E_UNSUPPORTED, "gradient step: grid too large");
    hipLaunchKernelGGL(grad_refresh_p1_kernel, dim3((unsigned)grid), dim3(256), 0, ctx->stream, V, GA, GAlo, sGAt, P1, G2, batch);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

}  // namespace jstsp
