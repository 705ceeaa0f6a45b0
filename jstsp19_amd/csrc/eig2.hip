// Fast paths of the batched Hermitian eigen-solver for Gram matrices of order n <= 64
// (the SVT of benchmark_algorithms/svt.m:5-10 and the spectral norms of
// proposed_algorithm.m:67,69 at the BASELINE shapes).  One workgroup per matrix, everything in LDS.
//
//  * jacobi2_kernel<NE>: parallel-order two-sided Jacobi where each thread owns whole 2x2
//    blocks (pair a, pair b) of G and applies J_a^H . J_b to them in registers — one LDS
//    read + one write per element per round and two barriers per round (the general kernel
//    in eig.hip makes separate column and row passes).  (Measured and dropped: one barrier per
//    round with ping-pong LDS buffers and the two rotations recomputed by every thread — the
//    rounds are VALU/LDS-throughput bound, not barrier bound: 613 vs 463 us per launch.)  WARM START: the eigenvector basis of
//    the previous ADMM iteration is kept per problem; G' = U^H G U (two 64^3 complex GEMMs
//    on the fp32 MFMA, operands straight from LDS) is already nearly diagonal because the
//    ADMM iterates move slowly, so 2-3 sweeps replace 7-8.  Q = U diag(q) U^H is a third
//    in-LDS MFMA GEMM.
//  * lmax_kernel<NE>: lambda_max only — Householder tridiagonalisation (zhetd2-style) in LDS,
//    then 256-way multisection on the Sturm sequence of the real tridiagonal matrix.
#include "common.h"
#include <cstdlib>
#include <type_traits>

namespace jstsp {

typedef float f32x16 __attribute__((ext_vector_type(16)));

// C[i + ldc*j] = sum_k a(i,k) b(k,j) for an NE x NE x NE complex product with all operands in
// LDS.  a(i,k) = A[i*sAi + k*sAk] (conj if CA), b(k,j) = B[k*sBk + j*sBj] (conj if CB).
// Each wave computes 32 x 32 blocks; MFMA fed (A-op = b, B-op = a) so lanes hold consecutive i.
// If Cg != nullptr the result goes to global memory (ld = ldg) instead of LDS.
template <int NE, bool CA, bool CB>
__device__ __forceinline__ void lds_cgemm(const float2 *A, int sAi, int sAk, const float2 *B, int sBk,
                                          int sBj, float2 *C, int ldc, float2 *Cg, int ldg, int nvalid)
{
    constexpr int NBLK = (NE / 32) * (NE / 32);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int l31 = lane & 31, lhi = lane >> 5;
    const int nwaves = blockDim.x >> 6;
    for (int blk = wave; blk < NBLK; blk += nwaves) {
        const int i0 = (blk % (NE / 32)) * 32, j0 = (blk / (NE / 32)) * 32;
        f32x16 re, im;
#pragma unroll
        for (int r = 0; r < 16; ++r) { re[r] = 0.f; im[r] = 0.f; }
#pragma unroll 4
        for (int kp = 0; kp < NE / 2; ++kp) {
            const int k = 2 * kp + lhi;
            float2 av = A[(i0 + l31) * sAi + k * sAk];
            float2 bv = B[k * sBk + (j0 + l31) * sBj];
            if (CA) av.y = -av.y;
            if (CB) bv.y = -bv.y;
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, av.x, re, 0, 0, 0);
            re = __builtin_amdgcn_mfma_f32_32x32x2f32(-bv.y, av.y, re, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.x, av.y, im, 0, 0, 0);
            im = __builtin_amdgcn_mfma_f32_32x32x2f32(bv.y, av.x, im, 0, 0, 0);
        }
        const int i = i0 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int j = j0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
            if (Cg) {
                if (i < nvalid && j < nvalid) Cg[i + (size_t)ldg * j] = make_float2(re[r], im[r]);
            } else {
                C[i + ldc * j] = make_float2(re[r], im[r]);
            }
        }
    }
}

__device__ __forceinline__ void rr_pair2(int n, int s, int k, int &p, int &q)
{
    int a, b;
    if (k == 0) { a = n - 1; b = s; }
    else {
        a = s + k; if (a >= n - 1) a -= n - 1;
        b = s - k; if (b < 0) b += n - 1;
    }
    p = min(a, b);
    q = max(a, b);
}

__device__ __forceinline__ float2 cmulf(float2 a, float2 b)
{
    return make_float2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x);
}
__device__ __forceinline__ float2 cmulcf(float2 a, float2 b)   // conj(a) * b
{
    return make_float2(a.x * b.x + a.y * b.y, a.x * b.y - a.y * b.x);
}

template <int NE, int NT>
__global__ __launch_bounds__(NT) void jacobi2_kernel(int mode, int n, const float2 *Gpart, long long sGt,
                                                       int nsplit, long long sGs, const TrialParams *prm,
                                                       const float *tau, float2 *Q, float *lam_out,
                                                       float2 *Uwarm, int warm, float conv_tol, int max_sweeps,
                                                       int *sweep_stat, int fn_aware)
{
    constexpr int LD = NE + 1;
    constexpr int H = NE / 2;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2 *G = reinterpret_cast<float2 *>(smem_raw);       // [NE][LD] column-major
    float2 *U = G + NE * LD;
    float2 *T = U + NE * LD;
    float *rot = reinterpret_cast<float *>(T + NE * LD);    // [H][4]: c, wx, wy, (p | q<<16)
    float *red = rot + 4 * H;                               // [8]
    float *qv = red + 24;                                   // [NE]   (red: [0..3] scalars, [4..19] per-wave)
    const int t = blockIdx.x, tid = threadIdx.x;
    float2 *Uw = Uwarm ? Uwarm + (size_t)t * NE * NE : nullptr;

    // ---- load G (sum of split-K partials, zero padded), U (previous basis or identity) ------
    for (int e = tid; e < NE * NE; e += NT) {
        const int i = e % NE, j = e / NE;
        float2 g = make_float2(0.f, 0.f);
        if (i < n && j < n) {
            const float2 *src = Gpart + (long long)t * sGt + i + (long long)n * j;
            for (int s = 0; s < nsplit; ++s) {
                const float2 v = src[(long long)s * sGs];
                g.x += v.x; g.y += v.y;
            }
        }
        G[i + LD * j] = g;
        U[i + LD * j] = (warm && Uw) ? Uw[e] : make_float2(i == j ? 1.f : 0.f, 0.f);
    }
    __syncthreads();
    // Guard of svt.m:7-12: a singular value that is exactly 0 makes softThres NaN and the reference returns the ZERO
    // matrix.  The one input for which LAPACK's zero is exact on every platform is the all-zero matrix (the svt
    // argument of the first ADMM iteration): all-zero Gram => Q = I, i.e. Y = Z - Q Z = 0, without any sweep.
    // (A zero row in the middle of the input gives sigma_min ~ 1e-16, not 0, in LAPACK's gesdd — see DESIGN.md; such
    // components are simply removed by the threshold, as the oracle does.)
    if (mode == EIG_SVT_Q) {
        if (tid == 0) red[2] = 0.f;
        __syncthreads();
        for (int i = tid; i < n; i += NT)
            if (G[i + LD * i].x != 0.f) red[2] = 1.f;
        __syncthreads();
        if (red[2] == 0.f) {
            for (int e = tid; e < n * n; e += NT)
                Q[(size_t)t * n * n + e] = make_float2((e % n == e / n) ? 1.f : 0.f, 0.f);
            if (Uw && !warm)        // the caller treats the basis as valid from now on
                for (int e = tid; e < NE * NE; e += NT) Uw[e] = make_float2((e % NE == e / NE) ? 1.f : 0.f, 0.f);
            return;
        }
    }
    if (warm && Uw) {
        // G' = U^H (G U)
        lds_cgemm<NE, false, false>(G, 1, LD, U, 1, LD, T, LD, nullptr, 0, NE);
        __syncthreads();
        lds_cgemm<NE, true, false>(U, LD, 1, T, 1, LD, G, LD, nullptr, 0, NE);
        __syncthreads();
    }
    // Hermitian-symmetrise (MFMA products are Hermitian only up to rounding)
    for (int e = tid; e < NE * NE; e += NT) {
        const int i = e % NE, j = e / NE;
        if (i < j) {
            const float2 u = G[i + LD * j], l = G[j + LD * i];
            const float2 a = make_float2(0.5f * (u.x + l.x), 0.5f * (u.y - l.y));
            G[i + LD * j] = a;
            G[j + LD * i] = make_float2(a.x, -a.y);
        } else if (i == j) {
            G[i + LD * i].y = 0.f;
        }
    }
    __syncthreads();
    {
        float m = 0.f;
        for (int i = tid; i < NE; i += NT) m = fmaxf(m, fabsf(G[i + LD * i].x));
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) red[4 + (tid >> 6)] = m;
        __syncthreads();
        if (tid == 0) { float mm = red[4]; for (int wv = 1; wv < NT / 64; ++wv) mm = fmaxf(mm, red[4 + wv]); red[1] = mm; }
        __syncthreads();
    }
    const float dmax = red[1];
    // How far to diagonalise.  A coupling e_ij left between eigen-directions i and j changes f(G) = tau G^(-1/2)
    // (the projector when no singular value is clipped) by tau e_ij / (s_i s_j (s_i + s_j)), hence Q Z by
    // tau |e_ij| / (min(s_i, s_j) (s_i + s_j)) in one singular direction (first-order perturbation of a matrix
    // function: the divided difference of f).  Once that is below 2^-27 of ||Z||_2 = s_max >= sqrt(dmax) for every
    // pair - a quarter of an fp32 ulp of the data - further sweeps cannot change Y.  With the reference's
    // tau_Y = 1 / ||Y||_F^2 this is reached one to two sweeps before the plain tolerance.  The rule uses the levels a
    // sweep STARTED from (what it leaves is lower still) and needs them below 1e-2 in the plain measure too, so that
    // the diagonal entries it reads are eigenvalue estimates; a clipped spectrum (some s_i <= tau) keeps the plain rule.
    const float tv0 = (mode == EIG_SVT_Q && fn_aware) ? (tau ? tau[t] : prm[t].tauY_rho) : 0.f;
    const float fn_lim = 7.4505806e-9f * sqrtf(dmax);

    constexpr int NBLKS = H * H;                       // 2x2 blocks of G per round
    constexpr int BPT = (NBLKS + NT - 1) / NT;           // blocks per thread
    const int MAX_SWEEPS = max_sweeps;
    int sweeps_done = 0;
    for (int sweep = 0; sweep < MAX_SWEEPS; ++sweep) {
        // Function-aware rule on the matrix AS IT STANDS (round 3): the rule below learns the levels a sweep started from only
        // while rotating, i.e. it confirms convergence with one sweep that changes nothing Y can see.  One pass over the
        // off-diagonal entries (a hundredth of a sweep) measures the same two quantities before rotating: with a warm start
        // the basis of the previous ADMM iteration often already satisfies the rule (2.25 -> 1.3 sweeps per call at
        // BASELINE configs[1]).  Same thresholds, same guarantee; the plain rule keeps its start-of-sweep semantics.
        if (tv0 > 0.f) {
            if (tid == 0) { red[0] = 0.f; red[3] = 0.f; }
            __syncthreads();
            float cw = 0.f, cf = 0.f;
            for (int e = tid; e < NE * NE; e += NT) {
                const int p = e % NE, q = e / NE;
                if (p >= q) continue;
                const float a = G[p + LD * p].x, dd = G[q + LD * q].x;
                const float2 bq = G[p + LD * q];
                const float ab = __builtin_amdgcn_sqrtf(bq.x * bq.x + bq.y * bq.y);
                const float scale = __builtin_amdgcn_sqrtf(fabsf(a) * fabsf(dd));
                if (ab > 0.f && ab > 1e-8f * scale) {
                    cw = fmaxf(cw, ab * __builtin_amdgcn_rcpf(fmaxf(scale, 1e-3f * dmax)));
                    const float lo2 = fminf(a, dd);
                    cf = fmaxf(cf, (lo2 > tv0 * tv0) ? tv0 * ab * __builtin_amdgcn_rcpf(scale + lo2) : 3.0e38f);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { cw = fmaxf(cw, __shfl_xor(cw, o)); cf = fmaxf(cf, __shfl_xor(cf, o)); }
            if ((tid & 63) == 0) {
                atomicMax(reinterpret_cast<int *>(&red[0]), __float_as_int(cw));
                atomicMax(reinterpret_cast<int *>(&red[3]), __float_as_int(cf));
            }
            __syncthreads();
            const float w0 = red[0], f0 = red[3];
            __syncthreads();
            if (w0 < 1e-2f && f0 < fn_lim) break;
        }
        ++sweeps_done;
        if (tid == 0) { red[0] = 0.f; red[3] = 0.f; }
        float worst = 0.f, worst_fn = 0.f;
        for (int s = 0; s < NE - 1; ++s) {
            // -- rotation of each of the H disjoint pairs of this round
            if (tid < H) {
                int p, q;
                rr_pair2(NE, s, tid, p, q);
                const float a = G[p + LD * p].x, dd = G[q + LD * q].x;
                const float2 bq = G[p + LD * q];
                // hardware sqrt / rcp / rsq (1 ulp): the chain below is the serial part of a round; a rotation that is
                // unitary to 2 ulp instead of 1 costs the iteration nothing (Jacobi corrects itself)
                const float ab2 = bq.x * bq.x + bq.y * bq.y;
                const float ab = __builtin_amdgcn_sqrtf(ab2);
                float c = 1.f, wx = 0.f, wy = 0.f;
                const float scale = __builtin_amdgcn_sqrtf(fabsf(a) * fabsf(dd));
                if (ab > 0.f && ab > 1e-8f * scale) {
                    const float iab = __builtin_amdgcn_rcpf(ab);
                    worst = fmaxf(worst, ab * __builtin_amdgcn_rcpf(fmaxf(scale, 1e-3f * dmax)));
                    if (tv0 > 0.f) {       // min(s_i, s_j) (s_i + s_j) = s_i s_j + min(s_i, s_j)^2
                        const float lo2 = fminf(a, dd);
                        worst_fn = fmaxf(worst_fn, (lo2 > tv0 * tv0) ? tv0 * ab * __builtin_amdgcn_rcpf(scale + lo2) : 3.0e38f);
                    }
                    const float zeta = 0.5f * (dd - a) * iab;
                    const float tt = copysignf(__builtin_amdgcn_rcpf(fabsf(zeta) + __builtin_amdgcn_sqrtf(1.f + zeta * zeta)), zeta);
                    c = __builtin_amdgcn_rsqf(1.f + tt * tt);
                    const float sn = tt * c * iab;
                    wx = sn * bq.x;
                    wy = sn * bq.y;
                }
                rot[4 * tid + 0] = c; rot[4 * tid + 1] = wx; rot[4 * tid + 2] = wy;
                rot[4 * tid + 3] = __int_as_float(p | (q << 16));
            }
            __syncthreads();
            // -- G <- J^H G J on 2x2 blocks (pair a rows, pair b columns); U <- U J on 2 x 2 blocks
#pragma unroll
            for (int it = 0; it < BPT; ++it) {
                const int blk = tid + NT * it;
                if (NBLKS % NT != 0 && blk >= NBLKS) break;
                const int a = blk % H, b = blk / H;
                const float4 ra = *reinterpret_cast<const float4 *>(&rot[4 * a]);
                const float4 rb = *reinterpret_cast<const float4 *>(&rot[4 * b]);
                const int pa = __float_as_int(ra.w) & 0xffff, qa = __float_as_int(ra.w) >> 16;
                const int pb = __float_as_int(rb.w) & 0xffff, qb = __float_as_int(rb.w) >> 16;
                const float ca = ra.x, cb = rb.x;
                const float2 wa = make_float2(ra.y, ra.z), wb = make_float2(rb.y, rb.z);
                const bool ida = (ra.y == 0.f && ra.z == 0.f), idb = (rb.y == 0.f && rb.z == 0.f);
                // ---- G block
                if (!(ida && idb)) {
                    float2 gpp = G[pa + LD * pb], gpq = G[pa + LD * qb];
                    float2 gqp = G[qa + LD * pb], gqq = G[qa + LD * qb];
                    // right: [x_p, x_q] -> [c x_p - conj(w) x_q, w x_p + c x_q]   (columns pb, qb)
                    float2 t0 = cmulcf(wb, gpq), t1 = cmulf(wb, gpp);
                    float2 n_pp = make_float2(cb * gpp.x - t0.x, cb * gpp.y - t0.y);
                    float2 n_pq = make_float2(t1.x + cb * gpq.x, t1.y + cb * gpq.y);
                    t0 = cmulcf(wb, gqq); t1 = cmulf(wb, gqp);
                    float2 n_qp = make_float2(cb * gqp.x - t0.x, cb * gqp.y - t0.y);
                    float2 n_qq = make_float2(t1.x + cb * gqq.x, t1.y + cb * gqq.y);
                    // left: [y_p; y_q] -> [c y_p - w y_q; conj(w) y_p + c y_q]     (rows pa, qa)
                    t0 = cmulf(wa, n_qp); t1 = cmulcf(wa, n_pp);
                    gpp = make_float2(ca * n_pp.x - t0.x, ca * n_pp.y - t0.y);
                    gqp = make_float2(t1.x + ca * n_qp.x, t1.y + ca * n_qp.y);
                    t0 = cmulf(wa, n_qq); t1 = cmulcf(wa, n_pq);
                    gpq = make_float2(ca * n_pq.x - t0.x, ca * n_pq.y - t0.y);
                    gqq = make_float2(t1.x + ca * n_qq.x, t1.y + ca * n_qq.y);
                    if (a == b) {       // the annihilated block: exact zeros off the diagonal, real diagonal
                        gpq = make_float2(0.f, 0.f); gqp = make_float2(0.f, 0.f);
                        gpp.y = 0.f; gqq.y = 0.f;
                    }
                    G[pa + LD * pb] = gpp; G[pa + LD * qb] = gpq;
                    G[qa + LD * pb] = gqp; G[qa + LD * qb] = gqq;
                }
                // ---- U block: rows 2a, 2a+1; columns pb, qb
                if (!idb) {
                    const int r0 = 2 * a, r1 = 2 * a + 1;
                    const float2 u0p = U[r0 + LD * pb], u0q = U[r0 + LD * qb];
                    const float2 u1p = U[r1 + LD * pb], u1q = U[r1 + LD * qb];
                    float2 t0 = cmulcf(wb, u0q), t1 = cmulf(wb, u0p);
                    U[r0 + LD * pb] = make_float2(cb * u0p.x - t0.x, cb * u0p.y - t0.y);
                    U[r0 + LD * qb] = make_float2(t1.x + cb * u0q.x, t1.y + cb * u0q.y);
                    t0 = cmulcf(wb, u1q); t1 = cmulf(wb, u1p);
                    U[r1 + LD * pb] = make_float2(cb * u1p.x - t0.x, cb * u1p.y - t0.y);
                    U[r1 + LD * qb] = make_float2(t1.x + cb * u1q.x, t1.y + cb * u1q.y);
                }
            }
            __syncthreads();
        }
        if (tid < H) {
            atomicMax(reinterpret_cast<int *>(&red[0]), __float_as_int(worst));
            atomicMax(reinterpret_cast<int *>(&red[3]), __float_as_int(worst_fn));
        }
        __syncthreads();
        const float w = red[0], wf = red[3];
        __syncthreads();
        if (w < conv_tol || (tv0 > 0.f && w < 1e-2f && wf < fn_lim)) break;
    }

    if (sweep_stat && tid == 0) atomicAdd(sweep_stat, sweeps_done);
    if (mode == EIG_LMAX) {
        float m = -1e30f;
        for (int i = tid; i < n; i += NT) m = fmaxf(m, G[i + LD * i].x);
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((tid & 63) == 0) red[4 + (tid >> 6)] = m;
        __syncthreads();
        if (tid == 0) { float mm = red[4]; for (int wv = 1; wv < NT / 64; ++wv) mm = fmaxf(mm, red[4 + wv]); lam_out[t] = mm; }
        return;
    }
    // ---- Q = U diag(q) U^H, q_i = min(1, tau/sigma_i); keep U for the next warm start ----------
    const float tv = tau ? tau[t] : prm[t].tauY_rho;
    for (int i = tid; i < NE; i += NT) {
        const float sig = sqrtf(fmaxf(G[i + LD * i].x, 0.f));
        qv[i] = (sig > 0.f) ? fminf(1.f, tv / sig) : 1.f;
    }
    __syncthreads();
    for (int e = tid; e < NE * NE; e += NT) {
        const int i = e % NE, k = e / NE;
        const float2 u = U[i + LD * k];
        T[i + LD * k] = make_float2(u.x * qv[k], u.y * qv[k]);
        if (Uw) Uw[e] = u;
    }
    __syncthreads();
    // Q[i][j] = sum_k T[i][k] conj(U[j][k])
    lds_cgemm<NE, false, true>(T, 1, LD, U, LD, 1, nullptr, 0, Q + (size_t)t * n * n, n, n);
}

// ---------------------------------------------------------------------------------------------
// lambda_max by Householder tridiagonalisation + Sturm multisection.
template <int NE>
__global__ __launch_bounds__(256) void lmax_kernel(int n, const float2 *Gpart, long long sGt, int nsplit,
                                                    long long sGs, float *lam_out)
{
    constexpr int LD = NE + 1;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float2 *G = reinterpret_cast<float2 *>(smem_raw);       // [n][LD]
    float2 *v = G + NE * LD;                                // [NE]
    float2 *p = v + NE;                                     // [NE]
    float *d = reinterpret_cast<float *>(p + NE);           // [NE] diagonal
    float *e2 = d + NE;                                     // [NE] squared off-diagonal
    float *sc = e2 + NE;                                    // [16] scalars
    int *cnt = reinterpret_cast<int *>(sc + 16);            // [256]
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63;

    for (int e = tid; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        const float2 *src = Gpart + (long long)t * sGt + e;
        float2 g = make_float2(0.f, 0.f);
        for (int s = 0; s < nsplit; ++s) {
            const float2 x = src[(long long)s * sGs];
            g.x += x.x; g.y += x.y;
        }
        G[i + LD * j] = g;
    }
    __syncthreads();
    for (int e = tid; e < n * n; e += 256) {       // symmetrise
        const int i = e % n, j = e / n;
        if (i < j) {
            const float2 u = G[i + LD * j], l = G[j + LD * i];
            const float2 a = make_float2(0.5f * (u.x + l.x), 0.5f * (u.y - l.y));
            G[i + LD * j] = a;
            G[j + LD * i] = make_float2(a.x, -a.y);
        } else if (i == j) G[i + LD * i].y = 0.f;
    }
    __syncthreads();

    for (int k = 0; k + 1 < n; ++k) {
        const int m0 = k + 1;                      // active block rows/cols m0 .. n-1
        // (1) reflector for column k below the diagonal (wave 0)
        if (tid < 64) {
            float ss = 0.f;
            for (int i = m0 + 1 + lane; i < n; i += 64) {
                const float2 x = G[i + LD * k];
                ss += x.x * x.x + x.y * x.y;
            }
            for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
            const float2 alpha = G[m0 + LD * k];
            float beta, taur, taui;
            float2 scal;
            if (ss == 0.f && alpha.y == 0.f) {      // nothing to annihilate: H = I
                beta = alpha.x; taur = 0.f; taui = 0.f; scal = make_float2(0.f, 0.f);
            } else {
                const float nrm = sqrtf(alpha.x * alpha.x + alpha.y * alpha.y + ss);
                beta = (alpha.x >= 0.f) ? -nrm : nrm;
                taur = (beta - alpha.x) / beta;
                taui = -alpha.y / beta;
                const float dr = alpha.x - beta, di = alpha.y, den = dr * dr + di * di;
                scal = make_float2(dr / den, -di / den);          // 1/(alpha - beta)
            }
            for (int i = m0 + lane; i < n; i += 64) {
                float2 x = G[i + LD * k];
                v[i] = (i == m0) ? make_float2(1.f, 0.f) : cmulf(x, scal);
            }
            if (lane == 0) {
                d[k] = G[k + LD * k].x;
                e2[k] = beta * beta;
                sc[0] = taur; sc[1] = taui;
            }
        }
        __syncthreads();
        const float2 tauc = make_float2(sc[0], sc[1]);
        const int m = n - m0;
        if (tauc.x != 0.f || tauc.y != 0.f) {
            // (2) p = tau * A v  (A = G[m0:, m0:]); 4 lanes per row, shuffle-reduced
            for (int base = 0; base < m; base += 64) {
                const int i = m0 + base + (tid >> 2), c = tid & 3;
                float2 acc = make_float2(0.f, 0.f);
                if (i < n)
                    for (int j = m0 + c; j < n; j += 4) {
                        const float2 g = G[i + LD * j], vj = v[j];
                        acc.x += g.x * vj.x - g.y * vj.y;
                        acc.y += g.x * vj.y + g.y * vj.x;
                    }
                acc.x += __shfl_xor(acc.x, 1); acc.y += __shfl_xor(acc.y, 1);
                acc.x += __shfl_xor(acc.x, 2); acc.y += __shfl_xor(acc.y, 2);
                if (c == 0 && i < n) p[i] = cmulf(tauc, acc);
            }
            __syncthreads();
            // (3) w = p - (tau/2)(p^H v) v   (wave 0)
            if (tid < 64) {
                float2 dot = make_float2(0.f, 0.f);
                for (int i = m0 + lane; i < n; i += 64) {
                    const float2 c = cmulcf(p[i], v[i]);
                    dot.x += c.x; dot.y += c.y;
                }
                for (int o = 32; o > 0; o >>= 1) { dot.x += __shfl_xor(dot.x, o); dot.y += __shfl_xor(dot.y, o); }
                const float2 f = cmulf(make_float2(0.5f * tauc.x, 0.5f * tauc.y), dot);
                for (int i = m0 + lane; i < n; i += 64) {
                    const float2 fv = cmulf(f, v[i]);
                    p[i] = make_float2(p[i].x - fv.x, p[i].y - fv.y);
                }
            }
            __syncthreads();
            // (4) A <- A - v w^H - w v^H
            for (int e = tid; e < m * m; e += 256) {
                const int i = m0 + e % m, j = m0 + e / m;
                const float2 vi = v[i], wi = p[i], vj = v[j], wj = p[j];
                float2 g = G[i + LD * j];
                // v_i conj(w_j) + w_i conj(v_j)
                g.x -= (vi.x * wj.x + vi.y * wj.y) + (wi.x * vj.x + wi.y * vj.y);
                g.y -= (vi.y * wj.x - vi.x * wj.y) + (wi.y * vj.x - wi.x * vj.y);
                G[i + LD * j] = g;
            }
            __syncthreads();
        }
    }
    if (tid == 0) { d[n - 1] = G[(n - 1) + LD * (n - 1)].x; e2[n - 1] = 0.f; }
    __syncthreads();

    // ---- Gershgorin bounds, then multisection for the largest eigenvalue ------------------------
    if (tid < 64) {
        float lo = 1e30f, hi = -1e30f;
        for (int i = lane; i < n; i += 64) {
            const float r = (i > 0 ? sqrtf(e2[i - 1]) : 0.f) + (i + 1 < n ? sqrtf(e2[i]) : 0.f);
            lo = fminf(lo, d[i] - r);
            hi = fmaxf(hi, d[i] + r);
        }
        for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o)); hi = fmaxf(hi, __shfl_xor(hi, o)); }
        if (lane == 0) { sc[2] = lo; sc[3] = hi; }
    }
    __syncthreads();
    float lo = sc[2], hi = sc[3];
    const float span0 = fmaxf(hi - lo, 1e-30f);
    hi += 1e-6f * span0 + 1e-30f;
    for (int round = 0; round < 5; ++round) {
        // candidate x_j = lo + (j+1) (hi-lo)/257 ; count(x) = #eigenvalues < x ; lambda_max in (x_j, x_{j+1}]
        const float step = (hi - lo) / 257.f;
        const float x = lo + (tid + 1) * step;
        int c = 0;
        float q = 1.f;
        for (int i = 0; i < n; ++i) {
            q = d[i] - x - (i > 0 ? e2[i - 1] / q : 0.f);
            if (fabsf(q) < 1e-30f) q = -1e-30f;
            c += (q < 0.f);
        }
        cnt[tid] = c;
        __syncthreads();
        // largest j with count(x_j) < n  => lambda_max > ... ; find first j with count == n
        if (tid == 0) {
            int first = 256;
            for (int j = 0; j < 256; ++j) if (cnt[j] >= n) { first = j; break; }
            sc[4] = lo + first * step;                    // count < n at this point (or lo)
            sc[5] = (first < 256) ? lo + (first + 1) * step : hi;
        }
        __syncthreads();
        lo = sc[4]; hi = sc[5];
        __syncthreads();
    }
    if (tid == 0) lam_out[t] = 0.5f * (lo + hi);
}


// ---------------------------------------------------------------------------------------------
// lambda_max by Lanczos tridiagonalisation (Paige's ordering: u = G v - beta v_prev; alpha = <v, u>; u -= alpha v),
// FOUR WAVES per matrix and one barrier per step: every wave keeps the whole Lanczos vectors (lane i owns component
// i, and i + 64 for orders above 64) and a quarter of the columns of G in registers; a step is a register mat-vec
// over the wave's columns (v_k broadcast by v_readlane), an exchange of the four partial products through a
// double-buffered 4 KiB of LDS, and two wave reductions that every wave repeats identically (same operands, same
// order: the copies of v stay bitwise equal).
//
// COLD (no warm-start record, or no usable vector in it): n steps from a generic start vector (or until the Krylov space is
// exhausted) without reorthogonalisation: the largest Ritz value converges first and stays converged (ghost copies do not
// move it); measured against float64 on Gram matrices with flat, clustered, graded (1e-8) and structured low-rank spectra:
// <= 1.5e-6 relative, typically 1e-7.  Largest eigenvalue of the tridiagonal matrix by 256-way multisection on the Sturm count.
//
// WARM (round 5; the convergence_error norms of proposed_algorithm.m:67,69 and sparse_admm.m:32 / mc_admm.m:28 ask for
// lambda_max of matrices that barely move from one ADMM iteration to the next): the Ritz vector of the previous call is the
// start vector.  Phase 0 runs at most LZ_KMAX steps from it; after each step from the LZ_KMIN-th on, wave 0 takes the top
// Ritz pair (theta, y) of the small tridiagonal T_m (64-way multisection, then the eigenvector by the twisted factorisation
// of T_m - theta I: both recurrences run in their stable direction) and stops when the residual of the Ritz pair,
// ||G x - theta x|| = beta_m |y_m|, is below tol * theta (1e-5: the eigenvalue itself is then right to
// min(res, res^2 / gap), i.e. to fp32 resolution for every gap above 1e-3); the new Ritz vector x = sum_i y_i v_i comes from
// the m start-up vectors wave 0 kept in LDS.  If phase 0 does not converge the matrix is done COLD (phase 1: generic start,
// n steps, multisection - exactly the cold path) and a fresh Ritz vector is formed for the next call: y from the twisted
// factorisation of the full T_m (wave 0, serial), then the SAME recurrence is run once more (phase 2: same code, same bits)
// accumulating x = sum_j y_j v_j - no n x n basis is ever stored.
// A residual test cannot tell the largest eigenpair from another one, and a vector that tracked the largest eigenvalue
// through an exact crossing would keep following the wrong branch.  So every `vperiod`-th call a converged phase 0 is
// followed by the cold phase 1 anyway: its value is the one returned, a relative difference above 2e-5 counts as a mismatch
// (device counter, reported per solve) and replaces the vector.  ALL matrices of a launch are verified in the same call: a
// launch lasts as long as its slowest workgroup, and a cold run is 12 x a warm one - staggering the verifications over the
// matrices (the first version) put a few cold workgroups into EVERY launch and the kernel took as long as before
// (profiles/r05a_kernel_stats.csv: 280 us average with 5 Lanczos steps per matrix instead of 64).
// NW waves per matrix (4: lowest latency - the default of rounds 1-2; 1: no exchange, no barrier, no redundant reductions -
// a quarter of the instructions per matrix at four times the latency)
constexpr int LZ_KMAX = 12, LZ_KMIN = 3;
// Order 128 (sparse_admm's and mc_admm's error curves): 4 % of the warm attempts did not reach the residual in 12 steps and
// fell back to the cold 128-step run - 40 of the 1024 workgroups of a launch, which then lasts as long as they do (0.60 ms
// against 4.0 steps per matrix on average).  More room for the warm attempt there.
template <int NE> struct LzKmax { static constexpr int value = NE > 64 ? 32 : LZ_KMAX; };

__device__ __forceinline__ float lz_guard(float d) { return fabsf(d) < 1e-30f ? (d < 0.f ? -1e-30f : 1e-30f) : d; }

// Largest eigenvalue of the m x m tridiagonal matrix (diagonal sd[0..m-1], squared off-diagonals se[0..m-2]) by ONE wave:
// five rounds of 64-way multisection on the Sturm count between max(diag) and the Gershgorin bound.
__device__ __forceinline__ float lz_top_small(const float *sd, const float *se, int m, int lane)
{
    float lo = sd[0], hi = -3.0e38f;
    for (int i = 0; i < m; ++i) {
        const float r = (i > 0 ? sqrtf(se[i - 1]) : 0.f) + (i + 1 < m ? sqrtf(se[i]) : 0.f);
        lo = fmaxf(lo, sd[i]);
        hi = fmaxf(hi, sd[i] + r);
    }
    const float span0 = fmaxf(hi - lo, 1e-30f);
    lo -= 1e-6f * fabsf(lo) + 1e-30f;           // count(lo) < m strictly
    hi += 1e-6f * span0 + 1e-30f;
    for (int round = 0; round < 5; ++round) {
        const float step = (hi - lo) / 65.f;
        const float x = lo + (lane + 1) * step;
        float q = 1.f, eprev = 0.f;
        int c = 0;
        for (int i = 0; i < m; ++i) {
            q = (sd[i] - x) - eprev * __builtin_amdgcn_rcpf(q);
            if (fabsf(q) < 1e-30f) q = -1e-30f;
            c += (q < 0.f);
            eprev = se[i];
        }
        const unsigned long long full = __ballot(c >= m);
        const int first = full ? (int)__ffsll((long long)full) - 1 : 64;
        const float nlo = lo + first * step;
        const float nhi = (first < 64) ? lo + (first + 1) * step : hi;
        lo = nlo; hi = nhi;
    }
    return 0.5f * (lo + hi);
}

// Eigenvector of the m x m tridiagonal matrix for the (approximate) eigenvalue th by the twisted factorisation of T - th I:
// pivots of the factorisation from the top (sdp) and from the bottom (sdm), the twist index r where |gamma_r| is smallest,
// then y_r = 1 and both recurrences away from r.  Every lane of the calling wave runs the same serial code (uniform LDS
// addresses); y goes to sy[0..m-1] UNNORMALISED, the return value is ||y||^2.
__device__ __forceinline__ float lz_twisted(const float *sd, const float *se, int m, float th, float *sdp, float *sdm, float *sy)
{
    float dp = sd[0] - th;
    sdp[0] = dp;
    for (int i = 1; i < m; ++i) {
        dp = (sd[i] - th) - se[i - 1] * __builtin_amdgcn_rcpf(lz_guard(dp));
        sdp[i] = dp;
    }
    float dm = sd[m - 1] - th;
    sdm[m - 1] = dm;
    for (int i = m - 2; i >= 0; --i) {
        dm = (sd[i] - th) - se[i] * __builtin_amdgcn_rcpf(lz_guard(dm));
        sdm[i] = dm;
    }
    int r = 0;
    float best = 3.0e38f;
    for (int i = 0; i < m; ++i) {
        const float g = fabsf(sdp[i] + sdm[i] - (sd[i] - th));
        if (g < best) { best = g; r = i; }
    }
    float y = 1.f, nrm = 1.f;
    sy[r] = 1.f;
    for (int i = r; i + 1 < m; ++i) {
        y = -sqrtf(se[i]) * y * __builtin_amdgcn_rcpf(lz_guard(sdm[i + 1]));
        sy[i + 1] = y;
        nrm += y * y;
    }
    y = 1.f;
    for (int i = r; i > 0; --i) {
        y = -sqrtf(se[i - 1]) * y * __builtin_amdgcn_rcpf(lz_guard(sdp[i - 1]));
        sy[i - 1] = y;
        nrm += y * y;
    }
    return nrm;
}

template <int NE, int NW, int OCC>
__global__ __launch_bounds__(64 * NW, OCC) void lanczos_lmax_kernel(int n, const float2 *Gpart, long long sGt, int nsplit,
                                                           long long sGs, float *lam_out, float2 *wx, int *wst,
                                                           unsigned *wmis, int call, int vperiod, float tol)
{
    constexpr int R = NE / 64;              // components per lane
    constexpr int KW = NE / NW;             // columns of G per wave
    constexpr int NT = 64 * NW;
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    // LDS: the exchange of the partial products, the tridiagonal matrix, and (warm start) the first LZ_KMAX Lanczos vectors
    // (round 3: the matrix itself is no longer staged here - 33 KiB per workgroup for the kernel's whole life kept
    // eigen-decomposition workgroups, 101 KiB, off the CU)
    float2 *part = reinterpret_cast<float2 *>(smem_raw);       // [2][NW waves][NE] partial products
    int *sflag = reinterpret_cast<int *>(part + 2 * NW * NE);   // [2]: wave 0's verdict on step j, slot j & 1
    float *sd = reinterpret_cast<float *>(sflag + 4);          // [NE] d, [NE] e2, then [2][4] firsts, m, ...
    float *se = sd + NE;
    int *sfirst = reinterpret_cast<int *>(se + NE);             // [12]
    float *sy = reinterpret_cast<float *>(sfirst + 12);         // [NE] eigenvector of T
    float *sdp = sy + NE, *sdm = sdp + NE;                      // [NE] each: pivots of the twisted factorisation
    float *sres = sdm + NE;                                     // [4]
    float2 *vb = reinterpret_cast<float2 *>(sres + 4);          // [LZ_KMAX][NE] start-up vectors of phase 0 (wave 0's copy)
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    // this wave's columns straight from memory: lane i owns row i (coalesced), the split-K partials summed on the way.
    // (The Gram is Hermitian up to the rounding of its MFMA sums, 1e-7 relative: its stored entries are used as they are.)
    float2 grow[KW * R];
    const int kbase = wave * KW;
#pragma unroll
    for (int kk = 0; kk < KW; ++kk)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r, k = kbase + kk;
            float2 g = make_float2(0.f, 0.f);
            if (i < n && k < n) {
                const float2 *src = Gpart + (long long)t * sGt + i + (long long)n * k;
                for (int s = 0; s < nsplit; ++s) {
                    const float2 x = src[(long long)s * sGs];
                    g.x += x.x; g.y += x.y;
                }
                if (i == k) g.y = 0.f;
            }
            grow[kk * R + r] = g;
        }

    auto bcast = [](float x, int k) {       // k is wave-uniform
        return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), k));
    };
    // wave-wide sum on the DPP path (four row-local adds + four v_readlane): a butterfly of __shfl_xor costs six
    // dependent ds_bpermute round trips, which was two thirds of a Lanczos step
    auto wsum = [&](float x) {
        auto dpp = [](float y, auto ctrl) {
            return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, y), decltype(ctrl)::value,
                                                                         0xf, 0xf, true));
        };
        x += dpp(x, std::integral_constant<int, 0xB1>{});       // quad_perm [1,0,3,2]
        x += dpp(x, std::integral_constant<int, 0x4E>{});       // quad_perm [2,3,0,1]
        x += dpp(x, std::integral_constant<int, 0x124>{});      // row_ror 4
        x += dpp(x, std::integral_constant<int, 0x128>{});      // row_ror 8: every lane holds its row's sum
        return (bcast(x, 0) + bcast(x, 16)) + (bcast(x, 32) + bcast(x, 48));
    };

    // phase 0: warm attempt; 1: cold run (generic start vector, n steps); 2: the cold recurrence once more for its Ritz vector.
    // Every decision below is uniform over the workgroup: kernel arguments, one global word read by all, or LDS words
    // written by wave 0 and read behind a barrier.
    const bool warm_on = wx != nullptr;
    int phase = 1;
    if (warm_on && wst[t] == 1) phase = 0;
    const bool verify = warm_on && vperiod > 0 && (call % vperiod == vperiod - 1);      // (all matrices of a launch together: see above)
    bool have_w = false;
    float theta_w = 0.f;
    int m = 0, mcold = 0;
    float2 v[R], vp[R], u[R];
    for (;;) {
        // start vector: the previous call's Ritz vector, or a generic one (no structured eigenvector is orthogonal to it)
        float nrm = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = lane + 64 * r;
            const float fi = (float)i;
            if (phase == 0) v[r] = (i < n) ? wx[(long long)t * NE + i] : make_float2(0.f, 0.f);
            else v[r] = (i < n) ? make_float2(cosf(0.7f + 1.37f * fi + 0.011f * fi * fi), sinf(0.3f + 2.11f * fi))
                                : make_float2(0.f, 0.f);
            vp[r] = make_float2(0.f, 0.f);
            if (phase == 2 && wave == 0) vb[lane + 64 * r] = make_float2(0.f, 0.f);     // x accumulates here (wave 0's own words)
            nrm += v[r].x * v[r].x + v[r].y * v[r].y;
        }
        {
            const float inv = 1.f / sqrtf(wsum(nrm));
#pragma unroll
            for (int r = 0; r < R; ++r) { v[r].x *= inv; v[r].y *= inv; }
        }
        float beta = 0.f, scale = 0.f;
        m = 0;
        const int jmax = (phase == 0) ? min(LzKmax<NE>::value, n) : (phase == 2 ? mcold : n);
        __syncthreads();                    // the LDS words of the previous phase are free (and sy of phase 1 is visible)
        for (int j = 0; j < jmax; ++j) {
            if (phase == 0 && wave == 0) {
#pragma unroll
                for (int r = 0; r < R; ++r) vb[j * NE + lane + 64 * r] = v[r];
            }
            if (phase == 2 && wave == 0) {
                const float yj = sy[j];
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    float2 xa = vb[lane + 64 * r];
                    xa.x = fmaf(yj, v[r].x, xa.x); xa.y = fmaf(yj, v[r].y, xa.y);
                    vb[lane + 64 * r] = xa;
                }
            }
            // partial product over this wave's columns (two independent chains per component)
            float px[R][2], py[R][2];
#pragma unroll
            for (int r = 0; r < R; ++r) { px[r][0] = px[r][1] = 0.f; py[r][0] = py[r][1] = 0.f; }
#pragma unroll
            for (int kk = 0; kk < KW; ++kk) {
                const int k = kbase + kk;                                   // wave-uniform; (k >> 6) selects the register
                const float vx = (R == 1 || k < 64) ? bcast(v[0].x, k & 63) : bcast(v[R - 1].x, k & 63);
                const float vy = (R == 1 || k < 64) ? bcast(v[0].y, k & 63) : bcast(v[R - 1].y, k & 63);
#pragma unroll
                for (int r = 0; r < R; ++r) {
                    const float2 g = grow[kk * R + r];
                    px[r][kk & 1] = fmaf(g.x, vx, px[r][kk & 1]);
                    py[r][kk & 1] = fmaf(g.x, vy, py[r][kk & 1]);
                    px[r][kk & 1] = fmaf(-g.y, vy, px[r][kk & 1]);
                    py[r][kk & 1] = fmaf(g.y, vx, py[r][kk & 1]);
                }
            }
            float2 *pw = part + (j & 1) * NW * NE;
            if constexpr (NW > 1) {
#pragma unroll
                for (int r = 0; r < R; ++r)
                    pw[wave * NE + lane + 64 * r] = make_float2(px[r][0] + px[r][1], py[r][0] + py[r][1]);
                __syncthreads();
            }
            // The ONLY data-dependent exit: wave 0's verdict on the previous step, read by every wave from one LDS word behind
            // the barrier above - the number of barriers each wave executes cannot differ, whatever the four waves' redundant
            // arithmetic does (round 2 relied on it being bitwise identical; the step computed in between is discarded).
            if (j > 0 && sflag[(j - 1) & 1]) break;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r;
                float2 ps;
                if constexpr (NW == 4) {
                    const float2 p0 = pw[i], p1 = pw[NE + i], p2 = pw[2 * NE + i], p3 = pw[3 * NE + i];
                    ps = make_float2((p0.x + p1.x) + (p2.x + p3.x), (p0.y + p1.y) + (p2.y + p3.y));
                } else if constexpr (NW == 2) {
                    const float2 p0 = pw[i], p1 = pw[NE + i];
                    ps = make_float2(p0.x + p1.x, p0.y + p1.y);
                } else {
                    ps = make_float2(px[r][0] + px[r][1], py[r][0] + py[r][1]);
                }
                u[r] = make_float2(ps.x - beta * vp[r].x, ps.y - beta * vp[r].y);
            }
            float a = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) a += v[r].x * u[r].x + v[r].y * u[r].y;
            const float alpha = wsum(a);
            float b2 = 0.f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                u[r].x -= alpha * v[r].x; u[r].y -= alpha * v[r].y;
                b2 += u[r].x * u[r].x + u[r].y * u[r].y;
            }
            const float bb = wsum(b2);
            const float bnew = sqrtf(bb);
            scale = fmaxf(scale, fabsf(alpha) + beta + bnew);
            const bool last = (j == n - 1) || !(bnew > 4e-7f * scale);      // Krylov space exhausted (also catches NaN)
            // T_m: diagonal sd[0..m-1], squared off-diagonals se[0..m-2]; se[m-1] is the outgoing beta^2 (not part of T_m)
            if (wave == 0) { sd[j] = alpha; se[j] = bb; }
            m = j + 1;
            int flag = last ? 1 : 0;        // 1: tridiagonalisation complete, 2: phase 0 converged, 3: phase 0 gave up
            if (phase == 0 && wave == 0 && !last) {
                if (m >= LZ_KMIN) {
                    const float th = lz_top_small(sd, se, m, lane);
                    const float ny = lz_twisted(sd, se, m, th, sdp, sdm, sy);
                    const float res = bnew * fabsf(sy[m - 1]) * __builtin_amdgcn_rsqf(ny);   // ||G x - theta x||
                    if (res <= tol * th) { flag = 2; if (lane == 0) { sres[0] = th; sres[1] = ny; } }      // (NaN: false)
                }
                if (flag == 0 && m == jmax) flag = 3;
            }
            if (wave == 0 && lane == 0) sflag[j & 1] = flag;
            if (j + 1 == jmax) break;
            const float ib = 1.f / bnew;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                vp[r] = v[r];
                v[r] = make_float2(u[r].x * ib, u[r].y * ib);
            }
            beta = bnew;
        }
        __syncthreads();
        const int fin = m > 0 ? sflag[(m - 1) & 1] : 1;

        if (phase == 0) {
            if (fin == 2) {
                theta_w = sres[0];
                have_w = true;
                if (wave == 0) {            // x = sum_i y_i v_i from the start-up vectors; y (unnormalised) is still in sy
                    const float iny = __builtin_amdgcn_rsqf(sres[1]);
                    float2 x[R];
                    float nx = 0.f;
#pragma unroll
                    for (int r = 0; r < R; ++r) {
                        x[r] = make_float2(0.f, 0.f);
                        for (int i = 0; i < m; ++i) {
                            const float yi = sy[i] * iny;
                            const float2 vi = vb[i * NE + lane + 64 * r];
                            x[r].x = fmaf(yi, vi.x, x[r].x); x[r].y = fmaf(yi, vi.y, x[r].y);
                        }
                        nx += x[r].x * x[r].x + x[r].y * x[r].y;
                    }
                    const float inx = __builtin_amdgcn_rsqf(wsum(nx));
#pragma unroll
                    for (int r = 0; r < R; ++r) wx[(long long)t * NE + lane + 64 * r] = make_float2(x[r].x * inx, x[r].y * inx);
                }
                if (tid == 0 && wmis) atomicAdd(wmis + 3, (unsigned)m);               // [3] steps of converged warm attempts
                if (!verify) {
                    if (tid == 0) lam_out[t] = theta_w;
                    return;
                }
            }
            if (tid == 0 && wmis) { atomicAdd(wmis + (fin == 2 ? 2 : 1), 1u); }      // [2] verifications, [1] warm attempts that failed
            phase = 1;                      // not converged (or due for verification): the cold run
            continue;
        }
        if (phase == 2) {
            if (wave == 0) {
                float2 xacc[R];
                float nx = 0.f;
#pragma unroll
                for (int r = 0; r < R; ++r) { xacc[r] = vb[lane + 64 * r]; nx += xacc[r].x * xacc[r].x + xacc[r].y * xacc[r].y; }
                const float sx = wsum(nx);
                const bool ok = sx > 1e-30f && sx < 3.0e38f;        // (NaN: false)
                const float inx = ok ? __builtin_amdgcn_rsqf(sx) : 0.f;
#pragma unroll
                for (int r = 0; r < R; ++r) wx[(long long)t * NE + lane + 64 * r] = make_float2(xacc[r].x * inx, xacc[r].y * inx);
                if (lane == 0) wst[t] = ok ? 1 : 0;
            }
            return;
        }

        // ---- phase 1: Gershgorin bounds of T_m, then 256-way multisection for its largest eigenvalue: every wave takes 64
        //      of the candidates (all read wave 0's d / e^2 from LDS: uniform-address reads broadcast and run ahead of the
        //      serial Sturm recurrence), the waves' results meet in LDS
        float lo, hi;
        {
            float emax = 0.f, dmin = 3.0e38f, dmax = -3.0e38f;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int i = lane + 64 * r;
                if (i < m) {
                    emax = fmaxf(emax, i < m - 1 ? sqrtf(se[i]) : 0.f);
                    dmin = fminf(dmin, sd[i]); dmax = fmaxf(dmax, sd[i]);
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                emax = fmaxf(emax, __shfl_xor(emax, o));
                dmin = fminf(dmin, __shfl_xor(dmin, o));
                dmax = fmaxf(dmax, __shfl_xor(dmax, o));
            }
            lo = dmin - 2.f * emax;             // every Gershgorin disc lies inside [dmin - 2 emax, dmax + 2 emax]
            hi = dmax + 2.f * emax;
        }
        const float span0 = fmaxf(hi - lo, 1e-30f);
        hi += 1e-6f * span0 + 1e-30f;
        constexpr int NROUND = NW == 4 ? 4 : (NW == 2 ? 5 : 6);         // (64 NW + 1)^NROUND >= 3e10 sub-intervals
        for (int round = 0; round < NROUND; ++round) {
            // candidates x_c = lo + (c+1) (hi-lo)/257, c = 64 wave + lane; count(x) = #eigenvalues < x;
            // lambda_max in (x_first-1, x_first]
            const float step = (hi - lo) / (float)(NT + 1);
            const float x = lo + (64 * wave + lane + 1) * step;
            float q = 1.f, eprev = 0.f;
            int c = 0;
            for (int i = 0; i < m; ++i) {
                q = (sd[i] - x) - eprev * __builtin_amdgcn_rcpf(q);      // (1 ulp reciprocal: the count only has to be
                if (fabsf(q) < 1e-30f) q = -1e-30f;                      //  right away from the eigenvalues)
                c += (q < 0.f);
                eprev = se[i];
            }
            const unsigned long long full = __ballot(c >= m);            // candidates above every eigenvalue
            if (lane == 0) sfirst[(round & 1) * 4 + wave] = full ? 64 * wave + (int)__ffsll((long long)full) - 1 : NT;
            __syncthreads();
            const int *sf = sfirst + (round & 1) * 4;
            int first = sf[0];
#pragma unroll
            for (int wv = 1; wv < NW; ++wv) first = min(first, sf[wv]);
            const float nlo = lo + first * step;
            const float nhi = (first < NT) ? lo + (first + 1) * step : hi;
            lo = nlo; hi = nhi;
        }
        const float lam = 0.5f * (lo + hi);
        if (tid == 0) lam_out[t] = lam;
        if (!warm_on) return;
        if (have_w) {
            if (fabsf(lam - theta_w) <= 2e-5f * fabsf(lam)) return;      // verified: the vector phase 0 stored stands
            if (tid == 0) atomicAdd(wmis, 1u);
        }
        // a fresh Ritz vector for the next call: y of T_m for lam (wave 0), then the recurrence once more
        mcold = m;
        if (wave == 0) (void)lz_twisted(sd, se, m, lam, sdp, sdm, sy);
        phase = 2;
    }
}


template <int NE> static size_t jacobi2_smem()
{
    return (size_t)3 * NE * (NE + 1) * sizeof(float2) + (size_t)(4 * (NE / 2) + 24 + NE) * sizeof(float);
}
template <int NE> static size_t lmax_smem()
{
    return (size_t)NE * (NE + 1) * sizeof(float2) + (size_t)2 * NE * sizeof(float2) +
           (size_t)(2 * NE + 16) * sizeof(float) + 256 * sizeof(int);
}

template <int NE, int NT>
static int launch_jacobi2_t(jstsp_ctx *ctx, int mode, int n, int batch, const float2 *Gpart, long long sGt,
                            int nsplit, long long sGs, const TrialParams *prm, const float *tau, float2 *Q,
                            float *lam_out, float2 *Uwarm, int warm)
{
    const size_t sh = jacobi2_smem<NE>();
    JSTSP_HIP(hipFuncSetAttribute((const void *)jacobi2_kernel<NE, NT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)sh));
    // Stop rule: `worst` is the largest relative off-diagonal met BEFORE its rotation during a sweep.  Cyclic Jacobi
    // converges quadratically, so a sweep that started below 1e-4 leaves off-diagonals of order 1e-8 — under the
    // fp32 resolution — and the confirming sweep a 3e-7 threshold would cost (one of ~4 with a warm start) buys
    // nothing: 3.4 instead of 4.3 sweeps per warm-started call at BASELINE configs[1], parity unchanged
    // (|dNMSE| 1e-7 at both benchmark shapes).
    const float tol = 1e-4f;
    const int maxsw = 14, fn_aware = 1;       // (the stop rule that bounds what the remaining couplings can do to Q Z: DESIGN section 5)
    hipLaunchKernelGGL((jacobi2_kernel<NE, NT>), dim3(batch), dim3(NT), sh, ctx->stream, mode, n, Gpart, sGt, nsplit,
                       sGs, prm, tau, Q, lam_out, Uwarm, warm, tol, maxsw, (int *)nullptr, fn_aware);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

// SVT projector with warm start; n <= 64.  Uwarm: batch * NE*NE float2 (NE = 32 or 64), or nullptr.
int launch_eig_fast(jstsp_ctx *ctx, int mode, int n, int batch, const float2 *Gpart, long long sGt, int nsplit,
                    long long sGs, const TrialParams *prm, const float *tau, float2 *Q, float *lam_out,
                    float2 *Uwarm, int warm)
{
    JSTSP_REQUIRE(n >= 1 && n <= 64, JSTSP_E_UNSUPPORTED, "launch_eig_fast: n = %d > 64", n);
    if (n <= 32)
        return launch_jacobi2_t<32, 256>(ctx, mode, n, batch, Gpart, sGt, nsplit, sGs, prm, tau, Q, lam_out, Uwarm, warm);
    // (512 threads per matrix - two 2 x 2 blocks each, a lighter resident - measured 790 instead of 600 us, round 3: dropped)
    return launch_jacobi2_t<64, 1024>(ctx, mode, n, batch, Gpart, sGt, nsplit, sGs, prm, tau, Q, lam_out, Uwarm, warm);
}

int eig_fast_ne(int n) { return n <= 32 ? 32 : 64; }

template <int NE>
static int launch_lmax_t(jstsp_ctx *ctx, int n, int batch, const float2 *Gpart, long long sGt, int nsplit,
                         long long sGs, float *lam_out)
{
    const size_t sh = lmax_smem<NE>();
    JSTSP_HIP(hipFuncSetAttribute((const void *)lmax_kernel<NE>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)sh));
    hipLaunchKernelGGL((lmax_kernel<NE>), dim3(batch), dim3(256), sh, ctx->stream, n, Gpart, sGt, nsplit, sGs,
                       lam_out);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

template <int NE, int NW, int OCC>
static int launch_lanczos_t(jstsp_ctx *ctx, int n, int batch, const float2 *Gpart, long long sGt, int nsplit,
                            long long sGs, float *lam_out, const LanczosWarm *lw, int first)
{
    // exchange, flags, T, firsts, y + the two pivot arrays of the twisted factorisation, 4 scalars, start-up vectors
    const size_t sh = (size_t)2 * NW * NE * sizeof(float2) + 16 + (size_t)2 * NE * sizeof(float) + 12 * sizeof(int) +
                      (size_t)3 * NE * sizeof(float) + 16 + (size_t)LzKmax<NE>::value * NE * sizeof(float2);
    JSTSP_HIP(hipFuncSetAttribute((const void *)lanczos_lmax_kernel<NE, NW, OCC>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                  (int)sh));
    const bool warm = lw && lw->x && lw->ne == NE && tune().lanczos_warm != 0;
    hipLaunchKernelGGL((lanczos_lmax_kernel<NE, NW, OCC>), dim3(batch), dim3(64 * NW), sh, ctx->stream, n, Gpart, sGt, nsplit, sGs,
                       lam_out, warm ? lw->x + (size_t)first * NE : nullptr, warm ? lw->state + first : nullptr,
                       warm ? lw->mismatch : nullptr, warm ? lw->call : 0, tune().lanczos_verify, 1e-5f);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

int lanczos_ne(int n) { return n <= 64 ? 64 : 128; }

// lam_out[t] = lambda_max of the n x n Hermitian matrix sum_s Gpart[t][s]; n <= 128.
// lanczos: the four-wave Lanczos kernel (1e-6 relative; the ADMM loops' convergence_error) instead of Householder + Sturm;
// lw (with lanczos): warm-start record of matrices [first, first + batch) - see the kernel
int launch_lmax(jstsp_ctx *ctx, int n, int batch, const float2 *Gpart, long long sGt, int nsplit, long long sGs,
                float *lam_out, bool lanczos, const LanczosWarm *lw, int first)
{
    if (n > 128) return launch_eig_large(ctx, EIG_LMAX, n, batch, Gpart, sGt, nsplit, sGs, nullptr, nullptr, nullptr, lam_out);
    JSTSP_REQUIRE(n >= 1, JSTSP_E_UNSUPPORTED, "launch_lmax: n = %d", n);
    const bool lz = lanczos && tune().lanczos != 0;
    if (lz) {
        // four waves per matrix (one or two measured slower: too little parallelism per matrix, round 2)
        if (n <= 64) return launch_lanczos_t<64, 4, 1>(ctx, n, batch, Gpart, sGt, nsplit, sGs, lam_out, lw, first);
        // order 65..128: two workgroups per CU (256 registers per lane, a dozen spilled to scratch) - one per CU with no spills
        // measured slower at BASELINE configs[2] (sparse_admm x 100 at batch 1024: 0.42 s against 0.31 s, profiles/r05a)
        return launch_lanczos_t<128, 4, 2>(ctx, n, batch, Gpart, sGt, nsplit, sGs, lam_out, lw, first);
    }
    if (n <= 32) return launch_lmax_t<32>(ctx, n, batch, Gpart, sGt, nsplit, sGs, lam_out);
    if (n <= 64) return launch_lmax_t<64>(ctx, n, batch, Gpart, sGt, nsplit, sGs, lam_out);
    return launch_lmax_t<128>(ctx, n, batch, Gpart, sGt, nsplit, sGs, lam_out);
}

}  // namespace jstsp
