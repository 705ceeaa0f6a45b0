// jstsp_mmv_omp_f64 — joint (simultaneous / MMV) orthogonal matching pursuit in FLOAT64: the algorithm, the three stop rules, the
// shapes and the conventions of jstsp_mmv_omp_c32 (mmv_omp.hip states them), with every stored value and every sum a double:
// residual, basis, triangular factor, coefficients, row scores, dot products, the back-substitution and Z.  Nothing is narrowed.
//     repeat K times:  g* = argmax_g || A(:,g)^H R ||_p  (p = 2 or 1; first index on ties),
//                      support += g*;  Z(support,:) = least squares of Y on A(:,support);  R = Y - A(:,support) Z
// One workgroup per problem, as in the fp32 kernel: the problems of this path are small and many.  What differs from it:
//  - the correlation c = A(:,g)^H r is carried in FOUR real fma chains (xx, yy, xy, yx) joined at the end, c = (xx + yy, xy - yx).
//    A column equal to column j, to -j or to +-1i j runs the same four chains up to signs and a swap, so c comes out as +-c or
//    +-1i c of column j on the bits; |c|^2 is then formed with contraction off (x*x + y*y, a commutative sum of two rounded
//    squares), so that the swap cannot turn fma(x, x, y*y) into fma(y, y, x*x): such columns tie exactly and the lowest index wins.
//  - the new atom is orthogonalised by two passes of classical Gram-Schmidt: the k dot products of a pass are independent, one
//    per wave at a time, instead of 2 k block-wide reductions in sequence (cgs2_append of ws64.h, shared with omp64.hip, as are
//    the block sum and the exponent of the scaling).
//  - ||Y||_F^2 is summed on the scaled Y, so that after the exact scaling by 2^-e nothing depends on the scale of Y.
// Every sum is formed in a fixed order by a fixed thread: no atomics, a repeated call returns the same bits, and a problem's
// result does not depend on its batch mates or on the memspace.
#include "solver_common.h"
#include "ws64.h"
#include <algorithm>
#include <cfloat>
#include <cstring>

namespace jstsp {

namespace {

// workspace per problem (global): R N x S | Q N x K | Rt K x K | T K x S | D K
__global__ __launch_bounds__(256) void mmv_omp64_kernel(int N, int Gr, int S, int K, int pnorm, const double2 *A, long long strideA,
                                                        const double2 *Y, double2 *Rws, double2 *Qws, double2 *Rtws, double2 *Tws,
                                                        double2 *Dws, double2 *Z, int32_t *index_out, int32_t *count_out)
{
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    double *part = reinterpret_cast<double *>(smem_raw);          // [256] partial scores
    double *score = part + 256;                                   // [Gr]
    double *red = score + Gr;                                     // [8]
    int *taken = reinterpret_cast<int *>(red + 8);                // [Gr]
    __shared__ int s_best, s_stop;
    const int t = blockIdx.x, tid = threadIdx.x;
    const double2 *a = A + (long long)t * strideA;
    const double2 *y = Y + (long long)t * N * S;
    double2 *R = Rws + (long long)t * N * S, *Q = Qws + (long long)t * N * K, *Rt = Rtws + (long long)t * K * K,
            *T = Tws + (long long)t * K * S, *D = Dws + (long long)t * K;
    double2 *z = Z + (long long)t * Gr * S;
    int32_t *io = index_out + (long long)t * K;
    const long long NS = (long long)N * S;

    // the problem is solved on Y * 2^-ey (largest finite component in [0.5, 1)): exact unless a component underflows
    const int ey = finite_max_exponent(y, NS, red + 4);
    double y2 = 0.0;
    for (long long e = tid; e < NS; e += 256) {
        const double2 v = y[e];
        const double2 r = make_double2(ldexp(v.x, -ey), ldexp(v.y, -ey));
        R[e] = r;
        y2 = fma(r.x, r.x, y2);
        y2 = fma(r.y, r.y, y2);
    }
    for (long long e = tid; e < (long long)Gr * S; e += 256) z[e] = make_double2(0.0, 0.0);
    for (long long e = tid; e < (long long)K * K; e += 256) Rt[e] = make_double2(0.0, 0.0);
    for (int g = tid; g < Gr; g += 256) taken[g] = 0;
    for (int k = tid; k < K; k += 256) io[k] = 0;
    y2 = block_sum64(y2, red);
    const int kmax = min(K, min(N, Gr));
    int k = 0;
    // deterministic split of the (atom, column) correlations: thread -> atom g = tid % gp, column group tid / gp
    int gp = 1;
    while (gp < Gr && gp < 256) gp <<= 1;                          // power of two >= Gr (<= 256)
    const int ncg = 256 / gp;                                     // column groups
    for (; k < kmax; ++k) {
        // ---- scores: || A(:,g)^H R ||_p over the S columns
        for (int g0 = 0; g0 < Gr; g0 += gp) {
            const int g = g0 + tid % gp, cg = tid / gp;
            double acc = 0.0;
            if (g < Gr)
                for (int s = cg; s < S; s += ncg) {
                    Dot4 d = {0.0, 0.0, 0.0, 0.0};
                    const double2 *ag = a + (long long)N * g, *rs = R + (long long)N * s;
                    for (int i = 0; i < N; ++i) dot4_step(d, ag[i], rs[i]);
                    const double c2 = abs2_sym(d.xx + d.yy, d.xy - d.yx);
                    acc += (pnorm == 1) ? sqrt(c2) : c2;
                }
            part[tid] = acc;
            __syncthreads();
            if (cg == 0 && g < Gr) {
                double sc = 0.0;
                for (int c = 0; c < ncg; ++c) sc += part[c * gp + (tid % gp)];     // fixed order: reproducible
                score[g] = taken[g] ? -1.0 : sc;
            }
            __syncthreads();
        }
        if (tid == 0) {
            double best = -1.0;
            int bi = -1;
            for (int g = 0; g < Gr; ++g) {
                const double sc = score[g];
                if (sc == sc && sc > best) { best = sc; bi = g; }  // first index on ties
            }
            s_best = bi;
        }
        __syncthreads();
        const int gsel = s_best;
        if (gsel < 0) break;
        // ---- q_k = atom orthogonalised against q_0 .. q_{k-1}: two passes of classical Gram-Schmidt
        double2 *q = Q + (long long)N * k;
        double n0 = 0.0;
        for (int i = tid; i < N; i += 256) {
            const double2 v = a[(long long)N * gsel + i];
            q[i] = v;
            n0 = fma(v.x, v.x, n0);
            n0 = fma(v.y, v.y, n0);
        }
        n0 = block_sum64(n0, red);                                 // (its barriers publish q)
        const double n1 = cgs2_append(q, Q, N, k, Rt + (long long)K * k, D, red);
        if (!(n1 > 1e-10 * n0) || !(n0 > 0.0)) break;             // atom numerically inside the span of the support
        const double nrm = sqrt(n1), inv = 1.0 / nrm;
        for (int i = tid; i < N; i += 256) { double2 v = q[i]; v.x *= inv; v.y *= inv; q[i] = v; }
        if (tid == 0) { Rt[k + (long long)K * k] = make_double2(nrm, 0.0); io[k] = gsel + 1; taken[gsel] = 1; }
        __syncthreads();
        // ---- T(k,:) = q_k^H R;  R -= q_k T(k,:);  ||R||_F^2
        double r2 = 0.0;
        for (int s = tid; s < S; s += 256) {
            double2 *rs = R + (long long)N * s;
            Dot4 d = {0.0, 0.0, 0.0, 0.0};
            for (int i = 0; i < N; ++i) dot4_step(d, q[i], rs[i]);
            const double fx = d.xx + d.yy, fy = d.xy - d.yx;
            T[k + (long long)K * s] = make_double2(fx, fy);
            for (int i = 0; i < N; ++i) {
                const double2 u = q[i];
                double2 v = rs[i];
                v.x -= fx * u.x - fy * u.y;
                v.y -= fx * u.y + fy * u.x;
                rs[i] = v;
                r2 = fma(v.x, v.x, r2);
                r2 = fma(v.y, v.y, r2);
            }
        }
        r2 = block_sum64(r2, red);
        if (tid == 0) s_stop = (r2 <= 1e-12 * y2);
        __syncthreads();
        if (s_stop) { ++k; break; }
    }
    const int nsel = k;
    if (tid == 0) count_out[t] = nsel;
    __syncthreads();
    // ---- Z(support,:) = Rt^-1 T (back-substitution, one column per thread), then back to the scale of Y
    for (int s = tid; s < S; s += 256) {
        for (int r = nsel - 1; r >= 0; --r) {
            double2 acc = T[r + (long long)K * s];
            for (int c = r + 1; c < nsel; ++c) {
                const double2 u = Rt[r + (long long)K * c];
                const double2 v = z[(io[c] - 1) + (long long)Gr * s];
                acc.x -= u.x * v.x - u.y * v.y;
                acc.y -= u.x * v.y + u.y * v.x;
            }
            const double d = Rt[r + (long long)K * r].x;
            z[(io[r] - 1) + (long long)Gr * s] = make_double2(acc.x / d, acc.y / d);
        }
        if (ey != 0)
            for (int r = 0; r < nsel; ++r) {
                double2 &v = z[(io[r] - 1) + (long long)Gr * s];
                v = make_double2(ldexp(v.x, ey), ldexp(v.y, ey));
            }
    }
}

}  // namespace

}  // namespace jstsp

using namespace jstsp;

extern "C" int jstsp_mmv_omp_f64(jstsp_ctx *ctx, int N, int Gr, int S, int batch, const jstsp_c64 *A_, long long strideA,
                                 const jstsp_c64 *Y_, int K, int pnorm, jstsp_c64 *Z_out, int32_t *index_out,
                                 int32_t *count_out, int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(A_ && Y_ && Z_out, JSTSP_E_NULL, "mmv_omp (float64): NULL array argument");
    JSTSP_REQUIRE(N > 0 && Gr > 0 && S > 0 && batch > 0 && K > 0, JSTSP_E_SHAPE, "mmv_omp (float64): bad shape");
    JSTSP_REQUIRE(Gr <= 4096, JSTSP_E_UNSUPPORTED, "mmv_omp (float64): Gr = %d > 4096", Gr);
    JSTSP_REQUIRE(pnorm == 1 || pnorm == 2, JSTSP_E_ARG, "mmv_omp (float64): pnorm must be 1 or 2");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_REQUIRE(strideA == 0 || strideA >= (long long)N * Gr, JSTSP_E_SHAPE, "strideA too small");
    JSTSP_ENTER(ctx);
    const int Kc = std::min(K, std::min(N, Gr));                   // at most min(N, Gr) independent atoms
    const size_t szA = strideA ? (size_t)strideA * (batch - 1) + (size_t)N * Gr : (size_t)N * Gr;
    const size_t ns = (size_t)N * S, gs = (size_t)Gr * S;
    size_t need = rnd256(batch * ns * sizeof(double2)) + rnd256((size_t)batch * N * Kc * sizeof(double2)) +
                  rnd256((size_t)batch * Kc * Kc * sizeof(double2)) + rnd256((size_t)batch * Kc * S * sizeof(double2)) +
                  rnd256((size_t)batch * Kc * sizeof(double2)) + rnd256(batch * gs * sizeof(double2)) +
                  rnd256((size_t)batch * Kc * sizeof(int32_t)) + rnd256((size_t)batch * sizeof(int32_t));
    if (memspace == JSTSP_HOST) need += rnd256(szA * sizeof(double2)) + rnd256(batch * ns * sizeof(double2));
    JSTSP_TRY(ctx->arena.reserve(need));
    ctx->arena.reset();
    Arena &ar = ctx->arena;
    const double2 *A, *Y;
    JSTSP_TRY(stage_in(ctx, reinterpret_cast<const double2 *>(A_), szA, memspace, &A));
    JSTSP_TRY(stage_in(ctx, reinterpret_cast<const double2 *>(Y_), batch * ns, memspace, &Y));
    double2 *R = ar.get<double2>(batch * ns), *Q = ar.get<double2>((size_t)batch * N * Kc),
            *Rt = ar.get<double2>((size_t)batch * Kc * Kc), *T = ar.get<double2>((size_t)batch * Kc * S),
            *D = ar.get<double2>((size_t)batch * Kc), *Z = ar.get<double2>(batch * gs);
    int32_t *io = ar.get<int32_t>((size_t)batch * Kc), *cnt = ar.get<int32_t>(batch);
    JSTSP_REQUIRE(R && Q && Rt && T && D && Z && io && cnt, JSTSP_E_NOMEM, "mmv_omp (float64): workspace exhausted");
    const size_t sh = (256 + (size_t)Gr + 8) * sizeof(double) + (size_t)Gr * sizeof(int);
    JSTSP_HIP(hipFuncSetAttribute((const void *)mmv_omp64_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    hipLaunchKernelGGL(mmv_omp64_kernel, dim3(batch), dim3(256), sh, ctx->stream, N, Gr, S, Kc, pnorm, A, strideA, Y, R, Q, Rt, T, D, Z,
                       io, cnt);
    JSTSP_HIP(hipGetLastError());
    JSTSP_TRY(stage_out(ctx, reinterpret_cast<double2 *>(Z_out), Z, batch * gs, memspace));
    if (index_out) {
        // the caller's array has K entries per problem; entries beyond the count are 0
        if (Kc == K) JSTSP_TRY(stage_out(ctx, index_out, io, (size_t)batch * K, memspace));
        else {
            if (memspace == JSTSP_DEVICE) JSTSP_HIP(hipMemsetAsync(index_out, 0, (size_t)batch * K * sizeof(int32_t), ctx->stream));
            else memset(index_out, 0, (size_t)batch * K * sizeof(int32_t));
            JSTSP_HIP(hipMemcpy2DAsync(index_out, (size_t)K * sizeof(int32_t), io, (size_t)Kc * sizeof(int32_t),
                                       (size_t)Kc * sizeof(int32_t), batch,
                                       memspace == JSTSP_DEVICE ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    if (count_out) JSTSP_TRY(stage_out(ctx, count_out, cnt, (size_t)batch, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
