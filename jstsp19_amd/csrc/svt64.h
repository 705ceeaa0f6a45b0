// The float64 singular-value threshold shared by proposed64.hip, mc64.hip and sparse_admm64.hip (internal): the in-LDS two-sided
// Jacobi for Gram orders n <= 64 and the steps Y = svt(Z, thr), lambda_max(Z Z^H) built on it and on zgemm64.hip.
// Everything sits in an anonymous namespace: each file that includes this compiles kernels of its own (no relocatable device code).
#pragma once
#include "ws64.h"
#include "zgemm64.h"

namespace jstsp {
namespace {

constexpr int P64_LDS_ORDER = 64;        // largest Gram order of the in-LDS Jacobi
constexpr int P64_MAX_ORDER = 512;       // largest Gram order at all
constexpr int P64_SWEEPS = 30;

// ---- two-sided cyclic Jacobi in LDS ------------------------------------------------------------------------------------------
// round r of the circle ordering of n players (n even): slot s meets slot n - 1 - s, player 0 fixed, the others rotate by r
__device__ __forceinline__ void pair_of(int n, int r, int s, int &p, int &q)
{
    const int nm = n - 1;
    const int a = s == 0 ? 0 : 1 + (s - 1 + r) % nm, b = 1 + (n - 2 - s + r) % nm;
    p = min(a, b); q = max(a, b);
}

// The sweeps themselves, on H (n x n, n even) already in LDS [and U = I]: every thread of the workgroup of 256 calls; rs, rc: room
// for the n / 2 rotations; floor_abs = eps^2 dmax.  On return the diagonal of H holds the eigenvalues (a barrier has passed).
// Shared by jacobi64_lds_kernel below and by the kernels that build their Gram in LDS themselves (inputgen.hip: sigma_max of a tap).
template <bool VECS>
__device__ __forceinline__ void jacobi64_lds_sweeps(int n, double2 *H, double2 *U, double2 *rs, double *rc, double floor_abs)
{
    const int h2 = n / 2, tid = threadIdx.x;
    const double EPS = 1.1102230246251565e-16;
    for (int sweep = 0; sweep < P64_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int r = 0; r < n - 1; ++r) {
            if (tid < h2) {
                int p, q;
                pair_of(n, r, tid, p, q);
                const double hpp = H[p + n * p].x, hqq = H[q + n * q].x;
                const double2 hpq = H[p + n * q];
                const double a = hypot(hpq.x, hpq.y);
                double c = 1.0;
                double2 sn = make_double2(0.0, 0.0);
                if (a > floor_abs && a > EPS * sqrt(fabs(hpp) * fabs(hqq))) {
                    // the real rotation of [hpp, a; a, hqq] after the phase e = hpq / |hpq| is pulled out
                    const double tau = (hqq - hpp) / (2.0 * a);
                    const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + tt * tt);
                    const double sr = tt * c;
                    sn = make_double2(sr * hpq.x / a, sr * hpq.y / a);
                    rotated = 1;
                }
                rc[tid] = c; rs[tid] = sn;
            }
            __syncthreads();
            // H <- J^H H J on the 2 x 2 block (row pair k, column pair l), J = [c, s; -conj(s), c] on the coordinates (p, q)
            for (int idx = tid; idx < h2 * h2; idx += 256) {
                const int l = idx % h2, k = idx / h2;
                const double cl = rc[l], ck = rc[k];
                const double2 sl = rs[l], sk = rs[k];
                if (sl.x == 0.0 && sl.y == 0.0 && sk.x == 0.0 && sk.y == 0.0) continue;        // neither pair rotates (s = 0: identity)
                int pl, ql, pk, qk;
                pair_of(n, r, l, pl, ql);
                pair_of(n, r, k, pk, qk);
                const double2 a00 = H[pk + n * pl], a01 = H[pk + n * ql], a10 = H[qk + n * pl], a11 = H[qk + n * ql];
                // columns: [x_p, x_q] J_l = [c x_p - conj(s) x_q, s x_p + c x_q]
                const double2 u0 = zmul(zconj(sl), a01), u1 = zmul(sl, a00), u2 = zmul(zconj(sl), a11), u3 = zmul(sl, a10);
                const double2 b00 = make_double2(cl * a00.x - u0.x, cl * a00.y - u0.y), b01 = make_double2(u1.x + cl * a01.x, u1.y + cl * a01.y);
                const double2 b10 = make_double2(cl * a10.x - u2.x, cl * a10.y - u2.y), b11 = make_double2(u3.x + cl * a11.x, u3.y + cl * a11.y);
                // rows: J_k^H [y_p; y_q] = [c y_p - s y_q; conj(s) y_p + c y_q]
                const double2 v0 = zmul(sk, b10), v1 = zmul(sk, b11), w0 = zmul(zconj(sk), b00), w1 = zmul(zconj(sk), b01);
                double2 c00 = make_double2(ck * b00.x - v0.x, ck * b00.y - v0.y), c01 = make_double2(ck * b01.x - v1.x, ck * b01.y - v1.y);
                double2 c10 = make_double2(w0.x + ck * b10.x, w0.y + ck * b10.y), c11 = make_double2(w1.x + ck * b11.x, w1.y + ck * b11.y);
                if (k == l) { c01 = make_double2(0.0, 0.0); c10 = c01; c00.y = 0.0; c11.y = 0.0; }       // the annihilated pair, exactly
                H[pk + n * pl] = c00; H[pk + n * ql] = c01; H[qk + n * pl] = c10; H[qk + n * ql] = c11;
            }
            if (VECS)
                for (int idx = tid; idx < n * h2; idx += 256) {          // U <- U J: row i, column pair l
                    const int i = idx % n, l = idx / n;
                    const double cl = rc[l];
                    const double2 sl = rs[l];
                    if (sl.x == 0.0 && sl.y == 0.0) continue;
                    int pl, ql;
                    pair_of(n, r, l, pl, ql);
                    const double2 xp = U[i + n * pl], xq = U[i + n * ql];
                    const double2 u0 = zmul(zconj(sl), xq), u1 = zmul(sl, xp);
                    U[i + n * pl] = make_double2(cl * xp.x - u0.x, cl * xp.y - u0.y);
                    U[i + n * ql] = make_double2(u1.x + cl * xq.x, u1.y + cl * xq.y);
                }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated)) break;
    }
}

// G (n0 x n0 Hermitian, leading dimension n0) = U diag(lam) U^H.  VECS: U and all lam are written; otherwise lam[t] = lambda_max.
// LDS: H (n x n), [U (n x n)], n / 2 rotations (c, s), n even >= n0 (an odd order gets a decoupled zero row and column).
// A pair is rotated when |h_pq| > eps sqrt(|h_pp h_qq|) and |h_pq| > eps^2 dmax, dmax the largest diagonal entry of G (entries below
// the second level are rounding residue of a rank-deficient G: rotating them moves no eigenvalue by more than eps^2 dmax).
template <bool VECS>
__global__ __launch_bounds__(256) void jacobi64_lds_kernel(int n0, const double2 *G, long long sG, double2 *Uout, double *lam)
{
    extern __shared__ double2 sm[];
    const int n = (n0 + 1) & ~1, h2 = n / 2, t = blockIdx.x, tid = threadIdx.x;
    double2 *H = sm, *U = sm + (size_t)n * n, *rs = U + (VECS ? (size_t)n * n : 0);
    double *rc = reinterpret_cast<double *>(rs + h2), *red = rc + h2;
    const double EPS = 1.1102230246251565e-16;
    const double2 *g = G + (long long)t * sG;
    double dm = 0.0;
    for (int e = tid; e < n * n; e += 256) {
        const int i = e % n, j = e / n;
        double2 x = make_double2(0.0, 0.0);
        if (i < n0 && j < n0) x = g[i + (long long)n0 * j];
        if (i == j) { x.y = 0.0; dm = fmax(dm, fabs(x.x)); }
        H[e] = x;
        if (VECS) U[e] = make_double2(i == j ? 1.0 : 0.0, 0.0);
    }
    for (int o = 32; o > 0; o >>= 1) dm = fmax(dm, __shfl_xor(dm, o));
    if ((tid & 63) == 0) red[tid >> 6] = dm;
    __syncthreads();
    const double floor_abs = EPS * EPS * fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
    jacobi64_lds_sweeps<VECS>(n, H, U, rs, rc, floor_abs);
    if (VECS) {
        for (int e = tid; e < n0 * n0; e += 256) Uout[(long long)t * n0 * n0 + e] = U[(e % n0) + n * (e / n0)];
        for (int i = tid; i < n0; i += 256) lam[(long long)t * n0 + i] = H[i + n * i].x;
    } else if (tid == 0) {
        double m = H[0].x;
        for (int i = 1; i < n0; ++i) m = fmax(m, H[i + n * i].x);
        lam[t] = m;
    }
}

size_t jacobi_lds_bytes(int n0, bool vecs)
{
    const size_t n = (size_t)((n0 + 1) & ~1);
    return (vecs ? 2 : 1) * n * n * sizeof(double2) + (n / 2) * (sizeof(double2) + sizeof(double)) + 4 * sizeof(double);
}

__global__ __launch_bounds__(256) void lam_max_kernel(int n, int nmat, const double *lam, double *out)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nmat) return;
    double m = lam[(long long)t * n];
    for (int i = 1; i < n; ++i) m = fmax(m, lam[(long long)t * n + i]);
    out[t] = m;
}

// Uf(:, c) = max(0, 1 - tau / sigma_c) U(:, c), sigma_c = sqrt(lambda_c); a non-positive lambda_c gives 0
__global__ __launch_bounds__(256) void svt_scale64_kernel(int n, const double *thr, long long thr_stride5, const double *lam, const double2 *U, double2 *Uf)
{
    const int t = blockIdx.y;
    const double tau = thr[(long long)t * thr_stride5];
    for (int e = blockIdx.x * 256 + threadIdx.x; e < n * n; e += gridDim.x * 256) {
        const double l = lam[(long long)t * n + e / n];
        const double sg = l > 0.0 ? sqrt(l) : 0.0;
        const double f = sg > tau ? 1.0 - tau / sg : 0.0;
        const double2 u = U[(long long)t * n * n + e];
        Uf[(long long)t * n * n + e] = make_double2(f * u.x, f * u.y);
    }
}

// D = X - H, n elements
__global__ __launch_bounds__(256) void diff64_kernel(long long n, const double2 *X, const double2 *H, double2 *D)
{
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < n; e += (long long)gridDim.x * 256) {
        const double2 x = X[e], h = H[e];
        D[e] = make_double2(x.x - h.x, x.y - h.y);
    }
}

// ce(it, t) = num[t] / den[t] (IEEE: x / 0 = Inf, 0 / 0 = NaN, as the reference); ce laid out Imax per trial
__global__ __launch_bounds__(256) void ratio64_kernel(int batch, int Imax, int it, const double *num, const double *den, double *ce)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < batch) ce[(long long)t * Imax + it] = num[t] / den[t];
}

// U, lam of nmat Hermitian matrices G of order n, n * n elements apart (n <= 64: in LDS, asynchronous; above: vamp64.hip's
// Jacobi, which synchronises; freeze: zgemm64.h, eig64_global)
int eig64(hipStream_t st, int n, int nmat, const double2 *G, double2 *U, double *lam, bool freeze)
{
    if (n <= P64_LDS_ORDER) {
        const size_t sh = jacobi_lds_bytes(n, true);
        JSTSP_HIP(hipFuncSetAttribute((const void *)jacobi64_lds_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
        hipLaunchKernelGGL(jacobi64_lds_kernel<true>, dim3(nmat), dim3(256), sh, st, n, G, (long long)n * n, U, lam);
        JSTSP_HIP(hipGetLastError());
        return 0;
    }
    return eig64_global(st, n, nmat, G, (long long)n * n, U, lam, freeze);
}

// svt of `batch` matrices Z (N x M) with thresholds thr[t * thr_stride]: the arrays it needs (layout) and the steps
struct Svt64 {
    int N, M, n, batch;
    bool left;              // n = N: G = Z Z^H, Y = Q Z; otherwise G = Z^H Z, Y = Z Q
    bool freeze = false;    // n > 64: a matrix that has converged is not swept on with its batch mates (zgemm64.h: eig64_global)
    double2 *G, *U, *Uf, *Q, *ws;
    double *lam;
    static size_t ws_elems(int N, int M, int batch)
    {
        const int n = std::min(N, M), k = std::max(N, M);
        return std::max(std::max(zgemm64_ws_elems(n, n, k, batch), zgemm64_ws_elems(n, n, n, batch)), zgemm64_ws_elems(N, M, n, batch));
    }
    void layout(Slab &s, int N_, int M_, int batch_)
    {
        N = N_; M = M_; batch = batch_; n = std::min(N, M); left = N <= M;
        const size_t nn = (size_t)n * n * batch;
        G = s.get<double2>(nn); U = s.get<double2>(nn); Uf = s.get<double2>(nn); Q = s.get<double2>(nn);
        ws = s.get<double2>(std::max<size_t>(1, ws_elems(N, M, batch)));
        lam = s.get<double>((size_t)n * batch);
    }
    int gram(hipStream_t st, const double2 *Z, double2 *Gout) const
    {
        const Mat64 z{Z, (long long)N * M, N};
        return left ? zgemm64(st, 'N', 'C', n, n, M, batch, z, z, Gout, (long long)n * n, n, ws)
                    : zgemm64(st, 'C', 'N', n, n, N, batch, z, z, Gout, (long long)n * n, n, ws);
    }
    // lmax[t] = lambda_max of the Gram of Z[t]
    int lambda_max(hipStream_t st, const double2 *Z, double *lmax) const
    {
        JSTSP_TRY(gram(st, Z, G));
        if (n <= P64_LDS_ORDER) {
            const size_t sh = jacobi_lds_bytes(n, false);
            JSTSP_HIP(hipFuncSetAttribute((const void *)jacobi64_lds_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
            hipLaunchKernelGGL(jacobi64_lds_kernel<false>, dim3(batch), dim3(256), sh, st, n, G, (long long)n * n, (double2 *)nullptr, lmax);
        } else {
            JSTSP_TRY(eig64_global(st, n, batch, G, (long long)n * n, U, lam, freeze));
            hipLaunchKernelGGL(lam_max_kernel, dim3((batch + 255) / 256), dim3(256), 0, st, n, batch, lam, lmax);
        }
        JSTSP_HIP(hipGetLastError());
        return 0;
    }
    // Y = svt(Z, thr)
    int apply(hipStream_t st, const double2 *Z, const double *thr, long long thr_stride, double2 *Y) const
    {
        const long long snn = (long long)n * n, snm = (long long)N * M;
        JSTSP_TRY(gram(st, Z, G));
        JSTSP_TRY(eig64(st, n, batch, G, U, lam, freeze));
        hipLaunchKernelGGL(svt_scale64_kernel, dim3((unsigned)std::min((n * n + 255) / 256, 64), batch), dim3(256), 0, st, n, thr, thr_stride, lam, U, Uf);
        JSTSP_HIP(hipGetLastError());
        JSTSP_TRY(zgemm64(st, 'N', 'C', n, n, n, batch, Mat64{Uf, snn, n}, Mat64{U, snn, n}, Q, snn, n, ws));
        return left ? zgemm64(st, 'N', 'N', N, M, N, batch, Mat64{Q, snn, n}, Mat64{Z, snm, N}, Y, snm, N, ws)
                    : zgemm64(st, 'N', 'N', N, M, M, batch, Mat64{Z, snm, N}, Mat64{Q, snn, n}, Y, snm, N, ws);
    }
};

}  // namespace
}  // namespace jstsp
