// cosamp.hip - batched CoSaMP (Needell & Tropp, Algorithm 1) on dense and Kronecker dictionaries, float64 on the device.
//
// The loop of include/jstsp.h ("CoSaMP") runs in the COEFFICIENT DOMAIN, as omp.hip's Kronecker path does.  With
// c0 = Phi' u and G = Phi' Phi (both float64, formed once per call):
//     proxy               c = c0 - G(:, kept) a(kept)                       (K columns of G)
//     least squares on T  G(T,T) b = c0(T)                                  (Cholesky, one step of refinement)
//     residual            ||v||^2 = ||u||^2 - 2 Re(a' c0) + a' G a
// so an iteration never touches the measurements.  For the Kronecker dictionary Phi = kron(Bf.', Af) an entry of G is the
// product of one entry of Af' Af and one of conj(Bf Bf'): G is never formed, and size_d = Gr G2 may reach 65 536.
//
// Why float64 and not the fp32 storage of the other solvers: the output is b restricted to `kept`, and b depends on the whole
// of T.  The 2K-th and (2K+1)-th largest |c| are always noise-level neighbours; an fp32 proxy would put different noise
// atoms into T on different dispatch paths and move x_hat by far more than an fp32 tolerance.  Products of two fp32 values
// are exact in float64, so a _c32 call is a float64 evaluation on exactly the values it was given.
//
// Three launches per iteration for the whole batch (proxy, select, solve); a stopped problem's workgroups exit at once and
// the host reads no flag back.  Every sum has a fixed order (the only atomics count histogram bins), so a call repeated is
// bit-identical, and a problem's result does not depend on the batch it is in.
#include "solver_common.h"
#include "ws64.h"

namespace jstsp {
namespace {

constexpr int CS_KMAX = 256;          // 3K <= 768 rows: one thread per row of T in the solve, 54 KiB of LDS
constexpr int CS_DMAX = 65536;        // atoms: the selection's membership bitmap is 8 KiB of LDS
constexpr double CS_PIVOT = 1e-12;    // rank rule: a Cholesky pivot at or below this times the largest diagonal entry of G(T,T)

__device__ __forceinline__ double2 zmulc(double2 a, double2 b) { return make_double2(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }   // a conj(b)
__device__ __forceinline__ double2 zsub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 zscale(double2 a, double s) { return make_double2(a.x * s, a.y * s); }

// G = Phi' Phi as the kernels see it: dense (size_d x size_d per dictionary) or the two factor Grams
// GA = Af' Af (Gr x Gr), GB(h, h') = sum_m conj(Bf(h,m)) Bf(h',m) (G2 x G2); stride 0 = one dictionary for the batch
struct CsGram {
    const double2 *G; long long sG;
    const double2 *GA; long long sGA;
    const double2 *GB; long long sGB;
    int size_d, Gr, G2, kron;
};
__device__ __forceinline__ double2 cs_entry(const CsGram &g, int t, int i, int j)
{
    if (!g.kron) return g.G[(long long)t * g.sG + i + (long long)g.size_d * j];
    const int gi = i % g.Gr, hi = i / g.Gr, gj = j % g.Gr, hj = j / g.Gr;
    return zmul(g.GA[(long long)t * g.sGA + gi + g.Gr * gj], g.GB[(long long)t * g.sGB + hi + g.G2 * hj]);
}

struct CsState {
    double2 *c0;      // [batch][size_d]  Phi' u
    double *score;    // [batch][size_d]  |c|^2 of this iteration
    int *T, *nT;      // [batch][3K]      merged index set, ascending
    int *kept, *nk;   // [batch][K]       the kept set, ascending (nk = 0 before the first iteration, K after)
    double2 *aval;    // [batch][K]       a(kept)
    double2 *W;       // [batch][3K x 3K] G(T,T), then its Cholesky factor (lower) and the factor's adjoint (upper)
    double *u2, *resid;
    int *iters, *status, *done;
};

template <class T> __global__ void cs_widen_kernel(const T *in, double2 *out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = make_double2((double)in[i].x, (double)in[i].y);
}
template <class T> __global__ void cs_narrow_kernel(const double2 *in, T *out, size_t n)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) { T v; v.x = in[i].x; v.y = in[i].y; out[i] = v; }
}

// C[t][i + ldc j] = sum_k opa(A[t sAt + i ai + k ak]) opb(B[t sBt + k bk + j bj]),  op = conj when the flag is set.
// 16 x 16 outputs per workgroup, k in panels of 16 through LDS; terms are added in ascending k.
__global__ __launch_bounds__(256) void cs_zgemm_kernel(int m, int n, int kdim, const double2 *A, long long sAt, long long ai, long long ak,
                                                       int ca, const double2 *B, long long sBt, long long bk, long long bj, int cb,
                                                       double2 *C, long long sCt, int ldc)
{
    __shared__ double2 as[16][17], bs[16][17];
    const int t = blockIdx.z, i0 = blockIdx.x * 16, j0 = blockIdx.y * 16, tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
    const double2 *a = A + (long long)t * sAt, *b = B + (long long)t * sBt;
    const bool a_kfast = ak < ai, b_kfast = bk < bj;          // the faster thread index runs along the contiguous direction
    double2 acc = make_double2(0.0, 0.0);
    for (int k0 = 0; k0 < kdim; k0 += 16) {
        {
            const int ii = a_kfast ? ty : tx, kk = a_kfast ? tx : ty;
            double2 v = make_double2(0.0, 0.0);
            if (i0 + ii < m && k0 + kk < kdim) v = a[(long long)(i0 + ii) * ai + (long long)(k0 + kk) * ak];
            if (ca) v.y = -v.y;
            as[ii][kk] = v;
        }
        {
            const int jj = b_kfast ? ty : tx, kk = b_kfast ? tx : ty;
            double2 v = make_double2(0.0, 0.0);
            if (j0 + jj < n && k0 + kk < kdim) v = b[(long long)(k0 + kk) * bk + (long long)(j0 + jj) * bj];
            if (cb) v.y = -v.y;
            bs[jj][kk] = v;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < 16; ++kk) {
            const double2 p = as[tx][kk], q = bs[ty][kk];
            acc.x += p.x * q.x - p.y * q.y;
            acc.y += p.x * q.y + p.y * q.x;
        }
        __syncthreads();
    }
    if (i0 + tx < m && j0 + ty < n) C[(long long)t * sCt + (i0 + tx) + (long long)ldc * (j0 + ty)] = acc;
}

// sum over the workgroup in a fixed order (lanes by xor shuffles, then the waves in ascending order); every thread gets it
__device__ __forceinline__ double cs_block_sum(double v, double *red)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    const int wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[wave] = v;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < nw; ++w) s += red[w];
    return s;
}

// ||u||^2 and the start state: a = 0, kept = {}, ||v|| / ||u|| = 1; u = 0 is finished before it starts
__global__ __launch_bounds__(256) void cs_init_kernel(const double2 *u, int meas, CsState s)
{
    __shared__ double red[4];
    const int t = blockIdx.x;
    double acc = 0.0;
    for (int i = threadIdx.x; i < meas; i += 256) { const double2 v = u[(long long)t * meas + i]; acc += v.x * v.x + v.y * v.y; }
    acc = cs_block_sum(acc, red);
    if (threadIdx.x == 0) {
        s.u2[t] = acc; s.resid[t] = acc > 0.0 ? 1.0 : 0.0;
        s.iters[t] = 0; s.status[t] = 0; s.nk[t] = 0; s.nT[t] = 0; s.done[t] = acc > 0.0 ? 0 : 1;
    }
}

// c = c0 - G(:, kept) a(kept);  score = |c|^2
__global__ __launch_bounds__(256) void cs_proxy_kernel(CsGram g, CsState s, int K)
{
    const int t = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (s.done[t] || i >= g.size_d) return;
    double2 c = s.c0[(long long)t * g.size_d + i];
    const int nk = s.nk[t];
    for (int k = 0; k < nk; ++k) c = zsub(c, zmul(cs_entry(g, t, i, s.kept[t * K + k]), s.aval[t * K + k]));
    s.score[(long long)t * g.size_d + i] = c.x * c.x + c.y * c.y;
}

// exclusive prefix count of `flag` over the workgroup's threads in thread order, and the total (wave64 ballots, 16 waves)
__device__ __forceinline__ int cs_block_rank(bool flag, int *wsum, int *total)
{
    const unsigned long long mask = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int pre = __popcll(mask & ((1ull << lane) - 1ull));
    __syncthreads();
    if (lane == 0) wsum[wave] = __popcll(mask);
    __syncthreads();
    int before = 0, tot = 0;
    for (int w = 0; w < 16; ++w) { const int c = wsum[w]; if (w < wave) before += c; tot += c; }
    *total = tot;
    return before + pre;
}

// Omega = the k = min(2K, size_d) atoms of largest score, the smaller index first among equal scores; T = sort(Omega U kept).
// A non-negative float64 orders as its bit pattern does: radix select from the top byte down (eight histogram passes) gives
// the k-th largest value `thr` and how many atoms equal to it belong to Omega; the atoms then enter a bitmap in LDS (those
// equal to thr in index order, by an ordered count), and T is the bitmap compacted in index order.
__global__ __launch_bounds__(1024) void cs_select_kernel(CsState s, int size_d, int K)
{
    __shared__ unsigned hist[256];
    __shared__ unsigned bm[CS_DMAX / 32];
    __shared__ unsigned long long s_prefix;
    __shared__ int s_need, wsum[16];
    const int t = blockIdx.x, tid = threadIdx.x, n3 = 3 * K;
    if (s.done[t]) return;
    const double *sc = s.score + (long long)t * size_d;
    int need = min(2 * K, size_d);
    unsigned long long prefix = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (int i = tid; i < size_d; i += 1024) {
            const unsigned long long key = (unsigned long long)__double_as_longlong(sc[i]);
            if (shift == 56 || (key >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(key >> shift) & 255], 1u);
        }
        __syncthreads();
        if (tid == 0) {
            int cum = 0, b = 255;
            for (; b > 0; --b) { if (cum + (int)hist[b] >= need) break; cum += hist[b]; }
            s_prefix = prefix | ((unsigned long long)b << shift); s_need = need - cum;
        }
        __syncthreads();
        prefix = s_prefix; need = s_need;
        __syncthreads();
    }
    for (int w = tid; w < (size_d + 31) / 32; w += 1024) bm[w] = 0;
    __syncthreads();
    if (tid < s.nk[t]) { const int j = s.kept[t * K + tid]; atomicOr(&bm[j >> 5], 1u << (j & 31)); }
    int base = 0, tot;
    for (int c = 0; c < size_d; c += 1024) {
        const int i = c + tid;
        const unsigned long long key = i < size_d ? (unsigned long long)__double_as_longlong(sc[i]) : 0ull;
        const bool eq = i < size_d && key == prefix;
        const int rank = base + cs_block_rank(eq, wsum, &tot);
        if (i < size_d && (key > prefix || (eq && rank < need))) atomicOr(&bm[i >> 5], 1u << (i & 31));
        base += tot;
    }
    __syncthreads();
    base = 0;
    for (int c = 0; c < size_d; c += 1024) {
        const int i = c + tid;
        const bool in = i < size_d && ((bm[i >> 5] >> (i & 31)) & 1u);
        const int pos = base + cs_block_rank(in, wsum, &tot);
        if (in && pos < n3) s.T[t * n3 + pos] = i;
        base += tot;
    }
    if (tid == 0) s.nT[t] = min(base, n3);
}

// L L' x = w for the factor in W (lower: L, upper: L', diagonal in dg), in place; z is scratch.  One barrier per column:
// column j of the forward sweep reads only w[j], which thread j finished in column j - 1; the backward sweep likewise.
__device__ void cs_chol_solve(const double2 *W, int n3, int n, const double *dg, double2 *w, double2 *z)
{
    const int tid = threadIdx.x;
    for (int j = 0; j < n; ++j) {
        __syncthreads();
        const double2 zj = zscale(w[j], 1.0 / dg[j]);
        if (tid == j) z[j] = zj;
        else if (tid > j && tid < n) w[tid] = zsub(w[tid], zmul(W[tid + (long long)n3 * j], zj));
    }
    for (int j = n - 1; j >= 0; --j) {
        __syncthreads();
        const double2 xj = zscale(z[j], 1.0 / dg[j]);
        if (tid == j) w[j] = xj;
        else if (tid < j) z[tid] = zsub(z[tid], zmul(W[tid + (long long)n3 * j], xj));
    }
    __syncthreads();
}

// One workgroup per problem, thread i owns row i of T:  b = argmin ||Phi(:,T) b - u|| from the normal equations
// G(T,T) b = c0(T) (left-looking Cholesky in global memory / L2, the current row of L in LDS; two triangular sweeps; one
// step of refinement on the normal-equations residual), then prune to the K largest |b|^2, the residual norm and the stop test.
// Rank rule: a pivot <= CS_PIVOT * max diag G(T,T) ends the problem with status 1 and leaves kept / a / resid as they were.
__global__ void cs_solve_kernel(CsGram g, CsState s, int K, double tol)
{
    extern __shared__ double2 cs_sh[];
    __shared__ double red[16];
    __shared__ double s_piv;
    const int t = blockIdx.x, tid = threadIdx.x, n3 = 3 * K;
    if (s.done[t]) return;
    double2 *w = cs_sh, *b = w + n3, *row = b + n3;
    double *dg = reinterpret_cast<double *>(row + n3), *sq = dg + n3;
    int *Ti = reinterpret_cast<int *>(sq + n3), *fl = Ti + n3;
    const int n = s.nT[t];
    double2 *W = s.W + (size_t)t * n3 * n3;
    const double2 *c0 = s.c0 + (long long)t * g.size_d;
    if (tid < n) Ti[tid] = s.T[t * n3 + tid];
    __syncthreads();
    if (tid < n) {
        for (int j = 0; j <= tid; ++j) W[tid + (long long)n3 * j] = cs_entry(g, t, Ti[tid], Ti[j]);
        dg[tid] = W[tid + (long long)n3 * tid].x;
    }
    __syncthreads();
    double maxd = 0.0;
    for (int j = 0; j < n; ++j) maxd = fmax(maxd, dg[j]);
    bool bad = false;
    for (int j = 0; j < n; ++j) {
        __syncthreads();                                              // column j - 1 of the factor is in memory
        if (tid < j) row[tid] = W[tid + (long long)n3 * j];           // conj(L(j, 0..j-1)): column j of the adjoint
        __syncthreads();
        double2 acc = make_double2(0.0, 0.0);
        if (tid >= j && tid < n) {
            acc = W[tid + (long long)n3 * j];
            for (int k = 0; k < j; ++k) acc = zsub(acc, zmul(W[tid + (long long)n3 * k], row[k]));
            if (tid == j) s_piv = acc.x;
        }
        __syncthreads();
        const double piv = s_piv;
        if (!(piv > CS_PIVOT * maxd)) { bad = true; break; }          // the same value in every thread
        if (tid >= j && tid < n) {
            const double d = sqrt(piv);
            const double2 l = tid == j ? make_double2(d, 0.0) : zscale(acc, 1.0 / d);
            W[tid + (long long)n3 * j] = l;
            W[j + (long long)n3 * tid] = make_double2(l.x, -l.y);
            if (tid == j) dg[j] = d;
        }
    }
    if (bad) {
        if (tid == 0) { s.status[t] = 1; s.done[t] = 1; }
        return;
    }
    if (tid < n) w[tid] = c0[Ti[tid]];
    cs_chol_solve(W, n3, n, dg, w, row);
    if (tid < n) b[tid] = w[tid];
    __syncthreads();
    if (tid < n) {                                                    // refinement: G(T,T) d = c0(T) - G(T,T) b,  b += d
        double2 r = c0[Ti[tid]];
        for (int j = 0; j < n; ++j) r = zsub(r, zmul(cs_entry(g, t, Ti[tid], Ti[j]), b[j]));
        w[tid] = r;
    }
    cs_chol_solve(W, n3, n, dg, w, row);
    if (tid < n) { b[tid].x += w[tid].x; b[tid].y += w[tid].y; sq[tid] = b[tid].x * b[tid].x + b[tid].y * b[tid].y; }
    __syncthreads();
    // prune: the K largest |b|^2, the smaller position first among equal values
    if (tid < n) {
        const double mine = sq[tid];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (sq[j] > mine || (sq[j] == mine && j < tid)) ? 1 : 0;
        fl[tid] = rank < K ? 1 : 0;
    }
    __syncthreads();
    // ||v||^2 = ||u||^2 + sum over kept i of Re( conj(a_i) ( (G a)_i - 2 c0_i ) )
    double term = 0.0;
    if (tid < n && fl[tid]) {
        double2 ga = make_double2(0.0, 0.0);
        for (int j = 0; j < n; ++j)
            if (fl[j]) { const double2 p = zmul(cs_entry(g, t, Ti[tid], Ti[j]), b[j]); ga.x += p.x; ga.y += p.y; }
        const double2 ci = c0[Ti[tid]];
        term = b[tid].x * (ga.x - 2.0 * ci.x) + b[tid].y * (ga.y - 2.0 * ci.y);
        int pos = 0;
        for (int j = 0; j < tid; ++j) pos += fl[j];
        s.kept[t * K + pos] = Ti[tid];
        s.aval[t * K + pos] = b[tid];
    }
    term = cs_block_sum(term, red);
    if (tid == 0) {
        const double u2 = s.u2[t], v2 = fmax(0.0, u2 + term), rel = sqrt(v2 / u2);
        s.nk[t] = K; s.iters[t] += 1; s.resid[t] = rel;
        if (tol > 0.0 && rel <= tol) s.done[t] = 1;
    }
}

// x_hat (zeroed by the caller) <- a(kept); support_out = kept, 1-based (0 where nothing was kept)
__global__ void cs_finish_kernel(CsState s, int size_d, int K, double2 *x, int32_t *sup)
{
    const int t = blockIdx.x, k = threadIdx.x;
    if (k >= K) return;
    const bool have = k < s.nk[t];
    if (have) x[(long long)t * size_d + s.kept[t * K + k]] = s.aval[t * K + k];
    sup[t * K + k] = have ? s.kept[t * K + k] + 1 : 0;
}

int cs_zgemm(jstsp_ctx *ctx, int m, int n, int kdim, int count, const double2 *A, long long sAt, long long ai, long long ak, int ca,
             const double2 *B, long long sBt, long long bk, long long bj, int cb, double2 *C, long long sCt, int ldc)
{
    hipLaunchKernelGGL(cs_zgemm_kernel, dim3((m + 15) / 16, (n + 15) / 16, count), dim3(256), 0, ctx->stream, m, n, kdim, A, sAt, ai, ak,
                       ca, B, sBt, bk, bj, cb, C, sCt, ldc);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

inline const double2 *as_d2(const jstsp_c64 *p) { return reinterpret_cast<const double2 *>(p); }
inline const float2 *as_d2(const jstsp_c32 *p) { return reinterpret_cast<const float2 *>(p); }

// an input array as float64 on the device: staged when it is on the host, widened when it is fp32
template <class Tin> int cs_input(jstsp_ctx *ctx, const Tin *src, size_t n, int memspace, const double2 **out)
{
    const Tin *d;
    JSTSP_TRY(stage_in(ctx, src, n, memspace, &d));
    if constexpr (sizeof(Tin) == sizeof(double2)) { *out = reinterpret_cast<const double2 *>(d); return 0; }
    else {
        double2 *wide = ctx->arena.get<double2>(n);
        JSTSP_REQUIRE(wide, JSTSP_E_NOMEM, "CoSaMP: workspace exhausted");
        hipLaunchKernelGGL(cs_widen_kernel<Tin>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d, wide, n);
        JSTSP_HIP(hipGetLastError());
        *out = wide;
        return 0;
    }
}

// kron == 0: A is the dictionary (rows x cols = measures x size_d), B unused.  kron == 1: A = Af (N x Gr), B = Bf (G2 x M).
template <class Tin, class Tout>
int cosamp_run(jstsp_ctx *ctx, int kron, int N, int M, int Gr, int G2, int batch, const Tin *A_, long long strideA, const Tin *B_,
               long long strideB, const Tin *u_, int K, int iters, double tol, Tout *x_hat, int32_t *support_out, int32_t *iters_out,
               double *resid_out, int32_t *status_out, int memspace)
{
    const char *nm = kron ? "cosamp_kron" : "cosamp";
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(A_ && u_ && x_hat && (!kron || B_), JSTSP_E_NULL, "%s: NULL array argument", nm);
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", nm);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    const long long meas_ll = (long long)N * M, d_ll = (long long)Gr * G2;
    JSTSP_REQUIRE(meas_ll < (1ll << 30) && d_ll < (1ll << 30), JSTSP_E_SHAPE, "%s: bad shape", nm);
    const int meas = (int)meas_ll, size_d = (int)d_ll;
    JSTSP_REQUIRE(K >= 1 && 2ll * K <= size_d && 3ll * K <= meas, JSTSP_E_ARG,
                  "%s: K = %d needs 1 <= K, 2K <= size_d = %d and 3K <= measures = %d", nm, K, size_d, meas);
    JSTSP_REQUIRE(iters >= 1 && tol >= 0.0, JSTSP_E_ARG, "%s: iters = %d, tol = %g (need iters >= 1, tol >= 0)", nm, iters, tol);
    const size_t eA = (size_t)N * Gr, eB = kron ? (size_t)G2 * M : 0;
    JSTSP_REQUIRE(strideA == 0 || strideA >= (long long)eA, JSTSP_E_SHAPE, "strideA too small");
    JSTSP_REQUIRE(!kron || strideB == 0 || strideB >= (long long)eB, JSTSP_E_SHAPE, "strideB too small");
    JSTSP_REQUIRE(K <= CS_KMAX, JSTSP_E_UNSUPPORTED, "%s: K = %d > %d", nm, K, CS_KMAX);
    JSTSP_REQUIRE(size_d <= CS_DMAX, JSTSP_E_UNSUPPORTED, "%s: size_d = %d > %d", nm, size_d, CS_DMAX);
    JSTSP_REQUIRE(kron || size_d <= 4096, JSTSP_E_UNSUPPORTED, "cosamp: a dense dictionary of more than 4096 atoms (size_d = %d)", size_d);
    JSTSP_ENTER(ctx);
    const int nA = strideA ? batch : 1, nB = strideB ? batch : 1, n3 = 3 * K;
    const size_t szA = strideA ? (size_t)strideA * (batch - 1) + eA : eA, szB = strideB ? (size_t)strideB * (batch - 1) + eB : eB;
    const size_t szU = (size_t)batch * meas, bd = (size_t)batch * size_d;
    size_t need = 0;
    const size_t in_elems[3] = {szA, szB, szU};
    for (size_t e : in_elems) {
        if (memspace == JSTSP_HOST) need += rnd256(e * sizeof(Tin));
        if (sizeof(Tin) != sizeof(double2)) need += rnd256(e * sizeof(double2));
    }
    if (kron) need += rnd256((size_t)nA * Gr * Gr * 16) + rnd256((size_t)nB * G2 * G2 * 16) + rnd256((size_t)batch * Gr * M * 16);
    else need += rnd256((size_t)nA * size_d * size_d * 16);
    need += rnd256(bd * 16) * 2 + rnd256(bd * 8) + rnd256(bd * sizeof(Tout)) + rnd256((size_t)batch * n3 * n3 * 16) +
            2 * rnd256((size_t)batch * n3 * 4) + rnd256((size_t)batch * K * 16) + 2 * rnd256((size_t)batch * K * 4) + 8 * rnd256((size_t)batch * 8);
    JSTSP_REQUIRE(need <= ((size_t)24 << 30), JSTSP_E_UNSUPPORTED, "%s: the float64 workspace would be %.1f GiB (limit 24)", nm,
                  (double)need / (double)((size_t)1 << 30));
    JSTSP_TRY(ctx->arena.reserve(need));
    ctx->arena.reset();
    Arena &ar = ctx->arena;
    const double2 *A, *B = nullptr, *u;
    JSTSP_TRY(cs_input(ctx, as_d2(A_), szA, memspace, &A));
    if (kron) JSTSP_TRY(cs_input(ctx, as_d2(B_), szB, memspace, &B));
    JSTSP_TRY(cs_input(ctx, as_d2(u_), szU, memspace, &u));
    CsState s;
    CsGram g{};
    g.size_d = size_d; g.Gr = Gr; g.G2 = G2; g.kron = kron;
    s.c0 = ar.get<double2>(bd); s.score = ar.get<double>(bd);
    double2 *xw = ar.get<double2>(bd);
    s.W = ar.get<double2>((size_t)batch * n3 * n3);
    s.T = ar.get<int>((size_t)batch * n3); s.nT = ar.get<int>(batch);
    s.kept = ar.get<int>((size_t)batch * K); s.nk = ar.get<int>(batch); s.aval = ar.get<double2>((size_t)batch * K);
    s.u2 = ar.get<double>(batch); s.resid = ar.get<double>(batch);
    s.iters = ar.get<int>(batch); s.status = ar.get<int>(batch); s.done = ar.get<int>(batch);
    int32_t *sup = ar.get<int32_t>((size_t)batch * K);
    JSTSP_REQUIRE(s.c0 && s.score && xw && s.W && s.T && s.nT && s.kept && s.nk && s.aval && s.u2 && s.resid && s.iters && s.status &&
                  s.done && sup, JSTSP_E_NOMEM, "%s: workspace exhausted", nm);
    hipStream_t st = ctx->stream;
    if (kron) {
        double2 *GA = ar.get<double2>((size_t)nA * Gr * Gr), *GB = ar.get<double2>((size_t)nB * G2 * G2);
        double2 *Wm = ar.get<double2>((size_t)batch * Gr * M);
        JSTSP_REQUIRE(GA && GB && Wm, JSTSP_E_NOMEM, "%s: workspace exhausted", nm);
        JSTSP_TRY(cs_zgemm(ctx, Gr, Gr, N, nA, A, strideA, N, 1, 1, A, strideA, 1, N, 0, GA, (long long)Gr * Gr, Gr));     // Af' Af
        JSTSP_TRY(cs_zgemm(ctx, G2, G2, M, nB, B, strideB, 1, G2, 1, B, strideB, G2, 1, 0, GB, (long long)G2 * G2, G2));   // conj(Bf Bf')
        // c0 = vec(Af' Y conj(Bf).'):  W = Af' Y (Gr x M), c0(g, h) = sum_m W(g, m) conj(Bf(h, m))
        JSTSP_TRY(cs_zgemm(ctx, Gr, M, N, batch, A, strideA, N, 1, 1, u, (long long)meas, 1, N, 0, Wm, (long long)Gr * M, Gr));
        JSTSP_TRY(cs_zgemm(ctx, Gr, G2, M, batch, Wm, (long long)Gr * M, 1, Gr, 0, B, strideB, G2, 1, 1, s.c0, (long long)size_d, Gr));
        g.GA = GA; g.sGA = strideA ? (long long)Gr * Gr : 0; g.GB = GB; g.sGB = strideB ? (long long)G2 * G2 : 0;
    } else {
        double2 *G = ar.get<double2>((size_t)nA * size_d * size_d);
        JSTSP_REQUIRE(G, JSTSP_E_NOMEM, "%s: workspace exhausted", nm);
        JSTSP_TRY(cs_zgemm(ctx, size_d, size_d, meas, nA, A, strideA, meas, 1, 1, A, strideA, 1, meas, 0, G, (long long)size_d * size_d, size_d));
        JSTSP_TRY(cs_zgemm(ctx, size_d, 1, meas, batch, A, strideA, meas, 1, 1, u, (long long)meas, 1, meas, 0, s.c0, (long long)size_d, size_d));
        g.G = G; g.sG = strideA ? (long long)size_d * size_d : 0;
    }
    hipLaunchKernelGGL(cs_init_kernel, dim3(batch), dim3(256), 0, st, u, meas, s);
    const int nt = min(1024, (n3 + 63) / 64 * 64);
    const size_t lds = (size_t)n3 * (3 * sizeof(double2) + 2 * sizeof(double) + 2 * sizeof(int));
    for (int it = 0; it < iters; ++it) {
        hipLaunchKernelGGL(cs_proxy_kernel, dim3((size_d + 255) / 256, batch), dim3(256), 0, st, g, s, K);
        hipLaunchKernelGGL(cs_select_kernel, dim3(batch), dim3(1024), 0, st, s, size_d, K);
        hipLaunchKernelGGL(cs_solve_kernel, dim3(batch), dim3(nt), lds, st, g, s, K, tol);
    }
    JSTSP_HIP(hipMemsetAsync(xw, 0, bd * sizeof(double2), st));
    hipLaunchKernelGGL(cs_finish_kernel, dim3(batch), dim3(CS_KMAX), 0, st, s, size_d, K, xw, sup);
    JSTSP_HIP(hipGetLastError());
    if constexpr (sizeof(Tout) == sizeof(jstsp_c64)) {
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<double2 *>(x_hat), xw, bd, memspace));
    } else {
        float2 *xn = ar.get<float2>(bd);
        JSTSP_REQUIRE(xn, JSTSP_E_NOMEM, "%s: workspace exhausted", nm);
        hipLaunchKernelGGL(cs_narrow_kernel<float2>, dim3((unsigned)((bd + 255) / 256)), dim3(256), 0, st, xw, xn, bd);
        JSTSP_HIP(hipGetLastError());
        JSTSP_TRY(stage_out(ctx, reinterpret_cast<float2 *>(x_hat), xn, bd, memspace));
    }
    JSTSP_TRY(stage_out(ctx, support_out, sup, (size_t)batch * K, memspace));
    JSTSP_TRY(stage_out(ctx, iters_out, s.iters, (size_t)batch, memspace));
    JSTSP_TRY(stage_out(ctx, resid_out, s.resid, (size_t)batch, memspace));
    JSTSP_TRY(stage_out(ctx, status_out, s.status, (size_t)batch, memspace));
    if (memspace == JSTSP_HOST) JSTSP_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // namespace
}  // namespace jstsp

using namespace jstsp;

extern "C" {

int jstsp_cosamp_c32(jstsp_ctx *ctx, int measures, int size_d, int batch, const jstsp_c32 *A, long long strideA, const jstsp_c32 *u,
                     int K, int iters, double tol, jstsp_c32 *x_hat, int32_t *support_out, int32_t *iters_out, double *resid_out,
                     int32_t *status_out, int memspace)
{
    return cosamp_run<jstsp_c32, jstsp_c32>(ctx, 0, measures, 1, size_d, 1, batch, A, strideA, nullptr, 0, u, K, iters, tol, x_hat,
                                            support_out, iters_out, resid_out, status_out, memspace);
}

int jstsp_cosamp_c64(jstsp_ctx *ctx, int measures, int size_d, int batch, const jstsp_c64 *A, long long strideA, const jstsp_c64 *u,
                     int K, int iters, double tol, jstsp_c64 *x_hat, int32_t *support_out, int32_t *iters_out, double *resid_out,
                     int32_t *status_out, int memspace)
{
    return cosamp_run<jstsp_c64, jstsp_c64>(ctx, 0, measures, 1, size_d, 1, batch, A, strideA, nullptr, 0, u, K, iters, tol, x_hat,
                                            support_out, iters_out, resid_out, status_out, memspace);
}

int jstsp_cosamp_kron_c32(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c32 *Af, long long strideA,
                          const jstsp_c32 *Bf, long long strideB, const jstsp_c32 *y, int K, int iters, double tol, jstsp_c32 *x_hat,
                          int32_t *support_out, int32_t *iters_out, double *resid_out, int32_t *status_out, int memspace)
{
    return cosamp_run<jstsp_c32, jstsp_c32>(ctx, 1, N, M, Gr, G2, batch, Af, strideA, Bf, strideB, y, K, iters, tol, x_hat, support_out,
                                            iters_out, resid_out, status_out, memspace);
}

int jstsp_cosamp_kron_c64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *Af, long long strideA,
                          const jstsp_c64 *Bf, long long strideB, const jstsp_c64 *y, int K, int iters, double tol, jstsp_c64 *x_hat,
                          int32_t *support_out, int32_t *iters_out, double *resid_out, int32_t *status_out, int memspace)
{
    return cosamp_run<jstsp_c64, jstsp_c64>(ctx, 1, N, M, Gr, G2, batch, Af, strideA, Bf, strideB, y, K, iters, tol, x_hat, support_out,
                                            iters_out, resid_out, status_out, memspace);
}

}  // extern "C"
