// jstsp_pinv_f64 / jstsp_ls_f64 - MATLAB's SVD-based `pinv` and the least-squares estimate pinv(A)*Y*pinv(B)
// (plot_errorVSsnr.m:83) computed AND returned in float64, for dictionary factors of any driver size:
// min(rows, cols) <= 512, max(rows, cols) <= 8192.  Nothing is narrowed and no Gram matrix is formed, so the error grows
// like cond * eps64 (the Gram routes of hinv.hip square the condition number).
//
// Route: one-sided (Hestenes) Jacobi directly on the columns of W in GLOBAL memory, W = A when
// rows >= cols and W = A^H otherwise (pinv(A) = pinv(A^H)^H); W is m x n, m >= n.  A round-robin round has n/2 disjoint
// column pairs; one kernel launch per round, one wave (m <= 512) or one workgroup (m > 512) per pair, the three inner
// products a = |w_p|^2, b = |w_q|^2, g = w_p^H w_q by wave reductions in a fixed order, consecutive lanes on consecutive
// 16-byte elements of a column.  The same plane rotation is applied to the columns of V (n x n, starts as I), so that
//     W V = U Sigma (columns orthogonal)   =>   pinv(W) = V Sigma^-2 (W V)^H,
// which the f64-MFMA GEMM (zgemm64.hip) assembles.  As in svdvals.hip the operand is first scaled by a power of two to
// max |entry| in [1/2, 1) (exact), and a column whose norm has fallen to eps |W|_F / sqrt(n) is left alone.  The sweeps of
// a matrix end when one of them met no pair with |g| > sqrt(m) eps sqrt(a b) (its own flag: a matrix's result does not depend
// on the batch around it); whether any matrix of the call is still rotating is read on the host once per sweep, so a call
// synchronises the context's stream.  Drop rule (pinv.m): sigma_k is kept iff sigma_k > max(rows, cols) * eps(sigma_max),
// eps(x) = 2^(floor(log2 x) - 52) - one place, pinv64_drop_tol (pinv64.h).  No atomics anywhere: a repeated call returns the same bits.
#include "pinv64.h"

#include <algorithm>

namespace jstsp {

namespace {

constexpr int PV_SWEEPS = 40;            // cap (the tested inputs stop after 6 to 12)
constexpr int PV_WAVE_ROWS = 512;        // columns up to this length: one wave per pair; longer: one workgroup per pair
constexpr double PV_EPS = 2.220446049250313e-16;

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double wave_max(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}

// One workgroup per matrix: W = sc * A (rows >= cols) or sc * A^H, V = I, meta.  Sums in a fixed order.
__global__ __launch_bounds__(1024) void p64_prep_kernel(int rows, int cols, const double2 *A, long long sA, double2 *W, double2 *V, PvMeta *meta)
{
    __shared__ double red[16];
    __shared__ int sbad;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool tr = rows < cols;
    const int m = tr ? cols : rows, n = tr ? rows : cols;
    const long long cnt = (long long)rows * cols;
    const double2 *a = A + (long long)t * sA;
    double2 *Wt = W + (long long)t * m * n, *Vt = V + (long long)t * n * n;
    if (tid == 0) sbad = 0;
    __syncthreads();
    double amax = 0.0;
    int bad = 0;
    for (long long e = tid; e < cnt; e += 1024) {
        const double2 v = a[e];
        bad |= !isfinite(v.x) || !isfinite(v.y);
        amax = fmax(amax, fmax(fabs(v.x), fabs(v.y)));
    }
    amax = wave_max(amax);
    if (lane == 0) red[w] = amax;
    if (bad) sbad = 1;                                            // (every writer stores the same value)
    __syncthreads();
    bad = sbad;
    amax = 0.0;
    for (int i = 0; i < 16; ++i) amax = fmax(amax, red[i]);
    int ex = 0;
    if (!bad && amax > 0.0) frexp(amax, &ex);
    ex = max(-1000, min(1000, ex));
    const double sc = ldexp(1.0, -ex);
    double f2 = 0.0;
    for (long long e = tid; e < cnt; e += 1024) {
        const double2 v = a[e];
        const double x = v.x * sc, y = v.y * sc;
        f2 += x * x + y * y;
        if (!tr) Wt[e] = make_double2(x, y);
        else {
            const long long i = e % rows, j = e / rows;           // a(i, j) -> w(j, i) = conj
            Wt[j + (long long)m * i] = make_double2(x, -y);
        }
    }
    for (long long e = tid; e < (long long)n * n; e += 1024) Vt[e] = make_double2(e % n == e / n ? 1.0 : 0.0, 0.0);
    f2 = wave_sum(f2);
    __syncthreads();                                              // every wave has read the maxima
    if (lane == 0) red[w] = f2;
    __syncthreads();
    if (tid == 0) {
        f2 = 0.0;
        for (int i = 0; i < 16; ++i) f2 += red[i];
        PvMeta mt;
        mt.sc = sc; mt.fro2 = f2; mt.bad = bad; mt.done = 0; mt.rot = 0; mt.pad = 0;
        meta[t] = mt;
    }
}

// One round of the round-robin schedule: pair k of round r rotates columns (p, q) of W and of V.  TPP threads per pair:
// 64 (four pairs per workgroup, no barrier) or 256 (one pair per workgroup, the four waves' partial sums added in wave order).
template <int TPP>
__global__ __launch_bounds__(256) void p64_round_kernel(int m, int n, int r, double2 *W, double2 *V, PvMeta *meta)
{
    __shared__ double red[16];
    const int t = blockIdx.y;
    PvMeta *mt = meta + t;
    if (mt->bad || mt->done) return;
    const int ne = n + (n & 1), half = ne / 2, ring = ne - 1;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int k = TPP == 64 ? (int)blockIdx.x * 4 + w : (int)blockIdx.x;
    const int g0 = TPP == 64 ? lane : (int)threadIdx.x;
    if (k >= half) return;                                        // (TPP == 256: the grid has exactly `half` workgroups)
    const int u = k == 0 ? ring : (r + k) % ring, v = k == 0 ? r : (r + ring - k) % ring;
    const int p = min(u, v), q = max(u, v);
    if (q >= n) return;                                           // the idle slot of an odd n (uniform over the pair's threads)
    double2 *cp = W + ((long long)t * n + p) * m, *cq = W + ((long long)t * n + q) * m;
    double a = 0.0, b = 0.0, gr = 0.0, gi = 0.0;
    for (int i = g0; i < m; i += TPP) {
        const double2 x = cp[i], y = cq[i];
        a += x.x * x.x + x.y * x.y;
        b += y.x * y.x + y.y * y.y;
        gr += x.x * y.x + x.y * y.y;                              // conj(x) y
        gi += x.x * y.y - x.y * y.x;
    }
    a = wave_sum(a); b = wave_sum(b); gr = wave_sum(gr); gi = wave_sum(gi);
    if (TPP == 256) {
        if (lane == 0) { red[w] = a; red[4 + w] = b; red[8 + w] = gr; red[12 + w] = gi; }
        __syncthreads();
        a = ((red[0] + red[1]) + red[2]) + red[3];
        b = ((red[4] + red[5]) + red[6]) + red[7];
        gr = ((red[8] + red[9]) + red[10]) + red[11];
        gi = ((red[12] + red[13]) + red[14]) + red[15];
    }
    const double floor2 = mt->fro2 * PV_EPS * PV_EPS / (double)n;
    const double g = hypot(gr, gi), ab = sqrt(a) * sqrt(b);
    // a column at rounding level stays as it is; a pair that is orthogonal to the last bit needs nothing
    if (a <= floor2 || b <= floor2 || !(g > 0.25 * PV_EPS * ab)) return;
    if (g > sqrt((double)m) * PV_EPS * ab && g0 == 0) mt->rot = 1;        // (every writer stores the same value)
    const double z = (b - a) / (2.0 * g);
    const double tt = copysign(1.0, z) / (fabs(z) + hypot(1.0, z));
    const double c = 1.0 / sqrt(1.0 + tt * tt), s = c * tt;
    const double wr = gr / g, wi = gi / g;
    for (int i = g0; i < m; i += TPP) {
        const double2 x = cp[i], y = cq[i];
        const double yr = y.x * wr + y.y * wi, yi = y.y * wr - y.x * wi;  // y conj(w)
        cp[i] = make_double2(c * x.x - s * yr, c * x.y - s * yi);
        cq[i] = make_double2(s * x.x + c * yr, s * x.y + c * yi);
    }
    double2 *vp = V + ((long long)t * n + p) * n, *vq = V + ((long long)t * n + q) * n;
    for (int i = g0; i < n; i += TPP) {
        const double2 x = vp[i], y = vq[i];
        const double yr = y.x * wr + y.y * wi, yi = y.y * wr - y.x * wi;
        vp[i] = make_double2(c * x.x - s * yr, c * x.y - s * yi);
        vq[i] = make_double2(s * x.x + c * yr, s * x.y + c * yi);
    }
}

// After a sweep: a matrix whose sweep met no significant pair is finished; *any = 1 while one matrix is not.
__global__ __launch_bounds__(256) void p64_sweep_end_kernel(int batch, PvMeta *meta, int *any)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= batch) return;
    PvMeta *mt = meta + t;
    if (mt->bad || mt->done) return;
    if (mt->rot) { mt->rot = 0; *any = 1; }                       // (every writer stores the same value)
    else mt->done = 1;
}

// One workgroup per matrix: sigma_k = |column k of W V|, the drop rule, rcond, rank, and Vs = V diag(sc / sigma_k^2) with
// zeros for the dropped components.  LDS: n doubles.
__global__ __launch_bounds__(256) void p64_sigma_kernel(int rows, int cols, const double2 *W, const double2 *V, double2 *Vs, const PvMeta *meta,
                                                        double *rcond, int32_t *rank)
{
    __shared__ double sig2[PV_MAX_ORDER];
    __shared__ double stol;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int m = max(rows, cols), n = min(rows, cols);
    const PvMeta mt = meta[t];
    const double2 *Wt = W + (long long)t * m * n, *Vt = V + (long long)t * n * n;
    double2 *Vst = Vs + (long long)t * n * n;
    if (mt.bad) {
        if (tid == 0) {
            if (rcond) rcond[t] = __builtin_nan("");
            if (rank) rank[t] = 0;
        }
        return;
    }
    for (int k = w; k < n; k += 4) {
        const double2 *c = Wt + (long long)k * m;
        double a = 0.0;
        for (int i = lane; i < m; i += 64) a += c[i].x * c[i].x + c[i].y * c[i].y;
        a = wave_sum(a);
        if (lane == 0) sig2[k] = a;
    }
    __syncthreads();
    if (tid == 0) {
        double smax2 = 0.0;
        for (int k = 0; k < n; ++k) smax2 = fmax(smax2, sig2[k]);
        const double smax = sqrt(smax2);
        const double tol = pinv64_drop_tol(m, smax);              // pinv.m: tol = max(size(A)) * eps(norm(A))
        double smin = smax;
        int kept = 0;
        for (int k = 0; k < n; ++k) {
            const double s = sqrt(sig2[k]);
            if (s > tol) { ++kept; smin = fmin(smin, s); }
        }
        stol = tol;
        if (rcond) rcond[t] = kept ? smin / smax : 0.0;
        if (rank) rank[t] = kept;
    }
    __syncthreads();
    const double tol = stol;
    for (int e = tid; e < n * n; e += 256) {
        const int k = e / n;
        const double s2 = sig2[k];
        const double f = sqrt(s2) > tol ? mt.sc / s2 : 0.0;
        const double2 v = Vt[e];
        Vst[e] = make_double2(v.x * f, v.y * f);
    }
}

// NaN for the matrices that held a non-finite entry
__global__ __launch_bounds__(256) void p64_nan_kernel(long long cnt, double2 *P, long long sP, const PvMeta *meta)
{
    const int t = blockIdx.y;
    if (!meta[t].bad) return;
    const double q = __builtin_nan("");
    double2 *Pt = P + (long long)t * sP;
    for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < cnt; e += (long long)gridDim.x * 256) Pt[e] = make_double2(q, q);
}

// out[0] = the smallest of v[0 .. cnt), NaN when one of them is NaN
__global__ void p64_min_kernel(int cnt, const double *v, double *out)
{
    double r = v[0];
    for (int i = 1; i < cnt; ++i) r = (r != r || v[i] != v[i]) ? __builtin_nan("") : fmin(r, v[i]);
    *out = r;
}


// One workgroup per matrix: the first n_keep column norms of the rotated W in descending order, scaled back, to sv[k + n_keep t]
// (the singular values alone, spectrum_values below); NaN for a matrix with a non-finite entry.  Equal norms keep column order.
__global__ __launch_bounds__(256) void p64_values_kernel(int m, int n, const double2 *W, const PvMeta *meta, int n_keep, double *sv)
{
    __shared__ double sig[PV_MAX_ORDER];
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const PvMeta mt = meta[t];
    double *out = sv + (long long)n_keep * t;
    if (mt.bad) {
        for (int k = tid; k < n_keep; k += 256) out[k] = __builtin_nan("");
        return;
    }
    const double2 *Wt = W + (long long)t * m * n;
    for (int k = w; k < n; k += 4) {
        const double2 *c = Wt + (long long)k * m;
        double a = 0.0;
        for (int i = lane; i < m; i += 64) a += c[i].x * c[i].x + c[i].y * c[i].y;
        a = wave_sum(a);
        if (lane == 0) sig[k] = sqrt(a);
    }
    __syncthreads();
    const double unscale = 1.0 / mt.sc;                           // (a power of two: exact)
    for (int i = tid; i < n; i += 256) {
        const double v = sig[i];
        int rank = 0;
        for (int k = 0; k < n; ++k) rank += (sig[k] > v) || (sig[k] == v && k < i);
        if (rank < n_keep) out[rank] = v * unscale;
    }
}

// One workgroup per matrix, after the sweeps: the leading n_keep singular triplets (pinv64_svd, pinv64.h).  The norms are those of
// p64_values_kernel, summed the same way; column j of W V goes to place[j] in descending order of the norms.
__global__ __launch_bounds__(256) void p64_vectors_kernel(int rows, int cols, const double2 *W, const double2 *V, const PvMeta *meta, int n_keep,
                                                          double2 *U, double *sv, double2 *Vout, int32_t *rank, int32_t *conv)
{
    __shared__ double sig[PV_MAX_ORDER];
    __shared__ int place[PV_MAX_ORDER];
    __shared__ double stol;
    const int t = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bool tall = rows >= cols;
    const int m = tall ? rows : cols, n = tall ? cols : rows;
    const PvMeta mt = meta[t];
    double *out = sv + (long long)n_keep * t;
    double2 *Lt = tall ? U : Vout, *St = tall ? Vout : U;         // long side: m x n_keep; short side: n x n_keep
    if (Lt) Lt += (long long)t * m * n_keep;
    if (St) St += (long long)t * n * n_keep;
    if (mt.bad) {
        const double q = __builtin_nan("");
        for (int k = tid; k < n_keep; k += 256) out[k] = q;
        if (Lt) for (long long e = tid; e < (long long)m * n_keep; e += 256) Lt[e] = make_double2(q, q);
        if (St) for (long long e = tid; e < (long long)n * n_keep; e += 256) St[e] = make_double2(q, q);
        if (tid == 0) {
            if (rank) rank[t] = 0;
            if (conv) conv[t] = 0;
        }
        return;
    }
    const double2 *Wt = W + (long long)t * m * n, *Vt = V + (long long)t * n * n;
    for (int k = w; k < n; k += 4) {
        const double2 *c = Wt + (long long)k * m;
        double a = 0.0;
        for (int i = lane; i < m; i += 64) a += c[i].x * c[i].x + c[i].y * c[i].y;
        a = wave_sum(a);
        if (lane == 0) sig[k] = sqrt(a);
    }
    __syncthreads();
    const double unscale = 1.0 / mt.sc;                           // (a power of two: exact)
    for (int i = tid; i < n; i += 256) {
        const double v = sig[i];
        int pl = 0;
        for (int k = 0; k < n; ++k) pl += (sig[k] > v) || (sig[k] == v && k < i);
        place[i] = pl;
        if (pl < n_keep) out[pl] = v * unscale;
    }
    if (tid == 0) {
        double smax = 0.0;
        for (int k = 0; k < n; ++k) smax = fmax(smax, sig[k]);
        const double tol = pinv64_drop_tol(m, smax);
        int kept = 0;
        for (int k = 0; k < n; ++k) kept += sig[k] > tol;
        stol = tol;
        if (rank) rank[t] = kept;
        if (conv) conv[t] = (mt.done || n == 1) ? 1 : 0;          // (a single column has no pair and no sweep)
    }
    __syncthreads();
    const double tol = stol;
    if (Lt)
        for (long long e = tid; e < (long long)m * n; e += 256) {
            const int j = (int)(e / m), i = (int)(e % m), pl = place[j];
            if (pl >= n_keep) continue;
            const double s = sig[j];
            const double2 x = Wt[e];
            Lt[i + (long long)m * pl] = s > tol ? make_double2(x.x / s, x.y / s) : make_double2(0.0, 0.0);
        }
    if (St)
        for (int e = tid; e < n * n; e += 256) {
            const int j = e / n, i = e % n, pl = place[j];
            if (pl < n_keep) St[i + (long long)n * pl] = Vt[e];
        }
}

}  // namespace

// The prescale and the sweeps of `count` matrices: what pinv64_run and pinv64_values share.  Synchronises the stream once per sweep.
static int p64_decompose(hipStream_t st, const Pinv64Arrays &w, int rows, int cols, int count, const double2 *A, long long sA)
{
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    double2 *W = w.W, *V = w.V;
    PvMeta *meta = w.meta;
    int *any = w.any;
    hipLaunchKernelGGL(p64_prep_kernel, dim3(count), dim3(1024), 0, st, rows, cols, A, sA, W, V, meta);
    JSTSP_HIP(hipGetLastError());
    const int ne = n + (n & 1), half = ne / 2, ring = ne - 1;
    for (int sweep = 0; sweep < PV_SWEEPS && n > 1; ++sweep) {
        for (int r = 0; r < ring; ++r) {
            if (m <= PV_WAVE_ROWS) hipLaunchKernelGGL(p64_round_kernel<64>, dim3((half + 3) / 4, count), dim3(256), 0, st, m, n, r, W, V, meta);
            else hipLaunchKernelGGL(p64_round_kernel<256>, dim3(half, count), dim3(256), 0, st, m, n, r, W, V, meta);
        }
        JSTSP_HIP(hipGetLastError());
        JSTSP_HIP(hipMemsetAsync(any, 0, sizeof(int), st));
        hipLaunchKernelGGL(p64_sweep_end_kernel, dim3((count + 255) / 256), dim3(256), 0, st, count, meta, any);
        int h_any = 0;
        JSTSP_HIP(hipMemcpyAsync(&h_any, any, sizeof(int), hipMemcpyDeviceToHost, st));
        JSTSP_HIP(hipStreamSynchronize(st));
        if (!h_any) break;
    }
    return 0;
}

// ---- what the float64 entry points that invert a factor share (pinv64.h) -------------------------------------------------------
bool pinv64_shape_ok(int rows, int cols) { return std::min(rows, cols) <= PV_MAX_ORDER && std::max(rows, cols) <= PV_MAX_LONG; }

size_t pinv64_gemm_ws(int rows, int cols, int count)
{
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    return std::max<size_t>(1, rows >= cols ? zgemm64_ws_elems(n, m, n, count) : zgemm64_ws_elems(m, n, n, count));
}

// P[t] (cols x rows, contiguous) = pinv(A[t]) (rows x cols, sA elements apart), t < count; rcond / rank: nullptr or device [count].
// Synchronises the stream once per sweep.
int pinv64_run(hipStream_t st, const Pinv64Arrays &w, int rows, int cols, int count, const double2 *A, long long sA, double2 *P, double *rcond,
               int32_t *rank)
{
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    const size_t mn = (size_t)m * n, nn = (size_t)n * n;
    double2 *W = w.W, *V = w.V, *Vs = w.Vs, *ws = w.ws;
    PvMeta *meta = w.meta;
    JSTSP_TRY(p64_decompose(st, w, rows, cols, count, A, sA));
    hipLaunchKernelGGL(p64_sigma_kernel, dim3(count), dim3(256), 0, st, rows, cols, W, V, Vs, meta, rcond, rank);
    JSTSP_HIP(hipGetLastError());
    const long long smn = (long long)mn, snn = (long long)nn;
    if (rows >= cols) JSTSP_TRY(zgemm64(st, 'N', 'C', n, m, n, count, Mat64{Vs, snn, n}, Mat64{W, smn, m}, P, smn, n, ws));     // V f (W V)^H
    else JSTSP_TRY(zgemm64(st, 'N', 'C', m, n, n, count, Mat64{W, smn, m}, Mat64{Vs, snn, n}, P, smn, m, ws));               // its adjoint
    hipLaunchKernelGGL(p64_nan_kernel, dim3((unsigned)std::min<size_t>((mn + 255) / 256, 1024), count), dim3(256), 0, st, (long long)mn, P, smn, meta);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

// sv[k + n_keep t] = the k-th largest singular value of A[t], k < n_keep <= min(rows, cols) (device): the same prescale, rounds
// and per-matrix stop as pinv64_run, then the sorted column norms.  V is rotated along and discarded (the round kernel is the
// one jstsp_pinv_f64 runs, unchanged); w.Vs and w.ws are not used.  Synchronises the stream once per sweep.
int pinv64_values(hipStream_t st, const Pinv64Arrays &w, int rows, int cols, int count, const double2 *A, long long sA, int n_keep, double *sv)
{
    JSTSP_TRY(p64_decompose(st, w, rows, cols, count, A, sA));
    hipLaunchKernelGGL(p64_values_kernel, dim3(count), dim3(256), 0, st, std::max(rows, cols), std::min(rows, cols), w.W, w.meta, n_keep, sv);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

// The leading singular triplets (pinv64.h).  V is the rotated identity of p64_decompose; w.Vs and w.ws are not used.
// Synchronises the stream once per sweep.
int pinv64_svd(hipStream_t st, const Pinv64Arrays &w, int rows, int cols, int count, const double2 *A, long long sA, int n_keep, double2 *U,
               double *sv, double2 *Vout, int32_t *rank, int32_t *conv)
{
    JSTSP_TRY(p64_decompose(st, w, rows, cols, count, A, sA));
    hipLaunchKernelGGL(p64_vectors_kernel, dim3(count), dim3(256), 0, st, rows, cols, w.W, w.V, w.meta, n_keep, U, sv, Vout, rank, conv);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

// out[0] = the smallest of v[0 .. cnt) on the device, NaN when one of them is NaN
int pinv64_min(hipStream_t st, int cnt, const double *v, double *out)
{
    hipLaunchKernelGGL(p64_min_kernel, dim3(1), dim3(1), 0, st, cnt, v, out);
    JSTSP_HIP(hipGetLastError());
    return 0;
}

}  // namespace jstsp

using namespace jstsp;

extern "C" {

int jstsp_pinv_f64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *A_, jstsp_c64 *P_, double *rcond_out, int32_t *rank_out, int memspace)
{
    const char *nm = "pinv (float64)";
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(rows > 0 && cols > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", nm);
    JSTSP_REQUIRE(A_ && P_, JSTSP_E_NULL, "%s: NULL argument", nm);
    JSTSP_REQUIRE(pinv64_shape_ok(rows, cols) && batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: %d x %d, batch %d: need min(rows, cols) <= %d, max(rows, cols) <= %d and batch <= 65535", nm, rows, cols, batch, PV_MAX_ORDER,
                  PV_MAX_LONG);
    const bool host = memspace == JSTSP_HOST;
    hipStream_t st = ctx->stream;
    const double2 *A;
    double2 *P;
    double *rc;
    int32_t *rk;
    Pinv64 pv;
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nm, batch, [&](Slab &w, int b) {
        const size_t e = (size_t)rows * cols * b;
        A = w.in(reinterpret_cast<const double2 *>(A_), e, host);
        P = w.out(reinterpret_cast<double2 *>(P_), e, host);
        rc = w.out(rcond_out, b, host);
        rk = w.out(rank_out, b, host);
        pv.layout(w, rows, cols, b);
    }));
    JSTSP_TRY(pinv64_run(st, pv, rows, cols, batch, A, (long long)rows * cols, P, rc, rk));
    if (host) {
        JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(P_), P, (size_t)rows * cols * batch));
        if (rcond_out) JSTSP_TRY(s.copy_back(rcond_out, rc, batch));
        if (rank_out) JSTSP_TRY(s.copy_back(rank_out, rk, batch));
        JSTSP_HIP(hipStreamSynchronize(st));
    }
    return 0;
}

int jstsp_ls_f64(jstsp_ctx *ctx, int N, int M, int Gr, int G2, int batch, const jstsp_c64 *Y_, const jstsp_c64 *A_, long long strideA,
                 const jstsp_c64 *B_, long long strideB, jstsp_c64 *S_out, double *rcond_out, int memspace)
{
    const char *nm = "ls (float64)";
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "ctx is NULL");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "bad memspace %d", memspace);
    JSTSP_ENTER(ctx);
    JSTSP_REQUIRE(N > 0 && M > 0 && Gr > 0 && G2 > 0 && batch > 0 && strideA >= 0 && strideB >= 0, JSTSP_E_SHAPE, "%s: bad shape", nm);
    JSTSP_REQUIRE(Y_ && A_ && B_ && S_out, JSTSP_E_NULL, "%s: NULL argument", nm);
    JSTSP_REQUIRE((strideA == 0 || strideA == (long long)N * Gr) && (strideB == 0 || strideB == (long long)G2 * M), JSTSP_E_ARG,
                  "%s: a factor stride is 0 (shared) or the size of one factor", nm);
    JSTSP_REQUIRE(pinv64_shape_ok(N, Gr) && pinv64_shape_ok(G2, M) && batch <= 65535, JSTSP_E_UNSUPPORTED,
                  "%s: A %d x %d, B %d x %d, batch %d: need min(rows, cols) <= %d, max(rows, cols) <= %d per factor and batch <= 65535", nm, N, Gr, G2, M,
                  batch, PV_MAX_ORDER, PV_MAX_LONG);
    const bool host = memspace == JSTSP_HOST;
    hipStream_t st = ctx->stream;
    const int nA = strideA ? batch : 1, nB = strideB ? batch : 1;
    const double2 *Y, *A, *B;
    double2 *S, *PA, *PB, *T, *ws;
    double *rcA, *rcB, *rcd;
    Pinv64 pvA, pvB;
    Slab s(st);
    JSTSP_TRY(ws64_open(s, nm, batch, [&](Slab &w, int b) {
        const int bA = strideA ? b : 1, bB = strideB ? b : 1;
        const size_t eA = (size_t)N * Gr * bA, eB = (size_t)G2 * M * bB;
        Y = w.in(reinterpret_cast<const double2 *>(Y_), (size_t)N * M * b, host);
        A = w.in(reinterpret_cast<const double2 *>(A_), eA, host);
        B = w.in(reinterpret_cast<const double2 *>(B_), eB, host);
        S = w.out(reinterpret_cast<double2 *>(S_out), (size_t)Gr * G2 * b, host);
        PA = w.get<double2>(eA); PB = w.get<double2>(eB); T = w.get<double2>((size_t)Gr * M * b);
        ws = w.get<double2>(std::max<size_t>(1, std::max(zgemm64_ws_elems(Gr, M, N, b), zgemm64_ws_elems(Gr, G2, M, b))));
        rcA = w.get<double>(bA); rcB = w.get<double>(bB); rcd = w.get<double>(2);
        pvA.layout(w, N, Gr, bA);
        pvB.layout(w, G2, M, bB);
    }));
    double *rc2 = rcond_out;
    // a shared factor is inverted once for the call
    JSTSP_TRY(pinv64_run(st, pvA, N, Gr, nA, A, (long long)N * Gr, PA, rcA, nullptr));
    JSTSP_TRY(pinv64_run(st, pvB, G2, M, nB, B, (long long)G2 * M, PB, rcB, nullptr));
    JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, M, N, batch, Mat64{PA, strideA ? (long long)Gr * N : 0, Gr}, Mat64{Y, (long long)N * M, N}, T, (long long)Gr * M, Gr,
                      ws));
    JSTSP_TRY(zgemm64(st, 'N', 'N', Gr, G2, M, batch, Mat64{T, (long long)Gr * M, Gr}, Mat64{PB, strideB ? (long long)M * G2 : 0, M}, S, (long long)Gr * G2,
                      Gr, ws));
    if (rcond_out) {
        if (host) rc2 = rcd;
        JSTSP_TRY(pinv64_min(st, nA, rcA, rc2));
        JSTSP_TRY(pinv64_min(st, nB, rcB, rc2 + 1));
        if (host) JSTSP_TRY(s.copy_back(rcond_out, rcd, 2));
    }
    if (host) JSTSP_TRY(s.copy_back(reinterpret_cast<double2 *>(S_out), S, (size_t)Gr * G2 * batch));
    JSTSP_HIP(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
