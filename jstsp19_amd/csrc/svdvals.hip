// Singular values in float64 by one-sided (Hestenes) Jacobi, and the spectrum sweep of plot_rankR.m:
//
//   plot_rankR.m:49 ([U,S,V] = svd(Y); only diag(S) is used) -> svdvals_kernel: the singular values of given matrices
//   plot_rankR.m:24-50                                        -> rank_sweep_kernel: the channel and pilots of
//                                                                jstsp_build_trials_c32's trial t, the noise-free
//                                                                Y = sum_l H_l Psi_bar_l (proposed_hbf.m:15-20), its values
//
// Why not a Gram: the other spectral kernels of the library (eig*.hip, vamp64.hip) decompose Y Y^H, whose condition number is
// the square of Y's, so a zero singular value comes back near sqrt(eps) sigma_1 even in float64 - and the figure is about
// exactly that tail.  Here the rotations act on the columns of Y itself: one workgroup holds the matrix in LDS as complex
// double, oriented to n = min(rows, cols) columns of length m = max(rows, cols) (Y^H when rows < cols), and runs cyclic sweeps
// over the column pairs.  For a pair (p, q): a = |c_p|^2, b = |c_q|^2, g = c_p^H c_q; if |g| > tol sqrt(a b) the plane rotation
//   c_p <- c c_p - s w* c_q,  c_q <- s c_p + c w* c_q,   w = g / |g|,  t = sign(z) / (|z| + sqrt(1 + z^2)),  z = (b - a) / (2 |g|)
// makes the two columns orthogonal.  The n/2 disjoint pairs of a round-robin round run in parallel, one wave per pair with
// the three inner products by wave reductions; a column is a run of consecutive 16-byte elements, so the 64 lanes of a wave
// read whole 256-byte bank rows without conflicts.  The loop ends when a full sweep rotates nothing, or after SV_SWEEPS
// sweeps.  The singular values are the final column norms, sorted; no singular vector is formed.  The operand is scaled by a
// power of two to max |entry| in [1/2, 1) first (exact), so no squared norm overflows or underflows; a non-finite entry
// gives NaN for that matrix.  Columns that have shrunk to eps |Y|_F / sqrt(n) are not rotated any further (jacobi_sweeps).
#include "inputgen.h"

using namespace jstsp;

namespace {

constexpr int SV_NMAX = 64;         // columns: min(rows, cols)
constexpr int SV_ELEMS = 8192;      // rows * cols: 128 KiB of complex double in LDS
constexpr int SV_SWEEPS = 30;       // cap (converged inputs stop after 5 to 9)
constexpr int SV_WAVES = 8;
constexpr int SV_RED = 16;          // doubles of LDS for the block reduction

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double2 ld2(const float2 &v) { return make_double2(v.x, v.y); }
__device__ __forceinline__ double2 ld2(const double2 &v) { return v; }

// Scale the `count` entries of A (LDS, written by this workgroup, not yet synchronised) by the power of two that brings
// max(|re|, |im|) into [1/2, 1).  Returns true when an entry is not finite; *unscale: the factor that undoes the scaling;
// *fro2: the squared Frobenius norm of the scaled matrix.
__device__ bool prescale(double2 *A, int count, double *red, double *unscale, double *fro2)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    __syncthreads();
    double amax = 0.0;
    int bad = 0;
    for (int e = tid; e < count; e += blockDim.x) {
        const double2 v = A[e];
        bad |= !isfinite(v.x) || !isfinite(v.y);
        amax = fmax(amax, fmax(fabs(v.x), fabs(v.y)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
    if (lane == 0) red[w] = amax;
    if (__syncthreads_or(bad)) return true;
    amax = 0.0;
    for (int i = 0; i < nw; ++i) amax = fmax(amax, red[i]);
    int ex = 0;
    if (amax > 0.0) frexp(amax, &ex);
    ex = max(-1000, min(1000, ex));
    const double sc = ldexp(1.0, -ex);
    double f2 = 0.0;
    for (int e = tid; e < count; e += blockDim.x) {
        const double2 v = make_double2(A[e].x * sc, A[e].y * sc);
        A[e] = v;
        f2 += v.x * v.x + v.y * v.y;
    }
    f2 = wave_sum(f2);
    __syncthreads();                                               // every wave has read the maxima
    if (lane == 0) red[w] = f2;
    __syncthreads();
    f2 = 0.0;
    for (int i = 0; i < nw; ++i) f2 += red[i];
    *unscale = ldexp(1.0, ex);
    *fro2 = f2;
    return false;
}

// Cyclic one-sided Jacobi on the n columns (length m, column-major) of A in LDS; every thread of the workgroup calls it.
// A column whose norm has fallen to eps |A|_F / sqrt(n) is left alone: it is a zero singular value to working accuracy
// (ignoring all such columns moves no singular value by more than eps |A|_F), while rotating it against the others would go
// on for as many sweeps as it takes its rounding residue - a factor eps smaller each time - to underflow.
__device__ void jacobi_sweeps(double2 *A, int m, int n, double fro2)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int ne = n + (n & 1), half = ne / 2, ring = ne - 1;      // odd n: one idle slot per round
    const double eps = 2.220446049250313e-16, tol = sqrt((double)m) * eps, floor2 = fro2 * eps * eps / (double)n;
    for (int sweep = 0; sweep < SV_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int r = 0; r < ring; ++r) {                           // round-robin: ring rounds of `half` disjoint pairs
            for (int k = w; k < half; k += nw) {
                const int u = k == 0 ? ring : (r + k) % ring, v = k == 0 ? r : (r + ring - k) % ring;
                const int p = min(u, v), q = max(u, v);
                if (q >= n) continue;
                double2 *cp = A + (size_t)m * p, *cq = A + (size_t)m * q;
                double a = 0.0, b = 0.0, gr = 0.0, gi = 0.0;
                for (int i = lane; i < m; i += 64) {
                    const double2 x = cp[i], y = cq[i];
                    a += x.x * x.x + x.y * x.y;
                    b += y.x * y.x + y.y * y.y;
                    gr += x.x * y.x + x.y * y.y;                   // conj(x) y
                    gi += x.x * y.y - x.y * y.x;
                }
                a = wave_sum(a); b = wave_sum(b); gr = wave_sum(gr); gi = wave_sum(gi);
                const double g = hypot(gr, gi);
                if (a <= floor2 || b <= floor2 || !(g > tol * sqrt(a) * sqrt(b))) continue;
                rotated = 1;
                const double z = (b - a) / (2.0 * g);
                const double t = copysign(1.0, z) / (fabs(z) + hypot(1.0, z));
                const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
                const double wr = gr / g, wi = gi / g;
                for (int i = lane; i < m; i += 64) {
                    const double2 x = cp[i], y = cq[i];
                    const double yr = y.x * wr + y.y * wi, yi = y.y * wr - y.x * wi;      // y conj(w)
                    cp[i] = make_double2(c * x.x - s * yr, c * x.y - s * yi);
                    cq[i] = make_double2(s * x.x + c * yr, s * x.y + c * yi);
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated)) break;
    }
}

// The first n_keep column norms of A in descending order, times unscale, to out.  nrm: n doubles of LDS.
__device__ void sorted_norms(const double2 *A, int m, int n, double *nrm, double unscale, int n_keep, double *out)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int j = w; j < n; j += nw) {
        double a = 0.0;
        for (int i = lane; i < m; i += 64) {
            const double2 x = A[i + (size_t)m * j];
            a += x.x * x.x + x.y * x.y;
        }
        a = wave_sum(a);
        if (lane == 0) nrm[j] = sqrt(a);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const double v = nrm[i];
        int rank = 0;
        for (int k = 0; k < n; ++k) rank += (nrm[k] > v) || (nrm[k] == v && k < i);
        if (rank < n_keep) out[rank] = v * unscale;
    }
}

// After A (m x n, oriented) has been written: scale, sweep, sort.  LDS behind A: n doubles (norms), SV_RED doubles.
__device__ void singular_values_block(double2 *A, int m, int n, int n_keep, double *out)
{
    double *nrm = reinterpret_cast<double *>(A + (size_t)m * n), *red = nrm + n;
    double unscale, fro2;
    if (prescale(A, m * n, red, &unscale, &fro2)) {
        for (int i = threadIdx.x; i < n_keep; i += blockDim.x) out[i] = __builtin_nan("");
        return;
    }
    jacobi_sweeps(A, m, n, fro2);
    sorted_norms(A, m, n, nrm, unscale, n_keep, out);
}

inline size_t sv_lds_bytes(int m, int n) { return (size_t)m * n * sizeof(double2) + (size_t)(n + SV_RED) * sizeof(double); }
inline int sv_threads(int n) { return 64 * std::max(1, std::min(SV_WAVES, (n + 1) / 2)); }
inline bool sv_fits(int rows, int cols) { return std::min(rows, cols) <= SV_NMAX && (long long)rows * cols <= SV_ELEMS; }

template <class T> __global__ __launch_bounds__(64 * SV_WAVES) void svdvals_kernel(int rows, int cols, const T *Y, double *sv)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x;
    const bool tall = rows >= cols;
    const int m = tall ? rows : cols, n = tall ? cols : rows;
    const T *Yt = Y + (size_t)rows * cols * t;
    for (int e = threadIdx.x; e < rows * cols; e += blockDim.x) {
        const double2 v = ld2(Yt[e]);
        if (tall) lds[e] = v;
        else lds[e / rows + m * (e % rows)] = make_double2(v.x, -v.y);            // Y^H
    }
    singular_values_block(lds, m, n, n, sv + (size_t)n * t);
}

// One workgroup per trial: Y = [H_1 .. H_L] Psi (proposed_hbf.m:15-20 with N = 0), Nr x Tp, in LDS, then its singular values.
__global__ __launch_bounds__(64 * SV_WAVES) void rank_sweep_kernel(Model mdl, const float2 *Hmat, const float2 *psym, float pscale,
                                                                   int n_keep, double *sv)
{
    extern __shared__ double2 lds[];
    const int t = blockIdx.x;
    const bool tall = mdl.Nr >= mdl.Tp;
    const int m = tall ? mdl.Nr : mdl.Tp, n = tall ? mdl.Tp : mdl.Nr;
    const float2 *H = Hmat + (size_t)t * mdl.Nr * mdl.NtL;
    const float2 *sym = psym + (size_t)t * mdl.Nt * mdl.Tp;
    for (int e = threadIdx.x; e < mdl.Nr * mdl.Tp; e += blockDim.x) {
        const int r = e % mdl.Nr, j = e / mdl.Nr;
        const double2 v = received_entry(mdl, H, sym, pscale, r, j);
        if (tall) lds[e] = v;
        else lds[j + m * r] = make_double2(v.x, -v.y);
    }
    singular_values_block(lds, m, n, n_keep, sv + (size_t)n_keep * t);
}

template <class T>
int singular_values_impl(jstsp_ctx *ctx, int rows, int cols, int batch, const T *Y, double *sv, int memspace, const char *what)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "%s: NULL context", what);
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "%s: bad memspace", what);
    JSTSP_REQUIRE(Y && sv, JSTSP_E_NULL, "%s: NULL argument", what);
    JSTSP_REQUIRE(rows > 0 && cols > 0 && batch > 0, JSTSP_E_SHAPE, "%s: bad shape", what);
    JSTSP_REQUIRE(sv_fits(rows, cols), JSTSP_E_UNSUPPORTED, "%s: need min(rows, cols) <= %d and rows * cols <= %d", what, SV_NMAX,
                  SV_ELEMS);
    JSTSP_ENTER(ctx);
    const int m = std::max(rows, cols), n = std::min(rows, cols);
    const size_t nY = (size_t)rows * cols * batch, nS = (size_t)n * batch;
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(ctx->arena.reserve(rnd256(nY * sizeof(T)) + rnd256(nS * 8) + 4096));
        ctx->arena.reset();
    }
    const T *y;
    JSTSP_TRY(stage_in(ctx, Y, nY, memspace, &y));
    double *o = memspace == JSTSP_DEVICE ? sv : ctx->arena.get<double>(nS);
    JSTSP_REQUIRE(o, JSTSP_E_NOMEM, "%s: workspace exhausted", what);
    const size_t sh = sv_lds_bytes(m, n);
    JSTSP_HIP(hipFuncSetAttribute((const void *)svdvals_kernel<T>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    svdvals_kernel<T><<<batch, sv_threads(n), sh, ctx->stream>>>(rows, cols, y, o);
    JSTSP_HIP(hipGetLastError());
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(stage_out(ctx, sv, o, nS, memspace));
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

}  // namespace

extern "C" {

int jstsp_singular_values_c32(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c32 *Y, double *sv, int memspace)
{
    return singular_values_impl(ctx, rows, cols, batch, reinterpret_cast<const float2 *>(Y), sv, memspace, "singular_values_c32");
}

int jstsp_singular_values_c64(jstsp_ctx *ctx, int rows, int cols, int batch, const jstsp_c64 *Y, double *sv, int memspace)
{
    return singular_values_impl(ctx, rows, cols, batch, reinterpret_cast<const double2 *>(Y), sv, memspace, "singular_values_c64");
}

int jstsp_rank_trials_c32(jstsp_ctx *ctx, const jstsp_model *mp, uint64_t seed, int sweep_idx, long long trial0, int batch,
                          int n_keep, double *sv, int memspace)
{
    JSTSP_REQUIRE(ctx, JSTSP_E_NULL, "rank_trials: NULL context");
    JSTSP_REQUIRE(memspace == JSTSP_HOST || memspace == JSTSP_DEVICE, JSTSP_E_ARG, "rank_trials: bad memspace");
    JSTSP_REQUIRE(mp && sv, JSTSP_E_NULL, "rank_trials: NULL argument");
    JSTSP_ENTER(ctx);
    Model m{};
    m.Nt = mp->Nt; m.Nr = mp->Nr; m.L = mp->L; m.Tp = mp->T_prop; m.clusters = mp->clusters; m.rays = mp->rays;
    JSTSP_REQUIRE(m.Nt > 0 && m.Nr > 0 && m.L > 0 && m.Tp > 0 && m.clusters > 0 && m.rays > 0 && batch > 0 && trial0 >= 0 &&
                      sweep_idx >= 0,
                  JSTSP_E_SHAPE, "rank_trials: bad model dimensions");
    JSTSP_REQUIRE(m.L <= m.Tp, JSTSP_E_SHAPE, "rank_trials: L > T_prop");
    JSTSP_REQUIRE(mp->pilots == JSTSP_PILOTS_QAM4 || mp->pilots == JSTSP_PILOTS_GAUSS, JSTSP_E_ARG, "rank_trials: bad pilots kind");
    const int rows = m.Nr, cols = m.Tp, n = std::min(rows, cols), mm = std::max(rows, cols);
    JSTSP_REQUIRE(n_keep >= 1 && n_keep <= n, JSTSP_E_SHAPE, "rank_trials: need 1 <= n_keep <= min(Nr, T_prop)");
    m.Np = m.clusters * m.rays; m.NtL = m.Nt * m.L;
    JSTSP_REQUIRE(sv_fits(rows, cols) && channel_lds_bytes(m) <= 150 * 1024, JSTSP_E_UNSUPPORTED,
                  "rank_trials: need min(Nr, T_prop) <= %d and Nr * T_prop <= %d", SV_NMAX, SV_ELEMS);
    const size_t nS = (size_t)n_keep * batch;
    JSTSP_TRY(ctx->arena.reserve(operands_bytes(m, (size_t)batch) + rnd256(nS * 8) + 4096));
    ctx->arena.reset();
    Operands op;
    JSTSP_TRY(draw_operands(ctx, m, mp, seed, (uint64_t)sweep_idx, trial0, batch, &op));
    double *o = memspace == JSTSP_DEVICE ? sv : ctx->arena.get<double>(nS);
    JSTSP_REQUIRE(o, JSTSP_E_NOMEM, "rank_trials: workspace exhausted");
    const size_t sh = sv_lds_bytes(mm, n);
    JSTSP_HIP(hipFuncSetAttribute((const void *)rank_sweep_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh));
    rank_sweep_kernel<<<batch, sv_threads(n), sh, ctx->stream>>>(m, op.Hmat, op.psym, op.pscale, n_keep, o);
    JSTSP_HIP(hipGetLastError());
    if (memspace == JSTSP_HOST) {
        JSTSP_TRY(stage_out(ctx, sv, o, nS, memspace));
        JSTSP_HIP(hipStreamSynchronize(ctx->stream));
    }
    return 0;
}

}  // extern "C"
