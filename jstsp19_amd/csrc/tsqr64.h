// The tall-skinny Householder QR in front of the in-LDS Jacobi (internal): the chunk rule, the scale pre-pass of a matrix operand
// and the reduction [R; chunk] -> R that svdvals.hip (values only: tsqr_values_kernel) and svd64.hip (values and vectors:
// svd64_tall_forward_kernel, which keeps the reflectors) share - ONE reduction.  Everything sits in an anonymous namespace (no
// relocatable device code).
#pragma once
#include "jacobi64.h"

namespace jstsp {
namespace {

constexpr int TQ_THREADS = 512;
constexpr int TQ_NMAX = SV_NMAX;    // the triangle goes to the in-LDS Jacobi
constexpr int TQ_MMAX = 65536;
constexpr int TQ_PRE = 12;          // chunk entries a thread fetches ahead: 128 * 48 / 512

__host__ __device__ inline int tq_chunk(int n) { return n <= 48 ? 128 : 64; }             // rows per chunk: R and the chunk within 144 KiB
inline size_t tq_lds_bytes(int n) { return ((size_t)n * n + (size_t)tq_chunk(n) * n) * sizeof(double2); }
inline bool tq_fits(int rows, int cols) { return std::min(rows, cols) <= TQ_NMAX && std::max(rows, cols) <= TQ_MMAX; }

// the largest of v over the workgroup and whether any thread saw a non-finite entry (red: 8 doubles of LDS)
__device__ __forceinline__ bool block_max_or_bad(double &amax, int bad, double *red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) amax = fmax(amax, __shfl_xor(amax, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = amax;
    if (__syncthreads_or(bad)) return true;
    amax = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) amax = fmax(amax, red[i]);
    return false;
}

// Loaders of the reduction kernels: bind(t) selects matrix t; scan() is the pre-pass - true when an entry is not finite, else *ex is
// the exponent whose power of two the entries are divided by; at(r, c, sc) is entry (r, c) of the rows x cols operand times sc.
template <class T> struct MatrixLoader {
    const T *Y;
    int rows, cols;
    __device__ void bind(int t) { Y += (size_t)rows * cols * t; }
    __device__ bool scan(double *red, int *ex) const
    {
        double amax = 0.0;
        int bad = 0;
        for (int e = threadIdx.x; e < rows * cols; e += blockDim.x) {
            const double2 v = ld2(Y[e]);
            bad |= !isfinite(v.x) || !isfinite(v.y);
            amax = fmax(amax, fmax(fabs(v.x), fabs(v.y)));
        }
        if (block_max_or_bad(amax, bad, red)) return true;
        int e2 = 0;
        if (amax > 0.0) frexp(amax, &e2);
        *ex = max(-1000, min(1000, e2));
        return false;
    }
    __device__ __forceinline__ double2 at(int r, int c, double sc) const
    {
        const double2 v = ld2(Y[r + (size_t)rows * c]);
        return make_double2(v.x * sc, v.y * sc);
    }
};

// a loader like MatrixLoader: the difference S - Z of two operands, formed in float64 entry by entry as it is loaded and never
// stored; the scale comes from the largest component of the difference itself, which may be 1e-9 of the operands'
template <class T> struct DiffLoader {
    const T *S, *Z;
    int rows, cols;
    __device__ void bind(int t) { S += (size_t)rows * cols * t; Z += (size_t)rows * cols * t; }
    __device__ bool scan(double *red, int *ex) const
    {
        double amax = 0.0;
        int bad = 0;
        for (int e = threadIdx.x; e < rows * cols; e += blockDim.x) {
            const double2 s = ld2(S[e]), z = ld2(Z[e]);
            const double dx = s.x - z.x, dy = s.y - z.y;
            bad |= !isfinite(dx) || !isfinite(dy);
            amax = fmax(amax, fmax(fabs(dx), fabs(dy)));
        }
        if (block_max_or_bad(amax, bad, red)) return true;
        int e2 = 0;
        if (amax > 0.0) frexp(amax, &e2);
        *ex = max(-1000, min(1000, e2));
        return false;
    }
    __device__ __forceinline__ double2 at(int r, int c, double sc) const
    {
        const size_t e = r + (size_t)rows * c;
        const double2 s = ld2(S[e]), z = ld2(Z[e]);
        return make_double2((s.x - z.x) * sc, (s.y - z.y) * sc);
    }
};

// [R; chunk] -> R: column j's reflector P = I - u u^H / (|x| (|x| + |alpha|)), x = (alpha; y) with alpha = R(j, j) and y the chunk's
// column j, u = x - beta e_1, beta = -(alpha / |alpha|) |x| (no cancellation in u_1), applied to the columns k > j, one wave
// per column.  Every wave forms the reflector itself from the same numbers in the same order, so none waits for another; one
// barrier per column.  R: n x n, ld n; Ck: the chunk, cc rows, ld C.  A column whose chunk part is zero is left as it is.
// Column j of the chunk is not touched after step j: on return the chunk holds the reflector tails y_j.  KEEP: the head of
// reflector j goes to refl[3 j ..] (global memory) as u_1 (re, im) and 1 / (|x| (|x| + |alpha|)), 0 for a column left as it is;
// the arithmetic and the values-only instantiation are the same with and without it.
template <bool KEEP = false> __device__ void tq_reduce(double2 *R, double2 *Ck, int n, int C, int cc, double *refl = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    for (int j = 0; j < n; ++j) {
        const double2 *y = Ck + (size_t)C * j;
        double s2 = 0.0;
        for (int i = lane; i < cc; i += 64) s2 += y[i].x * y[i].x + y[i].y * y[i].y;
        s2 = wave_sum(s2);
        if (!(s2 > 0.0)) {                                         // (the same bits in every wave)
            if constexpr (KEEP)
                if (tid == 0) refl[3 * j + 2] = 0.0;
            continue;
        }
        const double2 alpha = R[j + (size_t)n * j];
        const double aa = hypot(alpha.x, alpha.y), nx = sqrt(aa * aa + s2);
        const double px = aa > 0.0 ? alpha.x / aa : 1.0, py = aa > 0.0 ? alpha.y / aa : 0.0;
        const double u0x = px * (aa + nx), u0y = py * (aa + nx), inv = 1.0 / (nx * (nx + aa));
        if constexpr (KEEP)
            if (tid == 0) {
                refl[3 * j] = u0x;
                refl[3 * j + 1] = u0y;
                refl[3 * j + 2] = inv;
            }
        for (int k = j + 1 + w; k < n; k += nw) {
            double2 *a = Ck + (size_t)C * k;
            double dr = 0.0, di = 0.0;
            for (int i = lane; i < cc; i += 64) {
                const double2 yy = y[i], v = a[i];
                dr += yy.x * v.x + yy.y * v.y;                     // conj(y) a
                di += yy.x * v.y - yy.y * v.x;
            }
            dr = wave_sum(dr); di = wave_sum(di);
            const double2 rjk = R[j + (size_t)n * k];
            dr += u0x * rjk.x + u0y * rjk.y;                       // conj(u_1) R(j, k)
            di += u0x * rjk.y - u0y * rjk.x;
            const double fr = dr * inv, fi = di * inv;
            if (lane == 0) R[j + (size_t)n * k] = make_double2(rjk.x - (u0x * fr - u0y * fi), rjk.y - (u0x * fi + u0y * fr));
            for (int i = lane; i < cc; i += 64) {
                const double2 yy = y[i], v = a[i];
                a[i] = make_double2(v.x - (yy.x * fr - yy.y * fi), v.y - (yy.x * fi + yy.y * fr));
            }
        }
        __syncthreads();
        if (tid == 0) R[j + (size_t)n * j] = make_double2(-px * nx, -py * nx);
    }
}

}  // namespace
}  // namespace jstsp
