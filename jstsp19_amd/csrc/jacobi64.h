// The in-LDS one-sided (Hestenes) Jacobi of the float64 singular-value kernels (internal): the power-of-two prescale, the cyclic
// sweeps and the sorted column norms that svdvals.hip (values only) and svd64.hip (values and vectors) share - ONE sweep loop.
// A column of the operand is a run of `m` consecutive 16-byte elements followed by `extra` more that are rotated along with it
// but take no part in the inner products: svd64.hip keeps the accumulated rotations V there (column j of V under column j of the
// operand), svdvals.hip passes 0 and gets the bits it always had.  Everything sits in an anonymous namespace (no relocatable
// device code).
#pragma once
#include "common.h"

#include <algorithm>

namespace jstsp {
namespace {

constexpr int SV_NMAX = 64;         // columns: min(rows, cols)
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

inline int sv_threads(int n) { return 64 * std::max(1, std::min(SV_WAVES, (n + 1) / 2)); }

// Scale the m x n operand in A (LDS, column stride m + extra, written by this workgroup, not yet synchronised) by the power of
// two that brings max(|re|, |im|) into [1/2, 1).  Returns true when an entry is not finite; *unscale: the factor that undoes the
// scaling; *fro2: the squared Frobenius norm of the scaled matrix.  The `extra` elements under each column are not touched.
// Entry e of the m n operand entries goes to thread e mod blockDim whatever `extra` is: the sums do not depend on it.
__device__ bool prescale(double2 *A, int m, int extra, int n, double *red, double *unscale, double *fro2)
{
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    const int count = m * n;
    __syncthreads();
    double amax = 0.0;
    int bad = 0;
    for (int e = tid; e < count; e += blockDim.x) {
        const double2 v = A[extra ? e + extra * (e / m) : e];
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
        const int a = extra ? e + extra * (e / m) : e;
        const double2 v = make_double2(A[a].x * sc, A[a].y * sc);
        A[a] = v;
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

// Cyclic one-sided Jacobi on the n columns (length m, column stride m + extra) of A in LDS; every thread of the workgroup calls
// it.  The inner products of a pair run over the first m entries of the two columns, the rotation over all m + extra.
// A column whose norm has fallen to eps |A|_F / sqrt(n) is left alone: it is a zero singular value to working accuracy
// (ignoring all such columns moves no singular value by more than eps |A|_F), while rotating it against the others would go
// on for as many sweeps as it takes its rounding residue - a factor eps smaller each time - to underflow.
// Returns true when a sweep rotated nothing, false when the cap of SV_SWEEPS sweeps ended the iteration.
__device__ bool jacobi_sweeps(double2 *A, int m, int extra, int n, double fro2)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const int ne = n + (n & 1), half = ne / 2, ring = ne - 1;      // odd n: one idle slot per round
    const int ld = m + extra;
    const double eps = 2.220446049250313e-16, tol = sqrt((double)m) * eps, floor2 = fro2 * eps * eps / (double)n;
    for (int sweep = 0; sweep < SV_SWEEPS; ++sweep) {
        int rotated = 0;
        for (int r = 0; r < ring; ++r) {                           // round-robin: ring rounds of `half` disjoint pairs
            for (int k = w; k < half; k += nw) {
                const int u = k == 0 ? ring : (r + k) % ring, v = k == 0 ? r : (r + ring - k) % ring;
                const int p = min(u, v), q = max(u, v);
                if (q >= n) continue;
                double2 *cp = A + (size_t)ld * p, *cq = A + (size_t)ld * q;
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
                for (int i = lane; i < ld; i += 64) {
                    const double2 x = cp[i], y = cq[i];
                    const double yr = y.x * wr + y.y * wi, yi = y.y * wr - y.x * wi;      // y conj(w)
                    cp[i] = make_double2(c * x.x - s * yr, c * x.y - s * yi);
                    cq[i] = make_double2(s * x.x + c * yr, s * x.y + c * yi);
                }
            }
            __syncthreads();
        }
        if (!__syncthreads_or(rotated)) return true;
    }
    return false;
}

// nrm[j] = |column j of A| over its first m entries (column stride m + extra), j < n; ends with a barrier.
__device__ void column_norms(const double2 *A, int m, int extra, int n, double *nrm)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    for (int j = w; j < n; j += nw) {
        double a = 0.0;
        for (int i = lane; i < m; i += 64) {
            const double2 x = A[i + (size_t)(m + extra) * j];
            a += x.x * x.x + x.y * x.y;
        }
        a = wave_sum(a);
        if (lane == 0) nrm[j] = sqrt(a);
    }
    __syncthreads();
}

// the place of nrm[i] in descending order; equal norms keep column order
__device__ __forceinline__ int norm_place(const double *nrm, int n, int i)
{
    const double v = nrm[i];
    int place = 0;
    for (int k = 0; k < n; ++k) place += (nrm[k] > v) || (nrm[k] == v && k < i);
    return place;
}

// The first n_keep column norms of A in descending order, times unscale, to out.  nrm: n doubles of LDS.
__device__ void sorted_norms(const double2 *A, int m, int extra, int n, double *nrm, double unscale, int n_keep, double *out)
{
    column_norms(A, m, extra, n, nrm);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const int place = norm_place(nrm, n, i);
        if (place < n_keep) out[place] = nrm[i] * unscale;
    }
}

}  // namespace
}  // namespace jstsp
