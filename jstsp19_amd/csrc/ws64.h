// Host plumbing and device helpers shared by the float64 entry points (internal): the per-call workspace slab, which measures a
// layout and then lays it out with the same code, the refusal above the family's 24 GiB limit, host <-> device staging, and the
// complex and reduction helpers of the float64 kernels.  Everything sits in an anonymous namespace: each file that includes this
// compiles its own copy (no relocatable device code).
#pragma once
#include "common.h"

#include <algorithm>
#include <cfloat>

namespace jstsp {
namespace {

constexpr size_t WS64_LIMIT = (size_t)24 << 30;        // the largest per-call workspace of the float64 family

// ---- device helpers ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double2 zmul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 zconj(double2 a) { return make_double2(a.x, -a.y); }

__device__ __forceinline__ double wave_sum64(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// x^2 + y^2 from two rounded squares and one sum (symmetric in x and y whatever the compiler would like to contract)
__device__ __forceinline__ double abs2_sym(double x, double y)
{
#pragma clang fp contract(off)
    const double a = x * x, b = y * y;
    return a + b;
}

// conj(u)^T v: (sum ux vx, sum uy vy, sum ux vy, sum uy vx), c = (xx + yy, xy - yx)
struct Dot4 {
    double xx, yy, xy, yx;
};
__device__ __forceinline__ void dot4_step(Dot4 &d, double2 u, double2 v)
{
    d.xx = fma(u.x, v.x, d.xx);
    d.yy = fma(u.y, v.y, d.yy);
    d.xy = fma(u.x, v.y, d.xy);
    d.yx = fma(u.y, v.x, d.yx);
}

// ---- the tie-safe append of omp64.hip and mmv_omp64.hip (workgroups of 256 threads, every thread calls).  The order of every fma
// and sum below is a contract: exact ties between columns equal up to a factor -1 or +-1i, and the scale invariance, depend on it.

// the sum of v over the workgroup: xor tree per wave, then the four waves in order (sh: 4 doubles; one barrier before the
// write, which also publishes what the workgroup stored before the call, and one after)
__device__ __forceinline__ double block_sum64(double v, double *sh)
{
    v = wave_sum64(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sh[0] + sh[1]) + (sh[2] + sh[3]);
}

// e of frexp for the largest finite |component| of v[0 .. n) (0 when there is none or it is 0): v 2^-e has it in [0.5, 1), and
// the scaling is exact unless a component underflows (sh: 4 doubles, barriers as block_sum64)
__device__ __forceinline__ int finite_max_exponent(const double2 *v, long long n, double *sh)
{
    double vmax = 0.0;
    for (long long e = threadIdx.x; e < n; e += 256) {
        const double ax = fabs(v[e].x), ay = fabs(v[e].y);
        if (ax <= DBL_MAX) vmax = fmax(vmax, ax);                 // (not NaN, not Inf)
        if (ay <= DBL_MAX) vmax = fmax(vmax, ay);
    }
    for (int o = 32; o > 0; o >>= 1) vmax = fmax(vmax, __shfl_xor(vmax, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = vmax;
    __syncthreads();
    vmax = fmax(fmax(sh[0], sh[1]), fmax(sh[2], sh[3]));
    int ev = 0;
    if (vmax > 0.0) (void)frexp(vmax, &ev);
    return ev;
}

// q (len entries, already published by a barrier) is orthogonalised against the k orthonormal columns of Q (len x k) by two passes
// of classical Gram-Schmidt: the k dot products d_j = q_j^H q of a pass are independent, one wave per j; D[j] = d_j (k entries,
// LDS or global) and Rcol[j] += d_j, the column of the triangular factor; then q -= sum_j q_j d_j with j ascending.  Returns
// ||q||^2 after the passes, summed per thread in one fma chain over tid, tid + 256, ... and then over the workgroup.
__device__ __forceinline__ double cgs2_append(double2 *q, const double2 *Q, int len, int k, double2 *Rcol, double2 *D, double *sh)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int pass = 0; pass < 2 && k > 0; ++pass) {
        for (int j = wave; j < k; j += 4) {
            const double2 *qj = Q + (long long)len * j;
            Dot4 d = {0.0, 0.0, 0.0, 0.0};
            for (int e = lane; e < len; e += 64) dot4_step(d, qj[e], q[e]);
            const double dx = wave_sum64(d.xx + d.yy), dy = wave_sum64(d.xy - d.yx);
            if (lane == 0) {
                D[j] = make_double2(dx, dy);
                Rcol[j] = make_double2(Rcol[j].x + dx, Rcol[j].y + dy);
            }
        }
        __syncthreads();
        for (int e = tid; e < len; e += 256) {
            double2 v = q[e];
            for (int j = 0; j < k; ++j) {
                const double2 w = Q[(long long)len * j + e], d = D[j];
                v.x -= d.x * w.x - d.y * w.y;
                v.y -= d.x * w.y + d.y * w.x;
            }
            q[e] = v;
        }
        __syncthreads();
    }
    double n1 = 0.0;
    for (int e = tid; e < len; e += 256) {
        const double2 v = q[e];
        n1 = fma(v.x, v.x, n1);
        n1 = fma(v.y, v.y, n1);
    }
    return block_sum64(n1, sh);
}

// ---- workspace: one stream-ordered slab, bump allocation -----------------------------------------------------------------------
// An entry point states its arrays once, as a function of (Slab &, batch).  On a slab without memory (before reserve()) that
// function only measures: get() advances the offset and returns nullptr, in() uploads nothing.  After reserve() the same calls
// hand out the arrays, 256-byte aligned, and in() uploads in the order of the calls.  ws64_open() runs the two passes.
struct Slab {
    hipStream_t st;
    char *base = nullptr;
    size_t off = 0;
    hipError_t err = hipSuccess;            // the first staged upload that failed
    explicit Slab(hipStream_t s) : st(s) {}
    Slab(const Slab &) = delete;
    ~Slab() { if (base) (void)hipFreeAsync(base, st); }
    int reserve(size_t bytes, const char *nm)
    {
        const hipError_t e = hipMallocAsync((void **)&base, std::max<size_t>(bytes, 256), st);
        if (e != hipSuccess) { base = nullptr; set_error("%s: hipMallocAsync(%zu) failed: %s", nm, bytes, hipGetErrorString(e)); return JSTSP_E_NOMEM; }
        off = 0;
        return 0;
    }
    template <class T> T *get(size_t n)
    {
        T *p = base ? reinterpret_cast<T *>(base + off) : nullptr;
        off += (n * sizeof(T) + 255) & ~(size_t)255;
        return p;
    }
    // an input of n elements: the caller's array when it is on the device, otherwise a copy staged here
    template <class T> const T *in(const T *caller, size_t n, bool host)
    {
        if (!host) return caller;
        T *p = get<T>(n);
        if (base && err == hipSuccess) err = hipMemcpyAsync(p, caller, n * sizeof(T), hipMemcpyHostToDevice, st);
        return p;
    }
    // an output of n elements: the caller's array when it is on the device, otherwise an array here (copy_back() returns it)
    template <class T> T *out(T *caller, size_t n, bool host) { return host ? get<T>(n) : caller; }
    template <class T> int copy_back(T *caller, const T *dev, size_t n) const
    {
        JSTSP_HIP(hipMemcpyAsync(caller, dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
        return 0;
    }
};

// Opens the workspace of a call: layout(s, batch) is measured, refused above WS64_LIMIT with the largest batch that would fit
// (found by measuring again), otherwise allocated once and laid out.  The measuring passes touch neither HIP nor the arrays.
template <class Layout> int ws64_open(Slab &s, const char *nm, int batch, Layout &&layout)
{
    auto bytes = [&](int b) {
        Slab m(s.st);
        layout(m, b);
        return m.off;
    };
    const size_t need = bytes(batch);
    if (need > WS64_LIMIT) {
        int fit = batch;
        while (fit > 1 && bytes(fit) > WS64_LIMIT) fit = fit > 64 ? fit - fit / 16 : fit - 1;
        set_error("%s: the float64 workspace would be %.1f GiB (limit 24); the largest batch that fits is about %d", nm,
                  (double)need / (double)((size_t)1 << 30), fit);
        return JSTSP_E_UNSUPPORTED;
    }
    JSTSP_TRY(s.reserve(need, nm));
    layout(s, batch);
    if (s.err != hipSuccess) {
        (void)hipStreamSynchronize(s.st);           // (the uploads before it may still read the caller's arrays)
        set_error("%s: staging an input on the device failed: %s", nm, hipGetErrorString(s.err));
        return (int)s.err;
    }
    return 0;
}

}  // namespace
}  // namespace jstsp
