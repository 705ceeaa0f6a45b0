// The float64 pseudo-inverse of pinv64.hip for the entry points that invert a dictionary factor themselves (internal):
// jstsp_pinv_f64, jstsp_ls_f64 (pinv64.hip) and jstsp_proposed_std_f64 (proposed64.hip) run ONE implementation.
#pragma once
#include "ws64.h"
#include "zgemm64.h"

#include <algorithm>

namespace jstsp {

constexpr int PV_MAX_ORDER = 512;        // min(rows, cols): the float64 family's largest order (svt64.h: P64_MAX_ORDER)
constexpr int PV_MAX_LONG = 8192;        // max(rows, cols)

struct PvMeta {
    double sc;          // the power of two the operand was multiplied by
    double fro2;        // squared Frobenius norm of the scaled operand
    int bad;            // a non-finite entry: the matrix is not decomposed, its outputs are NaN
    int done;           // a whole sweep met no significant pair
    int rot;            // the running sweep met one
    int pad;
};

// the arrays of pinv64_run for `count` matrices (rows x cols): Pinv64::layout below hands them out
struct Pinv64Arrays {
    double2 *W, *V, *Vs, *ws;
    PvMeta *meta;
    int *any;
};

bool pinv64_shape_ok(int rows, int cols);
size_t pinv64_gemm_ws(int rows, int cols, int count);

// P[t] (cols x rows, contiguous) = pinv(A[t]) (rows x cols, sA elements apart), t < count; rcond / rank: nullptr or device [count]
// (rank: the number of singular values pinv.m's drop rule keeps, 0 for a matrix with a NaN or Inf).  A matrix's result does not
// depend on the matrices around it.  Synchronises the stream once per sweep.
int pinv64_run(hipStream_t st, const Pinv64Arrays &w, int rows, int cols, int count, const double2 *A, long long sA, double2 *P, double *rcond,
               int32_t *rank);
// sv[k + n_keep t] (device) = the k-th largest singular value of A[t], k < n_keep: the same one-sided Jacobi without the inverse
// (jstsp_spectrum_*, svdvals.hip).  Uses w.W, w.V, w.meta and w.any only.  Synchronises the stream once per sweep.
int pinv64_values(hipStream_t st, const Pinv64Arrays &w, int rows, int cols, int count, const double2 *A, long long sA, int n_keep, double *sv);
// out[0] = the smallest of v[0 .. cnt) (device arrays), NaN when one of them is NaN
int pinv64_min(hipStream_t st, int cnt, const double *v, double *out);

namespace {

struct Pinv64 : Pinv64Arrays {
    void layout(Slab &s, int rows, int cols, int count)
    {
        const size_t m = std::max(rows, cols), n = std::min(rows, cols);
        W = s.get<double2>(m * n * count); V = s.get<double2>(n * n * count); Vs = s.get<double2>(n * n * count);
        meta = s.get<PvMeta>(count);
        any = s.get<int>(1);
        ws = s.get<double2>(pinv64_gemm_ws(rows, cols, count));
    }
};

}  // namespace
}  // namespace jstsp
