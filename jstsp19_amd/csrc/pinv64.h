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

// pinv.m's drop rule, the one place: sigma_k is kept iff sigma_k > max(size(A)) * eps(sigma_max), eps(x) = 2^(floor(log2 x) - 52).
// longer = max(rows, cols); smax may be the largest singular value of the operand times any power of two, as long as the
// values compared with the result carry the same factor.
__host__ __device__ inline double pinv64_drop_tol(int longer, double smax)
{
    return smax > 0.0 ? (double)longer * ldexp(1.0, ilogb(smax) - 52) : 0.0;
}

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
// The leading n_keep <= n = min(rows, cols) singular triplets of A[t] (jstsp_svd_f64 beyond the LDS limit, svd64.hip): the same
// prescale, rounds and per-matrix stop, then one workgroup per matrix sorts the column norms of W V = U Sigma (equal norms keep
// column order) and writes sv[k + n_keep t], U (rows x n_keep per matrix) and Vout (cols x n_keep per matrix), all on the device;
// U, Vout, rank and conv may each be nullptr.  The short-side factor (Vout when rows >= cols, else U) is the accumulated
// rotations; the long-side one is column / norm, zero for the columns the drop rule above drops.  rank[t]: the number kept;
// conv[t]: 1 when a sweep of matrix t met no significant pair (PvMeta::done), 0 when the cap ended its sweeps.  A non-finite
// entry: NaN, rank 0, conv 0 for that matrix.  Uses w.W, w.V, w.meta and w.any only.  Synchronises the stream once per sweep.
int pinv64_svd(hipStream_t st, const Pinv64Arrays &w, int rows, int cols, int count, const double2 *A, long long sA, int n_keep, double2 *U,
               double *sv, double2 *Vout, int32_t *rank, int32_t *conv);
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
