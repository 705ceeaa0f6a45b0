// Float64 pieces shared by zgemm64.hip, proposed64.hip and vamp64.hip (internal).
#pragma once
#include "common.h"

namespace jstsp {

// one operand of a batched product: column-major, leading dimension ld, st elements between trials (0 = shared by the batch)
struct Mat64 {
    const double2 *p; long long st; int ld;
};

// C[t] (m x n, column-major, leading dimension ldc, sC elements between trials) = op(A[t]) op(B[t]) on v_mfma_f64_16x16x4_f64;
// opX: 'N' as stored, 'C' conjugate transpose.  Any m, n, k >= 1.  A product with a small result and a long inner dimension is
// cut along k (zgemm64_splits, a function of the shape alone - never of the batch) into partial products that a second kernel
// adds in a fixed order: `ws` must then hold zgemm64_ws_elems() elements.  No atomics: a repeated call returns the same bits.
int zgemm64(hipStream_t st, char opA, char opB, int m, int n, int k, int batch, Mat64 A, Mat64 B, double2 *C, long long sC, int ldc,
            double2 *ws);
int zgemm64_splits(int m, int n, int k);
size_t zgemm64_ws_elems(int m, int n, int k, int batch);

// vamp64.hip's global-memory two-sided Jacobi (any order; reads one norm per sweep on the host, so it synchronises the stream):
// U (n x n each) and lam (n each) of nmat Hermitian matrices G (column-major, leading dimension n, sG elements apart).
// The sweeps go on while ANY matrix of the call is above the stop criterion; freeze = true leaves a matrix alone from the sweep
// on at whose start it meets the criterion itself, so that its bits do not depend on the matrices around it.
int eig64_global(hipStream_t st, int n, int nmat, const double2 *G, long long sG, double2 *U, double *lam, bool freeze = false);

}  // namespace jstsp
