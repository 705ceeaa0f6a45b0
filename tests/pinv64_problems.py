"""Problems with a KNOWN pseudo-inverse for the float64 pinv / least-squares entries (jstsp_pinv_f64, jstsp_ls_f64).

``factor(rng, rows, cols, cond, rank)`` is tests/std_problems.py's construction (Haar singular vectors, geometric singular
values 1 .. 1/cond) extended by a rank r <= min(rows, cols): A = U diag(s) V^H with r columns in U and V.  The exact
pseudo-inverse of the UNROUNDED factor is V diag(1/s) U^H, formed in float64 from the same pieces - it carries only the
rounding of its own product (a few 2^-53 relative to ||P||), not an SVD's error, so it can judge numpy and the device alike.

Shapes (include/jstsp.h: min <= 512, max <= 8192): 64 x 64, 140 x 16, 16 x 140 (small, both orientations), 7 x 13 (ragged),
256 x 1024, 1024 x 256, 512 x 512, 512 x 4096, 4096 x 512 (the drivers' B_hbf and its transpose), each at cond 1e2, 1e5, 1e8,
1e10; rank-deficient at cond 1e2, 1e5, 1e8 of the kept values: 64 x 64 rank 40, 512 x 640 and 640 x 512 rank 300.

One change of case: the drop threshold max(rows, cols) * 2^-52 grows with the long side, and at cond 1e10 the smallest
singular value of a matrix 1024 or 4096 long is only 440 or 110 times it (tests/test_pinv64_problems.py asks for 1e3, so that
no rounding decides what is dropped).  The four shapes with a side >= 1024 therefore take 1e9 as their largest condition
number (1100 times the threshold at 4096) instead of 1e10; every other shape keeps 1e10.
"""
import functools

import numpy as np

from std_problems import haar

EPS53 = 2.0 ** -53
CONDS = (1e2, 1e5, 1e8, 1e10)
DEFICIENT_CONDS = (1e2, 1e5, 1e8)          # at 1e10 the smallest kept value comes within 1e3 of the drop threshold
FULL_SHAPES = ((64, 64), (140, 16), (16, 140), (7, 13), (256, 1024), (1024, 256), (512, 512), (512, 4096), (4096, 512))
DEFICIENT_SHAPES = ((64, 64, 40), (512, 640, 300), (640, 512, 300))

# (rows, cols, cond, rank or None): every case of the accuracy test
CASES = [(r, c, (1e9 if k == 1e10 and max(r, c) >= 1024 else k), None) for (r, c) in FULL_SHAPES for k in CONDS] + [(r, c, k, q) for (r, c, q) in DEFICIENT_SHAPES for k in DEFICIENT_CONDS]


def case_id(case):
    r, c, k, q = case
    return "%dx%d-cond1e%d%s" % (r, c, int(round(np.log10(k))), "" if q is None else "-rank%d" % q)


def factor(rng, rows, cols, cond, rank=None):
    """(A, P_exact, s): rows x cols complex128 of rank `rank` (default min(rows, cols)) with singular values
    s = geomspace(1, 1 / cond, rank), and V diag(1 / s) U^H."""
    k = min(rows, cols) if rank is None else int(rank)
    assert 1 <= k <= min(rows, cols)
    s = np.geomspace(1.0, 1.0 / cond, k)
    U, V = haar(rng, rows, k), haar(rng, cols, k)
    return (U * s) @ V.conj().T, (V / s) @ U.conj().T, s


@functools.lru_cache(maxsize=None)
def build(case):
    """The case's (A, P_exact, s); the generator is seeded by the case itself."""
    r, c, k, q = case
    rng = np.random.default_rng([20190913, r, c, int(round(np.log10(k))), 0 if q is None else q])
    return factor(rng, r, c, k, q)


def drop_threshold(rows, cols, sigma_max):
    """pinv.m: max(size(A)) * eps(norm(A)), eps(x) = 2^(floor(log2 x) - 52)."""
    return max(rows, cols) * 2.0 ** (np.floor(np.log2(sigma_max)) - 52) if sigma_max > 0 else 0.0


def numpy_pinv(A):
    """numpy's SVD-based pinv with pinv.m's relative cut-off max(size) * 2^-52 (the device's reference)."""
    return np.linalg.pinv(A, rcond=max(A.shape) * 2.0 ** -52)


def rel2(X, ref):
    """||X - ref||_2 / ||ref||_2 (spectral norms)."""
    return float(np.linalg.norm(X - ref, 2) / np.linalg.norm(ref, 2))


@functools.lru_cache(maxsize=None)
def numpy_error(case):
    """d_ref of the case: numpy's own distance from the exact pseudo-inverse."""
    A, P, _ = build(case)
    return rel2(numpy_pinv(A), P)


def device_bound(case):
    """8 * max(d_ref, cond * 2^-53): what the device result is held to (relative spectral-norm distance from P_exact)."""
    return 8.0 * max(numpy_error(case), case[2] * EPS53)


def gram_pinv(A):
    """The float64 Gram route the feature must NOT take: solve(A'A, A') for a tall matrix, its counterpart for a wide one."""
    Ah = A.conj().T
    if A.shape[0] >= A.shape[1]:
        return np.linalg.solve(Ah @ A, Ah)
    return np.linalg.solve(A @ Ah, A).conj().T


def repeated_column(rows=64, cols=32, src=5, dst=17):
    """rows x cols complex Gaussian matrix whose column `dst` is a copy of column `src`: rank cols - 1 exactly."""
    rng = np.random.default_rng([20190913, rows, cols, src, dst])
    A = (rng.standard_normal((rows, cols)) + 1j * rng.standard_normal((rows, cols))) / np.sqrt(2)
    A[:, dst] = A[:, src]
    return A


def penrose(A, P):
    """The four Penrose residuals, each relative to the size of its own terms (spectral norms)."""
    n = lambda X: float(np.linalg.norm(X, 2))
    AP, PA = A @ P, P @ A
    return (n(AP @ A - A) / n(A), n(PA @ P - P) / n(P), n(AP - AP.conj().T) / n(AP), n(PA - PA.conj().T) / n(PA))


def batch_of_five(rows=140, cols=16):
    """Five different matrices of one shape (conds 1e2 .. 1e8 and a rank-deficient one): (A (5, rows, cols), P, cond, rank)."""
    spec = ((1e2, None), (1e5, None), (1e8, None), (1e3, cols - 5), (1e6, None))
    rng = np.random.default_rng([20190913, rows, cols, 5])
    out = [factor(rng, rows, cols, k, q) for k, q in spec]
    return (np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), [k for k, _ in spec],
            [min(rows, cols) if q is None else q for _, q in spec])
