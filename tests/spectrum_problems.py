"""Shared problem builders of the spectrum tests (not a test module), numpy only: random operands, U diag(sigma) V^H with given
sigma, the float64 reference, the error measure, and a numpy restatement of the chunked-QR route of csrc/svdvals.hip."""
import numpy as np

CHUNK = 128


def rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def orth(rng, n, k):
    q, _ = np.linalg.qr(rand(rng, n, k))
    return q


def usv(rng, rows, cols, sigma):
    """U diag(sigma) V^H in float64 with random orthonormal U (rows x k) and V (cols x k)."""
    sigma = np.asarray(sigma, dtype=np.float64)
    return (orth(rng, rows, sigma.size) * sigma) @ orth(rng, cols, sigma.size).conj().T


def ref(Y):
    """float64 singular values per matrix on the operand values the device saw."""
    return np.linalg.svd(np.asarray(Y, dtype=np.complex128), compute_uv=False)


def err(sv, r):
    """max_k |sv_k - ref_k| / ref_1, the largest over the batch."""
    sv, r = np.atleast_2d(sv), np.atleast_2d(r)
    assert sv.shape == r.shape, (sv.shape, r.shape)
    return float(np.max(np.abs(sv - r) / r[:, :1]))


def ordered(sv):
    sv = np.atleast_2d(sv)
    return bool(np.all(sv >= 0) and np.all(np.diff(sv, axis=1) <= 0))


def graded(n, scale=1.0):
    return scale * np.logspace(0, -12, n)


REPEATED = np.repeat([2.0, 1.0, 1.0, 0.25, 0.25], 10)


def conditioning_cases(rng, rows, cols, count=2):
    """rank 6, sigma graded over 12 decades, repeated sigma: (name, (count, rows, cols) complex128)."""
    n = min(rows, cols)
    return [("rank6", np.stack([usv(rng, rows, cols, rng.uniform(0.5, 2.0, 6)) for _ in range(count)])),
            ("graded", np.stack([usv(rng, rows, cols, graded(n, 3.0)) for _ in range(count)])),
            ("repeated", np.stack([usv(rng, rows, cols, REPEATED[:n]) for _ in range(count)]))]


def chunked_qr_values(Y, chunk=CHUNK):
    """The route of tsqr_values_kernel in numpy: orient to m >= n, reduce [R; chunk] to R chunk after chunk by Householder QR
    (numpy's, mode 'r'), then the singular values of the n x n triangle."""
    Y = np.asarray(Y, dtype=np.complex128)
    W = Y if Y.shape[0] >= Y.shape[1] else Y.conj().T
    n = W.shape[1]
    R = np.zeros((n, n), complex)
    for i0 in range(0, W.shape[0], chunk):
        R = np.linalg.qr(np.vstack([R, W[i0:i0 + chunk]]), mode="r")
    return np.linalg.svd(R, compute_uv=False)


def cpu_cases(rng):
    """The six problems the restatement is checked on: (name, matrix)."""
    return [("random 64x4096", rand(rng, 64, 4096) * 0.3),
            ("rank6 64x1000", usv(rng, 64, 1000, rng.uniform(0.5, 2.0, 6))),
            ("graded 64x1000", usv(rng, 64, 1000, graded(64, 3.0))),
            ("repeated 64x1000", usv(rng, 64, 1000, REPEATED)),
            ("random 4097x33", rand(rng, 4097, 33)),
            ("graded 128x640", usv(rng, 128, 640, graded(128, 3.0)))]
