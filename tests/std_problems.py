"""Problems for the least-squares paths of proposed_algorithm 'std', jstsp_ls_c32 and jstsp_pinv_c32 (tests/test_gpu_std_parity.py).

* ``pinv_fits`` / ``route``: which device code a factor takes - the float64 in-LDS pinv kernel (csrc/pinv.hip), or the fp32 Gram
  inverse (csrc/hinv.hip) by eigen-decomposition (order <= 128) or Newton-Schulz (order > 128).
* ``factor``: ``U diag(s) V^H`` with Haar unitaries and geometrically spaced singular values, for a prescribed condition number.
"""
import numpy as np

LDS_LIMIT = 156 * 1024          # pinv.hip: pinv_fits
EIG_MAX_ORDER = 128             # hinv.hip: hermitian_inverse
EPS32 = 2.0 ** -23              # the cut of the eigen route is n * EPS32 * lambda_max (hinv.hip: scale_cols_inv_kernel)
GRAM_REFUSE = 1e-6              # runtime.hip: diag_check_host refuses lambda_min/lambda_max below this


def pinv_lds(rows, cols):
    """Bytes of LDS the pinv kernel needs: W (ne x m) and V (ne x ne) in complex float64, sigma^2 and 8 reduction slots."""
    m, n = max(rows, cols), min(rows, cols)
    ne = (n + 1) & ~1
    return (ne * m + ne * ne) * 16 + (ne + 8) * 8


def pinv_fits(rows, cols):
    return rows > 0 and cols > 0 and pinv_lds(rows, cols) <= LDS_LIMIT


def largest_fitting(n_small):
    """The largest m such that an m x n_small (or n_small x m) matrix still fits the pinv kernel."""
    m = n_small
    while pinv_fits(m + 1, n_small):
        m += 1
    return m


def gram_route(order):
    return "eig" if order <= EIG_MAX_ORDER else "ns"


def route(N, M, Gr, G2):
    """(route of A, route of B) for the factors A (N x Gr) and B (G2 x M)."""
    ra = "pinv" if pinv_fits(N, Gr) else gram_route(Gr)
    rb = "pinv" if pinv_fits(G2, M) else gram_route(G2)
    return ra, rb


def refuse_threshold(order):
    """lambda_min/lambda_max of a factor Gram below which the eigen route drops a component or the call is refused."""
    return max(GRAM_REFUSE, order * EPS32)


def haar(rng, n, k):
    """n x k with orthonormal columns, Haar distributed (QR of a complex Gaussian with the phases of R's diagonal removed)."""
    Z = (rng.standard_normal((n, k)) + 1j * rng.standard_normal((n, k))) / np.sqrt(2)
    Q, R = np.linalg.qr(Z)
    d = np.diagonal(R)
    return Q * (d / np.abs(d))


def factor(rng, rows, cols, cond, scale=1.0):
    """rows x cols complex128 matrix of rank min(rows, cols) with singular values geomspace(scale, scale / cond)."""
    k = min(rows, cols)
    s = scale * np.geomspace(1.0, 1.0 / cond, k)
    return (haar(rng, rows, k) * s) @ haar(rng, cols, k).conj().T


def factor_two_level(rng, rows, cols, cond, flat=False):
    """rows x cols (rows <= cols) with half of its singular values 1 and half 1 / cond, in random order; left singular vectors
    Haar or (flat) the unitary DFT, which makes B B^H circulant.  Either way the Gram is about lambda_max times a projector onto
    half the space, whose columns spread over every coordinate: ||B B^H||_1 ~ sqrt(rows) lambda_max / 2, the slowest start of
    the Newton-Schulz inverse (X0 = I / ||G||_1), against ~ 2 lambda_max for a geometric spectrum."""
    assert rows <= cols
    s = np.where(rng.permutation(rows) < rows // 2, 1.0, 1.0 / cond)
    U = np.fft.fft(np.eye(rows)) / np.sqrt(rows) if flat else haar(rng, rows, rows)
    return (U * s) @ haar(rng, cols, rows).conj().T


def cond(X):
    s = np.linalg.svd(np.asarray(X, dtype=np.complex128), compute_uv=False)
    return float(s[0] / s[-1])
