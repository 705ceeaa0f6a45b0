"""Problems and a numpy restatement for the float64 SVD with vectors on the QR route (jstsp_svd_tall_f64 / jstsp_lowrank_tall_f64,
csrc/svd64.hip, csrc/tsqr64.h) - not a test module, numpy only; imports neither the device code nor the oracle.

``tsqr_svd_ref`` restates the route in complex128: orientation to m >= n columns, the power-of-two prescale from the largest
component, the chunked Householder reduction [R; chunk] -> R with the chunk rule ``tq_chunk`` and the reflector of tq_reduce
(u_0 = (alpha / |alpha|) (|alpha| + |x|), 1 / (|x| (|x| + |alpha|)), a zero chunk part skipped), the one-sided Jacobi with vectors
on the triangle (``jacobi_svd_ref`` of tests/svd64_problems.py, imported), the drop rule of pinv.m with the LONG side of the
operand, the back-application of the kept reflectors, last chunk first, to [U_R; 0], and the first-order correction
L (I + E^H E / 2) with E what the back-application leaves in the top block.  It differs from the device in summation order only.
``av_long_side`` is the long-side factor the route replaces, A V Sigma^-1 from the same R; ``tsqr_svd_ref(A, correct=False)`` is
the route without the correction.

Why the correction: [0; W] = Q [R; 0] holds with a backward error of eps |W|, so the top block of Q [u_k; 0] is not zero but
(error) v_k / sigma_k, of size eps sigma_1 / sigma_k.  Q [U_R; 0] as a whole is orthonormal to rounding level; its rows below
the top block alone satisfy L^H L = I - E^H E, a second-order loss: nothing at sigma_k ~ sigma_1, 8e-10 on the graded class
(sigma over 12 decades), against 4e-4 for A V Sigma^-1, whose loss is first order.  L (I + E^H E / 2) is orthonormal to
O(|E|^4).

The bounds of tests/test_gpu_svd64_tall.py for the reconstruction and the two orthogonality measures are MARGIN x the worst value
this restatement reaches over SHAPES and one 64 x 65536 matrix, recorded in tests/golden/svd64_tall_restatement_worst.json by
tests/golden/make_svd64_tall_fixture.py."""
import functools
import json
import os

import numpy as np

import spectrum_problems as P
import svd64_problems as S

MARGIN = S.MARGIN
QR_TOL = 1.1e-13                                          # tests/test_gpu_spectrum.py, for this reduction
BATCH = S.BATCH
N_MAX, M_MAX = 64, 65536
# A rank is compared with the drop rule on numpy's values only where no reference value lies within this factor of the threshold.
# tests/svd64_problems.py uses 4; the graded class at 9000 x 33 has sigma_33 = 3e-12 under a threshold of 4e-12 (a factor 1.33),
# and that distance, 1e-12 = 3.3e-13 sigma_1, is still three times the accuracy the values are held to (QR_TOL).
CLEAR = 1.25

# the smallest shapes at which each branch of the route can go wrong: one ragged chunk; exactly one chunk of 128, one plus 2 rows;
# chunk 64 with two full chunks plus one row; n = 64; the shapes jstsp_svd_f64 refuses; several chunks with a ragged last one
SHAPES = [(5, 3), (3, 5), (1, 7), (7, 1), (128, 48), (130, 48), (129, 49), (64, 64), (200, 64), (64, 200), (8193, 2), (2, 8193), (9000, 33)]
BIG_SHAPE = (64, 65536)

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svd64_tall_restatement_worst.json")


def tq_chunk(n):
    """Rows per chunk (csrc/tsqr64.h)."""
    return 128 if n <= 48 else 64


def workspace_bytes(rows, cols, n_keep):
    """What one matrix of jstsp_svd_tall_f64 takes beside its operand and outputs: the reflector tails, (u_0, 1/..) per chunk and
    column, the top block, its correction and the flag."""
    m, n = max(rows, cols), min(rows, cols)
    return m * n * 16 + 3 * n * (-(-m // tq_chunk(n))) * 8 + (n * n_keep + n_keep * n_keep) * 16 + 4


def _orient(A):
    A = np.asarray(A, dtype=np.complex128)
    if A.ndim == 2:
        A = A[None]
    tall = A.shape[1] >= A.shape[2]
    W = A.copy() if tall else np.conj(np.swapaxes(A, 1, 2)).copy()
    amax = np.max(np.maximum(np.abs(W.real), np.abs(W.imag)), axis=(1, 2))
    ex = np.clip(np.where(amax > 0, np.frexp(np.where(amax > 0, amax, 1.0))[1], 0), -1000, 1000)
    W *= np.ldexp(1.0, -ex)[:, None, None]                                    # exact
    return W, ex, tall


def forward(W):
    """The chunked reduction of a scaled, oriented batch W (B, m, n): (R, Y, u0, inv) - the triangle, the reflector tails in the
    operand's place, u_0 (B, chunks, n) and 1 / (|x| (|x| + |alpha|)) (B, chunks, n), 0 where the reflector was skipped."""
    B, m, n = W.shape
    C = tq_chunk(n)
    nch = -(-m // C)
    R = np.zeros((B, n, n), complex)
    Y = W.copy()
    u0 = np.zeros((B, nch, n), complex)
    inv = np.zeros((B, nch, n))
    for c in range(nch):
        Ck = Y[:, c * C:min(m, (c + 1) * C), :]
        for j in range(n):
            y = Ck[:, :, j]
            s2 = np.sum(y.real ** 2 + y.imag ** 2, axis=1)
            act = s2 > 0
            if not act.any():
                continue
            alpha = R[:, j, j].copy()
            aa = np.hypot(alpha.real, alpha.imag)
            nx = np.sqrt(aa * aa + s2)
            p = np.where(aa > 0, alpha / np.where(aa > 0, aa, 1.0), 1.0)
            u = p * (aa + nx)
            iv = np.where(act, 1.0 / np.where(act, nx * (nx + aa), 1.0), 0.0)
            u0[:, c, j], inv[:, c, j] = np.where(act, u, 0.0), iv
            if j + 1 < n:
                d = np.conj(u)[:, None] * R[:, j, j + 1:] + np.einsum("bi,bik->bk", np.conj(y), Ck[:, :, j + 1:])
                f = d * iv[:, None]
                R[:, j, j + 1:] -= u[:, None] * f
                Ck[:, :, j + 1:] -= y[:, :, None] * f[:, None, :]
            R[:, j, j] = np.where(act, -p * nx, alpha)
    return R, Y, u0, inv


def backward(T, Y, u0, inv):
    """Q [T; 0]: (the (B, m, k) rows below the top block, what is left in the top block) - the chunks last to first, column
    j = n - 1 .. 0 within a chunk."""
    B, m, n = Y.shape
    C = tq_chunk(n)
    T = T.copy()
    L = np.zeros((B, m, T.shape[2]), complex)
    for c in reversed(range(u0.shape[1])):
        Ck = Y[:, c * C:min(m, (c + 1) * C), :]
        Wk = np.zeros((B, Ck.shape[1], T.shape[2]), complex)
        for j in reversed(range(n)):
            iv = inv[:, c, j]
            if not iv.any():
                continue
            y, u = Ck[:, :, j], u0[:, c, j]
            d = np.conj(u)[:, None] * T[:, j, :] + np.einsum("bi,biq->bq", np.conj(y), Wk)
            f = d * iv[:, None]
            T[:, j, :] -= u[:, None] * f
            Wk -= y[:, :, None] * f[:, None, :]
        L[:, c * C:c * C + Ck.shape[1], :] = Wk
    return L, T


def _middle(R, m):
    """The Jacobi on the triangle with the drop rule on the long side m of the operand: (U_R with the dropped columns zero, the
    values in the triangle's scale, V, rank, conv)."""
    n = R.shape[1]
    UR, sR, VR, _, conv, _ = S.jacobi_svd_ref(R, "lds")
    kept = sR > S.drop_threshold(m, n, sR[:, 0])[:, None]
    return np.where(kept[:, None, :], UR, 0.0), sR, VR, kept.sum(axis=1).astype(np.int32), conv


def tsqr_svd_ref(A, correct=True):
    """(U, sv, V, rank, conv) of a batch A (count, rows, cols) by the restated route; U (count, rows, n), sv (count, n),
    V (count, cols, n).  correct=False: the long-side factor as the back-application leaves it."""
    W, ex, tall = _orient(A)
    R, Y, u0, inv = forward(W)
    UR, sR, VR, rank, conv = _middle(R, W.shape[1])
    long, E = backward(UR, Y, u0, inv)
    if correct:
        long = long + long @ (0.5 * (np.conj(np.swapaxes(E, 1, 2)) @ E))
    sv = sR * np.ldexp(1.0, ex)[:, None]
    U, V = (long, VR) if tall else (VR, long)
    return U, sv, V, rank, conv


def av_long_side(A):
    """What the route replaces: the long-side factor as (oriented A) V Sigma^-1 from the same triangle; (count, m, n), dropped
    columns zero."""
    W, ex, tall = _orient(A)
    R = forward(W)[0]
    _, sR, VR, rank, _ = _middle(R, W.shape[1])
    keep = np.arange(sR.shape[1])[None, :] < rank[:, None]
    return np.where(keep[:, None, :], (W @ VR) / np.where(keep, sR, 1.0)[:, None, :], 0.0)


def classes(rows, cols, count=BATCH):
    return S.classes(rows, cols, count)


def drops_a_value(rows, cols, ref):
    """True when pinv.m's drop rule drops a reference value that is not zero to the accuracy of the values (the 33rd of the graded
    class at 9000 x 33: 3e-12 under a threshold of 4e-12): the long-side factor has a zero column there and the reconstruction
    lacks sigma_k / sigma_1, whatever the arithmetic."""
    ref = np.atleast_2d(ref)
    dropped = ref <= S.drop_threshold(rows, cols, ref[:, 0])[:, None]
    return bool(np.any(dropped & (ref > QR_TOL * ref[:, :1])))


def record(rows, cols, count=BATCH):
    """Per class of a shape: (name, worst measures of the restatement, worst of numpy's SVD, all converged, drops_a_value)."""
    out = []
    for name, A in classes(rows, cols, count):
        ref = P.ref(A)
        U, sv, V, _, conv = tsqr_svd_ref(A)
        Un, sn, Vn = S.numpy_svd(A)
        mine = S.worst([S.measures(A[t], U[t], sv[t], V[t], ref[t]) for t in range(A.shape[0])])
        nump = S.worst([S.measures(A[t], Un[t], sn[t], Vn[t], ref[t]) for t in range(A.shape[0])])
        out.append((name, mine, nump, bool(conv.all()), drops_a_value(rows, cols, ref)))
    return out


@functools.lru_cache(maxsize=None)
def small_records():
    return [(r, c) + rec for r, c in SHAPES for rec in record(r, c)]


def recomputed_worst():
    """The restatement's worst measures over SHAPES (the 64 x 65536 matrix of the fixture takes a minute and is not recomputed),
    and the worst e_rec over the cases in which no value is dropped."""
    w = S.worst([r[3] for r in small_records()])
    w["e_rec_nothing_dropped"] = max(r[3]["e_rec"] for r in small_records() if not r[6])
    return w


def big_problem():
    """The one 64 x 65536 matrix of the GPU test and of the fixture: (1, 64, 65536), random."""
    return P.rand(np.random.default_rng(65536064), 1, *BIG_SHAPE) * 0.3


@functools.lru_cache(maxsize=None)
def bounds():
    """The asserted bounds: e_sv = QR_TOL; the others MARGIN x the recorded worst of the restatement.  e_rec_nothing_dropped: the
    same for the reconstruction of the problems in which the drop rule drops no value (``drops_a_value``) - the recorded worst
    e_rec is the dropped sigma_33 / sigma_1 = 1e-12 of one class and would hide a loss of two digits everywhere else."""
    with open(FIXTURE) as f:
        w = json.load(f)["restatement"]
    return {"e_sv": QR_TOL, "e_rec": MARGIN * w["e_rec"], "e_long": MARGIN * w["e_long"], "e_short": MARGIN * w["e_short"],
            "e_rec_nothing_dropped": MARGIN * w["e_rec_nothing_dropped"]}


@functools.lru_cache(maxsize=None)
def recorded_small():
    """The restatement's recorded worst measures over SHAPES alone, what ``recomputed_worst`` recomputes."""
    with open(FIXTURE) as f:
        return json.load(f)["small_shapes"]["restatement"]
