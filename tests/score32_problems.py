"""Shapes, route labels and case generators for the fp32 scoring entries (jstsp_nmse_spectral_c32 / jstsp_rate_c32, csrc/api_misc.hip).

The reference is score64_problems' (ref_nmse, ref_rate, rate_from_sigma, rel, pair), unchanged, always evaluated on the operand
values the device sees: S and Zbar rounded to complex64, then widened.  Nothing of the library is restated here except the two
dispatch functions below, which serve only to label the cases."""
import functools

import numpy as np

import score64_problems as P64
from score64_problems import pair, rand, rate_from_sigma, ref_nmse, ref_rate, rel  # noqa: F401

NOISE_VAR = 0.1


def pick_nsplit(n, kc, batch):
    """jstsp19_amd/csrc/runtime.hip:164 (pick_nsplit): split-k partial Grams of an n x n Gram contracted over kc"""
    tiles = ((n + 63) // 64) ** 2
    want = (1024 + batch * tiles - 1) // (batch * tiles)
    kmax = max(1, kc // 256)
    return min(max(1, min(want, kmax)), 32)


def eig_needs_global_v(n):
    """jstsp19_amd/csrc/eig.hip:244 (eig_needs_global_v): the eigenvectors do not fit in LDS beside G"""
    ne = (n + 1) & ~1
    mat = ne * (ne + 1) * 8
    extra = (4 * (ne // 2) + 8 + ne) * 4
    return 2 * mat + extra > 160 * 1024


def route(R, C, batch):
    """(orientation, nsplit, lambda_max route, rate eigen route) of an R x C x batch call"""
    n, kc = min(R, C), max(R, C)
    lmax = "h32" if n <= 32 else "h64" if n <= 64 else "h128" if n <= 128 else "block"      # eig2.hip: launch_lmax
    rate = "n/a" if n > 128 else ("hbm" if eig_needs_global_v(n) else "lds")                 # eig.hip: launch_eig
    return ("ZZh" if R <= C else "ZhZ"), pick_nsplit(n, kc, batch), lmax, rate


# the smallest shapes at which each route can go wrong
NMSE_SHAPES = [(32, 16), (16, 32),          # both orientations
               (1, 7), (7, 1),              # order 1
               (32, 40),                    # last order of NE = 32
               (33, 40),                    # odd order, NE = 64 with padding
               (64, 64),                    # full LDS tile, nsplit 1
               (64, 512), (512, 64),        # nsplit 2 in both orientations
               (33, 4097),                  # nsplit 16 with a k-tail
               (65, 65),                    # first order of NE = 128
               (128, 130),                  # last order of NE = 128
               (129, 140),                  # first order of the block route: 3 blocks of 64, 63 padded
               (200, 136),                  # block route, tall input
               (260, 257)]                  # 5 blocks
RATE_SHAPES = [(32, 16), (12, 40), (40, 12),        # Nr = R on either side of n
               (64, 64),                            # full LDS tile
               (64, 512),                           # the eigen-kernel sums 2 partials
               (65, 70),                            # first order above 64
               (100, 100), (101, 101),              # the LDS / HBM eigenvector boundary
               (128, 128),                          # last supported order
               (128, 600),                          # HBM eigenvectors and nsplit 2
               (130, 64)]                           # R > 128 is legal: the limit is on min(R, C)
SHAPES = NMSE_SHAPES + [s for s in RATE_SHAPES if s not in NMSE_SHAPES]
# one shape per lambda_max route (one per route in each table): batches 1, 3 and 300; 3 elsewhere
MANY = {(32, 16): "h32", (33, 40): "h64", (64, 64): "h64", (65, 65): "h128", (65, 70): "h128", (129, 140): "block"}
ONE_PER_ROUTE = [(32, 16), (33, 40), (65, 65), (129, 140)]
RATE_ROUTES = [(32, 16), (64, 64), (65, 70), (101, 101)]       # h32 / h64 / h128 with LDS eigenvectors, h128 with HBM eigenvectors
STRIDING = ((64, 512), 40)                  # 1.31 M entries: the element-wise kernels stride
GENERATORS = (0, 2, 4, "lowrank")           # pair(k): S = Zbar + 10^-k noise (k = 0: capped trials); a rank-4 Zbar
SCALES = (-40, -16, 16, 40)                 # S, Zbar scaled by 2^s: the NMSE is unchanged
RATE_SCALES = (-8, 20, 40)                  # (smaller scales make the reference rate underflow to 0)


def batches(shape):
    return (1, 3, 300) if shape in MANY else (3,)


def has_rate(R, C):
    return min(R, C) <= 128                 # (api_misc.hip: jstsp_rate_c32 is JSTSP_E_UNSUPPORTED above)


def generators(batch):
    """every generator at batches 1 and 3; a capped and an uncapped one at batch 300 (the reference costs 4 SVDs per trial)"""
    return GENERATORS if batch <= 3 else (0, 2)


def lowrank_pair(rng, batch, R, C):
    """Zbar of rank 4 plus 1e-3 noise - the rate then sums over near-zero eigenvalues, which come out negative in fp32 and are
    clamped - and S = Zbar + 1e-2 noise.  complex128 (batch, R, C), at the magnitude of pair()."""
    Z = 0.3 * (rand(rng, batch, R, 4) @ rand(rng, batch, 4, C)) / 2.0 + 1e-3 * 0.3 * rand(rng, batch, R, C)
    return Z + 1e-2 * 0.3 * rand(rng, batch, R, C), Z


def _round(X):
    return np.asarray(X, np.complex128).astype(np.complex64).astype(np.complex128)


@functools.lru_cache(maxsize=None)
def _generate(R, C, batch, gen):
    """k = 0 draws S - Zbar as large as Zbar, so a trial is capped with probability 1/2: the first draw (salt 0, 1, ...) whose
    REFERENCE has a capped trial - and, in a batch, an uncapped one beside it - is the case."""
    for salt in range(64):
        rng = np.random.default_rng([R, C, batch, 99 if gen == "lowrank" else int(gen), salt])
        S, Z = lowrank_pair(rng, batch, R, C) if gen == "lowrank" else pair(rng, batch, R, C, gen)
        S, Z = _round(S), _round(Z)
        e = ref_nmse(S, Z)
        if gen != 0 or (np.any(e == 1.0) and (batch == 1 or np.any(e < 1.0))):
            break
    for a in (S, Z, e):
        a.setflags(write=False)
    return S, Z, e


def operands(R, C, batch, gen):
    """S, Zbar as the device sees them: rounded to complex64, widened to complex128 (read-only)"""
    return _generate(R, C, batch, gen)[:2]


@functools.lru_cache(maxsize=None)
def case(R, C, batch, gen, want_rate=False):
    """(S, Zbar, ref_nmse, ref_rate or None) of one case, computed once and shared: the arrays are read-only"""
    S, Z, e = _generate(R, C, batch, gen)
    r = ref_rate(S, Z, NOISE_VAR) if want_rate else None
    if r is not None:
        r.setflags(write=False)
    return S, Z, e, r


def cases():
    """(R, C, batch, gen) of every case; the NMSE is checked on all of them, the rate wherever has_rate(R, C)"""
    out = [(R, C, b, g) for (R, C) in SHAPES for b in batches((R, C)) for g in generators(b)]
    return out + [STRIDING[0] + (STRIDING[1], 2)]


def ref_rate_sigma(S, Z, noise_var):
    """ref_rate in its closed form, rate_from_sigma on the singular values of Zbar with the uncapped ref_e: the determinant of
    ref_rate overflows float64 once the operands are scaled by 2^20 (orders above 22) or 2^40, the sum of logarithms does not.
    For R > C the determinant is also ill-conditioned there (R - C unit eigenvalues beside C of the order 2^(2 s): 1e-6 relative
    at 2^20 on 32 x 16).  The two agree to 1e-12 wherever the determinant is finite and R <= C (tests/test_score32_problems.py)."""
    return np.array([rate_from_sigma(np.linalg.svd(Z[t], compute_uv=False), Z.shape[1], noise_var, P64.ref_e(S[t], Z[t]))
                     for t in range(Z.shape[0])])


def scaled(X, s):
    """X 2^s, exact in complex64 for every case of this module (no entry leaves the normal range)"""
    Y = np.ldexp(X.real, s) + 1j * np.ldexp(X.imag, s)
    assert np.array_equal(_round(Y), Y)
    return Y
