"""Case generators and the float64 reference of the device scoring entries (jstsp_nmse_spectral_f64 / jstsp_rate_f64).

The reference is montecarlo._score_f64's two formulas written out in numpy - plot_errorVSsnr.m:138-141 and
plot_rateVSframelength.m:81 - and nothing of the library: the code under test is not its own reference."""
import numpy as np

TINY = np.finfo(np.float64).tiny

# (rows, cols) per route of csrc/svdvals.hip: the smallest shapes at which each can go wrong - both orientations, one column or
# row, the LDS limit (64 x 64), one chunk plus one row (129), the chunk of 64 (n > 48) and of 128, many chunks (4097), one order
# above the LDS kernel's (65), a long side above one wave's rows (600)
LDS_SHAPES = [(32, 16), (5, 5), (1, 7), (7, 1), (64, 64)]
QR_SHAPES = [(64, 129), (129, 64), (64, 512), (33, 4097)]
GLOBAL_SHAPES = [(65, 65), (128, 65), (96, 600)]
MANY = {(32, 16), (64, 129), (65, 65)}             # the shape of each route that also runs at batch 1 and 300


def route(rows, cols):
    m, n = max(rows, cols), min(rows, cols)
    if n <= 64 and rows * cols <= 8192:
        return "lds"
    return "qr" if n <= 64 and m <= 65536 else "global"


def rand(rng, *shape):
    return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)


def pair(rng, batch, rows, cols, k):
    """Zbar and S = Zbar + 10^-k noise, complex128 (batch, rows, cols)."""
    Z = rand(rng, batch, rows, cols) * 0.3
    return Z + 10.0 ** -k * rand(rng, batch, rows, cols) * 0.3, Z


def close_pair(rng, batch, rows, cols, rel=1e-9):
    """S = Zbar (1 + rel eps) entry by entry: the NMSE is of the order rel^2."""
    Z = rand(rng, batch, rows, cols) * 0.3
    return Z * (1.0 + rel * rand(rng, batch, rows, cols)), Z


def ref_e(S, Z):
    """the uncapped (norm(S - Zbar, 2) / norm(Zbar, 2))^2 of one trial; NaN for a non-finite entry (numpy's SVD raises there)"""
    if not (np.all(np.isfinite(S)) and np.all(np.isfinite(Z))):
        return np.float64("nan")
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.float64(np.linalg.norm(S - Z, 2)) / np.float64(np.linalg.norm(Z, 2))) ** 2


def ref_nmse(S, Z):
    S, Z = np.asarray(S, np.complex128), np.asarray(Z, np.complex128)
    out = np.empty(S.shape[0])
    for t in range(S.shape[0]):
        e = ref_e(S[t], Z[t])
        out[t] = min(1.0, e) if e == e else e
    return out


def ref_rate(S, Z, noise_var):
    S, Z = np.asarray(S, np.complex128), np.asarray(Z, np.complex128)
    nr = Z.shape[1]
    out = np.empty(S.shape[0])
    for t in range(S.shape[0]):
        e = ref_e(S[t], Z[t])
        out[t] = np.log2(np.real(np.linalg.det(np.eye(nr) + Z[t] @ Z[t].conj().T / nr / (noise_var + e))))
    return out


def rate_from_sigma(sigma, nr, noise_var, e):
    """sum_k log2(1 + sigma_k^2 / (nr (noise_var + e))): the determinant above in closed form"""
    return float(np.sum(np.log2(1.0 + np.asarray(sigma, np.float64) ** 2 / (nr * (noise_var + e)))))


def rel(x, ref):
    """max over trials of |x - ref| / max(|ref|, tiny)"""
    x, ref = np.asarray(x, np.float64), np.asarray(ref, np.float64)
    return float(np.max(np.abs(x - ref) / np.maximum(np.abs(ref), TINY)))
