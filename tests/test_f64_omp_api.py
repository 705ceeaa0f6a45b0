"""The public surface of the float64 OMP and sparse_admm without a GPU: the three Python names exist and are exported, the
library exports the three symbols and the ctypes table binds them, a call fails loudly without a GPU (no fallback), and a shape
error is a ValueError before any device work."""
import numpy as np
import pytest

import jstsp19_amd as J

NAMES = ("OMP_f64", "omp_kron_f64", "sparse_admm_f64")


def test_the_three_names_and_symbols_are_exported():
    from jstsp19_amd import _lib, solvers
    for n in NAMES:
        assert callable(getattr(J, n)) and n in solvers.__all__
    lib = J.load()
    for n in ("jstsp_omp_f64", "jstsp_omp_kron_f64", "jstsp_sparse_admm_f64"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    assert _lib.SIGNATURES["jstsp_omp_f64"] == _lib.SIGNATURES["jstsp_omp_c64"]
    assert _lib.SIGNATURES["jstsp_omp_kron_f64"] == _lib.SIGNATURES["jstsp_omp_kron_c32"]
    assert _lib.SIGNATURES["jstsp_sparse_admm_f64"] == _lib.SIGNATURES["jstsp_sparse_admm_c64"]


def test_they_raise_without_a_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    rng = np.random.default_rng(0)
    c = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    calls = [lambda: J.OMP_f64(c(6, 9), c(6), 3), lambda: J.OMP_f64(c(6, 9).astype(np.complex64), c(2, 6), 3, want_target=False),
             lambda: J.omp_kron_f64(c(3, 4), c(5, 2), c(6), 3),
             lambda: J.sparse_admm_f64(c(4, 3), c(4, 3), c(4, 4), c(3, 3), 5),
             lambda: J.sparse_admm_f64(None, c(2, 4, 3), c(4, 4), c(3, 3), 5, want_ce=False)]
    for f in calls:
        with pytest.raises(J.JstspError):
            f()


def test_bad_shapes_raise_value_error_before_any_device_work():
    z = lambda *s: np.zeros(s, complex)
    with pytest.raises(ValueError):
        J.OMP_f64(z(6, 9), z(5), 3)                               # length(v) != size(A,1)
    with pytest.raises(ValueError):
        J.OMP_f64(z(2, 6, 9), z(3, 6), 3)                         # three problems, two dictionaries
    with pytest.raises(ValueError):
        J.OMP_f64(z(6, 9), z(6), 0)
    with pytest.raises(ValueError):
        J.omp_kron_f64(z(3, 4), z(5, 2), z(7), 3)                 # length(y) != N M
    with pytest.raises(ValueError):
        J.sparse_admm_f64(z(4, 3), z(4, 3), z(4, 5), z(3, 3), 5)  # Dr not square
    with pytest.raises(ValueError):
        J.sparse_admm_f64(z(4, 4), z(4, 3), z(4, 4), z(3, 3), 5)  # Htrue not the shape of OH
    with pytest.raises(ValueError):
        J.sparse_admm_f64(z(4, 3), z(4, 3), z(2, 4, 4), z(3, 3), 5)
    with pytest.raises(ValueError):
        J.sparse_admm_f64(None, z(4, 3), z(4, 4), z(3, 3), 5)     # the error curve needs Htrue
