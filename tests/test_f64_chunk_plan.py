"""The chunk plan of the float64 proposed_algorithm functions (jstsp19_amd/solvers.py: _f64_admm_bytes, _f64_chunks).  Above Gram
order 64 the global Jacobi sweeps a chunk's trials together (include/jstsp.h), so the plan is part of a result's last bits: the
per-trial byte estimate of each of the four public functions is held against the formula that function had when it carried its
own, restated here literally, on every combination of shared / per-trial dictionaries, host / device and given / inverted factors."""
import itertools

import pytest

from jstsp19_amd import solvers

SHAPES = [(32, 35, 40, 48), (72, 80, 64, 72)]


def _plain_alg2(N, M, Gr, G2, sA, sB, own_PA, own_PB, host):
    n = min(N, M)
    per = 16 * (8 * N * M + 5 * Gr * G2 + Gr * M + N * G2 + 20 * n * n + (G2 * G2 if sB else 0) + (Gr * Gr if sA else 0))
    if host:
        per += 16 * (2 * N * M + Gr * G2 + (G2 * M if sB else 0) + (N * Gr if sA else 0)) + 8 * N * M
    return per


def _plain_std(N, M, Gr, G2, sA, sB, own_PA, own_PB, host):
    n = min(N, M)
    per = 16 * (8 * N * M + 2 * Gr * G2 + Gr * M + N * G2 + 20 * n * n)
    per += 16 * ((2 * N * Gr + 3 * Gr * Gr if sA and own_PA else 0) + (2 * G2 * M + 3 * G2 * G2 if sB and own_PB else 0))
    if host:
        per += 16 * (2 * N * M + Gr * G2 + 2 * (G2 * M if sB else 0) + 2 * (N * Gr if sA else 0)) + 8 * N * M
    return per


def _resumed(std, N, M, Gr, G2, sA, sB, own_PA, own_PB, host):
    n = min(N, M)
    ne = 4 * N * M + 2 * Gr * G2
    per = 16 * (8 * N * M + 5 * Gr * G2 + Gr * M + N * G2 + 20 * n * n + (G2 * G2 if sB else 0) + (Gr * Gr if sA else 0))
    if std:
        per += 16 * ((2 * N * Gr + 3 * Gr * Gr if sA and own_PA else 0) + (2 * G2 * M + 3 * G2 * G2 if sB and own_PB else 0))
    if host:
        per += 16 * (2 * N * M + Gr * G2 + 2 * (G2 * M if sB else 0) + 2 * (N * Gr if sA else 0) + 2 * ne) + 8 * N * M
    return per


@pytest.mark.parametrize("shape", SHAPES)
def test_the_byte_estimate_of_each_caller_is_the_formula_it_had(shape):
    N, M, Gr, G2 = shape
    seen = set()
    for per_A, per_B, own_PA, own_PB, host in itertools.product((False, True), repeat=5):
        sA, sB = (N * Gr if per_A else 0), (G2 * M if per_B else 0)
        a = (N, M, Gr, G2, sA, sB, own_PA, own_PB, host)
        got = lambda std, resumed: solvers._f64_admm_bytes(N, M, Gr, G2, sA, sB, std, own_PA, own_PB, host, resumed)
        assert got(False, False) == _plain_alg2(*a)                # proposed_algorithm_f64
        assert got(True, False) == _plain_std(*a)                  # proposed_algorithm_std_f64
        assert got(False, True) == _resumed(False, *a)             # proposed_algorithm_resume_f64
        assert got(True, True) == _resumed(True, *a)               # proposed_algorithm_std_resume_f64
        seen.add((got(False, False), got(True, False), got(False, True), got(True, True)))
    assert len(seen) > 8                                           # (the combinations do move the estimates)


def test_the_chunks_of_a_batch(monkeypatch):
    per = solvers._f64_admm_bytes(72, 80, 64, 72, 72 * 64, 0, True, True, False, True, True)
    monkeypatch.setattr(solvers, "_F64_CHUNK_BYTES", 3 * per)
    assert list(solvers._f64_chunks(7, per)) == [(0, 3), (3, 3), (6, 1)]
