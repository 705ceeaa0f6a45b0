"""The float64 margin oracle and the engineered OMP problems of tests/omp_problems.py (CPU only): the generator produces
what tests/test_gpu_omp_paths.py relies on."""
import numpy as np
import pytest

import omp_problems as P
from conftest import load_golden
from oracle import solvers as O


def test_omp_literal_margins_is_omp_literal_plus_the_gaps():
    g = load_golden("omp")
    rng = np.random.default_rng(3)
    A = rng.standard_normal((30, 50)) + 1j * rng.standard_normal((30, 50))
    cases = [(g["A0"], g["v0"], int(g["m0"])), (g["A1"], g["v1"], int(g["m1"])), (A, A[:, 7] - 2 * A[:, 11], 6),
             (np.eye(3), np.array([2.0, 0, 0]), 3), (A, np.zeros(30), 4), (A[:, :1], A[:, 0], 2)]
    for A_, v, m in cases:
        x, idx, vv, T = O.omp_literal(A_, v, m)
        x2, idx2, vv2, T2, gaps = O.omp_literal_margins(A_, v, m)
        assert np.array_equal(idx, idx2) and np.array_equal(x, x2) and np.array_equal(T, T2) and np.array_equal(vv, vv2)
        assert gaps.shape == (m,) and np.all((gaps >= 0) & (gaps <= 1))
    # gap of the first iteration by hand; the identity with v = 2 e1: a decisive pick, then all-zero correlations (a tie)
    _, _, _, _, gaps = O.omp_literal_margins(A, A[:, 7] - 2 * A[:, 11], 1)
    c = np.sort(np.abs(A.conj().T @ (A[:, 7] - 2 * A[:, 11])))
    assert gaps[0] == (c[-1] - c[-2]) / c[-1]
    assert list(O.omp_literal_margins(np.eye(3), np.array([2.0, 0, 0]), 2)[4]) == [1.0, 0.0]
    assert list(O.omp_literal_margins(A[:, :1], A[:, 0], 2)[4]) == [1.0, 1.0]


def _check_groups(groups, m):
    main = {r: row for G in groups for r, row in G["rows"].items()}
    assert set(main) == {"E1", "E2", "E3hi", "E3lo", "E4a", "E4b", "E5", "E6v-100", "E6v-70", "E6v+70", "E6v+100",
                         "E6A-40", "E6A+40"}
    for G in groups:
        Phi = G["Phi64"]
        if G["name"] != "ident":           # every iteration selects from a residual that is not round-off
            assert np.linalg.matrix_rank(Phi) >= m, G["name"]
        for name, row in G["rows"].items():
            v, ref = row["v"], row["ref"]
            assert v.dtype == np.complex64 and ref["idx"].shape == (m,)
            # the reference ran on exactly these values
            assert np.array_equal(ref["idx"], O.omp_literal(Phi, v.astype(complex), m)[1]), name
            g = ref["gaps"]
            if row["kind"] in ("E1", "E6"):
                assert g.min() >= P.DECISIVE, (name, g.min())
            elif row["kind"] == "E2":
                c = P.first_corr(Phi, v)
                j, ks = row["j"], row["copies"]
                assert all(k > j for k in ks) and np.array_equal(Phi[:, ks[0]], Phi[:, j]) and np.array_equal(Phi[:, ks[1]], -Phi[:, j])
                assert all(c[k] == c[j] for k in ks) and c[j] == c.max() and g[0] == 0.0 and ref["idx"][0] == j + 1
                assert np.all((g[1:] >= P.DECISIVE) | (g[1:] == 0.0))
            elif row["kind"] in ("E3hi", "E3lo"):
                c = P.first_corr(Phi, v)
                p, q, win = row["p"], row["q"], row["winner"]
                lose = q if win == p else p
                assert p < q and win == (q if row["kind"] == "E3hi" else p) and ref["idx"][0] == win + 1
                assert 1.0 <= (c[win] - c[lose]) / P.ulp32(c[win]) <= 4.0
                assert np.delete(c, [p, q]).max() < 0.8 * c[lose] and g[1:].min() >= P.DECISIVE
            elif row["kind"] in ("E4a", "E4b"):
                s = row["s"]
                res = P.e4_residual_norms(Phi, v, ref["idx"])
                assert np.all(res[:s - 1] > 0) and res[s - 1] == 0.0                   # exactly zero after s atoms
                assert sorted(ref["idx"][:s] - 1) == list(row["support"]) and np.all(ref["idx"][s:] == 1)
                assert np.all(g[:s] >= P.DECISIVE) and np.all(g[s:] == 0.0)
                if row["kind"] == "E4b":
                    assert res[s] == 0.0 and 0 not in row["support"]
                else:
                    # the duplicate of atom 1: pinv splits its coefficient (OMP.m:19, 29-32)
                    x0 = np.linalg.lstsq(Phi[:, row["support"]], v.astype(complex), rcond=None)[0][0]
                    assert abs(ref["x"][0] - x0 / 2) < 1e-12 * abs(x0)
            elif row["kind"] == "E5":
                assert not np.any(v) and np.all(ref["idx"] == 1) and not np.any(ref["x"]) and np.all(np.isfinite(ref["x"]))
        if G["name"] == "main":
            e1 = G["rows"]["E1"]
            for k in P.V_SCALES:
                row = G["rows"]["E6v%+d" % k]
                assert np.array_equal(row["v"], e1["v"] * np.float32(2.0 ** k))              # exact in complex64
                assert np.array_equal(row["v"] * np.float32(2.0 ** -k), e1["v"])
                assert np.array_equal(row["ref"]["idx"], e1["ref"]["idx"])
    e1 = main["E1"]
    for k in P.A_SCALES:
        assert np.array_equal(main["E6A%+d" % k]["ref"]["idx"], e1["ref"]["idx"])
        assert np.array_equal(main["E6A%+d" % k]["v"], e1["v"])


@pytest.mark.parametrize("meas,size_d,m", [(96, 160, 10), (1024, 256, 24)])
def test_dense_engineered_problems_are_what_they_claim(meas, size_d, m):
    _check_groups(P.dense_groups(meas, size_d, m, seed=meas + m), m)


@pytest.mark.parametrize("m", [24, 97])
def test_kron_engineered_problems_are_what_they_claim(m):
    groups = P.kron_groups(8, 16, 8, 16, m, seed=m)
    for G in groups:
        Af, Bf = G["dict"]
        assert Af.dtype == Bf.dtype == np.complex64 and np.array_equal(G["Phi64"], P.kron_phi((Af, Bf)))
    _check_groups(groups, m)
