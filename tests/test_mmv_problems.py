"""The engineered joint-OMP problem set of tests/mmv_problems.py is what it claims to be (CPU only): every fact the device
tests of tests/test_gpu_mmv_omp_paths.py rely on is checked here against float64 arithmetic on the complex64 values."""
import collections

import numpy as np
import pytest

import mmv_problems as P
from oracle import solvers as O


@pytest.fixture(scope="module")
def rows():
    return P.problems()["rows"]


def _kind(rows, kind):
    return [r for r in rows if r["kind"] == kind]


def test_every_kind_contributes_its_rows_and_every_row_its_references(rows):
    assert dict(collections.Counter(r["kind"] for r in rows)) == P.COUNTS
    for r in rows:
        assert r["A"].dtype == np.complex64 and r["Y"].dtype == np.complex64 and r["A"].shape[0] == r["Y"].shape[0]
        assert np.all(np.isfinite(r["A"])) and np.all(np.isfinite(r["Y"]))
        for norm in P.NORMS:
            ref = r["ref"][norm]
            Z, sup = O.mmv_omp(r["A"], r["Y"], r["K"], norm)                   # the margins variant changes no answer
            assert np.array_equal(sup, ref["sup"]) and np.array_equal(Z, ref["Z"])
            assert ref["count"] == len(ref["sup"]) == len(ref["gaps"]) <= min(r["K"], *r["A"].shape)
            assert len(set(ref["sup"].tolist())) == ref["count"] and np.all(ref["gaps"] >= 0) and np.all(ref["gaps"] <= 1)
            assert np.count_nonzero(np.abs(Z).sum(axis=1)) <= ref["count"]


def test_margins_are_the_gaps_of_the_scores():
    """``mmv_omp_margins`` on a problem small enough to restate by hand: two orthogonal atoms and a third between them."""
    A = np.array([[1, 0, 0.6], [0, 1, 0.8]], complex)
    Y = np.array([[2.0, 0.0], [0.0, 1.0]], complex)
    for norm, s in (("l2", [4.0, 1.0, 1.44 + 0.64]), ("l1", [2.0, 1.0, 1.2 + 0.8])):
        Z, sup, gaps = O.mmv_omp_margins(A, Y, 2, norm)
        top = sorted(s)
        assert sup[0] == 1 and gaps[0] == pytest.approx((top[2] - top[1]) / top[2], abs=1e-14)
        assert len(gaps) == len(sup) == 2
    Z, sup, gaps = O.mmv_omp_margins(A[:, :1], Y, 3)
    assert sup.tolist() == [1] and gaps.tolist() == [1.0]                      # a single candidate
    Z, sup, gaps = O.mmv_omp_margins(A, 0 * Y, 3)
    assert sup.tolist() == [1] and gaps.tolist() == [0.0] and not Z.any()      # every score 0: a tie


def test_m1_shapes_gaps_and_conditioning(rows):
    m1 = _kind(rows, "M1")
    assert [r["shape"] for r in m1[:len(P.M1_SHAPES)]] == P.M1_SHAPES
    for r in m1:
        N, Gr, S, K = r["shape"]
        assert r["A"].shape == (N, Gr) and r["Y"].shape == (N, S) and r["K"] == K
        for norm in P.NORMS:
            ref = r["ref"][norm]
            assert ref["count"] == min(K, N, Gr)                               # noisy: no early stop
            assert ref["gaps"].min() >= P.DECISIVE
            assert P.support_cond(r["A"], ref["sup"]) <= P.COND_MAX
            if Gr > 256:                                                       # a kernel that skipped its last atom pass fails
                assert np.isin(ref["sup"] - 1, P.last_pass(Gr)).any(), (r["name"], norm)
    pr = P.problems()
    own, shared = [P.by_name(n) for n in pr["own"]], [P.by_name(n) for n in pr["shared"]]
    assert len(own) == len(shared) == 3
    assert all(np.array_equal(r["A"], m1[0]["A"]) for r in shared)
    assert not np.array_equal(own[0]["A"], own[1]["A"]) and not np.array_equal(own[1]["A"], own[2]["A"])
    # the branches of the score split the shapes were chosen for: gp = power of two >= Gr (<= 256), ncg = 256 / gp
    split = set()
    for N, Gr, S, K in P.M1_SHAPES:
        gp = 1
        while gp < Gr and gp < 256:
            gp <<= 1
        ncg = 256 // gp
        split.add((ncg, -(-Gr // gp) > 1, Gr % gp != 0, S < ncg, S > 256, N > 256))
    assert {s[0] for s in split} >= {1, 4, 8, 32, 256}
    for i in range(1, 6):
        assert any(s[i] for s in split) and any(not s[i] for s in split), i


def test_m2_ties_are_exact(rows):
    m2 = _kind(rows, "M2")
    assert {r["A"].shape[1] > 256 for r in m2} == {True, False}
    for r in m2:
        A, j, (k1, k2, k3) = r["A"], r["j"], r["copies"]
        assert j < k1 < k2 < k3
        assert np.array_equal(A[:, k1], A[:, j]) and np.array_equal(A[:, k2], -A[:, j])
        assert np.array_equal(A[:, k3].real, -A[:, j].imag) and np.array_equal(A[:, k3].imag, A[:, j].real)
        C = np.abs(A.astype(complex).conj().T @ r["Y"].astype(complex))
        for norm in P.NORMS:
            ref = r["ref"][norm]
            score = C.sum(axis=1) if norm == "l1" else (C ** 2).sum(axis=1)
            assert int(np.argmax(score)) == j and score[k1] == score[j]
            assert ref["sup"][0] == j + 1 and ref["gaps"][0] == 0.0
            assert ref["gaps"][1:].min() >= P.DECISIVE and ref["count"] == r["K"]
            assert not set(ref["sup"].tolist()) & {k1 + 1, k2 + 1, k3 + 1}     # a copy is dependent once j is in: never chosen


def test_m3_residual_is_exactly_zero_after_s_atoms(rows):
    m3 = _kind(rows, "M3")
    assert {r["A"].shape[0] > 256 for r in m3} == {True, False}
    for r in m3:
        A, Y, s = r["A"], r["Y"], r["s"]
        assert s < r["K"]
        G = A.astype(complex).conj().T @ A.astype(complex)
        assert np.array_equal(G, np.eye(A.shape[1]))                          # axis-aligned: exactly orthonormal
        assert np.array_equal(A.astype(complex) @ r["Z_exact"].astype(complex), Y.astype(complex))
        assert np.array_equal(r["Z_exact"].real, np.round(r["Z_exact"].real)) and np.abs(r["Z_exact"]).max() <= s
        for norm in P.NORMS:
            ref = r["ref"][norm]
            assert ref["count"] == s and np.array_equal(ref["sup"], r["atoms"]) and ref["gaps"].min() >= 0.1
            assert np.max(np.abs(ref["Z"] - r["Z_exact"])) < 1e-12


def test_m4_reference_stops_at_the_sparsity(rows):
    m4 = _kind(rows, "M4")
    for r in m4:
        s = r["s"]
        assert s < r["K"] <= min(r["A"].shape)
        for norm in P.NORMS:
            ref = r["ref"][norm]
            assert ref["count"] == s and ref["gaps"].min() >= P.DECISIVE
            assert P.support_cond(r["A"], ref["sup"]) <= P.COND_MAX
            R = r["Y"].astype(complex) - r["A"].astype(complex) @ ref["Z"]
            rel = np.linalg.norm(R) / np.linalg.norm(r["Y"])
            assert 1e-9 < rel < 1e-6                                           # complex64 rounding of Y: under the stop, not 0


def test_m5_reference_stops_at_the_rank(rows):
    m5 = _kind(rows, "M5")
    assert [("p" in r) for r in m5] == [False, True]
    for r in m5:
        sv = np.linalg.svd(r["A"].astype(complex), compute_uv=False)
        assert r["r"] < r["K"] and sv[r["r"]] < 1e-6 * sv[0] and sv[r["r"] - 1] > 1e-2 * sv[0]
        first = 0
        if "p" in r:
            p, q = r["p"], r["q"]
            assert p < q and np.array_equal(r["A"][:, p], r["A"][:, q])
            first = 1
        for norm in P.NORMS:
            ref = r["ref"][norm]
            assert ref["count"] == r["r"] and ref["gaps"][first:].min() >= P.DECISIVE
            if first:
                assert ref["sup"][0] == r["p"] + 1 and ref["gaps"][0] == 0.0 and r["q"] + 1 not in ref["sup"]
            R = r["Y"].astype(complex) - r["A"].astype(complex) @ ref["Z"]
            assert np.linalg.norm(R) > 0.1 * np.linalg.norm(r["Y"])            # stopped by dependence, not by the residual


def test_m6_zero_input(rows):
    m6 = _kind(rows, "M6")
    assert {r["A"].shape[1] > 256 for r in m6} == {True, False}
    for r in m6:
        assert not r["Y"].any()
        for norm in P.NORMS:
            ref = r["ref"][norm]
            assert ref["sup"].tolist() == [1] and ref["count"] == 1 and not ref["Z"].any()


def test_m7_scaling_is_exact_and_the_reference_scale_free(rows):
    m7 = _kind(rows, "M7")
    assert sorted(r["scale_y"] for r in m7 if "scale_y" in r) == sorted(P.Y_SCALES)
    assert sorted(r["scale_a"] for r in m7 if "scale_a" in r) == sorted(P.A_SCALES)
    for r in m7:
        base = P.by_name(r["base"])
        assert base["kind"] == "M1"
        ky, ka = r.get("scale_y", 0), r.get("scale_a", 0)
        assert np.array_equal(r["Y"].astype(complex), base["Y"].astype(complex) * 2.0 ** ky)
        assert np.array_equal(r["A"].astype(complex), base["A"].astype(complex) * 2.0 ** ka)
        assert np.all(np.isfinite(r["Y"])) and np.all(np.isfinite(r["A"]))
        tiny = np.finfo(np.float32).tiny
        for X in (r["Y"], r["A"]):                                             # no component lost to the denormal range
            comp = np.abs(np.concatenate([X.real.ravel(), X.imag.ravel()]))
            assert comp[comp > 0].min() >= tiny
        for norm in P.NORMS:
            ref, b = r["ref"][norm], base["ref"][norm]
            assert np.array_equal(ref["sup"], b["sup"])
            np.testing.assert_allclose(ref["gaps"], b["gaps"], rtol=1e-9)
            np.testing.assert_allclose(ref["Z"], b["Z"] * 2.0 ** (ky - ka), rtol=0, atol=1e-10 * np.abs(b["Z"]).max() * 2.0 ** (ky - ka))
    with pytest.raises(AssertionError):
        P.exact_scale(np.array([1e-30 + 0j], np.complex64), -100)              # would leave the normal range: refused
