"""CPU checks of tests/std_problems.py: the pinv_fits mirror against the formula in csrc/pinv.hip, and the factor builder's
condition numbers."""
import os
import re

import numpy as np
import pytest

import std_problems as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pinv_fits_mirror_matches_the_kernel_formula():
    """The mirror restates pinv_lds / pinv_fits of csrc/pinv.hip term by term: if the kernel's LDS layout changes, this fails
    and the mirror (and the boundary shapes of the GPU tests) must follow."""
    src = open(os.path.join(ROOT, "jstsp19_amd", "csrc", "pinv.hip")).read()
    body = re.search(r"size_t pinv_lds\(int rows, int cols\)\s*\{(.*?)\n\}", src, re.S).group(1)
    assert "const int m = std::max(rows, cols), n = std::min(rows, cols), ne = (n + 1) & ~1;" in body
    expr = " ".join(re.search(r"return (.*?);", body, re.S).group(1).split())
    assert expr == ("((size_t)ne * m + (size_t)ne * ne) * sizeof(d2) + (size_t)(ne + 8) * sizeof(double)")
    assert re.search(r"struct d2 \{ double x, y; \};", src)
    assert "return rows > 0 && cols > 0 && pinv_lds(rows, cols) <= 156 * 1024;" in src
    assert P.LDS_LIMIT == 156 * 1024
    for rows in (1, 2, 3, 17, 64, 91, 92, 607, 608):
        for cols in (1, 2, 3, 16, 17, 64):
            m, n = max(rows, cols), min(rows, cols)
            ne = n + (n & 1)
            assert P.pinv_lds(rows, cols) == (ne * m + ne * ne) * 16 + (ne + 8) * 8
            assert P.pinv_fits(rows, cols) == (P.pinv_lds(rows, cols) <= P.LDS_LIMIT) == P.pinv_fits(cols, rows)


def test_pinv_fits_boundaries_and_routes():
    # the shapes INTEGRATION.md names as fitting, and the boundaries the GPU tests use
    assert P.pinv_fits(64, 64) and P.pinv_fits(140, 16) and P.pinv_fits(512, 16)
    assert P.largest_fitting(16) == 607 and not P.pinv_fits(16, 608)
    assert P.largest_fitting(64) == 91 and not P.pinv_fits(64, 92)
    assert P.largest_fitting(63) == P.largest_fitting(64)               # odd orders are padded to even
    assert P.route(32, 70, 32, 16) == ("pinv", "pinv")                   # the Alg. 1 driver (plot_errorVSsnr_approx.m)
    assert P.route(32, 92, 31, 64) == ("pinv", "eig")
    assert P.route(24, 200, 17, 140) == ("pinv", "ns")
    assert P.route(100, 100, 64, 65) == ("eig", "eig")
    assert P.gram_route(128) == "eig" and P.gram_route(129) == "ns"
    assert P.refuse_threshold(8) == 1e-6 and P.refuse_threshold(128) == pytest.approx(1.526e-5, rel=1e-3)


@pytest.mark.parametrize("rows,cols", [(16, 16), (40, 17), (17, 40), (64, 92), (140, 160)])
@pytest.mark.parametrize("c", [1.0, 10.0, 1e3, 1e5])
def test_factor_has_the_condition_it_claims(rows, cols, c):
    rng = np.random.default_rng(rows * 1000 + cols)
    X = P.factor(rng, rows, cols, c, scale=3.0)
    s = np.linalg.svd(X, compute_uv=False)
    assert len(s) == min(rows, cols)
    assert s[0] == pytest.approx(3.0, rel=1e-12)
    assert P.cond(X) == pytest.approx(c, rel=1e-9)
    np.testing.assert_allclose(s, 3.0 * np.geomspace(1.0, 1.0 / c, len(s)), rtol=1e-9)      # geometric spacing
    # what the device sees: rounded to complex64, the condition moves by at most ~ eps32 * cond
    assert P.cond(X.astype(np.complex64)) == pytest.approx(c, rel=max(1e-6, 20 * 6e-8 * c))


@pytest.mark.parametrize("flat", [False, True])
def test_two_level_factor_has_its_condition_and_spread(flat):
    rng = np.random.default_rng(11)
    n = 256
    X = P.factor_two_level(rng, n, n + 24, 300.0, flat=flat)
    s = np.linalg.svd(X, compute_uv=False)
    assert P.cond(X) == pytest.approx(300.0, rel=1e-9)
    assert np.sum(np.isclose(s, 1.0)) == n // 2 and np.sum(np.isclose(s, 1 / 300.0)) == n // 2
    G = X @ X.conj().T
    g1 = np.abs(G).sum(axis=0).max() / np.linalg.eigvalsh(G)[-1]
    assert g1 > 0.3 * np.sqrt(n)            # the slow Newton-Schulz start the GPU test is there for


def test_haar_columns_are_orthonormal_and_unbiased():
    rng = np.random.default_rng(3)
    Q = P.haar(rng, 50, 20)
    np.testing.assert_allclose(Q.conj().T @ Q, np.eye(20), atol=1e-13)
    # phases fixed by R's diagonal: the mean of many draws of an entry is ~0 (a plain QR biases diag(R) > 0)
    m = np.mean([P.haar(rng, 4, 4)[0, 0] for _ in range(4000)])
    assert abs(m) < 0.05
