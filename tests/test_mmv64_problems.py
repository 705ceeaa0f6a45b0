"""CPU checks of tests/mmv64_problems.py - that the GPU test of jstsp_mmv_omp_f64 (tests/test_gpu_mmv_omp64.py) asks for what
the algorithm can give and for nothing less:

1. the generator facts: 32 reused rows, the M8 rows' close selection has a float64 gap inside M8_GAP with the larger row at
   the higher index and every other gap >= 1e-3, the M9 rows are exact powers of two of the first row with its support;
2. the float64 numpy restatement of the kernel's algorithm selects the oracle's support on every (row, score) pair and its Z
   lies within TOL_Z / 100 of the oracle's: the device bound leaves two decades for the order of the sums;
3. the public surface without a GPU: the names exist and fail loudly, ``mmv_precision`` defaults to "f32" and is validated
   before any device work."""
import inspect

import numpy as np
import pytest

import mmv64_problems as Q
import mmv_problems as P
from conftest import check_below, rel_err

import jstsp19_amd as J


def test_the_reused_rows_and_the_generator_facts():
    pr = Q.problems()
    base = P.problems()["rows"]
    assert len(base) == 32 and all(a is b for a, b in zip(pr["rows"], base))
    m8 = [r for r in pr["rows"] if r["kind"] == "M8"]
    m9 = [r for r in pr["rows"] if r["kind"] == "M9"]
    assert len(m8) == 2 and len(m9) == len(Q.Y64_SCALES)
    for r in m8:
        assert r["A"].dtype == np.complex128 and r["atoms"][3] > r["atoms"][0]
        for norm in Q.NORMS:
            g = r["ref"][norm]["gaps"]
            print("%s %s gaps %s" % (r["name"], norm, g))
            assert Q.M8_GAP[0] <= g[1] <= Q.M8_GAP[1] and g[1] >= Q.GAP_MIN
            assert min(g[0], g[2], g[3]) >= P.DECISIVE
            assert r["ref"][norm]["sup"][1] == r["atoms"][3] and r["ref"][norm]["sup"][2] == r["atoms"][0]
            assert Q.decisive(r, norm)
        # the same values rounded to complex64 are an exact tie of the close pair: only float64 sees the difference.  Each atom
        # of the axis-aligned dictionary owns one row of Y, whose entries all have the planted magnitude
        row_of = lambda g: int(np.flatnonzero(r["A"][:, g - 1])[0])
        hi, lo = (np.abs(r["Y"][row_of(r["atoms"][i])]) for i in (3, 0))
        assert np.all(hi > lo) and np.all(hi == 3.0 * (1.0 + r["d"])) and np.all(lo == 3.0)
        y32 = r["Y"].astype(np.complex64)
        assert np.array_equal(np.abs(y32[row_of(r["atoms"][3])]), np.abs(y32[row_of(r["atoms"][0])]))
    for r in m9:
        b = Q.by_name(r["base"])
        k = r["scale_y"]
        assert np.array_equal(r["Y"], b["Y"].astype(np.complex128) * 2.0 ** k)
        for norm in Q.NORMS:
            assert np.array_equal(r["ref"][norm]["sup"], b["ref"][norm]["sup"])


@pytest.mark.parametrize("norm", Q.NORMS)
def test_the_restatement_agrees_with_the_oracle_on_every_row(norm):
    worst = 0.0
    for r in Q.problems()["rows"]:
        Z, sup, ratio = Q.restate(r["A"], r["Y"], r["K"], norm)
        ref = r["ref"][norm]
        assert np.array_equal(sup, ref["sup"]), (r["name"], norm, sup.tolist(), ref["sup"].tolist())
        err = rel_err(Z, ref["Z"])
        worst = max(worst, err)
        if r["kind"] == "M3":
            assert np.array_equal(Z, r["Z_exact"])
        if r["kind"] == "M6":
            assert not Z.any()
        check_below("mmv64_problems/restatement.Z", err, Q.TOL_Z / 100)
    print("restatement, %s: largest rel_err(Z) %.3g" % (norm, worst))


def test_the_names_are_exported_and_fail_loudly_without_a_gpu():
    from jstsp19_amd import _lib, solvers
    for n in ("mmv_omp_f64", "mc_svt_f64", "mc_admm_f64", "tssr_f64"):
        assert callable(getattr(J, n)) and n in solvers.__all__
    lib = J.load()
    for n in ("jstsp_mmv_omp_f64", "jstsp_mc_svt_f64", "jstsp_mc_admm_f64"):
        assert hasattr(lib, n) and n in _lib.SIGNATURES
    with pytest.raises(ValueError):
        J.mmv_omp_f64(np.zeros((4, 6), complex), np.zeros((5, 3), complex), 2)
    with pytest.raises(ValueError):
        J.mc_svt_f64(np.zeros((4, 6), complex), np.zeros((4, 5)), 3, 0.1, 0.1)
    import torch
    if not torch.cuda.is_available():
        with pytest.raises(J.JstspError):
            J.mmv_omp_f64(np.eye(3, dtype=complex), np.ones((3, 2), complex), 2)
        with pytest.raises(J.JstspError):
            J.mc_svt_f64(np.ones((3, 4), complex), np.ones((3, 4)), 2, 0.1, 0.1)
        with pytest.raises(J.JstspError):
            J.mc_admm_f64(None, np.ones((3, 4), complex), np.ones((3, 4)), 2, 0.1, 0.1, want_ce=False)


def test_mmv_precision_is_validated_before_any_device_work():
    from jstsp19_amd import montecarlo as mc
    with pytest.raises(ValueError):
        mc.run_points([], 1, mmv_precision="f16", device="cpu", builder=lambda *a: None)
    with pytest.raises(ValueError):
        mc._hip_baselines({}, 100, mmv_precision="double")
    assert inspect.signature(mc.run_points).parameters["mmv_precision"].default == "f32"
    assert inspect.signature(mc._hip_baselines).parameters["mmv_precision"].default == "f32"
    assert inspect.signature(mc.run_points).parameters["ls_precision"].default == "f32"
