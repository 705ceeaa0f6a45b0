"""CPU checks of tests/omp64_problems.py - that the GPU test of jstsp_omp_f64 / jstsp_omp_kron_f64 (tests/test_gpu_omp64.py)
asks for what the algorithm can give and for nothing less:

1. the generator facts: the D1 rows are complex128, their iteration-1 float64 gap lies in [1e-9, 1e-8] with the higher index
   winning ``D1hi`` and the lower ``D1lo``, and rounded to complex64 they are another problem; the D2 rows are E1's v times
   2^+-400 with E1's index set;
2. on every row of the set (E1-E6 and D) every selection of the literal reference has a float64 gap >= 1e-9 or exactly 0 - the
   premise of the device contract - and on the D rows every gap after the first is >= 1e-4 or exactly 0;
3. the literal OMP.m (``omp_literal``: pinv) and the structured one (``omp``: lstsq) select the same index set on every row."""
import numpy as np

import omp64_problems as Q
import omp_problems as P
from oracle import solvers as O


def test_the_d_rows_are_what_only_float64_can_express():
    for shape, groups in [(s, Q.dense_groups(s)) for s in Q.DENSE] + [(s, Q.kron_groups(s)) for s in Q.KRON]:
        main = groups[0]
        rows, Phi = main["rows"], main["Phi64"]
        for name, high in (("D1hi", True), ("D1lo", False)):
            r = rows[name]
            g = r["ref"]["gaps"]
            print(shape, name, "gaps", g)
            assert r["v"].dtype == np.complex128 and Q.D1_GAP[0] <= g[0] <= Q.D1_GAP[1]
            assert r["winner"] == (r["q"] if high else r["p"]) and r["ref"]["idx"][0] == r["winner"] + 1 and r["p"] < r["q"]
            c = P.first_corr(Phi, r["v"])
            lead = sorted(np.argsort(c)[-2:].tolist())
            assert lead == [r["p"], r["q"]] and np.delete(c, lead).max() < 0.8 * c[lead].min()
            assert not np.array_equal(r["v"].astype(np.complex64).astype(np.complex128), r["v"])
            assert abs(c[r["p"]] - c[r["q"]]) < 0.2 * P.ulp32(c.max())           # below what an fp32 correlation could hold
        for k in Q.V64_SCALES:
            r = rows["D2v%+d" % k]
            assert np.array_equal(r["v"], rows["E1"]["v"].astype(np.complex128) * 2.0 ** k)
            assert np.array_equal(r["ref"]["idx"], rows["E1"]["ref"]["idx"])
            big = np.max(np.abs(r["v"]))
            assert big > 3.5e38 or big < 1e-46                    # outside the complex64 range altogether


def test_every_selection_is_decisive_in_float64_or_an_exact_tie():
    n = 0
    for tag, G, name, r in Q.all_rows():
        assert Q.decisive(r), (tag, G["name"], name, r["ref"]["gaps"])
        if r["kind"].startswith("D1"):
            g = r["ref"]["gaps"][1:]
            assert np.all((g >= P.DECISIVE) | (g == 0.0)), (tag, name, g)
        n += 1
    assert n >= 3 * 15


def test_the_literal_and_the_structured_reference_select_the_same_atoms():
    for tag, G, name, r in Q.all_rows():
        m = len(r["ref"]["idx"])
        v = np.asarray(r["v"], np.complex128)
        _, i_lit, _, _ = O.omp_literal(G["Phi64"], v, m)
        _, i_str, _, _ = O.omp(G["Phi64"], v, m)
        assert np.array_equal(i_lit, r["ref"]["idx"]), (tag, G["name"], name)
        assert np.array_equal(i_lit, i_str), (tag, G["name"], name, i_lit.tolist(), i_str.tolist())
