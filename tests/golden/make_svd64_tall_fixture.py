#!/usr/bin/env python3
"""Writes tests/golden/svd64_tall_restatement_worst.json: the worst error measures of the numpy restatement of the QR route
(tests/svd64_tall_problems.py) and of numpy.linalg.svd over SHAPES x the problem classes and over the one 64 x 65536 matrix of the
GPU test, from which tests/test_gpu_svd64_tall.py takes its bounds.  numpy only; the large matrix takes a few minutes.

    python tests/golden/make_svd64_tall_fixture.py
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import spectrum_problems as P          # noqa: E402
import svd64_problems as S             # noqa: E402
import svd64_tall_problems as T        # noqa: E402


def main():
    small = T.small_records()
    A = T.big_problem()
    ref = P.ref(A)
    U, sv, V, rank, conv = T.tsqr_svd_ref(A)
    Un, sn, Vn = S.numpy_svd(A)
    big = S.measures(A[0], U[0], sv[0], V[0], ref[0])
    big_np = S.measures(A[0], Un[0], sn[0], Vn[0], ref[0])
    assert all(r[5] for r in small) and conv[0] == 1 and rank[0] == min(T.BIG_SHAPE)
    worst = S.worst([r[3] for r in small] + [big])
    worst["e_rec_nothing_dropped"] = max([r[3]["e_rec"] for r in small if not r[6]] + [big["e_rec"]])
    rec = {"restatement": worst,
           "numpy": S.worst([r[4] for r in small] + [big_np]),
           "small_shapes": {"restatement": T.recomputed_worst(), "numpy": S.worst([r[4] for r in small])},
           "%dx%d" % T.BIG_SHAPE: {"restatement": big, "numpy": big_np},
           "drops_a_value": ["%dx%d %s" % (r[0], r[1], r[2]) for r in small if r[6]],
           "per_case": {"%dx%d %s" % (r[0], r[1], r[2]): r[3] for r in small}}
    with open(T.FIXTURE, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: rec[k] for k in ("restatement", "numpy")}, sort_keys=True))


if __name__ == "__main__":
    main()
