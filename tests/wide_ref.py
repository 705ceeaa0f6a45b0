"""Helper of the widened-support-order tests (not a test module), numpy: the order ``jstsp_support_order_wide_c32`` / ``_f64``
return, from the definition in include/jstsp.h."""
import numpy as np

import drift_ref as D

PRIMARIES = ("neighbourhood", "ties")


def wide_keys(S, Gt, wr, wt, dtype):
    """``(own, nbr)`` of one trial ``S`` (Gr, Gt*L) in the key space of csrc/support_key.h, each (Gr*Gt*L,) uint64 in vec(S)
    order: ``own = ~bits(|z|^2)`` in ``dtype`` (a NaN: 0), ``nbr`` the minimum of ``own`` over the ``(2 wr + 1) x (2 wt + 1)``
    window that is circular in the rows and in the ``Gt`` columns of its own delay block."""
    S = np.asarray(S)
    Gr, G2 = S.shape
    assert G2 % Gt == 0 and 2 * wr + 1 <= Gr and 2 * wt + 1 <= Gt
    L = G2 // Gt
    m2 = D.support_key(S, dtype)                                   # vec(S), column-major
    bits = m2.view(np.uint32).astype(np.uint64) if dtype is np.float32 else m2.view(np.uint64)
    full = np.uint64(0xFFFFFFFF if dtype is np.float32 else 0xFFFFFFFFFFFFFFFF)
    own = np.where(np.isnan(m2), np.uint64(0), bits ^ full)
    cube = own.reshape(L, Gt, Gr).transpose(2, 0, 1)               # (Gr, L, Gt): entry (r, l, g) is S(r, l*Gt + g)
    nbr = cube.copy()
    for dr in range(-wr, wr + 1):
        for dg in range(-wt, wt + 1):
            nbr = np.minimum(nbr, np.roll(cube, (dr, dg), axis=(0, 2)))
    return own, nbr.transpose(1, 2, 0).reshape(-1)


def support_order_wide_ref(S, Gt, wr, wt, primary, dtype):
    """1-based order of one trial: ascending ``(nbr, own, index)`` for ``"neighbourhood"``, ``(own, nbr, index)`` for ``"ties"``."""
    assert primary in PRIMARIES
    own, nbr = wide_keys(S, Gt, wr, wt, dtype)
    index = np.arange(own.size)
    order = np.lexsort((index, own, nbr)) if primary == "neighbourhood" else np.lexsort((index, nbr, own))
    return (order + 1).astype(np.int32)
