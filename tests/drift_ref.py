"""Helper of the drifting-channel and support-order tests (not a test module), float64 numpy: the angle walk of
``jstsp_build_trials_tracked_drift_c32``, the channel of wideband_mmwave_channel.m:12-35 from given angles, and the order
``jstsp_support_order_c32`` / ``_f64`` return."""
import numpy as np

from oracle import system_model as osm


def walk(z, drift):
    """``phi_f - phi_0`` for f = 0 .. F from the increments ``z`` (F, ...): ``drift * sum_{k=1..f} z_k``, summed in ascending k in
    float64 and multiplied once.  Returns (F + 1, ...); row 0 is zero."""
    z = np.asarray(z, dtype=np.float64)
    acc = np.zeros((z.shape[0] + 1,) + z.shape[1:])
    for k in range(z.shape[0]):
        acc[k + 1] = acc[k] + z[k]
    return float(drift) * acc


def channel_from_angles(gains, phi_r, phi_t, clusters, rays, Nr, Nt):
    """oracle/system_model.py:103-115 (wideband_mmwave_channel.m:12-33) with the angles given instead of the uniform draws:
    ``gains`` (L, Np) complex, ``phi_r`` / ``phi_t`` (Np,) the angles of tap 1 - which every tap uses (:24).  The cumulative ``Hl``
    is added once per cluster (:29).  Returns H (Nr, Nt, L) complex128."""
    gains = np.asarray(gains, dtype=complex)
    L, Np = gains.shape
    assert Np == clusters * rays
    Ar = np.stack([osm._steer(phi_r[i], Nr) for i in range(Np)], axis=1)        # :20-21, page 1
    At = np.stack([osm._steer(phi_t[i], Nt) for i in range(Np)], axis=1)        # :22
    H = np.zeros((Nr, Nt, L), complex)
    for l in range(L):
        Hl = np.zeros((Nr, Nt), complex)
        index = 0
        for _tap in range(clusters):
            for _ray in range(rays):
                Hl = Hl + gains[l, index] * np.outer(Ar[:, index], At[:, index].conj())     # :24
                index += 1
            H[:, :, l] = H[:, :, l] + Hl                                        # :29
        H[:, :, l] = H[:, :, l] / np.sqrt(Np)                                   # :33
    return H


def support_key(S, dtype):
    """``|z|^2 = x*x + y*y`` of vec(S) (column-major) with every product and the sum rounded to ``dtype`` (np.float32 or
    np.float64)."""
    v = np.asarray(S).reshape(-1, order="F")
    x, y = v.real.astype(dtype), v.imag.astype(dtype)
    with np.errstate(over="ignore", invalid="ignore"):
        return (x * x).astype(dtype) + (y * y).astype(dtype)


def support_order_ref(S, dtype):
    """``[~, indx] = sort(abs(vec(S)), 'descend')``, 1-based: a stable argsort of the negated key in ``dtype``, NaN first (as
    MATLAB's descending sort), then +Inf; equal keys in ascending index."""
    key = support_key(S, dtype)
    order = np.argsort(-key, kind="stable")                    # numpy sorts a NaN last, in index order
    nan = np.isnan(key[order])
    return (np.concatenate([order[nan], order[~nan]]) + 1).astype(np.int32)
