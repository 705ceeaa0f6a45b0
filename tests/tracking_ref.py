"""Float64 numpy restatement of the path-gain model of a tracked channel (include/jstsp.h: jstsp_build_trials_tracked_c32), written
as the RECURSION of tools/run_tracking.py

    g_0 = w_0,    g_f = corr g_{f-1} + sqrt(1 - corr^2) w_f,

while the library evaluates the closed form  g_f = corr^f w_0 + sqrt(1 - corr^2) sum_{k=1..f} corr^(f-k) w_k:  the two forms check
each other.  ``w``: the innovations, frame index first, any trailing shape, real or complex."""
import numpy as np


def gains_recursion(w, corr):
    """All frames g_0 .. g_{F-1} of the recursion on the innovations ``w`` (F, ...); float64 / complex128, same shape."""
    w = np.asarray(w)
    w = w.astype(np.complex128 if np.iscomplexobj(w) else np.float64)
    corr = float(corr)
    if not 0.0 <= corr <= 1.0:
        raise ValueError("corr must lie in [0, 1]")
    s = np.sqrt(1.0 - corr * corr)
    g = np.empty_like(w)
    g[0] = w[0]
    for f in range(1, len(w)):
        g[f] = corr * g[f - 1] + s * w[f]
    return g


def gain_at(w, corr, frame):
    """g_frame of the recursion on ``w[0 .. frame]``."""
    return gains_recursion(np.asarray(w)[:frame + 1], corr)[frame]


def coefficients(corr, frame):
    """The closed form's weights c_0 .. c_frame of w_0 .. w_frame:  c_0 = corr^frame, c_k = sqrt(1 - corr^2) corr^(frame-k)."""
    corr = float(corr)
    c = np.sqrt(1.0 - corr * corr) * corr ** (frame - np.arange(frame + 1, dtype=np.float64))
    c[0] = corr ** float(frame)
    return c


def gains_closed_form(w, corr, frame):
    """g_frame by the closed form, accumulated in ascending k; terms whose coefficient is exactly zero are skipped."""
    w = np.asarray(w)
    acc = np.zeros(w.shape[1:], dtype=np.complex128 if np.iscomplexobj(w) else np.float64)
    for k, c in enumerate(coefficients(corr, frame)):
        if c != 0.0:
            acc = acc + c * w[k]
    return acc
