"""Monte-Carlo sweep runner — the counterpart of plot_errorVSsnr.m:48-180.

Loop structure of the reference: for each sweep point (SNR) and each realisation build the
system (:57-136), call ``proposed_algorithm`` (:137) and ``proposed_algorithm_angles`` (:144),
turn S into the capped spectral NMSE (:138-141,:145-148) and average over realisations (:170).

Here the (sweep point, trial) pairs are flattened, cut into contiguous blocks, one block per
rank (one process per GPU), solved ``batch`` trials at a time, and the per-point NMSE sums are
combined with ONE all-reduce at the end (RCCL over xGMI when the process group is "nccl";
a few hundred bytes, latency-bound).  Random numbers are keyed by (seed, sweep idx, trial idx),
so the result does not depend on the number of ranks.
"""
from __future__ import annotations

import torch

from .system_model import SweepParams, TrainingParams, ase_trials, build_trials, build_trials_training, rank_trials, spectrum_trials

__all__ = ["partition", "run_sweep", "run_points", "sweep_points", "run_approx_sweep", "driver", "run_driver",
           "admmiters_points", "run_convergence_curves", "zy_points", "run_zy", "capacity_points", "capacity_designs",
           "power_model", "run_capacity", "rank_points", "run_rank", "load_channel", "run_tracking"]


def partition(n_items, world, rank):
    """Contiguous block [lo, hi) of rank ``rank`` when n_items are split over ``world`` ranks
    (first n_items % world ranks get one extra item)."""
    q, r = divmod(n_items, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def sweep_points(base: SweepParams, name, values):
    """Sweep points of the sibling drivers: vary one parameter of ``base`` —
    ``snr_db`` (plot_errorVSsnr.m:24,48), ``L`` (plot_errorVSdelays.m:45-51), ``T``
    (plot_errorVSframelength.m:46-51), ``Mr`` (plot_errorVSnrf.m:46), ``Nt`` (plot_errorVSnt.m:46-52),
    ``rays`` (plot_errorVSpaths.m:47-51)."""
    return [base.replace(**{name: v}) for v in values]


def driver(name):
    """The sweep of one of the reference's drivers at ITS OWN parameters: ``dict(points, Imax, numOfnz, n_trials,
    metric, axis, values)`` ready for ``run_points(d["points"], d["n_trials"], Imax=d["Imax"], numOfnz=d["numOfnz"],
    metric=d["metric"], baselines=True)``.  Each driver's construction quirks are kept: beamformer kind, the
    min/max eigenvalue in rho, the (L, T) and (Nt, T) pairs that move together.

    ====================== ======================================= =====================================================
    name                   sweep axis                              cite
    ====================== ======================================= =====================================================
    errorVSsnr             snr_db = -15:3:15                       plot_errorVSsnr.m:8-25,124-130
    errorVSdelays          L = 2,4,6,8,10 with T = 5,10,...,25     plot_errorVSdelays.m:7-21,43-46,122,128
    errorVSframelength     T = 5,15,25,35 (Nt = 8, 'fft')          plot_errorVSframelength.m:7-22,44-46,123,129
    errorVSnrf             Mr = 4,8,12,16 (T = 5)                  plot_errorVSnrf.m:7-22,44-46,122,128
    errorVSnt              Nt = 4,6,8,12,16 with T = 35,..,35,25   plot_errorVSnt.m:7-22,44-48,123,129
    errorVSpaths           rays = 1,3,6,9,12                       plot_errorVSpaths.m:7-23,45,122,128
    rateVSframelength      T = 5,10,15 (Nt = 8, 'fft'), rate       plot_rateVSframelength.m:7-22,44-46,116,122
    errorVSsnr_nyuwireless snr_db = -15:3:15, a SUPPLIED channel   plot_errorVSsnr_nyuwireless.m:9-26,60-69,135-141
    ====================== ======================================= =====================================================

    ``errorVSsnr_nyuwireless`` draws no channel: it loads one (``Hf{l}``, one matrix per delay tap) from a file the reference
    does not ship.  Its dict carries ``needs_channel=True``; pass any channel as ``run_driver(name, channel=H)`` (``load_channel``
    reads one from a file).
    """
    snr = lambda db: dict(snr_db=float(db))
    if name == "errorVSsnr":
        base = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4)
        axis, values, pts = "snr_db", list(range(-15, 16, 3)), None
        cfg = dict(Imax=100, numOfnz=100, n_trials=1, metric="nmse")
    elif name == "errorVSdelays":
        base = SweepParams(Nt=4, Nr=32, L=2, T=5, Mr=4, rho_rule="max", **snr(5))
        axis, values = "L", [2, 4, 6, 8, 10]
        pts = [base.replace(L=L, T=5 * (i + 1)) for i, L in enumerate(values)]
        cfg = dict(Imax=100, numOfnz=50, n_trials=10, metric="nmse")
    elif name == "errorVSframelength":
        base = SweepParams(Nt=8, Nr=32, L=4, T=5, Mr=4, beamformer="fft", **snr(15))
        axis, values, pts = "T", [5, 15, 25, 35], None
        cfg = dict(Imax=100, numOfnz=50, n_trials=1, metric="nmse")
    elif name == "errorVSnrf":
        base = SweepParams(Nt=4, Nr=32, L=4, T=5, Mr=4, rho_rule="max", **snr(5))
        axis, values, pts = "Mr", [4, 8, 12, 16], None
        cfg = dict(Imax=100, numOfnz=100, n_trials=50, metric="nmse")
    elif name == "errorVSnt":
        base = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, beamformer="fft", rho_rule="max", **snr(15))
        axis, values = "Nt", [4, 6, 8, 12, 16]
        pts = [base.replace(Nt=nt, T=t) for nt, t in zip(values, [35, 35, 35, 35, 25])]
        cfg = dict(Imax=100, numOfnz=50, n_trials=50, metric="nmse")
    elif name == "errorVSpaths":
        base = SweepParams(Nt=4, Nr=32, L=4, T=35, Mr=4, rho_rule="max", **snr(5))
        axis, values, pts = "rays", [1, 3, 6, 9, 12], None
        cfg = dict(Imax=100, numOfnz=100, n_trials=1, metric="nmse")
    elif name == "rateVSframelength":
        base = SweepParams(Nt=8, Nr=32, L=4, T=5, Mr=4, beamformer="fft", **snr(15))
        axis, values, pts = "T", [5, 10, 15], None
        cfg = dict(Imax=100, numOfnz=50, n_trials=1, metric="rate")
    elif name == "errorVSsnr_nyuwireless":
        base = SweepParams(Nt=4, Nr=32, L=4, T=25, Mr=4, Mr_e=32)
        axis, values, pts = "snr_db", list(range(-15, 16, 3)), None
        cfg = dict(Imax=100, numOfnz=250, n_trials=50, metric="nmse", needs_channel=True)
    else:
        raise ValueError("unknown driver %r" % (name,))
    cfg.update(points=pts if pts is not None else sweep_points(base, axis, values), axis=axis, values=values)
    return cfg


def run_driver(name, n_trials=None, **kw):
    """``run_points`` on the preset of ``driver(name)`` (all seven columns' worth of baselines unless overridden);
    ``n_trials`` defaults to the driver's own maxMCRealizations."""
    d = driver(name)
    if d.get("needs_channel") and kw.get("channel") is None:
        raise ValueError("driver %r draws no channel: pass one as run_driver(%r, channel=H) with H of shape (Nr_src, Nt_src, L) "
                         "(load_channel(path) reads .npy / .npz / .mat; tools/run_driver.py takes --channel FILE)" % (name, name))
    kw.setdefault("baselines", True)
    return run_points(d["points"], d["n_trials"] if n_trials is None else n_trials, Imax=d["Imax"], numOfnz=d["numOfnz"],
                      metric=d["metric"], **kw)


def load_channel(path):
    """A channel for ``build_trials(..., channel=)`` from a file: ``.npy``, or ``.npz`` with key ``Hf`` or ``H``, holding an
    array ``(Nr_src, Nt_src, L)``; or a ``.mat`` file with the cell array ``Hf`` of the reference's own file (``Hf{l}``, one
    matrix per delay tap, plot_errorVSsnr_nyuwireless.m:6,63) or a 3-D array ``Hf`` / ``H``, through ``scipy.io.loadmat``
    (scipy is imported only then).  Returns a complex numpy array ``(Nr_src, Nt_src, L)``."""
    import numpy as np
    ext = str(path).lower().rsplit(".", 1)[-1]
    if ext == "npy":
        H = np.load(path, allow_pickle=False)
    elif ext == "npz":
        with np.load(path, allow_pickle=False) as z:
            keys = [k for k in ("Hf", "H") if k in z.files]
            if not keys:
                raise ValueError("%s holds %s, neither 'Hf' nor 'H'" % (path, sorted(z.files)))
            H = z[keys[0]]
    elif ext == "mat":
        with open(path, "rb") as f:
            head = f.read(128)
        if head[:8] == b"\x89HDF\r\n\x1a\n" or b"MATLAB 7.3" in head:
            raise ValueError("%s is a MATLAB v7.3 (HDF5) file, which scipy.io.loadmat does not read: save it again with "
                             "save(..., '-v7'), or convert it to .npy" % (path,))
        try:
            from scipy.io import loadmat
        except ImportError as e:
            raise ImportError("reading %s needs scipy (scipy.io.loadmat), which is not installed: convert the channel to "
                              ".npy, an array (Nr_src, Nt_src, L)" % (path,)) from e
        m = loadmat(path)
        keys = [k for k in ("Hf", "H") if k in m]
        if not keys:
            raise ValueError("%s holds %s, neither 'Hf' nor 'H'" % (path, sorted(k for k in m if not k.startswith("__"))))
        H = m[keys[0]]
        if H.dtype == object:                                   # the cell array Hf{l}
            taps = [np.asarray(t) for t in H.reshape(-1)]
            if len({t.shape for t in taps}) != 1 or taps[0].ndim != 2:
                raise ValueError("the cells of %s in %s are not matrices of one size" % (keys[0], path))
            H = np.stack(taps, axis=2)
    else:
        raise ValueError("channel file %s: expected .npy, .npz or .mat" % (path,))
    H = np.asarray(H)
    if H.ndim == 2:
        H = H[:, :, None]
    if H.ndim != 3:
        raise ValueError("the channel in %s has shape %r, expected (Nr_src, Nt_src, L)" % (path, H.shape))
    return H.astype(np.complex128 if H.dtype != np.complex64 else np.complex64, copy=False)


def _score(S, zb, metric, noise_var):
    """Per-trial figure of merit: capped spectral NMSE (plot_errorVSsnr.m:138-141) or the rate of
    plot_rateVSframelength.m:81,113,130,135."""
    from . import solvers as J
    return J.nmse_spectral(S, zb) if metric == "nmse" else J.rate(S, zb, noise_var)


def _eye(n, like):
    from .solvers import colmajor
    return colmajor(torch.eye(n, dtype=torch.complex64, device=like.device))


def _times_h(Y, B):
    """``Y*B'`` (plot_errorVSsnr.m:80; also ``B*B'`` of :79 with Y = B) on the library's correlation kernel:
    ``jstsp_correlate_c32`` computes ``A'*K*B'``, here with A = I."""
    from . import solvers as J
    return J.correlate(Y, _eye(Y.shape[-2], Y), B)


def _times(A, S, P):
    """``A*S*P`` (``Y*pinv(B)`` of plot_errorVSsnr.m:117 with A = I; ``A*S_ls``; ``A'*Y*pinv(B)`` of plot_errorVSzy.m:73) on the
    library's synthesis kernel (``jstsp_synthesize_c32``).  ``A`` None = identity."""
    from . import solvers as J
    return J.synthesize(S, _eye(S.shape[-2], S) if A is None else A, P)


def _hip_baselines(inp, numOfnz, metric="nmse", noise_var=1.0, tssr=None, vamp_max_order=128, ls_precision="f32",
                   mmv_precision="f32", score="host"):
    """LS, VAMP and MMV-OMP baselines of plot_errorVSsnr.m:73-121 on the conventional-HBF measurement; with
    ``tssr = (Imax, rho)`` also the commented TSSR recipe (:151,158-162) on the proposed scheme's measurement.
    Every product goes through the library (correlate / synthesize entry points), nothing through torch matmuls.

    LS of a factor too large for the float64 pinv kernel takes the fp32 Gram-inverse route, whose accuracy is
    ``6e-8 * cond(B B')``; the library records the conditioning on the device (``jstsp_last_conditioning``).  Where that
    record says the digits are not there (``lambda_min/lambda_max < 1e-6``, or 0: a truncated or unconverged inverse) the LS
    column - and the MMV-OMP column when it had to be built from that LS estimate - is NaN instead of a wrong number.

    ``ls_precision="f64"`` (opt-in; the default "f32" is the behaviour above, unchanged): ``pinv(B)``, ``S_ls`` and
    ``Y*pinv(B)`` come from the float64 entries (``jstsp_pinv_f64`` / ``jstsp_ls_f64``: SVD-based, no Gram matrix, any
    factor up to 512 x 8192), the LS column is scored in float64 (``_score_f64``), and the LS and MMV-OMP columns are
    numbers where the default gives NaN.  With ``mmv_precision="f32"`` the joint OMP itself stays the fp32 kernel (its input is
    narrowed).

    ``mmv_precision="f64"`` (opt-in, independent of ``ls_precision``): the MMV-OMP column is
    ``mmv_omp_f64(A_hbf, Y_hbf*pinv_f64(B_hbf), numOfnz)`` and the TSSR / SVT-based columns come from ``tssr_f64`` - float64
    matrix completion, pinv, products and joint OMP (``jstsp_mc_svt_f64``, ``jstsp_mmv_omp_f64``), at every driver size -
    and all three are scored in float64 (``_score_f64``).  The default "f32" leaves every column as it was.

    ``score="device"`` (opt-in; the default "host" is ``_score_f64``, unchanged): the columns ``_score_f64`` scores are scored
    by ``nmse_spectral_f64`` / ``rate_f64`` on the device instead (``_score_f64_device``: float64 singular values, no Gram
    matrix; only one double per trial crosses the bus).  The fp32 columns keep ``_score``."""
    from . import _lib
    from . import solvers as J
    _check_precisions(ls_precision, mmv_precision)
    _check_score(score)
    zb = J.colmajor(inp["Zbar"].to(torch.complex64))
    ctx = _lib.default_context(inp["Y_hbf"].device.index or 0)
    nan = lambda: torch.full((inp["Y_hbf"].shape[0],), float("nan"), dtype=torch.float64)
    Bh = inp["B_hbf"]
    G2 = Bh.shape[1]
    if ls_precision == "f64":
        return _hip_baselines_f64(inp, numOfnz, metric, noise_var, tssr, vamp_max_order, mmv_precision, score)
    try:
        PB = J.pinv(Bh)                                                                  # pinv(B)  :83, :117
    except J.JstspError as e:
        if e.code != _lib.E_UNSUPPORTED:                                                 # (too large for the in-LDS kernel)
            raise
        PB = None
    S_ls = J.ls_estimate(inp["Y_hbf"], inp["A_hbf"], Bh)                                 # :83
    ls_ok = True
    if PB is None:                                                                       # the Gram-inverse route ran for B
        rcond, _ = ctx.last_conditioning()
        ls_ok = rcond * rcond >= 1e-6
    out = {"ls": _score(S_ls, zb, metric, noise_var) if ls_ok else nan()}
    if G2 <= vamp_max_order and inp["A_hbf"].shape[0] <= 128:       # (orders above 128: one block-Jacobi decomposition of that order per trial)
        Gb = _times_h(Bh, Bh)                                                            # (B*B')  :79
        Ym = _times_h(inp["Y_hbf"], Bh)                                                  # Y_hbf*B' :80
        out["vamp"] = _score(J.vamp_kron(Ym, inp["A_hbf"], Gb, 1.0, numOfnz), zb, metric, noise_var)   # :100
    if mmv_precision == "f64":
        out.update(_mmv_columns_f64(inp, numOfnz, metric, noise_var, tssr, score=score))
        return out
    Ypb = None
    if PB is not None:
        Ypb = _times(None, inp["Y_hbf"], PB)                                             # Y_hbf_nr*pinv(B)  :117
    elif inp["A_hbf"].shape[0] == inp["A_hbf"].shape[1] and ls_ok:
        # B too large for the pinv kernel, A square: Y*pinv(B) = A*(pinv(A)*Y*pinv(B)) = A*S_ls (A invertible: a unitary
        # dictionary times the beamformer), with the Gram-inverse route of jstsp_ls_c32 behind S_ls
        Ypb = _times(inp["A_hbf"], S_ls, _eye(G2, S_ls))
    if Ypb is not None:
        Z, _, _ = J.mmv_omp(inp["A_hbf"], Ypb, numOfnz)                                  # :116-117
        out["omp_mmv"] = _score(Z, zb, metric, noise_var)
    elif not ls_ok:
        out["omp_mmv"] = nan()
    if tssr is not None:
        try:
            St, _, Ssvt = J.tssr(inp["subY"], inp["Omega"], inp["A"], inp["B"], tssr[0], inp["tau_Y"].numpy(), tssr[1],
                                 2 * numOfnz)                                            # :151,:160-161
            out["tssr"] = _score(St, zb, metric, noise_var)
            out["svt"] = _score(Ssvt, zb, metric, noise_var)                             # :152-153
        except J.JstspError as e:
            if e.code != _lib.E_UNSUPPORTED:
                raise
    return out


def _score_f64(S, zb, metric, noise_var):
    """``_score`` for a float64 estimate: the same two formulas (plot_errorVSsnr.m:138-141, plot_rateVSframelength.m:81)
    evaluated in float64 on the host - the library's scoring kernels store fp32, which would put back the rounding that the
    float64 least squares removes.  ``S``, ``zb``: (batch, R, C) tensors; returns a float64 tensor (batch,)."""
    import numpy as np
    Sh, zh = S.detach().cpu().numpy().astype(np.complex128), zb.detach().cpu().numpy().astype(np.complex128)
    out = np.empty(Sh.shape[0], dtype=np.float64)
    for t in range(Sh.shape[0]):
        e = (np.linalg.norm(Sh[t] - zh[t], 2) / np.linalg.norm(zh[t], 2)) ** 2
        if metric == "nmse":
            out[t] = min(1.0, e) if e == e else e
        else:
            nr = zh.shape[1]
            out[t] = np.log2(np.real(np.linalg.det(np.eye(nr) + zh[t] @ zh[t].conj().T / nr / (noise_var + e))))
    return torch.from_numpy(out)


def _score_f64_device(S, zb, metric, noise_var):
    """``_score_f64`` on the device (``score="device"``): the same two formulas by ``nmse_spectral_f64`` / ``rate_f64`` - float64
    singular values of ``S - Zbar`` and ``Zbar`` themselves, nothing narrowed, no Gram matrix.  ``S``: (batch, R, C) complex128,
    ``zb`` complex64 or complex128 (widened on the device), CUDA tensors as the solvers and ``build_trials`` leave them.
    Returns what ``_score_f64`` returns: a float64 CPU tensor (batch,)."""
    from . import solvers as J
    S, zb = J.colmajor(S.detach().to(torch.complex128)), J.colmajor(zb.detach())
    out = J.nmse_spectral_f64(S, zb) if metric == "nmse" else J.rate_f64(S, zb, noise_var)
    return out.cpu()


def _scorer_f64(score):
    return _score_f64_device if score == "device" else _score_f64


def _check_score(score):
    if score not in ("host", "device"):
        raise ValueError("score must be 'host' or 'device'")


def _check_precisions(ls_precision, mmv_precision):
    if ls_precision not in ("f32", "f64"):
        raise ValueError("ls_precision must be 'f32' or 'f64'")
    if mmv_precision not in ("f32", "f64"):
        raise ValueError("mmv_precision must be 'f32' or 'f64'")


def _mmv_columns_f64(inp, numOfnz, metric, noise_var, tssr, PB=None, score="host"):
    """The MMV-OMP column and, with ``tssr = (Imax, rho)``, the TSSR and SVT-based columns in float64
    (``mmv_precision="f64"``); ``PB``: ``pinv_f64(B_hbf)`` where the caller has it; ``score``: see ``_hip_baselines``."""
    from . import solvers as J
    score_f64 = _scorer_f64(score)
    wide = lambda x: x.to(torch.complex128)
    Bh, Ah, Yh = inp["B_hbf"], inp["A_hbf"], inp["Y_hbf"]
    if PB is None:
        PB = J.pinv_f64(wide(Bh))                                                        # pinv(B)  :117
    eye = J.colmajor(torch.eye(Yh.shape[-2], dtype=torch.complex128, device=Yh.device))
    Z, _, _ = J.mmv_omp_f64(wide(Ah), J.synthesize_f64(wide(Yh), eye, PB), numOfnz)      # :116-117
    out = {"omp_mmv": score_f64(Z, inp["Zbar"], metric, noise_var)}
    if tssr is not None:
        St, _, Ssvt = J.tssr_f64(inp["subY"], inp["Omega"], inp["A"], inp["B"], tssr[0], inp["tau_Y"].numpy(), tssr[1],
                                 2 * numOfnz)                                            # :151,:160-161
        out["tssr"] = score_f64(St, inp["Zbar"], metric, noise_var)
        out["svt"] = score_f64(Ssvt, inp["Zbar"], metric, noise_var)                    # :152-153
    return out


def _hip_baselines_f64(inp, numOfnz, metric, noise_var, tssr, vamp_max_order, mmv_precision="f32", score="host"):
    """``_hip_baselines`` with the least-squares pieces in float64 (``ls_precision="f64"``)."""
    from . import solvers as J
    score_f64 = _scorer_f64(score)
    zb = J.colmajor(inp["Zbar"].to(torch.complex64))
    Bh, Ah, Yh = inp["B_hbf"], inp["A_hbf"], inp["Y_hbf"]
    G2 = Bh.shape[1]
    wide = lambda x: x.to(torch.complex128)
    PB = J.pinv_f64(wide(Bh))                                                            # pinv(B)  :83, :117
    S_ls = J.ls_estimate_f64(wide(Yh), wide(Ah), wide(Bh))                               # :83
    out = {"ls": score_f64(S_ls, inp["Zbar"], metric, noise_var)}
    if G2 <= vamp_max_order and Ah.shape[0] <= 128:
        Gb = _times_h(Bh, Bh)                                                            # (B*B')  :79
        Ym = _times_h(Yh, Bh)                                                            # Y_hbf*B' :80
        out["vamp"] = _score(J.vamp_kron(Ym, Ah, Gb, 1.0, numOfnz), zb, metric, noise_var)   # :100
    if mmv_precision == "f64":
        out.update(_mmv_columns_f64(inp, numOfnz, metric, noise_var, tssr, PB, score))
        return out
    eye = J.colmajor(torch.eye(Yh.shape[-2], dtype=torch.complex128, device=Yh.device))
    Ypb = J.synthesize_f64(wide(Yh), eye, PB).to(torch.complex64)                        # Y_hbf_nr*pinv(B)  :117
    Z, _, _ = J.mmv_omp(Ah, Ypb, numOfnz)                                                # :116-117
    out["omp_mmv"] = _score(Z, zb, metric, noise_var)
    if tssr is not None:
        try:
            St, _, Ssvt = J.tssr(inp["subY"], inp["Omega"], inp["A"], inp["B"], tssr[0], inp["tau_Y"].numpy(), tssr[1],
                                 2 * numOfnz)                                            # :151,:160-161
            out["tssr"] = _score(St, zb, metric, noise_var)
            out["svt"] = _score(Ssvt, zb, metric, noise_var)                             # :152-153
        except J.JstspError as e:
            from . import _lib
            if e.code != _lib.E_UNSUPPORTED:
                raise
    return out


def _hip_solvers(device, metric="nmse"):
    """Default solver pair: the HIP path.  Raises if the library / GPU is missing."""
    from . import solvers as J

    def solve(inp, Imax, noise_var=1.0):
        S, _, _ = J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], inp["B"], Imax, inp["tau_Y"].numpy(),
                                       inp["tau_Z"].numpy(), inp["rho"].numpy(), "approximate", want_ce=False)
        Sa, _, _ = J.proposed_algorithm_angles(inp["subY"], inp["Omega"], inp["indx_S"], inp["A"], inp["B"], Imax,
                                               inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy(),
                                               "approximate", None, want_ce=False)
        zb = J.colmajor(inp["Zbar"].to(torch.complex64))
        return _score(S, zb, metric, noise_var), _score(Sa, zb, metric, noise_var)

    return solve


def _resolve_builder(builder, device=None):
    """None / "hip": the library's own input kernels; otherwise a callable hook (see ``run_points``)."""
    if builder is None or builder == "hip":
        if device is not None and torch.device(device).type != "cuda":
            raise ValueError("builder=None / 'hip' builds the inputs with the library's kernels and needs a CUDA (ROCm) device; on "
                             "device=%r pass a callable builder (the CPU-side tests use tests/torch_builder.py: builder)" % (device,))
        return "hip"
    if not callable(builder):
        raise ValueError("builder must be None, 'hip' or a callable (p, trial_ids, seed, sweep_idx, device, with_hbf) -> inputs "
                         "(the torch tensor-op builder of rounds 1-3 is tests/torch_builder.py: builder)")
    return builder


def _merge_key(p):
    """Sweep points whose trials may share one solver call: same array shapes and the same trial-independent A (the
    SNR, the number of paths and the rho rule only enter the per-trial arrays, which are built per point)."""
    return (p.Nt, p.Nr, p.L, p.T, p.Mr, p.Mr_e, p.Gr, p.Gt, p.beamformer, p.T_prop)


def _merge_inputs(inps):
    """Concatenate the per-trial arrays of several ``build_trials`` results (column-major layout kept)."""
    if len(inps) == 1:
        return inps[0]
    out = {}
    for k, v0 in inps[0].items():
        if k in ("A", "A_hbf"):                          # trial-independent: beamformer x dictionary
            out[k] = v0
        elif v0.is_cuda and v0.ndim == 3:
            out[k] = torch.cat([x[k].transpose(1, 2) for x in inps], 0).transpose(1, 2)
        else:
            out[k] = torch.cat([x[k] for x in inps], 0)
    return out


def _merge_cap(p, batch, with_hbf):
    """Trials per merged solver call: small problems are latency-bound per launch (one workgroup per matrix in the
    eigen-decompositions), so trials of several sweep points go into one call - up to about 1.5 GB of inputs."""
    N, M, Gr, G2 = p.solver_shape
    per_trial = 8 * (G2 * M + 2 * N * M + 2 * Gr * G2 + ((G2 + p.Nr) * p.T_hbf if with_hbf else 0))
    return max(batch, min(4096, int(1.5e9 // max(per_trial, 1))))


def run_points(points, n_trials, *, Imax=100, batch=64, seed=20190913, device=None, solve_fn=None, dist=None,
               baselines=False, numOfnz=100, builder=None, metric="nmse", tssr=None, merge=True, vamp_max_order=128,
               samples=None, ls_precision="f32", mmv_precision="f32", channel=None, channel_normalize="reference", score="host"):
    """Mean capped NMSE per sweep point; columns (proposed_algorithm, proposed_algorithm_angles[, LS, VAMP, MMV-OMP
    [, TSSR]]).  ``metric="rate"``: the rate of plot_rateVSframelength.m:81 instead of the NMSE (HIP solvers only).
    ``tssr=(Imax_svt, rho_svt)`` adds the commented recipes of plot_errorVSsnr.m:151-162 as columns six and seven: TSSR
    (``mc_svt`` then joint OMP) and "SVT-based" (``pinv(A)*Y_svt*pinv(B)``).

    ``solve_fn(inputs, Imax) -> (nmse, nmse_angles)`` (two tensors of per-trial NMSE) defaults to the HIP path.
    ``baselines=True`` adds the LS and VAMP columns of plot_errorVSsnr.m:83-105 (HIP path only; VAMP is NaN
    where the delay factor's order L*Gt exceeds ``vamp_max_order`` - 128 by default: above that every trial costs one
    block-Jacobi eigen-decomposition of that order, csrc/eig_large.hip).  ``dist``: ``torch.distributed`` (initialised) or None.
    ``builder``: None / "hip" — inputs from the library's own kernels (``jstsp_build_trials_c32``) — or a callable
    ``builder(p, trial_ids, seed, sweep_idx, device, with_hbf) -> inputs`` (the CPU-side tests pass the torch tensor-op
    builder of tests/torch_builder.py, which runs without a GPU; it has its own random streams, so its curves agree with
    the library builder's statistically, not sample by sample).
    ``samples``: a list that receives, per sweep point, a float64 tensor (trials of THIS rank, ncol) of the per-trial values
    before averaging (what plot_errorVSsnr.m:138-141 computes per realisation) - for distributional checks.
    ``ls_precision="f64"``: the LS column, and the ``Y*pinv(B)`` in front of the MMV-OMP column, from the float64
    least-squares entries (see ``_hip_baselines``); the default "f32" leaves every column as it was.
    ``mmv_precision="f64"``: the MMV-OMP, TSSR and SVT-based columns from the float64 entries (``mmv_omp_f64``, ``tssr_f64``),
    scored in float64 - numbers also where the fp32 chain refuses the size of ``B``; the default "f32" changes nothing.
    ``channel``, ``channel_normalize``: handed to ``build_trials`` - a supplied channel instead of the drawn one, shared
    ``(Nr_src, Nt_src, L)`` or one per trial ``(n_trials, Nr_src, Nt_src, L)`` (the same n_trials channels at every sweep
    point); library builder only.
    ``score="device"``: the float64 columns of the baselines are scored on the device (``nmse_spectral_f64`` / ``rate_f64``)
    instead of by ``_score_f64`` on the host; the default "host" changes nothing (see ``_hip_baselines``).
    Returns a float64 tensor (len(points), ncol) identical on every rank.
    """
    _check_precisions(ls_precision, mmv_precision)
    _check_score(score)
    if channel is not None:
        if builder is not None and builder != "hip":
            raise ValueError("channel= goes to the library's builder; a callable builder makes its own channel")
        if len(channel.shape) == 4 and channel.shape[0] != n_trials:
            raise ValueError("a per-trial channel needs n_trials = %d channels, not %d" % (n_trials, channel.shape[0]))
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    builder = _resolve_builder(builder, device)
    if metric not in ("nmse", "rate"):
        raise ValueError("metric must be 'nmse' or 'rate'")
    custom = solve_fn is not None
    if custom and metric != "nmse":
        raise ValueError("metric='rate' needs the HIP solvers (solve_fn=None)")
    if solve_fn is None:
        solve_fn = _hip_solvers(device, metric)
    n_pts = len(points)
    ncol = (7 if tssr is not None else 5) if baselines else 2
    lo, hi = partition(n_pts * n_trials, world, rank)
    acc = torch.zeros((n_pts, ncol + 1), dtype=torch.float64)   # sums per column, then the trial count
    # HIP path, NMSE metric: chunks of consecutive sweep points with equal shapes are solved in ONE call (the per-trial
    # results do not depend on what else is in the batch; a rate sweep keeps one noise variance per call)
    merging = merge and not custom and builder == "hip" and metric == "nmse"
    item = lo
    while item < hi:
        chunks, inps, total = [], [], 0
        while item < hi:
            pt = item // n_trials
            t0 = item % n_trials
            t1 = min(n_trials, t0 + batch, t0 + (hi - item))
            p = points[pt]
            if chunks and (not merging or _merge_key(p) != _merge_key(points[chunks[0][0]])
                           or total + (t1 - t0) > _merge_cap(p, batch, baselines)):
                break
            if builder == "hip":
                if channel is None:
                    inps.append(build_trials(p, t0, t1 - t0, seed=seed, sweep_idx=pt, device=device, with_hbf=baselines))
                else:
                    inps.append(build_trials(p, t0, t1 - t0, seed=seed, sweep_idx=pt, device=device, with_hbf=baselines,
                                             channel=channel if len(channel.shape) == 3 else channel[t0:t1],
                                             channel_normalize=channel_normalize))
            else:
                inps.append(builder(p, range(t0, t1), seed, pt, device, baselines))
            chunks.append((pt, t1 - t0))
            total += t1 - t0
            item += t1 - t0
        inp = _merge_inputs(inps)
        del inps
        p = points[chunks[0][0]]
        e, ea = solve_fn(inp, Imax) if custom else solve_fn(inp, Imax, p.noise_var)
        cols = [torch.as_tensor(e).double().cpu(), torch.as_tensor(ea).double().cpu()]
        if baselines:
            b = _hip_baselines(inp, numOfnz, metric, p.noise_var, tssr, vamp_max_order, ls_precision, mmv_precision, score)
            for key in ("ls", "vamp", "omp_mmv", "tssr", "svt")[:ncol - 2]:
                cols.append(b[key].double().cpu() if key in b else torch.full((total,), float("nan"), dtype=torch.float64))
        o = 0
        for pt, cnt in chunks:
            for col, v in enumerate(cols):
                acc[pt, col] += float(v[o:o + cnt].sum())
            acc[pt, ncol] += cnt
            if samples is not None:
                while len(samples) < n_pts:
                    samples.append(torch.zeros((0, ncol), dtype=torch.float64))
                samples[pt] = torch.cat([samples[pt], torch.stack([v[o:o + cnt] for v in cols], dim=1)], 0)
            o += cnt
    if dist is not None:
        buf = acc.to(device) if dist.get_backend() == "nccl" else acc
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)       # the single collective of the sweep
        acc = buf.cpu()
    return acc[:, :ncol] / acc[:, ncol:ncol + 1]         # plot_errorVSsnr.m:170-171


def run_sweep(base: SweepParams, snr_db_list, n_trials, **kw):
    """The SNR sweep of plot_errorVSsnr.m:48-180 (see ``run_points``)."""
    return run_points(sweep_points(base, "snr_db", [float(s) for s in snr_db_list]), n_trials, **kw)


def _hip_alg12(inp, Imax):
    """plot_errorVSsnr_approx.m:60-72 on the HIP path: Alg.1 ('std') and Alg.2 ('approximate'), each scored
    through its completed measurement, ``S = pinv(A)*Y*pinv(B)``."""
    from . import solvers as J
    zb = J.colmajor(inp["Zbar"].to(torch.complex64))
    out = []
    for kind in ("std", "approximate"):
        _, Y, _ = J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], inp["B"], Imax, inp["tau_X"].numpy(),
                                       inp["tau_S"].numpy(), inp["rho"].numpy(), kind, want_ce=False)   # :60,:67
        out.append(J.nmse_spectral(J.ls_estimate(Y, inp["A"], inp["B"]), zb))                            # :61-65
    return out


def _hip_alg12_f64(inp, Imax_list, score="host", resume=False):
    """``_hip_alg12`` in float64 for every Imax of the list on ONE batch of trials: ``pinv_f64(A)`` and ``pinv_f64(B)`` are
    computed once and serve the least-squares step of every Alg. 1 solve (``proposed_algorithm_std_f64(..., PA=, PB=)``) and
    the scoring product ``pinv(A)*Y*pinv(B)`` of both columns (on the f64 matrix pipe: ``correlate_f64`` with the adjoints of
    the factors).  Alg. 2 is ``proposed_algorithm_f64``; the columns are scored by ``_score_f64``.  Returns one
    ``(e_std, e_approx)`` per Imax.  ``score="device"``: scored by ``nmse_spectral_f64`` on the device instead.
    ``resume=True``: one solve per algorithm instead of one per Imax - the list is stepped through in ascending order with the
    ADMM state carried (``proposed_algorithm_resume_f64`` / ``proposed_algorithm_std_resume_f64``; 10 / 30 / 50 is 10, then
    20 more, then 20 more: 50 iterations instead of 90).  The float64 solver carries nothing but that state, so the columns
    are those of ``resume=False`` bit for bit."""
    from . import solvers as J
    _check_score(score)
    score_f64 = _scorer_f64(score)
    wide = lambda x: J.colmajor(x.to(torch.complex128))
    subY, A, B, zb = wide(inp["subY"]), wide(inp["A"]), wide(inp["B"]), wide(inp["Zbar"])
    Om = J.colmajor(inp["Omega"].to(torch.float64))
    prm = (inp["tau_X"].numpy(), inp["tau_S"].numpy(), inp["rho"].numpy())
    PA, PB = J.pinv_f64(A), J.pinv_f64(B)
    PAh, PBh = J.colmajor(PA.mH), J.colmajor(PB.mH)
    if resume:
        out, it0, st1, st2, e = [None] * len(Imax_list), 0, None, None, None
        for k in sorted(range(len(Imax_list)), key=lambda k: int(Imax_list[k])):
            more = int(Imax_list[k]) - it0
            if more > 0:                                    # (an Imax listed twice is scored once)
                _, Y1, _, st1 = J.proposed_algorithm_std_resume_f64(subY, Om, A, B, more, *prm, PA=PA, PB=PB, want_ce=False, state=st1, it0=it0)
                _, Y2, _, st2 = J.proposed_algorithm_resume_f64(subY, Om, A, B, more, *prm, want_ce=False, state=st2, it0=it0)
                e = tuple(score_f64(J.correlate_f64(Y, PAh, PBh), zb, "nmse", 0.0) for Y in (Y1, Y2))
                it0 += more
            out[k] = e
        return out
    out = []
    for Imax in Imax_list:
        _, Y1, _ = J.proposed_algorithm_std_f64(subY, Om, A, B, int(Imax), *prm, PA=PA, PB=PB, want_ce=False)     # :60
        _, Y2, _ = J.proposed_algorithm_f64(subY, Om, A, B, int(Imax), *prm, "approximate", want_ce=False)        # :67
        out.append(tuple(score_f64(J.correlate_f64(Y, PAh, PBh), zb, "nmse", 0.0) for Y in (Y1, Y2)))           # :61-65, :68-72
    return out


def _run_approx_sweep_f64(base, snr_db_list, Imax_list, n_trials, *, batch, seed, device, dist, builder, score="host", resume=False):
    """``run_approx_sweep(precision="f64")``: the (SNR, trial) pairs are sharded over ranks; a batch of trials is built once and
    solved for every Imax (its Philox key is the sweep index of the point (SNR, Imax_list[0]) of the default sweep, so that
    column sees the realisations the fp32 sweep sees)."""
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1
    nI = len(Imax_list)
    lo, hi = partition(len(snr_db_list) * n_trials, world, rank)
    acc = torch.zeros((len(snr_db_list), nI, 3), dtype=torch.float64)
    item = lo
    while item < hi:
        si = item // n_trials
        t0 = item % n_trials
        t1 = min(n_trials, t0 + batch, t0 + (hi - item))
        p = TrainingParams(base.Nt, base.Nr, base.L, base.T, base.ratio, base.clusters, base.rays, float(snr_db_list[si]))
        if builder == "hip":
            inp = build_trials_training(p, t0, t1 - t0, seed=seed, sweep_idx=si * nI, device=device)
        else:
            inp = builder(p, range(t0, t1), seed, si * nI, device, False)
        for ii, (e1, e2) in enumerate(_hip_alg12_f64(inp, Imax_list, score, resume)):
            acc[si, ii, 0] += float(e1.sum())
            acc[si, ii, 1] += float(e2.sum())
            acc[si, ii, 2] += t1 - t0
        item += t1 - t0
    if dist is not None:
        buf = acc.to(device) if dist.get_backend() == "nccl" else acc
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        acc = buf.cpu()
    mean = torch.clamp(acc[..., :2] / acc[..., 2:3], max=1.0)                              # :76-77
    return mean.transpose(0, 1).contiguous()


def run_approx_sweep(base: TrainingParams, snr_db_list, Imax_list, n_trials, *, batch=64, seed=20190913, device=None,
                     solve_fn=None, dist=None, builder=None, precision="f32", score="host", resume=False):
    """The Alg.1-vs-Alg.2 sweep of plot_errorVSsnr_approx.m:34-85: for each SNR and each Imax, ``n_trials`` fresh
    realisations of wideband_hybBF_comm_system_training, both solver variants, capped NMSE of
    ``pinv(A)*Y*pinv(B)``, mean then ``min(., 1)`` (:76-77).

    Returns a float64 tensor (len(Imax_list), len(snr_db_list), 2) — ``[..., 0]`` is mean_error_proposed,
    ``[..., 1]`` mean_error_proposed_approx — identical on every rank.  ``solve_fn(inputs, Imax) -> (e_std, e_approx)``
    defaults to the HIP path; the (sweep point, trial) pairs are sharded over ranks as in ``run_points``.
    ``builder``: None / "hip" - the inputs from the library's own kernels (``jstsp_build_trials_c32`` with the training model
    fields) - or a callable hook as in ``run_points``.
    ``precision="f64"`` (opt-in; the default "f32" is the behaviour above, unchanged): both columns evaluated and scored in
    float64 - Alg. 1 by ``proposed_algorithm_std_f64``, Alg. 2 by ``proposed_algorithm_f64``, ``_score_f64``.  The reference
    draws fresh realisations for every (SNR, Imax) point; here a batch of trials is built once per SNR and solved for every
    Imax of the list, so that ``pinv_f64(A)`` and ``pinv_f64(B)`` are computed once per batch (``_hip_alg12_f64``).  No
    ``solve_fn`` hook.  ``score="device"`` scores the float64 columns on the device (``nmse_spectral_f64``) instead of by
    ``_score_f64`` on the host; it changes nothing at ``precision="f32"``.
    ``resume=True`` (opt-in, ``precision="f64"`` only): each batch is solved once per algorithm, stepping through the sorted
    ``Imax_list`` with the ADMM state carried, instead of once per Imax from zero; the result is that of ``resume=False`` bit
    for bit (``_hip_alg12_f64``).
    """
    if precision not in ("f32", "f64"):
        raise ValueError("precision must be 'f32' or 'f64'")
    if resume and precision != "f64":
        raise ValueError("resume=True steps the float64 solvers through Imax_list: it needs precision='f64'")
    _check_score(score)
    if precision == "f64" and solve_fn is not None:
        raise ValueError("precision='f64' solves with the library's float64 entries: no solve_fn")
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    builder = _resolve_builder(builder, device)
    if precision == "f64":
        return _run_approx_sweep_f64(base, snr_db_list, Imax_list, n_trials, batch=batch, seed=seed, device=device, dist=dist,
                                     builder=builder, score=score, resume=resume)
    if solve_fn is None:
        solve_fn = _hip_alg12
    pts = [(si, ii) for si in range(len(snr_db_list)) for ii in range(len(Imax_list))]    # loop order of :34-38
    lo, hi = partition(len(pts) * n_trials, world, rank)
    acc = torch.zeros((len(pts), 3), dtype=torch.float64)
    item = lo
    while item < hi:
        pt = item // n_trials
        t0 = item % n_trials
        t1 = min(n_trials, t0 + batch, t0 + (hi - item))
        si, ii = pts[pt]
        p = TrainingParams(base.Nt, base.Nr, base.L, base.T, base.ratio, base.clusters, base.rays, float(snr_db_list[si]))
        if builder == "hip":
            inp = build_trials_training(p, t0, t1 - t0, seed=seed, sweep_idx=pt, device=device)
        else:
            inp = builder(p, range(t0, t1), seed, pt, device, False)
        e1, e2 = solve_fn(inp, int(Imax_list[ii]))
        acc[pt, 0] += float(torch.as_tensor(e1).double().sum())
        acc[pt, 1] += float(torch.as_tensor(e2).double().sum())
        acc[pt, 2] += t1 - t0
        item += t1 - t0
    if dist is not None:
        buf = acc.to(device) if dist.get_backend() == "nccl" else acc
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        acc = buf.cpu()
    mean = torch.clamp(acc[:, :2] / acc[:, 2:3], max=1.0)                                  # :76-77
    return mean.reshape(len(snr_db_list), len(Imax_list), 2).transpose(0, 1).contiguous()


def _generic_sharded(points, n_trials, width, work, *, batch, seed, device, dist, builder):
    """Shared skeleton of the curve-type drivers: shard the (point, trial) pairs over ranks, build ``batch`` trials at
    a time, add ``work(inputs, point) -> (batch, width)`` per-trial rows, one all-reduce, mean per point."""
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1
    lo, hi = partition(len(points) * n_trials, world, rank)
    acc = torch.zeros((len(points), width + 1), dtype=torch.float64)
    item = lo
    while item < hi:
        pt = item // n_trials
        t0 = item % n_trials
        t1 = min(n_trials, t0 + batch, t0 + (hi - item))
        p = points[pt]
        if builder == "hip":
            inp = build_trials(p, t0, t1 - t0, seed=seed, sweep_idx=pt, device=device)
        else:
            inp = builder(p, range(t0, t1), seed, pt, device, False)
        rows = torch.as_tensor(work(inp, p)).double().reshape(t1 - t0, width).cpu()
        acc[pt, :width] += rows.sum(dim=0)
        acc[pt, width] += t1 - t0
        item += t1 - t0
    if dist is not None:
        buf = acc.to(device) if dist.get_backend() == "nccl" else acc
        dist.all_reduce(buf, op=dist.ReduceOp.SUM)
        acc = buf.cpu()
    return acc[:, :width] / acc[:, width:width + 1]


def admmiters_points():
    """The four panels of plot_errorVSadmmiters.m (:10-24, :76-90, :141-154, :206-219): (Nt, frame, SNR) =
    (4, 40, 15 dB), (16, 160, 15 dB), (16, 160, 5 dB), (16, 480, 5 dB); Mr = 16, 'ps' combiner, the frame is T
    itself (:21), 20 realisations, Imax = 100."""
    mk = lambda Nt, T, db: SweepParams(Nt=Nt, Nr=32, L=4, T=T, Mr=16, snr_db=float(db), beamformer="ps", T_prop=T)
    return [mk(4, 40, 15), mk(16, 160, 15), mk(16, 160, 5), mk(16, 480, 5)]


def run_convergence_curves(points, n_trials=20, *, Imax=100, batch=20, seed=20190913, device=None, solve_fn=None,
                           dist=None, builder=None):
    """plot_errorVSadmmiters.m:32-71: the mean over realisations of ``convergence_error`` (Imax x 3) of
    ``proposed_algorithm`` (:61) and of ``proposed_algorithm_angles`` (:64) per panel.

    Returns float64 (len(points), 2, Imax, 3): ``[:, 0]`` = mean_error_k, ``[:, 1]`` = mean_error_angles_k.
    ``solve_fn(inputs, Imax) -> (ce, ce_angles)`` (each (batch, Imax, 3)) defaults to the HIP path.
    """
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    builder = _resolve_builder(builder, device)

    def hip(inp, Imax_):
        from . import solvers as J
        args = (Imax_, inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy(), "approximate")
        _, _, ce = J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], inp["B"], *args)
        _, _, cea = J.proposed_algorithm_angles(inp["subY"], inp["Omega"], inp["indx_S"], inp["A"], inp["B"], *args)
        return ce, cea

    fn = hip if solve_fn is None else solve_fn

    def work(inp, p):
        ce, cea = fn(inp, Imax)
        return torch.stack([torch.as_tensor(ce).double().cpu(), torch.as_tensor(cea).double().cpu()], dim=1)

    out = _generic_sharded(points, n_trials, 2 * Imax * 3, work, batch=batch, seed=seed, device=device, dist=dist,
                           builder=builder)
    return out.reshape(len(points), 2, Imax, 3)


def zy_points(F_range=(5,)):
    """plot_errorVSzy.m:7-22,30: Nt = 16, Nr = 32, Mr = 16, 6 rays, frame = 16*F columns, 15 dB, 'ps', rho halved."""
    return [SweepParams(Nt=16, Nr=32, L=4, T=16 * F, Mr=16, rays=6, snr_db=15.0, beamformer="ps", rho_scale=0.5,
                        T_prop=16 * F) for F in F_range]


def run_zy(points=None, n_trials=1, *, Imax=50, batch=32, seed=20190913, device=None, solve_fn=None, dist=None,
           builder=None):
    """plot_errorVSzy.m:28-84: per frame length the mean capped NMSE of the solver's ``S`` (the "Z" curve, :67-71)
    and of ``A'*Y*pinv(B)`` built from its completed measurement (the "Y" curve, :73-77).
    Returns float64 (len(points), 2).  ``solve_fn(inputs, Imax) -> (e_z, e_y)`` defaults to the HIP path."""
    if points is None:
        points = zy_points()
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    builder = _resolve_builder(builder, device)

    def hip(inp, Imax_):
        from . import solvers as J
        S, Y, _ = J.proposed_algorithm(inp["subY"], inp["Omega"], inp["A"], inp["B"], Imax_, inp["tau_Y"].numpy(),
                                       inp["tau_Z"].numpy(), inp["rho"].numpy(), "approximate", want_ce=False)   # :66
        zb = J.colmajor(inp["Zbar"].to(torch.complex64))
        Sy = _times(J.colmajor(inp["A"].conj().transpose(-1, -2).contiguous()), Y, J.pinv(inp["B"]))             # :73
        return J.nmse_spectral(S, zb), J.nmse_spectral(Sy, zb)

    fn = hip if solve_fn is None else solve_fn

    def work(inp, p):
        ez, ey = fn(inp, Imax)
        return torch.stack([torch.as_tensor(ez).double().cpu(), torch.as_tensor(ey).double().cpu()], dim=1)

    return _generic_sharded(points, n_trials, 2, work, batch=batch, seed=seed, device=device, dist=dist, builder=builder)


# (Nr, Mr_e) of the three panels of plot_capacity.m (:8-19, :92-103, :175-186); plot_ee.m (:1-12) is panel 2's shape
CAPACITY_PANELS = {1: (32, 32), 2: (64, 32), 3: (128, 64)}
CAPACITY_DESIGNS = ("DBF", "HBF-PS", "HBF-ZC", "proposed")


def capacity_points(panel):
    """The 11 Mr points ``1:3:32`` of one panel of plot_capacity.m (panel 3: ``1:3:floor(Mr_e/2)``, the same points):
    Nt = 16, L = 4, T = 5, 2 clusters x 3 rays, Gr = Nr, sigma^2 = 10^(-15/10); the frame is T itself."""
    Nr, Mr_e = CAPACITY_PANELS[panel]
    return [SweepParams(Nt=16, Nr=Nr, L=4, T=5, Mr=Mr, Mr_e=Mr_e, snr_db=15.0, T_prop=5) for Mr in range(1, 33, 3)]


def capacity_designs(p):
    """The four combiners of plot_capacity.m at point ``p``: DBF ('ZC', all Nr columns, :45-47), HBF-PS ('quantized', first
    Mr, :50-52), HBF-ZC ('ZC', first Mr, :55-57), proposed ('quantized', Mr of the first Mr_e drawn per realisation, :61-64)."""
    return [("ZC", p.Nr, 0), ("quantized", p.Mr, 0), ("ZC", p.Mr, 0), ("quantized", p.Mr, p.Mr_e)]


def power_model(Nr, Mr, Mr_e, *, Psw=0.005, Pps=0.015, Plna=0.02, Pps_zc=0.06, Pcirc=0.0):
    """plot_ee.m:69-77 — power of (DBF, HBF-PS, HBF-ZC, proposed); EE = mean ASE / power (:84-87)."""
    return [Pcirc + Nr * Nr * Plna + Nr * (Nr + 1) * Pps_zc,
            Pcirc + Mr * Nr * Plna + Nr * (Mr + 1) * Pps,
            Pcirc + Mr * Nr * Plna + Nr * (Mr + 1) * Pps_zc,
            Pcirc + Mr_e * Nr * Plna + Mr_e * Psw + Nr * (Mr_e + 1) * Pps]


def run_capacity(points, n_trials, *, batch=4096, seed=20190913, sweep0=0, device=None, dist=None):
    """plot_capacity.m:32-75 / plot_ee.m:33-88 on the HIP path: per point the mean ASE of the four designs of
    ``capacity_designs`` over ``n_trials`` fresh realisations (point i is sweep index ``sweep0 + i``), sharded over the
    ranks of ``dist`` with one all-reduce of the sums.  Returns float64 numpy (mean, standard error), each
    (len(points), 4)."""
    import numpy as np
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())

    def build(p, trials, seed_, pt, device_, _):
        return ase_trials(p, capacity_designs(p), trials.start, len(trials), seed=seed_, sweep_idx=sweep0 + pt, device=device_)

    def work(a, p):
        return torch.cat([a, a * a], dim=1)

    m = _generic_sharded(points, n_trials, 8, work, batch=batch, seed=seed, device=device, dist=dist, builder=build).numpy()
    mean = m[:, :4]
    var = np.maximum(m[:, 4:] - mean * mean, 0.0) * (n_trials / max(n_trials - 1, 1))
    return mean, np.sqrt(var / n_trials)


# (Nr, clusters, rays) of the six panels of plot_rankR.m (:9-19, :70-80, :128-138, :189-199, :251-261, :313-323)
RANK_PANELS = {1: (32, 2, 3), 2: (64, 2, 3), 3: (128, 2, 3), 4: (32, 3, 12), 5: (64, 3, 12), 6: (128, 3, 12)}


def rank_points(panel):
    """The three points ``L = 1, 4, 8`` of one panel of plot_rankR.m: Nt = 4, Mr_e = 32, Mr = 4, Gr = Nr, 4-QAM pilots; the
    frame is T = 50 itself (the script passes T to proposed_hbf).  ``min(Nr, Mr_e) = 32`` values are kept per curve."""
    Nr, clusters, rays = RANK_PANELS[panel]
    return [SweepParams(Nt=4, Nr=Nr, L=L, T=50, Mr=4, Mr_e=32, clusters=clusters, rays=rays, T_prop=50) for L in (1, 4, 8)]


def run_rank(points, n_trials=1, *, n_keep=None, batch=4096, seed=20190913, sweep0=0, device=None, dist=None, channel=None,
             channel_normalize="reference"):
    """plot_rankR.m:24-50 on the HIP path: per point the mean over ``n_trials`` realisations of the first ``n_keep``
    singular values (default ``min(Nr, Mr_e, T_prop)`` of the first point) of the noise-free receive signal (point i is
    sweep index ``sweep0 + i``), sharded over the ranks of ``dist`` with one all-reduce of the sums.

    The reference plots ONE realisation per curve: its ``mean(eig_dist, 3)`` (:52) acts on a 2-D array and does nothing.  So
    ``n_trials`` defaults to 1; larger values give the averaged curve, which the script's author presumably meant.

    Any shape ``spectrum_trials`` takes (at the figure's shapes: the kernel and the bits of ``rank_trials``).  ``channel``,
    ``channel_normalize``: a supplied channel instead of the drawn one, as ``run_points(..., channel=H)`` takes it - shared
    ``(Nr_src, Nt_src, L)`` or one per trial ``(n_trials, Nr_src, Nt_src, L)``, every point with that L; the marker is then
    ``L*Nt``, the only bound known without the channel's own rank.

    Returns float64 numpy ``(spectrum, marker)``: (len(points), n_keep) mean singular values, and per point the rank bound
    ``min(Np, L*Nt)`` whose successor index the script marks with a vertical line (:61-62)."""
    import numpy as np
    if channel is not None:                     # refused here, before anything touches a device
        from .system_model import _check_channel
        per_trial = len(getattr(channel, "shape", ())) == 4
        for p in points:
            _check_channel(p, n_trials if per_trial else 1, channel, channel_normalize)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if n_keep is None:
        n_keep = min(points[0].Nr, points[0].Mr_e, points[0].T_prop)

    def build(p, trials, seed_, pt, device_, _):
        ch = channel if channel is None or len(channel.shape) == 3 else channel[trials.start:trials.stop]
        return spectrum_trials(p, trials.start, len(trials), seed=seed_, sweep_idx=sweep0 + pt, n_keep=n_keep, device=device_,
                               channel=ch, channel_normalize=channel_normalize)

    mean = _generic_sharded(points, n_trials, n_keep, lambda sv, p: sv, batch=batch, seed=seed, device=device, dist=dist,
                            builder=build).numpy()
    return mean, np.array([min(p.clusters * p.rays, p.L * p.Nt) if channel is None else p.L * p.Nt for p in points])


TRACKING_MODES = ("cold", "warm", "warm_vs")
# accepted beside the default three: they pass an indx_S (the wide ones: of support_order_wide*) or refresh one inside the solver
TRACKING_PAI_MODES = ("pai", "pai_prev", "warm_pai_prev", "pai_wide_prev", "warm_pai_wide_prev", "refresh", "warm_refresh",
                      "pai_prev_refresh")
_PREV_MODES = ("pai_prev", "warm_pai_prev", "pai_wide_prev", "warm_pai_wide_prev", "pai_prev_refresh")
_WIDE_MODES = ("pai_wide_prev", "warm_pai_wide_prev")
_REFRESH_MODES = ("refresh", "warm_refresh", "pai_prev_refresh")      # float64 only: proposed_algorithm_refresh_f64
# float64 only, with stop=(tol, min_iters): one solve per frame at cold_imax by proposed_algorithm_until_f64, each trial stopped
# when its iterate has settled
TRACKING_UNTIL_MODES = ("cold_until", "warm_until", "refresh_until", "warm_refresh_until")


def run_tracking(p: SweepParams, n_seqs, n_frames, corr, *, imax=(10, 20, 30, 50, 100), cold_imax=100, modes=TRACKING_MODES,
                 precision="f64", batch=16, seed=20190913, sweep_idx=0, device=None, drift=None, widen=(1, 1),
                 widen_primary="neighbourhood", refresh=(0, 1), refresh_f32=False, stop=None, until_f32=False, refit=None):
    """What a warm start of the ADMM buys on a slowly varying channel (DESIGN.md sections 9n, 9o): the loop of
    tools/run_tracking.py on frames the library builds.  ``n_seqs`` independent sequences of ``n_frames`` frames at point ``p``;
    sequence t, frame f is ``build_trials(p, t, 1, seed=seed, sweep_idx=sweep_idx, frame=f, corr=corr)`` - fixed angles, path gains
    ``g_f = corr g_{f-1} + sqrt(1 - corr^2) w_f``, pilots, noise and sampling pattern of the frame's own - so SNR point
    (``sweep_idx``) and frame vary independently and the result does not depend on ``batch``, the number of sequences built and
    solved per call.

    Per frame and sequence, at each Imax of ``imax`` (``cold`` also at ``cold_imax``), by ``proposed_algorithm_resume_f64`` and
    ``nmse_spectral_f64`` (``precision="f64"``) or their fp32 siblings (``"f32"``):
      cold     from zero
      warm     from the previous frame's whole state [X | V1 | V2 | C | v | S]; each Imax is a chain of its own
      warm_vs  from the previous frame's v and S only (X = V1 = V2 = C = 0)
    and, when asked for in ``modes``, the "Proposed - PAI" variants, which pass an ``indx_S``:
      pai            from zero, with the frame's own ``indx_S`` from the builder (the genie of plot_errorVSsnr.m:143-145)
      pai_prev       from zero, with ``support_order`` (``support_order_f64``) of the S this (mode, Imax) chain returned at the
                     previous frame - what a receiver has; frame 0 is solved without ``indx_S``
      warm_pai_prev  from the previous frame's whole state, ``indx_S`` as ``pai_prev``
    and the same two with the order widened over neighbouring angle cells:
      pai_wide_prev, warm_pai_wide_prev  ``pai_prev`` / ``warm_pai_prev`` with ``support_order_wide`` (``_f64``) at the radii
                     ``widen = (wr, wt)`` and ``widen_primary`` ("neighbourhood" or "ties") in place of ``support_order``
    and (``precision="f64"`` only) the support refreshed from the solver's own iterate inside the loop, by
    ``proposed_algorithm_refresh_f64`` at ``refresh = (start, period)``:
      refresh           from zero, no order in force until the first refresh
      warm_refresh      from the previous frame's whole state, no order in force until the first refresh
      pai_prev_refresh  from zero, ``support_order_f64`` of the chain's previous S in force until the first refresh
    ``refresh_f32=True`` (``precision="f32"`` only) runs these three through the fp32 solver instead, by
    ``proposed_algorithm_refresh`` with ``support_order`` for the prior; without it ``precision="f32"`` refuses them as before.
    and (``precision="f64"`` only, selected by ``stop = (tol, min_iters)`` or ``stop = tol``) the stopping
    rule of ``proposed_algorithm_until_f64``: ONE solve per frame with ``Imax = cold_imax``, each trial stopped at its own iteration:
      cold_until, warm_until                  ``cold`` / ``warm`` with the rule
      refresh_until, warm_refresh_until       ``refresh`` / ``warm_refresh`` with the rule
    ``until_f32=True`` (``precision="f32"`` only, with ``stop``) runs these four through the fp32 solver
    instead, by ``proposed_algorithm_until``; without it ``precision="f32"`` refuses them as before.
    Their results also carry ``mean_iters``, ``median_iters``, ``max_iters`` and ``mean_iters_by_frame`` over the scored frames.
    ``refit = (K, iters)`` (``precision="f64"`` only): the S that is scored is also re-fitted on its ``K``
    largest entries by ``iters`` conjugate-gradient steps of ``refit_f64`` and scored again; every (mode, Imax) row then also
    carries ``mean_nmse_refit``, ``mean_nmse_refit_by_frame`` and ``refit_estimates_per_s`` (the re-fit's own time).  The re-fitted
    S is only scored: it is never fed back into a state or into a previous-estimate order, so every other number of the result is
    what it is with ``refit=None``.
    ``drift``: a float lets the angles of every sequence walk (``build_trials(..., drift=)``: standard deviation of one frame's
    increment, radians), so the support moves; ``None`` (the default) builds the frames that were built before.
    States, estimates and scores stay on the device; the scores come to the host once per chunk of sequences.  Frame 0, where every
    mode starts from zero, is not scored.  Single process: sequences are not sharded over ranks.

    Returns the dictionary tools/run_tracking.py prints - per (mode, Imax) ``mean_nmse`` over the scored frames, ``sem_over_seqs``,
    ``median_nmse``, ``mean_nmse_by_frame`` and ``estimates_per_s`` (solver time only, frame 0 left out) - plus
    ``"channel": "device"``, ``"drift"`` when one was given, and ``"widen"``, ``"widen_primary"`` when a wide mode was asked for and ``"refresh"`` when a refresh mode was."""
    import time
    import numpy as np
    from . import solvers as J
    n_seqs, n_frames, batch, corr = int(n_seqs), int(n_frames), int(batch), float(corr)
    imax = [int(i) for i in imax]
    if n_seqs < 1 or n_frames < 2 or batch < 1:
        raise ValueError("run_tracking needs n_seqs >= 1, n_frames >= 2 (frame 0 is not scored) and batch >= 1")
    if not 0.0 <= corr <= 1.0:
        raise ValueError("corr must lie in [0, 1], not %r" % (corr,))
    if precision not in ("f64", "f32"):
        raise ValueError("precision must be 'f64' or 'f32', not %r" % (precision,))
    every = TRACKING_MODES + TRACKING_PAI_MODES + TRACKING_UNTIL_MODES
    if not modes or any(m not in every for m in modes) or not imax or min(imax + [int(cold_imax)]) < 1:
        raise ValueError("modes must be a non-empty subset of %r, and every Imax >= 1" % (every,))
    until = [m for m in TRACKING_UNTIL_MODES if m in modes]
    stop_tol = stop_min = None
    if until_f32 and precision != "f32":
        raise ValueError("until_f32 runs the *_until modes on the fp32 solver: precision must be 'f32', not %r" % (precision,))
    if until_f32 and stop is None:
        raise ValueError("until_f32 needs stop=(tol, min_iters): it selects the solver of the modes %r" % (TRACKING_UNTIL_MODES,))
    if until:
        if precision != "f64" and not until_f32:
            raise ValueError("the modes %r stop inside the float64 solver: precision must be 'f64'" % (TRACKING_UNTIL_MODES,))
        if stop is None:
            raise ValueError("the modes %r need stop=(tol, min_iters)" % (TRACKING_UNTIL_MODES,))
        try:
            stop_tol, stop_min = (float(stop[0]), int(stop[1])) if np.ndim(stop) else (float(stop), 2)
        except (TypeError, ValueError, IndexError):
            raise ValueError("stop must be tol or a pair (tol, min_iters), not %r" % (stop,)) from None
        if not stop_tol > 0.0 or stop_min < 1:
            raise ValueError("stop = %r: need tol > 0 and min_iters >= 1" % (stop,))
    if refit is not None:
        try:
            refit_K, refit_iters = (int(x) for x in refit)
        except (TypeError, ValueError):
            raise ValueError("refit must be a pair (K, iters), not %r" % (refit,)) from None
        if precision != "f64":
            raise ValueError("refit re-fits in float64 (refit_f64): precision must be 'f64', not %r" % (precision,))
        g_all = p.solver_shape[2] * p.solver_shape[3]
        if not 1 <= refit_K <= g_all or (refit_K > J._lib.SUPPORT_TOP_MAX and refit_K != g_all) or refit_iters < 1:
            raise ValueError("refit = %r: need 1 <= K <= min(Gr*G2, %d) or K = Gr*G2 = %d, and iters >= 1"
                             % (refit, J._lib.SUPPORT_TOP_MAX, g_all))
    if drift is not None:
        drift = float(drift)
        if not (np.isfinite(drift) and drift >= 0.0):
            raise ValueError("drift must be finite and >= 0, not %r" % (drift,))
    try:
        wr, wt = (int(x) for x in widen)
    except (TypeError, ValueError):
        raise ValueError("widen must be a pair (wr, wt) of radii, not %r" % (widen,)) from None
    if wr < 0 or wt < 0:
        raise ValueError("widen must be a pair of radii >= 0, not %r" % (widen,))
    if widen_primary not in ("neighbourhood", "ties"):
        raise ValueError("widen_primary must be 'neighbourhood' or 'ties', not %r" % (widen_primary,))
    if any(m in _WIDE_MODES for m in modes) and (2 * wr + 1 > p.Gr or 2 * wt + 1 > p.Gt):
        raise ValueError("widen = %r: a window of %d x %d cells meets itself round the %d x %d angle grid"
                         % ((wr, wt), 2 * wr + 1, 2 * wt + 1, p.Gr, p.Gt))
    try:
        r_start, r_period = (int(x) for x in refresh)
    except (TypeError, ValueError):
        raise ValueError("refresh must be a pair (start, period), not %r" % (refresh,)) from None
    if r_start < 0 or r_period < 0:
        raise ValueError("refresh must be a pair (start, period) >= 0, not %r" % (refresh,))
    if refresh_f32 and precision != "f32":
        raise ValueError("refresh_f32 runs the refresh modes on the fp32 solver: precision must be 'f32', not %r" % (precision,))
    if precision != "f64" and not refresh_f32 and any(m in _REFRESH_MODES for m in modes):
        raise ValueError("the modes %r refresh the support inside the float64 solver: precision must be 'f64'" % (_REFRESH_MODES,))
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    N, M, Gr, G2 = p.solver_shape
    nm = N * M
    f64 = precision == "f64"
    wide = (lambda x: J.colmajor(x.to(torch.complex128))) if f64 else (lambda x: x)
    solve = J.proposed_algorithm_resume_f64 if f64 else J.proposed_algorithm_resume
    solve_refresh = J.proposed_algorithm_refresh_f64 if f64 else J.proposed_algorithm_refresh
    solve_until = J.proposed_algorithm_until_f64 if f64 else J.proposed_algorithm_until
    score = J.nmse_spectral_f64 if f64 else J.nmse_spectral
    order = J.support_order_f64 if f64 else J.support_order
    order_wide = J.support_order_wide_f64 if f64 else J.support_order_wide
    keys = [("cold", i) for i in sorted(set(imax + [int(cold_imax)])) if "cold" in modes] + \
           [(m, i) for m in ("warm", "warm_vs") + TRACKING_PAI_MODES if m in modes for i in imax] + [(m, int(cold_imax)) for m in until]
    frame_kw = {} if drift is None else {"drift": drift}
    err = {k: [] for k in keys}                                     # per chunk: (scored frames, chunk) on the host
    secs = {k: 0.0 for k in keys}
    its = {k: [] for k in keys if k[0] in until}                    # per chunk: iterations, (scored frames, chunk) on the host
    err_fit = {k: [] for k in keys if refit is not None}            # the re-fitted S, scored as err is
    secs_fit = {k: 0.0 for k in err_fit}
    for t0 in range(0, n_seqs, batch):
        nb = min(batch, n_seqs - t0)
        state, prev_S = {}, {}
        e_dev = {k: [] for k in keys}
        i_dev = {k: [] for k in its}
        f_dev = {k: [] for k in err_fit}
        for f in range(n_frames):
            inp = build_trials(p, t0, nb, seed=seed, sweep_idx=sweep_idx, device=device, frame=f, corr=corr, **frame_kw)
            args = (wide(inp["subY"]), J.colmajor(inp["Omega"].to(torch.float64)) if f64 else inp["Omega"], wide(inp["A"]),
                    wide(inp["B"]))
            prm = (inp["tau_Y"].numpy(), inp["tau_Z"].numpy(), inp["rho"].numpy())
            zb = wide(inp["Zbar"])
            for k in keys:
                mode, n_it = k
                warm = mode in ("warm", "warm_vs", "warm_pai_prev", "warm_pai_wide_prev", "warm_refresh", "warm_until", "warm_refresh_until")
                st = state.get(k) if warm else None
                if st is not None and mode == "warm_vs":
                    st = st.clone()
                    st[:, :4 * nm] = 0
                ix = {}
                if mode == "pai":
                    ix = {"indx_S": inp["indx_S"]}
                elif mode in _WIDE_MODES and k in prev_S:
                    ix = {"indx_S": order_wide(prev_S[k], p.Gt, wr, wt, primary=widen_primary)}
                elif mode in _PREV_MODES and k in prev_S:
                    ix = {"indx_S": order(prev_S[k])}               # (not timed: the solver's rate is what estimates_per_s reports)
                torch.cuda.synchronize(device)
                c0 = time.perf_counter()
                if mode in until:
                    S, _, _, out, _, n_ran, _ = solve_until(
                        *args, n_it, *prm, tol=stop_tol, min_iters=stop_min, refresh=(r_start, r_period) if "refresh" in mode else None,
                        state=st, return_state=warm)
                elif mode in _REFRESH_MODES:
                    S, _, _, out, _ = solve_refresh(*args, n_it, *prm, start=r_start, period=r_period, want_ce=False, state=st,
                                                    return_state=warm, **ix)
                else:
                    S, _, _, out = solve(*args, n_it, *prm, want_ce=False, state=st, return_state=warm, **ix)
                torch.cuda.synchronize(device)
                dt = time.perf_counter() - c0
                if warm:
                    state[k] = out
                if mode in _PREV_MODES:
                    prev_S[k] = S
                if f:
                    secs[k] += dt
                    e_dev[k].append(torch.as_tensor(score(S, zb)).double())
                    if mode in until:
                        i_dev[k].append(n_ran)
                    if refit is not None:                           # (after everything the chain keeps: S itself goes on unchanged)
                        torch.cuda.synchronize(device)
                        c0 = time.perf_counter()
                        S_fit, _ = J.refit_f64(*args, S, refit_K, refit_iters)
                        torch.cuda.synchronize(device)
                        secs_fit[k] += time.perf_counter() - c0
                        f_dev[k].append(torch.as_tensor(score(S_fit, zb)).double())
        for k in keys:
            err[k].append(torch.stack(e_dev[k]).cpu().numpy())
        for k in its:
            its[k].append(torch.stack(i_dev[k]).cpu().numpy())
        for k in err_fit:
            err_fit[k].append(torch.stack(f_dev[k]).cpu().numpy())

    def summary(k):
        e = np.concatenate(err[k], axis=1)                          # (scored frames, seqs)
        per_seq = e.mean(axis=0)
        out = {"mode": k[0], "Imax": k[1], "mean_nmse": float(e.mean()),
               "sem_over_seqs": float(per_seq.std(ddof=1) / np.sqrt(len(per_seq))) if len(per_seq) > 1 else None,
               "median_nmse": float(np.median(e)), "mean_nmse_by_frame": [float(x) for x in e.mean(axis=1)],
               "estimates_per_s": n_seqs * (n_frames - 1) / secs[k]}
        if k in its:
            n = np.concatenate(its[k], axis=1)                      # (scored frames, seqs)
            out.update(mean_iters=float(n.mean()), median_iters=float(np.median(n)), max_iters=int(n.max()),
                       mean_iters_by_frame=[float(x) for x in n.mean(axis=1)])
        if k in err_fit:
            ef = np.concatenate(err_fit[k], axis=1)                 # (scored frames, seqs)
            out.update(mean_nmse_refit=float(ef.mean()), mean_nmse_refit_by_frame=[float(x) for x in ef.mean(axis=1)],
                       refit_estimates_per_s=n_seqs * (n_frames - 1) / secs_fit[k])
        return out

    res = {"tool": "run_tracking", "precision": precision, "shape": [N, M, Gr, G2], "frames": n_frames, "seqs": n_seqs, "corr": corr,
           "clusters": p.clusters, "rays": p.rays, "snr_db": p.snr_db, "seed": seed, "scored_frames": list(range(1, n_frames)),
           "cold_imax": int(cold_imax), "results": [summary(k) for k in keys], "channel": "device"}
    if drift is not None:
        res["drift"] = drift
    if any(m in _WIDE_MODES for m in modes):
        res["widen"], res["widen_primary"] = [wr, wt], widen_primary
    if refit is not None:
        res["refit"] = [refit_K, refit_iters]
    if until:
        res["stop"] = [stop_tol, stop_min]
        if until_f32:
            res["until_f32"] = True
    if any(m in _REFRESH_MODES for m in modes) or any("refresh" in m for m in until):
        res["refresh"] = [r_start, r_period]
        if refresh_f32:
            res["refresh_f32"] = True
    return res
