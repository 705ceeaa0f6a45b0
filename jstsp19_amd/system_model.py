"""Batched, device-resident construction of the solver inputs (the caller side of the hot path).

What plot_errorVSsnr.m:57-136 does per trial on the host — channel, pilots, noise, the
random-spatial-sampling measurement, the dictionary factors A, B and the hyper-parameters —
is done for a whole batch of Monte-Carlo trials by the library's own kernels
(``jstsp_build_trials_c32``, csrc/inputgen.hip), so that the solver's inputs are born in HBM;
this module holds the parameter classes (names as in the reference's scripts) and the two thin
wrappers around that call.  Not the timed hot path.  The quirks of the
reference (tap-1 steering reuse, cumulative cluster sum, Hermitian Toeplitz pilots, sigma_6 in rho)
are reproduced by the kernels and checked against oracle/system_model.py on the library's own draws.

Random numbers come from counter-based Philox streams keyed by (seed, sweep index, global trial
index), so a trial's inputs do not depend on how trials are sharded over GPUs.

(Rounds 1-3 also kept a torch tensor-op implementation of the same construction here; it now lives in
tests/torch_builder.py, where the CPU-side tests of the sweep runner use it.)
"""
from __future__ import annotations

import math

import torch

__all__ = ["SweepParams", "TrainingParams", "build_trials", "build_trials_training", "ase_trials", "rank_trials", "spectrum_trials"]


class SweepParams:
    """Parameters of one sweep point — names follow plot_errorVSsnr.m:8-25.

    What the sibling drivers change in the construction: ``beamformer`` ('ZC', or 'fft' / 'ps' — the same unitary
    DFT matrix, createBeamformer.m:5,12-13), ``rho_rule`` ('min': min(eigs(Y'Y)) = the 6th largest eigenvalue,
    'max': the largest), ``rho_scale`` (plot_errorVSzy.m:65 halves rho) and ``T_prop`` (plot_errorVSadmmiters.m:21 and
    plot_errorVSzy.m:30 use the frame length itself instead of T*Nt).
    """

    def __init__(self, Nt, Nr, L, T, Mr, Mr_e=None, Gr=None, Gt=None, clusters=2, rays=3, snr_db=5.0,
                 beamformer="ZC", rho_rule="min", rho_scale=1.0, T_prop=None):
        self.Nt, self.Nr, self.L, self.T, self.Mr = Nt, Nr, L, T, Mr
        self.Mr_e = Nr if Mr_e is None else Mr_e
        self.Gr = Nr if Gr is None else Gr
        self.Gt = Nt if Gt is None else Gt
        self.clusters, self.rays = clusters, rays
        self.snr_db = float(snr_db)
        if beamformer not in ("ZC", "fft", "ps") or rho_rule not in ("min", "max"):
            raise ValueError("beamformer must be 'ZC', 'fft' or 'ps'; rho_rule 'min' or 'max'")
        self.beamformer, self.rho_rule, self.rho_scale = beamformer, rho_rule, float(rho_scale)
        self._T_prop = T_prop

    def replace(self, **kw):
        """A copy with some parameters changed (``Gt`` follows ``Nt`` unless given, as the drivers keep Gt = Nt)."""
        cur = dict(Nt=self.Nt, Nr=self.Nr, L=self.L, T=self.T, Mr=self.Mr, Mr_e=self.Mr_e, Gr=self.Gr, Gt=self.Gt,
                   clusters=self.clusters, rays=self.rays, snr_db=self.snr_db, beamformer=self.beamformer,
                   rho_rule=self.rho_rule, rho_scale=self.rho_scale, T_prop=self._T_prop)
        if "Nt" in kw and "Gt" not in kw:
            cur["Gt"] = kw["Nt"]
        cur.update(kw)
        return SweepParams(**cur)

    @property
    def T_prop(self):                       # plot_errorVSsnr.m:23
        return self.T * self.Nt if self._T_prop is None else self._T_prop

    @property
    def noise_var(self):                    # :49
        return 10.0 ** (-self.snr_db / 10.0)

    @property
    def T_hbf(self):                        # plot_errorVSsnr.m:22 — MATLAB round() is half away from zero
        x = self.T / (self.Nr / self.Mr)
        return int(math.floor(abs(x) + 0.5) * (1 if x >= 0 else -1)) * self.Nt

    @property
    def solver_shape(self):
        """(N, M, Gr, G2) of the proposed_algorithm call."""
        return self.Mr_e, self.T_prop, self.Gr, self.L * self.Gt


class TrainingParams:
    """Parameters of the Alg.1-vs-Alg.2 driver — names follow plot_errorVSsnr_approx.m:8-20
    (``Gr = Nr``, ``Gt = Nt``; the frame is T columns, not T*Nt)."""

    def __init__(self, Nt=4, Nr=32, L=4, T=70, ratio=0.75, clusters=2, rays=3, snr_db=5.0):
        self.Nt, self.Nr, self.L, self.T, self.ratio = Nt, Nr, L, T, float(ratio)
        self.Gr, self.Gt = Nr, Nt
        self.clusters, self.rays = clusters, rays
        self.snr_db = float(snr_db)

    @property
    def Lr(self):                           # wideband_hybBF_comm_system_training.m:5 (MATLAB round)
        return int(math.floor(self.ratio * self.Nr + 0.5))

    @property
    def noise_var(self):                    # plot_errorVSsnr_approx.m:35
        return 10.0 ** (-self.snr_db / 10.0)

    @property
    def solver_shape(self):
        return self.Nr, self.T, self.Gr, self.L * self.Gt


def build_trials_training(p: TrainingParams, trial0, batch, *, seed=20190913, sweep_idx=0, device=None, want_draws=False,
                          want_H=False, ctx=None):
    """wideband_hybBF_comm_system_training.m:1-58 + plot_errorVSsnr_approx.m:45-58 for trials [trial0, trial0 + batch) on
    the HIP path: the same library call as ``build_trials`` with the model fields that make it that builder — Gaussian
    Hermitian-Toeplitz pilots (:19-22), the unitary DFT combiner over all Nr outputs (:10), ``Lr = round(ratio*Nr)``
    of them kept per column (:5,:48-53), the frame T itself, ``rho = sqrt(lambda_6 (tau_X + tau_S)/2)`` (:51-53).
    Keys: subY, Omega, A, B, Zbar (complex64, column-major), indx_S, tau_X, tau_S, rho - the dict ``build_inputs_training`` of
    tests/torch_builder.py returns."""
    q = SweepParams(p.Nt, p.Nr, p.L, p.T, p.Lr, Mr_e=p.Nr, Gr=p.Gr, Gt=p.Gt, clusters=p.clusters, rays=p.rays,
                    snr_db=p.snr_db, beamformer="fft", rho_rule="min", rho_scale=math.sqrt(0.75), T_prop=p.T)
    o = build_trials(q, trial0, batch, seed=seed, sweep_idx=sweep_idx, device=device, want_draws=want_draws, want_H=want_H,
                     ctx=ctx, pilots="gauss")
    o["tau_X"] = o.pop("tau_Y")                                                 # plot_errorVSsnr_approx.m:50
    o["tau_S"] = o["tau_X"] / 2.0                                               # :51
    del o["tau_Z"]
    return o


_CHANNEL_NORMALIZE = {"asis": 0, "reference": 1, "unit": 2}         # JSTSP_CHAN_* (include/jstsp.h)


def _check_channel(p, batch, channel, channel_normalize):
    """Shape and dtype of a supplied channel, on the Python side (nothing of the library is touched): returns
    (per_trial, Nr_src, Nt_src)."""
    if channel_normalize not in _CHANNEL_NORMALIZE:
        raise ValueError("channel_normalize must be 'asis', 'reference' or 'unit', not %r" % (channel_normalize,))
    if not hasattr(channel, "shape") or not hasattr(channel, "dtype"):
        raise TypeError("channel must be a numpy or torch complex array, not %s" % type(channel).__name__)
    cplx = channel.is_complex() if torch.is_tensor(channel) else channel.dtype.kind == "c"
    if not cplx:
        raise TypeError("channel must be complex (complex64, or complex128 which is narrowed once), not %s" % (channel.dtype,))
    shape = tuple(channel.shape)
    if len(shape) not in (3, 4):
        raise ValueError("channel must be (Nr_src, Nt_src, L) or (batch, Nr_src, Nt_src, L), not %r" % (shape,))
    if len(shape) == 4 and shape[0] != batch:
        raise ValueError("a per-trial channel needs one channel per trial of the call: %d, not %d" % (batch, shape[0]))
    nr, nt, L = shape[-3:]
    if L != p.L:
        raise ValueError("channel has %d delay taps, the model has L = %d" % (L, p.L))
    if nr < p.Nr or nt < p.Nt:
        raise ValueError("the source taps are %d x %d, smaller than Nr x Nt = %d x %d" % (nr, nt, p.Nr, p.Nt))
    return len(shape) == 4, nr, nt


def _channel_on_device(channel, device):
    """The supplied channel as a complex64 tensor on ``device`` whose taps are column-major, as MATLAB stores H(:,:,l):
    strides (1, Nr_src, Nr_src*Nt_src), trial index slowest.  complex128 is narrowed once, on the host side; a tensor that
    already is complex64, on the device and in that layout is returned as it is."""
    x = channel if torch.is_tensor(channel) else None
    if x is None:
        import numpy as np
        x = torch.from_numpy(np.ascontiguousarray(np.asarray(channel).astype(np.complex64, copy=False)))
    elif x.dtype != torch.complex64:
        x = x.to(torch.complex64)
    nr, nt, L = x.shape[-3:]
    want = (1, nr, nr * nt) if x.ndim == 3 else (nr * nt * L, 1, nr, nr * nt)
    if x.device == device and tuple(x.stride()) == want:
        return x
    x = x.to(device)
    perm = (2, 1, 0) if x.ndim == 3 else (0, 3, 2, 1)
    return x.permute(*perm).contiguous().permute(*perm)


def build_trials(p: SweepParams, trial0, batch, *, seed=20190913, sweep_idx=0, device=None, with_hbf=False,
                 want_draws=False, want_H=False, shared_pilots=False, ctx=None, pilots="qam4", channel=None,
                 channel_normalize="reference", frame=0, corr=None, drift=None):
    """plot_errorVSsnr.m:57-136 for trials [trial0, trial0 + batch) on the HIP path
    (``jstsp_build_trials_c32``, csrc/inputgen.hip): draws, channel, pilots, measurement, A, B,
    hyper-parameters and indx_S are produced by the library's own kernels — nothing but the output
    allocation goes through torch.  Keys: subY, Omega, A, B, Zbar (complex64, column-major), indx_S, tau_Y, tau_Z, rho
    (the dict ``build_inputs`` of tests/torch_builder.py returns);
    ``shared_pilots``: one pilot set for the whole sweep point (``B`` identical for every trial: pass ``B[0]``).
    ``want_draws`` adds the raw draws (gains, u_r, u_t, noise, qam_idx) for checking against a CPU
    restatement.  The Philox streams are keyed by (seed, sweep_idx, global trial index).

    ``channel``: a numpy or torch complex array that replaces the drawn channel (``jstsp_build_trials_from_channel_c32``, the
    first lines of plot_errorVSsnr_nyuwireless.m:60-69) - ``(Nr_src, Nt_src, L)`` with ``channel[:, :, l]`` as tap l, one
    channel for every trial, or ``(batch, Nr_src, Nt_src, L)``, one per trial; ``Nr_src >= p.Nr``, ``Nt_src >= p.Nt`` (the
    leading block is used, :63-64), ``L == p.L``.  ``channel_normalize`` per tap, with s = norm(H_l): "asis", "reference"
    (H_l / s^2, :65-66 as written - a tap of norm 1/s) or "unit" (H_l / s).  The result has the same keys plus ``sigma_max``,
    float64 ``(L,)`` or ``(batch, L)`` (left out where "asis" meets min(Nr, Nt) > 64, the one case the library needs no s
    for and cannot compute it); ``want_draws`` then adds noise, qam_idx and pilot_sym only - nothing else was drawn.  Noise,
    pilots and Omega are those of the drawn call with the same seed, sweep index and trial.

    ``corr``: a float in [0, 1] makes trial t a SEQUENCE of channels and returns its frame ``frame`` (0..65535) by
    ``jstsp_build_trials_tracked_c32``: the angles of the drawn call at every frame, the path gains
    ``g_f = corr g_{f-1} + sqrt(1 - corr^2) w_f`` (in closed form: a frame depends on no earlier call), noise, pilots and Omega of
    the frame's own.  Frame 0 is the drawn call on the bits; ``want_draws`` returns the frame's ``gains``.  ``corr=None`` (the
    default) is the drawn call and takes no ``frame``; ``corr`` with ``channel=`` is a ``ValueError``.

    ``drift``: a finite float >= 0 (it needs ``corr``) lets the angles of that sequence walk
    (``jstsp_build_trials_tracked_drift_c32``): ``phi_f = phi_0 + drift * sum_{k=1..f} z_k``, z_k ~ N(0, 1) independent per path
    and array end, ``drift`` the standard deviation of one frame's increment in radians.  ``u_r``, ``u_t`` stay the drawn call's;
    ``want_draws`` also returns ``dphi_r``, ``dphi_t``, float64 ``(batch, Np)``: ``phi_f - phi_0``.  ``drift=0.0`` returns the
    arrays of ``drift=None`` on the bits, and ``drift=None`` (the default) calls what was called before.  ``drift`` without
    ``corr``, negative or non-finite is a ``ValueError``.
    """
    if corr is not None and channel is not None:
        raise ValueError("corr= (a tracked channel) and channel= (a supplied channel) exclude each other")
    if corr is None and frame != 0:
        raise ValueError("frame=%r needs corr=, the correlation of the sequence from one frame to the next" % (frame,))
    if drift is not None:
        if corr is None:
            raise ValueError("drift=%r needs corr=: the angles walk along a tracked sequence" % (drift,))
        drift = float(drift)
        if not (math.isfinite(drift) and drift >= 0.0):
            raise ValueError("drift must be finite and >= 0 (the standard deviation of one frame's angle increment), not %r" % (drift,))
    import ctypes as C
    import numpy as np
    from . import _lib
    from .solvers import empty_colmajor
    if channel is not None:
        per_trial, nr_src, nt_src = _check_channel(p, batch, channel, channel_normalize)
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    c = ctx if ctx is not None else _lib.default_context(device.index or 0)
    c.use_torch_stream()
    N, M, Gr, G2 = p.solver_shape
    Np = p.clusters * p.rays
    Th = p.T_hbf if with_hbf else 0
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, Th,
                       1 if shared_pilots else 0, p.noise_var, _lib.BF_ZC if p.beamformer == "ZC" else _lib.BF_DFT,
                       _lib.RHO_MAX if p.rho_rule == "max" else _lib.RHO_MIN6, p.rho_scale,
                       _lib.PILOTS_GAUSS if pilots == "gauss" else _lib.PILOTS_QAM4)
    c64, f32 = torch.complex64, torch.float32
    out = dict(subY=empty_colmajor(batch, N, M, c64, device), Omega=empty_colmajor(batch, N, M, f32, device),
               A=empty_colmajor(1, N, Gr, c64, device)[0], B=empty_colmajor(batch, G2, M, c64, device),
               Zbar=empty_colmajor(batch, Gr, G2, c64, device),
               indx_S=torch.empty((batch, Gr * G2), dtype=torch.int32, device=device))
    if want_H:
        out["H"] = empty_colmajor(batch, p.Nr, p.Nt * p.L, c64, device)
    if with_hbf:
        out["Y_hbf"] = empty_colmajor(batch, p.Nr, Th, c64, device)
        out["A_hbf"] = empty_colmajor(1, p.Nr, Gr, c64, device)[0]
        out["B_hbf"] = empty_colmajor(batch, G2, Th, c64, device)
    if want_draws and channel is None:
        out["gains"] = torch.empty((batch, p.L, Np), dtype=c64, device=device)
        out["u_r"] = torch.empty((batch, Np), dtype=f32, device=device)
        out["u_t"] = torch.empty((batch, Np), dtype=f32, device=device)
    if want_draws:
        out["noise"] = empty_colmajor(batch, p.Nr, p.T_prop, c64, device)
        out["qam_idx"] = torch.empty((batch, p.Nt, p.T_prop), dtype=torch.uint8, device=device)
        out["pilot_sym"] = torch.empty((batch, p.Nt, p.T_prop), dtype=c64, device=device)
    hyp = {k: np.empty(batch, dtype=np.float64) for k in ("tau_Y", "tau_Z", "rho")}
    tr = _lib.Trials()
    for k, v in out.items():
        setattr(tr, k, v.data_ptr())
    for k, v in hyp.items():
        setattr(tr, k, v.ctypes.data_as(C.POINTER(C.c_double)))
    if drift is not None:
        dphi = {k: torch.empty((batch, Np), dtype=torch.float64, device=device) for k in ("dphi_r", "dphi_t")} if want_draws else {}
        rc = c._lib.jstsp_build_trials_tracked_drift_c32(
            c.handle, C.byref(model), C.c_uint64(seed), int(sweep_idx), int(trial0), int(batch), int(frame), float(corr), drift,
            C.byref(tr), dphi["dphi_r"].data_ptr() if dphi else None, dphi["dphi_t"].data_ptr() if dphi else None, _lib.DEVICE)
        _lib.check(rc, "jstsp_build_trials_tracked_drift_c32")
        out.update(dphi)
    elif corr is not None:
        rc = c._lib.jstsp_build_trials_tracked_c32(c.handle, C.byref(model), C.c_uint64(seed), int(sweep_idx), int(trial0),
                                                   int(batch), int(frame), float(corr), C.byref(tr), _lib.DEVICE)
        _lib.check(rc, "jstsp_build_trials_tracked_c32")
    elif channel is None:
        rc = c._lib.jstsp_build_trials_c32(c.handle, C.byref(model), C.c_uint64(seed), int(sweep_idx), int(trial0),
                                           int(batch), C.byref(tr), _lib.DEVICE)
        _lib.check(rc, "jstsp_build_trials_c32")
    else:
        src = _channel_on_device(channel, device)
        mode = _CHANNEL_NORMALIZE[channel_normalize]
        sig = None
        if mode != _lib.CHAN_ASIS or min(p.Nr, p.Nt) <= 64:
            sig = np.empty((batch, p.L) if per_trial else (p.L,), dtype=np.float64)
        rc = c._lib.jstsp_build_trials_from_channel_c32(
            c.handle, C.byref(model), C.c_uint64(seed), int(sweep_idx), int(trial0), int(batch), src.data_ptr(), nr_src, nt_src,
            nr_src * nt_src * p.L if per_trial else 0, mode, C.byref(tr),
            sig.ctypes.data_as(C.POINTER(C.c_double)) if sig is not None else None, _lib.DEVICE)
        _lib.check(rc, "jstsp_build_trials_from_channel_c32")
        if sig is not None:
            out["sigma_max"] = torch.from_numpy(sig)
    out.update({k: torch.from_numpy(v) for k, v in hyp.items()})
    return out


def ase_trials(p: SweepParams, designs, trial0, batch, *, seed=20190913, sweep_idx=0, want_cols=False, device=None, ctx=None,
               shared_pilots=False, pilots="qam4"):
    """plot_capacity.m:35-64 / plot_ee.m:36-65 for trials [trial0, trial0 + batch) on the HIP path
    (``jstsp_ase_trials_c32``, csrc/capacity.hip): the achievable spectral efficiency of every combiner design on one
    realisation, ``real(log2(det(eye(Mr) + 1/(noise_var*Nt) W_c'*(Y*Y')*W_c)))`` with the noise-free ``Y`` of the frame
    ``p.T_prop``.  Trial t has the channel and pilots ``build_trials(p, ...)`` returns for t with the same seed, sweep index,
    ``shared_pilots`` and ``pilots`` (the drivers: fresh 4-QAM pilots per realisation, the defaults of both).

    ``designs``: (kind, n_cols, pool) per design, kind as ``solvers.beamformer``; pool = 0: the first n_cols columns
    (hbf.m:23), pool > 0: n_cols columns drawn per trial from the first pool (plot_capacity.m:63-64).
    Returns the float64 (batch, len(designs)) ASE on the device; with ``want_cols`` also the int32 (batch, sum of n_cols of
    the pool > 0 designs) 1-based subsets, design after design."""
    import ctypes as C
    from . import _lib
    from .solvers import _bf_kind
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    c = ctx if ctx is not None else _lib.default_context(device.index or 0)
    c.use_torch_stream()
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, 0, 1 if shared_pilots else 0,
                       p.noise_var, _lib.BF_ZC, _lib.RHO_MIN6, 1.0,
                       _lib.PILOTS_GAUSS if pilots == "gauss" else _lib.PILOTS_QAM4)
    ds = (_lib.AseDesign * len(designs))(*[_lib.AseDesign(_bf_kind(k), int(n), int(pool)) for k, n, pool in designs])
    n_sel = sum(int(n) for _, n, pool in designs if int(pool) > 0)
    out = torch.empty((batch, len(designs)), dtype=torch.float64, device=device)
    cols = torch.empty((batch, max(n_sel, 1)), dtype=torch.int32, device=device) if want_cols else None
    rc = c._lib.jstsp_ase_trials_c32(c.handle, C.byref(model), ds, len(designs), C.c_uint64(seed), int(sweep_idx),
                                     int(trial0), int(batch), out.data_ptr(), cols.data_ptr() if want_cols else None,
                                     _lib.DEVICE)
    _lib.check(rc, "jstsp_ase_trials_c32")
    return (out, cols[:, :n_sel]) if want_cols else out


def rank_trials(p: SweepParams, trial0, batch, *, seed=20190913, sweep_idx=0, n_keep=None, device=None, ctx=None,
                shared_pilots=False, pilots="qam4"):
    """plot_rankR.m:24-50 for trials [trial0, trial0 + batch) on the HIP path (``jstsp_rank_trials_c32``, csrc/svdvals.hip):
    the first ``n_keep`` singular values (default ``min(Nr, Mr_e, T_prop)``; the script keeps ``min(Nr, Mr_e)``) of the
    noise-free ``Y = sum_l H_l Psi_bar_l`` (Nr x ``p.T_prop``) of one realisation, by float64 one-sided Jacobi on ``Y`` itself.
    Trial t has the channel and pilots ``build_trials(p, ...)`` returns for t with the same seed, sweep index,
    ``shared_pilots`` and ``pilots``.  Returns float64 (batch, n_keep) on the device, descending per trial."""
    import ctypes as C
    from . import _lib
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    c = ctx if ctx is not None else _lib.default_context(device.index or 0)
    c.use_torch_stream()
    if n_keep is None:
        n_keep = min(p.Nr, p.Mr_e, p.T_prop)
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, 0, 1 if shared_pilots else 0,
                       p.noise_var, _lib.BF_ZC, _lib.RHO_MIN6, 1.0,
                       _lib.PILOTS_GAUSS if pilots == "gauss" else _lib.PILOTS_QAM4)
    out = torch.empty((batch, int(n_keep)), dtype=torch.float64, device=device)
    rc = c._lib.jstsp_rank_trials_c32(c.handle, C.byref(model), C.c_uint64(seed), int(sweep_idx), int(trial0), int(batch),
                                      int(n_keep), out.data_ptr(), _lib.DEVICE)
    _lib.check(rc, "jstsp_rank_trials_c32")
    return out


def spectrum_trials(p: SweepParams, trial0, batch, *, seed=20190913, sweep_idx=0, n_keep=None, channel=None,
                    channel_normalize="reference", device=None, ctx=None, shared_pilots=False, pilots="qam4", want_sigma=False):
    """:func:`rank_trials` at every driver size and on any channel (``jstsp_spectrum_trials_c32``, csrc/svdvals.hip): the first
    ``n_keep`` singular values of the noise-free ``Y`` (Nr x ``p.T_prop``) of trials [trial0, trial0 + batch), for
    ``min(Nr, T_prop) <= 64`` with ``max(Nr, T_prop) <= 65536`` (float64 Householder tall-skinny QR in front of the Jacobi) or
    ``min <= 512`` with ``max <= 8192`` (the global-memory Jacobi); on the shapes ``rank_trials`` accepts, its bits.

    ``channel``, ``channel_normalize``: as in :func:`build_trials` - trial t then has the channel and pilots
    ``build_trials(p, ..., channel=channel)`` returns for t, and ``p.clusters`` / ``p.rays`` are not used.  ``want_sigma`` (with a
    channel) returns ``(sv, sigma_max)``, the float64 norm(H_l) per tap as ``build_trials`` reports it.
    Returns float64 (batch, n_keep) on the device, descending per trial."""
    import ctypes as C
    import numpy as np
    from . import _lib
    if channel is not None:
        per_trial, nr_src, nt_src = _check_channel(p, batch, channel, channel_normalize)
    elif want_sigma:
        raise ValueError("want_sigma needs a supplied channel")
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    c = ctx if ctx is not None else _lib.default_context(device.index or 0)
    c.use_torch_stream()
    if n_keep is None:
        n_keep = min(p.Nr, p.Mr_e, p.T_prop)
    model = _lib.Model(p.Nt, p.Nr, p.L, p.T_prop, p.Mr, p.Mr_e, p.Gr, p.Gt, p.clusters, p.rays, 0, 1 if shared_pilots else 0,
                       p.noise_var, _lib.BF_ZC, _lib.RHO_MIN6, 1.0,
                       _lib.PILOTS_GAUSS if pilots == "gauss" else _lib.PILOTS_QAM4)
    out = torch.empty((batch, int(n_keep)), dtype=torch.float64, device=device)
    src, sig, ld, stride, mode = None, None, (0, 0), 0, 0
    if channel is not None:
        src = _channel_on_device(channel, device)
        mode = _CHANNEL_NORMALIZE[channel_normalize]
        ld, stride = (nr_src, nt_src), nr_src * nt_src * p.L if per_trial else 0
        if want_sigma:
            sig = np.empty((batch, p.L) if per_trial else (p.L,), dtype=np.float64)
    rc = c._lib.jstsp_spectrum_trials_c32(c.handle, C.byref(model), C.c_uint64(seed), int(sweep_idx), int(trial0), int(batch),
                                          src.data_ptr() if src is not None else None, ld[0], ld[1], stride, mode, int(n_keep),
                                          out.data_ptr(), sig.ctypes.data_as(C.POINTER(C.c_double)) if sig is not None else None,
                                          _lib.DEVICE)
    _lib.check(rc, "jstsp_spectrum_trials_c32")
    return (out, torch.from_numpy(sig)) if want_sigma else out
