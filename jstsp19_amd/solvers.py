"""Host-side mirror of the reference's solver functions on top of the C ABI.

Same names, argument order and meaning as the MATLAB functions they replace:

    [S, Y, convergence_error] = proposed_algorithm(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type)
    [S, Y, convergence_error] = proposed_algorithm_angles(subY, Omega, indx_S, A, B, Imax, tau_Y, tau_S, rho, type, greedy_nnz)
    [x_hat, indexSet, v, targetMatrix] = OMP(A, v, m, snr)
    [S, convergence_error] = sparse_admm(Htrue, OH, Dr, Dt, Imax)
    X = svt(Y, tau);  X = mc_svt(OH, Omega, Imax, tau, rho);  [X, ce] = mc_admm(Htrue, OH, Omega, Imax, tau, rho)

Array arguments are numpy arrays (host: the library copies over PCIe) or torch CUDA tensors
(device-resident, asynchronous on torch's current stream).  A leading batch dimension stacks
independent problems: ``subY`` is (N, M) or (batch, N, M); a 2-D ``A``/``B`` with batched
``subY`` means one dictionary shared by the batch.  The C ABI is column-major; numpy inputs
are re-laid-out here, torch inputs must already be column-major per problem
(``colmajor(t)``: stride (R*C, 1, R)) so that nothing is copied on the device.

All compute happens in libjstsp_mi355x.so; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import DEVICE, HOST, JstspError, check

__all__ = ["proposed_algorithm", "proposed_algorithm_angles", "svt", "mc_svt", "mc_admm", "OMP", "omp_kron",
           "sparse_admm", "vamp", "vamp_kron", "cosamp", "cosamp_kron", "sparse_sca_estim", "cawgn_estim_out", "ls_estimate", "pinv", "mmv_omp", "tssr", "rate", "correlate", "synthesize", "gradient_head", "nmse_spectral", "colmajor",
           "empty_colmajor", "beamformer", "ase", "singular_values", "spectrum",
           "proposed_algorithm_f64", "proposed_algorithm_angles_f64", "svt_f64", "correlate_f64", "synthesize_f64",
           "pinv_f64", "ls_estimate_f64", "mmv_omp_f64", "mc_svt_f64", "mc_admm_f64", "tssr_f64",
           "OMP_f64", "omp_kron_f64", "sparse_admm_f64", "proposed_algorithm_std_f64", "proposed_algorithm_angles_std_f64",
           "svd_f64", "lowrank_f64", "svd_tall_f64", "lowrank_tall_f64", "nmse_spectral_f64", "rate_f64",
           "admm_state_elems", "proposed_algorithm_resume_f64", "proposed_algorithm_std_resume_f64",
           "proposed_algorithm_resume", "proposed_algorithm_angles_resume", "support_order", "support_order_f64",
           "support_order_wide", "support_order_wide_f64", "support_top_f64", "proposed_algorithm_refresh_f64",
           "support_top", "proposed_algorithm_refresh", "refit_f64"]


# ----------------------------------------------------------------------------- array plumbing
def _is_torch(x):
    return type(x).__module__.startswith("torch")


def colmajor(t):
    """Return a torch tensor with the same logical shape (..., R, C) whose last two dims are
    stored column-major (stride (..., 1, R)) — the layout the C ABI expects."""
    return t.transpose(-1, -2).contiguous().transpose(-1, -2)


def empty_colmajor(batch, R, C_, dtype, device):
    import torch
    return torch.empty((batch, C_, R), dtype=dtype, device=device).transpose(1, 2)


class _Arg:
    """A matrix argument normalised to (batch, R, C) + pointer in the C ABI's layout."""

    def __init__(self, x, np_dtype, name, allow_none=False):
        self.keep = None
        self.name = name
        if x is None:
            if not allow_none:
                raise ValueError("%s is required" % name)
            self.ptr, self.batch, self.R, self.C, self.torch, self.batched = None, 0, 0, 0, False, False
            return
        self.torch = _is_torch(x)
        self.batched = x.ndim == 3
        if x.ndim not in (2, 3):
            raise ValueError("%s must be 2-D or 3-D (batch first), got shape %s" % (name, tuple(x.shape)))
        if self.torch:
            import torch
            want = {np.complex64: torch.complex64, np.complex128: torch.complex128, np.float32: torch.float32, np.float64: torch.float64,
                    np.int32: torch.int32}[np_dtype]
            if not x.is_cuda:
                raise ValueError("%s: torch tensors must live on the GPU (numpy arrays use the host path)" % name)
            if x.dtype != want:
                raise ValueError("%s: expected dtype %s, got %s" % (name, want, x.dtype))
            x3 = x if x.ndim == 3 else x.unsqueeze(0)
            b, R, Cc = x3.shape
            ok = (x3.stride(1) == 1 or R == 1) and (x3.stride(2) == R or Cc == 1) and (x3.stride(0) == R * Cc or b == 1)
            if not ok:
                raise ValueError("%s: device tensors must be column-major per problem "
                                 "(use jstsp19_amd.colmajor); strides %s" % (name, x3.stride()))
            self.keep = x3
            self.ptr = x3.data_ptr()
            self.device = x3.device
        else:
            x3 = np.asarray(x)
            x3 = x3 if x3.ndim == 3 else x3[None]
            b, R, Cc = x3.shape
            buf = np.ascontiguousarray(np.swapaxes(x3, 1, 2), dtype=np_dtype)     # [t][c][r]
            self.keep = buf
            self.ptr = buf.ctypes.data
        self.batch, self.R, self.C = int(b), int(R), int(Cc)


def _out(kind_torch, batch, R, Cc, np_dtype, device=None):
    """Allocate an output in the C ABI's layout; returns (ptr, finisher) where finisher(squeeze)
    gives the user-facing (batch, R, C) (or (R, C)) array."""
    if kind_torch:
        import torch
        td = {np.complex64: torch.complex64, np.complex128: torch.complex128, np.float32: torch.float32, np.float64: torch.float64,
              np.int32: torch.int32}[np_dtype]
        buf = torch.empty((batch, Cc, R), dtype=td, device=device)
        return buf.data_ptr(), (lambda sq: (buf.transpose(1, 2)[0] if sq else buf.transpose(1, 2)))
    buf = np.empty((batch, Cc, R), dtype=np_dtype)
    return buf.ctypes.data, (lambda sq: (np.swapaxes(buf, 1, 2)[0] if sq else np.swapaxes(buf, 1, 2)))


def _scalars(v, batch, name):
    a = np.asarray(v, dtype=np.float64).reshape(-1)
    if a.size == 1:
        a = np.full(batch, a[0], dtype=np.float64)
    a = np.ascontiguousarray(a)
    if a.size != batch:
        raise ValueError("%s must be a scalar or have one entry per problem (%d), got %d" % (name, batch, a.size))
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _ctx_for(args, ctx):
    tor = [a for a in args if a.ptr is not None and a.torch]
    npy = [a for a in args if a.ptr is not None and not a.torch]
    if tor and npy:
        raise ValueError("mixing numpy (host) and torch CUDA (device) array arguments is not supported")
    if tor:
        dev = tor[0].device.index or 0
        c = ctx or _lib.default_context(dev)
        c.use_torch_stream()
        return c, DEVICE, tor[0].device
    return ctx or _lib.default_context(0), HOST, None


def _shared_stride(arg, rows_cols, batch, name):
    if arg.batched:
        if arg.batch != batch:
            raise ValueError("%s has batch %d, expected %d" % (name, arg.batch, batch))
        return rows_cols
    return 0


# ----------------------------------------------------------------------------- proposed_algorithm
def _indx_arg(indx_S, batch, n):
    """indx_S (1-based linear indices, (n,) or (batch, n)) as a (batch, n, 1) int32 argument; ``None`` stays absent."""
    if indx_S is None:
        return _Arg(None, np.int32, "indx_S", allow_none=True)
    if _is_torch(indx_S):
        import torch
        ix2 = indx_S.reshape(batch, n, 1).to(torch.int32).contiguous()
    else:
        ix2 = np.asarray(indx_S).reshape(batch, n, 1).astype(np.int32)
    return _Arg(ix2, np.int32, "indx_S")


class _AdmmCall:
    """What every ``proposed_algorithm*`` call builds first, for the solver's complex dtype ``cdt`` (complex128: the inputs are widened).
    The constructor touches no device - the arguments and their shape checks, ``indx_S``, the strides of the dictionaries, the
    per-trial scalars - so every ``ValueError`` of the arguments comes before the context; :meth:`open` makes the context and the
    outputs ``S``, ``Y``, ``convergence_error``, :meth:`result` returns them to the caller."""

    def __init__(self, cdt, subY, Omega, A, B, indx_S, tau_Y, tau_S, rho, Imax, PA=None, PB=None):
        f64 = cdt == np.complex128
        wide = _wide if f64 else (lambda x, real=False: x)
        self.cdt = cdt
        self.sub = _Arg(wide(subY), cdt, "subY")
        self.om = _Arg(wide(Omega, real=True), np.float64 if f64 else np.float32, "Omega")
        self.A = _Arg(wide(A), cdt, "A")
        self.B = _Arg(wide(B), cdt, "B")
        self.PA = _Arg(wide(PA), cdt, "PA", allow_none=True)
        self.PB = _Arg(wide(PB), cdt, "PB", allow_none=True)
        self.batch, self.N, self.M = batch, N, M = self.sub.batch, self.sub.R, self.sub.C
        self.Gr, self.G2 = Gr, G2 = self.A.C, self.B.R
        self.Imax = int(Imax)
        if (self.om.batch, self.om.R, self.om.C) != (batch, N, M):
            raise ValueError("Omega must have the shape of subY")
        if self.A.R != N or self.B.C != M:
            raise ValueError("size(A,1) must equal size(subY,1) and size(B,2) must equal size(subY,2)")
        for a_P, a_F, nmP in ((self.PA, self.A, "PA"), (self.PB, self.B, "PB")):
            if a_P.ptr is not None and ((a_P.R, a_P.C) != (a_F.C, a_F.R) or a_P.batched != a_F.batched or a_P.batch != a_F.batch):
                raise ValueError("%s must have the shape of pinv(%s), batched as %s is" % (nmP, nmP[1], nmP[1]))
        self.ix = _indx_arg(indx_S, batch, Gr * G2)
        self.sA = _shared_stride(self.A, N * Gr, batch, "A")
        self.sB = _shared_stride(self.B, G2 * M, batch, "B")
        self.tY, self.ptY = _scalars(tau_Y, batch, "tau_Y")
        self.tS, self.ptS = _scalars(tau_S, batch, "tau_S")
        self.rh, self.prh = _scalars(rho, batch, "rho")
        # where a state of this call lives (:func:`_state_arg`), known before the context
        self.state_mem, self.state_dev = DEVICE if self.sub.torch else HOST, getattr(self.sub, "device", None)

    def open(self, want_ce, ctx):
        self.ctx, self.mem, self.dev = _ctx_for([self.sub, self.om, self.A, self.B, self.PA, self.PB, self.ix], ctx)
        tor = self.mem == DEVICE
        self.pS, fS = _out(tor, self.batch, self.Gr, self.G2, self.cdt, self.dev)
        self.pY, fY = _out(tor, self.batch, self.N, self.M, self.cdt, self.dev)
        self.pce, fce = _out(tor, self.batch, self.Imax, 3, np.float64, self.dev) if want_ce else (None, None)
        self._finish = (fS, fY, fce)

    def c32_args(self, type):
        """the argument list that the three fp32 entries share: the context's handle ... ce_out"""
        tcode = _lib.TYPE_APPROXIMATE if type == "approximate" else _lib.TYPE_STD
        return (self.ctx.handle, self.N, self.M, self.Gr, self.G2, self.batch, self.sub.ptr, self.om.ptr, self.A.ptr, self.sA, self.B.ptr, self.sB,
                self.Imax, self.ptY, self.ptS, self.prh, tcode, self.ix.ptr, self.pS, self.pY, self.pce)

    def result(self):
        sq = not self.sub.batched
        return tuple(None if f is None else f(sq) for f in self._finish)


def proposed_algorithm(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type="approximate", *, indx_S=None,
                       want_ce=True, ctx=None):
    """basic_system_functions/proposed_algorithm.m:1 — returns (S, Y, convergence_error).

    ``convergence_error`` is (batch, Imax, 3) float64 (``None`` with ``want_ce=False``, the
    analogue of calling the MATLAB function with fewer than three outputs).
    """
    q = _AdmmCall(np.complex64, subY, Omega, A, B, indx_S, tau_Y, tau_S, rho, Imax)
    q.open(want_ce, ctx)
    check(q.ctx._lib.jstsp_proposed_algorithm_c32(*q.c32_args(type), q.mem), "jstsp_proposed_algorithm_c32")
    return q.result()


def proposed_algorithm_resume(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type="approximate", *, indx_S=None, want_ce=True, ctx=None,
                              state=None, it0=0, return_state=True):
    """:func:`proposed_algorithm` resumed from a saved state (include/jstsp.h: jstsp_proposed_resume_c32): iterations
    ``it0 + 1 ... it0 + Imax`` of the reference loop from ``state``.  Returns ``(S, Y, ce, state)``; ``ce`` holds the rows of this
    call, ``state`` is complex64 ``(batch, admm_state_elems(N, M, Gr, G2))`` (always two-dimensional; ``None`` with
    ``return_state=False``), a new array of the kind of the inputs.  ``state=None``: from zero (``it0`` must be 0).  A split fp32
    solve is fp32-equivalent to the uninterrupted one, not bit-identical (the header says what is not carried)."""
    q = _AdmmCall(np.complex64, subY, Omega, A, B, indx_S, tau_Y, tau_S, rho, Imax)
    it0 = int(it0)
    if type not in ("approximate", "std"):
        raise ValueError("type must be 'approximate' or 'std'")
    if it0 < 0 or (state is None and it0 != 0):
        raise ValueError("it0 must be >= 0, and 0 when there is no state to start from")
    ne = admm_state_elems(q.N, q.M, q.Gr, q.G2)
    p_in, keep_in = _state_arg(state, q.batch, ne, q.state_mem, q.state_dev, np.complex64)
    q.open(want_ce, ctx)
    p_out, st_out = _state_out(return_state, q.batch, ne, q.mem, q.dev, np.complex64)
    check(q.ctx._lib.jstsp_proposed_resume_c32(*q.c32_args(type), it0, p_in, p_out, q.mem), "jstsp_proposed_resume_c32")
    del keep_in
    return q.result() + (st_out,)


def proposed_algorithm_angles_resume(subY, Omega, indx_S, A, B, Imax, tau_Y, tau_S, rho, type="approximate", greedy_nnz=None, *,
                                     want_ce=True, ctx=None, state=None, it0=0, return_state=True):
    """:func:`proposed_algorithm_angles` resumed from a saved state (see :func:`proposed_algorithm_resume`): the mask of the call's
    iteration ``it`` has ``min(10 + 5 (it0 + it), Gr G2)`` entries."""
    return proposed_algorithm_resume(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S=indx_S, want_ce=want_ce, ctx=ctx, state=state,
                                     it0=it0, return_state=return_state)


class PendingSolve:
    """Handle of :func:`proposed_algorithm_begin`: the solve is running on the context's stream; :meth:`end` completes it and
    returns ``(S, Y, convergence_error)``.  Keeps every array of the call alive until then."""

    def __init__(self, ctx, handle, keep, result):
        self._ctx, self._h, self._keep, self._result = ctx, handle, keep, result
        self.fallbacks = None

    def end(self):
        if self._h is None:
            raise JstspError("this solve has already been completed")
        n = C.c_int(0)
        h, self._h = self._h, None
        check(self._ctx._lib.jstsp_proposed_algorithm_end(self._ctx.handle, h, C.byref(n)), "jstsp_proposed_algorithm_end")
        self.fallbacks = int(n.value)
        self._keep = None
        return self._result


def proposed_algorithm_begin(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type="approximate", *, indx_S=None, want_ce=True,
                             ctx=None):
    """The two-phase form of :func:`proposed_algorithm` for torch CUDA tensors (include/jstsp.h:
    jstsp_proposed_algorithm_begin_c32 / _end): enqueues the solve and returns a :class:`PendingSolve` without waiting for the
    GPU; ``handle.end()`` returns the outputs.  Between the two the host is free (e.g. to build the next batch)."""
    q = _AdmmCall(np.complex64, subY, Omega, A, B, indx_S, tau_Y, tau_S, rho, Imax)
    q.open(want_ce, ctx)
    if q.mem != DEVICE:
        raise ValueError("proposed_algorithm_begin takes torch CUDA tensors (a host call has nothing to overlap: use proposed_algorithm)")
    h = C.c_void_p()
    check(q.ctx._lib.jstsp_proposed_algorithm_begin_c32(*q.c32_args(type), C.byref(h)), "jstsp_proposed_algorithm_begin_c32")
    return PendingSolve(q.ctx, h, (q.sub, q.om, q.A, q.B, q.ix, q.tY, q.tS, q.rh), q.result())


def proposed_algorithm_angles(subY, Omega, indx_S, A, B, Imax, tau_Y, tau_S, rho, type="approximate",
                              greedy_nnz=None, *, want_ce=True, ctx=None):
    """basic_system_functions/proposed_algorithm_angles.m:1 (``greedy_nnz`` is unused there too).
    ``indx_S``: 1-based column-major linear indices, (Gr*G2,) or (batch, Gr*G2)."""
    return proposed_algorithm(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S=indx_S,
                              want_ce=want_ce, ctx=ctx)


# ----------------------------------------------------------------------------- kernel level
def correlate(K, A, B, *, ctx=None):
    """``A' * K * B'`` (Gr x G2) — ``K2'*k`` of proposed_algorithm.m:47 in structured form."""
    a_K, a_A, a_B = _Arg(K, np.complex64, "K"), _Arg(A, np.complex64, "A"), _Arg(B, np.complex64, "B")
    batch, N, M, Gr, G2 = a_K.batch, a_K.R, a_K.C, a_A.C, a_B.R
    if a_A.R != N or a_B.C != M:
        raise ValueError("shape mismatch")
    c, mem, dev = _ctx_for([a_K, a_A, a_B], ctx)
    p, f = _out(mem == DEVICE, batch, Gr, G2, np.complex64, dev)
    check(c._lib.jstsp_correlate_c32(c.handle, N, M, Gr, G2, batch, a_K.ptr, a_A.ptr,
                                     _shared_stride(a_A, N * Gr, batch, "A"), a_B.ptr,
                                     _shared_stride(a_B, G2 * M, batch, "B"), p, mem), "jstsp_correlate_c32")
    return f(not a_K.batched)


def synthesize(S, A, B, *, ctx=None):
    """``A * S * B`` (N x M) — ``K2*s`` of proposed_algorithm.m:38,58."""
    a_S, a_A, a_B = _Arg(S, np.complex64, "S"), _Arg(A, np.complex64, "A"), _Arg(B, np.complex64, "B")
    batch, Gr, G2, N, M = a_S.batch, a_S.R, a_S.C, a_A.R, a_B.C
    if a_A.C != Gr or a_B.R != G2:
        raise ValueError("shape mismatch")
    c, mem, dev = _ctx_for([a_S, a_A, a_B], ctx)
    p, f = _out(mem == DEVICE, batch, N, M, np.complex64, dev)
    check(c._lib.jstsp_synthesize_c32(c.handle, N, M, Gr, G2, batch, a_S.ptr, a_A.ptr,
                                      _shared_stride(a_A, N * Gr, batch, "A"), a_B.ptr,
                                      _shared_stride(a_B, G2 * M, batch, "B"), p, mem), "jstsp_synthesize_c32")
    return f(not a_S.batched)


def gradient_head(Tc, A, GA, RV=None, *, ctx=None):
    """``Res = A'*Tc - RV`` and ``P1 = GA*Res`` (Gr x G2 each) — the 64-term products of the gradient step,
    proposed_algorithm.m:47-48, as the solver forms them (N = Gr = 64, G2 a multiple of 64)."""
    a_T, a_A, a_G = _Arg(Tc, np.complex64, "Tc"), _Arg(A, np.complex64, "A"), _Arg(GA, np.complex64, "GA")
    a_R = _Arg(RV, np.complex64, "RV", allow_none=True)
    batch, N, G2, Gr = a_T.batch, a_T.R, a_T.C, a_A.C
    if a_A.R != N or (a_G.R, a_G.C) != (Gr, Gr) or (RV is not None and (a_R.batch, a_R.R, a_R.C) != (batch, Gr, G2)):
        raise ValueError("shape mismatch")
    c, mem, dev = _ctx_for([a_T, a_A, a_G, a_R], ctx)
    pr, fr = _out(mem == DEVICE, batch, Gr, G2, np.complex64, dev)
    pp, fp = _out(mem == DEVICE, batch, Gr, G2, np.complex64, dev)
    check(c._lib.jstsp_gradient_head_c32(c.handle, N, Gr, G2, batch, a_T.ptr, a_A.ptr, _shared_stride(a_A, N * Gr, batch, "A"),
                                         a_G.ptr, _shared_stride(a_G, Gr * Gr, batch, "GA"), a_R.ptr, pr, pp, mem),
          "jstsp_gradient_head_c32")
    return fr(not a_T.batched), fp(not a_T.batched)


def ls_estimate(Y, A, B, *, ctx=None):
    """``pinv(A)*Y*pinv(B)`` — the LS baseline of plot_errorVSsnr.m:83 (SVD-based float64 pinv of every factor that
    fits the in-LDS kernel; the fp32 Gram inverse with a conditioning check for larger, full-rank factors)."""
    a_Y, a_A, a_B = _Arg(Y, np.complex64, "Y"), _Arg(A, np.complex64, "A"), _Arg(B, np.complex64, "B")
    batch, N, M, Gr, G2 = a_Y.batch, a_Y.R, a_Y.C, a_A.C, a_B.R
    if a_A.R != N or a_B.C != M:
        raise ValueError("shape mismatch")
    c, mem, dev = _ctx_for([a_Y, a_A, a_B], ctx)
    p, f = _out(mem == DEVICE, batch, Gr, G2, np.complex64, dev)
    check(c._lib.jstsp_ls_c32(c.handle, N, M, Gr, G2, batch, a_Y.ptr, a_A.ptr, _shared_stride(a_A, N * Gr, batch, "A"),
                              a_B.ptr, _shared_stride(a_B, G2 * M, batch, "B"), p, mem), "jstsp_ls_c32")
    return f(not a_Y.batched)


def pinv(A, *, ctx=None):
    """MATLAB's ``pinv(A)`` as the drivers call it (plot_errorVSsnr.m:83): SVD-based, float64 on the device,
    singular values below ``max(size(A))*eps(norm(A))`` dropped.  ``A``: (rows, cols) or (batch, rows, cols)."""
    a_A = _Arg(A, np.complex64, "A")
    c, mem, dev = _ctx_for([a_A], ctx)
    p, f = _out(mem == DEVICE, a_A.batch, a_A.C, a_A.R, np.complex64, dev)
    check(c._lib.jstsp_pinv_c32(c.handle, a_A.R, a_A.C, a_A.batch, a_A.ptr, p, mem), "jstsp_pinv_c32")
    return f(not a_A.batched)


def svt(Y, tau, *, ctx=None):
    """benchmark_algorithms/svt.m:1 — singular-value soft threshold."""
    a_Y = _Arg(Y, np.complex64, "Y")
    c, mem, dev = _ctx_for([a_Y], ctx)
    t, pt = _scalars(tau, a_Y.batch, "tau")
    p, f = _out(mem == DEVICE, a_Y.batch, a_Y.R, a_Y.C, np.complex64, dev)
    check(c._lib.jstsp_svt_c32(c.handle, a_Y.R, a_Y.C, a_Y.batch, a_Y.ptr, pt, p, mem), "jstsp_svt_c32")
    return f(not a_Y.batched)


def nmse_spectral(S, Zbar, *, ctx=None):
    """plot_errorVSsnr.m:138-141 — ``min(1, norm(S-Zbar)^2/norm(Zbar)^2)`` with spectral norms."""
    a_S, a_Z = _Arg(S, np.complex64, "S"), _Arg(Zbar, np.complex64, "Zbar")
    if (a_S.batch, a_S.R, a_S.C) != (a_Z.batch, a_Z.R, a_Z.C):
        raise ValueError("S and Zbar must have the same shape")
    c, mem, dev = _ctx_for([a_S, a_Z], ctx)
    if mem == DEVICE:
        import torch
        out = torch.empty(a_S.batch, dtype=torch.float64, device=dev)
        ptr = out.data_ptr()
    else:
        out = np.empty(a_S.batch, dtype=np.float64)
        ptr = out.ctypes.data
    check(c._lib.jstsp_nmse_spectral_c32(c.handle, a_S.R, a_S.C, a_S.batch, a_S.ptr, a_Z.ptr, ptr, mem),
          "jstsp_nmse_spectral_c32")
    return out if a_S.batched else out[0]


def lambda_max_sequence(G, *, ctx=None):
    """``lambda_max`` of a sequence of batches of Hermitian matrices, ``G``: (steps, batch, n, n) numpy complex64 (each matrix
    column-major = its transpose in C order; Hermitian, so the conjugate).  Matrix t of step s is warm-started from matrix t of
    step s - 1 — the kernel behind ``convergence_error(:,1:2)`` (proposed_algorithm.m:67,69) as the ADMM loops drive it.
    Returns (steps, batch) float32."""
    G = np.asarray(G)
    if G.ndim != 4 or G.shape[2] != G.shape[3]:
        raise ValueError("G must be (steps, batch, n, n)")
    steps, batch, n, _ = G.shape
    Gc = np.ascontiguousarray(np.swapaxes(G, 2, 3).astype(np.complex64))        # column-major matrices
    c = ctx if ctx is not None else _lib.default_context(0)
    out = np.empty((steps, batch), dtype=np.float32)
    check(c._lib.jstsp_lambda_max_sequence_c32(c.handle, n, batch, steps, Gc.ctypes.data, out.ctypes.data, HOST),
          "jstsp_lambda_max_sequence_c32")
    return out


def rate(S, Zbar, noise_var, *, ctx=None):
    """plot_rateVSframelength.m:81,113,130,135 — ``log2(real(det(eye(Nr) + 1/Nr*Zbar*Zbar'/(noise_var + nmse))))`` with
    the (uncapped) spectral-norm NMSE of ``S``."""
    a_S, a_Z = _Arg(S, np.complex64, "S"), _Arg(Zbar, np.complex64, "Zbar")
    if (a_S.batch, a_S.R, a_S.C) != (a_Z.batch, a_Z.R, a_Z.C):
        raise ValueError("S and Zbar must have the same shape")
    c, mem, dev = _ctx_for([a_S, a_Z], ctx)
    if mem == DEVICE:
        import torch
        out = torch.empty(a_S.batch, dtype=torch.float64, device=dev)
        ptr = out.data_ptr()
    else:
        out = np.empty(a_S.batch, dtype=np.float64)
        ptr = out.ctypes.data
    check(c._lib.jstsp_rate_c32(c.handle, a_S.R, a_S.C, a_S.batch, a_S.ptr, a_Z.ptr, float(noise_var), ptr, mem),
          "jstsp_rate_c32")
    return out if a_S.batched else out[0]


def mmv_omp(A, Y, K, *, norm="l2", ctx=None):
    """Joint (MMV) OMP — ``spx.pursuit.joint.OrthogonalMatchingPursuit(A, K).solve(Y).Z`` of the drivers
    (plot_errorVSsnr.m:116-117; sparse-plex is un-vendored and unpinned: the published simultaneous OMP, atom score
    ``||A(:,g)'*R||_2`` or ``_1``).  ``A``: (N, Gr) or (batch, N, Gr); ``Y``: (N, S) or (batch, N, S).
    Returns (Z (Gr, S), support (1-based atoms in selection order, 0 beyond the count), count)."""
    a_A, a_Y = _Arg(A, np.complex64, "A"), _Arg(Y, np.complex64, "Y")
    batch, N, S, Gr = a_Y.batch, a_Y.R, a_Y.C, a_A.C
    if a_A.R != N:
        raise ValueError("size(A,1) must equal size(Y,1)")
    c, mem, dev = _ctx_for([a_A, a_Y], ctx)
    pz, fz = _out(mem == DEVICE, batch, Gr, S, np.complex64, dev)
    pi, fi = _out(mem == DEVICE, batch, int(K), 1, np.int32, dev)
    pc, fc = _out(mem == DEVICE, batch, 1, 1, np.int32, dev)
    check(c._lib.jstsp_mmv_omp_c32(c.handle, N, Gr, S, batch, a_A.ptr, _shared_stride(a_A, N * Gr, batch, "A"), a_Y.ptr,
                                   int(K), 1 if norm == "l1" else 2, pz, pi, pc, mem), "jstsp_mmv_omp_c32")
    sq = not a_Y.batched
    return fz(sq), fi(sq)[..., 0], fc(sq)[..., 0, 0]


def tssr(Y_prop, Omega, A, B, Imax, tau, rho, K, *, norm="l2", ctx=None):
    """The drivers' two-stage TSSR baseline (plot_errorVSsnr.m:151,158-162, a commented recipe): matrix completion by
    ``mc_svt`` followed by joint OMP on ``Y_svt*pinv(B)`` with the dictionary ``A``.  Returns (S_tssr, Y_svt, S_svt) with
    ``S_svt = pinv(A)*Y_svt*pinv(B)`` the "SVT-based" estimate of :151-152."""
    Y_svt = mc_svt(Y_prop, Omega, Imax, tau, rho, ctx=ctx)
    PB = pinv(B, ctx=ctx)
    # Y_svt*pinv(B) and pinv(A)*(...): both on the library's synthesis kernel (A*S*B with one factor the identity)
    n = Y_svt.shape[-2]
    if _is_torch(Y_svt):
        import torch
        eye = colmajor(torch.eye(n, dtype=torch.complex64, device=Y_svt.device))
    else:
        eye = np.eye(n, dtype=np.complex64)
    T = synthesize(Y_svt, eye, PB, ctx=ctx)
    S_svt = ls_estimate(Y_svt, A, B, ctx=ctx)             # pinv(A)*Y_svt*pinv(B)  (:151)
    Z, _, _ = mmv_omp(A, T, K, norm=norm, ctx=ctx)
    return Z, Y_svt, S_svt


def mc_svt(OH, Omega, Imax, tau, rho, *, ctx=None):
    """benchmark_algorithms/mc_svt.m:1."""
    a_O, a_om = _Arg(OH, np.complex64, "OH"), _Arg(Omega, np.float32, "Omega")
    c, mem, dev = _ctx_for([a_O, a_om], ctx)
    t, pt = _scalars(tau, a_O.batch, "tau")
    r, pr = _scalars(rho, a_O.batch, "rho")
    p, f = _out(mem == DEVICE, a_O.batch, a_O.R, a_O.C, np.complex64, dev)
    check(c._lib.jstsp_mc_svt_c32(c.handle, a_O.R, a_O.C, a_O.batch, a_O.ptr, a_om.ptr, int(Imax), pt, pr, p,
                                  mem), "jstsp_mc_svt_c32")
    return f(not a_O.batched)


def mc_admm(Htrue, OH, Omega, Imax, tau, rho, *, want_ce=True, ctx=None):
    """benchmark_algorithms/mc_admm.m:1 — returns (X, convergence_error (batch, Imax))."""
    a_H = _Arg(Htrue, np.complex64, "Htrue", allow_none=not want_ce)
    a_O, a_om = _Arg(OH, np.complex64, "OH"), _Arg(Omega, np.float32, "Omega")
    c, mem, dev = _ctx_for([a_H, a_O, a_om], ctx)
    t, pt = _scalars(tau, a_O.batch, "tau")
    r, pr = _scalars(rho, a_O.batch, "rho")
    p, f = _out(mem == DEVICE, a_O.batch, a_O.R, a_O.C, np.complex64, dev)
    if want_ce:
        pce, fce = _out(mem == DEVICE, a_O.batch, int(Imax), 1, np.float64, dev)
    else:
        pce, fce = None, None
    check(c._lib.jstsp_mc_admm_c32(c.handle, a_O.R, a_O.C, a_O.batch, a_H.ptr, a_O.ptr, a_om.ptr, int(Imax), pt,
                                   pr, p, pce, mem), "jstsp_mc_admm_c32")
    sq = not a_O.batched
    ce = None
    if want_ce:
        ce = fce(sq)
        ce = ce[..., 0]
    return f(sq), ce


def sparse_admm(Htrue, OH, Dr, Dt, Imax, *, want_ce=True, ctx=None):
    """benchmark_algorithms/sparse_admm.m:1 — returns (S, convergence_error (batch, Imax))."""
    a_H = _Arg(Htrue, np.complex64, "Htrue", allow_none=not want_ce)
    a_O = _Arg(OH, np.complex64, "OH")
    a_Dr, a_Dt = _Arg(Dr, np.complex64, "Dr"), _Arg(Dt, np.complex64, "Dt")
    if a_Dr.batched or a_Dt.batched:
        raise ValueError("Dr and Dt are shared by the batch (2-D)")
    c, mem, dev = _ctx_for([a_H, a_O, a_Dr, a_Dt], ctx)
    p, f = _out(mem == DEVICE, a_O.batch, a_O.R, a_O.C, np.complex64, dev)
    if want_ce:
        pce, fce = _out(mem == DEVICE, a_O.batch, int(Imax), 1, np.float64, dev)
    else:
        pce, fce = None, None
    check(c._lib.jstsp_sparse_admm_c32(c.handle, a_O.R, a_O.C, a_Dr.C, a_Dt.C, a_O.batch, a_H.ptr, a_O.ptr,
                                       a_Dr.ptr, a_Dt.ptr, int(Imax), p, pce, mem), "jstsp_sparse_admm_c32")
    sq = not a_O.batched
    return f(sq), (fce(sq)[..., 0] if want_ce else None)


def OMP(A, v, m, snr=None, *, want_target=True, ctx=None):
    """benchmark_algorithms/OMP.m:1 — returns (x_hat, indexSet, v, targetMatrix).

    ``A``: (measures, size_d) or (batch, measures, size_d); ``v``: (measures,) or (batch, measures).
    ``indexSet`` is an int32 array of 1-based atom indices (the reference's 1 x m cell).
    ``snr`` is accepted and ignored, as in the reference."""
    a_A = _Arg(A, np.complex64, "A")
    tor = _is_torch(v)
    single = v.ndim == 1
    v3 = (v.reshape(1, -1, 1) if single else v.reshape(v.shape[0], -1, 1))
    if tor:
        v3 = colmajor(v3)
    a_v = _Arg(v3, np.complex64, "v")
    batch, meas, size_d = a_v.batch, a_A.R, a_A.C
    if a_v.R != meas:
        raise ValueError("length(v) must equal size(A,1)")
    c, mem, dev = _ctx_for([a_A, a_v], ctx)
    px, fx = _out(mem == DEVICE, batch, size_d, 1, np.complex64, dev)
    pi, fi = _out(mem == DEVICE, batch, int(m), 1, np.int32, dev)
    if want_target:
        pt, ft = _out(mem == DEVICE, batch, meas, int(m), np.complex64, dev)
    else:
        pt, ft = None, None
    check(c._lib.jstsp_omp_c32(c.handle, meas, size_d, batch, a_A.ptr, _shared_stride(a_A, meas * size_d, batch, "A"),
                               a_v.ptr, int(m), px, pi, pt, mem), "jstsp_omp_c32")
    x = fx(single)[..., 0]
    idx = fi(single)[..., 0]
    return x, idx, v, (ft(single) if want_target else None)


def omp_kron(Af, Bf, y, m, *, ctx=None):
    """OMP.m on the Kronecker dictionary ``kron(Bf.', Af)`` given by its factors (never formed;
    plot_errorVSdelays.m:77 builds the dictionary this way).  ``y``: (N*M,) or (batch, N*M) in
    column-major vec order.  Returns (x_hat (Gr*G2), indexSet (1-based))."""
    a_A, a_B = _Arg(Af, np.complex64, "Af"), _Arg(Bf, np.complex64, "Bf")
    tor = _is_torch(y)
    single = y.ndim == 1
    y3 = (y.reshape(1, -1, 1) if single else y.reshape(y.shape[0], -1, 1))
    if tor:
        y3 = colmajor(y3)
    a_y = _Arg(y3, np.complex64, "y")
    batch, N, Gr, G2, M = a_y.batch, a_A.R, a_A.C, a_B.R, a_B.C
    if a_y.R != N * M:
        raise ValueError("length(y) must be N*M")
    c, mem, dev = _ctx_for([a_A, a_B, a_y], ctx)
    px, fx = _out(mem == DEVICE, batch, Gr * G2, 1, np.complex64, dev)
    pi, fi = _out(mem == DEVICE, batch, int(m), 1, np.int32, dev)
    check(c._lib.jstsp_omp_kron_c32(c.handle, N, M, Gr, G2, batch, a_A.ptr, _shared_stride(a_A, N * Gr, batch, "Af"),
                                    a_B.ptr, _shared_stride(a_B, G2 * M, batch, "Bf"), a_y.ptr, int(m), px, pi, mem),
          "jstsp_omp_kron_c32")
    return fx(single)[..., 0], fi(single)[..., 0]


def _cosamp_call(kron, mats, y, K, iters, tol, ctx):
    f64 = all(_is_c128(m) for m in mats) and _is_c128(y)
    cdt = np.complex128 if f64 else np.complex64
    a_m = [_Arg(m, cdt, n) for m, n in zip(mats, ("Af", "Bf") if kron else ("Phi",))]
    tor = _is_torch(y)
    single = y.ndim == 1
    y3 = (y.reshape(1, -1, 1) if single else y.reshape(y.shape[0], -1, 1))
    if tor:
        y3 = colmajor(y3)
    a_y = _Arg(y3, cdt, "y")
    batch, K = a_y.batch, int(K)
    if kron:
        N, Gr, G2, M = a_m[0].R, a_m[0].C, a_m[1].R, a_m[1].C
        meas, size_d = N * M, Gr * G2
    else:
        meas, size_d = a_m[0].R, a_m[0].C
    if a_y.R != meas:
        raise ValueError("length(y) must equal the number of rows of the dictionary (%d)" % meas)
    c, mem, dev = _ctx_for(a_m + [a_y], ctx)
    px, fx = _out(mem == DEVICE, batch, size_d, 1, cdt, dev)
    ps, fs = _out(mem == DEVICE, batch, max(K, 1), 1, np.int32, dev)
    pi, fi = _out(mem == DEVICE, batch, 1, 1, np.int32, dev)
    pr, fr = _out(mem == DEVICE, batch, 1, 1, np.float64, dev)
    pt, ft = _out(mem == DEVICE, batch, 1, 1, np.int32, dev)
    name = "jstsp_cosamp%s_%s" % ("_kron" if kron else "", "c64" if f64 else "c32")
    fn = getattr(c._lib, name)
    if kron:
        rc = fn(c.handle, N, M, Gr, G2, batch, a_m[0].ptr, _shared_stride(a_m[0], N * Gr, batch, "Af"), a_m[1].ptr,
                _shared_stride(a_m[1], G2 * M, batch, "Bf"), a_y.ptr, K, int(iters), float(tol), px, ps, pi, pr, pt, mem)
    else:
        rc = fn(c.handle, meas, size_d, batch, a_m[0].ptr, _shared_stride(a_m[0], meas * size_d, batch, "Phi"), a_y.ptr, K,
                int(iters), float(tol), px, ps, pi, pr, pt, mem)
    check(rc, name)
    return fx(single)[..., 0], {"support": fs(single)[..., 0], "iters": fi(single)[..., 0, 0], "resid": fr(single)[..., 0, 0],
                                "status": ft(single)[..., 0, 0]}


def cosamp(Phi, y, K, *, iters=12, tol=1e-6, info=False, ctx=None):
    """``x = CoSaMP(Phi, y, K)`` (plot_time_comparisions.m:96): the published algorithm (Needell & Tropp, Algorithm 1) as
    include/jstsp.h states it, float64 on the device whatever the input type.

    ``Phi``: (measures, size_d) or (batch, measures, size_d); ``y``: (measures,) or (batch, measures).  complex128 inputs
    take ``jstsp_cosamp_c64`` (float64 in and out), complex64 inputs ``jstsp_cosamp_c32`` (x rounded once to fp32).
    ``iters`` = 12 and ``tol`` = 1e-6 (stop when ||y - Phi x|| <= tol ||y||) are this library's choice: the driver passes
    neither.  ``iters`` is a definition, not a convergence guarantee: on the driver's own problem (512 x 512, K = 100) the
    float64 iteration does not settle (relative residual between 0.17 and 0.21 over 12 iterations).
    ``info=True`` also returns a dict: ``support`` (K, 1-based, ascending), ``iters``, ``resid``, ``status`` (1: the least
    squares met a rank-deficient Phi(:,T) and the problem kept its previous iterate)."""
    x, rec = _cosamp_call(False, [Phi], y, K, iters, tol, ctx)
    return (x, rec) if info else x


def cosamp_kron(Af, Bf, y, K, *, iters=12, tol=1e-6, info=False, ctx=None):
    """``cosamp`` on the Kronecker dictionary ``kron(Bf.', Af)`` given by its factors (never formed), conventions of
    ``omp_kron``: ``y`` (N*M,) or (batch, N*M) in column-major vec order, atoms indexed g + Gr*h.  The driver's dictionary is
    ``Af = A``, ``Bf = B*B'``, ``y = vec(Y*B')`` (plot_time_comparisions.m:74-75)."""
    x, rec = _cosamp_call(True, [Af, Bf], y, K, iters, tol, ctx)
    return (x, rec) if info else x


def _is_c128(x):
    return str(getattr(x, "dtype", "")) in ("complex128", "torch.complex128")


def vamp(y, A, sigma, L, *, nit=100, ctx=None):
    """benchmark_algorithms/vamp.m:1 — ``x = vamp(y, A, sigma, L)`` (dense dictionary, min(M, N) <= 2048:
    the drivers' 512 x 512 ``kron((B*B').', A)`` included).
    ``y``: (M,) or (batch, M).  ``nit`` = 100 is what the reference always runs.

    complex128 inputs (``y`` and ``A``) take ``jstsp_vamp_c64``: float64 storage and arithmetic on the device (csrc/vamp64.hip):
    within 1e-9 of the float64 oracle at nit = 12, inside the spread of two float64 restatements at nit = 50 and 100 (the
    iteration is chaotic), statistical NMSE parity at nit = 100; complex64 inputs the fp32-storage path."""
    f64 = _is_c128(A) and _is_c128(y)
    cdt = np.complex128 if f64 else np.complex64
    a_A = _Arg(A, cdt, "A")
    tor = _is_torch(y)
    single = y.ndim == 1
    y3 = (y.reshape(1, -1, 1) if single else y.reshape(y.shape[0], -1, 1))
    if tor:
        y3 = colmajor(y3)
    a_y = _Arg(y3, cdt, "y")
    batch, M, N = a_y.batch, a_A.R, a_A.C
    if a_y.R != M:
        raise ValueError("length(y) must equal size(A,1)")
    c, mem, dev = _ctx_for([a_A, a_y], ctx)
    px, fx = _out(mem == DEVICE, batch, N, 1, cdt, dev)
    fn = c._lib.jstsp_vamp_c64 if f64 else c._lib.jstsp_vamp_c32
    check(fn(c.handle, M, N, batch, a_y.ptr, a_A.ptr, _shared_stride(a_A, M * N, batch, "A"),
             float(sigma), float(L), int(nit), px, mem), "jstsp_vamp_c64" if f64 else "jstsp_vamp_c32")
    return fx(single)[..., 0]


def vamp_kron(Y, Af, Gb, sigma, L, *, nit=100, ctx=None):
    """``vamp(vec(Y), kron(Gb.', Af), sigma, L)`` without forming the dictionary — the call of
    plot_errorVSsnr.m:79-80,100 with ``Gb = B*B'``, ``Y = Y_hbf*B'``.  Returns X (Gr x G2), x = vec(X).
    complex128 inputs (all three) take the float64 path ``jstsp_vamp_kron_c64`` (see ``vamp``)."""
    f64 = _is_c128(Y) and _is_c128(Af) and _is_c128(Gb)
    cdt = np.complex128 if f64 else np.complex64
    a_Y, a_A, a_G = _Arg(Y, cdt, "Y"), _Arg(Af, cdt, "Af"), _Arg(Gb, cdt, "Gb")
    batch, Na, G2, Gr = a_Y.batch, a_Y.R, a_Y.C, a_A.C
    if a_A.R != Na or (a_G.R, a_G.C) != (G2, G2):
        raise ValueError("shape mismatch")
    c, mem, dev = _ctx_for([a_Y, a_A, a_G], ctx)
    px, fx = _out(mem == DEVICE, batch, Gr, G2, cdt, dev)
    fn = c._lib.jstsp_vamp_kron_c64 if f64 else c._lib.jstsp_vamp_kron_c32
    check(fn(c.handle, Na, Gr, G2, batch, a_Y.ptr, a_A.ptr, _shared_stride(a_A, Na * Gr, batch, "Af"), a_G.ptr,
             _shared_stride(a_G, G2 * G2, batch, "Gb"), float(sigma), float(L), int(nit), px, mem),
          "jstsp_vamp_kron_c64" if f64 else "jstsp_vamp_kron_c32")
    return fx(not a_Y.batched)


def sparse_sca_estim(rhat, rvar, var0, p1, *, ctx=None):
    """``[xhat, xvar] = SparseScaEstim(CAwgnEstimIn(0, var0), p1).estim(rhat, rvar)`` on real coordinates with the complex
    log-likelihood branch (MPbased_solvers/main/SparseScaEstim.m:76-166, CAwgnEstimIn.m:94-102,181-184) - the denoiser of every
    VAMP iteration (vamp.m:23-25), stand-alone.  ``rhat``: 1-D float64 numpy array (host path); returns two float64 arrays."""
    r = np.ascontiguousarray(np.asarray(rhat, dtype=np.float64).reshape(-1))
    c = ctx or _lib.default_context(0)
    xh, xv = np.empty_like(r), np.empty_like(r)
    check(c._lib.jstsp_sparse_sca_estim_f64(c.handle, r.size, r.ctypes.data, float(rvar), float(var0), float(p1), xh.ctypes.data, xv.ctypes.data,
                                            HOST), "jstsp_sparse_sca_estim_f64")
    return xh.reshape(np.shape(rhat)), xv.reshape(np.shape(rhat))


def cawgn_estim_out(y, phat, pvar, wvar, *, ctx=None):
    """``[zhat, zvar] = CAwgnEstimOut(y, wvar).estim(phat, pvar)`` with scale = 1 (MPbased_solvers/main/CAwgnEstimOut.m:97-108) on real
    coordinates - the likelihood of every VAMP iteration (vamp.m:30), stand-alone.  Returns (zhat array, zvar scalar)."""
    yy = np.ascontiguousarray(np.asarray(y, dtype=np.float64).reshape(-1))
    pp = np.ascontiguousarray(np.asarray(phat, dtype=np.float64).reshape(-1))
    if yy.size != pp.size:
        raise ValueError("y and phat must have the same number of entries")
    c = ctx or _lib.default_context(0)
    zh = np.empty_like(yy)
    zv = C.c_double(0.0)
    check(c._lib.jstsp_cawgn_estim_out_f64(c.handle, yy.size, yy.ctypes.data, pp.ctypes.data, float(pvar), float(wvar), zh.ctypes.data,
                                           C.byref(zv), HOST), "jstsp_cawgn_estim_out_f64")
    return zh.reshape(np.shape(y)), float(zv.value)


# ----------------------------------------------------------------------------- capacity / energy efficiency
BEAMFORMER_KINDS = {"ZC": _lib.BF_ZC, "fft": _lib.BF_DFT, "ps": _lib.BF_DFT, "quantized": _lib.BF_QUANTIZED,
                    "quantized_4": _lib.BF_QUANTIZED4}


def _bf_kind(kind):
    if kind not in BEAMFORMER_KINDS:
        raise ValueError("beamformer kind must be one of %s, got %r" % (sorted(BEAMFORMER_KINDS), kind))
    return BEAMFORMER_KINDS[kind]


def beamformer(N, kind, *, dtype=np.complex64, device=None, ctx=None):
    """createBeamformer.m:1-35 — ``createBeamformer(N, kind)`` for 'ZC', 'fft', 'ps', 'quantized', 'quantized_4' (N x N).
    numpy (host path) by default; ``device``: a column-major torch tensor on that GPU.  ``dtype=np.complex128`` takes
    ``jstsp_beamformer_c64`` (phases evaluated in float64)."""
    k = _bf_kind(kind)
    f64 = np.dtype(dtype) == np.complex128
    N = int(N)
    if device is not None:
        import torch
        dev = torch.device(device)
        c = ctx or _lib.default_context(dev.index or 0)
        c.use_torch_stream()
        W = empty_colmajor(1, N, N, torch.complex128 if f64 else torch.complex64, dev)[0]
        ptr, mem = W.data_ptr(), DEVICE
    else:
        c = ctx or _lib.default_context(0)
        buf = np.empty((N, N), dtype=np.complex128 if f64 else np.complex64)       # [column][row]
        ptr, mem = buf.ctypes.data, HOST
    fn, name = (c._lib.jstsp_beamformer_c64, "jstsp_beamformer_c64") if f64 else (c._lib.jstsp_beamformer_c32, "jstsp_beamformer_c32")
    check(fn(c.handle, N, k, ptr, mem), name)
    return W if device is not None else buf.T


def ase(Y, W, scale, Mr=None, cols=None, *, ctx=None):
    """plot_capacity.m:47,52,57,64 — ``real(log2(det(eye(Mr) + scale * W_c'*(Y*Y')*W_c)))`` per problem, with
    ``W_c = W(:, cols)`` (1-based, per problem) or ``W(:, 1:Mr)`` (hbf.m:23).  ``Y``: (Nr, T) or (batch, Nr, T); ``W``: (Nr, Ncols),
    shared; ``cols``: (Mr,) or (batch, Mr) integers.  complex128 ``Y`` and ``W`` take ``jstsp_ase_c64``.  Returns float64
    (batch,) (a scalar for 2-D ``Y``); a bad column index gives NaN for its problem."""
    f64 = _is_c128(Y) and _is_c128(W)
    cdt = np.complex128 if f64 else np.complex64
    a_Y, a_W = _Arg(Y, cdt, "Y"), _Arg(W, cdt, "W")
    if a_W.batched:
        raise ValueError("W is shared by the batch: pass one (Nr, Ncols) matrix")
    if a_W.R != a_Y.R:
        raise ValueError("Y and W must have the same number of rows")
    c, mem, dev = _ctx_for([a_Y, a_W], ctx)
    if mem == DEVICE and a_W.device != dev:
        raise ValueError("Y and W must live on the same GPU")
    batch = a_Y.batch
    cptr, keep = None, None
    if cols is not None:
        # cols lives where Y and W live: the library reads it in the call's memspace
        if mem == DEVICE:
            import torch
            if not (_is_torch(cols) and cols.is_cuda and cols.device == dev and cols.dtype == torch.int32):
                raise ValueError("cols: with device arrays pass an int32 CUDA tensor on the device of Y (%s)" % dev)
            keep = cols.reshape(-1, cols.shape[-1]).contiguous()
        else:
            if _is_torch(cols):
                raise ValueError("cols: with host (numpy) arrays pass a numpy integer array, not a torch tensor")
            keep = np.ascontiguousarray(np.asarray(cols, dtype=np.int32).reshape(-1, np.shape(cols)[-1]))
        if keep.shape[0] == 1 and batch > 1:
            keep = keep.expand(batch, -1).contiguous() if _is_torch(keep) else np.ascontiguousarray(np.repeat(keep, batch, 0))
        if keep.shape[0] != batch:
            raise ValueError("cols must have one row per problem (%d), got %d" % (batch, keep.shape[0]))
        if Mr is not None and int(Mr) != keep.shape[1]:
            raise ValueError("Mr disagrees with cols")
        Mr = keep.shape[1]
        cptr = keep.data_ptr() if _is_torch(keep) else keep.ctypes.data
    elif Mr is None:
        Mr = a_W.C
    if mem == DEVICE:
        import torch
        out = torch.empty(batch, dtype=torch.float64, device=dev)
        optr = out.data_ptr()
    else:
        out = np.empty(batch, dtype=np.float64)
        optr = out.ctypes.data
    fn, name = (c._lib.jstsp_ase_c64, "jstsp_ase_c64") if f64 else (c._lib.jstsp_ase_c32, "jstsp_ase_c32")
    check(fn(c.handle, a_Y.R, a_Y.C, a_W.C, int(Mr), batch, a_Y.ptr, a_W.ptr, cptr, float(scale), optr, mem), name)
    return out if a_Y.batched else out[0]


def singular_values(Y, *, ctx=None):
    """``svd(Y)`` without the vectors (plot_rankR.m:49) — the singular values of ``Y``: (rows, cols) or (batch, rows, cols),
    numpy or a column-major torch CUDA tensor, complex64 (``jstsp_singular_values_c32``) or complex128 (``_c64``).  float64
    one-sided Jacobi on the matrix itself, not on a Gram matrix, so values down to ``eps * sigma_1`` are resolved (what a
    numerical rank is read from).  Returns float64 (batch, min(rows, cols)) (one row less for 2-D ``Y``), descending, where
    ``Y`` lives; min(rows, cols) <= 64 and rows * cols <= 8192, else ``JstspError`` (code -3); a non-finite entry gives NaN for
    its own matrix."""
    f64 = _is_c128(Y)
    a_Y = _Arg(Y, np.complex128 if f64 else np.complex64, "Y")
    c, mem, dev = _ctx_for([a_Y], ctx)
    n = min(a_Y.R, a_Y.C)
    if mem == DEVICE:
        import torch
        out = torch.empty((a_Y.batch, n), dtype=torch.float64, device=dev)
        optr = out.data_ptr()
    else:
        out = np.empty((a_Y.batch, n), dtype=np.float64)
        optr = out.ctypes.data
    fn, name = (c._lib.jstsp_singular_values_c64, "jstsp_singular_values_c64") if f64 else \
        (c._lib.jstsp_singular_values_c32, "jstsp_singular_values_c32")
    check(fn(c.handle, a_Y.R, a_Y.C, a_Y.batch, a_Y.ptr, optr, mem), name)
    return out if a_Y.batched else out[0]


def spectrum(Y, n_keep=None, *, ctx=None):
    """The leading ``n_keep`` (default: all ``min(rows, cols)``) singular values of ``Y`` at every driver size
    (``jstsp_spectrum_c32`` / ``_c64``, csrc/svdvals.hip): the arguments and the result of :func:`singular_values`, without its
    shape limit.  Shapes that function accepts return its bits; ``min(rows, cols) <= 64`` with ``max(rows, cols) <= 65536`` goes
    through a float64 Householder tall-skinny QR in front of the same Jacobi; orders 65..512 with ``max(rows, cols) <= 8192``
    through the global-memory one-sided Jacobi of :func:`pinv_f64`.  No Gram matrix on any route.  Anything larger raises
    ``JstspError`` (code -3).  A batch whose workspace would exceed the library's 24 GiB limit is computed in chunks."""
    f64 = _is_c128(Y)
    a_Y = _Arg(Y, np.complex128 if f64 else np.complex64, "Y")
    c, mem, dev = _ctx_for([a_Y], ctx)
    m, n = max(a_Y.R, a_Y.C), min(a_Y.R, a_Y.C)
    keep = n if n_keep is None else int(n_keep)
    if not 1 <= keep <= n:
        raise ValueError("n_keep must lie in 1..min(rows, cols) = %d, got %d" % (n, keep))
    batch = a_Y.batch
    if mem == DEVICE:
        import torch
        out = torch.empty((batch, keep), dtype=torch.float64, device=dev)
        optr = out.data_ptr()
    else:
        out = np.empty((batch, keep), dtype=np.float64)
        optr = out.ctypes.data
    fn, name = (c._lib.jstsp_spectrum_c64, "jstsp_spectrum_c64") if f64 else (c._lib.jstsp_spectrum_c32, "jstsp_spectrum_c32")
    esz = 16 if f64 else 8
    # bytes of workspace per matrix (csrc/svdvals.hip): the staged copy of a host operand; above order 64 the float64 operand,
    # its rotated copy and V
    per = (a_Y.R * a_Y.C * esz if mem == HOST else 0) + 8 * (keep + n)
    if n > 64:
        per += 16 * (m * n + n * n) + (0 if f64 else 16 * m * n)
    for t0, nb in _f64_chunks(batch, per):
        check(fn(c.handle, a_Y.R, a_Y.C, nb, _off(a_Y.ptr, t0 * a_Y.R * a_Y.C, esz), keep, _off(optr, t0 * keep, 8), mem), name)
    return out if a_Y.batched else out[0]


# ----------------------------------------------------------------------------- float64 solver
_F64_CHUNK_BYTES = 20 << 30        # the library refuses a float64 workspace above 24 GiB (include/jstsp.h): stay under it


def _wide(x, real=False):
    """complex64 / float32 (or any real / complex numpy dtype) -> complex128 / float64, exactly; layout kept."""
    if x is None:
        return None
    if _is_torch(x):
        import torch
        return x.to(torch.float64 if real else torch.complex128)
    return np.asarray(x, dtype=np.float64 if real else np.complex128)


def _off(ptr, elems, size):
    return None if ptr is None else ptr + int(elems) * size


def _f64_chunks(batch, per):
    """(t0, nb) of the calls that solve a batch whose float64 state is ``per`` bytes a problem, each under the limit."""
    step = max(1, min(batch, _F64_CHUNK_BYTES // max(per, 1), 65535))
    for t0 in range(0, batch, step):
        yield t0, min(step, batch - t0)


def proposed_algorithm_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type="approximate", *, indx_S=None,
                           want_ce=True, ctx=None):
    """:func:`proposed_algorithm` evaluated in float64 on the device (include/jstsp.h: jstsp_proposed_algorithm_f64) -
    nothing is narrowed.  Same arguments; complex64 / float32 inputs are widened exactly, the outputs are complex128
    (numpy in -> numpy out, torch CUDA tensors in -> torch CUDA tensors out).  ``'approximate'`` only.  A batch whose
    float64 workspace would exceed the library's limit is solved in chunks."""
    if type not in ("approximate", "std"):
        raise ValueError("type must be 'approximate' or 'std'")
    tcode = _lib.TYPE_APPROXIMATE if type == "approximate" else _lib.TYPE_STD          # ('std': the library refuses and says where to go)
    return _admm_f64(False, False, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, tcode, indx_S, None, None, want_ce, False, ctx)[:3]


def proposed_algorithm_angles_f64(subY, Omega, indx_S, A, B, Imax, tau_Y, tau_S, rho, type="approximate",
                                  greedy_nnz=None, *, want_ce=True, ctx=None):
    """:func:`proposed_algorithm_angles` in float64 on the device (see :func:`proposed_algorithm_f64`)."""
    return proposed_algorithm_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type, indx_S=indx_S, want_ce=want_ce, ctx=ctx)


def proposed_algorithm_std_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, *, indx_S=None, PA=None, PB=None, want_ce=True,
                               info=False, ctx=None):
    """Alg. 1 - ``proposed_algorithm(..., 'std')`` - evaluated in float64 on the device (include/jstsp.h:
    jstsp_proposed_std_f64): the least-squares step ``v = U\\(L\\k)`` as ``pinv(A) K pinv(B)``, which needs ``K2`` of full column
    rank (``N >= Gr``, ``M >= G2``; a rank-deficient factor raises ``JstspError`` with code -6).  Arguments and outputs as
    :func:`proposed_algorithm_f64`.  ``PA`` / ``PB``: ``None``, or ``pinv(A)`` / ``pinv(B)`` - e.g. from :func:`pinv_f64`, which
    gives the bits of the ``None`` call - batched exactly as ``A`` / ``B`` are; a caller that solves several times on the same
    dictionaries inverts them once.  ``info=True`` also returns ``rcond``: float64 (2,), the smallest over the ``A`` and over the
    ``B`` factors the call inverted, NaN for a side that was given (the smallest over the chunks when the batch is chunked)."""
    out = _admm_f64(True, False, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, None, indx_S, PA, PB, want_ce, info, ctx)
    return out[:3] + (out[4],) if info else out[:3]


def proposed_algorithm_angles_std_f64(subY, Omega, indx_S, A, B, Imax, tau_Y, tau_S, rho, greedy_nnz=None, *, PA=None, PB=None,
                                      want_ce=True, info=False, ctx=None):
    """``proposed_algorithm_angles(..., 'std')`` in float64 on the device (see :func:`proposed_algorithm_std_f64`)."""
    return proposed_algorithm_std_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, indx_S=indx_S, PA=PA, PB=PB, want_ce=want_ce,
                                      info=info, ctx=ctx)


# ----------------------------------------------------------------------------- float64 solver, resumed from a saved state
def admm_state_elems(N, M, Gr, G2):
    """Complex elements of one trial's ADMM state ``[X | V1 | V2 | C | v | S]`` (include/jstsp.h: jstsp_admm_state_elems)."""
    return 4 * int(N) * int(M) + 2 * int(Gr) * int(G2)


def _state_arg(state, batch, elems, mem, dev, np_dtype=np.complex128):
    """``state`` ((batch, elems), or (elems,) for one problem; of the solver's complex type and of the kind of the other arrays) as
    (pointer, keep-alive)."""
    if state is None:
        return None, None
    if _is_torch(state) != (mem == DEVICE):
        raise ValueError("state must be of the kind of the other arrays (numpy on the host path, torch CUDA on the device path)")
    if tuple(state.shape) not in ((batch, elems), (elems,) if batch == 1 else None):
        raise ValueError("state must have shape (%d, %d), got %s" % (batch, elems, tuple(state.shape)))
    if mem == DEVICE:
        import torch
        want = torch.complex128 if np_dtype == np.complex128 else torch.complex64
        if state.dtype != want or state.device != dev:
            raise ValueError("state: expected a %s tensor on %s" % (want, dev))
        buf = state.contiguous()
        return buf.data_ptr(), buf
    buf = np.ascontiguousarray(state, dtype=np_dtype)
    return buf.ctypes.data, buf


def _state_out(wanted, batch, elems, mem, dev, np_dtype=np.complex128):
    """A new ``(batch, elems)`` state array where the inputs live, as (pointer, array); (None, None) when none is wanted."""
    if not wanted:
        return None, None
    if mem == DEVICE:
        import torch
        st = torch.empty((batch, elems), dtype=torch.complex128 if np_dtype == np.complex128 else torch.complex64, device=dev)
        return st.data_ptr(), st
    st = np.empty((batch, elems), dtype=np_dtype)
    return st.ctypes.data, st


def _f64_admm_bytes(N, M, Gr, G2, sA, sB, std, own_PA, own_PB, host, resumed, *, refresh=False):
    """Bytes of float64 state per trial of a float64 ``proposed_algorithm`` call (csrc/proposed64.hip), which sets the chunks of a large
    batch: the N x M and Gr x G2 arrays, the products, the svt, the Grams of a per-trial dictionary, for Alg. 1 (``std``) the Hestenes
    arrays of a per-trial factor the call inverts (``own_PA`` / ``own_PB``), and the staged copies of a host call.  The plain Alg. 1
    call counts 2 Gr x G2 arrays and no Grams, the plain Alg. 2 call stages a per-trial dictionary once and the others twice, and only
    a resumed call stages the two state blocks.  Above Gram order 64 a chunk's trials are swept together (include/jstsp.h), so a
    change of these counts can change last bits.  ``refresh``: the refreshed solve's rank array and, staged, its two orders."""
    n, g = min(N, M), Gr * G2
    plain_std = std and not resumed
    per = 8 * N * M + (2 if plain_std else 5) * g + Gr * M + N * G2 + 20 * n * n
    if not plain_std:
        per += (G2 * G2 if sB else 0) + (Gr * Gr if sA else 0)
    if std:
        per += (2 * N * Gr + 3 * Gr * Gr if sA and own_PA else 0) + (2 * G2 * M + 3 * G2 * G2 if sB and own_PB else 0)
    per *= 16
    if host:
        dicts = (G2 * M if sB else 0) + (N * Gr if sA else 0)
        states = 2 * admm_state_elems(N, M, Gr, G2) if resumed else 0
        per += 16 * (2 * N * M + g + (2 if std or resumed else 1) * dicts + states) + 8 * N * M
    if refresh:
        per += 4 * g + (4 * (g + min(g, _lib.SUPPORT_TOP_MAX)) if host else 0)
    return per


def _f64_until_bytes(N, M, Gr, G2, sA, sB, host):
    """Bytes per trial of a ``proposed_algorithm_until_f64`` call: the refreshed, resumed Alg. 2 call of :func:`_f64_admm_bytes` plus
    what the stopping rule's compaction adds (csrc/proposed64.hip, Shadow64) - a second copy of X, V1, V2, C, A S B, v, S and the
    rank, one of subY, Omega and a per-trial dictionary (two for a device call: the caller's own arrays are never written), the
    Grams of a per-trial dictionary, the order by slot and its shadow, and the small per-trial arrays."""
    g, twice = Gr * G2, 1 if host else 2
    per = _f64_admm_bytes(N, M, Gr, G2, sA, sB, False, True, True, host, True, refresh=True)
    per += 16 * (5 * N * M + 2 * g) + 24 * N * M * twice + 4 * g + 8 * min(g, _lib.SUPPORT_TOP_MAX) + 1024
    per += 16 * ((N * Gr * twice + Gr * Gr if sA else 0) + (G2 * M * twice + G2 * G2 if sB else 0))
    return per


def _admm_f64(std, resumed, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, tcode, indx_S, PA, PB, want_ce, info, ctx, state=None, it0=0,
              return_state=False):
    """The frame of the four float64 ``proposed_algorithm`` functions: Alg. 1 (``std``) or Alg. 2, through the plain C entry or -
    ``resumed`` - the one that takes ``it0`` and the states.  Returns ``(S, Y, ce, state, rcond)``; ``rcond`` with ``info`` (Alg. 1)."""
    q = _AdmmCall(np.complex128, subY, Omega, A, B, indx_S, tau_Y, tau_S, rho, Imax, PA, PB)
    N, M, Gr, G2, batch, Imax, sA, sB = q.N, q.M, q.Gr, q.G2, q.batch, q.Imax, q.sA, q.sB
    it0 = int(it0)
    if it0 < 0 or (state is None and it0 != 0):
        raise ValueError("it0 must be >= 0, and 0 when there is no state to start from")
    ne = admm_state_elems(N, M, Gr, G2)
    p_in, keep_in = _state_arg(state, batch, ne, q.state_mem, q.state_dev)
    q.open(want_ce, ctx)
    mem = q.mem
    p_out, st_out = _state_out(return_state, batch, ne, mem, q.dev)
    per = _f64_admm_bytes(N, M, Gr, G2, sA, sB, std, q.PA.ptr is None, q.PB.ptr is None, mem == HOST, resumed)
    name = {(False, False): "jstsp_proposed_algorithm_f64", (False, True): "jstsp_proposed_resume_f64",
            (True, False): "jstsp_proposed_std_f64", (True, True): "jstsp_proposed_std_resume_f64"}[bool(std), bool(resumed)]
    dp = C.POINTER(C.c_double)
    rcs = []
    for t0, nb in _f64_chunks(batch, per):
        prc, rc1 = _vec_out(mem == DEVICE, 2, np.float64, q.dev) if info else (None, None)
        head = (q.ctx.handle, N, M, Gr, G2, nb, _off(q.sub.ptr, t0 * N * M, 16), _off(q.om.ptr, t0 * N * M, 8), _off(q.A.ptr, t0 * sA, 16), sA,
                _off(q.B.ptr, t0 * sB, 16), sB)
        prm = (Imax, q.tY[t0:].ctypes.data_as(dp), q.tS[t0:].ctypes.data_as(dp), q.rh[t0:].ctypes.data_as(dp))
        outs = (_off(q.ix.ptr, t0 * Gr * G2, 4), _off(q.pS, t0 * Gr * G2, 16), _off(q.pY, t0 * N * M, 16), _off(q.pce, t0 * 3 * Imax, 8))
        tail = ((it0, _off(p_in, t0 * ne, 16), _off(p_out, t0 * ne, 16)) if resumed else ()) + (mem,)
        if std:
            args = head + (_off(q.PA.ptr, t0 * (Gr * N if sA else 0), 16), _off(q.PB.ptr, t0 * (M * G2 if sB else 0), 16)) + prm + outs + (prc,) + tail
        else:
            args = head + prm + (tcode,) + outs + tail
        check(getattr(q.ctx._lib, name)(*args), name)
        rcs.append(rc1)
    del keep_in
    rcond = rcs[0]
    for r in rcs[1:] if info else ():          # (min propagates NaN in numpy and in torch)
        rcond = np.minimum(rcond, r) if mem == HOST else rcond.minimum(r)
    return q.result() + (st_out, rcond)


def proposed_algorithm_resume_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, type="approximate", *, indx_S=None, want_ce=True, ctx=None,
                                  state=None, it0=0, return_state=True):
    """:func:`proposed_algorithm_f64` resumed from a saved state (include/jstsp.h: jstsp_proposed_resume_f64): iterations
    ``it0 + 1 ... it0 + Imax`` of the reference loop from ``state``.  Returns ``(S, Y, ce, state)``: ``ce`` holds the ``Imax`` rows
    this call ran, ``state`` - complex128 ``(batch, admm_state_elems(N, M, Gr, G2))``, a new array of the kind of the inputs, or
    ``None`` with ``return_state=False`` - is what a later call takes to go on.  The state is always two-dimensional: for one
    unbatched problem (``subY`` 2-D, where ``S``, ``Y`` and ``ce`` come back without the batch axis) it is ``(1, elems)``, one row per
    trial as the C ABI lays it out; as an argument both ``(1, elems)`` and ``(elems,)`` are taken.  ``state=None``: from zero (``it0`` must be 0),
    the bits of :func:`proposed_algorithm_f64`.  Legs (a, b) return the bits of one solve of ``a + b`` iterations.  The state
    may come from another problem of the same shape (a warm start); ``it0`` then only sets the mask count of ``indx_S``."""
    if type != "approximate":
        raise ValueError("type must be 'approximate' (Alg. 1: proposed_algorithm_std_resume_f64)")
    return _admm_f64(False, True, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, _lib.TYPE_APPROXIMATE, indx_S, None, None, want_ce, False, ctx,
                     state, it0, return_state)[:4]


def proposed_algorithm_std_resume_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, *, indx_S=None, PA=None, PB=None, want_ce=True, ctx=None,
                                      state=None, it0=0, return_state=True):
    """:func:`proposed_algorithm_std_f64` resumed from a saved state (include/jstsp.h: jstsp_proposed_std_resume_f64); arguments
    and outputs as :func:`proposed_algorithm_resume_f64`, ``PA`` / ``PB`` as the sibling's.  Alg. 1 recomputes ``v`` in every
    iteration: the ``v`` of ``state`` is ignored."""
    return _admm_f64(True, True, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, None, indx_S, PA, PB, want_ce, False, ctx, state, it0,
                     return_state)[:4]


# ----------------------------------------------------------------------------- float64 solver, support refreshed from its own iterate
def _refresh_first(it0, Imax, start, period):
    """The first refresh iteration (global, 1-based) among ``it0 + 1 ... it0 + Imax``, or ``None``: iteration ``i`` refreshes when
    ``i > start`` and ``(i - start - 1) % period == 0`` (``period >= 1``), or only ``i == start + 1`` (``period == 0``)."""
    lo, hi = it0 + 1, it0 + Imax
    first = start + 1
    if first < lo and period:
        first += -(-(lo - first) // period) * period
    return first if lo <= first <= hi else None


def _refresh_open(cdt, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, start, period, indx_S, want_ce, ctx, state, it0, return_state):
    """What the two refreshed wrappers do before their library call, for the solver's complex dtype ``cdt``: every ``ValueError`` of
    the arguments (before any device call), then the context, the outputs, the states and ``order`` - a new (batch, R) array when the
    call runs a refresh, else ``indx_S`` as given.  Returns ``(q, n, start, period, it0, p_in, keep_in, p_out, st_out, order, p_ord)``."""
    start, period, it0 = int(start), int(period), int(it0)
    if start < 0 or period < 0:
        raise ValueError("start and period must be >= 0, not %r and %r" % (start, period))
    q = _AdmmCall(cdt, subY, Omega, A, B, None, tau_Y, tau_S, rho, Imax)
    batch, g = q.batch, q.Gr * q.G2
    R = min(g, _lib.SUPPORT_TOP_MAX)
    n = 0
    if indx_S is not None:
        n = int(indx_S.shape[-1]) if len(indx_S.shape) else 0
        size = int(indx_S.numel() if _is_torch(indx_S) else np.asarray(indx_S).size)
        if not 1 <= n <= g or size != batch * n:
            raise ValueError("indx_S must be (n,) or (batch, n) with 1 <= n <= Gr*G2 = %d and batch = %d, got shape %s"
                             % (g, batch, tuple(indx_S.shape)))
        q.ix = _indx_arg(indx_S, batch, n)
    if it0 < 0 or (state is None and it0 != 0):
        raise ValueError("it0 must be >= 0, and 0 when there is no state to start from")
    ne = admm_state_elems(q.N, q.M, q.Gr, q.G2)
    p_in, keep_in = _state_arg(state, batch, ne, q.state_mem, q.state_dev, cdt)
    q.open(want_ce, ctx)
    p_out, st_out = _state_out(return_state, batch, ne, q.mem, q.dev, cdt)
    order, p_ord = indx_S, None
    if _refresh_first(it0, q.Imax, start, period) is not None:
        if q.mem == DEVICE:
            import torch
            order = torch.empty((batch, R), dtype=torch.int32, device=q.dev)
            p_ord = order.data_ptr()
        else:
            order = np.empty((batch, R), dtype=np.int32)
            p_ord = order.ctypes.data
    return q, n, start, period, it0, p_in, keep_in, p_out, st_out, order, p_ord


def proposed_algorithm_refresh(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, *, start=0, period=1, indx_S=None, want_ce=True, ctx=None,
                               state=None, it0=0, return_state=True):
    """:func:`proposed_algorithm_refresh_f64` on the fp32 solver (include/jstsp.h: jstsp_proposed_refresh_c32):
    :func:`proposed_algorithm_resume` ('approximate') with its support refreshed from its own iterate inside the loop, by the
    schedule, ``indx_S`` and limit of the float64 sibling.  Returns ``(S, Y, ce, state, order)``: complex64 arrays as the resumed
    call's, ``order`` int32 ``(batch, min(Gr*G2, 4096))`` the list of the call's last refresh - :func:`support_top` of that
    iteration's ``v`` - or, when the call ran no refresh, the caller's ``indx_S`` as it was given.  Legs that pass ``order`` on are
    fp32-equivalent to the uninterrupted call, not bit-identical, as every split fp32 solve."""
    q, n, start, period, it0, p_in, keep_in, p_out, st_out, order, p_ord = _refresh_open(
        np.complex64, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, start, period, indx_S, want_ce, ctx, state, it0, return_state)
    name = "jstsp_proposed_refresh_c32"
    args = q.c32_args("approximate")         # (... rho, type, indx_S, S, Y, ce)
    check(getattr(q.ctx._lib, name)(*args[:-3], n, start, period, *args[-3:], it0, p_in, p_out, p_ord, q.mem), name)
    del keep_in
    return q.result() + (st_out, order)


def proposed_algorithm_refresh_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, *, start=0, period=1, indx_S=None, want_ce=True, ctx=None,
                                   state=None, it0=0, return_state=True):
    """:func:`proposed_algorithm_resume_f64` (Alg. 2) with its support refreshed from its own iterate inside the loop (include/jstsp.h:
    jstsp_proposed_refresh_f64): at the global iterations ``i > start`` with ``(i - start - 1) % period == 0``
    (``period=0``: only ``i == start + 1``) the mask becomes the top ``min(10 + 5 i, Gr*G2)`` of the new ``v``, and stays the top of
    that ``v`` - growing by the iteration's count - until the next refresh.  Until the first refresh the order in force is
    ``indx_S`` (1-based, ``(n,)`` or ``(batch, n)`` with ``1 <= n <= Gr*G2``; entries it does not list are never admitted), or none.
    ``start=0, period=1`` needs no prior at all.  Returns ``(S, Y, ce, state, order)``: the first four as the sibling's, ``order``
    int32 ``(batch, min(Gr*G2, 4096))`` the list of the call's last refresh where the inputs live - or, when the call ran no
    refresh (a function of ``it0``, ``Imax``, ``start``, ``period``), the caller's ``indx_S`` as it was given.  A later leg passes
    ``order`` as ``indx_S`` with the same ``start`` and ``period`` and its own ``it0`` and returns the bits of the uninterrupted call.
    A refreshed order lists at most 4096 entries, so above ``Gr*G2 = 4096`` the mask stops growing at iteration 818.  A batch whose
    float64 workspace would exceed the library's limit is solved in chunks."""
    q, n, start, period, it0, p_in, keep_in, p_out, st_out, order, p_ord = _refresh_open(
        np.complex128, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, start, period, indx_S, want_ce, ctx, state, it0, return_state)
    N, M, Gr, G2, batch, Imax, sA, sB, mem = q.N, q.M, q.Gr, q.G2, q.batch, q.Imax, q.sA, q.sB, q.mem
    g, ne, R = Gr * G2, admm_state_elems(N, M, Gr, G2), min(Gr * G2, _lib.SUPPORT_TOP_MAX)
    per = _f64_admm_bytes(N, M, Gr, G2, sA, sB, False, True, True, mem == HOST, True, refresh=True)
    dp = C.POINTER(C.c_double)
    name = "jstsp_proposed_refresh_f64"
    for t0, nb in _f64_chunks(batch, per):
        check(getattr(q.ctx._lib, name)(
            q.ctx.handle, N, M, Gr, G2, nb, _off(q.sub.ptr, t0 * N * M, 16), _off(q.om.ptr, t0 * N * M, 8), _off(q.A.ptr, t0 * sA, 16), sA,
            _off(q.B.ptr, t0 * sB, 16), sB, Imax, q.tY[t0:].ctypes.data_as(dp), q.tS[t0:].ctypes.data_as(dp), q.rh[t0:].ctypes.data_as(dp),
            _off(q.ix.ptr, t0 * n, 4), n, start, period, _off(q.pS, t0 * g, 16), _off(q.pY, t0 * N * M, 16), _off(q.pce, t0 * 3 * Imax, 8),
            it0, _off(p_in, t0 * ne, 16), _off(p_out, t0 * ne, 16), _off(p_ord, t0 * R, 4), mem), name)
    del keep_in
    return q.result() + (st_out, order)


# ----------------------------------------------------------------------------- float64 solver, each trial stopped when it has settled
def proposed_algorithm_until_f64(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, *, tol, min_iters=2, check=1, indx_S=None, refresh=None,
                                 state=None, it0=0, want_ce=False, return_state=True, type="approximate", ctx=None):
    """:func:`proposed_algorithm_refresh_f64` - with ``refresh=None`` :func:`proposed_algorithm_resume_f64` - with a stopping rule
    (include/jstsp.h: jstsp_proposed_until_f64): trial ``t`` stops after the first iteration ``i`` of the call
    with ``i >= min_iters`` and ``convergence_error[i, 2] = |v_i - v_{i-1}|^2 / |v_{i-1}|^2 <= tol[t]``, failing that after ``Imax``.
    ``tol``: a scalar or ``(batch,)``; an entry that is zero, negative or NaN never stops its trial.  ``refresh``: ``None`` or
    ``(start, period)``.  ``check``: the iterations between two compactions of the batch, each of which reads one number back; it
    never changes a result (the default is the fastest measured at BASELINE configs[1]: DESIGN.md section 9t).  Returns ``(S, Y, ce, state, order, iters, ce3)``: the first five as the sibling's for every trial
    alone over ``iters[t]`` iterations (bit for bit for ``min(N, M) <= 64``); rows of ``ce`` after ``iters[t]`` are NaN; a row of
    ``order`` is all zeros for a trial that stopped before its first refresh; ``iters`` int32 ``(batch,)`` and ``ce3`` float64
    ``(batch,)`` - the last iteration's ``ce[:, 2]`` - live where the inputs live.  The rule is memoryless, so an unstopped trial
    (``iters[t] == Imax`` and ``ce3[t] > tol[t]``) is resumed by a later call with ``state`` and ``it0``.  Alg. 2 only."""
    if type != "approximate":
        raise ValueError("type must be 'approximate': the stopping rule reads the gradient step of Alg. 2")
    min_iters, check_every, it0, Imax = int(min_iters), int(check), int(it0), int(Imax)
    if min_iters < 1 or check_every < 1:
        raise ValueError("min_iters and check must be >= 1, not %r and %r" % (min_iters, check_every))
    if refresh is None:
        start, period = it0 + max(Imax, 0), 0               # (for the checks below: a schedule that never refreshes in this call)
    else:
        start, period = refresh
    q, n, start, period, it0, p_in, keep_in, p_out, st_out, order, p_ord = _refresh_open(
        np.complex128, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, start, period, indx_S, want_ce, ctx, state, it0, return_state)
    if refresh is None:
        start, period = 0, -1
    N, M, Gr, G2, batch, Imax, sA, sB, mem = q.N, q.M, q.Gr, q.G2, q.batch, q.Imax, q.sA, q.sB, q.mem
    tl, _ = _scalars(tol, batch, "tol")
    g, ne, R = Gr * G2, admm_state_elems(N, M, Gr, G2), min(Gr * G2, _lib.SUPPORT_TOP_MAX)
    p_it, iters = _vec_out(mem == DEVICE, batch, np.int32, q.dev)
    p_c3, ce3 = _vec_out(mem == DEVICE, batch, np.float64, q.dev)
    per = _f64_until_bytes(N, M, Gr, G2, sA, sB, mem == HOST)
    dp = C.POINTER(C.c_double)
    name = "jstsp_proposed_until_f64"
    for t0, nb in _f64_chunks(batch, per):
        _lib.check(getattr(q.ctx._lib, name)(
            q.ctx.handle, N, M, Gr, G2, nb, _off(q.sub.ptr, t0 * N * M, 16), _off(q.om.ptr, t0 * N * M, 8), _off(q.A.ptr, t0 * sA, 16), sA,
            _off(q.B.ptr, t0 * sB, 16), sB, Imax, q.tY[t0:].ctypes.data_as(dp), q.tS[t0:].ctypes.data_as(dp), q.rh[t0:].ctypes.data_as(dp),
            _off(q.ix.ptr, t0 * n, 4), n, start, period, tl[t0:].ctypes.data_as(dp), min_iters, check_every,
            _off(q.pS, t0 * g, 16), _off(q.pY, t0 * N * M, 16), _off(q.pce, t0 * 3 * Imax, 8),
            it0, _off(p_in, t0 * ne, 16), _off(p_out, t0 * ne, 16), _off(p_ord, t0 * R, 4), _off(p_it, t0, 4), _off(p_c3, t0, 8), mem), name)
    del keep_in
    return q.result() + (st_out, order, iters, ce3)


UNTIL_CHECK_F32 = 1     # iterations between two reads of the running count: the fastest measured


def proposed_algorithm_until(subY, Omega, A, B, Imax, tau_Y, tau_S, rho, *, tol, min_iters=2, check=UNTIL_CHECK_F32, indx_S=None,
                             refresh=None, state=None, it0=0, want_ce=False, return_state=True, type="approximate", ctx=None):
    """:func:`proposed_algorithm_until_f64` on the fp32 solver (include/jstsp.h: jstsp_proposed_until_c32):
    :func:`proposed_algorithm_refresh` - with ``refresh=None`` :func:`proposed_algorithm_resume` ('approximate') - where trial ``t``
    stops after the first iteration ``i`` of the call with ``i >= min_iters`` and ``convergence_error[i, 2] <= tol[t]``, failing
    that after ``Imax``.  The arguments and the returned ``(S, Y, ce, state, order, iters, ce3)`` are the float64 sibling's, in
    complex64.  The fp32 batch is not compacted: a stopped trial runs on until every trial has stopped, so ``check`` - the iterations
    between two reads of the running count - and the other trials' ``tol`` never change a trial's result, to the bit; against
    the sibling run for that trial alone over ``iters[t]`` iterations the values are fp32-equivalent.  Alg. 2 only."""
    if type != "approximate":
        raise ValueError("type must be 'approximate': the stopping rule reads the gradient step of Alg. 2")
    min_iters, check_every, it0, Imax = int(min_iters), int(check), int(it0), int(Imax)
    if min_iters < 1 or check_every < 1:
        raise ValueError("min_iters and check must be >= 1, not %r and %r" % (min_iters, check_every))
    if refresh is None:
        start, period = it0 + max(Imax, 0), 0               # (for the checks below: a schedule that never refreshes in this call)
    else:
        start, period = refresh
    tl, ptl = _scalars(tol, int(subY.shape[0]) if len(subY.shape) == 3 else 1, "tol")      # (refused before the context, as the rest)
    q, n, start, period, it0, p_in, keep_in, p_out, st_out, order, p_ord = _refresh_open(
        np.complex64, subY, Omega, A, B, Imax, tau_Y, tau_S, rho, start, period, indx_S, want_ce, ctx, state, it0, return_state)
    if refresh is None:
        start, period = 0, -1
    p_it, iters = _vec_out(q.mem == DEVICE, q.batch, np.int32, q.dev)
    p_c3, ce3 = _vec_out(q.mem == DEVICE, q.batch, np.float64, q.dev)
    name = "jstsp_proposed_until_c32"
    args = q.c32_args("approximate")         # (... rho, type, indx_S, S, Y, ce)
    _lib.check(getattr(q.ctx._lib, name)(*args[:-3], n, start, period, ptl, min_iters, check_every, *args[-3:], it0, p_in, p_out, p_ord,
                                         p_it, p_c3, q.mem), name)
    del keep_in, tl
    return q.result() + (st_out, order, iters, ce3)


def svt_f64(Y, tau, *, ctx=None):
    """benchmark_algorithms/svt.m:1 in float64 on the device (jstsp_svt_f64); complex128 out."""
    a_Y = _Arg(_wide(Y), np.complex128, "Y")
    c, mem, dev = _ctx_for([a_Y], ctx)
    t, pt = _scalars(tau, a_Y.batch, "tau")
    p, f = _out(mem == DEVICE, a_Y.batch, a_Y.R, a_Y.C, np.complex128, dev)
    check(c._lib.jstsp_svt_f64(c.handle, a_Y.R, a_Y.C, a_Y.batch, a_Y.ptr, pt, p, mem), "jstsp_svt_f64")
    return f(not a_Y.batched)


def correlate_f64(K, A, B, *, ctx=None):
    """``A' * K * B'`` (Gr x G2) in float64 on the f64 matrix pipe (jstsp_correlate_f64); complex128 out."""
    a_K, a_A, a_B = _Arg(_wide(K), np.complex128, "K"), _Arg(_wide(A), np.complex128, "A"), _Arg(_wide(B), np.complex128, "B")
    batch, N, M, Gr, G2 = a_K.batch, a_K.R, a_K.C, a_A.C, a_B.R
    if a_A.R != N or a_B.C != M:
        raise ValueError("shape mismatch")
    c, mem, dev = _ctx_for([a_K, a_A, a_B], ctx)
    p, f = _out(mem == DEVICE, batch, Gr, G2, np.complex128, dev)
    check(c._lib.jstsp_correlate_f64(c.handle, N, M, Gr, G2, batch, a_K.ptr, a_A.ptr,
                                     _shared_stride(a_A, N * Gr, batch, "A"), a_B.ptr,
                                     _shared_stride(a_B, G2 * M, batch, "B"), p, mem), "jstsp_correlate_f64")
    return f(not a_K.batched)


def synthesize_f64(S, A, B, *, ctx=None):
    """``A * S * B`` (N x M) in float64 on the f64 matrix pipe (jstsp_synthesize_f64); complex128 out."""
    a_S, a_A, a_B = _Arg(_wide(S), np.complex128, "S"), _Arg(_wide(A), np.complex128, "A"), _Arg(_wide(B), np.complex128, "B")
    batch, Gr, G2, N, M = a_S.batch, a_S.R, a_S.C, a_A.R, a_B.C
    if a_A.C != Gr or a_B.R != G2:
        raise ValueError("shape mismatch")
    c, mem, dev = _ctx_for([a_S, a_A, a_B], ctx)
    p, f = _out(mem == DEVICE, batch, N, M, np.complex128, dev)
    check(c._lib.jstsp_synthesize_f64(c.handle, N, M, Gr, G2, batch, a_S.ptr, a_A.ptr,
                                      _shared_stride(a_A, N * Gr, batch, "A"), a_B.ptr,
                                      _shared_stride(a_B, G2 * M, batch, "B"), p, mem), "jstsp_synthesize_f64")
    return f(not a_S.batched)


def _vec_out(kind_torch, n, np_dtype, device=None):
    """A length-n output vector where the call's arrays live: (ptr, array)."""
    if kind_torch:
        import torch
        buf = torch.empty(n, dtype={np.float64: torch.float64, np.int32: torch.int32}[np_dtype], device=device)
        return buf.data_ptr(), buf
    buf = np.empty(n, dtype=np_dtype)
    return buf.ctypes.data, buf


def pinv_f64(A, *, info=False, ctx=None):
    """MATLAB's ``pinv(A)`` computed and returned in float64 on the device (include/jstsp.h: jstsp_pinv_f64): one-sided Jacobi
    SVD of the matrix itself - no Gram matrix - with ``pinv.m``'s drop rule ``sigma <= max(size(A)) * eps(sigma_max)``.
    ``A``: (rows, cols) or (batch, rows, cols), numpy or a column-major torch CUDA tensor; complex64 / real inputs are widened
    exactly; complex128 out, where ``A`` lives.  min(rows, cols) <= 512 and max(rows, cols) <= 8192, else ``JstspError``
    (code -3).  An ill-conditioned or rank-deficient matrix is not an error: ``info=True`` also returns ``rcond`` (float64,
    the smallest kept singular value over the largest) and ``rank`` (int32), one entry per matrix.  A non-finite entry gives
    NaN for its own matrix."""
    a_A = _Arg(_wide(A), np.complex128, "A")
    c, mem, dev = _ctx_for([a_A], ctx)
    p, f = _out(mem == DEVICE, a_A.batch, a_A.C, a_A.R, np.complex128, dev)
    prc, rc = _vec_out(mem == DEVICE, a_A.batch, np.float64, dev) if info else (None, None)
    prk, rk = _vec_out(mem == DEVICE, a_A.batch, np.int32, dev) if info else (None, None)
    check(c._lib.jstsp_pinv_f64(c.handle, a_A.R, a_A.C, a_A.batch, a_A.ptr, p, prc, prk, mem), "jstsp_pinv_f64")
    P = f(not a_A.batched)
    if not info:
        return P
    return (P, rc, rk) if a_A.batched else (P, rc[0], rk[0])


def _svd_arg(A, keep, what):
    """The operand of svd_f64 / lowrank_f64 as a complex128 argument, and ``keep`` checked against min(rows, cols) - before any
    device call."""
    if getattr(A, "ndim", None) is None:
        A = np.asarray(A)
    if A.ndim not in (2, 3):
        raise ValueError("A must be 2-D or 3-D (batch first), got shape %s" % (tuple(A.shape),))
    if _is_torch(A) and not A.is_cuda:
        raise ValueError("A: torch tensors must live on the GPU (numpy arrays use the host path)")
    n = int(min(A.shape[-2:]))
    keep = n if keep is None else int(keep)
    if not 1 <= keep <= n:
        raise ValueError("%s must lie in 1..min(rows, cols) = %d, got %d" % (what, n, keep))
    return _Arg(_wide(A), np.complex128, "A"), keep


def _svd_per_matrix(a_A, keep, mem):
    """bytes of workspace per matrix (csrc/svd64.hip): the staged copies of a host call; beyond the LDS limit the rotated operand, V
    and the meta record"""
    m, n = max(a_A.R, a_A.C), min(a_A.R, a_A.C)
    per = 16 * (a_A.R * a_A.C + (a_A.R + a_A.C) * keep) + 8 * keep + 8 if mem == HOST else 0
    if n > 64 or (m + n) * n * 16 + (n + 16) * 8 + n * 4 > 159 * 1024:
        per += 16 * (m * n + n * n) + 32
    return per + 1024


def _svd_call(entry, per_matrix, A, n_keep, info, ctx):
    """svd_f64 / svd_tall_f64: the outputs where ``A`` lives, the batch in chunks under the 24 GiB limit"""
    a_A, keep = _svd_arg(A, n_keep, "n_keep")
    c, mem, dev = _ctx_for([a_A], ctx)
    batch, R, Cc = a_A.batch, a_A.R, a_A.C
    pU, fU = _out(mem == DEVICE, batch, R, keep, np.complex128, dev)
    pV, fV = _out(mem == DEVICE, batch, Cc, keep, np.complex128, dev)
    ps, fs = _out(mem == DEVICE, batch, keep, 1, np.float64, dev)
    prk, rk = _vec_out(mem == DEVICE, batch, np.int32, dev) if info else (None, None)
    pcv, cv = _vec_out(mem == DEVICE, batch, np.int32, dev) if info else (None, None)
    fn = getattr(c._lib, entry)
    for t0, nb in _f64_chunks(batch, per_matrix(a_A, keep, mem)):
        check(fn(c.handle, R, Cc, nb, _off(a_A.ptr, t0 * R * Cc, 16), keep, _off(pU, t0 * R * keep, 16),
                 _off(ps, t0 * keep, 8), _off(pV, t0 * Cc * keep, 16), _off(prk, t0, 4), _off(pcv, t0, 4), mem),
              entry)
    sq = not a_A.batched
    sv = fs(False)[:, :, 0]
    out = (fU(sq), sv[0] if sq else sv, fV(sq))
    if not info:
        return out
    return out + ((rk, cv) if a_A.batched else (rk[0], cv[0]))


def _lowrank_call(entry, per_matrix, A, R, info, ctx):
    """lowrank_f64 / lowrank_tall_f64"""
    a_A, rr = _svd_arg(A, R, "R")
    c, mem, dev = _ctx_for([a_A], ctx)
    batch, Rw, Cc = a_A.batch, a_A.R, a_A.C
    pX, fX = _out(mem == DEVICE, batch, Rw, Cc, np.complex128, dev)
    ptl, tl = _vec_out(mem == DEVICE, batch, np.float64, dev) if info else (None, None)
    per = per_matrix(a_A, min(rr + 1, min(Rw, Cc)), HOST) + (16 * Rw * Cc if mem == HOST else 0) + 32 * Rw * Cc
    fn = getattr(c._lib, entry)
    for t0, nb in _f64_chunks(batch, per):
        check(fn(c.handle, Rw, Cc, nb, _off(a_A.ptr, t0 * Rw * Cc, 16), rr, _off(pX, t0 * Rw * Cc, 16), _off(ptl, t0, 8), mem), entry)
    X = fX(not a_A.batched)
    if not info:
        return X
    return (X, tl) if a_A.batched else (X, tl[0])


def svd_f64(A, n_keep=None, *, info=False, ctx=None):
    """``[U,S,V] = svd(A,'econ')`` in float64 on the device (include/jstsp.h: jstsp_svd_f64): returns ``(U, s, V)`` with
    ``A = U @ diag(s) @ V^H`` - ``V``, not ``V^H``, as MATLAB does - or their leading ``n_keep`` columns / values.  ``A``:
    (rows, cols) or (batch, rows, cols), numpy or a column-major torch CUDA tensor; complex64 / real inputs are widened exactly;
    ``U`` (.., rows, n_keep) and ``V`` (.., cols, n_keep) complex128, ``s`` (.., n_keep) float64 descending, where ``A`` lives.
    One-sided Jacobi on the matrix itself, no Gram matrix: one launch with the matrix in LDS for min(rows, cols) <= 64 and
    shapes such as 64 x 64, 32 x 140, 128 x 50; the global-memory route of :func:`pinv_f64` up to 512 x 8192; anything larger
    raises ``JstspError`` (code -3).  ``info=True`` also returns ``rank`` (int32, the singular values ``pinv``'s drop rule
    keeps; the long-side factor has zero columns from there on) and ``converged`` (int32, 0 where the sweep cap ended the
    iteration), one entry per matrix.  A non-finite entry gives NaN for its own matrix.  A batch whose workspace would exceed
    the library's 24 GiB limit is computed in chunks."""
    return _svd_call("jstsp_svd_f64", _svd_per_matrix, A, n_keep, info, ctx)


def lowrank_f64(A, R, *, info=False, ctx=None):
    """The best rank-``R`` approximation of ``A`` in the spectral and Frobenius norms, ``sum_{k < R} s_k u_k v_k^H`` of
    :func:`svd_f64`'s factors (jstsp_lowrank_f64), complex128, where ``A`` lives; arguments, limits and chunking as
    :func:`svd_f64`, ``1 <= R <= min(rows, cols)``.  ``info=True`` also returns ``tail``: float64, ``s_{R+1}`` per matrix (0 for
    ``R = min(rows, cols)``), which is ``||A - X||_2``."""
    return _lowrank_call("jstsp_lowrank_f64", _svd_per_matrix, A, R, info, ctx)


def _svd_tall_per_matrix(a_A, keep, mem):
    """bytes of workspace per matrix on the QR route (csrc/svd64.hip, tall_layout): the staged copies of a host call, the
    reflector tails (the operand's size), three doubles per chunk and column, the top block, its correction and the flag"""
    m, n = max(a_A.R, a_A.C), min(a_A.R, a_A.C)
    chunk = 128 if n <= 48 else 64
    per = 16 * (a_A.R * a_A.C + (a_A.R + a_A.C) * keep) + 8 * keep + 8 if mem == HOST else 0
    return per + 16 * m * n + 24 * n * (-(-m // chunk)) + 16 * (n * keep + keep * keep) + 4 + 2048


def svd_tall_f64(A, n_keep=None, *, info=False, ctx=None):
    """:func:`svd_f64` for ``min(rows, cols) <= 64`` and a long side up to 65536 (include/jstsp.h: jstsp_svd_tall_f64): the
    same arguments, results and conventions.  Always the QR route, whatever the shape: a streaming Householder reduction to the
    n x n triangle with the reflectors kept, the one-sided Jacobi with vectors on the triangle, the reflectors applied back to
    its left vectors, and a first-order correction that keeps the long-side factor orthonormal to rounding level.  ``rank``
    follows ``pinv``'s drop rule with the long side of ``A``.  Anything larger raises ``JstspError`` (code -3); a batch whose
    workspace (the operand's size again per matrix for the reflectors) would exceed 24 GiB is computed in chunks."""
    return _svd_call("jstsp_svd_tall_f64", _svd_tall_per_matrix, A, n_keep, info, ctx)


def lowrank_tall_f64(A, R, *, info=False, ctx=None):
    """:func:`lowrank_f64` on the factors of :func:`svd_tall_f64` (jstsp_lowrank_tall_f64): ``min(rows, cols) <= 64``, a long
    side up to 65536."""
    return _lowrank_call("jstsp_lowrank_tall_f64", _svd_tall_per_matrix, A, R, info, ctx)


def ls_estimate_f64(Y, A, B, *, info=False, ctx=None):
    """``pinv(A)*Y*pinv(B)`` (plot_errorVSsnr.m:83) in float64 on the device (jstsp_ls_f64): :func:`pinv_f64` of every
    factor - a 2-D ``A`` / ``B`` is shared by the batch and inverted once - and two products on the f64 matrix pipe.
    complex128 out; ``info=True`` also returns ``rcond``: float64 (2,), the smallest over the ``A`` and over the ``B`` factors."""
    a_Y, a_A, a_B = _Arg(_wide(Y), np.complex128, "Y"), _Arg(_wide(A), np.complex128, "A"), _Arg(_wide(B), np.complex128, "B")
    batch, N, M, Gr, G2 = a_Y.batch, a_Y.R, a_Y.C, a_A.C, a_B.R
    if a_A.R != N or a_B.C != M:
        raise ValueError("shape mismatch")
    c, mem, dev = _ctx_for([a_Y, a_A, a_B], ctx)
    p, f = _out(mem == DEVICE, batch, Gr, G2, np.complex128, dev)
    prc, rc = _vec_out(mem == DEVICE, 2, np.float64, dev) if info else (None, None)
    check(c._lib.jstsp_ls_f64(c.handle, N, M, Gr, G2, batch, a_Y.ptr, a_A.ptr, _shared_stride(a_A, N * Gr, batch, "A"),
                              a_B.ptr, _shared_stride(a_B, G2 * M, batch, "B"), p, prc, mem), "jstsp_ls_f64")
    S = f(not a_Y.batched)
    return (S, rc) if info else S


def mmv_omp_f64(A, Y, K, *, norm="l2", ctx=None):
    """:func:`mmv_omp` in float64 on the device (include/jstsp.h: jstsp_mmv_omp_f64): residual, basis, scores, least squares
    and ``Z`` are doubles, nothing is narrowed.  complex64 inputs are widened exactly; ``Z`` is complex128, where the inputs
    live.  Returns (Z (Gr, S), support (1-based atoms in selection order, 0 beyond the count), count)."""
    a_A, a_Y = _Arg(_wide(A), np.complex128, "A"), _Arg(_wide(Y), np.complex128, "Y")
    batch, N, S, Gr = a_Y.batch, a_Y.R, a_Y.C, a_A.C
    if a_A.R != N:
        raise ValueError("size(A,1) must equal size(Y,1)")
    if norm not in ("l2", "l1"):
        raise ValueError("norm must be 'l2' or 'l1'")
    c, mem, dev = _ctx_for([a_A, a_Y], ctx)
    pz, fz = _out(mem == DEVICE, batch, Gr, S, np.complex128, dev)
    pi, fi = _out(mem == DEVICE, batch, int(K), 1, np.int32, dev)
    pc, fc = _out(mem == DEVICE, batch, 1, 1, np.int32, dev)
    check(c._lib.jstsp_mmv_omp_f64(c.handle, N, Gr, S, batch, a_A.ptr, _shared_stride(a_A, N * Gr, batch, "A"), a_Y.ptr,
                                   int(K), 1 if norm == "l1" else 2, pz, pi, pc, mem), "jstsp_mmv_omp_f64")
    sq = not a_Y.batched
    return fz(sq), fi(sq)[..., 0], fc(sq)[..., 0, 0]


def mc_svt_f64(OH, Omega, Imax, tau, rho, *, ctx=None):
    """benchmark_algorithms/mc_svt.m:1 in float64 on the device (jstsp_mc_svt_f64); complex128 out."""
    a_O, a_om = _Arg(_wide(OH), np.complex128, "OH"), _Arg(_wide(Omega, real=True), np.float64, "Omega")
    if (a_om.batch, a_om.R, a_om.C) != (a_O.batch, a_O.R, a_O.C):
        raise ValueError("Omega must have the shape of OH")
    c, mem, dev = _ctx_for([a_O, a_om], ctx)
    t, pt = _scalars(tau, a_O.batch, "tau")
    r, pr = _scalars(rho, a_O.batch, "rho")
    p, f = _out(mem == DEVICE, a_O.batch, a_O.R, a_O.C, np.complex128, dev)
    check(c._lib.jstsp_mc_svt_f64(c.handle, a_O.R, a_O.C, a_O.batch, a_O.ptr, a_om.ptr, int(Imax), pt, pr, p, mem),
          "jstsp_mc_svt_f64")
    return f(not a_O.batched)


def mc_admm_f64(Htrue, OH, Omega, Imax, tau, rho, *, want_ce=True, ctx=None):
    """benchmark_algorithms/mc_admm.m:1 in float64 on the device (jstsp_mc_admm_f64) - returns (X complex128,
    convergence_error (batch, Imax) float64, ``None`` with ``want_ce=False``: ``Htrue`` may then be ``None``)."""
    a_H = _Arg(_wide(Htrue) if want_ce else None, np.complex128, "Htrue", allow_none=not want_ce)
    a_O, a_om = _Arg(_wide(OH), np.complex128, "OH"), _Arg(_wide(Omega, real=True), np.float64, "Omega")
    if (a_om.batch, a_om.R, a_om.C) != (a_O.batch, a_O.R, a_O.C) or (want_ce and (a_H.batch, a_H.R, a_H.C) != (a_O.batch, a_O.R, a_O.C)):
        raise ValueError("Omega and Htrue must have the shape of OH")
    c, mem, dev = _ctx_for([a_H, a_O, a_om], ctx)
    t, pt = _scalars(tau, a_O.batch, "tau")
    r, pr = _scalars(rho, a_O.batch, "rho")
    p, f = _out(mem == DEVICE, a_O.batch, a_O.R, a_O.C, np.complex128, dev)
    pce, fce = _out(mem == DEVICE, a_O.batch, int(Imax), 1, np.float64, dev) if want_ce else (None, None)
    check(c._lib.jstsp_mc_admm_f64(c.handle, a_O.R, a_O.C, a_O.batch, a_H.ptr, a_O.ptr, a_om.ptr, int(Imax), pt, pr, p, pce,
                                   mem), "jstsp_mc_admm_f64")
    sq = not a_O.batched
    return f(sq), (fce(sq)[..., 0] if want_ce else None)


def tssr_f64(Y_prop, Omega, A, B, Imax, tau, rho, K, *, norm="l2", ctx=None):
    """:func:`tssr` in float64 on the device, at every driver size (``pinv_f64`` has no in-LDS limit): returns
    (S_tssr, Y_svt, S_svt) as complex128 with ``Y_svt = mc_svt_f64(...)``, ``S_svt = pinv(A)*Y_svt*pinv(B)`` from
    ``ls_estimate_f64`` and ``S_tssr`` the float64 joint OMP of ``Y_svt*pinv_f64(B)`` on ``A``."""
    Y_svt = mc_svt_f64(Y_prop, Omega, Imax, tau, rho, ctx=ctx)
    PB = pinv_f64(B, ctx=ctx)
    n = Y_svt.shape[-2]
    if _is_torch(Y_svt):
        import torch
        eye = colmajor(torch.eye(n, dtype=torch.complex128, device=Y_svt.device))
    else:
        eye = np.eye(n, dtype=np.complex128)
    T = synthesize_f64(Y_svt, eye, PB, ctx=ctx)               # Y_svt*pinv(B)  (:160)
    S_svt = ls_estimate_f64(Y_svt, A, B, ctx=ctx)             # pinv(A)*Y_svt*pinv(B)  (:151)
    Z, _, _ = mmv_omp_f64(A, T, K, norm=norm, ctx=ctx)
    return Z, Y_svt, S_svt


def _vec3(v):
    """a vector (n,) or a batch of vectors (batch, n) as (batch, n, 1), column-major for torch: (array, single)."""
    single = v.ndim == 1
    v3 = v.reshape(1, -1, 1) if single else v.reshape(v.shape[0], -1, 1)
    return (colmajor(v3) if _is_torch(v) else v3), single


def OMP_f64(A, v, m, snr=None, *, want_target=True, ctx=None):
    """:func:`OMP` in float64 on the device (include/jstsp.h: jstsp_omp_f64): residual, basis, correlations, scores and the
    least squares are doubles, nothing is narrowed.  Same arguments; complex64 inputs are widened exactly, ``x_hat`` and
    ``targetMatrix`` are complex128, where the inputs live.  A batch whose float64 workspace would exceed the library's limit
    is solved in chunks.  Returns (x_hat, indexSet, v, targetMatrix)."""
    a_A = _Arg(_wide(A), np.complex128, "A")
    v3, single = _vec3(_wide(v))
    a_v = _Arg(v3, np.complex128, "v")
    batch, meas, size_d, m = a_v.batch, a_A.R, a_A.C, int(m)
    if a_v.R != meas:
        raise ValueError("length(v) must equal size(A,1)")
    if m < 1:
        raise ValueError("m must be at least 1")
    sA = _shared_stride(a_A, meas * size_d, batch, "A")
    c, mem, dev = _ctx_for([a_A, a_v], ctx)
    px, fx = _out(mem == DEVICE, batch, size_d, 1, np.complex128, dev)
    pi, fi = _out(mem == DEVICE, batch, m, 1, np.int32, dev)
    pt, ft = _out(mem == DEVICE, batch, meas, m, np.complex128, dev) if want_target else (None, None)
    # bytes of float64 state per problem (csrc/omp64.hip): residual, basis, triangular factor, correlations, staged copies
    per = 16 * (2 * meas + meas * m + m * m + m + 2 * size_d + (meas * size_d if sA else 0) + (meas * m if want_target else 0)) + 16 * m
    for t0, nb in _f64_chunks(batch, per):
        check(c._lib.jstsp_omp_f64(c.handle, meas, size_d, nb, _off(a_A.ptr, t0 * sA, 16), sA, _off(a_v.ptr, t0 * meas, 16), m,
                                   _off(px, t0 * size_d, 16), _off(pi, t0 * m, 4), _off(pt, t0 * meas * m, 16), mem), "jstsp_omp_f64")
    return fx(single)[..., 0], fi(single)[..., 0], v, (ft(single) if want_target else None)


def omp_kron_f64(Af, Bf, y, m, *, ctx=None):
    """:func:`omp_kron` in float64 on the device (jstsp_omp_kron_f64): OMP.m on ``kron(Bf.', Af)`` given by its factors, the
    correlation ``Af' R Bf'`` on the f64 matrix pipe; complex128 out.  Returns (x_hat (Gr*G2), indexSet (1-based))."""
    a_A, a_B = _Arg(_wide(Af), np.complex128, "Af"), _Arg(_wide(Bf), np.complex128, "Bf")
    y3, single = _vec3(_wide(y))
    a_y = _Arg(y3, np.complex128, "y")
    batch, N, Gr, G2, M, m = a_y.batch, a_A.R, a_A.C, a_B.R, a_B.C, int(m)
    if a_y.R != N * M:
        raise ValueError("length(y) must be N*M")
    if m < 1:
        raise ValueError("m must be at least 1")
    sA, sB = _shared_stride(a_A, N * Gr, batch, "Af"), _shared_stride(a_B, G2 * M, batch, "Bf")
    c, mem, dev = _ctx_for([a_A, a_B, a_y], ctx)
    px, fx = _out(mem == DEVICE, batch, Gr * G2, 1, np.complex128, dev)
    pi, fi = _out(mem == DEVICE, batch, m, 1, np.int32, dev)
    per = 16 * (2 * N * M + N * M * m + m * m + m + 2 * Gr * G2 + 17 * Gr * M + sA + sB) + 16 * m
    for t0, nb in _f64_chunks(batch, per):
        check(c._lib.jstsp_omp_kron_f64(c.handle, N, M, Gr, G2, nb, _off(a_A.ptr, t0 * sA, 16), sA, _off(a_B.ptr, t0 * sB, 16), sB,
                                        _off(a_y.ptr, t0 * N * M, 16), m, _off(px, t0 * Gr * G2, 16), _off(pi, t0 * m, 4), mem),
              "jstsp_omp_kron_f64")
    return fx(single)[..., 0], fi(single)[..., 0]


def sparse_admm_f64(Htrue, OH, Dr, Dt, Imax, *, want_ce=True, ctx=None):
    """:func:`sparse_admm` in float64 on the device (jstsp_sparse_admm_f64) - returns (S complex128, convergence_error
    (batch, Imax) float64, ``None`` with ``want_ce=False``: ``Htrue`` may then be ``None``).  ``Dr`` and ``Dt`` are square
    (the reference adds R to Z) and shared by the batch; a NaN or Inf in them raises ``JstspError`` (code -6)."""
    a_H = _Arg(_wide(Htrue) if want_ce else None, np.complex128, "Htrue", allow_none=not want_ce)
    a_O = _Arg(_wide(OH), np.complex128, "OH")
    a_Dr, a_Dt = _Arg(_wide(Dr), np.complex128, "Dr"), _Arg(_wide(Dt), np.complex128, "Dt")
    if a_Dr.batched or a_Dt.batched:
        raise ValueError("Dr and Dt are shared by the batch (2-D)")
    batch, Mr, Mt, Imax = a_O.batch, a_O.R, a_O.C, int(Imax)
    if (a_Dr.R, a_Dr.C) != (Mr, Mr) or (a_Dt.R, a_Dt.C) != (Mt, Mt):
        raise ValueError("Dr must be size(OH,1) x size(OH,1) and Dt size(OH,2) x size(OH,2) (sparse_admm.m:21 adds R to Z)")
    if want_ce and (a_H.batch, a_H.R, a_H.C) != (batch, Mr, Mt):
        raise ValueError("Htrue must have the shape of OH")
    if Imax < 0:
        raise ValueError("Imax must not be negative")
    c, mem, dev = _ctx_for([a_H, a_O, a_Dr, a_Dt], ctx)
    p, f = _out(mem == DEVICE, batch, Mr, Mt, np.complex128, dev)
    pce, fce = _out(mem == DEVICE, batch, Imax, 1, np.float64, dev) if want_ce else (None, None)
    n = min(Mr, Mt)
    per = 16 * (10 * Mr * Mt + (6 * n * n + 16 * Mr * Mt if want_ce else 0)) + 8 * Imax
    for t0, nb in _f64_chunks(batch, per):
        check(c._lib.jstsp_sparse_admm_f64(c.handle, Mr, Mt, a_Dr.C, a_Dt.C, nb, _off(a_H.ptr, t0 * Mr * Mt, 16), _off(a_O.ptr, t0 * Mr * Mt, 16),
                                           a_Dr.ptr, a_Dt.ptr, Imax, _off(p, t0 * Mr * Mt, 16), _off(pce, t0 * Imax, 8), mem),
              "jstsp_sparse_admm_f64")
    sq = not a_O.batched
    return f(sq), (fce(sq)[..., 0] if want_ce else None)


# ----------------------------------------------------------------------------- scoring a float64 estimate
def _score_f64_call(entry, S, Zbar, extra, ctx):
    if _is_torch(Zbar):
        import torch
        if Zbar.dtype == torch.complex64:                       # what build_trials returns: widened on the device (exact)
            Zbar = Zbar.to(torch.complex128)
    a_S, a_Z = _Arg(S, np.complex128, "S"), _Arg(Zbar, np.complex128, "Zbar")
    if (a_S.batch, a_S.R, a_S.C) != (a_Z.batch, a_Z.R, a_Z.C):
        raise ValueError("S and Zbar must have the same shape")
    c, mem, dev = _ctx_for([a_S, a_Z], ctx)
    batch, R, Cc = a_S.batch, a_S.R, a_S.C
    if mem == DEVICE:
        import torch
        out = torch.empty(batch, dtype=torch.float64, device=dev)
        optr = out.data_ptr()
    else:
        out = np.empty(batch, dtype=np.float64)
        optr = out.ctypes.data
    m, n = max(R, Cc), min(R, Cc)
    # bytes of workspace per trial (csrc/svdvals.hip): the staged copies of host operands, the values; above order 64 the
    # difference, its rotated copy and V
    per = (2 * 16 * R * Cc if mem == HOST else 0) + 8 * (n + 2)
    if n > 64:
        per += 16 * (R * Cc + m * n + n * n)
    fn = getattr(c._lib, entry)
    for t0, nb in _f64_chunks(batch, per):
        check(fn(c.handle, R, Cc, nb, _off(a_S.ptr, t0 * R * Cc, 16), _off(a_Z.ptr, t0 * R * Cc, 16), *extra, _off(optr, t0, 8), mem), entry)
    return out if a_S.batched else out[0]


def nmse_spectral_f64(S, Zbar, *, ctx=None):
    """:func:`nmse_spectral` for a float64 estimate, without narrowing (``jstsp_nmse_spectral_f64``, csrc/svdvals.hip):
    ``min(1, (norm(S-Zbar, 2) / norm(Zbar, 2))^2)`` from float64 singular values of ``S - Zbar`` and ``Zbar`` themselves - no Gram
    matrix, so an error 1e-9 of ``Zbar`` keeps its digits.  ``S``: (R, C) or (batch, R, C), numpy or a column-major torch CUDA
    tensor, complex128; ``Zbar`` likewise, and a complex64 CUDA ``Zbar`` (what ``build_trials`` returns) is widened on the
    device.  Shapes of :func:`spectrum`, else ``JstspError`` (code -3).  Returns float64 (batch,) where ``S`` lives; a non-finite
    entry gives NaN for its own trial."""
    return _score_f64_call("jstsp_nmse_spectral_f64", S, Zbar, (), ctx)


def rate_f64(S, Zbar, noise_var, *, ctx=None):
    """:func:`rate` for a float64 estimate, without narrowing (``jstsp_rate_f64``): ``sum_k log2(1 + sigma_k(Zbar)^2 / (R (noise_var +
    e)))`` = ``log2(real(det(eye(R) + 1/R*Zbar*Zbar'/(noise_var + e))))`` with ``e`` the uncapped spectral-norm NMSE of ``S`` and R
    the rows of ``Zbar``.  Arguments and result as :func:`nmse_spectral_f64`; ``noise_var`` >= 0."""
    return _score_f64_call("jstsp_rate_f64", S, Zbar, (float(noise_var),), ctx)


# ----------------------------------------------------------------------------- the order of a support
def _support_order_call(entry, S, np_dtype, ctx):
    a_S = _Arg(S, np_dtype, "S")
    c, mem, dev = _ctx_for([a_S], ctx)
    batch, Gr, G2 = a_S.batch, a_S.R, a_S.C
    if mem == DEVICE:
        import torch
        out = torch.empty((batch, Gr * G2), dtype=torch.int32, device=dev)
        optr = out.data_ptr()
    else:
        out = np.empty((batch, Gr * G2), dtype=np.int32)
        optr = out.ctypes.data
    check(getattr(c._lib, entry)(c.handle, Gr, G2, batch, a_S.ptr, optr, mem), entry)
    return out


def support_order(S, *, ctx=None):
    """``[~, indx_S] = sort(abs(vec(S)), 'descend')`` per trial (plot_errorVSsnr.m:143) on the device
    (``jstsp_support_order_c32``, csrc/support.hip): what ``proposed_algorithm_angles`` takes as ``indx_S``, from an ``S`` that
    need not be the true channel's - in a tracker, the previous frame's estimate.  ``S``: (Gr, G2) or (batch, Gr, G2), numpy or a
    column-major torch CUDA tensor, complex64.  Returns int32 (batch, Gr*G2), 1-based column-major linear indices, where ``S``
    lives.  The key is ``|z|^2`` in fp32 - the trial builder's, so ``support_order(Zbar)`` is ``build_trials``' ``indx_S`` on the
    bits; equal keys (the exact zeros of a thresholded ``S``) come in ascending index, a NaN first, then Inf."""
    return _support_order_call("jstsp_support_order_c32", S, np.complex64, ctx)


def support_order_f64(S, *, ctx=None):
    """:func:`support_order` for a complex128 ``S`` without narrowing (``jstsp_support_order_f64``): the key is ``|z|^2`` in
    float64.  Arguments and result as :func:`support_order`."""
    return _support_order_call("jstsp_support_order_f64", S, np.complex128, ctx)


def support_top_f64(S, count, *, ctx=None):
    """The first ``count`` entries of :func:`support_order_f64` per trial, bit for bit, without sorting the trial
    (``jstsp_support_top_f64``, csrc/support_top.hip): one selection kernel - a radix select of the ``count``-th key, the ties in
    index order, a sort of the selected entries in LDS - which is what :func:`proposed_algorithm_refresh_f64` runs inside its
    loop.  ``S`` as :func:`support_order_f64` takes it; ``1 <= count <= min(Gr*G2, 4096)`` (``JstspError`` code -4 otherwise).
    Returns int32 (batch, count), 1-based column-major linear indices, where ``S`` lives."""
    return _support_top_call("jstsp_support_top_f64", S, count, np.complex128, ctx)


def support_top(S, count, *, ctx=None):
    """The first ``count`` entries of :func:`support_order` per trial, bit for bit, without sorting the trial
    (``jstsp_support_top_c32``): :func:`support_top_f64`'s selection kernel on the 32-bit key ``|z|^2`` in fp32, which is what
    :func:`proposed_algorithm_refresh` runs inside its loop.  ``S`` as :func:`support_order` takes it (complex64);
    ``1 <= count <= min(Gr*G2, 4096)`` (``JstspError`` code -4 otherwise).  Returns int32 (batch, count), 1-based column-major
    linear indices, where ``S`` lives."""
    return _support_top_call("jstsp_support_top_c32", S, count, np.complex64, ctx)


def _support_top_call(entry, S, count, np_dtype, ctx):
    count = int(count)
    a_S = _Arg(S, np_dtype, "S")
    c, mem, dev = _ctx_for([a_S], ctx)
    batch, Gr, G2 = a_S.batch, a_S.R, a_S.C
    rows = max(count, 1)
    if mem == DEVICE:
        import torch
        out = torch.empty((batch, rows), dtype=torch.int32, device=dev)
        optr = out.data_ptr()
    else:
        out = np.empty((batch, rows), dtype=np.int32)
        optr = out.ctypes.data
    check(getattr(c._lib, entry)(c.handle, Gr, G2, batch, a_S.ptr, count, optr, mem), entry)
    return out


_WIDE_PRIMARY = {"neighbourhood": 0, "ties": 1}


def _support_order_wide_call(entry, S, Gt, wr, wt, primary, np_dtype, ctx):
    if primary not in _WIDE_PRIMARY:
        raise ValueError("primary must be 'neighbourhood' or 'ties', not %r" % (primary,))
    Gt, wr, wt = int(Gt), int(wr), int(wt)
    a_S = _Arg(S, np_dtype, "S")
    if Gt < 1 or a_S.C % Gt:
        raise ValueError("Gt = %d must divide the %d columns of S (column l*Gt + g is transmit cell g of delay tap l)" % (Gt, a_S.C))
    c, mem, dev = _ctx_for([a_S], ctx)
    batch, Gr, G2 = a_S.batch, a_S.R, a_S.C
    if mem == DEVICE:
        import torch
        out = torch.empty((batch, Gr * G2), dtype=torch.int32, device=dev)
        optr = out.data_ptr()
    else:
        out = np.empty((batch, Gr * G2), dtype=np.int32)
        optr = out.ctypes.data
    check(getattr(c._lib, entry)(c.handle, Gr, Gt, G2 // Gt, batch, a_S.ptr, wr, wt, _WIDE_PRIMARY[primary], optr, mem), entry)
    return out


def support_order_wide(S, Gt, wr=1, wt=1, *, primary="neighbourhood", ctx=None):
    """:func:`support_order` widened over neighbouring angle cells (``jstsp_support_order_wide_c32``, csrc/support.hip): a support
    that can follow a peak which moves a cell per frame.  ``S`` and the result as :func:`support_order`; column ``l*Gt + g`` of ``S``
    is transmit cell ``g`` of delay tap ``l``, so ``Gt`` must divide the column count.  With ``own`` the key of an entry and ``nbr``
    the smallest key (largest magnitude) of its ``(2 wr + 1) x (2 wt + 1)`` window - circular in both angle grids, inside its own
    delay tap - the order is ascending ``(nbr, own, index)`` for ``primary="neighbourhood"`` (a strong entry, then its window) and
    ``(own, nbr, index)`` for ``"ties"`` (the plain order; equal keys, the exact zeros of a thresholded ``S``, by their strongest
    neighbour).  ``wr = wt = 0`` is :func:`support_order` on the bits.  ``ValueError`` for a ``Gt`` that does not divide the columns
    or an unknown ``primary``, before anything touches a device; ``JstspError`` (code -4) for a negative radius or a window wider
    than its grid, (code -2) for more than 2^21 entries per trial."""
    return _support_order_wide_call("jstsp_support_order_wide_c32", S, Gt, wr, wt, primary, np.complex64, ctx)


def support_order_wide_f64(S, Gt, wr=1, wt=1, *, primary="neighbourhood", ctx=None):
    """:func:`support_order_wide` for a complex128 ``S`` without narrowing (``jstsp_support_order_wide_f64``): the key is ``|z|^2``
    in float64.  Arguments and result as :func:`support_order_wide`."""
    return _support_order_wide_call("jstsp_support_order_wide_f64", S, Gt, wr, wt, primary, np.complex128, ctx)


# ----------------------------------------------------------------------------- a least-squares re-fit of an estimate on its support
REFIT_ITERS = 20        # the default of refit_f64: see its docstring


def refit_f64(subY, Omega, A, B, S, K, iters=REFIT_ITERS, lam=0.0, tol=0.0, indx_S=None, return_resid=False, *, ctx=None):
    """A float64 least-squares re-fit of the estimate ``S`` on ``K`` of its entries (include/jstsp.h: jstsp_refit_f64, DESIGN.md
    section 9v): ``iters`` conjugate-gradient steps, started from ``S`` restricted to its support, on the normal equations of
    ``min ||Omega .* (A S B) - subY||_F^2 + lam ||S||_F^2`` over the entries of the support.  A stage after a solve - the ADMM takes
    one steepest-descent step per iteration, so its ``S`` is not the fit on its own strong entries; nothing of the solver changes.

    ``subY``, ``Omega``, ``A``, ``B`` as :func:`proposed_algorithm_f64` takes them (widened exactly), ``S`` (Gr, G2) or (batch, Gr,
    G2) complex128 of the kind of the other arrays.  The support is the first ``K`` entries of ``indx_S`` - 1-based column-major
    linear indices, ``(n,)`` or ``(batch, n)`` with ``K <= n <= Gr*G2``, e.g. the builder's genie order - or, with ``indx_S=None``,
    of :func:`support_order_f64` of ``S`` itself, taken by the selection kernel of :func:`support_top_f64` (``K <= 4096``).
    ``K == Gr*G2`` fits every entry.  ``tol > 0`` freezes a trial once its squared residual has fallen to ``tol^2`` of its first;
    a trial also freezes when the residual is exactly zero or a search direction has no positive curvature.  ``K`` and ``iters``
    are regularisers: with every entry and many steps the fit follows the noise.

    Returns ``(S_fit, steps)`` - complex128 like ``S`` and int32 ``(batch,)``, the steps each trial took - and with
    ``return_resid`` also ``resid`` float64 ``(batch, iters + 1)``: the squared residual ``gamma_0 ... gamma_iters`` of the normal
    equations, NaN after a trial's last step.  For one unbatched problem the batch axis is dropped from all three.  A repeated
    call returns the same bits, and a trial's bits do not depend on the batch.  ``ValueError`` for a bad ``K``, ``iters``, ``lam``,
    ``tol`` or ``indx_S`` before anything touches a device.

    The default ``iters`` = 20 is the largest count measured on the device (5, 10 and 20 steps at 256 trials),
    and for ``K >= 2048`` at the 64 x 4096, 64 x 512 shape the NMSE was still falling there: 20 is the best measured, not a measured
    optimum, and a larger count may do better.  ``K`` has no default."""
    K, iters, lam, tol = int(K), int(iters), float(lam), float(tol)
    a_sub = _Arg(_wide(subY), np.complex128, "subY")
    a_om = _Arg(_wide(Omega, real=True), np.float64, "Omega")
    a_A, a_B = _Arg(_wide(A), np.complex128, "A"), _Arg(_wide(B), np.complex128, "B")
    a_S = _Arg(S, np.complex128, "S")
    batch, N, M, Gr, G2 = a_sub.batch, a_sub.R, a_sub.C, a_A.C, a_B.R
    g = Gr * G2
    if (a_om.batch, a_om.R, a_om.C) != (batch, N, M):
        raise ValueError("Omega must have the shape of subY")
    if a_A.R != N or a_B.C != M:
        raise ValueError("size(A,1) must equal size(subY,1) and size(B,2) must equal size(subY,2)")
    if (a_S.batch, a_S.R, a_S.C) != (batch, Gr, G2) or a_S.batched != a_sub.batched:
        raise ValueError("S must be (Gr, G2) = (%d, %d) per problem, batched as subY is" % (Gr, G2))
    if not 1 <= K <= g:
        raise ValueError("K = %d: need 1 <= K <= Gr*G2 = %d" % (K, g))
    if iters < 1:
        raise ValueError("iters = %d: need at least 1" % iters)
    if not lam >= 0.0 or not tol >= 0.0:
        raise ValueError("lam = %r, tol = %r: neither may be negative or NaN" % (lam, tol))
    n = 0
    if indx_S is None:
        if K != g and K > _lib.SUPPORT_TOP_MAX:
            raise ValueError("K = %d without indx_S: the selection kernel lists at most %d entries (or K = Gr*G2 = %d)"
                             % (K, _lib.SUPPORT_TOP_MAX, g))
    else:
        shp = tuple(indx_S.shape)
        if len(shp) not in (1, 2) or (len(shp) == 2 and shp[0] != batch) or (len(shp) == 1 and batch != 1 and a_sub.batched):
            raise ValueError("indx_S must be (n,) for one problem or (batch, n) = (%d, n), got %s" % (batch, shp))
        n = int(shp[-1])
        if not K <= n <= g:
            raise ValueError("indx_S lists %d entries per problem: need K = %d <= n <= Gr*G2 = %d" % (n, K, g))
    a_ix = _indx_arg(indx_S, batch, n)
    sA = _shared_stride(a_A, N * Gr, batch, "A")
    sB = _shared_stride(a_B, G2 * M, batch, "B")
    c, mem, dev = _ctx_for([a_sub, a_om, a_A, a_B, a_S, a_ix], ctx)
    tor = mem == DEVICE
    pS, fS = _out(tor, batch, Gr, G2, np.complex128, dev)
    p_it, steps = _vec_out(tor, batch, np.int32, dev)
    if return_resid:
        if tor:
            import torch
            resid = torch.empty((batch, iters + 1), dtype=torch.float64, device=dev)
            p_rs = resid.data_ptr()
        else:
            resid = np.empty((batch, iters + 1), dtype=np.float64)
            p_rs = resid.ctypes.data
    else:
        resid, p_rs = None, None
    # bytes of workspace per trial (csrc/refit64.hip): x's three companions, the three intermediates, the rank, the partial products of
    # a split product; staged copies of a host call
    per = 16 * (3 * g + N * M + Gr * M + N * G2 + 32 * 4096) + 4 * g + 64
    if mem == HOST:
        per += 16 * (N * M + 2 * g + (N * Gr if sA else 0) + (G2 * M if sB else 0)) + 8 * N * M + 4 * n + 8 * (iters + 2)
    name = "jstsp_refit_f64"
    for t0, nb in _f64_chunks(batch, per):
        check(getattr(c._lib, name)(
            c.handle, N, M, Gr, G2, nb, _off(a_sub.ptr, t0 * N * M, 16), _off(a_om.ptr, t0 * N * M, 8), _off(a_A.ptr, t0 * sA, 16), sA,
            _off(a_B.ptr, t0 * sB, 16), sB, _off(a_S.ptr, t0 * g, 16), _off(a_ix.ptr, t0 * n, 4), n, K, iters, lam, tol,
            _off(pS, t0 * g, 16), _off(p_rs, t0 * (iters + 1), 8), _off(p_it, t0, 4), mem), name)
    sq = not a_sub.batched
    out = (fS(sq), steps[0] if sq else steps)
    return out + ((resid[0] if sq else resid),) if return_resid else out
