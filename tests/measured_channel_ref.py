"""Helper of the supplied-channel tests (not a test module): small synthetic channels and the float64 restatement of what
``jstsp_build_trials_from_channel_c32`` builds from one - the first lines of plot_errorVSsnr_nyuwireless.m (:60-69) in front of
the chain of plot_errorVSsnr.m:57-136, composed of the oracle's own functions only."""
import numpy as np

from oracle import system_model as osm


def _steer(f, n):
    """ULA response at spatial frequency f (cycles per element): on the DFT grid of size G when f = g / G."""
    return np.exp(-2j * np.pi * f * np.arange(n))


def make_channel(Nr_src, Nt_src, L, seed, kind, d=None):
    """Synthetic taps (Nr_src, Nt_src, L) complex128 from a numpy generator - not reference data.

    ``"paths"``: per tap four steering-vector outer products with complex normal gains, two on the DFT grid of the source
    size and two off it.  ``"svd"``: ``U diag(d) V^H`` per tap with Haar-like U, V (QR of complex normal matrices), so that
    norm(H_l) = max(d) is known; ``d``: one sequence for every tap or one per tap (default 1, 1/2, 1/4, ...)."""
    rng = np.random.default_rng(seed)
    cn = lambda *s: rng.standard_normal(s) + 1j * rng.standard_normal(s)
    H = np.zeros((Nr_src, Nt_src, L), complex)
    n = min(Nr_src, Nt_src)
    for l in range(L):
        if kind == "paths":
            for k in range(4):
                gr, gt = int(rng.integers(0, Nr_src)), int(rng.integers(0, Nt_src))
                off = 0.0 if k < 2 else 0.37
                g = cn() / np.sqrt(2)
                H[:, :, l] += g * np.outer(_steer((gr + off) / Nr_src, Nr_src), _steer((gt + off) / Nt_src, Nt_src).conj())
            H[:, :, l] /= 2.0
        elif kind == "svd":
            dl = d if d is None or np.ndim(d[0]) == 0 else d[l]
            dl = 0.5 ** np.arange(n) if dl is None else np.asarray(dl, float)
            U, _ = np.linalg.qr(cn(Nr_src, n))
            V, _ = np.linalg.qr(cn(Nt_src, n))
            H[:, :, l] = (U[:, :dl.size] * dl) @ V[:, :dl.size].conj().T
        else:
            raise ValueError(kind)
    return H


def cut_and_scale(p, H_src, normalize):
    """plot_errorVSsnr_nyuwireless.m:62-67: the leading Nr x Nt block of every tap (:63-64), s = norm(H_l) (:65) and the
    scaling - "reference": rho = 1/norm(H_l)^2, H_l = rho*H_l, lines :65-66 as written; "unit": H_l / s; "asis": none.
    Returns (H (Nr, Nt, L) complex128, s (L,))."""
    H = np.array(np.asarray(H_src)[:p.Nr, :p.Nt, :], dtype=complex)
    assert H.shape == (p.Nr, p.Nt, p.L)
    sig = np.array([np.linalg.norm(H[:, :, l], 2) for l in range(p.L)])
    for l in range(p.L):
        if normalize == "reference":
            rho = 1 / sig[l] ** 2                       # :65
            H[:, :, l] = rho * H[:, :, l]               # :66
        elif normalize == "unit":
            H[:, :, l] = H[:, :, l] / sig[l]
        elif normalize != "asis":
            raise ValueError(normalize)
    return H, sig


def reference_inputs(p, H_src, normalize, draws, with_hbf=False):
    """The dict ``oracle.system_model.training_inputs_errorVSsnr`` returns, for the cut and scaled channel instead of the drawn
    one: ``Zbar_l = Dr' H_l Dt`` (plot_errorVSsnr_nyuwireless.m:67,69), everything after it by the oracle's functions.
    ``p``: SweepParams; ``draws``: dict(noise, qam_idx, omega_rows) as for the oracle.  Adds ``sigma`` (norm of every cut tap)
    and, ``with_hbf``, Y_hbf / A_hbf / B_hbf (plot_errorVSsnr_nyuwireless.m:84-89)."""
    Nt, Nr, L, Gr, Gt, T_prop = p.Nt, p.Nr, p.L, p.Gr, p.Gt, p.T_prop
    H, sig = cut_and_scale(p, H_src, normalize)
    Dr = np.exp(-1j * np.arange(Nr)[:, None] * 2 * np.pi * np.arange(Gr)[None, :] / Gr) / np.sqrt(Nr)   # :58
    Dt = np.exp(-1j * np.arange(Nt)[:, None] * 2 * np.pi * np.arange(Gt)[None, :] / Gt) / np.sqrt(Nt)   # :59
    Z = np.zeros((Gr, Gt, L), complex)
    for l in range(L):
        Z[:, :, l] = Dr.conj().T @ H[:, :, l] @ Dt      # :67
    Zbar = Z.reshape(Gr, L * Gt, order="F")             # :69
    Nn = np.sqrt(p.noise_var / 2) * draws["noise"]      # :72
    alphabet = osm.qam4_alphabet()
    Psi_rows = np.zeros((L, T_prop, Nt), complex)
    for k in range(Nt):                                 # :75-79
        Psi_rows[:, :, k] = osm.toeplitz_rows(alphabet[draws["qam_idx"][k]], L)
    W = osm.create_beamformer(Nr, p.beamformer)         # :135
    Y_prop, W_tilde, Psi_bar, Omega, _ = osm.proposed_hbf(H, Nn, Psi_rows, T_prop, p.Mr_e, p.Mr, W, draws["omega_rows"])   # :136
    tau_Y = 1 / np.linalg.norm(Y_prop, "fro") ** 2      # :138
    tau_Z = 1 / np.linalg.norm(Zbar, "fro") ** 2 / 2    # :139
    rho = p.rho_scale * osm.rho_from_eigs(Y_prop, "max" if p.rho_rule == "max" else "min6")   # :140-141
    A = W_tilde.conj().T @ Dr                           # :143
    B = np.zeros((L * Gt, T_prop), complex)             # :144
    for l in range(L):
        B[l * Gt:(l + 1) * Gt, :] = Dt.conj().T @ Psi_bar[:, :, l]   # :146
    absz = np.abs(Zbar.reshape(-1, order="F"))
    indx_S = np.argsort(-absz, kind="stable") + 1
    out = dict(subY=Y_prop, Omega=Omega, A=A, B=B, tau_Y=float(tau_Y), tau_Z=float(tau_Z), rho=rho, Zbar=Zbar, H=H,
               indx_S=indx_S, sigma=sig)
    if with_hbf:
        Th = p.T_hbf
        Yc, Wc, Psi_bar_c, _ = osm.hbf(H, Nn[:, :Th], Psi_rows[:, :Th, :], Th, Nr, W)       # :84
        out["Y_hbf"] = Yc
        out["A_hbf"] = Wc.conj().T @ Dr                                                        # :85
        out["B_hbf"] = np.concatenate([Dt.conj().T @ Psi_bar_c[:, :, l] for l in range(L)]) if Th else np.zeros((L * Gt, 0), complex)
    return out


def oracle_params(p):
    """``params`` of oracle.system_model.training_inputs_errorVSsnr / draw_trial for a SweepParams."""
    return dict(Nt=p.Nt, Nr=p.Nr, Mr_e=p.Mr_e, Gr=p.Gr, Gt=p.Gt, clusters=p.clusters, rays=p.rays, L=p.L, Mr=p.Mr, T=p.T,
                noise_var=p.noise_var, beamformer=p.beamformer, rho_rule=p.rho_rule, rho_scale=p.rho_scale, T_prop=p.T_prop)
