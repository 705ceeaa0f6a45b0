"""ctypes binding of libjstsp_mi355x.so (the C ABI declared in include/jstsp.h).

There is NO CPU fallback: importing this module without the built library, or creating a
context without an MI355X, raises.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libjstsp_mi355x.so")

HOST, DEVICE = 0, 1
TYPE_APPROXIMATE, TYPE_STD = 0, 1
BF_ZC, BF_DFT, BF_QUANTIZED, BF_QUANTIZED4 = 0, 1, 2, 3
RHO_MIN6, RHO_MAX = 0, 1
PILOTS_QAM4, PILOTS_GAUSS = 0, 1
CHAN_ASIS, CHAN_REFERENCE, CHAN_UNIT = 0, 1, 2

c_void_p, c_int, c_ll, c_dp, c_ip = C.c_void_p, C.c_int, C.c_longlong, C.POINTER(C.c_double), C.POINTER(C.c_int)



class Model(C.Structure):
    """struct jstsp_model (include/jstsp.h)."""
    _fields_ = [(n, c_int) for n in ("Nt", "Nr", "L", "T_prop", "Mr", "Mr_e", "Gr", "Gt", "clusters", "rays",
                                     "T_hbf", "shared_pilots")] + [("noise_var", C.c_double), ("beamformer", c_int),
                                                                   ("rho_rule", c_int), ("rho_scale", C.c_double),
                                                                   ("pilots", c_int)]


class Trials(C.Structure):
    """struct jstsp_trials (include/jstsp.h): output pointers, NULL = not wanted."""
    _fields_ = [(n, c_void_p) for n in ("subY", "Omega", "A", "B", "Zbar", "H", "indx_S")] + \
               [(n, c_dp) for n in ("tau_Y", "tau_Z", "rho")] + \
               [(n, c_void_p) for n in ("Y_hbf", "A_hbf", "B_hbf", "gains", "u_r", "u_t", "noise", "qam_idx", "pilot_sym")]


class AseDesign(C.Structure):
    """jstsp_ase_design (include/jstsp.h): codebook kind, columns, pool (0 = the first n_cols columns)."""
    _fields_ = [("kind", c_int), ("n_cols", c_int), ("pool", c_int)]


# name -> (restype, argtypes); mirrors include/jstsp.h one to one
SIGNATURES = {
    "jstsp_create": (c_int, [c_int, C.POINTER(c_void_p)]),
    "jstsp_destroy": (c_int, [c_void_p]),
    "jstsp_set_stream": (c_int, [c_void_p, c_void_p]),
    "jstsp_use_own_stream": (c_int, [c_void_p]),
    "jstsp_synchronize": (c_int, [c_void_p]),
    "jstsp_last_error": (C.c_char_p, []),
    "jstsp_version": (C.c_char_p, []),
    "jstsp_workspace_bytes": (C.c_size_t, [c_void_p]),
    "jstsp_correlate_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_ll,
                                    c_void_p, c_ll, c_void_p, c_int]),
    "jstsp_synthesize_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_ll,
                                     c_void_p, c_ll, c_void_p, c_int]),
    "jstsp_gradient_head_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_ll, c_void_p, c_ll,
                                        c_void_p, c_void_p, c_void_p, c_int]),
    "jstsp_proposed_algorithm_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                             c_void_p, c_ll, c_void_p, c_ll, c_int, c_dp, c_dp, c_dp, c_int,
                                             c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "jstsp_proposed_algorithm_begin_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                                   c_void_p, c_ll, c_void_p, c_ll, c_int, c_dp, c_dp, c_dp, c_int,
                                                   c_void_p, c_void_p, c_void_p, c_void_p, C.POINTER(c_void_p)]),
    "jstsp_proposed_algorithm_end": (c_int, [c_void_p, c_void_p, c_ip]),
    "jstsp_ls_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_ll, c_void_p, c_ll,
                             c_void_p, c_int]),
    "jstsp_pinv_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int]),
    "jstsp_last_conditioning": (c_int, [c_void_p, c_dp, c_dp]),
    "jstsp_last_fused_fallbacks": (c_int, [c_void_p, c_ip]),
    "jstsp_last_lanczos_mismatches": (c_int, [c_void_p, c_ip]),
    "jstsp_last_dictionary_block": (c_int, [c_void_p, c_ip]),
    "jstsp_svt_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_dp, c_void_p, c_int]),
    "jstsp_omp_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_ll, c_void_p, c_int, c_void_p,
                              c_void_p, c_void_p, c_int]),
    "jstsp_omp_kron_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_ll, c_void_p, c_ll,
                                   c_void_p, c_int, c_void_p, c_void_p, c_int]),
    "jstsp_cosamp_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_ll, c_void_p, c_int, c_int, C.c_double, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "jstsp_cosamp_kron_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_ll, c_void_p, c_ll, c_void_p,
                                      c_int, c_int, C.c_double, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int]),
    "jstsp_mmv_omp_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_ll, c_void_p, c_int, c_int, c_void_p,
                                  c_void_p, c_void_p, c_int]),
    "jstsp_rate_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, C.c_double, c_void_p, c_int]),
    "jstsp_sparse_admm_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                      c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_int]),
    "jstsp_mc_svt_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_dp, c_dp,
                                 c_void_p, c_int]),
    "jstsp_mc_admm_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int, c_dp,
                                  c_dp, c_void_p, c_void_p, c_int]),
    "jstsp_vamp_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_ll, C.c_double, C.c_double, c_int,
                               c_void_p, c_int]),
    "jstsp_vamp_kron_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_ll, c_void_p, c_ll,
                                    C.c_double, C.c_double, c_int, c_void_p, c_int]),
    "jstsp_sparse_sca_estim_f64": (c_int, [c_void_p, c_ll, c_void_p, C.c_double, C.c_double, C.c_double, c_void_p, c_void_p, c_int]),
    "jstsp_cawgn_estim_out_f64": (c_int, [c_void_p, c_ll, c_void_p, c_void_p, C.c_double, C.c_double, c_void_p, c_dp, c_int]),
    "jstsp_lambda_max_sequence_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int]),
    "jstsp_nmse_spectral_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_int]),
    "jstsp_build_trials_c32": (c_int, [c_void_p, C.POINTER(Model), C.c_uint64, c_int, c_ll, c_int, C.POINTER(Trials),
                                       c_int]),
    "jstsp_build_trials_from_channel_c32": (c_int, [c_void_p, C.POINTER(Model), C.c_uint64, c_int, c_ll, c_int, c_void_p, c_int,
                                                    c_int, c_ll, c_int, C.POINTER(Trials), c_dp, c_int]),
    "jstsp_build_trials_tracked_c32": (c_int, [c_void_p, C.POINTER(Model), C.c_uint64, c_int, c_ll, c_int, c_int, C.c_double,
                                               C.POINTER(Trials), c_int]),
    "jstsp_build_trials_tracked_drift_c32": (c_int, [c_void_p, C.POINTER(Model), C.c_uint64, c_int, c_ll, c_int, c_int, C.c_double,
                                                     C.c_double, C.POINTER(Trials), c_void_p, c_void_p, c_int]),
    "jstsp_support_order_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int]),
    "jstsp_support_order_f64": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int]),
    "jstsp_support_order_wide_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int]),
    "jstsp_support_order_wide_f64": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_int, c_int, c_int, c_void_p, c_int]),
    "jstsp_beamformer_c32": (c_int, [c_void_p, c_int, c_int, c_void_p, c_int]),
    "jstsp_ase_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, C.c_double, c_void_p,
                              c_int]),
    "jstsp_ase_trials_c32": (c_int, [c_void_p, C.POINTER(Model), C.POINTER(AseDesign), c_int, C.c_uint64, c_int, c_ll, c_int,
                                     c_void_p, c_void_p, c_int]),
    "jstsp_singular_values_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int]),
    "jstsp_rank_trials_c32": (c_int, [c_void_p, C.POINTER(Model), C.c_uint64, c_int, c_ll, c_int, c_int, c_void_p, c_int]),
    "jstsp_spectrum_c32": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int]),
    "jstsp_spectrum_trials_c32": (c_int, [c_void_p, C.POINTER(Model), C.c_uint64, c_int, c_ll, c_int, c_void_p, c_int, c_int, c_ll,
                                          c_int, c_int, c_void_p, c_dp, c_int]),
    "jstsp_set_profiling": (c_int, [c_void_p, c_int]),
    "jstsp_get_profile": (c_int, [c_void_p, C.c_char_p, c_ip, c_dp]),
}


for _n in ("correlate", "synthesize", "proposed_algorithm", "svt", "omp", "sparse_admm", "mc_svt", "mc_admm", "vamp", "ls", "pinv",
           "mmv_omp", "vamp_kron", "nmse_spectral", "rate", "beamformer", "ase", "singular_values", "spectrum", "cosamp", "cosamp_kron"):
    # the double-complex forms take the same argument lists (pointers are void* here)
    SIGNATURES["jstsp_%s_c64" % _n] = SIGNATURES["jstsp_%s_c32" % _n]


for _n in ("correlate", "synthesize", "proposed_algorithm", "svt"):
    # the float64 solver (csrc/proposed64.hip, csrc/zgemm64.hip): argument lists of the _c64 namesakes
    SIGNATURES["jstsp_%s_f64" % _n] = SIGNATURES["jstsp_%s_c32" % _n]

# pinv and least squares in float64 (csrc/pinv64.hip): the _c64 argument lists plus the rcond / rank outputs
SIGNATURES["jstsp_pinv_f64"] = (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int])
SIGNATURES["jstsp_ls_f64"] = (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_ll, c_void_p, c_ll,
                                      c_void_p, c_void_p, c_int])

# [U,S,V] = svd(A,'econ') and the best rank-R approximation in float64 (csrc/svd64.hip)
SIGNATURES["jstsp_svd_f64"] = (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int])
SIGNATURES["jstsp_lowrank_f64"] = (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_void_p, c_int])
# the same for min(rows, cols) <= 64 and a long side up to 65536: the QR route with the reflectors kept
SIGNATURES["jstsp_svd_tall_f64"] = SIGNATURES["jstsp_svd_f64"]
SIGNATURES["jstsp_lowrank_tall_f64"] = SIGNATURES["jstsp_lowrank_f64"]

# Alg. 1 ('std') in float64 (csrc/proposed64.hip): the jstsp_proposed_algorithm_f64 list with PA, PB for `type` and rcond_out
SIGNATURES["jstsp_proposed_std_f64"] = (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_ll,
                                                c_void_p, c_ll, c_void_p, c_void_p, c_int, c_dp, c_dp, c_dp, c_void_p, c_void_p,
                                                c_void_p, c_void_p, c_void_p, c_int])

# the float64 ADMM resumed from a saved state (csrc/proposed64.hip): the sibling's list with it0, state_in, state_out before memspace
SIGNATURES["jstsp_admm_state_elems"] = (C.c_size_t, [c_int, c_int, c_int, c_int])
for _n, _sib in (("jstsp_proposed_resume_f64", "jstsp_proposed_algorithm_f64"), ("jstsp_proposed_std_resume_f64", "jstsp_proposed_std_f64"),
                 ("jstsp_proposed_resume_c32", "jstsp_proposed_algorithm_c32"), ("jstsp_proposed_resume_c64", "jstsp_proposed_algorithm_c64")):
    SIGNATURES[_n] = (c_int, SIGNATURES[_sib][1][:-1] + [c_int, c_void_p, c_void_p, c_int])

# the head of an order by a selection kernel (csrc/support_top.hip), and the float64 ADMM that refreshes its support with it
# (csrc/proposed64.hip): ... rho, indx_S, n_indx, refresh_start, refresh_period, S, Y, ce, it0, state_in, state_out, indx_out, memspace
SUPPORT_TOP_MAX = 4096
SIGNATURES["jstsp_support_top_f64"] = (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p, c_int])
SIGNATURES["jstsp_proposed_refresh_f64"] = (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_ll,
                                                    c_void_p, c_ll, c_int, c_dp, c_dp, c_dp, c_void_p, c_int, c_int, c_int,
                                                    c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int])
# the float64 ADMM with a stopping rule (csrc/proposed64.hip): the refreshed entry's list with tol, min_iters, check after
# refresh_period and iters_out, ce3_out before memspace
SIGNATURES["jstsp_proposed_until_f64"] = (c_int, SIGNATURES["jstsp_proposed_refresh_f64"][1][:20] + [c_dp, c_int, c_int]
                                          + SIGNATURES["jstsp_proposed_refresh_f64"][1][20:-1] + [c_void_p, c_void_p, c_int])
# the same in fp32 (csrc/support_top.hip, csrc/proposed.hip, csrc/c64.hip): the float64 lists, with `type` after rho as in
# jstsp_proposed_resume_c32 ('std' is refused)
SIGNATURES["jstsp_support_top_c32"] = SIGNATURES["jstsp_support_top_f64"]
for _n in ("jstsp_proposed_refresh_c32", "jstsp_proposed_refresh_c64"):
    SIGNATURES[_n] = (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_ll,
                              c_void_p, c_ll, c_int, c_dp, c_dp, c_dp, c_int, c_void_p, c_int, c_int, c_int,
                              c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int])
# the fp32 ADMM with a stopping rule (csrc/proposed.hip, csrc/until.hip, csrc/c64.hip): the refreshed entry's list with tol, min_iters,
# check after refresh_period and iters_out, ce3_out before memspace
for _n in ("jstsp_proposed_until_c32", "jstsp_proposed_until_c64"):
    SIGNATURES[_n] = (c_int, SIGNATURES["jstsp_proposed_refresh_c32"][1][:21] + [c_dp, c_int, c_int]
                      + SIGNATURES["jstsp_proposed_refresh_c32"][1][21:-1] + [c_void_p, c_void_p, c_int])

# the float64 least-squares re-fit of an estimate on its support (csrc/refit64.hip): ... B, strideB, S_in, indx_S, n_indx, K, iters,
# lam, tol, S_out, resid_out, iters_out, memspace
SIGNATURES["jstsp_refit_f64"] = (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p, c_ll, c_void_p, c_ll,
                                         c_void_p, c_void_p, c_int, c_int, c_int, C.c_double, C.c_double, c_void_p, c_void_p, c_void_p,
                                         c_int])

for _n in ("mmv_omp", "mc_svt", "mc_admm"):
    # joint OMP and matrix completion in float64 (csrc/mmv_omp64.hip, csrc/mc64.hip): the argument lists of the _c32 / _c64 namesakes
    # (pointers are void* here, so the two are one list)
    SIGNATURES["jstsp_%s_f64" % _n] = SIGNATURES["jstsp_%s_c32" % _n]

for _n in ("omp", "omp_kron", "sparse_admm"):
    # OMP (dense and Kronecker) and sparse_admm in float64 (csrc/omp64.hip, csrc/sparse_admm64.hip): the _c32 argument lists
    SIGNATURES["jstsp_%s_f64" % _n] = SIGNATURES["jstsp_%s_c32" % _n]

for _n in ("nmse_spectral", "rate"):
    # scoring a float64 estimate without narrowing (csrc/svdvals.hip): the argument lists of the _c64 namesakes
    SIGNATURES["jstsp_%s_f64" % _n] = SIGNATURES["jstsp_%s_c32" % _n]


class JstspError(RuntimeError):
    """A failed C-ABI call; ``code`` is its status (< 0: JSTSP_E_*, > 0: hipError_t), None when raised on the Python side."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


E_UNSUPPORTED, E_ILLCOND = -3, -6          # include/jstsp.h


_lib = None


def load():
    """Load the shared library (once) and declare every prototype of include/jstsp.h."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise JstspError(
            "%s is missing: build it with `python -m jstsp19_amd.build` (hipcc, gfx950). "
            "jstsp19_amd has no CPU fallback." % LIB_PATH)
    # One HIP runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 /
    # libhsa-runtime64; if ours (from /opt/rocm) were loaded first, torch would later find
    # "No HIP GPUs".  Importing torch first makes the loader resolve this library's
    # libamdhip64.so.7 dependency to the copy that is already mapped.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)       # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what=""):
    if rc != 0:
        msg = load().jstsp_last_error().decode("utf-8", "replace")
        raise JstspError("%s failed with code %d: %s" % (what or "jstsp call", rc, msg), rc)


class Context:
    """One jstsp_ctx: a HIP stream + grow-only device workspace on one GPU."""

    def __init__(self, device=0):
        lib = load()
        h = c_void_p()
        check(lib.jstsp_create(int(device), C.byref(h)), "jstsp_create")
        self._h = h
        self.device = int(device)
        self._lib = lib

    @property
    def handle(self):
        if self._h is None:
            raise JstspError("context already destroyed")
        return self._h

    def set_stream(self, stream_ptr):
        check(self._lib.jstsp_set_stream(self.handle, c_void_p(stream_ptr)), "jstsp_set_stream")

    def use_torch_stream(self):
        import torch
        self.set_stream(torch.cuda.current_stream(self.device).cuda_stream)

    def synchronize(self):
        check(self._lib.jstsp_synchronize(self.handle), "jstsp_synchronize")

    def workspace_bytes(self):
        return int(self._lib.jstsp_workspace_bytes(self.handle))

    def set_profiling(self, on):
        check(self._lib.jstsp_set_profiling(self.handle, int(bool(on))), "jstsp_set_profiling")

    def get_profile(self, kernel):
        n, ms = c_int(0), C.c_double(0.0)
        check(self._lib.jstsp_get_profile(self.handle, kernel.encode(), C.byref(n), C.byref(ms)),
              "jstsp_get_profile")
        return n.value, ms.value

    def last_fused_fallbacks(self):
        """Trials of the last proposed_algorithm call re-solved after a k-scale overflow in the fused pass."""
        n = C.c_int(0)
        check(self._lib.jstsp_last_fused_fallbacks(self.handle, C.byref(n)), "jstsp_last_fused_fallbacks")
        return int(n.value)

    def last_lanczos_mismatches(self):
        """Periodic cold checks of the last solve's warm-started lambda_max values that disagreed (2e-5 relative)."""
        n = C.c_int(0)
        check(self._lib.jstsp_last_lanczos_mismatches(self.handle, C.byref(n)), "jstsp_last_lanczos_mismatches")
        return int(n.value)

    def last_dictionary_block(self):
        """Block height of the block-Toeplitz structure the last proposed_algorithm call found in its dictionary (0: none)."""
        n = C.c_int(0)
        check(self._lib.jstsp_last_dictionary_block(self.handle, C.byref(n)), "jstsp_last_dictionary_block")
        return int(n.value)

    def last_conditioning(self):
        """(rcond_min, ns_residual_max) of the last call that (pseudo-)inverted a dictionary factor."""
        rc, res = C.c_double(1.0), C.c_double(0.0)
        check(self._lib.jstsp_last_conditioning(self.handle, C.byref(rc), C.byref(res)), "jstsp_last_conditioning")
        return rc.value, res.value

    def close(self):
        if self._h is not None:
            self._lib.jstsp_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = {}


def default_context(device=0):
    ctx = _default_ctx.get(device)
    if ctx is None:
        ctx = _default_ctx[device] = Context(device)
    return ctx
