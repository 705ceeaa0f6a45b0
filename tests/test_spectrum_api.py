"""The public surface of the spectrum entries without a GPU: the header declares jstsp_spectrum_c32 / _c64 /
jstsp_spectrum_trials_c32, the ctypes table binds them with the header's arguments, the built library exports them, the
wrappers raise JstspError without a GPU and ValueError for a CPU torch tensor, and run_rank refuses a malformed channel before
any device call."""
import os
import re

import numpy as np
import pytest
import torch

import jstsp19_amd as J
from jstsp19_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("jstsp_spectrum_c32", "jstsp_spectrum_c64", "jstsp_spectrum_trials_c32")


def _args(name):
    h = open(os.path.join(ROOT, "include", "jstsp.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, h)
    assert m, "no prototype of %s" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_three_entries():
    for name, el in (("jstsp_spectrum_c32", "jstsp_c32"), ("jstsp_spectrum_c64", "jstsp_c64")):
        assert _args(name) == ["jstsp_ctx *ctx", "int rows", "int cols", "int batch", "const %s *Y" % el, "int n_keep", "double *sv",
                               "int memspace"]
    assert _args("jstsp_spectrum_trials_c32") == [
        "jstsp_ctx *ctx", "const jstsp_model *model", "uint64_t seed", "int sweep_idx", "long long trial0", "int batch",
        "const jstsp_c32 *Hsrc", "int ld_rows", "int ld_cols", "long long strideH", "int normalize", "int n_keep", "double *sv",
        "double *sigma_max", "int memspace"]


def test_signature_table_and_library():
    lib = J.load()
    for name in NAMES:
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_int and len(args) == len(_args(name))
        assert hasattr(lib, name) and getattr(lib, name).argtypes == args
    rank = _lib.SIGNATURES["jstsp_rank_trials_c32"][1]
    chan = _lib.SIGNATURES["jstsp_build_trials_from_channel_c32"][1]
    args = _lib.SIGNATURES["jstsp_spectrum_trials_c32"][1]
    assert args[:6] == rank[:6] and args[6:11] == chan[6:11] and args[13] is _lib.c_dp           # the two calls it joins, in place
    assert "spectrum" in J.__all__ if hasattr(J, "__all__") else hasattr(J, "spectrum")
    from jstsp19_amd import solvers, system_model
    assert "spectrum" in solvers.__all__ and "spectrum_trials" in system_model.__all__


def test_wrappers_refuse_cpu_tensors_and_never_fall_back():
    Y = (np.ones((2, 64, 200)) + 0j).astype(np.complex64)
    with pytest.raises(ValueError):
        J.spectrum(torch.from_numpy(Y))
    with pytest.raises(ValueError):
        J.spectrum(np.ones((5, 3, 4, 2), complex))
    if torch.cuda.is_available():
        with pytest.raises(ValueError):
            J.spectrum(Y, n_keep=65)
        return
    with pytest.raises(J.JstspError):
        J.spectrum(Y)
    from jstsp19_amd import montecarlo as M
    from jstsp19_amd.system_model import spectrum_trials
    p = M.SweepParams(Nt=4, Nr=64, L=4, T=160, Mr=4, Mr_e=32, T_prop=160)
    with pytest.raises((J.JstspError, RuntimeError, AssertionError)):
        spectrum_trials(p, 0, 2)


def test_run_rank_refuses_a_malformed_channel_before_any_device_call():
    from jstsp19_amd import montecarlo as M
    pts = [M.SweepParams(Nt=4, Nr=64, L=4, T=160, Mr=4, Mr_e=32, T_prop=160)]
    good = np.ones((64, 4, 4), complex)
    bad = [(good[:, :, :3], ValueError),                   # L of the file is not the model's
           (good[:32], ValueError),                        # fewer rows than Nr
           (good.real, TypeError),                         # not complex
           (good[0], ValueError),                          # not 3-D / 4-D
           (np.ones((5, 64, 4, 4), complex), ValueError),  # per trial, but 5 channels for 3 trials
           ([[1j]], TypeError)]                            # not an array
    for ch, exc in bad:
        with pytest.raises(exc):
            M.run_rank(pts, 3, channel=ch)
    with pytest.raises(ValueError):
        M.run_rank(pts, 3, channel=good, channel_normalize="loud")
