"""The tracked-channel builder's public surface without a GPU: the header declares jstsp_build_trials_tracked_c32 with its 10
arguments, the ctypes table binds it, the built library exports it, build_trials takes frame= / corr=, and run_tracking is a
public name of the sweep runner."""
import inspect
import os
import re

import pytest

import jstsp19_amd as J
from jstsp19_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "jstsp_build_trials_tracked_c32"


def test_header_declares_the_entry_with_its_10_arguments():
    h = open(os.path.join(ROOT, "include", "jstsp.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, h)
    assert m, "no prototype of %s" % NAME
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["jstsp_ctx *ctx", "const jstsp_model *model", "uint64_t seed", "int sweep_idx", "long long trial0", "int batch",
                    "int frame", "double corr", "const jstsp_trials *out", "int memspace"]
    doc = h[:m.start()].rsplit("/*", 1)[1]                       # the comment in front of the prototype
    assert "wideband_mmwave_channel.m:19" in doc and "O(frame)" in doc and "65535" in doc and "JSTSP_E_ARG" in doc


def test_signature_table_has_it():
    import ctypes as C
    res, args = _lib.SIGNATURES[NAME]
    assert res is _lib.c_int and len(args) == 10
    drawn = _lib.SIGNATURES["jstsp_build_trials_c32"][1]
    assert args[:6] == drawn[:6] and args[8:] == drawn[6:]       # the drawn call's arguments, in place
    assert args[6] is _lib.c_int and args[7] is C.c_double


def test_the_built_library_exports_it():
    lib = J.load()
    assert hasattr(lib, NAME) and hasattr(lib, "jstsp_build_trials_c32")
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]


def test_build_trials_takes_frame_and_corr():
    from jstsp19_amd.system_model import SweepParams, build_trials
    sig = inspect.signature(build_trials).parameters
    assert sig["frame"].kind is inspect.Parameter.KEYWORD_ONLY and sig["frame"].default == 0
    assert sig["corr"].kind is inspect.Parameter.KEYWORD_ONLY and sig["corr"].default is None
    p = SweepParams(Nt=2, Nr=8, L=2, T=4, Mr=2)
    import numpy as np
    with pytest.raises(ValueError):                              # refused before anything touches a device
        build_trials(p, 0, 1, corr=0.5, channel=np.zeros((8, 2, 2), dtype=np.complex64))
    with pytest.raises(ValueError):
        build_trials(p, 0, 1, frame=3)


def test_run_tracking_is_public():
    from jstsp19_amd import montecarlo
    assert "run_tracking" in montecarlo.__all__
    sig = inspect.signature(montecarlo.run_tracking).parameters
    assert list(sig)[:4] == ["p", "n_seqs", "n_frames", "corr"]
    for name, default in (("imax", (10, 20, 30, 50, 100)), ("cold_imax", 100), ("modes", ("cold", "warm", "warm_vs")),
                          ("precision", "f64"), ("seed", 20190913), ("sweep_idx", 0), ("device", None)):
        assert sig[name].kind is inspect.Parameter.KEYWORD_ONLY and sig[name].default == default, name
    assert sig["batch"].kind is inspect.Parameter.KEYWORD_ONLY
    from jstsp19_amd.system_model import SweepParams
    p = SweepParams(Nt=2, Nr=8, L=2, T=4, Mr=2)
    for bad in (dict(n_frames=1), dict(corr=1.5), dict(precision="f16"), dict(modes=("hot",))):     # refused on the Python side
        kw = dict(n_seqs=2, n_frames=3, corr=0.5)
        kw.update(bad)
        with pytest.raises(ValueError):
            montecarlo.run_tracking(p, kw.pop("n_seqs"), kw.pop("n_frames"), kw.pop("corr"), **kw)
