"""The supplied-channel builder's public surface without a GPU: the header declares jstsp_build_trials_from_channel_c32 and its
three normalisation constants, the ctypes table binds it with the header's 14 arguments, and the built library exports it."""
import os
import re

import jstsp19_amd as J
from jstsp19_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "jstsp_build_trials_from_channel_c32"


def _header():
    return open(os.path.join(ROOT, "include", "jstsp.h")).read()


def test_header_declares_the_entry_and_the_three_constants():
    h = _header()
    m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, h)
    assert m, "no prototype of %s" % NAME
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 14
    for want, got in zip(("jstsp_ctx *ctx", "const jstsp_model *model", "uint64_t seed", "int sweep_idx", "long long trial0",
                          "int batch", "const jstsp_c32 *Hsrc", "int ld_rows", "int ld_cols", "long long strideH", "int normalize",
                          "const jstsp_trials *out", "double *sigma_max", "int memspace"), args):
        assert " ".join(got.split()) == want
    e = re.search(r"enum\s*\{\s*JSTSP_CHAN_ASIS\s*=\s*0\s*,\s*JSTSP_CHAN_REFERENCE\s*=\s*1\s*,\s*JSTSP_CHAN_UNIT\s*=\s*2\s*\}", h)
    assert e, "the JSTSP_CHAN_* constants are not declared as 0, 1, 2"
    assert (_lib.CHAN_ASIS, _lib.CHAN_REFERENCE, _lib.CHAN_UNIT) == (0, 1, 2)
    assert "plot_errorVSsnr_nyuwireless.m" in h and ":65-66" in h


def test_signature_table_has_it_with_14_arguments():
    res, args = _lib.SIGNATURES[NAME]
    assert res is _lib.c_int and len(args) == 14
    drawn = _lib.SIGNATURES["jstsp_build_trials_c32"][1]
    assert args[:6] == drawn[:6] and args[11] == drawn[6] and args[13] == drawn[7]          # the drawn call's arguments, in place
    assert args[6] is _lib.c_void_p and args[7:11] == [_lib.c_int, _lib.c_int, _lib.c_ll, _lib.c_int] and args[12] is _lib.c_dp


def test_the_built_library_exports_it():
    lib = J.load()
    assert hasattr(lib, NAME) and hasattr(lib, "jstsp_build_trials_c32")
    assert getattr(lib, NAME).argtypes == _lib.SIGNATURES[NAME][1]
