"""The C-ABI library loads and exports every symbol include/jstsp.h declares (no compute:
there is no GPU in the CPU test tier), the ctypes table mirrors the header, and the product
fails loudly — never silently falls back — without a GPU."""
import ctypes
import os
import re

import pytest

import jstsp19_amd
from jstsp19_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    txt = open(os.path.join(ROOT, "include", "jstsp.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(jstsp_[a-z0-9_]+)\s*\(", txt)))


def test_header_symbols_are_exported_and_bound():
    names = _declared()
    assert "jstsp_proposed_algorithm_c32" in names and "jstsp_correlate_c32" in names and len(names) >= 18
    assert os.path.exists(_lib.LIB_PATH), "build the library first: python -m jstsp19_amd.build"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(lib, n), "library does not export %s" % n
    assert sorted(_lib.SIGNATURES) == names, "jstsp19_amd/_lib.py SIGNATURES out of sync with include/jstsp.h"


def test_version_and_error_string_without_gpu():
    lib = jstsp19_amd.load()
    assert b"gfx950" in lib.jstsp_version()


def test_no_cpu_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(jstsp19_amd.JstspError):
        jstsp19_amd.Context(0)
    import numpy as np
    with pytest.raises(jstsp19_amd.JstspError):
        jstsp19_amd.svt(np.eye(3, dtype=complex), 0.1)


def test_product_does_not_import_the_oracle():
    """oracle/ is test infrastructure: nothing under jstsp19_amd/ may import it."""
    pkg = os.path.join(ROOT, "jstsp19_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dp, f), errors="replace").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), os.path.join(dp, f)


def test_device_code_has_no_packed_fp32_instructions(tmp_path):
    """The library is built with -target-feature -packed-fp32-ops (jstsp19_amd/build.py, DESIGN.md section 5
    'Reproducibility': dependent v_pk_fma_f32 chains returned run-to-run different results beside MFMA-heavy waves on
    MI355X).  Checked on the code objects inside the shared library."""
    import shutil
    import subprocess
    from jstsp19_amd import build as B
    assert "-packed-fp32-ops" in B.FLAGS
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not available")
    lib = str(tmp_path / "lib.so")
    shutil.copy(_lib.LIB_PATH, lib)
    subprocess.run([objdump, "--offloading", lib], cwd=str(tmp_path), check=True, capture_output=True)
    devs = [f for f in os.listdir(tmp_path) if "gfx950" in f]
    assert devs, "no gfx950 code object found in the library"
    mfma = 0
    for f in devs:
        asm = subprocess.run([objdump, "-d", str(tmp_path / f)], capture_output=True, text=True, check=True).stdout
        mfma += "v_mfma_f32" in asm
        for op in ("v_pk_fma_f32", "v_pk_mul_f32", "v_pk_add_f32"):
            assert op not in asm, "%s found in %s" % (op, f)
    assert mfma >= 5        # the disassembly really is the kernels'


# The switches of the experiments that were measured and dropped (HISTORY.md): their code is gone from the library.
REMOVED_SWITCHES = ("JSTSP_GRAM_REFINE", "JSTSP_RV_REFRESH", "JSTSP_RV_ALWAYS", "JSTSP_RV_COMP", "JSTSP_GRAD_HEAD", "JSTSP_SVT_SKIP",
                    "JSTSP_PASS_ACC", "JSTSP_INV2", "JSTSP_HGEMM_MAP", "JSTSP_HGEMM_PAIR", "JSTSP_OMP_REG", "JSTSP_OMP_GRAM",
                    "JSTSP_SADMM_FUSE", "JSTSP_SADMM_OVERLAP", "JSTSP_M3_MINK", "JSTSP_HOST_TRACE", "JSTSP_BJ_TRACE", "JSTSP_FUSED_DBG")


def test_one_build_and_every_environment_switch_is_documented_and_tested():
    """The library has one build, and include/jstsp.h lists its JSTSP_* switches: 10 to 15 of them, every name that a getenv /
    env_int call of jstsp19_amd/csrc reads must be in that list, and every one must be toggled by a test.  One build: no
    xp_getenv, JSTSP_EXPERIMENTS or JSTSP_PK_FP32_FILES in jstsp19_amd/csrc or its build script, no "Experiments build"
    paragraph in the header, and no switch of a dropped experiment named in jstsp19_amd/csrc, the header or tests/."""
    import glob
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    shipped = set()
    pat = r'(?<![a-z_])(?:getenv|env_int|env_flt)\("(JSTSP_[A-Z0-9_]+)"'
    srcs = glob.glob(os.path.join(root, "jstsp19_amd", "csrc", "*.hip")) + glob.glob(os.path.join(root, "jstsp19_amd", "csrc", "*.h"))
    for f in srcs + [os.path.join(root, "jstsp19_amd", "build.py"), os.path.join(root, "jstsp19_amd", "_lib.py")]:
        src = open(f).read()
        for name in ("xp_getenv", "JSTSP_EXPERIMENTS", "JSTSP_PK_FP32_FILES") + REMOVED_SWITCHES:
            assert name not in src, (os.path.basename(f), name)
        if f in srcs:
            shipped |= set(re.findall(pat, src))
    header = open(os.path.join(root, "include", "jstsp.h")).read()
    env = header[header.index("---- Environment"):header.index("---- kernel-level entry points")]
    assert "Experiments build" not in header
    assert not [n for n in REMOVED_SWITCHES if n in header], [n for n in REMOVED_SWITCHES if n in header]
    assert 10 <= len(shipped) <= 15, sorted(shipped)
    assert not [n for n in shipped if ("  " + n) not in env], sorted(shipped)
    assert not (shipped & set(REMOVED_SWITCHES))
    tests = "".join(open(f).read() for f in glob.glob(os.path.join(root, "tests", "test_*.py")) if not f.endswith("test_capi_symbols.py"))
    assert not [n for n in shipped if n not in tests], [n for n in shipped if n not in tests]
    assert not [n for n in REMOVED_SWITCHES if n in tests], [n for n in REMOVED_SWITCHES if n in tests]
