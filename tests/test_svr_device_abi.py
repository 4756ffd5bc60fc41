"""CPU tests of the singular-vector DoF importance's entry point (kpilqr_dof_importance_svd): declared, bound, exported, and
refusing a NULL context without touching a device."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import trajoptkp_amd
from trajoptkp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "kpilqr_dof_importance_svd"


def test_header_declares_it():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "kpilqr.h")).read(), flags=re.S)
    assert re.search(r"int\s+" + NAME + r"\s*\(\s*kpilqr_ctx\s*\*\s*ctx\s*,\s*int\s+sampling_k_interval\s*,\s*double\s*\*\s*sums\s*\)", src)


def test_binding_lists_it():
    assert NAME in _lib.SYMBOLS
    assert trajoptkp_amd.load().kpilqr_dof_importance_svd.argtypes == [C.c_void_p, C.c_int, C.c_void_p]


def test_library_exports_it():
    trajoptkp_amd.load()
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    assert re.search(r"\bT " + NAME + r"\b", out)


def test_null_arguments_are_rejected():
    L = trajoptkp_amd.load()
    sums = np.zeros(4)
    assert L.kpilqr_dof_importance_svd(None, 1, sums.ctypes.data_as(C.c_void_p)) == _lib.ERR_ARG
    assert L.kpilqr_dof_importance_svd(None, 0, None) == _lib.ERR_ARG
